"""The summaries and the strand balance of whole sets of profiles against the per-profile entries, in one process, on the same
tables in HBM: kpal_stats_set_device against a loop of kpal_stats_device, kpal_strand_balance_set_device against a loop of
kpal_strand_balance (which uploads its table: the only single-profile entry there is; it is kpal_strand_balance_set with one
table, so that "loop" column loops the set entry at n = 1 -- the committed profiles/sets/setbench.json was taken when it still had
kernels of its own, on the same grid).  Shapes: 20 000 x k = 6, 4 000 x k = 8
with the Poisson counts 10 kb reads give, 64 x k = 12.  One warm-up of either side, then alternating repeats, host clock around
calls that end in a device synchronise, the median; the kernel-time share of one more, profiled run of each (kpal_prof_*).
Then the public API: ``[p.summary() for p in batch]`` on a fresh Profile.from_fastq_by_record batch of generated reads, against
the loop of kpal_stats_device over the same batch's tables.  Needs a GPU.

Usage: python tools/setbench.py [--out DIR] [--repeats N] [--quick]   (writes DIR/setbench.json; default profiles/sets)"""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (k, tables, Poisson mean of a count, distinct tables generated on the host -- the set repeats them)
SHAPES = ((6, 20000, 10000.0 / 4 ** 6, 512), (8, 4000, 10000.0 / 4 ** 8, 256), (12, 64, 0.6, 8))
QUICK = ((6, 300, 10000.0 / 4 ** 6, 64), (8, 100, 10000.0 / 4 ** 8, 32), (12, 4, 0.6, 2))


def timed(ctx, call):
    ctx.sync()
    t0 = time.perf_counter()
    result = call()
    ctx.sync()
    return time.perf_counter() - t0, result


def profiled(ctx, call):
    """-> (wall seconds, {kernel: {ms, launches}}) of one run with the per-kernel events on"""
    ctx.prof_enable(True)
    ctx.prof_reset()
    seconds, _ = timed(ctx, call)
    kernels = dict((name, {'ms': ms, 'launches': n}) for name, (ms, n) in ctx.prof_get().items() if n)
    ctx.prof_enable(False)
    return seconds, kernels


def compare(ctx, set_call, loop_call, repeats):
    """Warm-up, alternating repeats, medians, and one profiled run of each side."""
    set_call()
    loop_call()
    runs = {'set': [], 'loop': []}
    for _ in range(repeats):
        runs['set'].append(timed(ctx, set_call)[0])
        runs['loop'].append(timed(ctx, loop_call)[0])
    out = {}
    for side, call in (('set', set_call), ('loop', loop_call)):
        seconds, kernels = profiled(ctx, call)
        kernel_ms = sum(v['ms'] for v in kernels.values())
        out[side] = {'seconds': runs[side], 'median_s': statistics.median(runs[side]), 'profiled_run_s': seconds, 'kernel_ms': kernel_ms,
                     'kernel_share_of_profiled_run': kernel_ms / (1e3 * seconds), 'launches': sum(v['launches'] for v in kernels.values()),
                     'kernels': kernels}
    out['loop_over_set'] = out['loop']['median_s'] / out['set']['median_s']
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sets'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='small sets: a rehearsal of the tool, not a measurement')
    ap.add_argument('--reads', type=int, default=4000)
    ap.add_argument('--length', type=int, default=10000)
    args = ap.parse_args()
    from kpal_amd import _native, klib
    if _native.device_count() < 1:
        raise SystemExit('setbench needs a GPU')
    ctx = _native.context()
    rng = np.random.default_rng(41)
    report = {'repeats': args.repeats, 'quick': bool(args.quick), 'shapes': []}
    for k, n, mean, distinct in (QUICK if args.quick else SHAPES):
        bins = 4 ** k
        distinct = min(distinct, n)
        host = rng.poisson(mean, (distinct, bins)).astype(np.int64)
        ptr = ctx.alloc(n * bins * 8)
        try:
            ctx.h2d(ptr, host)
            for at in range(distinct, n, distinct):               # the set repeats the distinct tables
                ctx.d2d(ptr + at * bins * 8, ptr, min(distinct, n - at) * bins * 8)
            ctx.sync()
            # the two sides agree before they are timed
            got = ctx.stats_set_device(ptr, n, bins)
            for i in (0, n // 2, n - 1):
                one = ctx.stats_device(ptr + i * bins * 8, bins)
                assert (got[i].total, got[i].non_zero, got[i].min, got[i].max, got[i].median, got[i].mean) == \
                    (one.total, one.non_zero, one.min, one.max, one.median, one.mean), (k, i)
                assert abs(got[i].std - one.std) <= 1e-12 * one.std, (k, i)
            scores = ctx.strand_balance_set_device(k, n, ptr)
            for i in (0, n // 2, n - 1):
                one = ctx.strand_balance(host[i % distinct], k)
                assert abs(scores[i] - one) <= 1e-12 * abs(one), (k, i)
            stats = compare(ctx, lambda: ctx.stats_set_device(ptr, n, bins),
                            lambda: [ctx.stats_device(ptr + i * bins * 8, bins) for i in range(n)], args.repeats)
            balance = compare(ctx, lambda: ctx.strand_balance_set_device(k, n, ptr),
                              lambda: [ctx.strand_balance(host[i % distinct], k) for i in range(n)], args.repeats)
        finally:
            ctx.sync()
            ctx.free(ptr)
        table_gb = n * bins * 8 / 1e9
        for side in (stats, balance):
            side['set']['table_gb_per_s_of_median'] = table_gb / side['set']['median_s']
        report['shapes'].append({'k': k, 'tables': n, 'poisson_mean': mean, 'table_bytes': n * bins * 8, 'stats': stats, 'strand_balance': balance})
        print('k=%d n=%d  stats: set %.4f s, loop %.4f s (x%.1f)   balance: set %.4f s, loop %.4f s (x%.1f)' % (
            k, n, stats['set']['median_s'], stats['loop']['median_s'], stats['loop_over_set'],
            balance['set']['median_s'], balance['loop']['median_s'], balance['loop_over_set']), flush=True)

    # the public API on a fresh batch of reads
    K = 8
    reads, length = (200, 2000) if args.quick else (args.reads, args.length)
    seqs = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, (reads, length))]
    qual = b'I' * length
    text = b''.join(b'@read%d\n%s\n+\n%s\n' % (i, seqs[i].tobytes(), qual) for i in range(reads))

    def fresh():
        return list(klib.Profile.from_fastq_by_record(io.BytesIO(text), K))

    def api():
        batch = fresh()
        ctx.sync()
        t0 = time.perf_counter()
        out = [p.summary() for p in batch]
        ctx.sync()
        seconds = time.perf_counter() - t0
        assert all(p._device_counts() is not None for p in batch)
        return seconds, out, batch

    def loop(batch):
        return [d[0].stats_device(d[1], 4 ** K) for d in (p._device_counts() for p in batch)]

    api()
    runs = {'summaries': [], 'loop': [], 'scan': []}
    for _ in range(args.repeats):
        scan_s, _ = timed(ctx, fresh)
        seconds, got, batch = api()
        loop_s, want = timed(ctx, lambda: loop(batch))
        assert all(g['total'] == w.total and g['median'] == w.median and g['mean'] == w.mean for g, w in zip(got, want))
        runs['scan'].append(scan_s)
        runs['summaries'].append(seconds)
        runs['loop'].append(loop_s)
        del batch
    report['api'] = {'k': K, 'reads': reads, 'read_length': length,
                     'what': '[p.summary() for p in batch] on a fresh from_fastq_by_record batch; loop: kpal_stats_device per table of the same batch; '
                             'scan: the from_fastq_by_record call alone',
                     'seconds': runs, 'median_s': dict((key, statistics.median(v)) for key, v in runs.items()),
                     'loop_over_summaries': statistics.median(runs['loop']) / statistics.median(runs['summaries'])}
    print('api k=%d reads=%d  summaries %.4f s, loop %.4f s, scan %.4f s' % (K, reads, report['api']['median_s']['summaries'],
                                                                            report['api']['median_s']['loop'], report['api']['median_s']['scan']), flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, 'setbench_quick.json' if args.quick else 'setbench.json')
    with open(path, 'w') as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    main()
