"""The balance, the shrink and the pool of whole sets of tables against the per-table entries, in one process, on the same
tables in HBM: kpal_balance_set_device (in place) against a loop of kpal_balance_device, kpal_shrink_set_device against a loop
of kpal_shrink_device (factor 2), kpal_pool_set_device against tables - 1 calls of kpal_merge_device with the sum merger.
Shapes: those of tools/setbench.py -- 20 000 x k = 6, 4 000 x k = 8 with the Poisson counts 10 kb reads give, 64 x k = 12.  Two
warm-ups of either side, then alternating repeats, host clock around calls that end in a device synchronise, the median and
the spread (smallest and largest repeat); the kernel-time share of one more, profiled run of each (kpal_prof_*).
Then the public API: ``klib.balance_profiles(batch)`` on a fresh Profile.from_fastq_by_record batch of generated reads against
what ``for p in batch: p.balance()`` did before there was a set entry -- the batch downloaded, every table uploaded, balanced
by one launch and downloaded again.  Needs a GPU.

Usage: python tools/transformbench.py [--out DIR] [--repeats N] [--quick]   (writes DIR/transformbench.json; default
profiles/transforms)"""
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
FACTOR = 2
WARMUPS = 2


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
    """Warm-ups, alternating repeats, medians and spread, and one profiled run of each side."""
    for _ in range(WARMUPS):
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
        out[side] = {'seconds': runs[side], 'median_s': statistics.median(runs[side]), 'min_s': min(runs[side]), 'max_s': max(runs[side]),
                     'profiled_run_s': seconds, 'kernel_ms': kernel_ms, 'kernel_share_of_profiled_run': kernel_ms / (1e3 * seconds),
                     'launches': sum(v['launches'] for v in kernels.values()), 'kernels': kernels}
    out['loop_over_set'] = out['loop']['median_s'] / out['set']['median_s']
    # the set route loses when even its fastest repeat is slower than the loop's slowest
    out['set_loses_past_the_spread'] = bool(out['set']['min_s'] > out['loop']['max_s'])
    return out


def fetch(ctx, ptr, n):
    out = np.empty(n, dtype=np.int64)
    ctx.d2h(out, ptr)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'transforms'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='small sets: a rehearsal of the tool, not a measurement')
    ap.add_argument('--reads', type=int, default=4000)
    ap.add_argument('--length', type=int, default=10000)
    args = ap.parse_args()
    from kpal_amd import _native, klib
    if _native.device_count() < 1:
        raise SystemExit('transformbench needs a GPU')
    ctx = _native.context()
    rng = np.random.default_rng(43)
    report = {'repeats': args.repeats, 'warmups': WARMUPS, 'quick': bool(args.quick), 'shrink_factor': FACTOR, 'shapes': []}
    for k, n, mean, distinct in (QUICK if args.quick else SHAPES):
        bins, small = 4 ** k, 4 ** (k - FACTOR)
        tb = bins * 8
        distinct = min(distinct, n)
        host = rng.poisson(mean, (distinct, bins)).astype(np.int64)
        ptr, work, out = ctx.alloc(n * tb), ctx.alloc(n * tb), ctx.alloc(n * tb)
        try:
            ctx.h2d(ptr, host)
            for at in range(distinct, n, distinct):               # the set repeats the distinct tables
                ctx.d2d(ptr + at * tb, ptr, min(distinct, n - at) * tb)
            ctx.sync()

            def loop_balance():
                for i in range(n):
                    ctx.balance_device(k, work + i * tb)

            def loop_shrink():
                for i in range(n):
                    ctx.shrink_device(k, FACTOR, ptr + i * tb, out + i * small * 8)

            def loop_pool():
                ctx.d2d(out, ptr, tb)
                for i in range(1, n):
                    ctx.merge_device(bins, out, ptr + i * tb, _native.MERGE_SUM, out)

            # the two sides agree before they are timed
            picks = sorted({0, n // 2, n - 1})
            ctx.d2d(work, ptr, n * tb)
            ctx.balance_set_device(k, n, work, work)
            got = [fetch(ctx, work + i * tb, bins) for i in picks]
            ctx.d2d(work, ptr, n * tb)
            loop_balance()
            assert all(np.array_equal(g, fetch(ctx, work + i * tb, bins)) for g, i in zip(got, picks)), ('balance', k)
            ctx.shrink_set_device(k, FACTOR, n, ptr, out)
            got = [fetch(ctx, out + i * small * 8, small) for i in picks]
            loop_shrink()
            assert all(np.array_equal(g, fetch(ctx, out + i * small * 8, small)) for g, i in zip(got, picks)), ('shrink', k)
            ctx.pool_set_device(n, bins, ptr, out)
            got = fetch(ctx, out, bins)
            loop_pool()
            assert np.array_equal(got, fetch(ctx, out, bins)), ('pool', k)

            ctx.d2d(work, ptr, n * tb)        # (balanced again and again in place: the values wrap, the time does not care)
            balance = compare(ctx, lambda: ctx.balance_set_device(k, n, work, work), loop_balance, args.repeats)
            shrink = compare(ctx, lambda: ctx.shrink_set_device(k, FACTOR, n, ptr, out), loop_shrink, args.repeats)
            pool = compare(ctx, lambda: ctx.pool_set_device(n, bins, ptr, out), loop_pool, args.repeats)
        finally:
            ctx.sync()
            for p in (ptr, work, out):
                ctx.free(p)
        table_gb = n * tb / 1e9
        for side in (balance, shrink, pool):
            side['set']['table_gb_per_s_of_median'] = table_gb / side['set']['median_s']
        report['shapes'].append({'k': k, 'tables': n, 'poisson_mean': mean, 'table_bytes': n * tb, 'balance': balance, 'shrink': shrink, 'pool': pool})
        print('k=%d n=%d' % (k, n) + ''.join('   %s: set %.5f s, loop %.5f s (x%.1f)' % (name, side['set']['median_s'], side['loop']['median_s'],
                                                                                        side['loop_over_set'])
                                             for name, side in (('balance', balance), ('shrink', shrink), ('pool', pool))), flush=True)

    # the public API on a fresh batch of reads
    K = 8
    reads, length = (200, 2000) if args.quick else (args.reads, args.length)
    seqs = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, (reads, length))]
    qual = b'I' * length
    text = b''.join(b'@read%d\n%s\n+\n%s\n' % (i, seqs[i].tobytes(), qual) for i in range(reads))

    def fresh():
        return list(klib.Profile.from_fastq_by_record(io.BytesIO(text), K))

    def sets(batch):
        klib.balance_profiles(batch)
        assert all(p._device_counts() is not None for p in batch)

    def loop(batch):
        for p in batch:
            p.counts          # (the first one brings the whole batch over)
            p.balance()       # host counts: upload, one launch, download

    for _ in range(WARMUPS):
        sets(fresh())
        loop(fresh())
    runs = {'balance_profiles': [], 'loop': [], 'scan': []}
    for _ in range(args.repeats):
        scan_s, batch = timed(ctx, fresh)
        runs['scan'].append(scan_s)
        runs['balance_profiles'].append(timed(ctx, lambda: sets(batch))[0])
        other = fresh()
        runs['loop'].append(timed(ctx, lambda: loop(other))[0])
        assert all(np.array_equal(a.counts, b.counts) for a, b in zip(batch[::max(1, reads // 7)], other[::max(1, reads // 7)]))
        del batch, other
    report['api'] = {'k': K, 'reads': reads, 'read_length': length,
                     'what': 'klib.balance_profiles(batch) on a fresh from_fastq_by_record batch, the tables stay in HBM; loop: for p in batch: '
                             'p.counts; p.balance() on another fresh batch -- the batch downloaded, every table uploaded, balanced and downloaded; '
                             'scan: the from_fastq_by_record call alone',
                     'seconds': runs, 'median_s': dict((key, statistics.median(v)) for key, v in runs.items()),
                     'min_s': dict((key, min(v)) for key, v in runs.items()), 'max_s': dict((key, max(v)) for key, v in runs.items()),
                     'loop_over_balance_profiles': statistics.median(runs['loop']) / statistics.median(runs['balance_profiles'])}
    print('api k=%d reads=%d  balance_profiles %.4f s, loop %.4f s, scan %.4f s' % (
        K, reads, report['api']['median_s']['balance_profiles'], report['api']['median_s']['loop'], report['api']['median_s']['scan']), flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, 'transformbench_quick.json' if args.quick else 'transformbench.json')
    with open(path, 'w') as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    main()
