"""The pool of a set of profiles by label against the loop it replaces, in one process, on the same tables in HBM:
``klib.pooled_by(profiles, labels)`` (kpal_pool_groups_device: every table read once where it lies, one or two launches)
against ``[klib.pooled(members) for members in groups]`` (per group a gather of the members, device to device, and
kpal_pool_set_device) -- the member lists of the loop are made before the clock starts, only the ``pooled`` calls are timed.
Shapes: 100 000 x k = 4 in 200 groups (contigs binned by composition), 20 000 x k = 6 in 64 groups, uniform and with one group
of 90 % of the tables, 4 000 x k = 8 in 64 groups, 64 x k = 12 in 8 groups; the tables of a group are interleaved with the
others'.  Two warm-ups of either side, then alternating repeats, host clock around calls that end in a device synchronise, the
median and the spread (smallest and largest repeat); the outputs of the two sides are compared for equality at the timed size.
Of the C-ABI call alone: the same median over the host clock, and the table bytes per second of its kernels from the device
events (kpal_prof_*) of one more run.  Then end to end: ``kdistlib.pooled_nearest`` on fresh ``from_fastq_by_record`` profiles
(k = 8) against a panel of 64, against ``nearest_profiles`` and the ``pooled`` loop.  The device stays in its default clock
mode.  Needs a GPU.

Usage: python tools/poolbench.py [--out DIR] [--repeats N] [--quick]   (writes DIR/poolbench.json; default profiles/pool_groups)"""
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

# (name, k, tables, groups, share of the tables in group 0 (None: uniform), Poisson mean of a count, distinct tables generated)
SHAPES = (('contigs', 4, 100000, 200, None, 40.0, 1024), ('uniform', 6, 20000, 64, None, 10000.0 / 4 ** 6, 512),
          ('skewed', 6, 20000, 64, 0.9, 10000.0 / 4 ** 6, 512), ('reads', 8, 4000, 64, None, 10000.0 / 4 ** 8, 256),
          ('large', 12, 64, 8, None, 0.6, 8))
QUICK = (('contigs', 4, 2000, 20, None, 40.0, 64), ('uniform', 6, 600, 8, None, 2.4, 64), ('skewed', 6, 600, 8, 0.9, 2.4, 64),
         ('reads', 8, 100, 8, None, 0.15, 32), ('large', 12, 4, 2, None, 0.6, 2))
WARMUPS = 2


def timed(ctx, call):
    ctx.sync()
    t0 = time.perf_counter()
    result = call()
    ctx.sync()
    return time.perf_counter() - t0, result


def side(runs):
    return {'seconds': runs, 'median_s': statistics.median(runs), 'min_s': min(runs), 'max_s': max(runs)}


def labels_of(n, groups, share):
    """Interleaved: table j in group j % groups -- or, with ``share`` of the tables in group 0, every 1 / (1 - share)-th table
    in turn in one of the other groups."""
    j = np.arange(n)
    if share is None:
        return (j % groups).astype(np.int64)
    every = int(round(1.0 / (1.0 - share)))
    return np.where(j % every != 0, 0, 1 + (j // every) % (groups - 1)).astype(np.int64)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pool_groups'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='small sets: a rehearsal of the tool, not a measurement')
    ap.add_argument('--reads', type=int, default=4000)
    ap.add_argument('--length', type=int, default=10000)
    args = ap.parse_args()
    from kpal_amd import _native, kdistlib, klib
    if _native.device_count() < 1:
        raise SystemExit('poolbench needs a GPU')
    ctx = _native.context()
    rng = np.random.default_rng(47)
    report = {'repeats': args.repeats, 'warmups': WARMUPS, 'quick': bool(args.quick), 'shapes': [],
              'what': 'set: klib.pooled_by(profiles, labels); loop: [klib.pooled(members) for members in groups], the member lists made before '
                      'the clock starts; abi: kpal_pool_groups_device alone on the same tables'}
    for name, k, n, groups, share, mean, distinct in (QUICK if args.quick else SHAPES):
        bins = 4 ** k
        tb = bins * 8
        distinct = min(distinct, n)
        host = rng.poisson(mean, (distinct, bins)).astype(np.int64)
        batch = klib._DeviceBatch(ctx, n * tb, n)
        ctx.h2d(batch.ptr, host)
        for at in range(distinct, n, distinct):                   # the set repeats the distinct tables
            ctx.d2d(batch.ptr + at * tb, batch.ptr, min(distinct, n - at) * tb)
        ctx.sync()
        profiles = [klib.Profile._from_device(batch, j, k, None) for j in range(n)]
        labels = labels_of(n, groups, share)
        label_list = labels.tolist()
        members = [[p for p, l in zip(profiles, label_list) if l == g] for g in range(groups)]
        assert all(members)

        def set_call():
            return klib.pooled_by(profiles, label_list)

        def loop_call():
            return [klib.pooled(m) for m in members]

        # the two sides agree before they are timed, at this size
        keys, pools = set_call()
        loop = loop_call()
        assert all(p._device_counts() is not None for p in pools + loop)
        assert sorted(keys) == list(range(groups))
        for key, p in zip(keys, pools):
            assert np.array_equal(p.counts, loop[key].counts), (name, key)
        del pools, loop, p

        for _ in range(WARMUPS):
            set_call()
            loop_call()
        runs = {'set': [], 'loop': []}
        for _ in range(args.repeats):
            runs['set'].append(timed(ctx, set_call)[0])
            runs['loop'].append(timed(ctx, loop_call)[0])
        out = ctx.alloc(groups * tb)
        try:
            def abi_call():
                ctx.pool_groups_device(n, bins, batch.ptr, labels, groups, out)

            for _ in range(WARMUPS):
                abi_call()
            abi = [timed(ctx, abi_call)[0] for _ in range(args.repeats)]
            ctx.prof_enable(True)
            ctx.prof_reset()
            timed(ctx, abi_call)
            kernels = dict((kn, {'ms': ms, 'launches': cnt}) for kn, (ms, cnt) in ctx.prof_get().items() if cnt)
            ctx.prof_enable(False)
        finally:
            ctx.sync()
            ctx.free(out)
        kernel_ms = sum(v['ms'] for v in kernels.values())
        shape = {'name': name, 'k': k, 'tables': n, 'groups': groups, 'share_of_group_0': share, 'table_bytes': n * tb,
                 'largest_group': int(np.bincount(labels).max()), 'set': side(runs['set']), 'loop': side(runs['loop']), 'abi': side(abi),
                 'kernels': kernels, 'kernel_ms': kernel_ms, 'kernel_table_gb_per_s': n * tb / 1e9 / (kernel_ms / 1e3)}
        shape['loop_over_set'] = shape['loop']['median_s'] / shape['set']['median_s']
        # the set route loses when even its fastest repeat is slower than the loop's slowest
        shape['set_loses_past_the_spread'] = bool(shape['set']['min_s'] > shape['loop']['max_s'])
        report['shapes'].append(shape)
        print('%-8s k=%d n=%d groups=%d  set %.5f s, loop %.5f s (x%.1f); abi %.6f s, kernels %.4f ms %s, %.0f GB/s' % (
            name, k, n, groups, shape['set']['median_s'], shape['loop']['median_s'], shape['loop_over_set'], shape['abi']['median_s'], kernel_ms,
            sorted(kernels), shape['kernel_table_gb_per_s']), flush=True)
        del profiles, members, batch

    # end to end: reads binned by their nearest panel member
    K, R = 8, 64
    reads, length = (200, 2000) if args.quick else (args.reads, args.length)
    seqs = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, (reads, length))]
    qual = b'I' * length
    text = b''.join(b'@read%d\n%s\n+\n%s\n' % (i, seqs[i].tobytes(), qual) for i in range(reads))
    panel = [klib.Profile(rng.poisson(0.15 + 0.01 * r, 4 ** K).astype(np.int64), name='taxon%d' % r) for r in range(R)]
    dist = kdistlib.ProfileDistance()

    def fresh():
        return klib.Profile.from_fastq_by_record(io.BytesIO(text), K)

    def set_call():
        return kdistlib.pooled_nearest(fresh(), panel, dist)

    def loop_call():
        batch = list(fresh())
        indices, distances = kdistlib.nearest_profiles(batch, panel, dist, 1)
        hits = [[p for p, i, d in zip(batch, indices[:, 0].tolist(), distances[:, 0].tolist()) if i == r and d == d] for r in range(R)]
        return indices[:, 0], distances[:, 0], [klib.pooled(m, name=panel[r].name) if m else None for r, m in enumerate(hits)]

    a, b = set_call(), loop_call()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)
    for x, y in zip(a[2], b[2]):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x.counts, y.counts))
    bins_hit = sum(1 for x in a[2] if x is not None)
    del a, b, x, y
    for _ in range(WARMUPS):
        set_call()
        loop_call()
    runs = {'pooled_nearest': [], 'loop': [], 'scan': []}
    for _ in range(args.repeats):
        runs['pooled_nearest'].append(timed(ctx, set_call)[0])
        runs['loop'].append(timed(ctx, loop_call)[0])
        runs['scan'].append(timed(ctx, lambda: list(fresh()))[0])
    report['api'] = {'k': K, 'reads': reads, 'read_length': length, 'panel': R, 'bins_hit': bins_hit,
                     'what': 'pooled_nearest(from_fastq_by_record(text), panel, dist): scan, selection and pool, the pools stay in HBM; loop: '
                             'nearest_profiles on the list of the same scan, then klib.pooled per hit panel member; scan: the scan alone',
                     'pooled_nearest': side(runs['pooled_nearest']), 'loop': side(runs['loop']), 'scan': side(runs['scan']),
                     'loop_over_pooled_nearest': statistics.median(runs['loop']) / statistics.median(runs['pooled_nearest'])}
    print('api k=%d reads=%d panel=%d  pooled_nearest %.4f s, loop %.4f s, scan %.4f s' % (
        K, reads, R, report['api']['pooled_nearest']['median_s'], report['api']['loop']['median_s'], report['api']['scan']['median_s']), flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, 'poolbench_quick.json' if args.quick else 'poolbench.json')
    with open(path, 'w') as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    main()
