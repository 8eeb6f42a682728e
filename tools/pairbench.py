"""The distances of the linked pairs of two sets of profiles against what served them before, in one process, on the same tables
in HBM: kpal_paired_distance_device against (a) the loop of one pair entry per pair -- kpal_pair_distance_device for a plain
metric, kpal_profile_distance_device with options -- and (b), for the first two shapes, the diagonal of the rectangle entry
(kpal_cross_distance_device / kpal_cross_profile_distance_device), where that entry accepts the shape.  Three option sets:
'prod', -S, euclidean.  Shapes: 20 000 pairs at k = 6, 4 000 at k = 8 with the Poisson counts 10 kb reads give, 64 at k = 12.
Two warm-ups of every side, then alternating repeats, host clock around calls that end in a device synchronise, the median and
the spread (smallest and largest repeat).
Then the public API: ``kdistlib.successive_distances(windows, dist)`` on fresh ``Profile.from_fasta_by_window`` profiles (k = 8,
5 kb windows, step 500) against the Python loop of ``dist.distance(windows[i], windows[i + 1])``.  Needs a GPU.

--smooth: the same three shapes under dynamic smoothing, option sets -m, -m -S and -m -s average -t 2:
kpal_paired_smooth_distance_device against the route that served them before and is still there, kpal_paired_distance_device
with do_smooth (the pair pipeline once per pair), in the same process on the same tables; then ``klib.smooth_profiles`` on fresh
``from_fasta_by_window`` profiles against the loop of ``dist.dynamic_smooth``, and ``kdistlib.successive_distances`` with -m
against the Python loop.

Usage: python tools/pairbench.py [--out DIR] [--repeats N] [--quick] [--smooth]
(writes DIR/pairbench.json, with --smooth DIR/pairbench_smooth.json; default profiles/pairs)"""
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

# (k, pairs, Poisson mean of a count, distinct tables generated on the host per side -- a side repeats them, whether the diagonal
# of the rectangle is a baseline)
SHAPES = ((6, 20000, 10000.0 / 4 ** 6, 512, True), (8, 4000, 10000.0 / 4 ** 8, 256, True), (12, 64, 0.6, 8, False))
QUICK = ((6, 300, 10000.0 / 4 ** 6, 64, True), (8, 100, 10000.0 / 4 ** 8, 32, True), (12, 4, 0.6, 2, False))
WARMUPS = 2
RTOL = 1e-9


def timed(ctx, call):
    ctx.sync()
    t0 = time.perf_counter()
    result = call()
    ctx.sync()
    return time.perf_counter() - t0, result


def compare(ctx, calls, repeats):
    """{side: call} -> warm-ups, alternating repeats, medians and spread of every side, and the ratios to 'paired'."""
    for _ in range(WARMUPS):
        for call in calls.values():
            call()
    runs = dict((side, []) for side in calls)
    for _ in range(repeats):
        for side, call in calls.items():
            runs[side].append(timed(ctx, call)[0])
    out = {}
    for side in calls:
        out[side] = {'seconds': runs[side], 'median_s': statistics.median(runs[side]), 'min_s': min(runs[side]), 'max_s': max(runs[side])}
    for side in calls:
        if side != 'paired':
            out[side + '_over_paired'] = out[side]['median_s'] / out['paired']['median_s']
    # the paired entry loses to the per-pair loop when even its fastest repeat is slower than the loop's slowest
    out['paired_loses_past_the_spread'] = bool(out['paired']['min_s'] > out['loop']['max_s'])
    return out


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((np.abs(a - b) <= RTOL * np.abs(b)) | (np.isnan(a) & np.isnan(b))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pairs'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='small sets: a rehearsal of the tool, not a measurement')
    ap.add_argument('--genome', type=int, default=900000, help='bases of the generated sequence of the end-to-end figure')
    ap.add_argument('--smooth', action='store_true', help='the option sets with dynamic smoothing against the per-pair route')
    args = ap.parse_args()
    from kpal_amd import _native, klib, kdistlib, metrics
    if _native.device_count() < 1:
        raise SystemExit('pairbench needs a GPU')
    ctx = _native.context()
    rng = np.random.default_rng(47)

    def opts(**kw):
        o = _native.DistanceOptions(0, 0, 0, 0, 0.0, 0, 0, 0)
        for name, v in kw.items():
            setattr(o, name, v)
        return o

    option_sets = (('prod', opts(metric=_native.PAIRWISE_PROD), _native.PAIRWISE_PROD), ('scale', opts(do_scale=1), None),
                   ('euclidean', opts(metric=_native.EUCLIDEAN), _native.EUCLIDEAN))
    if args.smooth:
        option_sets = (('-m', opts(do_smooth=1), None), ('-m -S', opts(do_smooth=1, do_scale=1), None),
                       ('-m -s average -t 2', opts(do_smooth=1, summary=1, threshold=2.0), None))
    report = {'repeats': args.repeats, 'warmups': WARMUPS, 'quick': bool(args.quick), 'shapes': []}
    for k, n, mean, distinct, with_rectangle in (QUICK if args.quick else SHAPES):
        bins = 4 ** k
        tb = bins * 8
        distinct = min(distinct, n)
        left, right = ctx.alloc(n * tb), ctx.alloc(n * tb)
        shape = {'k': k, 'pairs': n, 'poisson_mean': mean, 'table_bytes_both_sides': 2 * n * tb, 'options': {}}
        try:
            for ptr in (left, right):
                ctx.h2d(ptr, rng.poisson(mean, (distinct, bins)).astype(np.int64))
                for at in range(distinct, n, distinct):               # a side repeats its distinct tables
                    ctx.d2d(ptr + at * tb, ptr, min(distinct, n - at) * tb)
            ctx.sync()
            for name, options, plain_metric in option_sets:
                def paired():
                    if args.smooth:
                        return ctx.paired_smooth_distance_device(k, n, left, right, options)
                    return ctx.paired_distance_device(k, n, left, right, options)

                def loop():
                    if args.smooth:      # the pair pipeline once per pair inside the library
                        return ctx.paired_distance_device(k, n, left, right, options)
                    if plain_metric is not None:
                        return [ctx.pair_distance_device(bins, left + i * tb, right + i * tb, plain_metric) for i in range(n)]
                    return [ctx.profile_distance_device(k, left + i * tb, right + i * tb, options) for i in range(n)]

                def rectangle():
                    if plain_metric is not None:
                        return np.diagonal(ctx.cross_distance_device(k, n, left, n, right, plain_metric))
                    return np.diagonal(ctx.cross_profile_distance_device(k, n, left, n, right, options))

                calls = {'paired': paired, 'loop': loop}
                got = paired()
                assert close(got, loop()), ('loop', k, name)       # the sides agree before they are timed
                skipped = None
                if with_rectangle and not args.smooth:
                    try:
                        diagonal = rectangle()
                        if close(got, diagonal):
                            calls['rectangle_diagonal'] = rectangle
                        else:      # (the paired entry agreed with the per-pair loop above: the rectangle is the odd one out, and is not timed)
                            off = ~((np.abs(got - diagonal) <= RTOL * np.abs(got)) | (np.isnan(got) & np.isnan(diagonal)))
                            skipped = 'disagrees with the per-pair loop and the paired entry in %d of %d pairs' % (int(off.sum()), n)
                    except (ValueError, MemoryError) as e:             # the rectangle entry does not take this shape
                        skipped = 'refused: ' + str(e)
                result = compare(ctx, calls, args.repeats)
                if skipped is not None:
                    result['rectangle_diagonal_not_timed'] = skipped
                result['paired']['table_gb_per_s_of_median'] = 2 * n * tb / 1e9 / result['paired']['median_s']
                shape['options'][name] = result
                print('k=%d pairs=%d %-9s paired %.5f s, loop %.5f s (x%.1f)%s' % (
                    k, n, name, result['paired']['median_s'], result['loop']['median_s'], result['loop_over_paired'],
                    ', rectangle diagonal %.5f s (x%.1f)' % (result['rectangle_diagonal']['median_s'], result['rectangle_diagonal_over_paired'])
                    if 'rectangle_diagonal' in result else ', rectangle diagonal not timed (%s)' % result['rectangle_diagonal_not_timed']
                    if 'rectangle_diagonal_not_timed' in result else ''), flush=True)
        finally:
            ctx.sync()
            ctx.free(left)
            ctx.free(right)
        report['shapes'].append(shape)

    # the public API on fresh windows of one sequence
    K, W, S = 8, 5000, 500
    genome = 60000 if args.quick else args.genome
    seq = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, genome)].tobytes().decode()
    text = '>genome\n' + '\n'.join(seq[j:j + 70] for j in range(0, genome, 70)) + '\n'
    dist = kdistlib.ProfileDistance(do_smooth=True) if args.smooth else kdistlib.ProfileDistance()

    def fresh():
        return list(klib.Profile.from_fasta_by_window(io.StringIO(text), K, W, S))

    def python_loop(windows):
        return np.array([dist.distance(windows[i], windows[i + 1]) for i in range(len(windows) - 1)])

    windows = fresh()
    assert close(kdistlib.successive_distances(windows, dist), python_loop(windows))
    for _ in range(WARMUPS - 1):
        kdistlib.successive_distances(fresh(), dist)
        python_loop(fresh())
    runs = {'successive_distances': [], 'loop': [], 'scan': []}
    for _ in range(args.repeats):
        scan_s, windows = timed(ctx, fresh)
        runs['scan'].append(scan_s)
        runs['successive_distances'].append(timed(ctx, lambda: kdistlib.successive_distances(windows, dist))[0])
        runs['loop'].append(timed(ctx, lambda: python_loop(windows))[0])
    if args.smooth:
        # klib.smooth_profiles: the first half of the windows against the second half, against the loop of dist.dynamic_smooth
        def halves(windows):
            return windows[:len(windows) // 2], windows[len(windows) // 2:2 * (len(windows) // 2)]

        def smooth_loop(windows):
            for l, r in zip(*halves(windows)):
                dist.dynamic_smooth(l, r)
            return windows

        a, b = fresh(), fresh()
        klib.smooth_profiles(*(halves(a) + (dist,)))
        smooth_loop(b)
        assert all(np.array_equal(x.counts, y.counts) for x, y in zip(a, b))
        sruns = {'smooth_profiles': [], 'loop': []}
        for _ in range(args.repeats):
            a, b = fresh(), fresh()
            sruns['smooth_profiles'].append(timed(ctx, lambda: klib.smooth_profiles(*(halves(a) + (dist,))))[0])
            sruns['loop'].append(timed(ctx, lambda: smooth_loop(b))[0])
        report['smooth_profiles'] = {'k': K, 'pairs': len(a) // 2,
                                     'what': 'klib.smooth_profiles(first half, second half, ProfileDistance(do_smooth=True)) on fresh from_fasta_by_window '
                                             'profiles, the tables in HBM before and after; loop: dist.dynamic_smooth(l, r) pair by pair on as fresh profiles '
                                             '(the first pair downloads the batch)',
                                     'seconds': sruns, 'median_s': dict((key, statistics.median(v)) for key, v in sruns.items()),
                                     'min_s': dict((key, min(v)) for key, v in sruns.items()), 'max_s': dict((key, max(v)) for key, v in sruns.items()),
                                     'loop_over_smooth_profiles': statistics.median(sruns['loop']) / statistics.median(sruns['smooth_profiles'])}
        print('smooth_profiles k=%d pairs=%d  %.4f s, loop %.4f s' % (K, len(a) // 2, report['smooth_profiles']['median_s']['smooth_profiles'],
                                                                      report['smooth_profiles']['median_s']['loop']), flush=True)
    report['api'] = {'k': K, 'window': W, 'step': S, 'bases': genome, 'windows': len(windows),
                     'what': 'kdistlib.successive_distances(windows, ProfileDistance(%s)) on fresh from_fasta_by_window profiles, the tables in HBM; ' % ('do_smooth=True' if args.smooth else '') +
                             'loop: [dist.distance(windows[i], windows[i + 1])] on the same profiles; scan: the from_fasta_by_window call alone',
                     'seconds': runs, 'median_s': dict((key, statistics.median(v)) for key, v in runs.items()),
                     'min_s': dict((key, min(v)) for key, v in runs.items()), 'max_s': dict((key, max(v)) for key, v in runs.items()),
                     'loop_over_successive_distances': statistics.median(runs['loop']) / statistics.median(runs['successive_distances'])}
    print('api k=%d windows=%d  successive_distances %.4f s, loop %.4f s, scan %.4f s' % (
        K, len(windows), report['api']['median_s']['successive_distances'], report['api']['median_s']['loop'], report['api']['median_s']['scan']), flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, 'pairbench%s%s.json' % ('_smooth' if args.smooth else '', '_quick' if args.quick else ''))
    with open(path, 'w') as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    main()
