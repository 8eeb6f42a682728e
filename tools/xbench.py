#!/usr/bin/env python
"""Developer harness for the rectangle of distances: Q + R profiles at k, counted from synthetic reads on the device
(seed 100 + p), kpal_cross_distance_device timed against the two ways to the same numbers without it, in one process on
the same tables: one kpal_pair_distance_device call per pair, and kpal_distance_matrix_device on the gathered concatenation
with the rectangle picked out (timed as a caller meets it -- allocation, the two device-to-device gathers, the
triangle, the pick-out -- and, for the kernel-against-kernel comparison, the triangle call alone on an allocation gathered
beforehand).  Host clock around synchronised calls, a warm-up, then --reps repeats of each.  Writes one
JSON record (and prints it).
    python tools/xbench.py --Q 16 --R 512 --k 10 [--metric prod] [--reps 10] [--reads 200000] [--out FILE]
With --options="-S --positive" (any of -b --positive -S -d, -D cosine|euclidean, -P sum): kpal_cross_profile_distance_device
timed against one kpal_profile_distance_device call per pair -- what cross_distances did for such a distance before the
rectangle took options -- in the same process on the same tables.
    python tools/xbench.py --Q 64 --R 64 --k 12 --options=-S --out profiles/cross/xbench_options_k12_64x64_S.json
With -m among the options (dynamic smoothing; -s min|average|median, -t THRESHOLD): kpal_cross_smooth_distance_device -- one
pyramid per profile, launches that do not grow with Q x R -- timed against kpal_cross_profile_distance_device on the same
tables, which loops the pair pipeline inside the library as every smoothed rectangle did before (--pair-reps: its repeats).
    python tools/xbench.py --Q 64 --R 64 --k 12 --options="-m -S" --pair-reps 1 --out profiles/cross/xbench_smooth_k12_64x64_m_S.json"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from kpal_amd import _native
import bench

HBM_PEAK_SPEC, HBM_PEAK_COPY = 8.0e12, 6.29e12      # bytes/s: datasheet, and a measured float4 copy

ap = argparse.ArgumentParser()
ap.add_argument('--Q', type=int, required=True)
ap.add_argument('--R', type=int, required=True)
ap.add_argument('--k', type=int, default=10)
ap.add_argument('--metric', default='prod', choices=('prod', 'sum', 'euclidean'))
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--pair-reps', type=int, default=None, help='repeats of the per-pair loop (default: --reps, fewer when one takes long)')
ap.add_argument('--reads', type=int, default=200_000)
ap.add_argument('--out', default=None)
ap.add_argument('--options', default=None, help='time the option rectangle for this option set; write it as --options="-S --positive"')
a = ap.parse_args()
assert a.reps >= 10, 'at least ten repeats'
ctx = _native.Context(0)
n, Q, R = 4 ** a.k, a.Q, a.R
table = n * 8
metric = {'prod': 0, 'sum': 1, 'euclidean': 2}[a.metric]
nbytes = a.reads * 151
d = ctx.alloc(nbytes)
dleft, dright = ctx.alloc(Q * table), ctx.alloc(R * table)
for p in range(Q + R):
    ctx.synth_reads_device(100 + p, 0, a.reads, 150, d)
    ctx.count_begin(a.k)
    ctx.count_feed_device(d, nbytes)
    ctx.count_finish(to_host=False)
    src, _ = ctx.count_table()
    ctx.d2d(dleft + p * table if p < Q else dright + (p - Q) * table, src, table)
ctx.sync()
ctx.free(d)


def timed(run, reps):
    run()                                               # warm-up
    times, out = [], None
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        out = run()
        ctx.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return out, {'min_ms': min(times), 'median_ms': float(np.median(times)), 'max_ms': max(times), 'reps': reps}


def cross():
    return ctx.cross_distance_device(a.k, Q, dleft, R, dright, metric)


def per_pair():
    out = np.empty((Q, R))
    for q in range(Q):
        for r in range(R):
            out[q, r] = ctx.pair_distance_device(n, dleft + q * table, dright + r * table, metric)
    return out


def concatenated():
    both = ctx.alloc((Q + R) * table)
    try:
        ctx.d2d(both, dleft, Q * table)
        ctx.d2d(both + Q * table, dright, R * table)
        tri = ctx.distance_matrix_device(Q + R, a.k, both, metric)
    finally:
        ctx.sync()
        ctx.free(both)
    out = np.empty((Q, R))
    for r in range(R):
        i = Q + r
        out[:, r] = tri[i * (i - 1) // 2:i * (i - 1) // 2 + Q]
    return out


def triangle_alone():
    return ctx.distance_matrix_device(Q + R, a.k, both_kept, metric)


def option_run():
    op = argparse.ArgumentParser()
    op.add_argument('-b', dest='do_balance', action='store_true')
    op.add_argument('--positive', dest='do_positive', action='store_true')
    op.add_argument('-S', dest='do_scale', action='store_true')
    op.add_argument('-d', dest='down', action='store_true')
    op.add_argument('-D', dest='function', default=None, choices=('euclidean', 'cosine'))
    op.add_argument('-P', dest='pairwise', default='prod', choices=('prod', 'sum'))
    op.add_argument('-m', dest='do_smooth', action='store_true')
    op.add_argument('-s', dest='summary', default='min', choices=('min', 'average', 'median'))
    op.add_argument('-t', dest='threshold', type=float, default=0.0)
    o = op.parse_args(a.options.split())
    code = {'euclidean': 2, 'cosine': 3}[o.function] if o.function else {'prod': 0, 'sum': 1}[o.pairwise]
    options = _native.DistanceOptions(do_balance=int(o.do_balance), do_positive=int(o.do_positive), do_scale=int(o.do_scale),
                                      down=int(o.down), metric=code, do_smooth=int(o.do_smooth),
                                      summary=('min', 'average', 'median').index(o.summary), threshold=o.threshold)

    def rectangle():
        if o.do_smooth:
            return ctx.cross_smooth_distance_device(a.k, Q, dleft, R, dright, options)
        return ctx.cross_profile_distance_device(a.k, Q, dleft, R, dright, options)

    def pair_loop():
        if o.do_smooth:                                 # the pair pipeline per pair inside the library: the entry as it was
            return ctx.cross_profile_distance_device(a.k, Q, dleft, R, dright, options)
        out = np.empty((Q, R))
        for q in range(Q):
            for r in range(R):
                out[q, r] = ctx.profile_distance_device(a.k, dleft + q * table, dright + r * table, options)
        return out

    got, t_rect = timed(rectangle, a.reps)
    ctx.prof_enable(True); ctx.prof_reset()
    rectangle()
    kernels = {name: {'ms': ms, 'launches': cnt} for name, (ms, cnt) in ctx.prof_get().items() if cnt}
    ctx.prof_enable(False)
    want, t_pair = timed(pair_loop, a.pair_reps or a.reps)
    with np.errstate(all='ignore'):
        rel = np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want))
    same_kind = bool((np.isnan(got) == np.isnan(want)).all() and (got[np.isinf(want)] == want[np.isinf(want)]).all())
    worst_rel = float(rel[np.isfinite(want)].max()) if np.isfinite(want).any() else 0.0
    assert same_kind and worst_rel <= 2e-9, (same_kind, worst_rel)        # each is within 1e-9 of the reference's value
    rec = {'tool': 'tools/xbench.py --options', 'src_sha': bench.source_sha(), 'k': a.k, 'Q': Q, 'R': R, 'options': a.options,
           'reads_per_profile': a.reads, 'cross_smooth_distance_device' if o.do_smooth else 'cross_profile_distance_device': t_rect,
           'cross_profile_distance_device_pair_loop' if o.do_smooth else 'per_pair_loop': t_pair,
           'median_below_per_pair_min': t_rect['median_ms'] < t_pair['min_ms'],
           'speedup_median_over_per_pair_min': t_pair['min_ms'] / t_rect['median_ms'],
           'table_bytes_read_once': (Q + R) * table, 'kernels_of_one_call': kernels, 'max_relative_difference': worst_rel}
    text = json.dumps(rec, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if a.options is not None:
    option_run()
    sys.exit(0)

got, t_cross = timed(cross, a.reps)
ctx.prof_enable(True); ctx.prof_reset()
cross()
kernels = {name: {'ms': ms, 'launches': cnt} for name, (ms, cnt) in ctx.prof_get().items() if cnt}
ctx.prof_enable(False)
want_c, t_concat = timed(concatenated, a.reps)
both_kept = ctx.alloc((Q + R) * table)
ctx.d2d(both_kept, dleft, Q * table)
ctx.d2d(both_kept + Q * table, dright, R * table)
ctx.sync()
_, t_triangle = timed(triangle_alone, a.reps)
ctx.free(both_kept)
pair_reps = a.pair_reps or a.reps
want_p, t_pair = timed(per_pair, pair_reps)


def worst(x, y):
    if a.metric == 'euclidean':
        return 0.0 if np.array_equal(x, y) else float('inf')
    with np.errstate(all='ignore'):
        rel = np.abs(x - y) / np.where(y == 0, 1.0, np.abs(y))
    return float(rel.max())


agree = {'cross_vs_per_pair': worst(got, want_p), 'cross_vs_concatenated': worst(got, want_c)}
assert max(agree.values()) <= (0.0 if a.metric == 'euclidean' else 2e-9), agree    # each is within 1e-9 of the reference's value
bar = min(t_pair['min_ms'], t_concat['min_ms'])
rec = {'tool': 'tools/xbench.py', 'src_sha': bench.source_sha(), 'k': a.k, 'Q': Q, 'R': R, 'metric': a.metric, 'reads_per_profile': a.reads,
       'cross_distance_device': t_cross, 'per_pair_loop': t_pair, 'distance_matrix_of_concatenation': t_concat,
       'triangle_call_alone_on_a_gathered_allocation': t_triangle, 'median_below_triangle_alone_min': t_cross['median_ms'] < t_triangle['min_ms'],
       'bar_ms_faster_parent_method_min': bar, 'median_below_bar': t_cross['median_ms'] < bar,
       'kernels_of_one_call': kernels, 'max_relative_difference': agree}
if Q <= 16:
    stream = R * table
    main_ms = max(v['ms'] for v in kernels.values())
    rec['right_side_bytes'] = stream
    rec['bytes_per_s_of_call_median'] = stream / (t_cross['median_ms'] * 1e-3)
    rec['bytes_per_s_of_longest_kernel'] = stream / (main_ms * 1e-3)
    rec['hbm_peak_bytes_per_s'] = {'spec': HBM_PEAK_SPEC, 'measured_copy': HBM_PEAK_COPY}
    rec['share_of_measured_copy_peak_call'] = rec['bytes_per_s_of_call_median'] / HBM_PEAK_COPY
    rec['share_of_measured_copy_peak_kernel'] = rec['bytes_per_s_of_longest_kernel'] / HBM_PEAK_COPY
text = json.dumps(rec, indent=1, sort_keys=True)
print(text)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text + '\n')
