#!/usr/bin/env python
"""Time the nearest-n selection on the device (kpal_cross_nearest_device) against the route it replaces, in one process on the
same tables in HBM.

The route it replaces is ``kdistlib.nearest(kdistlib.cross_distances(left, right, dist), n)``; for consecutive device-resident
tables and one chunk of the right side that is one call of kpal_cross_distance_device / kpal_cross_profile_distance_device --
the Q x R doubles finished on the host -- and ``np.argsort`` over every row, and those two calls are what is timed as "old".
"new" is one call of ``Context.cross_nearest_device``.  Per shape and option set: two warm-up calls of each route, then
``--repeats`` (>= 5) timed calls of each, alternating; a call ends in a device synchronisation, so the host clock around it is
the call's time.  Reported: the median, the minimum and the maximum of each route, and ``spread`` = (max - min) / median of the
noisier route, which is what a difference between the medians has to exceed to mean anything.  The tool changes no device
setting: the numbers are for the clock mode the device is found in (reported by ``rocm-smi --showperflevel`` when available).

  python tools/nearbench.py --out profiles/nearest/nearbench.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kpal_amd import _native, kdistlib   # noqa: E402

PROD, SUM, EUCLIDEAN = 0, 1, 2
# (k, Q, R, does the old route run it)
SHAPES = [(8, 4000, 64, True), (6, 20000, 512, True), (12, 64, 64, True), (6, 60000, 8192, False)]
OPTION_SETS = [('prod', dict(metric=PROD)), ('scale', dict(metric=PROD, do_scale=1)), ('euclidean', dict(metric=EUCLIDEAN))]


def upload_tables(ctx, k, count, seed):
    """``count`` consecutive int64 tables of 4^k bins in HBM: one random table rotated and shifted per profile (fast to make,
    no two equal, counts below 2^16)."""
    bins = 4 ** k
    rs = np.random.RandomState(seed)
    base = rs.randint(0, 40, bins).astype(np.int64)
    ptr = ctx.alloc(count * bins * 8)
    for p in range(count):
        table = np.roll(base, (p * 7919) % bins)
        table = table + (rs.randint(0, 1 + p % 7, bins) if bins < 1 << 20 else p % 7)
        ctx.h2d(ptr + p * bins * 8, np.ascontiguousarray(table, dtype=np.int64))
    ctx.sync()
    return ptr


def clock_mode():
    try:
        out = subprocess.run(['rocm-smi', '--showperflevel'], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=30).stdout.decode()
        levels = sorted(set(line.split(':')[-1].strip() for line in out.splitlines() if 'Performance Level' in line))
        return ', '.join(levels) or 'unknown'
    except (OSError, subprocess.SubprocessError):
        return 'unknown'


def timed(run):
    t = time.perf_counter()
    out = run()
    return time.perf_counter() - t, out


def summary(times):
    return {'median_ms': 1e3 * float(np.median(times)), 'min_ms': 1e3 * min(times), 'max_ms': 1e3 * max(times)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the JSON here as well as to stdout')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('-n', type=int, default=5, dest='n')
    ap.add_argument('--budgets', type=int, nargs='*', default=[1 << 30, 4 << 30],
                    help='workspace budgets (bytes) the shape the old route refuses is timed at (KPAL_NEAREST_BUDGET)')
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error('--repeats must be at least 5')
    if _native.device_count() < 1:
        sys.exit('nearbench needs a GPU: a time taken anywhere else says nothing')
    ctx = _native.context()
    results = {'n': args.n, 'repeats': args.repeats, 'clock_mode': clock_mode(), 'runs': []}
    for k, Q, R, old_runs in SHAPES:
        left, right = upload_tables(ctx, k, Q, 1), upload_tables(ctx, k, R, 2)
        try:
            for name, fields in OPTION_SETS if old_runs else OPTION_SETS[:1]:
                options = _native.DistanceOptions(**fields)

                def new():
                    return ctx.cross_nearest_device(k, Q, left, R, right, options, args.n)

                def old():
                    if fields.get('do_scale'):
                        values = ctx.cross_profile_distance_device(k, Q, left, R, right, options)
                    else:
                        values = ctx.cross_distance_device(k, Q, left, R, right, fields['metric'])
                    order = kdistlib.nearest(values, args.n)
                    return np.take_along_axis(values, order, axis=1), order

                run = {'k': k, 'Q': Q, 'R': R, 'options': name}
                if old_runs:
                    for _ in range(2):
                        a, b = new(), old()
                    run['same_indices'] = bool(np.array_equal(a[1], b[1]))
                    run['same_distances'] = bool(np.array_equal(a[0], b[0]))
                    t_new, t_old = [], []
                    for _ in range(args.repeats):
                        t_new.append(timed(new)[0])
                        t_old.append(timed(old)[0])
                    run['new'], run['old'] = summary(t_new), summary(t_old)
                    run['spread'] = max((s['max_ms'] - s['min_ms']) / s['median_ms'] for s in (run['new'], run['old']))
                    run['old_over_new'] = run['old']['median_ms'] / run['new']['median_ms']
                else:
                    run['budgets'] = []
                    for budget in args.budgets:
                        os.environ['KPAL_NEAREST_BUDGET'] = str(budget)
                        for _ in range(2):
                            new()
                        s = summary([timed(new)[0] for _ in range(args.repeats)])
                        s['budget_bytes'] = budget
                        run['budgets'].append(s)
                    os.environ.pop('KPAL_NEAREST_BUDGET', None)
                results['runs'].append(run)
                print(json.dumps(run), flush=True)
        finally:
            ctx.sync()
            ctx.free(left)
            ctx.free(right)
    text = json.dumps(results, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
