"""The count-of-counts spectra of whole sets of profiles (klib.distributions -> kpal_distribution_set_device) against the two
host routes, in one process, on the same tables in HBM:

  (a) the route before the set entry: ``sorted(Counter(p.counts).items())`` per profile, the download of the batch included;
  (b) ``np.unique(p.counts, return_counts=True)`` per profile, the download included: the honest host opponent.

Shapes: 20 000 x k = 6 and 4 000 x k = 8 with the Poisson counts 10 kb reads give, 64 x k = 12, one k = 12 table with a mean
near 800 and a homopolymer tail past the window's cap (the overflow list is exercised), one k = 15 table.  Two warm-ups of every
side, then five alternating calls, host clock around calls that end in a device synchronise, the median.

The host routes cost the same per table whatever the set, and (a) takes minutes on the larger shapes: where a shape has more
than ``--opponent-bins`` bins in all, an opponent is timed on the first tables that hold that many (never less than one, the
download of exactly those tables included) and its time for the whole shape is that times tables / tables timed -- the JSON
says ``tables_timed`` and ``extrapolated`` for every such figure.  The k = 15 table has no (a) at all (a Python loop over 2^30
bins: a quarter of an hour a call) and ONE call of (b), no warm-up.  Needs a GPU.

Usage: python tools/spectrumbench.py [--out DIR] [--repeats N] [--quick]   (writes DIR/spectrumbench.json; default profiles/spectrum)"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, k, tables, kind, distinct tables generated on the host -- the set repeats them)
SHAPES = (('reads_k6', 6, 20000, 'reads', 512), ('reads_k8', 8, 4000, 'reads', 256), ('set_k12', 12, 64, 'sparse', 4),
          ('deep_k12', 12, 1, 'deep', 1), ('one_k15', 15, 1, 'sparse15', 1))
QUICK = (('reads_k6', 6, 300, 'reads', 64), ('reads_k8', 8, 50, 'reads', 16), ('set_k12', 10, 4, 'sparse', 2),
         ('deep_k12', 10, 1, 'deep', 1), ('one_k15', 11, 1, 'sparse15', 1))


def make_tables(rng, kind, k, distinct):
    bins = 4 ** k
    if kind == 'reads':
        return rng.poisson(10000.0 / bins, (distinct, bins)).astype(np.int64)
    if kind == 'sparse':
        return rng.poisson(0.6, (distinct, bins)).astype(np.int64)
    if kind == 'deep':                                   # a deep count: mean near 800, 200 homopolymer-like bins far above it
        t = rng.poisson(800.0, (distinct, bins)).astype(np.int64)
        t[0, rng.choice(bins, 200, replace=False)] = (10.0 ** rng.uniform(4.0, 7.0, 200)).astype(np.int64)
        return t
    assert kind == 'sparse15'                            # a block of 4^(k-2) bins, repeated to fill the table
    return rng.poisson(0.5, (1, 4 ** (k - 2))).astype(np.int64)


def timed(ctx, call):
    ctx.sync()
    t0 = time.perf_counter()
    result = call()
    ctx.sync()
    return time.perf_counter() - t0, result


def counter_route(vector):
    return sorted(collections.Counter(vector).items())


def unique_route(vector):
    values, numbers = np.unique(vector, return_counts=True)
    return list(zip(values.tolist(), numbers.tolist()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'spectrum'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmups', type=int, default=2)
    ap.add_argument('--opponent-bins', type=int, default=4 ** 13, help='bins an opponent is timed on at most per call (never less than one table)')
    ap.add_argument('--quick', action='store_true', help='small sets: a rehearsal of the tool, not a measurement')
    args = ap.parse_args()
    from kpal_amd import _native, klib
    if _native.device_count() < 1:
        raise SystemExit('spectrumbench needs a GPU')
    ctx = _native.context()
    rng = np.random.default_rng(43)
    report = {'repeats': args.repeats, 'warmups': args.warmups, 'quick': bool(args.quick), 'opponent_bins': args.opponent_bins, 'shapes': []}
    for name, k, n, kind, distinct in (QUICK if args.quick else SHAPES):
        bins = 4 ** k
        distinct = min(distinct, n)
        host = make_tables(rng, kind, k, distinct)
        batch = klib._DeviceBatch(ctx, n * bins * 8, n)
        ctx.h2d(batch.ptr, host)
        block = host.size
        for at in range(block, n * bins, block):                  # the set repeats what the host generated
            ctx.d2d(batch.ptr + at * 8, batch.ptr, min(block, n * bins - at) * 8)
        ctx.sync()
        del host

        def fresh(count=n):
            """Profiles on the batch's tables that nobody has looked at; the batch forgets what it downloaded before."""
            batch.host = None
            return [klib.Profile._from_device(batch, j, k, 'p%d' % j) for j in range(count)]

        def device():
            ps = fresh()
            out = klib.distributions(ps)
            assert all(p._device_counts() is not None for p in ps)
            return out

        single = kind == 'sparse15'
        sub = max(1, min(n, args.opponent_bins // bins))

        def opponent(route, count):
            # only the tables that are timed are downloaded: a batch of exactly those
            part = klib._DeviceBatch(ctx, count * bins * 8, count)
            ctx.d2d(part.ptr, batch.ptr, count * bins * 8)
            ctx.sync()

            def call():
                part.host = None
                return [route(p.counts) for p in (klib.Profile._from_device(part, j, k, 'p%d' % j) for j in range(count))]
            return call

        a_call = None if single else opponent(counter_route, sub)
        b_call = opponent(unique_route, n if single else sub)
        # the sides agree before they are timed
        got = device()
        want = b_call() if not single else None
        if want is not None:
            assert got[:len(want)] == want, name
        if a_call is not None and bins * sub <= 4 ** 10:
            assert a_call() == want, name
        sides = {'device': device}
        if a_call is not None:
            sides['a_counter'] = a_call
        if not single:
            sides['b_unique'] = b_call
        runs = dict((side, []) for side in sides)
        for _ in range(args.warmups):
            for side, call in sides.items():
                call()
        for _ in range(args.repeats):
            for side, call in sides.items():
                runs[side].append(timed(ctx, call)[0])
        if single:                                                # one call, no warm-up; it must agree, too
            seconds, want = timed(ctx, b_call)
            assert got == want, name
            runs['b_unique'] = [seconds]
        ctx.prof_enable(True)
        ctx.prof_reset()
        device()
        kernels = dict((kname, {'ms': ms, 'launches': c}) for kname, (ms, c) in ctx.prof_get().items() if c)
        ctx.prof_enable(False)
        entry = {'name': name, 'k': k, 'tables': n, 'kind': kind, 'table_bytes': n * bins * 8, 'pairs': sum(len(g) for g in got),
                 'device_kernels': kernels, 'sides': {}}
        for side, seconds in runs.items():
            timed_tables = n if side == 'device' or single else sub
            median = statistics.median(seconds)
            entry['sides'][side] = {'seconds': seconds, 'median_s': median, 'spread_s': max(seconds) - min(seconds), 'tables_timed': timed_tables,
                                    'extrapolated': timed_tables != n, 'whole_shape_s': median * n / timed_tables,
                                    'calls': len(seconds), 'warmups': 0 if (single and side == 'b_unique') else args.warmups}
        if a_call is None:
            entry['a_counter_left_out'] = 'a Python loop over 4^%d bins takes about a quarter of an hour a call' % k
        dev = entry['sides']['device']['median_s']
        for side in ('a_counter', 'b_unique'):
            if side in entry['sides']:
                entry[side + '_over_device'] = entry['sides'][side]['whole_shape_s'] / dev
        report['shapes'].append(entry)
        print('%s k=%d n=%d  device %.4f s   %s' % (name, k, n, dev, '   '.join(
            '%s %.4f s whole shape (x%.1f, %d tables timed)' % (side, entry['sides'][side]['whole_shape_s'], entry[side + '_over_device'],
                                                                entry['sides'][side]['tables_timed'])
            for side in ('a_counter', 'b_unique') if side in entry['sides'])), flush=True)
        del batch, a_call, b_call, got, want
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, 'spectrumbench_quick.json' if args.quick else 'spectrumbench.json')
    with open(path, 'w') as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', path)


if __name__ == '__main__':
    main()
