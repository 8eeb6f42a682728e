"""kpal_cross_profile_distance[_device] / kpal_profile_distance_matrix_device on the GPU: the rectangle and the triangle of
distances for a ProfileDistance WITH options (kpal_amd/csrc/cross_option_kernels.hpp, kpal_cross.hip).

Every expected value is ``oracle.profile_distance(l, r, k, **options)`` on that pair.  Contract: relative 1e-9 (the project's
tolerance for distances); where the oracle is not finite the result is non-finite of the same kind (NaN for NaN, the same
infinity); an exact 0 of the oracle is an exact 0.  Smoothed cases equal the pair entry bit for bit (the same kernels on the
same tables).

How the library decides: plain options -> the plain rectangle; do_smooth -> the pair pipeline per pair on tables balanced
once; everything else -> cross_option_super (k >= 6 and more than four profiles on both sides) or cross_option_tile, after
cross_option_totals (scale) or cross_option_masked_* (scale + positive).

Measured duration of this file on an MI355X: 43 s (test_larger_k_poisson 22 s and test_k12_sampled 15 s of it, mostly the
oracle); the worst difference from the oracle over all cases was 6e-14 relative.
"""
import io
import itertools
import os

import numpy as np
import pytest

import matrix_cases
import memh5
import oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
METRICS = ('prod', 'sum', 'euclidean', 'cosine')
SUMMARY = {'min': 0, 'average': 1, 'median': 2}
RECTANGLE_KERNELS = ('cross_option_super', 'cross_option_tile', 'cross_option_masked_super', 'cross_option_masked_tile')
PER_PAIR_KERNELS = ('option_distance', 'totals', 'positive', 'smooth_level', 'smooth_apply')


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


def options(balance=False, positive=False, scale=False, down=False, metric='prod', smooth=False, summary='min', threshold=0):
    """(kpal_distance_options, the oracle's keyword arguments) of one option set."""
    from kpal_amd import _native
    native = _native.DistanceOptions(do_balance=int(balance), do_positive=int(positive), do_smooth=int(smooth), summary=SUMMARY[summary],
                                     threshold=float(threshold), do_scale=int(scale), down=int(down), metric=METRICS.index(metric))
    kwargs = dict(do_balance=balance, do_positive=positive, do_smooth=smooth, summary=summary, threshold=threshold, do_scale=scale,
                  down=down, metric=metric)
    return native, kwargs


def oracle_rect(left, right, k, kwargs):
    with np.errstate(all='ignore'):
        return np.array([[oracle.profile_distance(l, r, k, **kwargs) for r in right] for l in left], dtype=np.float64)


def assert_close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (what, 'NaN', np.flatnonzero((np.isnan(got) != nan).ravel())[:8])
    inf = np.isinf(want)
    assert (got[inf] == want[inf]).all(), (what, 'inf', np.flatnonzero((inf & (got != want)).ravel())[:8])
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    bound = RTOL * np.abs(want[fin])
    worst = float((err / np.where(want[fin] == 0, 1.0, np.abs(want[fin]))).max()) if err.size else 0.0
    print('%s: worst relative difference %.3g over %d finite, %d NaN, %d infinite values' % (what, worst, int(fin.sum()), int(nan.sum()), int(inf.sum())))
    assert (err <= bound).all(), (what, worst, np.flatnonzero((np.abs(got - want) > RTOL * np.abs(want)).ravel())[:8])


def launched(ctx, run):
    """(result of run(), {kernel: launches}) with the context's profiler on for just that call."""
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        out = run()
        got = {name: cnt for name, (_, cnt) in ctx.prof_get().items() if cnt}
    finally:
        ctx.prof_enable(False)
    return out, got


def scale_sets(k, Q, R, seed=None):
    """A left and a right set in which both branches of get_scale occur: left totals below, above and equal to right totals
    (right[1] is left[2] rotated by one bin: the same total, another vector), an all-zero profile on the right
    (matrix_cases' P - 2), an identical pair on the left."""
    prof = matrix_cases.build('plain', k, max(8, Q + R), seed=seed).profiles
    left, right = prof[:Q].copy(), prof[Q:Q + R].copy()
    right[1] = np.roll(left[2], 1)
    tl, tr = left.sum(axis=1), right.sum(axis=1)
    assert (tl[:, None] < tr[None, :]).any() and (tl[:, None] > tr[None, :]).any() and tl[2] == tr[1] and not np.array_equal(left[2], right[1])
    assert (tr == 0).any()
    return left, right


GRID = [dict(balance=b, positive=p, scale=s, down=d, metric=m)
        for b, p, (s, d), m in itertools.product((False, True), (False, True), ((False, False), (True, False), (True, True)), METRICS)]


@pytest.mark.parametrize('k,Q,R', [(6, 33, 65), (6, 3, 130), (5, 20, 20)], ids=['k6_33x65_super', 'k6_3x130_tile', 'k5_20x20_tile'])
def test_option_grid(ctx, k, Q, R):
    """{balance} x {positive} x {none, scale, scale + down} x {prod, sum, euclidean, cosine}: 48 option sets (the three plain
    ones go to the plain rectangle)."""
    left, right = scale_sets(k, Q, R)
    for o in GRID:
        native, kwargs = options(**o)
        got = ctx.cross_profile_distance(left, right, k, native)
        assert_close(got, oracle_rect(left, right, k, kwargs), (k, Q, R, o))


def test_smoothing_small_rectangle(ctx):
    """Dynamic smoothing: one call, the pair pipeline per pair inside the library -- bit for bit the pair entry, and the oracle."""
    k, Q, R = 6, 5, 7
    left, right = scale_sets(k, Q, R, seed=21)
    for o in (dict(smooth=True), dict(smooth=True, summary='average', threshold=1.5, scale=True, balance=True),
              dict(smooth=True, summary='median', threshold=1, positive=True, metric='cosine'),
              dict(smooth=True, threshold=2.5, scale=True, down=True, metric='sum', balance=True),
              dict(smooth=True, summary='average', threshold=1, metric='euclidean')):
        native, kwargs = options(**o)
        got, names = launched(ctx, lambda: ctx.cross_profile_distance(left, right, k, native))
        pairs = np.array([[ctx.profile_distance(l, r, k, native) for r in right] for l in left])
        np.testing.assert_array_equal(got, pairs, err_msg=str(o))
        assert_close(got, oracle_rect(left, right, k, kwargs), ('smooth', o))
        assert names.get('smooth_apply') == Q * R, names
        if o.get('balance'):
            assert names.get('balance_tiled') == Q + R, names      # balanced once per profile, not once per pair


def test_zero_totals(ctx):
    """Masked totals 0 / 0 (disjoint supports under --positive -S) and an all-zero profile under -S: non-finite where the
    oracle is, of the same kind."""
    k = 6
    n = 4 ** k
    rs = np.random.RandomState(4)
    for Q, R in ((6, 7), (2, 5)):                       # staged, register tiles
        left = rs.randint(0, 9, (Q, n)).astype(np.int64)
        right = rs.randint(0, 9, (R, n)).astype(np.int64)
        left[0, n // 2:] = 0
        right[0, :n // 2] = 0                           # (left 0, right 0): disjoint supports
        right[R - 1] = 0                                # all zero
        left[1] = 0
        for o in (dict(positive=True, scale=True), dict(positive=True, scale=True, down=True, metric='cosine'), dict(scale=True),
                  dict(scale=True, metric='sum'), dict(scale=True, down=True, metric='euclidean'), dict(scale=True, metric='cosine'),
                  dict(positive=True, scale=True, metric='euclidean'), dict(positive=True, metric='cosine')):
            native, kwargs = options(**o)
            want = oracle_rect(left, right, k, kwargs)
            assert not np.isfinite(want).all(), o
            assert_close(ctx.cross_profile_distance(left, right, k, native), want, ('zero totals', Q, R, o))


def test_larger_k_poisson(ctx):
    """k = 8 .. 11, Poisson tables (as test_gpu_options.test_options_vs_oracle_larger_k makes them), random option sets."""
    rs = np.random.RandomState(11)
    for k in (8, 9, 10, 11):
        n = 4 ** k
        Q, R = (5, 6) if k < 11 else (5, 5)
        left = rs.poisson(1.2, (Q, n)).astype(np.int64) * rs.randint(1, 4, (Q, 1))
        right = rs.poisson(0.9, (R, n)).astype(np.int64) * rs.randint(1, 4, (R, 1))
        left[:, n // 3: n // 2] = 0
        right[:, n // 3: n // 3 + n // 8] //= 2
        for trial in range(6 if k < 11 else 3):
            o = dict(balance=bool(rs.rand() < 0.5), positive=bool(rs.rand() < 0.4), scale=bool(rs.rand() < 0.7), down=bool(rs.rand() < 0.5),
                     metric=METRICS[rs.randint(4)])
            if not (o['positive'] or o['scale']):
                o['metric'] = 'cosine'                  # (keep every trial on the option kernels)
            native, kwargs = options(**o)
            got = ctx.cross_profile_distance(left, right, k, native)
            assert_close(got, oracle_rect(left, right, k, kwargs), (k, o))


def test_k12_sampled(ctx):
    """6 x 7 at k = 12: the oracle on a handful of pairs per option set."""
    k, Q, R = 12, 6, 7
    prof = matrix_cases.build('plain', k, Q + R, seed=77).profiles
    left, right = prof[:Q], prof[Q:]
    pairs = [(0, 0), (0, 6), (5, 0), (2, 3), (4, 5), (5, 6)]
    for o in (dict(scale=True), dict(scale=True, positive=True, balance=True), dict(metric='cosine'), dict(scale=True, down=True, metric='sum')):
        native, kwargs = options(**o)
        got = ctx.cross_profile_distance(left, right, k, native)
        assert got.shape == (Q, R)
        with np.errstate(all='ignore'):
            want = np.array([oracle.profile_distance(left[q], right[r], k, **kwargs) for q, r in pairs])
        assert_close(np.array([got[q, r] for q, r in pairs]), want, ('k12', o))


@pytest.mark.parametrize('kind', ('max_65536', 'max_2p31', 'norm_2p53', 'int64_extreme'))
@pytest.mark.parametrize('P', (12, 41))
def test_boundaries(ctx, kind, P):
    """Left = the even, right = the odd profiles of the boundary set and the other way round, with -S and with --positive,
    every metric: wrapping totals and large counts follow NumPy's int64 wrap."""
    case = matrix_cases.build(kind, 6, P)
    even, odd = case.profiles[0::2], case.profiles[1::2]
    for left, right in ((even, odd), (odd, even)):
        for metric in METRICS:
            for o in (dict(scale=True, metric=metric), dict(positive=True, metric=metric)):
                native, kwargs = options(**o)
                got = ctx.cross_profile_distance(left, right, 6, native)
                assert_close(got, oracle_rect(left, right, 6, kwargs), (kind, P, o))


FASTA_RECORDS = 12


def _by_record_profiles(tmp_path, k):
    from kpal_amd import klib
    rs = np.random.RandomState(11)
    path = os.path.join(str(tmp_path), 'records.fa')
    with open(path, 'w') as fh:
        for i in range(FASTA_RECORDS):
            fh.write('>rec%02d\n' % i)
            seq = ''.join(rs.choice(list('ACGT'), 3000 + 100 * i))
            fh.write('\n'.join(seq[j:j + 70] for j in range(0, len(seq), 70)) + '\n')
    with open(path) as fh:
        return list(klib.Profile.from_fasta_by_record(fh, k))


class CountingContext(object):
    """Counts ctx.alloc / ctx.d2d / ctx.h2d / ctx.free while it stands in for them."""

    def __init__(self, ctx):
        self.ctx, self.calls = ctx, {'alloc': [], 'd2d': 0, 'h2d': 0, 'free': 0}

    def __enter__(self):
        c = self.ctx
        self.saved = (c.alloc, c.d2d, c.h2d, c.free)

        def alloc(nbytes):
            self.calls['alloc'].append(int(nbytes))
            return self.saved[0](nbytes)

        def d2d(*a):
            self.calls['d2d'] += 1
            return self.saved[1](*a)

        def h2d(*a):
            self.calls['h2d'] += 1
            return self.saved[2](*a)

        def free(p):
            self.calls['free'] += 1
            return self.saved[3](p)

        c.alloc, c.d2d, c.h2d, c.free = alloc, d2d, h2d, free
        return self.calls

    def __exit__(self, *exc):
        for name in ('alloc', 'd2d', 'h2d', 'free'):
            delattr(self.ctx, name)


def _lower(square):
    return np.array([square[i, j] for i in range(1, square.shape[0]) for j in range(i)])


def _matrix_values(text, count):
    lines = text.split('\n')
    assert lines[0] == str(count)
    return np.array([float(x) for line in lines[1 + count:] if line for x in line.split(' ')])


def test_triangle_device_resident(tmp_path):
    """By-record profiles still in HBM: the triangle entry == the rectangle of the set against itself below the diagonal ==
    the oracle; consecutive batch tables are used where they lie; scattered ones are gathered and released."""
    from kpal_amd import kdistlib, metrics
    k = 6
    profs = _by_record_profiles(tmp_path, k)
    assert len(profs) == FASTA_RECORDS and all(p._device_counts() is not None for p in profs)
    dctx = profs[0]._device_counts()[0]
    tables = np.empty((FASTA_RECORDS, 4 ** k), dtype=np.int64)
    for i, p in enumerate(profs):
        dctx.d2h(tables[i], p._device_counts()[1])
    base = profs[0]._device_counts()[1]
    dists = ((dict(scale=True, balance=True), kdistlib.ProfileDistance(do_scale=True, do_balance=True)),
             (dict(scale=True, positive=True, down=True, metric='sum'),
              kdistlib.ProfileDistance(do_scale=True, do_positive=True, down=True, pairwise=metrics.pairwise['sum'])),
             (dict(metric='cosine'), kdistlib.ProfileDistance(distance_function=metrics.cosine_similarity)),
             (dict(positive=True, metric='euclidean'), kdistlib.ProfileDistance(do_positive=True, distance_function=metrics.euclidean)),
             (dict(smooth=True, threshold=1, scale=True), kdistlib.ProfileDistance(do_smooth=True, threshold=1, do_scale=True)))
    for o, dist in dists:
        native, kwargs = options(**o)
        want = _lower(oracle_rect(tables, tables, k, kwargs))
        with CountingContext(dctx) as calls:
            tri, names = launched(dctx, lambda: dctx.profile_distance_matrix_device(FASTA_RECORDS, k, base, native))
            square = kdistlib.cross_distances(profs, profs, dist)
            out = io.StringIO()
            kdistlib.distance_matrix(profs, out, 10, dist)
        assert calls == {'alloc': [], 'd2d': 0, 'h2d': 0, 'free': 0}, (o, calls)
        assert_close(tri, want, ('triangle', o))
        assert_close(tri, _lower(square), ('triangle against the rectangle', o))
        assert np.abs(_matrix_values(out.getvalue(), FASTA_RECORDS) - tri).max() <= 0.5000001e-10, o      # the text is the triangle's values
        if not o.get('smooth'):
            assert not set(names) & set(PER_PAIR_KERNELS), names
        # scattered: gathered inside the try that frees the allocation
        order = [4, 0, 2, 7, 11]
        with CountingContext(dctx) as calls:
            out = io.StringIO()
            kdistlib.distance_matrix([profs[i] for i in order], out, 10, dist)
        assert calls['d2d'] == len(order) and calls['h2d'] == 0 and len(calls['alloc']) == 1 and calls['free'] == 1, calls
        sub = _lower(oracle_rect(tables[order], tables[order], k, kwargs))
        assert np.abs(_matrix_values(out.getvalue(), len(order)) - sub).max() <= RTOL * np.abs(sub).max() + 0.5000001e-10, o
    assert all(p._device_counts() is not None for p in profs)


@pytest.mark.parametrize('P', (3, 12, 41))
def test_triangle_host_profiles(ctx, P):
    """kpal_profile_distance_matrix (host tables: uploaded once, then the triangle entry) == the rectangle of the set against
    itself below the diagonal == the oracle.  P = 3: register tiles; 12: one super-tile; 41: six of them, three on the diagonal."""
    k = 6
    prof = matrix_cases.build('plain', k, max(8, P), seed=P).profiles[:P]
    for o in (dict(scale=True), dict(scale=True, positive=True, balance=True), dict(positive=True), dict(metric='cosine', balance=True),
              dict(scale=True, down=True, metric='euclidean'), dict(positive=True, scale=True, metric='cosine')):
        native, kwargs = options(**o)
        tri, names = launched(ctx, lambda: ctx.profile_distance_matrix(prof, k, native))
        assert not set(names) & set(PER_PAIR_KERNELS), names
        assert_close(tri, _lower(oracle_rect(prof, prof, k, kwargs)), ('host triangle', P, o))
        assert_close(tri, _lower(ctx.cross_profile_distance(prof, prof, k, native)), ('host triangle against the rectangle', P, o))
    native, _ = options(smooth=True, threshold=1, scale=True, balance=True)
    tri = ctx.profile_distance_matrix(prof, k, native)
    pairs = np.array([ctx.profile_distance(prof[i], prof[j], k, native) for i in range(1, P) for j in range(i)])
    np.testing.assert_array_equal(tri, pairs)


def test_deterministic(ctx):
    k, Q, R = 6, 33, 65
    left, right = scale_sets(k, Q, R)
    for o in (dict(scale=True), dict(scale=True, positive=True, metric='sum'), dict(scale=True, metric='cosine', balance=True)):
        native, _ = options(**o)
        a = ctx.cross_profile_distance(left, right, k, native)
        b = ctx.cross_profile_distance(left, right, k, native)
        np.testing.assert_array_equal(a, b, err_msg=str(o))


def test_launch_structure(ctx):
    """A batched option set is a fixed list of launches whatever Q and R are: no per-pair option kernels, one balance per
    profile, and positive + scale costs exactly one rectangle launch more than scale."""
    k = 6
    lists = {}
    for Q, R in ((33, 65), (64, 130)):
        left, right = scale_sets(k, Q, R)
        for key, o in (('S', dict(scale=True)), ('S positive', dict(scale=True, positive=True)), ('cosine', dict(metric='cosine')),
                       ('S sum', dict(scale=True, metric='sum')), ('positive', dict(positive=True, metric='euclidean'))):
            native, _ = options(**o)
            _, names = launched(ctx, lambda: ctx.cross_profile_distance(left, right, k, native))
            assert not set(names) & set(PER_PAIR_KERNELS), (key, names)
            lists.setdefault(key, []).append(names)
        native, _ = options(scale=True, balance=True)
        _, names = launched(ctx, lambda: ctx.cross_profile_distance(left, right, k, native))
        assert names.get('balance_tiled') == Q + R and not set(names) & set(PER_PAIR_KERNELS), names
        assert {n: c for n, c in names.items() if n != 'balance_tiled'} == lists['S'][-1], names
    for key, (small, large) in lists.items():
        assert small == large, (key, small, large)

    def rectangles(names):
        return sum(c for n, c in names.items() if n in RECTANGLE_KERNELS)

    assert lists['S'][0] == {'cross_option_totals': 1, 'cross_option_super': 1, 'reduce_partials': 2}, lists['S'][0]
    assert rectangles(lists['S'][0]) == 1 and rectangles(lists['S positive'][0]) == 2, lists
    assert lists['cosine'][0] == {'cross_option_super': 1, 'reduce_partials': 1}, lists['cosine'][0]
    # few profiles on a side, and k < 6: the register-tile form
    for kk, Q, R in ((6, 3, 130), (5, 20, 20)):
        left, right = scale_sets(kk, Q, R)
        _, names = launched(ctx, lambda: ctx.cross_profile_distance(left, right, kk, options(scale=True, positive=True)[0]))
        assert names == {'cross_option_masked_tile': 1, 'cross_option_tile': 1, 'reduce_partials': 2}, names
    # plain options are the plain rectangle's launches
    left, right = scale_sets(k, 33, 65)
    _, names = launched(ctx, lambda: ctx.cross_profile_distance(left, right, k, options()[0]))
    assert names == {'cross_rdiff': 1, 'reduce_partials': 1}, names


def test_option_errors(ctx):
    from kpal_amd import _native
    v = [np.ones(16, dtype=np.int64)] * 2
    with pytest.raises(ValueError):
        ctx.cross_profile_distance(v, v, 2, _native.DistanceOptions(metric=7))
    with pytest.raises(ValueError):
        ctx.cross_profile_distance(v, v, 2, _native.DistanceOptions(do_smooth=1, summary=5))
    with pytest.raises(ValueError):
        ctx.cross_profile_distance(v, v, 3, _native.DistanceOptions(do_scale=1))
    with pytest.raises(ValueError):
        ctx.profile_distance_matrix_device(0, 2, 0, _native.DistanceOptions(do_scale=1))


def test_cli_cross_and_matrix(ctx, tmp_path, tutorial_dir, monkeypatch):
    """``kpal cross ... -S --positive -b`` and ``kpal matrix ... -S`` on the tutorial files counted at k = 8 (HDF5 replaced by
    tests/memh5.py): the oracle's values at the printed precision (ten decimals: half a unit of the last one on top of the
    1e-9), and no per-pair option kernel."""
    from kpal_amd import files, kmer
    k = 8
    store = memh5.Store()
    monkeypatch.setattr(files, 'open_profile_file', store.open)
    monkeypatch.chdir(tmp_path)
    fastas = sorted(f for f in os.listdir(tutorial_dir) if f.endswith('.fa'))
    assert len(fastas) >= 4, fastas
    half = len(fastas) // 2
    tables, order = {}, {}
    for side, names in (('left', fastas[:half]), ('right', fastas[half:])):
        kmer.main(['count', '-k', str(k)] + [os.path.join(tutorial_dir, f) for f in names] + [side + '.k8'])
        handle = store.open(side + '.k8', 'r')
        order[side] = sorted(handle['profiles'].keys())
        tables[side] = np.stack([handle['profiles/' + n][:] for n in order[side]])
    Q, R = len(order['left']), len(order['right'])
    want = oracle_rect(tables['left'], tables['right'], k, options(scale=True, positive=True, balance=True)[1])
    _, names = launched(ctx, lambda: kmer.main(['cross', 'left.k8', 'right.k8', 'cross.txt', '-S', '--positive', '-b']))
    assert not set(names) & set(PER_PAIR_KERNELS) and sum(c for n, c in names.items() if n in RECTANGLE_KERNELS) == 2, names
    lines = open('cross.txt').read().split('\n')
    assert lines[0] == '%d %d' % (Q, R) and lines[1:1 + Q + R] == order['left'] + order['right']
    got = np.array([[float(x) for x in line.split(' ')] for line in lines[1 + Q + R:] if line])
    assert got.shape == want.shape and (np.abs(got - want) <= RTOL * np.abs(want) + 0.5000001e-10).all(), (got, want)
    want = _lower(oracle_rect(tables['left'], tables['left'], k, options(scale=True)[1]))
    _, names = launched(ctx, lambda: kmer.main(['matrix', 'left.k8', 'matrix.txt', '-S']))
    assert not set(names) & set(PER_PAIR_KERNELS) and sum(c for n, c in names.items() if n in RECTANGLE_KERNELS) == 1, names
    got = _matrix_values(open('matrix.txt').read(), Q)
    assert got.shape == want.shape and (np.abs(got - want) <= RTOL * np.abs(want) + 0.5000001e-10).all(), (got, want)
