"""kpal_cross_distance[_device], kdistlib.cross_distances and ``kpal cross`` on the GPU (kpal_amd/csrc/kpal_cross.hip).

Every expected value is the oracle's pair function on that pair (``oracle.distance_matrix_values`` deals the pairs of the
stacked sets to threads; each value still comes from the single-threaded pair function, and only the left x right entries
are looked at).  Contract: euclidean bit for bit; multiset within 1e-9 relative, exactly 0, the same NaN and the same infinity
where the oracle gives one.

How cross_core decides (n = 4^k bins): k >= 6 and more than four profiles on BOTH sides -> the staged kernels: cross_rdiff
('prod', counts in [0, 2^16)) / cross_rsum ('sum', counts in [0, 1024)), each handing on to cross_super through its `big`
flag; euclidean -> cross_gram + cross_norm, handing on to cross_super when some |x|^2 >= 2^53.  Otherwise cross_tile.
"""
import os

import numpy as np
import pytest

import matrix_cases
import memh5
import oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
METRICS = ('prod', 'sum', 'euclidean')
CROSS_KERNELS = ('cross_tile', 'cross_super', 'cross_rdiff', 'cross_rsum', 'cross_gram', 'cross_norm')
ALLOWED = CROSS_KERNELS + ('reduce_partials', 'balance_tiled', 'balance_oop', 'balance_inplace')
THREADS = min(16, os.cpu_count() or 1)


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


def oracle_rect(left, right, k, metric, bal=False):
    left, right = np.asarray(left), np.asarray(right)
    Q = left.shape[0]
    both = np.concatenate([left, right])
    with np.errstate(all='ignore'):
        tri = oracle.distance_matrix_values(both, k, bal, metric, threads=THREADS)
    out = np.empty((Q, right.shape[0]), dtype=np.float64)
    for r in range(right.shape[0]):
        i = Q + r                                      # row Q + r of the triangle holds its distances to 0 .. Q + r - 1
        out[:, r] = tri[i * (i - 1) // 2:i * (i - 1) // 2 + Q]
    return out


def assert_matches_oracle(got, want, metric, what):
    assert got.shape == want.shape, what
    if metric == 'euclidean':
        np.testing.assert_array_equal(got, want, err_msg=str(what))
        return
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (what, np.flatnonzero(np.isnan(got) != nan)[:8])
    inf = np.isinf(want)
    assert (got[inf] == want[inf]).all(), (what, np.flatnonzero(inf & (got != want))[:8])
    zero = want == 0
    assert (got[zero] == 0).all(), (what, np.flatnonzero(zero & (got != 0))[:8])
    fin = np.isfinite(want) & ~zero
    rel = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    assert rel.size == 0 or rel.max() <= RTOL, (what, float(rel.max()), int(np.flatnonzero(fin)[rel.argmax()]))


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


def sets(k, Q, R, seed=None):
    prof = matrix_cases.build('plain', k, max(8, Q + R), seed=seed).profiles
    return prof[:Q], prof[Q:Q + R]


# (65 and 130 queries: more than one 64-profile block and more than four super-tile rows on the LEFT side as well)
SHAPES = [(Q, R) for Q in (1, 2, 15, 16, 17, 33, 64) for R in (1, 7, 16, 65, 130)] + [(65, 17), (130, 17), (130, 65)]


@pytest.mark.parametrize('Q,R', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_shapes_k6(ctx, Q, R):
    left, right = sets(6, Q, R)
    for metric in METRICS:
        for bal in (False, True):
            want = oracle_rect(left, right, 6, metric, bal)
            got = ctx.cross_distance(left, right, 6, METRICS.index(metric), do_balance=bal)
            assert_matches_oracle(got, want, metric, (Q, R, metric, bal))


@pytest.mark.parametrize('k,Q,R', [(3, 5, 9), (5, 17, 33), (9, 1, 65), (9, 16, 33), (9, 33, 17), (10, 17, 20), (10, 2, 7)])
def test_shapes_other_k(ctx, k, Q, R):
    left, right = sets(k, Q, R)
    for metric in METRICS:
        for bal in (False, True):
            want = oracle_rect(left, right, k, metric, bal)
            got = ctx.cross_distance(left, right, k, METRICS.index(metric), do_balance=bal)
            assert_matches_oracle(got, want, metric, (k, Q, R, metric, bal))


def test_k12_sampled(ctx):
    """20 x 24 at k = 12 ('prod', 'euclidean'): the oracle on every pair of row 0 and of column 0 and on 40 pairs drawn
    with a fixed seed."""
    k, Q, R = 12, 20, 24
    left, right = sets(k, Q, R, seed=77)
    rs = np.random.RandomState(5)
    pairs = {(0, r) for r in range(R)} | {(q, 0) for q in range(Q)} | {(int(rs.randint(Q)), int(rs.randint(R))) for _ in range(40)}
    for metric in ('prod', 'euclidean'):
        got = ctx.cross_distance(left, right, k, METRICS.index(metric))
        assert got.shape == (Q, R)
        for q, r in sorted(pairs):
            want = oracle.distance(left[q], right[r], k, False, metric)
            if metric == 'euclidean':
                assert got[q, r] == want, (metric, q, r)
            else:
                assert abs(got[q, r] - want) <= RTOL * abs(want), (metric, q, r, got[q, r], want)


BOUNDARY_KINDS = ('plain', 'max_511', 'max_512', 'max_65535', 'max_65536', 'max_2p31m1', 'max_2p31', 'norm_2p53m1', 'norm_2p53',
                  'neg_small', 'neg_large', 'int64_extreme')


@pytest.mark.parametrize('kind', BOUNDARY_KINDS)
@pytest.mark.parametrize('P', (12, 41))
def test_boundaries(ctx, kind, P):
    """Left = the even, right = the odd profiles of the boundary set and the other way round: the boundary profile (P // 2,
    and P // 2 + 1 next to it) is once on each side.  P = 12: six a side (staged); P = 41: 21 x 20."""
    case = matrix_cases.build(kind, 6, P)
    even, odd = case.profiles[0::2], case.profiles[1::2]
    for left, right in ((even, odd), (odd, even)):
        for metric in METRICS:
            want = oracle_rect(left, right, 6, metric)
            got = ctx.cross_distance(left, right, 6, METRICS.index(metric))
            assert_matches_oracle(got, want, metric, (kind, P, metric))


def test_boundaries_tile_kernel(ctx):
    """The register-tile kernel (k = 4, and three profiles against many at k = 6) on the extreme values."""
    for kind in ('max_2p31', 'neg_small', 'int64_extreme'):
        case = matrix_cases.build(kind, 4, 12)
        for metric in METRICS:
            got = ctx.cross_distance(case.profiles[0::2], case.profiles[1::2], 4, METRICS.index(metric))
            assert_matches_oracle(got, oracle_rect(case.profiles[0::2], case.profiles[1::2], 4, metric), metric, (kind, metric))
        case = matrix_cases.build(kind, 6, 12)
        left, right = case.profiles[5:8], case.profiles
        for metric in METRICS:
            got = ctx.cross_distance(left, right, 6, METRICS.index(metric))
            assert_matches_oracle(got, oracle_rect(left, right, 6, metric), metric, (kind, metric, 'few'))


def test_paths_and_launch_counts(ctx):
    """Only the rectangle's own kernels (and balance / reduce) are launched; the launches do not grow with Q * R; a `big`
    value takes the fallback."""
    per_shape = {}
    for Q, R in ((33, 65), (64, 130)):
        left, right = sets(6, Q, R)
        for metric, want_kernels in (('prod', {'cross_rdiff': 1}), ('sum', {'cross_rsum': 1}), ('euclidean', {'cross_gram': 1, 'cross_norm': 1})):
            got, names = launched(ctx, lambda: ctx.cross_distance(left, right, 6, METRICS.index(metric)))
            assert set(names) <= set(ALLOWED), names
            assert {n: c for n, c in names.items() if n in CROSS_KERNELS} == want_kernels, (Q, R, metric, names)
            assert names.get('reduce_partials') == 1, names
            per_shape.setdefault(metric, []).append(sum(names.values()))
            assert_matches_oracle(got, oracle_rect(left, right, 6, metric), metric, (Q, R, metric))
        _, names = launched(ctx, lambda: ctx.cross_distance(left, right, 6, 0, do_balance=True))
        assert names.get('balance_tiled') == Q + R and set(names) <= set(ALLOWED), names
    for metric, counts in per_shape.items():
        assert counts[0] == counts[1], (metric, counts)
    # few queries, and k < 6: the register-tile kernel alone
    for k, Q, R in ((6, 4, 130), (6, 33, 3), (5, 20, 20)):
        left, right = sets(k, Q, R)
        for metric in METRICS:
            _, names = launched(ctx, lambda: ctx.cross_distance(left, right, k, METRICS.index(metric)))
            assert names == {'cross_tile': 1, 'reduce_partials': 1}, (k, Q, R, metric, names)
    # a count of 2^16 ('prod'), of 1024 or more ('sum'), a norm of 2^53 (euclidean): the fast form, then cross_super
    for kind, metric, first in (('max_65536', 'prod', {'cross_rdiff': 1}), ('max_65535', 'sum', {'cross_rsum': 1}),
                                ('norm_2p53', 'euclidean', {'cross_gram': 1, 'cross_norm': 1})):
        case = matrix_cases.build(kind, 6, 40)
        left, right = case.profiles[0::2], case.profiles[1::2]
        got, names = launched(ctx, lambda: ctx.cross_distance(left, right, 6, METRICS.index(metric)))
        assert {n: c for n, c in names.items() if n in CROSS_KERNELS} == dict(first, cross_super=1), (kind, names)
        assert_matches_oracle(got, oracle_rect(left, right, 6, metric), metric, (kind, metric))
    case = matrix_cases.build('max_65535', 6, 40)
    _, names = launched(ctx, lambda: ctx.cross_distance(case.profiles[0::2], case.profiles[1::2], 6, 0))
    assert 'cross_super' not in names and names.get('cross_rdiff') == 1, names


def _triangle_case(shape):
    kind, k, P = shape
    return matrix_cases.build(kind, k, max(8, P)).profiles[:P]


# k = 5, 7 profiles: the tile form with one masked row.  k = 6, 13 profiles: one super-tile with a masked row and a group above
# the diagonal (plain: matrix_rdiff / matrix_rsum against cross_rdiff / cross_rsum; max_65536: both sides hand over to the
# super kernel).  k = 6, 70 profiles: five super rows, idle groups above the diagonal in every diagonal super-tile.
TRIANGLE_SHAPES = [('plain', 5, 7), ('plain', 6, 13), ('max_65536', 6, 13), ('plain', 6, 70)]


@pytest.mark.parametrize('shape', TRIANGLE_SHAPES, ids=['%s-k%d-P%d' % s for s in TRIANGLE_SHAPES])
def test_triangle_is_the_set_crossed_with_itself(ctx, shape):
    """The lower triangle from distance_matrix_device equals, bit for bit, the entries below the diagonal of
    cross_distance_device of the set against itself: one set of kernels serves both, the triangle leaving out the tiles
    above the diagonal.  The bits can agree because the partial grouping does: at k = 6 both sides get gx = 64 workgroups
    per super-tile (n / 64 = 64 chunks clamps it: 256 CUs * 8 / 15 or 25 super-tiles of the triangle, / 16 or 25 of the
    square, are all above 64), so bin-group g adds the chunks g, g + 64, ... on either side and the fixed-order reduction adds
    the same 64 partials; at k = 5 the tile form's slices are clamped by ceil(n / 256) = 4 likewise.  Euclidean runs on the
    set whose norms reach 2^53 (same shapes): both sides leave the Gram form for the exact int64 kernel."""
    kind, k, P = shape
    table = 8 * 4 ** k
    lower = [(i, j) for i in range(1, P) for j in range(i)]
    for metric in METRICS:
        prof = _triangle_case(('norm_2p53', k, P) if metric == 'euclidean' else shape)
        dev = ctx.alloc(P * table)
        try:
            ctx.h2d(dev, prof)
            tri = ctx.distance_matrix_device(P, k, dev, METRICS.index(metric))
            square = ctx.cross_distance_device(k, P, dev, P, dev, METRICS.index(metric))
        finally:
            ctx.free(dev)
        below = np.array([square[i, j] for i, j in lower])
        assert np.array_equal(tri, below), (shape, metric, [lower[t] for t in np.flatnonzero(tri != below)[:8]])


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


def test_residency_and_aliasing(tmp_path):
    from kpal_amd import klib, kdistlib, metrics
    k = 6
    profs = _by_record_profiles(tmp_path, k)
    assert len(profs) == FASTA_RECORDS and all(p._device_counts() is not None for p in profs)
    dctx = profs[0]._device_counts()[0]
    dist = kdistlib.ProfileDistance()
    # the oracle's inputs: copies of the tables fetched from the device, the profiles themselves stay resident
    tables = np.empty((FASTA_RECORDS, 4 ** k), dtype=np.int64)
    for i, p in enumerate(profs):
        dctx.d2h(tables[i], p._device_counts()[1])
    assert all(p._device_counts() is not None for p in profs)
    left, right = profs[:5], profs[5:]
    want = oracle_rect(tables[:5], tables[5:], k, 'prod')
    # consecutive tables of one batch: used where they lie
    with CountingContext(dctx) as calls:
        got = kdistlib.cross_distances(left, right, dist)
    assert calls == {'alloc': [], 'd2d': 0, 'h2d': 0, 'free': 0}, calls
    assert_matches_oracle(got, want, 'prod', 'in place')
    # scattered device profiles: gathered by device-to-device copies, and released
    order_l, order_r = [4, 0, 2], [11, 5, 9, 7]
    with CountingContext(dctx) as calls:
        got = kdistlib.cross_distances([profs[i] for i in order_l], [profs[i] for i in order_r], dist)
    assert calls['d2d'] == 7 and calls['h2d'] == 0 and len(calls['alloc']) == 2 and calls['free'] == 2, calls
    assert_matches_oracle(got, oracle_rect(tables[order_l], tables[order_r], k, 'prod'), 'prod', 'gathered')
    # host profiles, and a mix of both on the right
    host = [klib.Profile(tables[i].copy(), 'h%d' % i) for i in range(FASTA_RECORDS)]
    got = kdistlib.cross_distances(host[:5], host[5:], kdistlib.ProfileDistance(do_balance=True))
    assert_matches_oracle(got, oracle_rect(tables[:5], tables[5:], k, 'prod', True), 'prod', 'host')
    mixed = [profs[5], host[6], profs[7], host[8], profs[9], profs[10], host[11]]
    got = kdistlib.cross_distances(left, mixed, dist)
    assert_matches_oracle(got, want, 'prod', 'mixed')
    # a set against itself: the symmetric square, an exactly zero diagonal, the oracle's triangle below it
    for metric, d in (('prod', dist), ('euclidean', kdistlib.ProfileDistance(distance_function=metrics.euclidean))):
        with CountingContext(dctx) as calls:
            square = kdistlib.cross_distances(profs, profs, d)
        assert calls == {'alloc': [], 'd2d': 0, 'h2d': 0, 'free': 0}, calls
        assert square.shape == (FASTA_RECORDS, FASTA_RECORDS)
        assert (np.diag(square) == 0).all() and np.array_equal(square, square.T)
        tri = oracle.distance_matrix_values(tables, k, False, metric)
        lower = np.array([square[i, j] for i in range(1, FASTA_RECORDS) for j in range(i)])
        assert_matches_oracle(lower, tri, metric, 'square')


def test_chunking(ctx):
    from kpal_amd import klib, kdistlib, metrics
    k, Q, R = 6, 9, 13
    left, right = sets(k, Q, R, seed=3)
    lp = [klib.Profile(v.copy(), 'l%d' % i) for i, v in enumerate(left)]
    rp = [klib.Profile(v.copy(), 'r%d' % i) for i, v in enumerate(right)]
    table = 8 * 4 ** k
    dists = {'prod': kdistlib.ProfileDistance(), 'sum': kdistlib.ProfileDistance(pairwise=metrics.pairwise['sum']),
             'euclidean': kdistlib.ProfileDistance(distance_function=metrics.euclidean)}
    for metric, dist in dists.items():
        want = oracle_rect(left, right, k, metric)
        results = []
        for max_bytes, chunks in ((R * table, 1), (5 * table, 3), (table - 1, R)):
            assert len(kdistlib.cross_chunks(table, R, max_bytes)) == chunks
            _, names = launched(ctx, lambda: results.append(kdistlib.cross_distances(lp, (p for p in rp), dist, max_bytes=max_bytes)))
            assert names.get('reduce_partials') == chunks, (metric, max_bytes, names)
            assert_matches_oracle(results[-1], want, metric, (metric, max_bytes))
        if metric == 'euclidean':
            assert np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])


def test_fallback_with_options():
    from kpal_amd import klib, kdistlib
    k, Q, R = 5, 3, 4
    left, right = sets(k, Q, R, seed=8)
    lp = [klib.Profile(v.copy(), 'l%d' % i) for i, v in enumerate(left)]
    rp = [klib.Profile(v.copy(), 'r%d' % i) for i, v in enumerate(right)]
    got = kdistlib.cross_distances(lp, rp, kdistlib.ProfileDistance(do_positive=True))
    want = np.array([[oracle.profile_distance(l, r, k, do_positive=True) for r in right] for l in left])
    assert_matches_oracle(got, want, 'prod', 'do_positive')


def test_cli_cross(tmp_path, tutorial_dir, monkeypatch):
    """``kpal cross`` on the tutorial files counted at k = 8 into two profile files (HDF5 replaced by tests/memh5.py)."""
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
    want = oracle_rect(tables['left'], tables['right'], k, 'prod')
    scaled = want * 1e10   # (no value near a rounding boundary of the tenth decimal: the text cannot hinge on the last bits)
    assert np.all(np.abs(scaled - np.floor(scaled) - 0.5) > 1e-13 * np.maximum(scaled, 1.0))
    kmer.main(['cross', 'left.k8', 'right.k8', 'cross.txt'])
    text = ['%d %d' % want.shape] + order['left'] + order['right'] + [' '.join('%.10f' % v for v in row) for row in want]
    assert open('cross.txt').read() == '\n'.join(text) + '\n'
    kmer.main(['cross', 'left.k8', 'right.k8', 'nearest.txt', '--nearest', '2'])
    lines = []
    for q, name in enumerate(order['left']):
        for r in np.argsort(want[q], kind='stable')[:2]:
            lines.append('%s %s %.10f' % (name, order['right'][r], want[q, r]))
    assert open('nearest.txt').read() == '\n'.join(lines) + '\n'
