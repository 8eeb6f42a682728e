"""kpal_cross_nearest[_device], kdistlib.nearest_profiles and ``kpal cross --nearest`` on the GPU (kpal_amd/csrc/kpal_nearest.hip,
nearest_kernels.hpp, nearest_plan.hpp): the n nearest right profiles of every left profile, finished and selected on the
device in tiles.

Every expected distance is ``oracle.profile_distance`` on that pair, every expected index ``np.argsort(kind='stable')`` over the
oracle's row.  Contract: distances within 1e-9 relative of the oracle (NaN where it has NaN), unscaled euclidean and cosine
bit for bit; a one-tile call returns exactly the doubles of kpal_cross_profile_distance for the pairs it selects.  Where a test
is not about ties it first asserts that neighbouring sorted oracle distances of every row differ by more than 1e-6 relative,
so that 1e-9 cannot reorder them.

Shapes: k = 3 (64 bins, the register-tile kernels) and k = 6 (4096 bins) at Q = 9, R = 21 -- one tile takes the staged kernels
(the Gram kernels for euclidean); tiles of at most 4 x 8 are nine tiles with ragged edges of which the last band (one row) and
the last column (five profiles, against four rows) take the register-tile kernels instead.
"""
import os

import numpy as np
import pytest

import memh5
import oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
GAP = 1e-6
METRICS = ('prod', 'sum', 'euclidean', 'cosine')
SUMMARY = {'min': 0, 'average': 1, 'median': 2}
Q, R = 9, 21
TILE_Q, TILE_R = 4, 8

OPTION_SETS = {
    'prod': dict(), 'sum': dict(metric='sum'), 'euclidean': dict(metric='euclidean'), 'cosine': dict(metric='cosine'),
    'balance': dict(balance=True), 'scale': dict(scale=True), 'scale_down': dict(scale=True, down=True), 'positive': dict(positive=True),
    'positive_scale': dict(positive=True, scale=True), 'smooth': dict(smooth=True, summary='min', threshold=3),
}
BIT_EXACT = ('euclidean', 'cosine')


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


def random_sets(k, seed, q=Q, r=R):
    """Poisson counts with a rate of its own per profile: distances that lie far apart."""
    rs = np.random.RandomState(seed)
    rates = rs.uniform(2.0, 40.0, q + r)
    prof = np.stack([rs.poisson(rate, 4 ** k) for rate in rates]).astype(np.int64)
    return prof[:q], prof[q:]


_RECT = {}


def oracle_rect(k, seed, name):
    """The oracle's rectangle of random_sets(k, seed) under OPTION_SETS[name]: computed once, shared, never written."""
    key = (k, seed, name)
    if key not in _RECT:
        left, right = random_sets(k, seed)
        kwargs = options(**OPTION_SETS[name])[1]
        with np.errstate(all='ignore'):
            rect = np.array([[oracle.profile_distance(l, r, k, **kwargs) for r in right] for l in left], dtype=np.float64)
        rect.setflags(write=False)
        _RECT[key] = rect
    return _RECT[key]


def assert_separated(want, what):
    """Neighbouring sorted values of every row differ by more than GAP relative: no row is let off."""
    assert np.isfinite(want).all(), what
    s = np.sort(want, axis=1)
    gap = (s[:, 1:] - s[:, :-1]) / np.maximum(np.abs(s[:, 1:]), np.abs(s[:, :-1]))
    assert gap.min() > GAP, (what, float(gap.min()))


def assert_nearest(got, want, n, exact, what, first=0):
    """got = (dist, index) of shape (rows, n) against the oracle rectangle ``want`` whose column c is right profile first + c."""
    dist, index = got
    rows, cols = want.shape
    m = min(n, cols)
    assert dist.shape == index.shape == (rows, n), what
    order = np.argsort(want, axis=1, kind='stable')[:, :m]
    np.testing.assert_array_equal(index[:, :m], order + first, err_msg=str(what))
    assert (index[:, m:] == -1).all() and np.isnan(dist[:, m:]).all(), what
    expect = np.take_along_axis(want, order, axis=1)
    if exact:
        np.testing.assert_array_equal(dist[:, :m], expect, err_msg=str(what))
        return
    nan = np.isnan(expect)
    assert (np.isnan(dist[:, :m]) == nan).all(), what
    err = np.abs(dist[:, :m][~nan] - expect[~nan])
    worst = float((err / np.where(expect[~nan] == 0, 1.0, np.abs(expect[~nan]))).max()) if err.size else 0.0
    print('%s: worst relative difference %.3g' % (what, worst))
    assert (err <= RTOL * np.abs(expect[~nan])).all(), (what, worst)


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


SEEDS = {3: 31, 6: 61}


@pytest.mark.parametrize('name', sorted(OPTION_SETS))
@pytest.mark.parametrize('k', (3, 6))
def test_option_sets_one_tile_and_tiled(ctx, k, name):
    left, right = random_sets(k, SEEDS[k])
    want = oracle_rect(k, SEEDS[k], name)
    assert_separated(want, (k, name))
    native = options(**OPTION_SETS[name])[0]
    for n in (1, 3, R, R + 5):
        for tile in ((0, 0), (TILE_Q, TILE_R)):
            got = ctx.cross_nearest(left, right, k, native, n, tile_q=tile[0], tile_r=tile[1])
            assert_nearest(got, want, n, name in BIT_EXACT, (k, name, n, tile))


@pytest.mark.parametrize('k', (3, 6))
def test_one_tile_returns_the_doubles_of_the_rectangle_entry(ctx, k):
    """The device finish: the same kernels on the same grid, so every selected distance IS the value kpal_cross_profile_distance
    returns for that pair."""
    left, right = random_sets(k, SEEDS[k])
    for name in sorted(set(OPTION_SETS) - {'smooth'}):   # (a smoothed set is selected on the host: nothing is finished on the device)
        native = options(**OPTION_SETS[name])[0]
        rect = ctx.cross_profile_distance(left, right, k, native)
        dist, index = ctx.cross_nearest(left, right, k, native, R, tile_q=Q, tile_r=R)
        assert (np.sort(index, axis=1) == np.arange(R)).all(), name
        np.testing.assert_array_equal(dist.view(np.int64), np.take_along_axis(rect, index, axis=1).view(np.int64), err_msg=name)


def tie_sets():
    """k = 6; right profiles 2, 10 and 19 -- one in each column of tiles -- are the same table."""
    left, right = random_sets(6, 62)
    right = right.copy()
    right[10] = right[2]
    right[19] = right[2]
    with np.errstate(all='ignore'):
        want = np.array([[oracle.profile_distance(l, r, 6, metric='euclidean') for r in right] for l in left])
    assert (want[:, 2] == want[:, 10]).all() and (want[:, 2] == want[:, 19]).all()
    return left, right, want


def test_ties_go_to_the_lower_index(ctx):
    left, right, want = tie_sets()
    native = options(metric='euclidean')[0]
    # make the tied profile the nearest of some row, so that n = 1 and n = 2 cut through the tie there
    left = left.copy()
    left[4] = right[2]
    left[4, 0] += 1
    with np.errstate(all='ignore'):
        want[4] = [oracle.profile_distance(left[4], r, 6, metric='euclidean') for r in right]
    assert list(np.argsort(want[4], kind='stable')[:3]) == [2, 10, 19]
    for n in (1, 2, 3, R):
        for tile in ((0, 0), (TILE_Q, TILE_R)):
            assert_nearest(ctx.cross_nearest(left, right, 6, native, n, tile_q=tile[0], tile_r=tile[1]), want, n, True, ('ties', n, tile))
    # a candidate carried over from an earlier call does not beat a lower index that arrives later: the upper part of the
    # right side first, then the lower part with a lower right_first
    for n in (1, 2, 3, 5):
        dist, index = ctx.cross_nearest(left, right[8:], 6, native, n, right_first=8, tile_q=TILE_Q, tile_r=TILE_R)
        assert_nearest((dist.copy(), index.copy()), want[:, 8:], n, True, ('upper part', n), first=8)
        ctx.cross_nearest(left, right[:8], 6, native, n, right_first=0, have=min(n, R - 8), tile_q=TILE_Q, tile_r=TILE_R, dist=dist, index=index)
        assert_nearest((dist, index), want, n, True, ('carried', n))


@pytest.mark.parametrize('name', ('cosine', 'scale'))
def test_nan_sorts_last_by_index(ctx, name):
    """All-zero tables: NaN under the cosine similarity and under -S.  An all-zero left profile makes every candidate NaN."""
    k = 6
    left, right = random_sets(k, 63)
    left, right = left.copy(), right.copy()
    right[[3, 12, 20]] = 0
    left[5] = 0
    native, kwargs = options(**OPTION_SETS[name])
    with np.errstate(all='ignore'):
        want = np.array([[oracle.profile_distance(l, r, k, **kwargs) for r in right] for l in left], dtype=np.float64)
    assert np.isnan(want[:, [3, 12, 20]]).all() and np.isnan(want[5]).all() and np.isfinite(np.delete(want, 5, axis=0)[:, :3]).all()
    finite = np.delete(np.delete(want, 5, axis=0), [3, 12, 20], axis=1)
    assert_separated(finite, name)
    for n in (3, R - 2, R):
        for tile in ((0, 0), (TILE_Q, TILE_R)):
            got = ctx.cross_nearest(left, right, k, native, n, tile_q=tile[0], tile_r=tile[1])
            assert_nearest(got, want, n, name in BIT_EXACT, ('nan', name, n, tile))
    dist, index = ctx.cross_nearest(left, right, k, native, 4, tile_q=TILE_Q, tile_r=TILE_R)
    assert list(index[5]) == [0, 1, 2, 3] and np.isnan(dist[5]).all()


def test_fast_forms_give_up(ctx):
    """A count of 2^16 makes the reciprocal form of 'prod' hand on to the pair-of-counts kernel; counts of 2^21 in every bin
    make a norm 2^54, past what the Gram form is exact for: the int64 kernels run for the tiles that see it.  Tiles of at
    most 5 x 8: the three tiles of the first band (five rows) are staged and try the fast form, the one of them that holds
    the large table hands on to cross_super; the three of the second band (four rows) take cross_tile."""
    k = 6
    left, right = random_sets(k, 64)
    right = right.copy()
    right[5, 7] = 1 << 16
    for name, table in (('prod', None), ('euclidean', np.full(4 ** k, 1 << 21, dtype=np.int64))):
        if table is not None:
            right[13] = table
        native, kwargs = options(**OPTION_SETS[name])
        with np.errstate(all='ignore'):
            want = np.array([[oracle.profile_distance(l, r, k, **kwargs) for r in right] for l in left], dtype=np.float64)
        assert_separated(want, ('give up', name))
        for tile in ((0, 0), (5, 8)):
            got, names = launched(ctx, lambda: ctx.cross_nearest(left, right, k, native, 4, tile_q=tile[0], tile_r=tile[1]))
            assert_nearest(got, want, 4, name == 'euclidean', ('give up', name, tile))
            fast, tiles = (1, 0) if tile == (0, 0) else (3, 3)
            assert names.get('cross_rdiff' if name == 'prod' else 'cross_gram') == fast, names
            assert names.get('cross_super') == 1 and names.get('cross_tile', 0) == tiles, names


@pytest.mark.parametrize('name', ('prod', 'euclidean', 'cosine', 'positive_scale'))
def test_right_side_in_two_calls(ctx, name):
    k = 6
    left, right = random_sets(k, SEEDS[k])
    want = oracle_rect(k, SEEDS[k], name)
    native = options(**OPTION_SETS[name])[0]
    for n in (3, R):
        one = ctx.cross_nearest(left, right, k, native, n)
        dist, index = ctx.cross_nearest(left, right[:8], k, native, n)
        ctx.cross_nearest(left, right[8:], k, native, n, right_first=8, have=min(n, 8), dist=dist, index=index)
        np.testing.assert_array_equal(index, one[1])
        if name == 'euclidean':
            np.testing.assert_array_equal(dist, one[0])
        assert_nearest((dist, index), want, n, name in BIT_EXACT, ('two calls', name, n))


def test_launches_do_not_grow_with_the_tile(ctx):
    k = 6
    for name in ('prod', 'euclidean', 'scale', 'cosine'):
        native = options(**OPTION_SETS[name])[0]
        counts = []
        for q, r in ((6, 7), (12, 14)):
            left, right = random_sets(k, 65, q, r)
            _, names = launched(ctx, lambda: ctx.cross_nearest(left, right, k, native, 3, tile_q=q, tile_r=r))
            assert names.get('nearest_select') == 1 and names.get('reduce_partials', 0) >= 1, names
            counts.append(sum(names.values()))
        assert counts[0] == counts[1], (name, counts)


def test_arguments(ctx):
    left, right = random_sets(3, 1, 2, 3)
    native = options()[0]
    for kw in (dict(n=0), dict(n=-1), dict(n=65), dict(n=2, have=-1), dict(n=2, have=3), dict(n=2, tile_q=-1), dict(n=2, tile_r=-1)):
        n = kw.pop('n')
        with pytest.raises(ValueError):
            ctx.cross_nearest(left, right, 3, native, n, **kw)
    dist, index = ctx.cross_nearest(left, right, 3, native, 64)
    assert (np.sort(index[:, :3], axis=1) == np.arange(3)).all() and (index[:, 3:] == -1).all() and np.isnan(dist[:, 3:]).all()


FASTQ_READS = 6


def test_nearest_profiles_of_fastq_reads(tmp_path):
    """Six reads counted one profile each (tables in HBM) against five host panel profiles, both sides in chunks."""
    from kpal_amd import klib, kdistlib, metrics
    k, n = 4, 2
    rs = np.random.RandomState(17)
    path = os.path.join(str(tmp_path), 'reads.fq')
    with open(path, 'w') as fh:
        for i in range(FASTQ_READS):
            seq = ''.join(rs.choice(list('ACGT'), 300 + 40 * i, p=(0.1 + 0.05 * (i % 4), 0.3, 0.4 - 0.05 * (i % 4), 0.2)))
            fh.write('@read%d\n%s\n+\n%s\n' % (i, seq, 'I' * len(seq)))
    with open(path) as fh:
        tables = np.stack([np.array(p.counts) for p in klib.Profile.from_fastq_by_record(fh, k)])
    assert tables.shape == (FASTQ_READS, 4 ** k)
    panel = np.stack([rs.poisson(3.0 + 2 * j, 4 ** k) for j in range(5)]).astype(np.int64)
    profiles = [klib.Profile(t.copy(), 'panel%d' % j) for j, t in enumerate(panel)]
    table_bytes = 8 * 4 ** k
    for dist, kwargs in ((kdistlib.ProfileDistance(), dict()),
                         (kdistlib.ProfileDistance(do_scale=True, distance_function=metrics.euclidean), dict(do_scale=True, metric='euclidean'))):
        with np.errstate(all='ignore'):
            want = np.array([[oracle.profile_distance(l, r, k, **kwargs) for r in panel] for l in tables], dtype=np.float64)
        assert_separated(want, ('fastq', kwargs))
        for max_bytes in (None, 2 * table_bytes):
            with open(path) as fh:
                indices, distances = kdistlib.nearest_profiles(klib.Profile.from_fastq_by_record(fh, k), profiles, dist, n, max_bytes=max_bytes)
            assert_nearest((distances, indices), want, n, False, ('fastq', kwargs, max_bytes))
    with open(path) as fh:
        chunks = list(kdistlib.nearest_chunks(klib.Profile.from_fastq_by_record(fh, k), profiles, kdistlib.ProfileDistance(), n,
                                              max_bytes=2 * table_bytes))
    assert [len(c) for c, _, _ in chunks] == [2, 2, 2]


def test_cli_cross_nearest_scaled(tmp_path, tutorial_dir, monkeypatch):
    """``kpal cross --nearest 2 -S`` on the tutorial files counted at k = 8 (HDF5 replaced by tests/memh5.py)."""
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
    want = np.array([[oracle.profile_distance(l, r, k, do_scale=True) for r in tables['right']] for l in tables['left']])
    scaled = want * 1e10   # (no value near a rounding boundary of the tenth decimal: the text cannot hinge on the last bits)
    assert np.all(np.abs(scaled - np.floor(scaled) - 0.5) > 1e-13 * np.maximum(scaled, 1.0))
    if want.shape[1] > 1:
        assert_separated(want, 'cli')
    kmer.main(['cross', 'left.k8', 'right.k8', 'nearest.txt', '--nearest', '2', '-S'])
    lines = []
    for q, name in enumerate(order['left']):
        for r in np.argsort(want[q], kind='stable')[:2]:
            lines.append('%s %s %.10f' % (name, order['right'][r], want[q, r]))
    assert open('nearest.txt').read() == '\n'.join(lines) + '\n'
