"""kpal_cross_nearest[_device] on rows PAST a wave, a register and a chunk of nearest_select_kernel, and on tiles past one trip of
the nearest_finish_* kernels (kpal_amd/csrc/nearest_kernels.hpp).  tests/test_gpu_nearest.py runs Q = 9, R = 21: there lanes
0 .. 20 of wave 0 hold the candidates in register 0, a row is one chunk, a list never holds 64, and the finish kernels are one
workgroup.  Here a row has 4500 candidates (tests/nearest_cases.py; tests/test_nearest_cases_host.py asserts on the CPU what the
cases below rely on).

Every expected distance is ``oracle.profile_distance`` on that pair, every expected index ``np.argsort(kind='stable')`` of the
oracle's row.  Contract as in test_gpu_nearest.py: unscaled euclidean and cosine bit for bit, ties and NaN included; the other
option sets within 1e-9 relative, after asserting that the first n + 1 sorted oracle values of every row they are held on lie
more than 1e-6 apart.

Which case reaches what (a row of a tile: chunks of 2048 candidates, 8 registers a thread, 4 waves; finish trips at 256 compute
units):

    case                                  tiles          chunks a row    registers   waves   list        finish trips
    wide, caps (0, 0)                     1              3 (.., 404)     8           4       up to 64    1
    wide, caps (4, 2500)                  2 x 2          2 and 1         8           4       had = 64    1
    wide, caps (0, 2048)                  3              1 (exactly)     8           4       had = 64    1
    wide, caps (0, 2049)                  3              2 (.., 1)       8           4       had = 64    1
    wide, caps (5, 300)                   2 x 15         1               2           4       had = 64    1
    sparse cosine                         1 and 2        2 and 1         8           4       NaN give way
    two calls, right[2100:] first         1 + 1          2 and 2         8           4       have = 64 from the caller
    right_first = 2^40                    1              3               8           4       indices past 32 bits
    finish, 130 x 4100 (k = 3, k = 6)     1              3               8           4       8           2 (pairs past cu * 2048)
    smoothing, 3 x 300                    1 and 2 x 3    (host merge)                        up to 64
    nearest_profiles, max_bytes           3 calls a row  2, 2 and 1      8           4       have = 64 over device chunks

The smoothed case holds one right table three times (columns 5, 69 and 261, planted for the ties of another row): for those
the oracle's values are equal, and an option set held to 1e-9 does not promise equal doubles for them from different tiles.
So there the indices are held up to which copy of that table stands where, the list must be in the library's order by its
own doubles, and rows without copies among their first n + 1 go through assert_nearest as everywhere else.

Measured on an MI355X (256 compute units): 28 tests, 17 s for this file run alone -- 4.3 s in the tests (the slowest: k = 6,
130 x 4100 at 0.9 s, most of it drawing 17 million Poisson counts), the rest the first test's fixtures (the context, and
torch's query of the device).  Worst relative difference from the oracle per option set held to 1e-9: prod 3.8e-16, scale
3.0e-16, positive_scale 3.0e-16, balance 3.6e-16, smooth 2.9e-16, prod at 130 x 4100 2.3e-16; euclidean and cosine equal it
bit for bit.  No kernel needed a change.

Checked once by hand, not part of the suite: scratch builds of the library with one slip each (all give wrong results, none
a fault), tests/test_gpu_nearest.py (34 tests) and this file against each:
    the selection's `mine[i]` loop cut to `i < 1`                 test_gpu_nearest.py green; 26 fail here (all but smoothing)
    the cross-wave minimum over slot 0 alone (`w < 1`)            test_gpu_nearest.py green; 26 fail here
    `old` read while `tid < have` in place of `tid < count`       test_gpu_nearest.py green; 21 fail here -- every case with a
      (the list is lost from the second chunk on)                   second chunk; caps (0, 2048), (5, 300) and smoothing pass
    `p += pairs` as the step of both finish kernels (one trip)    test_gpu_nearest.py green; test_finish_second_trip fails, twice
    `cur ^= 1` left out                                           31 of test_gpu_nearest.py fail already (the list written is
                                                                    never the one stored, at any width); 26 fail here
"""
import numpy as np
import pytest

import nearest_cases as nc
from test_gpu_nearest import BIT_EXACT, GAP, OPTION_SETS, RTOL, assert_nearest, launched, options, random_sets

pytestmark = pytest.mark.gpu

NS = (1, 5, 6, 63, 64)
# (tile_q, tile_r) -> tiles of the 6 x 4500 rectangle
CAPS = {(0, 0): 1, (4, 2500): 4, (0, 2048): 3, (0, 2049): 3, (5, 300): 30}
TOLERANCE_ROWS = [0, 1, 2, 4]


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


@pytest.fixture(scope='module')
def cu():
    """Compute units of the part: the device property kpal_ctx sizes its grids with."""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def wide_rect(name):
    left, right = nc.wide_sets()
    return nc.oracle_rect(('wide', name), left, right, nc.K, options(**OPTION_SETS[name])[1])


def tiles_of(caps, q=nc.Q, r=nc.R):
    tq, tr = min(q, caps[0] or q), min(r, caps[1] or r)
    return -(-q // tq) * -(-r // tr)


# ---- a. wide rows, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('caps', sorted(CAPS), ids=lambda c: '%dx%d' % c)
@pytest.mark.parametrize('name', BIT_EXACT)
def test_wide_rows_bit_exact(ctx, name, caps):
    """All six rows.  k = 3 is not staged: euclidean is cross_tile and nearest_finish_slots_kernel, cosine the option route."""
    left, right = nc.wide_sets()
    want = wide_rect(name)
    native = options(**OPTION_SETS[name])[0]
    assert tiles_of(caps) == CAPS[caps]
    for n in NS:
        got, names = launched(ctx, lambda: ctx.cross_nearest(left, right, nc.K, native, n, tile_q=caps[0], tile_r=caps[1]))
        assert_nearest(got, want, n, True, ('wide', name, n, caps))
        assert names.get('nearest_select') == CAPS[caps] and names.get('nearest_finish') == CAPS[caps], names
        assert 'cross_gram' not in names and 'nearest_finish_gram' not in names, names
        if name == 'euclidean':
            assert names.get('cross_tile') == CAPS[caps], names


# ---- b. wide rows, within 1e-9 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('caps', [(0, 0), (4, 2500)], ids=lambda c: '%dx%d' % c)
@pytest.mark.parametrize('name', ('prod', 'scale', 'positive_scale', 'balance'))
def test_wide_rows_tolerance(ctx, name, caps):
    """Rows 0, 1, 2 and 4 (row 3 is ties, row 5 NaN under scale)."""
    left, right = nc.wide_sets()
    left = left[TOLERANCE_ROWS]
    want = wide_rect(name)[TOLERANCE_ROWS]
    native = options(**OPTION_SETS[name])[0]
    for n in NS:
        gap = nc.gaps(want, n)
        assert gap.min() > GAP, (name, n, gap)
        got, names = launched(ctx, lambda: ctx.cross_nearest(left, right, nc.K, native, n, tile_q=caps[0], tile_r=caps[1]))
        assert_nearest(got, want, n, False, ('wide', name, n, caps))
        assert names.get('nearest_select') == tiles_of(caps, q=len(left)), names


# ---- c. sparse cosine ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('caps', [(0, 0), (0, 2048)], ids=lambda c: '%dx%d' % c)
def test_sparse_cosine(ctx, caps):
    """Ten numbers in a row of NaN: the NaN that fill a list in chunk 0 give way to the numbers of chunk 1 (of the second
    tile), those that stay are in index order."""
    left, right = nc.sparse_sets()
    native, kwargs = options(**OPTION_SETS['cosine'])
    want = nc.oracle_rect(('sparse', 'cosine'), left, right, nc.K, kwargs)
    assert (np.isfinite(want).sum(axis=1) == 10).all()
    for n in (4, 10, 11, 64):
        got = ctx.cross_nearest(left, right, nc.K, native, n, tile_q=caps[0], tile_r=caps[1])
        assert_nearest(got, want, n, True, ('sparse', n, caps))
        if n > 10:
            assert np.isnan(got[0][:, 10:]).all() and (got[1][:, 10:12] == np.arange(min(2, n - 10))).all()


# ---- d. the right side in two calls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (3, 64))
def test_right_side_in_two_calls_at_width(ctx, n):
    """The upper part first: a carried list of n (64: the full list) whose every entry has a higher index than what arrives --
    ties against a carried candidate go to the later, lower index (row 3; row 4's own)."""
    left, right = nc.wide_sets()
    want = wide_rect('euclidean')
    native = options(**OPTION_SETS['euclidean'])[0]
    cut = 2100
    one = ctx.cross_nearest(left, right, nc.K, native, n)
    dist, index = ctx.cross_nearest(left, right[cut:], nc.K, native, n, right_first=cut)
    assert_nearest((dist.copy(), index.copy()), want[:, cut:], n, True, ('upper part', n), first=cut)
    ctx.cross_nearest(left, right[:cut], nc.K, native, n, right_first=0, have=n, dist=dist, index=index)
    np.testing.assert_array_equal(index, one[1])
    np.testing.assert_array_equal(dist.view(np.int64), one[0].view(np.int64))
    assert_nearest((dist, index), want, n, True, ('carried', n))


# ---- e. indices past 32 bits -----------------------------------------------------------------------------------------------------
def test_indices_past_32_bits(ctx):
    left, right = nc.wide_sets()
    want = wide_rect('euclidean')
    native = options(**OPTION_SETS['euclidean'])[0]
    for n in (5, 64):
        got = ctx.cross_nearest(left, right, nc.K, native, n, right_first=2 ** 40)
        assert got[1].min() >= 2 ** 40
        assert_nearest(got, want, n, True, ('2^40', n), first=2 ** 40)


# ---- f. the finish kernels past one trip -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,name', [(3, 'prod'), (6, 'euclidean')], ids=['k3_prod_slots', 'k6_euclidean_gram'])
def test_finish_second_trip(ctx, cu, k, name):
    """One tile of 130 x 4100 pairs: more than the cu * 8 workgroups of 256 threads the finish kernels are capped at take in
    one trip.  Every row against the rectangle entry (the same doubles, the stable order of them); the rows the second trip
    writes, and the one that straddles it, against the oracle."""
    Qf, Rf, n = 130, 4100, 8
    assert Qf * Rf > cu * 2048, (Qf, Rf, cu)
    left, right = random_sets(k, 90 + k, Qf, Rf)
    native, kwargs = options(**OPTION_SETS[name])
    rect = ctx.cross_profile_distance(left, right, k, native)
    (dist, index), names = launched(ctx, lambda: ctx.cross_nearest(left, right, k, native, n))
    assert names.get('nearest_select') == 1, names
    if k == 6:
        assert names.get('cross_gram') == 1 and names.get('nearest_finish_gram') == 1 and 'nearest_finish' not in names, names
    else:
        assert names.get('nearest_finish') == 1 and 'nearest_finish_gram' not in names, names
    np.testing.assert_array_equal(index, np.argsort(rect, axis=1, kind='stable')[:, :n])
    np.testing.assert_array_equal(dist.view(np.int64), np.take_along_axis(rect, index, axis=1).view(np.int64))
    start = cu * 2048 // Rf - 1
    assert 0 <= start < Qf - 1
    want = nc.oracle_rect(('trip', k, start), left[start:], right, k, kwargs)
    if name not in BIT_EXACT:
        assert nc.gaps(want, n).min() > GAP
    assert_nearest((dist[start:], index[start:]), want, n, name in BIT_EXACT, ('second trip', k, name))


# ---- g. dynamic smoothing: the host merge ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('caps', [(0, 0), (2, 128)], ids=lambda c: '%dx%d' % c)
def test_smoothed_host_merge(ctx, caps):
    left, right = nc.wide_sets()
    left, right = left[:3], right[:300]
    native, kwargs = options(**OPTION_SETS['smooth'])
    want = nc.oracle_rect(('smooth',), left, right, nc.K, kwargs)
    first = nc.copies(right)
    for n in (5, 64):
        assert nc.gaps(want, n, right).min() > GAP, n
        dist, index = ctx.cross_nearest(left, right, nc.K, native, n, tile_q=caps[0], tile_r=caps[1])
        assert dist.shape == index.shape == (3, n)
        order = np.argsort(want, axis=1, kind='stable')[:, :n]
        expect = np.take_along_axis(want, order, axis=1)
        # which table stands where; no column twice; 1e-9; in the library's order by its own doubles
        np.testing.assert_array_equal(first[index], first[order], err_msg=str((n, caps)))
        assert all(len(set(row)) == n for row in index)
        err = np.abs(dist - expect) / np.abs(expect)
        print('smooth %s n = %d: worst relative difference %.3g' % (caps, n, err.max()))
        assert (err <= RTOL).all(), (n, caps, float(err.max()))
        assert ((dist[:, 1:] > dist[:, :-1]) | ((dist[:, 1:] == dist[:, :-1]) & (index[:, 1:] > index[:, :-1]))).all(), (n, caps)
        rows = np.flatnonzero(nc.gaps(want, n) > GAP)
        assert len(rows) >= 2
        assert_nearest((dist[rows], index[rows]), want[rows], n, False, ('smooth', n, caps))


# ---- h. kdistlib.nearest_profiles over device chunks of the right side -----------------------------------------------------------
def test_nearest_profiles_in_device_chunks(ctx):
    """Right chunks of 2100, 2100 and 300 profiles: `have` and `right_first` carried over calls with a full list of 64."""
    from kpal_amd import klib, kdistlib, metrics
    left, right = nc.wide_sets()
    want = wide_rect('euclidean')
    lp = [klib.Profile(t.copy(), 'left%d' % i) for i, t in enumerate(left)]
    rp = [klib.Profile(t.copy(), 'right%d' % i) for i, t in enumerate(right)]
    max_bytes = 2100 * 8 * nc.BINS
    assert kdistlib.cross_chunks(8 * nc.BINS, nc.R, max_bytes) == [(0, 2100), (2100, 4200), (4200, 4500)]
    dist = kdistlib.ProfileDistance(distance_function=metrics.euclidean)
    (indices, distances), names = launched(ctx, lambda: kdistlib.nearest_profiles(lp, rp, dist, nc.NMAX, max_bytes=max_bytes))
    assert names.get('nearest_select') == 3, names
    assert_nearest((distances, indices), want, nc.NMAX, True, 'nearest_profiles')
