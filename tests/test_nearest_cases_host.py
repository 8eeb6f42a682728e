"""What tests/test_gpu_nearest_rows.py relies on in the inputs of tests/nearest_cases.py, asserted on the CPU from the oracle
alone: the planted prefixes, which chunks, waves and registers of nearest_select_kernel the best of a row come from, the NaN
structure of the sparse sets, the separation the tolerance metrics need, and that each of five plausible wrong selections
changes what the GPU tests expect.  A change of seed or shape fails here instead of quietly weakening the GPU tests."""
import numpy as np
import pytest

import nearest_cases as nc
from test_gpu_nearest import BIT_EXACT, GAP, OPTION_SETS, options

# the option sets of test_gpu_nearest_rows.py that are held to 1e-9, and the rows they are held on
TOLERANCE_SETS = ('prod', 'sum', 'balance', 'scale', 'positive_scale')
TOLERANCE_ROWS = [0, 1, 2, 4]
NS = (1, 5, 6, 63, 64)


def wide_rect(name):
    left, right = nc.wide_sets()
    return nc.oracle_rect(('wide', name), left, right, nc.K, options(**OPTION_SETS[name])[1])


def test_shapes():
    left, right = nc.wide_sets()
    assert left.shape == (nc.Q, nc.BINS) and right.shape == (nc.R, nc.BINS) and left.dtype == right.dtype == np.int64
    assert [min(nc.CHUNK, nc.R - c) for c in range(0, nc.R, nc.CHUNK)] == [2048, 2048, 404]
    assert not left[5].any() and right.any(axis=1).all() and left[:5].any(axis=1).all()
    planted = [at for p in nc.PLANTED.values() for at in p]
    assert len(set(planted)) == len(planted) == 64 + 64 + 12 + 6
    for j in (0, 7, 63):
        d = nc.near(left[0], j) - left[0]
        assert d.sum() == j + 1 and set(d) <= {0, 1}


def test_planted_prefixes():
    """Under euclidean the stable order of rows 0 to 3 begins with exactly the planted positions in the planted order, at
    exactly sqrt(j + 1) (row 3: six times 1.0)."""
    want = wide_rect('euclidean')
    order = np.argsort(want, axis=1, kind='stable')
    for row, planted in nc.PLANTED.items():
        assert list(order[row, :len(planted)]) == planted, row
    for row in (0, 1, 2):
        m = len(nc.PLANTED[row])
        np.testing.assert_array_equal(want[row, order[row, :m]], np.sqrt(np.arange(1, m + 1)))
        assert want[row, order[row, m]] > np.sqrt(m + 1)
    assert (want[3, nc.TIES] == 1.0).all() and want[3, order[3, 6]] > 1.0
    assert nc.TIES == sorted(nc.TIES)
    # where the planted tables sit
    assert set(nc.where(nc.LATE)[0]) == {2} and nc.LATE == sorted(nc.LATE, reverse=True)
    c, reg, wave, _ = nc.where(nc.EARLY)
    assert set(c) == {0} and set(reg) == set(range(nc.PER)) and set(wave) == {0, 1, 2, 3}
    c, reg, wave, lane = (list(a) for a in nc.where(nc.EDGES))
    slots = list(zip(c, reg, wave, lane))
    assert slots[:5] == [(0, 7, 3, 63), (1, 0, 0, 0), (1, 7, 3, 63), (2, 0, 0, 0), (2, 1, 1, 19)]
    assert slots[5:] == [(0, 0, 0, 0), (0, 0, 3, 63), (0, 1, 0, 0), (0, 0, 0, 63), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 0, 1)]
    c, reg, wave, lane = nc.where(nc.TIES)
    assert set(c) == {0, 1, 2} and len(set(zip(c, reg, wave))) == 6 and set(lane) == {5, 48}


@pytest.mark.parametrize('name', BIT_EXACT)
def test_coverage(name):
    """The 64 best of rows 2 to 5 come from all three chunks; those of row 4, random tables only, from every wave and every
    register.  Row 4 has exact ties of its own among its 65 best under euclidean.  Row 5 is NaN throughout under cosine: its
    best are columns 0 to 63."""
    want = wide_rect(name)
    order = np.argsort(want, axis=1, kind='stable')[:, :nc.NMAX]
    for row in (2, 3, 4, 5) if name == 'euclidean' else (2, 3, 4):
        c, reg, wave, _ = nc.where(order[row])
        print(name, 'row', row, 'chunks', np.bincount(c, minlength=3), 'registers', np.bincount(reg, minlength=8), 'waves', np.bincount(wave, minlength=4))
        assert set(c) == {0, 1, 2}, (name, row)
        if row == 4 or (row == 5 and name == 'euclidean'):
            assert set(reg) == set(range(nc.PER)) and set(wave) == {0, 1, 2, 3}, (name, row)
    if name == 'euclidean':
        s = np.sort(want[4])[:nc.NMAX + 1]
        assert (s[1:] == s[:-1]).sum() >= 3
        assert np.isfinite(want).all()
    else:
        assert np.isnan(want[5]).all() and np.isfinite(want[:5]).all()
        assert list(order[5]) == list(range(nc.NMAX))


def test_scale_is_nan_on_the_zero_profile():
    for name in ('scale', 'positive_scale'):
        want = wide_rect(name)
        assert np.isnan(want[5]).all() and np.isfinite(want[:5]).all(), name


@pytest.mark.parametrize('name', TOLERANCE_SETS)
def test_separation(name):
    """Rows 0, 1, 2 and 4: neighbours among the first n + 1 sorted oracle values differ by more than GAP relative, so that a
    result within 1e-9 cannot reorder them or change which n are kept."""
    want = wide_rect(name)[TOLERANCE_ROWS]
    for n in NS:
        g = nc.gaps(want, n)
        print(name, n, g)
        assert g.min() > GAP, (name, n, g)
    assert nc.gaps(want, nc.NMAX + 1).min() > 1.6e-6, name


def test_separation_smoothed():
    """left[:3] against right[:300] under dynamic smoothing.  Columns 5, 69 and 261 hold one table three times (TIES): those
    three are one candidate under three indices and the only neighbours that are not apart."""
    left, right = nc.wide_sets()
    right = right[:300]
    want = nc.oracle_rect(('smooth',), left[:3], right, nc.K, options(**OPTION_SETS['smooth'])[1])
    first = nc.copies(right)
    assert {i: f for i, f in enumerate(first) if i != f} == {69: 5, 261: 5}
    for n in (5, 64):
        assert nc.gaps(want, n, right).min() > GAP, n
    assert nc.gaps(want, 5).min() > GAP and nc.gaps(want, 64)[0] == 0 and nc.gaps(want, 64)[1:].min() > GAP


def test_sparse_structure():
    """Cosine on the sparse sets: ten numbers, then NaN at 0, 1, 2, ... with the ten positions skipped; chunk 0 of a row alone
    fills a list of 64 with six numbers and NaN, chunk 1 brings four more numbers."""
    left, right = nc.sparse_sets()
    assert left.shape == (2, nc.BINS) and right.shape == (nc.SPARSE_R, nc.BINS) and nc.CHUNK < nc.SPARSE_R <= 2 * nc.CHUNK
    np.testing.assert_array_equal(left, nc.wide_sets()[0][:2])
    assert sorted(np.flatnonzero(right.any(axis=1))) == sorted(nc.SPARSE_AT) and len(set(nc.SPARSE_AT)) == 10
    assert sum(at < nc.CHUNK for at in nc.SPARSE_AT) == 6
    want = nc.oracle_rect(('sparse', 'cosine'), left, right, nc.K, options(**OPTION_SETS['cosine'])[1])
    rest = [r for r in range(nc.SPARSE_R) if r not in nc.SPARSE_AT]
    for row in range(2):
        assert sorted(np.flatnonzero(np.isfinite(want[row]))) == sorted(nc.SPARSE_AT) and np.isnan(want[row, rest]).all()
        order = np.argsort(want[row], kind='stable')
        assert sorted(order[:10]) == sorted(nc.SPARSE_AT) and list(order[10:]) == rest
        assert nc.gaps(want[row:row + 1, nc.SPARSE_AT], 9).min() > 0
        # the best ten hold a number of chunk 1 in front of one of chunk 0: a merge, not an append
        assert any(a >= nc.CHUNK and b < nc.CHUNK for a, b in zip(order[:9], order[1:10]))


# ---- wrong selections ----------------------------------------------------------------------------------------------------------
def _kept(name):
    """The columns of a one-tile row of R candidates that a wrong nearest_select_kernel would still look at."""
    c, reg, wave, _ = nc.where(np.arange(nc.R))
    return {'register 0 only': reg == 0, 'wave 0 only': wave == 0, 'last register dropped': reg != nc.PER - 1,
            'first chunk lost': c != 0, 'last chunk lost': c != 2}[name]


WRONG = ('register 0 only', 'wave 0 only', 'last register dropped', 'first chunk lost', 'last chunk lost')


@pytest.mark.parametrize('wrong', WRONG)
@pytest.mark.parametrize('name', BIT_EXACT)
def test_wrong_selections_show(name, wrong):
    """The best 64 among the columns a wrong kernel keeps differ from the best 64 of the row in at least one row (plain numpy)."""
    want = wide_rect(name)
    keep = np.flatnonzero(_kept(wrong))
    right = np.argsort(want, axis=1, kind='stable')[:, :nc.NMAX]
    got = keep[np.argsort(want[:, keep], axis=1, kind='stable')[:, :nc.NMAX]]
    rows = [row for row in range(nc.Q) if not np.array_equal(right[row], got[row])]
    print(name, wrong, 'rows that differ:', rows)
    assert rows, (name, wrong)
