"""The plan switches of the table-set kernels that only a LARGE set or a LARGE table crosses, on the GPU, against plain CPU
references (the oracle per table, ``collections.Counter``, ``np.unique``): integers and pairs for equality, mean, std and the
strand balance under the rules of tests/test_gpu_stat_sets.py (``check_stats``, RTOL = 1e-9; no tolerance of this file's own).

  * the pass seam at 65 535 tables (kStatSetMaxProfiles, stat_plan.hpp): the table number is blockIdx.y, so a set of small
    tables is cut there and nowhere else -- 65 605 tables of 4, 16 and 64 bins through kpal_stats_set_device,
    kpal_strand_balance_set_device and kpal_distribution_set_device, every table compared, the tables at both sides of the seam
    alone as well, and the launches of 65 535 tables (one pass) against those of 65 536 (two).  KPAL_STAT_SET_PROFILES, with
    which every other seam test cuts small sets, is unset in every test here.
  * the window cap of the spectra (kSpectrumWindowCap = 2^20, spectrum_plan.hpp), which binds from bins > 2^20 on: 4^11 bins
    with keys at both sides of the cap, a spread of exactly cap - 1 and of exactly cap, and 2^20 + 1 distinct values.
  * the budget seam that follows from the cap: 33 tables of 2^20 bins are passes of 31 and 2.

Measured on an MI355X: the whole file (13 tests) in 5.1 s; the slowest cases are test_stats_past_the_grid (0.85 s each, most
of it the 65 605 oracle calls and their comparison on the host), the strand balance at k = 3 (0.44 s) and the 33 tables of the
budget seam (0.26 s).  Worst difference from the oracle seen over all tables here, in the units RTOL = 1e-9 is applied to: mean
2.4e-16 (of the mean magnitude of the table), std 3.7e-16 and strand balance 6.2e-16 (relative).  Run on the GPU box:
pytest -m gpu; -s prints the three figures."""
import math

import numpy as np
import pytest

import oracle
import test_gpu_spectrum_sets as spectrum_sets
import test_gpu_stat_sets as stat_sets
from test_gpu_stat_sets import RTOL, check_stats, launches, on_device

pytestmark = pytest.mark.gpu

GRID_Y = 65535                   # kStatSetMaxProfiles: the second dimension of a grid
N = GRID_Y + 70
SEAM = (GRID_Y - 1, GRID_Y, N - 1)   # the last table of the first pass, the first and the last one of the second
CAP = 1 << 20                    # kSpectrumWindowCap
SEEN = {'mean': 0.0, 'std': 0.0, 'balance': 0.0}   # the worst differences in units of what the rule allows RTOL of (pytest -s prints them)


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


@pytest.fixture(autouse=True)
def no_cap(monkeypatch):
    monkeypatch.delenv('KPAL_STAT_SET_PROFILES', raising=False)


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    print('\nworst differences from the oracle, relative: %r' % SEEN)


def frozen(tables):
    tables.setflags(write=False)
    return tables


@pytest.fixture(scope='module')
def stat_tables():
    """-> get(bins): (N tables of the kinds of test_gpu_stat_sets.py in turn, their kinds), made once."""
    made = {}

    def get(bins):
        if bins not in made:
            tables, kinds = stat_sets.make_set(7000 + bins, bins, N, shift=bins)
            made[bins] = frozen(tables), kinds
        return made[bins]
    return get


@pytest.fixture(scope='module')
def spectrum_tables():
    """-> get(bins): (N tables of the kinds of test_gpu_spectrum_sets.py in turn, their kinds), made once."""
    made = {}

    def get(bins):
        if bins not in made:
            tables, kinds = spectrum_sets.make_set(8000 + bins, bins, N, shift=bins + 1)
            made[bins] = frozen(tables), kinds
        return made[bins]
    return get


@pytest.fixture(scope='module')
def count_tables(stat_tables):
    """-> get(k): N tables of counts below 1000 for the strand balance: those of stat_tables folded (k <= 2), one Poisson draw
    with a rate per table at k = 3; tables of zeros among them."""
    made = {}

    def get(k):
        if k not in made:
            if k <= 2:
                made[k] = frozen(np.abs(stat_tables(4 ** k)[0]) % 1000)
            else:
                rs = np.random.RandomState(k)
                tables = rs.poisson(rs.choice([0.3, 2.0, 40.0], size=(N, 1)), (N, 4 ** k)).astype(np.int64)
                tables[::97] = 0
                made[k] = frozen(tables)
        return made[k]
    return get


def note(what, got, want, scale):
    if scale > 0:
        SEEN[what] = max(SEEN[what], abs(got - want) / scale)


# ---- A1: sets past 65 535 tables ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bins', (4, 16))
def test_stats_past_the_grid(ctx, stat_tables, bins):
    """Two passes, 65 535 + 70: every summary against the oracle, and the tables next to the seam alone give the same bytes."""
    tables, kinds = stat_tables(bins)
    with on_device(ctx, tables) as ptr:
        got = ctx.stats_set_device(ptr, N, bins)
        assert len(got) == N
        for i in SEAM:
            alone = ctx.stats_set_device(ptr + 8 * bins * i, 1, bins)
            assert bytes(alone[0]) == bytes(got[i]), (bins, i, kinds[i])
    for i in range(N):
        want = oracle.stats(tables[i])
        check_stats(got[i], want, (bins, i, kinds[i]), tables[i])
        note('mean', got[i].mean, want['mean'], float(np.abs(tables[i].astype(np.float64)).mean()))
        note('std', got[i].std, want['std'], abs(want['std']))


@pytest.mark.parametrize('k', (1, 2, 3))
def test_strand_balance_past_the_grid(ctx, count_tables, k):
    tables = count_tables(k)
    with on_device(ctx, tables) as ptr:
        for pairwise, native in (('prod', 0), ('sum', 1)):
            got = ctx.strand_balance_set_device(k, N, ptr, native)
            assert got.shape == (N,) and got.dtype == np.float64
            for i in SEAM:
                alone = ctx.strand_balance_set_device(k, 1, ptr + 8 * 4 ** k * i, native)
                assert alone.tobytes() == got[i:i + 1].tobytes(), (k, pairwise, i)
            for i in range(N):
                want = oracle.strand_balance(tables[i], k, pairwise)
                if math.isnan(want):
                    assert math.isnan(got[i]), (k, i, pairwise)
                else:
                    assert abs(got[i] - want) <= RTOL * abs(want), (k, i, pairwise, got[i], want)
                    note('balance', got[i], want, abs(want))


@pytest.mark.parametrize('bins', (4, 16))
def test_spectra_past_the_grid(ctx, spectrum_tables, bins):
    tables, kinds = spectrum_tables(bins)
    with on_device(ctx, tables) as ptr:
        got = ctx.distribution_set_device(ptr, N, bins)
        alone = [ctx.distribution_set_device(ptr + 8 * bins * i, 1, bins) for i in SEAM]
    spectrum_sets.check(got, tables, (bins, 'past the grid'))
    offsets, values, numbers = got
    for i, (_, v, c) in zip(SEAM, alone):
        a, b = int(offsets[i]), int(offsets[i + 1])
        assert v.tobytes() == values[a:b].tobytes() and c.tobytes() == numbers[a:b].tobytes(), (bins, i, kinds[i])


def test_one_pass_up_to_the_grid_and_two_past_it(ctx, stat_tables, count_tables):
    """65 535 tables are one pass, 65 536 are two: every kernel that runs once per pass.  (The select kernels run once per digit
    of a pass, and the digits of a pass depend on its tables.)"""
    tables, _ = stat_tables(4)
    counts = count_tables(1)
    with on_device(ctx, tables[:GRID_Y + 1]) as ptr, on_device(ctx, counts[:GRID_Y + 1]) as counts_ptr:
        for n, passes in ((GRID_Y, 1), (GRID_Y + 1, 2)):
            got, seen = launches(ctx, lambda: ctx.stats_set_device(ptr, n, 4))
            assert len(got) == n and got[n - 1].total == int(tables[n - 1].sum()), n
            assert [seen.get(name) for name in ('stats_set', 'stats_set_final', 'var_set', 'var_set_final', 'median_set')] == [passes] * 5, (n, seen)
            spectra, seen = launches(ctx, lambda: ctx.distribution_set_device(ptr, n, 4))
            assert spectrum_sets.pairs_of(spectra, n - 1) == spectrum_sets.reference(tables[n - 1]), n
            assert [seen.get(name) for name in ('stats_set', 'spectrum_range', 'spectrum_hist', 'spectrum_nonzero', 'spectrum_scan',
                                                'spectrum_compact')] == [passes] * 6, (n, seen)
            for native in (0, 1):
                scores, seen = launches(ctx, lambda: ctx.strand_balance_set_device(1, n, counts_ptr, native))
                assert len(scores) == n and seen == {'strand_balance_set': passes, 'reduce_partials': passes}, (n, native, seen)


def test_host_entries_equal_the_device_entries_past_the_grid(ctx, stat_tables):
    tables, _ = stat_tables(16)
    with on_device(ctx, tables) as ptr:
        stats = ctx.stats_set_device(ptr, N, 16)
        spectra = ctx.distribution_set_device(ptr, N, 16)
    assert bytes(ctx.stats_set(tables)) == bytes(stats)
    host = ctx.distribution_set(tables)
    assert int(host[0][-1]) == len(host[1]) and all(a.tobytes() == b.tobytes() for a, b in zip(host, spectra))


# ---- A2: the window cap ------------------------------------------------------------------------------------------------------
def same_pairs(result, t, row, what):
    """Table t of ``result`` holds the pairs of ``np.unique(row)``."""
    offsets, values, numbers = result
    a, b = int(offsets[t]), int(offsets[t + 1])
    want_values, want_numbers = np.unique(row, return_counts=True)
    assert np.array_equal(values[a:b], want_values), (what, t)
    assert np.array_equal(numbers[a:b], want_numbers.astype(np.uint64)), (what, t)


def rows_of(result, t):
    offsets, values, numbers = result
    a, b = int(offsets[t]), int(offsets[t + 1])
    return values[a:b].tobytes(), numbers[a:b].tobytes()


def cap_table(rs, bins, smallest, offsets):
    """Poisson counts from ``smallest`` on, and 2 + 3 i entries at smallest + offsets[i], at places of their own."""
    v = rs.poisson(3.0, bins).astype(np.int64) + smallest
    places = rs.permutation(bins)[:4 * len(offsets) * len(offsets) + 8]
    at = 0
    for i, offset in enumerate(offsets):
        v[places[at:at + 2 + 3 * i]] = smallest + offset
        at += 2 + 3 * i
    assert v.min() == smallest and v.max() == smallest + max(offsets)
    return v


@pytest.fixture(scope='module')
def cap_tables():
    """Three tables of 4^11 bins: smallest value 0 and -7 with keys at both sides of the cap, and a narrow one."""
    rs = np.random.RandomState(411)
    bins = 4 ** 11
    edges = (CAP - 2, CAP - 1, CAP, CAP + 1, CAP + 5)
    return frozen(np.stack([cap_table(rs, bins, 0, edges), cap_table(rs, bins, -7, edges), rs.poisson(3.0, bins).astype(np.int64)]))


def test_keys_at_both_sides_of_the_window_cap(ctx, cap_tables):
    """4^11 bins: the window is 2^20 counters, a quarter of the table.  Offsets cap - 2 and cap - 1 are its last counters, cap,
    cap + 1 and cap + 5 the first keys past it; alone and in a set of three, the same bytes."""
    bins = cap_tables.shape[1]
    with on_device(ctx, cap_tables) as ptr:
        three, seen = launches(ctx, lambda: ctx.distribution_set_device(ptr, 3, bins))
        assert seen.get('spectrum_overflow') == 1 and seen['spectrum_hist'] == 1, seen
        alone = []
        for t in (0, 1):
            one, seen = launches(ctx, lambda: ctx.distribution_set_device(ptr + 8 * bins * t, 1, bins))
            assert seen.get('spectrum_overflow') == 1, (t, seen)
            alone.append(one)
    for t in range(3):
        same_pairs(three, t, cap_tables[t], 'three')
    for t in (0, 1):
        assert rows_of(alone[t], 0) == rows_of(three, t), t
        numbers = dict(zip(alone[t][1].tolist(), alone[t][2].tolist()))
        smallest = (0, -7)[t]
        assert [numbers[smallest + e] for e in (CAP - 2, CAP - 1, CAP, CAP + 1, CAP + 5)] == [2, 5, 8, 11, 14], t


def test_a_spread_of_the_cap_fits_the_window_and_one_more_does_not(ctx):
    """Largest - smallest = cap - 1: cap counters hold every key, nothing is listed.  One entry moved to offset cap: one launch
    of the overflow kernel -- and the same pairs as NumPy finds, both times."""
    bins, smallest = 4 ** 11, -7
    rs = np.random.RandomState(20)
    v = cap_table(rs, bins, smallest, (CAP - 2, CAP - 1))
    assert int(v.max()) - int(v.min()) == CAP - 1
    with on_device(ctx, v[None]) as ptr:
        fits, seen = launches(ctx, lambda: ctx.distribution_set_device(ptr, 1, bins))
        assert 'spectrum_overflow' not in seen and seen['spectrum_hist'] == 1, seen
        same_pairs(fits, 0, v, 'cap - 1')
        moved = v.copy()
        moved[np.flatnonzero(moved == smallest + CAP - 1)[0]] = smallest + CAP
        ctx.h2d(ptr, moved)
        past, seen = launches(ctx, lambda: ctx.distribution_set_device(ptr, 1, bins))
        assert seen.get('spectrum_overflow') == 1, seen
        same_pairs(past, 0, moved, 'cap')
    assert past[1][-1] == smallest + CAP and past[2][-1] == 1 and len(past[1]) == len(fits[1]) + 1


def test_a_window_one_counter_short_of_the_table(ctx):
    """2^20 + 1 bins holding every value of [0, bins) once: the window is the cap, one counter short; the value 2^20 is the one
    entry past it."""
    bins = CAP + 1
    v = np.random.RandomState(21).permutation(bins).astype(np.int64)
    with on_device(ctx, v[None]) as ptr:
        (offsets, values, numbers), seen = launches(ctx, lambda: ctx.distribution_set_device(ptr, 1, bins))
    assert seen.get('spectrum_overflow') == 1, seen
    assert offsets.tolist() == [0, bins]
    assert np.array_equal(values, np.arange(bins, dtype=np.int64)) and np.array_equal(numbers, np.ones(bins, dtype=np.uint64))


# ---- A3: the budget seam of the spectra --------------------------------------------------------------------------------------
def test_budget_seam_of_the_spectra(ctx):
    """33 tables of 2^20 bins: 268 435 456 / 8 397 848 = 31 tables a pass, so passes of 31 and 2.  Table 30 (the last one of
    the first pass) and table 32 are wide, so that both passes take the full window; the others hold 30 values.  Tables 30 and
    31 alone -- 31 with a window of its own 30 counters -- give the same bytes as in the set."""
    n, bins = 33, 1 << 20
    rs = np.random.RandomState(33)
    tables = rs.randint(0, 30, size=(n, bins), dtype=np.int64)
    for t in (30, 32):
        places, low = rs.permutation(bins)[:3000], -(1 << 40) - 5
        tables[t, places] = rs.randint(-(1 << 40), 1 << 40, size=3000, dtype=np.int64)
        tables[t, places[0]] = low
        tables[t, places[1:41]] = low + np.repeat([CAP - 1, CAP, CAP + 1, 1 << 30], 10)
    with on_device(ctx, tables) as ptr:
        got, seen = launches(ctx, lambda: ctx.distribution_set_device(ptr, n, bins))
        alone = [ctx.distribution_set_device(ptr + 8 * bins * t, 1, bins) for t in (30, 31)]
    assert seen['spectrum_hist'] == 2 and seen['stats_set'] == 2 and seen['spectrum_overflow'] == 2, seen
    assert len(got[0]) == n + 1 and got[0][0] == 0 and int(got[0][-1]) == len(got[1]) == len(got[2])
    for t in range(n):
        same_pairs(got, t, tables[t], 'budget seam')
    for t, one in zip((30, 31), alone):
        assert rows_of(one, 0) == rows_of(got, t), t
