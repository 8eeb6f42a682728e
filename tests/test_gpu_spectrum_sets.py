"""The count-of-counts spectra of whole SETS of tables on the GPU (kpal_distribution_set_device, kpal_distribution_set,
kpal_distribution_fetch; kpal/metrics.py:22-33) against the reference's definition, ``sorted(Counter(row).items())``, computed
here: equality is exact.  A table's pairs do not depend on the set it is in, on its place there or on where the passes are cut;
the launches do not grow with the set.  Run on the GPU box: pytest -m gpu.

The two edge constants are spectrum_plan.hpp's: a table's dense window has min(widest spread of the pass, bins, 2^20) counters
from its smallest value on, the first 4096 of them are kept in LDS.  (A value whose number exceeds 2^32 takes a k = 16 table,
32 GiB: no test here can afford it.  Every counter and every number is a 64-bit word by construction.)"""
import collections
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WINDOW_CAP = 1 << 20     # kSpectrumWindowCap
LDS_BINS = 4096          # kSpectrumLdsBins
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
BINS = (1, 63, 64, 4096, 8192, 8193, 4 ** 7)
KINDS = ('zeros', 'constant', 'poisson', 'sparse', 'huge', 'signed', 'extremes', 'distinct', 'window_edge', 'lds_edge')


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


class on_device(object):
    """The rows of a 2-d int64 array as consecutive tables in device memory."""

    def __init__(self, ctx, tables):
        self.ctx, self.tables = ctx, np.ascontiguousarray(tables, dtype=np.int64)

    def __enter__(self):
        self.ptr = self.ctx.alloc(self.tables.nbytes)
        self.ctx.h2d(self.ptr, self.tables)
        return self.ptr

    def __exit__(self, *exc):
        self.ctx.sync()
        self.ctx.free(self.ptr)


def launches(ctx, call):
    """(result, {kernel name: launches}) of ``call()``"""
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        result = call()
        seen = dict((name, count) for name, (_, count) in ctx.prof_get().items() if count)
    finally:
        ctx.prof_enable(False)
    return result, seen


def make_table(rs, bins, kind):
    """One table of ``bins`` entries.  Where a kind needs more entries than there are, what fits is kept."""
    v = np.zeros(bins, dtype=np.int64)

    def put(values):
        """``values`` at distinct random places (as many as fit)"""
        places = rs.permutation(bins)[:len(values)]
        v[places] = np.array(values[:len(places)], dtype=np.int64)

    if kind == 'zeros':
        pass
    elif kind == 'constant':           # one pair whose number spans the slices
        v[:] = 7
    elif kind == 'poisson':
        v[:] = rs.poisson(3.0, bins)
    elif kind == 'sparse':             # 0.1 % non-zero
        hits = rs.permutation(bins)[:max(1, bins // 1000)]
        v[hits] = rs.randint(1, 40, size=len(hits))
    elif kind == 'huge':               # one huge value among small ones: past any window
        v[:] = rs.poisson(1.5, bins)
        put([10 ** 15])
    elif kind == 'signed':
        v[:] = rs.randint(-50, 51, size=bins)
    elif kind == 'extremes':           # the spread does not fit an int64
        v[:] = rs.randint(-3, 4, size=bins)
        put([I64_MIN, I64_MAX, I64_MAX, I64_MIN + 1, I64_MAX - 1])
    elif kind == 'distinct':           # everything but the smallest value lies past the window
        while True:
            v[:] = rs.randint(I64_MIN, I64_MAX, size=bins, dtype=np.int64)
            if len(set(v.tolist())) == bins:
                break
    elif kind == 'window_edge':        # smallest value 0: the window of a pass that holds a wide table ends behind min(bins, cap) - 1
        w = min(bins, WINDOW_CAP)
        put([w - 1, w - 1, w, w, w, w + 1, w - 2])
    else:
        assert kind == 'lds_edge'      # smallest value 0: counter 4095 is the last one in LDS, 4096 the first one past it
        put([LDS_BINS - 1] * 3 + [LDS_BINS] * 2 + [LDS_BINS + 1, LDS_BINS - 2, 2 * LDS_BINS - 1, 2 * LDS_BINS])
    return v


def make_set(seed, bins, n, shift=0):
    """n tables of every kind in turn, the first of kind ``shift``: sets of different (n, shift) mix them in different places."""
    rs = np.random.RandomState(seed)
    kinds = [KINDS[(i + shift) % len(KINDS)] for i in range(n)]
    return np.stack([make_table(rs, bins, kind) for kind in kinds]), kinds


def reference(row):
    return sorted(collections.Counter(row.tolist()).items())


def pairs_of(result, t):
    offsets, values, numbers = result
    a, b = int(offsets[t]), int(offsets[t + 1])
    return list(zip(values[a:b].tolist(), numbers[a:b].tolist()))


def check(result, tables, what):
    offsets, values, numbers = result
    n, bins = tables.shape
    assert offsets.dtype == np.uint64 and values.dtype == np.int64 and numbers.dtype == np.uint64
    assert len(offsets) == n + 1 and offsets[0] == 0 and len(values) == len(numbers) == int(offsets[-1])
    for t in range(n):
        got = pairs_of(result, t)
        assert got == reference(tables[t]), (what, t)
        assert sum(number for _, number in got) == bins and all(number >= 1 for _, number in got)


# ---- every bins x every set ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 3, 300))
@pytest.mark.parametrize('bins', BINS)
def test_sets_vs_counter(ctx, bins, n):
    """1, 3 and 300 tables (the scan of the non-zero counts runs past one workgroup's worth of entries from 8192 bins on) of
    mixed kinds; bins of less than a wave, a whole slice, one bin in the second slice, two slices."""
    tables, kinds = make_set(1000 * n + bins, bins, n, shift=bins + n)
    with on_device(ctx, tables) as ptr:
        check(ctx.distribution_set_device(ptr, n, bins), tables, (bins, n, kinds))


@pytest.mark.parametrize('bins', BINS)
def test_two_pass_seams(ctx, bins, monkeypatch):
    """5 tables in passes of 2, 2 and 1: the pairs of one pass, bit for bit."""
    tables, kinds = make_set(bins, bins, 5, shift=3 + bins % 7)
    with on_device(ctx, tables) as ptr:
        whole, whole_launches = launches(ctx, lambda: ctx.distribution_set_device(ptr, 5, bins))
        monkeypatch.setenv('KPAL_STAT_SET_PROFILES', '2')
        cut, cut_launches = launches(ctx, lambda: ctx.distribution_set_device(ptr, 5, bins))
        monkeypatch.delenv('KPAL_STAT_SET_PROFILES')
    check(cut, tables, (bins, kinds))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, cut))
    assert whole_launches['spectrum_hist'] == 1 and cut_launches['spectrum_hist'] == 3      # the cap was read on that call, and only there


@pytest.mark.parametrize('kind', KINDS)
def test_every_kind_alone_and_in_a_set_of_its_own(ctx, kind):
    """A set of one, and four tables of one kind: the window of the pass is the kind's own (a narrow one for the small counts)."""
    bins = 8193
    rs = np.random.RandomState(KINDS.index(kind))
    tables = np.stack([make_table(rs, bins, kind) for _ in range(4)])
    with on_device(ctx, tables) as ptr:
        check(ctx.distribution_set_device(ptr, 1, bins), tables[:1], kind)
        check(ctx.distribution_set_device(ptr, 4, bins), tables, kind)


def test_scan_past_one_workgroup_of_tables(ctx):
    """1100 tables of 64 bins: one non-zero count per table, more of them than the scan's workgroup has threads."""
    tables, kinds = make_set(11, 64, 1100, shift=2)
    with on_device(ctx, tables) as ptr:
        check(ctx.distribution_set_device(ptr, 1100, 64), tables, 'scan')


def test_window_and_lds_edges(ctx):
    """The counters at both sides of the two edges, counted in one table each: 4^7 bins, smallest value 0, so the window is
    16384 counters wide -- 16383 the last key inside, 16384 the first outside -- and counter 4095 the last one in LDS."""
    bins = 4 ** 7
    w = min(bins, WINDOW_CAP)
    rs = np.random.RandomState(3)
    for edge in (w, LDS_BINS):
        v = np.zeros(bins, dtype=np.int64)
        places = rs.permutation(bins)
        v[places[:300]] = edge - 1
        v[places[300:500]] = edge
        v[places[500:600]] = edge + 1
        v[places[600:650]] = edge - 2
        v[places[650]] = w + 5                       # (so that the widest spread is past the window for the LDS edge too)
        with on_device(ctx, v[None]) as ptr:
            got = pairs_of(ctx.distribution_set_device(ptr, 1, bins), 0)
        want = [(0, bins - 651), (edge - 2, 50), (edge - 1, 300), (edge, 200), (edge + 1, 100), (w + 5, 1)]
        assert got == sorted(want) == reference(v), edge


# ---- a table's pairs do not depend on the set ------------------------------------------------------------------------------
def test_position_independence(ctx, monkeypatch):
    """One table alone, at the front, in the middle and at the end of different sets, with and without a pass seam, twice: the
    same bits.  The sets around it give the pass another window each time."""
    bins = 8193
    rs = np.random.RandomState(5)
    table = make_table(rs, bins, 'poisson')
    table[rs.permutation(bins)[:40]] = rs.randint(-5000, 9000, size=40)     # in LDS, in the global window or past it, by the set
    seen = []
    for n, at, shift, cap in ((1, 0, 0, None), (5, 0, 0, None), (9, 4, 3, None), (4, 3, 6, None), (9, 4, 3, '2'), (3, 1, 1, None), (3, 2, 1, '1')):
        tables, _ = make_set(50 + n, bins, n, shift)
        if (n, at) == (3, 1):
            tables[:] = rs.poisson(2.0, tables.shape)                                # narrow neighbours: the window is this table's own spread
        tables[at] = table
        if cap:
            monkeypatch.setenv('KPAL_STAT_SET_PROFILES', cap)
        with on_device(ctx, tables) as ptr:
            got = ctx.distribution_set_device(ptr, n, bins)
            again = ctx.distribution_set_device(ptr, n, bins)
        if cap:
            monkeypatch.delenv('KPAL_STAT_SET_PROFILES')
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
        a, b = int(got[0][at]), int(got[0][at + 1])
        seen.append((got[1][a:b].tobytes(), got[2][a:b].tobytes()))
    assert len(set(seen)) == 1
    assert list(zip(np.frombuffer(seen[0][0], dtype=np.int64).tolist(), np.frombuffer(seen[0][1], dtype=np.uint64).tolist())) == reference(table)


# ---- launches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kinds,total', ((('poisson', 'sparse', 'signed'), 6), (('poisson', 'huge', 'extremes'), 7)))
def test_launches_do_not_grow_with_the_set(ctx, kinds, total):
    """3 and 300 tables of the same bins and kinds: the same launches -- six, and one more where entries lie past the window."""
    bins = 8193
    seen = []
    for n in (3, 300):
        rs = np.random.RandomState(n)
        tables = np.stack([make_table(rs, bins, kinds[i % 3]) for i in range(n)])
        with on_device(ctx, tables) as ptr:
            got, counts = launches(ctx, lambda: ctx.distribution_set_device(ptr, n, bins))
        assert pairs_of(got, n - 1) == reference(tables[n - 1])
        seen.append(counts)
    assert seen[0] == seen[1], seen
    want = {'stats_set': 1, 'spectrum_range': 1, 'spectrum_hist': 1, 'spectrum_nonzero': 1, 'spectrum_scan': 1, 'spectrum_compact': 1}
    if total == 7:
        want['spectrum_overflow'] = 1
    assert seen[0] == want and sum(seen[0].values()) == total, seen[0]


# ---- the host entry, fetch, errors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('bins', (1, 1001, 8193))
def test_host_entry_equals_the_device_entry(ctx, bins):
    tables, kinds = make_set(bins + 1, bins, 9, shift=4)
    host = ctx.distribution_set(tables)
    check(host, tables, (bins, kinds))
    with on_device(ctx, tables) as ptr:
        device = ctx.distribution_set_device(ptr, 9, bins)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(host, device))
    # other integer types and one table: the Python layer converts
    one = ctx.distribution_set(tables[2:3].astype(np.int32) % 100)
    check(one, (tables[2:3].astype(np.int32) % 100).astype(np.int64), 'int32')


def test_fetch_in_pieces_and_its_errors(ctx):
    from kpal_amd import _native
    L, h = ctx._L, ctx._h
    tables, _ = make_set(21, 1001, 6, shift=2)
    offsets, values, numbers = ctx.distribution_set(tables)
    total = int(offsets[-1])
    assert total > 20
    # in pieces: per table, one pair at a time, nothing at all, twice
    for t in range(6):
        v, c = ctx.distribution_fetch(int(offsets[t]), int(offsets[t + 1] - offsets[t]))
        assert list(zip(v.tolist(), c.tolist())) == reference(tables[t])
    singles = [ctx.distribution_fetch(i, 1) for i in range(total)]
    assert np.concatenate([v for v, _ in singles]).tobytes() == values.tobytes()
    assert np.concatenate([c for _, c in singles]).tobytes() == numbers.tobytes()
    assert L.kpal_distribution_fetch(h, total, 0, None, None) == 0 and L.kpal_distribution_fetch(h, 0, 0, None, None) == 0
    # past the end
    v, c = np.zeros(total + 2, dtype=np.int64), np.zeros(total + 2, dtype=np.uint64)
    for first, count in ((0, total + 1), (total, 1), (total + 1, 0), (1, total), ((1 << 64) - 1, 2), (2, (1 << 64) - 1)):
        rc = L.kpal_distribution_fetch(h, first, count, v.ctypes.data, c.ctypes.data)
        assert rc == _native._E_INVALID, (first, count)
        with pytest.raises(ValueError):
            _native._check(rc)
    assert L.kpal_distribution_fetch(h, 0, 1, None, c.ctypes.data) == _native._E_INVALID
    assert L.kpal_distribution_fetch(None, 0, 1, v.ctypes.data, c.ctypes.data) == _native._E_INVALID
    assert ctx.distribution_fetch(0, total)[0].tobytes() == values.tobytes()          # the pairs are still there
    # nothing pending: a begin call that fails leaves none
    off = np.zeros(8, dtype=np.uint64)
    assert L.kpal_distribution_set(h, 0, 1001, tables.ctypes.data, off.ctypes.data) == _native._E_INVALID
    rc = L.kpal_distribution_fetch(h, 0, 0, v.ctypes.data, c.ctypes.data)
    assert rc == _native._E_INVALID
    with pytest.raises(ValueError):
        ctx.distribution_fetch(0, 1)


def test_argument_errors(ctx):
    """Every misuse of the begin entries is KPAL_E_INVALID (a ValueError), decided before anything is launched."""
    from kpal_amd import _native
    L, h = ctx._L, ctx._h
    tables = np.arange(2 * 256, dtype=np.int64).reshape(2, 256)
    off = np.zeros(3, dtype=np.uint64)
    with on_device(ctx, tables) as ptr:
        def calls():
            for entry, where in ((L.kpal_distribution_set_device, ptr), (L.kpal_distribution_set, tables.ctypes.data)):
                yield entry(None, 2, 256, where, off.ctypes.data)
                yield entry(h, 2, 256, None, off.ctypes.data)
                yield entry(h, 2, 256, where, None)
                yield entry(h, 0, 256, where, off.ctypes.data)
                yield entry(h, 2, 0, where, off.ctypes.data)
                yield entry(h, 1, 256, where + 4, off.ctypes.data)
                yield entry(h, 1 << 40, 1 << 40, where, off.ctypes.data)
        codes, seen = launches(ctx, lambda: list(calls()))
        assert len(codes) == 14 and all(rc == _native._E_INVALID for rc in codes), codes
        for rc in codes:
            with pytest.raises(ValueError):
                _native._check(rc)
        assert seen == {}
        # the Python layer names its own
        with pytest.raises(ValueError):
            ctx.distribution_set(np.zeros((0, 4), dtype=np.int64))
        with pytest.raises(ValueError):
            ctx.distribution_set(np.zeros(16, dtype=np.int64))
        with pytest.raises(TypeError):
            ctx.distribution_set(np.zeros((2, 16)))
        # and the entries still work afterwards
        assert pairs_of(ctx.distribution_set_device(ptr, 2, 256), 1) == [(value, 1) for value in range(256, 512)]


def test_symbols_are_exported(ctx):
    for name in ('kpal_distribution_set_device', 'kpal_distribution_set', 'kpal_distribution_fetch'):
        assert callable(getattr(ctx._L, name))
