"""The pool of a set of tables BY LABEL on the GPU at the C-ABI (kpal_pool_groups_device): out[g] = the sum of the tables whose
label is g, int64 wrap.  The expectation is restated here in NumPy -- per group ``tables[labels == g].view(uint64).sum(axis=0)``
as int64 -- and every bin is compared for equality; values reach past +-2^62, so sums wrap.  Every case asserts its launches:
one ("pool_groups") when no member list is cut, two ("pool_groups", "pool_groups_final") otherwise, and nothing for a refused
call.  The shapes are the smallest at which the kernels can still go wrong: tables narrower than a workgroup (64, 256 bins:
several items share one), one and eight column groups, lists of one table, of less than an unroll, of several chunks.
Run on the GPU box: pytest -m gpu."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ('pool_groups', 'pool_groups_final', 'pool_set', 'pool_set_final')


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


@pytest.fixture(scope='module')
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def make_tables(seed, n, bins):
    """Counts of every size: small ones, negative ones, and in every third table values up to +-2^62 and past it."""
    rs = np.random.RandomState(seed)
    tables = rs.randint(-1000, 1 << 20, size=(n, bins)).astype(np.int64)
    tables[1::3] = rs.randint(-(1 << 62), 1 << 62, size=tables[1::3].shape).astype(np.int64) * 2 + 1
    tables[2::7] = 0
    return tables


def expected(tables, labels, n_groups, before=None):
    out = np.zeros((n_groups, tables.shape[1]), dtype=np.uint64) if before is None else before.view(np.uint64).copy()
    for g in range(n_groups):
        members = tables[labels == g]
        if len(members):
            out[g] += members.view(np.uint64).sum(axis=0)
    return out.view(np.int64)


def is_cut(labels, n_groups, bins, num_cu):
    """The rule of pool_groups_plan.hpp, restated: whether some group has more tables than a chunk holds."""
    if bins >= 1 << 20:
        return False
    column_groups = -(-((bins + 1) // 2) // 256)
    chunk_tables = max(16, -(-len(labels) // -(-8 * num_cu // column_groups)))
    counts = np.bincount(labels[labels >= 0], minlength=n_groups)
    return bool(counts.max() > chunk_tables)


class device_buffers(object):
    """Device allocations of the given byte counts, freed at the end."""

    def __init__(self, ctx, *nbytes):
        self.ctx, self.nbytes = ctx, nbytes

    def __enter__(self):
        self.ptrs = [self.ctx.alloc(n) for n in self.nbytes]
        return self.ptrs

    def __exit__(self, *exc):
        self.ctx.sync()
        for p in self.ptrs:
            self.ctx.free(p)


def launches(ctx, call):
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        result = call()
        ctx.sync()
        seen = dict((name, count) for name, (_, count) in ctx.prof_get().items() if count)
    finally:
        ctx.prof_enable(False)
    return result, seen


def fetch(ctx, ptr, shape):
    out = np.empty(shape, dtype=np.int64)
    ctx.d2h(out, ptr)
    return out


def check(ctx, num_cu, tables, labels, n_groups, offset=0, against_pool_set=False):
    """Both values of `accumulate` over rows that held something; -> whether the lists were cut."""
    n, bins = tables.shape
    labels = np.asarray(labels, dtype=np.int64)
    before = np.random.RandomState(n + bins).randint(-(1 << 62), 1 << 62, size=(n_groups, bins)).astype(np.int64)
    want = {0: expected(tables, labels, n_groups), 1: expected(tables, labels, n_groups, before)}
    cut = is_cut(labels, n_groups, bins, num_cu)
    with device_buffers(ctx, tables.nbytes + 16, before.nbytes + 16) as (src, dst):
        src, dst = src + offset, dst + offset
        ctx.h2d(src, tables)
        for accumulate in (0, 1):
            ctx.h2d(dst, before)
            _, seen = launches(ctx, lambda: ctx.pool_groups_device(n, bins, src, labels, n_groups, dst, accumulate=accumulate))
            got = fetch(ctx, dst, before.shape)
            assert seen == ({'pool_groups': 1, 'pool_groups_final': 1} if cut else {'pool_groups': 1}), (bins, n, n_groups, seen)
            assert np.array_equal(got, want[accumulate]), (bins, n, n_groups, accumulate, np.argwhere(got != want[accumulate])[:4])
        if against_pool_set:
            ctx.pool_set_device(n, bins, src, dst)
            assert np.array_equal(fetch(ctx, dst, (bins,)), want[0][0])
        assert np.array_equal(fetch(ctx, src, tables.shape), tables), 'the tables were written'
    return cut


@pytest.fixture(scope='module')
def sets():
    made = {}

    def get(n, bins):
        if (n, bins) not in made:
            made[n, bins] = make_tables(1000 * bins + n, n, bins)
            made[n, bins].setflags(write=False)
        return made[n, bins]
    return get


@pytest.mark.parametrize('n', (1, 40, 3000))
@pytest.mark.parametrize('bins', (64, 256, 1024, 4096))
def test_one_group_of_everything(ctx, num_cu, sets, bins, n):
    """What kpal_pool_set_device gives.  40 tables are more than a chunk of 16: cut, as 3000 are."""
    cut = check(ctx, num_cu, sets(n, bins), np.zeros(n, dtype=np.int64), 1, against_pool_set=True)
    assert cut == (n > 1)


@pytest.mark.parametrize('n', (1, 40, 3000))
@pytest.mark.parametrize('bins', (64, 256, 1024, 4096))
def test_one_group_per_table(ctx, num_cu, sets, bins, n):
    """A copy of the tables (onto rows that held something: their sum with it), in one launch -- in reversed order, so that a
    row is not the table of the same number."""
    cut = check(ctx, num_cu, sets(n, bins), np.arange(n, dtype=np.int64)[::-1].copy(), n)
    assert not cut


def test_skew(ctx, num_cu, sets):
    """2700 of 3000 tables in group 5, 250 groups of one table, 40 groups of none, 50 tables in no group, all interleaved: only
    the long list is cut, the short ones and the empty ones go through the same two launches."""
    n, bins, n_groups = 3000, 64, 291
    labels = np.full(n, 5, dtype=np.int64)
    places = np.random.RandomState(7).permutation(n)
    singles = [g for g in range(n_groups) if g != 5][:250]       # the groups 251 .. 290 stay empty
    labels[places[:250]] = singles
    labels[places[250:300]] = -1 - np.arange(50)
    counts = np.bincount(labels[labels >= 0], minlength=n_groups)
    assert counts[5] == 2700 and (counts == 1).sum() == 250 and (counts == 0).sum() == 40 and (labels < 0).sum() == 50
    assert check(ctx, num_cu, sets(n, bins), labels, n_groups)


def test_odd_rows_and_odd_addresses(ctx, num_cu, sets):
    """An odd number of bins and ranges at odd multiples of 8 bytes: the 8-byte form of the kernel, a last single column."""
    labels = np.arange(40, dtype=np.int64) % 3
    assert not check(ctx, num_cu, sets(40, 1001), labels, 3)
    labels[::5] = -1
    assert not check(ctx, num_cu, sets(40, 64), labels, 3, offset=8)
    assert check(ctx, num_cu, sets(40, 64), np.zeros(40, dtype=np.int64), 2, offset=8)       # cut, and a group of none
    assert check(ctx, num_cu, sets(40, 1001), np.zeros(40, dtype=np.int64), 1)


def test_accumulate_twice_is_twice_the_sums_and_empty_groups_keep_theirs(ctx, sets):
    n, bins, n_groups = 40, 256, 6
    tables = sets(n, bins)
    labels = np.array([0, 3, 3, -1, 5] * 8, dtype=np.int64)      # the groups 1, 2 and 4 are empty
    once = expected(tables, labels, n_groups)
    before = np.arange(n_groups * bins, dtype=np.int64).reshape(n_groups, bins) - 99
    with device_buffers(ctx, tables.nbytes, before.nbytes) as (src, dst):
        ctx.h2d(src, tables)
        ctx.h2d(dst, before)
        ctx.pool_groups_device(n, bins, src, labels, n_groups, dst, accumulate=True)
        ctx.pool_groups_device(n, bins, src, labels, n_groups, dst, accumulate=True)
        got = fetch(ctx, dst, before.shape)
        with np.errstate(over='ignore'):
            assert np.array_equal(got, before + once + once)
        for g in (1, 2, 4):
            assert np.array_equal(got[g], before[g])
        ctx.pool_groups_device(n, bins, src, labels, n_groups, dst, accumulate=False)
        got = fetch(ctx, dst, before.shape)
        assert np.array_equal(got, once) and not got[[1, 2, 4]].any()


def test_large_bins_are_never_cut(ctx, num_cu):
    n, bins = 5, 1 << 20
    tables = make_tables(20, n, bins)
    assert not check(ctx, num_cu, tables, np.array([1, 0, 1, 1, -1], dtype=np.int64), 2)


def test_refusals_launch_nothing(ctx, sets):
    from kpal_amd import _native
    n, bins, n_groups = 40, 64, 3
    tables = sets(n, bins)
    labels = np.arange(n, dtype=np.int64) % 3
    high = labels.copy()
    high[17] = 3
    huge = 1 << 62

    def raw(n_tables, n_bins, groups):
        _native._check(ctx._L.kpal_pool_groups_device(ctx._h, n_tables, n_bins, ctypes.c_void_p(src), ctypes.c_void_p(labels.ctypes.data),
                                                      groups, 0, ctypes.c_void_p(dst)))

    with device_buffers(ctx, 2 * tables.nbytes, n_groups * bins * 8) as (src, dst):
        ctx.h2d(src, tables)
        filled = np.full((n_groups, bins), -1, dtype=np.int64)
        ctx.h2d(dst, filled)
        bad = [
            (lambda: ctx.pool_groups_device(n, bins, 0, labels, n_groups, dst), 'NULL pointer'),
            (lambda: ctx.pool_groups_device(n, bins, src, labels, n_groups, 0), 'NULL pointer'),
            (lambda: ctx.pool_groups_device(n, bins, src, None, n_groups, dst), 'NULL pointer'),
            (lambda: ctx.pool_groups_device(0, bins, src, labels, n_groups, dst), 'empty set'),
            (lambda: ctx.pool_groups_device(n, 0, src, labels, n_groups, dst), 'empty vector'),
            (lambda: ctx.pool_groups_device(n, bins, src, labels, 0, dst), 'no groups'),
            (lambda: ctx.pool_groups_device(n, bins, src + 4, labels, n_groups, dst), 'not 8-byte aligned'),
            (lambda: ctx.pool_groups_device(n, bins, src, labels, n_groups, dst + 4), 'not 8-byte aligned'),
            (lambda: raw(huge, bins, n_groups), 'too many bytes'),
            (lambda: raw(n, bins, huge), 'too many bytes'),
            (lambda: raw(1 << 31, 1, n_groups), 'too many bytes'),                       # more tables than a 32-bit index counts
            (lambda: ctx.pool_groups_device(n, bins, src, high, n_groups, dst), 'table 17 has label 3'),
            (lambda: ctx.pool_groups_device(n, bins, src, labels, n_groups, src), 'overlaps'),
            (lambda: ctx.pool_groups_device(n, bins, src, labels, n_groups, src + 8 * (n * bins - 1)), 'overlaps'),
            (lambda: ctx.pool_groups_device(n, bins, src + 8 * bins, labels, n_groups, src), 'overlaps'),   # the LAST output row reaches them
        ]
        for call, text in bad:
            with pytest.raises(ValueError) as err:
                launches(ctx, call)
            assert text in str(err.value), (text, str(err.value))
        ctx.prof_enable(True)
        try:
            ctx.prof_reset()
            for call, _ in bad:
                with pytest.raises(ValueError):
                    call()
            ctx.sync()
            assert not any(count for _, count in ctx.prof_get().values()), ctx.prof_get()
        finally:
            ctx.prof_enable(False)
        assert np.array_equal(fetch(ctx, dst, filled.shape), filled)
        assert np.array_equal(fetch(ctx, src, tables.shape), tables)
        # a good call afterwards still answers; the output may begin where the tables end
        ctx.pool_groups_device(n, bins, src, labels, n_groups, src + tables.nbytes)
        assert np.array_equal(fetch(ctx, src + tables.nbytes, filled.shape), expected(tables, labels, n_groups))
