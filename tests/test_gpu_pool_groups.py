"""The pool of a set of tables BY LABEL on the GPU at the C-ABI (kpal_pool_groups_device): out[g] = the sum of the tables whose
label is g, int64 wrap.  The expectation is restated here in NumPy -- per group ``tables[labels == g].view(uint64).sum(axis=0)``
as int64 -- and every bin is compared for equality; values reach past +-2^62, so sums wrap.  Every case asserts its launches:
one ("pool_groups") when no member list is cut, two ("pool_groups", "pool_groups_final") otherwise, and nothing for a refused
call.  The shapes are the smallest at which the kernels can still go wrong: tables narrower than a workgroup (64, 256 bins:
several items share one), one and eight column groups, lists of one table, of less than an unroll, of several chunks.

Every packing of small tables is launched: an item takes 2^shift threads, shift 0 (one or two bins, 256 items to a workgroup)
to 8 (one item); up to shift 5 several items share a wave and the bounds of their lists differ lane by lane, from shift 6 on
the item is the same for a wave and is taken through readfirstlane.  PACKED_BINS reaches the shifts that 64 (5), 256 (7) and
the larger bins (8) leave out, in the 16-byte and in the 8-byte form.  More workgroups of items than a grid is high
(65 535) take a second trip of the kernel's stride: 65 605 groups of 512 bins, the smallest shape that has one.

Measured on an MI355X: the whole file (133 tests) in 13.7 s, 11.5 s of it the start of the first context; the slowest cases
are one group of 3000 tables of 4096 bins (0.21 s) and test_more_item_workgroups_than_a_grid_is_high (0.18 s: two uploads and two
downloads of 268 MB); every packing case takes 0.03 s or less.
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


def skewed_labels():
    """-> (labels of 3000 tables, 291 groups): 2700 tables in group 5, 250 groups of one table, 40 groups of none, 50 tables in
    no group, all interleaved."""
    n, n_groups = 3000, 291
    labels = np.full(n, 5, dtype=np.int64)
    places = np.random.RandomState(7).permutation(n)
    singles = [g for g in range(n_groups) if g != 5][:250]       # the groups 251 .. 290 stay empty
    labels[places[:250]] = singles
    labels[places[250:300]] = -1 - np.arange(50)
    counts = np.bincount(labels[labels >= 0], minlength=n_groups)
    assert counts[5] == 2700 and (counts == 1).sum() == 250 and (counts == 0).sum() == 40 and (labels < 0).sum() == 50
    return labels, n_groups


def test_skew(ctx, num_cu, sets):
    """2700 of 3000 tables in group 5, 250 groups of one table, 40 groups of none, 50 tables in no group, all interleaved: only
    the long list is cut, the short ones and the empty ones go through the same two launches."""
    labels, n_groups = skewed_labels()
    assert check(ctx, num_cu, sets(3000, 64), labels, n_groups)


# ---- every packing of small tables ---------------------------------------------------------------------------------------------
PACKED_BINS = (1, 2, 3, 4, 5, 16, 17, 32, 100, 128, 129)
PACKED_SHIFT = {1: 0, 2: 0, 3: 1, 4: 1, 5: 2, 16: 3, 17: 4, 32: 4, 100: 6, 128: 6, 129: 7}
PACKED = [(bins, 0) for bins in PACKED_BINS] + [(bins, 8) for bins in PACKED_BINS if bins % 2 == 0]   # (bins, byte offset of both ranges)


def lane_shift(bins):
    """The rule of pool_groups_plan.hpp (pool_groups_lane_shift), restated: log2 of the power of two of threads that holds the
    column pairs of a table, 8 at most."""
    pairs, shift = (bins + 1) // 2, 0
    while shift < 8 and (1 << shift) < pairs:
        shift += 1
    return shift


def test_packed_bins_reach_every_shift_the_other_tests_leave_out():
    """(tests/test_pool_groups_plan_host.py asks the header itself for the same literals: a change of the rule fails there.)"""
    assert dict((bins, lane_shift(bins)) for bins in PACKED_BINS) == PACKED_SHIFT
    assert sorted(set(PACKED_SHIFT.values()) | set(lane_shift(bins) for bins in (64, 256, 1001, 1024, 4096))) == list(range(9))
    # 3000 items leave the last workgroup ragged up to shift 4 (16 items to a workgroup); four and two items divide 3000, there
    # the 291 groups of the skewed labelling do
    assert all(3000 % (256 >> shift) != 0 for shift in PACKED_SHIFT.values() if shift <= 4)
    assert all(291 % (256 >> shift) != 0 for shift in PACKED_SHIFT.values())


@pytest.mark.parametrize('n', (40, 3000))
@pytest.mark.parametrize('bins,offset', PACKED)
def test_packed_one_group_of_everything(ctx, num_cu, sets, bins, offset, n):
    """Cut both times: the first pass has as many items as there are chunks, the second pass one."""
    assert check(ctx, num_cu, sets(n, bins), np.zeros(n, dtype=np.int64), 1, offset=offset)


@pytest.mark.parametrize('n', (1, 3000))
@pytest.mark.parametrize('bins,offset', PACKED)
def test_packed_one_group_per_table(ctx, num_cu, sets, bins, offset, n):
    """One item of one table per group, in reversed order; 3000 items fill no whole number of workgroups."""
    assert not check(ctx, num_cu, sets(n, bins), np.arange(n, dtype=np.int64)[::-1].copy(), n, offset=offset)


@pytest.mark.parametrize('bins,offset', PACKED)
def test_packed_fewer_groups_than_a_workgroup_has_items(ctx, num_cu, sets, bins, offset):
    """One workgroup with idle items: one group fewer than it has room for (one group where it takes two)."""
    per = 256 >> lane_shift(bins)
    n_groups = max(1, per - 1)
    labels = np.arange(40, dtype=np.int64) * 7 % n_groups
    labels[3::11] = -1
    check(ctx, num_cu, sets(40, bins), labels, n_groups, offset=offset)


@pytest.mark.parametrize('bins,offset', PACKED)
def test_packed_skew(ctx, num_cu, sets, bins, offset):
    """The labelling of test_skew: lists of 2700, of one and of none in the lanes of one wave."""
    labels, n_groups = skewed_labels()
    assert check(ctx, num_cu, sets(3000, bins), labels, n_groups, offset=offset)


# ---- the stride over the workgroups of items -------------------------------------------------------------------------------------
def test_more_item_workgroups_than_a_grid_is_high(ctx, num_cu):
    """512 bins are one column group and one item to a workgroup, so 65 535 + 70 groups are 70 more workgroups of items than the
    grid is high: the workgroups 0 .. 69 take a second item, 65 535 further on.  The whole output is compared, 268 MB -- the
    least any shape with a second trip takes (65 535 workgroups x 256 threads x 16 bytes) -- with accumulate = 0 over rows of -1
    (a group of no table, on either trip, writes zeros) and accumulate = 1 over a pattern (and keeps what it holds)."""
    n, bins, n_groups = 300, 512, 65535 + 70
    rs = np.random.RandomState(512)
    tables = make_tables(512, n, bins)
    labels = rs.randint(0, n_groups, size=n).astype(np.int64)
    labels[:14] = [0, 1, 65534, 65535, 65536, n_groups - 1, 65535, 65535, 65536, n_groups - 1, 0, 65534, 65600, 65600]
    labels[20:30] = 65570                                         # ten tables in one group of the second trip
    labels[40:50] = -1
    assert lane_shift(bins) == 8 and not is_cut(labels, n_groups, bins, num_cu)
    sums = np.zeros((n_groups, bins), dtype=np.uint64)
    np.add.at(sums, labels[labels >= 0], tables[labels >= 0].view(np.uint64))
    got = np.empty((n_groups, bins), dtype=np.int64)
    with device_buffers(ctx, tables.nbytes, got.nbytes) as (src, dst):
        ctx.h2d(src, tables)
        for accumulate in (0, 1):
            before = np.full(got.shape, -1, dtype=np.int64) if accumulate == 0 else np.arange(got.size, dtype=np.int64).reshape(got.shape)
            ctx.h2d(dst, before)
            _, seen = launches(ctx, lambda: ctx.pool_groups_device(n, bins, src, labels, n_groups, dst, accumulate=accumulate))
            assert seen == {'pool_groups': 1}, seen
            ctx.d2h(got, dst)
            want = sums if accumulate == 0 else before.view(np.uint64) + sums
            assert np.array_equal(got.view(np.uint64), want), (accumulate, np.argwhere(got.view(np.uint64) != want)[:4])
        assert np.array_equal(fetch(ctx, src, tables.shape), tables), 'the tables were written'


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
