"""The balance, the shrink and the pool of whole SETS of tables on the GPU at the C-ABI (kpal_balance_set_device,
kpal_shrink_set_device, kpal_pool_set_device; kpal/klib.py:285-298, 329-352, 269-283) against the oracle per table.  Counts
are integers: every comparison is exact.  A table's result does not depend on the set it is in, the launches do not grow with
the set, and a bad argument launches nothing.  The shrink of ONE table on the device (kpal_shrink_device) is here too, where
its input lies at an odd multiple of 8 bytes: it shares the launch of the set entry (shrink_launch).

Measured on an MI355X: the whole file (76 tests) in 5.1 s, 3.4 s of it the tables of one balance test; the slowest shrink
case is (8, 7) at 70 tables, 0.14 s.
Run on the GPU box: pytest -m gpu."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

KINDS = ('poisson', 'zeros', 'constant', 'one', 'heavy', 'negative', 'wide', 'wrapping')   # those of tests/test_gpu_stat_sets.py
SET_KERNELS = ('balance_set', 'balance_tiled_set', 'shrink_set', 'pool_set', 'pool_set_final')


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


@pytest.fixture(scope='module')
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def make_table(rs, bins, kind):
    if kind == 'poisson':
        return rs.poisson(rs.choice([0.02, 0.7, 3.0, 800.0]), bins).astype(np.int64)
    if kind == 'zeros':
        return np.zeros(bins, dtype=np.int64)
    if kind == 'constant':
        return np.full(bins, 7, dtype=np.int64)
    if kind == 'one':
        v = np.zeros(bins, dtype=np.int64)
        v[rs.randint(0, bins)] = 5
        return v
    if kind == 'heavy':
        v = rs.poisson(1.5, bins).astype(np.int64)
        v[rs.randint(0, bins, max(1, bins // 300))] = 10 ** 12
        return v
    if kind == 'negative':
        return rs.randint(-10 ** 6, 10 ** 6, size=bins).astype(np.int64)
    if kind == 'wide':
        return rs.randint(-(1 << 62), 1 << 62, size=bins).astype(np.int64)
    assert kind == 'wrapping'
    return rs.randint(1 << 60, 1 << 62, size=bins).astype(np.int64)


def make_set(seed, bins, n, shift=0):
    rs = np.random.RandomState(seed)
    return np.stack([make_table(rs, bins, KINDS[(i + shift) % len(KINDS)]) for i in range(n)])


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


# ---- balance ---------------------------------------------------------------------------------------------------------------
def single_balance(ctx, table, k):
    """One table alone through the set entry: what a table gives in any set must equal this, bit for bit."""
    with device_buffers(ctx, table.nbytes, table.nbytes) as (src, dst):
        ctx.h2d(src, table)
        ctx.balance_set_device(k, 1, src, dst)
        return fetch(ctx, dst, table.shape)


def check_balance(ctx, k, n, seed):
    bins = 4 ** k
    tables = make_set(seed, bins, n, shift=k + n)
    want = np.stack([oracle.balance(t, k) for t in tables])
    name = 'balance_set' if k <= 5 else 'balance_tiled_set'
    with device_buffers(ctx, tables.nbytes, tables.nbytes) as (src, dst):
        ctx.h2d(src, tables)
        ctx.h2d(dst, np.full(tables.shape, -1, dtype=np.int64))
        _, seen = launches(ctx, lambda: ctx.balance_set_device(k, n, src, dst))
        assert seen == {name: 1}, (k, n, seen)
        out_of_place = fetch(ctx, dst, tables.shape)
        assert np.array_equal(fetch(ctx, src, tables.shape), tables), (k, n, 'the input was written')
        _, seen = launches(ctx, lambda: ctx.balance_set_device(k, n, src, src))
        assert seen == {name: 1}, (k, n, seen)
        in_place = fetch(ctx, src, tables.shape)
    assert np.array_equal(out_of_place, want), (k, n, np.argwhere(out_of_place != want)[:4])
    assert np.array_equal(in_place, want), (k, n, np.argwhere(in_place != want)[:4])
    # the same table alone: the same bits
    for i in sorted({0, n // 2, n - 1}):
        assert np.array_equal(single_balance(ctx, tables[i], k), out_of_place[i]), (k, n, i)


@pytest.mark.parametrize('n', (1, 3, 70))
@pytest.mark.parametrize('k', (1, 2, 3, 4, 5, 6, 7, 8))
def test_balance_sets_vs_oracle(ctx, k, n):
    """k <= 5: the flat kernel (even k has palindromes, odd k none); k = 6: one self tile per table; k = 7: two pairs of
    different tiles; k = 8: self pairs and others.  Out of place and in place, one launch each."""
    check_balance(ctx, k, n, 1000 * k + n)


def test_balance_k9_three_tables(ctx):
    check_balance(ctx, 9, 3, 9003)


def test_balance_workgroups_take_several_items_across_tables(ctx, num_cu):
    """More items than twice the CUs: a persistent workgroup takes more than one, its next item lies in another table
    (k = 6: 700 items of one table each; k = 8: 10 pairs a table, 70 tables)."""
    assert 700 > 2 * num_cu, num_cu
    check_balance(ctx, 6, 700, 6700)
    check_balance(ctx, 8, 70, 8070)


# ---- shrink ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 3, 70))
@pytest.mark.parametrize('k,factor', ((2, 1), (6, 3), (6, 4), (8, 7), (5, 2), (8, 1), (8, 2), (8, 3), (8, 4)))
def test_shrink_sets_vs_oracle(ctx, k, factor, n):
    """(6, 3): 64 inputs an output, the last case of the shuffle kernel; (6, 4): the wave-per-output kernel.  70 tables of
    k = 8 are 2.29 M input pairs, more than the 8 x CUs x 256 threads of the shuffle kernel's grid: it goes around its rounds
    more than once, the last time with part of the grid, for 4, 16 and 64 inputs an output; (8, 4) is the first factor past it."""
    tables = make_set(100 * k + 10 * factor + n, 4 ** k, n, shift=factor + n)
    want = np.stack([oracle.shrink(t, k, factor) for t in tables])
    with device_buffers(ctx, tables.nbytes, want.nbytes) as (src, dst):
        ctx.h2d(src, tables)
        ctx.h2d(dst, np.full(want.shape, -1, dtype=np.int64))
        _, seen = launches(ctx, lambda: ctx.shrink_set_device(k, factor, n, src, dst))
        got = fetch(ctx, dst, want.shape)
        assert np.array_equal(fetch(ctx, src, tables.shape), tables)
    assert seen == {'shrink_set': 1}, seen
    assert np.array_equal(got, want), (k, factor, n, np.argwhere(got != want)[:4])


def test_shrink_of_large_tables_is_a_launch_per_table(ctx):
    """From k = 12 on the plan gives every table a launch of its own (transform_plan.hpp: the one launch was measured to lose)."""
    k, factor, n = 12, 2, 2
    tables = ((np.arange(n * 4 ** k, dtype=np.int64) * 2654435761) % 1009 - 4).reshape(n, 4 ** k)
    want = np.stack([oracle.shrink(t, k, factor) for t in tables])
    with device_buffers(ctx, tables.nbytes, want.nbytes) as (src, dst):
        ctx.h2d(src, tables)
        _, seen = launches(ctx, lambda: ctx.shrink_set_device(k, factor, n, src, dst))
        got = fetch(ctx, dst, want.shape)
    assert seen == {'shrink_set': 2}, seen
    assert np.array_equal(got, want)


def test_shrink_of_tables_at_an_odd_multiple_of_eight_bytes(ctx):
    tables = make_set(77, 4 ** 4, 5, shift=2)
    want = np.stack([oracle.shrink(t, 4, 1) for t in tables])
    with device_buffers(ctx, tables.nbytes + 16, want.nbytes) as (src, dst):
        ctx.h2d(src + 8, tables)
        ctx.shrink_set_device(4, 1, 5, src + 8, dst)
        assert np.array_equal(fetch(ctx, dst, want.shape), want)


def test_shrink_of_a_set_at_an_odd_multiple_of_eight_bytes_by_64(ctx):
    """(6, 3): the largest factor of the shuffle kernel, which reads 16 bytes at a time -- not from here."""
    k, factor, n = 6, 3, 5
    tables = make_set(63, 4 ** k, n, shift=1)
    want = np.stack([oracle.shrink(t, k, factor) for t in tables])
    with device_buffers(ctx, tables.nbytes + 16, want.nbytes) as (src, dst):
        ctx.h2d(src + 8, tables)
        ctx.h2d(dst, np.full(want.shape, -1, dtype=np.int64))
        _, seen = launches(ctx, lambda: ctx.shrink_set_device(k, factor, n, src + 8, dst))
        assert seen == {'shrink_set': 1}, seen
        assert np.array_equal(fetch(ctx, dst, want.shape), want)
        assert np.array_equal(fetch(ctx, src + 8, tables.shape), tables)


@pytest.mark.parametrize('k,factor', ((4, 1), (4, 3), (6, 2), (6, 3), (8, 1)))
def test_shrink_of_one_table_at_an_odd_multiple_of_eight_bytes(ctx, k, factor):
    """kpal_shrink_device asks for 8-byte alignment only: up to 64 inputs an output it takes the kernel that reads 16 bytes at
    a time where the input allows it, and the 8-byte one here."""
    table = make_set(100 * k + factor, 4 ** k, 3, shift=5)[2]       # values of 2^60 to 2^62: the sums wrap
    want = oracle.shrink(table, k, factor)
    with device_buffers(ctx, table.nbytes + 16, want.nbytes) as (src, dst):
        assert src % 16 == 0
        ctx.h2d(src + 8, table)
        ctx.h2d(dst, np.full(want.shape, -1, dtype=np.int64))
        _, seen = launches(ctx, lambda: ctx.shrink_device(k, factor, src + 8, dst))
        assert seen == {'shrink': 1}, seen
        assert np.array_equal(fetch(ctx, dst, want.shape), want)
        assert np.array_equal(fetch(ctx, src + 8, table.shape), table), 'the input was written'
        # and from a 16-byte aligned address: the same sums
        ctx.h2d(src, table)
        ctx.h2d(dst, np.full(want.shape, -1, dtype=np.int64))
        _, seen = launches(ctx, lambda: ctx.shrink_device(k, factor, src, dst))
        assert seen == {'shrink': 1} and np.array_equal(fetch(ctx, dst, want.shape), want)


# ---- pool ------------------------------------------------------------------------------------------------------------------
def pool_slices(n_tables, bins, num_cu):
    """The rule of transform_plan.hpp (pool_slices), restated."""
    if n_tables <= 1 or bins >= 1 << 20:
        return 1
    groups = -(-((bins + 1) // 2) // 256)
    return max(1, min(-(-8 * num_cu // groups), -(-n_tables // 16), n_tables))


def check_pool(ctx, bins, n, seed, num_cu, offset=0):
    tables = make_set(seed, bins, n, shift=seed % 8)
    if n > 1:
        tables[1] = make_table(np.random.RandomState(seed + 1), bins, 'wrapping')      # sums past 2^63 wrap
    before = make_table(np.random.RandomState(seed + 2), bins, 'negative')
    with np.errstate(over='ignore'):
        total = tables.sum(axis=0, dtype=np.int64)
        want = {0: total, 1: total + before}
    slices = pool_slices(n, bins, num_cu)
    with device_buffers(ctx, tables.nbytes + 16, 8 * bins + 16) as (src, dst):
        src, dst = src + offset, dst + offset
        ctx.h2d(src, tables)
        for accumulate in (0, 1):
            ctx.h2d(dst, before)
            _, seen = launches(ctx, lambda: ctx.pool_set_device(n, bins, src, dst, accumulate=accumulate))
            got = fetch(ctx, dst, (bins,))
            assert seen == ({'pool_set': 1} if slices == 1 else {'pool_set': 1, 'pool_set_final': 1}), (bins, n, seen)
            assert np.array_equal(got, want[accumulate]), (bins, n, accumulate, np.argwhere(got != want[accumulate])[:4])
        assert np.array_equal(fetch(ctx, src, tables.shape), tables)
    return slices


@pytest.mark.parametrize('n', (1, 2, 257))
@pytest.mark.parametrize('bins', (4, 64, 4096, 65536))
def test_pool_sets(ctx, num_cu, bins, n):
    slices = check_pool(ctx, bins, n, bins + n, num_cu)
    assert slices == (1 if n < 17 else 17 if bins <= 4096 else min(17, -(-8 * num_cu // 128)))


def test_pool_of_many_small_tables_in_several_slices(ctx, num_cu):
    assert check_pool(ctx, 64, 3000, 3064, num_cu) == 188


def test_pool_of_odd_rows_and_odd_addresses(ctx, num_cu):
    """An odd number of bins and ranges at odd multiples of 8 bytes: the 8-byte form of the kernel, a last single column."""
    assert check_pool(ctx, 1001, 40, 1041, num_cu) == 3
    check_pool(ctx, 64, 40, 2041, num_cu, offset=8)


# ---- arguments -------------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(ctx):
    k, n = 4, 3
    bins = 4 ** k
    tables = make_set(5, bins, n)
    with device_buffers(ctx, 2 * tables.nbytes, tables.nbytes) as (src, dst):
        ctx.h2d(src, tables)
        huge = 1 << 62
        bad = [
            (lambda: ctx.balance_set_device(k, n, 0, dst), 'NULL pointer'),
            (lambda: ctx.balance_set_device(k, n, src, 0), 'NULL pointer'),
            (lambda: ctx.balance_set_device(k, 0, src, dst), 'empty set'),
            (lambda: ctx.balance_set_device(0, n, src, dst), 'k=0 out of range'),
            (lambda: ctx.balance_set_device(17, n, src, dst), 'k=17 out of range'),
            (lambda: ctx.balance_set_device(k, n, src + 4, dst), 'not 8-byte aligned'),
            (lambda: ctx.balance_set_device(k, n, src, dst + 4), 'not 8-byte aligned'),
            (lambda: ctx.balance_set_device(k, huge, src, dst), 'too many bytes'),
            (lambda: ctx.balance_set_device(k, n, src, src + 8), 'overlaps'),               # partial, above
            (lambda: ctx.balance_set_device(k, n, src + 8 * bins, src), 'overlaps'),        # partial, below
            (lambda: ctx.shrink_set_device(k, 1, n, 0, dst), 'NULL pointer'),
            (lambda: ctx.shrink_set_device(k, 1, 0, src, dst), 'empty set'),
            (lambda: ctx.shrink_set_device(17, 1, n, src, dst), 'k=17 out of range'),
            (lambda: ctx.shrink_set_device(k, 0, n, src, dst), 'Reduction factor should be smaller than k-mer size.'),
            (lambda: ctx.shrink_set_device(k, k, n, src, dst), 'Reduction factor should be smaller than k-mer size.'),
            (lambda: ctx.shrink_set_device(k, 1, n, src + 4, dst), 'not 8-byte aligned'),
            (lambda: ctx.shrink_set_device(k, 1, huge, src, dst), 'too many bytes'),
            (lambda: ctx.shrink_set_device(k, 1, n, src, src), 'overlaps'),
            (lambda: ctx.shrink_set_device(k, 1, n, src, src + 8 * (n * bins - 1)), 'overlaps'),
            (lambda: ctx.pool_set_device(n, bins, 0, dst), 'NULL pointer'),
            (lambda: ctx.pool_set_device(n, bins, src, 0), 'NULL pointer'),
            (lambda: ctx.pool_set_device(0, bins, src, dst), 'empty set'),
            (lambda: ctx.pool_set_device(n, 0, src, dst), 'empty vector'),
            (lambda: ctx.pool_set_device(n, bins, src, dst + 4), 'not 8-byte aligned'),
            (lambda: ctx.pool_set_device(huge, bins, src, dst), 'too many bytes'),
            (lambda: ctx.pool_set_device(n, bins, src, src), 'overlaps'),
            (lambda: ctx.pool_set_device(n, bins, src, src + 8 * (n * bins - 1)), 'overlaps'),
        ]
        ctx.h2d(dst, np.full(tables.shape, -1, dtype=np.int64))
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
        assert np.array_equal(fetch(ctx, dst, tables.shape), np.full(tables.shape, -1, dtype=np.int64))
        assert np.array_equal(fetch(ctx, src, tables.shape), tables)
        # a good call afterwards still answers; the output may begin where the input ends
        ctx.balance_set_device(k, n, src, src + tables.nbytes)
        got = fetch(ctx, src + tables.nbytes, tables.shape)
    assert np.array_equal(got, np.stack([oracle.balance(t, k) for t in tables]))
