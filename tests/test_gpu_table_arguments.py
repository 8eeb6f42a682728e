"""What the entries that take count tables and make summaries, spectra or new tables answer to bad arguments: kpal_balance[_device],
kpal_split, kpal_stats[_device], kpal_merge[_device], kpal_shrink[_device] (kpal_amd/csrc/kpal_vec.hip), kpal_stats_set[_device],
kpal_strand_balance, kpal_strand_balance_set[_device] (kpal_sets.hip), kpal_distribution_set[_device], kpal_distribution_fetch
(kpal_spectrum.hip), kpal_balance_set_device, kpal_shrink_set_device, kpal_pool_set_device (kpal_transform.hip) and
kpal_pool_groups_device (kpal_pool_groups.hip), called through ctypes where the Python face would stop the call first.

Every case is refused on the host: the return code is KPAL_E_INVALID, kpal_last_error() is the literal below (the text in the
source), the context's profiler records no launch and the poisoned outputs stay as they are.  Where two faults coincide the ORDER
of an entry's checks decides the message; the double faults pin it -- the context before everything, k before the factor, both
before the pointers, the pointers before the sizes (empty set, then empty vector, then the groups), the pairwise of the strand
balance between the empty set and the alignment, the alignment before the bytes, the bytes before the overlap, the overlap of the
pool by label before its labels.  What two sibling entries answer differently is recorded as it is: the balance pair names its
pointer, the merge pair takes n == 0 (after its pointers and its merger), a refused distribution call drops the pending pairs.
The last test calls every entry once with good arguments: 3 tables of k = 4 (256 bins each) in one device buffer of 16 KiB."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, T, BINS = 4, 3, 256
SET = T * BINS * 8      # bytes of the three tables
E_INVALID = -1
POISON = -12345.5
INDEX_POISON = -777
HUGE = 1 << 62          # tables whose bytes no size_t holds

CTX_NULL = 'ctx is NULL'
K_RANGE = {0: 'k=0 out of range', 17: 'k=17 out of range', -1: 'k=-1 out of range'}
FACTOR = 'Reduction factor should be smaller than k-mer size.'
NULL_POINTER = 'NULL pointer'
DEV_INOUT = 'dev_inout is NULL'
HOST_INOUT = 'host_inout is NULL'
EMPTY_SET = 'empty set'
EMPTY_VECTOR = 'empty vector'
NO_GROUPS = 'no groups'
ALIGNED = 'tables are not 8-byte aligned'
PAIRWISE = 'pairwise must be prod or sum'
BAD_MERGER = {-1: 'unknown merger -1', 4: 'unknown merger 4'}
MANY_BINS = '4611686018427387904 tables of 256 bins: too many bytes'
MANY_AT_K = '4611686018427387904 tables at k=4: too many bytes'
MANY_TABLES_GROUPS = '4611686018427387904 tables of 256 bins in 2 groups: too many bytes'
MANY_GROUPS = '3 tables of 256 bins in 4611686018427387904 groups: too many bytes'
MANY_INDEX = '2147483648 tables of 1 bins in 2 groups: too many bytes'
BALANCE_OVERLAP = 'balance of a set: the output overlaps the input without being the input'
SHRINK_OVERLAP = 'shrink of a set: the output overlaps the input'
POOL_OVERLAP = 'pool of a set: the output overlaps the tables'
GROUPS_OVERLAP = 'pool of groups: the output overlaps the tables'
BAD_LABEL = 'table 1 has label 2: there are 2 groups'
NOT_PENDING = 'no distribution pending'


@pytest.fixture(scope='module')
def env():
    from kpal_amd import _native

    class Env(object):
        pass
    e = Env()
    e.native = _native
    e.ctx = _native.context()
    e.L, e.h = e.ctx._L, e.ctx._h
    rng = np.random.RandomState(11)
    e.tables = np.ascontiguousarray((rng.randint(0, 9, (T, BINS)) * rng.randint(0, 2, (T, BINS))).astype(np.int64))
    e.dev = e.ctx.alloc(2 * 8192)          # the tables at its start, the outputs from its middle on
    e.out = e.dev + 8192
    e.ctx.h2d(e.dev, e.tables)
    e.ctx.h2d(e.out, np.full(T * BINS, -7, dtype=np.int64))
    e.ctx.sync()
    yield e
    e.ctx.free(e.dev)


class Refusals(object):
    """Runs calls that must be refused; `done` asserts that every one was, with its text and without a launch."""

    def __init__(self, env):
        self.env, self.wrong = env, []

    def __call__(self, what, call, text, rc_wanted=E_INVALID):
        ctx = self.env.ctx
        ctx.prof_enable(True)
        try:
            ctx.prof_reset()
            rc = call()
            names = {name: cnt for name, (_, cnt) in ctx.prof_get().items() if cnt}
        finally:
            ctx.prof_enable(False)
        got = self.env.L.kpal_last_error().decode() if rc != 0 else None
        if rc != rc_wanted or got != text or names:
            self.wrong.append((what, rc, got, text, names))

    def accepted(self, what, call):
        """A call that is taken and launches nothing."""
        self(what, call, None, 0)

    def done(self):
        assert not self.wrong, '\n'.join('%r: rc %d, "%s" where "%s" was expected, launches %r' % w for w in self.wrong)


def f64p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def addr(a):
    return None if a is None else a.ctypes.data


def untouched(env):
    after = np.empty(T * BINS, dtype=np.int64)
    env.ctx.d2h(after, env.out)
    return (after == -7).all()


def test_balance_pair(env):
    host = env.tables[0].copy()
    refuse = Refusals(env)
    for name, good, null_text in (('kpal_balance_device', env.out, DEV_INOUT), ('kpal_balance', host.ctypes.data, HOST_INOUT)):
        fn = getattr(env.L, name)

        def call(h=env.h, k=K, p=good, fn=fn):
            return lambda: fn(h, k, p)

        refuse((name, 'ctx'), call(h=None), CTX_NULL)
        refuse((name, 'ctx', 'k'), call(h=None, k=0), CTX_NULL)
        refuse((name, 'ctx', 'pointer'), call(h=None, p=None), CTX_NULL)
        for k, text in K_RANGE.items():
            refuse((name, k), call(k=k), text)
            refuse((name, k, 'pointer'), call(k=k, p=None), text)           # k before the pointer
        refuse((name, 'pointer'), call(p=None), null_text)
    refuse.done()
    assert np.array_equal(host, env.tables[0]) and untouched(env)


def test_split(env):
    counts = env.tables[0]
    forward, reverse = np.full(BINS, INDEX_POISON, dtype=np.int64), np.full(BINS, INDEX_POISON, dtype=np.int64)
    n_out = ctypes.c_uint64(99)
    refuse = Refusals(env)

    def call(h=env.h, k=K, c=counts, f=forward, r=reverse):
        return lambda: env.L.kpal_split(h, k, addr(c), addr(f), addr(r), ctypes.byref(n_out))

    refuse(('ctx',), call(h=None), CTX_NULL)
    refuse(('ctx', 'k'), call(h=None, k=17), CTX_NULL)
    for k, text in K_RANGE.items():
        refuse((k,), call(k=k), text)
        refuse((k, 'counts'), call(k=k, c=None), text)
    for null in ('c', 'f', 'r'):
        refuse((null,), call(**{null: None}), NULL_POINTER)
    refuse.done()
    assert (forward == INDEX_POISON).all() and (reverse == INDEX_POISON).all() and n_out.value == 99


def test_stats_pair(env):
    stats = env.native.ProfileStats(1, 2, 3, 4, 5.0, 6.0, 7.0)
    refuse = Refusals(env)
    for name, good in (('kpal_stats_device', env.dev), ('kpal_stats', env.tables.ctypes.data)):
        fn = getattr(env.L, name)

        def call(h=env.h, n=BINS, c=good, out=ctypes.byref(stats), fn=fn):
            return lambda: fn(h, n, c, out)

        refuse((name, 'ctx'), call(h=None), CTX_NULL)
        refuse((name, 'ctx', 'counts'), call(h=None, c=None), CTX_NULL)
        refuse((name, 'counts'), call(c=None), NULL_POINTER)
        refuse((name, 'out'), call(out=None), NULL_POINTER)
        refuse((name, 'n'), call(n=0), EMPTY_VECTOR)
        refuse((name, 'counts', 'n'), call(c=None, n=0), NULL_POINTER)      # the pointers before n
        refuse((name, 'out', 'n'), call(out=None, n=0), NULL_POINTER)
    refuse.done()
    assert (stats.total, stats.non_zero, stats.min, stats.max, stats.mean, stats.median, stats.std) == (1, 2, 3, 4, 5.0, 6.0, 7.0)


def test_merge_pair(env):
    host_out = np.full(BINS, INDEX_POISON, dtype=np.int64)
    refuse = Refusals(env)
    for name, left, right, out in (('kpal_merge_device', env.dev, env.dev + BINS * 8, env.out),
                                   ('kpal_merge', env.tables[0].ctypes.data, env.tables[1].ctypes.data, host_out.ctypes.data)):
        fn = getattr(env.L, name)

        def call(h=env.h, n=BINS, l=left, r=right, merger=0, o=out, fn=fn):
            return lambda: fn(h, n, l, r, merger, o)

        refuse((name, 'ctx'), call(h=None), CTX_NULL)
        refuse((name, 'ctx', 'merger'), call(h=None, merger=4), CTX_NULL)
        for null in ('l', 'r', 'o'):
            refuse((name, null), call(**{null: None}), NULL_POINTER)
            refuse((name, null, 'merger'), call(merger=4, **{null: None}), NULL_POINTER)   # the pointers before the merger
            refuse((name, null, 'n'), call(n=0, **{null: None}), NULL_POINTER)             # ... and before n == 0
        for merger, text in BAD_MERGER.items():
            refuse((name, merger), call(merger=merger), text)
            refuse((name, merger, 'n'), call(merger=merger, n=0), text)                    # the merger before n == 0
        for merger in range(4):
            refuse.accepted((name, 'n', merger), call(n=0, merger=merger))                 # nothing to merge is no error
    refuse.done()
    assert (host_out == INDEX_POISON).all() and untouched(env)


def test_shrink_pair(env):
    host_out = np.full(BINS, INDEX_POISON, dtype=np.int64)
    refuse = Refusals(env)
    for name, counts, out in (('kpal_shrink_device', env.dev, env.out), ('kpal_shrink', env.tables.ctypes.data, host_out.ctypes.data)):
        fn = getattr(env.L, name)

        def call(h=env.h, k=K, factor=1, c=counts, o=out, fn=fn):
            return lambda: fn(h, k, factor, c, o)

        refuse((name, 'ctx'), call(h=None), CTX_NULL)
        refuse((name, 'ctx', 'k'), call(h=None, k=0), CTX_NULL)
        for k, text in K_RANGE.items():
            refuse((name, k), call(k=k), text)
            refuse((name, k, 'factor'), call(k=k, factor=0), text)          # k before the factor
            refuse((name, k, 'counts'), call(k=k, c=None), text)
        for factor in (0, -1, K, K + 1):
            refuse((name, 'factor', factor), call(factor=factor), FACTOR)
            refuse((name, 'factor', factor, 'counts'), call(factor=factor, c=None), FACTOR)   # the factor before the pointers
            refuse((name, 'factor', factor, 'out'), call(factor=factor, o=None), FACTOR)
        refuse((name, 'counts'), call(c=None), NULL_POINTER)
        refuse((name, 'out'), call(o=None), NULL_POINTER)
    refuse.done()
    assert (host_out == INDEX_POISON).all() and untouched(env)


def set_ladder(refuse, name, call):
    """The checks kpal_stats_set[_device] and kpal_distribution_set[_device] share: the pointers, the empty set, the empty vector,
    the alignment, the bytes.  call(n=, bins=, t=, out=, off=, h=): t None is a NULL table pointer, off a byte offset to it."""
    refuse((name, 'ctx'), call(h=None), CTX_NULL)
    refuse((name, 'ctx', 'tables'), call(h=None, t=None), CTX_NULL)
    refuse((name, 'ctx', 'n'), call(h=None, n=0), CTX_NULL)
    refuse((name, 'tables'), call(t=None), NULL_POINTER)
    refuse((name, 'out'), call(out=None), NULL_POINTER)
    refuse((name, 'tables', 'n'), call(t=None, n=0), NULL_POINTER)          # the pointers before the sizes
    refuse((name, 'out', 'bins'), call(out=None, bins=0), NULL_POINTER)
    refuse((name, 'out', 'aligned'), call(out=None, off=4), NULL_POINTER)
    refuse((name, 'n'), call(n=0), EMPTY_SET)
    refuse((name, 'n', 'bins'), call(n=0, bins=0), EMPTY_SET)               # the set before the vector
    refuse((name, 'n', 'aligned'), call(n=0, off=4), EMPTY_SET)
    refuse((name, 'bins'), call(bins=0), EMPTY_VECTOR)
    refuse((name, 'bins', 'aligned'), call(bins=0, off=4), EMPTY_VECTOR)    # the vector before the alignment
    refuse((name, 'bins', 'bytes'), call(bins=0, n=HUGE), EMPTY_VECTOR)
    for off in (1, 4, 7):
        refuse((name, 'aligned', off), call(off=off), ALIGNED)
    refuse((name, 'aligned', 'bytes'), call(off=4, n=HUGE), ALIGNED)        # the alignment before the bytes
    refuse((name, 'bytes'), call(n=HUGE), MANY_BINS)
    refuse((name, 'bytes', 'few'), call(n=1 << 61, bins=2), '2305843009213693952 tables of 2 bins: too many bytes')


def test_stats_set_pair(env):
    stats = (env.native.ProfileStats * T)()
    for s in stats:
        s.total = INDEX_POISON
    refuse = Refusals(env)
    for name, good in (('kpal_stats_set_device', env.dev), ('kpal_stats_set', env.tables.ctypes.data)):
        fn = getattr(env.L, name)

        def call(h=env.h, n=T, bins=BINS, t=good, out=stats, off=0, fn=fn):
            return lambda: fn(h, n, bins, None if t is None else t + off, out)

        set_ladder(refuse, name, call)
    refuse.done()
    assert all(s.total == INDEX_POISON for s in stats)


def test_distribution_set_pair_and_fetch(env):
    offsets = np.full(T + 1, 99, dtype=np.uint64)
    values, numbers = np.full(BINS, INDEX_POISON, dtype=np.int64), np.full(BINS, 99, dtype=np.uint64)
    refuse = Refusals(env)

    def fetch(h=env.h, first=0, n=1, v=values, m=numbers):
        return lambda: env.L.kpal_distribution_fetch(h, first, n, addr(v), addr(m))

    def begin():
        assert env.L.kpal_distribution_set_device(env.h, 1, BINS, env.dev, offsets.ctypes.data) == 0
        have = int(offsets[1])
        offsets[:] = 99
        return have

    for name, good in (('kpal_distribution_set_device', env.dev), ('kpal_distribution_set', env.tables.ctypes.data)):
        fn = getattr(env.L, name)

        def call(h=env.h, n=T, bins=BINS, t=good, out=offsets, off=0, fn=fn):
            return lambda: fn(h, n, bins, None if t is None else t + off, addr(out))

        set_ladder(refuse, name, call)
        # a refused call has dropped the pairs of the call before it -- but for the one without a context
        begin()
        refuse((name, 'ctx', 'pending'), call(h=None), CTX_NULL)
        refuse.accepted((name, 'fetch after ctx'), fetch(n=0))
        refuse((name, 'tables', 'pending'), call(t=None), NULL_POINTER)
        refuse((name, 'fetch after refusal'), fetch(), NOT_PENDING)
        refuse((name, 'fetch nothing after refusal'), fetch(n=0), NOT_PENDING)
    have = begin()
    assert 1 <= have <= 9
    refuse(('fetch', 'ctx'), fetch(h=None), CTX_NULL)
    refuse(('fetch', 'ctx', 'values'), fetch(h=None, v=None), CTX_NULL)
    refuse(('fetch', 'first'), fetch(first=have + 1, n=0), 'pairs %d .. +0 of %d' % (have + 1, have))
    refuse(('fetch', 'n'), fetch(first=1, n=have), 'pairs 1 .. +%d of %d' % (have, have))
    refuse(('fetch', 'wrap'), fetch(first=2, n=(1 << 64) - 1), 'pairs 2 .. +18446744073709551615 of %d' % have)
    refuse(('fetch', 'n', 'values'), fetch(first=1, n=have, v=None), 'pairs 1 .. +%d of %d' % (have, have))   # the range before the pointers
    refuse(('fetch', 'values'), fetch(v=None), NULL_POINTER)
    refuse(('fetch', 'numbers'), fetch(m=None), NULL_POINTER)
    refuse.accepted(('fetch', 'nothing'), fetch(first=have, n=0, v=None, m=None))       # no pair asked for: no pointer looked at
    refuse.done()
    assert (offsets == 99).all() and (values == INDEX_POISON).all() and (numbers == 99).all()


def test_strand_balance_entries(env):
    out = np.full(T, POISON)
    refuse = Refusals(env)
    entries = [('kpal_strand_balance_set_device', env.dev, True), ('kpal_strand_balance_set', env.tables.ctypes.data, True),
               ('kpal_strand_balance', env.tables.ctypes.data, False)]
    for name, good, is_set in entries:
        fn = getattr(env.L, name)

        def call(h=env.h, k=K, n=T, t=good, pairwise=0, res=out, off=0, fn=fn, is_set=is_set):
            t = None if t is None else t + off
            return (lambda: fn(h, k, n, t, pairwise, f64p(res))) if is_set else (lambda: fn(h, k, t, pairwise, f64p(res)))

        refuse((name, 'ctx'), call(h=None), CTX_NULL)
        refuse((name, 'ctx', 'k'), call(h=None, k=0), CTX_NULL)
        for k, text in K_RANGE.items():
            refuse((name, k), call(k=k), text)
            refuse((name, k, 'tables'), call(k=k, t=None), text)            # k before the pointers
            refuse((name, k, 'pairwise'), call(k=k, pairwise=2), text)
        refuse((name, 'tables'), call(t=None), NULL_POINTER)
        refuse((name, 'out'), call(res=None), NULL_POINTER)
        refuse((name, 'tables', 'pairwise'), call(t=None, pairwise=2), NULL_POINTER)
        refuse((name, 'out', 'aligned'), call(res=None, off=4), NULL_POINTER)
        for pairwise in (-1, 2, 3):
            refuse((name, 'pairwise', pairwise), call(pairwise=pairwise), PAIRWISE)
            refuse((name, 'pairwise', pairwise, 'aligned'), call(pairwise=pairwise, off=4), PAIRWISE)   # the pairwise before the alignment
        for off in (1, 4):
            refuse((name, 'aligned', off), call(off=off), ALIGNED)
        if is_set:
            refuse((name, 'tables', 'n'), call(t=None, n=0), NULL_POINTER)  # the pointers before the empty set
            refuse((name, 'n'), call(n=0), EMPTY_SET)
            refuse((name, 'n', 'pairwise'), call(n=0, pairwise=2), EMPTY_SET)   # the empty set before the pairwise
            refuse((name, 'n', 'aligned'), call(n=0, off=4), EMPTY_SET)
            refuse((name, 'pairwise', 'bytes'), call(pairwise=2, n=HUGE), PAIRWISE)
            refuse((name, 'aligned', 'bytes'), call(off=4, n=HUGE), ALIGNED)    # the alignment before the bytes
            refuse((name, 'bytes'), call(n=HUGE), MANY_AT_K)
            refuse((name, 'bytes', 'k 16'), call(k=16, n=1 << 29), '536870912 tables at k=16: too many bytes')
    refuse.done()
    assert (out == POISON).all()


def test_balance_and_shrink_set_device(env):
    refuse = Refusals(env)

    def balance(h=env.h, k=K, n=T, i=env.dev, o=env.out):
        return lambda: env.L.kpal_balance_set_device(h, k, n, i, o)

    def shrink(h=env.h, k=K, factor=1, n=T, i=env.dev, o=env.out):
        return lambda: env.L.kpal_shrink_set_device(h, k, factor, n, i, o)

    for name, call in (('balance', balance), ('shrink', shrink)):
        refuse((name, 'ctx'), call(h=None), CTX_NULL)
        refuse((name, 'ctx', 'k'), call(h=None, k=17), CTX_NULL)
        for k, text in K_RANGE.items():
            refuse((name, k), call(k=k), text)
            refuse((name, k, 'in'), call(k=k, i=None), text)                # k before the pointers
            refuse((name, k, 'n'), call(k=k, n=0), text)
        refuse((name, 'in'), call(i=None), NULL_POINTER)
        refuse((name, 'out'), call(o=None), NULL_POINTER)
        refuse((name, 'in', 'n'), call(i=None, n=0), NULL_POINTER)          # the pointers before the empty set
        refuse((name, 'out', 'aligned'), call(o=None, i=env.dev + 4), NULL_POINTER)
        refuse((name, 'n'), call(n=0), EMPTY_SET)
        refuse((name, 'n', 'aligned'), call(n=0, i=env.dev + 4), EMPTY_SET)     # the empty set before the alignment
        refuse((name, 'in + 4'), call(i=env.dev + 4), ALIGNED)
        refuse((name, 'out + 4'), call(o=env.out + 4), ALIGNED)
        refuse((name, 'out + 4', 'bytes'), call(o=env.out + 4, n=HUGE), ALIGNED)    # the alignment before the bytes
        refuse((name, 'bytes'), call(n=HUGE), MANY_AT_K)
        refuse((name, 'bytes', 'overlap'), call(n=HUGE, o=env.dev + 8), MANY_AT_K)  # the bytes before the overlap
    refuse(('balance', 'overlap above'), balance(o=env.dev + 8), BALANCE_OVERLAP)
    refuse(('balance', 'overlap below'), balance(i=env.dev + 8 * BINS, o=env.dev), BALANCE_OVERLAP)
    refuse(('balance', 'overlap last'), balance(o=env.dev + SET - 8), BALANCE_OVERLAP)
    for k, text in K_RANGE.items():
        refuse(('shrink', k, 'factor'), shrink(k=k, factor=0), text)        # k before the factor
    for factor in (0, -1, K, K + 1):
        refuse(('shrink', 'factor', factor), shrink(factor=factor), FACTOR)
        refuse(('shrink', 'factor', factor, 'in'), shrink(factor=factor, i=None), FACTOR)      # the factor before the pointers ...
        refuse(('shrink', 'factor', factor, 'n'), shrink(factor=factor, n=0), FACTOR)          # ... the empty set ...
        refuse(('shrink', 'factor', factor, 'aligned'), shrink(factor=factor, i=env.dev + 4), FACTOR)
        refuse(('shrink', 'factor', factor, 'bytes'), shrink(factor=factor, n=HUGE), FACTOR)   # ... and the bytes
    refuse(('shrink', 'in place'), shrink(o=env.dev), SHRINK_OVERLAP)
    refuse(('shrink', 'overlap last'), shrink(o=env.dev + SET - 8), SHRINK_OVERLAP)
    refuse(('shrink', 'overlap below'), shrink(i=env.dev + 8, o=env.dev), SHRINK_OVERLAP)
    refuse.done()
    assert untouched(env)


def test_pool_entries(env):
    labels = np.array([1, -1, 1], dtype=np.int64)
    high = np.array([1, 2, 5], dtype=np.int64)
    refuse = Refusals(env)

    def pool(h=env.h, n=T, bins=BINS, t=env.dev, o=env.out):
        return lambda: env.L.kpal_pool_set_device(h, n, bins, t, 0, o)

    def groups(h=env.h, n=T, bins=BINS, t=env.dev, lab=labels, g=2, o=env.out):
        return lambda: env.L.kpal_pool_groups_device(h, n, bins, t, addr(lab), g, 0, o)

    for name, call in (('pool', pool), ('groups', groups)):
        refuse((name, 'ctx'), call(h=None), CTX_NULL)
        refuse((name, 'ctx', 'tables'), call(h=None, t=None), CTX_NULL)
        refuse((name, 'tables'), call(t=None), NULL_POINTER)
        refuse((name, 'out'), call(o=None), NULL_POINTER)
        refuse((name, 'tables', 'n'), call(t=None, n=0), NULL_POINTER)      # the pointers before the sizes
        refuse((name, 'out', 'bins'), call(o=None, bins=0), NULL_POINTER)
        refuse((name, 'n'), call(n=0), EMPTY_SET)
        refuse((name, 'n', 'bins'), call(n=0, bins=0), EMPTY_SET)           # the set before the vector
        refuse((name, 'bins'), call(bins=0), EMPTY_VECTOR)
        refuse((name, 'bins', 'aligned'), call(bins=0, t=env.dev + 4), EMPTY_VECTOR)    # the vector before the alignment
        refuse((name, 'tables + 4'), call(t=env.dev + 4), ALIGNED)
        refuse((name, 'out + 4'), call(o=env.out + 4), ALIGNED)
    refuse(('pool', 'aligned', 'bytes'), pool(o=env.out + 4, n=HUGE), ALIGNED)          # the alignment before the bytes
    refuse(('pool', 'bytes'), pool(n=HUGE), MANY_BINS)
    refuse(('pool', 'bytes', 'overlap'), pool(n=HUGE, o=env.dev), MANY_BINS)            # the bytes before the overlap
    refuse(('pool', 'columns'), pool(n=1, bins=1 << 60), '1 tables of 1152921504606846976 bins: too many bytes')
    refuse(('pool', 'in place'), pool(o=env.dev), POOL_OVERLAP)
    refuse(('pool', 'overlap last'), pool(o=env.dev + SET - 8), POOL_OVERLAP)
    refuse(('pool', 'overlap below'), pool(t=env.dev + 8, o=env.dev), POOL_OVERLAP)
    refuse(('groups', 'labels'), groups(lab=None), NULL_POINTER)
    refuse(('groups', 'labels', 'groups'), groups(lab=None, g=0), NULL_POINTER)
    refuse(('groups', 'groups'), groups(g=0), NO_GROUPS)
    refuse(('groups', 'bins', 'groups'), groups(bins=0, g=0), EMPTY_VECTOR)             # the vector before the groups
    refuse(('groups', 'groups', 'aligned'), groups(g=0, o=env.out + 4), NO_GROUPS)      # the groups before the alignment
    refuse(('groups', 'aligned', 'bytes'), groups(t=env.dev + 4, n=HUGE), ALIGNED)
    refuse(('groups', 'bytes', 'tables'), groups(n=HUGE), MANY_TABLES_GROUPS)
    refuse(('groups', 'bytes', 'groups'), groups(g=HUGE), MANY_GROUPS)
    refuse(('groups', 'bytes', 'index'), groups(n=1 << 31, bins=1), MANY_INDEX)         # more tables than a 32-bit index counts
    refuse(('groups', 'bytes', 'overlap'), groups(n=HUGE, o=env.dev), MANY_TABLES_GROUPS)   # the bytes before the overlap
    refuse(('groups', 'in place'), groups(o=env.dev), GROUPS_OVERLAP)
    refuse(('groups', 'overlap last row'), groups(t=env.dev + 8 * BINS, n=2, o=env.dev), GROUPS_OVERLAP)
    refuse(('groups', 'overlap', 'label'), groups(o=env.dev, lab=high), GROUPS_OVERLAP)     # the overlap before the labels
    refuse(('groups', 'label'), groups(lab=high), BAD_LABEL)                               # the first bad table is named
    refuse(('groups', 'label', 'one group'), groups(lab=labels, g=1), 'table 0 has label 1: there are 1 groups')
    refuse.done()
    assert untouched(env)


# ---- good arguments, once per entry, against NumPy ----------------------------------------------------------------------------
def rc_index(k):
    i = np.arange(4 ** k)
    out = np.zeros_like(i)
    for d in range(k):
        out = out * 4 + (3 - ((i >> (2 * d)) & 3))
    return out


def np_split(c, k):
    i, rc = np.arange(4 ** k), rc_index(k)
    keep = i <= rc
    return np.where(i < rc, 2 * c, c)[keep], np.where(i < rc, 2 * c[rc], c)[keep]


def np_strand_balance(c, k, pairwise):
    f, r = (a.astype(np.float64) for a in np_split(c, k))
    nz = (f != 0) | (r != 0)
    f, r = f[nz], r[nz]
    d = np.abs(f - r) / ((f + 1) * (r + 1)) if pairwise == 0 else np.abs(f - r) / (f + r + 1)
    return d.sum() / (len(d) + 1)


def close(a, b):
    return abs(a - b) <= 1e-9 * abs(b)


def same_stats(s, c):
    return ((s.total, s.non_zero, s.min, s.max, s.median) == (int(c.sum()), int(np.count_nonzero(c)), int(c.min()), int(c.max()), float(np.median(c)))
            and close(s.mean, c.mean()) and close(s.std, c.std()))


def test_good_calls(env):
    ctx, L, h, tables = env.ctx, env.L, env.h, env.tables
    rc = rc_index(K)
    balanced = tables + tables[:, rc]

    def fetch(n):
        got = np.empty(n, dtype=np.int64)
        ctx.d2h(got, env.out)
        return got

    # one vector
    ctx.h2d(env.out, tables[0])
    assert L.kpal_balance_device(h, K, env.out) == 0
    assert np.array_equal(fetch(BINS), balanced[0])
    host = tables[1].copy()
    assert L.kpal_balance(h, K, host.ctypes.data) == 0
    assert np.array_equal(host, balanced[1])
    m = (BINS + 4 ** (K // 2)) // 2
    forward, reverse, n_out = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64), ctypes.c_uint64(0)
    assert L.kpal_split(h, K, tables[2].ctypes.data, forward.ctypes.data, reverse.ctypes.data, ctypes.byref(n_out)) == 0
    want_f, want_r = np_split(tables[2], K)
    assert n_out.value == m and np.array_equal(forward, want_f) and np.array_equal(reverse, want_r)
    stats = env.native.ProfileStats()
    assert L.kpal_stats_device(h, BINS, env.dev + BINS * 8, ctypes.byref(stats)) == 0
    assert same_stats(stats, tables[1])
    stats = env.native.ProfileStats()
    assert L.kpal_stats(h, BINS, tables[2].ctypes.data, ctypes.byref(stats)) == 0
    assert same_stats(stats, tables[2])
    assert L.kpal_merge_device(h, BINS, env.dev, env.dev + BINS * 8, 1, env.out) == 0
    assert np.array_equal(fetch(BINS), (tables[0] + tables[1]) * np.logical_xor(tables[0], tables[1]))
    merged = np.zeros(BINS, dtype=np.int64)
    assert L.kpal_merge(h, BINS, tables[1].ctypes.data, tables[2].ctypes.data, 3, merged.ctypes.data) == 0
    assert np.array_equal(merged, tables[1] * np.logical_not(tables[2]))
    assert L.kpal_shrink_device(h, K, 2, env.dev, env.out) == 0
    assert np.array_equal(fetch(16), tables[0].reshape(16, 16).sum(axis=1))
    shrunk = np.zeros(64, dtype=np.int64)
    assert L.kpal_shrink(h, K, 1, tables[1].ctypes.data, shrunk.ctypes.data) == 0
    assert np.array_equal(shrunk, tables[1].reshape(64, 4).sum(axis=1))
    score = np.zeros(1)
    assert L.kpal_strand_balance(h, K, tables[0].ctypes.data, 1, f64p(score)) == 0
    assert close(score[0], np_strand_balance(tables[0], K, 1))

    # sets
    for fn, where in ((L.kpal_stats_set_device, env.dev), (L.kpal_stats_set, tables.ctypes.data)):
        many = (env.native.ProfileStats * T)()
        assert fn(h, T, BINS, where, many) == 0
        assert all(same_stats(many[t], tables[t]) for t in range(T))
    for fn, where, pairwise in ((L.kpal_strand_balance_set_device, env.dev, 0), (L.kpal_strand_balance_set, tables.ctypes.data, 1)):
        scores = np.zeros(T)
        assert fn(h, K, T, where, pairwise, f64p(scores)) == 0
        assert all(close(scores[t], np_strand_balance(tables[t], K, pairwise)) for t in range(T))
    for fn, where in ((L.kpal_distribution_set_device, env.dev), (L.kpal_distribution_set, tables.ctypes.data)):
        offsets = np.zeros(T + 1, dtype=np.uint64)
        assert fn(h, T, BINS, where, offsets.ctypes.data) == 0
        pairs = int(offsets[T])
        values, numbers = np.zeros(pairs, dtype=np.int64), np.zeros(pairs, dtype=np.uint64)
        assert L.kpal_distribution_fetch(h, 0, pairs, values.ctypes.data, numbers.ctypes.data) == 0
        assert offsets[0] == 0
        for t in range(T):
            v, n = np.unique(tables[t], return_counts=True)
            a, b = int(offsets[t]), int(offsets[t + 1])
            assert np.array_equal(values[a:b], v) and np.array_equal(numbers[a:b], n.astype(np.uint64))
    assert L.kpal_balance_set_device(h, K, T, env.dev, env.out) == 0
    assert np.array_equal(fetch(T * BINS).reshape(T, BINS), balanced)
    assert L.kpal_shrink_set_device(h, K, 1, T, env.dev, env.out) == 0
    assert np.array_equal(fetch(T * 64).reshape(T, 64), tables.reshape(T, 64, 4).sum(axis=2))
    assert L.kpal_pool_set_device(h, T, BINS, env.dev, 0, env.out) == 0
    assert np.array_equal(fetch(BINS), tables.sum(axis=0))
    labels = np.array([1, -1, 1], dtype=np.int64)
    assert L.kpal_pool_groups_device(h, T, BINS, env.dev, labels.ctypes.data, 2, 0, env.out) == 0
    assert np.array_equal(fetch(2 * BINS).reshape(2, BINS), np.stack([np.zeros(BINS, dtype=np.int64), tables[0] + tables[2]]))
    # the inputs were read only
    after = np.empty((T, BINS), dtype=np.int64)
    ctx.d2h(after, env.dev)
    assert np.array_equal(after, tables)
