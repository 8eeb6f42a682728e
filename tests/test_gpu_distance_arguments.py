"""What the distance entries that tests/test_gpu_set_arguments.py does not reach answer to bad arguments:
kpal_cross_smooth_distance_device and kpal_smooth_distance_matrix_device (kpal_amd/csrc/kpal_cross.hip), kpal_cross_nearest and
kpal_cross_nearest_device (kpal_nearest.hip), kpal_paired_smooth_device (kpal_paired_smooth.hip) and, for coinciding faults, the
four distance entries of the linked pairs (kpal_paired.hip, kpal_paired_smooth.hip), called through ctypes where the Python
face would stop the call first.

Every case is refused on the host: the return code is KPAL_E_INVALID, kpal_last_error() is the literal below (the text in the
source), the context's profiler records no launch and the poisoned outputs stay as they are.  Where two faults coincide the ORDER
of an entry's checks decides the message; the double faults pin it -- the rectangle's smoothing entry and the nearest entries look
at the options first, the triangle's at P and k before them, the linked pairs at N, k, the pointers and the alignment before the
options, and the nearest entries at n, have and the tile caps after everything else (the host entry after its upload, which names
a NULL profile first).  3 profiles a side at k = 2 (16 bins each); no kernel runs."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, P, N = 2, 3, 16
TABLE = N * 8
E_INVALID = -1
POISON = -12345.5
INDEX_POISON = -777
HUGE = 1 << 40      # tables of k = 16 whose bytes no size_t holds

NULL_POINTER = 'NULL pointer'
TABLES_ALIGNED = 'device tables must be 16-byte aligned'
OUTPUT_ALIGNED = 'output tables must be 16-byte aligned'
OVERLAP = 'output tables overlap each other or the inputs'
OPTIONS_NULL = 'options are NULL'
P_SMALL = 'P must be >= 1'
N_SMALL = 'N must be >= 1'
QR_SMALL = 'Q and R must be >= 1'
K_RANGE = {0: 'k=0 out of range', 17: 'k=17 out of range'}
BAD_METRIC = 'unknown metric 4'
BAD_SUMMARY = 'unknown summary function 3'
BAD_CHUNK = 'chunk_pairs must be >= 0'
TOO_MANY = '%d pairs at k=16: too many bytes'
BAD_N = {0: 'nearest: n=0 out of range 1..64', 65: 'nearest: n=65 out of range 1..64'}
BAD_HAVE = {-1: 'nearest: have=-1 out of range 0..n=2', 3: 'nearest: have=3 out of range 0..n=2'}
BAD_TILE = 'nearest: negative tile cap'


@pytest.fixture(scope='module')
def env():
    from kpal_amd import _native

    class Env(object):
        pass
    e = Env()
    e.native = _native
    e.ctx = _native.context()
    e.L, e.h = e.ctx._L, e.ctx._h
    rng = np.random.RandomState(6)
    e.host = [np.ascontiguousarray(rng.randint(0, 50, N).astype(np.int64)) for _ in range(2 * P)]
    e.dev = e.ctx.alloc(2 * P * TABLE + 64)      # the left set, then the right set
    e.right = e.dev + P * TABLE
    e.res = e.ctx.alloc(2 * P * TABLE + 64)      # the two output sets of kpal_paired_smooth_device
    e.ctx.h2d(e.dev, np.concatenate(e.host))
    e.ctx.h2d(e.res, np.full(2 * P * N, -7, dtype=np.int64))
    e.ctx.sync()
    yield e
    e.ctx.free(e.res)
    e.ctx.free(e.dev)


class Refusals(object):
    """Runs calls that must be refused; `done` asserts that every one was, with its text and without a launch."""

    def __init__(self, env):
        self.env, self.wrong = env, []

    def __call__(self, what, call, text):
        ctx = self.env.ctx
        ctx.prof_enable(True)
        try:
            ctx.prof_reset()
            rc = call()
            names = {name: cnt for name, (_, cnt) in ctx.prof_get().items() if cnt}
        finally:
            ctx.prof_enable(False)
        got = self.env.L.kpal_last_error().decode()
        if rc != E_INVALID or got != text or names:
            self.wrong.append((what, rc, got, text, names))

    def done(self):
        assert not self.wrong, '\n'.join('%r: rc %d, "%s" where "%s" was expected, launches %r' % w for w in self.wrong)


def options(env, **kw):
    if kw.pop('null', False):
        return None
    o = env.native.DistanceOptions(0, 0, 0, 0, 0.0, 0, 0, 0)
    for name, v in kw.items():
        setattr(o, name, v)
    return ctypes.byref(o)


def ptrs(env, rows, null_at=None):
    return (ctypes.c_void_p * P)(*[None if i == null_at else env.host[r].ctypes.data for i, r in enumerate(rows)])


def f64p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def i64p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


# The option sets of the entries that smooth: with smoothing (the batched path), with the positive step before it (one pair
# pipeline per pair), without smoothing (the option rectangle), and the cosine alone.
SMOOTH_SETS = (dict(do_smooth=1), dict(do_smooth=1, do_scale=1, metric=3), dict(do_smooth=1, do_positive=1), dict(do_scale=1), dict(metric=3))


def test_cross_smooth_distance_device(env):
    out = np.full(P * P, POISON)
    refuse = Refusals(env)

    def call(k=K, q=P, left=env.dev, r=P, right=env.right, o=None, res=out, **kw):
        return lambda: env.L.kpal_cross_smooth_distance_device(env.h, k, q, left, r, right, options(env, **dict(o or {}, **kw)), f64p(res))

    for o in SMOOTH_SETS:
        for q, r in ((0, P), (P, 0), (0, 0), (-1, P)):
            refuse((o, q, r), call(q=q, r=r, o=o), QR_SMALL)
        for k, text in K_RANGE.items():
            refuse((o, k), call(k=k, o=o), text)
            refuse((o, k, 'metric'), call(k=k, o=o, metric=4), BAD_METRIC)      # the options first
            refuse((o, k, 'Q'), call(k=k, q=0, o=o), QR_SMALL)                  # Q and R before k
            refuse((o, k, 'left'), call(k=k, left=None, o=o), text)             # k before the pointers
        refuse((o, 'metric'), call(o=o, metric=4), BAD_METRIC)
        refuse((o, 'metric', 'Q'), call(q=0, o=o, metric=4), BAD_METRIC)
        refuse((o, 'metric', 'left'), call(left=None, o=o, metric=4), BAD_METRIC)
        refuse((o, 'left'), call(left=None, o=o), NULL_POINTER)
        refuse((o, 'right'), call(right=None, o=o), NULL_POINTER)
        refuse((o, 'out'), call(res=None, o=o), NULL_POINTER)
        refuse((o, 'left + 8'), call(left=env.dev + 8, o=o), TABLES_ALIGNED)
        refuse((o, 'right + 8'), call(right=env.right + 8, o=o), TABLES_ALIGNED)
        refuse((o, 'out', 'left + 8'), call(left=env.dev + 8, res=None, o=o), NULL_POINTER)   # the pointers before the alignment
    for o in SMOOTH_SETS[:3]:
        refuse((o, 'summary'), call(o=o, summary=3), BAD_SUMMARY)
        refuse((o, 'summary', 'k'), call(k=0, o=o, summary=3), BAD_SUMMARY)
        refuse((o, 'summary', 'metric'), call(o=o, summary=3, metric=4), BAD_METRIC)   # the metric before the summary
        refuse((o, 'summary -1'), call(o=o, summary=-1), 'unknown summary function -1')
    refuse('options', call(null=True), OPTIONS_NULL)
    refuse(('options', 'Q'), call(q=0, null=True), OPTIONS_NULL)
    refuse(('options', 'k'), call(k=0, null=True), OPTIONS_NULL)
    refuse(('options', 'left'), call(left=None, null=True), OPTIONS_NULL)
    refuse.done()
    assert (out == POISON).all()


def test_smooth_distance_matrix_device(env):
    out = np.full(P * P, POISON)
    refuse = Refusals(env)

    def run(p=P, k=K, prof=env.dev, o=None, res=out, **kw):
        return env.L.kpal_smooth_distance_matrix_device(env.h, p, k, prof, options(env, **dict(o or {}, **kw)), f64p(res))

    def call(**kw):
        return lambda: run(**kw)

    for o in SMOOTH_SETS:
        refuse((o, 'P 0'), call(p=0, o=o), P_SMALL)
        refuse((o, 'P -1'), call(p=-1, o=o), P_SMALL)
        for k, text in K_RANGE.items():
            refuse((o, k), call(k=k, o=o), text)
            refuse((o, k, 'P'), call(p=0, k=k, o=o), P_SMALL)                   # P before k
            refuse((o, k, 'metric'), call(k=k, o=o, metric=4), text)            # k before the options
            refuse((o, k, 'P 1'), call(p=1, k=k, o=o), text)
        refuse((o, 'metric'), call(o=o, metric=4), BAD_METRIC)
        refuse((o, 'metric', 'P'), call(p=0, o=o, metric=4), P_SMALL)
        refuse((o, 'metric', 'P 1'), call(p=1, o=o, metric=4), BAD_METRIC)      # the options before P == 1
        refuse((o, 'metric', 'profiles'), call(prof=None, o=o, metric=4), BAD_METRIC)
        refuse((o, 'profiles'), call(prof=None, o=o), NULL_POINTER)
        refuse((o, 'out'), call(res=None, o=o), NULL_POINTER)
        refuse((o, 'profiles + 8'), call(prof=env.dev + 8, o=o), TABLES_ALIGNED)
        refuse((o, 'out', 'profiles + 8'), call(prof=env.dev + 8, res=None, o=o), NULL_POINTER)
        assert run(p=1, o=o) == 0 and run(p=1, prof=None, res=None, o=o) == 0   # one profile: OK before the pointers are looked at
    for o in SMOOTH_SETS[:3]:
        refuse((o, 'summary'), call(o=o, summary=3), BAD_SUMMARY)
        refuse((o, 'summary', 'k'), call(k=17, o=o, summary=3), K_RANGE[17])
        refuse((o, 'summary', 'P 1'), call(p=1, o=o, summary=3), BAD_SUMMARY)
    refuse('options', call(null=True), OPTIONS_NULL)
    refuse(('options', 'P 1'), call(p=1, null=True), OPTIONS_NULL)
    refuse(('options', 'P'), call(p=0, null=True), P_SMALL)
    refuse(('options', 'k'), call(k=0, null=True), K_RANGE[0])
    refuse(('options', 'profiles'), call(prof=None, null=True), OPTIONS_NULL)
    refuse.done()
    assert (out == POISON).all()


# The routes of the nearest entries: plain, the Gram form, the option rectangle, smoothing on the host.
NEAREST_SETS = (dict(), dict(metric=2), dict(do_scale=1, do_positive=1), dict(do_smooth=1))


def test_cross_nearest(env):
    n = 2
    dist, index = np.full(P * 64, POISON), np.full(P * 64, INDEX_POISON, dtype=np.int64)
    refuse = Refusals(env)

    def device(k=K, q=P, left=env.dev, r=P, right=env.right, o=None, n_=n, have=0, tq=0, tr=0, d=dist, x=index, **kw):
        return lambda: env.L.kpal_cross_nearest_device(env.h, k, q, left, r, right, options(env, **dict(o or {}, **kw)), n_, 0, have, tq, tr, f64p(d), i64p(x))

    def host(k=K, q=P, left='left', r=P, right='right', o=None, n_=n, have=0, tq=0, tr=0, d=dist, x=index, **kw):
        left = ptrs(env, range(P)) if isinstance(left, str) else left
        right = ptrs(env, range(P, 2 * P)) if isinstance(right, str) else right
        return lambda: env.L.kpal_cross_nearest(env.h, k, q, left, r, right, options(env, **dict(o or {}, **kw)), n_, 0, have, tq, tr, f64p(d), i64p(x))

    for name, call in (('device', device), ('host', host)):
        for o in NEAREST_SETS:
            at = (name, tuple(o))
            for q, r in ((0, P), (P, 0), (-1, P)):
                refuse(at + (q, r), call(q=q, r=r, o=o), QR_SMALL)
            for k, text in K_RANGE.items():
                refuse(at + (k,), call(k=k, o=o), text)
                refuse(at + (k, 'metric'), call(k=k, o=o, metric=4), BAD_METRIC)      # the options first
                refuse(at + (k, 'Q'), call(k=k, q=0, o=o), QR_SMALL)
                refuse(at + (k, 'left'), call(k=k, left=None, o=o), text)
                refuse(at + (k, 'n'), call(k=k, n_=0, o=o), text)                     # n, have and the caps after everything else
                refuse(at + (k, 'have'), call(k=k, have=-1, o=o), text)
                refuse(at + (k, 'cap'), call(k=k, tq=-1, o=o), text)
            refuse(at + ('metric',), call(o=o, metric=4), BAD_METRIC)
            refuse(at + ('metric', 'n'), call(n_=65, o=o, metric=4), BAD_METRIC)
            for null in ('left', 'right', 'd', 'x'):
                refuse(at + (null,), call(o=o, **{null: None}), NULL_POINTER)
                refuse(at + (null, 'n'), call(n_=0, o=o, **{null: None}), NULL_POINTER)
                refuse(at + (null, 'cap'), call(tr=-1, o=o, **{null: None}), NULL_POINTER)
            refuse(at + ('Q', 'n'), call(q=0, n_=0, o=o), QR_SMALL)
            for bad, text in BAD_N.items():
                refuse(at + ('n', bad), call(n_=bad, o=o), text)
                refuse(at + ('n', bad, 'have'), call(n_=bad, have=-1, o=o), text)     # n before have
                refuse(at + ('n', bad, 'cap'), call(n_=bad, tq=-1, o=o), text)
            for bad, text in BAD_HAVE.items():
                refuse(at + ('have', bad), call(have=bad, o=o), text)
                refuse(at + ('have', bad, 'cap'), call(have=bad, tr=-1, o=o), text)   # have before the caps
            refuse(at + ('cap q',), call(tq=-1, o=o), BAD_TILE)
            refuse(at + ('cap r',), call(tr=-5, o=o), BAD_TILE)
        refuse((name, 'summary'), call(do_smooth=1, summary=3), BAD_SUMMARY)
        refuse((name, 'summary', 'n'), call(do_smooth=1, summary=3, n_=0), BAD_SUMMARY)
        refuse((name, 'options'), call(null=True), OPTIONS_NULL)
        refuse((name, 'options', 'Q'), call(q=0, null=True), OPTIONS_NULL)
        refuse((name, 'options', 'k'), call(k=17, null=True), OPTIONS_NULL)
        refuse((name, 'options', 'left'), call(left=None, null=True), OPTIONS_NULL)
        refuse((name, 'options', 'n'), call(n_=0, null=True), OPTIONS_NULL)
    for o in NEAREST_SETS:
        # the device entry: the alignment behind the pointers, before n
        refuse(('left + 8', tuple(o)), device(left=env.dev + 8, o=o), TABLES_ALIGNED)
        refuse(('right + 8', tuple(o)), device(right=env.right + 8, o=o), TABLES_ALIGNED)
        refuse(('left + 8', 'n', tuple(o)), device(left=env.dev + 8, n_=0, o=o), TABLES_ALIGNED)
        refuse(('right + 8', 'cap', tuple(o)), device(right=env.right + 8, tq=-1, o=o), TABLES_ALIGNED)
        refuse(('left + 8', 'd', tuple(o)), device(left=env.dev + 8, d=None, o=o), NULL_POINTER)
        # the host entry uploads before it looks at n: a NULL profile is named first, left before right
        refuse(('left 1', tuple(o)), host(left=ptrs(env, range(P), 1), o=o), 'left profile 1 is NULL')
        refuse(('right 2', tuple(o)), host(right=ptrs(env, range(P, 2 * P), 2), o=o), 'right profile 2 is NULL')
        refuse(('left 0', 'right 0', tuple(o)), host(left=ptrs(env, range(P), 0), right=ptrs(env, range(P, 2 * P), 0), o=o), 'left profile 0 is NULL')
        refuse(('left 1', 'n', tuple(o)), host(left=ptrs(env, range(P), 1), n_=0, o=o), 'left profile 1 is NULL')
        refuse(('right 2', 'cap', tuple(o)), host(right=ptrs(env, range(P, 2 * P), 2), tr=-1, o=o), 'right profile 2 is NULL')
        refuse(('left 1', 'k', tuple(o)), host(left=ptrs(env, range(P), 1), k=0, o=o), K_RANGE[0])
    refuse.done()
    assert (dist == POISON).all() and (index == INDEX_POISON).all()


def test_paired_smooth_device(env):
    """The single faults are test_gpu_paired_smooth.test_arguments'; here where two coincide: N, k, the three pointers of
    paired_checks, the alignment of the inputs, the right output, the summary, chunk_pairs, the bytes, the alignment of the
    outputs, the overlaps."""
    refuse = Refusals(env)
    ol, orr = env.res, env.res + P * TABLE

    def call(k=K, n=P, l=env.dev, r=env.right, s=0, chunk=0, a=ol, b=orr):
        return lambda: env.L.kpal_paired_smooth_device(env.h, k, n, l, r, s, 1.0, chunk, a, b)

    refuse(('N', 'k'), call(n=0, k=17), N_SMALL)
    refuse(('N', 'left'), call(n=-2, l=None), N_SMALL)
    refuse(('N', 'summary'), call(n=0, s=3), N_SMALL)
    refuse(('k', 'left'), call(k=17, l=None), K_RANGE[17])
    refuse(('k', 'out left'), call(k=0, a=None), K_RANGE[0])
    refuse(('k', 'summary'), call(k=0, s=3), K_RANGE[0])
    refuse(('left', 'right + 8'), call(l=None, r=env.right + 8), NULL_POINTER)
    refuse(('out left', 'left + 8'), call(a=None, l=env.dev + 8), NULL_POINTER)
    refuse(('left + 8', 'out right'), call(l=env.dev + 8, b=None), TABLES_ALIGNED)   # the right output is looked at behind the inputs' alignment
    refuse(('right + 8', 'summary'), call(r=env.right + 8, s=3), TABLES_ALIGNED)
    refuse(('out right', 'summary'), call(b=None, s=3), NULL_POINTER)
    refuse(('out right', 'chunk'), call(b=None, chunk=-1), NULL_POINTER)
    refuse(('summary', 'chunk'), call(s=3, chunk=-1), BAD_SUMMARY)
    refuse(('summary -1', 'bytes'), call(s=-1, k=16, n=HUGE), 'unknown summary function -1')
    refuse(('chunk', 'bytes'), call(chunk=-1, k=16, n=HUGE), BAD_CHUNK)
    refuse(('chunk', 'out left + 8'), call(chunk=-1, a=ol + 8), BAD_CHUNK)
    refuse(('bytes',), call(k=16, n=HUGE), TOO_MANY % HUGE)
    refuse(('bytes', 'out left + 8'), call(k=16, n=HUGE, a=ol + 8), TOO_MANY % HUGE)
    refuse(('out left + 8', 'overlap'), call(a=ol + 8, b=ol), OUTPUT_ALIGNED)
    refuse(('out right + 8', 'overlap'), call(a=env.dev, b=orr + 8), OUTPUT_ALIGNED)
    refuse(('overlap',), call(a=env.dev, b=env.right), OVERLAP)
    refuse.done()
    after = np.empty(2 * P * N, dtype=np.int64)
    env.ctx.d2h(after, env.res)
    assert (after == -7).all()


def test_paired_distance_entries(env):
    """The options against N, k, the pointers, chunk_pairs and the bytes on kpal_paired_distance[_device] and
    kpal_paired_smooth_distance[_device]: the two device entries answer alike, the two host entries answer alike."""
    out = np.full(P, POISON)
    refuse = Refusals(env)
    for name in ('kpal_paired_distance_device', 'kpal_paired_smooth_distance_device'):
        fn = getattr(env.L, name)

        def call(k=K, n=P, l=env.dev, r=env.right, chunk=0, res=out, fn=fn, **kw):
            return lambda: fn(env.h, k, n, l, r, options(env, **kw), chunk, f64p(res))

        for bad, text in ((dict(null=True), OPTIONS_NULL), (dict(metric=4), BAD_METRIC), (dict(do_smooth=1, summary=3), BAD_SUMMARY),
                          (dict(do_smooth=1, summary=3, metric=4), BAD_METRIC)):
            at = (name, tuple(bad))
            refuse(at, call(**bad), text)
            refuse(at + ('N',), call(n=0, **bad), N_SMALL)                       # N, k, the pointers and the alignment before the options
            refuse(at + ('N', 'k'), call(n=0, k=0, **bad), N_SMALL)
            refuse(at + ('k 0',), call(k=0, **bad), K_RANGE[0])
            refuse(at + ('k 17',), call(k=17, **bad), K_RANGE[17])
            refuse(at + ('left',), call(l=None, **bad), NULL_POINTER)
            refuse(at + ('out',), call(res=None, **bad), NULL_POINTER)
            refuse(at + ('left + 8',), call(l=env.dev + 8, **bad), TABLES_ALIGNED)
            refuse(at + ('right + 8',), call(r=env.right + 8, **bad), TABLES_ALIGNED)
            refuse(at + ('chunk',), call(chunk=-1, **bad), text)                 # ... chunk_pairs and the bytes after them
            refuse(at + ('bytes',), call(k=16, n=HUGE, **bad), text)
        for good in (dict(), dict(do_smooth=1), dict(do_scale=1, metric=3)):
            at = (name, tuple(good))
            refuse(at + ('N', 'k'), call(n=0, k=17, **good), N_SMALL)
            refuse(at + ('k', 'left'), call(k=17, l=None, **good), K_RANGE[17])
            refuse(at + ('chunk', 'bytes'), call(chunk=-1, k=16, n=HUGE, **good), BAD_CHUNK)
            refuse(at + ('bytes',), call(k=16, n=HUGE, **good), TOO_MANY % HUGE)
            refuse(at + ('N', 'chunk'), call(n=0, chunk=-1, **good), N_SMALL)
    many = 1 << 29
    for name in ('kpal_paired_distance', 'kpal_paired_smooth_distance'):
        fn = getattr(env.L, name)

        def call(k=K, n=P, l='left', r='right', res=out, fn=fn, **kw):
            l = ptrs(env, range(P)) if isinstance(l, str) else l
            r = ptrs(env, range(P, 2 * P)) if isinstance(r, str) else r
            return lambda: fn(env.h, k, n, l, r, options(env, **kw), f64p(res))

        for bad, text in ((dict(null=True), OPTIONS_NULL), (dict(metric=4), BAD_METRIC), (dict(do_smooth=1, summary=3), BAD_SUMMARY)):
            at = (name, tuple(bad))
            refuse(at, call(**bad), text)
            refuse(at + ('N',), call(n=0, **bad), N_SMALL)
            refuse(at + ('N', 'k'), call(n=-1, k=17, **bad), N_SMALL)
            refuse(at + ('k 0',), call(k=0, **bad), K_RANGE[0])
            refuse(at + ('k 17',), call(k=17, **bad), K_RANGE[17])
            refuse(at + ('left',), call(l=None, **bad), NULL_POINTER)
            refuse(at + ('right',), call(r=None, **bad), NULL_POINTER)
            refuse(at + ('out',), call(res=None, **bad), NULL_POINTER)
            refuse(at + ('bytes',), call(k=16, n=many, **bad), text)             # the options before the bytes and the profiles
            refuse(at + ('left 1',), call(l=ptrs(env, range(P), 1), **bad), text)
        for good in (dict(), dict(do_smooth=1), dict(do_scale=1, metric=3)):
            at = (name, tuple(good))
            refuse(at + ('bytes',), call(k=16, n=many, **good), TOO_MANY % many)
            refuse(at + ('left 1',), call(l=ptrs(env, range(P), 1), **good), 'left profile 1 is NULL')
            refuse(at + ('right 0',), call(r=ptrs(env, range(P, 2 * P), 0), **good), 'right profile 0 is NULL')
            refuse(at + ('left 2', 'right 1'), call(l=ptrs(env, range(P), 2), r=ptrs(env, range(P, 2 * P), 1), **good), 'right profile 1 is NULL')   # pair by pair
            refuse(at + ('k', 'left 1'), call(k=17, l=ptrs(env, range(P), 1), **good), K_RANGE[17])
    refuse.done()
    assert (out == POISON).all()
