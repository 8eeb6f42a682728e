"""What the distance entries answer to bad arguments: kpal_distance_matrix[_device], kpal_profile_distance_matrix[_device],
kpal_cross_distance[_device], kpal_cross_profile_distance[_device] (kpal_amd/csrc/kpal_cross.hip), kpal_pair_distance_device
and kpal_profile_distance[_device] (kpal_pair.hip), called through ctypes where the Python face would stop the call first.

Every case is refused on the host, before any launch: the return code is KPAL_E_INVALID and kpal_last_error() is the literal
below, which is the text in the source.  Where two faults coincide the ORDER of an entry's checks decides the message; the
double faults pin it -- the matrix entries look at P before the options, the rectangle's option entries at the options first.
3 profiles of k = 2 (16 bins each)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, P, N = 2, 3, 16
E_INVALID = -1
POISON = -12345.5

NULL_POINTER = 'NULL pointer'
TABLES_ALIGNED = 'device tables must be 16-byte aligned'
VECTORS_ALIGNED = 'device vectors must be 16-byte aligned'
OPTIONS_NULL = 'options are NULL'
P_SMALL = 'P must be >= 1'
QR_SMALL = 'Q and R must be >= 1'
K_RANGE = {0: 'k=0 out of range', 17: 'k=17 out of range'}
BAD_METRIC = {3: 'unknown metric 3', 4: 'unknown metric 4'}
BAD_SUMMARY = 'unknown summary function 3'
NEEDS_4K = 'do_balance needs n == 4^k'


@pytest.fixture(scope='module')
def env():
    from kpal_amd import _native

    class Env(object):
        pass
    e = Env()
    e.native = _native
    e.ctx = _native.context()
    e.L, e.h = e.ctx._L, e.ctx._h
    rng = np.random.RandomState(5)
    e.host = [np.ascontiguousarray(rng.randint(0, 50, N).astype(np.int64)) for _ in range(P)]
    e.dev = e.ctx.alloc(P * N * 8 + 64)
    e.ctx.h2d(e.dev, np.concatenate(e.host))
    e.ctx.sync()
    yield e
    e.ctx.free(e.dev)


def ptrs(env, null_at=None):
    return (ctypes.c_void_p * P)(*[None if i == null_at else a.ctypes.data for i, a in enumerate(env.host)])


def options(env, **kw):
    o = env.native.DistanceOptions(0, 0, 0, 0, 0.0, 0, 0, 0)
    for name, v in kw.items():
        setattr(o, name, v)
    return ctypes.byref(o)


def out_array(count=P * P):
    return np.full(count, POISON, dtype=np.float64)


def f64p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def refused(env, rc, text):
    assert rc == E_INVALID, (rc, text)
    assert env.L.kpal_last_error().decode() == text


# ---- the four entries of a set against itself: (name, call(P, k, profiles, metric or options, out)) -----------------------------
def tri_plain_device(env, p, k, prof, metric, out):
    return env.L.kpal_distance_matrix_device(env.h, p, k, prof, metric, 0, out)


def tri_plain_host(env, p, k, prof, metric, out):
    return env.L.kpal_distance_matrix(env.h, p, k, prof, metric, 0, out)


def tri_option_device(env, p, k, prof, opt, out):
    return env.L.kpal_profile_distance_matrix_device(env.h, p, k, prof, opt, out)


def tri_option_host(env, p, k, prof, opt, out):
    return env.L.kpal_profile_distance_matrix(env.h, p, k, prof, opt, out)


def test_triangle_plain(env):
    out = out_array()
    for call, prof in ((tri_plain_device, env.dev), (tri_plain_host, ptrs(env))):
        refused(env, call(env, 0, K, prof, 0, f64p(out)), P_SMALL)
        refused(env, call(env, -1, K, prof, 0, f64p(out)), P_SMALL)
        for k, text in K_RANGE.items():
            refused(env, call(env, P, k, prof, 0, f64p(out)), text)
            refused(env, call(env, P, k, prof, 3, f64p(out)), text)      # bad k and bad metric: k is looked at first
        refused(env, call(env, P, K, prof, 3, f64p(out)), BAD_METRIC[3])
        refused(env, call(env, P, K, None, 0, f64p(out)), NULL_POINTER)
        refused(env, call(env, P, K, prof, 0, None), NULL_POINTER)
        refused(env, call(env, 0, 0, prof, 3, f64p(out)), P_SMALL)
        assert call(env, 1, K, prof, 0, f64p(out)) == 0                  # one profile: no pair, nothing written
    # the device entry looks at the metric before the pointers, the host entry uploads (and names a NULL profile) before it
    refused(env, tri_plain_device(env, P, K, None, 3, f64p(out)), BAD_METRIC[3])
    refused(env, tri_plain_host(env, P, K, None, 3, f64p(out)), NULL_POINTER)
    refused(env, tri_plain_host(env, P, K, ptrs(env, 1), 0, f64p(out)), 'profile 1 is NULL')
    refused(env, tri_plain_host(env, P, K, ptrs(env, 2), 3, f64p(out)), 'profile 2 is NULL')
    # a single profile is OK before the pointers are looked at
    assert tri_plain_device(env, 1, K, None, 0, None) == 0 and tri_plain_host(env, 1, K, None, 0, None) == 0
    assert (out == POISON).all()


def test_triangle_options(env):
    out = out_array()
    scaled = dict(do_scale=1)
    for call, prof in ((tri_option_device, env.dev), (tri_option_host, ptrs(env))):
        for kw in ({}, scaled):
            refused(env, call(env, 0, K, prof, options(env, **kw), f64p(out)), P_SMALL)
            for k, text in K_RANGE.items():
                refused(env, call(env, P, k, prof, options(env, **kw), f64p(out)), text)
                refused(env, call(env, P, k, prof, options(env, metric=4, **kw), f64p(out)), text)   # k before the options
            refused(env, call(env, P, K, prof, options(env, metric=4, **kw), f64p(out)), BAD_METRIC[4])
            refused(env, call(env, P, K, prof, options(env, do_smooth=1, summary=3, **kw), f64p(out)), BAD_SUMMARY)
            refused(env, call(env, P, K, prof, options(env, do_smooth=1, summary=-1, **kw), f64p(out)), 'unknown summary function -1')
            refused(env, call(env, P, K, prof, options(env, metric=4, do_smooth=1, summary=3, **kw), f64p(out)), BAD_METRIC[4])
            refused(env, call(env, P, K, None, options(env, **kw), f64p(out)), NULL_POINTER)
            refused(env, call(env, P, K, prof, options(env, **kw), None), NULL_POINTER)
            refused(env, call(env, 1, K, prof, options(env, metric=4, **kw), f64p(out)), BAD_METRIC[4])   # the options before P == 1
            assert call(env, 1, K, prof, options(env, **kw), f64p(out)) == 0
            assert call(env, 1, K, None, options(env, **kw), None) == 0
        refused(env, call(env, P, K, prof, None, f64p(out)), OPTIONS_NULL)
        refused(env, call(env, 1, K, prof, None, f64p(out)), OPTIONS_NULL)
        refused(env, call(env, 0, K, prof, None, f64p(out)), P_SMALL)      # NULL options and P = 0: P first
        refused(env, call(env, P, 0, prof, None, f64p(out)), K_RANGE[0])   # ... and k
    for kw in ({}, scaled, dict(metric=3)):
        refused(env, tri_option_host(env, P, K, ptrs(env, 1), options(env, **kw), f64p(out)), 'profile 1 is NULL')
    # an address off by 8 bytes: the option pipeline refuses it (the plain entry it delegates to has no such check)
    refused(env, tri_option_device(env, P, K, env.dev + 8, options(env, **scaled), f64p(out)), TABLES_ALIGNED)
    refused(env, tri_option_device(env, P, K, env.dev + 8, options(env, metric=3), f64p(out)), TABLES_ALIGNED)
    assert (out == POISON).all()


# ---- the four entries of a left set against a right set --------------------------------------------------------------------------
def rect_plain_device(env, k, q, left, r, right, metric, out):
    return env.L.kpal_cross_distance_device(env.h, k, q, left, r, right, metric, 0, out)


def rect_plain_host(env, k, q, left, r, right, metric, out):
    return env.L.kpal_cross_distance(env.h, k, q, left, r, right, metric, 0, out)


def rect_option_device(env, k, q, left, r, right, opt, out):
    return env.L.kpal_cross_profile_distance_device(env.h, k, q, left, r, right, opt, out)


def rect_option_host(env, k, q, left, r, right, opt, out):
    return env.L.kpal_cross_profile_distance(env.h, k, q, left, r, right, opt, out)


def test_rectangle_plain(env):
    out = out_array()
    for call, prof in ((rect_plain_device, env.dev), (rect_plain_host, ptrs(env))):
        for q, r in ((0, P), (P, 0), (0, 0), (-1, P)):
            refused(env, call(env, K, q, prof, r, prof, 0, f64p(out)), QR_SMALL)
        for k, text in K_RANGE.items():
            refused(env, call(env, k, P, prof, P, prof, 0, f64p(out)), text)
            refused(env, call(env, k, P, prof, P, prof, 3, f64p(out)), text)
        refused(env, call(env, K, P, prof, P, prof, 3, f64p(out)), BAD_METRIC[3])
        refused(env, call(env, K, P, None, P, prof, 3, f64p(out)), BAD_METRIC[3])   # the metric before the pointers
        refused(env, call(env, K, P, None, P, prof, 0, f64p(out)), NULL_POINTER)
        refused(env, call(env, K, P, prof, P, None, 0, f64p(out)), NULL_POINTER)
        refused(env, call(env, K, P, prof, P, prof, 0, None), NULL_POINTER)
        refused(env, call(env, 0, 0, prof, P, prof, 3, f64p(out)), QR_SMALL)
    refused(env, rect_plain_host(env, K, P, ptrs(env, 0), P, ptrs(env), 0, f64p(out)), 'left profile 0 is NULL')
    refused(env, rect_plain_host(env, K, P, ptrs(env), P, ptrs(env, 2), 0, f64p(out)), 'right profile 2 is NULL')
    refused(env, rect_plain_host(env, K, P, ptrs(env, 1), P, ptrs(env, 0), 0, f64p(out)), 'left profile 1 is NULL')
    refused(env, rect_plain_device(env, K, P, env.dev + 8, P, env.dev, 0, f64p(out)), TABLES_ALIGNED)
    refused(env, rect_plain_device(env, K, P, env.dev, P, env.dev + 8, 0, f64p(out)), TABLES_ALIGNED)
    assert (out == POISON).all()


def test_rectangle_options(env):
    out = out_array()
    scaled = dict(do_scale=1)
    for call, prof in ((rect_option_device, env.dev), (rect_option_host, ptrs(env))):
        for kw in ({}, scaled):
            for q, r in ((0, P), (P, 0)):
                refused(env, call(env, K, q, prof, r, prof, options(env, **kw), f64p(out)), QR_SMALL)
            for k, text in K_RANGE.items():
                refused(env, call(env, k, P, prof, P, prof, options(env, **kw), f64p(out)), text)
                refused(env, call(env, k, P, prof, P, prof, options(env, metric=4, **kw), f64p(out)), BAD_METRIC[4])   # the options first
            refused(env, call(env, K, P, prof, P, prof, options(env, metric=4, **kw), f64p(out)), BAD_METRIC[4])
            refused(env, call(env, K, 0, prof, P, prof, options(env, metric=4, **kw), f64p(out)), BAD_METRIC[4])
            refused(env, call(env, K, P, prof, P, prof, options(env, do_smooth=1, summary=3, **kw), f64p(out)), BAD_SUMMARY)
            refused(env, call(env, K, P, None, P, prof, options(env, **kw), f64p(out)), NULL_POINTER)
            refused(env, call(env, K, P, prof, P, None, options(env, **kw), f64p(out)), NULL_POINTER)
            refused(env, call(env, K, P, prof, P, prof, options(env, **kw), None), NULL_POINTER)
        refused(env, call(env, K, P, prof, P, prof, None, f64p(out)), OPTIONS_NULL)
        refused(env, call(env, K, 0, prof, P, prof, None, f64p(out)), OPTIONS_NULL)   # NULL options and Q = 0: the options first
        refused(env, call(env, 0, P, prof, P, prof, None, f64p(out)), OPTIONS_NULL)
    for kw in ({}, scaled, dict(metric=3)):
        refused(env, rect_option_host(env, K, P, ptrs(env, 2), P, ptrs(env), options(env, **kw), f64p(out)), 'left profile 2 is NULL')
        refused(env, rect_option_host(env, K, P, ptrs(env), P, ptrs(env, 0), options(env, **kw), f64p(out)), 'right profile 0 is NULL')
        refused(env, rect_option_device(env, K, P, env.dev + 8, P, env.dev, options(env, **kw), f64p(out)), TABLES_ALIGNED)
        refused(env, rect_option_device(env, K, P, env.dev, P, env.dev + 8, options(env, **kw), f64p(out)), TABLES_ALIGNED)
    assert (out == POISON).all()


# ---- one pair --------------------------------------------------------------------------------------------------------------------
def test_pair_distance_device(env):
    out = out_array(1)
    L, h, d = env.L, env.h, env.dev
    for metric in (0, 3):
        refused(env, L.kpal_pair_distance_device(h, N, None, d, metric, 0, K, f64p(out), None), NULL_POINTER)
        refused(env, L.kpal_pair_distance_device(h, N, d, None, metric, 0, K, f64p(out), None), NULL_POINTER)
        refused(env, L.kpal_pair_distance_device(h, N, d, d, metric, 0, K, None, None), NULL_POINTER)
    refused(env, L.kpal_pair_distance_device(h, N, d, d, 3, 0, K, f64p(out), None), BAD_METRIC[3])
    refused(env, L.kpal_pair_distance_device(h, N, d, d, -1, 0, K, f64p(out), None), 'unknown metric -1')
    refused(env, L.kpal_pair_distance_device(h, N, d + 8, d, 3, 0, K, f64p(out), None), BAD_METRIC[3])   # the metric before the alignment
    refused(env, L.kpal_pair_distance_device(h, N, d + 8, d, 0, 0, K, f64p(out), None), VECTORS_ALIGNED)
    refused(env, L.kpal_pair_distance_device(h, N, d, d + 8, 0, 0, K, f64p(out), None), VECTORS_ALIGNED)
    # k matters with do_balance only, and after everything else
    for k in (0, 17, 3):
        refused(env, L.kpal_pair_distance_device(h, N, d, d, 0, 1, k, f64p(out), None), NEEDS_4K)
        refused(env, L.kpal_pair_distance_device(h, N, d, d, 3, 1, k, f64p(out), None), BAD_METRIC[3])
        refused(env, L.kpal_pair_distance_device(h, N, d + 8, d, 0, 1, k, f64p(out), None), VECTORS_ALIGNED)
    assert (out == POISON).all()


def test_profile_distance(env):
    out = out_array(1)
    L, h, d = env.L, env.h, env.dev
    hl, hr = env.host[0].ctypes.data, env.host[1].ctypes.data
    for call, l, r in ((L.kpal_profile_distance_device, d, d + N * 8), (L.kpal_profile_distance, hl, hr)):
        for kw in ({}, dict(do_scale=1)):
            for k, text in K_RANGE.items():
                refused(env, call(h, k, l, r, options(env, **kw), f64p(out)), text)
                refused(env, call(h, k, l, r, options(env, metric=4, **kw), f64p(out)), text)     # bad k and bad metric: k first
                refused(env, call(h, k, None, r, None, f64p(out)), text)
            refused(env, call(h, K, None, r, options(env, **kw), f64p(out)), NULL_POINTER)
            refused(env, call(h, K, l, None, options(env, **kw), f64p(out)), NULL_POINTER)
            refused(env, call(h, K, l, r, options(env, **kw), None), NULL_POINTER)
            refused(env, call(h, K, l, r, options(env, metric=4, **kw), f64p(out)), BAD_METRIC[4])
            refused(env, call(h, K, l, r, options(env, do_smooth=1, summary=3, **kw), f64p(out)), BAD_SUMMARY)
            refused(env, call(h, K, None, r, options(env, metric=4, **kw), f64p(out)), NULL_POINTER)   # the pointers before the options
        refused(env, call(h, K, l, r, None, f64p(out)), OPTIONS_NULL)
        refused(env, call(h, K, None, r, None, f64p(out)), NULL_POINTER)
    refused(env, L.kpal_profile_distance_device(h, K, d + 8, d, options(env), f64p(out)), VECTORS_ALIGNED)
    refused(env, L.kpal_profile_distance_device(h, K, d, d + 8, options(env, do_scale=1), f64p(out)), VECTORS_ALIGNED)
    refused(env, L.kpal_profile_distance_device(h, K, d + 8, d, None, f64p(out)), VECTORS_ALIGNED)     # the alignment before the options
    assert (out == POISON).all()


def test_good_arguments_still_answer(env):
    """The same calls with nothing wrong return OK and the values of the pair function (the harness above would also pass
    on a library that refuses everything)."""
    L, h = env.L, env.h
    tri = out_array(3)
    assert tri_plain_device(env, P, K, env.dev, 0, f64p(tri)) == 0
    pair = out_array(1)
    assert L.kpal_pair_distance_device(h, N, env.dev + N * 8, env.dev, 0, 0, K, f64p(pair), None) == 0
    assert abs(tri[0] - pair[0]) <= 1e-12 * abs(pair[0]) and np.isfinite(tri).all()   # (16 bins added in two orders)
    rect = out_array()
    assert rect_option_device(env, K, P, env.dev, P, env.dev, options(env, do_scale=1), f64p(rect)) == 0
    assert np.isfinite(rect).all() and (np.diag(rect.reshape(P, P)) == 0).all()
