"""The distance-matrix dispatch table (distance_matrix_core, kpal_amd/csrc/kpal_cross.hip; its decisions: matrix_plan.hpp), row by row.

kpal_distance_matrix picks one of several kernels from the profile count P, the table size 4^k, the metric and the counts it
meets; the staged kernels give up through their `big` flag and hand the work on.  Each row below names the kernels it must
launch -- read off distance_matrix_core, not found by running it -- and the profiler's launch counts (LAUNCH in kpal_host.hpp)
prove the path, so that a dispatch edit which sends a case to another kernel fails here even when that kernel's values are
right.  Every entry is compared with the oracle's pair function on every pair: multiset within 1e-9 relative (exactly 0,
the same NaN or the same infinity where the oracle gives one), euclidean bit for bit.

How distance_matrix_core decides (n = 4^k bins, "tiled" = k >= 6):
  * euclidean, P > 8, tiled: the fp64 Gram matrix (gram_mfma: one launch for the diagonal 64-profile blocks, a second one for
    the off-diagonal block pairs when P > 64); if some |x|^2 >= 2^53 it gives up and matrix_super<2> runs;
  * multiset, 17 <= P <= 64, tiled: matrix_rdiff_all ('prod') / matrix_rsum_all ('sum'); a count outside [0, 2^16)
    ('prod') or [0, 1024) ('sum') raises `big` and the super-tile path below runs;
  * P > 8, tiled (and what the above handed on): matrix_rdiff ('prod') / matrix_rsum ('sum'), with the same limits, then
    matrix_super; euclidean: matrix_super directly;
  * otherwise (k <= 5 or P <= 8): matrix_tile.
The profile sets come from tests/matrix_cases.py; tests/test_abi_and_host.py checks that they sit on the boundaries they name.
"""
import functools
import io
import os

import numpy as np
import pytest

import matrix_cases
import oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
METRICS = ('prod', 'sum', 'euclidean')
MATRIX_KERNELS = ('gram_mfma', 'matrix_rdiff_all', 'matrix_rsum_all', 'matrix_rdiff', 'matrix_rsum', 'matrix_super', 'matrix_tile')


def L(*names, gram=0):
    """Expected launches: one of each named kernel, ``gram`` launches of gram_mfma."""
    out = {name: 1 for name in names}
    if gram:
        out['gram_mfma'] = gram
    return out


TILE = L('matrix_tile')
RDIFF, RSUM = L('matrix_rdiff'), L('matrix_rsum')
RDIFF_ALL, RSUM_ALL = L('matrix_rdiff_all'), L('matrix_rsum_all')
RDIFF_SUPER, RSUM_SUPER = L('matrix_rdiff', 'matrix_super'), L('matrix_rsum', 'matrix_super')
RDIFF_ALL_CHAIN = L('matrix_rdiff_all', 'matrix_rdiff', 'matrix_super')
RSUM_ALL_CHAIN = L('matrix_rsum_all', 'matrix_rsum', 'matrix_super')
G1, G2 = L(gram=1), L(gram=2)
G1_SUPER, G2_SUPER = L('matrix_super', gram=1), L('matrix_super', gram=2)

ROWS = []   # (k, P, metric, do_balance, kind, expected launches, also through distance_matrix_device)


def row(k, P, metric, kind, expected, bal=False, device=False):
    ROWS.append((k, P, metric, bal, kind, expected, device))


# untiled (k <= 5): the register-tile kernel for every metric (no Gram matrix below 4096 bins)
for k in (3, 5):
    for P in (9, 40, 70):
        for metric in METRICS:
            row(k, P, metric, 'plain', TILE, bal=(k, P) == (5, 40), device=(k, P) == (3, 70))

# the profile-count boundaries at k = 6
for P, prod, sum_, euc in ((8, TILE, TILE, TILE),
                           (9, RDIFF, RSUM, G1),
                           (16, RDIFF, RSUM, G1),
                           (17, RDIFF_ALL, RSUM_ALL, G1),              # (the 256-thread form of the *_all kernels)
                           (32, RDIFF_ALL, RSUM_ALL, G1),
                           (33, RDIFF_ALL, RSUM_ALL, G1),              # (the 1024-thread form)
                           (64, RDIFF_ALL, RSUM_ALL, G1),
                           (65, RDIFF, RSUM, G2)):                     # (Gram: off-diagonal block pairs)
    for metric, want in zip(METRICS, (prod, sum_, euc)):
        row(6, P, metric, 'plain', want, device=P in (8, 65))

# more than 64 profiles; k = 10: every workgroup loops over many 64-bin slabs
for k, P, bal in ((6, 100, False), (7, 128, True), (6, 129, False), (6, 200, True), (10, 130, False)):
    for metric, want in zip(METRICS, (RDIFF, RSUM, G2)):
        row(k, P, metric, 'plain', want, bal=bal, device=P == 129)

# count limits (k = 6) at 17..64 profiles and at more than 64: the reciprocal table of matrix_rdiff (512), kRsumTable / 2 of
# the 'sum' kernels (1024), kRdiffMaxCount (2^16), the float fast path of the tile kernels (2^31); |x|^2 >= 2^53 from 2^26 on
for kind, prod40, sum40, euc40, prod70, sum70, euc70 in (
        ('max_511', RDIFF_ALL, RSUM_ALL, G1, RDIFF, RSUM, G2),
        ('max_512', RDIFF_ALL, RSUM_ALL, G1, RDIFF, RSUM, G2),
        ('max_1023', RDIFF_ALL, RSUM_ALL, G1, RDIFF, RSUM, G2),
        ('max_1024', RDIFF_ALL, RSUM_ALL_CHAIN, G1, RDIFF, RSUM_SUPER, G2),
        ('max_65535', RDIFF_ALL, RSUM_ALL_CHAIN, G1, RDIFF, RSUM_SUPER, G2),
        ('max_65536', RDIFF_ALL_CHAIN, RSUM_ALL_CHAIN, G1, RDIFF_SUPER, RSUM_SUPER, G2),
        ('max_2p31m1', RDIFF_ALL_CHAIN, RSUM_ALL_CHAIN, G1_SUPER, RDIFF_SUPER, RSUM_SUPER, G2_SUPER),
        ('max_2p31', RDIFF_ALL_CHAIN, RSUM_ALL_CHAIN, G1_SUPER, RDIFF_SUPER, RSUM_SUPER, G2_SUPER)):
    for metric, want in zip(METRICS, (prod40, sum40, euc40)):
        row(6, 40, metric, kind, want)
    for metric, want in zip(METRICS, (prod70, sum70, euc70)):
        row(6, 70, metric, kind, want, device=kind == 'max_65536')

# the Gram path's exactness limit: the last exact norm stays on the matrix cores, 2^53 falls back (both bit-identical)
for P, below, at in ((40, G1, G1_SUPER), (129, G2, G2_SUPER)):
    row(6, P, 'euclidean', 'norm_2p53m1', below, device=True)
    row(6, P, 'euclidean', 'norm_2p53', at, device=True)
for metric, want in zip(METRICS, (RDIFF_ALL_CHAIN, RSUM_ALL_CHAIN, G1)):
    row(6, 40, metric, 'norm_2p53m1', want)

# negative and int64-extreme counts: every staged multiset kernel must give up; the Gram path stays while the norms allow
for k, P, neg_prod, neg_sum, neg_euc, ext_euc in ((4, 40, TILE, TILE, TILE, TILE),
                                                  (6, 8, TILE, TILE, TILE, TILE),
                                                  (6, 12, RDIFF_SUPER, RSUM_SUPER, G1, G1_SUPER),
                                                  (6, 40, RDIFF_ALL_CHAIN, RSUM_ALL_CHAIN, G1, G1_SUPER),
                                                  (6, 70, RDIFF_SUPER, RSUM_SUPER, G2, G2_SUPER)):
    for kind in ('neg_small', 'neg_large', 'int64_extreme'):
        euc = ext_euc if kind == 'int64_extreme' else neg_euc
        for metric, want in zip(METRICS, (neg_prod, neg_sum, euc)):
            row(k, P, metric, kind, want, device=kind == 'int64_extreme' and P == 40)


def _row_id(r):
    k, P, metric, bal, kind, _, device = r
    return 'k%d-P%d-%s-%s%s%s' % (k, P, metric, kind, '-balance' if bal else '', '-device' if device else '')


IDS = [_row_id(r) for r in ROWS]
assert len(set(IDS)) == len(IDS)


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


@functools.lru_cache(maxsize=2)
def _case(kind, k, P):
    return matrix_cases.build(kind, k, P)


def _launched(ctx, run):
    """(result of run(), {matrix kernel: launches}) with the context's profiler on for just that call."""
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        out = run()
        got = {name: cnt for name, (_, cnt) in ctx.prof_get().items() if cnt and name in MATRIX_KERNELS}
    finally:
        ctx.prof_enable(False)
    return out, got


def assert_matches_oracle(got, want, metric, what):
    assert got.shape == want.shape, what
    if metric == 'euclidean':
        np.testing.assert_array_equal(got, want, err_msg=str(what))
        return
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (what, np.flatnonzero(np.isnan(got) != nan)[:8])
    inf = np.isinf(want)
    assert (got[inf] == want[inf]).all(), (what, np.flatnonzero(inf & (got != want))[:8])
    zero = want == 0
    assert (got[zero] == 0).all(), (what, np.flatnonzero(zero & (got != 0))[:8])
    fin = np.isfinite(want) & ~zero
    rel = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    assert rel.size == 0 or rel.max() <= RTOL, (what, float(rel.max()), int(np.flatnonzero(fin)[rel.argmax()]))


@pytest.mark.parametrize('k,P,metric,bal,kind,expected,device', ROWS, ids=IDS)
def test_matrix_dispatch_row(ctx, k, P, metric, bal, kind, expected, device):
    case = _case(kind, k, P)
    code = METRICS.index(metric)
    with np.errstate(all='ignore'):
        want = oracle.distance_matrix_values(case.profiles, k, bal, metric, threads=os.cpu_count() or 1)
    got, launched = _launched(ctx, lambda: ctx.distance_matrix(case.profiles, k, code, do_balance=bal))
    assert launched == expected, ('distance_matrix', launched, expected)
    assert_matches_oracle(got, want, metric, 'distance_matrix')
    if device:
        d = ctx.alloc(case.profiles.nbytes)
        try:
            ctx.h2d(d, case.profiles)
            got, launched = _launched(ctx, lambda: ctx.distance_matrix_device(P, k, d, code, bal))
        finally:
            ctx.free(d)
        assert launched == expected, ('distance_matrix_device', launched, expected)
        assert_matches_oracle(got, want, metric, 'distance_matrix_device')


def test_every_matrix_kernel_has_a_row():
    seen = {}
    for r in ROWS:
        for name, cnt in r[5].items():
            seen.setdefault(name, set()).add(cnt)
    assert set(seen) == set(MATRIX_KERNELS)
    assert seen['gram_mfma'] == {1, 2}


def test_matrix_text_of_70_host_profiles():
    """kdistlib.distance_matrix of 70 host klib.Profiles (k = 6: the super-tile path past 64 profiles) at precision 10,
    against the oracle's text."""
    from kpal_amd import klib, kdistlib
    case = matrix_cases.build('plain', 6, 70, seed=9)
    names = ['p%02d' % p for p in range(case.P)]
    profs = [klib.Profile(case.profiles[p].copy(), names[p]) for p in range(case.P)]
    want = oracle.distance_matrix_values(case.profiles, 6, False, 'prod', threads=os.cpu_count() or 1)
    # no value within 1e-13 relative of a rounding boundary of the tenth decimal (the seed is chosen for that; the kernels agree
    # with the oracle to ~1e-15): the text cannot hinge on the last bits of a value
    scaled = want * 1e10
    assert np.all(np.abs(scaled - np.floor(scaled) - 0.5) > 1e-13 * np.maximum(scaled, 1.0))
    out = io.StringIO()
    kdistlib.distance_matrix(profs, out, 10, kdistlib.ProfileDistance())
    assert out.getvalue() == oracle.distance_matrix_text(names, want, 10)
