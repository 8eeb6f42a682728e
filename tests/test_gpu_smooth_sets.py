"""kpal_cross_smooth_distance_device / kpal_smooth_distance_matrix_device on the GPU: dynamic smoothing over a whole rectangle or
triangle of profiles in a number of launches that does not grow with the number of pairs (kpal_amd/csrc/smooth_plan.hpp,
smooth_set_kernels.hpp, kpal_cross.hip), and the Python layer's route to them.

Every expected value is ``oracle.profile_distance(l, r, k, **options)`` on that pair, by the contract of
test_gpu_cross_options.assert_close: relative 1e-9; where the oracle is not finite the result is non-finite of the same kind;
an exact 0 of the oracle is an exact 0.  The existing entries (one pair pipeline per pair) are the second reference: 1e-9
everywhere, and bit for bit for unscaled euclidean and cosine, whose accumulators are wrapping int64 in both.

How the library decides (smooth_plan.hpp: smooth_batched): do_smooth without do_positive and pyramids within the budget ->
k x smooth_set_level, smooth_set_codes, two passes of smooth_set_super (k >= 6 and more than four profiles on both sides) or
smooth_set_tile, one reduce_partials; do_positive + do_smooth -> the existing entry's loop.

Measured duration of this file on an MI355X: 3.7 s; the worst difference from the oracle over all cases was 4.4e-13 relative
(2.3e-14 outside the planted edge cases).
"""
import io

import numpy as np
import pytest

import option_cases
from test_gpu_cross_options import PER_PAIR_KERNELS, CountingContext, _by_record_profiles, _lower, _matrix_values, assert_close, launched, options, oracle_rect, scale_sets

pytestmark = pytest.mark.gpu

SET_KERNELS = ('smooth_set_level', 'smooth_set_codes', 'smooth_set_super', 'smooth_set_tile')
# on matrix_cases' 'plain' tables (mean count 10 .. 15) these flag nodes of three or four heights, and not all of any
SETTINGS = (dict(summary='min', threshold=0), dict(summary='average', threshold=8), dict(summary='median', threshold=40),
            dict(summary='min', threshold=3), dict(summary='average', threshold=30), dict(summary='median', threshold=6))


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


class Tables(object):
    """Consecutive int64 tables in HBM for the length of a ``with``."""

    def __init__(self, ctx, tables):
        self.ctx, self.host = ctx, np.ascontiguousarray(tables, dtype=np.int64)

    def __enter__(self):
        self.ptr = self.ctx.alloc(self.host.nbytes)
        self.ctx.h2d(self.ptr, self.host)
        return self

    def read(self):
        out = np.empty_like(self.host)
        self.ctx.d2h(out, self.ptr)
        return out

    def __exit__(self, *exc):
        self.ctx.sync()
        self.ctx.free(self.ptr)


def small_sets(k, Q, R, seed):
    """Counts 0 .. 5, a third of the bins zero: at k <= 3 every height has flagged and unflagged nodes for thresholds near 1."""
    rs = np.random.RandomState(seed)
    n = 4 ** k
    return [(rs.randint(0, 6, (P, n)) * (rs.rand(P, n) < 0.67)).astype(np.int64) for P in (Q, R)]


def option_sets(k):
    if k >= 6:
        return (dict(), dict(summary='average', threshold=8, scale=True, balance=True), dict(summary='median', threshold=40, metric='cosine'),
                dict(threshold=3, scale=True, down=True, metric='sum', balance=True), dict(summary='average', threshold=30, metric='euclidean'),
                dict(summary='median', threshold=6, scale=True, metric='cosine'))
    return (dict(), dict(summary='average', threshold=1.5, scale=True, balance=True), dict(summary='median', threshold=1, metric='cosine'),
            dict(threshold=1, scale=True, down=True, metric='sum', balance=True), dict(summary='average', threshold=2.25 * 4 ** (k - 1), metric='euclidean'),
            dict(summary='median', threshold=2, scale=True, metric='cosine'))


@pytest.mark.parametrize('k,Q,R', [(1, 3, 5), (1, 1, 1), (2, 3, 5), (2, 1, 1), (3, 3, 5), (3, 1, 1), (6, 5, 7), (6, 3, 40), (6, 17, 33), (7, 17, 18)],
                         ids=lambda v: str(v))
def test_rectangle(ctx, k, Q, R):
    """k <= 3: register tiles, a pyramid of 1, 5 and 21 nodes.  k = 6: 5 x 7 is one super-tile with most rows masked, 3 x 40 the
    register tiles of a short side, 17 x 33 crosses the 16-profile edge on both sides and its 1365 nodes end in 43 dead
    elements; k = 7: 5461 nodes."""
    left, right = scale_sets(k, Q, R) if k >= 6 else small_sets(k, Q, R, seed=10 * k + Q)
    with Tables(ctx, left) as dl, Tables(ctx, right) as dr:
        for o in option_sets(k):
            native, kwargs = options(smooth=True, **o)
            got, names = launched(ctx, lambda: ctx.cross_smooth_distance_device(k, Q, dl.ptr, R, dr.ptr, native))
            assert_close(got, oracle_rect(left, right, k, kwargs), ('rectangle', k, Q, R, o))
            staged = k >= 6 and Q > 4 and R > 4
            want = {'smooth_set_level': k, 'smooth_set_codes': 1, 'smooth_set_super' if staged else 'smooth_set_tile': 2, 'reduce_partials': 1}
            assert {n: c for n, c in names.items() if not n.startswith('balance')} == want, names
        assert np.array_equal(dl.read(), left) and np.array_equal(dr.read(), right)      # (balanced copies are the library's own)


@pytest.mark.parametrize('P', (3, 12, 18))
def test_triangle(ctx, P):
    """P = 3: register tiles; 12: one super-tile; 18: three super-tiles, two on the diagonal -- each equal to the rectangle
    of the set with itself below the diagonal, and to the oracle."""
    k = 6
    prof = scale_sets(k, P, 8)[0]
    with Tables(ctx, prof) as dp:
        for o in option_sets(k):
            native, kwargs = options(smooth=True, **o)
            tri = ctx.smooth_distance_matrix_device(P, k, dp.ptr, native)
            square = ctx.cross_smooth_distance_device(k, P, dp.ptr, P, dp.ptr, native)
            assert_close(tri, _lower(oracle_rect(prof, prof, k, kwargs)), ('triangle', P, o))
            assert_close(tri, _lower(square), ('triangle against the rectangle', P, o))
            if not o.get('scale') and o.get('metric') in ('euclidean', 'cosine'):
                np.testing.assert_array_equal(tri, _lower(square), err_msg=str(o))      # exact int64 sums whatever the grid
        assert np.array_equal(dp.read(), prof)


def test_edge_cases_meet_each_other(ctx):
    """The left vectors of option_cases.edge_cases(6) against their right vectors: ties at heights 0, 1, k - 2 and k - 1 and in
    a level's last node, a root that collapses, nothing that collapses, four depths, sums that wrap or round, negative counts
    and zero totals -- every kind against every other, at every summary's tie thresholds and at 0, -0.25, +inf, 1e300, NaN."""
    k = 6
    cases = option_cases.edge_cases(k)
    assert {c.kind for c in cases} >= {'tie_min', 'tie_average', 'tie_median', 'collapse_each_level', 'big_sums', 'negative', 'totals', 'collapse_root'}
    cases.append(option_cases.build('collapse_none', k))
    cases.append(option_cases.build('negative', k, variant='zero_total'))
    left, right = np.stack([c.left for c in cases]), np.stack([c.right for c in cases])
    variants = (dict(metric='prod'), dict(metric='sum', scale=True), dict(metric='euclidean'), dict(metric='cosine', scale=True, down=True),
                dict(metric='prod', scale=True, down=True), dict(metric='sum'), dict(metric='euclidean', scale=True), dict(metric='cosine'))
    at = 0
    with Tables(ctx, left) as dl, Tables(ctx, right) as dr:
        for summary in option_cases.SUMMARIES:
            for threshold in option_cases.TIE_THRESHOLDS[summary] + (0, -0.25, float('inf'), 1e300, float('nan')):
                for o in variants[at % 2::2]:
                    native, kwargs = options(smooth=True, summary=summary, threshold=threshold, **o)
                    with np.errstate(all='ignore'):
                        got = ctx.cross_smooth_distance_device(k, len(cases), dl.ptr, len(cases), dr.ptr, native)
                    assert_close(got, oracle_rect(left, right, k, kwargs), ('edges', summary, threshold, o))
                at += 1


def test_option_grid(ctx):
    """{balance} x {none, scale, scale + down} x {prod, sum, euclidean, cosine} with smoothing, the settings in turn."""
    k, Q, R = 6, 17, 33
    left, right = scale_sets(k, Q, R)
    at = 0
    with Tables(ctx, left) as dl, Tables(ctx, right) as dr:
        for balance in (False, True):
            for scale, down in ((False, False), (True, False), (True, True)):
                for metric in ('prod', 'sum', 'euclidean', 'cosine'):
                    o = dict(balance=balance, scale=scale, down=down, metric=metric, **SETTINGS[at % len(SETTINGS)])
                    at += 1
                    native, kwargs = options(smooth=True, **o)
                    got = ctx.cross_smooth_distance_device(k, Q, dl.ptr, R, dr.ptr, native)
                    assert_close(got, oracle_rect(left, right, k, kwargs), ('grid', o))


@pytest.mark.parametrize('k,Q,R', [(6, 9, 11), (6, 3, 8), (3, 3, 5)], ids=['k6_9x11_super', 'k6_3x8_tile', 'k3_3x5_tile'])
def test_against_the_pair_pipeline(ctx, k, Q, R):
    """The existing entries loop the pair pipeline: within 1e-9 of it everywhere; unscaled euclidean and cosine bit for bit."""
    left, right = scale_sets(k, Q, R) if k >= 6 else small_sets(k, Q, R, seed=5)
    settings = SETTINGS[1:3] if k >= 6 else (dict(summary='average', threshold=1.5), dict(summary='median', threshold=2))
    with Tables(ctx, left) as dl, Tables(ctx, right) as dr:
        for setting in settings:
            for metric in ('prod', 'sum', 'euclidean', 'cosine'):
                for scale in (False, True):
                    o = dict(metric=metric, scale=scale, balance=scale, **setting)
                    native, _ = options(smooth=True, **o)
                    new = ctx.cross_smooth_distance_device(k, Q, dl.ptr, R, dr.ptr, native)
                    old, names = launched(ctx, lambda: ctx.cross_profile_distance_device(k, Q, dl.ptr, R, dr.ptr, native))
                    assert names.get('smooth_apply') == Q * R, names
                    assert_close(new, old, ('pair pipeline', k, Q, R, o))
                    if not scale and metric in ('euclidean', 'cosine'):
                        np.testing.assert_array_equal(new, old, err_msg=str(o))
    if k == 6 and Q == 9:
        P = 9
        with Tables(ctx, left) as dp:
            for metric, scale in (('euclidean', False), ('cosine', False), ('prod', True)):
                native, _ = options(smooth=True, metric=metric, scale=scale, **SETTINGS[4])
                new = ctx.smooth_distance_matrix_device(P, k, dp.ptr, native)
                old = ctx.profile_distance_matrix_device(P, k, dp.ptr, native)
                assert_close(new, old, ('pair pipeline, triangle', metric, scale))
                if not scale:
                    np.testing.assert_array_equal(new, old, err_msg=metric)


def test_positive_keeps_the_pair_pipeline(ctx):
    """With do_positive the masks come before the smoothing, node sums depend on the partner: the documented fall-back."""
    k, Q, R = 6, 5, 7
    left, right = scale_sets(k, Q, R, seed=21)
    with Tables(ctx, left) as dl, Tables(ctx, right) as dr:
        for o in (dict(summary='median', threshold=1, positive=True, metric='cosine'), dict(threshold=3, positive=True, scale=True, balance=True)):
            native, kwargs = options(smooth=True, **o)
            got, names = launched(ctx, lambda: ctx.cross_smooth_distance_device(k, Q, dl.ptr, R, dr.ptr, native))
            assert names.get('smooth_apply') == Q * R and not set(names) & set(SET_KERNELS), names
            np.testing.assert_array_equal(got, ctx.cross_profile_distance_device(k, Q, dl.ptr, R, dr.ptr, native), err_msg=str(o))
            assert_close(got, oracle_rect(left, right, k, kwargs), ('positive', o))
        native, _ = options(smooth=True, positive=True, threshold=3)
        tri, names = launched(ctx, lambda: ctx.smooth_distance_matrix_device(Q, k, dl.ptr, native))
        assert names.get('smooth_apply') == Q * (Q - 1) // 2 and not set(names) & set(SET_KERNELS), names
        np.testing.assert_array_equal(tri, ctx.profile_distance_matrix_device(Q, k, dl.ptr, native))


def test_without_smoothing_is_the_existing_entry(ctx):
    k, Q, R = 6, 5, 7
    left, right = scale_sets(k, Q, R)
    with Tables(ctx, left) as dl, Tables(ctx, right) as dr:
        for o in (dict(scale=True), dict(), dict(metric='cosine', positive=True)):
            native, _ = options(**o)
            got, names = launched(ctx, lambda: ctx.cross_smooth_distance_device(k, Q, dl.ptr, R, dr.ptr, native))
            assert not set(names) & set(SET_KERNELS + PER_PAIR_KERNELS), names
            np.testing.assert_array_equal(got, ctx.cross_profile_distance_device(k, Q, dl.ptr, R, dr.ptr, native))
            np.testing.assert_array_equal(ctx.smooth_distance_matrix_device(Q, k, dl.ptr, native), ctx.profile_distance_matrix_device(Q, k, dl.ptr, native))


def test_launch_structure(ctx):
    """The launches do not depend on Q and R: k levels, the codes, two rectangle passes, one reduction -- k + 4 -- and one
    balance per profile on top under do_balance."""
    k = 6
    seen = []
    for Q, R in ((17, 33), (40, 70)):
        left, right = scale_sets(k, Q, R)
        with Tables(ctx, left) as dl, Tables(ctx, right) as dr:
            for o in (dict(scale=True, balance=True, summary='average', threshold=8), dict(metric='cosine', threshold=3)):
                native, _ = options(smooth=True, **o)
                _, names = launched(ctx, lambda: ctx.cross_smooth_distance_device(k, Q, dl.ptr, R, dr.ptr, native))
                assert not set(names) & set(PER_PAIR_KERNELS), names
                assert names.get('balance_tiled', 0) == (Q + R if o.get('balance') else 0), names
                rest = {n: c for n, c in names.items() if n != 'balance_tiled'}
                assert sum(rest.values()) <= k + 4, rest
                seen.append(rest)
    assert all(s == seen[0] for s in seen), seen
    assert seen[0] == {'smooth_set_level': k, 'smooth_set_codes': 1, 'smooth_set_super': 2, 'reduce_partials': 1}, seen[0]


def test_deterministic(ctx):
    k, Q, R = 6, 17, 33
    left, right = scale_sets(k, Q, R)
    with Tables(ctx, left) as dl, Tables(ctx, right) as dr:
        for o in (dict(scale=True, summary='average', threshold=8), dict(scale=True, metric='cosine', balance=True, threshold=3), dict(metric='sum')):
            native, _ = options(smooth=True, **o)
            a = ctx.cross_smooth_distance_device(k, Q, dl.ptr, R, dr.ptr, native)
            b = ctx.cross_smooth_distance_device(k, Q, dl.ptr, R, dr.ptr, native)
            assert a.tobytes() == b.tobytes(), o
            c = ctx.smooth_distance_matrix_device(Q, k, dl.ptr, native)
            assert c.tobytes() == ctx.smooth_distance_matrix_device(Q, k, dl.ptr, native).tobytes(), o


def test_errors(ctx):
    from kpal_amd import _native
    smooth = _native.DistanceOptions(do_smooth=1)
    with Tables(ctx, np.ones((2, 16), dtype=np.int64)) as d:
        for bad in (lambda: ctx.cross_smooth_distance_device(2, 2, d.ptr, 2, d.ptr, _native.DistanceOptions(metric=7)),
                    lambda: ctx.cross_smooth_distance_device(2, 2, d.ptr, 2, d.ptr, _native.DistanceOptions(do_smooth=1, summary=5)),
                    lambda: ctx.cross_smooth_distance_device(17, 2, d.ptr, 2, d.ptr, smooth),
                    lambda: ctx.cross_smooth_distance_device(2, 0, d.ptr, 2, d.ptr, smooth),
                    lambda: ctx.cross_smooth_distance_device(2, 2, 0, 2, d.ptr, smooth),
                    lambda: ctx.cross_smooth_distance_device(2, 2, d.ptr + 8, 1, d.ptr, smooth),
                    lambda: ctx.smooth_distance_matrix_device(0, 2, d.ptr, smooth),
                    lambda: ctx.smooth_distance_matrix_device(2, 0, d.ptr, smooth),
                    lambda: ctx.smooth_distance_matrix_device(2, 2, 0, smooth),
                    lambda: ctx.smooth_distance_matrix_device(2, 2, d.ptr + 8, smooth)):
            with pytest.raises(ValueError):
                bad()
        assert ctx.smooth_distance_matrix_device(1, 2, d.ptr, smooth).size == 0


def _profiles(tables, prefix):
    from kpal_amd import klib
    return [klib.Profile(t.copy(), name='%s%d' % (prefix, i)) for i, t in enumerate(tables)]


def test_python_routing_host_counts(ctx):
    """kdistlib.cross_distances and kdistlib.distance_matrix with a smoothing ProfileDistance over host counts: the oracle's
    values, the set kernels, never a smooth_apply (before these entries: one per pair)."""
    from kpal_amd import kdistlib, metrics
    k, Q, R = 6, 6, 9
    left, right = scale_sets(k, Q, R)
    lp, rp = _profiles(left, 'l'), _profiles(right, 'r')
    for o, dist in ((dict(summary='average', threshold=8, scale=True, balance=True),
                     kdistlib.ProfileDistance(do_smooth=True, summary=metrics.summary['average'], threshold=8, do_scale=True, do_balance=True)),
                    (dict(summary='median', threshold=40, metric='cosine'),
                     kdistlib.ProfileDistance(do_smooth=True, summary=metrics.summary['median'], threshold=40, distance_function=metrics.cosine_similarity))):
        _, kwargs = options(smooth=True, **o)
        got, names = launched(ctx, lambda: kdistlib.cross_distances(lp, rp, dist))
        assert 'smooth_apply' not in names and names.get('smooth_set_super') == 2, names
        assert_close(got, oracle_rect(left, right, k, kwargs), ('cross_distances', o))
        out = io.StringIO()
        _, names = launched(ctx, lambda: kdistlib.distance_matrix(rp, out, 10, dist))
        assert 'smooth_apply' not in names and names.get('smooth_set_super') == 2, names
        want = _lower(oracle_rect(right, right, k, kwargs))
        text = _matrix_values(out.getvalue(), R)
        np.testing.assert_array_equal(np.isfinite(text), np.isfinite(want))
        np.testing.assert_array_equal(text[~np.isfinite(want)], want[~np.isfinite(want)])
        fin = np.isfinite(want)
        assert (np.abs(text[fin] - want[fin]) <= 1e-9 * np.abs(want[fin]) + 0.5000001e-10).all(), o      # ten decimals printed
    assert all(np.array_equal(p.counts, t) for p, t in zip(lp + rp, list(left) + list(right)))


def test_python_routing_device_resident(tmp_path):
    """from_fasta_by_record profiles still in HBM: used where they lie (no alloc / d2d / h2d / free), the set kernels, the
    oracle's values."""
    from kpal_amd import kdistlib, metrics
    k = 6
    profs = _by_record_profiles(tmp_path, k)
    count = len(profs)
    assert all(p._device_counts() is not None for p in profs)
    dctx = profs[0]._device_counts()[0]
    tables = np.empty((count, 4 ** k), dtype=np.int64)
    for i, p in enumerate(profs):
        dctx.d2h(tables[i], p._device_counts()[1])
    o = dict(summary='average', threshold=1, scale=True)
    dist = kdistlib.ProfileDistance(do_smooth=True, summary=metrics.summary['average'], threshold=1, do_scale=True)
    _, kwargs = options(smooth=True, **o)
    want = oracle_rect(tables, tables, k, kwargs)
    with CountingContext(dctx) as calls:
        square, names = launched(dctx, lambda: kdistlib.cross_distances(profs, profs, dist))
        out = io.StringIO()
        _, names2 = launched(dctx, lambda: kdistlib.distance_matrix(profs, out, 10, dist))
    assert calls == {'alloc': [], 'd2d': 0, 'h2d': 0, 'free': 0}, calls
    for got in (names, names2):
        assert 'smooth_apply' not in got and got.get('smooth_set_super') == 2 and got.get('smooth_set_level') == k, got
    assert_close(square, want, 'device-resident rectangle')
    assert np.abs(_matrix_values(out.getvalue(), count) - _lower(want)).max() <= 1e-9 * np.abs(want).max() + 0.5000001e-10
    assert all(p._device_counts() is not None for p in profs)


def test_custom_summary_stays_in_numpy(ctx):
    """A user-supplied summary callable cannot enter a kernel: the reference's recursion pair by pair, no kernel of either
    smoothing path."""
    from kpal_amd import kdistlib
    k = 3
    left, right = small_sets(k, 2, 3, seed=9)
    dist = kdistlib.ProfileDistance(do_smooth=True, summary=lambda q: np.min(q), threshold=1)
    got, names = launched(ctx, lambda: kdistlib.cross_distances(_profiles(left, 'l'), _profiles(right, 'r'), dist))
    assert not set(names) & set(SET_KERNELS + ('smooth_apply', 'smooth_level')), names
    assert_close(got, oracle_rect(left, right, k, options(smooth=True, threshold=1)[1]), 'custom summary')
