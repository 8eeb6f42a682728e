"""The pair pipeline of ProfileDistance.distance with options (kpal_profile_distance, kpal_profile_distance_device,
kpal_dynamic_smooth: positive, smooth_level, smooth_apply, totals, option_distance) at value and threshold edges.

G13 (tests/golden/option_edges.*: the reference on the cases of tests/option_cases.py, k = 1 .. 6) through the Python API and
through both C entries; the same kinds planted into Poisson tables at k = 8 and k = 11 against the oracle, with tie nodes at
levels 0, 1, k - 2 and k - 1 and one of them in the last node of its level (at k = 11 a node the grid-stride loops reach on
their second trip); the launches of a call; determinism.  Smoothed vectors bit for bit; distances by the contract of
test_gpu_cross_options.assert_close (1e-9 relative, NaN for NaN, the same infinity, an exact 0 for an exact 0).

Measured duration of this file on an MI355X: NOT YET MEASURED; the worst difference from the reference and the oracle: NOT YET
MEASURED.
"""
import os

import numpy as np
import pytest

import option_cases
import oracle
from test_gpu_cross_options import SUMMARY, assert_close, launched, options

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
OPTION_KERNELS = ('positive', 'smooth_level', 'smooth_apply', 'totals', 'option_distance')


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


@pytest.fixture(scope='module')
def g13():
    return option_cases.load_golden(GOLDEN_DIR)


def short(kwargs):
    """oracle.profile_distance keywords -> the keywords of test_gpu_cross_options.options."""
    return dict(balance=kwargs['do_balance'], positive=kwargs['do_positive'], scale=kwargs['do_scale'], down=kwargs['down'],
                metric=kwargs['metric'], smooth=kwargs.get('do_smooth', False), summary=kwargs.get('summary', 'min'),
                threshold=kwargs.get('threshold', 0))


def make_distance(kwargs):
    from kpal_amd import kdistlib, metrics
    fn = {'prod': None, 'sum': None, 'euclidean': metrics.vector_distance['euclidean'], 'cosine': metrics.vector_distance['cosine']}[kwargs['metric']]
    return kdistlib.ProfileDistance(
        do_balance=kwargs['do_balance'], do_positive=kwargs['do_positive'], do_smooth=kwargs.get('do_smooth', False),
        summary=metrics.summary[kwargs.get('summary', 'min')], threshold=kwargs.get('threshold', 0), do_scale=kwargs['do_scale'],
        down=kwargs['down'], distance_function=fn, pairwise=metrics.pairwise[kwargs['metric'] if kwargs['metric'] in ('prod', 'sum') else 'prod'])


def test_g13_through_the_python_api(g13):
    from kpal_amd import kdistlib, klib, metrics
    got, want = [], []
    for g in g13:
        left, right = klib.Profile(g.left.copy(), 'l'), klib.Profile(g.right.copy(), 'r')
        for kwargs, value in g.distances:
            d = make_distance(kwargs)
            assert d._native_options() is not None
            got.append(d.distance(left, right))
            want.append(value)
        np.testing.assert_array_equal(left.counts, g.left, err_msg=g.name)      # inputs are left unmodified
        np.testing.assert_array_equal(right.counts, g.right, err_msg=g.name)
        for fn, th, a, b in g.smoothed:
            l, r = klib.Profile(g.left.copy()), klib.Profile(g.right.copy())
            kdistlib.ProfileDistance(do_smooth=True, summary=metrics.summary[fn], threshold=th).dynamic_smooth(l, r)
            np.testing.assert_array_equal(l.counts, a, err_msg='%s %s %r' % (g.name, fn, th))
            np.testing.assert_array_equal(r.counts, b, err_msg='%s %s %r' % (g.name, fn, th))
    assert_close(got, want, 'G13 through ProfileDistance')


def test_g13_through_the_c_abi(ctx, g13):
    """Host entry and device entry: the same bits, the reference's values, the device tables untouched."""
    size = 2 * 8 * 4 ** 6
    dev = ctx.alloc(size)
    try:
        host, device, want = [], [], []
        for g in g13:
            n = 4 ** g.k
            both = np.concatenate([g.left, g.right])
            ctx.h2d(dev, both)
            for kwargs, value in g.distances:
                native, _ = options(**short(kwargs))
                host.append(ctx.profile_distance(g.left, g.right, g.k, native))
                device.append(ctx.profile_distance_device(g.k, dev, dev + 8 * n, native))
                want.append(value)
            after = np.empty_like(both)
            ctx.d2h(after, dev)
            np.testing.assert_array_equal(after, both, err_msg=g.name)
            for fn, th, a, b in g.smoothed:
                l, r = g.left.copy(), g.right.copy()
                ctx.dynamic_smooth(l, r, g.k, SUMMARY[fn], th)
                np.testing.assert_array_equal(l, a, err_msg='%s %s %r' % (g.name, fn, th))
                np.testing.assert_array_equal(r, b, err_msg='%s %s %r' % (g.name, fn, th))
        np.testing.assert_array_equal(np.array(host).view(np.uint64), np.array(device).view(np.uint64))
        assert_close(host, want, 'G13 through kpal_profile_distance')
    finally:
        ctx.sync()
        ctx.free(dev)


def test_device_entry_wants_aligned_tables(ctx):
    dev = ctx.alloc(8 * 16 * 3)
    try:
        with pytest.raises(ValueError):
            ctx.profile_distance_device(2, dev + 8, dev + 8 * 17, options(scale=True)[0])
    finally:
        ctx.free(dev)


@pytest.mark.parametrize('k', (8, 11))
def test_edges_against_the_oracle(ctx, k):
    rs = np.random.RandomState(100 + k)
    got, want = [], []
    for case in option_cases.edge_cases(k):
        settings = option_cases.smooth_settings(case) if k <= 8 else [(case.summary, case.threshold)]
        if case.kind.startswith('tie_'):
            assert case.label['level'] in (0, 1, k - 2, k - 1)
        for fn, th in settings:
            l, r = case.left.copy(), case.right.copy()
            ctx.dynamic_smooth(l, r, k, SUMMARY[fn], th)
            ol, orr = oracle.dynamic_smooth(case.left, case.right, k, fn, th)
            np.testing.assert_array_equal(l, ol, err_msg='%s %s %r' % (case.name, fn, th))
            np.testing.assert_array_equal(r, orr, err_msg='%s %s %r' % (case.name, fn, th))
            if case.kind.startswith('tie_') and (fn, th) == (case.summary, case.threshold) and case.label['level']:     # the tie and the node below it
                span = 4 ** (k - case.label['level'])                                           # collapsed, the one above did not
                for node, collapsed in ((case.label['tie'], True), (case.label['below'], True), (case.label['above'], False)):
                    assert (not l[node * span + 1:(node + 1) * span].any() and not r[node * span + 1:(node + 1) * span].any()) == collapsed, (case, node)
        picks = [option_cases.GRID[i] for i in rs.choice(len(option_cases.GRID), 6 if k <= 8 else 2, replace=False)]
        sets = [dict(picks[0])] + [dict(o, do_smooth=True, summary=case.summary, threshold=case.threshold) for o in picks[1:]]
        if k <= 8:
            sets.append(dict(picks[1], do_smooth=True, summary='average', threshold=[-1.5, float('inf'), float('nan'), 1e300][rs.randint(4)]))
        for kwargs in sets:
            native, _ = options(**short(kwargs))
            got.append(ctx.profile_distance(case.left, case.right, k, native))
            with np.errstate(all='ignore'):
                want.append(oracle.profile_distance(case.left, case.right, k, **kwargs))
    assert_close(got, want, 'edges at k = %d against the oracle' % k)


def test_unusual_thresholds(ctx):
    """Negative thresholds collapse nothing on non-negative counts, +inf leaves the whole table in bin 0, NaN never collapses."""
    k = 8
    case = option_cases.build('collapse_each_level', k)
    for fn in option_cases.SUMMARIES:
        for th, what in ((-0.25, 'same'), (float('nan'), 'same'), (float('inf'), 'root'), (1e300, 'root'), (-1e300, 'same')):
            l, r = case.left.copy(), case.right.copy()
            ctx.dynamic_smooth(l, r, k, SUMMARY[fn], th)
            if what == 'same':
                np.testing.assert_array_equal(l, case.left)
                np.testing.assert_array_equal(r, case.right)
            else:
                assert l[0] == case.left.sum() and r[0] == case.right.sum() and not l[1:].any() and not r[1:].any(), (fn, th)


@pytest.mark.parametrize('k', (1, 2, 6, 11))
def test_launch_structure(ctx, k):
    """A smoothed distance at k is k smooth_level launches and one smooth_apply; totals only under do_scale, positive only
    under do_positive; a plain option set launches no option kernel."""
    case = option_cases.build('collapse_none', k)
    for o in (dict(smooth=True, threshold=4), dict(smooth=True, scale=True, metric='sum'), dict(smooth=True, positive=True, metric='cosine'),
              dict(smooth=True, positive=True, scale=True, down=True, balance=True, metric='euclidean'), dict(scale=True), dict(positive=True),
              dict(metric='cosine'), dict(), dict(balance=True, metric='sum'), dict(metric='euclidean')):
        native, _ = options(**o)
        _, names = launched(ctx, lambda: ctx.profile_distance(case.left, case.right, k, native))
        want = {'smooth_level': k if o.get('smooth') else 0, 'smooth_apply': 1 if o.get('smooth') else 0, 'totals': 1 if o.get('scale') else 0,
                'positive': 1 if o.get('positive') else 0,
                'option_distance': 1 if (o.get('smooth') or o.get('scale') or o.get('positive') or o.get('metric') == 'cosine') else 0}
        assert {name: names.get(name, 0) for name in OPTION_KERNELS} == want, (k, o, names)


def test_deterministic(ctx):
    k = 8
    for case in (option_cases.build('tie_median', k, d=k - 2, side='left', last=True, noise=True), option_cases.build('big_sums', k)):
        runs = []
        for _ in range(2):
            l, r = case.left.copy(), case.right.copy()
            ctx.dynamic_smooth(l, r, k, SUMMARY[case.summary], case.threshold)
            values = [ctx.profile_distance(case.left, case.right, k, options(**dict(short(o), smooth=True, summary=case.summary, threshold=case.threshold))[0])
                      for o in option_cases.GRID[::5]]
            runs.append((l, r, np.array(values).view(np.uint64)))
        for a, b in zip(*runs):
            np.testing.assert_array_equal(a, b, err_msg=case.name)
