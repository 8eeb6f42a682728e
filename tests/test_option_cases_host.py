"""G13 (tools/gen_golden.py g13: the reference on the cases of tests/option_cases.py) on the CPU: the oracle against the
reference's smoothed vectors and distances, the labels of the cases, and the cases' teeth -- a small model of the pair pipeline
with a switch for each plausible mistake, every one of which some G13 case must notice.

The switch ``totals_early`` takes the scale totals before positive AND smoothing: smoothing alone conserves both totals (mod
2^64: a collapsed node keeps its wrapped sum), so totals taken between positive and smoothing are the same numbers and no case
can tell.  The switch ``scale_le`` (``<=`` for ``<`` in get_scale) differs from the reference only where the totals are equal:
non-zero equal totals give the factor 1.0 on either side, and with 0 == 0 the NaN factor moves to the other profile, which
leaves every metric NaN -- it is visible in the recorded scale factors alone, and that is what its test looks at.
"""
import os

import numpy as np
import pytest

import option_cases
import oracle
from option_cases import wrap64
from test_gpu_cross_options import assert_close

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SMOOTH_SWITCHES = ('lt', 'median_lower', 'median_upper', 'average_intdiv', 'average_int64_first', 'nowrap')
DISTANCE_SWITCHES = ('positive_late', 'totals_early')


@pytest.fixture(scope='module')
def g13():
    return option_cases.load_golden(GOLDEN_DIR)


def test_inputs_are_the_cases(g13):
    """The stored inputs are what option_cases builds today, every kind is present, and both files together stay below the
    largest golden file."""
    cases = option_cases.golden_cases()
    assert [c.name for c in cases] == [g.name for g in g13] and len(set(g.name for g in g13)) == len(g13)
    for c, g in zip(cases, g13):
        np.testing.assert_array_equal(c.left, g.left, err_msg=c.name)
        np.testing.assert_array_equal(c.right, g.right, err_msg=c.name)
        assert (c.summary, c.threshold, c.k) == (g.summary, g.threshold, g.k)
        assert [(fn, th) for fn, th, _, _ in g.smoothed] == [(fn, float(th)) for fn, th in option_cases.smooth_settings(c)]
    assert set(c.kind for c in cases) == set(option_cases.KINDS)
    assert set(c.k for c in cases) >= {1, 2, 4, 6}
    size = sum(os.path.getsize(os.path.join(GOLDEN_DIR, f)) for f in ('option_edges.json', 'option_edges.npz'))
    assert size < os.path.getsize(os.path.join(GOLDEN_DIR, 'vectors.npz')), size


@pytest.mark.parametrize('case', option_cases.golden_cases(), ids=lambda c: c.name)
def test_label(case):
    option_cases.check_label(case)


@pytest.mark.parametrize('k', (8, 11))
def test_labels_of_the_planted_cases(k):
    """The cases tests/test_gpu_option_edges.py runs at k = 8 and k = 11: the same label checks, and the levels and the last
    nodes that module relies on (at k = 11 the last node of level 10 is past the first trip of the grid-stride loops:
    8 blocks of 256 threads on each of 256 compute units cover 524288 of its 1048576 nodes)."""
    cases = option_cases.edge_cases(k)
    for case in cases:
        option_cases.check_label(case)
    ties = [c for c in cases if c.kind.startswith('tie_')]
    assert {c.label['level'] for c in ties} == {0, 1, k - 2, k - 1}
    assert {c.kind for c in ties} == {'tie_min', 'tie_average', 'tie_median'} and {c.label['side'] for c in ties} == {'left', 'right'}
    last = [c for c in ties if c.args.get('last')]
    assert {c.label['level'] for c in last} == {k - 2, k - 1} and all(c.label['tie'] == 4 ** c.label['level'] - 1 for c in last)
    if k == 11:
        assert 4 ** 10 - 1 >= 8 * 256 * 256


def test_oracle_smoothing_is_the_reference(g13):
    checked = 0
    for g in g13:
        for fn, th, a, b in g.smoothed:
            oa, ob = oracle.dynamic_smooth(g.left, g.right, g.k, fn, th)
            np.testing.assert_array_equal(oa, a, err_msg='%s %s %r' % (g.name, fn, th))
            np.testing.assert_array_equal(ob, b, err_msg='%s %s %r' % (g.name, fn, th))
            checked += 1
    assert checked == 3 * len(g13)


def test_oracle_distances_are_the_reference(g13):
    got, want = [], []
    for g in g13:
        for kwargs, value in g.distances:
            with np.errstate(all='ignore'):
                got.append(oracle.profile_distance(g.left, g.right, g.k, **kwargs))
            want.append(value)
    assert len(want) > 5000 and np.isnan(want).any() and np.isinf(want).any() and (np.array(want) == 0).any()
    assert_close(got, want, 'oracle against G13')


# ---- the model ---------------------------------------------------------------------------------------------------------
def model_summary(q, summary, sw):
    if summary == 'min':
        return float(min(q))
    if summary == 'average':
        if sw == 'average_intdiv':
            return float(sum(q) // 4)
        if sw == 'average_int64_first':
            return float(wrap64(sum(q))) / 4.0
        return (((float(q[0]) + float(q[1])) + float(q[2])) + float(q[3])) / 4.0
    s = sorted(q)
    if sw == 'median_lower':
        return float(s[1])
    if sw == 'median_upper':
        return float(s[2])
    return (float(s[1]) + float(s[2])) / 2.0


def model_smooth(left, right, k, summary, threshold, sw=None):
    """The level sweep: bottom-up the node sums and decisions of every level, then top-down the topmost deciding node wins.
    Python ints throughout (lists), wrapped to int64 where NumPy's sums wrap."""
    add = sum if sw == 'nowrap' else (lambda q: wrap64(sum(q)))
    sums = {k: ([int(x) for x in left], [int(x) for x in right])}
    decide = {}
    for d in range(k - 1, -1, -1):
        cl, cr = sums[d + 1]
        sl, sr, dec = [], [], []
        for j in range(4 ** d):
            ql, qr = cl[4 * j:4 * j + 4], cr[4 * j:4 * j + 4]
            sl.append(add(ql))
            sr.append(add(qr))
            f = min(model_summary(ql, summary, sw), model_summary(qr, summary, sw))
            dec.append(f < threshold if sw == 'lt' else f <= threshold)
        sums[d], decide[d] = (sl, sr), dec
    out_l, out_r = list(sums[k][0]), list(sums[k][1])
    todo = [(0, 0)]
    while todo:
        d, j = todo.pop()
        if d == k:
            continue
        if decide[d][j]:
            span = 4 ** (k - d)
            out_l[j * span:(j + 1) * span] = [sums[d][0][j]] + [0] * (span - 1)
            out_r[j * span:(j + 1) * span] = [sums[d][1][j]] + [0] * (span - 1)
        else:
            todo.extend((d + 1, 4 * j + c) for c in range(4))
    return out_l, out_r


def model_balance(v, k):
    idx = np.arange(4 ** k)
    comp, rc = 4 ** k - 1 - idx, np.zeros(4 ** k, dtype=np.int64)
    for _ in range(k):
        rc, comp = rc * 4 + comp % 4, comp // 4
    return v + v[rc]


def model_factors(tl, tr, sw=None):
    with np.errstate(all='ignore'):
        if (tl <= tr) if sw == 'scale_le' else (tl < tr):
            return np.int64(tr) / np.int64(tl), 1.0
        return 1.0, np.int64(tl) / np.int64(tr)


def model_distance(left, right, k, sw=None, do_balance=False, do_positive=False, do_smooth=False, summary='min', threshold=0,
                   do_scale=False, down=False, metric='prod'):
    def positive(l, r):
        l = l * (r != 0)
        return l, r * (l != 0)

    with np.errstate(all='ignore'):
        l, r = np.array(left, dtype=np.int64), np.array(right, dtype=np.int64)
        if do_balance:
            l, r = model_balance(l, k), model_balance(r, k)
        early = (int(l.sum()), int(r.sum()))
        if do_positive and sw != 'positive_late':
            l, r = positive(l, r)
        if do_smooth:
            l, r = (np.array(v, dtype=np.int64) for v in model_smooth(l, r, k, summary, threshold, sw))
        if do_positive and sw == 'positive_late':
            l, r = positive(l, r)
        if do_scale:
            tl, tr = early if sw == 'totals_early' else (int(l.sum()), int(r.sum()))
            ls, rs = model_factors(tl, tr, sw)
            if down:
                top = max(ls, rs)
                ls, rs = ls / top, rs / top
            l, r = l * ls, r * rs
        if metric in ('prod', 'sum'):
            keep = (l != 0) | (r != 0)
            x, y = l[keep], r[keep]
            terms = np.abs(x - y) / ((x + 1) * (y + 1)) if metric == 'prod' else np.abs(x - y) / (x + y + 1)
            return float(terms.sum() / (len(terms) + 1))
        if metric == 'euclidean':
            return float(np.sqrt(np.dot(l - r, l - r)))
        return float(np.dot(l, r) / (np.sqrt(np.dot(l, l)) * np.sqrt(np.dot(r, r))))


def moved(got, want):
    """A distance that is another kind of value, or more than 1e-6 relative away."""
    if np.isnan(want) or np.isnan(got):
        return bool(np.isnan(want) != np.isnan(got))
    if np.isinf(want) or np.isinf(got):
        return got != want
    return abs(got - want) > 1e-6 * abs(want)


def test_model_is_the_reference(g13):
    """With every switch off the model gives the recorded smoothed vectors bit for bit, the recorded scale factors and the
    recorded distances."""
    got, want = [], []
    for g in g13:
        for fn, th, a, b in g.smoothed:
            ml, mr = model_smooth(g.left, g.right, g.k, fn, th)
            assert ml == [int(x) for x in a] and mr == [int(x) for x in b], (g, fn, th)
        assert_close(model_factors(int(g.left.sum()), int(g.right.sum())), g.scale, None)
        for kwargs, value in g.distances:
            got.append(model_distance(g.left, g.right, g.k, **kwargs))
            want.append(value)
    assert_close(got, want, 'model against G13')


@pytest.mark.parametrize('sw', SMOOTH_SWITCHES)
def test_smoothing_mistakes_are_noticed(g13, sw):
    caught = []
    for g in g13:
        for fn, th, a, b in g.smoothed:
            ml, mr = model_smooth(g.left, g.right, g.k, fn, th, sw)
            if ml != [int(x) for x in a] or mr != [int(x) for x in b]:
                caught.append((g.name, fn, th))
    print(sw, len(caught), caught[:6])
    assert caught, sw
    if sw in ('lt', 'median_lower', 'median_upper'):       # the tie cases are what these are for
        assert any(name.startswith('tie_') for name, _, _ in caught), caught
    if sw in ('average_int64_first', 'nowrap'):
        assert any(name.startswith('big_sums') for name, _, _ in caught), caught


@pytest.mark.parametrize('sw', DISTANCE_SWITCHES)
def test_pipeline_order_mistakes_are_noticed(g13, sw):
    caught = []
    for g in g13:
        for kwargs, value in g.distances:
            if not ((kwargs['do_positive'] and kwargs.get('do_smooth')) if sw == 'positive_late' else (kwargs['do_positive'] and kwargs['do_scale'])):
                continue
            if moved(model_distance(g.left, g.right, g.k, sw, **kwargs), value):
                caught.append((g.name, kwargs))
                break
    print(sw, len(caught), caught[:3])
    assert caught, sw


def test_scale_branch_mistake_is_noticed_in_the_factors(g13):
    """``<=`` for ``<``: see the module docstring -- the recorded factors of the equal-total cases move, no distance can."""
    caught = []
    for g in g13:
        tl, tr = int(g.left.sum()), int(g.right.sum())
        wrong = model_factors(tl, tr, 'scale_le')
        if any(moved(a, b) for a, b in zip(wrong, g.scale)):
            caught.append(g.name)
            assert tl == tr == 0, g
            for kwargs, value in g.distances:
                if kwargs['do_scale']:
                    assert np.isnan(value) and np.isnan(model_distance(g.left, g.right, g.k, 'scale_le', **kwargs)), (g, kwargs)
    print(caught)
    assert any('zero_total' in name or 'both_zero' in name for name in caught), caught
