"""Profile pairs for the pair-distance option pipeline (tests/test_option_cases_host.py, tests/test_gpu_option_edges.py, and
group G13 of tools/gen_golden.py) -- pure NumPy, no GPU.

``build(kind, k, **variant)`` returns a :class:`Case`: two int64 vectors of 4^k bins made from a fixed seed, the case's own
smoothing setting (``summary``, ``threshold``) and a ``label`` of the properties the pair is BUILT to have.  ``check_label(case)``
measures those properties from the vectors in exact Python-int arithmetic, so that an edit here cannot move a case off its
edge without a CPU test failing.  ``golden_cases()`` is the list of cases the reference is run on for G13.

Dynamic smoothing visits the base-4 prefix tree from the root: node ``j`` of level ``d`` (4^d nodes, d = 0 .. k - 1) covers the
bins ``[j * 4^(k-d), (j + 1) * 4^(k-d))``; it collapses when min(f(quarter sums left), f(quarter sums right)) <= threshold.

Kinds:
  tie_min, tie_average, tie_median   (``d``: level, ``side``: 'left' / 'right', ``last``: tie in the level's last node, ``noise``)
        every bin is 2000 .. 2003 (above every threshold used), except in three children of one level-(d - 1) node, written
        on ``side`` only: the TIE node's summary equals the threshold exactly, the ABOVE node is one count over it (min + 1,
        average + 1/4, median + 1/2) and the BELOW node one count under.  The other side stays far above the threshold, so
        the decision is the min over the two sides.  d = 0 has the root alone.  ``noise``: Poisson tables with every level of
        the tree below the root above the threshold are used in place of the constant-like base (k >= 8 cases).
  collapse_root        counts 0 / 1 and a threshold of 4^k: the root collapses
  collapse_none        counts 5 .. 8, threshold 4, min: nothing collapses
  collapse_each_level  the four top-level quarters collapse at four different depths (k = 4: 1, 2, 3 and never)
  big_sums             quarter sums near 2^53 in top-level quarter 0 (np.mean's float64 sum rounds: the node collapses although
                       the exact average is above the threshold), near 2^60 .. 2^62 in the others; the root's int64 sum wraps
  negative             ``variant``: 'small' (-6 .. -2), 'large' (-1000 .. -600), 'zero_total' (left total exactly 0, vector
                       not zero), 'neg_total' (left total negative and below the right total: get_scale's first branch with a
                       negative factor)
  totals               ``variant``: 'equal' (equal totals, different vectors), 'left_zero', 'right_zero', 'both_zero', 'wrap'
                       (matrix_cases' int64_extreme values: the totals wrap int64)
"""
from fractions import Fraction

import numpy as np

INT64_MAX = np.iinfo(np.int64).max
INT64_MIN = np.iinfo(np.int64).min
SUMMARIES = ('min', 'average', 'median')
METRICS = ('prod', 'sum', 'euclidean', 'cosine')
TIE_THRESHOLDS = {'min': (3, 1000), 'average': (2.25, 2.5, 2.75, 1000.5), 'median': (2.5, 3, 1000.5)}
KINDS = ('tie_min', 'tie_average', 'tie_median', 'collapse_root', 'collapse_none', 'collapse_each_level', 'big_sums', 'negative',
         'totals')
NEGATIVE_VARIANTS = ('small', 'large', 'zero_total', 'neg_total')
TOTALS_VARIANTS = ('equal', 'left_zero', 'right_zero', 'both_zero', 'wrap')

#: {balance} x {positive} x {none, scale, scale + down} x {prod, sum, euclidean, cosine}
GRID = [dict(do_balance=b, do_positive=p, do_scale=s, down=dn, metric=m)
        for b in (False, True) for p in (False, True) for s, dn in ((False, False), (True, False), (True, True)) for m in METRICS]


class Case(object):
    def __init__(self, kind, k, args, left, right, summary, threshold, label):
        self.kind, self.k, self.args = kind, k, args
        self.left, self.right = left, right              # int64[4^k] each
        self.summary, self.threshold = summary, threshold
        self.label = label
        self.name = '_'.join([kind, 'k%d' % k] + ['%s%s' % (key[0], args[key]) for key in sorted(args)])

    def __repr__(self):
        return 'Case(%s)' % self.name


# ---- exact arithmetic --------------------------------------------------------------------------------------------------
def wrap64(v):
    """A Python int reduced to int64 the way NumPy's int64 arithmetic wraps."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def exact_sum(v):
    """Sum of an int64 vector as a Python int, without wrap-around (long vectors: NumPy sums of 2048 small values at a time,
    the large values one by one)."""
    if v.size <= 4096:
        return sum(int(x) for x in v)
    big = (v >= 1 << 40) | (v <= -(1 << 40))           # (few of them; the small ones cannot wrap a sum of 2048)
    return sum(int(x) for x in v[big]) + sum(int(c) for c in np.where(big, 0, v).reshape(-1, 2048).sum(axis=1))


def quarter_sums(v, k, d, j):
    """The four quarter sums of node j of level d as ndarray.sum gives them: Python ints, wrapped to int64."""
    span = 4 ** (k - d)
    q = span // 4
    return [wrap64(exact_sum(v[j * span + i * q: j * span + (i + 1) * q])) for i in range(4)]


def exact_summary(q, summary):
    """min / mean / median of four ints as an exact Fraction."""
    if summary == 'min':
        return Fraction(min(q))
    if summary == 'average':
        return Fraction(sum(q), 4)
    s = sorted(q)
    return Fraction(s[1] + s[2], 2)


def numpy_summary(q, summary):
    """The same as NumPy evaluates it on an int64 array of four: the values converted to float64 one by one and summed."""
    if summary == 'min':
        return float(min(q))
    if summary == 'average':
        return (((float(q[0]) + float(q[1])) + float(q[2])) + float(q[3])) / 4.0
    s = sorted(q)
    return (float(s[1]) + float(s[2])) / 2.0


def total(v):
    """np.sum of an int64 vector: (exact Python int, wrapped to int64)."""
    t = exact_sum(v)
    return t, wrap64(t)


# ---- builders ----------------------------------------------------------------------------------------------------------
def _seed(kind, k, args):
    text = kind + repr(k) + repr(sorted(args.items()))
    return sum((i + 1) * ord(c) for i, c in enumerate(text)) % (1 << 31)


def _plant(v, k, d, j, q, rs):
    """Make q the quarter sums of node j of level d: one bin per quarter holds the sum, the rest of the node is zero."""
    span = 4 ** (k - d)
    qs = span // 4
    v[j * span:(j + 1) * span] = 0
    for i in range(4):
        v[j * span + i * qs + rs.randint(qs)] = q[i]


def tie_quarters(summary, threshold):
    """(tie, above, below): quarter sums whose summary is the threshold, one count over it and one count under it."""
    T = Fraction(threshold)
    if summary == 'min':
        t = int(T)
        assert t == T
        return [t + 2, t, t + 7, t + 1], [t + 2, t + 1, t + 7, t + 1], [t + 2, t - 1, t + 7, t + 1]
    if summary == 'average':
        S = int(4 * T)
        assert S == 4 * T
        a = S // 4
        q = [a + 1, a - 1, S - 3 * a, a]
        return q, [q[0] + 1] + q[1:], [q[0], q[1] - 1] + q[2:]
    M = int(2 * T)
    assert M == 2 * T
    lo = (M - 1) // 2                                    # lower and upper middle: lo < hi, lo + hi = 2 T
    hi = M - lo
    return [hi + 5, lo, max(lo - 2, 0), hi], [hi + 5, lo, max(lo - 2, 0), hi + 1], [hi + 5, lo - 1, max(lo - 2, 0), hi]


def _tie(kind, k, args, rs):
    summary = kind[4:]
    d, side, last, noise = args['d'], args.get('side', 'left'), args.get('last', False), args.get('noise', False)
    if not 0 <= d < k:
        raise ValueError('no level %d at k = %d' % (d, k))
    n = 4 ** k
    threshold = args.get('threshold', TIE_THRESHOLDS[summary][d % len(TIE_THRESHOLDS[summary])])
    if noise:
        own, other = rs.poisson(3000, n).astype(np.int64), rs.poisson(3500, n).astype(np.int64)
    else:
        own, other = (2000 + (rs.rand(n) < 0.125) * rs.randint(1, 4, n)).astype(np.int64), (2000 + (rs.rand(n) < 0.125) * rs.randint(1, 4, n)).astype(np.int64)
    tie, above, below = tie_quarters(summary, threshold)
    label = {'summary': summary, 'threshold': threshold, 'level': d, 'side': side, 'above': None, 'below': None}
    if d == 0:
        _plant(own, k, 0, 0, tie, rs)
        label['tie'] = 0
    else:
        parent = 4 ** (d - 1) - 1 if last else int(rs.randint(4 ** (d - 1)))
        kids = [3, 2, 1] if last else [int(c) for c in rs.permutation(4)[:3]]
        label['tie'], label['above'], label['below'] = (4 * parent + c for c in kids)
        _plant(own, k, d, label['tie'], tie, rs)
        _plant(own, k, d, label['above'], above, rs)
        _plant(own, k, d, label['below'], below, rs)
    left, right = (own, other) if side == 'left' else (other, own)
    return Case(kind, k, args, left, right, summary, threshold, label)


def _collapse(kind, k, args, rs):
    n = 4 ** k
    if kind == 'collapse_root':
        left, right = rs.randint(0, 2, n).astype(np.int64), rs.randint(0, 2, n).astype(np.int64)
        left[n - 1] = right[0] = 1                       # (never all zero)
        return Case(kind, k, args, left, right, 'average', float(n), {'collapsed': {0: [0]}})
    if kind == 'collapse_none':
        left, right = rs.randint(5, 9, n).astype(np.int64), rs.randint(5, 9, n).astype(np.int64)
        return Case(kind, k, args, left, right, 'min', 4, {'collapsed': {}})
    if k < 4:
        raise ValueError('four different depths need k >= 4')
    depths = [1, 2, 3, None] if k == 4 else [1, 2, k - 1, 3]
    left, right = np.full(n, 5, dtype=np.int64), np.full(n, 6, dtype=np.int64)
    top = n // 4
    for quarter, depth in enumerate(depths):
        if depth is None:
            continue
        span = 4 ** (k - depth)                          # every level-`depth` node of this quarter gets one small quarter sum,
        for j in range(quarter * top // span, (quarter + 1) * top // span):   # on the left or on the right
            v = left if rs.randint(2) else right
            qs = span // 4
            at = j * span + int(rs.randint(4)) * qs
            v[at:at + qs] = 0
            v[at + rs.randint(qs)] = 2
    return Case(kind, k, args, left, right, 'min', 3, {'depths': depths})


def _big_offsets(rs, base, threshold, int_first_differs):
    """Four offsets o with base + o the quarter sums of a node whose NumPy average is <= threshold while the exact average
    (and, if asked for, the average of the int64 sum) is above it."""
    for _ in range(10000):
        q = [base + int(o) for o in rs.randint(0, 16, 4)]
        if (numpy_summary(q, 'average') <= threshold < exact_summary(q, 'average')
                and (not int_first_differs or float(wrap64(sum(q))) / 4.0 > threshold)):
            return q
    raise ValueError('no offsets found')


def _big_sums(kind, k, args, rs):
    n = 4 ** k
    left = np.zeros(n, dtype=np.int64)
    if k == 1:
        threshold = float(1 << 62)
        q = _big_offsets(rs, 1 << 62, threshold, False)         # the root itself: sums near 2^62, wraps, rounds
        left[:] = q
        label = {'rounds': (0, 0), 'wraps_root': True, 'near': [62]}
    else:
        threshold = float(1 << 53)
        q0 = _big_offsets(rs, 1 << 53, threshold, True)        # level-1 node 0: collapses by rounding alone
        _plant(left, k, 1, 0, q0, rs)
        for node in (1, 2, 3):                           # the other three: about 2^62 each, never collapsing on 'average'
            _plant(left, k, 1, node, [(1 << 60) + int(o) for o in rs.randint(1, 1 << 20, 4)], rs)
        label = {'rounds': (1, 0), 'wraps_root': True, 'near': [53, 60, 62]}
    right = left.copy()
    right[right != 0] += 4096 * rs.randint(1, 5, int((right != 0).sum()))   # the same tree, every float64 summary above the left's
    return Case(kind, k, args, left, right, 'average', threshold, label)


def _negative(kind, k, args, rs):
    n = 4 ** k
    variant = args['variant']
    left, right = rs.randint(0, 9, n).astype(np.int64), rs.randint(0, 9, n).astype(np.int64)
    some = max(2, n // 8)
    label = {'variant': variant, 'negative': True}
    if variant in ('small', 'zero_total', 'neg_total'):
        for v in (left, right):
            bins = rs.choice(n, some, replace=False)
            v[bins] = -rs.randint(2, 7, some)
        left[0], right[1] = -6, -2
        label['min'] = -6
    else:
        for v in (left, right):
            bins = rs.choice(n, some, replace=False)
            v[bins] = -rs.randint(600, 1001, some)
        left[0] = -1000
        label['min'] = -1000
    if variant == 'zero_total':
        left[n - 1] = 0
        left[n - 1] = -int(left.sum())
        label['left_total'] = 0
        label['min'] = min(int(left.min()), int(right.min()))
    elif variant == 'neg_total':
        left[n - 1] = 0
        left[n - 1] = -int(left.sum()) - 7               # left total -7, right total made positive
        right[n - 2] = 0
        right[n - 2] = 12 - int(right.sum())
        label['left_total'], label['right_total'] = -7, 12
        label['min'] = min(int(left.min()), int(right.min()))
    return Case(kind, k, args, left, right, 'average', -2.5, label)


def _totals(kind, k, args, rs):
    n = 4 ** k
    variant = args['variant']
    left, right = rs.randint(0, 9, n).astype(np.int64), rs.randint(0, 12, n).astype(np.int64)
    left[0], right[n - 1] = 3, 4
    label = {'variant': variant}
    if variant == 'equal':
        right = np.roll(left, 1)
        right[0], right[1] = right[1], right[0]
        if np.array_equal(left, right):
            right[2] += 1
            right[3] -= 1
        label['equal'] = True
    elif variant == 'left_zero':
        left[:] = 0
    elif variant == 'right_zero':
        right[:] = 0
    elif variant == 'both_zero':
        left[:] = 0
        right[:] = 0
    elif variant == 'wrap':
        if n < 16:                                       # four bins: one wrapping value pair per side
            left[1], left[2] = INT64_MAX, (1 << 34) - 1
            right[1], right[2] = INT64_MIN, -(1 << 30)
            left[3], right[3] = INT64_MAX, -2
        else:
            bins = rs.choice(np.arange(1, n - 1), 6, replace=False)
            left[bins], right[bins] = 0, 0
            left[bins[0]] = -2
            left[bins[1]] = INT64_MAX
            right[bins[2]] = INT64_MIN
            left[bins[3]], right[bins[3]] = (1 << 34) - 1, 1 << 30
            left[bins[4]] = INT64_MAX                    # two INT64_MAX: the left total wraps
            right[bins[5]] = -(1 << 40)                  # INT64_MIN + 2^30 - 2^40 + small counts: the right total wraps
        label['wraps'] = True
    else:
        raise ValueError(variant)
    return Case(kind, k, args, left, right, 'median', 1, label)


def build(kind, k, **args):
    rs = np.random.RandomState(_seed(kind, k, args))
    if kind.startswith('tie_') and kind[4:] in SUMMARIES:
        return _tie(kind, k, args, rs)
    if kind.startswith('collapse_'):
        return _collapse(kind, k, args, rs)
    if kind == 'big_sums':
        return _big_sums(kind, k, args, rs)
    if kind == 'negative':
        return _negative(kind, k, args, rs)
    if kind == 'totals':
        return _totals(kind, k, args, rs)
    raise ValueError(kind)


def golden_cases():
    """Every case of G13, k = 1 .. 6."""
    out = []
    for k in (1, 2, 4, 6):
        for summary in SUMMARIES:
            for d in range(k):
                for side in ('left', 'right'):
                    out.append(build('tie_' + summary, k, d=d, side=side))
        out.append(build('collapse_root', k))
        out.append(build('collapse_none', k))
    out.append(build('collapse_each_level', 4))
    out.append(build('collapse_each_level', 6))
    for k in (1, 2, 3, 5):
        out.append(build('big_sums', k))
    for k in (1, 2, 4):
        for variant in NEGATIVE_VARIANTS:
            out.append(build('negative', k, variant=variant))
        for variant in TOTALS_VARIANTS:
            out.append(build('totals', k, variant=variant))
    return out


def edge_cases(k):
    """The planted cases of the GPU tests at k = 8 and k = 11: ties at levels 0, 1, k - 2 and k - 1 of every summary function
    between them, on both sides, two in the last node of their level; at k = 8 the other kinds too."""
    out = [build('tie_min', k, d=0, side='left', noise=True),
           build('tie_average', k, d=1, side='right', noise=True),
           build('tie_median', k, d=k - 2, side='left', last=True, noise=True),
           build('tie_average', k, d=k - 1, side='right', last=True, noise=True)]
    if k <= 8:
        out += [build('tie_median', k, d=k - 1, side='left', noise=True), build('tie_min', k, d=k - 2, side='right', noise=True),
                build('collapse_each_level', k), build('big_sums', k),
                build('negative', k, variant='neg_total'), build('totals', k, variant='wrap'),
                build('totals', k, variant='both_zero'), build('collapse_root', k)]
    return out


def full_grid(case):
    """Kinds about scaling and signs keep the whole option grid in G13; the others a fixed-seed sample of it."""
    return case.kind in ('big_sums', 'negative', 'totals')


def smooth_settings(case):
    """Three (summary, threshold) per case, the case's own first."""
    others = {'tie_min': [('average', 2000.5), ('median', 4001)], 'tie_average': [('min', 2001), ('median', 1999.5)],
              'tie_median': [('min', 0), ('average', 2001.75)]}
    if case.kind in others:
        rest = others[case.kind]
    elif case.kind == 'big_sums':
        rest = [('min', float('inf')), ('median', float(1 << 60))]
    else:
        rest = [('min', 0), ('median', 5.5)] if case.summary == 'average' else [('average', 6.25), ('median', 0.5)]
    return [(case.summary, case.threshold)] + rest


# ---- labels ------------------------------------------------------------------------------------------------------------
def decisions(case, summary=None, threshold=None, numpy_rounding=True):
    """{level: [collapsed nodes]} as the top-down recursion reaches them, in Python ints (float64 summaries as NumPy rounds
    them, or exact Fractions with ``numpy_rounding=False``)."""
    summary = summary or case.summary
    threshold = case.threshold if threshold is None else threshold
    f = numpy_summary if numpy_rounding else exact_summary
    out, k = {}, case.k
    todo = [(0, 0)]
    while todo:
        d, j = todo.pop()
        if d == k:
            continue
        if min(f(quarter_sums(case.left, k, d, j), summary), f(quarter_sums(case.right, k, d, j), summary)) <= threshold:
            out.setdefault(d, []).append(j)
        else:
            todo.extend((d + 1, 4 * j + c) for c in range(4))
    return {d: sorted(v) for d, v in out.items()}


def check_label(case):
    """AssertionError unless the case has every property its label claims."""
    k, lab = case.k, case.label
    n = 4 ** k
    for v in (case.left, case.right):
        assert v.dtype == np.int64 and v.shape == (n,), case
    if case.kind.startswith('tie_'):
        d, T = lab['level'], Fraction(lab['threshold'])
        assert lab['summary'] == case.summary == case.kind[4:] and lab['threshold'] == case.threshold, case
        own, other = (case.left, case.right) if lab['side'] == 'left' else (case.right, case.left)
        step = {'min': Fraction(1), 'average': Fraction(1, 4), 'median': Fraction(1, 2)}[case.summary]
        assert exact_summary(quarter_sums(own, k, d, lab['tie']), case.summary) == T, case
        assert exact_summary(quarter_sums(other, k, d, lab['tie']), case.summary) > T + 100, case
        if d == 0:
            assert lab['tie'] == 0 and lab['above'] is None and lab['below'] is None, case
        else:
            assert len({lab['tie'] // 4, lab['above'] // 4, lab['below'] // 4}) == 1, case      # siblings
            assert len({lab['tie'], lab['above'], lab['below']}) == 3, case
            assert exact_summary(quarter_sums(own, k, d, lab['above']), case.summary) == T + step, case
            assert exact_summary(quarter_sums(own, k, d, lab['below']), case.summary) == T - step, case
            assert sum(quarter_sums(own, k, d, lab['above'])) - sum(quarter_sums(own, k, d, lab['tie'])) == 1, case
            assert sum(quarter_sums(own, k, d, lab['tie'])) - sum(quarter_sums(own, k, d, lab['below'])) == 1, case
            for node in (lab['above'], lab['below']):
                assert exact_summary(quarter_sums(other, k, d, node), case.summary) > T + 100, case
        j = lab['tie']
        for up in range(d - 1, -1, -1):                  # every ancestor is visited and passed: both sides above the threshold
            j //= 4
            for v in (own, other):
                assert exact_summary(quarter_sums(v, k, up, j), case.summary) > T, (case, up, j)
        if k <= 8:                                       # (the whole recursion in Python ints)
            got = decisions(case)
            assert lab['tie'] in got.get(d, []), (case, got)
            if d:
                assert lab['below'] in got[d] and lab['above'] not in got[d], (case, got)
        if case.args.get('last'):
            assert lab['tie'] == 4 ** d - 1, case
    elif case.kind in ('collapse_root', 'collapse_none'):
        assert decisions(case) == lab['collapsed'], (case, decisions(case))
        assert case.left.any() and case.right.any() and case.left.min() >= 0 and case.right.min() >= 0, case
    elif case.kind == 'collapse_each_level':
        got = decisions(case)
        assert 0 not in got, case
        for quarter, depth in enumerate(lab['depths']):
            for d in range(1, k):
                lo, hi = quarter * 4 ** (d - 1), (quarter + 1) * 4 ** (d - 1)
                mine = [j for j in got.get(d, []) if lo <= j < hi]
                assert mine == (list(range(lo, hi)) if d == depth else []), (case, quarter, d, mine)
        assert len(set(lab['depths'])) == 4, case
    elif case.kind == 'big_sums':
        d, j = lab['rounds']
        q = quarter_sums(case.left, k, d, j)
        T = Fraction(case.threshold)
        assert numpy_summary(q, 'average') <= case.threshold and exact_summary(q, 'average') > T, (case, q)
        if k > 1:
            assert float(wrap64(sum(q))) / 4.0 > case.threshold, (case, q)     # summed in int64 first: another decision
        exact, wrapped = total(case.left)
        assert lab['wraps_root'] and exact != wrapped, case
        found = [x for dd in range(min(k, 2)) for jj in range(4 ** dd) for x in quarter_sums(case.left, k, dd, jj)]
        for bits in lab['near']:
            assert any((1 << bits) <= x < (1 << bits) + (1 << 24) for x in found), (case, bits)
        assert decisions(case) != decisions(case, numpy_rounding=False), case
        for dd, nodes in decisions(case).items():        # the right side never decides: the left's summary is the min
            for jj in nodes:
                assert numpy_summary(quarter_sums(case.left, k, dd, jj), 'average') <= numpy_summary(quarter_sums(case.right, k, dd, jj), 'average'), case
    elif case.kind == 'negative':
        assert min(int(case.left.min()), int(case.right.min())) == lab['min'] < 0, case
        assert not ((case.left == -1) | (case.right == -1)).any() or lab['variant'] in ('zero_total', 'neg_total'), case
        if 'left_total' in lab:
            assert total(case.left) == (lab['left_total'],) * 2 and case.left.any(), case
        if 'right_total' in lab:
            assert total(case.right) == (lab['right_total'],) * 2, case
            assert total(case.left)[1] < total(case.right)[1] and total(case.left)[1] < 0, case     # first branch, negative factor
    elif case.kind == 'totals':
        (le, lw), (re, rw) = total(case.left), total(case.right)
        v = lab['variant']
        if v == 'equal':
            assert lw == rw and le == re and not np.array_equal(case.left, case.right), case
        assert (not case.left.any()) == (v in ('left_zero', 'both_zero')), case
        assert (not case.right.any()) == (v in ('right_zero', 'both_zero')), case
        assert ((le != lw) and (re != rw)) == bool(lab.get('wraps')), (case, le, lw, re, rw)
    else:
        raise AssertionError(case.kind)


# ---- G13 ---------------------------------------------------------------------------------------------------------------
class Golden(object):
    """One G13 record: the stored inputs, the reference's smoothed vectors [(summary, threshold, left, right)], its scale
    factors, and its distances [(keyword arguments of oracle.profile_distance, value)]."""

    def __init__(self, rec, grid, z):
        self.name, self.kind, self.k, self.args = rec['name'], rec['kind'], rec['k'], rec['args']
        self.summary, self.threshold = rec['summary'], float(rec['threshold'])
        n, at = 4 ** self.k, rec['at']
        self.left, self.right = z['g13_inputs'][at:at + n], z['g13_inputs'][at + n:at + 2 * n]
        self.smoothed = []
        for fn, th, off, cnt in rec['smoothed']:
            a, b = self.left.copy(), self.right.copy()
            idx = z['g13_changed_idx'][off:off + cnt]
            a[idx], b[idx] = z['g13_changed_l'][off:off + cnt], z['g13_changed_r'][off:off + cnt]
            self.smoothed.append((fn, float(th), a, b))
        self.scale = [float(x) for x in rec['scale']]
        self.distances = [(dict(grid[gi]), float(v)) for gi, v in rec['plain']]
        self.distances += [(dict(grid[gi], do_smooth=True, summary=self.summary, threshold=self.threshold), float(v)) for gi, v in rec['smooth']]
        self.distances += [(dict(grid[gi], do_smooth=True, summary=fn, threshold=float(th)), float(v)) for gi, fn, th, v in rec['extra']]

    def __repr__(self):
        return 'Golden(%s)' % self.name


def load_golden(golden_dir):
    """[Golden] of tests/golden/option_edges.json and option_edges.npz."""
    import json
    import os
    with open(os.path.join(golden_dir, 'option_edges.json')) as fh:
        g = json.load(fh)['G13']
    z = dict(np.load(os.path.join(golden_dir, 'option_edges.npz')))
    return [Golden(rec, g['grid'], z) for rec in g['cases']]
