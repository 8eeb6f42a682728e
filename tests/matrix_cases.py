"""Profile sets for the distance-matrix dispatch tests (tests/test_gpu_matrix_paths.py) -- pure NumPy, no GPU.

``build(kind, k, P)`` returns a :class:`Case`: P int64 profiles of 4^k bins made from a fixed seed, and a ``label`` of the
properties the set is BUILT to have -- the boundary it sits on.  ``properties(case)`` measures the same properties from the
profiles (exact squared norms as Python ints), and tests/test_abi_and_host.py checks that the two agree for every case the
GPU module uses, so that an edit here cannot move a case off its boundary without a CPU test failing.

Every set carries the degenerate profiles next to its boundary values:
  * profile 0 and profile 1 are identical (distance exactly 0),
  * profiles 2 and 3 differ in one bin,
  * profile P - 2 is all zero (not the last one: at 65 profiles the last one is alone in its 64-profile block, and a zero
    there would hide a wrong lookup of the off-diagonal Gram blocks).
The boundary values go into profile P // 2 (and, for pairs of values, P // 2 + 1), which for P >= 8 is none of those.

Kinds (``label``: ``max`` / ``min`` = the largest / smallest count, ``negative``, ``norm_max`` = the largest exact |x|^2):
  plain          counts 0..200
  max_<N>        counts 0..200 and a few bins at N - j (j < 300) with N itself present: the table and limit edges of the
                 staged kernels (511 / 512: the reciprocal table of matrix_rdiff; 1023 / 1024: kRsumTable / 2 of the 'sum'
                 kernels; 65535 / 65536: kRdiffMaxCount; 2^31 - 1 / 2^31: the float fast path of the tile kernels)
  norm_2p53m1    one profile with |x|^2 = 2^53 - 1 exactly, every other one far below: the Gram path's last exact norm
  norm_2p53      one profile with |x|^2 = 2^53 exactly: the Gram path must give up
  neg_small      counts -6..-2 in a few bins of two profiles (no -1), norms far below 2^53
  neg_large      counts -1000..-600 in a few bins of two profiles: every 'prod' and 'sum' denominator non-zero
  int64_extreme  in bins where every other profile is 0: profile P // 2 holds -2, INT64_MAX (x + 1 wraps) and 2^34 - 1,
                 profile P // 2 + 1 holds INT64_MIN (|x - y| wraps: NumPy's abs keeps it negative) and 2^30 in the bin of
                 the 2^34 - 1, so that (x + 1)(y + 1) = 2^64 + 2^34 wraps to 2^34 while |x - y| is large; profile P - 1
                 alone holds a -1 (denominator 0: +inf in every 'prod' pair of it), apart from the wrapping values.
                 ``wrap_visible(case)`` shows that 'prod' and 'sum' of the pairs (P // 2, 0), (P // 2 + 1, 0) and
                 (P // 2 + 1, P // 2) are finite and tell NumPy's wrap-around from arithmetic without it.

The label also carries ``norms``, every profile's exact |x|^2 as a Python int (what the Gram path's 2^53 check decides on).
"""
import math

import numpy as np

INT64_MAX = np.iinfo(np.int64).max
INT64_MIN = np.iinfo(np.int64).min
TOP = 200                                              # largest count of the plain profiles

MAX_KINDS = {'max_511': 511, 'max_512': 512, 'max_1023': 1023, 'max_1024': 1024, 'max_65535': 65535, 'max_65536': 65536,
             'max_2p31m1': (1 << 31) - 1, 'max_2p31': 1 << 31}
KINDS = ('plain', 'norm_2p53m1', 'norm_2p53', 'neg_small', 'neg_large', 'int64_extreme') + tuple(MAX_KINDS)


class Case(object):
    def __init__(self, kind, k, P, profiles, label):
        self.kind, self.k, self.P = kind, k, P
        self.profiles = profiles                       # int64[P, 4^k]
        self.label = label                             # what the set is built to have (see the module docstring)

    def __repr__(self):
        return 'Case(%s, k=%d, P=%d)' % (self.kind, self.k, self.P)


def exact_norm(v):
    """sum(x^2) of an int64 vector as a Python int (no wrap-around)."""
    v = np.asarray(v, dtype=np.int64)
    big = (v > (1 << 26)) | (v < -(1 << 26))
    small = np.where(big, 0, v)
    sq = small * small                                 # < 2^52 each: 2048 of them sum below 2^63
    pad = (-sq.size) % 2048
    chunks = np.concatenate([sq, np.zeros(pad, dtype=np.int64)]).reshape(-1, 2048).sum(axis=1)
    return sum(int(c) for c in chunks) + sum(int(x) * int(x) for x in v[big])


def four_squares(N):
    """Four non-negative integers whose squares sum to N (greedy from the top, a short search below each square)."""
    A = math.isqrt(N)
    for a in range(A, max(-1, A - 1000), -1):
        r1 = N - a * a
        B = math.isqrt(r1)
        for b in range(B, max(-1, B - 100), -1):
            r2 = r1 - b * b
            C = math.isqrt(r2)
            for c in range(C, max(-1, C - 30), -1):
                d = math.isqrt(r2 - c * c)
                if c * c + d * d == r2:
                    return a, b, c, d
    raise ValueError(N)


def _base(rs, k, P):
    n = 4 ** k
    prof = np.empty((P, n), dtype=np.int64)
    for p, hi in enumerate(rs.choice([2, 11, 121], P)):   # sparse, small and larger counts; a quarter of the bins zero
        v = rs.randint(0, hi, n, dtype=np.uint8)
        v[rs.randint(0, 4, n, dtype=np.uint8) == 0] = 0
        prof[p] = v
    prof[0, 7] = TOP                                   # TOP is present
    prof[1] = prof[0]                                  # identical pair: distance 0
    prof[3] = prof[2]
    prof[3, n // 3] += 1                               # one bin apart
    prof[P - 2] = 0                                    # all zero
    return prof


def build(kind, k, P, seed=None):
    if P < 8:
        raise ValueError('the degenerate profiles and the boundary rows need P >= 8')
    n = 4 ** k
    rs = np.random.RandomState(seed if seed is not None else (k * 1009 + P * 31 + KINDS.index(kind)) % (1 << 31))
    prof = _base(rs, k, P)
    h = P // 2
    label = {'P': P, 'k': k, 'max': TOP, 'min': 0, 'negative': False, 'norm_max_below': 1 << 53}
    if kind == 'plain':
        pass
    elif kind in MAX_KINDS:
        N = MAX_KINDS[kind]
        bins = rs.choice(n, min(50, n // 4), replace=False)
        prof[h, bins] = N - rs.randint(0, 300, bins.size)
        prof[h, bins[0]] = N
        prof[h + 1, bins[1]] = N                       # equal large counts in one bin of two profiles
        prof[h, bins[1]] = N
        label['max'] = N
        if N >= 1 << 26:                               # (the norms of these profiles leave the Gram path)
            label['norm_max_below'] = None
    elif kind in ('norm_2p53m1', 'norm_2p53'):
        N = (1 << 53) - 1 if kind == 'norm_2p53m1' else 1 << 53
        vals = four_squares(N) if kind == 'norm_2p53m1' else (1 << 26, 1 << 26)
        prof[h] = 0
        prof[h, rs.choice(n, len(vals), replace=False)] = vals
        label['max'] = max(max(vals), TOP)
        label['norm_max'] = N
        label['norm_max_below'] = None
    elif kind == 'neg_small':
        for p in (h, h + 1):
            bins = rs.choice(n, max(4, n // 64), replace=False)
            prof[p, bins] = -rs.randint(2, 7, bins.size)
        prof[h, 0] = -6
        prof[h + 1, 1] = -2
        label['min'] = -6
        label['negative'] = True
    elif kind == 'neg_large':
        for p in (h, h + 1):
            bins = rs.choice(n, max(4, n // 64), replace=False)
            prof[p, bins] = -rs.randint(600, 1001, bins.size)
        prof[h, 0] = -1000
        label['min'] = -1000
        label['negative'] = True
    elif kind == 'int64_extreme':
        free = np.setdiff1d(np.arange(n), [7, n // 3])   # (not the bins of TOP and of the one-bin pair)
        bins = rs.choice(free, 5, replace=False)
        prof[:, bins] = 0
        prof[h, bins[0]] = -2
        prof[h, bins[1]] = INT64_MAX                   # against 0: x + 1 wraps to INT64_MIN
        prof[h + 1, bins[2]] = INT64_MIN               # against 0: x - y = INT64_MIN, np.abs keeps it negative
        prof[h, bins[3]] = (1 << 34) - 1               # against 2^30: (x + 1)(y + 1) = 2^64 + 2^34 wraps to 2^34
        prof[h + 1, bins[3]] = 1 << 30
        prof[P - 1, bins[4]] = -1                      # a profile of its own: (x + 1)(y + 1) = 0
        label['max'] = INT64_MAX
        label['min'] = INT64_MIN
        label['negative'] = True
        label['norm_max_below'] = None
    else:
        raise ValueError(kind)
    label['norms'] = [exact_norm(p) for p in prof]
    return Case(kind, k, P, prof, label)


def properties(case):
    """The label's properties as measured on the profiles."""
    prof = case.profiles
    norms = [exact_norm(p) for p in prof]
    out = {'P': prof.shape[0], 'k': int(round(math.log(prof.shape[1], 4))), 'max': int(prof.max()), 'min': int(prof.min()),
           'negative': bool((prof < 0).any()), 'norms': norms}
    return out


def check_label(case):
    """AssertionError unless the case has every property its label claims (and its degenerate profiles)."""
    got = properties(case)
    lab = case.label
    assert case.profiles.dtype == np.int64 and case.profiles.shape == (case.P, 4 ** case.k), case
    for key in ('P', 'k', 'max', 'min', 'negative'):
        assert got[key] == lab[key], (case, key, got[key], lab[key])
    assert lab['norms'] == got['norms'], case
    if 'norm_max' in lab:
        assert max(lab['norms']) == lab['norm_max'], (case, max(lab['norms']), lab['norm_max'])
        assert sorted(lab['norms'])[-2] < 1 << 40, case            # one profile on the edge, the others far below
    if lab['norm_max_below'] is not None:
        assert max(lab['norms']) < lab['norm_max_below'], case
    else:
        assert max(lab['norms']) >= (1 << 53) or lab.get('norm_max') == (1 << 53) - 1, case
    if case.kind == 'int64_extreme':
        wrap_visible(case)
    prof = case.profiles
    assert (prof[0] == prof[1]).all()
    assert int((prof[2] != prof[3]).sum()) == 1
    assert not prof[case.P - 2].any() and prof[case.P - 1].any()


def _wrap64(v):
    """A Python int reduced to int64 the way NumPy's int64 arithmetic wraps."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def multiset_model(left, right, pairwise, wrap_den=True, wrap_abs=True):
    """metrics.multiset of two int64 vectors in Python ints: with both flags NumPy's own arithmetic (x - y, the denominator
    and np.abs wrap to int64), without a flag the arithmetic a kernel would do if it missed that wrap-around.  The terms are
    correctly rounded quotients summed exactly (math.fsum), or by NumPy when one is not finite."""
    terms = []
    for x, y in zip(map(int, left), map(int, right)):
        if x == 0 and y == 0:
            continue
        if wrap_abs:
            d = _wrap64(x - y)
            num = _wrap64(-d) if d < 0 else d          # np.abs(INT64_MIN) == INT64_MIN
        else:
            num = abs(x - y)
        den = (x + 1) * (y + 1) if pairwise == 'prod' else x + y + 1
        if wrap_den:
            den = _wrap64(den)
        if den == 0:
            terms.append(float('nan') if num == 0 else float('inf'))
        else:
            terms.append(float(num) / float(den) if wrap_abs and wrap_den else num / den)
    t = np.array(terms, dtype=np.float64)
    total = math.fsum(t) if np.isfinite(t).all() else t.sum()
    return total / (len(t) + 1)


def wrap_visible(case):
    """AssertionError unless the int64-extreme set can show each missed wrap-around: for 'prod' and 'sum', every one of the
    pairs (h, 0), (h + 1, 0), (h + 1, h) has a finite value, and for each way of missing the wrap (denominator, |x - y|, both)
    some pair's value moves by more than 1e-6 relative."""
    h, prof = case.P // 2, case.profiles
    pairs = ((h, 0), (h + 1, 0), (h + 1, h))
    for pw in ('prod', 'sum'):
        right = [multiset_model(prof[i], prof[j], pw) for i, j in pairs]
        assert np.isfinite(right).all(), (case, pw, right)
        for flags in ((False, True), (True, False), (False, False)):
            wrong = [multiset_model(prof[i], prof[j], pw, *flags) for i, j in pairs]
            moved = max(abs(a - b) / abs(b) for a, b in zip(wrong, right))
            assert moved > 1e-6, (case, pw, flags, right, wrong)
