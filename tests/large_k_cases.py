"""Tables and references for the whole-table operations at large k (tests/test_gpu_large_k.py) -- pure NumPy, no GPU.

A table of k = 15 or 16 (8 / 32 GiB) does not fit the dense oracle, so its references are restated here over the COMPACTED
SUPPORT of a sparse table: the sorted indices where a value is non-zero, and the values there.  Every restatement follows the
oracle's statement (oracle/kpal_oracle.c) and is pinned to the dense oracle on full tables of k = 5 to 10 by
tests/test_abi_and_host.py::test_large_k_restatements_equal_the_dense_oracle, before the GPU module trusts it.

  * sparse_table / sparse_pair: structured sparse tables -- both ends of the table, palindromes (even k), pairs i / rc(i)
    both non-zero, entries in self-paired 64 x 64 tiles, the first and last row and column of tiles, tiles on either side of
    every bit of the tile number (the bits that the tile order of k >= 13 permutes among them), indices at and above 2^31 and
    just below 2^32 where the table has them -- with values beyond 2^32, negatives, INT64_MAX (x + 1 wraps) and pairs whose
    (x + 1)(y + 1) wraps.
  * balance, positive, smooth, scale, merge, shrink, stats, profile_distance: the operations on (idx, val) supports.  Zero
    bins add nothing to a multiset, euclidean or cosine sum and are skipped by the multiset, so the oracle's metric run on
    the values at the union of two supports, in index order, is the metric of the full tables.
  * DenseTable: a full table made chunk by chunk from a seed (a few distinct values plus some extremes), with the exact
    count of every distinct value, from which total, mean, median and std follow without holding the table.
"""
import math

import numpy as np

import oracle

INT64_MAX = np.iinfo(np.int64).max
INT64_MIN = np.iinfo(np.int64).min
MERGERS = ('sum', 'xor', 'int', 'nint')


# -- indices ---------------------------------------------------------------------------------------------------------------
def rc_index(idx, k):
    """reverse_complement for every index (vectorised klib.py:394-412: complement, then the k digits in reverse order)."""
    comp = ~np.asarray(idx, dtype=np.uint64)
    rc = np.zeros_like(comp)
    for d in range(k):
        rc |= ((comp >> np.uint64(2 * d)) & np.uint64(3)) << np.uint64(2 * (k - 1 - d))
    return rc.astype(np.int64)


def tile_of(idx, k):
    """The 64 x 64 tile (k - 6 middle digits) of the tiled balance kernels that holds each index (k >= 6)."""
    return (np.asarray(idx, dtype=np.int64) >> 6) & ((1 << (2 * (k - 6))) - 1)


def _at(a, md, b, k):
    """Index of row a (top 3 digits), tile M (k - 6 middle digits), column b (low 3 digits)."""
    return (np.asarray(a, dtype=np.int64) << (2 * (k - 3))) | (np.asarray(md, dtype=np.int64) << 6) | np.asarray(b, dtype=np.int64)


def structured_indices(k, rs, n_random):
    """Indices where a large-k kernel can go wrong (see the module docstring), plus n_random uniform ones."""
    n = 1 << (2 * k)
    parts = [np.array([0, n - 1, 1, n - 2, n // 2 - 1, n // 2], dtype=np.int64)]
    for at in ((1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, (1 << 32) - 2, (1 << 32) - 64, 3 << 30):
        if at < n:
            parts.append(np.array([at], dtype=np.int64))
    if n > (1 << 31):
        parts.append(rs.randint(1 << 31, min(n, 1 << 32), size=2000, dtype=np.int64))
    parts.append(rs.randint(0, n, size=n_random, dtype=np.int64))
    if k % 2 == 0:                                   # palindromes: high half = rc(low half)
        low = rs.randint(0, 1 << k, size=500, dtype=np.int64)
        parts.append((rc_index(low, k // 2) << k) | low)
    both = rs.randint(0, n, size=2000, dtype=np.int64)
    parts += [both, rc_index(both, k)]               # i and rc(i) both non-zero
    if k >= 6:
        md = k - 6
        nM = 1 << (2 * md)
        tiles = [rs.randint(0, nM, size=8, dtype=np.int64)]
        if md % 2 == 0:                              # self-paired tiles M = rc(M)
            h = rs.randint(0, 1 << md, size=8, dtype=np.int64) if md else np.zeros(1, dtype=np.int64)
            tiles.append((rc_index(h, md // 2) << md) | h if md else h)
        for bit in range(2 * md):                    # either side of every tile-number bit
            m0 = rs.randint(0, nM, size=2, dtype=np.int64)
            tiles += [m0 & ~np.int64(1 << bit), m0 | np.int64(1 << bit)]
        tiles.append(np.array([0, nM - 1], dtype=np.int64))                 # the first and the last tile
        tiles = np.unique(np.concatenate(tiles))
        edge = np.array([0, 63], dtype=np.int64)
        any64 = rs.randint(0, 64, size=6, dtype=np.int64)
        for M in tiles:                              # first and last row and column of each of these tiles
            parts.append(_at(edge[:, None], M, any64[None, :], k).ravel())
            parts.append(_at(any64[:, None], M, edge[None, :], k).ravel())
            parts.append(_at(rs.randint(0, 64, size=4), M, rs.randint(0, 64, size=4), k))
    idx = np.unique(np.concatenate(parts))
    assert idx[0] >= 0 and idx[-1] < n
    return idx


def wide_values(rs, size, negative=True):
    """Values of 2^32 .. 2^62, some negative: sums, products and x + 1 wrap where NumPy's int64 wraps."""
    v = rs.randint(1 << 32, 1 << 62, size=size, dtype=np.int64)
    if negative:
        v[rs.rand(size) < 0.2] *= -1
    return v


def _values(rs, size, wide):
    """Non-zero values: Poisson counts + 1 and a few of 2^20 .. 2^24; wide: also negatives (-1 among them) and 2% of
    2^32 .. 2^62 (some negative)."""
    v = rs.poisson(3.0, size=size).astype(np.int64) + 1
    big = rs.rand(size) < 0.005
    v[big] = rs.randint(1 << 20, 1 << 24, size=int(big.sum()))
    if wide:
        neg = rs.rand(size) < 0.01
        v[neg] = -rs.randint(1, 50, size=int(neg.sum()))
        w = rs.rand(size) < 0.02
        v[w] = wide_values(rs, int(w.sum()))
    return v


def sparse_table(k, seed, n_random=10 ** 6, wide=True):
    """(idx, val): a structured sparse table, every val non-zero, idx sorted.  wide: with the extremes INT64_MAX (x + 1
    wraps) and INT64_MIN + 1, and values beyond 2^32 -- for the integer operations and the multiset; the distances with
    squares (euclidean, cosine) of such tables mostly wrap to NaN, so those take wide=False."""
    rs = np.random.RandomState(seed)
    idx = structured_indices(k, rs, n_random)
    val = _values(rs, idx.size, wide)
    if wide:
        val[idx.size // 3] = INT64_MAX
        val[idx.size // 3 + 1] = INT64_MIN + 1
    return idx, val


def sparse_pair(k, seed, n_random=10 ** 6, wide=True):
    """Two structured sparse tables that share about half of their supports; wide: with pairs whose (x + 1)(y + 1) wraps."""
    li, lv = sparse_table(k, seed, n_random, wide)
    rs = np.random.RandomState(seed + 1000)
    share = li[rs.rand(li.size) < 0.5]
    ri = np.unique(np.concatenate([share, structured_indices(k, rs, n_random // 2)]))
    rv = _values(rs, ri.size, wide)
    if wide:
        common = np.intersect1d(li, ri)[:64]         # (x + 1)(y + 1) = 2^80 + ... wraps
        lv[np.searchsorted(li, common)] = (1 << 40) + np.arange(common.size)
        rv[np.searchsorted(ri, common)] = (1 << 40) - np.arange(common.size)
    return li, lv, ri, rv


def dense(idx, val, n):
    out = np.zeros(n, dtype=np.int64)
    out[idx] = val
    return out


# -- operations on supports ----------------------------------------------------------------------------------------------
def value_at(idx, val, where):
    """val at each of `where` (0 off the support)."""
    pos = np.searchsorted(idx, where)
    pos = np.minimum(pos, idx.size - 1)
    hit = idx[pos] == where if idx.size else np.zeros(where.shape, dtype=bool)
    return np.where(hit, val[pos] if idx.size else 0, 0).astype(np.int64)


def union(li, lv, ri, rv):
    """(u, l, r): the union of two supports, sorted, with both tables' values there."""
    u = np.union1d(li, ri)
    return u, value_at(li, lv, u), value_at(ri, rv, u)


def balance(idx, val, k):
    """Profile.balance (klib.py:285-298) on a support: v[i] + v[rc(i)] (palindromes doubled), int64 wrapping."""
    u = np.union1d(idx, rc_index(idx, k))
    return u, value_at(idx, val, u) + value_at(idx, val, rc_index(u, k))


def positive(l, r):
    """metrics.positive (kpal_oracle_positive): left * bool(right), then right * bool(new left)."""
    l2 = np.where(r != 0, l, 0)
    return l2, np.where(l2 != 0, r, 0)


def _summary(q, summary):
    """summary4 of kpal_oracle.c on rows of four int64."""
    if summary == 'min':
        return q.min(axis=1).astype(np.float64)
    if summary == 'average':
        f = q.astype(np.float64)
        return (((0.0 + f[:, 0]) + f[:, 1]) + f[:, 2] + f[:, 3]) / 4.0
    t = np.sort(q, axis=1)
    return (t[:, 1].astype(np.float64) + t[:, 2].astype(np.float64)) / 2.0


def _group_sums(keys, *vals):
    """(unique keys, wrapping int64 sum of each val per key) for sorted keys."""
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    return (keys[starts],) + tuple(np.add.reduceat(v, starts) for v in vals)


def smooth(u, l, r, k, summary, threshold):
    """ProfileDistance.dynamic_smooth (kdistlib.py:53-124; dynamic_smooth_rec of kpal_oracle.c) over the prefix tree of a
    union support u.  A node of depth d (4^(k-d) bins) collapses when min(f(left quarters), f(right quarters)) <= threshold;
    every entry takes the decision of its shallowest collapsing ancestor: the node's sums go to its first bin, the rest is 0.
    Nodes outside the support hold zeros (summary 0 <= threshold >= 0) and stay zero."""
    assert threshold >= 0
    first = np.full(u.size, k)
    for d in range(k):
        quarter = u >> (2 * (k - d - 1))
        q, sl, sr = _group_sums(quarter, l, r)
        node = q >> 2
        nodes, inv = np.unique(node, return_inverse=True)
        ql = np.zeros((nodes.size, 4), dtype=np.int64)
        qr = np.zeros((nodes.size, 4), dtype=np.int64)
        ql[inv, q & 3] = sl
        qr[inv, q & 3] = sr
        collapse = np.minimum(_summary(ql, summary), _summary(qr, summary)) <= threshold
        here = collapse[np.searchsorted(nodes, u >> (2 * (k - d)))]
        first = np.where((first == k) & here, d, first)
    keep = first == k
    out_i, out_l, out_r = [u[keep]], [l[keep]], [r[keep]]
    for d in range(k):
        sel = first == d
        if sel.any():
            nodes, sl, sr = _group_sums(u[sel] >> (2 * (k - d)), l[sel], r[sel])
            out_i.append(nodes << (2 * (k - d)))
            out_l.append(sl)
            out_r.append(sr)
    i = np.concatenate(out_i)
    order = np.argsort(i, kind='stable')
    return i[order], np.concatenate(out_l)[order], np.concatenate(out_r)[order]


def scale(l, r, down=False):
    """metrics.get_scale / scale_down (kpal_oracle_profile_distance): the two factors, from wrapping int64 totals."""
    tl, tr = np.int64(l.sum()), np.int64(r.sum())
    ls, rs = 1.0, 1.0
    with np.errstate(divide='ignore', invalid='ignore'):
        if tl < tr:
            ls = float(np.float64(tr) / np.float64(tl))
        else:
            rs = float(np.float64(tl) / np.float64(tr))
        if down:
            top = max(ls, rs)
            ls, rs = ls / top, rs / top
    return ls, rs


def _seqsum(x):
    """Left-to-right float64 sum (the oracle's plain loops)."""
    return np.cumsum(x)[-1] if x.size else np.float64(0.0)


def metric(l, r, name, scaled=None):
    """The final metric of kpal_oracle_profile_distance on the values at a union support, in index order.  scaled: (ls, rs)
    or None.  IEEE float64 throughout: a wrapped negative dot gives NaN, a zero norm infinity, as in C."""
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        if scaled is None:
            if name in ('prod', 'sum'):
                return oracle.multiset(l, r, name)
            if name == 'euclidean':
                return oracle.euclidean(l, r)
            lr, ll, rr = (np.float64(np.dot(a, b)) for a, b in ((l, r), (l, l), (r, r)))     # int64, wrapping
            return float(lr / (np.sqrt(ll) * np.sqrt(rr)))
        fl, fr = l.astype(np.float64) * scaled[0], r.astype(np.float64) * scaled[1]
        if name in ('prod', 'sum'):
            return oracle.multiset(fl, fr, name)
        if name == 'euclidean':
            return float(np.sqrt(_seqsum((fl - fr) * (fl - fr))))
        return float(_seqsum(fl * fr) / (np.sqrt(_seqsum(fl * fl)) * np.sqrt(_seqsum(fr * fr))))


def profile_distance(li, lv, ri, rv, k, do_balance=False, do_positive=False, do_smooth=False, summary='min', threshold=0,
                     do_scale=False, down=False, metric_name='prod'):
    """oracle.profile_distance on two supports: balance through rc, positive, smoothing, scaling, then the metric."""
    if do_balance:
        li, lv = balance(li, lv, k)
        ri, rv = balance(ri, rv, k)
    u, l, r = union(li, lv, ri, rv)
    if do_positive:
        l, r = positive(l, r)
    if do_smooth:
        u, l, r = smooth(u, l, r, k, summary, threshold)
    return metric(l, r, metric_name, scale(l, r, down) if do_scale else None)


def merge(l, r, merger):
    """oracle.merge on the values at a union support (every merger maps (0, 0) to 0)."""
    return oracle.merge(l, r, merger)


def shrink(idx, val, factor):
    """Profile.shrink (klib.py:329-352) on a support: wrapping sums over idx >> 2 factor."""
    return _group_sums(np.asarray(idx) >> (2 * factor), np.asarray(val, dtype=np.int64))


def _select_key(x):
    return (int(x) ^ (1 << 63)) & ((1 << 64) - 1)


def _launches_of_select(mn, mx, v0, v1):
    """The radix-select launches of kpal_stats_device: select_hist once per byte from the highest one in which min and max
    differ, select_next when the upper middle element is a larger value than the lower one."""
    if mn == mx:
        return {}
    a, b = _select_key(mn), _select_key(mx)
    top = 7
    while (a >> (8 * top)) & 255 == (b >> (8 * top)) & 255:
        top -= 1
    out = {'select_hist': top + 1}
    if v1 != v0:
        out['select_next'] = 1
    return out


def stats_from_counts(counts, n):
    """oracle.stats from {value: how often} (Python ints; absent zeros are added) -> (stats dict, launches of the select)."""
    counts = {int(v): int(c) for v, c in counts.items() if c}
    have = sum(counts.values())
    assert have <= n
    if have < n:
        counts[0] = counts.get(0, 0) + (n - have)
    values = sorted(counts)
    total = sum(v * c for v, c in counts.items())
    wrapped = (total + (1 << 63)) % (1 << 64) - (1 << 63)
    mean = total / n
    sq = math.fsum(c * (v - mean) ** 2 for v, c in counts.items())
    r0, r1 = (n - 1) // 2, n // 2
    acc, v0, v1 = 0, None, None
    for v in values:
        acc += counts[v]
        if v0 is None and r0 < acc:
            v0 = v
        if v1 is None and r1 < acc:
            v1 = v
            break
    st = {'total': wrapped, 'non_zero': n - counts.get(0, 0), 'min': values[0], 'max': values[-1], 'mean': mean,
          'median': (float(v0) + float(v1)) / 2.0, 'std': math.sqrt(sq / n)}
    return st, _launches_of_select(values[0], values[-1], v0, v1)


def stats(idx, val, n):
    """oracle.stats of the table with support (idx, val) and zeros elsewhere."""
    vals, cnt = np.unique(val, return_counts=True)
    return stats_from_counts(dict(zip(vals.tolist(), cnt.tolist())), n)


# The option sets of the large-k rows: each option alone and combined, every metric, every summary, thresholds 0 / 1 / 2.5,
# scaling up and down, and do_balance with do_positive (the out-of-place balance, then positive in place).
OPTION_GRID = (
    dict(),
    dict(metric_name='sum', do_balance=True),
    dict(metric_name='euclidean', do_balance=True),
    dict(metric_name='cosine'),
    dict(do_positive=True),
    dict(metric_name='sum', do_balance=True, do_positive=True),
    dict(do_scale=True),
    dict(metric_name='sum', do_scale=True, down=True),
    dict(metric_name='euclidean', do_scale=True),
    dict(metric_name='cosine', do_scale=True, down=True),
    dict(do_smooth=True, summary='min', threshold=0),
    dict(metric_name='euclidean', do_smooth=True, summary='average', threshold=1),
    dict(metric_name='cosine', do_smooth=True, summary='median', threshold=2.5),
    dict(do_balance=True, do_positive=True, do_smooth=True, summary='median', threshold=1, do_scale=True, down=True),
    dict(metric_name='euclidean', do_balance=True, do_smooth=True, summary='average', threshold=2.5, do_scale=True),
)


def oracle_options(o):
    """An OPTION_GRID entry as keyword arguments of oracle.profile_distance."""
    o = dict(o)
    o['metric'] = o.pop('metric_name', 'prod')
    return o


# -- dense tables made in chunks -----------------------------------------------------------------------------------------
class DenseTable(object):
    """A full table of 4^k entries, 2^chunk_bits at a time: chunk c is ``values_c[base]`` for one fixed random pattern `base`
    of alphabet codes and a per-chunk permutation of the alphabet, then a few extreme values at per-chunk positions.  The
    count of every distinct value is exact (``counts``), so the summaries of the whole table follow without holding it."""
    ALPHABET = np.array([0, 1, 2, 3, 5, 8, 13, 40], dtype=np.int64)
    EXTREMES = np.array([(1 << 40) + 3, -7, (1 << 62) + 1, -(1 << 33), INT64_MAX, 1 << 32], dtype=np.int64)

    def __init__(self, k, seed, chunk_bits=24):
        self.k, self.n = k, 1 << (2 * k)
        self.chunk = 1 << min(chunk_bits, 2 * k)
        self.chunks = self.n // self.chunk
        self.seed = seed
        rs = np.random.RandomState(seed)
        self.base = rs.randint(0, self.ALPHABET.size, size=self.chunk).astype(np.uint8)
        self.base_counts = np.bincount(self.base, minlength=self.ALPHABET.size)

    def _plan(self, c):
        rs = np.random.RandomState([self.seed, c])
        values = self.ALPHABET[rs.permutation(self.ALPHABET.size)]
        at = np.unique(rs.randint(0, self.chunk, size=3))
        return values, at, self.EXTREMES[rs.randint(0, self.EXTREMES.size, size=at.size)]

    def get(self, c):
        values, at, ext = self._plan(c)
        out = values[self.base]
        out[at] = ext
        return out

    def counts(self):
        tally = {}
        for c in range(self.chunks):
            values, at, ext = self._plan(c)
            for v, m in zip(values.tolist(), self.base_counts.tolist()):
                tally[v] = tally.get(v, 0) + m
            for v in values[self.base[at]].tolist():
                tally[v] -= 1
            for v in ext.tolist():
                tally[v] = tally.get(v, 0) + 1
        return tally


def close(got, want, rtol):
    """got == want within rtol relative; the same NaN or infinity where want is one."""
    if np.isnan(want):
        return bool(np.isnan(got))
    if np.isinf(want):
        return got == want
    return got == want or abs(got - want) <= rtol * abs(want)
