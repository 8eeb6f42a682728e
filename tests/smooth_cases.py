"""Shapes and inputs for the set-smoothing tests in which a workgroup walks more than one chunk
(tests/test_gpu_smooth_sets_trips.py, tests/test_smooth_plan_host.py) -- pure Python and NumPy, no GPU.

``trips(cu, k, Q, R, tri)`` restates, for a part of ``cu`` compute units, the grid rules the host launches a smoothed rectangle
(``tri``: the lower triangle of a set of Q against itself) with -- cross_staged, cross_grid and option_totals_gx of
kpal_amd/csrc/matrix_plan.hpp, smooth_stride and smooth_level_nodes of smooth_plan.hpp, and cross_smooth_core's rule that the
pyramid pass takes the kernel kind and the gx of the bins pass -- and says how many times the strided loops of the kernels go
round.  tests/test_smooth_plan_host.py holds it against the two plan programs, so that it cannot drift from the headers.

A trip count is a (fewest, most) pair over the walkers of a launch that have anything to do: the bin-groups of a staged
super-tile (chunks g, g + gx, ... of elements / 64), the threads of a register tile (elements i, i + gx * 256, ...), the threads
of smooth_set_level and smooth_set_codes (stride per * 256).  Walkers past the end of a short range -- the pyramid pass runs on
the grid of the three times longer bins, a level of few nodes leaves most of a workgroup idle -- make no trip and are not
counted: ``fewest`` is 1 there, never 0.

``codes_reference`` restates the definitions at the top of smooth_plan.hpp (node sums, flags, codes 0 / 1 / 2) in NumPy; it is
used to check INPUTS only (``inputs_ok``), never for an expected distance.
"""
import numpy as np

SUPER_BINS = 64          # matrix_plan.hpp: kSuperBins
BLOCK = 256              # threads of every kernel here
SUMMARIES = ('min', 'average', 'median')


# The shapes of tests/test_gpu_smooth_sets_trips.py and what a part of 256 compute units makes of them, written down from the
# rules: (k, Q, R, tri) -> route, units (super-tiles or 4 x 4 tiles), gx, and the (fewest, most) trips of the bins pass, the
# pyramid pass, smooth_set_level at height 0 and smooth_set_codes (None: not part of what the case is for).
TABLE_CU = 256
TABLE = {
    (8, 17, 33, False): dict(staged=True, units=6, gx=336, bins=(3, 4), pyramid=(1, 2), level0=(1, 2), codes=(2, 3)),
    (9, 5, 17, False): dict(staged=True, units=2, gx=1024, bins=(4, 4), pyramid=(1, 2), level0=(2, 3), codes=(3, 4)),
    (10, 5, 5, False): dict(staged=True, units=1, gx=2048, bins=(8, 8), pyramid=(2, 3), level0=(5, 6), codes=(6, 7)),
    (9, 18, 18, True): dict(staged=True, units=3, gx=680, bins=(6, 7), pyramid=(2, 3), level0=None, codes=None),
    (9, 1, 64, False): dict(staged=False, units=16, gx=256, bins=(4, 4), pyramid=(1, 2), level0=None, codes=None),
    (9, 3, 20, False): dict(staged=False, units=5, gx=819, bins=(1, 2), pyramid=(1, 1), level0=None, codes=None),
    (10, 2, 13, False): dict(staged=False, units=4, gx=1024, bins=(4, 4), pyramid=(1, 2), level0=None, codes=None),
}


def cross_staged(Q, R, n):
    return n >= 4096 and Q > 4 and R > 4


def cross_grid(cu, Q, R, n, tri, staged):
    """(units, gx) of matrix_plan.hpp's cross_grid: super-tiles or 4 x 4 tiles, workgroups per unit."""
    sideQ, sideR, superQ, superR = (Q + 3) // 4, (R + 3) // 4, (Q + 15) // 16, (R + 15) // 16
    ntiles = sideQ * (sideQ + 1) // 2 if tri else sideQ * sideR
    nsuper = superQ * (superQ + 1) // 2 if tri else superQ * superR
    if staged:
        gx = max(1, min(n // SUPER_BINS, max(1, cu * 8 // nsuper)))
        return nsuper, max(8, gx // 8 * 8)
    return ntiles, max(1, min((n + 255) // 256, max(1, cu * 16 // ntiles)))


def option_totals_gx(cu, nprof, n):
    return max(1, min((n + 255) // 256, max(1, cu * 8 // nprof)))


def smooth_level_nodes(k, h):
    return 4 ** (k - 1 - h)


def smooth_level_offset(k, h):
    return (4 ** k - 4 ** (k - h)) // 3


def smooth_nodes(k):
    return (4 ** k - 1) // 3


def smooth_stride(k):
    return (smooth_nodes(k) + SUPER_BINS - 1) // SUPER_BINS * SUPER_BINS


def _span(count, walkers):
    """(fewest, most) trips of the walkers u = 0 .. walkers - 1 that take items u, u + walkers, ... of `count`, over those
    that take any."""
    last = min(walkers, count) - 1
    return -(-(count - last) // walkers), -(-count // walkers)


def trips(cu, k, Q, R, tri=False):
    n = 4 ** k
    if tri:
        R = Q
    staged = cross_staged(Q, R, n)
    units, gx = cross_grid(cu, Q, R, n, tri, staged)
    stride = smooth_stride(k)
    nprof = Q if tri else Q + R
    if staged:
        bins, pyramid = _span(n // SUPER_BINS, gx), _span(stride // SUPER_BINS, gx)
    else:
        bins, pyramid = _span(n, gx * BLOCK), _span(stride, gx * BLOCK)
    levels = [_span(smooth_level_nodes(k, h), option_totals_gx(cu, nprof, smooth_level_nodes(k, h)) * BLOCK) for h in range(k)]
    codes = _span(stride, option_totals_gx(cu, nprof, stride) * BLOCK)
    # `first`: the elements every walker of a pass has seen after its first trip
    return dict(staged=staged, units=units, gx=gx, first=gx * (SUPER_BINS if staged else BLOCK), bins=bins, pyramid=pyramid,
                levels=levels, codes=codes)


def last_trip_chunk(count, walkers, walker=0):
    """The item of `count` that walker `walker` takes on its LAST trip, and which trip (0-based) that is."""
    assert walker < min(walkers, count)
    trip = (count - 1 - walker) // walkers
    return walker + trip * walkers, trip


# ---- the definitions of smooth_plan.hpp in NumPy ---------------------------------------------------------------------------
def _summarise(q, summary):
    """f(quarter sums) of an int64[nodes, 4] as NumPy evaluates it on an int64 array of four."""
    if summary == 'min':
        return q.min(axis=1).astype(np.float64)
    f = q.astype(np.float64)
    if summary == 'average':
        return (((f[:, 0] + f[:, 1]) + f[:, 2]) + f[:, 3]) / 4.0
    if summary == 'median':
        s = np.sort(q, axis=1).astype(np.float64)
        return (s[:, 1] + s[:, 2]) / 2.0
    raise ValueError(summary)


def codes_reference(table, k, summary, threshold):
    """One profile's pyramid by the definitions: per height h = 0 .. k - 1 the wrapping int64 ``sums`` of its 4^(k-1-h) nodes,
    their ``flags`` (f(quarter sums) <= threshold) and ``codes`` (1: flagged and no strict ancestor is; 2: a strict ancestor
    is flagged; 0: otherwise); ``pyramid``: the codes bottom height first, padded with 2 to smooth_stride(k); ``dead_bins``:
    whether a bin has a flagged node above it."""
    table = np.asarray(table, dtype=np.int64)
    assert table.shape == (4 ** k,)
    sums, flags = [], []
    below = table
    for h in range(k):
        q = below.reshape(-1, 4)
        with np.errstate(over='ignore'):
            sums.append(q.sum(axis=1, dtype=np.int64))              # wraps like ndarray.sum
        with np.errstate(invalid='ignore'):
            flags.append(_summarise(q, summary) <= threshold)
        below = sums[-1]
    codes = [None] * k
    above = np.zeros(1, dtype=bool)                                 # the root has no ancestor
    for h in range(k - 1, -1, -1):
        codes[h] = np.where(above, 2, flags[h].astype(np.uint8)).astype(np.uint8)
        above = np.repeat(above | flags[h], 4)                      # ... of the height below, then of the bins
    pyramid = np.full(smooth_stride(k), 2, dtype=np.uint8)
    for h in range(k):
        pyramid[smooth_level_offset(k, h):smooth_level_offset(k, h) + smooth_level_nodes(k, h)] = codes[h]
    return dict(sums=sums, flags=flags, codes=codes, pyramid=pyramid, dead_bins=above)


def inputs_ok(left, right, k, settings, first, pyramid_trips, tri=False):
    """AssertionError unless the two sets are inputs at which a wrong later trip shows.  ``first``: trips()['first'];
    ``pyramid_trips``: trips()['pyramid'].  For every (summary, threshold) of ``settings``, over the two sets:
      * nodes with code 1 occur at three or more heights;
      * no pair has all its bins live, and every pair has a live element (a bin or a node);
      * some pair has a live bin at or behind bin ``first``: the later trips of the bins pass carry terms;
      * some pair has a live node at or behind pyramid element ``first`` -- under every setting where every walker of the
        pyramid pass makes a second trip, under at least one setting where only some do (behind ``first`` lie then only the
        top heights, which the small thresholds never flag), not at all where the pyramid pass is one trip.
    What it cannot ask, with profiles of mean count 0.4 among them (test_gpu_cross_options.scale_sets): that no pair has all
    its bins dead.  Such a profile collapses in every height-0 node under an average threshold of 8, and an all-zero one at its
    root under every threshold >= 0; by the definition that kills every bin of every pair they are in, and the pair's distance
    is then the pyramid pass alone.  Those pairs are counted and returned, not refused.
    Returns {setting: dict(heights, pairs, all_dead, late_bins, late_nodes)}: pairs with all bins dead, with a late live bin,
    with a late live node."""
    left, right = np.asarray(left), np.asarray(right)
    report = {}
    for setting in settings:
        summary, threshold = setting
        refs = [[codes_reference(t, k, summary, threshold) for t in side] for side in ((left,) if tri else (left, right))]
        if tri:
            refs.append(refs[0])
        heights = sorted({h for side in refs for r in side for h in range(k) if (r['codes'][h] == 1).any()})
        assert len(heights) >= 3, (setting, 'code-1 nodes at heights', heights)
        pairs = all_dead = late_bins = late_nodes = 0
        for i, l in enumerate(refs[0]):
            for j, r in enumerate(refs[1]):
                if tri and j >= i:
                    continue
                live_bins = ~(l['dead_bins'] | r['dead_bins'])
                live_nodes = np.maximum(l['pyramid'], r['pyramid']) == 1
                assert not live_bins.all(), (setting, i, j, 'every bin is live')
                assert live_bins.any() or live_nodes.any(), (setting, i, j, 'no live element')
                pairs += 1
                all_dead += not live_bins.any()
                late_bins += bool(live_bins[first:].any())
                late_nodes += bool(live_nodes[first:].any())
        assert late_bins >= 1, (setting, 'no pair has a live bin behind the first trip')
        assert late_nodes >= 1 or pyramid_trips[0] < 2, (setting, 'no pair has a live node behind the first trip')
        report[setting] = dict(heights=heights, pairs=pairs, all_dead=all_dead, late_bins=late_bins, late_nodes=late_nodes)
    assert pyramid_trips[1] < 2 or any(r['late_nodes'] for r in report.values()), ('no setting has a live node behind the first trip', report)
    return report
