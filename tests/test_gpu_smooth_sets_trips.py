"""Dynamic smoothing over whole rectangles and triangles (kpal_cross_smooth_distance_device, kpal_smooth_distance_matrix_device)
at shapes where a workgroup walks MORE THAN ONE chunk: the `more` branch of cross_super_kernel with its second staged stream
(nextc, put_code(cur ^ 1, ...), the flip of cur), the second trip of cross_tile_kernel's bin loop, and the strides of
smooth_set_level and smooth_set_codes over a pyramid longer than the grid.  tests/test_gpu_smooth_sets.py covers the one-trip
shapes at k <= 7; this file k = 8 .. 10, and k = 4 and 5, which nothing ran before.

Every expected value is ``oracle.profile_distance(l, r, k, **options)`` on that pair, by the contract of
test_gpu_cross_options.assert_close: relative 1e-9; where the oracle is not finite the result is non-finite of the same kind;
an exact 0 of the oracle is an exact 0.  One exception: at k = 8, 17 x 33 the oracle runs on one pair of every 4 x 4 tile (45
of 561) and the whole rectangle is held against the per-pair entry, ctx.cross_profile_distance_device (1e-9 everywhere, bit
for bit for unscaled euclidean and cosine).  smooth_cases.codes_reference checks inputs only.

Each case first asserts smooth_cases.trips() for the compute units of the part it runs on -- a change of a grid rule, or
another part, fails there instead of quietly running one trip.  At 256 compute units (smooth_cases.TABLE; fewest - most trips
over the walkers of a launch):

    case                     route                             bins pass   pyramid pass   level h = 0 / codes
    k = 8, 17 x 33           staged, 6 super-tiles, gx 336     3 - 4       1 - 2          1 - 2 / 2 - 3
    k = 9, 5 x 17            staged, 2 super-tiles, gx 1024    4           1 - 2          2 - 3 / 3 - 4
    k = 10, 5 x 5            staged, 1 super-tile, gx 2048     8           2 - 3          5 - 6 / 6 - 7
    k = 9, triangle P = 18   staged, 3 super-tiles, gx 680     6 - 7       2 - 3
    k = 9, 1 x 64            tiles, 16 tiles, gx 256           4           1 - 2
    k = 9, 3 x 20            tiles, 5 tiles, gx 819            1 - 2       1
    k = 10, 2 x 13           tiles, 4 tiles, gx 1024           4           1 - 2
    k = 9, 7 x 7 (edges)     staged, 1 super-tile, gx 2048     2           1

test_one_late_chunk_decides plants the whole distance of a pair in the elements a walker reaches on its LAST trip: 64 (staged)
or 256 (tiles) bins, or one node.  Height 0 of a k = 9 pyramid is its first 65536 elements, which is exactly the first trip
of both routes, so the node is one of height 1, the lowest height a second trip of the pyramid pass reaches.

Measured duration of this file on an MI355X: 23 s run alone -- 10.5 s in the tests, the rest the first test's fixtures (the
context, and torch's query of the device); the worst difference from the oracle over all cases was 1.8e-11 relative (the
planted edge cases under scale + down; 3.9e-13 outside them).

Checked once by hand, not part of the suite: with `put_code(cur, ...)` in place of `put_code(cur ^ 1, ...)` inside
`if (more)`, and with nextc read at `ch` in place of `ch + blk.ngroups`, tests/test_gpu_smooth_sets.py stays green and eleven
tests of this file fail -- every staged case with a second bin trip.
"""
import numpy as np
import pytest

import option_cases
import oracle
import smooth_cases
from test_gpu_cross_options import PER_PAIR_KERNELS, _lower, assert_close, launched, options, oracle_rect, scale_sets
from test_gpu_smooth_sets import SET_KERNELS, SETTINGS, Tables, option_sets, small_sets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


@pytest.fixture(scope='module')
def cu():
    """Compute units of the part: the device property kpal_ctx sizes its grids with."""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def need_trips(cu, k, Q, R, tri=False, bins=None, pyramid=None, codes=None):
    """trips() of the shape, after asserting its precondition: 'every' -- every walker makes a second trip; 'some' -- some do."""
    t = smooth_cases.trips(cu, k, Q, R, tri)
    for name, want in (('bins', bins), ('pyramid', pyramid), ('codes', codes)):
        if want is not None:
            assert t[name][0 if want == 'every' else 1] >= 2, (name, want, cu, k, Q, R, tri, t)
    return t


def sets(k, Q, R):
    """scale_sets(k, Q, R); a left side of fewer than the three profiles scale_sets plants its pairs in is cut from one of three."""
    left, right = scale_sets(k, max(Q, 3), R)
    return left[:Q], right


def setting_of(o):
    return (o.get('summary', 'min'), o.get('threshold', 0))


def structure(names, k, staged):
    """k levels, the codes, two rectangle passes, one reduction, nothing per pair (one balance per profile apart)."""
    assert not set(names) & set(PER_PAIR_KERNELS), names
    want = {'smooth_set_level': k, 'smooth_set_codes': 1, 'smooth_set_super' if staged else 'smooth_set_tile': 2, 'reduce_partials': 1}
    assert {n: c for n, c in names.items() if not n.startswith('balance')} == want, names


def oracle_lower(prof, k, kwargs):
    with np.errstate(all='ignore'):
        return np.array([oracle.profile_distance(prof[i], prof[j], k, **kwargs) for i in range(1, len(prof)) for j in range(i)], dtype=np.float64)


def integer_form(o):
    return not o.get('scale') and o.get('metric') in ('euclidean', 'cosine')


# which of option_sets(6) a case runs: between them every metric, scale, scale + down, balance, both unscaled integer forms
#   0 prod, min 0            1 prod, average 8, scale, balance     2 cosine, median 40
#   3 sum, min 3, scale + down, balance      4 euclidean, average 30      5 cosine, median 6, scale
RECTANGLES = [(8, 17, 33, (2, 3, 4), dict(bins='every', pyramid='some', codes='every')),
              (9, 5, 17, (0, 1, 5), dict(bins='every', pyramid='some', codes='every')),
              (10, 5, 5, (0, 3), dict(bins='every', pyramid='every', codes='every')),
              (9, 1, 64, (0, 5), dict(bins='every', pyramid='some')),
              (9, 3, 20, (2, 3), dict(bins='some')),
              (10, 2, 13, (1, 4), dict(bins='every', pyramid='some'))]


def test_option_sets_cover():
    used = [option_sets(6)[i] for _, _, _, which, _ in RECTANGLES for i in which] + [option_sets(6)[i] for i in TRIANGLE_SETS]
    assert {o.get('metric', 'prod') for o in used} == {'prod', 'sum', 'euclidean', 'cosine'}
    assert any(o.get('scale') and not o.get('down') for o in used) and any(o.get('scale') and o.get('down') for o in used)
    assert any(o.get('balance') for o in used) and any(integer_form(o) for o in used)
    assert {setting_of(o) for o in used} == {(s['summary'], s['threshold']) for s in SETTINGS}


@pytest.mark.parametrize('k,Q,R,which,need', RECTANGLES, ids=['k%d_%dx%d' % c[:3] for c in RECTANGLES])
def test_rectangle(ctx, cu, k, Q, R, which, need):
    t = need_trips(cu, k, Q, R, **need)
    left, right = sets(k, Q, R)
    chosen = [option_sets(6)[i] for i in which]
    report = smooth_cases.inputs_ok(left, right, k, [setting_of(o) for o in chosen], t['first'], t['pyramid'])
    print('k = %d, %d x %d: %s; inputs %s' % (k, Q, R, t, report))
    if (k, Q, R) == (8, 17, 33):
        # the oracle on one pair of every 4 x 4 tile; the whole rectangle against the pair pipeline below
        pairs = [(min(4 * ti + (ti + tj) % 4, Q - 1), min(4 * tj + (2 * ti + tj) % 4, R - 1)) for ti in range((Q + 3) // 4) for tj in range((R + 3) // 4)]
        assert {(q // 4, r // 4) for q, r in pairs} == {(ti, tj) for ti in range(5) for tj in range(9)} and len(pairs) == 45
    with Tables(ctx, left) as dl, Tables(ctx, right) as dr:
        for o in chosen:
            native, kwargs = options(smooth=True, **o)
            got, names = launched(ctx, lambda: ctx.cross_smooth_distance_device(k, Q, dl.ptr, R, dr.ptr, native))
            structure(names, k, t['staged'])
            assert got.shape == (Q, R)
            if (k, Q, R) == (8, 17, 33):
                with np.errstate(all='ignore'):
                    want = np.array([oracle.profile_distance(left[q], right[r], k, **kwargs) for q, r in pairs])
                assert_close(np.array([got[q, r] for q, r in pairs]), want, ('rectangle, a pair of every tile', k, Q, R, o))
                old, names = launched(ctx, lambda: ctx.cross_profile_distance_device(k, Q, dl.ptr, R, dr.ptr, native))
                assert names.get('smooth_apply') == Q * R, names
                assert_close(got, old, ('rectangle against the pair pipeline', k, Q, R, o))
                if integer_form(o):
                    np.testing.assert_array_equal(got, old, err_msg=str(o))
            else:
                assert_close(got, oracle_rect(left, right, k, kwargs), ('rectangle', k, Q, R, o))
            if (k, Q, R) == (9, 5, 17):
                again = ctx.cross_smooth_distance_device(k, Q, dl.ptr, R, dr.ptr, native)
                assert got.tobytes() == again.tobytes(), o
        assert np.array_equal(dl.read(), left) and np.array_equal(dr.read(), right)


TRIANGLE_SETS = (4, 1)


def test_triangle(ctx, cu):
    """k = 9, P = 18: three super-tiles, two on the diagonal, six to seven bin trips -- the oracle, the rectangle of the set
    with itself below the diagonal, and bit for bit on the integer forms."""
    k, P = 9, 18
    t = need_trips(cu, k, P, P, tri=True, bins='every', pyramid='every')
    assert t['staged']
    prof = scale_sets(k, P, 8)[0]
    chosen = [option_sets(6)[i] for i in TRIANGLE_SETS]
    report = smooth_cases.inputs_ok(prof, prof, k, [setting_of(o) for o in chosen], t['first'], t['pyramid'], tri=True)
    print('k = %d, triangle of %d: %s; inputs %s' % (k, P, t, report))
    with Tables(ctx, prof) as dp:
        for o in chosen:
            native, kwargs = options(smooth=True, **o)
            tri, names = launched(ctx, lambda: ctx.smooth_distance_matrix_device(P, k, dp.ptr, native))
            structure(names, k, True)
            square = ctx.cross_smooth_distance_device(k, P, dp.ptr, P, dp.ptr, native)
            assert_close(tri, oracle_lower(prof, k, kwargs), ('triangle', k, P, o))
            assert_close(tri, _lower(square), ('triangle against the rectangle', k, P, o))
            if integer_form(o):
                np.testing.assert_array_equal(tri, _lower(square), err_msg=str(o))
        assert np.array_equal(dp.read(), prof)


# ---- one late chunk decides the distance -------------------------------------------------------------------------------------
BLOCK = 256     # bins zeroed at a time below: a height-3 node, four staged chunks, one trip of one tile workgroup


def late_sets(k, Q, R, setting, variant, t):
    """Left: Q profiles of counts 20 .. 59 in which every second-of-four block of 256 bins is zero (dead under both settings,
    and under ('min', 0) everything that shares a height-4 node with one), except around the TARGET, whose height-4 node is
    dense, so that the target is live.  Right: copies of the left profiles; two in three differ from their original in the target alone.
      'bins'     the target is the run of bins one walker (a staged bin-group: 64; a tile workgroup: 256) takes on its last
                 trip of the bins pass; the copies add 0 .. 4 to its counts
      'node'     the target is one height-1 node whose pyramid element a walker takes on its last trip of the pyramid pass;
                 its 16 bins sit one count above the setting's threshold in the left profiles and on it in the changed copies,
                 so its flag flips and the pair's live elements are that node alone
    The run the same walker took one trip EARLIER is dead in every pair: codes left over from it would drop the target.
    Returns (left, right, changed right profiles, target slice of bins, earlier slice of elements of that pass)."""
    n, staged, gx = 4 ** k, t['staged'], t['gx']
    rs = np.random.RandomState(1000 * Q + R + (variant == 'node'))
    left = rs.randint(20, 60, (Q, n)).astype(np.int64)
    blocks = left.reshape(Q, n // BLOCK, BLOCK)
    blocks[:, 1::4] = 0
    width = smooth_cases.SUPER_BINS if staged else BLOCK
    if variant == 'bins':
        walker = 5 * gx // 8 + 3
        item, trip = smooth_cases.last_trip_chunk(n // width, gx, walker)
        assert trip == t['bins'][1] - 1 >= 1, (trip, t)
        target = slice(item * width, (item + 1) * width)
        earlier = slice((item - gx) * width, (item - gx + 1) * width)
        dead_bins = earlier
    else:
        stride = smooth_cases.smooth_stride(k)
        if staged:
            walker = (stride // width - gx) // 2                     # a bin-group that has a second chunk of the pyramids
            item, trip = smooth_cases.last_trip_chunk(stride // width, gx, walker)
            element = item * width + 7
            earlier = slice((item - gx) * width, (item - gx + 1) * width)
        else:
            thread = (stride - gx * BLOCK) // 2 // BLOCK * BLOCK + 7     # ... a thread that has a second element
            element, trip = smooth_cases.last_trip_chunk(stride, gx * BLOCK, thread)
            earlier = slice((thread // BLOCK) * BLOCK, (thread // BLOCK + 1) * BLOCK)
        assert trip == t['pyramid'][1] - 1 >= 1, (trip, t)
        node = element - smooth_cases.smooth_level_offset(k, 1)
        assert 0 <= node < smooth_cases.smooth_level_nodes(k, 1), 'the second trip starts in height 1'
        assert earlier.stop <= smooth_cases.smooth_level_nodes(k, 0), 'the first trip lies in height 0'
        target = slice(16 * node, 16 * node + 16)
        dead_bins = slice(4 * earlier.start, 4 * earlier.stop)      # the bins under those height-0 nodes
    top = target.start // (4 * BLOCK) * (4 * BLOCK)
    assert dead_bins.stop <= top or dead_bins.start >= top + 4 * BLOCK
    left[:, top:top + 4 * BLOCK] = rs.randint(20, 60, (Q, 4 * BLOCK))
    left[:, dead_bins] = 0
    if variant == 'node':
        if setting == ('min', 0):           # quarter sums 1, 8, 8, 8: min 1 > 0; the copy's first height-0 node sums to 0
            left[:, target] = [1, 0, 0, 0] + [2] * 12
            change = np.array([-1] + [0] * 15)
        else:                               # ('average', 8): quarter sums 9, 8, 8, 8: 8.25 > 8; the copy's are 8 each: a tie
            assert setting == ('average', 8)
            left[:, target] = [3] + [2] * 15
            change = np.array([-1] + [0] * 15)
    right = np.stack([left[j % Q] for j in range(R)])
    changed = [j for j in range(R) if j % 3]
    for j in changed:
        right[j, target] += ((np.arange(target.stop - target.start) * (j % 4 + 1)) % 5) if variant == 'bins' else change
        assert not np.array_equal(right[j], left[j % Q])
    return left, right, changed, target, earlier


@pytest.mark.parametrize('setting', [('min', 0), ('average', 8)], ids=['min_0', 'average_8'])
@pytest.mark.parametrize('variant', ['bins', 'node'])
@pytest.mark.parametrize('Q,R', [(5, 17), (1, 64)], ids=['5x17_staged', '1x64_tiles'])
def test_one_late_chunk_decides(ctx, cu, Q, R, variant, setting):
    """Unscaled euclidean between a profile and its copy comes from the changed elements alone: a 1e-9 check of a sum over
    262144 bins cannot see one chunk; here the chunk is the sum."""
    k = 9
    t = need_trips(cu, k, Q, R, bins='every', pyramid='some')
    assert t['staged'] == (Q > 4)
    left, right, changed, target, earlier = late_sets(k, Q, R, setting, variant, t)
    # the inputs are what the docstring of late_sets says, by the definitions
    refs = {}
    for j in sorted({0, changed[0], changed[-1]}):
        l, r = (refs.setdefault(key, smooth_cases.codes_reference(v, k, *setting)) for key, v in ((('l', j % Q), left[j % Q]), (('r', j), right[j])))
        live_bins = ~(l['dead_bins'] | r['dead_bins'])
        live_nodes = np.maximum(l['pyramid'], r['pyramid']) == 1
        differ = np.flatnonzero(left[j % Q] != right[j])
        if variant == 'bins':
            assert live_bins[target].all() and not live_bins[earlier].any(), (j, setting)
            assert (differ.size > 0) == (j in changed) and ((differ >= target.start) & (differ < target.stop)).all()
        else:
            element = smooth_cases.smooth_level_offset(k, 1) + target.start // 16
            assert not live_nodes[earlier].any() and not (j in changed and live_bins[target].any()), (j, setting)
            assert bool(live_nodes[element]) == (j in changed) and (l['pyramid'][element], r['pyramid'][element]) == (0, 1 if j in changed else 0), (j, setting)
            assert l['sums'][1][target.start // 16] - r['sums'][1][target.start // 16] == (1 if j in changed else 0)
    native, kwargs = options(smooth=True, metric='euclidean', summary=setting[0], threshold=setting[1])
    want = oracle_rect(left, right, k, kwargs)
    same = np.array([[j % Q == i and j not in changed for j in range(R)] for i in range(Q)])
    assert (want[same] == 0).all() and same.sum() == len(range(0, R, 3)) and (want[~same] > 0).all()
    if variant == 'node':
        assert all(want[j % Q, j] == 1.0 for j in changed), 'the flipped node alone: sums one apart'
    else:
        d = (right[changed[0], target] - left[changed[0] % Q, target]).astype(np.float64)
        assert want[changed[0] % Q, changed[0]] == np.sqrt((d * d).sum()), 'the target bins alone'
    with Tables(ctx, left) as dl, Tables(ctx, right) as dr:
        got, names = launched(ctx, lambda: ctx.cross_smooth_distance_device(k, Q, dl.ptr, R, dr.ptr, native))
        structure(names, k, t['staged'])
        assert_close(got, want, ('late chunk', Q, R, variant, setting))
        assert (got[same] == 0).all()
        for j in changed:                               # the square root of one small exact integer in both
            assert got[j % Q, j] == want[j % Q, j], (j, got[j % Q, j], want[j % Q, j])
        assert np.array_equal(dl.read(), left) and np.array_equal(dr.read(), right)


# ---- k = 4 and 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,Q,R', [(4, 5, 7), (4, 17, 33), (5, 5, 7), (5, 17, 33), (5, 1, 1)], ids=lambda v: str(v))
def test_small_k_rectangle(ctx, cu, k, Q, R):
    """Pyramids of 85 and 341 nodes, padded to 128 and 384: 43 dead elements behind the root at both k.  Always register
    tiles: 4 (of which 5 x 7 masks three rows and one column), 45 and 1."""
    t = smooth_cases.trips(cu, k, Q, R)
    assert not t['staged'] and t['units'] == ((Q + 3) // 4) * ((R + 3) // 4)
    assert smooth_cases.smooth_stride(k) - smooth_cases.smooth_nodes(k) == 43
    left, right = small_sets(k, Q, R, seed=10 * k + Q)
    with Tables(ctx, left) as dl, Tables(ctx, right) as dr:
        for o in option_sets(k):
            native, kwargs = options(smooth=True, **o)
            got, names = launched(ctx, lambda: ctx.cross_smooth_distance_device(k, Q, dl.ptr, R, dr.ptr, native))
            structure(names, k, False)
            assert_close(got, oracle_rect(left, right, k, kwargs), ('small k', k, Q, R, o))
        assert np.array_equal(dl.read(), left) and np.array_equal(dr.read(), right)


def test_small_k_triangle(ctx):
    k, P = 5, 18
    prof = small_sets(k, P, 1, seed=77)[0]
    with Tables(ctx, prof) as dp:
        for o in option_sets(k):
            native, kwargs = options(smooth=True, **o)
            tri, names = launched(ctx, lambda: ctx.smooth_distance_matrix_device(P, k, dp.ptr, native))
            structure(names, k, False)
            square = ctx.cross_smooth_distance_device(k, P, dp.ptr, P, dp.ptr, native)
            assert_close(tri, oracle_lower(prof, k, kwargs), ('small k triangle', P, o))
            assert_close(tri, _lower(square), ('small k triangle against the rectangle', P, o))
            if integer_form(o):
                np.testing.assert_array_equal(tri, _lower(square), err_msg=str(o))
        assert np.array_equal(dp.read(), prof)


def test_small_k_settings_flag_something():
    """The k < 6 option sets on small_sets tables: under most some bins die and some live (the average threshold of
    2.25 * 4^(k-1) collapses every profile at its root), and between them nodes with code 1 occur at three or more heights."""
    for k in (4, 5):
        left, right = small_sets(k, 17, 33, seed=10 * k + 17)
        heights, mixed = set(), 0
        for o in option_sets(k):
            refs = [smooth_cases.codes_reference(v, k, *setting_of(o)) for v in list(left) + list(right)]
            heights |= {h for r in refs for h in range(k) if (r['codes'][h] == 1).any()}
            dead = np.mean([r['dead_bins'].mean() for r in refs])
            mixed += 0.02 < dead < 0.98
        assert len(heights) >= 3 and mixed >= 4, (k, heights, mixed)


# ---- edge cases at a k with several trips --------------------------------------------------------------------------------------
EDGE_VARIANTS = (dict(metric='prod'), dict(metric='sum', scale=True), dict(metric='euclidean'), dict(metric='cosine', scale=True, down=True),
                 dict(metric='prod', scale=True, down=True), dict(metric='sum'), dict(metric='euclidean', scale=True), dict(metric='cosine'))
EDGE_TIES = {'min': 3, 'average': 2.25, 'median': 3}      # option_cases.TIE_THRESHOLDS; median 3 is the tie of the planted tie_median case


@pytest.fixture(scope='module')
def edge_sets():
    """One case each of collapse_root, collapse_each_level, big_sums, negative and a tie in a level's last node -- the kinds of
    option_cases.edge_cases, whose own list stops at the ties past k = 8 -- and collapse_none and negative's zero_total."""
    k = 9
    last = [c for c in option_cases.edge_cases(k) if c.kind.startswith('tie_') and c.args.get('last')]
    cases = [option_cases.build('collapse_root', k), option_cases.build('collapse_each_level', k), option_cases.build('big_sums', k),
             option_cases.build('negative', k, variant='neg_total'), last[0],
             option_cases.build('collapse_none', k), option_cases.build('negative', k, variant='zero_total')]
    assert [c.kind for c in cases] == ['collapse_root', 'collapse_each_level', 'big_sums', 'negative', 'tie_median', 'collapse_none', 'negative']
    assert last[0].label['tie'] == 4 ** last[0].label['level'] - 1 and last[0].threshold == EDGE_TIES['median']
    return k, np.stack([c.left for c in cases]), np.stack([c.right for c in cases])


@pytest.mark.parametrize('summary', option_cases.SUMMARIES)
def test_edge_cases_meet_each_other(ctx, cu, edge_sets, summary):
    """Left vectors against right vectors, every kind against every other, at the summary's tie threshold (two option sets), at
    0 and at NaN: four calls of 49 pairs per summary, the eight option variants of the k = 6 test in turn (its two groups
    alternate).  Seven profiles a side are staged in one super-tile whose bin-groups make two trips."""
    k, left, right = edge_sets
    P = len(left)
    t = need_trips(cu, k, P, P, bins='every')
    assert t['staged'] and P > 4
    at = 4 * option_cases.SUMMARIES.index(summary)
    with Tables(ctx, left) as dl, Tables(ctx, right) as dr:
        for threshold in (EDGE_TIES[summary], EDGE_TIES[summary], 0, float('nan')):
            o = EDGE_VARIANTS[at % len(EDGE_VARIANTS)]
            at += 1
            native, kwargs = options(smooth=True, summary=summary, threshold=threshold, **o)
            with np.errstate(all='ignore'):
                got, names = launched(ctx, lambda: ctx.cross_smooth_distance_device(k, P, dl.ptr, P, dr.ptr, native))
            structure(names, k, True)
            assert_close(got, oracle_rect(left, right, k, kwargs), ('edges', summary, threshold, o))
        assert np.array_equal(dl.read(), left) and np.array_equal(dr.read(), right)
