"""kpal_paired_smooth_distance[_device] and kpal_paired_smooth_device on the GPU: dynamic smoothing over the linked pairs of two
sets of profiles in a number of launches that does not grow with the number of pairs (kpal_amd/csrc/pair_smooth_plan.hpp,
pair_smooth_kernels.hpp, kpal_paired_smooth.hip).

Every expected distance is ``oracle.profile_distance`` on that pair under the contract of
test_gpu_paired.assert_matches_oracle: 1e-9 relative, exactly 0, the same NaN and the same infinity where the oracle gives one
(unscaled euclidean bit for bit).  Every expected table is ``oracle.dynamic_smooth`` on that pair, bit for bit.  Unscaled
euclidean and cosine are int64 sums and equal ``kpal_profile_distance_device`` bit for bit.

How the library decides: do_smooth without do_positive -> per chunk the set balance (do_balance), k x smooth_set_level and
smooth_set_codes over the distinct tables, ONE pair_smooth, ONE reduce_partials; k <= 6 the wave form (a unit is four pairs, a
wave adds a pair's bins and its pyramid), else a unit is one (pair, slice) item: the bin slices of 2^16 bins, then the node
slices of 2^16 pyramid elements -- k = 8 is 1 + 1, k = 9 is 4 + 2.  Without do_smooth, or with do_positive: the entry of
test_gpu_paired.py.

Measured duration of this file on an MI355X: 2.0 s (13 s when it is the first to import torch for the CU count); the worst
difference from the oracle over all cases was 1.7e-13 relative (printed by the tests under pytest -s).
"""
import ctypes
import os

import numpy as np
import pytest

import matrix_cases
import option_cases
import oracle
import smooth_cases
from test_gpu_cross_options import scale_sets
from test_gpu_paired import E_INVALID, GOLDEN_DIR, SUMMARY, assert_matches_oracle, exact_for, launched, on_device, options, oracle_pairs
from test_gpu_smooth_sets import option_sets, small_sets

pytestmark = pytest.mark.gpu

WORST = [0.0]


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


@pytest.fixture(scope='module')
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def opts(balance=False, scale=False, down=False, metric='prod', summary='min', threshold=0, positive=False, smooth=True):
    """test_gpu_smooth_sets' option names -> (kpal_distance_options, the oracle's keyword arguments)."""
    return options(do_balance=balance, do_positive=positive, do_scale=scale, down=down, metric=metric, do_smooth=smooth, summary=summary, threshold=threshold)


def check(got, want, kwargs, what):
    assert_matches_oracle(got, want, exact_for(kwargs), what)
    got, want = np.asarray(got), np.asarray(want)
    fin = np.isfinite(want) & (want != 0)
    if fin.any():
        WORST[0] = max(WORST[0], float((np.abs(got[fin] - want[fin]) / np.abs(want[fin])).max()))
        print('%s: worst relative difference so far %.3g' % (what, WORST[0]))


def smooth_device(ctx, k, N, dl, dr, native, chunk_pairs=0):
    return ctx.paired_smooth_distance_device(k, N, dl, dr, native, chunk_pairs)


def paired_smooth(ctx, left, right, k, native, chunk_pairs=0):
    left, right = np.asarray(left), np.asarray(right)
    with on_device(ctx, np.concatenate([left, right])) as dev:
        return smooth_device(ctx, k, left.shape[0], dev, dev + left.nbytes, native, chunk_pairs)


def apply_device(ctx, k, left, right, summary, threshold, lag=None, chunk_pairs=0):
    """The two smoothed sets of kpal_paired_smooth_device, and the launches.  lag: right = the left set `lag` tables on."""
    left = np.ascontiguousarray(left, dtype=np.int64)
    N = left.shape[0] - (lag or 0)
    data = left if lag is not None else np.concatenate([left, np.ascontiguousarray(right, dtype=np.int64)])
    table = 8 * 4 ** k
    with on_device(ctx, data) as dev, on_device(ctx, np.full((2 * N, 4 ** k), -7, dtype=np.int64)) as out:
        dr = dev + lag * table if lag is not None else dev + left.nbytes
        _, names = launched(ctx, lambda: ctx.paired_smooth_device(k, N, dev, dr, SUMMARY[summary], threshold, out, out + N * table, chunk_pairs))
        res, after = np.empty((2 * N, 4 ** k), dtype=np.int64), np.empty_like(data)
        ctx.d2h(res, out)
        ctx.d2h(after, dev)
    np.testing.assert_array_equal(after, data)      # the inputs are never written
    return res[:N], res[N:], names


def check_apply(ctx, k, left, right, summary, threshold, what, lag=None):
    got_l, got_r, names = apply_device(ctx, k, left, right, summary, threshold, lag)
    pairs = zip(left[:len(left) - lag], left[lag:]) if lag is not None else zip(left, right)
    for i, (l, r) in enumerate(pairs):
        wl, wr = oracle.dynamic_smooth(l, r, k, summary, threshold)
        np.testing.assert_array_equal(got_l[i], wl, err_msg=str((what, 'left', i)))
        np.testing.assert_array_equal(got_r[i], wr, err_msg=str((what, 'right', i)))
    assert names == {'smooth_set_level': k, 'smooth_set_codes': 1, 'pair_smooth_apply': 1}, names


def sets_of(k, N):
    if k >= 6:      # (scale_sets needs four profiles a side: a single pair is the first pair of four)
        left, right = scale_sets(k, max(N, 4), max(N, 4))
        return left[:N], right[:N]
    return small_sets(k, N, N, seed=10 * k + N)


SHAPES = [(1, 5), (1, 1), (2, 5), (3, 5), (3, 1), (6, 1), (6, 4), (6, 5), (6, 65), (7, 5), (8, 4), (9, 5)]


@pytest.mark.parametrize('k,N', SHAPES, ids=lambda v: str(v))
def test_shapes(ctx, k, N):
    """k <= 3: pyramids of 1, 5 and 21 nodes behind 63, 59 and 43 dead elements; k = 6: the wave form, N = 5 and 65 leave a ragged
    last unit; k = 7: the slice form, one bin slice and one node slice; k = 8: exactly one bin slice; k = 9: four bin slices
    and two node slices."""
    left, right = sets_of(k, N)
    with on_device(ctx, np.concatenate([left, right])) as dev:
        for o in option_sets(k):
            native, kwargs = opts(**o)
            got, names = launched(ctx, lambda: smooth_device(ctx, k, N, dev, dev + left.nbytes, native))
            check(got, oracle_pairs(left, right, k, kwargs), kwargs, ('shapes', k, N, o))
            want = {'smooth_set_level': k, 'smooth_set_codes': 1, 'pair_smooth': 1, 'reduce_partials': 1}
            assert {n: c for n, c in names.items() if not n.startswith('balance')} == want, names
    for i, o in enumerate(option_sets(k)[:3]):      # one setting per summary
        check_apply(ctx, k, left, right, o.get('summary', 'min'), o.get('threshold', 0), ('apply', k, N, o))
    if N >= 5:
        o = option_sets(k)[1]
        check_apply(ctx, k, left, None, o['summary'], o['threshold'], ('apply, lag 1', k, N), lag=1)


def test_host_entry(ctx):
    k, N = 6, 5
    left, right = sets_of(k, N)
    for o in option_sets(k):
        native, kwargs = opts(**o)
        dev = paired_smooth(ctx, left, right, k, native)
        host = ctx.paired_smooth_distance(list(left), list(right), k, native)
        assert np.array_equal(host.view(np.uint64), dev.view(np.uint64)), o


def test_k9_inputs_make_the_late_slices_matter(ctx):
    """k = 9, N = 5: pairs 1 and 2 have live bins in the last bin slice and live nodes in the second node slice under the small
    thresholds, with code-1 nodes at heights 0 and 1; under (median, 40) and (average, 30) no bin is live and the distance is
    the pyramid alone.  (smooth_cases.codes_reference is used for the inputs only.  On these inputs: 436 .. 8092 live bins in the
    last bin slice -- the fewest under (average, 8) -- and 183 .. 3140 live nodes in the second node slice.)"""
    k, N = 9, 5
    left, right = sets_of(k, N)
    last_bins = slice(3 << 16, 4 << 16)
    for summary, threshold in (('min', 0), ('average', 8), ('min', 3), ('median', 6)):
        for p in (1, 2):
            l, r = (smooth_cases.codes_reference(t, k, summary, threshold) for t in (left[p], right[p]))
            assert (~(l['dead_bins'] | r['dead_bins']))[last_bins].sum() >= 400, (summary, threshold, p)
            assert (np.maximum(l['pyramid'], r['pyramid'])[1 << 16:] == 1).sum() >= 150, (summary, threshold, p)
            assert all((np.maximum(l['codes'][h], r['codes'][h]) == 1).any() for h in (0, 1)), (summary, threshold, p)
    for summary, threshold in (('median', 40), ('average', 30)):
        for p in range(N):
            l, r = (smooth_cases.codes_reference(t, k, summary, threshold) for t in (left[p], right[p]))
            assert (l['dead_bins'] | r['dead_bins']).all(), (summary, threshold, p)


def test_one_late_element_decides(ctx):
    """Two tables at k = 9 that collapse everywhere but for (a) one live bin of the last bin slice, (b) one live node of height
    1 (the second node slice): the whole distance sits there."""
    k = 9
    n = 4 ** k
    # (a) 'min' <= 0: a node with a zero quarter collapses.  All bins zero on both sides but one count in the first bin of each of
    # the four children of every ancestor of bin `at`: no ancestor of `at` is flagged, every other node is flagged or lies under
    # a flagged one.  The two tables differ in bin `at` alone, by 9.
    at = n - 5
    left = np.zeros(n, dtype=np.int64)
    for h in range(k):
        node = at >> (2 * (h + 1))
        for q in range(4):
            left[((node << 2) + q) << (2 * h)] += 3
    right = left.copy()
    left[at] += 9
    l, r = (smooth_cases.codes_reference(t, k, 'min', 0) for t in (left, right))
    live = np.flatnonzero(~(l['dead_bins'] | r['dead_bins']))
    assert list(live) == [n - 8, n - 7, n - 6, n - 5] and at >= 3 << 16      # the last height-0 node but one: the last bin slice
    for metric in ('euclidean', 'prod', 'cosine'):
        native, kwargs = opts(metric=metric)
        got = paired_smooth(ctx, left[None], right[None], k, native)
        check(got, oracle_pairs(left[None], right[None], k, kwargs), kwargs, ('late bin', metric))
        if metric == 'euclidean':
            assert got[0] == 9.0
    check_apply(ctx, k, left[None], right[None], 'min', 0, 'late bin, apply')
    # (b) 'min' <= 5 on tables of ones: the quarters of a node of height 0, 1, 2 are 1, 4, 16 -- every node of heights 0 and 1 is
    # flagged, none above: the live elements are the height-1 nodes, no bin is live.  The tables differ in one bin of a late
    # height-1 node, by 1: the two sums are 17 and 16.
    left, right = np.ones(n, dtype=np.int64), np.ones(n, dtype=np.int64)
    node1 = 4 ** (k - 2) - 3
    left[node1 * 16 + 5] = 2
    summary, threshold = 'min', 5
    l, r = (smooth_cases.codes_reference(t, k, summary, threshold) for t in (left, right))
    code = np.maximum(l['pyramid'], r['pyramid'])
    assert (l['dead_bins'] | r['dead_bins']).all()      # no live bin: the pyramid alone
    live_nodes = np.flatnonzero(code == 1)
    assert live_nodes[0] == 1 << 16 and live_nodes.size == 4 ** (k - 2) and live_nodes[-1] == (1 << 16) + 4 ** (k - 2) - 1      # height 1: the second node slice
    for metric in ('euclidean', 'sum'):
        native, kwargs = opts(metric=metric, summary=summary, threshold=threshold)
        got = paired_smooth(ctx, left[None], right[None], k, native)
        check(got, oracle_pairs(left[None], right[None], k, kwargs), kwargs, ('late node', metric))
        if metric == 'euclidean':
            assert got[0] == 1.0
    check_apply(ctx, k, left[None], right[None], summary, threshold, 'late node, apply')


def test_more_units_than_the_persistent_grid(ctx, num_cu):
    """k = 4, the wave form: two rounds and three units over, a last unit of one pair; equal pairs, equal bits."""
    k, distinct = 4, 61
    slots = 8 * num_cu
    units = 2 * slots + 3
    N = 4 * (units - 1) + 1
    base_l, base_r = small_sets(k, distinct, distinct, seed=5)
    pick = np.arange(N) % distinct
    left, right = base_l[pick], base_r[pick]
    with on_device(ctx, np.concatenate([left, right])) as dev:
        for o in (dict(threshold=1), dict(summary='average', threshold=1.5, scale=True, balance=True, metric='sum'), dict(summary='median', threshold=2, metric='cosine')):
            native, kwargs = opts(**o)
            got, names = launched(ctx, lambda: smooth_device(ctx, k, N, dev, dev + left.nbytes, native))
            assert names.get('pair_smooth') == 1 and names.get('smooth_set_level') == k, names
            check(got, oracle_pairs(base_l, base_r, k, kwargs)[pick], kwargs, ('persistent grid', o))
            assert np.array_equal(got.view(np.uint64), got[:distinct][pick].view(np.uint64)), o


def test_edges(ctx):
    """option_cases.edge_cases(6) left against right as linked pairs, with collapse_none and the zero-total variant, at every
    summary's tie thresholds and 0, -0.25, +inf, 1e300, NaN, under the eight metric and scale variants of
    test_gpu_smooth_sets.test_edge_cases_meet_each_other."""
    k = 6
    cases = option_cases.edge_cases(k)
    cases.append(option_cases.build('collapse_none', k))
    cases.append(option_cases.build('negative', k, variant='zero_total'))
    left, right = np.stack([c.left for c in cases]), np.stack([c.right for c in cases])
    variants = (dict(metric='prod'), dict(metric='sum', scale=True), dict(metric='euclidean'), dict(metric='cosine', scale=True, down=True),
                dict(metric='prod', scale=True, down=True), dict(metric='sum'), dict(metric='euclidean', scale=True), dict(metric='cosine'))
    at = 0
    with on_device(ctx, np.concatenate([left, right])) as dev:
        for summary in option_cases.SUMMARIES:
            for threshold in option_cases.TIE_THRESHOLDS[summary] + (0, -0.25, float('inf'), 1e300, float('nan')):
                for o in variants[at % 2::2]:
                    native, kwargs = opts(summary=summary, threshold=threshold, **o)
                    with np.errstate(all='ignore'):
                        got = smooth_device(ctx, k, len(cases), dev, dev + left.nbytes, native)
                    check(got, oracle_pairs(left, right, k, kwargs), kwargs, ('edges', summary, threshold, o))
                at += 1


def test_apply_edges(ctx):
    """Wrapping sums (big_sums), a root that collapses ([sum, 0, ...]), nothing that collapses."""
    k = 6
    for kind in ('big_sums', 'collapse_root', 'collapse_none', 'collapse_each_level'):
        case = option_cases.build(kind, k)
        for summary, threshold in option_cases.smooth_settings(case):
            check_apply(ctx, k, case.left[None], case.right[None], summary, threshold, (kind, summary, threshold))
    case = option_cases.build('collapse_root', k)
    got_l, got_r, _ = apply_device(ctx, k, case.left[None], case.right[None], case.summary, case.threshold)
    with np.errstate(over='ignore'):
        assert got_l[0, 0] == case.left.sum() and not got_l[0, 1:].any() and got_r[0, 0] == case.right.sum() and not got_r[0, 1:].any()


def test_reference_goldens(ctx):
    """The G13 records of k = 4, stacked as one set: every distance the reference recorded with do_smooth and without
    do_positive, and every smoothed pair of tables it recorded."""
    k = 4
    goldens = [g for g in option_cases.load_golden(GOLDEN_DIR) if g.k == k]
    assert len(goldens) >= 9
    left, right = np.stack([g.left for g in goldens]), np.stack([g.right for g in goldens])
    recorded = {}
    for i, g in enumerate(goldens):
        for kwargs, value in g.distances:
            if kwargs.get('do_smooth') and not kwargs.get('do_positive'):
                recorded.setdefault(tuple(sorted(kwargs.items())), []).append((i, value))
    compared = 0
    with on_device(ctx, np.concatenate([left, right])) as dev:
        for key, values in sorted(recorded.items(), key=repr):
            native, kwargs = options(**dict(key))
            with np.errstate(all='ignore'):
                got = smooth_device(ctx, k, len(goldens), dev, dev + left.nbytes, native)
            at = [i for i, _ in values]
            assert_matches_oracle(got[at], np.array([v for _, v in values]), False, dict(key))
            compared += len(at)
    assert compared >= 9 * 12, compared
    tables = 0
    for g in goldens:
        for summary, threshold, want_l, want_r in g.smoothed:
            got_l, got_r, _ = apply_device(ctx, k, g.left[None], g.right[None], summary, threshold)
            np.testing.assert_array_equal(got_l[0], want_l, err_msg=g.name)
            np.testing.assert_array_equal(got_r[0], want_r, err_msg=g.name)
            tables += 1
    assert tables >= 9


@pytest.mark.parametrize('k,N', [(6, 9), (9, 3)])
def test_int64_sums_are_the_pair_entry_bit_for_bit(ctx, k, N):
    left, right = sets_of(k, N)
    table = 8 * 4 ** k
    with on_device(ctx, np.concatenate([left, right])) as dev:
        for metric in ('euclidean', 'cosine'):
            for o in (dict(), dict(summary='average', threshold=8, balance=True), dict(summary='median', threshold=40), dict(summary='median', threshold=6)):
                native, _ = opts(metric=metric, **o)
                got = smooth_device(ctx, k, N, dev, dev + left.nbytes, native)
                pairs = np.array([ctx.profile_distance_device(k, dev + i * table, dev + left.nbytes + i * table, native) for i in range(N)])
                assert np.array_equal(got.view(np.uint64), pairs.view(np.uint64)), (k, metric, o)


@pytest.mark.parametrize('k,N', [(6, 23), (9, 9)])
def test_a_pair_does_not_depend_on_its_set(ctx, k, N):
    """The bits of pair i: in the whole set, alone, at another position (the set reversed), and under chunk_pairs 1 and 7."""
    left, right = sets_of(k, N)
    table = 8 * 4 ** k
    with on_device(ctx, np.concatenate([left, right, left[::-1], right[::-1]])) as dev:
        dl, dr, rl, rr = (dev + i * left.nbytes for i in range(4))
        for o in option_sets(k)[:4]:
            native, _ = opts(**o)
            whole = smooth_device(ctx, k, N, dl, dr, native).view(np.uint64)
            for i in (0, 3, N // 2, N - 1):
                alone = smooth_device(ctx, k, 1, dl + i * table, dr + i * table, native).view(np.uint64)
                assert alone[0] == whole[i], (k, o, i)
            assert np.array_equal(smooth_device(ctx, k, N, rl, rr, native).view(np.uint64), whole[::-1]), (k, o)
            for chunk in (1, 7):
                got, names = launched(ctx, lambda: smooth_device(ctx, k, N, dl, dr, native, chunk))
                assert np.array_equal(got.view(np.uint64), whole), (k, o, chunk)
                assert names.get('pair_smooth') == -(-N // chunk) and names.get('smooth_set_codes') == -(-N // chunk), (chunk, names)


def test_aliasing(ctx):
    """A set against itself: zeros, NaN where the pair entry gives NaN.  Lag +-1 and +-3 against the oracle, with and without the
    balance -- the same bits as the two sides apart; ranges half a table apart; the inputs are not written."""
    k, N = 6, 12
    prof = scale_sets(k, N, 8)[0]
    prof[N - 2] = 0
    table = 8 * 4 ** k
    with on_device(ctx, np.concatenate([prof, prof])) as dev:
        for o in option_sets(k):
            native, kwargs = opts(**o)
            got = smooth_device(ctx, k, N, dev, dev, native)
            with np.errstate(all='ignore'):
                old = ctx.paired_distance_device(k, N, dev, dev, native)
            want = oracle_pairs(prof, prof, k, kwargs)
            if kwargs['metric'] != 'cosine':
                assert ((got == 0) | np.isnan(old)).all() and (np.isnan(got) == np.isnan(old)).all(), o
            check(got, want, kwargs, ('self', o))
            for lag in (1, 3):
                want = oracle_pairs(prof[:N - lag], prof[lag:], k, kwargs)
                fwd = smooth_device(ctx, k, N - lag, dev, dev + lag * table, native)
                check(fwd, want, kwargs, (lag, o))
                check(smooth_device(ctx, k, N - lag, dev + lag * table, dev, native), want, kwargs, (-lag, o))
                apart = smooth_device(ctx, k, N - lag, dev, dev + (N + lag) * table, native)      # the second copy: two sides
                assert np.array_equal(fwd.view(np.uint64), apart.view(np.uint64)), (lag, o)
        rows = np.concatenate([prof, prof[:1]]).reshape(-1)
        half = 4 ** k // 2
        shifted = rows[half:half + (N - 1) * 4 ** k].reshape(N - 1, 4 ** k)
        for o in (dict(balance=True, scale=True, threshold=3), dict(summary='average', threshold=8, metric='euclidean')):
            native, kwargs = opts(**o)
            got = smooth_device(ctx, k, N - 1, dev, dev + table // 2, native)
            check(got, oracle_pairs(prof[:N - 1], shifted, k, kwargs), kwargs, ('half a table', o))
        after = np.empty((2 * N, 4 ** k), dtype=np.int64)
        ctx.d2h(after, dev)
    np.testing.assert_array_equal(after, np.concatenate([prof, prof]))


def test_launches_do_not_grow_with_the_set(ctx):
    k = 6
    table = 8 * 4 ** k
    base = {'smooth_set_level': k, 'smooth_set_codes': 1, 'pair_smooth': 1, 'reduce_partials': 1}
    for N in (5, 300):
        left, right = scale_sets(k, N, N) if N < 100 else [matrix_cases.build('plain', k, 2 * N, seed=9).profiles[i * N:(i + 1) * N] for i in (0, 1)]
        with on_device(ctx, np.concatenate([left, right])) as dev:
            for o, extra in ((dict(threshold=3), {}), (dict(summary='average', threshold=8, scale=True, metric='cosine'), {}),
                             (dict(summary='median', threshold=6, balance=True, metric='sum'), {'balance_tiled_set': 2})):
                native, _ = opts(**o)
                _, names = launched(ctx, lambda: smooth_device(ctx, k, N, dev, dev + left.nbytes, native))
                assert names == dict(base, **extra), (N, o, names)
            # under a lag the union of the two ranges: still k level launches, one balance
            native, _ = opts(threshold=3, balance=True, scale=True)
            _, names = launched(ctx, lambda: smooth_device(ctx, k, N - 1, dev, dev + table, native))
            assert names == dict(base, balance_tiled_set=1), names
            _, names = launched(ctx, lambda: smooth_device(ctx, k, N, dev, dev, native))
            assert names == dict(base, balance_tiled_set=1), names
            # do_positive: the launches and the bits of the old entry
            native, _ = opts(threshold=3, positive=True, scale=True)
            M = min(N, 5)
            got, names = launched(ctx, lambda: smooth_device(ctx, k, M, dev, dev + left.nbytes, native))
            old, names_old = launched(ctx, lambda: ctx.paired_distance_device(k, M, dev, dev + left.nbytes, native))
            assert names == names_old and names.get('smooth_apply') == M and 'pair_smooth' not in names, names
            assert np.array_equal(got.view(np.uint64), old.view(np.uint64))
            # without do_smooth: the old entry
            native, _ = opts(smooth=False, scale=True)
            got, names = launched(ctx, lambda: smooth_device(ctx, k, N, dev, dev + left.nbytes, native))
            assert names == {'pair_set_totals': 1, 'pair_set': 1, 'reduce_partials': 2}, names
            assert np.array_equal(got.view(np.uint64), ctx.paired_distance_device(k, N, dev, dev + left.nbytes, native).view(np.uint64))


def test_arguments(ctx):
    """Every refusal of kpal_paired_distance_device with the same text; the refusals of the apply entry; nothing is launched
    and nothing written."""
    from kpal_amd import _native
    k, N = 2, 3
    L, h = ctx._L, ctx._h
    host = [np.ascontiguousarray(np.arange(16, dtype=np.int64) + i) for i in range(2 * N)]
    out = np.full(N, -12345.5)
    outp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def opt(**kw):
        o = _native.DistanceOptions(0, 0, 1, 0, 0.0, 0, 0, 0)
        for name, v in kw.items():
            setattr(o, name, v)
        return ctypes.byref(o)

    def ptrs(rows, null_at=None):
        return (ctypes.c_void_p * N)(*[None if i == null_at else host[r].ctypes.data for i, r in enumerate(rows)])

    with on_device(ctx, np.concatenate(host + [host[0]])) as dev, on_device(ctx, np.full((2 * N + 1, 16), -7, dtype=np.int64)) as res:
        right = dev + N * 128
        both = {}
        for name in ('kpal_paired_smooth_distance_device', 'kpal_paired_distance_device'):
            fn = getattr(L, name)
            both[name] = lambda k_=k, n=N, l=dev, r=right, o='default', chunk=0, res_=outp, fn=fn: fn(h, k_, n, l, r, opt() if o == 'default' else o, chunk, res_)
        hostcall = lambda k_=k, n=N, l=None, r=None, o=None, res_=outp: L.kpal_paired_smooth_distance(
            h, k_, n, l if l is not None else ptrs(range(N)), r if r is not None else ptrs(range(N, 2 * N)), o if o is not None else opt(), res_)
        device_cases = [dict(n=0), dict(n=-4), dict(k_=0), dict(k_=17), dict(l=None), dict(r=None), dict(res_=None), dict(l=dev + 8), dict(r=right + 8),
                        dict(o=None), dict(o=opt(metric=4)), dict(o=opt(summary=3)), dict(chunk=-1), dict(k_=16, n=1 << 40)]
        texts = []
        for kw in device_cases:
            got = []
            for name in ('kpal_paired_distance_device', 'kpal_paired_smooth_distance_device'):
                rc, names = launched(ctx, lambda: both[name](**kw))
                assert rc == E_INVALID and names == {}, (name, kw, rc, names)
                got.append(L.kpal_last_error().decode())
            assert got[0] == got[1] and got[0], (kw, got)
            texts.append(got[0])
        assert texts[0] == 'N must be >= 1' and texts[7] == 'device tables must be 16-byte aligned' and texts[11] == 'unknown summary function 3', texts
        for call, text in ((lambda: hostcall(n=0), 'N must be >= 1'), (lambda: hostcall(k_=17), 'k=17 out of range'),
                           (lambda: L.kpal_paired_smooth_distance(h, k, N, None, ptrs(range(N)), opt(), outp), 'NULL pointer'),
                           (lambda: hostcall(o=opt(metric=-1)), 'unknown metric -1'),
                           (lambda: hostcall(l=ptrs(range(N), null_at=1)), 'left profile 1 is NULL'), (lambda: hostcall(r=ptrs(range(N), null_at=2)), 'right profile 2 is NULL'),
                           (lambda: hostcall(k_=16, n=1 << 29), '536870912 pairs at k=16: too many bytes')):
            rc, names = launched(ctx, call)
            assert rc == E_INVALID and L.kpal_last_error().decode() == text and names == {}, (rc, text, L.kpal_last_error().decode())
        assert (out == -12345.5).all()
        assert both['kpal_paired_smooth_distance_device']() == 0 and hostcall() == 0
        # the apply entry
        ol, orr = res, res + N * 128
        apply = lambda k_=k, n=N, l=dev, r=right, s=0, t=1.0, chunk=0, a=ol, b=orr: L.kpal_paired_smooth_device(h, k_, n, l, r, s, t, chunk, a, b)
        for kw, text in ((dict(n=0), 'N must be >= 1'), (dict(k_=17), 'k=17 out of range'), (dict(l=None), 'NULL pointer'), (dict(a=None), 'NULL pointer'),
                         (dict(b=None), 'NULL pointer'), (dict(l=dev + 8), 'device tables must be 16-byte aligned'), (dict(s=3), 'unknown summary function 3'),
                         (dict(s=-1), 'unknown summary function -1'), (dict(chunk=-1), 'chunk_pairs must be >= 0'),
                         (dict(a=ol + 8), 'output tables must be 16-byte aligned'), (dict(b=orr + 8), 'output tables must be 16-byte aligned'),
                         (dict(b=ol), 'output tables overlap each other or the inputs'), (dict(b=orr - 128), 'output tables overlap each other or the inputs'),
                         (dict(a=dev), 'output tables overlap each other or the inputs'), (dict(b=right + 2 * 128), 'output tables overlap each other or the inputs')):
            rc, names = launched(ctx, lambda: apply(**kw))
            assert rc == E_INVALID and L.kpal_last_error().decode() == text and names == {}, (kw, rc, L.kpal_last_error().decode(), names)
        after = np.empty((2 * N + 1, 16), dtype=np.int64)
        ctx.d2h(after, res)
        assert (after == -7).all()      # nothing written by a refusal
        assert apply() == 0
