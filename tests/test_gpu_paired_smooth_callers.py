"""The callers of kpal_paired_smooth_distance_device and kpal_paired_smooth_device on the GPU: kdistlib.paired_distances and
kdistlib.successive_distances with a smoothing ProfileDistance, ``kpal distance -m`` (kmer.distance), klib.smooth_profiles and
``kpal smooth`` (kmer.smooth).  Every expected distance is the loop of ``dist.distance`` over the pairs within the project's 1e-9
relative tolerance (unscaled euclidean bit for bit: an int64 sum either way); every expected table is what
``dist.dynamic_smooth`` leaves in copies, bit for bit.

Measured duration of this file on an MI355X: 0.8 s; the worst difference from the loop was 4.0e-16 relative (printed by the
tests under pytest -s).
"""
import io

import numpy as np
import pytest

import memh5
from test_gpu_paired_callers import assert_close as _assert_close, fasta_text, five_profiles, launched, loop

pytestmark = pytest.mark.gpu

K = 6
SET_LAUNCHES = {'smooth_set_level': K, 'smooth_set_codes': 1, 'pair_smooth': 1, 'reduce_partials': 1}
APPLY_LAUNCHES = {'smooth_set_level': K, 'smooth_set_codes': 1, 'pair_smooth_apply': 1}


WORST = [0.0]


def assert_close(got, want, what):
    _assert_close(got, want, what)
    got, want = np.asarray(got), np.asarray(want)
    if (want != 0).any():
        WORST[0] = max(WORST[0], float((np.abs(got - want)[want != 0] / np.abs(want[want != 0])).max()))
    print('%s: worst relative difference so far %.3g' % (what, WORST[0]))


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


def smoothing():
    from kpal_amd import kdistlib, metrics
    return {'min': kdistlib.ProfileDistance(do_smooth=True, threshold=0),
            'average scale balance': kdistlib.ProfileDistance(do_smooth=True, summary=metrics.summary['average'], threshold=1.5, do_scale=True, do_balance=True),
            'median euclidean': kdistlib.ProfileDistance(do_smooth=True, summary=metrics.summary['median'], threshold=1, distance_function=metrics.euclidean),
            'min cosine down': kdistlib.ProfileDistance(do_smooth=True, threshold=2, do_scale=True, down=True, distance_function=metrics.cosine_similarity)}


def windows_of(seed=5):
    from kpal_amd import klib
    out = list(klib.Profile.from_fasta_by_window(io.StringIO(fasta_text(seed, 2, 4000)), K, 900, 300))
    assert len(out) > 12 and all(p._device_counts() is not None for p in out)
    return out


def test_paired_and_successive_distances(ctx):
    from kpal_amd import kdistlib
    windows = windows_of()
    N = len(windows)
    half = N // 2
    left, right = windows[:half], windows[half:2 * half]
    for name, dist in smoothing().items():
        balance = {'balance_tiled_set': 2} if 'balance' in name else {}
        got, names = launched(ctx, lambda: kdistlib.paired_distances(left, right, dist))
        want = loop(dist, left, right)
        assert_close(got, want, name)
        assert names == dict(SET_LAUNCHES, **balance), (name, names)
        if name == 'median euclidean':
            assert np.array_equal(got, want)
        for lag in (1, 3):
            got, names = launched(ctx, lambda: kdistlib.successive_distances(windows, dist, lag=lag))
            want = loop(dist, windows[:N - lag], windows[lag:])
            assert got.shape == (N - lag,)
            assert_close(got, want, (name, lag))
            assert names == dict(SET_LAUNCHES, **({'balance_tiled_set': 1} if balance else {})), (name, lag, names)      # N tables, N pyramids
        assert all(p._device_counts() is not None for p in windows), name
    # positive + smoothing keeps the pair pipeline per pair
    positive = kdistlib.ProfileDistance(do_smooth=True, do_positive=True, threshold=1)
    got, names = launched(ctx, lambda: kdistlib.paired_distances(left, right, positive))
    assert names.get('smooth_apply') == half and 'pair_smooth' not in names, names
    assert_close(got, loop(positive, left, right), 'positive')


def test_kmer_distance_with_smoothing_prints_the_lines_of_the_loop(ctx):
    from kpal_amd import klib, kmer, kdistlib, metrics
    left, right = five_profiles('left.k', 41, [K] * 5), five_profiles('right.k', 42, [K] * 5)
    names = ['p%d' % i for i in range(5)]
    for kwargs, dist in ((dict(do_smooth=True, threshold=1), kdistlib.ProfileDistance(do_smooth=True, threshold=1)),
                         (dict(do_smooth=True, summary='average', threshold=2, do_scale=True, pairwise='sum'),
                          kdistlib.ProfileDistance(do_smooth=True, summary=metrics.summary['average'], threshold=2, do_scale=True, pairwise=metrics.pairwise['sum']))):
        want = loop(dist, [klib.Profile.from_file(left, name=n) for n in names], [klib.Profile.from_file(right, name=n) for n in names])
        scaled = want * 1e10   # (no value near a rounding boundary of the tenth decimal: the text cannot hinge on the last bits)
        assert np.all(np.abs(scaled - np.floor(scaled) - 0.5) > 1e-13 * np.maximum(scaled, 1.0))
        out = io.StringIO()
        _, seen = launched(ctx, lambda: kmer.distance(left, right, out, **kwargs))
        assert out.getvalue() == ''.join('%s %s %.10f\n' % (n, n, v) for n, v in zip(names, want))
        assert seen == SET_LAUNCHES, seen


def copies(profiles):
    from kpal_amd import klib
    return [klib.Profile(np.array(p.counts), name=p.name) for p in profiles]


def smoothed_by_loop(dist, left, right):
    left, right = copies(left), copies(right)
    for l, r in zip(left, right):
        dist.dynamic_smooth(l, r)
    return [p.counts for p in left], [p.counts for p in right]


def test_smooth_profiles(ctx):
    from kpal_amd import kdistlib, klib, metrics
    dists = (kdistlib.ProfileDistance(threshold=1), kdistlib.ProfileDistance(summary=metrics.summary['average'], threshold=1.5),
             kdistlib.ProfileDistance(summary=metrics.summary['median'], threshold=2))
    for dist in dists:
        # resident: rows of a new batch, the windows' own batches unchanged.  (Asking a window for its counts brings it to the
        # host for good: the expected tables come from a second, identical set of windows.)
        windows, twins = windows_of(), windows_of()
        half = len(windows) // 2
        left, right = windows[:half], windows[half:2 * half]
        batches = list({id(p._device[0]): p._device[0] for p in windows}.values())
        before = [np.empty((b.n_tables, 4 ** K), dtype=np.int64) for b in batches]
        for b, t in zip(batches, before):
            ctx.d2h(t, b.ptr)
        want_l, want_r = smoothed_by_loop(dist, twins[:half], twins[half:2 * half])
        _, names = launched(ctx, lambda: klib.smooth_profiles(left, right, dist))
        assert names == APPLY_LAUNCHES, names
        assert all(p._device_counts() is not None and not any(p._device[0] is b for b in batches) for p in left + right)
        for b, t in zip(batches, before):
            after = np.empty_like(t)
            ctx.d2h(after, b.ptr)
            assert np.array_equal(t, after)      # batch tables are never written
        for p, w in zip(left + right, want_l + want_r):
            assert p.length == K and np.array_equal(p.counts, w), p.name
        # host: written into the arrays the profiles hold
        windows = windows_of(seed=6)
        left, right = copies(windows[:half]), copies(windows[half:2 * half])
        arrays = [p.counts for p in left + right]
        want_l, want_r = smoothed_by_loop(dist, left, right)
        _, names = launched(ctx, lambda: klib.smooth_profiles(left, right, dist))
        assert names == APPLY_LAUNCHES, names
        for p, a, w in zip(left + right, arrays, want_l + want_r):
            assert p.counts is a and np.array_equal(a, w), p.name
        # mixed: resident left profiles, host right profiles
        windows, twins = windows_of(seed=7), windows_of(seed=7)
        left, right = windows[:half], copies(twins[half:2 * half])
        arrays = [p.counts for p in right]
        want_l, want_r = smoothed_by_loop(dist, twins[:half], right)
        _, names = launched(ctx, lambda: klib.smooth_profiles(left, right, dist))
        assert names == APPLY_LAUNCHES, names
        assert all(p._device_counts() is not None for p in left) and all(p.counts is a for p, a in zip(right, arrays))
        for p, w in zip(left + right, want_l + want_r):
            assert np.array_equal(p.counts, w), p.name


def test_smooth_profiles_errors_and_fallbacks(ctx):
    from kpal_amd import kdistlib, klib
    rs = np.random.RandomState(8)

    def profile(k, dtype=np.int64):
        return klib.Profile(rs.poisson(1.0, 4 ** k).astype(dtype), 'p')

    dist = kdistlib.ProfileDistance(threshold=1)
    a, b = [profile(4) for _ in range(3)], [profile(4) for _ in range(3)]
    for bad_l, bad_r in ((a, b[:2]), (a, [b[0], b[1], a[0]]), ([a[0], a[1], a[0]], b), (a, [b[0], b[0], b[2]])):
        with pytest.raises(ValueError):
            klib.smooth_profiles(bad_l, bad_r, dist)
    # a custom summary, a non-numeric threshold, other counts, mixed k: dist.dynamic_smooth pair by pair
    custom = kdistlib.ProfileDistance(summary=lambda q: np.min(q), threshold=1)
    mixed_l, mixed_r = [profile(4), profile(5), profile(4)], [profile(4), profile(5), profile(4)]
    floats_l, floats_r = [profile(4), profile(4, np.float64)], [profile(4), profile(4)]
    for what, l, r, d in (('custom summary', a, b, custom), ('mixed k', mixed_l, mixed_r, dist), ('float counts', floats_l, floats_r, dist)):
        want_l, want_r = smoothed_by_loop(d, l, r)
        _, names = launched(ctx, lambda: klib.smooth_profiles(l, r, d))
        assert (what == 'custom summary') == ('pair_smooth_apply' not in names), (what, names)
        for p, w in zip(l + r, want_l + want_r):
            assert np.array_equal(p.counts, w), what
    klib.smooth_profiles([], [], dist)


def test_kmer_smooth(ctx):
    from kpal_amd import klib, kmer, kdistlib, metrics
    names = ['p%d' % i for i in range(5)]
    for kwargs, dist in ((dict(threshold=1), kdistlib.ProfileDistance(threshold=1)),
                         (dict(summary='median', threshold=3), kdistlib.ProfileDistance(summary=metrics.summary['median'], threshold=3))):
        left, right = five_profiles('left.k', 41, [K] * 5), five_profiles('right.k', 42, [K] * 5)
        want_l, want_r = smoothed_by_loop(dist, [klib.Profile.from_file(left, name=n) for n in names], [klib.Profile.from_file(right, name=n) for n in names])
        out_l, out_r = memh5.File('out_left.k'), memh5.File('out_right.k')
        _, seen = launched(ctx, lambda: kmer.smooth(left, right, out_l, out_r, **kwargs))
        # (save() summarises every profile it writes: stats, stats_var and select_hist are its launches)
        assert {n: c for n, c in seen.items() if 'smooth' in n} == APPLY_LAUNCHES, seen
        for handle, want in ((out_l, want_l), (out_r, want_r)):
            assert sorted(handle['profiles'].keys()) == names
            for n, w in zip(names, want):
                got = handle['profiles/' + n][:]
                assert got.dtype == np.int64 and np.array_equal(got, w), n
        assert any(not np.array_equal(w, klib.Profile.from_file(left, name=n).counts) for n, w in zip(names, want_l))      # something collapsed
    # another k at pair 3: the two pairs before it are written, then the error
    left, odd = five_profiles('left.k', 41, [K] * 5), five_profiles('odd.k', 42, [K, K, 5, K, K])
    out_l, out_r = memh5.File('out_left.k'), memh5.File('out_right.k')
    with pytest.raises(ValueError) as err:
        kmer.smooth(left, odd, out_l, out_r, threshold=1)
    assert str(err.value) == kmer.LENGTH_ERROR
    assert sorted(out_l['profiles'].keys()) == names[:2] and sorted(out_r['profiles'].keys()) == names[:2]
    dist = kdistlib.ProfileDistance(threshold=1)
    want_l, want_r = smoothed_by_loop(dist, [klib.Profile.from_file(left, name=n) for n in names[:2]], [klib.Profile.from_file(odd, name=n) for n in names[:2]])
    for n, wl, wr in zip(names[:2], want_l, want_r):
        assert np.array_equal(out_l['profiles/' + n][:], wl) and np.array_equal(out_r['profiles/' + n][:], wr)
