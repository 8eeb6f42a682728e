"""The callers of kpal_paired_distance_device on the GPU: kdistlib.paired_distances, kdistlib.successive_distances and
``kpal distance`` (kmer.distance).  Every expected value is the loop of ``dist.distance`` over the pairs -- what those callers
replace -- within the project's 1e-9 relative tolerance, unscaled euclidean bit for bit (an int64 sum either way)."""
import io
import os

import numpy as np
import pytest

import memh5

pytestmark = pytest.mark.gpu

RTOL = 1e-9
RECORDS = 12


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


def launched(ctx, run):
    """(result of run(), {kernel: launches}) with the context's profiler on for just that call."""
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        out = run()
        got = {name: cnt for name, (_, cnt) in ctx.prof_get().items() if cnt}
    finally:
        ctx.prof_enable(False)
    return out, got


def fasta_text(seed, records, length):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(records):
        seq = ''.join(rs.choice(list('ACGT'), length + 100 * i, p=(0.2 + 0.02 * (i % 5), 0.3, 0.3 - 0.02 * (i % 5), 0.2)))
        out.append('>rec%02d\n' % i + '\n'.join(seq[j:j + 70] for j in range(0, len(seq), 70)) + '\n')
    return ''.join(out)


def loop(dist, left, right):
    return np.array([dist.distance(l, r) for l, r in zip(left, right)], dtype=np.float64)


def assert_close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    assert np.isfinite(want).all() and (np.abs(got - want) <= RTOL * np.abs(want)).all(), (what, got, want)


def distances():
    from kpal_amd import kdistlib, metrics
    return {'prod': kdistlib.ProfileDistance(), 'balance sum': kdistlib.ProfileDistance(do_balance=True, pairwise=metrics.pairwise['sum']),
            'scale down': kdistlib.ProfileDistance(do_scale=True, down=True),
            'positive scale cosine': kdistlib.ProfileDistance(do_positive=True, do_scale=True, distance_function=metrics.cosine_similarity),
            'smooth': kdistlib.ProfileDistance(do_smooth=True, summary=metrics.summary['average'], threshold=1.5),
            'euclidean': kdistlib.ProfileDistance(distance_function=metrics.euclidean)}


def test_resident_profiles_stay_resident(tmp_path, ctx):
    from kpal_amd import klib, kdistlib
    k = 6
    path = os.path.join(str(tmp_path), 'records.fa')
    with open(path, 'w') as fh:
        fh.write(fasta_text(11, RECORDS, 3000))
    with open(path) as fh:
        profs = list(klib.Profile.from_fasta_by_record(fh, k))
    assert len(profs) == RECORDS and all(p._device_counts() is not None for p in profs)
    left, right = profs[:6], profs[6:]
    for name, dist in distances().items():
        got, names = launched(ctx, lambda: kdistlib.paired_distances(left, right, dist))
        assert all(p._device_counts() is not None for p in profs), name
        want = loop(dist, left, right)
        assert_close(got, want, name)
        if name == 'euclidean':
            assert np.array_equal(got, want)
        if name != 'smooth':
            assert names.get('pair_set') == 1 and 'pair_distance' not in names and 'option_distance' not in names, (name, names)
    # scattered rows, and host copies of the tables on one side
    order_l, order_r = [4, 0, 9], [11, 5, 2]
    dist = distances()['scale down']
    got = kdistlib.paired_distances([profs[i] for i in order_l], [profs[i] for i in order_r], dist)
    assert_close(got, loop(dist, [profs[i] for i in order_l], [profs[i] for i in order_r]), 'scattered')
    host = [klib.Profile(np.array(p.counts), 'h') for p in right]
    assert_close(kdistlib.paired_distances(left, host, dist), loop(dist, left, right), 'host right side')
    # groups bounded by max_bytes: two pairs a group, the same values
    whole = kdistlib.paired_distances(left, host, dist)
    got, names = launched(ctx, lambda: kdistlib.paired_distances(left, host, dist, max_bytes=4 * 8 * 4 ** k))
    assert names.get('pair_set') == 3 and np.array_equal(got.view(np.uint64), whole.view(np.uint64)), names


def test_fallbacks_and_errors(ctx):
    from kpal_amd import klib, kdistlib
    rs = np.random.RandomState(3)

    def profile(k, dtype=np.int64):
        return klib.Profile(rs.poisson(3.0, 4 ** k).astype(dtype), 'p')

    dist = kdistlib.ProfileDistance(do_scale=True)
    a, b = [profile(4) for _ in range(3)], [profile(4) for _ in range(3)]
    with pytest.raises(ValueError):
        kdistlib.paired_distances(a, b[:2], dist)
    assert kdistlib.paired_distances([], [], dist).shape == (0,)
    # a single pair keeps the route and the bits of dist.distance
    got, names = launched(ctx, lambda: kdistlib.paired_distances(a[:1], b[:1], dist))
    assert 'pair_set' not in names and got.shape == (1,) and got[0] == dist.distance(a[0], b[0]), names
    # mixed k (pair by pair the lengths agree), float counts, a user's pairwise function: the loop
    mixed_l, mixed_r = [a[0], profile(5), a[2]], [b[0], profile(5), b[2]]
    floats_l = [a[0], profile(4, np.float64), a[2]]
    custom = kdistlib.ProfileDistance(pairwise=lambda x, y: abs(x - y) / (x + y + 2.0))
    for what, l, r, d in (('mixed k', mixed_l, mixed_r, dist), ('float counts', floats_l, b, dist), ('custom pairwise', a, b, custom)):
        got, names = launched(ctx, lambda: kdistlib.paired_distances(l, r, d))
        assert 'pair_set' not in names, (what, names)
        assert np.array_equal(got, loop(d, l, r)), what
    assert np.array_equal(kdistlib.successive_distances(a + b, custom, lag=2), loop(custom, (a + b)[:-2], (a + b)[2:]))


def test_successive_windows(ctx):
    from kpal_amd import klib, kdistlib
    k, W, S = 6, 900, 300
    windows = list(klib.Profile.from_fasta_by_window(io.StringIO(fasta_text(5, 2, 4000)), k, W, S))
    N = len(windows)
    assert N > 12 and all(p._device_counts() is not None for p in windows)
    for name, dist in distances().items():
        for lag in (1, 2):
            got, names = launched(ctx, lambda: kdistlib.successive_distances(windows, dist, lag=lag))
            want = loop(dist, windows[:N - lag], windows[lag:])
            assert got.shape == (N - lag,)
            assert_close(got, want, (name, lag))
            if name == 'euclidean':
                assert np.array_equal(got, want)
            if name == 'balance sum':
                assert names.get('balance_tiled_set') == 1 and names.get('pair_set') == 1, names      # N tables balanced once
    dist = distances()['prod']
    for lag in (0, -1, N, N + 3):
        with pytest.raises(ValueError):
            kdistlib.successive_distances(windows, dist, lag=lag)
    assert kdistlib.successive_distances(windows, dist, lag=N - 1).shape == (1,)


def five_profiles(name, seed, lengths):
    from kpal_amd import klib
    rs = np.random.RandomState(seed)
    handle = memh5.File(name)
    for i, k in enumerate(lengths):
        klib.Profile(rs.poisson((0.4, 3.0, 40.0)[i % 3], 4 ** k).astype(np.int64), name='p%d' % i).save(handle)
    return handle


def test_kmer_distance_prints_the_lines_of_the_loop(ctx):
    from kpal_amd import klib, kmer, kdistlib, metrics
    left, right = five_profiles('left.k', 41, [6] * 5), five_profiles('right.k', 42, [6] * 5)
    names = ['p%d' % i for i in range(5)]
    for kwargs, dist in ((dict(), kdistlib.ProfileDistance()),
                         (dict(do_scale=True, do_balance=True, pairwise='sum'), kdistlib.ProfileDistance(do_scale=True, do_balance=True, pairwise=metrics.pairwise['sum']))):
        want = loop(dist, [klib.Profile.from_file(left, name=n) for n in names], [klib.Profile.from_file(right, name=n) for n in names])
        scaled = want * 1e10   # (no value near a rounding boundary of the tenth decimal: the text cannot hinge on the last bits)
        assert np.all(np.abs(scaled - np.floor(scaled) - 0.5) > 1e-13 * np.maximum(scaled, 1.0))
        out = io.StringIO()
        _, seen = launched(ctx, lambda: kmer.distance(left, right, out, **kwargs))
        assert out.getvalue() == ''.join('%s %s %.10f\n' % (n, n, v) for n, v in zip(names, want))
        assert seen.get('pair_set') == 1 and 'pair_distance' not in seen, seen
    # another k at pair 3: the lines of the two pairs before it are written, then the error
    odd = five_profiles('odd.k', 42, [6, 6, 5, 6, 6])
    out = io.StringIO()
    with pytest.raises(ValueError) as err:
        kmer.distance(left, odd, out)
    assert str(err.value) == kmer.LENGTH_ERROR
    want = loop(kdistlib.ProfileDistance(), [klib.Profile.from_file(left, name=n) for n in names[:2]], [klib.Profile.from_file(odd, name=n) for n in names[:2]])
    assert out.getvalue() == ''.join('%s %s %.10f\n' % (n, n, v) for n, v in zip(names[:2], want))
