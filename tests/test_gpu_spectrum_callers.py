"""The callers of the set spectrum (kpal_distribution_set_device): ``klib.distributions`` on profiles that are still in HBM and on
mixed lists, ``metrics.distribution`` on integer arrays, and ``kpal distr`` through ``kmer.main`` -- each against the reference's
``sorted(Counter(vector).items())`` (kpal/metrics.py:22-33, kpal/kmer.py:274-295), exactly.  Run on the GPU box: pytest -m gpu."""
import collections
import io
import random

import numpy as np
import pytest

import memh5

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


def counter_route(vector):
    return sorted(collections.Counter(vector).items())


def launches(ctx, call):
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        result = call()
        seen = dict((name, count) for name, (_, count) in ctx.prof_get().items() if count)
    finally:
        ctx.prof_enable(False)
    return result, seen


def fasta_text(rnd, n, k):
    """n short records, some shorter than k."""
    out = []
    for i in range(n):
        length = rnd.choice([0, 1, k - 1, k, k + 1, 30, 80, 200, 700])
        out.append('>rec%d some words\n%s\n' % (i, ''.join(rnd.choice('ACGTACGTN') for _ in range(length))))
    return ''.join(out).encode()


def same_pairs(got, want, what):
    """Equal pairs, Python ints, and the text the command prints."""
    assert got == want, what
    assert all(type(value) is int and type(number) is int for value, number in got), what
    assert ['{0} {1}'.format(*pair) for pair in got] == ['{0} {1}'.format(*pair) for pair in want], what


# ---- klib.distributions --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', (4, 6))
def test_distributions_of_profiles_in_hbm(ctx, k):
    """A dozen records fresh from from_fasta_by_record: counted where they lie, one set call per batch, still in HBM afterwards."""
    from kpal_amd import klib
    text = fasta_text(random.Random(k), 12, k)
    ps = list(klib.Profile.from_fasta_by_record(io.BytesIO(text), k))
    copies = list(klib.Profile.from_fasta_by_record(io.BytesIO(text), k))
    assert len(ps) == 12 and all(p._device_counts() is not None for p in ps)
    got, seen = launches(ctx, lambda: klib.distributions(ps))
    assert all(p._device_counts() is not None for p in ps)                           # nothing was downloaded
    assert seen.get('spectrum_hist') == 1 and seen.get('spectrum_compact') == 1, seen
    assert isinstance(got, list) and len(got) == 12
    for i, p in enumerate(copies):
        counts = np.array(p.counts)
        same_pairs(got[i], counter_route(counts), (k, i))
        assert sum(number for _, number in got[i]) == 4 ** k
    assert got == [[(int(v), n) for v, n in counter_route(np.array(p.counts))] for p in copies]


def test_distributions_of_a_mixed_list(ctx):
    """k = 3 and k = 5 host profiles, a scaled (float) one and device-resident ones, in one list: every answer at its place."""
    from kpal_amd import klib, metrics
    rs = np.random.RandomState(8)
    device = list(klib.Profile.from_fasta_by_record(io.BytesIO(fasta_text(random.Random(2), 12, 5)), 5))[3:6]
    k3 = [klib.Profile(rs.poisson(2.0, 4 ** 3).astype(np.int64), name='a%d' % i) for i in range(3)]
    k5 = [klib.Profile(rs.poisson(5.0, 4 ** 5).astype(np.int64), name='b%d' % i) for i in range(2)]
    k5[1].counts[7] = -(1 << 63)
    k5[1].counts[8] = (1 << 63) - 1
    scaled = klib.Profile(rs.poisson(5.0, 4 ** 3) * 0.37, name='scaled')
    mixed = [k3[0], k5[0], device[0], scaled, k3[1], device[2], k5[1], k3[2], device[1]]
    got = klib.distributions(mixed)
    assert all(p._device_counts() is not None for p in device)
    assert len(got) == len(mixed)
    for i, p in enumerate(mixed):
        counts = np.array(p.copy().counts)
        if p is scaled:
            assert got[i] == counter_route(counts) == metrics.distribution(counts) and isinstance(got[i][0][0], float)
        else:
            same_pairs(got[i], counter_route(counts), i)
    assert klib.distributions([]) == []
    assert klib.distributions(iter(k3)) == [counter_route(p.counts) for p in k3]


# ---- metrics.distribution ------------------------------------------------------------------------------------------------
def test_metrics_distribution_of_integer_arrays(ctx):
    from kpal_amd import metrics
    rs = np.random.RandomState(3)
    for vector in (rs.poisson(3.0, 4 ** 6).astype(np.int64),
                   rs.randint(-1000, 1000, size=1001).astype(np.int64),
                   np.array([-(1 << 63), (1 << 63) - 1, 0, -1, (1 << 63) - 1], dtype=np.int64),
                   rs.randint(-(1 << 31), 1 << 31, size=4 ** 4).astype(np.int32),
                   rs.poisson(1.0, 300).astype(np.int32),
                   rs.randint(0, 200, size=500).astype(np.uint8),
                   rs.randint(0, 2, size=4 ** 5).astype(bool),
                   np.zeros(7, dtype=bool)):
        got, seen = launches(ctx, lambda: metrics.distribution(vector))
        want = counter_route(vector)
        assert seen.get('spectrum_hist') == 1, (vector.dtype, seen)               # counted on the device
        assert got == want, vector.dtype
        assert ['{0} {1}'.format(*pair) for pair in got] == ['{0} {1}'.format(*pair) for pair in want], vector.dtype
        assert all(type(value) is type(expected) for (value, _), (expected, _) in zip(got, want)), vector.dtype
    # everything else keeps the reference's route: lists, float arrays, empty and two-dimensional arrays
    for vector in ([1, 1, 2], [], (3, 3, 1), np.array([0.5, 0.5, 2.0]), np.zeros(0, dtype=np.int64)):
        got, seen = launches(ctx, lambda: metrics.distribution(vector))
        assert got == counter_route(vector) and seen == {}
    assert metrics.distribution([1, 1, 2]) == [(1, 2), (2, 1)]


# ---- kpal distr ----------------------------------------------------------------------------------------------------------
def test_kpal_distr_prints_the_counter_lines(ctx, tmp_path, monkeypatch):
    """``kpal distr`` on a file of seven profiles of two lengths: the text of the Counter route, for all profiles and for -p
    names in an order of their own."""
    from kpal_amd import files, klib, kmer
    rs = np.random.RandomState(12)
    store = memh5.Store()
    monkeypatch.setattr(files, 'open_profile_file', store.open)
    monkeypatch.chdir(tmp_path)
    handle = files.ProfileFileType('w')('mixed.k')
    tables = {}
    for i, (name, k) in enumerate((('zeta', 4), ('alpha', 6), ('m_1', 4), ('beta', 6), ('m_2', 4), ('gamma', 4), ('delta', 6))):
        counts = rs.poisson((0.05, 3.0, 40.0)[i % 3], 4 ** k).astype(np.int64)
        if name == 'beta':
            counts[5] = 10 ** 13
        tables[name] = counts
        klib.Profile(counts, name=name).save(handle)

    def lines(names):
        return ''.join('\n'.join('{0} {1} {2}'.format(name, value, number) for value, number in counter_route(tables[name])) + '\n'
                       for name in names)

    for argv, names in ((['distr', 'mixed.k', 'all.txt'], sorted(tables)),
                        (['distr', 'mixed.k', 'some.txt', '-p', 'm_2', 'alpha', 'zeta', 'beta'], ['m_2', 'alpha', 'zeta', 'beta'])):
        _, seen = launches(ctx, lambda: kmer.main(argv))
        with open(argv[2]) as fh:
            assert fh.read() == lines(names), argv
        assert seen.get('spectrum_hist') == 2, seen                              # one set call per k-mer length, not one per profile
