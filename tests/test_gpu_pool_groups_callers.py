"""The callers of the pool by label (kpal_pool_groups_device): ``klib.pooled_by`` on profiles that are still in HBM and on host
profiles, ``kdistlib.pooled_nearest`` on the reads of a FASTQ text against a panel, and ``kpal cross --nearest 1 --pool`` on
files -- each against the loop it replaces, ``klib.pooled`` per group, bit for bit.  Run on the GPU box: pytest -m gpu."""
import contextlib
import io
import os
import random

import numpy as np
import pytest

import memh5

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


def launches(ctx, call):
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        result = call()
        ctx.sync()
        seen = dict((name, count) for name, (_, count) in ctx.prof_get().items() if count)
    finally:
        ctx.prof_enable(False)
    return result, seen


def in_hbm(profiles):
    return all(p._device_counts() is not None for p in profiles)


def pooled_loop(klib, profiles, labels, keys):
    return [klib.pooled([p for p, l in zip(profiles, labels) if l == key]) for key in keys]


# ---- pooled_by ---------------------------------------------------------------------------------------------------------------
def seam_kmers(sequence, k, window):
    """The table of the k-mers of ``sequence`` that lie in no window of ``window`` bases at a step of ``window``: those that
    begin left of a multiple of ``window`` and end right of it.  (A restatement: A, C, G, T are the digits 0 .. 3, the first
    base the most significant; any other letter breaks the k-mer.)"""
    table = np.zeros(4 ** k, dtype=np.int64)
    for seam in range(window, len(sequence), window):
        for start in range(max(0, seam - k + 1), seam):
            word = sequence[start:start + k]
            if len(word) == k and all(c in 'ACGT' for c in word):
                index = 0
                for c in word:
                    index = 4 * index + 'ACGT'.index(c)
                table[index] += 1
    return table


def test_windows_pool_back_to_their_records(ctx):
    """The windows of ``from_fasta_by_window`` pooled by record name: the loop of ``pooled``, bit for bit, in one launch or
    two; the results stay in HBM and no window's counts are asked for.  With window = step a record's windows add up to the
    record of ``from_fasta_by_record`` but for the k-mers that span a seam between two windows: those, counted here from the
    text, make up the difference exactly -- both comparisons were possible."""
    from kpal_amd import klib
    k, window = 4, 50
    rnd = random.Random(31)
    lengths = (0, 3, 49, 50, 51, 100, 333, 1000, 4, 217)
    sequences = [''.join(rnd.choice('ACGTACGTACGTN') for _ in range(n)) for n in lengths]
    text = ''.join('>rec%d words\n%s\n' % (i, s) for i, s in enumerate(sequences)).encode()
    windows = list(klib.Profile.from_fasta_by_window(io.BytesIO(text), k, window))
    assert len(windows) == sum(-(-n // window) for n in lengths) and in_hbm(windows)
    labels = [w.name.rsplit(':', 1)[0] for w in windows]
    (keys, pools), seen = launches(ctx, lambda: klib.pooled_by(windows, labels))
    assert seen in ({'pool_groups': 1}, {'pool_groups': 1, 'pool_groups_final': 1}), seen
    assert keys == ['rec%d' % i for i, n in enumerate(lengths) if n] and [p.name for p in pools] == keys
    assert in_hbm(pools) and in_hbm(windows) and all(p.length == k for p in pools)
    assert len(set(p._device[0] for p in pools)) == 1                      # rows of ONE batch
    loop = pooled_loop(klib, windows, labels, keys)
    records = dict((p.name, p) for p in klib.Profile.from_fasta_by_record(io.BytesIO(text), k))
    assert in_hbm(windows) and in_hbm(pools)
    some = 0
    for key, pool, want in zip(keys, pools, loop):
        assert np.array_equal(pool.counts, want.counts), key
        seams = seam_kmers(sequences[int(key[3:])], k, window)
        some += int(seams.sum())
        assert np.array_equal(pool.counts + seams, records[key].counts), key
    assert some > 30
    # labels of any hashable kind, None for no group; the order of first appearance
    odd = [None if i % 4 == 0 else (i % 3, 'x') for i in range(len(windows))]
    keys, pools = klib.pooled_by(iter(windows), iter(odd))
    assert keys == [(1, 'x'), (2, 'x'), (0, 'x')] and [p.name for p in pools] == ["(1, 'x')", "(2, 'x')", "(0, 'x')"]
    for pool, want in zip(pools, pooled_loop(klib, windows, odd, keys)):
        assert np.array_equal(pool.counts, want.counts)
    assert klib.pooled_by(windows, [None] * len(windows)) == ([], [])


def test_host_profiles_in_two_chunks(ctx, monkeypatch):
    from kpal_amd import klib
    k = 5
    rs = np.random.RandomState(32)
    tables = [rs.randint(-(1 << 62), 1 << 62, size=4 ** k).astype(np.int64) if i % 4 == 1 else rs.poisson(3.0, 4 ** k).astype(np.int64)
              for i in range(23)]
    profiles = [klib.Profile(t.copy(), name='h%d' % i) for i, t in enumerate(tables)]
    labels = ['abc'[i % 3] if i % 7 else None for i in range(23)]
    monkeypatch.setattr(klib, '_RECORD_BATCH_BYTES', 12 * 8 * 4 ** k)      # 12 tables a group: 12 + 11
    (keys, pools), seen = launches(ctx, lambda: klib.pooled_by(profiles, labels))
    assert seen == {'pool_groups': 2}, seen
    assert keys == ['b', 'c', 'a'] and not any(p._device_counts() for p in pools)
    for key, pool in zip(keys, pools):
        want = np.zeros(4 ** k, dtype=np.uint64)
        for t, l in zip(tables, labels):
            if l == key:
                want += t.view(np.uint64)
        assert pool.counts.dtype == np.int64 and np.array_equal(pool.counts, want.view(np.int64)), key
    for pool, want in zip(pools, pooled_loop(klib, profiles, labels, keys)):
        assert np.array_equal(pool.counts, want.counts)
    for p, t in zip(profiles, tables):
        assert np.array_equal(p.counts, t)
    # past the budget of live device tables the results of HBM profiles are downloaded
    text = ''.join('>r%d\n%s\n' % (i, 'ACGTTGCA' * (i + 1)) for i in range(6)).encode()
    records = list(klib.Profile.from_fasta_by_record(io.BytesIO(text), k))
    assert in_hbm(records)
    monkeypatch.setattr(klib, '_DEVICE_PROFILE_BYTES', 8 * 4 ** k)         # one table: two rows do not fit
    keys, pools = klib.pooled_by(records, [0, 1, 0, 1, 0, 1])
    assert keys == [0, 1] and not any(p._device_counts() for p in pools)
    for pool, want in zip(pools, pooled_loop(klib, records, [0, 1, 0, 1, 0, 1], keys)):
        assert np.array_equal(pool.counts, want.counts)


# ---- pooled_nearest ----------------------------------------------------------------------------------------------------------
def reads_and_panel(k):
    """200 reads as FASTQ text -- read 17 has one base: an all-zero profile -- and a panel of eight host profiles of which
    the last repeats the third: a tie goes to the lower position, so nobody's nearest is the last."""
    from kpal_amd import klib
    rnd = random.Random(33)
    out = []
    for i in range(200):
        length = 1 if i == 17 else rnd.choice([k, 30, 80, 150, 151])
        weights = ['ACGT', 'AACGT', 'ACCGT', 'ACGGT', 'ACGTT', 'AATT', 'CCGG'][i % 7]
        out.append('@read%d\n%s\n+\n%s\n' % (i, ''.join(rnd.choice(weights) for _ in range(length)), 'I' * length))
    rs = np.random.RandomState(34)
    panel = []
    for r in range(7):
        word = ['ACGT', 'AACGT', 'ACCGT', 'ACGGT', 'ACGTT', 'AATT', 'CCGG'][r]
        genome = ''.join(rs.choice(list(word), 5000))
        panel.append(klib.Profile(np.array(klib.Profile.from_sequences([genome], k).counts), name='taxon%d' % r))
    panel.append(klib.Profile(panel[2].counts.copy(), name='taxon7'))
    return ''.join(out).encode(), panel


@pytest.mark.parametrize('scaled', (False, True))
def test_pooled_nearest_bins_reads_by_their_nearest_panel_member(ctx, scaled):
    from kpal_amd import kdistlib, klib
    k = 5
    text, panel = reads_and_panel(k)
    dist = kdistlib.ProfileDistance(do_scale=scaled)
    reads = list(klib.Profile.from_fastq_by_record(io.BytesIO(text), k))
    assert len(reads) == 200 and in_hbm(reads) and not reads[17].counts.any()
    reads = list(klib.Profile.from_fastq_by_record(io.BytesIO(text), k))       # (fresh: read 17 was downloaded)
    want_i, want_d = kdistlib.nearest_profiles(reads, panel, dist, 1)
    want_i, want_d = want_i[:, 0], want_d[:, 0]
    assert np.isnan(want_d[17]) == scaled and np.isnan(want_d).sum() == (1 if scaled else 0)
    hit = [[q for q in range(200) if want_i[q] == r and not np.isnan(want_d[q])] for r in range(8)]
    assert not hit[7] and sum(1 for h in hit if h) >= 2
    want = [klib.pooled([reads[q] for q in h]) if h else None for h in hit]

    (indices, distances, pools), seen = launches(ctx, lambda: kdistlib.pooled_nearest(iter(reads), panel, dist))
    assert seen.get('pool_groups') == 1 and seen.get('pool_groups_final', 0) <= 1 and 'pool_set' not in seen, seen
    assert indices.dtype == np.int64 and distances.dtype == np.float64 and indices.shape == distances.shape == (200,)
    assert np.array_equal(indices, want_i) and np.array_equal(distances, want_d, equal_nan=True)
    assert len(pools) == 8 and pools[7] is None
    assert in_hbm(reads) and in_hbm([p for p in pools if p is not None])
    for r in range(8):
        assert (pools[r] is None) == (want[r] is None), r
        if want[r] is not None:
            assert pools[r].name == 'taxon%d' % r and pools[r].length == k
            assert np.array_equal(pools[r].counts, want[r].counts), r
    # three chunks of the left side: the same bits
    (indices3, distances3, pools3), seen = launches(ctx, lambda: kdistlib.pooled_nearest(iter(reads), panel, dist, max_bytes=70 * 8 * 4 ** k))
    assert seen.get('pool_groups') == 3, seen
    assert np.array_equal(indices3, want_i) and np.array_equal(distances3, want_d, equal_nan=True)
    for r in range(8):
        assert (pools3[r] is None) == (want[r] is None), r
        if want[r] is not None:
            assert np.array_equal(pools3[r].counts, want[r].counts), r


def test_pooled_nearest_with_a_callable_follows_the_fallbacks(ctx):
    from kpal_amd import kdistlib, klib
    k = 3
    rs = np.random.RandomState(35)
    left = [klib.Profile(rs.poisson(4.0, 4 ** k).astype(np.int64), name='l%d' % i) for i in range(9)]
    right = [klib.Profile(rs.poisson(4.0, 4 ** k).astype(np.int64), name='r%d' % i) for i in range(3)]
    dist = kdistlib.ProfileDistance(distance_function=lambda a, b: float(np.abs(a - b).sum()))
    indices, distances, pools = kdistlib.pooled_nearest(left, right, dist)
    want_i, want_d = kdistlib.nearest_profiles(left, right, dist, 1)
    assert np.array_equal(indices, want_i[:, 0]) and np.array_equal(distances, want_d[:, 0])
    for r in range(3):
        members = [left[q] for q in range(9) if indices[q] == r]
        assert (pools[r] is None) == (not members)
        if members:
            assert pools[r].name == 'r%d' % r and np.array_equal(pools[r].counts, klib.pooled(members).counts)
    with pytest.raises(ValueError):
        kdistlib.pooled_nearest(left, [], dist)
    # host profiles on the fast route: the pools come back to the host
    plain = kdistlib.ProfileDistance()
    indices, distances, pools = kdistlib.pooled_nearest(left, right, plain, max_bytes=4 * 8 * 4 ** k)
    want_i, want_d = kdistlib.nearest_profiles(left, right, plain, 1)
    assert np.array_equal(indices, want_i[:, 0]) and np.array_equal(distances, want_d[:, 0])
    for r in range(3):
        members = [left[q] for q in range(9) if indices[q] == r]
        assert (pools[r] is None) == (not members)
        if members:
            assert pools[r]._device_counts() is None and np.array_equal(pools[r].counts, klib.pooled(members).counts)


# ---- kpal cross --nearest 1 --pool -------------------------------------------------------------------------------------------
def test_cross_nearest_pool_on_the_command_line(ctx, tmp_path, monkeypatch):
    from kpal_amd import files, kdistlib, klib, kmer
    k = 5
    text, panel = reads_and_panel(k)
    store = memh5.Store()
    monkeypatch.setattr(files, 'open_profile_file', store.open)
    monkeypatch.chdir(tmp_path)
    left, right = files.ProfileFileType('w')('reads.k5'), files.ProfileFileType('w')('panel.k5')
    reads = list(klib.Profile.from_fastq_by_record(io.BytesIO(text), k))[:60]
    for p in reads:
        p.save(left)
    for p in panel:
        p.save(right)
    kmer.main(['cross', 'reads.k5', 'panel.k5', 'near.txt', '--nearest', '1', '--pool', 'bins.k5'])
    names_left, names_right = sorted(left['profiles']), sorted(right['profiles'])
    by_name = dict((p.name, p) for p in reads)
    ordered = [by_name[n] for n in names_left]
    want_i, want_d = kdistlib.nearest_profiles(ordered, [klib.Profile.from_file(right, name=n) for n in names_right],
                                               kdistlib.ProfileDistance(), 1)
    lines = (tmp_path / 'near.txt').read_text().split('\n')[:-1]
    assert len(lines) == 60 and [l.split()[:2] for l in lines] == [[n, names_right[r]] for n, r in zip(names_left, want_i[:, 0])]
    loop = memh5.File('loop.k5')
    hits = []
    for r, name in enumerate(names_right):
        members = [p for p, i in zip(ordered, want_i[:, 0]) if i == r]
        if members:
            hits.append(name)
            klib.pooled(members).save(loop, name=name)
    got = store.files[os.path.abspath('bins.k5')]
    assert list(got['profiles']) == hits == list(loop['profiles']) and 'taxon7' not in hits and len(hits) >= 2
    for name in hits:
        a, b = got['profiles/' + name], loop['profiles/' + name]
        assert a._data.dtype == b._data.dtype and np.array_equal(a._data, b._data), name
        assert sorted(a.attrs) == sorted(b.attrs) == ['length', 'mean', 'median', 'non_zero', 'std', 'total'], name
        for key in b.attrs:
            assert type(a.attrs[key]) is type(b.attrs[key]) and a.attrs[key] == b.attrs[key], (name, key)
    # --pool without --nearest: a usage error
    with contextlib.redirect_stderr(io.StringIO()), pytest.raises(SystemExit) as exc:
        kmer.main(['cross', 'reads.k5', 'panel.k5', 'x.txt', '--pool', 'y.k5'])
    assert exc.value.code == 2
