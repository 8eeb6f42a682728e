"""The callers of the set transforms (kpal_balance_set_device, kpal_shrink_set_device, kpal_merge_device over whole sets,
kpal_pool_set_device): ``klib.balance_profiles``, ``shrink_profiles``, ``merge_profiles`` and ``pooled`` on profiles that are still
in HBM, on host profiles and on mixed lists, the methods of one HBM profile, and ``kmer.balance`` / ``kmer.shrink`` on a file --
each against the oracle per table, exactly, and a result lives where its table lived.  Run on the GPU box: pytest -m gpu."""
import gc
import io
import random

import numpy as np
import pytest

import memh5
import oracle

pytestmark = pytest.mark.gpu

MERGERS = ('sum', 'xor', 'int', 'nint')


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


def fasta_text(rnd, n, k):
    """n short records, some shorter than k."""
    out = []
    for i in range(n):
        length = rnd.choice([0, 1, k - 1, k, k + 1, 30, 80, 200, 700])
        out.append('>rec%d some words\n%s\n' % (i, ''.join(rnd.choice('ACGTACGTN') for _ in range(length))))
    return ''.join(out).encode()


def fastq_text(rnd, n):
    out = []
    for i in range(n):
        length = rnd.choice([1, 5, 30, 80, 150])
        seq = ''.join(rnd.choice('ACGTACGTN') for _ in range(length))
        qual = ''.join(chr(33 + rnd.choice([2, 10, 25, 40])) for _ in range(length))
        out.append('@read%d\n%s\n+\n%s\n' % (i, seq, qual))
    return ''.join(out).encode()


def batch_of(k, n=12, seed=1):
    """(profiles fresh in HBM, their tables on the host from a second count of the same text)"""
    from kpal_amd import klib
    text = fasta_text(random.Random(seed), n, k)
    profiles = list(klib.Profile.from_fasta_by_record(io.BytesIO(text), k))
    tables = [np.array(p.counts) for p in klib.Profile.from_fasta_by_record(io.BytesIO(text), k)]
    assert len(profiles) == n and all(p._device_counts() is not None for p in profiles)
    return profiles, tables


def in_hbm(profiles):
    return all(p._device_counts() is not None for p in profiles)


# ---- profiles in HBM ---------------------------------------------------------------------------------------------------------
def test_balance_profiles_in_hbm(ctx):
    from kpal_amd import klib
    k = 6
    gc.collect()
    start = klib._DeviceBatch.live_bytes
    profiles, tables = batch_of(k)
    one_batch = 12 * 8 * 4 ** k
    assert klib._DeviceBatch.live_bytes == start + one_batch
    copies = [p.copy() for p in profiles[:3]]
    kept = sum(dict((id(c._device[0]), c._device[0].nbytes) for c in copies).values())   # (a file's records may come in several batches)
    stale = klib.summaries(profiles)                                    # cached with the old batch
    _, seen = launches(ctx, lambda: klib.balance_profiles(profiles))
    assert seen == {'balance_tiled_set': 1}, seen
    assert in_hbm(profiles)
    assert 0 < kept <= one_batch and klib._DeviceBatch.live_bytes == start + one_batch + kept   # the copies keep their old batches
    want = [oracle.balance(t, k) for t in tables]
    fresh = klib.summaries(profiles)
    assert in_hbm(profiles)
    for i, p in enumerate(profiles):
        assert int(fresh[i]['total']) == int(want[i].sum()) and fresh[i]['non_zero'] == np.count_nonzero(want[i]), i
        assert float(fresh[i]['mean']) == pytest.approx(want[i].mean(), rel=1e-9)
    assert any(int(a['total']) != int(b['total']) for a, b in zip(stale, fresh))
    for i, p in enumerate(profiles):
        assert p.length == k and np.array_equal(p.counts, want[i]), i
    for i, c in enumerate(copies):
        assert np.array_equal(c.counts, tables[i]), i                   # a copy taken before still yields the unbalanced table
    del profiles, copies, p, c
    gc.collect()
    assert klib._DeviceBatch.live_bytes == start


def test_live_bytes_grow_by_one_batch(ctx):
    from kpal_amd import klib
    gc.collect()
    start = klib._DeviceBatch.live_bytes
    profiles, _ = batch_of(6)
    one_batch = 12 * 8 * 4 ** 6
    klib.balance_profiles(profiles)
    gc.collect()
    assert klib._DeviceBatch.live_bytes == start + one_batch            # the old batch went when its last profile was re-pointed
    klib.shrink_profiles(profiles, 2)
    gc.collect()
    assert klib._DeviceBatch.live_bytes == start + one_batch // 16
    del profiles
    gc.collect()
    assert klib._DeviceBatch.live_bytes == start


def test_shrink_profiles_in_hbm(ctx):
    from kpal_amd import klib
    k = 6
    profiles, tables = batch_of(k, seed=2)
    _, seen = launches(ctx, lambda: klib.shrink_profiles(profiles, 2))
    assert seen == {'shrink_set': 1}, seen
    assert in_hbm(profiles) and all(p.length == k - 2 and p.number == 4 ** (k - 2) for p in profiles)
    for i, p in enumerate(profiles):
        assert np.array_equal(p.counts, oracle.shrink(tables[i], k, 2)), i


@pytest.mark.parametrize('merger', MERGERS)
def test_merge_profiles_in_hbm(ctx, merger):
    from kpal_amd import klib, metrics
    k = 6
    left, ltables = batch_of(k, seed=3)
    right, rtables = batch_of(k, seed=4)
    _, seen = launches(ctx, lambda: klib.merge_profiles(left, right, metrics.mergers[merger]))
    assert seen == {'merge': 1}, seen
    assert in_hbm(left) and in_hbm(right)
    for i, p in enumerate(left):
        assert np.array_equal(p.counts, oracle.merge(ltables[i], rtables[i], merger)), (merger, i)
        assert np.array_equal(right[i].counts, rtables[i]), i


def test_merge_profiles_with_a_callable_takes_the_host_route(ctx):
    from kpal_amd import klib
    left, ltables = batch_of(5, n=4, seed=5)
    right, rtables = batch_of(5, n=4, seed=6)
    klib.merge_profiles(left, right, lambda x, y: x * 2 + y)
    assert not any(p._device_counts() for p in left)
    for i, p in enumerate(left):
        assert np.array_equal(p.counts, ltables[i] * 2 + rtables[i]), i
    with pytest.raises(ValueError):
        klib.merge_profiles(left, right[:3])


def test_pooled_reads_are_the_file(ctx):
    """No k-mer spans two records: the per-read profiles of a FASTQ text add up to its profile, the same quality mask applied;
    the per-record profiles of a FASTA text to that of the FASTA text."""
    from kpal_amd import klib
    k = 5
    text = fastq_text(random.Random(7), 40)
    reads = list(klib.Profile.from_fastq_by_record(io.BytesIO(text), k, min_quality=20))
    assert len(reads) == 40 and in_hbm(reads)
    pool, seen = launches(ctx, lambda: klib.pooled(reads, name='all'))
    assert set(seen) <= {'pool_set', 'pool_set_final'} and seen.get('pool_set') == 1, seen
    assert pool._device_counts() is not None and in_hbm(reads) and pool.name == 'all' and pool.length == k
    whole = klib.Profile.from_fastq(io.BytesIO(text), k, min_quality=20)
    assert np.array_equal(pool.counts, whole.counts) and pool.counts.sum() > 0

    text = fasta_text(random.Random(8), 30, k)
    records = list(klib.Profile.from_fasta_by_record(io.BytesIO(text), k))
    pool = klib.pooled(records)
    assert pool._device_counts() is not None and pool.name is None
    assert np.array_equal(pool.counts, klib.Profile.from_fasta(io.BytesIO(text), k).counts)
    # host profiles and mixed lists: the result is on the host
    records[3].counts
    mixed = klib.pooled(records)
    assert mixed._device_counts() is None and np.array_equal(mixed.counts, pool.counts)
    with pytest.raises(ValueError):
        klib.pooled([])
    with pytest.raises(ValueError):
        klib.pooled([records[0], klib.Profile(np.zeros(4 ** 3, dtype=np.int64))])


def test_methods_of_one_profile_in_hbm_stay_there(ctx):
    from kpal_amd import klib, metrics
    k = 6
    profiles, tables = batch_of(k, seed=9)
    p, q, r = profiles[4], profiles[5], profiles[6]
    _, seen = launches(ctx, p.balance)
    assert seen == {'balance_tiled_set': 1} and p._device_counts() is not None
    _, seen = launches(ctx, lambda: q.shrink(3))
    assert seen == {'shrink_set': 1} and q._device_counts() is not None and q.length == 3
    _, seen = launches(ctx, lambda: r.merge(profiles[7], metrics.mergers['xor']))
    assert seen == {'merge': 1} and r._device_counts() is not None and profiles[7]._device_counts() is not None
    assert np.array_equal(p.counts, oracle.balance(tables[4], k))
    assert np.array_equal(q.counts, oracle.shrink(tables[5], k, 3))
    assert np.array_equal(r.counts, oracle.merge(tables[6], tables[7], 'xor'))
    # merged with itself: the reference's result, whatever the route
    s = profiles[8]
    s.merge(s)
    assert np.array_equal(s.counts, tables[8] * 2)
    # the other rows of the batch were not touched
    assert np.array_equal(profiles[0].counts, tables[0]) and np.array_equal(profiles[7].counts, tables[7])


# ---- host profiles -----------------------------------------------------------------------------------------------------------
def test_host_profiles(ctx):
    from kpal_amd import klib, metrics
    rs = np.random.RandomState(10)
    k = 6
    arrays = [rs.poisson(3.0, 4 ** k).astype(np.int64) for _ in range(5)]
    tables = [a.copy() for a in arrays]
    profiles = [klib.Profile(a, name='h%d' % i) for i, a in enumerate(arrays)]
    _, seen = launches(ctx, lambda: klib.balance_profiles(profiles))
    assert seen == {'balance_tiled_set': 1}, seen
    for i, p in enumerate(profiles):
        assert p.counts is arrays[i] and p._device_counts() is None              # the very array the caller holds
        assert np.array_equal(arrays[i], oracle.balance(tables[i], k)), i
    # int32 counts: written through, the dtype kept
    small = rs.poisson(3.0, 4 ** 3).astype(np.int32)
    p32, want32 = klib.Profile(small), oracle.balance(small.astype(np.int64), 3)
    klib.balance_profiles([p32])
    assert p32.counts is small and small.dtype == np.int32 and np.array_equal(small, want32)
    # float counts: what balance() gives
    scaled = rs.poisson(5.0, 4 ** 4) * 0.37
    a, b = klib.Profile(scaled.copy()), klib.Profile(scaled.copy())
    klib.balance_profiles([a])
    b.balance()
    assert a.counts.dtype == np.float64 and np.array_equal(a.counts, b.counts)
    # shrink and merge assign new int64 arrays
    profiles = [klib.Profile(t.copy()) for t in tables]
    _, seen = launches(ctx, lambda: klib.shrink_profiles(profiles, 1))
    assert seen == {'shrink_set': 1}, seen
    for i, p in enumerate(profiles):
        assert p.length == k - 1 and p.counts.dtype == np.int64 and np.array_equal(p.counts, oracle.shrink(tables[i], k, 1)), i
    left = [klib.Profile(t.copy()) for t in tables[:2]]
    right = [klib.Profile(t.copy()) for t in tables[2:4]]
    _, seen = launches(ctx, lambda: klib.merge_profiles(left, right, metrics.mergers['nint']))
    assert seen == {'merge': 1}, seen
    for i in range(2):
        assert np.array_equal(left[i].counts, oracle.merge(tables[i], tables[2 + i], 'nint')), i
        assert np.array_equal(right[i].counts, tables[2 + i]), i
    pool = klib.pooled([klib.Profile(t) for t in tables], name='sum')
    assert pool._device_counts() is None and np.array_equal(pool.counts, np.sum(tables, axis=0))


def test_errors_come_before_any_change(ctx):
    from kpal_amd import klib
    profiles, tables = batch_of(4, n=5, seed=11)
    host = klib.Profile(np.arange(4 ** 2, dtype=np.int64))
    for call in (lambda: klib.balance_profiles(profiles + [profiles[2]]),
                 lambda: klib.shrink_profiles(profiles + [profiles[0]], 1),
                 lambda: klib.merge_profiles(profiles[:2] + [profiles[0]], profiles[2:5]),
                 lambda: klib.shrink_profiles(profiles, 4),
                 lambda: klib.shrink_profiles(profiles + [host], 2),             # fine for k = 4, not for k = 2
                 lambda: klib.shrink_profiles([host] + profiles, 7)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        klib.shrink_profiles(profiles, -1)
    assert in_hbm(profiles) and all(p.length == 4 for p in profiles) and host.length == 2
    assert np.array_equal(host.counts, np.arange(16))
    for i, p in enumerate(profiles):
        assert np.array_equal(p.counts, tables[i]), i


def test_past_the_budget_the_results_are_on_the_host(ctx, monkeypatch):
    from kpal_amd import klib, metrics
    k = 6
    profiles, tables = batch_of(k, seed=12)
    others, otables = batch_of(k, seed=13)
    monkeypatch.setattr(klib, '_DEVICE_PROFILE_BYTES', 8 * 4 ** (k - 2))   # below one table, of the shrunk ones too
    klib.balance_profiles(profiles[:4])
    klib.shrink_profiles(profiles[4:8], 1)
    klib.merge_profiles(profiles[8:], others[8:], metrics.mergers['sum'])
    pool = klib.pooled(others[:8])
    assert not any(p._device_counts() for p in profiles) and pool._device_counts() is None
    for i in range(4):
        assert np.array_equal(profiles[i].counts, oracle.balance(tables[i], k)), i
        assert np.array_equal(profiles[4 + i].counts, oracle.shrink(tables[4 + i], k, 1)) and profiles[4 + i].length == k - 1, i
        assert np.array_equal(profiles[8 + i].counts, oracle.merge(tables[8 + i], otables[8 + i], 'sum')), i
    assert np.array_equal(pool.counts, np.sum(otables[:8], axis=0))


def test_mixed_lengths_and_residency(ctx):
    from kpal_amd import klib
    rs = np.random.RandomState(14)
    dev6, t6 = batch_of(6, n=5, seed=15)
    dev4, t4 = batch_of(4, n=5, seed=16)
    h6 = rs.poisson(2.0, 4 ** 6).astype(np.int64)
    h3 = rs.poisson(2.0, 4 ** 3).astype(np.int64)
    scaled = rs.poisson(5.0, 4 ** 3) * 0.5
    mixed = [dev6[3], klib.Profile(h6.copy()), dev4[0], klib.Profile(scaled.copy()), dev6[1], klib.Profile(h3.copy()), dev4[4]]
    want = [oracle.balance(t6[3], 6), oracle.balance(h6, 6), oracle.balance(t4[0], 4), None, oracle.balance(t6[1], 6), oracle.balance(h3, 3),
            oracle.balance(t4[4], 4)]
    resident = [p._device_counts() is not None for p in mixed]
    _, seen = launches(ctx, lambda: klib.balance_profiles(iter(mixed)))
    assert seen == {'balance_tiled_set': 2, 'balance_set': 2}, seen      # k = 6 in HBM, k = 6 host; k = 4 in HBM, k = 3 host
    assert [p._device_counts() is not None for p in mixed] == resident
    reference = klib.Profile(scaled.copy())
    reference.balance()
    for i, p in enumerate(mixed):
        assert np.array_equal(p.counts, reference.counts if want[i] is None else want[i]), i
    # the rows that were not in the call stay what they were
    assert np.array_equal(dev6[0].counts, t6[0]) and np.array_equal(dev4[2].counts, t4[2])
    lengths = [p.length for p in mixed if p.counts.dtype == np.int64]
    ints = [p for p in mixed if p.counts.dtype == np.int64]
    before = [np.array(p.counts) for p in ints]
    klib.shrink_profiles(ints, 2)
    for p, length, table in zip(ints, lengths, before):
        assert p.length == length - 2 and np.array_equal(p.counts, oracle.shrink(table, length, 2))


# ---- kpal balance, kpal shrink -------------------------------------------------------------------------------------------------
def nine_profiles():
    from kpal_amd import klib
    rs = np.random.RandomState(17)
    handle = memh5.File('in.k')
    for i, (name, k) in enumerate((('zeta', 4), ('alpha', 6), ('m_1', 4), ('beta', 6), ('m_2', 4), ('gamma', 4), ('delta', 6), ('eps', 5),
                                   ('eta', 7))):
        klib.Profile(rs.poisson((0.05, 3.0, 40.0)[i % 3], 4 ** k).astype(np.int64), name=name).save(handle)
    return handle


def same_files(got, want):
    assert list(got['profiles']) == list(want['profiles']) and len(got['profiles']) == 9
    for name in want['profiles']:
        a, b = got['profiles/' + name], want['profiles/' + name]
        assert a._data.dtype == b._data.dtype and np.array_equal(a._data, b._data), name
        assert sorted(a.attrs) == sorted(b.attrs) == ['length', 'mean', 'median', 'non_zero', 'std', 'total'], name
        for key in b.attrs:
            assert type(a.attrs[key]) is type(b.attrs[key]) and a.attrs[key] == b.attrs[key], (name, key, a.attrs[key], b.attrs[key])


def test_kmer_balance_and_shrink_write_what_the_loop_writes(ctx):
    from kpal_amd import klib, kmer
    source = nine_profiles()
    names = sorted(source['profiles'])
    loop = memh5.File('loop.k')
    for name in names:
        profile = klib.Profile.from_file(source, name=name)
        profile.balance()
        profile.save(loop)
    sets = memh5.File('sets.k')
    _, seen = launches(ctx, lambda: kmer.balance(source, sets))
    assert seen.get('balance_set') == 2 and seen.get('balance_tiled_set') == 2 and 'balance_tiled' not in seen, seen   # k = 4, 5; 6, 7
    same_files(sets, loop)

    loop = memh5.File('loop.k')
    for name in names:
        profile = klib.Profile.from_file(source, name=name)
        profile.shrink(2)
        profile.save(loop)
    sets = memh5.File('sets.k')
    _, seen = launches(ctx, lambda: kmer.shrink(source, sets, 2))
    assert seen.get('shrink_set') == 4 and 'shrink' not in seen, seen
    same_files(sets, loop)
    with pytest.raises(ValueError):
        kmer.shrink(source, memh5.File('bad.k'), 4)
