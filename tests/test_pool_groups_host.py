"""The pool of profiles by label (``klib.pooled_by``, ``kdistlib.pooled_nearest``, ``kpal cross --nearest N --pool FILE``): what
can be checked without a GPU -- the ABI, the command line, the keys and the errors of ``pooled_by``, its host loop for counts
that are no integers, and, against a small stand-in for ``_native.Context`` that keeps "device" memory on the host, what the two
functions ask of a context: one ``pool_groups_device`` per group of tables with ``accumulate`` after the first, results as rows
of one batch, and in ``pooled_nearest`` a chunk's tables made resident once for the selection and the pool."""
import contextlib
import io
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_and_binding():
    from kpal_amd import _native
    header = open(os.path.join(ROOT, 'include', 'kpal_hip.h')).read()
    assert 'kpal_pool_groups_device' in set(re.findall(r'\b(kpal_[a-z0-9_]+)\s*\(', header))
    assert 'kpal_pool_groups_device' in _native.SIGNATURES and hasattr(_native.load(), 'kpal_pool_groups_device')
    assert len(_native.SIGNATURES['kpal_pool_groups_device'][1]) == 8 and hasattr(_native.Context, 'pool_groups_device')


def test_cross_pool_parses(tmp_path, monkeypatch):
    import memh5
    from kpal_amd import files, kmer
    store = memh5.Store()
    monkeypatch.setattr(files, 'open_profile_file', store.open)
    monkeypatch.chdir(tmp_path)
    for name in ('reads.k8', 'panel.k8'):
        files.ProfileFileType('w')(name)
    parser = kmer.build_parser()
    args = parser.parse_args(['cross', 'reads.k8', 'panel.k8', 'x.txt', '--nearest', '3', '--pool', 'p.k8'])
    assert args.nearest == 3 and args.pool is store.files[os.path.abspath('p.k8')] and args.func is kmer.cross
    assert parser.parse_args(['cross', 'reads.k8', 'panel.k8', 'y.txt', '--nearest', '3']).pool is None
    assert parser.parse_args(['cross', 'reads.k8', 'panel.k8', 'z.txt']).pool is None
    for argv in (['cross', 'reads.k8', 'panel.k8', 'v.txt', '--pool', 'q.k8'], ['cross', 'reads.k8', 'panel.k8', '--pool', 'r.k8', 'w.txt']):
        with contextlib.redirect_stderr(io.StringIO()) as err, pytest.raises(SystemExit) as exc:
            parser.parse_args(argv)
        assert exc.value.code == 2 and '--pool needs --nearest' in err.getvalue()
    with contextlib.redirect_stderr(io.StringIO()), pytest.raises(SystemExit) as exc:
        kmer.main(['cross', 'reads.k8', 'panel.k8', 'u.txt', '--pool', 's.k8'])
    assert exc.value.code == 2
    # the function itself, called without the parser
    with pytest.raises(ValueError):
        kmer.cross(store.open('reads.k8', 'w'), store.open('panel.k8', 'w'), io.StringIO(), names_left=['a'], names_right=['b'], pool=store.open('t.k8', 'w'))


def test_pooled_by_of_float_counts_is_the_host_loop():
    from kpal_amd import klib, metrics
    rs = np.random.RandomState(1)
    k = 3
    profiles = [klib.Profile(rs.poisson(5.0, 4 ** k) * 0.37, name='f%d' % i) for i in range(7)]
    profiles[4] = klib.Profile(rs.poisson(5.0, 4 ** k).astype(np.int64), name='i4')      # one integer profile among them
    before = [np.array(p.counts) for p in profiles]
    labels = ['x', ('y', 2), None, 'x', ('y', 2), 'x', 7]
    keys, pools = klib.pooled_by(iter(profiles), iter(labels))
    assert keys == ['x', ('y', 2), 7] and [p.name for p in pools] == ['x', "('y', 2)", '7']
    for key, pool in zip(keys, pools):
        members = [p for p, l in zip(profiles, labels) if l == key]
        total = np.array(members[0].counts)
        for p in members[1:]:
            total = metrics.mergers['sum'](total, p.counts)
        assert pool.length == k and pool.counts.dtype == total.dtype and np.array_equal(pool.counts, total), key
        assert np.array_equal(pool.counts, klib.pooled(members).counts), key
    assert pools[2].counts is not profiles[6].counts              # a group of one is a copy
    for p, b in zip(profiles, before):
        assert np.array_equal(p.counts, b)


def test_pooled_by_errors_and_empty_results():
    from kpal_amd import klib
    a, b, c = (klib.Profile(np.arange(16, dtype=np.int64) + i, name='p%d' % i) for i in range(3))
    other = klib.Profile(np.arange(64, dtype=np.int64), name='k3')
    with pytest.raises(ValueError):
        klib.pooled_by([], [])
    with pytest.raises(ValueError):
        klib.pooled_by([a, b], ['x'])
    with pytest.raises(ValueError):
        klib.pooled_by([a], ['x', 'y'])
    with pytest.raises(ValueError):
        klib.pooled_by([a, other], ['x', 'x'])
    with pytest.raises(ValueError):
        klib.pooled_by([a, other], [None, None])                  # mixed k, even when nothing is pooled
    assert klib.pooled_by([a, b, c], [None, None, None]) == ([], [])


# ---- against a stand-in for the context ---------------------------------------------------------------------------------------
class HostContext(object):
    """``_native.Context`` as far as the pool by label needs it, "device" memory being host arrays at made-up addresses: the
    entries compute what the library computes (the selection with a distance of its own: the sum of absolute differences) and
    note their calls."""
    _h = True

    def __init__(self):
        self.blocks, self.next, self.calls = {}, 1 << 40, []

    def alloc(self, nbytes):
        base = self.next
        self.blocks[base] = np.zeros(int(nbytes), dtype=np.uint8)
        self.next += (int(nbytes) + 8191) // 4096 * 4096
        return base

    def free(self, ptr):
        del self.blocks[ptr]

    def view(self, address, shape):
        nbytes = 8 * int(np.prod(shape))
        for base, data in self.blocks.items():
            if base <= address and address + nbytes <= base + data.size:
                return data[address - base:address - base + nbytes].view(np.int64).reshape(shape)
        raise AssertionError('%d bytes at %#x lie in no allocation' % (nbytes, address))

    def h2d(self, dev_ptr, host_array):
        a = np.ascontiguousarray(host_array)
        self.calls.append(('h2d', dev_ptr))
        self.view(dev_ptr, (a.size,))[:] = a.reshape(-1)

    def d2h(self, host_array, dev_ptr):
        self.calls.append(('d2h', dev_ptr))
        host_array.reshape(-1)[:] = self.view(dev_ptr, (host_array.size,))

    def d2d(self, dev_dst, dev_src, nbytes):
        self.calls.append(('d2d', dev_dst))
        self.view(dev_dst, (nbytes // 8,))[:] = self.view(dev_src, (nbytes // 8,))

    def sync(self):
        pass

    def pool_set_device(self, n_tables, bins, dev_tables, dev_out, accumulate=False):
        self.pool_groups_device(n_tables, bins, dev_tables, np.zeros(n_tables, dtype=np.int64), 1, dev_out, accumulate, name='pool_set')

    def pool_groups_device(self, n_tables, bins, dev_tables, labels, n_groups, dev_out, accumulate=False, name='pool_groups'):
        labels = np.asarray(labels, dtype=np.int64)
        assert labels.shape == (n_tables,) and labels.max(initial=-1) < n_groups
        self.calls.append((name, n_tables, dev_tables, labels.tolist(), n_groups, dev_out, bool(accumulate)))
        tables, out = self.view(dev_tables, (n_tables, bins)), self.view(dev_out, (n_groups, bins))
        if not accumulate:
            out[:] = 0
        with np.errstate(over='ignore'):
            for t, g in enumerate(labels.tolist()):
                if g >= 0:
                    out[g] += tables[t]

    def cross_nearest_device(self, k, Q, dev_left, R, dev_right, options, n, right_first=0, have=0, dist=None, index=None):
        assert have == 0 and right_first == 0 and n == 1
        self.calls.append(('cross_nearest', Q, dev_left))
        left, right = self.view(dev_left, (Q, 4 ** k)), self.view(dev_right, (R, 4 ** k))
        values = np.abs(left[:, None, :] - right[None, :, :]).sum(axis=2).astype(np.float64)
        values[~left.any(axis=1)] = np.nan                         # an all-zero profile has no distance here
        index[:, 0] = np.argmin(np.where(np.isnan(values), np.inf, values), axis=1)
        dist[:, 0] = values[np.arange(Q), index[:, 0]]


@pytest.fixture
def fake(monkeypatch):
    from kpal_amd import _native, klib
    ctx = HostContext()
    monkeypatch.setattr(_native, 'context', lambda: ctx)
    yield ctx
    import gc
    gc.collect()
    pooled_tables = sum(len(v) for v in getattr(ctx, '_table_pool', {}).values())
    assert len(ctx.blocks) == pooled_tables, 'an allocation of a call was not freed'
    assert klib._DeviceBatch.live_bytes >= 0


def table(k, seed):
    return ((np.arange(4 ** k, dtype=np.int64) * 2654435761 + seed * 97) % 11) * (1 if seed % 5 else 1 << 61)


def resident(ctx, k, n, seed=0):
    from kpal_amd import klib
    batch = klib._DeviceBatch(ctx, n * 8 * 4 ** k, n)
    for j in range(n):
        ctx.h2d(batch.ptr + j * 8 * 4 ** k, table(k, seed + j))
    return [klib.Profile._from_device(batch, j, k, 'r%d' % (seed + j)) for j in range(n)]


def sums(tables, labels, key):
    total = np.zeros(tables[0].size, dtype=np.uint64)
    for t, l in zip(tables, labels):
        if l == key:
            total += t.view(np.uint64)
    return total.view(np.int64)


def test_pooled_by_of_host_integers_is_one_call_per_group_of_tables(fake, monkeypatch):
    from kpal_amd import klib
    k, n = 2, 11
    tables = [table(k, i) for i in range(n)]
    profiles = [klib.Profile(t.copy(), name='h%d' % i) for i, t in enumerate(tables)]
    labels = [None if i == 3 else 'abc'[i % 3] for i in range(n)]
    monkeypatch.setattr(klib, '_RECORD_BATCH_BYTES', 4 * 8 * 4 ** k)       # 4 tables a group: 4 + 4 + 3
    keys, pools = klib.pooled_by(profiles, labels)
    assert keys == ['a', 'b', 'c'] and not any(p._device_counts() for p in pools)
    calls = [c for c in fake.calls if c[0] == 'pool_groups']
    assert [(c[1], c[4], c[6]) for c in calls] == [(4, 3, False), (4, 3, True), (3, 3, True)]
    assert [c[3] for c in calls] == [[0, 1, 2, -1], [1, 2, 0, 1], [2, 0, 1]] and len(set(c[5] for c in calls)) == 1
    assert sum(1 for c in fake.calls if c[0] == 'h2d') == n and sum(1 for c in fake.calls if c[0] == 'd2h') == 1
    for key, pool in zip(keys, pools):
        assert pool.name == key and np.array_equal(pool.counts, sums(tables, labels, key)), key


def test_pooled_by_of_resident_profiles_gives_rows_of_one_batch(fake):
    from kpal_amd import klib
    k, n = 2, 9
    profiles = resident(fake, k, n)
    tables = [table(k, j) for j in range(n)]
    labels = [j % 4 if j != 5 else None for j in range(n)]
    del fake.calls[:]
    keys, pools = klib.pooled_by(profiles, labels)
    assert keys == [0, 1, 2, 3] and [p.name for p in pools] == ['0', '1', '2', '3']
    assert [c[0] for c in fake.calls] == ['pool_groups']               # used where they lie: no copy, nothing downloaded
    assert fake.calls[0][2] == profiles[0]._device_counts()[1]
    assert all(p._device_counts() for p in pools + profiles) and len(set(id(p._device[0]) for p in pools)) == 1
    assert [p._device[1] for p in pools] == [0, 1, 2, 3] and pools[0]._device[0] is not profiles[0]._device[0]
    for key, pool in zip(keys, pools):
        assert np.array_equal(pool.counts, sums(tables, labels, key)), key
    # a list that is no run of one batch is gathered for the call, and the result still stays
    del fake.calls[:]
    keys, again = klib.pooled_by(profiles[::-1], labels[::-1])
    assert [c[0] for c in fake.calls].count('d2d') == n and all(p._device_counts() for p in again)
    for key, pool in zip(keys, again):
        assert np.array_equal(pool.counts, sums(tables, labels, key)), key
    # past the budget of live tables the rows are downloaded
    saved, klib._DEVICE_PROFILE_BYTES = klib._DEVICE_PROFILE_BYTES, 8
    try:
        keys, host = klib.pooled_by(profiles, labels)
    finally:
        klib._DEVICE_PROFILE_BYTES = saved
    assert not any(p._device_counts() for p in host) and all(p._device_counts() for p in profiles)
    for key, pool in zip(keys, host):
        assert np.array_equal(pool.counts, sums(tables, labels, key)), key


def test_pooled_nearest_makes_a_chunk_resident_once(fake):
    from kpal_amd import kdistlib, klib
    k, n, R = 2, 10, 4
    tables = [table(k, i) % 7 for i in range(n)]
    tables[6][:] = 0                                                   # no distance: in no bin
    right = [klib.Profile(table(k, 50 + r) % 7, name='taxon%d' % r) for r in range(R)]
    right[3] = klib.Profile(right[1].counts.copy(), name='taxon3')     # a tie goes to the lower position: nobody's nearest

    def left():
        for i, t in enumerate(tables):
            yield klib.Profile(t.copy(), name='q%d' % i)

    dist = kdistlib.ProfileDistance()
    indices, distances, pools = kdistlib.pooled_nearest(left(), right, dist, max_bytes=4 * 8 * 4 ** k)
    calls = list(fake.calls)
    assert indices.shape == distances.shape == (n,) and indices.dtype == np.int64 and distances.dtype == np.float64
    want_i, want_d = kdistlib.nearest_profiles([klib.Profile(t) for t in tables], right, dist, 1)
    assert np.array_equal(indices, want_i[:, 0]) and np.array_equal(distances, want_d[:, 0], equal_nan=True) and np.isnan(distances[6])
    first = [c for c in calls if c[0] in ('cross_nearest', 'pool_groups')][:6]
    # chunks of 4, 4 and 2 tables: the selection, then the pool of the SAME tables, accumulated into the same R rows
    assert [c[0] for c in first] == ['cross_nearest', 'pool_groups'] * 3
    assert [(first[i][1], first[i + 1][1]) for i in (0, 2, 4)] == [(4, 4), (4, 4), (2, 2)]
    assert all(first[i][2] == first[i + 1][2] for i in (0, 2, 4))
    assert [first[i][6] for i in (1, 3, 5)] == [False, True, True] and len(set(first[i][5] for i in (1, 3, 5))) == 1
    assert all(first[i][4] == R for i in (1, 3, 5))
    uploads_before_last_pool = [c for c in calls[:calls.index(first[5]) + 1] if c[0] == 'h2d']
    assert len(uploads_before_last_pool) == n + R                      # every table went up once
    assert len(pools) == R and pools[3] is None
    for r in range(R):
        members = [t for t, i, d in zip(tables, indices, distances) if i == r and not np.isnan(d)]
        assert (pools[r] is None) == (not members), r
        if members:
            assert pools[r].name == 'taxon%d' % r and np.array_equal(pools[r].counts, np.sum(members, axis=0)), r
    # resident left profiles: the pools are rows of one batch, nothing is downloaded
    profiles = resident(fake, k, 6, seed=1)
    del fake.calls[:]
    indices, distances, pools = kdistlib.pooled_nearest(iter(profiles), right, dist)
    assert not any(c[0] == 'd2h' for c in fake.calls) and [c[0] for c in fake.calls if c[0] != 'h2d'] == ['cross_nearest', 'pool_groups']
    kept = [p for p in pools if p is not None]
    assert kept and all(p._device_counts() for p in kept) and len(set(id(p._device[0]) for p in kept)) == 1
    for r, p in enumerate(pools):
        members = [table(k, 1 + j) for j in range(6) if indices[j] == r and not np.isnan(distances[j])]
        assert (p is None) == (not members)
        if members:
            assert np.array_equal(p.counts, sums(members, [0] * len(members), 0))
