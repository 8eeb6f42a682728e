"""What the profile-set front end (klib's set transforms and summaries, kdistlib's set distances) asks of a context, without
a GPU: every function is driven against a recording stand-in for ``_native.Context`` and the ordered native calls, where every
profile ends up, and the live device bytes are compared with ``tests/golden/profile_set_calls.json``.

The golden file is a recording of this module itself (``python tests/test_profile_set_calls_host.py --record``), made before
the front end was consolidated: it pins the calls, their order and arguments, residency and the moment memory goes back, so
that a change to the Python scaffolding that moves any of them shows here.  Device addresses are written relative to the
allocation they fall in: ``s<N>+off`` for the N-th allocation made while a case was set up, ``a<N>+off`` for the N-th one
the function under test made.  On top of the recording every case checks that no access leaves its allocation or touches a
freed one, and that everything allocated outside a batch was freed."""
import contextlib
import ctypes
import gc
import io
import json
import os
import sys

import numpy as np
import pytest

from kpal_amd import _native, kdistlib, klib, metrics

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'profile_set_calls.json')
BASE = 1 << 40          # device "addresses" start here: any integer argument at or past it is one


class Recorder(object):
    """A stand-in for ``_native.Context``: a bump allocator over host memory, and the entries the set paths call, each of
    which appends ``[name, arguments]`` to ``calls`` and returns an array of the right shape and dtype."""
    _h = True           # (an open context: _DeviceBatch pools or frees its allocation)

    def __init__(self):
        self.calls, self.blocks, self.next, self.setup = [], [], BASE, True

    # -- memory --------------------------------------------------------------------------------
    def _block(self, address):
        for block in self.blocks:
            if block['base'] <= address < block['base'] + block['data'].size:
                return block
        raise AssertionError('address %#x lies in no allocation' % address)

    def _bytes(self, address, nbytes):
        block = self._block(address)
        assert not block['freed'], 'use of %s after its free' % block['label']
        at = address - block['base']
        assert at + nbytes <= block['data'].size, 'access past the end of %s' % block['label']
        return block['data'][at:at + nbytes]

    def label(self, address):
        block = self._block(address)
        return '%s+%d' % (block['label'], address - block['base'])

    def norm(self, value):
        if isinstance(value, (bool, np.bool_)) or value is None or isinstance(value, str):
            return value
        if isinstance(value, (int, np.integer)):
            return self.label(int(value)) if int(value) >= BASE else int(value)
        if isinstance(value, (float, np.floating)):
            return float(value)
        if isinstance(value, np.ndarray):
            return 'ndarray %s %s' % (value.dtype, list(value.shape))
        if isinstance(value, ctypes.Structure):
            return dict((name, self.norm(getattr(value, name))) for name, _ in value._fields_)
        if isinstance(value, (list, tuple)):
            return [self.norm(v) for v in value]
        raise AssertionError('unexpected argument %r' % (value,))

    def record(self, name, *args, **kwargs):
        if not self.setup:
            self.calls.append([name, [self.norm(a) for a in args]] + ([dict((k, self.norm(v)) for k, v in kwargs.items())] if kwargs else []))

    def alloc(self, nbytes):
        label = '%s%d' % ('s' if self.setup else 'a', sum(b['label'][0] == ('s' if self.setup else 'a') for b in self.blocks))
        self.blocks.append({'base': self.next, 'data': np.zeros(int(nbytes), dtype=np.uint8), 'label': label, 'freed': False})
        self.next += (int(nbytes) + 8191) // 4096 * 4096          # (a gap: two allocations are never consecutive tables)
        self.record('alloc', int(nbytes), label)
        return self.blocks[-1]['base']

    def free(self, ptr):
        block = self._block(ptr)
        assert ptr == block['base'] and not block['freed'], 'free of %#x' % ptr
        self.record('free', ptr)
        block['freed'] = True

    def h2d(self, dev_ptr, host_array):
        a = np.ascontiguousarray(host_array)
        self.record('h2d', dev_ptr, a)
        self._bytes(dev_ptr, a.nbytes)[:] = a.view(np.uint8).reshape(-1)

    def d2h(self, host_array, dev_ptr):
        assert host_array.flags['C_CONTIGUOUS']
        self.record('d2h', host_array, dev_ptr)
        host_array.view(np.uint8).reshape(-1)[:] = self._bytes(dev_ptr, host_array.nbytes)

    def d2d(self, dev_dst, dev_src, nbytes):
        self.record('d2d', dev_dst, dev_src, nbytes)
        self._bytes(dev_dst, nbytes)[:] = self._bytes(dev_src, nbytes)

    def sync(self):
        self.record('sync')

    def _tables(self, address, n_tables, bins):
        self._bytes(address, 8 * int(n_tables) * int(bins))

    # -- the set entries of klib ---------------------------------------------------------------
    def stats_set_device(self, dev_ptr, n_tables, bins):
        self.record('stats_set_device', dev_ptr, n_tables, bins)
        self._tables(dev_ptr, n_tables, bins)
        return (_native.ProfileStats * int(n_tables))()

    def balance_set_device(self, k, n_tables, dev_in, dev_out):
        self.record('balance_set_device', k, n_tables, dev_in, dev_out)
        self._tables(dev_in, n_tables, 4 ** k), self._tables(dev_out, n_tables, 4 ** k)

    def shrink_set_device(self, k, factor, n_tables, dev_in, dev_out):
        self.record('shrink_set_device', k, factor, n_tables, dev_in, dev_out)
        self._tables(dev_in, n_tables, 4 ** k), self._tables(dev_out, n_tables, 4 ** (k - factor))

    def merge_device(self, n, dev_left, dev_right, merger, dev_out):
        self.record('merge_device', n, dev_left, dev_right, merger, dev_out)
        self._tables(dev_left, 1, n), self._tables(dev_right, 1, n), self._tables(dev_out, 1, n)

    def paired_smooth_device(self, k, N, dev_left, dev_right, summary, threshold, dev_out_left, dev_out_right, chunk_pairs=0):
        self.record('paired_smooth_device', k, N, dev_left, dev_right, summary, threshold, dev_out_left, dev_out_right)
        for address in (dev_left, dev_right, dev_out_left, dev_out_right):
            self._tables(address, N, 4 ** k)

    def pool_set_device(self, n_tables, bins, dev_tables, dev_out, accumulate=False):
        self.record('pool_set_device', n_tables, bins, dev_tables, dev_out, accumulate=accumulate)
        self._tables(dev_tables, n_tables, bins), self._tables(dev_out, 1, bins)

    # -- the per-profile entries the fallbacks of klib take ------------------------------------
    def balance_inplace(self, counts, k):
        self.record('balance_inplace', counts, k)

    def shrink(self, counts, k, factor):
        self.record('shrink', np.asanyarray(counts), k, factor)
        return np.zeros(4 ** (k - factor), dtype=np.int64)

    def merge(self, left, right, merger):
        self.record('merge', np.asanyarray(left), np.asanyarray(right), merger)
        return np.zeros(np.asanyarray(left).size, dtype=np.int64)

    def dynamic_smooth(self, left, right, k, summary, threshold):
        self.record('dynamic_smooth', left, right, k, summary, threshold)

    def stats(self, counts):
        self.record('stats', np.asanyarray(counts))
        return _native.ProfileStats()

    # -- the set entries of kdistlib -----------------------------------------------------------
    def _rectangle(self, name, k, Q, dev_left, R, dev_right, *rest, **kwargs):
        self.record(name, k, Q, dev_left, R, dev_right, *rest, **kwargs)
        self._tables(dev_left, Q, 4 ** k), self._tables(dev_right, R, 4 ** k)
        return np.zeros((int(Q), int(R)), dtype=np.float64)

    def cross_distance_device(self, k, Q, dev_left, R, dev_right, metric, do_balance=False):
        return self._rectangle('cross_distance_device', k, Q, dev_left, R, dev_right, metric, do_balance=do_balance)

    def cross_profile_distance_device(self, k, Q, dev_left, R, dev_right, options):
        return self._rectangle('cross_profile_distance_device', k, Q, dev_left, R, dev_right, options)

    def cross_smooth_distance_device(self, k, Q, dev_left, R, dev_right, options):
        return self._rectangle('cross_smooth_distance_device', k, Q, dev_left, R, dev_right, options)

    def cross_nearest_device(self, k, Q, dev_left, R, dev_right, options, n, right_first=0, have=0, tile_q=0, tile_r=0,
                             dist=None, index=None):
        self._rectangle('cross_nearest_device', k, Q, dev_left, R, dev_right, options, n, right_first=right_first, have=have,
                        dist=dist, index=index)
        return dist, index

    def _pairs(self, name, k, N, dev_left, dev_right, options):
        self.record(name, k, N, dev_left, dev_right, options)
        self._tables(dev_left, N, 4 ** k), self._tables(dev_right, N, 4 ** k)
        return np.zeros(int(N), dtype=np.float64)

    def paired_distance_device(self, k, N, dev_left, dev_right, options, chunk_pairs=0):
        return self._pairs('paired_distance_device', k, N, dev_left, dev_right, options)

    def paired_smooth_distance_device(self, k, N, dev_left, dev_right, options, chunk_pairs=0):
        return self._pairs('paired_smooth_distance_device', k, N, dev_left, dev_right, options)

    def _triangle(self, name, P, k, dev_profiles, *rest, **kwargs):
        self.record(name, P, k, dev_profiles, *rest, **kwargs)
        self._tables(dev_profiles, P, 4 ** k)
        return np.zeros(P * (P - 1) // 2, dtype=np.float64)

    def distance_matrix_device(self, P, k, dev_profiles, metric, do_balance=False):
        return self._triangle('distance_matrix_device', P, k, dev_profiles, metric, do_balance=do_balance)

    def profile_distance_matrix_device(self, P, k, dev_profiles, options):
        return self._triangle('profile_distance_matrix_device', P, k, dev_profiles, options)

    def smooth_distance_matrix_device(self, P, k, dev_profiles, options):
        return self._triangle('smooth_distance_matrix_device', P, k, dev_profiles, options)

    # -- the host-array entries distance_matrix takes for host profiles ------------------------
    def distance_matrix(self, profiles, k, metric, do_balance=False):
        self.record('distance_matrix', [np.asanyarray(p) for p in profiles], k, metric, do_balance=do_balance)
        return np.zeros(len(profiles) * (len(profiles) - 1) // 2, dtype=np.float64)

    def profile_distance_matrix(self, profiles, k, options):
        self.record('profile_distance_matrix', [np.asanyarray(p) for p in profiles], k, options)
        return np.zeros(len(profiles) * (len(profiles) - 1) // 2, dtype=np.float64)


# ---- profiles ---------------------------------------------------------------------------------------------------------------
def table(k, seed):
    return (np.arange(4 ** k, dtype=np.int64) * 3 + seed) % 7


def resident(ctx, k, n, seed=0):
    """``n`` profiles whose tables are the rows of one new batch on ``ctx``."""
    batch = klib._DeviceBatch(ctx, n * 8 * 4 ** k, n)
    for j in range(n):
        ctx.h2d(batch.ptr + j * 8 * 4 ** k, table(k, seed + j))
    return [klib.Profile._from_device(batch, j, k, 'r%d_%d' % (seed, j)) for j in range(n)]


def host(k, seed):
    return klib.Profile(table(k, seed), name='h%d' % seed)


def floating(k, seed):
    return klib.Profile(table(k, seed) * 0.5, name='f%d' % seed)


def placement(ctx, p):
    at = p._device_counts()
    if at:
        assert at[0] is ctx
        return ['hbm', ctx.label(at[1]), p.length]
    return ['host', str(p._counts.dtype), list(p._counts.shape), p.length]


@contextlib.contextmanager
def patched(**values):
    """``_native.context`` and the named tunables of klib for the length of a case."""
    saved = dict((name, getattr(klib, name)) for name in values)
    saved_context = _native.context
    try:
        for name, value in values.items():
            setattr(klib, name, value)
        yield
    finally:
        _native.context = saved_context
        for name, value in saved.items():
            setattr(klib, name, value)


def observe(build, call, tunables=None):
    """One case: ``build(ctx)`` makes the profiles (a list, or a tuple of lists), ``call(ctx, profiles)`` runs the function
    under test and returns what else is to be written down.  Returns the observation that the golden file holds."""
    ctx = Recorder()
    gc.collect()
    start = klib._DeviceBatch.live_bytes
    with patched(**(tunables(ctx) if tunables else {})):
        _native.context = lambda: ctx
        made = build(ctx)
        everyone = made if isinstance(made, list) else [p for side in made for p in side]
        distinct = []
        for p in everyone:
            if all(p is not q for q in distinct):
                distinct.append(p)
        gc.collect()
        before = klib._DeviceBatch.live_bytes - start
        ctx.setup = False
        seen = {'error': None, 'extra': None}
        try:
            seen['extra'] = call(ctx, made)
        except (ValueError, TypeError) as error:
            seen['error'] = '%s: %s' % (type(error).__name__, error)
        ctx.setup = True
        gc.collect()
        seen['calls'] = ctx.calls
        seen['profiles'] = [placement(ctx, p) for p in distinct]
        seen['live_bytes'] = [before, klib._DeviceBatch.live_bytes - start]
        del made, everyone, distinct, p
        gc.collect()
        seen['live_bytes'].append(klib._DeviceBatch.live_bytes - start)
        # whatever was allocated outside a batch has been freed; a batch's allocation waits in the context's pool
        pooled = [ptr for ptrs in getattr(ctx, '_table_pool', {}).values() for ptr in ptrs]
        for block in ctx.blocks:
            assert block['freed'] or block['base'] in pooled, 'leaked: %s' % block['label']
        assert seen['live_bytes'][2] == 0
    return json.loads(json.dumps(seen))


# ---- the cases ---------------------------------------------------------------------------------------------------------------
ONE_LIST = ('consecutive', 'gathered', 'host', 'mixed', 'two_lengths', 'float', 'no_budget', 'seam_resident', 'seam_host')
TWO_LISTS = ONE_LIST + ('unequal', 'repeated', 'partner_is_target')


def one_list(ctx, scenario, k1, k2):
    if scenario in ('consecutive', 'seam_resident'):
        return resident(ctx, k1, 3)
    if scenario == 'gathered':
        a, b = resident(ctx, k1, 2), resident(ctx, k1, 1, 5)
        return [a[0], b[0], a[1]]
    if scenario in ('host', 'seam_host'):
        return [host(k1, i) for i in range(3)]
    if scenario == 'mixed':
        a, b = resident(ctx, k1, 2), resident(ctx, k1, 1, 5)
        return [a[1], host(k1, 1), b[0], a[0]]
    if scenario == 'two_lengths':
        a, b = resident(ctx, k1, 2), resident(ctx, k2, 2, 3)
        return [a[0], host(k2, 1), b[0], host(k1, 2), a[1], b[1], host(k2, 4)]
    if scenario == 'float':
        a = resident(ctx, k1, 2)
        return [a[0], floating(k1, 1), host(k1, 2), a[1]]
    if scenario == 'no_budget':
        return resident(ctx, k1, 3) + [host(k1, 3)]
    raise AssertionError(scenario)


def two_lists(ctx, scenario, k1, k2):
    if scenario in ('consecutive', 'seam_resident', 'no_budget'):
        return resident(ctx, k1, 3), resident(ctx, k1, 3, 4)
    if scenario == 'gathered':
        a, b = resident(ctx, k1, 2), resident(ctx, k1, 1, 5)
        return [a[0], b[0], a[1]], resident(ctx, k1, 3, 4)
    if scenario in ('host', 'seam_host'):
        return [host(k1, i) for i in range(3)], [host(k1, 3 + i) for i in range(3)]
    if scenario == 'mixed':
        a, b = resident(ctx, k1, 2), resident(ctx, k1, 2, 5)
        return [a[0], host(k1, 1), a[1]], [b[0], b[1], host(k1, 2)]
    if scenario == 'two_lengths':
        a, b, c = resident(ctx, k1, 2), resident(ctx, k2, 2, 3), resident(ctx, k1, 2, 6)
        return [a[0], host(k2, 1), b[0], host(k1, 2), b[1]], [c[0], host(k2, 3), host(k2, 4), c[1], a[1]]
    if scenario == 'float':
        a, b = resident(ctx, k1, 2), resident(ctx, k1, 2, 5)
        return [a[0], floating(k1, 1), host(k1, 2), a[1]], [b[0], host(k1, 3), floating(k1, 4), b[1]]
    if scenario == 'unequal':
        return resident(ctx, k1, 2), resident(ctx, k1, 3, 4)
    if scenario == 'repeated':
        a = resident(ctx, k1, 2)
        return [a[0], a[0]], resident(ctx, k1, 2, 4)
    if scenario == 'partner_is_target':
        a = resident(ctx, k1, 3)
        return [a[0], a[1], host(k1, 1)], [a[1], a[2], host(k1, 2)]
    raise AssertionError(scenario)


def tunables_of(scenario, k1, sides=1):
    if scenario == 'no_budget':
        return lambda ctx: {'_DEVICE_PROFILE_BYTES': 0}
    if scenario.startswith('seam'):
        return lambda ctx: {'_RECORD_BATCH_BYTES': 2 * 8 * 4 ** k1}       # two tables: a seam inside three profiles
    return None


def _pooled(ctx, profiles):
    result = klib.pooled(profiles, name='sum')
    return placement(ctx, result)


def _smooth(ctx, sides):
    klib.smooth_profiles(sides[0], sides[1], kdistlib.ProfileDistance(summary=metrics.summary['min'], threshold=0))


SET_CALLS = {
    'balance_profiles': (one_list, 1, 2, lambda ctx, profiles: klib.balance_profiles(profiles)),
    'shrink_profiles': (one_list, 2, 3, lambda ctx, profiles: klib.shrink_profiles(profiles, 1)),
    'pooled': (one_list, 1, 2, _pooled),
    'summaries': (one_list, 1, 2, lambda ctx, profiles: [sorted(s) for s in klib.summaries(profiles)]),
    'merge_profiles': (two_lists, 1, 2, lambda ctx, sides: klib.merge_profiles(sides[0], sides[1])),
    'smooth_profiles': (two_lists, 1, 2, _smooth),
}


def set_case(function, scenario):
    build, k1, k2, call = SET_CALLS[function]
    return observe(lambda ctx: build(ctx, scenario, k1, k2), call, tunables_of(scenario, k1))


DISTS = {'plain': {}, 'smooth': {'do_smooth': True}, 'scale': {'do_scale': True}}
K = 2
TABLE_BYTES = 8 * 4 ** K


def sets(ctx, scenario):
    """(left, right) for the distance functions; the one-set functions take the left side."""
    if scenario in ('consecutive', 'chunks'):
        return resident(ctx, K, 3), resident(ctx, K, 3, 4)
    if scenario == 'gathered':
        a, b, c = resident(ctx, K, 2), resident(ctx, K, 1, 5), resident(ctx, K, 2, 6)
        return [a[0], b[0], a[1]], [c[1], a[0], c[0]]
    if scenario == 'same':
        left = resident(ctx, K, 3)
        return left, list(left)
    if scenario == 'same_gathered':
        a = resident(ctx, K, 3)
        left = [a[2], host(K, 1), a[0]]
        return left, list(left)
    if scenario == 'host':
        return [host(K, i) for i in range(3)], [host(K, 3 + i) for i in range(3)]
    if scenario == 'mixed':
        a = resident(ctx, K, 2)
        return [a[0], host(K, 1), a[1]], [host(K, 2), a[1], a[0]]
    raise AssertionError(scenario)


def _nearest(ctx, sides, max_bytes):
    return [[len(chunk), list(i.shape), list(d.shape)] for chunk, i, d in kdistlib.nearest_chunks(sides[0], sides[1], sides[2], 2, max_bytes=max_bytes)]


def _matrix(ctx, sides):
    out = io.StringIO()
    kdistlib.distance_matrix(sides[0], out, 3, sides[2])
    return out.getvalue()


def _device_matrix(ctx, sides):
    values = kdistlib._device_matrix(sides[0], sides[2], sides[2]._native_metric())
    return None if values is None else list(values.shape)


PAIR_SCENARIOS = ('consecutive', 'gathered', 'same', 'same_gathered', 'host', 'mixed', 'chunks')
SET_SCENARIOS = ('consecutive', 'gathered', 'host', 'mixed')
DIST_CALLS = {
    'cross_distances': (PAIR_SCENARIOS, lambda ctx, s, mb: list(kdistlib.cross_distances(s[0], s[1], s[2], max_bytes=mb).shape), 2 * TABLE_BYTES),
    'paired_distances': (PAIR_SCENARIOS, lambda ctx, s, mb: list(kdistlib.paired_distances(s[0], s[1], s[2], max_bytes=mb).shape), 4 * TABLE_BYTES),
    'nearest_chunks': (PAIR_SCENARIOS, _nearest, 2 * TABLE_BYTES),
    'successive_distances': (SET_SCENARIOS, lambda ctx, s, mb: list(kdistlib.successive_distances(s[0], s[2], lag=1).shape), None),
    'distance_matrix': (SET_SCENARIOS, lambda ctx, s, mb: _matrix(ctx, s), None),
    '_device_matrix': (SET_SCENARIOS, lambda ctx, s, mb: _device_matrix(ctx, s), None),
}


def observe_dist(function, scenario, kind):
    """``observe`` keeps the ProfileDistance out of the profiles it describes."""
    _, call, chunk_bytes = DIST_CALLS[function]
    dist = kdistlib.ProfileDistance(**DISTS[kind])
    max_bytes = chunk_bytes if scenario == 'chunks' else None
    return observe(lambda ctx: sets(ctx, scenario), lambda ctx, made: call(ctx, (made[0], made[1], dist), max_bytes))


def streamed_nearest():
    """A left side that is made as it is read, one batch of two tables per chunk, by a caller that keeps nothing: the device
    bytes alive each time ``nearest_chunks`` yields, and the calls of the whole scan."""
    ctx = Recorder()
    gc.collect()
    start = klib._DeviceBatch.live_bytes
    with patched():
        _native.context = lambda: ctx
        right = resident(ctx, K, 3, 9)

        def left():
            for seed in range(3):
                ctx.setup = True
                batch = resident(ctx, K, 2, seed)
                ctx.setup = False
                for p in batch:
                    yield p
                del batch, p

        ctx.setup = False
        live = []
        for chunk, indices, distances in kdistlib.nearest_chunks(left(), right, kdistlib.ProfileDistance(), 2, max_bytes=2 * TABLE_BYTES):
            del chunk
            gc.collect()
            live.append(klib._DeviceBatch.live_bytes - start)
        del right
        gc.collect()
        live.append(klib._DeviceBatch.live_bytes - start)
    assert live[-1] == 0
    return json.loads(json.dumps({'calls': ctx.calls, 'live_bytes': live}))


def all_cases():
    cases = {}
    for function, (build, _, _, _) in sorted(SET_CALLS.items()):
        for scenario in (ONE_LIST if build is one_list else TWO_LISTS):
            cases['%s/%s' % (function, scenario)] = (set_case, (function, scenario))
    for function, (scenarios, _, _) in sorted(DIST_CALLS.items()):
        for scenario in scenarios:
            for kind in sorted(DISTS):
                cases['%s/%s/%s' % (function, scenario, kind)] = (observe_dist, (function, scenario, kind))
    cases['nearest_chunks/streamed'] = (streamed_nearest, ())
    return cases


CASES = all_cases()


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as handle:
        return json.load(handle)


def test_the_golden_file_holds_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize('case', sorted(CASES))
def test_calls_residency_and_live_bytes(golden, case):
    function, arguments = CASES[case]
    seen, want = function(*arguments), golden[case]
    assert seen['calls'] == want['calls']
    assert seen == want


def test_the_recorder_refuses_what_a_device_would_fault_on():
    ctx = Recorder()
    a = ctx.alloc(64)
    with pytest.raises(AssertionError):
        ctx.d2d(a + 32, a, 64)              # past the end
    ctx.free(a)
    with pytest.raises(AssertionError):
        ctx.d2h(np.zeros(8, dtype=np.int64), a)      # after the free
    with pytest.raises(AssertionError):
        ctx.free(a)


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        sys.exit('usage: test_profile_set_calls_host.py --record')
    with open(GOLDEN, 'w') as handle:
        handle.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(case), json.dumps(CASES[case][0](*CASES[case][1]), sort_keys=True))
                                        for case in sorted(CASES)) + '\n}\n')
