"""kpal_paired_distance[_device] on the GPU: out[i] = ProfileDistance.distance(left[i], right[i]) for the linked pairs of two
sets of profiles (kpal_amd/csrc/pair_set_plan.hpp, pair_set_kernels.hpp, kpal_paired.hip).

Every expected value is the oracle's pair function on that pair (``oracle.distance`` for a plain metric, else
``oracle.profile_distance``).  Contract, that of tests/test_gpu_cross.py: unscaled euclidean bit for bit; everything else within
1e-9 relative, exactly 0, the same NaN and the same infinity where the oracle gives one.  Unscaled euclidean and cosine are int64
sums and equal ``kpal_profile_distance_device`` bit for bit; smoothed option sets equal the pair entry bit for bit (the same
pipeline on the same tables).

How the library decides (n = 4^k bins): n <= 4096 (k <= 6) -> the wave form, a unit of work is four pairs, one per wave; else
the slice form, a unit is one (pair, slice of 2^16 bins) item -- k = 8 is exactly one slice, k = 9 four.  8 workgroups per CU
take the units round robin."""
import ctypes
import os

import numpy as np
import pytest

import matrix_cases
import option_cases
import oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
METRICS = ('prod', 'sum', 'euclidean', 'cosine')
SUMMARY = {'min': 0, 'average': 1, 'median': 2}
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PAIRED_KERNELS = ('pair_set', 'pair_set_totals')
E_INVALID = -1


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


@pytest.fixture(scope='module')
def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def options(do_balance=False, do_positive=False, do_scale=False, down=False, metric='prod', do_smooth=False, summary='min', threshold=0):
    """(kpal_distance_options, the oracle's keyword arguments) of one option set."""
    from kpal_amd import _native
    native = _native.DistanceOptions(do_balance=int(do_balance), do_positive=int(do_positive), do_smooth=int(do_smooth), summary=SUMMARY[summary],
                                     threshold=float(threshold), do_scale=int(do_scale), down=int(down), metric=METRICS.index(metric))
    kwargs = dict(do_balance=do_balance, do_positive=do_positive, do_smooth=do_smooth, summary=summary, threshold=threshold,
                  do_scale=do_scale, down=down, metric=metric)
    return native, kwargs


def oracle_pairs(left, right, k, kwargs):
    plain = not (kwargs['do_positive'] or kwargs['do_smooth'] or kwargs['do_scale']) and kwargs['metric'] != 'cosine'
    with np.errstate(all='ignore'):
        if plain:
            return np.array([oracle.distance(l, r, k, kwargs['do_balance'], kwargs['metric']) for l, r in zip(left, right)], dtype=np.float64)
        return np.array([oracle.profile_distance(l, r, k, **kwargs) for l, r in zip(left, right)], dtype=np.float64)


def assert_matches_oracle(got, want, exact, what):
    """test_gpu_cross.assert_matches_oracle: ``exact`` (unscaled euclidean) bit for bit, else NaN where the oracle has NaN, the
    same infinity, exactly 0 where it has 0, and 1e-9 relative everywhere else."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    if exact:
        np.testing.assert_array_equal(got, want, err_msg=str(what))
        return
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (what, 'NaN', np.flatnonzero(np.isnan(got) != nan)[:8])
    inf = np.isinf(want)
    assert (got[inf] == want[inf]).all(), (what, 'inf', np.flatnonzero(inf & (got != want))[:8])
    zero = want == 0
    assert (got[zero] == 0).all(), (what, 'zero', np.flatnonzero(zero & (got != 0))[:8])
    fin = np.isfinite(want) & ~zero
    rel = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    assert rel.size == 0 or rel.max() <= RTOL, (what, float(rel.max()), int(np.flatnonzero(fin)[rel.argmax()]))


def exact_for(kwargs):
    return kwargs['metric'] == 'euclidean' and not kwargs['do_scale']


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


class on_device(object):
    """``tables`` (any number of int64[4^k] rows) one behind the other in a device allocation, freed at the end: its address."""

    def __init__(self, ctx, tables):
        self.ctx, self.tables = ctx, np.ascontiguousarray(tables, dtype=np.int64)

    def __enter__(self):
        self.ptr = self.ctx.alloc(self.tables.nbytes)
        self.ctx.h2d(self.ptr, self.tables)
        return self.ptr

    def __exit__(self, *exc):
        self.ctx.sync()
        self.ctx.free(self.ptr)


def paired(ctx, left, right, k, native, chunk_pairs=0):
    """The device entry on left and right stacked in one allocation."""
    left, right = np.asarray(left), np.asarray(right)
    n = left.shape[0]
    with on_device(ctx, np.concatenate([left, right])) as dev:
        return ctx.paired_distance_device(k, n, dev, dev + left.nbytes, native, chunk_pairs)


def plain_sets(k, N, seed=None):
    prof = matrix_cases.build('plain', k, max(8, 2 * N), seed=seed).profiles
    return prof[:N], prof[N:2 * N]


PLAIN = [dict(metric=m, do_balance=b) for m in ('prod', 'sum', 'euclidean') for b in (False, True)]


@pytest.mark.parametrize('N', (1, 2, 3, 4, 5, 63, 64, 65, 257))
def test_shapes_k6(ctx, N):
    """The wave form: four pairs a workgroup, a ragged last workgroup unless four divides N; pair 0 is (profile 0, profile N)."""
    left, right = plain_sets(6, N)
    for o in PLAIN:
        native, kwargs = options(**o)
        got = ctx.paired_distance(left, right, 6, native)
        assert_matches_oracle(got, oracle_pairs(left, right, 6, kwargs), exact_for(kwargs), (N, o))


@pytest.mark.parametrize('k', (1, 2, 3, 5, 8, 9))
def test_table_sizes(ctx, k):
    """k = 1 .. 3: 2, 8 and 32 loads of 16 bytes for a wave of 64 lanes (the tail alone); k = 5: two whole rounds a lane; k = 8:
    exactly one slice; k = 9: four slices, the first reduction over more than one partial.  Pairs (0, 1) -- identical, exactly 0
    --, (2, 3) -- one bin apart --, the all-zero profile against itself and against another, and three ordinary pairs."""
    if k == 1:      # four bins: below matrix_cases' smallest table; the same degenerate rows
        prof = np.random.RandomState(1).randint(0, 120, (10, 4)).astype(np.int64)
        prof[1], prof[3], prof[8] = prof[0], prof[2], 0
        prof[3, 1] += 1
    else:
        prof = matrix_cases.build('plain', k, 10).profiles
    li, ri = [0, 2, 8, 8, 4, 5, 6], [1, 3, 8, 9, 7, 9, 2]
    left, right = prof[li], prof[ri]
    for o in PLAIN:
        native, kwargs = options(**o)
        want = oracle_pairs(left, right, k, kwargs)
        assert want[0] == 0 and want[2] == 0
        for got in (ctx.paired_distance(left, right, k, native), paired(ctx, left, right, k, native)):
            assert_matches_oracle(got, want, exact_for(kwargs), (k, o))


def test_k12_sampled(ctx):
    """Three pairs at k = 12 (256 slices each): the identical pair, the one-bin pair, an ordinary one."""
    k = 12
    prof = matrix_cases.build('plain', k, 8, seed=77).profiles
    left, right = prof[[0, 2, 4]], prof[[1, 3, 5]]
    # (the oracle balances copies inside every pair: its own balance of each table once, then its plain pair function, is the
    # same statement and a third of the time)
    balanced = [np.stack([oracle.balance(v, k) for v in side]) for side in (left, right)]
    with on_device(ctx, np.concatenate([left, right])) as dev:
        for o in PLAIN:
            native, kwargs = options(**o)
            got = ctx.paired_distance_device(k, 3, dev, dev + left.nbytes, native)
            l, r = balanced if o['do_balance'] else (left, right)
            assert_matches_oracle(got, oracle_pairs(l, r, k, dict(kwargs, do_balance=False)), exact_for(kwargs), (k, o))


def test_more_units_than_the_persistent_grid(ctx, num_cu):
    """k = 4 (256 bins, the wave form): 8 workgroups a CU take the units of four pairs round robin; two rounds and three units
    over, and a last unit of one pair.  The pairs repeat 61 distinct ones, so the oracle runs 61 times a metric."""
    k, distinct = 4, 61
    slots = 8 * num_cu
    units = 2 * slots + 3
    N = 4 * (units - 1) + 1
    rounds = -(-units // slots)
    assert rounds == 3 and -(-units // rounds) < units      # the planned grid is smaller than the units: workgroups loop
    base_l, base_r = plain_sets(k, distinct, seed=5)
    pick = np.arange(N) % distinct
    left, right = base_l[pick], base_r[pick]
    with on_device(ctx, np.concatenate([left, right])) as dev:
        for o in (dict(metric='prod'), dict(metric='euclidean', do_balance=True), dict(metric='sum', do_scale=True, do_positive=True)):
            native, kwargs = options(**o)
            got, names = launched(ctx, lambda: ctx.paired_distance_device(k, N, dev, dev + left.nbytes, native))
            assert names.get('pair_set') == 1, names
            want = oracle_pairs(base_l, base_r, k, kwargs)
            assert_matches_oracle(got, want[pick], exact_for(kwargs), (N, o))
            assert np.array_equal(got.view(np.uint64), got[:distinct][pick].view(np.uint64)), o      # equal pairs, equal bits, wherever they lie


VALUE_KINDS = ('neg_small', 'neg_large', 'int64_extreme', 'max_65535', 'max_65536', 'max_2p31m1', 'max_2p31', 'norm_2p53m1', 'norm_2p53')


@pytest.mark.parametrize('kind', VALUE_KINDS)
def test_value_edges(ctx, kind):
    """Every boundary set of matrix_cases at k = 6, pairs through the boundary profiles h = P // 2 and h + 1: the identical
    pair (0, 1), the all-zero profile against itself and another, the pairs wrap_visible names, and the profile with the -1
    (int64_extreme: infinity under 'prod')."""
    P = 12
    case = matrix_cases.build(kind, 6, P)
    h, prof = P // 2, case.profiles
    if kind == 'int64_extreme':
        matrix_cases.wrap_visible(case)
    li = [0, P - 2, P - 2, h, h + 1, h + 1, P - 1, P - 1, 2, h, 5]
    ri = [1, P - 2, 3, 0, 0, h, 0, h, 3, h + 1, h]
    left, right = prof[li], prof[ri]
    for o in PLAIN + [dict(metric='cosine'), dict(do_scale=True), dict(do_positive=True, metric='sum'), dict(do_scale=True, do_positive=True, metric='euclidean')]:
        native, kwargs = options(**o)
        want = oracle_pairs(left, right, 6, kwargs)
        if not (kwargs['do_scale'] or kwargs['metric'] == 'cosine'):
            assert want[0] == 0 and want[1] == 0, (kind, o)
        if kind == 'int64_extreme' and o == dict(metric='prod', do_balance=False):
            assert np.isinf(want[6]) and np.isinf(want[7])
        assert_matches_oracle(ctx.paired_distance(left, right, 6, native), want, exact_for(kwargs), (kind, o))


@pytest.mark.parametrize('k', (4, 6))
def test_option_grid(ctx, k):
    """All 48 option sets on the nine `negative` and `totals` pairs of option_cases, stacked as one set: negative factors, zero
    totals on either side, wrapping totals."""
    cases = [option_cases.build('negative', k, variant=v) for v in option_cases.NEGATIVE_VARIANTS]
    cases += [option_cases.build('totals', k, variant=v) for v in option_cases.TOTALS_VARIANTS]
    left, right = np.stack([c.left for c in cases]), np.stack([c.right for c in cases])
    with on_device(ctx, np.concatenate([left, right])) as dev:
        for o in option_cases.GRID:
            native, kwargs = options(**o)
            got = ctx.paired_distance_device(k, len(cases), dev, dev + left.nbytes, native)
            assert_matches_oracle(got, oracle_pairs(left, right, k, kwargs), exact_for(kwargs), (k, o))


def test_reference_goldens(ctx):
    """The G13 records of k = 4, stacked as one set: every distance the reference recorded without smoothing."""
    k = 4
    goldens = [g for g in option_cases.load_golden(GOLDEN_DIR) if g.k == k]
    assert len(goldens) >= 9
    left, right = np.stack([g.left for g in goldens]), np.stack([g.right for g in goldens])
    recorded = {}
    for i, g in enumerate(goldens):
        for kwargs, value in g.distances:
            if not kwargs.get('do_smooth'):
                recorded.setdefault(tuple(sorted(kwargs.items())), []).append((i, value))
    assert len(recorded) == 48
    compared = 0
    with on_device(ctx, np.concatenate([left, right])) as dev:
        for key, values in sorted(recorded.items()):
            native, kwargs = options(**dict(key))
            got = ctx.paired_distance_device(k, len(goldens), dev, dev + left.nbytes, native)
            at = [i for i, _ in values]
            assert_matches_oracle(got[at], np.array([v for _, v in values]), False, dict(key))
            compared += len(at)
    assert compared >= 48 * 9


@pytest.mark.parametrize('k,N', [(6, 9), (9, 3)])
def test_int64_sums_are_the_pair_entry_bit_for_bit(ctx, k, N):
    left, right = plain_sets(k, N, seed=31)
    table = 8 * 4 ** k
    with on_device(ctx, np.concatenate([left, right])) as dev:
        for metric in ('euclidean', 'cosine'):
            for o in (dict(), dict(do_balance=True), dict(do_positive=True), dict(do_positive=True, do_balance=True)):
                native, _ = options(metric=metric, **o)
                got = ctx.paired_distance_device(k, N, dev, dev + left.nbytes, native)
                pairs = np.array([ctx.profile_distance_device(k, dev + i * table, dev + left.nbytes + i * table, native) for i in range(N)])
                assert np.array_equal(got.view(np.uint64), pairs.view(np.uint64)), (k, metric, o)


def test_smoothing_is_the_pair_entry(ctx):
    """do_smooth: the pair pipeline per pair on tables balanced once -- the bits of kpal_profile_distance."""
    k = 8
    cases = option_cases.edge_cases(k)[:3]
    left, right = np.stack([c.left for c in cases]), np.stack([c.right for c in cases])
    for o in (dict(do_smooth=True, summary=cases[0].summary, threshold=cases[0].threshold),
              dict(do_smooth=True, summary='average', threshold=cases[1].threshold, do_scale=True, do_balance=True),
              dict(do_smooth=True, summary='median', threshold=cases[2].threshold, do_positive=True, metric='cosine')):
        native, _ = options(**o)
        got, names = launched(ctx, lambda: paired(ctx, left, right, k, native))
        pairs = np.array([ctx.profile_distance(l, r, k, native) for l, r in zip(left, right)])
        assert np.array_equal(got.view(np.uint64), pairs.view(np.uint64)), o
        assert names.get('smooth_apply') == 3 and not set(names) & set(PAIRED_KERNELS), names
        if o.get('do_balance'):
            assert names.get('balance_tiled_set') == 2 and 'balance_tiled' not in names, names      # once per side, not per pair


@pytest.mark.parametrize('k,N', [(6, 23), (9, 9)])
def test_a_pair_does_not_depend_on_its_set(ctx, k, N):
    """The bits of pair i: in the whole set, alone, at another position (the set reversed), and under chunk_pairs 1 and 7."""
    left, right = plain_sets(k, N, seed=13)
    right[3] = np.roll(left[3], 1)                       # equal totals
    table = 8 * 4 ** k
    with on_device(ctx, np.concatenate([left, right, left[::-1], right[::-1]])) as dev:
        dl, dr, rl, rr = (dev + i * left.nbytes for i in range(4))
        for o in (dict(), dict(do_scale=True, down=True), dict(do_positive=True, do_scale=True), dict(metric='cosine'),
                  dict(do_balance=True, metric='sum')):
            native, _ = options(**o)
            whole = ctx.paired_distance_device(k, N, dl, dr, native).view(np.uint64)
            for i in (0, 3, N // 2, N - 1):
                alone = ctx.paired_distance_device(k, 1, dl + i * table, dr + i * table, native).view(np.uint64)
                assert alone[0] == whole[i], (k, o, i)
            assert np.array_equal(ctx.paired_distance_device(k, N, rl, rr, native).view(np.uint64), whole[::-1]), (k, o)
            for chunk in (1, 7):
                got, names = launched(ctx, lambda: ctx.paired_distance_device(k, N, dl, dr, native, chunk))
                assert np.array_equal(got.view(np.uint64), whole), (k, o, chunk)
                assert names.get('pair_set') == -(-N // chunk), (chunk, names)


def test_aliasing(ctx):
    """A set against itself: zeros, NaN where the pair entry gives NaN (the all-zero profile under -S).  The same set one and
    three tables on: the oracle's values, with and without the balance.  The inputs are not written."""
    k, N = 6, 12
    prof = matrix_cases.build('plain', k, N, seed=3).profiles
    table = 8 * 4 ** k
    with on_device(ctx, prof) as dev:
        for o in PLAIN + [dict(metric='cosine', do_positive=True), dict(do_scale=True), dict(do_scale=True, do_balance=True, metric='euclidean')]:
            native, kwargs = options(**o)
            got = ctx.paired_distance_device(k, N, dev, dev, native)
            want = oracle_pairs(prof, prof, k, kwargs)
            if kwargs['metric'] != 'cosine':
                assert ((want == 0) | np.isnan(want)).all(), o
            if kwargs['do_scale']:
                assert np.isnan(want[N - 2])
            assert_matches_oracle(got, want, exact_for(kwargs), ('self', o))
            for lag in (1, 3):
                want = oracle_pairs(prof[:N - lag], prof[lag:], k, kwargs)
                assert_matches_oracle(ctx.paired_distance_device(k, N - lag, dev, dev + lag * table, native), want, exact_for(kwargs), (lag, o))
                assert_matches_oracle(ctx.paired_distance_device(k, N - lag, dev + lag * table, dev, native), want, exact_for(kwargs), (-lag, o))
        # half a table apart: no shortcut, the values of the overlapping tables as they lie
        rows = np.concatenate([prof, prof[:1]]).reshape(-1)
        half = 4 ** k // 2
        shifted = rows[half:half + (N - 1) * 4 ** k].reshape(N - 1, 4 ** k)
        native, kwargs = options(do_balance=True, do_scale=True)
        got = ctx.paired_distance_device(k, N - 1, dev, dev + table // 2, native)
        assert_matches_oracle(got, oracle_pairs(prof[:N - 1], shifted, k, kwargs), False, 'half a table')
        after = np.empty_like(prof)
        ctx.d2h(after, dev)
    np.testing.assert_array_equal(after, prof)


def test_launches_do_not_grow_with_the_set(ctx):
    k = 6
    table = 8 * 4 ** k
    seen = {}
    for N in (5, 300):
        left, right = plain_sets(k, N, seed=9)
        with on_device(ctx, np.concatenate([left, right])) as dev:
            for name, o in (('plain', dict()), ('scale', dict(do_scale=True)), ('positive + scale', dict(do_positive=True, do_scale=True, metric='cosine')),
                            ('balance', dict(do_balance=True, metric='sum'))):
                native, _ = options(**o)
                _, names = launched(ctx, lambda: ctx.paired_distance_device(k, N, dev, dev + left.nbytes, native))
                seen.setdefault(name, []).append(names)
            native, _ = options(do_balance=True)
            _, names = launched(ctx, lambda: ctx.paired_distance_device(k, N - 1, dev, dev + table, native))
            assert names == {'balance_tiled_set': 1, 'pair_set': 1, 'reduce_partials': 1}, names      # the union of the two ranges once
            _, names = launched(ctx, lambda: ctx.paired_distance_device(k, N, dev, dev, native))
            assert names == {'balance_tiled_set': 1, 'pair_set': 1, 'reduce_partials': 1}, names
    assert seen['plain'] == [{'pair_set': 1, 'reduce_partials': 1}] * 2, seen['plain']
    assert seen['scale'] == [{'pair_set_totals': 1, 'pair_set': 1, 'reduce_partials': 2}] * 2, seen['scale']
    assert seen['positive + scale'] == [{'pair_set_totals': 1, 'pair_set': 1, 'reduce_partials': 2}] * 2, seen['positive + scale']
    assert seen['balance'] == [{'balance_tiled_set': 2, 'pair_set': 1, 'reduce_partials': 1}] * 2, seen['balance']
    # below k = 6 a table has no 64 x 64 tile: the flat balance of the set, still one launch a side
    left, right = plain_sets(4, 9)
    native, _ = options(do_balance=True)
    _, names = launched(ctx, lambda: paired(ctx, left, right, 4, native))
    assert names == {'balance_set': 2, 'pair_set': 1, 'reduce_partials': 1}, names


def test_arguments(ctx):
    """Every refusal is KPAL_E_INVALID on the host: nothing is launched, nothing written."""
    from kpal_amd import _native
    k, N = 2, 3
    L, h = ctx._L, ctx._h
    host = [np.ascontiguousarray(np.arange(16, dtype=np.int64) + i) for i in range(2 * N)]
    out = np.full(N, -12345.5)
    outp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def opt(**kw):
        o = _native.DistanceOptions(0, 0, 0, 0, 0.0, 0, 0, 0)
        for name, v in kw.items():
            setattr(o, name, v)
        return ctypes.byref(o)

    def ptrs(rows, null_at=None):
        return (ctypes.c_void_p * N)(*[None if i == null_at else host[r].ctypes.data for i, r in enumerate(rows)])

    with on_device(ctx, np.concatenate(host + [host[0]])) as dev:
        right = dev + N * 128
        device = lambda k_=k, n=N, l=dev, r=right, o=None, chunk=0, res=outp: L.kpal_paired_distance_device(h, k_, n, l, r, o if o is not None else opt(), chunk, res)
        hostcall = lambda k_=k, n=N, l=None, r=None, o=None, res=outp: L.kpal_paired_distance(
            h, k_, n, l if l is not None else ptrs(range(N)), r if r is not None else ptrs(range(N, 2 * N)), o if o is not None else opt(), res)
        refusals = [
            (lambda: device(n=0), 'N must be >= 1'), (lambda: device(n=-4), 'N must be >= 1'),
            (lambda: device(k_=0), 'k=0 out of range'), (lambda: device(k_=17), 'k=17 out of range'),
            (lambda: L.kpal_paired_distance_device(h, k, N, None, right, opt(), 0, outp), 'NULL pointer'),
            (lambda: L.kpal_paired_distance_device(h, k, N, dev, None, opt(), 0, outp), 'NULL pointer'),
            (lambda: L.kpal_paired_distance_device(h, k, N, dev, right, opt(), 0, None), 'NULL pointer'),
            (lambda: device(l=dev + 8), 'device tables must be 16-byte aligned'), (lambda: device(r=right + 8), 'device tables must be 16-byte aligned'),
            (lambda: L.kpal_paired_distance_device(h, k, N, dev, right, None, 0, outp), 'options are NULL'),
            (lambda: device(o=opt(metric=4)), 'unknown metric 4'), (lambda: device(o=opt(do_smooth=1, summary=3)), 'unknown summary function 3'),
            (lambda: device(chunk=-1), 'chunk_pairs must be >= 0'),
            (lambda: device(k_=16, n=1 << 40), '1099511627776 pairs at k=16: too many bytes'),
            (lambda: hostcall(n=0), 'N must be >= 1'), (lambda: hostcall(k_=0), 'k=0 out of range'), (lambda: hostcall(k_=17), 'k=17 out of range'),
            (lambda: L.kpal_paired_distance(h, k, N, None, ptrs(range(N)), opt(), outp), 'NULL pointer'),
            (lambda: L.kpal_paired_distance(h, k, N, ptrs(range(N)), None, opt(), outp), 'NULL pointer'),
            (lambda: L.kpal_paired_distance(h, k, N, ptrs(range(N)), ptrs(range(N)), opt(), None), 'NULL pointer'),
            (lambda: L.kpal_paired_distance(h, k, N, ptrs(range(N)), ptrs(range(N)), None, outp), 'options are NULL'),
            (lambda: hostcall(o=opt(metric=-1)), 'unknown metric -1'),
            (lambda: hostcall(l=ptrs(range(N), null_at=1)), 'left profile 1 is NULL'), (lambda: hostcall(r=ptrs(range(N), null_at=2)), 'right profile 2 is NULL'),
            (lambda: hostcall(k_=16, n=1 << 29), '536870912 pairs at k=16: too many bytes'),
        ]
        for call, text in refusals:
            rc, names = launched(ctx, call)
            assert rc == E_INVALID and L.kpal_last_error().decode() == text, (rc, text, L.kpal_last_error().decode())
            assert names == {}, (text, names)
        assert (out == -12345.5).all()
        assert device() == 0 and hostcall() == 0
    with pytest.raises(ValueError):
        ctx.paired_distance(host[:2], host[:3], k, _native.DistanceOptions(0, 0, 0, 0, 0.0, 0, 0, 0))
