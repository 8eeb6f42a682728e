"""The summaries and the strand balance of whole SETS of profiles on the GPU (kpal_stats_set_device,
kpal_strand_balance_set_device; klib.summaries, klib.strand_balances; kpal/klib.py:193-225, kpal/kmer.py:243-245) against the
oracle per table: integers and the median exact, mean and std within 1e-9 relative, the balance score within 1e-9.  A table's
summary does not depend on the set it is in (bit for bit), the launches do not grow with the set, and profiles that are still
in HBM stay there.  Run on the GPU box: pytest -m gpu."""
import ctypes
import io
import math
import random

import numpy as np
import pytest

import memh5
import oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
SINGLE_STATS_KERNELS = ('stats', 'stats_var', 'select_hist', 'select_next')


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


class on_device(object):
    """The rows of a 2-d int64 array as consecutive tables in device memory."""

    def __init__(self, ctx, tables):
        self.ctx, self.tables = ctx, np.ascontiguousarray(tables, dtype=np.int64)

    def __enter__(self):
        self.ptr = self.ctx.alloc(self.tables.nbytes)
        self.ctx.h2d(self.ptr, self.tables)
        return self.ptr

    def __exit__(self, *exc):
        self.ctx.sync()
        self.ctx.free(self.ptr)


def launches(ctx, call):
    """(result, {kernel name: launches}) of ``call()``"""
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        result = call()
        seen = dict((name, count) for name, (_, count) in ctx.prof_get().items() if count)
    finally:
        ctx.prof_enable(False)
    return result, seen


def check_stats(got, want, what, v):
    """The rules of the single-profile summaries (tests/test_gpu_stats.py), restated."""
    assert (got.total, got.non_zero, got.min, got.max) == (want['total'], want['non_zero'], want['min'], want['max']), what
    assert got.median == want['median'], (what, got.median, want['median'])
    # mean: 1e-9 relative to the magnitude of the data (for counts, which are >= 0, that is 1e-9 relative)
    scale = float(np.abs(v.astype(np.float64)).mean())
    assert abs(got.mean - want['mean']) <= RTOL * scale + 1e-300, (what, 'mean', got.mean, want['mean'])
    assert abs(got.std - want['std']) <= RTOL * abs(want['std']) + 1e-300, (what, 'std', got.std, want['std'])


KINDS = ('poisson', 'zeros', 'constant', 'one', 'heavy', 'negative', 'wide', 'wrapping')


def make_table(rs, bins, kind):
    if kind == 'poisson':
        return rs.poisson(rs.choice([0.02, 0.7, 3.0, 800.0]), bins).astype(np.int64)
    if kind == 'zeros':
        return np.zeros(bins, dtype=np.int64)
    if kind == 'constant':
        return np.full(bins, 7, dtype=np.int64)
    if kind == 'one':
        v = np.zeros(bins, dtype=np.int64)
        v[rs.randint(0, bins)] = 5
        return v
    if kind == 'heavy':   # a few 10^12 among small counts: five select bytes where a Poisson neighbour needs one or two
        v = rs.poisson(1.5, bins).astype(np.int64)
        v[rs.randint(0, bins, max(1, bins // 300))] = 10 ** 12
        return v
    if kind == 'negative':
        return rs.randint(-10 ** 6, 10 ** 6, size=bins).astype(np.int64)
    if kind == 'wide':
        return rs.randint(-(1 << 62), 1 << 62, size=bins).astype(np.int64)
    assert kind == 'wrapping'
    return rs.randint(1 << 60, 1 << 62, size=bins).astype(np.int64)


def make_set(seed, bins, n, shift=0):
    """n tables of every kind in turn, the first of kind ``shift``: sets of different (n, shift) mix them in different places."""
    rs = np.random.RandomState(seed)
    kinds = [KINDS[(i + shift) % len(KINDS)] for i in range(n)]
    return np.stack([make_table(rs, bins, kind) for kind in kinds]), kinds


# ---- summaries against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 2, 65, 130))
@pytest.mark.parametrize('k', (1, 2, 3, 4, 5, 6, 8))
def test_stats_sets_vs_oracle(ctx, k, n):
    tables, kinds = make_set(100 * k + n, 4 ** k, n, shift=k + n)
    with on_device(ctx, tables) as ptr:
        got = ctx.stats_set_device(ptr, n, 4 ** k)
    assert len(got) == n
    for i in range(n):
        check_stats(got[i], oracle.stats(tables[i]), (k, n, i, kinds[i]), tables[i])


def test_stats_set_k10(ctx):
    tables, kinds = make_set(10, 4 ** 10, 3, shift=4)            # heavy, negative, wide: 128 slices each
    with on_device(ctx, tables) as ptr:
        got = ctx.stats_set_device(ptr, 3, 4 ** 10)
    for i in range(3):
        check_stats(got[i], oracle.stats(tables[i]), (10, i, kinds[i]), tables[i])


@pytest.mark.parametrize('bins', (1, 1001, 8193))
def test_stats_set_of_any_length_through_the_host_entry(ctx, bins):
    """The C-ABI takes any bins >= 1: shorter than a wave, no multiple of the workgroup, one entry into a second slice; tables
    at odd multiples of 8 bytes."""
    tables, kinds = make_set(bins, bins, 9, shift=3)
    got = ctx.stats_set(tables)
    for i in range(9):
        check_stats(got[i], oracle.stats(tables[i]), (bins, i, kinds[i]), tables[i])
        assert got[i].median == float(np.median(tables[i]))
    with on_device(ctx, tables) as ptr:
        same = ctx.stats_set_device(ptr, 9, bins)
    assert bytes(same) == bytes(got)


def test_position_independence(ctx):
    """One table at the front, in the middle and at the end of different sets, and alone: the same bytes.  Two calls: too."""
    bins = 4 ** 7                                              # two slices
    table = make_table(np.random.RandomState(5), bins, 'heavy')
    seen = []
    for n, at, shift in ((5, 0, 0), (9, 4, 3), (4, 3, 6), (1, 0, 0)):
        tables, _ = make_set(50 + n, bins, n, shift)
        tables[at] = table
        with on_device(ctx, tables) as ptr:
            got = ctx.stats_set_device(ptr, n, bins)
            again = ctx.stats_set_device(ptr, n, bins)
        assert bytes(got) == bytes(again)
        seen.append(bytes(got[at]))
    assert len(set(seen)) == 1 and len(seen[0]) == ctypes.sizeof(type(got[0])) == 56
    check_stats(got[0], oracle.stats(table), 'alone', table)


def test_chunk_seam(ctx, monkeypatch):
    """n = 20 in passes of 7, 7 and 6 profiles gives the bytes of one pass, for the summaries and for the strand balance."""
    k, n = 6, 20
    tables, _ = make_set(77, 4 ** k, n, shift=2)
    with on_device(ctx, tables) as ptr:
        whole, whole_launches = launches(ctx, lambda: ctx.stats_set_device(ptr, n, 4 ** k))
        balance = ctx.strand_balance_set_device(k, n, ptr)
        monkeypatch.setenv('KPAL_STAT_SET_PROFILES', '7')
        cut, cut_launches = launches(ctx, lambda: ctx.stats_set_device(ptr, n, 4 ** k))
        balance_cut, balance_launches = launches(ctx, lambda: ctx.strand_balance_set_device(k, n, ptr))
        monkeypatch.delenv('KPAL_STAT_SET_PROFILES')
    assert bytes(cut) == bytes(whole)
    assert balance_cut.tobytes() == balance.tobytes()
    assert cut_launches['stats_set'] == 3 and whole_launches['stats_set'] == 1      # the cap was read on that call, and only there
    assert balance_launches == {'strand_balance_tiled_set': 3, 'reduce_partials': 3}


# ---- launches ------------------------------------------------------------------------------------------------------------
def test_launch_structure(ctx):
    """5 and 300 tables of one count range: the same launches, none of the single-profile kernels, at most 3 per digit + 8."""
    k = 6
    seen = []
    for n in (5, 300):
        rs = np.random.RandomState(n)
        tables = rs.poisson(700.0, (n, 4 ** k)).astype(np.int64)
        tables[:, 0], tables[:, 1] = 3, 1500                     # min and max differ in the second byte: two digits everywhere
        assert tables.min() >= 0 and tables.max() < 65536 and tables.max() >= 256
        with on_device(ctx, tables) as ptr:
            got, stats_launches = launches(ctx, lambda: ctx.stats_set_device(ptr, n, 4 ** k))
            scores, balance_launches = launches(ctx, lambda: ctx.strand_balance_set_device(k, n, ptr))
        assert got[n - 1].median == float(np.median(tables[n - 1]))
        assert abs(scores[n - 1] - oracle.strand_balance(tables[n - 1], k)) <= RTOL * abs(scores[n - 1])
        assert balance_launches == {'strand_balance_tiled_set': 1, 'reduce_partials': 1}
        seen.append(stats_launches)
    assert seen[0] == seen[1], seen
    assert not any(name in seen[0] for name in SINGLE_STATS_KERNELS), seen[0]
    digits = seen[0]['select_hist_set']
    assert digits == 2 and seen[0]['stats_set'] == 1 and seen[0]['var_set'] == 1
    assert sum(seen[0].values()) <= 3 * digits + 8, seen[0]


# ---- strand balance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (1, 3, 70))
@pytest.mark.parametrize('k', (1, 2, 3, 4, 5, 6, 7, 8))
def test_strand_balance_sets_vs_oracle(ctx, k, n):
    """Odd and even k; k = 5 the last untiled one, k = 6 one tile, k = 7 four tiles with self-paired and mirrored ones."""
    rs = np.random.RandomState(1000 * k + n)
    tables = np.stack([rs.poisson(rs.choice([0.3, 2.0, 40.0]), 4 ** k) for _ in range(n)]).astype(np.int64)
    tables[(n - 1) // 2] = 0                                   # a table of zeros among them
    with on_device(ctx, tables) as ptr:
        for pairwise, native in (('prod', 0), ('sum', 1)):
            got = ctx.strand_balance_set_device(k, n, ptr, native)
            assert got.shape == (n,) and got.dtype == np.float64
            for i in range(n):
                want = oracle.strand_balance(tables[i], k, pairwise)
                if math.isnan(want):
                    assert math.isnan(got[i]), (k, n, i, pairwise)
                else:
                    assert abs(got[i] - want) <= RTOL * abs(want), (k, n, i, pairwise, got[i], want)


def test_host_pointer_entries_equal_the_device_entries(ctx):
    k, n = 7, 6
    tables, _ = make_set(9, 4 ** k, n, shift=5)
    counts = np.abs(tables) % 1000
    with on_device(ctx, tables) as ptr:
        assert bytes(ctx.stats_set(tables)) == bytes(ctx.stats_set_device(ptr, n, 4 ** k))
    with on_device(ctx, counts) as ptr:
        for native in (0, 1):
            assert ctx.strand_balance_set(counts, k, native).tobytes() == ctx.strand_balance_set_device(k, n, ptr, native).tobytes()
    # and a single table gives what the single-profile entry gives for it, exactly where both are exact
    one = ctx.stats(tables[2])
    got = ctx.stats_set(tables[2:3])[0]
    assert (got.total, got.non_zero, got.min, got.max, got.median, got.mean) == (one.total, one.non_zero, one.min, one.max, one.median, one.mean)


def test_single_strand_balance_is_the_set_entry_with_one_table(ctx):
    """kpal_strand_balance is kpal_strand_balance_set with one table: the same bits as the table alone in a set and as its row
    in a set of five, for both pairwise codes -- k = 1 to 5 untiled (one workgroup up to k = 4, four at k = 5), k = 6 one tile,
    k = 7 four tiles, k = 8 sixteen; a table of zeros at k = 3 and k = 6 -- and the same launches."""
    for k in range(1, 9):
        rs = np.random.RandomState(40 + k)
        tables = rs.poisson(rs.choice([0.3, 2.0, 40.0]), (5, 4 ** k)).astype(np.int64)
        if k in (3, 6):
            tables[2] = 0
        for native in (0, 1):
            five = ctx.strand_balance_set(tables, k, native)
            for i in (0, 2, 4):
                v = tables[i]
                one, seen = launches(ctx, lambda: ctx.strand_balance(v, k, native))
                alone, seen_set = launches(ctx, lambda: ctx.strand_balance_set(v[None], k, native))
                assert np.float64(one).tobytes() == alone.tobytes() == five[i:i + 1].tobytes(), (k, native, i, one, alone, five[i])
                assert seen == seen_set == {'strand_balance_tiled_set' if k >= 6 else 'strand_balance_set': 1, 'reduce_partials': 1}
    # the single entry refuses what the set entry refuses, before anything is launched: a table that is not 8-byte aligned
    from kpal_amd import _native
    raw = np.zeros(8 * 16 + 16, dtype=np.uint8)
    at = raw.ctypes.data + (4 if raw.ctypes.data % 8 == 0 else 8 - raw.ctypes.data % 8 + 4)
    out = ctypes.c_double(0.0)
    rc, seen = launches(ctx, lambda: ctx._L.kpal_strand_balance(ctx._h, 2, at, 0, ctypes.byref(out)))
    assert rc == _native._E_INVALID and seen == {}


def test_errors(ctx):
    """Every misuse is KPAL_E_INVALID (a ValueError), decided before anything is launched."""
    from kpal_amd import _native
    L, h = ctx._L, ctx._h
    tables = np.arange(2 * 256, dtype=np.int64).reshape(2, 256)
    out = (_native.ProfileStats * 2)()
    scores = np.zeros(2)
    f64p = scores.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    with on_device(ctx, tables) as ptr:
        def stats_calls():
            for entry, where in ((L.kpal_stats_set_device, ptr), (L.kpal_stats_set, tables.ctypes.data)):
                yield entry(None, 2, 256, where, out)
                yield entry(h, 2, 256, None, out)
                yield entry(h, 2, 256, where, None)
                yield entry(h, 0, 256, where, out)
                yield entry(h, 2, 0, where, out)
                yield entry(h, 1, 256, where + 4, out)
            for entry, where in ((L.kpal_strand_balance_set_device, ptr), (L.kpal_strand_balance_set, tables.ctypes.data)):
                yield entry(None, 4, 2, where, 0, f64p)
                yield entry(h, 4, 2, None, 0, f64p)
                yield entry(h, 4, 2, where, 0, None)
                yield entry(h, 4, 0, where, 0, f64p)
                yield entry(h, 0, 2, where, 0, f64p)
                yield entry(h, _native.KPAL_MAX_K + 1, 2, where, 0, f64p)
                yield entry(h, 4, 2, where, 2, f64p)
                yield entry(h, 4, 2, where, -1, f64p)
                yield entry(h, 4, 1, where + 4, 0, f64p)
        codes, seen = launches(ctx, lambda: list(stats_calls()))
        assert len(codes) == 30 and all(rc != 0 for rc in codes), codes
        for rc in codes:
            with pytest.raises(ValueError):
                _native._check(rc)
        assert seen == {}
        # the Python layer names its own
        with pytest.raises(ValueError):
            ctx.stats_set(np.zeros((0, 4), dtype=np.int64))
        with pytest.raises(ValueError):
            ctx.stats_set(np.zeros(16, dtype=np.int64))
        with pytest.raises(ValueError):
            ctx.strand_balance_set(np.zeros((2, 15), dtype=np.int64), 2)
        with pytest.raises(TypeError):
            ctx.stats_set(np.zeros((2, 16)))
        # and the entries still work afterwards
        assert ctx.stats_set_device(ptr, 2, 256)[1].total == int(tables[1].sum())


# ---- profiles ------------------------------------------------------------------------------------------------------------
def fasta_text(rnd, n, k):
    """n short records, some shorter than k."""
    out = []
    for i in range(n):
        length = rnd.choice([0, 1, k - 1, k, k + 1, 30, 80, 200])
        out.append('>rec%d some words\n%s\n' % (i, ''.join(rnd.choice('ACGTACGTN') for _ in range(length))))
    return ''.join(out).encode()


def fastq_text(rnd, n):
    out = []
    for i in range(n):
        length = rnd.choice([0, 2, 5, 40, 120])
        seq = ''.join(rnd.choice('ACGTACGTN') for _ in range(length))
        out.append('@read%d\n%s\n+\n%s\n' % (i, seq, 'I' * length))
    return ''.join(out).encode()


def same_summary(got, want, what):
    assert sorted(got) == sorted(want) == ['mean', 'median', 'non_zero', 'std', 'total'], what
    for key in got:
        assert type(got[key]) is type(want[key]), (what, key, type(got[key]), type(want[key]))
    assert (got['total'], got['non_zero'], got['median']) == (want['total'], want['non_zero'], want['median']), what
    assert abs(got['mean'] - want['mean']) <= RTOL * abs(want['mean']) + 1e-300, (what, got['mean'], want['mean'])
    assert abs(got['std'] - want['std']) <= RTOL * abs(want['std']) + 1e-300, (what, got['std'], want['std'])


@pytest.fixture(scope='module')
def record_profiles():
    """-> make(which): 70 fresh device-resident profiles at k = 4, of a FASTA text ('fasta') or of FASTQ reads ('fastq')."""
    from kpal_amd import klib
    texts = {'fasta': fasta_text(random.Random(4), 70, 4), 'fastq': fastq_text(random.Random(5), 70)}

    def make(which):
        if which == 'fasta':
            return list(klib.Profile.from_fasta_by_record(io.BytesIO(texts[which]), 4))
        return list(klib.Profile.from_fastq_by_record(io.BytesIO(texts[which]), 4))
    return make


@pytest.mark.parametrize('which', ('fasta', 'fastq'))
def test_summaries_of_device_profiles(ctx, record_profiles, which):
    from kpal_amd import klib
    ps, copies = record_profiles(which), record_profiles(which)
    assert len(ps) == 70 and all(p._device_counts() is not None for p in ps)
    (got, scores), seen = launches(ctx, lambda: (klib.summaries(ps), klib.strand_balances(ps)))
    assert all(p._device_counts() is not None for p in ps)                           # nothing was downloaded
    assert not any(name in seen for name in SINGLE_STATS_KERNELS), seen
    batches = len(set(id(p._device[0]) for p in ps))                                 # (a batch per piece of the text the scan took)
    assert seen['stats_set'] == batches <= 2 and seen['strand_balance_set'] == 1, seen   # one set call per batch; one gathered set
    want = [klib.Profile(p.counts.copy()).summary() for p in copies]
    assert len(got) == 70 and isinstance(scores, list) and all(type(s) is float for s in scores)
    for i in range(70):
        same_summary(got[i], want[i], (which, i))
        balance = oracle.strand_balance(copies[i].counts, 4)
        assert (math.isnan(balance) and math.isnan(scores[i])) or abs(scores[i] - balance) <= RTOL * abs(balance), (which, i)
    # the properties of a profile that is still in HBM read the batch's one set call
    (_, seen) = launches(ctx, lambda: [(p.mean, p.std, p.median, p.total, p.non_zero) for p in ps])
    assert seen == {} and all(p._device_counts() is not None for p in ps)
    assert int(ps[7].total) == int(copies[7].counts.sum()) and ps[7].non_zero == np.count_nonzero(copies[7].counts)


def test_save_takes_the_summary_before_the_counts(ctx, record_profiles):
    """Saving 70 device profiles: one set call, no single-profile stats kernel, the attributes of host copies saved one by one."""
    from kpal_amd import klib
    ps, copies = record_profiles('fasta'), record_profiles('fasta')
    mine, theirs = memh5.File(), memh5.File()
    batches = len(set(id(p._device[0]) for p in ps))
    _, seen = launches(ctx, lambda: [p.save(mine) for p in ps])
    assert seen.get('stats_set') == batches <= 2 and not any(name in seen for name in SINGLE_STATS_KERNELS), seen
    for p in copies:
        klib.Profile(p.counts.copy(), name=p.name).save(theirs)
    assert sorted(mine['profiles']) == sorted(theirs['profiles']) and len(mine['profiles']) == 70
    for name in mine['profiles']:
        a, b = mine['profiles/' + name], theirs['profiles/' + name]
        np.testing.assert_array_equal(a[:], b[:])
        assert sorted(a.attrs) == sorted(b.attrs) == ['length', 'mean', 'median', 'non_zero', 'std', 'total']
        assert a.attrs['length'] == b.attrs['length'] == 4
        same_summary(dict((key, a.attrs[key]) for key in a.attrs if key != 'length'),
                     dict((key, b.attrs[key]) for key in b.attrs if key != 'length'), name)


def test_no_stale_summary_after_the_counts_were_handed_out(ctx, record_profiles):
    from kpal_amd import klib
    ps = record_profiles('fastq')
    p = next(q for q in ps if q.summary()['total'] > 0)
    before = p.summary()['total']
    p.counts[0] += 1
    assert p._device_counts() is None
    assert p.summary()['total'] == before + 1 and klib.summaries([p])[0]['total'] == before + 1
    p.counts[0] += 2
    assert klib.summaries([p, ps[0]])[0]['total'] == before + 3 and int(p.total) == before + 3


def test_mixed_lengths_and_a_float_profile_come_back_in_order(ctx, record_profiles):
    from kpal_amd import klib
    rs = np.random.RandomState(8)
    device = record_profiles('fasta')[10:13]
    k3 = [klib.Profile(rs.poisson(2.0, 4 ** 3).astype(np.int64), name='a%d' % i) for i in range(3)]
    k4 = [klib.Profile(rs.poisson(5.0, 4 ** 4).astype(np.int64), name='b%d' % i) for i in range(2)]
    scaled = klib.Profile(rs.poisson(5.0, 4 ** 3) * 0.37, name='scaled')
    mixed = [k3[0], k4[0], device[0], scaled, k3[1], device[2], k4[1], k3[2], device[1]]
    got, scores = klib.summaries(mixed), klib.strand_balances(mixed, 'sum')
    assert all(p._device_counts() is not None for p in device)
    for i, p in enumerate(mixed):
        counts = np.array(p.copy().counts)
        if p is scaled:
            want = klib.Profile(counts).summary()
            assert got[i] == want and isinstance(got[i]['total'], np.float64)
            forward, reverse = klib.Profile(counts).split()
            from kpal_amd import metrics
            assert scores[i] == float(metrics.multiset(forward, reverse, metrics.pairwise['sum']))
        else:
            same_summary(got[i], klib.Profile(counts).summary(), i)
            want = oracle.strand_balance(counts, p.length, 'sum')
            assert (math.isnan(want) and math.isnan(scores[i])) or abs(scores[i] - want) <= RTOL * abs(want), i
    assert klib.summaries([]) == [] and klib.strand_balances([]) == []


# ---- commands ------------------------------------------------------------------------------------------------------------
def test_commands_print_the_single_profile_lines(ctx, record_profiles):
    """``kpal showbalance``, ``stats`` and ``info`` on a store of the 70 profiles: every line is the one built from the single
    profile's ``mean``, ``std``, ``summary()`` and ``Context.strand_balance``, formatted as the command formats it."""
    from kpal_amd import klib, kmer
    handle = memh5.File()
    handle.attrs.update({'version': '1.0.0', 'producer': 'the test'})
    for p in record_profiles('fasta'):
        p.save(handle)
    names = sorted(handle['profiles'])
    assert len(names) == 70
    singles = [klib.Profile.from_file(handle, name=name) for name in names]

    def run(command, balance_calls=0, **kwargs):
        """The command's lines; it made one set call for all 70 profiles where it scores the balance, and none per profile."""
        out = io.StringIO()
        _, seen = launches(ctx, lambda: command(handle, out, **kwargs))
        assert not any(name in seen for name in SINGLE_STATS_KERNELS), seen
        assert seen.get('strand_balance_set', 0) + seen.get('strand_balance_tiled_set', 0) == balance_calls, seen
        return out.getvalue().split('\n')

    lines = run(kmer.get_balance, balance_calls=1, precision=10)
    assert len(lines) == 71 and lines[-1] == ''
    assert lines[:70] == ['%s %.10f' % (name, ctx.strand_balance(p.counts, 4, 0)) for name, p in zip(names, singles)]
    lines = run(kmer.get_stats, precision=10)
    assert len(lines) == 71
    assert lines[:70] == ['%s %.10f %.10f' % (name, p.mean, p.std) for name, p in zip(names, singles)]
    lines = run(kmer.get_stats, precision=3, names=names[5:7])
    assert lines == ['%s %.3f %.3f' % (name, p.mean, p.std) for name, p in zip(names[5:7], singles[5:7])] + ['']
    lines = run(kmer.info)
    assert lines[:2] == ['File format version: 1.0.0', 'Produced by: the test'] and len(lines) == 2 + 9 * 70 + 1
    for i, (name, p) in enumerate(zip(names, singles)):
        s = p.summary()
        assert lines[2 + 9 * i:11 + 9 * i] == [
            '', 'Profile: %s' % name, '- k-mer length: 4 (256 k-mers)', '- Zero counts: %d' % (256 - s['non_zero']),
            '- Non-zero counts: %d' % s['non_zero'], '- Sum of counts: %d' % s['total'], '- Mean of counts: %.3f' % s['mean'],
            '- Median of counts: %.3f' % s['median'], '- Standard deviation of counts: %.3f' % s['std']], name
