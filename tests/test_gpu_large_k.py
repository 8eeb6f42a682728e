"""The whole-table operations at the k users count (12 to 16) against plain references, and the launches that prove the path.

balance, split, strand balance, pair distances with and without balance, the ProfileDistance option pipeline, dynamic smoothing,
summaries, merge and shrink: every one of them was compared with the oracle up to k = 11 only, while the tile order of the
balance family changes from k = 13 (canon_tiles, kpal_amd/csrc/kpal_vec.hip) and every index, grid and count held in 32 bits
would be wrong first at k = 16 (4^16 = 2^32 entries).

  * k = 12, 13, 14 through the host C-ABI, against the dense oracle on every bin: a counted table (oracle.count_flat of
    oracle.synth_reads), dense Poisson counts, wide values (2^32 .. 2^62, some negative: sums, products and x + 1 wrap where
    NumPy's int64 wraps) and the structured sparse tables of tests/large_k_cases.py.  The oracle's single-threaded balance
    takes 22 s at k = 14, so balanced copies come from its multithreaded form, and a reference with do_balance is the same
    reference on those copies (kdistlib.py:136-141 balances copies first).  At k = 14 the median is np.median (oracle.stats
    sorts with qsort).
  * k = 15 and 16 through the device entry points (kpal_balance_device, kpal_pair_distance_device, kpal_profile_distance_device,
    kpal_stats_device, kpal_merge_device, kpal_shrink_device), against the restatements over the compacted support of
    tests/large_k_cases.py -- pinned to the dense oracle by tests/test_abi_and_host.py -- and, for dense tables made chunk by
    chunk, against exact tallies kept while the chunks are uploaded.  kpal_split and kpal_strand_balance have host entry points
    only and stop at k = 14.  Smoothing runs at k = 15 only: at k = 16 the option pipeline with smoothing would need about
    150 GiB of HBM.  Full tables are compared on the device: the values at the expected support, and the count of non-zero
    entries (so nothing else is non-zero), without a download.
  * one path through the Python API at k = 12 with the tables still in HBM (Profile.from_fasta).

Every call states the kernels it must launch, with their counts, read off the dispatch code (the context's launch profiler:
LAUNCH in kpal_host.hpp), so that a dispatch change cannot route around the path under test:
  balance (k >= 6)            balance_tiled
  split                       split_count + split_write
  strand balance (k >= 6)     strand_balance_tiled_set + reduce_partials (the single entry is the set entry with one table)
  pair distance               pair_distance (do_balance: pair_distance_balanced) + reduce_partials
  options                     balance_tiled x 2, positive, smooth_level x k + smooth_apply, totals + reduce_partials,
                              option_distance + reduce_partials -- each as the options ask; without positive, smoothing and
                              scaling, and not cosine: the pair distance above
  dynamic smoothing           smooth_level x k + smooth_apply
  summaries                   stats + stats_var + select_hist x (bytes from the highest one in which min and max differ)
                              + select_next (when the two middle elements differ)
  merge / shrink              merge / shrink
Distances within 1e-9 relative (euclidean bit for bit), everything else exact.  Run on the GPU box: pytest -m gpu.
"""
import io
import os

import numpy as np
import pytest

import large_k_cases as lk
import oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
METRIC = {'prod': 0, 'sum': 1, 'euclidean': 2, 'cosine': 3}
SUMMARY = {'min': 0, 'average': 1, 'median': 2}
MERGE = {'sum': 0, 'xor': 1, 'int': 2, 'nint': 3}


def _context():
    from kpal_amd import _native
    return _native.Context(_native.default_device())


def run(ctx, want, call, what):
    """call() with the context's profiler on; its launches must be exactly `want`."""
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        out = call()
        got = {name: cnt for name, (_, cnt) in ctx.prof_get().items() if cnt}
    finally:
        ctx.prof_enable(False)
    assert got == want, (what, got, want)
    return out


def pair_launches(do_balance):
    return {'pair_distance_balanced' if do_balance else 'pair_distance': 1, 'reduce_partials': 1}


def option_launches(o, k):
    name = o.get('metric_name', 'prod')
    if not (o.get('do_positive') or o.get('do_smooth') or o.get('do_scale')) and name != 'cosine':
        return pair_launches(o.get('do_balance'))
    out = {'option_distance': 1, 'reduce_partials': 1}
    if o.get('do_balance'):
        out['balance_tiled'] = 2
    if o.get('do_positive'):
        out['positive'] = 1
    if o.get('do_smooth'):
        out['smooth_level'] = k
        out['smooth_apply'] = 1
    if o.get('do_scale'):
        out['totals'] = 1
        out['reduce_partials'] = 2
    return out


def native_options(o):
    from kpal_amd import _native
    return _native.DistanceOptions(do_balance=bool(o.get('do_balance')), do_positive=bool(o.get('do_positive')),
                                   do_smooth=bool(o.get('do_smooth')), summary=SUMMARY[o.get('summary', 'min')],
                                   threshold=float(o.get('threshold', 0)), do_scale=bool(o.get('do_scale')),
                                   down=bool(o.get('down')), metric=METRIC[o.get('metric_name', 'prod')])


def close(got, want, metric, what):
    if metric == 'euclidean':
        assert got == want or (np.isnan(got) and np.isnan(want)), (what, got, want)
    else:
        assert lk.close(got, want, RTOL), (what, got, want)


def stats_launches(v):
    n = v.size
    r0, r1 = (n - 1) // 2, n // 2
    part = np.partition(v, (r0, r1))
    return dict({'stats': 1, 'stats_var': 1}, **lk._launches_of_select(int(v.min()), int(v.max()), int(part[r0]), int(part[r1])))


def check_stats(got, want, what, scale=None):
    """check_stats of tests/test_gpu_stats.py: integers and median exact, mean and std within 1e-9 (mean: relative to the
    magnitude of the data)."""
    assert (got.total, got.non_zero, got.min, got.max) == (want['total'], want['non_zero'], want['min'], want['max']), what
    assert got.median == want['median'], (what, got.median, want['median'])
    scale = abs(want['mean']) if scale is None else scale
    assert abs(got.mean - want['mean']) <= RTOL * scale + 1e-300, (what, 'mean', got.mean, want['mean'])
    assert abs(got.std - want['std']) <= RTOL * abs(want['std']) + 1e-300, (what, 'std', got.std, want['std'])


def dense_stats(v, k):
    """oracle.stats, or at k = 14 the same quantities from NumPy (np.median: the reference's own arithmetic)."""
    if k < 14:
        return oracle.stats(v)
    return {'total': int(v.sum()), 'non_zero': int(np.count_nonzero(v)), 'min': int(v.min()), 'max': int(v.max()),
            'mean': float(v.mean()), 'median': float(np.median(v)), 'std': float(v.std())}


def host_inputs(k, kind):
    n = 4 ** k
    rng = np.random.default_rng(1000 + k)
    if kind == 'counted':
        return oracle.count_flat(oracle.synth_reads(40 + k, 0, n // 160, 150, noisy=True), k, threads=16)
    if kind == 'poisson':
        return rng.poisson(1.5, n).astype(np.int64)
    if kind == 'wide':
        return lk.wide_values(np.random.RandomState(k), n)
    raise ValueError(kind)


# -- k = 12, 13, 14: the host C-ABI against the dense oracle ---------------------------------------------------------------
@pytest.mark.parametrize('k', [12, 13, 14])
def test_balance_split_strand_and_pair_distance_vs_dense_oracle(k):
    n = 4 ** k
    ctx = _context()
    try:
        li, lv, ri, rv = lk.sparse_pair(k, 300 + k, n_random=200000)
        for kind in ('counted', 'sparse') + (('wide',) if k < 14 else ()):     # (wide tables at k = 14: summaries only, next test)
            if kind == 'sparse':
                a, b = lk.dense(li, lv, n), lk.dense(ri, rv, n)
            elif kind == 'counted':
                a, b = host_inputs(k, 'counted'), host_inputs(k, 'poisson')
            else:
                a, b = host_inputs(k, 'wide'), None
            what = '%s k=%d' % (kind, k)
            got = a.copy()
            run(ctx, {'balance_tiled': 1}, lambda: ctx.balance_inplace(got, k), what)
            ba = oracle.balance(a, k)
            assert np.array_equal(got, ba), what
            del got
            f, r = run(ctx, {'split_count': 1, 'split_write': 1}, lambda: ctx.split(a, k), what)
            assert f.size == r.size == (n + (2 ** k if k % 2 == 0 else 0)) // 2, what
            of, orr = oracle.split(a, k)
            assert np.array_equal(f, of) and np.array_equal(r, orr), what
            del f, r, of, orr
            if b is None:
                continue
            for pw, code in (('prod', 0), ('sum', 1)):
                got = run(ctx, {'strand_balance_tiled_set': 1, 'reduce_partials': 1}, lambda: ctx.strand_balance(a, k, code), what)
                assert lk.close(got, oracle.strand_balance(a, k, pw), RTOL), (what, pw)
            bb = oracle.balance(b, k)
            for name in ('prod', 'sum', 'euclidean'):
                for bal in (False, True):
                    got = run(ctx, pair_launches(bal), lambda: ctx.pair_distance(a, b, METRIC[name], do_balance=bal, k=k),
                              (what, name, bal))
                    want = lk.metric(ba, bb, name) if bal else lk.metric(a, b, name)
                    close(got, want, name, (what, name, bal))
            del a, b, ba, bb
    finally:
        ctx.close()


@pytest.mark.parametrize('k', [12, 13, 14])
def test_options_smoothing_summaries_merge_shrink_vs_dense_oracle(k):
    n = 4 ** k
    ctx = _context()
    try:
        pairs = [('sparse', lk.sparse_pair(k, 400 + k, n_random=200000, wide=False))]
        if k < 14:
            pairs.append(('counted', None))
        for kind, sp in pairs:
            if sp is None:
                a, b = host_inputs(k, 'counted'), host_inputs(k, 'poisson')
            else:
                a, b = lk.dense(sp[0], sp[1], n), lk.dense(sp[2], sp[3], n)
            ba, bb = oracle.balance(a, k), oracle.balance(b, k)
            for o in lk.OPTION_GRID:
                what = (kind, k, o)
                got = run(ctx, option_launches(o, k), lambda: ctx.profile_distance(a, b, k, native_options(o)), what)
                oo = lk.oracle_options(o)
                bal = oo.pop('do_balance', False)
                want = oracle.profile_distance(ba if bal else a, bb if bal else b, k, **oo)
                assert np.isfinite(want), what
                close(got, want, oo['metric'] if not o.get('do_scale') else None, what)
            del ba, bb
            for summary, th in (('min', 0), ('average', 1), ('median', 2.5)):
                x, y = a.copy(), b.copy()
                run(ctx, {'smooth_level': k, 'smooth_apply': 1}, lambda: ctx.dynamic_smooth(x, y, k, SUMMARY[summary], th),
                    (kind, k, summary))
                ox, oy = oracle.dynamic_smooth(a, b, k, summary, th)
                assert np.array_equal(x, ox) and np.array_equal(y, oy), (kind, k, summary)
                assert x.sum() == a.sum() and y.sum() == b.sum() and np.count_nonzero(x) < np.count_nonzero(a)
                del x, y, ox, oy
            del a, b
        li, lv, ri, rv = lk.sparse_pair(k, 500 + k, n_random=200000)
        for kind in ('counted', 'sparse', 'wide'):
            if kind == 'sparse':
                a, b = lk.dense(li, lv, n), lk.dense(ri, rv, n)
            else:
                a, b = host_inputs(k, kind), host_inputs(k, 'poisson')
            what = '%s k=%d' % (kind, k)
            got = run(ctx, stats_launches(a), lambda: ctx.stats(a), what)
            check_stats(got, dense_stats(a, k), what, scale=float(np.abs(a.astype(np.float64)).mean()))
            if kind == 'wide':
                continue
            for name in lk.MERGERS:
                got = run(ctx, {'merge': 1}, lambda: ctx.merge(a, b, MERGE[name]), (what, name))
                assert np.array_equal(got, oracle.merge(a, b, name)), (what, name)
            for factor in (1, 2, 3, 4, k - 1):
                got = run(ctx, {'shrink': 1}, lambda: ctx.shrink(a, k, factor), (what, factor))
                assert np.array_equal(got, oracle.shrink(a, k, factor)), (what, factor)
            del a, b, got
    finally:
        ctx.close()


# -- k = 15, 16: the device entry points against support restatements and exact tallies ------------------------------------
def _zeros(torch, n):
    t = torch.zeros(n, dtype=torch.int64, device='cuda')
    torch.cuda.synchronize()              # (torch fills on its own stream; the library writes on the context's)
    return t


def _scatter(torch, t, idx, val):
    t.zero_()
    t[torch.from_numpy(idx).cuda()] = torch.from_numpy(np.ascontiguousarray(val)).cuda()
    torch.cuda.synchronize()


def _check_table(torch, t, idx, val, what):
    """t (on the device) is the table with support (idx, val) and zeros elsewhere."""
    torch.cuda.synchronize()
    got = t[torch.from_numpy(idx).cuda()].cpu().numpy()
    assert np.array_equal(got, val), what
    assert int(torch.count_nonzero(t)) == int(np.count_nonzero(val)), what


@pytest.mark.parametrize('k', [15, 16])
def test_device_entry_points_on_structured_sparse_tables(k):
    torch = pytest.importorskip('torch')
    n = 4 ** k
    ctx = _context()
    L = R = O = None
    try:
        # wide values: multiset distances, summaries, merge, shrink, balance (in place, last)
        li, lv, ri, rv = lk.sparse_pair(k, 600 + k)
        u, ul, ur = lk.union(li, lv, ri, rv)
        bli, blv = lk.balance(li, lv, k)
        bri, brv = lk.balance(ri, rv, k)
        bu, bl, br = lk.union(bli, blv, bri, brv)
        L, R = _zeros(torch, n), _zeros(torch, n)
        _scatter(torch, L, li, lv)
        _scatter(torch, R, ri, rv)
        for name in ('prod', 'sum'):
            for bal in (False, True):
                got = run(ctx, pair_launches(bal), lambda: ctx.pair_distance_device(n, L.data_ptr(), R.data_ptr(), METRIC[name],
                                                                                   do_balance=bal, k=k), (k, name, bal))
                want = lk.metric(bl, br, name) if bal else lk.metric(ul, ur, name)
                close(got, want, name, (k, name, bal))
        want, launches = lk.stats(li, lv, n)
        got = run(ctx, dict({'stats': 1, 'stats_var': 1}, **launches), lambda: ctx.stats_device(L.data_ptr(), n), k)
        check_stats(got, want, 'sparse k=%d' % k, scale=float(np.abs(lv.astype(np.float64)).sum()) / n)
        O = _zeros(torch, n)
        for name in lk.MERGERS:
            run(ctx, {'merge': 1}, lambda: ctx.merge_device(n, L.data_ptr(), R.data_ptr(), MERGE[name], O.data_ptr()), name)
            ctx.sync()
            _check_table(torch, O, u, lk.merge(ul, ur, name), (k, name))
        for factor in (1, 2, 3, 4, k - 1):
            out = O[:4 ** (k - factor)]
            out.zero_()
            torch.cuda.synchronize()
            run(ctx, {'shrink': 1}, lambda: ctx.shrink_device(k, factor, L.data_ptr(), out.data_ptr()), factor)
            ctx.sync()
            si, sv = lk.shrink(li, lv, factor)
            _check_table(torch, out, si, sv, (k, factor))
        del O, out
        O = None
        torch.cuda.empty_cache()
        run(ctx, {'balance_tiled': 1}, lambda: ctx.balance_device(k, L.data_ptr()), k)
        ctx.sync()
        _check_table(torch, L, bli, blv, ('balance', k))
        # values without negatives or squares that wrap: euclidean, cosine and the option pipeline
        li, lv, ri, rv = lk.sparse_pair(k, 700 + k, wide=False)
        _scatter(torch, L, li, lv)
        _scatter(torch, R, ri, rv)
        bu, bl, br = lk.union(*(lk.balance(li, lv, k) + lk.balance(ri, rv, k)))
        u, ul, ur = lk.union(li, lv, ri, rv)
        for name in ('prod', 'euclidean'):
            for bal in (False, True):
                got = run(ctx, pair_launches(bal), lambda: ctx.pair_distance_device(n, L.data_ptr(), R.data_ptr(), METRIC[name],
                                                                                   do_balance=bal, k=k), (k, name, bal))
                want = lk.metric(bl, br, name) if bal else lk.metric(ul, ur, name)
                close(got, want, name, (k, name, bal))
        for o in lk.OPTION_GRID:
            if k == 16 and o.get('do_smooth'):
                continue
            what = (k, o)
            got = run(ctx, option_launches(o, k),
                      lambda: ctx.profile_distance_device(k, L.data_ptr(), R.data_ptr(), native_options(o)), what)
            want = lk.profile_distance(li, lv, ri, rv, k, **o)
            assert np.isfinite(want), what
            close(got, want, None, what)
        ctx.sync()
    finally:
        ctx.close()                   # (frees the option pipeline's working copies)
        del L, R, O
        torch.cuda.empty_cache()


@pytest.mark.parametrize('k', [15, 16])
def test_device_summaries_merge_shrink_on_dense_tables(k):
    """A full table made chunk by chunk (a non-zero median), its summaries against exact tallies; at k = 15 merge and shrink
    of two such tables compared chunk by chunk with NumPy on the same chunk."""
    torch = pytest.importorskip('torch')
    n = 4 ** k
    ctx = _context()
    A = B = O = None
    try:
        ta = lk.DenseTable(k, 800 + k)
        A = torch.empty(n, dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()
        step = ta.chunk * 8
        for c in range(ta.chunks):
            ctx.h2d(A.data_ptr() + c * step, ta.get(c))
        want, launches = lk.stats_from_counts(ta.counts(), n)
        assert want['median'] != 0 and want['min'] < 0
        got = run(ctx, dict({'stats': 1, 'stats_var': 1}, **launches), lambda: ctx.stats_device(A.data_ptr(), n), k)
        check_stats(got, want, 'dense k=%d' % k, scale=abs(want['mean']))
        if k == 16:
            return
        tb = lk.DenseTable(k, 900 + k)
        B = torch.empty(n, dtype=torch.int64, device='cuda')
        O = torch.empty(n, dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()
        for c in range(tb.chunks):
            ctx.h2d(B.data_ptr() + c * step, tb.get(c))
        buf = np.empty(ta.chunk, dtype=np.int64)
        for name in lk.MERGERS:
            run(ctx, {'merge': 1}, lambda: ctx.merge_device(n, A.data_ptr(), B.data_ptr(), MERGE[name], O.data_ptr()), name)
            for c in range(ta.chunks):
                ctx.d2h(buf, O.data_ptr() + c * step)
                assert np.array_equal(buf, oracle.merge(ta.get(c), tb.get(c), name)), (name, c)
        kc = (ta.chunk.bit_length() - 1) // 2                       # a chunk is a table of kc
        totals = np.array([ta.get(c).sum() for c in range(ta.chunks)], dtype=np.int64)
        for factor in (1, 2, 3, 4, k - 1):
            m = 4 ** (k - factor)
            run(ctx, {'shrink': 1}, lambda: ctx.shrink_device(k, factor, A.data_ptr(), O.data_ptr()), factor)
            out = np.empty(m, dtype=np.int64)
            ctx.d2h(out, O.data_ptr())
            if factor <= kc:
                want = np.concatenate([oracle.shrink(ta.get(c), kc, factor) for c in range(ta.chunks)])
            else:                                                    # groups of whole chunks
                want = totals.reshape(m, -1).sum(axis=1)
            assert np.array_equal(out, want), factor
    finally:
        ctx.close()
        del A, B, O
        torch.cuda.empty_cache()


# -- k = 12 through the Python API, with the tables still in HBM -----------------------------------------------------------
def test_python_api_on_tables_in_hbm_k12(tmp_path):
    from kpal_amd import kdistlib, klib, metrics
    k = 12
    profiles, counts = [], []
    for p in range(3):
        reads = oracle.synth_reads(1200 + p, 0, 60000 + 20000 * p, 150, noisy=True)
        path = os.path.join(str(tmp_path), 'p%d.fa' % p)
        with open(path, 'wb') as fh:
            for j, read in enumerate(reads.reshape(-1, 151)):
                fh.write(b'>r%d\n' % j + read.tobytes())
        with open(path) as fh:
            profiles.append(klib.Profile.from_fasta(fh, k, name='p%d' % p))
        counts.append(oracle.count_flat(reads, k, threads=16))
    assert all(p._device_counts() is not None for p in profiles)
    sets = [dict(do_balance=True, do_positive=True, metric_name='sum'),
            dict(do_smooth=True, summary='median', threshold=1),
            dict(do_balance=True, do_scale=True, down=True, metric_name='cosine')]
    fn = {'prod': None, 'sum': None, 'cosine': metrics.cosine_similarity}
    for o in sets:
        name = o.get('metric_name', 'prod')
        d = kdistlib.ProfileDistance(do_balance=o.get('do_balance', False), do_positive=o.get('do_positive', False),
                                     do_smooth=o.get('do_smooth', False), summary=metrics.summary[o.get('summary', 'min')],
                                     threshold=o.get('threshold', 0), do_scale=o.get('do_scale', False),
                                     down=o.get('down', False), distance_function=fn[name],
                                     pairwise=metrics.pairwise[name if name != 'cosine' else 'prod'])
        ctx = profiles[0]._device_counts()[0]
        got = run(ctx, option_launches(o, k), lambda: d.distance(profiles[1], profiles[0]), o)
        want = oracle.profile_distance(counts[1], counts[0], k, **lk.oracle_options(o))
        assert lk.close(got, want, RTOL), (o, got, want)
        buf = io.StringIO()
        kdistlib.distance_matrix(profiles, buf, 12, d)
        lines = buf.getvalue().split('\n')
        for i in range(1, 3):
            row = [float(x) for x in lines[3 + i].split(' ')]
            for j in range(i):
                e = oracle.profile_distance(counts[i], counts[j], k, **lk.oracle_options(o))
                assert abs(row[j] - e) <= max(1e-9 * abs(e), 1e-12), (o, i, j, row[j], e)
    for p, c in zip(profiles, counts):
        s = p.summary()
        assert p._device_counts() is not None                     # summaries read the device copy
        want = oracle.stats(c)
        assert (int(s['total']), s['non_zero'], s['median']) == (want['total'], want['non_zero'], want['median'])
        assert abs(s['mean'] - want['mean']) <= RTOL * want['mean'] and abs(s['std'] - want['std']) <= RTOL * want['std']
    for p, c in zip(profiles, counts):
        assert np.array_equal(p.counts, c)                        # the download
        assert p._device_counts() is None
        f, r = p.split()
        of, orr = oracle.split(c, k)
        assert np.array_equal(f, of) and np.array_equal(r, orr)
        p.balance()
        assert np.array_equal(p.counts, oracle.balance(c, k))
        p.shrink(3)
        assert p.length == k - 3 and np.array_equal(p.counts, oracle.shrink(oracle.balance(c, k), k, 3))
