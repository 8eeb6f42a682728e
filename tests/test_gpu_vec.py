"""Parity of the HIP balance / split / distance kernels (through the C-ABI and the
kpal-compatible Python API) with the oracle and the reference goldens.
Integers bit-exact; fp64 multiset sums within 1e-9 relative (north_star tolerance; observed
~1e-15).  Run on the GPU box: pytest -m gpu."""
import io
import math
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-9
THREADS = os.cpu_count() or 1                      # the oracle's pairs dealt to the host's cores (each value still single-threaded)
METRIC_NAMES = ('prod', 'sum', 'euclidean')


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


def close(a, b, rtol=RTOL):
    if np.isnan(b):
        return np.isnan(a)
    if np.isinf(b):
        return a == b
    return abs(a - b) <= rtol * abs(b) + 1e-300


def test_g5_rc_balance_split(golden_scalars, golden_vectors):
    from kpal_amd import klib
    g = golden_scalars['G5']
    for rec in g['rc']:
        p = klib.Profile(np.zeros(4, dtype=np.int64))
        p.length = rec['k']
        assert [p.reverse_complement(x) for x in rec['x']] == rec['rc']
    for rec in g['balance_split']:
        name, k = rec['name'], rec['k']
        v = golden_vectors['g5_%s_in' % name]
        p = klib.Profile(v.copy())
        f, r = p.split()
        np.testing.assert_array_equal(f, golden_vectors['g5_%s_fwd' % name])
        np.testing.assert_array_equal(r, golden_vectors['g5_%s_rev' % name])
        np.testing.assert_array_equal(p.counts, v)   # split does not modify
        p.balance()
        np.testing.assert_array_equal(p.counts, golden_vectors['g5_%s_bal' % name])


def test_balance_split_random_vs_oracle(ctx):
    rs = np.random.RandomState(3)
    for k in (1, 2, 3, 5, 6, 7, 9, 10, 11):
        v = rs.randint(0, 1 << 40, size=4 ** k).astype(np.int64)
        v[rs.rand(4 ** k) < 0.4] = 0
        b = v.copy()
        ctx.balance_inplace(b, k)
        np.testing.assert_array_equal(b, oracle.balance(v, k))
        f, r = ctx.split(v, k)
        fo, ro = oracle.split(v, k)
        np.testing.assert_array_equal(f, fo)
        np.testing.assert_array_equal(r, ro)
        for pw in (0, 1):
            assert close(ctx.strand_balance(v, k, pw), oracle.strand_balance(v, k, ('prod', 'sum')[pw]))


def test_g6_known_answers(golden_scalars, golden_counts):
    from kpal_amd import klib, kdistlib, metrics
    g = golden_scalars['G6']
    pa = klib.Profile.from_sequences(g['toy_k2']['a'], 2)
    pb = klib.Profile.from_sequences(g['toy_k2']['b'], 2)
    assert kdistlib.ProfileDistance().distance(pa, pb) == 0.0625      # tests/test_kdistlib.py:104-112
    fx = {c['fixture']: c['sequences'] for c in golden_counts['G1']}
    left = klib.Profile.from_sequences(fx['LENGTH_60'], 8, 'left')
    right = klib.Profile.from_sequences(fx['LENGTH_60_MORE'], 8, 'right')
    keep_l, keep_r = left.counts.copy(), right.counts.copy()
    o = g['left_right_k8']
    P = metrics.pairwise
    PD = kdistlib.ProfileDistance
    assert close(PD().distance(left, right), o['prod'])
    np.testing.assert_almost_equal(PD().distance(left, right), 0.4626209322)   # tests/test_kdistlib.py:114-122
    assert close(PD(pairwise=P['sum']).distance(left, right), o['sum'])
    assert close(PD(do_balance=True).distance(left, right), o['balance_prod'])
    assert close(PD(do_balance=True, pairwise=P['sum']).distance(left, right), o['balance_sum'])
    assert PD(distance_function=metrics.euclidean).distance(left, right) == o['euclidean']
    assert PD(do_balance=True, distance_function=metrics.euclidean).distance(left, right) == o['balance_euclidean']
    assert close(PD(distance_function=metrics.cosine_similarity).distance(left, right), o['cosine'])
    f, r = left.split()
    assert close(metrics.multiset(f, r, P['prod']), o['showbalance_left'])
    assert close(_ctx().strand_balance(left.counts, 8, 0), o['showbalance_left'])
    assert close(_ctx().strand_balance(left.counts, 8, 1), o['showbalance_left_sum'])
    # option branches that keep the reference's NumPy steps but end in the HIP reduction
    assert close(PD(do_smooth=True).distance(left, right), o['smooth_min'])
    assert close(PD(do_smooth=True, summary=np.mean).distance(left, right), o['smooth_avg'])
    assert close(PD(do_positive=True).distance(left, right), o['positive'])
    assert close(PD(do_scale=True).distance(left, right), o['scale'])
    assert close(PD(do_scale=True, down=True).distance(left, right), o['scale_down'])
    # inputs unmodified (tests/test_kdistlib.py:124-135)
    np.testing.assert_array_equal(left.counts, keep_l)
    np.testing.assert_array_equal(right.counts, keep_r)
    # custom pairwise callable -> reference formulation, same value as the built-in
    custom = lambda x, y: abs(x - y) / ((x + 1) * (y + 1))   # noqa: E731
    assert close(PD(pairwise=custom).distance(left, right), o['prod'])


def _ctx():
    from kpal_amd import _native
    return _native.context()


def test_g7_metrics(golden_scalars, golden_vectors, ctx):
    from kpal_amd import metrics
    for rec in golden_scalars['G7']:
        l = golden_vectors['g7_%s_l' % rec['name']]
        r = golden_vectors['g7_%s_r' % rec['name']]
        for pw in ('prod', 'sum'):
            with np.errstate(all='ignore'):
                d = metrics.multiset(l, r, metrics.pairwise[pw])
            assert close(d, rec[pw]), (rec['name'], pw, d, rec[pw])
            if l.dtype.kind == 'i':
                _, m = ctx.pair_distance(l, r, ('prod', 'sum').index(pw), return_aux=True)
                assert m == rec['m']
        if 'euclidean' in rec:
            d, dot = ctx.pair_distance(l, r, 2, return_aux=True)
            assert dot == rec['dot']
            assert d == rec['euclidean'] or (np.isnan(d) and np.isnan(rec['euclidean']))
            e = metrics.euclidean(l, r)
            assert e == rec['euclidean'] or (np.isnan(e) and np.isnan(rec['euclidean']))


def test_pair_distance_large_vs_oracle(ctx):
    rs = np.random.RandomState(11)
    for k, lam in ((9, 830), (10, 0.8), (11, 16.6)):
        n = 4 ** k
        l = rs.poisson(lam, n).astype(np.int64)
        r = rs.poisson(lam, n).astype(np.int64)
        for metric in ('prod', 'sum', 'euclidean'):
            for bal in (False, True):
                got = ctx.pair_distance(l, r, ('prod', 'sum', 'euclidean').index(metric), do_balance=bal, k=k)
                want = oracle.distance(l, r, k, do_balance=bal, metric=metric)
                if metric == 'euclidean':
                    assert got == want
                else:
                    assert close(got, want), (k, metric, bal, got, want)
    # odd length vector (not a power of 4) through the raw ABI
    l = rs.poisson(3, 1001).astype(np.int64)
    r = rs.poisson(3, 1001).astype(np.int64)
    assert close(ctx.pair_distance(l, r, 0), oracle.multiset(l, r, 'prod'))
    assert ctx.pair_distance(l, r, 2) == oracle.euclidean(l, r)


def test_g8_matrix_text(golden_scalars):
    from kpal_amd import klib, kdistlib, metrics
    g = golden_scalars['G8']
    profs = [klib.Profile.from_sequences(s, g['k'], n) for s, n in zip(g['sets'], g['names'])]
    for case in g['cases']:
        if case['pairwise'] == 'euclidean':
            dist = kdistlib.ProfileDistance(distance_function=metrics.euclidean)
        else:
            dist = kdistlib.ProfileDistance(do_balance=case['do_balance'], pairwise=metrics.pairwise[case['pairwise']])
        out = io.StringIO()
        kdistlib.distance_matrix(profs[:case['count']], out, case['precision'], dist)
        assert out.getvalue() == case['text'], case
    # reference test expectations (tests/test_kdistlib.py:38-74)
    out = io.StringIO()
    kdistlib.distance_matrix(profs[:1], out, 2, kdistlib.ProfileDistance())
    assert out.getvalue().strip().split('\n') == ['1', 'a']
    out = io.StringIO()
    kdistlib.distance_matrix(profs[:3], out, 2, kdistlib.ProfileDistance())
    assert out.getvalue().strip().split('\n') == ['3', 'a', 'b', 'c', '0.46', '0.00 0.46']


def test_matrix_vs_pairs_and_oracle(ctx):
    rs = np.random.RandomState(13)
    for k, P in ((6, 5), (8, 7), (9, 13), (7, 64)):
        profs = [rs.poisson(rs.choice([0.8, 16.6, 200]), 4 ** k).astype(np.int64) for _ in range(P)]
        for metric in ('prod', 'sum', 'euclidean'):
            for bal in (False, True):
                got = ctx.distance_matrix(profs, k, ('prod', 'sum', 'euclidean').index(metric), do_balance=bal)
                # every entry against the oracle; past 13 profiles against the pair kernel as well
                wants = [oracle.distance_matrix_values(profs, k, bal, metric, threads=THREADS)]
                if P > 13:
                    wants.append(np.array([ctx.pair_distance(profs[i], profs[j], ('prod', 'sum', 'euclidean').index(metric),
                                                             do_balance=bal, k=k) for i in range(1, P) for j in range(i)]))
                for want in wants:
                    assert got.shape == want.shape
                    if metric == 'euclidean':
                        np.testing.assert_array_equal(got, want)
                    else:
                        np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)


def test_matrix_super_tiles(ctx):
    """The LDS-staged 16 x 16 super-tile kernels (P > 8, k >= 6): ragged profile counts (clamped rows, idle
    groups, several super-tiles); counts >= 2^31 in some bins (the difference-of-reciprocals kernel of multiset 'prod'
    reports them and the pair-of-counts kernel reruns: int64 path next to the float path) and the same shapes with every
    count below 2^16 (the difference-of-reciprocals kernel's own result: table and computed reciprocals, zero masks);
    at k = 12 enough bins per thread for the packed byte counters of the term counts to be flushed; and (big = None) every
    count below 1024: multiset 'sum' on its reciprocal-table kernel up to the last table entries.  Every entry against the
    oracle; past 17 profiles, and at k = 12, against the pair kernel as well."""
    rs = np.random.RandomState(17)
    for k, P, big in ((6, 9, True), (6, 16, True), (7, 17, True), (6, 33, True), (8, 20, True),
                      (6, 9, False), (7, 17, False), (6, 33, False), (8, 20, False), (9, 64, False),
                      (6, 9, None), (7, 17, None), (8, 36, None)):
        profs = [rs.poisson(rs.choice([0.3, 5.0, 90.0]), 4 ** k).astype(np.int64) for _ in range(P)]
        if big is None:
            # multiset 'sum' stays on its table kernel (every count below 1024): the largest table entries, equal large counts
            profs[P // 2][rs.randint(0, 4 ** k, 50)] = 1023 - rs.randint(0, 30, 50)
            profs[0][5] = profs[1][5] = 1023
            profs[2][5] = 1022
        elif big:
            profs[P // 2][rs.randint(0, 4 ** k, 50)] = (1 << 31) + rs.randint(0, 1000, 50)     # beyond the float path
        else:
            # multiset 'prod' stays on the difference-of-reciprocals kernel (every count below 2^16): counts beyond its
            # reciprocal table (512) next to small ones, equal large counts, a count just below the limit
            profs[P // 2][rs.randint(0, 4 ** k, 50)] = 512 + rs.randint(0, 60000, 50)
            profs[0][5] = profs[1][5] = 55555
            profs[2][9] = (1 << 16) - 1
        profs[1][::7] = 0
        for metric in ('prod', 'sum', 'euclidean'):
            code = ('prod', 'sum', 'euclidean').index(metric)
            got = ctx.distance_matrix(profs, k, code)
            # every entry against the oracle; past 17 profiles against the pair kernel as well
            wants = [oracle.distance_matrix_values(profs, k, False, metric, threads=THREADS)]
            if P > 17:
                wants.append(np.array([ctx.pair_distance(profs[i], profs[j], code) for i in range(1, P) for j in range(i)]))
            for want in wants:
                if metric == 'euclidean':
                    np.testing.assert_array_equal(got, want)
                else:
                    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
    k, P = 12, 10
    profs = [ctx.count_bytes(k, oracle.synth_reads(300 + p, 0, 60000, 150)) for p in range(P)]
    profs[3][:1000] += 1 << 32
    for code in (0, 1, 2):
        got = ctx.distance_matrix(profs, k, code)
        for want in (oracle.distance_matrix_values(profs, k, False, METRIC_NAMES[code], threads=THREADS),
                     np.array([ctx.pair_distance(profs[i], profs[j], code) for i in range(1, P) for j in range(i)])):
            if code == 2:
                np.testing.assert_array_equal(got, want)
            else:
                np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
    metric = 'prod'
    for i, j in ((1, 0), (3, 2), (9, 3)):
        assert close(ctx.distance_matrix(profs, k, 0)[i * (i - 1) // 2 + j], oracle.distance(profs[i], profs[j], k, metric=metric))


def test_matrix_all_staged_once(ctx):
    """The kernels that stage every profile once per bin range (matrix_all_kernels.hpp; 17..64 profiles, multiset prod and
    sum): every profile count around their geometry's edges -- 17 / 32 (the 256-thread form, a last block of one / four
    rows), 33 / 48 / 61 / 64 (the 1024-thread form; dead slots; a diagonal slot whose second block is past the end) -- with
    zero bins (term counts from the zero masks), counts beyond the reciprocal table of 'prod' and up to the last entries of
    the table of 'sum'; every pair against the oracle and against kpal_pair_distance (IEEE divisions)."""
    rs = np.random.RandomState(23)
    for k, P in ((6, 17), (6, 32), (7, 33), (6, 48), (6, 61), (7, 64), (6, 18), (6, 29)):
        profs = [rs.poisson(rs.choice([0.3, 5.0, 90.0]), 4 ** k).astype(np.int64) for _ in range(P)]
        profs[P // 2][rs.randint(0, 4 ** k, 50)] = 512 + rs.randint(0, 500, 50)      # past the table of 'prod', inside the table of 'sum'
        profs[0][5] = profs[1][5] = 1023
        profs[2][5] = 1022
        profs[1][::7] = 0
        profs[P - 1][::3] = 0
        profs[P - 2][:] = 0                                                           # an empty profile: every bin a both-zero candidate
        for code, metric in ((0, 'prod'), (1, 'sum')):
            got = ctx.distance_matrix(profs, k, code)
            np.testing.assert_allclose(got, oracle.distance_matrix_values(profs, k, False, metric, threads=THREADS), rtol=RTOL, atol=0)
            want = np.array([ctx.pair_distance(profs[i], profs[j], code) for i in range(1, P) for j in range(i)])
            np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
            for i, j in ((1, 0), (P - 1, P - 2), (P - 1, 0), (P // 2, 3), (P - 2, 1)):
                assert close(got[i * (i - 1) // 2 + j], oracle.distance(profs[i], profs[j], k, metric=metric)), (k, P, metric, i, j)


def test_matrix_rdiff_worst_case(ctx):
    """The accuracy bound of multiset 'prod' as a difference of reciprocals (cross_recip_kernel<0>, launched as matrix_rdiff) where it is tightest: EVERY
    count just below the kernel's limit of 2^16 and neighbours differing by 1 or 2 -- each term 1/(y+1) - 1/(x+1) cancels all
    but the last ~16 bits of its operands.  Against the oracle (IEEE divisions of the integer formulation), 1e-9 relative; and
    one count AT the limit must take the pair-of-counts kernel (same answer)."""
    rs = np.random.RandomState(99)
    for k, P in ((6, 12), (8, 20)):
        profs = [((1 << 16) - 1 - rs.randint(0, 3, 4 ** k)).astype(np.int64) for _ in range(P)]
        got = ctx.distance_matrix(profs, k, 0)
        want = oracle.distance_matrix_values(profs, k, False, 'prod')
        rel = np.abs(got - want) / np.abs(want)
        assert rel.max() <= RTOL, (k, P, float(rel.max()))
        profs[3][11] = 1 << 16
        got = ctx.distance_matrix(profs, k, 0)
        want = oracle.distance_matrix_values(profs, k, False, 'prod')
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)      # IEEE divisions: the pair-of-counts kernel ran


def test_g4_tutorial_end_to_end(golden_scalars, tutorial_dir):
    """doc/tutorial.rst:44-144 through the drop-in API: count 8 FASTA files (60-column wrapped
    records), merge, distance, matrix, showbalance."""
    from kpal_amd import klib, kdistlib, metrics
    g = golden_scalars['G4']
    prof = {}
    for fname, rec in g['files'].items():
        if not fname.endswith('.fa'):
            continue
        with open(os.path.join(tutorial_dir, fname)) as fh:
            p = klib.Profile.from_fasta(fh, 8, name=fname[:-3])
        assert (int(p.total), int(p.non_zero)) == (rec['total'], rec['non_zero'])
        prof[p.name] = p
    d = kdistlib.ProfileDistance()
    assert close(d.distance(prof['c_1'], prof['c_2']), g['distance_c1_c2'])
    merged = []
    for s in 'abcd':
        m = prof[s + '_1'].copy()
        m.merge(prof[s + '_2'])
        m.name = s
        assert (int(m.total), int(m.non_zero)) == (g['files'][s + '_merged']['total'], g['files'][s + '_merged']['non_zero'])
        merged.append(m)
    out = io.StringIO()
    kdistlib.distance_matrix(merged, out, 3, d)
    assert out.getvalue() == g['matrix_abcd_p3']
    assert close(kdistlib.ProfileDistance(do_balance=True).distance(merged[0], merged[1]), g['distance_balanced_a_b'])
    f, r = merged[0].split()
    assert close(metrics.multiset(f, r, metrics.pairwise['prod']), g['showbalance_a'])


def test_from_fasta_by_record_and_names():
    from kpal_amd import klib
    fasta = '>one desc\nACGTAC\nGT\n>two\nNNNN\n>\nACGT\n'
    ps = list(klib.Profile.from_fasta_by_record(io.StringIO(fasta), 2, prefix='x'))
    assert [p.name for p in ps] == ['x_one', 'x_two', 'x_3']
    np.testing.assert_array_equal(ps[0].counts, oracle.from_sequences(['ACGTACGT'], 2))
    assert ps[1].total == 0
    with pytest.raises(ValueError):
        klib.Profile(np.zeros(16, dtype=np.int64), 'a/b')
    with pytest.raises(ValueError):
        klib.Profile.from_sequences(['ACGT'], 0)


def test_config5_matrix_k12_subset(ctx):
    """BASELINE config 5 shape at k = 12 on an 8-profile subset: each profile = counts of
    100 000 synthetic reads (sparse variant) -- matrix vs per-pair oracle, 1e-9 relative."""
    k, P = 12, 8
    profs = []
    for p in range(P):
        buf = oracle.synth_reads(100 + p, 0, 100000, 150)
        profs.append(ctx.count_bytes(k, buf))
    got = ctx.distance_matrix(profs, k, 0)
    want = oracle.distance_matrix_values(profs, k, False, 'prod')
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
    got = ctx.distance_matrix(profs[:3], k, 0, do_balance=True)
    want = oracle.distance_matrix_values(profs[:3], k, True, 'prod')
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)


@pytest.mark.parametrize('n_reads', [2_000_000, 100_000], ids=['dense', 'sparse'])
def test_config5_matrix_k12_64_profiles(ctx, n_reads):
    """BASELINE config 5 at its stated size: 64 profiles at k = 12, profile p = the
    count of n_reads synthetic reads with seed 100 + p (dense: 2 M reads, mean 16.6 per bin; sparse: 100 k
    reads, ~43 % zero bins), kdistlib.distance_matrix values through kpal_distance_matrix_device (64 profiles: multiset on the
    kernels that stage every profile once, matrix_rdiff_all / matrix_rsum_all; euclidean on the matrix cores, gram_mfma) for
    prod / sum / euclidean, prod also balanced on the dense variant (kdistlib.py:164-186):
      * ALL 2016 entries against the oracle (its pair function on every pair, dealt to the host's cores) for multiset prod
        (dense and sparse), multiset sum (dense and sparse) and euclidean (dense): <= 1e-9 relative, euclidean bit-identical;
      * the 276 entries of the first 24 profiles against the oracle for the other two combinations (dense: prod balanced;
        sparse: euclidean);
      * 60 entries of every combination against the pair kernel (IEEE divisions, another summation order);
      * the text of a 12-profile sub-matrix through kdistlib.distance_matrix against the oracle's text."""
    from kpal_amd import klib, kdistlib
    k, P = 12, 64
    n = 4 ** k
    rs = np.random.RandomState(n_reads % 1000 + 5)
    d = ctx.alloc(n_reads * 151)
    dprof = ctx.alloc(P * n * 8)
    host = np.empty((P, n), dtype=np.int64)
    threads = min(128, os.cpu_count() or 1)
    try:
        for p in range(P):
            ctx.synth_reads_device(100 + p, 0, n_reads, 150, d)
            ctx.count_begin(k)
            ctx.count_feed_device(d, n_reads * 151)
            host[p] = ctx.count_finish()
            assert host[p].sum() == n_reads * (150 - k + 1)
        ctx.h2d(dprof, host)
        if n_reads == 100_000:
            assert 0.40 < np.mean(host[0] == 0) < 0.46          # the sparse variant really is sparse
        pairs = [(i, j) for i in range(1, P) for j in range(i)]
        pick = [pairs[t] for t in rs.choice(len(pairs), 60, replace=False)]
        # the oracle on ALL 2016 pairs for prod, sum and (dense) euclidean; on the 276 pairs of the first 24 profiles for the other two
        # combinations (2016 pairs x 4^12 bins cost the host ~12 s each)
        full = {('prod', False), ('sum', False), ('euclidean', False)} if n_reads == 2_000_000 else {('prod', False), ('sum', False)}
        sub = 24
        combos = [('prod', False), ('prod', True), ('sum', False), ('euclidean', False)]   # (sum / euclidean with balancing: the smaller tests)
        if n_reads != 2_000_000:
            combos = [('prod', False), ('sum', False), ('euclidean', False)]
        for metric, bal in combos:
            code = ('prod', 'sum', 'euclidean').index(metric)
            if True:
                got = ctx.distance_matrix_device(P, k, dprof, code, bal)
                assert got.shape == (2016,)
                if (metric, bal) in full:
                    want = oracle.distance_matrix_values(host, k, bal, metric, threads=threads)
                    mine = got
                else:
                    want = oracle.distance_matrix_values(host[:sub], k, bal, metric, threads=threads)
                    mine = got[:sub * (sub - 1) // 2]          # rows 1 .. sub-1 of the lower triangle come first
                if metric == 'euclidean':
                    np.testing.assert_array_equal(mine, want)
                else:
                    rel = np.abs(mine - want) / np.abs(want)
                    assert rel.max() <= RTOL, (metric, bal, float(rel.max()), int(rel.argmax()))
                for i, j in pick:
                    byp = ctx.pair_distance_device(n, dprof + i * n * 8, dprof + j * n * 8, code, bal, k)
                    g = got[i * (i - 1) // 2 + j]
                    assert (g == byp) if metric == 'euclidean' else close(g, byp), (metric, bal, i, j, g, byp)
        # text (precision <= 8) of a sub-matrix through the drop-in API
        sub = [klib.Profile(host[p], 'p%d' % p) for p in range(0, 60, 5)]
        for prec in (3, 8):
            out = io.StringIO()
            kdistlib.distance_matrix(sub, out, prec, kdistlib.ProfileDistance())
            want = oracle.distance_matrix_values([s.counts for s in sub], k, False, 'prod')
            assert out.getvalue() == oracle.distance_matrix_text([s.name for s in sub], want, prec)
    finally:
        ctx.free(d)
        ctx.free(dprof)


def _multiset_expression(left, right, pairwise):
    """metrics.multiset (kpal/metrics.py:101-123) evaluated here: the reference's mask and NumPy terms, the terms summed
    exactly (math.fsum) -- or, when a term is not finite, by NumPy, which is then exact as well (inf, -inf or NaN)."""
    left, right = np.asanyarray(left), np.asanyarray(right)
    with np.errstate(all='ignore'):
        keep = np.logical_or(left, right)
        x, y = left[keep], right[keep]
        terms = np.abs(x - y) / ((x + 1) * (y + 1)) if pairwise == 'prod' else np.abs(x - y) / (x + y + 1)
        terms = np.asarray(terms, dtype=np.float64)
        total = math.fsum(terms) if np.isfinite(terms).all() else terms.sum()
    return total / (len(terms) + 1), len(terms)


def close_strict(a, b):
    """close() without its absolute floor: subnormal results must agree to 1e-9 relative as well."""
    if np.isnan(b) or np.isinf(b):
        return close(a, b)
    return abs(a - b) <= RTOL * abs(b)


def _float_vectors():
    """(name, left, right) float64 pairs for kpal_pair_distance_f64."""
    rs = np.random.RandomState(31)
    from kpal_amd import metrics
    out = []
    for n in [0, 1, 2, 3, 255, 257] + [4 ** k for k in range(1, 11)] + [4 ** 12]:
        l = rs.poisson(rs.choice([0.5, 16.6]), n).astype(np.int64)
        r = rs.poisson(rs.choice([0.5, 16.6, 200.0]), n).astype(np.int64)
        if n and not r.any():
            r[0] = 3
        if n and not l.any():
            l[-1] = 1
        for down in (False, True):
            with np.errstate(all='ignore'):
                ls, rsc = metrics.get_scale(l, r)              # (one of the factors is 1.0, the other the totals' ratio)
            if down:
                ls, rsc = metrics.scale_down(ls, rsc)
            out.append(('scaled_n%d%s' % (n, '_down' if down else ''), l * ls, r * rsc))
    n = 4 ** 6
    a = rs.uniform(-0.9, 40.0, n)
    b = rs.uniform(-0.9, 40.0, n)
    a[rs.rand(n) < 0.3] = 0.0
    out.append(('non_integer', a, b))
    c, d = a.copy(), b.copy()
    c[rs.randint(0, n, 40)] = -rs.uniform(1.5, 30.0, 40)    # negative denominators: negative terms
    d[rs.randint(0, n, 40)] = -rs.uniform(1.5, 30.0, 40)
    out.append(('negative', c, d))
    e = c.copy()
    e[[5, 77]] = -1.0                                        # x + 1 == 0: the terms are +inf / NaN
    out.append(('x_plus_1_zero', e, d))
    f = b.copy()
    f[9] = -1.0
    g = f.copy()                                             # -1 against -1: 0 / 0
    out.append(('both_minus_1', f, g))
    for name, val in (('nan', np.nan), ('inf', np.inf), ('minus_inf', -np.inf)):
        h = a.copy()
        h[100] = val
        out.append((name, h, b))
    z, w = a.copy(), b.copy()
    z[:50] = -0.0                                            # falsy in logical_or: no term where both are (-)0
    w[:50] = 0.0
    w[50:60] = -0.0
    z[50:60] = 0.0
    out.append(('minus_zero', z, w))
    s = np.zeros(n)
    s[::3] = np.finfo(np.float64).tiny * rs.rand((n + 2) // 3)   # subnormals (and a few zeros)
    s[1] = 5e-324
    t = np.zeros(n)
    t[::5] = 5e-324 * rs.randint(1, 1000, (n + 4) // 5)
    out.append(('subnormal', s, t))
    out.append(('subnormal_vs_counts', s, b))
    return out


def test_pair_distance_f64_vs_oracle_and_expression(ctx):
    """kpal_pair_distance_f64 (metrics.multiset on float vectors; ProfileDistance's NumPy path after do_scale) for prod and sum
    against oracle.multiset on float64 and against the reference's expression evaluated here: the same number of terms, the
    value within 1e-9 relative, the same NaN / infinity."""
    for name, l, r in _float_vectors():
        for code, pw in ((0, 'prod'), (1, 'sum')):
            got, m = ctx.pair_distance_f64(l, r, code, return_aux=True)
            want, m_want = _multiset_expression(l, r, pw)
            assert m == m_want, (name, pw, m, m_want)
            with np.errstate(all='ignore'):
                o, m_o = oracle.multiset(l, r, pw, return_m=True)
            assert m_o == m_want, (name, pw)
            assert close_strict(got, want), (name, pw, got, want)
            assert close_strict(got, o), (name, pw, got, o)
            if want == 0:
                assert got == 0, (name, pw, got)


def test_float_multiset_through_the_api(ctx):
    """metrics.multiset on float64 x float64 and int64 x float64 vectors (kpal_pair_distance_f64), and ProfileDistance with
    a summary callable and do_scale -- the reference's NumPy pipeline ending in that kernel -- against the oracle's
    ProfileDistance with the built-in summary the callable mimics."""
    from kpal_amd import klib, kdistlib, metrics
    rs = np.random.RandomState(37)
    n = 4 ** 7
    li = rs.poisson(3.0, n).astype(np.int64)
    ri = rs.poisson(40.0, n).astype(np.int64)
    ri[rs.rand(n) < 0.2] = 0
    lf, rf = li * 13.25, ri * 0.375
    for pw in ('prod', 'sum'):
        f = metrics.pairwise[pw]
        for a, b in ((lf, rf), (li, rf), (lf, ri)):
            got = metrics.multiset(a, b, f)
            assert close(got, oracle.multiset(a, b, pw)), (pw, a.dtype, b.dtype)
            assert close(got, _multiset_expression(a, b, pw)[0]), (pw, a.dtype, b.dtype)
    k = 5
    mimic = {'min': lambda v: np.min(v), 'median': lambda v: np.median(v)}
    for trial in range(3):
        l = rs.poisson(rs.choice([0.5, 4.0, 30.0]), 4 ** k).astype(np.int64)
        r = rs.poisson(rs.choice([0.5, 4.0, 30.0]), 4 ** k).astype(np.int64)
        for summary, fn in mimic.items():
            for down in (False, True):
                for pw in ('prod', 'sum'):
                    dist = kdistlib.ProfileDistance(do_smooth=True, summary=fn, do_scale=True, down=down,
                                                    pairwise=metrics.pairwise[pw])
                    got = dist.distance(klib.Profile(l.copy()), klib.Profile(r.copy()))
                    want = oracle.profile_distance(l, r, k, do_smooth=True, summary=summary, do_scale=True, down=down,
                                                   metric=pw)
                    assert close(got, want), (trial, summary, down, pw, got, want)


def test_vector_length_and_cosine_on_int64(ctx):
    """metrics.vector_length (the pair kernel against a zero vector) and metrics.cosine_similarity on int64 vectors, wrapping
    ones included, against the oracle's euclidean(v, 0) -- np.sqrt(np.dot(v, v)) with int64 wrap-around -- bit for bit."""
    from kpal_amd import metrics
    rs = np.random.RandomState(41)
    vecs = [rs.poisson(20.0, 4 ** 6).astype(np.int64), rs.randint(-1000, 1000, 4 ** 8).astype(np.int64),
            np.array([3, 4], dtype=np.int64), np.array([1 << 31, 1 << 31], dtype=np.int64),       # dot = 2^63: wraps negative
            np.array([np.iinfo(np.int64).max, 5, -7], dtype=np.int64), np.array([1 << 32, 3], dtype=np.int64),  # wraps to 9
            np.array([-(1 << 62), 1 << 62, 12345], dtype=np.int64), np.zeros(17, dtype=np.int64)]
    for v in vecs:
        want = oracle.euclidean(v, np.zeros_like(v))
        got = metrics.vector_length(v)
        assert got == want or (np.isnan(got) and np.isnan(want)), (v[:4], got, want)
    for a, b in ((vecs[0], vecs[0][::-1].copy()), (vecs[1], vecs[1] * 3), (vecs[3], vecs[3]), (vecs[4], vecs[4][::-1].copy()),
                 (vecs[6], vecs[6] + 1)):
        with np.errstate(all='ignore'):
            want = np.dot(a, b) / (oracle.euclidean(a, np.zeros_like(a)) * oracle.euclidean(b, np.zeros_like(b)))
            got = metrics.cosine_similarity(a, b)
        assert got == want or (np.isnan(got) and np.isnan(want)), (a[:4], b[:4], got, want)
