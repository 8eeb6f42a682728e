"""Parity of the HIP counting path (through the C-ABI) with the oracle and the reference
goldens.  Bit-exact: integer work.  Run on the GPU box: pytest -m gpu."""
import hashlib
import io
import os

import numpy as np
import pytest

import oracle
from conftest import dense

pytestmark = pytest.mark.gpu

# imported before any HIP work of this process: a late first import (inside a test, after tens of GB of device
# traffic) once sat in torch's module loading until the per-test timeout
torch = pytest.importorskip('torch')


def sha(v):
    return hashlib.sha256(np.ascontiguousarray(v, dtype='<i8').tobytes()).hexdigest()


# The exact-offset 'partition' (round 1), which AUTO no longer takes for any input, keeps its own cross-checks in the default
# run (test_small_partition_batches, test_partition_pipelines_on_skewed_inputs); KPAL_TEST_RETIRED=1 puts it back into every
# strategy loop.  The level-2 variants KPAL_LEVEL2=0/1 of the two-level path are checked at k = 13, 14
# (test_two_level_variants_of_level2) and k = 15 (test_two_level_k15_against_oracle).
RETIRED = os.environ.get('KPAL_TEST_RETIRED', '0') not in ('', '0')


def strategies(k):
    s = ['auto', 'global_atomic']
    if k <= 7:
        s.append('lds_direct')
    if 8 <= k <= 12:
        if RETIRED:
            s.append('partition')
        s.append('partition_chunked')
        s.append('partition_quads')
    if 13 <= k <= 16:
        s.append('partition2')
        s.append('partition2_quads')
    return s


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


def test_g1_fixtures_through_profile_api(golden_counts):
    from kpal_amd import klib
    for case in golden_counts['G1']:
        p = klib.Profile.from_sequences(case['sequences'], case['k'])
        assert p.counts.dtype == np.int64 and p.length == case['k']
        np.testing.assert_array_equal(p.counts, dense(case['counts']))
        assert p.total == case['total'] and p.non_zero == case['non_zero']
        fasta = ''.join('>r%d\n%s\n' % (i, s) for i, s in enumerate(case['sequences']))
        pf = klib.Profile.from_fasta(io.StringIO(fasta), case['k'])
        np.testing.assert_array_equal(pf.counts, p.counts)


def test_g2_randomized_all_strategies(golden_counts, ctx):
    for case in golden_counts['G2']:
        want = dense(case['counts'])
        flat = '\n'.join(case['sequences']).encode('latin-1', 'replace')
        for strat in strategies(case['k']):
            got = ctx.count_bytes(case['k'], flat, strat)
            np.testing.assert_array_equal(got, want, err_msg='k=%d %s %r' % (case['k'], strat, case['sequences']))


def test_empty_and_short_inputs(ctx):
    from kpal_amd import klib
    for seqs in ([], [''], ['AC', 'G'], ['N' * 40]):
        p = klib.Profile.from_sequences(seqs, 3)
        assert p.counts.shape == (64,) and p.total == 0
    for k in (1, 7, 8, 12, 13):
        for strat in strategies(k):
            assert ctx.count_bytes(k, b'', strat).sum() == 0
            assert ctx.count_bytes(k, b'ACGT'[:min(k - 1, 4)] or b'N', strat).sum() == 0


def test_k_equals_length_and_every_k(ctx):
    seq = b'GATTACAGATTACACATGCATGCAAACCCGGGTTT'
    for k in range(1, 16):
        want_total = max(0, len(seq) - k + 1)
        if k <= 13:
            want = oracle.count_flat(seq, k)
            for strat in strategies(k):
                np.testing.assert_array_equal(ctx.count_bytes(k, seq, strat), want, err_msg='k=%d %s' % (k, strat))
        elif k <= 15:   # big tables: check total and the positions of the hits only
            got = ctx.count_bytes(k, seq)
            assert got.sum() == want_total
            idx = np.nonzero(got)[0]
            ref = sorted(set(_enc(seq[i:i + k]) for i in range(want_total)))
            assert list(idx) == ref
    # k == len(seq) and k == len(seq) - 1 (tests/test_klib.py:72-81)
    s8 = b'GTACATGA'
    for k in (8, 7):
        np.testing.assert_array_equal(ctx.count_bytes(k, s8), oracle.count_flat(s8, k))


def _enc(b):
    v = 0
    for c in b:
        v = (v << 2) | 'ACGT'.index(chr(c))
    return v


def test_g3_config1(golden_synth, ctx):
    g = golden_synth['config1']
    buf = oracle.synth_reads(g['seed'], 0, g['n_reads'], g['read_len'])
    for strat in strategies(g['k']):
        c = ctx.count_bytes(g['k'], buf, strat)
        assert c.sum() == g['total'] == 1420000
        assert sha(c) == g['sha256'], strat
    from kpal_amd import klib
    p = klib.Profile.from_sequences((bytes(r) for r in buf.reshape(-1, 151)[:, :150]), g['k'])
    assert sha(p.counts) == g['sha256'] and p.non_zero == g['non_zero']


def test_g3_noisy_and_long(golden_synth, ctx):
    g = golden_synth['noisy']
    buf = oracle.synth_reads(g['seed'], 0, g['n_reads'], 150, noisy=True)
    for case in g['cases']:
        for strat in strategies(case['k']):
            c = ctx.count_bytes(case['k'], buf, strat)
            assert (int(c.sum()), int(np.count_nonzero(c)), sha(c)) == (case['total'], case['non_zero'], case['sha256']), (case['k'], strat)
    g = golden_synth['long']
    buf = oracle.synth_reads(g['seed'], 0, g['n_reads'], 150, noisy=True)
    seq = np.ascontiguousarray(buf.reshape(-1, 151)[:, :150]).reshape(-1)
    for case in g['cases']:
        for strat in strategies(case['k']):
            c = ctx.count_bytes(case['k'], seq, strat)
            assert (int(c.sum()), sha(c)) == (case['total'], case['sha256']), (case['k'], strat)


def test_generator_matches_oracle(ctx):
    for noisy in (False, True):
        n = 3001
        want = oracle.synth_reads(5, 12345, n, 150, noisy=noisy)
        d = ctx.alloc(want.size)
        try:
            ctx.synth_reads_device(5, 12345, n, 150, d, noisy=noisy)
            got = np.empty_like(want)
            ctx.d2h(got, d)
        finally:
            ctx.free(d)
        np.testing.assert_array_equal(got, want)
    # odd read length, single read
    want = oracle.synth_reads(9, 7, 1, 37)
    d = ctx.alloc(64)
    ctx.synth_reads_device(9, 7, 1, 37, d)
    got = np.empty_like(want)
    ctx.d2h(got, d)
    ctx.free(d)
    np.testing.assert_array_equal(got, want)


def test_unaligned_device_buffers_and_multiple_feeds(ctx):
    buf = oracle.synth_reads(31, 0, 700, 150, noisy=True)
    d = ctx.alloc(buf.size + 64)
    try:
        for off in (0, 1, 7, 15, 16, 33):
            ctx.h2d(d + off, buf)
            for k in (4, 10, 13):
                for strat in strategies(k):
                    ctx.count_begin(k, strat)
                    ctx.count_feed_device(d + off, buf.size)
                    got = ctx.count_finish()
                    np.testing.assert_array_equal(got, oracle.count_flat(buf, k), err_msg='off=%d k=%d %s' % (off, k, strat))
        # several feeds: windows never span feeds, even when a feed ends mid-read
        ctx.h2d(d, buf)
        cuts = [0, 1000, 1001, 5000, 77777, buf.size]
        for k in (6, 11):
            ctx.count_begin(k)
            want = np.zeros(4 ** k, dtype=np.int64)
            for a, b in zip(cuts[:-1], cuts[1:]):
                ctx.count_feed_device(d + a, b - a)
                want += oracle.count_flat(buf[a:b], k)
            np.testing.assert_array_equal(ctx.count_finish(), want)
    finally:
        ctx.free(d)


def test_host_feed_larger_than_staging(ctx):
    # 160 MB of noisy reads: crosses the 64 MiB pinned staging pieces (halo handling) and
    # several partition batches
    n = 1060000
    buf = oracle.synth_reads(41, 0, n, 150, noisy=True)
    assert buf.size > 2 * (64 << 20)
    for k in (5, 12):
        want = oracle.count_flat(buf, k, threads=8)
        got = ctx.count_bytes(k, buf)
        np.testing.assert_array_equal(got, want)
    # one long record with no separators at all across staging seams
    seq = np.ascontiguousarray(buf.reshape(-1, 151)[:, :150]).reshape(-1)
    np.testing.assert_array_equal(ctx.count_bytes(12, seq), oracle.count_flat(seq, 12, threads=8))


def test_two_level_batch_halving():
    """Two-level path when a coarse bucket would overflow its 32-bit offsets: the batch is halved
    recursively (forced here by lowering the limit); halo across the seams of the halves."""
    from kpal_amd import _native
    os.environ['KPAL_SPLIT_ABOVE'] = '20000'
    try:
        c2 = _native.Context(_native.default_device())
    finally:
        del os.environ['KPAL_SPLIT_ABOVE']
    buf = oracle.synth_reads(47, 0, 6000, 150, noisy=True)
    seq = np.ascontiguousarray(buf.reshape(-1, 151)[:, :150]).reshape(-1)
    homo = np.frombuffer(b'A' * 300000 + b'C' * 17 + b'N' + b'ACGT' * 5000, dtype=np.uint8)
    for k in (13, 14, 15):
        for data in (buf, seq, homo):
            assert np.array_equal(c2.count_bytes(k, data, 'partition2'), oracle.count_flat(data, k, threads=4)), k
    c2.close()


@pytest.mark.parametrize('steps', ['8', '7', '6', '4', '3', '2', '1'])
def test_quad_tile_sizes_against_oracle(steps):
    """Every tile size the quad scatters are compiled for (KPAL_QUAD_STEPS / KPAL_QUAD_STEPS2, read when the context is
    created; normally chosen per feed from a sample of the row loads), one- and two-level, on uniform and AT-rich input with a
    homopolymer stretch: bit-exact, and kpal_count_last_plan confirms that the forced size is the one that ran."""
    from kpal_amd import _native
    steps2 = {'1': '2'}.get(steps, steps)
    os.environ['KPAL_QUAD_STEPS'] = steps
    os.environ['KPAL_QUAD_STEPS2'] = steps2
    try:
        c2 = _native.Context(_native.default_device())
    finally:
        del os.environ['KPAL_QUAD_STEPS']
        del os.environ['KPAL_QUAD_STEPS2']
    rs = np.random.RandomState(int(steps))
    uniform = oracle.synth_reads(61, 0, 40000, 150, noisy=True)
    at_rich = np.frombuffer(b'ACGT', dtype=np.uint8)[rs.choice(4, size=5 << 20, p=[.4, .1, .1, .4])].copy()
    at_rich[::151] = 10
    at_rich[2 << 20:(2 << 20) + 300000] = ord('A')
    level1_sizes = {'partition_quads': (8, 7, 6, 4, 3, 2, 1), 'partition2_quads': (8, 7, 6, 3)}
    for k, strategy in ((12, 'partition_quads'), (10, 'partition_quads'), (13, 'partition2_quads'), (14, 'partition2_quads')):
        for data in (uniform, at_rich):
            assert np.array_equal(c2.count_bytes(k, data, strategy), oracle.count_flat(data, k, threads=8)), (k, strategy, steps)
            name, s1, s2 = c2.count_last_plan()
            assert name == strategy
            if int(steps) in level1_sizes[strategy]:
                assert s1 == int(steps), (strategy, steps, s1)
            if strategy == 'partition2_quads':
                assert s2 == int(steps2), (strategy, steps2, s2)
    c2.close()


def test_quad_tile_sizes_are_sampled_once_per_16_feeds():
    """A count streamed in feeds of about one size samples its row loads for the first feed and keeps the tile sizes for the
    next 16 (quad_plan.hpp: QuadTileCache); the 18th feed samples again, and so does a feed of more than twice the kept size.
    Seen in the launches of quad_sample, one- and two-level; the table is the sum of the feeds."""
    from kpal_amd import _native
    c2 = _native.Context(_native.default_device())
    c2.prof_enable(True)
    small = oracle.synth_reads(67, 0, 13889, 150)[:2 << 20]
    large = oracle.synth_reads(68, 0, 41666, 150)[:6 << 20]

    def samples():
        c2.sync()
        return c2.prof_get().get('quad_sample', (0.0, 0))[1]
    for k, strategy in ((10, 'partition_quads'), (12, 'partition_quads'), (13, 'partition2_quads')):
        c2.prof_reset()
        c2.count_begin(k, strategy)
        for _ in range(17):
            c2.count_feed(small)
        assert samples() == 1, k
        c2.count_feed(small)
        assert samples() == 2, k
        c2.count_feed(large)
        assert samples() == 3, k
        assert c2.count_last_plan()[0] == strategy
        want = 18 * oracle.count_flat(small, k, threads=8) + oracle.count_flat(large, k, threads=8)
        assert np.array_equal(c2.count_finish(), want), k
    c2.close()


def test_quad_pipelines_halve_an_oversized_piece():
    """A piece whose record pool would pass the limit of the quad scatters' 32-bit record offsets is counted as two
    halves, recursively (forced here by lowering the limit to 4 MiB); halo across the seams of the halves."""
    from kpal_amd import _native
    os.environ['KPAL_QUAD_POOL_MAX'] = str(4 << 20)
    try:
        c2 = _native.Context(_native.default_device())
    finally:
        del os.environ['KPAL_QUAD_POOL_MAX']
    buf = oracle.synth_reads(59, 0, 120000, 150, noisy=True)            # 18 MB: pool ~21 MiB -> several halvings
    seq = np.ascontiguousarray(buf.reshape(-1, 151)[:, :150]).reshape(-1)
    for k, strategy in ((12, 'partition_quads'), (9, 'partition_quads'), (13, 'partition2_quads'), (15, 'partition2_quads')):
        for data in (buf, seq):
            assert np.array_equal(c2.count_bytes(k, data, strategy), oracle.count_flat(data, k, threads=8)), (k, strategy)
    c2.close()


@pytest.mark.parametrize('mode', ['0', '1', '2'])
def test_two_level_variants_of_level2(mode):
    """The three level-2 pipelines of the two-level path (KPAL_LEVEL2: 0 count + exact offsets, 1 chunked
    per-tile runs, 2 chunked aligned lines = default) against the oracle, including skewed input."""
    from kpal_amd import _native
    os.environ['KPAL_LEVEL2'] = mode
    try:
        c2 = _native.Context(_native.default_device())
    finally:
        del os.environ['KPAL_LEVEL2']
    rs = np.random.RandomState(int(mode) + 3)
    buf = oracle.synth_reads(53, 0, 30000, 150, noisy=True)
    skew = np.frombuffer(b'ACGT', dtype=np.uint8)[rs.choice(4, size=6 << 20, p=[.4, .1, .1, .4])].copy()
    skew[1 << 20:(1 << 20) + 700000] = ord('A')                       # a stretch that abandons tiles
    skew[3 << 20:(3 << 20) + 300000] = np.resize(np.frombuffer(b'AC', dtype=np.uint8), 300000)
    for k in (13, 14):
        for data in (buf, skew):
            np.testing.assert_array_equal(c2.count_bytes(k, data), oracle.count_flat(data, k, threads=8))
    c2.close()


def test_chunk_overflow_lists(ctx):
    """A steadily hot bucket (70 % A: one scrambled bucket still receives ~6 % of all k-mers, ~1600 per
    tile -- no tile is abandoned) makes workgroups retire far more than the four chunks a table row
    holds: the overflow list, its grouping kernel and the slicing of the histogram stage."""
    rs = np.random.RandomState(91)
    n = 384 << 20
    buf = np.frombuffer(b'ACGT', dtype=np.uint8)[rs.choice(4, size=n, p=[.7, .1, .1, .1])]
    d = ctx.alloc(n)       # one device feed: a workgroup's share must be large enough to fill many chunks
    try:
        ctx.h2d(d, buf)
        for k, strat in ((12, 'auto'), (12, 'partition_chunked'), (12, 'partition_quads'), (13, 'auto'), (12, 'partition')):
            ctx.count_begin(k, strat)
            ctx.count_feed_device(d, n)
            np.testing.assert_array_equal(ctx.count_finish(), oracle.count_flat(buf, k, threads=32), err_msg='k=%d %s' % (k, strat))
    finally:
        ctx.free(d)


def test_mixed_feeds_in_one_count(ctx):
    """Host, device and FASTA feeds of very different sizes inside one begin/finish (AUTO switches
    between the atomic kernel for tiny feeds and the partition pipelines): the table is the sum."""
    buf = oracle.synth_reads(61, 0, 40000, 150, noisy=True)
    pieces = [buf[:10], buf[10:1000], buf[1000:300000], buf[300000:300001], buf[300001:]]
    fasta = b'>x\nACGTACGTACGTAAAC\nGGGTTT\n>y\nNNNN\nACGTTGCAACGTTGCA\n'
    fasta_seqs = ['ACGTACGTACGTAAACGGGTTT', 'NNNNACGTTGCAACGTTGCA']
    for k in (9, 12, 13):
        ctx.count_begin(k)
        want = np.zeros(4 ** k, dtype=np.int64)
        for i, piece in enumerate(pieces):
            if i % 2:
                d = ctx.alloc(max(piece.size, 16))
                ctx.h2d(d, piece)
                ctx.count_feed_device(d, piece.size)
                ctx.sync()
                ctx.free(d)
            else:
                ctx.count_feed(piece)
            want += oracle.count_flat(piece, k)
        ctx.count_feed_fasta(fasta)
        want += oracle.from_sequences(fasta_seqs, k)
        np.testing.assert_array_equal(ctx.count_finish(), want)


def test_small_partition_batches():
    """Partition path with 1 MiB batches: halo across batch seams inside one device feed."""
    from kpal_amd import _native
    os.environ['KPAL_BATCH_BYTES'] = str(1 << 20)
    try:
        c2 = _native.Context(_native.default_device())
    finally:
        del os.environ['KPAL_BATCH_BYTES']
    buf = oracle.synth_reads(43, 0, 40000, 150, noisy=True)
    seq = np.ascontiguousarray(buf.reshape(-1, 151)[:, :150]).reshape(-1)
    for k in (8, 12):
        np.testing.assert_array_equal(c2.count_bytes(k, buf, 'partition'), oracle.count_flat(buf, k, threads=4))
        np.testing.assert_array_equal(c2.count_bytes(k, seq, 'partition'), oracle.count_flat(seq, k, threads=4))
        np.testing.assert_array_equal(c2.count_bytes(k, buf, 'partition_chunked'), oracle.count_flat(buf, k, threads=4))
        np.testing.assert_array_equal(c2.count_bytes(k, seq, 'partition_chunked'), oracle.count_flat(seq, k, threads=4))
        np.testing.assert_array_equal(c2.count_bytes(k, buf, 'partition_quads'), oracle.count_flat(buf, k, threads=4))
        np.testing.assert_array_equal(c2.count_bytes(k, seq, 'partition_quads'), oracle.count_flat(seq, k, threads=4))
    c2.close()


def test_skewed_input_homopolymer(ctx):
    # every k-mer identical: one bucket, one bin (worst-case contention / bucket skew)
    buf = np.full(3_000_000, ord('A'), dtype=np.uint8)
    for k in (3, 12, 14):
        for strat in strategies(k):
            c = ctx.count_bytes(k, buf, strat)
            assert c[0] == buf.size - k + 1 and c.sum() == c[0], (k, strat)
    buf = np.frombuffer(b'ACGT' * 500000, dtype=np.uint8)
    for k in (9, 12):
        c = ctx.count_bytes(k, buf)
        np.testing.assert_array_equal(c, oracle.count_flat(buf, k))


@pytest.mark.parametrize('k,n_reads', [(12, 100_000_000), (9, 20_000_000)])
def test_full_size_properties_k12(ctx, k, n_reads):
    """BASELINE config 2 at full size (100 M x 150 bp, k = 12; and 20 M reads at k = 9) through AUTO (the quad pipeline,
    asserted): exact total, linearity over two shards, the chunked pipeline bin for bin at full size, the global-atomic kernel
    on a 10 M-read prefix, balance of every bin against the oracle -- and the WHOLE input (15.1 GB at k = 12) downloaded and
    counted by the all-cores CPU oracle, every bin compared."""
    from kpal_amd import dist
    nbytes = n_reads * 151
    d = ctx.alloc(nbytes)
    try:
        ctx.synth_reads_device(2, 0, n_reads, 150, d)
        ctx.count_begin(k)
        ctx.count_feed_device(d, nbytes)
        assert ctx.count_last_plan()[0] == 'partition_quads'
        full = ctx.count_finish()
        assert full.sum() == n_reads * (150 - k + 1)
        assert full.min() >= 0
        # linearity: counting two shards separately and adding gives the same table
        first, n0 = dist.shard_range(n_reads, 0, 2)
        parts = []
        for r in range(2):
            f, n = dist.shard_range(n_reads, r, 2)
            ctx.count_begin(k)
            ctx.count_feed_device(d + f * 151, n * 151)
            parts.append(ctx.count_finish())
        np.testing.assert_array_equal(parts[0] + parts[1], full)
        # the chunked round-1 pipeline agrees bin for bin at full size (key indices beyond 2^31)
        for strat in ('partition_chunked',):
            ctx.count_begin(k, strat)
            ctx.count_feed_device(d, nbytes)
            np.testing.assert_array_equal(ctx.count_finish(), full, err_msg=strat)
        # alternative strategy agrees on a 10 M-read prefix
        ctx.count_begin(k, 'global_atomic')
        ctx.count_feed_device(d, 10_000_000 * 151)
        a = ctx.count_finish()
        ctx.count_begin(k)
        ctx.count_feed_device(d, 10_000_000 * 151)
        np.testing.assert_array_equal(ctx.count_finish(), a)
        # the oracle on the WHOLE input: all reads downloaded, counted on the host cores (shared table, 16 threads)
        host = np.empty(nbytes, dtype=np.uint8)
        ctx.d2h(host, d)
        want = oracle.count_flat(host, k, threads=16)
        del host
        np.testing.assert_array_equal(full, want)
        del want
        # balance on the device table doubles the total (klib.py:285-298)
        ctx.count_begin(k)
        ctx.count_feed_device(d, nbytes)
        ctx.count_finish(to_host=False)
        ptr, bins = ctx.count_table()
        ctx.balance_device(k, ptr)
        bal = np.empty(bins, dtype=np.int64)
        ctx.d2h(bal, ptr)
        assert bal.sum() == 2 * full.sum()
        np.testing.assert_array_equal(bal, oracle.balance(full, k))   # every bin (klib.py:285-298)
    finally:
        ctx.free(d)


def test_full_size_k15(ctx):
    """BASELINE config 4 at its stated size (k = 15, 100 M x 150 bp reads, seed 4, 8 GiB table).  AUTO takes the two-level
    QUAD pipeline here (quad_scatter<15> -> quad2_scatter -> quad_hist -> quad2_finalize; asserted through
    kpal_count_last_plan) -- the pipeline bench.py --k 15 measures.  Checked at 100 M reads: exact total, no negative bin, and
    the whole 8 GiB table bin for bin against the round-1 two-level pipeline ('partition2': coarse_scatter -> chunk_key_lines
    -> chunk_hist, independent kernels and data layout) run on the same buffer by a second context, compared on the device;
    linearity over two half-shards.  AGAINST THE ORACLE AT FULL SIZE: the 15.1 GB of reads are downloaded and the all-cores
    CPU oracle (oracle.count_blocks, pinned to the golden count by tests/test_oracle_golden.py) counts 64 blocks of 2^20
    table entries -- the first and the last block, CCCCC / GGGGG, blocks together with the block of their reverse
    complements, the rest spread over the table: 2^26 bins, 512 MiB -- plain AND balanced (Profile.balance = the block's
    counts + the counts of the entries' reverse complements, which lie all over the table), compared with the tables the
    benchmarked pipeline produced from the same 100 M reads (kpal_count_finish / kpal_count_balance: FRESH mode, packed
    histogram bins, 8-bit staged forms, fused balance -- the regime bench.py --k 15 times).  With the quad pipeline FORCED
    on prefixes AUTO would hand to 'partition2': bin for bin against the global-atomic kernel (10 M reads) and against the
    CPU oracle on ALL bins (2 M reads)."""
    torch = pytest.importorskip('torch')
    from kpal_amd import _native, dist
    k, n_reads = 15, 100_000_000
    nbytes = n_reads * 151
    d = ctx.alloc(nbytes)
    other = _native.Context(ctx.device)
    # blocks of 2^20 consecutive entries (a block = the k-mers with one 5-base prefix) the oracle counts at full size
    block_bits = 20
    rs = np.random.RandomState(15)
    sel = [0, 1023, 341, 682, 27, oracle.reverse_complement(27, 5), 600, oracle.reverse_complement(600, 5), 1, 1022, 512, 511]
    sel += [int(b) for b in rs.permutation(1024) if int(b) not in sel][:64 - len(sel)]
    assert len(set(sel)) == 64
    try:
        sel_t = torch.as_tensor(sel, device='cuda:%d' % ctx.device)
        ctx.synth_reads_device(4, 0, n_reads, 150, d)
        ctx.count_begin(k)
        ctx.count_feed_device(d, nbytes)
        assert ctx.count_last_plan()[0] == 'partition2_quads'
        ctx.count_finish(to_host=False)
        ctx.sync()
        full = dist.table_as_tensor(ctx)
        assert full.numel() == 4 ** k
        assert int(full.sum()) == n_reads * (150 - k + 1)
        assert int(full.min()) >= 0
        # the same 100 M reads through the round-1 two-level pipeline: every one of the 4^15 bins
        other.count_begin(k, 'partition2')
        other.count_feed_device(d, nbytes)
        assert other.count_last_plan()[0] == 'partition2'
        other.count_finish(to_host=False)
        other.sync()
        assert torch.equal(dist.table_as_tensor(other), full)
        torch.cuda.synchronize()
        # count + balance as bench.py --k 15 times it: Profile.balance fused into the finalisation of the quad pipeline
        # (kpal_count_balance) against the round-1 pipeline's table balanced by the stand-alone kernel -- all 4^15 bins
        other.balance_device(k, other.count_table()[0])
        other.sync()
        ctx.count_begin(k)
        ctx.count_feed_device(d, nbytes)
        ctx.count_balance()
        ctx.count_finish(to_host=False)
        ctx.sync()
        bal = dist.table_as_tensor(ctx)
        assert int(bal.sum()) == 2 * n_reads * (150 - k + 1)
        assert torch.equal(bal, dist.table_as_tensor(other))
        bal_blocks = bal.view(-1, 1 << block_bits)[sel_t].cpu().numpy()
        torch.cuda.synchronize()
        ctx.count_begin(k)                       # the unbalanced table again, for the checks below
        ctx.count_feed_device(d, nbytes)
        ctx.count_finish(to_host=False)
        ctx.sync()
        full = dist.table_as_tensor(ctx)
        full_blocks = full.view(-1, 1 << block_bits)[sel_t].cpu().numpy()
        # linearity: the two half-shards counted by the second context (quad pipeline) add up to the same table
        half = n_reads // 2
        other.count_begin(k)
        other.count_feed_device(d, half * 151)
        assert other.count_last_plan()[0] == 'partition2_quads'
        other.count_finish(to_host=False)
        other.sync()
        acc = dist.table_as_tensor(other).clone()
        torch.cuda.synchronize()                 # torch's stream is not the context's: the copy must be done before the table is zeroed
        other.count_begin(k)
        other.count_feed_device(d + half * 151, half * 151)
        other.count_finish(to_host=False)
        other.sync()
        acc += dist.table_as_tensor(other)
        assert torch.equal(acc, full)
        del acc
        torch.cuda.synchronize()
        # the quad pipeline, forced, bin for bin with the global-atomic kernel on a 10 M-read prefix (both tables stay on the device)
        pre10 = 10_000_000 * 151
        ctx.count_begin(k, 'partition2_quads')
        ctx.count_feed_device(d, pre10)
        assert ctx.count_last_plan()[0] == 'partition2_quads'
        ctx.count_finish(to_host=False)
        other.count_begin(k, 'global_atomic')
        other.count_feed_device(d, pre10)
        other.count_finish(to_host=False)
        ctx.sync()
        other.sync()
        assert torch.equal(dist.table_as_tensor(ctx), dist.table_as_tensor(other))
        torch.cuda.synchronize()
        # the quad pipeline, forced, bin for bin with the oracle on a 2 M-read prefix
        pre = np.empty(2_000_000 * 151, dtype=np.uint8)
        ctx.d2h(pre, d)
        ctx.count_begin(k, 'partition2_quads')
        ctx.count_feed_device(d, pre.size)
        got = ctx.count_finish()
        want = oracle.count_flat(pre, k, threads=8)
        assert got.sum() == 2_000_000 * (150 - k + 1)
        assert np.array_equal(got, want)
        del got, want, pre
        # the oracle at FULL size on the selected blocks: all 100 M reads downloaded, counted on the host cores
        host = np.empty(nbytes, dtype=np.uint8)
        ctx.d2h(host, d)
        plain, mirror = oracle.count_blocks(host, k, block_bits, sel, threads=min(32, os.cpu_count() or 1))
        del host
        assert int(plain.sum()) > 0.05 * n_reads * (150 - k + 1)      # 64 of 1024 blocks of uniform reads: ~6 % of the k-mers
        np.testing.assert_array_equal(full_blocks, plain)
        np.testing.assert_array_equal(bal_blocks, plain + mirror)
    finally:
        other.close()
        ctx.free(d)


@pytest.mark.parametrize('mode', ['0', '1', '2'])
def test_two_level_k15_against_oracle(mode):
    """k = 15 (64 coarse buckets) through every level-2 pipeline, on inputs large enough for AUTO to take
    the two-level path (feeds above 256 KiB), bin for bin against the oracle: noisy reads, one unbroken
    sequence, and skewed composition with a tile-abandoning homopolymer stretch."""
    from kpal_amd import _native
    os.environ['KPAL_LEVEL2'] = mode
    try:
        c2 = _native.Context(_native.default_device())
    finally:
        del os.environ['KPAL_LEVEL2']
    rs = np.random.RandomState(int(mode) + 15)
    buf = oracle.synth_reads(54, 0, 40000, 150, noisy=True)
    seq = np.ascontiguousarray(buf.reshape(-1, 151)[:, :150]).reshape(-1)
    skew = np.frombuffer(b'ACGT', dtype=np.uint8)[rs.choice(4, size=5 << 20, p=[.4, .1, .1, .4])].copy()
    skew[1 << 20:(1 << 20) + 700000] = ord('A')
    skew[3 << 20:(3 << 20) + 300000] = np.resize(np.frombuffer(b'AC', dtype=np.uint8), 300000)
    try:
        for data in (buf, seq, skew):
            want = oracle.count_flat(data, 15, threads=8)
            got = c2.count_bytes(15, data, 'partition2')
            assert np.array_equal(got, want)
            del got
            if mode == '2':      # and the two-level quad pipeline (level-1 records, level-2 records, staged forms + combine)
                got = c2.count_bytes(15, data, 'partition2_quads')
                assert np.array_equal(got, want)
                del got
    finally:
        c2.close()


def test_count_balance_fused_with_the_finalisation():
    """kpal_count_balance (count + balance, the unit of the north-star metric).  On the two-level quad pipeline the balance
    is fused into the pass that adds the staged forms to the table (quad2_finalize_kernel<K, true>): against
    oracle.balance(oracle.count) for k = 13 (k = 14 -- even k: finalisation sets that are their own reverse complement -- in
    test_fresh_table_of_the_two_level_quad_pipeline) on one unbroken sequence and skewed composition, fed from the HOST (classic
    finalisation: the table is zeroed and read); with two feeds (the first one's forms are flushed
    unbalanced, the second's finalisation balances the sum); with entries beyond 32 bits already in the table; through
    kpal_balance_device on the table pointer; and on the pipelines without a staged finalisation (k = 5, 12: the
    stand-alone balance kernel).  k = 15 / 16 (8 / 32 GiB tables): test_full_size_k15, test_count_balance_fused_k16_on_device."""
    from kpal_amd import _native
    c2 = _native.Context(_native.default_device())
    rs = np.random.RandomState(23)
    buf = oracle.synth_reads(71, 0, 30000, 150, noisy=True)
    seq = np.ascontiguousarray(buf.reshape(-1, 151)[:, :150]).reshape(-1)
    skew = np.frombuffer(b'ACGT', dtype=np.uint8)[rs.choice(4, size=4 << 20, p=[.4, .1, .1, .4])].copy()
    skew[1 << 20:(1 << 20) + 500000] = ord('A')
    try:
        for k in (13,):
            for data in (seq, skew):
                want = oracle.balance(oracle.count_flat(data, k, threads=8), k)
                c2.count_begin(k, 'partition2_quads')
                c2.count_feed(data)
                assert c2.count_last_plan()[0] == 'partition2_quads'
                c2.count_balance()
                assert np.array_equal(c2.count_finish(), want), k
                del want
            if k != 13:
                continue
            # two feeds + entries beyond 32 bits that are already in the table when the last finalisation runs
            a, b = buf[:buf.size // 3], buf[buf.size // 3:]
            c2.count_begin(k, 'partition2_quads')
            c2.count_feed(a)
            ptr, bins = c2.count_table()
            big_at = np.array([0, 4 ** k - 1, 12345, 4 ** k // 2 + 77], dtype=np.int64)     # AAA.., TTT.. (partners), two others
            unb = oracle.count_flat(a, k) + oracle.count_flat(b, k)
            for j, at in enumerate(big_at):
                v = np.empty(1, dtype=np.int64)
                c2.d2h(v, ptr + int(at) * 8)
                v[0] += (1 << 40) + j
                c2.h2d(ptr + int(at) * 8, v)
                unb[at] += (1 << 40) + j
            c2.count_feed(b)
            c2.balance_device(k, ptr)            # == kpal_count_balance: the table pointer of a running count
            assert np.array_equal(c2.count_finish(), oracle.balance(unb, k)), k
            del unb
        for k in (5, 12):
            c2.count_begin(k)
            c2.count_feed(buf)
            c2.count_balance()
            assert np.array_equal(c2.count_finish(), oracle.balance(oracle.count_flat(buf, k), k))
    finally:
        c2.close()


@pytest.mark.parametrize('seg', [None, '8'])
def test_fresh_table_of_the_two_level_quad_pipeline(seg):
    """FRESH mode (k >= 13): kpal_count_begin leaves the table unzeroed, the first piece -- a whole DEVICE feed on the two-level
    quad pipeline -- lets its finalisation write the table without reading it, and the counts that bypass the records (items the
    spill list cannot hold, hot items, what is still carried when a scatter ends) wait in per-workgroup lists until then.
    Against the oracle: plain and balancing finalisation at k = 13 (k = 14: balancing), uniform and skewed input (homopolymer /
    two-letter stretches: the hot-item path), a second feed after a fresh piece, an empty count, feeds that take other
    pipelines, and -- seg = 8: list segments of eight entries, skewed input -- the overflow fallback (the table is zeroed after
    all and the piece counted again the classic way)."""
    from kpal_amd import _native
    if seg:
        os.environ['KPAL_DIRECT_SEG'] = seg
    try:
        c2 = _native.Context(_native.default_device())
    finally:
        os.environ.pop('KPAL_DIRECT_SEG', None)
    rs = np.random.RandomState(29)
    buf = oracle.synth_reads(73, 0, 30000, 150, noisy=True)
    skew = np.frombuffer(b'ACGT', dtype=np.uint8)[rs.choice(4, size=4 << 20, p=[.4, .1, .1, .4])].copy()
    skew[1 << 20:(1 << 20) + 500000] = ord('A')
    skew[3 << 20:(3 << 20) + 200000] = np.resize(np.frombuffer(b'AC', dtype=np.uint8), 200000)
    d = c2.alloc(max(buf.size, skew.size) + 64)
    try:
        for k, data in ((13, skew),) if seg else ((13, buf), (13, skew), (14, buf)):
            if True:
                want = oracle.count_flat(data, k, threads=8)
                c2.h2d(d, data)
                for balanced in (True,) if k == 14 else (False, True):
                    c2.count_begin(k, 'partition2_quads')
                    c2.count_feed_device(d, data.size)
                    assert c2.count_last_plan()[0] == 'partition2_quads'
                    if balanced:
                        c2.count_balance()
                    got = c2.count_finish()
                    assert np.array_equal(got, oracle.balance(want, k) if balanced else want), (k, balanced, seg)
                if k == 13 and data is buf:
                    # a second feed: the fresh piece is finalised (plain), the next one adds to a real table
                    c2.count_begin(k, 'partition2_quads')
                    c2.count_feed_device(d, data.size)
                    c2.count_feed_device(d, data.size // 2)
                    c2.count_balance()
                    assert np.array_equal(c2.count_finish(), oracle.balance(want + oracle.count_flat(data[:data.size // 2], k), k)), (k, seg)
                del want
        # nothing fed: the zeros are materialised on demand
        c2.count_begin(13, 'partition2_quads')
        assert int(c2.count_finish().sum()) == 0
        c2.count_begin(13)
        c2.count_balance()
        assert int(c2.count_finish().sum()) == 0
        # a tiny feed (atomic kernel) and a host feed after kpal_count_begin left the table unzeroed
        c2.h2d(d, skew)
        c2.count_begin(13)
        c2.count_feed(buf[:5000])
        c2.count_feed_device(d, 1000)
        assert np.array_equal(c2.count_finish(), oracle.count_flat(buf[:5000], 13) + oracle.count_flat(skew[:1000], 13))
    finally:
        c2.free(d)
        c2.close()


def test_staged_counts_beyond_eight_bits():
    """The histogram stage of the two-level quad pipeline stages 8-bit counts; a k-mer seen >= 256 times within ONE of its four
    item positions bypasses the staging (FRESH: the histogram stage's list segment; classic: atomic adds).  Input: a 300-base
    sequence repeated 1500 times (every k-mer ~375 times per position), one repeated 400 times (staged: ~100 per position) and one
    repeated 300 000 times (beyond 16 bits per position), shuffled among random reads.  k = 13 against the oracle
    (fresh, classic = second feed, balanced), k = 15 (packed histogram bins) against the global-atomic kernel on the device."""
    torch = pytest.importorskip('torch')
    from kpal_amd import _native, dist
    rs = np.random.RandomState(41)
    acgt = np.frombuffer(b'ACGT', dtype=np.uint8)
    blocks = [acgt[rs.randint(0, 4, size=300)].tobytes() for _ in range(2)]
    short = acgt[rs.randint(0, 4, size=40)].tobytes()
    reads = [blocks[0]] * 1500 + [blocks[1]] * 400 + [short] * 300000 + [acgt[rs.randint(0, 4, size=150)].tobytes() for _ in range(20000)]
    order = rs.permutation(len(reads))
    data = np.frombuffer(b'\n'.join(reads[i] for i in order), dtype=np.uint8)
    c2 = _native.Context(_native.default_device())
    other = _native.Context(_native.default_device())
    d = c2.alloc(data.size + 64)
    try:
        c2.h2d(d, data)
        k = 13
        want = oracle.count_flat(data, k, threads=8)
        assert want.max() >= 300000 and np.count_nonzero((want >= 1024) & (want < 65536)) > 200
        for balanced in (False, True):
            c2.count_begin(k, 'partition2_quads')
            c2.count_feed_device(d, data.size)                 # FRESH piece
            if balanced:
                c2.count_balance()
            got = c2.count_finish()
            assert np.array_equal(got, oracle.balance(want, k) if balanced else want), balanced
        c2.count_begin(k, 'partition2_quads')
        c2.count_feed_device(d, data.size)
        c2.count_feed_device(d, data.size)                     # classic: adds to a real table
        c2.count_balance()
        assert np.array_equal(c2.count_finish(), oracle.balance(2 * want, k))
        del want
        k = 15
        for feeds in (1, 2):
            c2.count_begin(k, 'partition2_quads')
            other.count_begin(k, 'global_atomic')
            for _ in range(feeds):
                c2.count_feed_device(d, data.size)
                other.count_feed_device(d, data.size)
            assert c2.count_last_plan()[0] == 'partition2_quads'
            c2.count_finish(to_host=False)
            other.count_finish(to_host=False)
            c2.sync()
            other.sync()
            assert torch.equal(dist.table_as_tensor(c2), dist.table_as_tensor(other)), feeds
            torch.cuda.synchronize()
    finally:
        c2.free(d)
        c2.close()
        other.close()


def test_count_balance_fused_k16_on_device():
    """k = 16 (32 GiB table, self-paired finalisation sets exist for even k): the fused finalisation + balance against the
    plain finalisation followed by the stand-alone balance kernel, compared on the device; and the plain finalisation
    against the global-atomic kernel."""
    torch = pytest.importorskip('torch')
    from kpal_amd import _native, dist
    k = 16
    buf = oracle.synth_reads(72, 0, 60000, 150, noisy=True)
    a = _native.Context(_native.default_device())
    b = _native.Context(_native.default_device())
    try:
        a.count_begin(k, 'partition2_quads')
        a.count_feed(buf)
        assert a.count_last_plan()[0] == 'partition2_quads'
        a.count_finish(to_host=False)            # plain finalisation
        b.count_begin(k, 'global_atomic')
        b.count_feed(buf)
        b.count_finish(to_host=False)
        a.sync()
        b.sync()
        ta, tb = dist.table_as_tensor(a), dist.table_as_tensor(b)
        assert int(ta.sum()) == int(tb.sum()) > 0
        assert torch.equal(ta, tb)
        torch.cuda.synchronize()
        b.balance_device(k, b.count_table()[0])  # stand-alone balance of the atomic kernel's table
        a.count_begin(k, 'partition2_quads')
        a.count_feed(buf)
        a.count_balance()                        # fused
        a.count_finish(to_host=False)
        a.sync()
        b.sync()
        assert torch.equal(dist.table_as_tensor(a), dist.table_as_tensor(b))
        torch.cuda.synchronize()
    finally:
        a.close()
        b.close()


def test_partition_pipelines_on_skewed_inputs(ctx):
    """Both k = 8..12 pipelines against the oracle on inputs that stress the chunk logic: skewed
    composition (buckets of very different sizes), long homopolymer / tandem-repeat stretches inside
    random sequence (rows overflowing into direct stores across chunk ends, abandoned tiles), runs of
    N, and one bucket receiving almost everything."""
    rs = np.random.RandomState(77)
    acgt = np.frombuffer(b'ACGT', dtype=np.uint8)
    n = 48 << 20

    def rnd(p, size):
        return acgt[rs.choice(4, size=size, p=p)]

    cases = {}
    cases['at_rich'] = rnd([.4, .1, .1, .4], n)
    mixed = rnd([.25, .25, .25, .25], n)
    at = 0
    while at < n - (1 << 20):                     # stretches of 2 KB .. 1 MB every ~1 MB
        length = int(rs.choice([2048, 10000, 70000, 300000, 1 << 20]))
        unit = [b'A', b'AC', b'AAT', b'ACGTT', b'N'][rs.randint(5)]
        mixed[at:at + length] = np.resize(np.frombuffer(unit, dtype=np.uint8), length)
        at += length + rs.randint(1 << 18, 1 << 21)
    cases['stretches'] = mixed
    mostly_a = np.full(n, ord('A'), dtype=np.uint8)
    idx = rs.randint(0, n, n // 50)
    mostly_a[idx] = rnd([.25, .25, .25, .25], idx.size)
    cases['mostly_a'] = mostly_a
    for name, buf in cases.items():
        for k in (12, 9):
            want = oracle.count_flat(buf, k, threads=8)
            for strat in ('partition_quads', 'partition_chunked', 'partition'):
                np.testing.assert_array_equal(ctx.count_bytes(k, buf, strat), want, err_msg='%s k=%d %s' % (name, k, strat))
        want = oracle.count_flat(buf, 13, threads=8)       # the two-level pipelines (level-1 rows, hot-item table, level 2)
        for strat in ('partition2_quads', 'partition2'):
            assert np.array_equal(ctx.count_bytes(13, buf, strat), want), '%s k=13 %s' % (name, strat)


def _kmers_numpy(buf, k, read_len=150):
    """All valid k-mer indices of '\\n'-terminated fixed-length reads, vectorised on the host."""
    lut = np.full(256, 255, dtype=np.uint8)
    for ch, v in zip(b'ACGTacgt', (0, 1, 2, 3, 0, 1, 2, 3)):
        lut[ch] = v
    codes = lut[buf.reshape(-1, read_len + 1)[:, :read_len]]
    n_win = read_len - k + 1
    idx = np.zeros((codes.shape[0], n_win), dtype=np.uint64)
    bad = np.zeros((codes.shape[0], n_win), dtype=bool)
    for i in range(k):
        c = codes[:, i:i + n_win]
        bad |= c == 255
        idx = (idx << np.uint64(2)) | (c & 3).astype(np.uint64)
    return idx[~bad]


def test_k16_two_level_on_device(ctx):
    """k = 16 (32 GiB table, never copied to the host): the two-level partition path against the
    k-mers enumerated with NumPy and against the global-atomic kernel, compared on the device."""
    torch = pytest.importorskip('torch')
    from kpal_amd import _native, dist
    k, n_reads = 16, 150_000
    buf = oracle.synth_reads(16, 0, n_reads, 150, noisy=True)
    want_idx, want_cnt = np.unique(_kmers_numpy(buf, k), return_counts=True)
    d = ctx.alloc(buf.size)
    other = _native.Context(ctx.device)
    try:
        ctx.h2d(d, buf)
        ctx.count_begin(k)                       # auto -> partition2
        ctx.count_feed_device(d, buf.size)
        ctx.count_feed(b'GATTACAGATTACACATGCATGCAAACCCGGGTTT')   # + a short host feed
        ctx.count_finish(to_host=False)
        ctx.sync()
        t = dist.table_as_tensor(ctx)
        assert t.numel() == 4 ** k
        extra = np.array([_enc(b'GATTACAGATTACACATGCATGCAAACCCGGGTTT'[i:i + k]) for i in range(35 - k + 1)], dtype=np.uint64)
        all_idx, all_cnt = np.unique(np.concatenate([np.repeat(want_idx, want_cnt), extra]), return_counts=True)
        assert int(t.sum()) == int(all_cnt.sum())
        assert int(torch.count_nonzero(t)) == all_idx.size
        got = t[torch.as_tensor(all_idx.astype(np.int64), device=t.device)].cpu().numpy()
        np.testing.assert_array_equal(got, all_cnt)
        other.count_begin(k, 'global_atomic')
        other.count_feed(buf)
        other.count_feed(b'GATTACAGATTACACATGCATGCAAACCCGGGTTT')
        other.count_finish(to_host=False)
        other.sync()
        assert torch.equal(t, dist.table_as_tensor(other))
    finally:
        ctx.free(d)
        other.close()


def test_from_sequences_through_the_gatherer(ctx, monkeypatch):
    """Profile.from_sequences on lists / tuples / generators of bytes, str, bytearray, memoryview and str with characters
    beyond latin-1 (separators, like every non-nucleotide: klib.py:152) goes through the C gatherer (kpal_amd/csrc/kpal_gather.c)
    and kpal_count_feed_pinned: with the usual 64 MiB buffer and with a 4 KiB one (buffer full in the middle of the list, a
    sequence longer than the buffer, foreign items at a buffer's end), against the oracle and against the interpreter's join."""
    from kpal_amd import klib
    assert klib._kpal_gather is not None, 'the gatherer extension was not built'
    rs = np.random.RandomState(8)
    reads = oracle.synth_reads(61, 0, 3000, 150, noisy=True).reshape(-1, 151)[:, :150]
    items = []
    for i, r in enumerate(reads):
        b = bytes(r[:rs.randint(0, 151)])
        items.append([b, b.decode(), bytearray(b), memoryview(b), b.decode() + 'ሴ' + 'ACGTACGTACGTA'][i % 5])
    items[100] = bytes(np.frombuffer(b'ACGT', dtype=np.uint8)[rs.randint(0, 4, 20000)])       # longer than the small buffer
    items[2000] = ('ACGTTGCA' * 1000) + '中' + 'TTGACCA' * 50                            # foreign AND longer than the small buffer
    as_text = [bytes(x).decode('latin-1') if not isinstance(x, str) else x.encode('latin-1', 'replace').decode('latin-1') for x in items]
    for k in (3, 9, 12):
        want = oracle.from_sequences(as_text, k)
        for shape in (list, tuple, iter):
            p = klib.Profile.from_sequences(shape(items), k)
            np.testing.assert_array_equal(p.counts, want, err_msg='k=%d %s' % (k, shape.__name__))
    small = ctx.host_alloc(4096)
    from kpal_amd import _native
    default = _native.context()
    saved = getattr(default, '_gather_buffer', None)
    try:
        default._gather_buffer = small
        for k in (4, 11):
            want = oracle.from_sequences(as_text, k)
            np.testing.assert_array_equal(klib.Profile.from_sequences(items, k).counts, want)
            np.testing.assert_array_equal(klib.Profile.from_sequences(iter(items), k).counts, want)
    finally:
        default._gather_buffer = saved
        ctx.host_free(small[0])
    # a page-locked buffer larger than one 64 MiB staging piece fed in place: the seams carry their k - 1 bytes of halo
    big = oracle.synth_reads(62, 0, 900000, 150, noisy=True)                     # 136 MB
    seq = np.ascontiguousarray(big.reshape(-1, 151)[:, :150]).reshape(-1)        # one unbroken sequence: every seam matters
    address, view = ctx.host_alloc(seq.size)
    try:
        view[:] = seq
        for k in (5, 12):
            ctx.count_begin(k)
            ctx.count_feed_pinned(address, seq.size)
            np.testing.assert_array_equal(ctx.count_finish(), oracle.count_flat(seq, k, threads=8))
    finally:
        ctx.host_free(address)
    with pytest.raises(ValueError):
        ctx.host_free(address)                                                   # not (any more) a buffer of this context
    # the interpreter's join (no extension) gives the same stream
    monkeypatch.setattr(klib, '_kpal_gather', None)
    np.testing.assert_array_equal(klib.Profile.from_sequences(items, 9).counts, oracle.from_sequences(as_text, 9))
    # empty inputs
    assert klib.Profile.from_sequences([], 5).total == 0 and klib.Profile.from_sequences([b'', ''], 5).total == 0
    with pytest.raises(ValueError):
        ctx.count_begin(5)
        ctx.count_feed_pinned(np.zeros(64, dtype=np.uint8).ctypes.data, 64)      # not page-locked memory
    ctx.count_finish()


def test_k12_staged_forms_and_fused_balance():
    """The one-level quad pipeline at k = 12 stages the four forms of its histogram stage as 8-bit counts and lets
    quad2_finalize_kernel<12> add them to the table -- balanced in the same pass when kpal_count_balance asks (what bench.py times
    at k = 12) -- instead of 67 M global atomics + a stand-alone balance.  Against the oracle: uniform noisy reads (40 MiB: AUTO
    takes the quad pipeline), plain and balanced; TWO feeds into one count (the first feed's pending forms are flushed before
    the second is staged), balanced; repeats whose counts do not fit a staged form (a 300-base sequence 1500 times: ~375 per
    position; a 40-base one 300 000 times); a device feed; and the atomic merge (KPAL_K12_STAGED=0) as the cross-check, which
    must give the same tables (its histogram bins are kept in the staging order too)."""
    from kpal_amd import _native
    rs = np.random.RandomState(12)
    acgt = np.frombuffer(b'ACGT', dtype=np.uint8)
    k = 12
    uniform = oracle.synth_reads(71, 0, 280000, 150, noisy=True)                 # 42 MB
    blocks = [acgt[rs.randint(0, 4, size=300)].tobytes() for _ in range(2)]
    short = acgt[rs.randint(0, 4, size=40)].tobytes()
    reads = [blocks[0]] * 1500 + [blocks[1]] * 400 + [short] * 300000 + [acgt[rs.randint(0, 4, size=150)].tobytes() for _ in range(150000)]
    order = rs.permutation(len(reads))
    repeats = np.frombuffer(b'\n'.join(reads[i] for i in order), dtype=np.uint8)
    assert repeats.size > (32 << 20)
    os.environ['KPAL_K12_STAGED'] = '0'
    try:
        atomic = _native.Context(_native.default_device())
    finally:
        del os.environ['KPAL_K12_STAGED']
    staged = _native.Context(_native.default_device())
    try:
        for data in (uniform, repeats):
            want = oracle.count_flat(data, k, threads=8)
            wantb = oracle.balance(want, k)
            # (AUTO hands the repeats to the chunked pipeline: the quad pipeline is forced there)
            strategy = 'auto' if data is uniform else 'partition_quads'
            for c in (staged, atomic):
                c.count_begin(k, strategy)
                c.count_feed(data)
                assert c.count_last_plan()[0] == 'partition_quads'
                np.testing.assert_array_equal(c.count_finish(), want)
                c.count_begin(k, strategy)
                c.count_feed(data)
                c.count_balance()
                np.testing.assert_array_equal(c.count_finish(), wantb)
                c.count_begin(k, strategy)            # two feeds, then balance: 2 x the counts
                c.count_feed(data)
                c.count_feed(data)
                c.count_balance()
                np.testing.assert_array_equal(c.count_finish(), 2 * wantb)
        assert oracle.count_flat(repeats, k).max() >= 300000
        d = staged.alloc(uniform.size + 64)
        staged.h2d(d + 3, uniform)
        staged.count_begin(k, 'partition_quads')
        staged.count_feed_device(d + 3, uniform.size)
        staged.count_balance()
        ptr, bins = staged.count_table()
        got = np.empty(bins, dtype=np.int64)
        staged.d2h(got, ptr)
        np.testing.assert_array_equal(got, oracle.balance(oracle.count_flat(uniform, k, threads=8), k))
        staged.count_finish(to_host=False)
        staged.free(d)
    finally:
        staged.close()
        atomic.close()


@pytest.mark.gpu
def test_auto_two_level_choice_fresh_and_later_pieces(ctx):
    """AUTO at k >= 13 (count_plan.hpp: plan_strategy / kpal_count.hip: count_device_range): the FIRST piece of a count that is a whole device buffer of at least
    64 MiB and an eighth of a byte per table entry goes through the two-level quad pipeline (FRESH table, fused balance); a later
    piece only once it holds three bytes per entry -- below that the round-1 two-level pipeline adds into the finished table.
    Both orders, with and without the balance, against the oracle run on the whole input."""
    k, n_reads = 13, 560_000                              # 84.6 MB per piece; 4^13 / 8 = 8.4 MB, 3 * 4^13 = 201 MB
    nbytes = n_reads * 151
    host = oracle.synth_reads(77, 0, 2 * n_reads, 150, noisy=True)
    want = oracle.count_flat(host, k, threads=8)
    d = ctx.alloc(2 * nbytes)
    try:
        ctx.h2d(d, host)
        for balance in (False, True):
            ctx.count_begin(k)
            ctx.count_feed_device(d, nbytes)
            assert ctx.count_last_plan()[0] == 'partition2_quads'
            ctx.count_feed_device(d + nbytes, nbytes)
            assert ctx.count_last_plan()[0] == 'partition2'
            if balance:
                ctx.count_balance()
            got = ctx.count_finish()
            np.testing.assert_array_equal(got, oracle.balance(want, k) if balance else want)
        # one piece of both halves: still the first piece of its count
        ctx.count_begin(k)
        ctx.count_feed_device(d, 2 * nbytes)
        assert ctx.count_last_plan()[0] == 'partition2_quads'
        np.testing.assert_array_equal(ctx.count_finish(), want)
        # a first piece below 64 MiB stays with the round-1 pipeline
        ctx.count_begin(k)
        ctx.count_feed_device(d, 40 << 20)
        assert ctx.count_last_plan()[0] == 'partition2'
        np.testing.assert_array_equal(ctx.count_finish(), oracle.count_flat(host[:40 << 20], k, threads=8))
    finally:
        ctx.free(d)
