"""FASTQ ingest where the short random reads of tests/test_gpu_fastq.py do not reach: events placed on the block, slice and wave
edges of the tokeniser (fastq_kernels.hpp: 4 KiB workgroup blocks of 16-byte thread slices), lines of one block up to a
megabase, malformed long records, byte ranges of a file fed one after another, FASTQ feeds mixed with the other feeds of one
count, mask options that change between feeds, and kpal_count_balance on a text whose last line lacks its '\\n'.  Everything is
compared bit for bit with the restatement of the rules (tests/fastq_cases.py, whose generators tests/test_fastq_host.py proves on
the CPU) and the oracle's counts.  Run on the GPU box: pytest -m gpu."""
import io
import random

import numpy as np
import pytest

import fastq_cases as fc
import oracle
from fastq_cases import Malformed, Ragged, fastq_reads, flat_of, random_fastq

pytestmark = pytest.mark.gpu

MQ = fc.MASK_QUALITY


def fresh_context(monkeypatch, chunk):
    """A context of its own whose staging chunk is `chunk` bytes (None: the default, 64 MiB)."""
    from kpal_amd import _native
    if chunk:
        monkeypatch.setenv('KPAL_FASTA_CHUNK', str(chunk))
    c = _native.Context(_native.default_device())
    monkeypatch.delenv('KPAL_FASTA_CHUNK', raising=False)
    return c


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


@pytest.fixture(scope='module')
def edge_cases():
    """[(label, text, {mq: the stream the restatement gives})]"""
    return [(label, text, {mq: flat_of(fastq_reads(text, mq)) for mq in (None, MQ)}) for label, text in fc.edge_texts()]


@pytest.fixture(scope='module')
def long_cases():
    """[(LongRead, {mq: reads})]"""
    return [(case, {mq: fastq_reads(case.text, mq) for mq in (None, MQ)}) for case in fc.long_read_texts()]


# ---- 1. edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', [None, 4096, 4097, 17])
def test_flatten_with_events_on_block_slice_and_wave_edges(monkeypatch, edge_cases, chunk):
    """kpal_fastq_flatten == the restatement, byte for byte, for every text of fastq_cases.edge_texts() (each '\\n', the '\\r' of
    a '\\r\\n', each first byte, an empty read, the end of the text -- at a block, slice or wave edge -2 .. +2), without the
    mask and with it at 20; the staging chunk at its default (the offsets of the text are the offsets of the kernels), at 4096
    and 4097 (a seam on, and drifting off, every block edge) and at 17 (the record carried through hundreds of chunks)."""
    c = fresh_context(monkeypatch, chunk)
    assert len(edge_cases) == len(fc.EVENTS) * len(fc.EDGES) * len(fc.DELTAS)
    for label, text, want in edge_cases:
        assert len(text) // (chunk or len(text)) + 2 <= fc.MAX_CHUNK_ITERATIONS, label
        for mq in (None, MQ):
            got = c.fastq_flatten(text, min_quality=mq)
            assert got == want[mq], (label, chunk, mq)
    c.close()


# ---- 2. long reads -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', [None, 65536, 4096])
def test_flatten_long_reads(monkeypatch, long_cases, chunk):
    """The same comparison for fastq_cases.long_read_texts(): sequence lines of 4095 .. 1 000 003 bytes (whole blocks that keep
    nothing, blocks that keep all 4096 bytes, a quality line many blocks behind its sequence line), a title longer than a
    block, 3000 one-base reads behind a long one, CRLF, no final newline; records larger than the chunk at 65 536 and 4096."""
    c = fresh_context(monkeypatch, chunk)
    ran = 0
    for case, reads in long_cases:
        if chunk and chunk < case.min_chunk:
            continue
        assert len(case.text) // (chunk or len(case.text)) + 2 <= fc.MAX_CHUNK_ITERATIONS, case.label
        for mq in (None, MQ):
            got = c.fastq_flatten(case.text, min_quality=mq)
            assert got == flat_of(reads[mq]), (case.label, chunk, mq)
        ran += 1
    assert ran >= len(long_cases) - 1
    c.close()


class CountedReads(object):
    """A handle that counts the read() calls that returned data (one FASTQ feed each)."""

    def __init__(self, inner):
        self.inner, self.feeds = inner, 0

    def read(self, n=-1):
        piece = self.inner.read(n)
        self.feeds += 1 if piece else 0
        return piece


@pytest.mark.parametrize('k', [8, 12, 13])
def test_counts_of_long_reads(tmp_path, long_cases, k):
    """Profile.from_fastq == oracle.from_sequences(reads) on every bin for the long-read texts at k = 8, 12 and 13, with the
    mask at 20 and (k = 8, 12) without it: through the file path (the library's own reads), io.BytesIO and -- for the texts that ragged
    pieces of at most 4096 bytes feed in no more than 4096 feeds -- the ragged handle (the long record carried from feed to
    feed)."""
    from kpal_amd import klib
    ragged = 0
    for case, reads in long_cases:
        path = tmp_path / (case.label + '.fq')
        path.write_bytes(case.text)
        for mq in ((None, MQ) if k < 13 else (MQ,)):                   # (k = 13: 512 MiB per table -- the masked text only)
            want = oracle.from_sequences(reads[mq], k)
            with open(str(path), 'rb') as fh:
                got = klib.Profile.from_fastq(fh, k, min_quality=mq).counts
            np.testing.assert_array_equal(got, want, err_msg='file %s k=%d mq=%s' % (case.label, k, mq))
            got = klib.Profile.from_fastq(io.BytesIO(case.text), k, min_quality=mq).counts
            np.testing.assert_array_equal(got, want, err_msg='BytesIO %s k=%d mq=%s' % (case.label, k, mq))
            if len(case.text) <= 140000 and (mq == MQ or k == 8):
                handle = CountedReads(Ragged(case.text, k))
                got = klib.Profile.from_fastq(handle, k, min_quality=mq).counts
                assert handle.feeds <= fc.MAX_CHUNK_ITERATIONS, case.label
                np.testing.assert_array_equal(got, want, err_msg='ragged %s k=%d mq=%s' % (case.label, k, mq))
                ragged += 1
            del want, got
    assert ragged >= 10


# ---- 3. malformed long records -------------------------------------------------------------------------------------------
def bad_long_texts():
    """{what: (text, min_quality)}: long records the rules refuse."""
    rnd = random.Random(77)
    short = b'@s\nACGTTGCAAC\n+\nIIII#IIIII\n'
    seq, qual = fc.long_sequence(rnd, 20000)
    bad_q = qual[:20000 - 5] + b' ' + qual[20000 - 4:]              # a byte below '!' in the last block of the quality line
    return {
        'quality one byte short': (short + b'@long\n' + seq + b'\n+\n' + qual[:-1] + b'\n' + short, None),
        'bad quality byte in the last block': (short + b'@long\n' + seq + b'\n+\n' + bad_q + b'\n' + short, MQ),
        'cut off after the sequence line': (short + short + b'@long\n' + seq + b'\n', None),
        'cut off inside the quality line': (short + b'@long\n' + seq + b'\n+\n' + qual[:12345], None),
        'separator without + four chunks behind the title': (short + b'@long\n' + seq + b'\n-\n' + qual + b'\n' + short, None),
        'next title without @ behind a long read': (short + b'@long\n' + seq + b'\n+\n' + qual + b'\nlong2\nAC\n+\nII\n', None),
    }


def test_malformed_long_records(tmp_path, monkeypatch, ctx):
    """Long records the rules refuse -- a quality line one byte short, a quality byte outside the offset's range in the last
    block of a 20 000-byte quality line (malformed under the mask only), a long read cut off at the end of the text, an error
    that only shows chunks after the one that holds the title -- raise ValueError with the record number the restatement gives:
    from_fastq on the file, the buffer and ragged pieces, and the flattening with a 4096-byte chunk."""
    from kpal_amd import klib
    c = fresh_context(monkeypatch, 4096)
    for what, (text, mq) in bad_long_texts().items():
        with pytest.raises(Malformed) as info:
            fastq_reads(text, mq)
        record = info.value.record
        assert record >= 2, what
        if mq is not None:
            fastq_reads(text, None)                                   # (legal without the mask: the bytes are not looked at)
            assert c.fastq_flatten(text) == flat_of(fastq_reads(text, None)), what
        path = tmp_path / 'bad.fq'
        path.write_bytes(text)
        for label, make in (('buffer', lambda: io.BytesIO(text)), ('ragged', lambda: Ragged(text, 5)), ('file', lambda: open(str(path), 'rb'))):
            handle = make()
            with pytest.raises(ValueError) as err:
                klib.Profile.from_fastq(handle, 8, min_quality=mq)
            assert 'record %d:' % record in str(err.value), (what, label, str(err.value))
        with pytest.raises(ValueError, match='record %d:' % record):
            c.fastq_flatten(text, min_quality=mq)
        with pytest.raises(ValueError, match='record %d:' % record):   # the C-ABI with the small chunk: feed, then the end of the text
            c.count_begin(8)
            c.count_feed_fastq(text, min_quality=mq)
            c.count_finish()
    good = b'@r1\nACGTACGTAC\n+\nIIIIIIIIII\n'
    c.count_begin(4)
    c.count_feed_fastq(good)
    np.testing.assert_array_equal(c.count_finish(), oracle.from_sequences(fastq_reads(good), 4))
    c.close()


# ---- 4. byte ranges of a file --------------------------------------------------------------------------------------------
def range_texts():
    rnd = random.Random(31)
    base = random_fastq(rnd, 90, noise=False)
    return {
        'final newline': base,
        'no final newline': base + b'@last\nACGTNACGTTGACCA\n+\nIIII#IIIII5IIII',
        'crlf': random_fastq(rnd, 60, crlf=True, noise=False),
        'noise': random_fastq(rnd, 90),
        'long read': [c for c in fc.long_read_texts() if c.label == 'seq_8192'][0].text,
    }


def feed_ranges(c, path, cuts, mq):
    fed = 0
    for begin, end in fc.ranges_of(cuts):
        if end == 0:
            continue                                                  # (end = 0 means "to the end of the file", not an empty range)
        c.count_feed_fastq_file(path, begin, end, min_quality=mq)
        fed += 1
    return fed


@pytest.mark.parametrize('k', [8, 13])
def test_file_ranges_continue_the_text(tmp_path, ctx, k):
    """kpal_count_feed_fastq_file with begin != 0: one feed per range of fastq_cases.range_cuts (cuts inside every line role
    and between '\\r' and '\\n', one-byte and empty ranges), then kpal_count_finish == the oracle over the reads of the whole
    text -- with and without a final newline, CRLF, a read longer than a block; masked and unmasked, which differ."""
    for t, (what, text) in enumerate(sorted(range_texts().items())):
        path = str(tmp_path / ('r%d.fq' % t))
        with open(path, 'wb') as fh:
            fh.write(text)
        wants = {mq: oracle.from_sequences(fastq_reads(text, mq), k) for mq in (None, MQ)}
        assert not np.array_equal(wants[None], wants[MQ]), what
        for cuts in fc.range_cuts(text, 100 + t)[:3 if k == 8 else 1]:
            for mq in (None, MQ):
                ctx.count_begin(k)
                assert feed_ranges(ctx, path, cuts, mq) >= 10
                np.testing.assert_array_equal(ctx.count_finish(), wants[mq], err_msg='%s k=%d mq=%s cuts=%r' % (what, k, mq, cuts))


def test_file_range_edge_cases(tmp_path, ctx):
    """An empty range (at the end, in the middle, of an otherwise unfed count) is a no-op; a path that does not exist raises
    OSError and the context counts correctly afterwards; a malformed record in the third range is reported with its number
    over the whole text."""
    text = random_fastq(random.Random(5), 50, noise=False)
    n = len(text)
    path = str(tmp_path / 'e.fq')
    with open(path, 'wb') as fh:
        fh.write(text)
    want = oracle.from_sequences(fastq_reads(text), 8)
    ctx.count_begin(8)
    ctx.count_feed_fastq_file(path, n, n)
    ctx.count_feed_fastq_file(path, 7, 7)
    assert not ctx.count_finish().any()
    ctx.count_begin(8)
    ctx.count_feed_fastq_file(path, 0, n // 2)
    ctx.count_feed_fastq_file(path, n // 2, n // 2)
    ctx.count_feed_fastq_file(path, n // 2, n)
    ctx.count_feed_fastq_file(path, n, n)
    np.testing.assert_array_equal(ctx.count_finish(), want)
    # no such file
    ctx.count_begin(8)
    ctx.count_feed_fastq_file(path, 0, n // 3)
    with pytest.raises(OSError):
        ctx.count_feed_fastq_file(str(tmp_path / 'missing.fq'), 0, 10)
    ctx.count_begin(8)
    ctx.count_feed_fastq_file(path, 0, n // 3)
    ctx.count_feed_fastq_file(path, n // 3, 0)
    np.testing.assert_array_equal(ctx.count_finish(), want)
    # a record without its '+' that begins in range 2 and ends in range 3
    spans = fc.line_spans(text)
    bad_line = 4 * 30 + 2
    s, e = spans[bad_line]
    bad = text[:s] + b'-' + text[s + 1:]
    with pytest.raises(Malformed) as info:
        fastq_reads(bad)
    assert info.value.record == 31
    with open(path, 'wb') as fh:
        fh.write(bad)
    cuts = [0, spans[4 * 11 + 1][0] + 1, spans[4 * 30 + 1][0] + 1, spans[4 * 33][1], n]
    ctx.count_begin(8)
    ctx.count_feed_fastq_file(path, cuts[0], cuts[1])
    ctx.count_feed_fastq_file(path, cuts[1], cuts[2])
    with pytest.raises(ValueError, match='record 31:'):
        ctx.count_feed_fastq_file(path, cuts[2], cuts[3])
    with pytest.raises(RuntimeError):                                  # the count is abandoned
        ctx.count_feed_fastq_file(path, cuts[3], cuts[4])
    ctx.count_begin(8)
    ctx.count_feed_fastq(text)
    np.testing.assert_array_equal(ctx.count_finish(), want)


# ---- 5. FASTQ feeds among the other feeds of one count --------------------------------------------------------------------
@pytest.mark.parametrize('k', [8, 13])
def test_fastq_feeds_mixed_with_other_feeds(ctx, k):
    """One count fed FASTQ text cut in the middle of a record, then flat reads (kpal_count_feed), then FASTA text
    (kpal_count_feed_fasta), then the rest of the FASTQ text: the carried record survives the feeds in between, and the counts
    are the sum of the three oracles."""
    rnd = random.Random(50 + k)
    text = random_fastq(rnd, 80, noise=False) + b'@last\nACGTTGACCAGTAGGCAT\n+\nIIIIIIII#IIIIIIIII'
    spans = fc.line_spans(text)
    carried = [r for r in range(40, 70) if spans[4 * r + 1][1] - spans[4 * r + 1][0] >= 2 * k][0]
    s, e = spans[4 * carried + 1]
    cut = (s + e) // 2                                                 # inside the sequence line of that record
    flat_reads = [bytes(rnd.choice(b'ACGT') for _ in range(rnd.randint(1, 200))) for _ in range(50)]
    fasta_seqs = [bytes(rnd.choice(b'ACGTacgtN') for _ in range(rnd.randint(1, 400))) for _ in range(20)]
    fasta = b''.join(b'>s%d\n' % i + b'\n'.join(q[j:j + 60] for j in range(0, len(q), 60)) + b'\n' for i, q in enumerate(fasta_seqs))
    want = oracle.from_sequences(fastq_reads(text), k) + oracle.from_sequences(flat_reads, k) + oracle.from_sequences(fasta_seqs, k)
    assert oracle.from_sequences([fastq_reads(text)[carried]], k).any()   # the record that is carried has k-mers
    ctx.count_begin(k)
    ctx.count_feed_fastq(text[:cut])
    ctx.count_feed(b'\n'.join(flat_reads))
    ctx.count_feed_fasta(fasta)
    ctx.count_feed_fastq(text[cut:])
    np.testing.assert_array_equal(ctx.count_finish(), want)


# ---- 6. mask options that change between feeds ----------------------------------------------------------------------------
def test_mask_options_across_feeds(ctx):
    """The record carried from one FASTQ feed into the next takes the options of the LATER feed (kpal_hip.h): records finished
    in the first feed keep its options."""
    text = random_fastq(random.Random(61), 60, noise=False)
    spans = fc.line_spans(text)
    plain, masked = fastq_reads(text), fastq_reads(text, MQ)
    carried = [r for r in range(20, 40) if plain[r] != masked[r] and len(plain[r]) >= 40][0]
    s, e = spans[4 * carried + 1]
    cut = (s + e) // 2
    done = text[:cut].count(b'\n') // 4                                # records whose four lines end inside the first feed
    assert done == carried
    for first, second in ((None, MQ), (MQ, None)):
        reads = (plain if first is None else masked)[:done] + (plain if second is None else masked)[done:]
        want = oracle.from_sequences(reads, 8)
        for other in (plain, masked, (plain if first is None else masked)[:done + 1] + (plain if second is None else masked)[done + 1:]):
            assert not np.array_equal(oracle.from_sequences(other, 8), want)   # the carried record's options are visible
        ctx.count_begin(8)
        ctx.count_feed_fastq(text[:cut], min_quality=first)
        ctx.count_feed_fastq(text[cut:], min_quality=second)
        np.testing.assert_array_equal(ctx.count_finish(), want, err_msg='%r then %r' % (first, second))


# ---- 7. balance ends the text ---------------------------------------------------------------------------------------------
OPEN_TEXT_TAIL = b'@last\nACGTTGACCAGTAGGCATCAAGTCAG\n+\nIIIIIIII#IIIIIIIIIIIIIIIII'     # no '\n' behind the quality line


@pytest.mark.parametrize('k,strategy', [(3, 'auto'), (8, 'auto'), (12, 'auto'), (13, 'auto'), (13, 'partition2_quads')])
def test_count_balance_ends_the_fastq_text(k, strategy):
    """kpal_count_balance after a FASTQ feed whose last line lacks its '\\n' (the last record is still carried), then
    kpal_count_finish: oracle.balance(oracle.from_sequences(reads)) on every bin -- the carried record is counted BEFORE the
    balance.  At k = 13 also with the two-level quad strategy forced, where the balance is fused into the pending finalisation.
    (Without the end of the text in kpal_count_balance the last read is counted but not balanced.)"""
    from kpal_amd import _native
    c = _native.Context(_native.default_device())
    text = random_fastq(random.Random(70 + k), 300, noise=False) + OPEN_TEXT_TAIL
    reads = fastq_reads(text)
    assert reads[-1] == OPEN_TEXT_TAIL.split(b'\n')[1]
    want = oracle.balance(oracle.from_sequences(reads, k), k)
    late = oracle.balance(oracle.from_sequences(reads[:-1], k), k) + oracle.from_sequences(reads[-1:], k)
    assert not np.array_equal(late, want)                              # balancing too early is visible in these counts
    del late
    try:
        for pieces in ((text,), (text[:len(text) // 2], text[len(text) // 2:])):
            c.count_begin(k, strategy)
            for piece in pieces:
                c.count_feed_fastq(piece)
            if strategy != 'auto':
                assert c.count_last_plan()[0] == strategy
            c.count_balance()
            np.testing.assert_array_equal(c.count_finish(), want, err_msg='k=%d %s' % (k, strategy))
        # a FASTQ feed after the balance begins a new text: record numbers start again
        c.count_begin(k, strategy)
        c.count_feed_fastq(text)
        c.count_balance()
        with pytest.raises(ValueError, match='record 2:'):
            c.count_feed_fastq(b'@a\nAC\n+\nII\n@b\nACG\n+\nII\n')
    finally:
        c.close()


def test_count_balance_refuses_a_cut_off_record(ctx):
    """The same text ending in a cut-off record: kpal_count_balance raises ValueError naming the record, as kpal_count_finish
    would, and abandons the count; kpal_count_begin then works again."""
    text = random_fastq(random.Random(9), 40, noise=False) + b'@cut\nACGTACGT\n+'
    with pytest.raises(Malformed) as info:
        fastq_reads(text)
    assert info.value.record == 41
    ctx.count_begin(8)
    ctx.count_feed_fastq(text)
    with pytest.raises(ValueError, match='record 41:'):
        ctx.count_balance()
    with pytest.raises(RuntimeError):
        ctx.count_finish()                                             # abandoned: nothing to finish
    good = text[:text.rindex(b'@cut')]
    ctx.count_begin(8)
    ctx.count_feed_fastq(good)
    ctx.count_balance()
    np.testing.assert_array_equal(ctx.count_finish(), oracle.balance(oracle.from_sequences(fastq_reads(good), 8), 8))
