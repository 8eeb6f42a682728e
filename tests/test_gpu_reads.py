"""One profile per FASTQ read, or per sliding window of a read (Profile.from_fastq_by_record / from_fastq_by_window,
kpal_fastq_records_begin / _file_open, ``kpal count --by-read``; beyond the reference, which reads FASTA only).  The reads are
those of the independent restatement of the format rules (tests/fastq_cases.py: ``fastq_reads``), every expected table is
``oracle.from_sequences([read], k)`` -- ``[read[a:b]]`` for a window -- and every comparison of counts is exact.
Run on the GPU box: pytest -m gpu."""
import io
import os
import random

import numpy as np
import pytest

import memh5
import oracle
from fastq_cases import Ragged, fastq_reads, line_spans, long_read_texts, random_fastq, range_cuts

pytestmark = pytest.mark.gpu

FQ_KERNELS = ('fq_newlines', 'fq_line_scan', 'fq_newline_pos', 'fq_records', 'fq_carry', 'fq_count', 'fq_offset', 'fq_scatter')


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


def context_with_chunk(monkeypatch, chunk):
    """A context whose file scans take pieces of `chunk` bytes (None: the default, 64 MiB)."""
    from kpal_amd import _native
    if chunk:
        monkeypatch.setenv('KPAL_FASTA_CHUNK', str(chunk))
    c = _native.Context(_native.default_device())
    monkeypatch.delenv('KPAL_FASTA_CHUNK', raising=False)
    return c


def read_names(text, n, prefix=''):
    """The names of the first n reads of a text: the first word of the title behind '@', else the 1-based number."""
    names = []
    for i, (s, e) in enumerate(line_spans(text)[0::4][:n]):
        words = text[s + 1:e].decode('latin-1').split()
        names.append(prefix + (words[0] if words else str(i + 1)))
    return names


def window_spans(L, W, S):
    out, j = [], 0
    while L > 0:
        out.append((j * S, min(j * S + W, L)))
        if out[-1][1] == L:
            break
        j += 1
    return out


def expected_reads(text, min_quality=None, offset=33, prefix=''):
    """(name, sequence) of every read; its table is oracle.from_sequences([sequence], k)."""
    reads = fastq_reads(text, min_quality, offset)
    return list(zip(read_names(text, len(reads), prefix), reads))


def expected_windows(text, W, S, min_quality=None, offset=33, prefix=''):
    """(name, sequence) of every window of every read, read-major."""
    reads = fastq_reads(text, min_quality, offset)
    out = []
    for name, read in zip(read_names(text, len(reads), prefix), reads):
        for a, b in window_spans(len(read), W, S):
            out.append(('%s:%d-%d' % (name, a + 1, b), read[a:b]))
    return out


def check(profiles, want, k, what):
    """Names and tables, profile by profile against the oracle (the generator is consumed as it goes and the expected tables
    are made one at a time: nothing piles up)."""
    profiles = iter(profiles)
    n = 0
    for (name, seq), p in zip(want, profiles):
        assert p.name == name, (what, n, p.name, name)
        np.testing.assert_array_equal(p.counts, oracle.from_sequences([seq], k), err_msg='%s %s' % (what, name))
        n += 1
    assert n == len(want) and next(profiles, None) is None, (what, n, len(want))


def make_text(rnd, lengths, offset=33, eol=b'\n'):
    """Reads of the given lengths: titles of several words, one title without a word, bases with 'N' and lower case, quality
    bytes over the whole range of the offset (a mask at 20 masks about a fifth of the bases)."""
    out = []
    for i, n in enumerate(lengths):
        title = b'@' if i == 2 else b'@read%d len=%d x' % (i, n)
        seq = bytes(rnd.choice(b'ACGTACGTACGTACGTacgtN') for _ in range(n))
        qual = bytes(rnd.randint(offset, 126) for _ in range(n))
        out.append(title + eol + seq + eol + (b'+' if i % 2 else b'+' + title[1:]) + eol + qual + eol)
    return b''.join(out)


# ---- the index at the C-ABI ----------------------------------------------------------------------------------------------
def index_texts():
    rnd = random.Random(77)
    texts = [('random', random_fastq(rnd, 60, max_len=300)), ('random_crlf', random_fastq(rnd, 60, max_len=300, crlf=True))]
    texts += [(case.label, case.text) for case in long_read_texts() if max(case.long_lines) <= 65537]
    assert len(texts) >= 8
    return texts


def whole_index(ctx, text):
    n, nf, consumed = ctx.fastq_records_begin(text, final=True)
    header_off, flat_start = ctx.fasta_records_index()
    return n, nf, consumed, header_off.tolist(), flat_start.tolist()


@pytest.mark.parametrize('label,text', index_texts(), ids=[label for label, _ in index_texts()])
def test_index_of_a_text_and_of_its_pieces(ctx, label, text):
    """kpal_fastq_records_begin(final) against the text read on the host: title-line offsets, flat starts = the running sum of
    1 + len(read), consumed = everything.  The same text cut at every list of range_cuts, each range behind the carried rest
    and only the last one final: the concatenated index is the one-call index."""
    reads = fastq_reads(text)
    n, nf, consumed, header_off, flat_start = whole_index(ctx, text)
    titles = [s for s, _ in line_spans(text)[0::4]][:len(reads)]
    starts = np.concatenate([[0], np.cumsum([1 + len(r) for r in reads])]).tolist()
    assert n == len(reads) and header_off == titles and flat_start == starts
    assert consumed == len(text) and nf == starts[-1]
    for c, cuts in enumerate(range_cuts(text, 5)):
        carry, at, before = b'', 0, 0
        got_titles, got_lengths = [], []
        for i in range(len(cuts) - 1):
            piece = carry + text[cuts[i]:cuts[i + 1]]
            final = i == len(cuts) - 2
            m, mf, used = ctx.fastq_records_begin(piece, None, 33, final, before)
            assert used <= len(piece) and (not final or used == len(piece))
            if m:
                hdr, st = ctx.fasta_records_index()
                assert st[0] == 0 and st[-1] == mf
                got_titles += (hdr + np.uint64(at)).tolist()
                got_lengths += (np.diff(st) - np.uint64(1)).tolist()
            else:
                assert mf == 0
            before += m
            at += used
            carry = piece[used:]
        assert before == n and got_titles == titles and got_lengths == [len(r) for r in reads], (label, c)


def test_index_numbers_a_malformed_record_over_the_whole_text(ctx):
    """records_before numbers the bad record; after the error the context holds no index, and takes a good text again."""
    rnd = random.Random(3)
    good = random_fastq(rnd, 20, max_len=80, noise=False)
    text = good + b'@bad\nACGT\n+\nIII\n' + good
    cut = len(good) // 2
    n1, _, used = ctx.fastq_records_begin(text[:cut], None, 33, False, 0)
    assert 0 < n1 < 20 and used <= cut
    with pytest.raises(ValueError, match='malformed FASTQ record 21: the quality line'):
        ctx.fastq_records_begin(text[used:], None, 33, True, n1)
    assert ctx.fasta_records_index()[0].size == 0
    ctx._records = 1                                     # (the binding's own count: the library itself has no index to hand out)
    with pytest.raises(RuntimeError):
        ctx.fasta_records_index()
    with pytest.raises(ValueError, match='quality_offset'):
        ctx.fastq_records_begin(good, None, 50, True, 0)
    assert whole_index(ctx, good)[0] == 20


@pytest.mark.parametrize('chunk', [64, 257])
def test_file_pieces_in_a_row(tmp_path, monkeypatch, chunk):
    """kpal_fasta_records_file_next called again and again on ONE open scan of reads (klib opens, takes one piece and closes):
    what the scan carries from piece to piece.  25 reads in about 3 KB, one of 700 bases -- 1400 bytes, gathered in pageable
    memory over many rounds -- and the file ends in a read.  Every piece begins where the piece before said the scan stood;
    title offsets and read lengths are those of the host tokeniser; a call after the end finds no scan open."""
    rnd = random.Random(chunk)
    lengths = [rnd.randint(0, 30) for _ in range(25)]
    lengths[9] = 700
    text = make_text(rnd, lengths)
    assert 2500 < len(text) < 3500
    reads = fastq_reads(text)
    titles = [s for s, _ in line_spans(text)[0::4]]
    assert len(reads) == len(titles) == 25
    path = tmp_path / 'row.fq'
    path.write_bytes(text)
    ctx2 = context_with_chunk(monkeypatch, chunk)
    try:
        ctx2.fastq_records_file_open(str(path))
        tell, pieces, got_titles, got_lengths = 0, 0, [], []
        while True:
            piece = ctx2.fasta_records_file_next()
            if piece is None:
                break
            n, nf, off = piece
            assert off == tell and n > 0, pieces
            hdr, starts = ctx2.fasta_records_index()
            assert hdr.size == n and starts[0] == 0 and starts[-1] == nf
            got_titles += (hdr + np.uint64(off)).tolist()
            got_lengths += (np.diff(starts) - np.uint64(1)).tolist()
            tell = ctx2.fasta_records_file_tell()
            pieces += 1
        assert pieces > 3 and tell == len(text), (pieces, tell)
        assert got_titles == titles
        assert got_lengths == [len(r) for r in reads]
        assert len(got_titles) == 25
        with pytest.raises(RuntimeError, match='without kpal_fasta_records_file_open'):
            ctx2.fasta_records_file_next()
    finally:
        ctx2.close()


# ---- by read -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('chunk', [17, 300, 4096, None])
@pytest.mark.parametrize('k', [1, 4, 8])
def test_by_read_against_the_oracle(tmp_path, monkeypatch, k, chunk):
    """Reads of length 0, 1, k - 1, k, k + 1 among ordinary ones and sequence lines of 4095, 4096 and 4097 bytes; pieces of 17,
    300, 4096 bytes and the default; batches of three tables (a piece spans several batches, a batch ends inside a piece);
    tables left in HBM and downloaded at once; no mask, a mask at 20, and a Phred-64 text masked at 20."""
    from kpal_amd import _native, klib
    rnd = random.Random(100 * k + (chunk or 0))
    lengths = [57, 0, 1, k - 1, k, k + 1, 300, 4095, 33, 4096, 150, 4097, 2, 91]
    t33 = make_text(rnd, lengths, 33, b'\n')
    t64 = make_text(rnd, lengths, 64, b'\r\n')
    monkeypatch.setattr(klib, '_RECORD_BATCH_BYTES', 3 * 8 * 4 ** k)
    ctx2 = context_with_chunk(monkeypatch, chunk)
    monkeypatch.setattr(_native, 'context', lambda: ctx2)
    try:
        for v, (text, mq, offset) in enumerate(((t33, None, 33), (t33, 20, 33), (t64, 20, 64))):
            path = tmp_path / ('reads%d.fq' % v)
            path.write_bytes(text)
            assert mq is None or fastq_reads(text, mq, offset) != fastq_reads(text)
            want = expected_reads(text, mq, offset, prefix='p_' if v else '')
            assert len(want) == len(lengths) and want[2][0] == ('p_3' if v else '3') and want[1][1] == b''
            for budget in (None, 0):
                with monkeypatch.context() as m:
                    if budget is not None:
                        m.setattr(klib, '_DEVICE_PROFILE_BYTES', budget)
                    with open(str(path), 'rb') as fh:
                        profiles = klib.Profile.from_fastq_by_record(fh, k, prefix='p' if v else None, min_quality=mq, quality_offset=offset)
                        first = next(profiles)
                        assert (first._device_counts() is None) == (budget == 0)
                        check([first] + list(profiles), want, k, 'k=%d chunk=%s text %d budget %s' % (k, chunk, v, budget))
                        assert fh.read() == b''
    finally:
        ctx2.close()


# ---- by window -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,W,S', [(4, 12, 4), (4, 16, 16), (8, 16, 2), (8, 8, 8)])
def test_by_window_against_the_oracle(tmp_path, monkeypatch, k, W, S):
    """Reads of length 0, k - 1, W - 1, W, W + 1, W + S and 4097; without the mask from memory, with it from a file in pieces of
    300 bytes; coordinates count masked bases; names <read>:<start + 1>-<end>."""
    from kpal_amd import _native, klib
    rnd = random.Random(1000 * k + 10 * W + S)
    lengths = [W + 1, 0, k - 1, W - 1, W, W + S, 4097, 3 * W + 5]
    text = make_text(rnd, lengths, 33, b'\n')
    monkeypatch.setattr(klib, '_RECORD_BATCH_BYTES', 64 * 8 * 4 ** k)
    want = expected_windows(text, W, S)
    assert want[0][0] == 'read0:1-%d' % W and want[1][0] == 'read0:%d-%d' % (S + 1, W + 1)
    assert [n for n, _ in want if n.startswith('3:')] == ['3:1-%d' % (k - 1)] and not any(n.startswith('read1:') for n, _ in want)
    check(klib.Profile.from_fastq_by_window(io.BytesIO(text), k, W, step=None if W == S else S), want, k, 'memory')
    masked = expected_windows(text, W, S, 20, 33, prefix='q_')
    assert [n for n, _ in masked] == ['q_' + n for n, _ in want]                   # a masked base is still a base
    assert sum(a != b for (_, a), (_, b) in zip(masked, want)) > len(want) // 2
    path = tmp_path / 'w.fq'
    path.write_bytes(text)
    ctx2 = context_with_chunk(monkeypatch, 300)
    monkeypatch.setattr(_native, 'context', lambda: ctx2)
    try:
        with open(str(path), 'rb') as fh:
            check(klib.Profile.from_fastq_by_window(fh, k, W, S, prefix='q', min_quality=20), masked, k, 'masked file')
    finally:
        ctx2.close()


# ---- routes ---------------------------------------------------------------------------------------------------------------
def test_routes_agree(tmp_path, monkeypatch):
    """A file on disk (text and binary mode), io.BytesIO, io.StringIO and ragged reads give identical names and tables, by
    read and by window; the file handle is left at its end."""
    from kpal_amd import klib
    rnd = random.Random(41)
    text = random_fastq(rnd, 60) + random_fastq(rnd, 20, crlf=True)
    k, W, S = 4, 12, 4
    monkeypatch.setattr(klib, '_RECORD_BATCH_BYTES', 7 * 8 * 4 ** k)
    path = tmp_path / 'routes.fq'
    path.write_bytes(text)
    for mq in (None, 20):
        by_read, by_window = expected_reads(text, mq), expected_windows(text, W, S, mq)
        assert len(by_read) == 80 and any(name.isdigit() for name, _ in by_read)
        routes = [('bytes', lambda: io.BytesIO(text)), ('str', lambda: io.StringIO(text.decode('latin-1'), newline='')),
                  ('ragged', lambda: Ragged(text, 7)), ('file rb', lambda: open(str(path), 'rb')),
                  ('file r', lambda: open(str(path), newline=''))]
        for label, make in routes:
            handle = make()
            check(klib.Profile.from_fastq_by_record(handle, k, min_quality=mq), by_read, k, label)
            if label.startswith('file'):
                assert handle.read() in (b'', '')
                handle.close()
            handle = make()
            check(klib.Profile.from_fastq_by_window(handle, k, W, S, min_quality=mq), by_window, k, label + ' windows')
            if label.startswith('file'):
                assert handle.read() in (b'', '')
                handle.close()
    empty = tmp_path / 'empty.fq'
    empty.write_bytes(b'')
    with open(str(empty), 'rb') as fh:
        assert list(klib.Profile.from_fastq_by_record(fh, 4)) == []
    assert list(klib.Profile.from_fastq_by_record(io.BytesIO(b'\n\n\n'), 4)) == []
    assert list(klib.Profile.from_fastq_by_window(io.BytesIO(b''), 4, 8)) == []


def test_one_table_at_a_time(tmp_path, monkeypatch):
    """A batch budget below two tables (what a large k meets): every read, every window through from_sequences, the reads
    taken from the device tokeniser, so the mask still applies and the names are the same."""
    from kpal_amd import klib
    rnd = random.Random(6)
    k = 4
    text = make_text(rnd, [30, 0, 17, 3, 44], 33, b'\r\n')
    monkeypatch.setattr(klib, '_RECORD_BATCH_BYTES', 8 * 4 ** k)
    path = tmp_path / 'one.fq'
    path.write_bytes(text)
    for mq in (None, 20):
        with open(str(path), 'rb') as fh:
            check(klib.Profile.from_fastq_by_record(fh, k, prefix='x', min_quality=mq), expected_reads(text, mq, prefix='x_'), k, 'file')
        check(klib.Profile.from_fastq_by_window(Ragged(text, 2), k, 12, 4, min_quality=mq), expected_windows(text, 12, 4, mq), k, 'ragged')


def test_generators_interleave(tmp_path, monkeypatch):
    """Generators are independent of each other on the process-wide context: two by-read scans of different files advanced by
    zip(), a by-read scan and a FASTA by-record scan advanced in turns, one scan abandoned half-way -- pieces of 300 bytes and
    batches of two tables, so that every scan finds its index overwritten again and again."""
    from kpal_amd import _native, klib
    rnd = random.Random(8)
    k = 4
    texts = [random_fastq(rnd, 30, max_len=120), random_fastq(rnd, 24, max_len=200, crlf=True), random_fastq(rnd, 12, max_len=90)]
    wants = [expected_reads(t) for t in texts]
    paths = []
    for i, t in enumerate(texts):
        paths.append(str(tmp_path / ('g%d.fq' % i)))
        open(paths[-1], 'wb').write(t)
    fasta_records = [('f%d' % i, ''.join(rnd.choice('ACGT') for _ in range(rnd.randint(1, 150)))) for i in range(25)]
    fasta = ''.join('>%s\n%s\n' % r for r in fasta_records)
    fasta_path = str(tmp_path / 'g.fa')
    open(fasta_path, 'w').write(fasta)
    monkeypatch.setattr(klib, '_RECORD_BATCH_BYTES', 2 * 8 * 4 ** k)
    ctx2 = context_with_chunk(monkeypatch, 300)
    monkeypatch.setattr(_native, 'context', lambda: ctx2)

    def same(profile, want):
        assert profile.name == want[0]
        np.testing.assert_array_equal(profile.counts, oracle.from_sequences([want[1]], k), err_msg=want[0])

    try:
        with open(paths[0], 'rb') as h0, open(paths[1], 'rb') as h1:
            pairs = list(zip(klib.Profile.from_fastq_by_record(h0, k), klib.Profile.from_fastq_by_record(h1, k, min_quality=None)))
            assert len(pairs) == 24
            for i, (a, b) in enumerate(pairs):
                same(a, wants[0][i])
                same(b, wants[1][i])
        # a file scan and a scan of text in memory
        with open(paths[2], 'rb') as h2:
            pairs = list(zip(klib.Profile.from_fastq_by_record(h2, k), klib.Profile.from_fastq_by_record(io.BytesIO(texts[0]), k)))
        assert len(pairs) == 12
        for i, (a, b) in enumerate(pairs):
            same(a, wants[2][i])
            same(b, wants[0][i])
        # FASTQ reads and FASTA records in turns; a third scan abandoned half-way
        with open(paths[1], 'rb') as h1, open(fasta_path) as hf, open(paths[2], 'rb') as h2:
            reads = klib.Profile.from_fastq_by_record(h1, k)
            records = klib.Profile.from_fasta_by_record(hf, k)
            abandoned = klib.Profile.from_fastq_by_window(h2, k, 12, 4)
            left = expected_windows(texts[2], 12, 4)
            assert len(left) > 9
            for i in range(24):
                same(next(reads), wants[1][i])
                same(next(records), fasta_records[i])
                if i < 9:
                    same(next(abandoned), left[i])
            assert next(reads, None) is None
            same(next(records), fasta_records[24])
            assert next(records, None) is None
            del abandoned
    finally:
        ctx2.close()


# ---- malformed ------------------------------------------------------------------------------------------------------------
def piece_counts(text, chunk):
    """Records per piece of a file scan whose pieces are `chunk` bytes behind the carried rest: a piece ends behind the last
    record whose four lines end inside it, gathers further when there is none, and the last piece takes what is left."""
    spans = line_spans(text)
    ends = [spans[i + 3][1] + 1 for i in range(0, len(spans) - 3, 4)]
    out, at = [], 0
    while at < len(text):
        limit = at + chunk
        while limit < len(text) and not any(at < e <= limit for e in ends):
            limit += chunk
        if limit >= len(text):
            out.append(None)                            # the last piece
            break
        done = [e for e in ends if at < e <= limit]
        out.append(len(done))
        at = done[-1]
    return out


def test_malformed_reads(tmp_path, monkeypatch):
    """A bad title in record 1, a length mismatch in a record of the second piece, a cut-off last record: ValueError naming the
    1-based record when the generator reaches the piece; the profiles of earlier pieces have been yielded, none of the bad
    piece; the context indexes a good text afterwards."""
    from kpal_amd import _native, klib
    rnd = random.Random(19)
    k = 4
    records = [b'@r%d\n' % i + bytes(rnd.choice(b'ACGT') for _ in range(40)) + b'\n+\n' + b'I' * 40 + b'\n' for i in range(12)]
    good = b''.join(records)
    bad_title = b'r0\nACGT\n+\nIIII\n' + good
    mismatch = b''.join(records[:4]) + b'@r4\nACGTAC\n+\nIIIII\n' + b''.join(records[5:])
    cut_off = good + b'@last\nACGTACGT\n'
    ctx2 = context_with_chunk(monkeypatch, 300)
    monkeypatch.setattr(_native, 'context', lambda: ctx2)
    try:
        for label, text, record, message in (('bad title', bad_title, 1, "does not begin with '@'"), ('length', mismatch, 5, 'not as long as'),
                                             ('cut off', cut_off, 13, 'cut off')):
            pieces = piece_counts(text, 300)
            before = 0                                   # records of the pieces before the bad record's
            for n in pieces:
                if n is None or before + n >= record:
                    break
                before += n
            if label == 'length':
                assert len(pieces) > 2 and before == pieces[0] > 0 and pieces[0] + pieces[1] >= record      # it lies in the second piece
            if label == 'cut off':
                assert before > 0
            path = tmp_path / 'bad.fq'
            path.write_bytes(text)
            names = read_names(text, before)
            for make in (lambda: klib.Profile.from_fastq_by_record(open(str(path), 'rb'), k),
                         lambda: klib.Profile.from_fastq_by_window(open(str(path), 'rb'), k, 12, 4)):
                got = []
                with pytest.raises(ValueError, match='malformed FASTQ record %d: .*%s' % (record, message)):
                    for p in make():
                        got.append(p.name.split(':')[0])
                assert sorted(set(got), key=got.index) == names, (label, got)
            # text in memory comes in one read(): nothing of it is yielded -- but the rest that read() leaves unfinished is
            # a piece of its own, which the end of the handle ends: the cut-off record lies there, behind the whole reads
            got = []
            with pytest.raises(ValueError, match='malformed FASTQ record %d:' % record):
                for p in klib.Profile.from_fastq_by_record(io.BytesIO(text), k):
                    got.append(p.name)
            assert got == (read_names(good, 12) if label == 'cut off' else [])
            check(klib.Profile.from_fastq_by_record(io.BytesIO(good), k), expected_reads(good), k, 'after ' + label)
        path = tmp_path / 'good.fq'
        path.write_bytes(good)
        with open(str(path), 'rb') as fh:
            check(klib.Profile.from_fastq_by_record(fh, k), expected_reads(good), k, 'file after the errors')
    finally:
        ctx2.close()


# ---- residency ------------------------------------------------------------------------------------------------------------
def test_profiles_stay_in_hbm_and_feed_the_rectangle(ctx):
    """The profiles of both generators are device tables until their counts are read; the rectangle reads x two references is
    computed from them where they lie, within the 1e-9 of the project's distances, and downloads no table."""
    from kpal_amd import kdistlib, klib
    rnd = random.Random(15)
    k = 6
    text = make_text(rnd, [rnd.randint(50, 400) for _ in range(40)])
    reads = fastq_reads(text)
    references = [''.join(rnd.choice('ACGT') for _ in range(5000)), ''.join(rnd.choice('AACGT') for _ in range(3000))]
    by_read = list(klib.Profile.from_fastq_by_record(io.BytesIO(text), k))
    by_window = list(klib.Profile.from_fastq_by_window(io.BytesIO(text), k, 100, 50))
    refs = [klib.Profile.from_sequences([r], k, name='ref%d' % i) for i, r in enumerate(references)]
    assert len(by_read) == len(reads) and len(by_window) >= len([r for r in reads if r])
    assert all(p._device_counts() is not None for p in by_read + by_window + refs)
    got = kdistlib.cross_distances(by_read, refs, kdistlib.ProfileDistance())
    assert got.shape == (len(reads), 2)
    assert all(p._device_counts() is not None for p in by_read + refs)                  # no table was downloaded
    tables = [oracle.from_sequences([r], k) for r in references]
    for q, read in enumerate(reads):
        mine = oracle.from_sequences([read], k)
        for r in range(2):
            want = oracle.profile_distance(mine, tables[r], k)
            assert abs(got[q, r] - want) <= 1e-9 * max(1.0, abs(want)), (q, r, got[q, r], want)
    np.testing.assert_array_equal(by_read[3].counts, oracle.from_sequences([reads[3]], k))
    assert by_read[3]._device_counts() is None and by_window[0].counts is not None and by_window[0]._device_counts() is None


# ---- the count path is the count path ------------------------------------------------------------------------------------
def count_launches(ctx, text, k):
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        ctx.count_begin(k)
        ctx.count_feed_fastq(text, 20, 33)
        table = ctx.count_finish(k)
        seen = dict((name, count) for name, (_, count) in ctx.prof_get().items() if count)
    finally:
        ctx.prof_enable(False)
    return seen, table


def test_count_path_launches_are_unchanged_by_an_index_call(ctx):
    """The launches of a FASTQ count of a text -- the tokeniser's eight kernels once per chunk, in front of the counting
    kernels -- are the same before and after the context has indexed reads; the index adds its own to the tokeniser's."""
    rnd = random.Random(2)
    text = random_fastq(rnd, 200, noise=False)
    before, table = count_launches(ctx, text, 8)
    assert dict((name, before.get(name)) for name in FQ_KERNELS) == dict((name, 1) for name in FQ_KERNELS)
    assert 'fq_title_offsets' not in before and 'fa_mark_scatter' not in before
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        n, _, _ = ctx.fastq_records_begin(text, 20, 33, True, 0)
        index = dict((name, count) for name, (_, count) in ctx.prof_get().items() if count)
    finally:
        ctx.prof_enable(False)
    assert n == 200
    want = dict((name, 1) for name in FQ_KERNELS + ('fq_title_offsets', 'fa_mark_count', 'fa_offset', 'fa_mark_scatter'))
    assert index == want
    after, again = count_launches(ctx, text, 8)
    assert after == before
    np.testing.assert_array_equal(table, again)
    np.testing.assert_array_equal(table, oracle.from_sequences(fastq_reads(text, 20), 8))


# ---- command line ---------------------------------------------------------------------------------------------------------
def test_count_by_read_on_the_command_line(tmp_path, monkeypatch):
    """``kpal count --by-read -k 4``; two inputs (names prefixed by the files' names); ``--by-read --by-window 12 --step 4
    --min-quality 20``: the stored datasets equal the oracle's."""
    from kpal_amd import files, kmer
    rnd = random.Random(33)
    text = make_text(rnd, [40, 0, 25, 3, 64, 13], 33, b'\n')
    other = make_text(rnd, [30, 12], 33, b'\r\n')
    (tmp_path / 'a.fq').write_bytes(text)
    (tmp_path / 'b.fq').write_bytes(other)
    store = memh5.Store()
    monkeypatch.setattr(files, 'open_profile_file', store.open)
    monkeypatch.chdir(tmp_path)

    def stored(name, want):
        handle = store.files[os.path.abspath(name)]
        assert sorted(handle['profiles']) == sorted(n for n, _ in want)
        for n, seq in want:
            np.testing.assert_array_equal(handle['profiles/' + n][:], oracle.from_sequences([seq], 4), err_msg=n)

    kmer.main(['count', '--by-read', '-k', '4', 'a.fq', 'one.k4'])
    stored('one.k4', expected_reads(text))
    assert '3' in store.files[os.path.abspath('one.k4')]['profiles']
    kmer.main(['count', '--by-read', '--fastq', '-k', '4', 'a.fq', 'b.fq', 'two.k4'])
    stored('two.k4', expected_reads(text, prefix='a_') + expected_reads(other, prefix='b_'))
    kmer.main(['count', '--by-read', '--by-window', '12', '--step', '4', '--min-quality', '20', '-k', '4', 'a.fq', 'three.k4'])
    stored('three.k4', expected_windows(text, 12, 4, 20))
    assert expected_windows(text, 12, 4, 20)[0][0] == 'read0:1-12'
