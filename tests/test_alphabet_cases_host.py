"""The byte-alphabet cases (tests/alphabet_cases.py) without a GPU: the reference counter against the oracle, the preconditions
of every text (asserted, not assumed: an edit of the generator cannot move a case off its place without a test failing), the
host tokeniser and the host encoders on all 256 byte values, and the gatherer's stream."""
import io

import numpy as np
import pytest

import alphabet_cases as ac
import oracle
from fastq_cases import Malformed, fastq_reads, flat_of


@pytest.fixture(scope='module')
def built():
    import __graft_entry__
    __graft_entry__.build()
    from kpal_amd import _native
    return _native


@pytest.mark.parametrize('k', range(1, 14))
def test_reference_counter_is_the_oracle(built, k):
    """The plain restatement of kpal/klib.py:152-168 and the oracle's switch-based counter, two independent readings of the
    reference, agree on all three texts -- as one flat stream and as one sequence."""
    for name in ac.FLAT_TEXTS:
        text = ac.flat_text(name)
        bins, counts = ac.reference_sparse([text], k)
        assert bins.size > 0
        for got in (oracle.count_flat(text, k), oracle.from_sequences([text], k)):
            assert got.shape == (4 ** k,) and got.dtype == np.int64
            found = np.flatnonzero(got)                               # (the whole table: its non-zero bins and their values)
            np.testing.assert_array_equal(found, bins, err_msg='%s k=%d' % (name, k))
            np.testing.assert_array_equal(got[found], counts, err_msg='%s k=%d' % (name, k))
        if k <= 8:
            np.testing.assert_array_equal(ac.flat_reference(name, k), oracle.count_flat(text, k))


def test_reference_counter_on_hand_cases():
    assert ac.reference_kmers(b'ACGT', 4) == [int('0123', 4)]
    assert ac.reference_kmers(b'acgtn', 2) == [1, 6, 11]
    assert ac.reference_kmers(b'AC\x00GT', 2) == [1, 11]
    assert ac.reference_kmers(b'AC\xc1GT\x41', 1) == [0, 1, 2, 3, 0]
    assert ac.reference_kmers(b'ACG', 4) == []
    assert ac.reference_count([b'AAAA', b'AA'], 2).tolist() == [4] + [0] * 15


def test_every_value_meets_every_chunk_offset():
    text = ac.flat_text('every_byte_every_slot')
    assert len(text) == 256 * 16 * 37 == 151552 == 148 * ac.WAVE_STEP
    a = np.frombuffer(text, dtype=np.uint8)
    marks = np.arange(ac.SLOT_FILL, len(text), ac.SLOT_FILL + 1)
    assert marks.size == 256 * 16
    pairs = set(zip(a[marks].tolist(), (marks % ac.CHUNK).tolist()))
    assert pairs == set((v, o) for v in range(256) for o in range(16))
    # everything between the marks is a letter
    rest = np.ones(len(text), dtype=bool)
    rest[marks] = False
    assert np.isin(a[rest], np.frombuffer(ac.LETTERS, dtype=np.uint8)).all()
    # interior wave-steps and both edges: marks lie in the first and in the last step, and in every step between
    assert set((marks // ac.WAVE_STEP).tolist()) == set(range(148))


def test_seam_walk_holds_every_distance():
    text = ac.flat_text('seam_walk')
    a = np.frombuffer(text, dtype=np.uint8)
    bad = np.flatnonzero(~np.isin(a, np.frombuffer(ac.LETTERS, dtype=np.uint8)))
    assert bad.size == 70
    seams = (bad + 512) // ac.WAVE_STEP
    assert seams.tolist() == list(range(1, 71))                       # one bad byte per seam, seam after seam
    found = set(zip((bad - seams * ac.WAVE_STEP).tolist(), a[bad].tolist()))
    assert found == set((d, b) for d in range(-17, 18) for b in (ord('N'), 0))
    assert len(text) % ac.WAVE_STEP == 40 and len(text) // ac.WAVE_STEP == 71


def test_long_seam_walk_holds_every_distance_inside_a_run():
    """Whatever number of steps (2 .. 16) a wave walks, every (distance, bad byte) pair stands at a seam inside some run."""
    text = ac.flat_text('seam_walk_long')
    assert len(text) == ac.WAVE_STEP * ac.LONG_STEPS + 40
    every = set((d, b) for d in range(-17, 18) for b in (ord('N'), 0))
    assert ac.interior_seam_pairs(text, 10 ** 9) == every
    for steps_per_wave in range(2, 17):
        assert ac.interior_seam_pairs(text, steps_per_wave) == every, steps_per_wave


@pytest.mark.parametrize('k', (1, 2, 5, 7, 11))
def test_numpy_reference_is_the_rolling_reference(built, k):
    for name in ac.FLAT_TEXTS:
        np.testing.assert_array_equal(ac.reference_count_numpy(ac.flat_text(name), k), ac.flat_reference(name, k), err_msg=name)
    for seq in (b'', b'ACG', b'ACGT', b'NACGTN', b'\x00' * 20, b'acgtACGT' * 3):
        np.testing.assert_array_equal(ac.reference_count_numpy(seq, k), ac.reference_count([seq], k))
    if k in (2, 7, 11):                     # the k the GPU test counts the long text at
        text = ac.flat_text('seam_walk_long')
        np.testing.assert_array_equal(ac.reference_count_numpy(text, k), oracle.count_flat(text, k, threads=4))


def test_near_misses_hold_every_neighbour():
    text = ac.flat_text('near_misses')
    assert len(text) == 64 << 10
    assert len(ac.NEAR_MISS_FLIPS) == 56 and set(ac.NEAR_MISS_VALUES) == set(c ^ (1 << b) for c, b in ac.NEAR_MISS_FLIPS)
    counts = np.bincount(np.frombuffer(text, dtype=np.uint8), minlength=256)
    for c, b in ac.NEAR_MISS_FLIPS:
        assert counts[c ^ (1 << b)] >= 16, (chr(c), b)
    assert set(np.flatnonzero(counts).tolist()) == set(ac.NEAR_MISS_VALUES) | set(ac.LETTERS)
    letters = sum(int(counts[c]) for c in ac.LETTERS)
    assert 0.45 < letters / len(text) < 0.62                          # half, plus the neighbours that are letters themselves
    # short dense runs: k-mers exist at small and medium k, and runs end everywhere
    assert len(ac.reference_kmers(text, 4)) > 1000 and len(ac.reference_kmers(text, 8)) > 10


@pytest.mark.parametrize('k,window,step', ac.WINDOW_TRIPLES)
def test_every_value_meets_every_straddle_offset(k, window, step):
    """Behind the end of the trimmed windows every offset 0 .. k - 2 sees every byte value the format can deliver: all but the
    line ends and the space in a FASTA record (the tokeniser drops them), all but '\\n' in a FASTQ read."""
    _, seq = ac.window_fasta(step)
    assert set(seq) == set(range(256)) - {10, 13, 32}
    assert ac.straddle_pairs(seq, k, window, step) == set((o, v) for o in range(k - 1) for v in set(seq))
    text, read = ac.window_fastq(step)
    assert set(read) == set(range(256)) - {10}
    assert ac.straddle_pairs(read, k, window, step) == set((o, v) for o in range(k - 1) for v in set(read))
    assert fastq_reads(text) == [read]
    spans = ac.window_spans(len(read), window, step)
    assert spans[0] == (0, window) and spans[-1][1] == len(read) and spans[-2][1] < len(read)
    assert all(e - s == window for s, e in spans[:-1]) and 0 < spans[-1][1] - spans[-1][0] <= window


def test_space_rule_is_str_isspace():
    assert sorted(ac.LATIN1_SPACE) == [9, 10, 11, 12, 13, 0x1c, 0x1d, 0x1e, 0x1f, 0x20, 0x85, 0xa0]
    assert sorted(ac.SOFT_BLANKS) == [9, 11, 12, 0x1c, 0x1d, 0x1e, 0x1f, 0x85, 0xa0]


def test_fasta_cases_hold_every_value_at_every_place():
    text = ac.fasta_case_text()
    assert text.encode('latin-1').decode('latin-1') == text
    records = dict((name, seq) for name, seq in ac.seqio_records(text))
    for b in range(256):
        if b in (10, 13):
            continue
        c = chr(b)
        soft, space = b in ac.SOFT_BLANKS, b == 32
        tag = 'v%02x_' % b
        assert records[tag + 'interior'] == ('ACGT' if space else 'AC' + c + 'GT')
        if c == '>':
            assert records[tag + 'leading'] == '' and records['ACGT'] == ''      # the line is a header
        else:
            assert records[tag + 'leading'] == ('ACGT' if space else c + 'ACGT')  # (lstrip is not in the rule: a leading tab stays)
        assert records[tag + 'trailing'] == ('ACGT' if soft or space else 'ACGT' + c)
        assert records[tag + 'trailing_blanks'] == ('ACGT' if soft or space else 'ACGT' + c)
        assert records[tag + 'blank_run'] == 'AC' + ('' if space else c) + '\t\x0cgt'
        assert records[tag + 'wrapped'] == ('aCGt' if soft or space else 'aC' + c + 'Gt')
        assert records[tag + 'header'] == 'ACGT'
    for tag in ('lf', 'cr', 'crlf'):
        for place in ('interior', 'leading', 'trailing', 'wrapped'):
            assert records['%s_%s' % (tag, place)] == ('aCGt' if place == 'wrapped' else 'ACGT')
        assert records[tag + '_before_blanks'] == 'ACGTAC'
    assert records['last'] == 'ACGTacgt' and not text.endswith('\n')
    flat = ac.expected_flat(text)
    assert flat.count(b'\n') == len(ac.seqio_records(text)) and b'\r' not in flat and b' ' not in flat


def test_chunk_sizes_cut_inside_both_kinds_of_blank_runs():
    """The chunk sizes the GPU test forces put a cut inside a run of soft blanks that trails its line and inside one that a
    base follows (the GPU test asserts it again for the sizes it takes)."""
    text = ac.fasta_case_text()
    found = [ac.blank_run_cuts(text, chunk) for chunk in ac.FASTA_CHUNKS]
    assert any(trailing for trailing, _ in found) and any(followed for _, followed in found)
    for chunk in (17, 64):
        trailing, followed = ac.blank_run_cuts(text, chunk)
        assert trailing and followed, chunk


def test_host_tokeniser_on_the_fasta_cases(built):
    """klib._fasta_records, the tokeniser of the paths that count record by record on the host, on a text handle and on a
    binary one: the names and sequences of the Biopython-rule tokeniser."""
    from kpal_amd import klib
    text = ac.fasta_case_text()
    want = ac.seqio_records(text)
    assert list(klib._fasta_records(io.StringIO(text))) == want
    assert list(klib._fasta_records(io.BytesIO(text.encode('latin-1')))) == want


def test_host_encoders_accept_exactly_the_alphabet(built):
    """klib._encode maps every one-byte character to its own byte and everything beyond latin-1 to a separator, so exactly
    ``ACGTacgt`` reach the kernels as bases; Profile.dna_to_binary takes exactly those eight, with the codes of
    kpal/klib.py:43-48."""
    from kpal_amd import klib
    codes = {'A': 0, 'a': 0, 'C': 1, 'c': 1, 'G': 2, 'g': 2, 'T': 3, 't': 3}
    p = klib.Profile(np.zeros(4, dtype=np.int64))
    for cp in list(range(0x300)) + [0xFF21, 0xFF23, 0xFF27, 0xFF34, 0x0391, 0x0410, 0x1D400, 0xFFFD]:
        ch = chr(cp)
        enc = klib._encode(ch)
        assert len(enc) == 1
        assert enc == (bytes(bytearray([cp])) if cp < 256 else b'?')
        assert (enc in [b'A', b'C', b'G', b'T', b'a', b'c', b'g', b't']) == (ch in codes)
        for raw in (bytes(bytearray([cp & 0xFF])), bytearray([cp & 0xFF]), memoryview(bytes(bytearray([cp & 0xFF])))):
            assert klib._encode(raw) == bytes(bytearray([cp & 0xFF]))
        if ch in codes:
            assert p.dna_to_binary(ch) == codes[ch]
            assert ac.reference_kmers(enc, 1) == [codes[ch]]
        else:
            with pytest.raises(KeyError):
                p.dna_to_binary(ch)
            with pytest.raises(KeyError):
                p.dna_to_binary('A' + ch)
            assert ac.reference_kmers(enc, 1) == []
    assert p.dna_to_binary('ACGTacgt') == int('01230123', 4)


def test_gatherer_stream_counts_to_the_reference(built):
    """every_byte_every_slot cut into items of odd lengths, as bytes, bytearray and latin-1 str in turn: the stream the C
    gatherer joins (every item followed by '\\n') and the interpreter's join count to the reference on the items."""
    from kpal_amd import klib
    assert klib._kpal_gather is not None, 'the gatherer extension was not built'
    text = ac.flat_text('every_byte_every_slot')
    rs = np.random.RandomState(7)
    items, raw, at = [], [], 0
    while at < len(text):
        n = int(rs.choice([1, 2, 15, 16, 17, 37, 150, 1000]))
        piece = text[at:at + n]
        raw.append(piece)
        items.append((piece, bytearray(piece), piece.decode('latin-1'))[len(items) % 3])
        at += n
    cap = len(text) + len(items) + 64
    for threads in (1, 5):
        out = np.full(cap, 7, dtype=np.uint8)
        nxt, nbytes, status = klib._kpal_gather.gather(items, 0, out.ctypes.data, cap, threads)
        assert (nxt, status) == (len(items), 0) and nbytes == len(text) + len(items)
        stream = out[:nbytes].tobytes()
        assert stream == b''.join(p + b'\n' for p in raw)
        for k in (1, 3, 8):
            np.testing.assert_array_equal(oracle.count_flat(stream, k), ac.reference_count(raw, k))
    assert klib._join_block(items[0::3]) == b'\n'.join(raw[0::3]) and klib._join_block(items[2::3]) == b'\n'.join(raw[2::3])
    assert klib._join_block(items) == b'\n'.join(raw)


@pytest.mark.parametrize('offset', ac.QUALITY_OFFSETS)
def test_quality_cases_and_their_boundaries(offset):
    for mq in ac.min_qualities(offset):
        assert 0 <= mq <= 93
        cases = ac.quality_cases(offset, mq)
        assert [c.q for c in cases] == [q for q in range(256) if q != 10]
        by_q = dict((c.q, c) for c in cases)
        for c in cases:
            unmasked = fastq_reads(c.text)                            # well formed but for the quality byte
            assert (c.reads is None) != (c.malformed is None)
            if c.malformed is not None:
                assert c.q < offset or c.q > 126
                assert c.malformed == c.q % 3 + 2 and len(unmasked) == c.malformed + 2
            else:
                assert offset <= c.q <= 126 and len(c.reads) == c.q % 3 + 2
                masked = c.q - offset < mq
                assert c.reads[-1] == (unmasked[-1][:1] + b'N' + unmasked[-1][2:] if masked else unmasked[-1])
                assert c.reads[:-1] == unmasked[:-1] or mq == 126 - offset      # (the records before it: '~' and '}')
        b = ac.quality_boundaries(offset, mq)
        assert list(b) == ['offset-1', 'offset', 'offset+min_quality-1', 'offset+min_quality', '~', '~+1', '0x80', '0xFF']

        def outcome(name):
            c = by_q[b[name]]
            return 'malformed' if c.malformed is not None else 'masked' if c.reads[-1][1:2] == b'N' else 'kept'

        assert outcome('offset-1') == 'malformed'
        assert outcome('offset') == ('masked' if mq > 0 else 'kept')
        assert outcome('offset+min_quality-1') == ('masked' if mq > 0 else 'malformed')
        assert outcome('offset+min_quality') == 'kept'
        assert outcome('~') == 'kept'
        assert outcome('~+1') == outcome('0x80') == outcome('0xFF') == 'malformed'


def test_all_bytes_fastq_line():
    text, line = ac.all_bytes_fastq()
    assert set(line) == set(range(256)) - {10} and not line.endswith(b'\r')
    assert fastq_reads(text) == [line] and flat_of([line]) == b'\n' + line
    with pytest.raises(Malformed):
        fastq_reads(text[:-2] + b'\n')
