"""Every byte value through the base classifiers and the text readers -- the case generator (pure Python / NumPy, no GPU, no
kpal_amd import).  tests/test_alphabet_cases_host.py holds every text against an independent reference and proves its
preconditions on the CPU; tests/test_gpu_byte_alphabet.py feeds the texts to the kernels.

Two decisions are made per input byte, in several independent places of the library: is the byte one of ``ACGTacgt`` (and
which 2-bit code does it get), and -- in the FASTA and FASTQ readers -- is it dropped, kept, masked or a line end.  The texts
here show all 256 byte values to each of those places, at every position of the structures the kernels work in:

  ``reference_count``        the reference's rule (kpal/klib.py:152-168): split at ``[^ACGTacgt]``, roll a 2-bit window.
  ``every_byte_every_slot``  each value at each of the 16 offsets of a 16-byte chunk (so: every byte of every dword, both
                             dwords of each pair whose flags are gathered together).
  ``near_misses``            valid letters and their one-bit neighbours, half and half: short dense runs.
  ``seam_walk``              one bad byte at every distance -17..+17 from a 1 KiB wave-step seam, ``N`` and 0x00.
  ``seam_walk_long``         the same over 9 MiB: a wave then walks several steps and carries its last chunk across the seam.
  ``fasta_case_text``        one FASTA record per byte value and place (interior, leading, trailing, trailing before blanks,
                             inside a run of blanks a base follows, between wrapped lines, inside the header line);
                             ``seqio_records`` / ``expected_flat`` are the Biopython-rule tokeniser the FASTA tests share.
  ``quality_cases``          FASTQ texts whose one interesting quality byte takes every value, per offset and min_quality.
  ``all_bytes_fastq``        a sequence line holding every byte value a FASTQ line can hold.
  ``window_fasta`` / ``window_fastq``
                             (11 filler bases + b) for all b, repeated one base further along per repetition, so that every
                             value falls on every offset of the k - 1 bases behind the end of a trimmed window.
"""
import collections
import re

import numpy as np

from fastq_cases import Malformed, fastq_reads

LETTERS = b'ACGTacgt'
WAVE_STEP = 1024          # 64 lanes x 16 bytes: lane 63 hands its chunk to lane 0 of the next step
CHUNK = 16                # bytes of one lane

# ----------------------------------------------------------------------------------------------------------------------------
# the reference counter
# ----------------------------------------------------------------------------------------------------------------------------
_NOT_ALPHABET = re.compile(b'[^ACGTacgt]')                                    # kpal/klib.py:152
_TO_BINARY = {ord('A'): 0, ord('a'): 0, ord('C'): 1, ord('c'): 1, ord('G'): 2, ord('g'): 2, ord('T'): 3, ord('t'): 3}   # klib.py:43-48


def reference_kmers(sequence, k):
    """The k-mers of one sequence (bytes) in the order the reference counts them (kpal/klib.py:152-168): the sequence is split
    at every byte outside ``ACGTacgt``; of every part at least k long the first k-mer is built, then one base is rolled in at a
    time."""
    out = []
    bitmask = 4 ** k - 1
    for part in _NOT_ALPHABET.split(bytes(sequence)):
        if len(part) >= k:
            binary = 0
            for c in part[:k]:
                binary = (binary << 2) | _TO_BINARY[c]
            out.append(binary)
            for c in part[k:]:
                binary = ((binary << 2) | _TO_BINARY[c]) & bitmask
                out.append(binary)
    return out


def reference_sparse(sequences, k):
    """(ascending bins, their counts) over all sequences: the non-zero part of the reference's table."""
    kmers = []
    for s in sequences:
        kmers += reference_kmers(s, k)
    return np.unique(np.asarray(kmers, dtype=np.int64), return_counts=True)


def dense(sparse, k):
    table = np.zeros(4 ** k, dtype=np.int64)
    table[sparse[0]] = sparse[1]
    return table


def reference_count(sequences, k):
    """int64[4**k]: the reference's table for an iterable of byte strings."""
    return dense(reference_sparse(sequences, k), k)


def reference_count_numpy(sequence, k):
    """The same table for ONE long sequence, by the rule's other reading (a k-mer is counted where k bytes in a row are in
    ``ACGTacgt``: SURVEY.md section 0 fact 7) in whole-array NumPy steps -- megabytes in a second, where the rolling loop above
    takes minutes.  tests/test_alphabet_cases_host.py holds the two against each other on the short texts."""
    a = np.frombuffer(bytes(sequence), dtype=np.uint8)
    n = a.size
    if n < k:
        return np.zeros(4 ** k, dtype=np.int64)
    lut = np.full(256, -1, dtype=np.int64)
    for c, v in _TO_BINARY.items():
        lut[c] = v
    codes = lut[a]
    bad = codes < 0
    seen = np.cumsum(bad)                                   # bad bytes up to and including i
    first = np.arange(0, n - k + 1)
    ok = ~bad[first] & (seen[first + (k - 1)] == seen[first])
    value = np.zeros(n - k + 1, dtype=np.int64)
    for j in range(k):
        value = (value << 2) | np.maximum(codes[j:n - k + 1 + j], 0)
    return np.bincount(value[ok], minlength=4 ** k).astype(np.int64)


# ----------------------------------------------------------------------------------------------------------------------------
# flat texts for the counting kernels
# ----------------------------------------------------------------------------------------------------------------------------
def filler(rs, n):
    """n random bases over all eight letters: case folding is always in play."""
    return bytes(bytearray(LETTERS[i] for i in rs.randint(0, 8, size=n)))


SLOT_FILL = 36            # one placement: 36 filler bases + the value; the period 37 is coprime to 16
SLOT_REPEATS = 16


def every_byte_every_slot():
    """256 values x 16 consecutive placements of (36 filler bases + value): 151 552 bytes = 148 wave-steps."""
    rs = np.random.RandomState(101)
    out = bytearray()
    for v in range(256):
        for _ in range(SLOT_REPEATS):
            out += filler(rs, SLOT_FILL)
            out.append(v)
    return bytes(out)


NEAR_MISS_BITS = (0, 1, 2, 3, 4, 6, 7)        # bit 5 is the case bit: flipping it gives the other case of the same letter
NEAR_MISS_FLIPS = tuple((c, b) for c in LETTERS for b in NEAR_MISS_BITS)      # 56 (letter, bit) pairs ...
NEAR_MISS_VALUES = tuple(sorted(set(c ^ (1 << b) for c, b in NEAR_MISS_FLIPS)))   # ... whose values coincide here and there


def near_misses():
    """64 KiB: every byte a valid letter with probability 1/2, else a valid letter with one of bits 0-4, 6, 7 flipped (56
    flips; a few give other letters, which the reference handles by itself)."""
    rs = np.random.RandomState(202)
    n = 64 << 10
    base = np.frombuffer(LETTERS, dtype=np.uint8)[rs.randint(0, 8, size=n)]
    flip = np.asarray(NEAR_MISS_BITS, dtype=np.uint8)[rs.randint(0, len(NEAR_MISS_BITS), size=n)]
    miss = rs.randint(0, 2, size=n).astype(bool)
    return np.where(miss, base ^ (np.uint8(1) << flip), base).astype(np.uint8).tobytes()


SEAM_DISTANCES = tuple(range(-17, 18))
SEAM_BAD = (ord('N'), 0)


def seam_walk():
    """For each d in -17..+17 and each of 'N' and 0x00 one bad byte at 1024 i + d, i = 1, 2, ...; everything else is filler.
    70 seams; the text ends 40 bytes behind a seam of its own, so the last wave-step is a partial one."""
    rs = np.random.RandomState(303)
    n_seams = len(SEAM_DISTANCES) * len(SEAM_BAD)
    out = bytearray(filler(rs, WAVE_STEP * (n_seams + 1) + 40))
    i = 1
    for d in SEAM_DISTANCES:
        for bad in SEAM_BAD:
            out[WAVE_STEP * i + d] = bad
            i += 1
    return bytes(out)


LONG_STEPS = 9216         # wave-steps of seam_walk_long: more than the waves of one launch, so a wave walks several
LONG_CYCLE = len(SEAM_DISTANCES) * len(SEAM_BAD) + 1     # 71 seams: the 70 of seam_walk and a clean one -- a prime, so the cycle
                                                         # meets every residue of the seam number modulo the steps a wave walks


def seam_walk_long():
    """9 MiB + 40 bytes: the seam walk again and again over 9216 seams.  The counting kernels give every wave a run of
    consecutive wave-steps and load the chunk left of the run afresh; only INSIDE a run does lane 63 hand its chunk to lane 0
    of the next step.  A text of fewer steps than a launch has waves (seam_walk) never gets there."""
    rs = np.random.RandomState(606)
    n = WAVE_STEP * LONG_STEPS + 40
    a = np.frombuffer(LETTERS, dtype=np.uint8)[rs.randint(0, 8, size=n)].copy()
    pairs = [(d, bad) for d in SEAM_DISTANCES for bad in SEAM_BAD]
    for i in range(1, LONG_STEPS + 1):
        j = (i - 1) % LONG_CYCLE
        if j < len(pairs):
            a[WAVE_STEP * i + pairs[j][0]] = pairs[j][1]
    return a.tobytes()


def interior_seam_pairs(text, steps_per_wave):
    """{(distance, bad byte)} found at the seams INSIDE the runs of `steps_per_wave` wave-steps a wave walks (seam i, between
    steps i - 1 and i, is inside a run unless i is a multiple of steps_per_wave)."""
    a = np.frombuffer(text, dtype=np.uint8)
    bad = np.flatnonzero(~np.isin(a, np.frombuffer(LETTERS, dtype=np.uint8)))
    seams = (bad + WAVE_STEP // 2) // WAVE_STEP
    inside = seams % steps_per_wave != 0
    return set(zip((bad - seams * WAVE_STEP)[inside].tolist(), a[bad][inside].tolist()))


FLAT_TEXTS = collections.OrderedDict([('every_byte_every_slot', every_byte_every_slot), ('near_misses', near_misses),
                                      ('seam_walk', seam_walk)])
_flat_cache = {}


def flat_text(name):
    if name not in _flat_cache:
        _flat_cache[name] = seam_walk_long() if name == 'seam_walk_long' else FLAT_TEXTS[name]()
    return _flat_cache[name]


_sparse_cache = {}


def flat_reference(name, k):
    """The reference's table of a flat text (computed once per (text, k); a fresh dense array per call)."""
    if (name, k) not in _sparse_cache:
        _sparse_cache[(name, k)] = reference_sparse([flat_text(name)], k)
    return dense(_sparse_cache[(name, k)], k)


# ----------------------------------------------------------------------------------------------------------------------------
# FASTA
# ----------------------------------------------------------------------------------------------------------------------------
def seqio_records(text):
    """(name, sequence) per record by Biopython's rules, written independently of kpal_amd.klib:
    universal newlines, lines before the first '>' skipped, name = first word of the title, every
    sequence line rstrip()-ed, ' ' and '\\r' removed from the joined record -- so a tab inside a
    line stays (and splits k-mer windows), a tab at the end of a line goes."""
    import re
    records, title, lines = [], None, []
    for line in re.split('\r\n|\r|\n', text):
        if line[:1] == '>':
            if title is not None:
                records.append((title, lines))
            title, lines = line[1:].rstrip(), []
        elif title is not None:
            lines.append(line.rstrip())
    if title is not None:
        records.append((title, lines))
    out = []
    for title, lines in records:
        words = title.split(None, 1)
        out.append((words[0] if words else '', ''.join(lines).replace(' ', '').replace('\r', '')))
    return out


def expected_flat(text):
    return b''.join(b'\n' + seq.encode('latin-1') for _, seq in seqio_records(text))


# str.isspace() over latin-1: what rstrip() takes off the end of a line
LATIN1_SPACE = frozenset(b for b in range(256) if chr(b).isspace())
SOFT_BLANKS = frozenset(LATIN1_SPACE - {ord('\n'), ord('\r'), ord(' ')})      # kept inside a line, dropped where they trail it
FASTA_PLACES = ('interior', 'leading', 'trailing', 'trailing_blanks', 'blank_run', 'wrapped', 'header')


def fasta_record(place, b, tag):
    """One record (latin-1 str, with its final '\\n') with the byte b at `place`."""
    c = b if isinstance(b, str) else chr(b)
    head = '>%s_%s d e\n' % (tag, place)
    if place == 'interior':
        return head + 'AC' + c + 'GT\n'
    if place == 'leading':
        return head + c + 'ACGT\n'
    if place == 'trailing':
        return head + 'ACGT' + c + '\n'
    if place == 'trailing_blanks':
        return head + 'ACGT' + c + ' \t\n'
    if place == 'blank_run':                       # (beyond the list of the issue: a run of blanks that a base follows)
        return head + 'AC' + c + '\t\x0c gt\n'
    if place == 'wrapped':
        return head + 'aC' + c + '\nGt\n'
    assert place == 'header'
    return '>%s_%s d%se\nACGT\n' % (tag, place, c)


def fasta_case_text():
    """One record per byte value and place.  '\\n' and '\\r' are line ends: they get explicit records of their own ('\\r\\n'
    too) at every place but the header and never directly behind a blank (a lone '\\r' is a line end to a file opened with
    universal newlines and to the kernels, not to a StringIO).  '>' at a line start makes its line a header: the tokeniser
    says what becomes of that record."""
    parts = ['text before the first header\nACGT\n']
    for b in range(256):
        if b in (10, 13):
            continue
        for place in FASTA_PLACES:
            parts.append(fasta_record(place, b, 'v%02x' % b))
    for tag, eol in (('lf', '\n'), ('cr', '\r'), ('crlf', '\r\n')):
        for place in ('interior', 'leading', 'trailing', 'wrapped'):
            parts.append(fasta_record(place, eol, tag))
        parts.append('>%s_before_blanks\nACGT%s \t\nAC\n' % (tag, eol))
    parts.append('>last\nACGTacgt')
    return ''.join(parts)


FASTA_CHUNKS = (17, 64, 257)      # forced chunk sizes of the file reader: cuts fall inside both kinds of blank runs (below)


def is_blank(ch):
    return ch == ' ' or ord(ch) in SOFT_BLANKS


def blank_run_cuts(text, chunk):
    """The cuts of `text` into pieces of `chunk` bytes that fall INSIDE a run of blanks of a sequence region (a blank on both
    sides, the left one a soft blank): -> (cuts whose run trails its line, cuts whose run a base -- any other byte -- follows)."""
    trailing, followed = [], []
    for c in range(chunk, len(text), chunk):
        if ord(text[c - 1]) in SOFT_BLANKS and is_blank(text[c]):
            j = c
            while j < len(text) and is_blank(text[j]):
                j += 1
            (trailing if j == len(text) or text[j] in '\r\n' else followed).append(c)
    return trailing, followed


# ----------------------------------------------------------------------------------------------------------------------------
# FASTQ
# ----------------------------------------------------------------------------------------------------------------------------
QUALITY_OFFSETS = (33, 64)
TOP_QUALITY = ord('~')


def min_qualities(offset):
    return (0, 1, 20, TOP_QUALITY - offset)


def quality_boundaries(offset, min_quality):
    """The quality bytes at which the outcome changes, by name."""
    return collections.OrderedDict([('offset-1', offset - 1), ('offset', offset), ('offset+min_quality-1', offset + min_quality - 1),
                                    ('offset+min_quality', offset + min_quality), ('~', TOP_QUALITY), ('~+1', TOP_QUALITY + 1),
                                    ('0x80', 0x80), ('0xFF', 0xFF)])


def quality_record(rs, q, number):
    """A three-base read whose middle base carries the quality byte q; its neighbours carry '~', which no mask touches."""
    return b'@q%02x_%d\n' % (q, number) + filler(rs, 3) + b'\n+\n~' + bytes(bytearray([q])) + b'~\n'


QualityCase = collections.namedtuple('QualityCase', 'label q text reads malformed')


def quality_cases(offset, min_quality):
    """One record per quality byte value q in 0..255 except 0x0a ('\\r' stands in the middle of its line, where it is a quality
    byte like any other).  Per q one text: the record of q as its LAST record behind q % 3 + 1 records that no mask objects to
    (so the number of the first malformed record varies), and -- where q is malformed -- one more good record and a second
    malformed one behind it, which must not be the one that is named.  ``reads`` (the masked sequences) or ``malformed`` (the
    1-based number of the first malformed record) is what tests/fastq_cases.fastq_reads makes of the text."""
    rs = np.random.RandomState(1000 * offset + min_quality)
    cases = []
    for q in range(256):
        if q == 10:
            continue
        records = [quality_record(rs, TOP_QUALITY - (i % 2), i) for i in range(q % 3 + 1)]
        records.append(quality_record(rs, q, len(records)))
        text = b''.join(records)
        try:
            reads, malformed = fastq_reads(text, min_quality, offset), None
        except Malformed as e:
            reads, malformed = None, e.record
            text += quality_record(rs, TOP_QUALITY, 8) + quality_record(rs, 0xFF if q != 0xFF else 0, 9)
            try:
                fastq_reads(text, min_quality, offset)
                raise AssertionError('the longer text is not malformed')
            except Malformed as e2:
                assert e2.record == malformed
        cases.append(QualityCase('q%02x' % q, q, text, reads, malformed))
    return cases


def all_bytes_fastq():
    """-> (text, sequence line): one record whose sequence line holds (3 filler bases + b) for every byte value b but '\\n';
    '\\r' is followed by more of the line, so it stays."""
    rs = np.random.RandomState(404)
    line = b''.join(filler(rs, 3) + bytes(bytearray([b])) for b in range(256) if b != 10) + filler(rs, 3)
    return b'@all\n' + line + b'\n+\n' + b'I' * len(line) + b'\n', line


# ----------------------------------------------------------------------------------------------------------------------------
# windows
# ----------------------------------------------------------------------------------------------------------------------------
WINDOW_TRIPLES = ((4, 16, 4), (8, 24, 3))      # (k, W, S)
WINDOW_FILL = 11
WINDOW_LEAD = 24


def window_line(step, exclude, pad=1):
    """(11 filler bases + b) for all byte values b not in `exclude`, `step` times over, `pad` more filler bases behind every
    repetition: a value's place moves by one base (mod the step) per repetition, so it meets every offset behind a window's end."""
    rs = np.random.RandomState(505 + step)
    out = bytearray(filler(rs, WINDOW_LEAD))        # (the first values lie behind the first window's end, too)
    for _ in range(step):
        for b in range(256):
            if b not in exclude:
                out += filler(rs, WINDOW_FILL)
                out.append(b)
        out += filler(rs, pad)
    return bytes(out + filler(rs, WINDOW_FILL))


def window_fasta(step):
    """-> (FASTA text as bytes, the record's sequence as the tokeniser flattens it).  The line ends are left out of the line (a
    record is one line here); the space is in it and the tokeniser drops it -- two pad bases per repetition make up for it."""
    line = window_line(step, (10, 13), pad=2)
    text = b'>win\n' + line + b'\n'
    (_, seq), = seqio_records(text.decode('latin-1'))
    return text, seq.encode('latin-1')


def window_fastq(step):
    """-> (FASTQ text, the read): the sequence line is taken verbatim."""
    line = window_line(step, (10,))
    return b'@win\n' + line + b'\n+\n' + b'I' * len(line) + b'\n', line


def window_spans(bases, window, step):
    """[(start, end)] of the sliding windows of a record of `bases` bases: none for an empty record, one for bases <= window,
    else ceil((bases - window) / step) + 1, only the last one truncated (Profile.from_fasta_by_window's documentation)."""
    if bases <= window:
        return [(0, bases)] if bases else []
    n = -(-(bases - window) // step) + 1
    return [(j * step, min(j * step + window, bases)) for j in range(n)]


def straddle_pairs(seq, k, window, step):
    """{(offset, value)}: the byte values found at offset 0 .. k - 2 behind the end of a window that ends before its record
    does -- where a k-mer that begins inside the window ends."""
    pairs = set()
    for start, end in window_spans(len(seq), window, step):
        if end < len(seq):
            for o in range(k - 1):
                if end + o < len(seq):
                    pairs.add((o, seq[end + o]))
    return pairs
