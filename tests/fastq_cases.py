"""FASTQ texts for the ingest tests (tests/test_gpu_fastq.py, tests/test_gpu_fastq_edges.py) -- pure Python, no GPU.

The reference reads FASTA only, so the written rules of kpal_count_feed_fastq (include/kpal_hip.h) are the specification.
``fastq_reads`` restates them independently of kpal_amd: four-line records, the '\\r' before a '\\n' dropped, roles by line index
mod 4, the length check, the optional quality mask, empty lines at the very end ignored, malformed records refused with their
number.  ``flat_of`` is the stream the counters see for those reads.

The generators put the tokeniser (kpal_amd/csrc/fastq_kernels.hpp) where its arithmetic can be off by one.  It works in
workgroup blocks of ``BLOCK`` = 4096 bytes, thread slices of ``SLICE`` = 16 bytes and waves of ``WAVE`` = 1024 bytes:

  ``edge_texts()``       (label, text): a chosen event (``EVENTS``) at a chosen edge (``EDGES``) plus a delta (``DELTAS``); the
                         label is '<event>@<edge><delta>', ``edge_target(label)`` the byte offset it names and
                         ``event_offset(event, text)`` the offset found by reading the text.
  ``long_read_texts()``  ``LongRead`` tuples: lines of one block and more, up to a megabase.
  ``range_cuts()``       cut points that split a text into consecutive byte ranges for kpal_count_feed_fastq_file.

tests/test_fastq_host.py proves on the CPU that every text is what its label says, so that an edit here cannot move a case off
its edge without a test failing.
"""
import collections
import random

BLOCK = 4096     # kFaBlockBytes: bytes of one workgroup
SLICE = 16       # kFaPerThread: bytes of one thread
WAVE = 1024      # 64 threads x 16 bytes


class Malformed(Exception):
    def __init__(self, record):
        super().__init__(record)
        self.record = record


def fastq_reads(data, min_quality=None, offset=33):
    """The reads of a FASTQ text by the rules (written independently of kpal_amd.klib): the sequence lines, masked bases as
    'N'.  Raises Malformed(1-based number of the first bad record)."""
    pieces = data.split(b'\n')
    lines = [p[:-1] if i < len(pieces) - 1 and p.endswith(b'\r') else p for i, p in enumerate(pieces)]
    last = max([i for i, line in enumerate(lines) if line] or [-1])
    reads = []
    for r in range((last + 4) // 4):
        rec = lines[4 * r:4 * r + 4]
        if not rec[0].startswith(b'@') or len(rec) < 4 or not rec[2].startswith(b'+') or len(rec[3]) != len(rec[1]):
            raise Malformed(r + 1)
        seq, qual = bytearray(rec[1]), rec[3]
        if min_quality is not None:
            for i, q in enumerate(qual):
                if q < offset or q > 126:
                    raise Malformed(r + 1)
                if q - offset < min_quality:
                    seq[i] = ord('N')
        reads.append(bytes(seq))
    return reads


def flat_of(reads):
    return b''.join(b'\n' + r for r in reads)


def random_fastq(rnd, n, max_len=300, crlf=False, offset=33, noise=True):
    """n records: titles and quality lines that begin with '@' or '+', empty reads, non-ACGT bytes, mixed or CRLF line ends."""
    out = []
    for i in range(n):
        eol = b'\r\n' if crlf or (noise and rnd.random() < 0.1) else b'\n'
        length = 0 if rnd.random() < 0.05 else rnd.randint(1, max_len)
        alphabet = b'ACGTACGTACGTacgtN' + (b'@+.- \t>' if noise else b'')
        seq = bytes(rnd.choice(alphabet) for _ in range(length))
        qual = bytes(rnd.randint(offset, 126) for _ in range(length))
        if length and offset == 33 and rnd.random() < 0.2:
            qual = bytes([rnd.choice(b'@+')]) + qual[1:]
        title = b'@' + rnd.choice([b'', b'read%d' % i, b'@@x +y', b'+plus'])
        sep = rnd.choice([b'+', b'+' + title[1:]])
        out.append(title + eol + seq + eol + sep + eol + qual + eol)
    return b''.join(out)


class Ragged(object):
    """A binary handle whose reads return pieces of random length (1 byte .. a few KiB)."""

    def __init__(self, data, seed):
        self._data, self._at, self._rnd = data, 0, random.Random(seed)

    def read(self, n=-1):
        take = self._rnd.choice([1, 2, 3, 7, 64, 333, 4096])
        piece = self._data[self._at:self._at + take]
        self._at += len(piece)
        return piece


def line_spans(text):
    """[(start, end)] of every line of the text, end = the offset of its '\\n' (len(text) for a last line without one; a text
    that ends in '\\n' has no line after it)."""
    spans, at = [], 0
    while at < len(text):
        nl = text.find(b'\n', at)
        if nl < 0:
            spans.append((at, len(text)))
            break
        spans.append((at, nl))
        at = nl + 1
    return spans


# ----------------------------------------------------------------------------------------------------------------------------
# edge texts
# ----------------------------------------------------------------------------------------------------------------------------
ROLES = ('title', 'seq', 'sep', 'qual')
EVENTS = tuple('nl_' + r for r in ROLES) + ('cr',) + tuple('first_' + r for r in ROLES) + ('empty_pair', 'eot')
# edge name -> byte offset of the first byte BEHIND the edge: a block begins there, or a thread's slice, or a wave
EDGES = collections.OrderedDict(
    [('block%d' % b, BLOCK * b) for b in (1, 2)]
    + [('slice%d' % j, BLOCK + SLICE * j) for j in (1, 37, 255)]          # the second, a middle and the last slice of block 1
    + [('wave%d' % w, BLOCK + WAVE * w) for w in (1, 2, 3)])
DELTAS = (-2, -1, 0, 1, 2)

EVENT_TITLE = b'@EVENT read'
_PRELUDE = b'@first\nACGTTGCA\n+\nIIII##II\n@second x\r\nGGN\r\n+second x\r\n@+I\r\n'
_SEQ = b'ACGTNacgtTTGACCAGTAGGCATCATGCAAGTNNACGTCAG'
_QUAL = b'@I#5II+I!IIIII&IIII5IIIIIII#IIII"II+IIIII~'
_TRAILER = b'@after\nTTGACGTAGCATGCA\n+after\n+IIIIII#IIIIIII\n@crlf\r\nACGGT\r\n+\r\nII#II\r\n'


def edge_label(event, edge, delta):
    return '%s@%s%+d' % (event, edge, delta)


def edge_target(label):
    """The byte offset a label names: its edge plus its delta."""
    event, rest = label.split('@')
    for edge, at in EDGES.items():
        if rest[:len(edge)] == edge and rest[len(edge)] in '+-':
            return at + int(rest[len(edge):])
    raise KeyError(label)


def _event_record(event):
    """-> (the record of the event, the offset of the event inside it)."""
    eol = b'\r\n' if event == 'cr' else b'\n'
    seq, qual = (b'', b'') if event == 'empty_pair' else (_SEQ, _QUAL)
    lines = [EVENT_TITLE, seq, b'+' + EVENT_TITLE[1:], qual]
    starts, at = [], 0
    for line in lines:
        starts.append(at)
        at += len(line) + len(eol)
    record = b''.join(line + eol for line in lines)
    if event.startswith('nl_'):
        r = ROLES.index(event[3:])
        return record, starts[r] + len(lines[r])
    if event.startswith('first_'):
        return record, starts[ROLES.index(event[6:])]
    if event == 'cr':
        return record, starts[1] + len(seq)
    if event == 'empty_pair':
        return record, starts[1]                    # the '\n' of the empty sequence line
    assert event == 'eot'
    return record[:-1], len(record) - 2             # the last quality byte ends the text


def edge_text(event, edge, delta):
    """A legal FASTQ text whose `event` sits at byte EDGES[edge] + delta: the title of the record before the event's record is
    padded to put it there."""
    target = EDGES[edge] + delta
    record, inside = _event_record(event)
    head = _PRELUDE + b'@pad '
    tail = b'\nACGTACGTAC\n+\nIIIII#IIII\n'
    fill = target - inside - len(head) - len(tail)
    assert fill >= 0, (event, edge, delta)
    return head + b'p' * fill + tail + record + (b'' if event == 'eot' else _TRAILER)


def edge_texts():
    """[(label, text)] over the whole product EVENTS x EDGES x DELTAS."""
    return [(edge_label(ev, edge, d), edge_text(ev, edge, d)) for ev in EVENTS for edge in EDGES for d in DELTAS]


def event_offset(event, text):
    """Where the event of an edge text really is, found by reading the text (lines by their '\\n', the event's record by its
    title) -- not by the arithmetic that built it."""
    spans = line_spans(text)
    first = [i for i in range(0, len(spans), 4) if text[spans[i][0]:spans[i][1]].startswith(EVENT_TITLE)]
    assert len(first) == 1, first
    rec = spans[first[0]:first[0] + 4]
    assert len(rec) == 4
    if event.startswith('nl_'):
        at = rec[ROLES.index(event[3:])][1]
        assert text[at:at + 1] == b'\n'
        return at
    if event.startswith('first_'):
        s, e = rec[ROLES.index(event[6:])]
        assert e > s
        return s
    if event == 'cr':
        at = rec[1][1] - 1
        assert text[at:at + 2] == b'\r\n' and at > rec[1][0]
        return at
    if event == 'empty_pair':
        assert rec[1][0] == rec[1][1] and rec[3][0] == rec[3][1] and text[rec[1][1]:rec[1][1] + 1] == b'\n'
        return rec[1][1]
    assert event == 'eot'
    assert first[0] + 4 == len(spans) and rec[3][1] == len(text) and not text.endswith(b'\n') and rec[3][1] > rec[3][0]
    return len(text) - 1


# ----------------------------------------------------------------------------------------------------------------------------
# long reads
# ----------------------------------------------------------------------------------------------------------------------------
# label, text, the lengths of the text's long lines (LONG_LINE bytes and more, line ends not counted) in order, and the
# smallest staging chunk the text is meant for (no case may need more than MAX_CHUNK_ITERATIONS chunks)
LongRead = collections.namedtuple('LongRead', 'label text long_lines min_chunk')
LONG_LINE = 4095
MAX_CHUNK_ITERATIONS = 4096
MASK_QUALITY = 20          # the mask the long reads' qualities are made for
MASK_PERIOD = 61           # every MASK_PERIOD-th base of a long read, unless it is an 'N', has a quality below MASK_QUALITY
MAX_N_RUN = 600            # the longest run of 'N' inside a long read


def long_sequence(rnd, n, plain=False):
    """(sequence, quality) of n bases: random ACGT with stretches of lower case and runs of 'N' (1, 15, 16, 17 and up to
    MAX_N_RUN bytes: around a thread's slice) unless `plain`; qualities random in 0..60 with quality 2 under every MASK_PERIOD-th base
    that is not an 'N', so that a mask at MASK_QUALITY changes a base in any stretch of MAX_N_RUN + 2 * MASK_PERIOD bytes."""
    seq = bytearray(rnd.choices(b'ACGT', k=n))
    if not plain:
        at = rnd.randint(0, 500)
        runs = [1, 15, 16, 17, MAX_N_RUN, 33, 2, 255]
        turn = 0
        while at < n:
            length = runs[turn % len(runs)]
            if turn % 3 == 2:
                seq[at:at + length + 40] = bytes(seq[at:at + length + 40]).lower()
            else:
                seq[at:at + length] = b'N' * min(length, n - at)
            at += length + rnd.randint(150, 900)
            turn += 1
    qual = bytearray(33 + q for q in rnd.choices(range(61), k=n))
    for i in range(7, n, MASK_PERIOD):
        if seq[i] != ord('N'):
            qual[i] = ord('#')
    return bytes(seq[:n]), bytes(qual)


def _record(title, seq, qual, eol=b'\n', sep=b'+'):
    return title + eol + seq + eol + sep + eol + qual + eol


def long_read_texts():
    """[LongRead]: sequence lines of 4095, 4096 (also beginning exactly at a block), 4097, 8192, 65 537 and 1 000 003 bytes
    between short records; a title longer than a block; a long read before 3000 one-base reads; a long read with CRLF line
    ends; every long read with runs of 'N', lower case and qualities that a mask at 20 acts on in every block."""
    rnd = random.Random(4096)
    short = _record(b'@s', b'ACGTTGCAAC', b'IIII#IIIII')
    out = []
    for n in (4095, 4096, 4097, 8192, 65537, 1000003):
        seq, qual = long_sequence(rnd, n)
        text = short + _record(b'@long %d' % n, seq, qual, sep=b'+long %d' % n) + short
        out.append(LongRead('seq_%d' % n, text, (n, n), 65536 if n > 100000 else BLOCK))
    seq, qual = long_sequence(rnd, BLOCK)
    head = short + b'@aligned '
    text = head + b'a' * (BLOCK - len(head) - 1) + b'\n' + seq + b'\n+\n' + qual + b'\n' + short
    assert text.index(seq) == BLOCK
    out.append(LongRead('seq_4096_at_block_start', text, (BLOCK, BLOCK), BLOCK))
    title = b'@' + bytes(rnd.choices(b'title @+\t', k=5000))
    out.append(LongRead('title_5001', short + _record(title, b'ACGTNNACGTAC', b'III#IIIII#II') + short, (5001,), BLOCK))
    seq, qual = long_sequence(rnd, 20000)
    singles = b''.join(_record(b'@%d' % i, b'ACGTN'[i % 5:i % 5 + 1], b'I#'[i % 2:i % 2 + 1]) for i in range(3000))
    out.append(LongRead('long_then_3000_singles', _record(b'@long', seq, qual) + singles, (20000, 20000), BLOCK))
    seq, qual = long_sequence(rnd, 12289)
    out.append(LongRead('long_crlf', short + _record(b'@crlf', seq, qual, eol=b'\r\n') + _record(b'@t', b'AC', b'II', eol=b'\r\n'),
                        (12289, 12289), BLOCK))
    seq, qual = long_sequence(rnd, 30001)
    out.append(LongRead('long_without_final_newline', short + _record(b'@open', seq, qual)[:-1], (30001, 30001), BLOCK))
    return out


def blocks_without_masked_base(text, min_quality=MASK_QUALITY):
    """For every long sequence line of the text: the 4 KiB stretches in which the mask at `min_quality` changes no base --
    the blocks of the text (multiples of BLOCK) that lie wholly inside the line, and the line's own first and last BLOCK bytes.
    -> [(line number, start, end)]; empty when the qualities do what long_sequence promises."""
    spans = line_spans(text)
    bad = []
    for li in range(1, len(spans), 4):
        s, e = spans[li]
        if e > s and text[e - 1:e] == b'\r':
            e -= 1
        if e - s < LONG_LINE:
            continue
        qs = spans[li + 2][0]
        stretches = [(s, min(s + BLOCK, e)), (max(s, e - BLOCK), e)]
        stretches += [(b, b + BLOCK) for b in range((s + BLOCK - 1) // BLOCK * BLOCK, e - BLOCK + 1, BLOCK)]
        for a, b in stretches:
            changed = any(text[qs + i - s] - 33 < min_quality and text[i] != ord('N') for i in range(a, b))
            if not changed:
                bad.append((li, a, b))
    return bad


# ----------------------------------------------------------------------------------------------------------------------------
# byte ranges
# ----------------------------------------------------------------------------------------------------------------------------
def range_cuts(text, seed):
    """Lists of cut points c[0] = 0 <= c[1] <= ... <= c[-1] = len(text): the consecutive ranges [c[i], c[i + 1]) tile the text.
    The first list cuts inside a line of every role, between every '\\r' and its '\\n' (the first few), makes one-byte ranges
    and empty ranges at 0, in the middle and at len(text); the second is ten random cuts; the third cuts into ranges of at
    most three bytes around the middle of the text."""
    n = len(text)
    rnd = random.Random(seed)
    spans = line_spans(text)
    cuts = [0, 0, n, n]
    for role in range(4):
        inside = [(s, e) for s, e in spans[role::4] if e - s >= 2]
        if inside:
            s, e = inside[rnd.randrange(len(inside))]
            c = rnd.randrange(s + 1, e)
            cuts += [c, c + 1]                              # a one-byte range inside the line
    at, found = 0, 0
    while found < 3:
        at = text.find(b'\r\n', at)
        if at < 0:
            break
        cuts.append(at + 1)
        at += 2
        found += 1
    if n:
        mid = rnd.randrange(n)
        cuts += [mid, mid]                                  # an empty range in the middle
    structured = sorted(cuts)
    scattered = sorted([0, n] + [rnd.randint(0, n) for _ in range(10)])
    lo = max(0, n // 2 - 40)
    hi = min(n, lo + 80)
    fine = [0, lo]
    while fine[-1] < hi:
        fine.append(min(hi, fine[-1] + rnd.randint(1, 3)))
    fine.append(n)
    return [structured, scattered, sorted(fine)]


def ranges_of(cuts):
    return list(zip(cuts[:-1], cuts[1:]))
