"""Drop-in for ``kpal.klib``: the :class:`Profile` container with k-mer counting, balance, split, merge, shrink and the
statistics running as HIP kernels on an MI355X.

Same constructor, classmethods, methods, properties and error behaviour as the reference class
(kpal/klib.py:26-487).  Differences are internal only:

* ``from_sequences`` / ``from_fasta`` do not loop over characters in Python: sequences are joined
  into a flat byte stream (one ``\\n`` between sequences -- any byte outside ``AaCcGgTt`` splits
  windows exactly like the reference's ``re.split``, kpal/klib.py:152-156) and fed to
  ``kpal_count_feed``.
* FASTA is tokenised here (the reference delegates to ``Bio.SeqIO.parse``, kpal/klib.py:111,131):
  lines starting with ``>`` open a record whose name is the first whitespace-delimited token;
  the record's remaining lines are concatenated with surrounding whitespace removed; text before
  the first ``>`` is ignored.
* ``balance`` / ``split`` / ``merge`` / ``shrink`` and the statistics of integer counts call ``kpal_balance`` / ``kpal_split`` /
  ``kpal_merge`` / ``kpal_shrink`` / ``kpal_stats``.
* A freshly counted table stays in HBM (``_DeviceBatch``) until something asks for ``counts``, within a budget of live bytes.
* Beyond the reference: one profile per record, per read and per sliding window (``from_fasta_by_record`` ...), and the
  operations over whole SETS of profiles -- ``summaries``, ``strand_balances``, ``distributions``, ``balance_profiles``,
  ``shrink_profiles``, ``merge_profiles``, ``smooth_profiles``, ``pooled``, ``pooled_by`` -- in launches that do not grow with the set.  They
  share one core: ``_may_stay`` (the residency budget), ``_groups`` (places by k-mer length in groups of bounded bytes) and
  ``kdistlib._DeviceSet`` (profiles as consecutive device tables, where they lie or gathered).

There is no CPU fallback for those paths: without libkpal_hip.so or without a GPU they raise.  Only what cannot enter a
kernel -- non-integer counts (scaled profiles), user callables, ``shuffle``, the printers, HDF5 I/O -- uses NumPy like the
reference.
"""
import codecs
import contextlib
import io
import itertools
import math
import os
import stat

import numpy as np

from . import _native, kdistlib, metrics

# The C gatherer of from_sequences (csrc/kpal_gather.c, built by __graft_entry__.build(): walks the list's objects and copies them on
# several threads); without it the sequences are joined by the interpreter -- same stream, ~3 x slower for lists of short reads.
try:
    from . import _kpal_gather
except ImportError:       # pragma: no cover
    _kpal_gather = None

_FEED_BYTES = 32 << 20  # host-side join buffer per feed
_GATHER_BYTES = 64 << 20  # page-locked gather buffer of from_sequences
_GATHER_THREADS = max(1, min(64, int(os.environ.get('KPAL_GATHER_THREADS', '16'))))   # threads of the gatherer (walk + copies; 4 / 8 / 16 / 32: 114 / 88 / 80 / 92 ms for 8 M reads)
_JOIN_BLOCK = 4096       # sequences joined per C-level call
_RECORD_BATCH_BYTES = 1 << 30   # tables counted per from_fasta_by_record batch
# from_fasta_by_record leaves its tables in HBM (Profile.counts downloads on first access) while no more than this many bytes of
# them are alive; past it a batch is downloaded at once into one host array (KPAL_DEVICE_PROFILE_BYTES; 0: always download)
_DEVICE_PROFILE_BYTES = int(os.environ.get('KPAL_DEVICE_PROFILE_BYTES', str(64 << 30)))


class _DeviceBatch(object):
    """The tables of one batch of ``from_fasta_by_record`` in device memory: n x 4^k int64, never written again.  Every
    profile of the batch that has not been asked for its counts yet holds a reference; the memory goes back when the last
    one is dropped or materialised."""
    live_bytes = 0

    _POOL_BYTES = 1 << 30      # freed allocations a context keeps for the next batch of the same size (hipMalloc + hipFree of a
                               # 128 MiB table cost a from_sequences call of a million reads 5 of its 23 ms)

    def __init__(self, ctx, nbytes, n_tables):
        self.ctx, self.nbytes, self.n_tables = ctx, int(nbytes), int(n_tables)
        self.ptr = None            # (an allocation that raises leaves a batch that never counted: __del__)
        pool = getattr(ctx, '_table_pool', None)
        if pool and pool.get(self.nbytes):
            self.ptr = pool[self.nbytes].pop()
            ctx._table_pool_bytes -= self.nbytes
        else:
            self.ptr = ctx.alloc(self.nbytes)
        self.host = None
        self._stats = None
        _DeviceBatch.live_bytes += self.nbytes

    def table(self, index):
        """Table ``index`` on the host.  The first request brings the WHOLE batch over in one copy (a profile at a time cost
        140 us per 512 KiB table: `kpal count --by-record` asks for every one of them); the rows are views of that array, as
        the tables of a batch that is downloaded at once are."""
        if self.host is None:
            host = np.empty((self.n_tables, self.nbytes // (8 * self.n_tables)), dtype=np.int64)
            self.ctx.d2h(host, self.ptr)
            self.host = host
        return self.host[index]

    def stats(self, index):
        """The summaries of table ``index``.  The first request summarises the WHOLE batch in one ``kpal_stats_set_device``
        call (launches that do not grow with the batch; a profile at a time cost five launches and five round trips each) and
        keeps the result: the tables of a batch are never written, so it stays valid."""
        if self._stats is None:
            self._stats = self.ctx.stats_set_device(self.ptr, self.n_tables, self.nbytes // (8 * self.n_tables))
        return self._stats[index]

    def __del__(self):
        try:
            if self.ptr is None:
                return
            _DeviceBatch.live_bytes -= self.nbytes
            ctx = self.ctx
            if getattr(ctx, '_h', None):           # (a context that has been closed took its allocations with it)
                if getattr(ctx, '_table_pool', None) is None:
                    ctx._table_pool, ctx._table_pool_bytes = {}, 0
                if ctx._table_pool_bytes + self.nbytes <= _DeviceBatch._POOL_BYTES:
                    ctx._table_pool.setdefault(self.nbytes, []).append(self.ptr)
                    ctx._table_pool_bytes += self.nbytes
                else:
                    ctx.free(self.ptr)
        except Exception:       # pragma: no cover  (interpreter shutdown)
            pass


def _may_stay(nbytes):
    """Whether ``nbytes`` more of tables may stay in HBM: the budget of live device tables (0: none ever does)."""
    return bool(_DEVICE_PROFILE_BYTES) and _DeviceBatch.live_bytes + nbytes <= _DEVICE_PROFILE_BYTES


def _tables_per_group(k, sides=1):
    """Places of ``sides`` tables of 4^k counts each that make ``_RECORD_BATCH_BYTES``, never fewer than one."""
    return max(1, _RECORD_BATCH_BYTES // (sides * 8 * 4 ** k))


def _groups(places, length_of, sides=1):
    """``places`` by k-mer length (``length_of(place)``), ascending k, in groups of at most ``_RECORD_BATCH_BYTES`` over
    ``sides`` tables per place, never fewer than one place: yields ``(k, group)``."""
    by_length = {}
    for i in places:
        by_length.setdefault(length_of(i), []).append(i)
    for k, same in sorted(by_length.items()):
        per = _tables_per_group(k, sides)
        for at in range(0, len(same), per):
            yield k, same[at:at + per]


def _kmer_length(length):
    """``length`` as an integer; ValueError unless it is a k-mer length the library counts."""
    length = int(length)
    if length < 1 or length > _native.KPAL_MAX_K:
        raise ValueError('k-mer length must be in 1..%d (got %d)' % (_native.KPAL_MAX_K, length))
    return length


_FASTA_CHUNK = 64 << 20  # FASTA text read per device feed (cut back to a record boundary)
_DROPPED = {ord(' '): None, ord('\r'): None}   # removed from the joined record (Biopython's SimpleFastaParser)


def _fasta_records(handle):
    """Yield ``(name, sequence)`` per FASTA record, tokenised like ``Bio.SeqIO.parse(handle, 'fasta')``
    (what kpal/klib.py:111 delegates to): text before the first ``>`` is skipped, the name is the
    first word of the title, every sequence line is ``rstrip()``-ed and the joined record loses its
    spaces and ``\\r`` -- whitespace such as a tab INSIDE a line stays and separates k-mer windows."""
    name = None
    parts = []
    for line in handle:
        if isinstance(line, bytes):
            line = line.decode('latin-1')      # (one character per byte, as the device reads them: 0x85 and 0xa0 are blanks)
        if line.startswith('>'):
            if name is not None:
                yield name, ''.join(parts).translate(_DROPPED)
            title = line[1:].strip()
            name = title.split(None, 1)[0] if title else ''
            parts = []
        elif name is not None:
            parts.append(line.rstrip())
    if name is not None:
        yield name, ''.join(parts).translate(_DROPPED)


def _ascii_compatible(handle):
    """Whether the bytes under the text handle ``handle`` are its ASCII text: an ASCII-compatible encoding."""
    try:
        return codecs.lookup(handle.encoding or '').name in ('utf-8', 'ascii', 'iso8859-1')
    except LookupError:
        return False


def _plain_file(handle):
    """``(path, byte position)`` when ``handle`` is an ordinary file opened for reading whose raw bytes ARE its text and whose
    position is known -- an ``open(path)`` / ``open(path, 'rb')`` / ``argparse.FileType('r')`` handle on a regular file, in an
    ASCII-compatible encoding, not yet read from (text mode) or at any position (binary mode) -- else None (StringIO, pipes,
    gzip / bz2 wrappers, sockets, handles somebody has read from ...).  The library then reads the file itself
    (``kpal_count_feed_fasta_file``); ``/proc/self/fd/N`` names the open file whatever its path was."""
    raw = handle
    text_mode = isinstance(handle, io.TextIOWrapper)
    if text_mode:
        if not _ascii_compatible(handle):
            return None
        raw = handle.buffer
    if isinstance(raw, io.BufferedReader):
        raw = raw.raw
    if type(raw) is not io.FileIO or not raw.readable():
        return None
    try:
        fd = raw.fileno()
        if not stat.S_ISREG(os.fstat(fd).st_mode):
            return None
        position = handle.tell()
    except (OSError, ValueError):
        return None
    if text_mode and position != 0:      # (a text handle's tell() is an opaque cookie anywhere but at the start)
        return None
    path = '/proc/self/fd/%d' % fd
    return (path, position) if os.path.exists(path) else None


def _first_boundary(text):
    """Index of the end-of-line byte before the first header line of ``text`` (the first
    occurrence of EOL followed by ``>``), or -1; a chunk that itself starts with ``>`` starts a
    record at 0 only if the previous chunk ended with an EOL, which the caller's carry contains."""
    a = text.find(b'\n>')
    b = text.find(b'\r>', 0, a + 1) if a >= 0 else text.find(b'\r>')   # only an earlier one matters
    if a < 0:
        return b
    return a if b < 0 else min(a, b)


def _last_boundary(text, begin):
    """Index of the end-of-line byte before the last header line at or after ``begin``, or -1."""
    a = text.rfind(b'\n>', begin)
    b = text.rfind(b'\r>', max(begin, a))    # only a later one matters
    return max(a, b)


def _line_end(text, start):
    """Index of the first end-of-line byte (``\\n`` or ``\\r``) of ``text`` at or after ``start``, or ``len(text)``."""
    a = text.find(b'\n', start)
    if a < 0:
        a = len(text)
    b = text.find(b'\r', start, a)
    return a if b < 0 else b


def _byte_reader(handle):
    """``(reader, encoding)``: what to ``read()`` the text of ``handle`` from -- the undecoded bytes under a text handle in an
    ASCII-compatible encoding that has not been read from yet (a pipe, a decompressing wrapper; titles are decoded with that
    encoding), else the handle itself."""
    if isinstance(handle, io.TextIOWrapper):
        try:
            if _ascii_compatible(handle) and handle.tell() == 0:
                return handle.buffer, handle.encoding
        except (OSError, ValueError):
            pass
    return handle, 'ascii'


def _whole_record_chunks(handle):
    """FASTA text of ``handle`` in pieces of about ``_FASTA_CHUNK`` bytes that hold WHOLE records: ``(bytes, str or None, encoding)`` --
    the text as bytes (what the device tokenises) and, for handles that yield ``str`` in an encoding of their own, the same
    text as the ``str`` the names are read from (one byte per character: positions agree)."""
    (reader, encoding), keep_str = _byte_reader(handle), False
    pending = bytearray()                 # text not handed out yet: ends inside a record
    pending_str = []
    while True:
        text = reader.read(_FASTA_CHUNK)
        if not text:
            break
        if not isinstance(text, bytes):
            keep_str = True
            pending_str.append(text)
            text = text.encode('latin-1', 'replace')
        searched = max(len(pending) - 1, 0)   # (a boundary is two bytes: EOL + '>')
        pending += text
        cut = _last_boundary(pending, searched)
        if cut >= 0:                      # whole records up to the end of line before the last header line
            out = bytes(pending[:cut + 1])
            del pending[:cut + 1]
            out_str = None
            if keep_str:
                joined = ''.join(pending_str)
                out_str, pending_str = joined[:cut + 1], [joined[cut + 1:]]
            yield out, out_str, encoding
    if pending:
        yield bytes(pending), (''.join(pending_str) if keep_str else None), encoding


def _fasta_texts(ctx, handle):
    """Pieces of whole records of a FASTA handle, each indexed on the device: ``(text, text_str, encoding, n_records, again)``,
    ``again()`` indexing the same text once more."""
    for text, text_str, encoding in _whole_record_chunks(handle):
        def again(text=text):
            return ctx.fasta_records_begin(text)[0]
        yield text, text_str, encoding, again(), again


def _four_line_ends(text):
    """Whether ``text`` holds the four ``\\n`` a FASTQ record needs."""
    at = -1
    for _ in range(4):
        at = text.find(b'\n', at + 1)
        if at < 0:
            return False
    return True


def _fastq_texts(ctx, handle, seen, min_quality, quality_offset):
    """The same for a FASTQ handle.  What ``read()`` returns is cut anywhere, and only the tokeniser knows where a read ends
    (a quality line may begin with ``@``): a piece is tokenised behind the rest the piece before left unfinished, the bytes of the
    reads it finishes are kept -- ``again()`` indexes those as a text that ends there -- and the rest is carried.  ``seen[0]``,
    the reads the caller has taken so far, numbers a malformed read over the whole handle."""
    reader, encoding = _byte_reader(handle)
    carry, carry_str = b'', None
    final = False
    while not final:
        text = reader.read(_FASTA_CHUNK)
        final = not text
        text_str = None
        if not isinstance(text, bytes):
            text_str = text if carry_str is None else carry_str + text
            text = text.encode('latin-1', 'replace')
        text = carry + text
        if not final and not _four_line_ends(text):      # (a read is four lines: nothing to index yet)
            carry, carry_str = text, text_str
            continue
        if not text:
            break
        before = seen[0]
        n_records, _, consumed = ctx.fastq_records_begin(text, min_quality, quality_offset, final, before)
        kept, carry = text[:consumed], text[consumed:]
        kept_str = None
        if text_str is not None:
            kept_str, carry_str = text_str[:consumed], text_str[consumed:]
        if n_records:
            def again(kept=kept, before=before):
                return ctx.fastq_records_begin(kept, min_quality, quality_offset, True, before)[0]
            yield kept, kept_str, encoding, n_records, again


def _indexed_pieces(ctx, handle, prefix, who, fastq=None, keep_text=False):
    """The records of a FASTA handle -- with ``fastq = (min_quality, quality_offset)``, the reads of a FASTQ handle -- piece by
    piece of whole records, each piece tokenised and indexed ON THE DEVICE (``kpal_fasta_records_begin`` /
    ``kpal_fastq_records_begin`` / ``kpal_fasta_records_file_next``): yields ``(names, bases, indexed)`` -- the records'
    names (``prefix`` + the first word of the title, or the 1-based index of an untitled record, kpal/klib.py:132), their
    lengths in bases, and a callable that makes sure the context still holds THIS piece's index.

    The reference's generators are independent of each other (zip() of two, nesting, one abandoned half-way), and the
    callers of this one yield with a piece indexed on the process-wide context.  So they call ``indexed()`` before every
    batch: when another scan has used the context since, the piece is indexed again.

    A malformed FASTQ read raises ``ValueError`` when the scan reaches its piece: nothing of that piece has been yielded.
    ``keep_text``: the handle is read here whatever it is, and ``indexed.text`` is the piece's text."""
    seen = [0]                                 # records seen so far

    def name_of(title):
        words = title.split(None, 1)
        seen[0] += 1
        return prefix + (words[0] if words else str(seen[0]))

    plain = None if keep_text else _plain_file(handle)
    if plain is not None and os.path.getsize(plain[0]) > plain[1]:
        # an ordinary file: the library reads it itself (parallel preads into pinned memory, pieces of whole records);
        # the names are read from the header lines through a read-only mapping of the file
        import mmap
        encoding = handle.encoding if isinstance(handle, io.TextIOWrapper) else 'ascii'
        # Nothing of the scan lives in the context across a yield: the scan is opened at `resume`, asked for ONE piece and
        # closed again; a piece that has to be indexed again is bytes [at, resume).
        def index_piece(begin, end, before):
            if fastq is None:
                ctx.fasta_records_file_open(plain[0], begin, end)
            else:
                ctx.fastq_records_file_open(plain[0], begin, end, fastq[0], fastq[1], before)
            try:
                piece = ctx.fasta_records_file_next()
                return piece, (ctx.fasta_records_file_tell() if piece is not None else end)
            finally:
                ctx.fasta_records_file_close()

        with open(plain[0], 'rb') as raw, mmap.mmap(raw.fileno(), 0, access=mmap.ACCESS_READ) as text:
            resume = plain[1]
            while True:
                before = seen[0]
                piece, resume = index_piece(resume, 0, before)
                if piece is None:
                    break
                n_records, _, at = piece
                if n_records == 0:
                    continue
                scan = [ctx._records_scan]
                header_off, flat_start = ctx.fasta_records_index()
                names = [name_of(text[h + 1:_line_end(text, h)].decode(encoding, 'replace')) for h in (header_off + np.uint64(at)).tolist()]

                def indexed(at=at, resume=resume, n_records=n_records, scan=scan, before=before):
                    if ctx._records_scan != scan[0]:
                        again, _ = index_piece(at, resume, before)
                        if again is None or again[0] != n_records:
                            raise RuntimeError('%s: bytes %d..%d of %s changed under the scan' % (who, at, resume, plain[0]))
                        scan[0] = ctx._records_scan

                yield names, np.diff(flat_start) - np.uint64(1), indexed
        handle.seek(0, os.SEEK_END)          # the handle has been consumed, as by the reference's SeqIO.parse loop
        return
    texts = _fasta_texts(ctx, handle) if fastq is None else _fastq_texts(ctx, handle, seen, fastq[0], fastq[1])
    for text, text_str, encoding, n_records, again in texts:
        if n_records == 0:
            continue
        header_off, flat_start = ctx.fasta_records_index()
        names = []
        for h in header_off.tolist():
            end = _line_end(text, h)
            names.append(name_of(text_str[h + 1:end] if text_str is not None else text[h + 1:end].decode(encoding, 'replace')))
        scan = [ctx._records_scan]

        def indexed(again=again, scan=scan):
            if ctx._records_scan != scan[0]:     # another scan used the context since the last batch: this text again
                again()
                scan[0] = ctx._records_scan

        if keep_text:
            indexed.text = text
        yield names, np.diff(flat_start) - np.uint64(1), indexed


def _window_count(bases, window, step):
    """Sliding windows of a record of ``bases`` bases (csrc/window_index.hpp: win_count)."""
    if bases <= window:
        return 1 if bases else 0
    return -(-(bases - window) // step) + 1


def _window_arguments(length, window, step):
    """``(length, window, step)`` as integers (``step`` defaults to ``window``); ValueError unless ``1 <= length <= window``,
    ``1 <= step <= window`` and ``step`` divides ``window``."""
    length, window = int(length), int(window)
    step = window if step is None else int(step)
    _kmer_length(length)
    if window < length:
        raise ValueError('the window (%d) must be at least as long as the k-mers (%d)' % (window, length))
    if step < 1 or step > window or window % step:
        raise ValueError('the step (%d) must be in 1..window and divide the window (%d)' % (step, window))
    if window > 1 << 62:
        raise ValueError('the window (%d) is too long' % window)
    return length, window, step


def _read_arguments(length, min_quality, quality_offset):
    """``length`` as an integer; ValueError unless it is a k-mer length and the mask options are those of ``from_fastq``."""
    length = _kmer_length(length)
    _native.fastq_options_check(min_quality, quality_offset)
    return length


def _fastq_reads(ctx, handle, prefix, min_quality, quality_offset):
    """``(name, read)`` per read of a FASTQ handle, the reads as the device tokeniser flattens them (``kpal_fastq_flatten``:
    masked bases are ``N``) -- for a k whose tables are counted one at a time."""
    for names, _, indexed in _indexed_pieces(ctx, handle, prefix, 'from_fastq', (min_quality, quality_offset), keep_text=True):
        reads = ctx.fastq_flatten(indexed.text, min_quality, quality_offset).split(b'\n')[1:]
        for pair in zip(names, reads):
            yield pair


def _named_sequences(handle, prefix, fastq):
    """``(name, sequence)`` per record of a FASTA handle -- with ``fastq = (min_quality, quality_offset)``, per read of a FASTQ
    handle -- for a k whose table alone exceeds the batch budget: ``from_sequences`` then counts them one by one."""
    if fastq is not None:
        return _fastq_reads(_native.context(), handle, prefix, fastq[0], fastq[1])
    return ((prefix + (record_name or str(i + 1)), seq) for i, (record_name, seq) in enumerate(_fasta_records(handle)))


def _join_block(block):
    """One flat byte string for a block of sequences, ``\\n`` between them: C-speed joins for the
    homogeneous cases (all ``str`` / all ``bytes``), per-item encoding otherwise."""
    try:
        return '\n'.join(block).encode('latin-1', 'replace')
    except TypeError:
        pass
    try:
        return b'\n'.join(block)
    except TypeError:
        return b'\n'.join(_encode(s) for s in block)


def _gather_feed(ctx, sequences):
    """Feed ``sequences`` to the running count through the C gatherer: the items of a list are copied (each followed by the
    separator ``\\n``) into a page-locked buffer by several threads and handed to ``kpal_count_feed_pinned`` buffer by
    buffer.  A sequence is never split over two feeds (windows do not span feeds); one that does not fit the buffer goes
    through ``kpal_count_feed`` on its own; items the gatherer does not know (``str`` with characters beyond latin-1,
    ``memoryview`` ...) are encoded here, one at a time."""
    # one page-locked buffer per context, kept ON the context: it goes when the context is closed (kpal_ctx_destroy frees it)
    if getattr(ctx, '_gather_buffer', None) is None:
        ctx._gather_buffer = ctx.host_alloc(_GATHER_BYTES)
    address, view = ctx._gather_buffer
    cap = view.size
    fill = 0
    it = None if isinstance(sequences, (list, tuple)) else iter(sequences)
    while True:
        block = sequences if it is None else list(itertools.islice(it, 1 << 16))
        pos = 0
        while pos < len(block):
            pos, nbytes, status = _kpal_gather.gather(block, pos, address + fill, cap - fill, _GATHER_THREADS)
            fill += nbytes
            if status == 0:
                break
            data = None
            if status == 2:                      # an item the gatherer does not read: encoded here
                data = _encode(block[pos]) + b'\n'
                if len(data) <= cap - fill:
                    view[fill:fill + len(data)] = np.frombuffer(data, dtype=np.uint8)
                    fill += len(data)
                    pos += 1
                    continue
            if fill:                             # the buffer is full: hand it over, go on with an empty one
                ctx.count_feed_pinned(address, fill)
                fill = 0
            elif data is not None or len(block[pos]) + 1 > cap:
                ctx.count_feed(data if data is not None else _encode(block[pos]))   # larger than the buffer: on its own
                pos += 1
        if it is None or not block:
            break
    if fill:
        ctx.count_feed_pinned(address, fill)


def _encode(sequence):
    if isinstance(sequence, (bytes, bytearray, memoryview)):
        return bytes(sequence)
    # non-latin-1 characters can never be nucleotides: they become '?' (a separator)
    return str(sequence).encode('latin-1', 'replace')


def _summary_dict(s):
    return {'total': np.int64(s.total), 'non_zero': int(s.non_zero), 'mean': np.float64(s.mean),
            'median': np.float64(s.median), 'std': np.float64(s.std)}


def _set_counts(profile):
    """Whether ``profile`` can be one table of a device set: 4^k integer counts, in HBM or on the host.  (A table in HBM is not
    asked for its counts.)"""
    if profile._device_counts():
        return True
    c = np.asanyarray(profile.counts)
    return c.dtype.kind in 'iub' and c.ndim == 1 and c.size == 4 ** profile.length


def _device_sets(profiles, indices):
    """``indices`` -- places in ``profiles`` of integer profiles -- by k-mer length and in groups of at most
    ``_RECORD_BATCH_BYTES`` of tables: yields (places, context, device address of their consecutive tables, k).  Tables that
    are consecutive in one batch are used where they lie, others are gathered (``kdistlib._DeviceSet``)."""
    for k, group in _groups(indices, lambda i: profiles[i].length):
        members = [profiles[i] for i in group]
        ctx = kdistlib._cross_context(members)
        with kdistlib._DeviceSet(ctx, members) as dset:
            yield group, ctx, dset.ptr, k


def summaries(profiles):
    """``[p.summary() for p in profiles]`` -- the same keys, types and values -- with the integer profiles summarised as SETS
    (``kpal_stats_set_device``: a number of launches that does not grow with the set).  A table that is still in HBM is
    summarised where it lies with the rest of its batch, once (``_DeviceBatch.stats``), and stays there; host counts of one
    k-mer length are uploaded in groups of at most ``_RECORD_BATCH_BYTES``.  Lengths may be mixed; profiles that are not
    integer counts (scaled ones) take their own ``summary()``."""
    profiles = list(profiles)
    out = [None] * len(profiles)
    host = []
    for i, p in enumerate(profiles):
        if p._device_counts():
            out[i] = p.summary()
        elif _set_counts(p):
            host.append(i)
        else:
            out[i] = p.summary()
    for group, ctx, ptr, k in _device_sets(profiles, host):
        stats = ctx.stats_set_device(ptr, len(group), 4 ** k)
        for j, i in enumerate(group):
            out[i] = _summary_dict(stats[j])
    return out


def strand_balances(profiles, pairwise='prod'):
    """The strand balance score of every profile (kpal/kmer.py:243-245: the multiset distance between the forward and the
    reverse-complement half) as a list of float, the integer profiles as SETS (``kpal_strand_balance_set_device``: two launches
    per set) under the rules of ``summaries``; no table that is still in HBM is downloaded.  ``pairwise``: 'prod' or 'sum'.
    Other profiles take the NumPy route of ``kmer.get_balance``: ``split`` and ``metrics.multiset``."""
    native = {'prod': _native.PAIRWISE_PROD, 'sum': _native.PAIRWISE_SUM}[pairwise]
    profiles = list(profiles)
    out = [None] * len(profiles)
    sets = []
    for i, p in enumerate(profiles):
        if _set_counts(p):
            sets.append(i)
        else:
            forward, reverse = p.split()
            out[i] = float(metrics.multiset(forward, reverse, metrics.pairwise[pairwise]))
    for group, ctx, ptr, k in _device_sets(profiles, sets):
        scores = ctx.strand_balance_set_device(k, len(group), ptr, native)
        for j, i in enumerate(group):
            out[i] = float(scores[j])
    return out


def distributions(profiles):
    """``[metrics.distribution(p.counts) for p in profiles]`` -- the count-of-counts spectrum of every profile as a list of
    ``(value, number)`` pairs of Python ints, values ascending -- with the integer profiles taken as SETS
    (``kpal_distribution_set_device``: no sort, a number of launches that does not grow with the set) under the rules of
    ``summaries``: a table that is still in HBM is used where it lies and stays there, host counts of one k-mer length are
    uploaded in groups of at most ``_RECORD_BATCH_BYTES``, lengths may be mixed.  Profiles that are not integer counts
    (scaled ones) take the ``Counter`` route of ``metrics.distribution``."""
    profiles = list(profiles)
    out = [None] * len(profiles)
    sets = []
    for i, p in enumerate(profiles):
        # (uint64 counts would be ordered as int64 on the device: they keep the host route)
        if _set_counts(p) and (p._device_counts() or np.asanyarray(p.counts).dtype != np.uint64):
            sets.append(i)
        else:
            out[i] = metrics.distribution(p.counts)
    for group, ctx, ptr, k in _device_sets(profiles, sets):
        offsets, values, numbers = ctx.distribution_set_device(ptr, len(group), 4 ** k)
        offsets, values, numbers = offsets.tolist(), values.tolist(), numbers.tolist()
        for j, i in enumerate(group):
            out[i] = list(zip(values[offsets[j]:offsets[j + 1]], numbers[offsets[j]:offsets[j + 1]]))
    return out


# ---- new profiles out of whole sets: balance, shrink, merge, pool -------------------------------------------------------------
# A result lives where its table lived.  A profile that is still in HBM gets row j of a NEW batch (the tables of a batch are
# never written: copies and other rows share them, and _DeviceBatch._stats caches their summaries) and is re-pointed to it;
# a profile with host integer counts is uploaded with its group, transformed and downloaded.  Everything else -- non-integer
# counts, user mergers, shapes that do not match -- takes the method of the profile.
def _no_repeats(profiles, who):
    if len(set(id(p) for p in profiles)) != len(profiles):
        raise ValueError('%s: a profile appears twice' % who)


def _fresh_batch(ctx, n_tables, bins):
    """A new batch of ``n_tables`` tables of ``bins`` entries on ``ctx``, or None when the budget of live device tables or the
    allocation itself says no: the caller then takes the per-profile route."""
    nbytes = 8 * bins * n_tables
    try:
        return _DeviceBatch(ctx, nbytes, n_tables) if _may_stay(nbytes) else None
    except MemoryError:
        return None


def _batch_or_methods(ctx, n_tables, bins, method, *sides):
    """``_fresh_batch`` for a group -- or, when there is none, None after the per-profile route has been taken for every
    member: ``method(p)`` for the profiles of one side, ``method(p, o)`` for the pairs of two, with the counts of ``p``
    downloaded first (a method whose profile is still in HBM would come back to the set functions)."""
    batch = _fresh_batch(ctx, n_tables, bins)
    if batch is None:
        for each in zip(*sides):
            each[0].counts
            method(*each)
    return batch


def _repoint(targets, batch, length):
    """Row j of ``batch`` becomes the table of ``targets[j]``, a profile of k-mer length ``length`` (None: that row is nobody's)."""
    for j, p in enumerate(targets):
        if p is not None:
            p._counts, p._device, p.length = None, (batch, j, False), length


def _hand_out(ctx, ptr, bins, targets, in_place):
    """Downloads ``len(targets)`` tables of ``bins`` counts from ``ptr`` and hands row j to ``targets[j]`` (None: to nobody):
    written into the array the profile holds (``in_place``), or as its new counts -- rows of one array, as the tables of a
    downloaded batch are."""
    tables = np.empty((len(targets), bins), dtype=np.int64)
    ctx.d2h(tables, ptr)
    for j, p in enumerate(targets):
        if p is None:
            continue
        if in_place:
            p.counts[...] = tables[j]
        else:
            p.counts = tables[j]


@contextlib.contextmanager
def _result_tables(ctx, batch, nbytes, sync=False):
    """Where a set call writes ``nbytes`` of results: the rows of ``batch``, or without one an allocation that lives as long
    as the ``with`` (``sync``: work queued on it is waited for before it goes)."""
    if batch is not None:
        yield batch.ptr
        return
    out = ctx.alloc(nbytes)
    try:
        yield out
    finally:
        if sync:
            ctx.sync()
        ctx.free(out)


def _by_placement(profiles, usable=_set_counts):
    """Places of the profiles whose table is in HBM, of those with host integer counts, and of the rest."""
    resident, host, other = [], [], []
    for i, p in enumerate(profiles):
        (resident if p._device_counts() else host if usable(p) else other).append(i)
    return resident, host, other


def balance_profiles(profiles):
    """``for p in profiles: p.balance()`` with the integer profiles balanced as SETS (``kpal_balance_set_device``: one launch
    per group) under the rules of ``summaries``: lengths may be mixed, groups hold at most ``_RECORD_BATCH_BYTES``.  A profile
    that is still in HBM stays there, as a row of a new batch; host counts are written into the array the profile holds.  A
    profile that appears twice is a ``ValueError``."""
    profiles = list(profiles)
    _no_repeats(profiles, 'balance_profiles')
    resident, host, other = _by_placement(profiles)
    for i in other:
        profiles[i].balance()
    for group, ctx, ptr, k in _device_sets(profiles, resident):
        members = [profiles[i] for i in group]
        batch = _batch_or_methods(ctx, len(group), 4 ** k, lambda p: p.balance(), members)
        if batch is not None:
            ctx.balance_set_device(k, len(group), ptr, batch.ptr)
            _repoint(members, batch, k)
    for group, ctx, ptr, k in _device_sets(profiles, host):
        ctx.balance_set_device(k, len(group), ptr, ptr)      # (host counts are gathered into an allocation of the group's own)
        _hand_out(ctx, ptr, 4 ** k, [profiles[i] for i in group], in_place=True)


def _shrink_arguments(length, factor):
    if length <= factor:
        raise ValueError('Reduction factor should be smaller than k-mer size.')
    if factor < 0:    # the reference fails in range() with a float step (4 ** factor)
        raise TypeError("'float' object cannot be interpreted as an integer")


def shrink_profiles(profiles, factor=1):
    """``for p in profiles: p.shrink(factor)`` with the integer profiles shrunk as SETS (``kpal_shrink_set_device``: one
    launch per group) under the rules of ``balance_profiles``.  The errors of ``shrink`` are raised before any profile is
    changed."""
    profiles = list(profiles)
    _no_repeats(profiles, 'shrink_profiles')
    for p in profiles:
        _shrink_arguments(p.length, factor)
    if not isinstance(factor, (int, np.integer)) or factor == 0:
        for p in profiles:
            p.shrink(factor)
        return
    factor = int(factor)
    resident, host, other = _by_placement(profiles)
    for i in other:
        profiles[i].shrink(factor)
    for group, ctx, ptr, k in _device_sets(profiles, resident):
        members = [profiles[i] for i in group]
        batch = _batch_or_methods(ctx, len(group), 4 ** (k - factor), lambda p: p.shrink(factor), members)
        if batch is not None:
            ctx.shrink_set_device(k, factor, len(group), ptr, batch.ptr)
            _repoint(members, batch, k - factor)
    for group, ctx, ptr, k in _device_sets(profiles, host):
        members = [profiles[i] for i in group]
        with _result_tables(ctx, None, len(group) * 8 * 4 ** (k - factor)) as out:
            ctx.shrink_set_device(k, factor, len(group), ptr, out)
            _hand_out(ctx, out, 4 ** (k - factor), members, in_place=False)
        for p in members:
            p.length = k - factor


def merge_profiles(profiles, others, merger=metrics.mergers['sum']):
    """``for p, o in zip(profiles, others): p.merge(o, merger)`` for two lists of one length, the pairs of integer profiles
    of one k-mer length merged as SETS (``kpal_merge_device`` over all entries of a group: one launch) under the rules of
    ``balance_profiles``.  The result of a pair that is in HBM on both sides stays there.  User callables and pairs that do not
    match in shape or are no integer counts take ``Profile.merge``."""
    profiles, others = list(profiles), list(others)
    if len(profiles) != len(others):
        raise ValueError('merge_profiles: %d profiles, %d partners' % (len(profiles), len(others)))
    _no_repeats(profiles, 'merge_profiles')
    code = metrics.merger_code(merger)
    if code is None or set(id(p) for p in profiles) & set(id(o) for o in others):
        # (a partner that is itself merged into: the order of the loop is part of the result)
        for p, o in zip(profiles, others):
            p.merge(o, merger)
        return
    resident, host = [], []
    for i, (p, o) in enumerate(zip(profiles, others)):
        if not (_set_counts(p) and _set_counts(o) and p.length == o.length):
            p.merge(o, merger)
        else:
            (resident if p._device_counts() and o._device_counts() else host).append(i)
    for in_hbm, places in ((True, resident), (False, host)):
        for k, group in _groups(places, lambda i: profiles[i].length):
            bins = 4 ** k
            left, right = [profiles[i] for i in group], [others[i] for i in group]
            ctx = kdistlib._cross_context(left + right)
            batch = _batch_or_methods(ctx, len(group), bins, lambda p, o: p.merge(o, merger), left, right) if in_hbm else None
            if in_hbm and batch is None:
                continue
            with kdistlib._DeviceSet(ctx, left) as lset, kdistlib._DeviceSet(ctx, right) as rset:
                if in_hbm:
                    ctx.merge_device(len(group) * bins, lset.ptr, rset.ptr, code, batch.ptr)
                    _repoint(left, batch, k)
                else:
                    # one side at least was gathered into an allocation of the group's own: the result goes there
                    out = lset.ptr if lset.owned is not None else rset.ptr
                    assert lset.owned is not None or rset.owned is not None
                    ctx.merge_device(len(group) * bins, lset.ptr, rset.ptr, code, out)
                    _hand_out(ctx, out, bins, left, in_place=False)


def _smooth_counts(profile):
    """Whether ``profile`` can be one table of a smoothed set: in HBM, or int64 counts that can be written in place."""
    return bool(profile._device_counts()) or (kdistlib._plain_int64(profile._counts) and profile._counts.size == 4 ** profile.length)


def smooth_profiles(profiles, others, dist):
    """``for p, o in zip(profiles, others): dist.dynamic_smooth(p, o)`` for two lists of one length, the pairs of integer
    profiles of one k-mer length smoothed as SETS (``kpal_paired_smooth_device``: one pyramid of node sums and codes per table
    and one kernel that writes both smoothed sets, per group of at most ``_RECORD_BATCH_BYTES`` over both sides) under the rules
    of ``merge_profiles`` and ``balance_profiles``: a profile that is still in HBM stays there, as a row of a new batch; host
    int64 counts are written into the array the profile holds.  A profile that appears twice anywhere over both sides, and
    lists of unequal length, are a ``ValueError``.  A custom summary, a non-numeric threshold, counts that are no int64
    array, pairs of mixed k and a batch that is refused take ``dist.dynamic_smooth`` pair by pair."""
    profiles, others = list(profiles), list(others)
    if len(profiles) != len(others):
        raise ValueError('smooth_profiles: %d profiles, %d partners' % (len(profiles), len(others)))
    _no_repeats(profiles + others, 'smooth_profiles')
    code = metrics.summary_code(dist._function)
    places = []
    for i, (p, o) in enumerate(zip(profiles, others)):
        if code is None or not kdistlib._is_number(dist._threshold) or not (_smooth_counts(p) and _smooth_counts(o) and p.length == o.length):
            dist.dynamic_smooth(p, o)
        else:
            places.append(i)
    for k, group in _groups(places, lambda i: profiles[i].length, sides=2):
        n, bins = len(group), 4 ** k
        both = [profiles[i] for i in group] + [others[i] for i in group]
        in_hbm = [p if p._device_counts() else None for p in both]
        resident = 2 * n - in_hbm.count(None)
        ctx = kdistlib._cross_context(both)
        # the two smoothed sets, left first: rows of a new batch when a profile stays in HBM, else an allocation of the group's
        batch = _fresh_batch(ctx, 2 * n, bins) if resident else None
        if resident and batch is None:
            for p, o in zip(both[:n], both[n:]):      # (dynamic_smooth downloads what it needs: no set function behind it)
                dist.dynamic_smooth(p, o)
            continue
        with _result_tables(ctx, batch, 2 * n * 8 * bins, sync=True) as out, \
                kdistlib._DeviceSet(ctx, both[:n]) as lset, kdistlib._DeviceSet(ctx, both[n:]) as rset:
            ctx.paired_smooth_device(k, n, lset.ptr, rset.ptr, code, dist._threshold, out, out + n * 8 * bins)
            if resident < 2 * n:
                _hand_out(ctx, out, bins, [p if stays is None else None for p, stays in zip(both, in_hbm)], in_place=True)
        _repoint(in_hbm, batch, k)      # (row j of the batch, whatever the profile's place among the resident ones)


def pooled(profiles, name=None):
    """A new profile: the sum of the tables of ``profiles`` (int64 wrap, as repeated ``merge`` with the sum merger), integer
    profiles summed as SETS (``kpal_pool_set_device``: at most two launches per group of at most ``_RECORD_BATCH_BYTES``).
    The per-record or per-read profiles of a file add up to the file's profile: no k-mer spans two records.  When every
    profile is still in HBM, so is the result.  An empty list and mixed k-mer lengths are a ``ValueError``."""
    profiles = list(profiles)
    if not profiles:
        raise ValueError('pooled: no profiles')
    k = profiles[0].length
    if any(p.length != k for p in profiles):
        raise ValueError('pooled: profiles of different k-mer lengths')
    if not all(_set_counts(p) for p in profiles):
        total = np.array(profiles[0].counts)
        for p in profiles[1:]:
            total = metrics.mergers['sum'](total, p.counts)
        return Profile(total, name=name)
    bins = 4 ** k
    ctx = kdistlib._cross_context(profiles)
    batch = _fresh_batch(ctx, 1, bins) if all(p._device_counts() for p in profiles) else None
    with _result_tables(ctx, batch, 8 * bins) as out:
        per = _tables_per_group(k)
        for at in range(0, len(profiles), per):
            members = profiles[at:at + per]
            with kdistlib._DeviceSet(ctx, members) as dset:
                ctx.pool_set_device(len(members), bins, dset.ptr, out, accumulate=at > 0)
        if batch is not None:
            return Profile._from_device(batch, 0, k, name)
        total = np.empty(bins, dtype=np.int64)
        ctx.d2h(total, out)
        return Profile(total, name=name)


def _label_codes(labels):
    """The distinct ``labels`` in order of first appearance (None: no label) and, per place, the position of its label among
    them as an int64 array (-1: none)."""
    keys, where = [], {}
    codes = np.full(len(labels), -1, dtype=np.int64)
    for i, label in enumerate(labels):
        if label is None:
            continue
        if label not in where:
            where[label] = len(keys)
            keys.append(label)
        codes[i] = where[label]
    return keys, codes


def pooled_by(profiles, labels):
    """``(keys, pooled)``: the distinct ``labels`` (any hashables; None: the profile is in no group) in order of first
    appearance, and for ``keys[i]`` a new profile named ``str(keys[i])`` whose counts are those of ``pooled([p for p, l in
    zip(profiles, labels) if l == keys[i]])``, bit for bit -- the reads that fell to each member of a panel, the contigs of a
    bin, the windows of a record.  Integer profiles are summed as SETS by label (``kpal_pool_groups_device``: every table read
    once where it lies, one or two launches per group of at most ``_RECORD_BATCH_BYTES`` of tables, whatever the number of
    labels).  When every profile is still in HBM, so are the results, as the rows of one new batch.  When any profile is not
    integer counts the sums are those of the sum merger, label by label.  Lists of unequal length, an empty list and mixed
    k-mer lengths are a ``ValueError``; when every label is None the result is ``([], [])``."""
    profiles, labels = list(profiles), list(labels)
    if len(profiles) != len(labels):
        raise ValueError('pooled_by: %d profiles, %d labels' % (len(profiles), len(labels)))
    if not profiles:
        raise ValueError('pooled_by: no profiles')
    k = profiles[0].length
    if any(p.length != k for p in profiles):
        raise ValueError('pooled_by: profiles of different k-mer lengths')
    keys, codes = _label_codes(labels)
    if not keys:
        return [], []
    names = [str(key) for key in keys]
    if not all(_set_counts(p) for p in profiles):
        totals = [None] * len(keys)
        for p, g in zip(profiles, codes.tolist()):
            if g >= 0:
                totals[g] = np.array(p.counts) if totals[g] is None else metrics.mergers['sum'](totals[g], p.counts)
        return keys, [Profile(total, name=name) for total, name in zip(totals, names)]
    bins, n_groups = 4 ** k, len(keys)
    ctx = kdistlib._cross_context(profiles)
    batch = _fresh_batch(ctx, n_groups, bins) if all(p._device_counts() for p in profiles) else None
    with _result_tables(ctx, batch, n_groups * 8 * bins) as out:
        per = _tables_per_group(k)
        for at in range(0, len(profiles), per):
            members = profiles[at:at + per]
            with kdistlib._DeviceSet(ctx, members) as dset:
                ctx.pool_groups_device(len(members), bins, dset.ptr, codes[at:at + per], n_groups, out, accumulate=at > 0)
        if batch is not None:
            return keys, [Profile._from_device(batch, i, k, name) for i, name in enumerate(names)]
        totals = np.empty((n_groups, bins), dtype=np.int64)
        ctx.d2h(totals, out)
        return keys, [Profile(totals[i], name=name) for i, name in enumerate(names)]


class Profile(object):
    """A k-mer profile: ``counts[i]`` is the count of the k-mer whose 2-bit big-endian encoding
    (A=0, C=1, G=2, T=3) is ``i`` (kpal/klib.py:26-61).

    :arg counts: ``numpy.ndarray`` of length ``4**k`` (kept by reference, like the original).
    :arg str name: optional profile name (no ``/`` or ``.``).
    """

    _nucleotide_to_binary = {'A': 0, 'a': 0, 'C': 1, 'c': 1, 'G': 2, 'g': 2, 'T': 3, 't': 3}
    _binary_to_nucleotide = {0: 'A', 1: 'C', 2: 'G', 3: 'T'}

    def __init__(self, counts, name=None):
        self.length = int(math.log(len(counts), 4))
        self.counts = counts
        self.name = name

    # ---- counts that may still be in HBM -----------------------------------------------------
    # The reference's ``counts`` is a plain attribute holding a NumPy array that callers read AND write in place
    # (kpal/klib.py:58-61, kmer.py:137-146).  Here it is a property: a profile made by from_fasta_by_record starts with its table
    # in device memory only (``_device`` = (batch, index)); the first access downloads it, and from then on the host array is
    # the one truth -- the device copy is let go at that moment, because whoever holds the array may change it.  Distances,
    # matrices and the summaries of profiles nobody has looked at read the device copies (kdistlib.py, _device_stats).
    @classmethod
    def _from_device(cls, batch, index, length, name, private=False):
        """private: a copy() of a profile that is still in HBM -- it shares the (never written) device table, but when it is asked
        for counts it downloads its own array: the row of the batch's host array may be in someone's hands already."""
        p = cls.__new__(cls)
        p._counts, p._device = None, (batch, int(index), bool(private))
        p.length = int(length)
        p.name = name
        return p

    @property
    def counts(self):
        if self._counts is None and self._device is not None:
            batch, index, private = self._device
            if private:
                out = np.empty(4 ** self.length, dtype=np.int64)
                batch.ctx.d2h(out, batch.ptr + index * out.nbytes)
            else:
                out = batch.table(index)
            self._counts, self._device = out, None
        return self._counts

    @counts.setter
    def counts(self, value):
        self._counts, self._device = value, None

    # (pickling / copy.deepcopy of a profile whose table is still in HBM: the counts travel, the device handle does not)
    def __getstate__(self):
        return {'counts': self.counts, 'name': self._name, 'length': self.length}

    def __setstate__(self, state):
        self._counts, self._device = state['counts'], None
        self.length, self._name = state['length'], state['name']

    def _device_counts(self):
        """(context, device address) of the int64 table while it lives in HBM only, else None."""
        if self._counts is None and self._device is not None:
            batch, index, _ = self._device
            return batch.ctx, batch.ptr + index * 8 * 4 ** self.length
        return None

    # ---- constructors --------------------------------------------------------------------
    @classmethod
    def from_file(cls, handle, name=None):
        """Load from an open HDF5 k-mer file (kpal/klib.py:63-76)."""
        name = name or sorted(handle['profiles'].keys())[0]
        return cls(handle['profiles/' + name][:], name=name)

    @classmethod
    def from_file_old_format(cls, handle, name=None):
        """Load the pre-1.0 plaintext format: three header lines, then one count per line
        (kpal/klib.py:78-95)."""
        for _ in range(3):
            next(handle)
        return cls(np.loadtxt(handle, dtype='int64'), name=name)

    @classmethod
    def from_fasta(cls, handle, length, name=None):
        """One profile over all records of a FASTA handle (kpal/klib.py:97-112).

        The text is handed to the GPU in chunks of whole records; header removal, line joining
        and record separation happen on the device (``kpal_count_feed_fasta``), so there is no
        per-character or per-line Python work."""
        length = _kmer_length(length)
        ctx = _native.context()
        ctx.count_begin(length)
        plain = _plain_file(handle)
        if plain is not None:
            # an ordinary file: the library reads it itself -- parallel preads into pinned memory, H2D copy, flattening and
            # counting pipelined chunk by chunk; no byte of the text passes through Python
            ctx.count_feed_fasta_file(plain[0], plain[1], 0)
            handle.seek(0, os.SEEK_END)      # the handle has been consumed, as by the reference's SeqIO.parse loop
            return cls._finish_count(ctx, length, name)
        reader, _ = _byte_reader(handle)      # (a pipe or a decompressing wrapper under a text handle: its bytes, undecoded)
        carry = b''   # the unfinished last record of the previous chunk (small)
        while True:
            text = reader.read(_FASTA_CHUNK)
            if not text:
                break
            if not isinstance(text, bytes):
                text = text.encode('latin-1', 'replace')
            view = np.frombuffer(text, dtype=np.uint8)   # zero-copy: slices below are views
            begin = 0
            if carry:
                # finish the straddling record: up to the first record boundary of this chunk
                first = _first_boundary(text)
                if first < 0:
                    carry += text
                    continue
                ctx.count_feed_fasta(carry + text[:first + 1])
                carry = b''
                begin = first + 1
            # whole records of this chunk; the (possibly unfinished) last one is carried over
            cut = _last_boundary(text, begin)
            if cut >= begin:
                ctx.count_feed_fasta(view[begin:cut + 1])
                carry = text[cut + 1:]
            else:
                carry = text[begin:]
        if carry:
            ctx.count_feed_fasta(carry)
        return cls._finish_count(ctx, length, name)

    @classmethod
    def from_fastq(cls, handle, length, name=None, min_quality=None, quality_offset=33):
        """One profile over all reads of a four-line FASTQ handle (beyond the reference, which reads FASTA only).

        Every read is its own record (k-mers never span two reads); its sequence line is counted verbatim, as one sequence of
        ``from_sequences``.  With ``min_quality`` (0..93) a base whose Phred quality (quality byte - ``quality_offset``, 33 or
        64) is below it is masked: it breaks k-mer windows like any byte outside ``ACGT``.  Tokenising, validation and masking
        run on the device (``kpal_count_feed_fastq``); Python does not look for record boundaries.  A malformed record raises
        ``ValueError`` naming its 1-based number, and no profile is returned."""
        length = _read_arguments(length, min_quality, quality_offset)
        ctx = _native.context()
        ctx.count_begin(length)
        plain = _plain_file(handle)
        if plain is not None:
            # an ordinary file: the library reads it itself (parallel preads into pinned memory, as from_fasta)
            ctx.count_feed_fastq_file(plain[0], plain[1], 0, min_quality, quality_offset)
            handle.seek(0, os.SEEK_END)
            return cls._finish_count(ctx, length, name)
        reader, _ = _byte_reader(handle)
        while True:
            text = reader.read(_FASTA_CHUNK)   # raw pieces cut anywhere: the library carries the unfinished record
            if not text:
                break
            if not isinstance(text, bytes):
                text = text.encode('latin-1', 'replace')
            ctx.count_feed_fastq(text, min_quality, quality_offset)
        return cls._finish_count(ctx, length, name)

    @classmethod
    def from_fasta_by_record(cls, handle, length, prefix=None):
        """One profile per FASTA record, named by record (kpal/klib.py:114-133).

        The text is handed to the GPU in chunks of whole records: the records are found ON THE DEVICE
        (``kpal_fasta_records_begin``: the flattening kernels of ``from_fasta`` + an index of record starts and header
        lines) and counted in batches (``kpal_fasta_records_count``: one kernel launch and one table download for up to
        ``_RECORD_BATCH_BYTES`` of tables).  The host reads the HEADER lines only, for the names; there is no per-line or
        per-character Python work.  A k whose table alone exceeds that budget falls back to ``from_sequences`` per
        record."""
        yield from cls._by_record(handle, _kmer_length(length), prefix, 'from_fasta_by_record')

    @classmethod
    def from_fasta_by_window(cls, handle, length, window, step=None, prefix=None):
        """One profile per sliding window of every FASTA record (beyond the reference: a compositional scan).

        Coordinates are bases of the record as the device tokeniser flattens it (line ends and spaces dropped).  For a
        record of L bases window j covers bases ``[j * step, min(j * step + window, L))``: none for an empty record, one for
        ``L <= window``, else ``ceil((L - window) / step) + 1`` -- only the last one of a record can be truncated, and no
        window spans two records.  Its profile holds the k-mers lying wholly inside it: what
        ``from_sequences([seq[j * step:j * step + window]], length)`` counts, bit for bit.  ``step`` defaults to ``window``
        and must divide it; ``length <= window``.  Profiles come record-major, named ``<record name>:<start + 1>-<end>``
        (1-based, inclusive), the record name being the one ``from_fasta_by_record`` gives.

        The records are indexed as for ``from_fasta_by_record`` and counted by ``kpal_fasta_windows_count``: every base is
        tokenised and counted once, whatever ``window / step`` is, and the tables stay in HBM under the same budgets.  A k
        whose table alone exceeds the batch budget falls back to ``from_sequences`` per window."""
        length, window, step = _window_arguments(length, window, step)
        yield from cls._by_window(handle, length, window, step, prefix, 'from_fasta_by_window')

    @classmethod
    def from_fastq_by_record(cls, handle, length, prefix=None, min_quality=None, quality_offset=33):
        """One profile per read of a four-line FASTQ handle (beyond the reference, which reads FASTA only), named as
        ``from_fasta_by_record`` names records: ``prefix_`` + the first word of the title behind ``@``, or the read's 1-based
        number over the handle when the title has no word.  An empty read gives an all-zero profile.

        Reads are tokenised, validated and masked (``min_quality``, ``quality_offset``: as ``from_fastq``) by the device
        tokeniser of ``from_fastq``, which here also indexes them (``kpal_fastq_records_begin`` / ``_file_open``); batches of
        reads are then counted exactly as batches of FASTA records are, and their tables stay in HBM under the same budgets.
        The handle is taken piece by piece -- an ordinary file is read by the library itself.  A malformed read raises
        ``ValueError`` naming its 1-based number when the generator reaches its piece: the profiles of earlier pieces have
        been yielded, none of that piece is (a piece of an ordinary file is a staging buffer's worth behind the carried rest;
        of any other handle, what one ``read()`` returns behind it -- the rest that the last one leaves is a piece of its
        own, which the end of the handle ends).  A k whose table alone exceeds the batch budget falls back to
        ``from_sequences`` per read, on the reads as the device masks them."""
        length = _read_arguments(length, min_quality, quality_offset)
        yield from cls._by_record(handle, length, prefix, 'from_fastq_by_record', (min_quality, quality_offset))

    @classmethod
    def from_fastq_by_window(cls, handle, length, window, step=None, prefix=None, min_quality=None, quality_offset=33):
        """One profile per sliding window of every read of a four-line FASTQ handle: the windows of
        ``from_fasta_by_window`` over the read's sequence line, named ``<read>:<start + 1>-<end>`` with the read names of
        ``from_fastq_by_record``.  Coordinates count masked bases (``min_quality``): a masked base is a base that breaks
        k-mers.  Indexing, batching, residency and errors are those of ``from_fastq_by_record``."""
        length, window, step = _window_arguments(length, window, step)
        _read_arguments(length, min_quality, quality_offset)
        yield from cls._by_window(handle, length, window, step, prefix, 'from_fastq_by_window', (min_quality, quality_offset))

    @classmethod
    def _by_record(cls, handle, length, prefix, who, fastq=None):
        """One profile per record of a FASTA handle -- with ``fastq = (min_quality, quality_offset)``, per read of a FASTQ
        handle: the records indexed on the device (``_indexed_pieces``) and counted in batches of ``_tables_per_group``
        tables, or, when fewer than two tables make a batch, one by one."""
        prefix = prefix + '_' if prefix else ''
        per_batch = _tables_per_group(length)
        if per_batch < 2:
            for name, seq in _named_sequences(handle, prefix, fastq):
                yield cls.from_sequences([seq], length, name=name)
            return
        ctx = _native.context()
        for names, _, indexed in _indexed_pieces(ctx, handle, prefix, who, fastq):
            for first in range(0, len(names), per_batch):
                indexed()
                n = min(per_batch, len(names) - first)
                for profile in cls._counted_batch(ctx, length, n, names[first:first + n],
                                                  lambda ptr: ctx.fasta_records_count_device(length, first, n, ptr),
                                                  lambda: ctx.fasta_records_count(length, first, n)):
                    yield profile

    @classmethod
    def _by_window(cls, handle, length, window, step, prefix, who, fastq=None):
        """One profile per sliding window of every record (``fastq``: of every read) of a handle, batched or one by one as
        ``_by_record`` does."""
        prefix = prefix + '_' if prefix else ''
        per_batch = _tables_per_group(length)
        if per_batch < 2:
            for name, seq in _named_sequences(handle, prefix, fastq):
                for start in range(0, _window_count(len(seq), window, step) * step, step):
                    end = min(start + window, len(seq))
                    yield cls.from_sequences([seq[start:end]], length, name='%s:%d-%d' % (name, start + 1, end))
            return
        ctx = _native.context()
        for names, bases, indexed in _indexed_pieces(ctx, handle, prefix, who, fastq):
            n_windows, first_window = ctx.fasta_windows_layout(window, step)
            for first in range(0, n_windows, per_batch):
                indexed()
                n = min(per_batch, n_windows - first)
                # names of windows [first, first + n): their records, their numbers inside them
                numbers = np.arange(first, first + n, dtype=np.uint64)
                records = np.searchsorted(first_window, numbers, side='right') - 1
                starts = (numbers - first_window[records]) * np.uint64(step)
                ends = np.minimum(starts + np.uint64(window), bases[records])
                window_names = ['%s:%d-%d' % (names[r], a + 1, b) for r, a, b in zip(records.tolist(), starts.tolist(), ends.tolist())]
                for profile in cls._counted_batch(ctx, length, n, window_names,
                                                  lambda ptr: ctx.fasta_windows_count_device(length, window, step, first, n, ptr),
                                                  lambda: ctx.fasta_windows_count(length, window, step, first, n)):
                    yield profile

    @classmethod
    def _finish_count(cls, ctx, length, name):
        """The finished count of ``ctx`` as a profile.  The table stays in HBM -- copied device-to-device out of the context's
        count table, which the next count reuses, into an allocation of its own -- until something asks for ``counts``
        (`kpal count` saving it: the one download it always was; a distance between two freshly counted profiles: none at all);
        past the budget of live device tables it is downloaded at once."""
        nbytes = 8 * 4 ** length
        if _may_stay(nbytes):
            ctx.count_finish(to_host=False)
            table, _ = ctx.count_table()
            batch = _DeviceBatch(ctx, nbytes, 1)
            ctx.d2d(batch.ptr, table, nbytes)
            ctx.sync()
            return cls._from_device(batch, 0, length, name)
        return cls(ctx.count_finish(), name=name)

    @classmethod
    def _counted_batch(cls, ctx, length, n, names, count_device, count_host):
        """The ``n`` profiles ``names`` of one batch of records or windows of the text the context has indexed.  Their tables
        stay in HBM (one allocation per batch, filled by ``count_device(address)``) while the budget of live device tables
        allows; else they are downloaded at once (``count_host()``: the n tables)."""
        nbytes = n * 8 * 4 ** length
        if _may_stay(nbytes):
            batch = _DeviceBatch(ctx, nbytes, n)
            count_device(batch.ptr)
            return [cls._from_device(batch, j, length, names[j]) for j in range(n)]
        tables = count_host()
        return [cls(tables[j], name=names[j]) for j in range(n)]

    @classmethod
    def from_sequences(cls, sequences, length, name=None):
        """Count all k-mers of every sequence (kpal/klib.py:135-170) on the GPU.

        Windows never span two sequences or a character outside ``AaCcGgTt``.
        """
        length = _kmer_length(length)
        ctx = _native.context()
        ctx.count_begin(length)
        if _kpal_gather is not None:
            _gather_feed(ctx, sequences)
            return cls._finish_count(ctx, length, name)
        it = iter(sequences)
        pending = []
        size = 0
        while True:
            block = list(itertools.islice(it, _JOIN_BLOCK))
            if not block:
                break
            data = _join_block(block)
            pending.append(data)
            size += len(data) + 1
            if size >= _FEED_BYTES:
                # feeds are independent: a window never spans two feeds, nor two sequences
                ctx.count_feed(pending[0] if len(pending) == 1 else b'\n'.join(pending))
                pending, size = [], 0
        if pending:
            ctx.count_feed(pending[0] if len(pending) == 1 else b'\n'.join(pending))
        return cls._finish_count(ctx, length, name)

    # ---- properties ------------------------------------------------------------------------
    @property
    def name(self):
        return self._name

    @name.setter
    def name(self, name):
        if name and ('/' in name or '.' in name):
            raise ValueError('Profile name may not contain / or . characters.')
        self._name = name

    @property
    def number(self):
        """Number of possible k-mers of this length."""
        return 4 ** self.length if self._counts is None and self._device is not None else len(self.counts)

    @property
    def non_zero(self):
        return int(self._device_stats().non_zero) if self._device_counts() else np.count_nonzero(self.counts)

    @property
    def total(self):
        return np.int64(self._device_stats().total) if self._device_counts() else self.counts.sum()

    def _device_stats(self):
        """``kpal_stats`` over integer counts (one upload, two streaming passes and a radix select), or None when the counts are
        not integers (scaled profiles keep NumPy's float formulation).  A table that is still in HBM is summarised there, with all
        tables of its batch at once (``_DeviceBatch.stats``); once its counts have been handed out, the host array is summarised
        anew every time -- whoever holds it may have changed it."""
        if self._device_counts():
            batch, index, _ = self._device
            return batch.stats(index)
        c = np.asanyarray(self.counts)
        if c.dtype.kind not in 'iub' or c.ndim != 1 or c.size == 0:
            return None
        return _native.context().stats(c)

    @property
    def mean(self):
        """Mean count (kpal/klib.py:206-211)."""
        s = self._device_stats()
        return self.counts.mean() if s is None else np.float64(s.mean)

    @property
    def median(self):
        """Median count (kpal/klib.py:213-218), exact: radix select on the device."""
        s = self._device_stats()
        return np.median(self.counts) if s is None else np.float64(s.median)

    @property
    def std(self):
        """Population standard deviation of the counts (kpal/klib.py:220-225)."""
        s = self._device_stats()
        return self.counts.std() if s is None else np.float64(s.std)

    def summary(self):
        """``total``, ``non_zero``, ``mean``, ``median`` and ``std`` at once: one ``kpal_stats`` call for integer
        counts (the attributes ``save`` writes and ``kpal info`` prints), the properties otherwise."""
        s = self._device_stats()
        if s is None:
            return dict((key, getattr(self, key)) for key in ('total', 'non_zero', 'mean', 'median', 'std'))
        return _summary_dict(s)

    # ---- I/O -------------------------------------------------------------------------------
    def save(self, handle, name=None):
        """Write to an open HDF5 k-mer file, dataset ``profiles/<name>`` with the summary
        attributes of format 1.0.0 (kpal/klib.py:227-256, doc/fileformat.rst:23-46)."""
        if name and ('/' in name or '.' in name):
            raise ValueError('Profile name may not contain / or . characters.')
        name = name or self.name or next(str(n) for n in itertools.count(1) if str(n) not in handle['profiles'])
        attrs = self.summary()        # before ``counts`` is touched: a table still in HBM is summarised there, with its whole batch
        dataset = handle.create_dataset('profiles/' + name, data=self.counts, dtype='int64', compression='gzip')
        dataset.attrs['length'] = self.length
        for key in ('total', 'non_zero', 'mean', 'median', 'std'):
            dataset.attrs[key] = attrs[key]
        handle.flush()
        return name

    def copy(self):
        """Deep copy (kpal/klib.py:258-267).  (A table that is still in HBM is never written: the copy shares it until either
        profile is asked for its counts.)"""
        if self._counts is None and self._device is not None:
            return type(self)._from_device(self._device[0], self._device[1], self.length, self.name, private=True)
        return type(self)(self.counts.copy(), name=self.name)

    def merge(self, profile, merger=metrics.mergers['sum']):
        """Merge another profile into this one with a vectorised merger (kpal/klib.py:269-283)."""
        code = metrics.merger_code(merger)
        if (code is not None and profile is not self and self._device_counts() and profile._device_counts()
                and self.length == profile.length):
            merge_profiles([self], [profile], merger)             # both tables in HBM: a set of one pair, the result stays there
            return
        l, r = np.asanyarray(self.counts), np.asanyarray(profile.counts)
        if code is not None and l.dtype.kind in 'iub' and r.dtype.kind in 'iub' and l.shape == r.shape and l.ndim == 1:
            self.counts = _native.context().merge(l, r, code)     # built-in merger: one HIP kernel
        else:
            self.counts = merger(self.counts, profile.counts)     # user callable / float profiles: as the reference

    # ---- hot path: balance / split ------------------------------------------------------------
    def _rc_index(self):
        """rc(i) for every i (vectorised form of reverse_complement, kpal/klib.py:394-412)."""
        k = self.length
        i = np.arange(4 ** k, dtype=np.uint64)
        rc = np.zeros_like(i)
        comp = ~i
        for d in range(k):
            rc |= ((comp >> np.uint64(2 * d)) & np.uint64(3)) << np.uint64(2 * (k - 1 - d))
        return rc.astype(np.int64)

    def balance(self):
        """``counts[i] += counts[rc(i)]`` for every k-mer, palindromes doubled, in place
        (kpal/klib.py:285-298) -- one HIP kernel for integer counts.  Non-integer counts (a scaled
        profile) cannot enter the integer kernel: they take the same sums as one NumPy expression, in
        the dtype of ``counts`` like the reference's loop.  A table that is still in HBM is balanced there, as a set of one
        (``balance_profiles``), and stays there."""
        if self._device_counts():
            balance_profiles([self])
            return
        c = np.asanyarray(self.counts)
        if c.dtype.kind not in 'iub':
            c[...] = c + c[self._rc_index()]
            return
        if c.dtype == np.int64 and c.flags['C_CONTIGUOUS'] and c.flags['WRITEABLE']:
            _native.context().balance_inplace(c, self.length)
        else:
            tmp = np.ascontiguousarray(c, dtype=np.int64).copy()
            _native.context().balance_inplace(tmp, self.length)
            self.counts[...] = tmp

    def split(self):
        """Doubled forward / reverse-complement halves in ascending k-mer order
        (kpal/klib.py:300-327) -- ``kpal_split``; NumPy for non-integer counts."""
        c = np.asanyarray(self.counts)
        if c.dtype.kind not in 'iub':
            rc = self._rc_index()
            i = np.arange(c.size)
            lower, pal = i < rc, i == rc
            keep = lower | pal
            forward = np.where(pal, c, c * 2)[keep]
            reverse = np.where(pal, c, c[rc] * 2)[keep]
            return forward, reverse
        return _native.context().split(c, self.length)

    # ---- container helpers ----------------------------------------------------------------------
    def shrink(self, factor=1):
        """Reduce k by ``factor`` by summing groups of ``4**factor`` bins (kpal/klib.py:329-352)."""
        _shrink_arguments(self.length, factor)
        if self._device_counts() and isinstance(factor, (int, np.integer)) and factor > 0:
            shrink_profiles([self], factor)                       # still in HBM: a set of one, the result stays there
            return
        c = np.asanyarray(self.counts)
        if factor == 0:   # groups of one: a fresh int64 copy
            self.counts = np.array(c, dtype='int64')
            return
        if c.dtype.kind in 'iub':
            self.counts = _native.context().shrink(c, self.length, factor)
        else:   # the reference builds int64 counts from whatever it holds (np.fromiter(..., dtype='int64'))
            self.counts = c.reshape(-1, 4 ** factor).sum(axis=1).astype('int64')
        self.length -= factor

    def shuffle(self):
        """Randomise the profile in place (kpal/klib.py:354-358)."""
        np.random.shuffle(self.counts)

    def dna_to_binary(self, sequence):
        """DNA string -> integer; ``KeyError`` on a non-ACGT character (kpal/klib.py:360-375)."""
        result = 0
        for nucleotide in sequence:
            result = (result << 2) | self._nucleotide_to_binary[nucleotide]
        return result

    def binary_to_dna(self, number):
        """Integer -> DNA string of this profile's k (kpal/klib.py:377-392)."""
        letters = []
        for _ in range(self.length):
            letters.append(self._binary_to_nucleotide[number & 3])
            number >>= 2
        return ''.join(reversed(letters))

    def reverse_complement(self, number):
        """Reverse complement in the binary representation (kpal/klib.py:394-412)."""
        return _native.reverse_complement(number, self.length)

    def _ratios_matrix(self):
        """All relative frequencies count[i]/count[j]/total, -1.0 where count[j] is 0
        (kpal/klib.py:414-437)."""
        c = np.asarray(self.counts, dtype='float64')
        total = float(self.total)
        with np.errstate(divide='ignore', invalid='ignore'):
            m = (c[:, None] / c[None, :]) / total
        m[:, c == 0] = -1.0
        return m.tolist()

    def _freq_diff_matrix(self):
        """All |count[i]-count[j]|/total, 0 where count[j] is 0 (kpal/klib.py:439-456)."""
        c = np.asarray(self.counts)
        total = self.total
        m = np.abs(c[:, None] - c[None, :]) / total
        out = m.tolist()
        for j in np.nonzero(c == 0)[0]:
            for row in out:
                row[j] = 0
        return out

    def print_counts(self):
        """Print ``<k-mer> <count>`` lines (kpal/klib.py:458-463)."""
        for i in range(self.number):
            print(self.binary_to_dna(i), self.counts[i])

    def _print_ratios(self, ratios):
        """Print a ratios matrix (kpal/klib.py:465-487)."""
        print((self.length + 1) * ' ', end=' ')
        for i in range(self.number):
            print(self.binary_to_dna(i), end='   ')
        print()
        for i in range(self.number):
            print(self.binary_to_dna(i), end=' ')
            for j in range(self.number):
                print('{{0:.{0}f}}'.format(self.length).format(ratios[i][j]), end=' ')
            print()
