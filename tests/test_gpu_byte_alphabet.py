"""Every byte value through the base classifiers and the text readers, on the GPU, bit for bit against the reference's rule.

The decisions "is this byte one of ACGTacgt, and which code does it get" and "does the reader drop, keep or mask this byte, or
end a line at it" are made in several independent places: classify4 / encode16 (kpal_device.hpp, under every counting
pipeline), the scalar classifier of window_trim_kernel, fa_classify / fa_is_soft_space / fa_trailing with the host's
tail_trailing, fq_classify with the quality mask.  tests/alphabet_cases.py builds texts that show all 256 byte values to each of
them at every place of the structures they work in (16-byte chunks, the dword pairs of the flag gather, the 1 KiB wave-step
seam -- also where one wave walks several steps and carries its last chunk across it --, the straddle zone behind a trimmed
window, cuts of the chunked file reader inside runs of blanks);
tests/test_alphabet_cases_host.py proves those preconditions on the CPU.  Expected values are the plain restatement of
kpal/klib.py:152-168 (``alphabet_cases.reference_count``), the Biopython-rule tokeniser (``seqio_records``) and the FASTQ rules
of tests/fastq_cases.py.  Integer work: no tolerance anywhere.

k >= 14 is left out: a table of 2 to 32 GiB cannot be downloaded and compared in a test of a few seconds; the full-size tests of
tests/test_gpu_count.py stay the cover there (the classifier is the same template at every k).

profiles/byte_alphabet/README.md lists the one-line mutants of the kernels these tests were held against.
Run on the GPU box: pytest -m gpu."""
import io
import os

import numpy as np
import pytest

import alphabet_cases as ac
from fastq_cases import flat_of

pytestmark = pytest.mark.gpu

RETIRED = os.environ.get('KPAL_TEST_RETIRED', '0') not in ('', '0')      # (as tests/test_gpu_count.py: the round-1 'partition')
QUALITY_ERROR = 'malformed FASTQ record %d: a quality byte outside the range of the quality offset'


def strategies(k):
    if k <= 7:
        return ['lds_direct', 'global_atomic', 'auto']
    if k <= 12:
        return ['global_atomic', 'partition_chunked', 'partition_quads', 'auto'] + (['partition'] if RETIRED else [])
    return ['partition2', 'partition2_quads', 'global_atomic']


def flat_texts(k):
    # k = 13: a 512 MiB table per count -- the two texts that walk the chunk and the seam
    return ('every_byte_every_slot', 'seam_walk') if k == 13 else tuple(ac.FLAT_TEXTS)


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


# ----------------------------------------------------------------------------------------------------------------------------
# counting
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', (1, 2, 3, 4, 7, 8, 11, 12, 13))
def test_flat_texts_on_every_pipeline(ctx, k):
    """Explicit strategies are taken as they are (only AUTO is re-planned for small feeds), so these small texts do run the
    partition and quad pipelines: kpal_count_last_plan says so."""
    for name in flat_texts(k):
        text = ac.flat_text(name)
        want = ac.flat_reference(name, k)
        for strategy in strategies(k):
            got = ctx.count_bytes(k, text, strategy)
            if strategy != 'auto':
                assert ctx.count_last_plan()[0] == strategy, (name, k, strategy)
            np.testing.assert_array_equal(got, want, err_msg='%s k=%d %s' % (name, k, strategy))
            del got


@pytest.mark.parametrize('k', (1, 2, 3, 4, 7, 8, 11, 12, 13))
def test_seam_walk_fed_from_device_offsets(ctx, k):
    """seam_walk from a device buffer at byte offsets 0 and 9 of an aligned allocation: the first fed byte's place in its chunk
    (Span::lo) moves the wave-step seams against the text; at 9 the bad bytes stand -8 .. +26 bytes from a seam."""
    text = np.frombuffer(ac.flat_text('seam_walk'), dtype=np.uint8)
    want = ac.flat_reference('seam_walk', k)
    d = ctx.alloc(text.size + 64)
    try:
        assert d % 16 == 0
        for off in (0, 9):
            ctx.h2d(d + off, text)
            for strategy in strategies(k):
                ctx.count_begin(k, strategy)
                ctx.count_feed_device(d + off, text.size)
                if strategy != 'auto':
                    assert ctx.count_last_plan()[0] == strategy, (k, strategy)
                got = ctx.count_finish()
                np.testing.assert_array_equal(got, want, err_msg='offset %d k=%d %s' % (off, k, strategy))
                del got
    finally:
        ctx.free(d)


@pytest.fixture(scope='module')
def cu():
    """Compute units of the part: the device property kpal_ctx sizes its grids with."""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize('k', (2, 7, 11))
def test_long_seam_walk_where_a_wave_walks_several_steps(ctx, cu, k):
    """9 MiB: more wave-steps than one launch of count_global_atomic (32 waves a CU) or count_lds_direct (16) has waves, so
    every wave walks two steps or more and the bad flags of lane 63 reach lane 0 through `carry` -- in the 70-seam text every
    wave loads the chunk to its left afresh."""
    assert ac.LONG_STEPS > 32 * cu, 'a wave of count_global_atomic walks one step: the text is too short for this part'
    text = ac.flat_text('seam_walk_long')
    want = ac.reference_count_numpy(text, k)
    for strategy in strategies(k):
        got = ctx.count_bytes(k, text, strategy)
        if strategy != 'auto':
            assert ctx.count_last_plan()[0] == strategy, (k, strategy)
        np.testing.assert_array_equal(got, want, err_msg='k=%d %s' % (k, strategy))


# ----------------------------------------------------------------------------------------------------------------------------
# FASTA
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def fasta_case():
    text = ac.fasta_case_text()
    records = ac.seqio_records(text)
    tables = [ac.reference_count([seq.encode('latin-1')], 4) for _, seq in records]
    return text, records, tables


def test_fasta_flatten_every_value_at_every_place(ctx, fasta_case):
    text, records, _ = fasta_case
    got = ctx.fasta_flatten(text.encode('latin-1'))
    want = ac.expected_flat(text)
    if got != want:                                  # name the first record that differs
        got_records = got.split(b'\n')[1:]
        for (name, seq), g in zip(records, got_records):
            assert g == seq.encode('latin-1'), name
        assert len(got_records) == len(records)
    assert got == want


def test_from_fasta_and_by_record_on_the_cases(ctx, fasta_case):
    from kpal_amd import klib
    text, records, tables = fasta_case
    whole = klib.Profile.from_fasta(io.StringIO(text), 4)
    np.testing.assert_array_equal(whole.counts, sum(tables))
    profiles = list(klib.Profile.from_fasta_by_record(io.StringIO(text), 4))
    assert len(profiles) == len(records)
    for i, (p, (name, _), want) in enumerate(zip(profiles, records, tables)):
        assert p.name == (name or str(i + 1))
        np.testing.assert_array_equal(p.counts, want, err_msg='record %d %s' % (i, name))
    from_bytes = list(klib.Profile.from_fasta_by_record(io.BytesIO(text.encode('latin-1')), 4))
    assert [p.name for p in from_bytes] == [p.name for p in profiles]
    for p, (name, _), want in zip(from_bytes, records, tables):
        np.testing.assert_array_equal(p.counts, want, err_msg=name)


def test_fasta_cases_from_a_file_in_small_chunks(fasta_case, tmp_path, monkeypatch):
    """The same text through the chunked readers with the chunk forced small (KPAL_FASTA_CHUNK, read when a context is
    created, as in test_gpu_fasta.test_chunk_seams_everywhere): the chunks are cut every `chunk` bytes, and the sizes taken put
    cuts inside a run of soft blanks that trails its line (tail_trailing true) and inside one that a base follows (false)."""
    from kpal_amd import _native
    text, records, tables = fasta_case
    raw = text.encode('latin-1')
    path = tmp_path / 'cases.fa'
    path.write_bytes(raw)
    want_flat, want = ac.expected_flat(text), sum(tables)
    seen_trailing = seen_followed = 0
    for chunk in ac.FASTA_CHUNKS:
        trailing, followed = ac.blank_run_cuts(text, chunk)
        seen_trailing += len(trailing)
        seen_followed += len(followed)
        monkeypatch.setenv('KPAL_FASTA_CHUNK', str(chunk))
        c = _native.Context(_native.default_device())
        monkeypatch.delenv('KPAL_FASTA_CHUNK')
        try:
            assert c.fasta_flatten(raw) == want_flat, chunk
            c.count_begin(4)
            c.count_feed_fasta_file(str(path))
            np.testing.assert_array_equal(c.count_finish(), want, err_msg='file, chunk %d' % chunk)
            c.count_begin(4)
            c.count_feed_fasta(raw)
            np.testing.assert_array_equal(c.count_finish(), want, err_msg='memory, chunk %d' % chunk)
        finally:
            c.close()
    assert seen_trailing > 0 and seen_followed > 0


# ----------------------------------------------------------------------------------------------------------------------------
# FASTQ
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('offset,min_quality', [(o, m) for o in ac.QUALITY_OFFSETS for m in ac.min_qualities(o)])
def test_every_quality_byte(ctx, offset, min_quality):
    """One text per quality byte value: without a malformed byte the masked stream and its table, with one the error that names
    the first such record and the kind -- from kpal_fastq_flatten and from kpal_count_feed_fastq."""
    cases = ac.quality_cases(offset, min_quality)
    by_q = dict((c.q, c) for c in cases)
    for name, q in ac.quality_boundaries(offset, min_quality).items():
        assert q in by_q, name
    for c in cases:
        if c.malformed is None:
            assert ctx.fastq_flatten(c.text, min_quality, offset) == flat_of(c.reads), c.label
            ctx.count_begin(2)
            ctx.count_feed_fastq(c.text, min_quality, offset)
            np.testing.assert_array_equal(ctx.count_finish(), ac.reference_count(c.reads, 2), err_msg=c.label)
        else:
            with pytest.raises(ValueError) as err:
                ctx.fastq_flatten(c.text, min_quality, offset)
            assert QUALITY_ERROR % c.malformed in str(err.value), (c.label, str(err.value))
            with pytest.raises(ValueError) as err:
                ctx.count_begin(2)
                ctx.count_feed_fastq(c.text, min_quality, offset)
                ctx.count_finish()
            assert QUALITY_ERROR % c.malformed in str(err.value), (c.label, str(err.value))
    # a count abandoned at an error and begun again holds only the new text
    good = by_q[126]
    ctx.count_begin(2)
    ctx.count_feed_fastq(good.text, min_quality, offset)
    np.testing.assert_array_equal(ctx.count_finish(), ac.reference_count(good.reads, 2))


def test_fastq_line_of_every_byte_value(ctx):
    """Mask off: a sequence line is taken verbatim, whatever its bytes, and counts like any sequence."""
    from kpal_amd import klib
    text, line = ac.all_bytes_fastq()
    assert ctx.fastq_flatten(text) == b'\n' + line
    for k in (1, 3, 4):
        want = ac.reference_count([line], k)
        ctx.count_begin(k)
        ctx.count_feed_fastq(text)
        np.testing.assert_array_equal(ctx.count_finish(), want, err_msg='k=%d' % k)
        np.testing.assert_array_equal(klib.Profile.from_fastq(io.BytesIO(text), k).counts, want, err_msg='from_fastq k=%d' % k)
    (by_record,) = list(klib.Profile.from_fastq_by_record(io.BytesIO(text), 3))
    np.testing.assert_array_equal(by_record.counts, ac.reference_count([line], 3))


# ----------------------------------------------------------------------------------------------------------------------------
# windows
# ----------------------------------------------------------------------------------------------------------------------------
def hold_windows(profiles, seq, k, window, step):
    spans = ac.window_spans(len(seq), window, step)
    assert len(profiles) == len(spans)
    lowest = min(int(p.counts.min()) for p in profiles)
    # the signature of the trim's classifier disagreeing with the counters': it takes back a k-mer that nobody counted
    assert lowest >= 0, 'a negative bin'
    for p, (start, end) in zip(profiles, spans):
        bins, counts = ac.reference_sparse([seq[start:end]], k)
        got = p.counts
        found = np.flatnonzero(got)                 # (the whole table: its non-zero bins and their values)
        np.testing.assert_array_equal(found, bins, err_msg='window %d-%d' % (start, end))
        np.testing.assert_array_equal(got[found], counts, err_msg='window %d-%d' % (start, end))


@pytest.mark.parametrize('k,window,step', ac.WINDOW_TRIPLES)
def test_fasta_windows_over_every_value(ctx, k, window, step):
    from kpal_amd import klib
    text, seq = ac.window_fasta(step)
    profiles = list(klib.Profile.from_fasta_by_window(io.BytesIO(text), k, window, step))
    hold_windows(profiles, seq, k, window, step)


@pytest.mark.parametrize('k,window,step', ac.WINDOW_TRIPLES)
def test_fastq_windows_over_every_value(ctx, k, window, step):
    from kpal_amd import klib
    text, read = ac.window_fastq(step)
    profiles = list(klib.Profile.from_fastq_by_window(io.BytesIO(text), k, window, step))
    hold_windows(profiles, read, k, window, step)
