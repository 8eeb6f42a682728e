"""FASTQ ingest on the device (kpal_count_feed_fastq / _file / kpal_fastq_flatten, Profile.from_fastq, ``kpal count --fastq``)
against an independent restatement of the format rules (tests/fastq_cases.py: four-line records, CR before LF dropped, roles by line index mod 4,
length check, optional quality mask, trailing empty lines ignored, malformed records refused) and the oracle's counts.  The
reference reads FASTA only, so the rules are the specification.  Run on the GPU box: pytest -m gpu."""
import gzip
import io
import os
import random

import numpy as np
import pytest

import memh5
import oracle
from fastq_cases import Malformed, Ragged, fastq_reads, flat_of, random_fastq

pytestmark = pytest.mark.gpu

KS = (1, 3, 8, 12, 13)


def texts_for(seed):
    rnd = random.Random(seed)
    base = random_fastq(rnd, 60)
    return [
        base,
        random_fastq(rnd, 40, crlf=True),
        base + b'@last\nACGTN\n+\nIIII#',                    # the last line without its '\n'
        base + b'\n\n\r\n\n\n',                              # empty lines at the very end
        b'@e\n\n+\n\n@f\n\n+\n',                             # empty reads; the last quality line empty and unterminated
        b'@a\nACGT\n+\n@+@+\n@b\nTTTT\n+b\n++++\n',           # quality lines that begin with '@' / '+'
        b'',
    ]


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


def test_flatten_matches_restatement(monkeypatch):
    """kpal_fastq_flatten == the restatement, with the staging chunk at 16, 17, 257, 5000 bytes and the default: seams inside
    every line role and inside '\\r\\n'; with and without the mask."""
    from kpal_amd import _native
    texts = texts_for(5)
    for chunk in (16, 17, 257, 5000, None):
        if chunk:
            monkeypatch.setenv('KPAL_FASTA_CHUNK', str(chunk))
        c = _native.Context(_native.default_device())
        monkeypatch.delenv('KPAL_FASTA_CHUNK', raising=False)
        for t, text in enumerate(texts):
            for mq in (None, 20):
                want = flat_of(fastq_reads(text, mq))
                assert c.fastq_flatten(text, min_quality=mq) == want, (chunk, t, mq)


def test_counts_every_path(tmp_path, ctx):
    """from_fastq == oracle.from_sequences(reads) for k in 1, 3, 8, 12, 13 (13: the two-level pipeline) through the file path,
    io.BytesIO, gzip.open in text and binary mode, and ragged pieces fed one after another (records cut between feeds)."""
    from kpal_amd import klib
    rnd = random.Random(11)
    text = random_fastq(rnd, 400) + random_fastq(rnd, 100, crlf=True)
    reads = fastq_reads(text)
    path = tmp_path / 'r.fq'
    path.write_bytes(text)
    gz = tmp_path / 'r.fq.gz'
    with gzip.open(str(gz), 'wb') as fh:
        fh.write(text)
    for k in KS:
        want = oracle.from_sequences(reads, k)
        with open(str(path)) as fh:
            np.testing.assert_array_equal(klib.Profile.from_fastq(fh, k).counts, want, err_msg='file k=%d' % k)
        with open(str(path), 'rb') as fh:
            np.testing.assert_array_equal(klib.Profile.from_fastq(fh, k).counts, want, err_msg='binary file k=%d' % k)
        np.testing.assert_array_equal(klib.Profile.from_fastq(io.BytesIO(text), k).counts, want, err_msg='BytesIO k=%d' % k)
        for mode in ('rt', 'rb'):
            with gzip.open(str(gz), mode) as fh:
                np.testing.assert_array_equal(klib.Profile.from_fastq(fh, k).counts, want, err_msg='gzip %s k=%d' % (mode, k))
        np.testing.assert_array_equal(klib.Profile.from_fastq(Ragged(text, k), k).counts, want, err_msg='ragged k=%d' % k)
    # the C-ABI directly: feeds cut at every few bytes, the count ended by kpal_count_finish
    ctx.count_begin(8)
    for at in range(0, len(text), 97):
        ctx.count_feed_fastq(text[at:at + 97])
    np.testing.assert_array_equal(ctx.count_finish(8), oracle.from_sequences(reads, 8))
    # an empty text is the all-zero profile
    assert not klib.Profile.from_fastq(io.BytesIO(b''), 5).counts.any()
    assert not klib.Profile.from_fastq(io.BytesIO(b'\n\n'), 5).counts.any()


def test_quality_mask(tmp_path):
    """min_quality 0, 20, 41 at offset 33 and 20 at offset 64 against the restatement, file and buffer paths."""
    from kpal_amd import klib
    rnd = random.Random(23)
    t33 = random_fastq(rnd, 300, noise=False)
    t64 = random_fastq(rnd, 300, offset=64, noise=False)
    for text, offset, mqs in ((t33, 33, (0, 20, 41)), (t64, 64, (20,))):
        path = tmp_path / ('q%d.fq' % offset)
        path.write_bytes(text)
        for mq in mqs:
            reads = fastq_reads(text, mq, offset)
            for k in (3, 8):
                want = oracle.from_sequences(reads, k)
                with open(str(path), 'rb') as fh:
                    got = klib.Profile.from_fastq(fh, k, min_quality=mq, quality_offset=offset).counts
                np.testing.assert_array_equal(got, want, err_msg='file offset %d q %d k %d' % (offset, mq, k))
                got = klib.Profile.from_fastq(Ragged(text, mq), k, min_quality=mq, quality_offset=offset).counts
                np.testing.assert_array_equal(got, want, err_msg='ragged offset %d q %d k %d' % (offset, mq, k))
        assert fastq_reads(text, 41 if offset == 33 else 20, offset) != fastq_reads(text)   # the mask did mask something


GOOD = b'@r1\nACGTACGT\n+\nIIIIIIII\n@r2\nGGCCTTAA\n+r2\n!!!!IIII\n'
BAD = {
    'missing @': (GOOD + b'r3\nACGT\n+\nIIII\n', 3, None),
    'missing +': (GOOD + b'@r3\nACGT\n-\nIIII\n', 3, None),
    'length': (GOOD + b'@r3\nACGT\n+\nIII\n' + GOOD, 3, None),
    'cut off': (GOOD + b'@r3\nACGT\n', 3, None),
    'cut off title only': (GOOD + b'@r3', 3, None),
    'quality byte': (GOOD + b'@r3\nACGT\n+\nII I\n', 3, 20),
    'quality above ~': (GOOD + b'@r3\nACGT\n+\nII\x7fI\n', 3, 0),
    'wrapped': (GOOD + b'@r3\nACGT\nACGT\n+\nIIII\nIIII\n', 3, None),
    'empty record inside': (GOOD + b'\n\n\n\n' + GOOD, 3, None),
}


def test_malformed_records(tmp_path, ctx, monkeypatch):
    """Every malformed kind raises ValueError naming the first bad record -- on the buffer path, the file path and with the
    record cut between feeds; the context counts correctly afterwards (from_fasta against the oracle)."""
    from kpal_amd import _native, klib
    fasta = b'>x\nACGTTGCAACGGT\nAC\n>y\nTTTTGGGG\n'
    fasta_want = oracle.from_sequences([b'ACGTTGCAACGGTAC', b'TTTTGGGG'], 4)
    for what, (text, record, mq) in BAD.items():
        with pytest.raises(Malformed) as info:
            fastq_reads(text, mq)
        assert info.value.record == record, what
        path = tmp_path / 'bad.fq'
        path.write_bytes(text)
        for label, make in (('buffer', lambda: io.BytesIO(text)), ('ragged', lambda: Ragged(text, 3)), ('file', lambda: open(str(path), 'rb'))):
            handle = make()
            with pytest.raises(ValueError) as err:
                klib.Profile.from_fastq(handle, 4, min_quality=mq)
            assert 'record %d:' % record in str(err.value), (what, label, str(err.value))
            np.testing.assert_array_equal(klib.Profile.from_fasta(io.BytesIO(fasta), 4).counts, fasta_want, err_msg=what)
    # the flattening refuses the same texts; a record cut at a staging seam is found in the right chunk
    monkeypatch.setenv('KPAL_FASTA_CHUNK', '17')
    c = _native.Context(_native.default_device())
    monkeypatch.delenv('KPAL_FASTA_CHUNK')
    for what, (text, record, mq) in BAD.items():
        with pytest.raises(ValueError, match='record %d:' % record):
            c.fastq_flatten(text, min_quality=mq)
    # a count abandoned at an error and begun again holds only the new text
    with pytest.raises(ValueError):
        ctx.count_begin(4)
        ctx.count_feed_fastq(BAD['length'][0])
    ctx.count_begin(4)
    ctx.count_feed_fastq(GOOD)
    np.testing.assert_array_equal(ctx.count_finish(4), oracle.from_sequences(fastq_reads(GOOD), 4))


def test_two_million_reads_k12(tmp_path):
    """2 M reads x 150 bp (~670 MB of FASTQ, titles of ~30 bytes, random qualities) at k = 12: every bin against the 16-thread
    oracle over the joined reads."""
    from kpal_amd import klib
    n, L = 2 << 20, 150
    rng = np.random.default_rng(12)
    rec = np.empty((n, 1 + 29 + 1 + L + 3 + L + 1), dtype=np.uint8)
    rec[:, 0] = ord('@')
    rec[:, 1:30] = rng.integers(ord('A'), ord('Z') + 1, size=(n, 29), dtype=np.uint8)
    rec[:, 30] = ord('\n')
    bases = np.frombuffer(b'ACGTN', dtype=np.uint8)[rng.choice(5, size=(n, L), p=[0.249, 0.249, 0.249, 0.249, 0.004])]
    rec[:, 31:31 + L] = bases
    rec[:, 31 + L:34 + L] = np.frombuffer(b'\n+\n', dtype=np.uint8)
    rec[:, 34 + L:34 + 2 * L] = rng.integers(33, 127, size=(n, L), dtype=np.uint8)
    rec[:, -1] = ord('\n')
    path = tmp_path / 'big.fq'
    rec.tofile(str(path))
    del rec
    joined = np.empty((n, L + 1), dtype=np.uint8)
    joined[:, 0] = ord('\n')
    joined[:, 1:] = bases
    del bases
    want = oracle.count_flat(joined.reshape(-1), 12, threads=16)
    del joined
    with open(str(path), 'rb') as fh:
        got = klib.Profile.from_fastq(fh, 12).counts
    np.testing.assert_array_equal(got, want)


def test_cli_count_fastq(tmp_path, monkeypatch):
    """kpal count --fastq -k 8 stores the table of the reads; --min-quality / --phred64 reach the mask; --by-record is refused."""
    from kpal_amd import files, kmer
    rnd = random.Random(8)
    text = random_fastq(rnd, 200, noise=False)
    (tmp_path / 'in.fq').write_bytes(text)
    store = memh5.Store()
    monkeypatch.setattr(files, 'open_profile_file', store.open)
    monkeypatch.chdir(tmp_path)
    kmer.main(['count', '--fastq', '-k', '8', 'in.fq', 'out.k8'])
    got = store.files[os.path.abspath('out.k8')]['profiles/in'][:]
    np.testing.assert_array_equal(got, oracle.from_sequences(fastq_reads(text), 8))
    kmer.main(['count', '--fastq', '--min-quality', '30', '-k', '8', 'in.fq', 'out_q.k8'])
    got = store.files[os.path.abspath('out_q.k8')]['profiles/in'][:]
    np.testing.assert_array_equal(got, oracle.from_sequences(fastq_reads(text, 30), 8))
    with pytest.raises(SystemExit) as ex:
        kmer.main(['count', '--fastq', '--by-record', '-k', '8', 'in.fq', 'out_r.k8'])
    assert ex.value.code == 2
