"""One profile per FASTQ read, or per window of a read, without a GPU: the two C entries are declared, exported and bound;
``from_fastq_by_record`` / ``from_fastq_by_window`` and the ``kpal count --by-read`` flag exist; the parser takes the flag with
its companions and still refuses what it refused; and every bad argument is a ``ValueError`` before any device call."""
import inspect
import io
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('kpal_fastq_records_begin', 'kpal_fastq_records_file_open')
FASTQ = '@r one\nACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIII\n'


@pytest.fixture(scope='module')
def built():
    import __graft_entry__
    __graft_entry__.build()
    from kpal_amd import _native
    return _native


def test_generators_and_their_signatures():
    from kpal_amd import klib
    assert inspect.isgeneratorfunction(klib.Profile.from_fastq_by_record)
    assert inspect.isgeneratorfunction(klib.Profile.from_fastq_by_window)
    by_record = inspect.signature(klib.Profile.from_fastq_by_record).parameters
    assert list(by_record) == ['handle', 'length', 'prefix', 'min_quality', 'quality_offset']
    assert [by_record[p].default for p in ('prefix', 'min_quality', 'quality_offset')] == [None, None, 33]
    by_window = inspect.signature(klib.Profile.from_fastq_by_window).parameters
    assert list(by_window) == ['handle', 'length', 'window', 'step', 'prefix', 'min_quality', 'quality_offset']
    assert [by_window[p].default for p in ('step', 'prefix', 'min_quality', 'quality_offset')] == [None, None, None, 33]


def test_parser_takes_by_read_and_keeps_its_refusals(tmp_path, monkeypatch):
    import memh5
    from kpal_amd import files, kmer
    monkeypatch.setattr(files, 'open_profile_file', memh5.Store().open)
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'a.fq').write_text(FASTQ)
    parser = kmer.build_parser()
    args = parser.parse_args(['count', '--by-read', 'a.fq', 'one.k9'])
    assert (args.by_read, args.by_window, args.step, args.min_quality, args.phred64, args.fastq, args.by_record) == \
        (True, None, None, None, False, False, False)
    args = parser.parse_args(['count', '--by-read', '--by-window', '200', '--step', '100', '--min-quality', '20', '--phred64', '-k', '4',
                              'a.fq', 'two.k4'])
    assert (args.by_read, args.by_window, args.step, args.min_quality, args.phred64, args.size) == (True, 200, 100, 20, True, 4)
    args = parser.parse_args(['count', '--by-read', '--fastq', 'a.fq', 'three.k9'])
    assert args.by_read and args.fastq
    assert parser.parse_args(['count', 'a.fq', 'four.k9']).by_read is False
    # kmer.count keeps its parameters in place; by_read is the last one
    params = inspect.signature(kmer.count).parameters
    assert list(params) == ['input_handles', 'output_handle', 'size', 'names', 'by_record', 'fastq', 'min_quality', 'phred64',
                            'by_window', 'step', 'by_read']
    assert params['by_read'].default is False
    # usage errors: exit status 2, nothing counted
    for n, flags in enumerate((['--by-read', '--by-record'], ['--by-read', '--step', '4'], ['--fastq', '--by-record'],
                               ['--by-window', '8', '--fastq'], ['--min-quality', '20'], ['--phred64'],
                               ['--by-read', '-k', '9', '--by-window', '8'], ['--by-read', '--min-quality', '94'])):
        with pytest.raises(SystemExit) as exc:
            kmer.main(['count'] + flags + ['a.fq', 'bad%d.k9' % n])
        assert exc.value.code == 2, flags


def test_bad_arguments_are_refused_before_any_device_call(monkeypatch):
    from kpal_amd import _native, klib, kmer

    def no_device(*a, **kw):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(_native, 'context', no_device)
    bad_record = [dict(length=0), dict(length=17), dict(length=4, min_quality=-1), dict(length=4, min_quality=94),
                  dict(length=4, min_quality=2.5), dict(length=4, min_quality=True), dict(length=4, quality_offset=0),
                  dict(length=4, quality_offset=32), dict(length=4, min_quality=20, quality_offset=65)]
    for kw in bad_record:
        with pytest.raises(ValueError):
            list(klib.Profile.from_fastq_by_record(io.StringIO(FASTQ), **kw))
    bad_window = [dict(length=5, window=4), dict(length=4, window=12, step=0), dict(length=4, window=12, step=13),
                  dict(length=4, window=12, step=5), dict(length=4, window=12, step=-3), dict(length=0, window=12),
                  dict(length=17, window=100), dict(length=4, window=0), dict(length=4, window=1 << 63),
                  dict(length=4, window=12, min_quality=94), dict(length=4, window=12, min_quality=-1),
                  dict(length=4, window=12, quality_offset=34)]
    for kw in bad_window:
        with pytest.raises(ValueError):
            list(klib.Profile.from_fastq_by_window(io.StringIO(FASTQ), **kw))
    handles, out = [io.StringIO(FASTQ)], object()
    for size, kw, word in ((4, dict(by_read=True, by_record=True), 'by-record'), (4, dict(by_read=True, step=4), '--step'),
                           (4, dict(by_read=True, by_window=8, step=3), 'step'), (4, dict(by_read=True, by_window=3), 'window'),
                           (4, dict(by_read=True, by_window=8, step=16), 'step'), (0, dict(by_read=True), 'k-mer length'),
                           (17, dict(by_read=True), 'k-mer length'), (4, dict(by_read=True, min_quality=94), 'min_quality'),
                           (4, dict(by_read=True, min_quality=-1), 'min_quality'), (4, dict(min_quality=20), 'FASTQ'),
                           (4, dict(phred64=True), 'FASTQ'), (4, dict(fastq=True, by_record=True), 'FASTQ'),
                           (4, dict(fastq=True, by_window=8), 'FASTQ')):
        with pytest.raises(ValueError, match=word):
            kmer.count(handles, out, size, **kw)
    # good arguments get as far as the device
    for make in (lambda: klib.Profile.from_fastq_by_record(io.StringIO(FASTQ), 4),
                 lambda: klib.Profile.from_fastq_by_record(io.StringIO(FASTQ), 16, prefix='p', min_quality=0, quality_offset=64),
                 lambda: klib.Profile.from_fastq_by_window(io.StringIO(FASTQ), 4, 12, step=3),
                 lambda: klib.Profile.from_fastq_by_window(io.StringIO(FASTQ), 4, 4, min_quality=93)):
        with pytest.raises(AssertionError, match='device call'):
            list(make())
    for kw in (dict(by_read=True), dict(by_read=True, fastq=True, min_quality=20, phred64=True), dict(by_read=True, by_window=8, step=4)):
        with pytest.raises(AssertionError, match='device call'):
            kmer.count(handles, out, 4, **kw)


def test_entries_declared_exported_and_bound(built):
    header = open(os.path.join(ROOT, 'include', 'kpal_hip.h')).read()
    L = built.load()
    for name in ENTRIES:
        assert name + '(' in header, name
        assert hasattr(L, name), 'libkpal_hip.so does not export %s' % name
        assert name in built.SIGNATURES
    for method in ('fastq_records_begin', 'fastq_records_file_open'):
        assert callable(getattr(built.Context, method))
    begin = inspect.signature(built.Context.fastq_records_begin).parameters
    assert list(begin) == ['self', 'text', 'min_quality', 'quality_offset', 'final', 'records_before']
    file_open = inspect.signature(built.Context.fastq_records_file_open).parameters
    assert list(file_open) == ['self', 'path', 'begin', 'end', 'min_quality', 'quality_offset', 'records_before']
