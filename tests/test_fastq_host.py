"""FASTQ input without a GPU: the argument checks of Profile.from_fastq (k, quality offset, min_quality) raise ValueError before
any device is touched, and the `kpal count` flags --fastq / --min-quality / --phred64 parse and are checked."""
import os

import pytest

import memh5


@pytest.mark.parametrize('kwargs', [dict(length=0), dict(length=17), dict(length=8, quality_offset=32),
                                    dict(length=8, quality_offset=0), dict(length=8, min_quality=-1),
                                    dict(length=8, min_quality=94), dict(length=8, min_quality=2.5),
                                    dict(length=8, min_quality=True)])
def test_from_fastq_argument_errors(kwargs):
    from kpal_amd import klib
    with pytest.raises(ValueError):
        klib.Profile.from_fastq(None, **kwargs)


def test_fastq_options_check_accepts():
    from kpal_amd import _native
    for mq in (None, 0, 20, 93):
        for off in (33, 64):
            _native.fastq_options_check(mq, off)


def test_count_parser_flags(tmp_path, monkeypatch):
    from kpal_amd import files, kmer
    (tmp_path / 'a.fq').write_bytes(b'@r\nACGT\n+\nIIII\n')
    monkeypatch.setattr(files, 'open_profile_file', memh5.Store().open)
    monkeypatch.chdir(tmp_path)
    parser = kmer.build_parser()
    args = parser.parse_args(['count', '--fastq', '--min-quality', '20', '--phred64', '-k', '5', 'a.fq', 'o1.k'])
    assert (args.fastq, args.min_quality, args.phred64, args.size, args.by_record) == (True, 20, True, 5, False)
    args.input_handles[0].close()
    args = parser.parse_args(['count', 'a.fq', 'o2.k'])
    assert (args.fastq, args.min_quality, args.phred64) == (False, None, False)
    args.input_handles[0].close()


@pytest.mark.parametrize('argv', [['count', '--fastq', '--by-record', 'a.fq', 'o.k'],
                                  ['count', '--min-quality', '20', 'a.fq', 'o.k'],
                                  ['count', '--phred64', 'a.fq', 'o.k']])
def test_count_refuses_flag_combinations(tmp_path, monkeypatch, capsys, argv):
    """--by-record with --fastq, and the quality flags without --fastq, end in the usage error before anything is counted."""
    from kpal_amd import files, kmer
    (tmp_path / 'a.fq').write_bytes(b'@r\nACGT\n+\nIIII\n')
    monkeypatch.setattr(files, 'open_profile_file', memh5.Store().open)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as ex:
        kmer.main(argv)
    assert ex.value.code == 2
    err = capsys.readouterr().err
    assert '--fastq' in err or 'FASTQ' in err
    assert os.path.exists('a.fq')
