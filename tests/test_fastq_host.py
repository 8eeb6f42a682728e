"""FASTQ input without a GPU: the argument checks of Profile.from_fastq (k, quality offset, min_quality) raise ValueError before
any device is touched, and the `kpal count` flags --fastq / --min-quality / --phred64 parse and are checked.

The FASTQ text generators of tests/fastq_cases.py are proved here before tests/test_gpu_fastq_edges.py trusts them: every edge
text is legal FASTQ with its event at the offset its label names, the labels cover the whole product, the long reads have the
line lengths they claim and qualities the mask acts on in every block, and the byte ranges tile their text."""
import itertools
import os
import random

import pytest

import fastq_cases as fc
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


@pytest.fixture(scope='module')
def edge_texts():
    return fc.edge_texts()


@pytest.fixture(scope='module')
def long_reads():
    return fc.long_read_texts()


def test_every_edge_text_parses_with_its_event_where_the_label_says(edge_texts):
    for label, text in edge_texts:
        event = label.split('@')[0]
        reads = fc.fastq_reads(text)
        assert len(reads) >= 4, label
        assert fc.fastq_reads(text, fc.MASK_QUALITY) != reads, label           # the mask at 20 is not a no-op on it
        assert fc.event_offset(event, text) == fc.edge_target(label), label     # (found by reading the text)
        assert (event == 'eot') == (not text.endswith(b'\n')), label


def test_edge_targets_are_the_edges_of_the_tokeniser():
    """block b: 4096 b; slice j, wave w: 16 j and 1024 w inside block 1; the deltas are -2 .. +2."""
    assert (fc.BLOCK, fc.SLICE, fc.WAVE) == (4096, 16, 1024)
    assert dict(fc.EDGES) == {'block1': 4096, 'block2': 8192, 'slice1': 4096 + 16, 'slice37': 4096 + 16 * 37, 'slice255': 4096 + 16 * 255,
                              'wave1': 4096 + 1024, 'wave2': 4096 + 2048, 'wave3': 4096 + 3072}
    assert fc.DELTAS == (-2, -1, 0, 1, 2)
    assert fc.edge_target('nl_seq@block2-1') == 8191 and fc.edge_target('cr@slice37+2') == 4096 + 592 + 2


def test_every_event_edge_and_delta_has_a_text(edge_texts):
    """The '\\n' of each of the four roles, the '\\r' of a '\\r\\n', the first byte of each role, an empty sequence-plus-quality
    pair and the end of the text without '\\n' -- each at every edge and every delta, once."""
    assert set(fc.EVENTS) == {'nl_title', 'nl_seq', 'nl_sep', 'nl_qual', 'cr', 'first_title', 'first_seq', 'first_sep', 'first_qual',
                              'empty_pair', 'eot'}
    want = sorted(fc.edge_label(ev, edge, d) for ev, edge, d in itertools.product(fc.EVENTS, fc.EDGES, fc.DELTAS))
    assert sorted(label for label, _ in edge_texts) == want
    assert len(want) == len(set(want)) == 11 * 8 * 5


def test_long_reads_have_the_lines_they_claim(long_reads):
    by_label = {c.label: c for c in long_reads}
    assert len(by_label) == len(long_reads)
    for n in (4095, 4096, 4097, 8192, 65537, 1000003):
        assert by_label['seq_%d' % n].long_lines == (n, n)                      # the sequence line and its quality line
    assert by_label['title_5001'].long_lines == (5001,)
    for case in long_reads:
        spans = fc.line_spans(case.text)
        lengths = [e - s - (1 if e > s and e < len(case.text) and case.text[e - 1:e] == b'\r' else 0) for s, e in spans]
        assert tuple(n for n in lengths if n >= fc.LONG_LINE) == case.long_lines, case.label
        reads = fc.fastq_reads(case.text)
        long_seqs = [r for r in reads if len(r) >= fc.LONG_LINE]
        if case.label == 'title_5001':
            assert not long_seqs and lengths.index(5001) % 4 == 0                # the long line is a title
        else:
            assert [len(r) for r in long_seqs] == [case.long_lines[0]], case.label
            seq = long_seqs[0]
            assert b'N' * 17 in seq and b'N' * (fc.MAX_N_RUN + 1) not in seq, case.label
            assert any(c in seq for c in b'acgt') and b'n' not in seq, case.label
        # no chunk setting the GPU tests use needs more than MAX_CHUNK_ITERATIONS chunks
        assert len(case.text) // case.min_chunk + 2 <= fc.MAX_CHUNK_ITERATIONS, case.label
    # the special shapes
    text = by_label['seq_4096_at_block_start'].text
    s, e = fc.line_spans(text)[5]
    assert (s, e) == (fc.BLOCK, 2 * fc.BLOCK)                                    # block 1 keeps all of its 4096 bytes
    assert by_label['seq_1000003'].min_chunk >= 65536
    assert by_label['long_crlf'].text.count(b'\r\n') == by_label['long_crlf'].text.count(b'\n') - 4
    singles = fc.fastq_reads(by_label['long_then_3000_singles'].text)
    assert len(singles) == 3001 and all(len(r) == 1 for r in singles[1:])
    assert not by_label['long_without_final_newline'].text.endswith(b'\n')


def test_the_mask_changes_a_base_in_every_block_of_a_long_read(long_reads):
    for case in long_reads:
        assert fc.blocks_without_masked_base(case.text) == [], case.label
        masked, plain = fc.fastq_reads(case.text, fc.MASK_QUALITY), fc.fastq_reads(case.text)
        assert masked != plain, case.label
    # ... and the check has teeth: qualities of 'I' throughout mask nothing
    seq, _ = fc.long_sequence(random.Random(1), 9000)
    assert fc.blocks_without_masked_base(b'@x\n' + seq + b'\n+\n' + b'I' * 9000 + b'\n')


def _role_at(spans, at):
    for i, (s, e) in enumerate(spans):
        if s <= at <= e:
            return i % 4, s < at < e
    raise AssertionError(at)


def test_range_cuts_tile_the_text(edge_texts, long_reads):
    texts = [edge_texts[0][1], dict(edge_texts)['cr@block1+0'], long_reads[0].text, long_reads[0].text[:-1],
             [c for c in long_reads if c.label == 'long_crlf'][0].text]
    for t, text in enumerate(texts):
        n = len(text)
        spans = fc.line_spans(text)
        lists = fc.range_cuts(text, 7 + t)
        assert len(lists) == 3
        for cuts in lists:
            assert cuts[0] == 0 and cuts[-1] == n and all(a <= b for a, b in zip(cuts, cuts[1:])), (t, cuts)
            ranges = fc.ranges_of(cuts)
            assert b''.join(text[a:b] for a, b in ranges) == text               # consecutive ranges, no gap, no overlap
        structured = lists[0]
        ranges = fc.ranges_of(structured)
        assert (0, 0) in ranges and (n, n) in ranges                             # empty ranges at both ends
        assert any(a == b and 0 < a < n for a, b in ranges)                      # ... and in the middle
        assert any(b - a == 1 for a, b in ranges)                                # one-byte ranges
        inside = {role for role, strictly in (_role_at(spans, c) for c in structured if 0 < c < n) if strictly}
        assert inside == {0, 1, 2, 3}, (t, inside)                               # a cut inside a line of every role
        if b'\r\n' in text:
            assert any(text[c - 1:c + 1] == b'\r\n' for c in structured if 0 < c < n), t
        assert any(b - a <= 3 for a, b in fc.ranges_of(lists[2])[1:-1])
