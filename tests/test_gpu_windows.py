"""One profile per sliding window of each FASTA record (Profile.from_fasta_by_window, kpal_fasta_windows_*; beyond the
reference).  Every expected table is ``oracle.from_sequences([substring], k)`` on sequences generated here -- window j of a
record of L bases is ``seq[j * S:min(j * S + W, L)]`` -- and every comparison is exact.  Run on the GPU box: pytest -m gpu."""
import contextlib
import io
import os
import random

import numpy as np
import pytest

import memh5
import oracle

pytestmark = pytest.mark.gpu

KS = (1, 2, 4, 6, 7, 8, 9)


def shapes(k):
    return [(W, S) for W, S in ((k, 1), (k, k), (12, 1), (16, 16), (48, 16), (1000, 250), (1024, 1024), (4112, 4112)) if k <= W]


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


def window_spans(L, W, S):
    """[start, end) of every window of a record of L bases, enumerated one by one."""
    out, j = [], 0
    while L > 0:
        out.append((j * S, min(j * S + W, L)))
        if out[-1][1] == L:
            break
        j += 1
    return out


def bases(rnd, n):
    return ''.join(rnd.choice('ACGT' * 5 + 'acgt') for _ in range(n))


def make_records(rnd, k, W, S):
    """(title, sequence) per record: the lengths at which the layout changes, a record of a few thousand bases where that
    stays within a few hundred windows, and records with a byte outside the alphabet exactly at a window end, right behind
    it, and exactly k - 1 and k before it (the first and the one before the first k-mer the trim takes off)."""
    lengths = [0, 1, k - 1, k, W - 1, W, W + 1, W + S - 1, W + S, 3 * W + 5]
    if S >= 16:
        lengths.append(max(3001, 2 * W + 77))
    records = [('len%d_%d some title' % (i, L), bases(rnd, L)) for i, L in enumerate(lengths)]
    records.insert(3, ('', bases(rnd, W + 3)))        # an untitled record: named by its 1-based index
    L = W + 2 * S + k                                 # the windows that end at W and at W + S end inside the record
    for i, (pos, ch) in enumerate(((W - 1, 'N'), (W, '\t'), (W - (k - 1), '\t'), (W - k, 'N'), (W + S - 1, '\t'), (W + S, 'N'),
                                   (W + S - (k - 1), 'n'), (W + S - k, '\t'))):
        seq = bases(rnd, L)
        records.append(('odd%d' % i, seq[:pos] + ch + seq[pos + 1:]))
    seq = bases(rnd, L)
    records.append(('lower', seq[:W - k] + seq[W - k:W + k].lower() + seq[W + k:]))
    return records


def fasta_text(rnd, records, eol):
    """The records as FASTA text, wrapped at widths that do not divide the step; a line never ends in a tab (a trailing tab
    would be stripped; these are interior)."""
    parts = []
    for r, (title, seq) in enumerate(records):
        parts.append('>' + title + eol)
        width = (7, 61, 10 ** 9, 13)[r % 4]
        i = 0
        while i < len(seq):
            j = min(i + width, len(seq))
            while j < len(seq) and seq[j - 1] == '\t':
                j += 1
            assert seq[j - 1] != '\t' or j == len(seq)
            parts.append(seq[i:j] + eol)
            i = j
    return ''.join(parts)


def expected(records, k, W, S, prefix=''):
    """(name, table) of every window, record-major."""
    out = []
    for i, (title, seq) in enumerate(records):
        name = prefix + (title.split()[0] if title.split() else str(i + 1))
        for a, b in window_spans(len(seq), W, S):
            out.append(('%s:%d-%d' % (name, a + 1, b), oracle.from_sequences([seq[a:b]], k)))
    return out


def check(profiles, want, what):
    assert [p.name for p in profiles] == [n for n, _ in want], what
    for p, (name, table) in zip(profiles, want):
        np.testing.assert_array_equal(p.counts, table, err_msg='%s window %s' % (what, name))


@pytest.mark.parametrize('k', KS)
def test_grid_of_small_shapes(k, monkeypatch):
    """Every shape of the grid over records of every length at which the layout changes: LDS (k <= 7) and global-atomic
    (k >= 8) tiles, m = 1 and m > 1, S < k - 1, empty records, records shorter than k, N / lowercase / interior tab at and
    around the window ends, line widths that do not divide S, LF and CRLF; batches that begin inside a record."""
    from kpal_amd import klib
    rnd = random.Random(1000 + k)
    assert any(W == S for W, S in shapes(k)) and any(W > S for W, S in shapes(k))
    assert k < 4 or any(S < k - 1 for _, S in shapes(k))
    for i, (W, S) in enumerate(shapes(k)):
        records = make_records(rnd, k, W, S)
        # a trailing tab on the last line of a record would be stripped: none of the generated records ends in one
        assert all(not seq.endswith('\t') for _, seq in records)
        text = fasta_text(rnd, records, '\r\n' if (i + k) % 2 else '\n')
        want = expected(records, k, W, S)
        assert k < 8 or len(want) <= 700
        monkeypatch.setattr(klib, '_RECORD_BATCH_BYTES', (37 if i % 2 else 1 << 20) * 8 * 4 ** k)
        profiles = list(klib.Profile.from_fasta_by_window(io.StringIO(text), k, W, step=None if W == S and i % 2 else S))
        check(profiles, want, 'k=%d W=%d S=%d' % (k, W, S))


@pytest.mark.parametrize('k,W,S', [(4, 12, 4), (4, 16, 16), (8, 16, 2), (8, 8, 8), (7, 48, 16)])
def test_every_range_equals_its_slice_of_the_piece(ctx, k, W, S):
    """kpal_fasta_windows_count over every (first, n) split of a piece's windows -- ranges that begin and end inside a
    record, n = 1 -- against the whole piece, itself against the oracle; the layout entry against the enumeration."""
    rnd = random.Random(k * 100 + S)
    records = [('a', bases(rnd, 2 * W + 5)), ('e', ''), ('b', bases(rnd, k - 1)), ('c', bases(rnd, W + S + 1)), ('d', bases(rnd, W))]
    records[0] = ('a', records[0][1][:W - 2] + 'N' + records[0][1][W - 1:])
    text = fasta_text(rnd, records, '\n').encode()
    n_records, _ = ctx.fasta_records_begin(text)
    assert n_records == len(records)
    want = expected(records, k, W, S)
    n_windows, first_window = ctx.fasta_windows_layout(W, S)
    counts = [len(window_spans(len(seq), W, S)) for _, seq in records]
    assert n_windows == len(want) and first_window.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    whole = ctx.fasta_windows_count(k, W, S, 0, n_windows)
    for row, (name, table) in zip(whole, want):
        np.testing.assert_array_equal(row, table, err_msg=name)
    for first in range(n_windows + 1):
        for n in range(0, n_windows - first + 1):
            got = ctx.fasta_windows_count(k, W, S, first, n)
            np.testing.assert_array_equal(got, whole[first:first + n], err_msg='windows %d..%d' % (first, first + n))
    for bad in ((k, W, S, n_windows, 1), (k, W, S, 0, n_windows + 1), (k, W, 0, 0, 1), (k, W, W + 1, 0, 1), (W + 1, W, S, 0, 1), (0, W, S, 0, 1)):
        if bad[0] <= 16:
            with pytest.raises(ValueError):
                ctx.fasta_windows_count(*bad)
    with pytest.raises(ValueError):
        ctx.fasta_windows_layout(12, 5)


def test_file_and_text_routes_agree(tmp_path, monkeypatch):
    """The plain-file route (the library reads the file itself, pieces forced down to a few hundred bytes: records span
    pieces, pieces hold several records) and the StringIO route: identical names and tables, both equal to the oracle."""
    from kpal_amd import _native, klib
    rnd = random.Random(9)
    for k, W, S in ((4, 48, 16), (8, 16, 2), (6, 40, 40)):
        records = make_records(rnd, k, W, S)[:14] + [('tail', bases(rnd, 700))]
        text = fasta_text(rnd, records, '\n')
        want = expected(records, k, W, S, prefix='p_')
        monkeypatch.setattr(klib, '_RECORD_BATCH_BYTES', 11 * 8 * 4 ** k)
        from_text = list(klib.Profile.from_fasta_by_window(io.StringIO(text), k, W, S, prefix='p'))
        check(from_text, want, 'text route k=%d' % k)
        path = tmp_path / ('w%d.fa' % k)
        path.write_text(text)
        for chunk in (300, 64 << 20):
            monkeypatch.setenv('KPAL_FASTA_CHUNK', str(chunk))
            ctx2 = _native.Context(_native.default_device())
            monkeypatch.delenv('KPAL_FASTA_CHUNK')
            with monkeypatch.context() as m:
                m.setattr(_native, 'context', lambda: ctx2)
                try:
                    with open(str(path)) as fh:
                        from_file = list(klib.Profile.from_fasta_by_window(fh, k, W, S, prefix='p'))
                        assert fh.read() == ''
                    check(from_file, want, 'file route k=%d chunk=%d' % (k, chunk))
                finally:
                    ctx2.close()
    empty = tmp_path / 'empty.fa'
    empty.write_bytes(b'')
    with open(str(empty)) as fh:
        assert list(klib.Profile.from_fasta_by_window(fh, 4, 8)) == []
    assert list(klib.Profile.from_fasta_by_window(io.StringIO('no header\nACGT\n'), 4, 8)) == []


def test_windows_stay_in_hbm_and_feed_the_rectangle(ctx, monkeypatch):
    """The profiles report device tables; the rectangle windows x [whole sequence] is computed where the tables lie -- no
    host-to-device and no device-to-device copy -- and matches the oracle's pair distance to 1e-9; past the budget of live
    device tables a batch is downloaded at once."""
    from kpal_amd import _native, kdistlib, klib
    rnd = random.Random(4)
    k, W, S = 4, 500, 100
    seq = bases(rnd, 6000)
    text = '>g\n' + seq + '\n'
    windows = list(klib.Profile.from_fasta_by_window(io.StringIO(text), k, W, S))
    whole = klib.Profile.from_sequences([seq], k, name='whole')
    spans = window_spans(len(seq), W, S)
    assert len(windows) == len(spans) and all(p._device_counts() is not None for p in windows) and whole._device_counts() is not None
    copies = []
    for name in ('h2d', 'd2d'):
        real = getattr(_native.Context, name)
        monkeypatch.setattr(_native.Context, name, lambda self, *a, _real=real, _name=name: (copies.append(_name), _real(self, *a))[1])
    got = kdistlib.cross_distances(windows, [whole], kdistlib.ProfileDistance())
    assert copies == [] and got.shape == (len(windows), 1)
    assert all(p._device_counts() is not None for p in windows)
    full = oracle.from_sequences([seq], k)
    for (a, b), value in zip(spans, got[:, 0]):
        want = oracle.profile_distance(oracle.from_sequences([seq[a:b]], k), full, k)
        assert abs(value - want) <= 1e-9 * max(1.0, abs(want)), (a, b, value, want)
    monkeypatch.setattr(klib, '_DEVICE_PROFILE_BYTES', 0)
    host = list(klib.Profile.from_fasta_by_window(io.StringIO(text), k, W, S))
    assert all(p._device_counts() is None for p in host)
    for p, q in zip(host, windows):
        np.testing.assert_array_equal(p.counts, q.counts)


def launches(ctx, text, k, W, S):
    """{kernel: launches} of ONE kpal_fasta_windows_count_device over all windows of text, and the tables."""
    ctx.fasta_records_begin(text.encode())
    n, _ = ctx.fasta_windows_layout(W, S)
    dev = ctx.alloc(n * 8 * 4 ** k)
    try:
        ctx.prof_enable(True)
        ctx.prof_reset()
        ctx.fasta_windows_count_device(k, W, S, 0, n, dev)
        ctx.sync()
        seen = dict((name, count) for name, (_, count) in ctx.prof_get().items() if count)
        out = np.empty((n, 4 ** k), dtype=np.int64)
        ctx.d2h(out, dev)
    finally:
        ctx.prof_enable(False)
        ctx.free(dev)
    return n, seen, out


def test_launch_structure_and_determinism(ctx):
    """The launches of one batch do not depend on the number of windows or on the overlap: tiles, running sum, trim.
    m = 1 launches no running sum; k <= 7 launches neither count_records nor the global-atomic tile kernel; k >= 8 launches
    the atomic tile kernel once.  Two calls give the same bits."""
    rnd = random.Random(12)
    short, long_ = '>s\n' + bases(rnd, 200 + 9 * 20) + '\n', '>l\n' + bases(rnd, 200 + 999 * 20) + '\n'
    n10, few, _ = launches(ctx, short, 4, 200, 20)
    n1000, many, first = launches(ctx, long_, 4, 200, 20)
    assert (n10, n1000) == (10, 1000)
    assert few == many == {'window_tiles': 1, 'window_slide': 1, 'window_trim': 1}
    _, again, second = launches(ctx, long_, 4, 200, 20)
    assert again == many
    np.testing.assert_array_equal(first, second)
    _, m2, _ = launches(ctx, long_, 4, 200, 100)
    _, m16, _ = launches(ctx, long_, 4, 320, 20)
    assert m2 == m16 == many
    _, m1, _ = launches(ctx, long_, 4, 200, 200)
    assert m1 == {'window_tiles': 1, 'window_trim': 1}
    n_long, long_tiles, tables = launches(ctx, long_, 7, 5000, 2500)      # steps past 2048 bases: eight waves per tile, the same names
    assert long_tiles == many
    want = expected([('l', long_[3:-1])], 7, 5000, 2500)
    assert n_long == len(want) == 8
    for row, (name, table) in zip(tables, want):
        np.testing.assert_array_equal(row, table, err_msg=name)
    text8 = '>l\n' + bases(rnd, 64 + 99 * 16) + '\n'
    n8, k8, a = launches(ctx, text8, 8, 64, 16)
    _, k8_again, b = launches(ctx, text8, 8, 64, 16)
    assert n8 == 100 and k8 == k8_again == {'window_tiles_atomic': 1, 'window_slide': 1, 'window_trim': 1}
    np.testing.assert_array_equal(a, b)
    _, k8_m1, _ = launches(ctx, text8, 8, 64, 64)
    assert k8_m1 == {'window_tiles_atomic': 1, 'window_trim': 1}


def test_count_by_window_on_the_command_line(tmp_path, monkeypatch):
    """``kpal count -k 4 --by-window 200 --step 100``: names and tables of the saved profiles; with two inputs the names
    carry the files' prefixes; the flag combinations that are refused end in a usage error."""
    from kpal_amd import files, kmer
    rnd = random.Random(21)
    records = [('chr1 first', bases(rnd, 1234)), ('chr2', bases(rnd, 150)), ('', bases(rnd, 401)), ('chr4', '')]
    text = fasta_text(rnd, records, '\n')
    (tmp_path / 'g.fa').write_text(text)
    (tmp_path / 'h.fa').write_text(text)
    store = memh5.Store()
    monkeypatch.setattr(files, 'open_profile_file', store.open)
    monkeypatch.chdir(tmp_path)
    kmer.main(['count', '-k', '4', '--by-window', '200', '--step', '100', 'g.fa', 'one.k4'])
    handle = store.files[os.path.abspath('one.k4')]
    want = expected(records, 4, 200, 100)
    assert sorted(handle['profiles']) == sorted(n for n, _ in want)
    assert 'chr1:1-200' in handle['profiles'] and 'chr1:1101-1234' in handle['profiles'] and '3:1-200' in handle['profiles']
    for name, table in want:
        np.testing.assert_array_equal(handle['profiles/' + name][:], table, err_msg=name)
    kmer.main(['count', '-k', '4', '--by-window', '200', 'g.fa', 'h.fa', 'two.k4'])
    handle = store.files[os.path.abspath('two.k4')]
    both = expected(records, 4, 200, 200, prefix='g_') + expected(records, 4, 200, 200, prefix='h_')
    assert sorted(handle['profiles']) == sorted(n for n, _ in both)
    for name, table in both:
        np.testing.assert_array_equal(handle['profiles/' + name][:], table, err_msg=name)
    for argv in (['count', '--by-window', '200', '--by-record', 'g.fa', 'x1.k9'], ['count', '--by-window', '200', '--fastq', 'g.fa', 'x2.k9'],
                 ['count', '--step', '100', 'g.fa', 'x3.k9'], ['count', '-k', '4', '--by-window', '200', '--step', '150', 'g.fa', 'x4.k4']):
        with contextlib.redirect_stderr(io.StringIO()), pytest.raises(SystemExit) as exc:
            kmer.main(argv)
        assert exc.value.code == 2
