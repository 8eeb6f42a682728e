"""Sliding-window profiles without a GPU: the three C entries are declared, exported and bound; ``from_fasta_by_window`` and
the ``kpal count --by-window / --step`` flags exist and refuse bad arguments before any device call; and the layout
arithmetic of kpal_amd/csrc/window_index.hpp -- driven by a stand-alone program built with the address and
undefined-behaviour sanitizers -- agrees line by line with a brute-force enumeration, as does the tile decomposition the
kernels rest on (window = its tiles - the k-mers that run past its end)."""
import collections
import inspect
import io
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('kpal_fasta_windows_layout', 'kpal_fasta_windows_count', 'kpal_fasta_windows_count_device')


@pytest.fixture(scope='module')
def built():
    import __graft_entry__
    __graft_entry__.build()
    from kpal_amd import _native
    return _native


def test_entries_declared_exported_and_bound(built):
    header = open(os.path.join(ROOT, 'include', 'kpal_hip.h')).read()
    L = built.load()
    for name in ENTRIES:
        assert name + '(' in header, name
        assert hasattr(L, name), 'libkpal_hip.so does not export %s' % name
        assert name in built.SIGNATURES
    for method in ('fasta_windows_layout', 'fasta_windows_count', 'fasta_windows_count_device'):
        assert callable(getattr(built.Context, method))


def test_python_and_cli_surface(tmp_path, monkeypatch):
    import memh5
    from kpal_amd import files, klib, kmer
    assert inspect.isgeneratorfunction(klib.Profile.from_fasta_by_window)
    assert list(inspect.signature(klib.Profile.from_fasta_by_window).parameters) == ['handle', 'length', 'window', 'step', 'prefix']
    monkeypatch.setattr(files, 'open_profile_file', memh5.Store().open)
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'a.fa').write_text('>r\nACGT\n')
    parser = kmer.build_parser()
    args = parser.parse_args(['count', '-k', '4', '--by-window', '200', '--step', '100', 'a.fa', 'one.k4'])
    assert (args.size, args.by_window, args.step, args.by_record, args.fastq) == (4, 200, 100, False, False)
    args = parser.parse_args(['count', '--by-window', '5000', 'a.fa', 'two.k9'])
    assert (args.by_window, args.step) == (5000, None)
    args = parser.parse_args(['count', 'a.fa', 'three.k9'])
    assert (args.by_window, args.step) == (None, None)
    # the usage errors of the front end: exit status 2, nothing counted
    for extra in (['--by-record'], ['--fastq'], ['--step', '7'], ['-k', '9', '--by-window', '8']):
        argv = ['count', '--by-window', '200'] + extra + ['a.fa', 'bad%d.k9' % len(extra[0])]
        if extra[0] == '-k':
            argv = ['count'] + extra + ['a.fa', 'badk.k9']
        with pytest.raises(SystemExit) as exc:
            kmer.main(argv)
        assert exc.value.code == 2


def test_bad_arguments_are_refused_before_any_device_call(monkeypatch):
    from kpal_amd import _native, klib, kmer

    def no_device(*a, **kw):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(_native, 'context', no_device)
    fasta = '>r\nACGTACGTACGT\n'
    bad = [dict(length=5, window=4), dict(length=4, window=12, step=0), dict(length=4, window=12, step=13),
           dict(length=4, window=12, step=5), dict(length=4, window=12, step=-3), dict(length=0, window=12),
           dict(length=17, window=100), dict(length=4, window=0), dict(length=4, window=1 << 63)]
    for kw in bad:
        with pytest.raises(ValueError):
            list(klib.Profile.from_fasta_by_window(io.StringIO(fasta), **kw))
    handles, out = [io.StringIO(fasta)], object()
    for kw, word in ((dict(by_window=8, by_record=True), 'by-record'), (dict(by_window=8, fastq=True), 'FASTQ'),
                     (dict(step=4), '--step'), (dict(by_window=8, step=3), 'step'), (dict(by_window=3), 'window'),
                     (dict(by_window=8, step=16), 'step')):
        with pytest.raises(ValueError, match=word):
            kmer.count(handles, out, 4, **kw)
    # good arguments get as far as the device
    with pytest.raises(AssertionError, match='device call'):
        list(klib.Profile.from_fasta_by_window(io.StringIO(fasta), 4, 12, step=3))
    with pytest.raises(AssertionError, match='device call'):
        list(klib.Profile.from_fasta_by_window(io.StringIO(fasta), 4, 4))


# ---- the layout, by brute force ---------------------------------------------------------------------------------------
def brute_layout(W, S, k, lengths):
    """The lines window_index_check prints, from the issue's definitions alone: windows enumerated one by one, tiles as the
    sets of ``base // S`` of the bases they hold."""
    lines = []
    starts, windows, n_tiles = [0], [], 0
    for L in lengths:
        starts.append(starts[-1] + 1 + L)
    first_w = first_t = 0
    for r, L in enumerate(lengths):
        mine = []
        j = 0
        while L > 0:
            a, b = j * S, min(j * S + W, L)
            mine.append((a, b))
            if b == L:
                break
            j += 1
        nt = len(set(p // S for p in range(L)))
        lines.append('record %d %d %d %d %d %d' % (r, L, len(mine), nt, first_w, first_t))
        for j, (a, b) in enumerate(mine):
            tiles = sorted(set(p // S for p in range(a, b)))
            assert tiles == list(range(tiles[0], tiles[-1] + 1)) and tiles[0] == j
            windows.append((r, j, a, b, first_t + tiles[0], first_t + tiles[-1] + 1, int(b < L), starts[r] + 1, L, tiles[-1] + 1))
        first_w += len(mine)
        first_t += nt
        n_tiles += nt
    lines.insert(len(lengths), 'total %d %d' % (first_w, n_tiles))
    for w, x in enumerate(windows):
        lines.append('window %d %d %d %d %d %d %d %d' % ((w,) + x[:7]))
    for first in range(len(windows)):
        for n in range(1, len(windows) - first + 1):
            a, b = windows[first], windows[first + n - 1]
            # the bytes the tiles' k-mers lie in: from the first window's first base to k - 1 bases past its last tile
            byte1 = b[7] + min(b[9] * S + k - 1, b[8])
            lines.append('range %d %d %d %d %d %d' % (first, n, a[4], b[5], a[7] + a[2], byte1))
    return lines


def layout_cases():
    cases = []
    for k, W, S in ((4, 12, 1), (4, 12, 12), (4, 12, 4), (9, 12, 3), (9, 9, 1), (1, 1, 1), (7, 48, 16), (3, 6, 2), (8, 16, 2)):
        lengths = [0, 1, k - 1, k, W - 1, W, W + 1, W + S - 1, W + S, 3 * W + 5]
        cases.append((k, W, S, lengths))
        cases.append((k, W, S, [3 * W + 5]))
    return cases


@pytest.fixture(scope='module')
def layout_program(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('window_index') / 'window_index_check')
    b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe,
                        os.path.join(ROOT, 'tests', 'native', 'window_index_check.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0, b.stdout.decode()[-3000:]
    return exe


def test_layout_against_brute_force(layout_program):
    assert any(S < k - 1 for k, W, S, _ in layout_cases()) and any(S == 1 for _, _, S, _ in layout_cases())
    for k, W, S, lengths in layout_cases():
        r = subprocess.run([layout_program, str(W), str(S), str(k)] + [str(L) for L in lengths], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=120)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0, got[-20:]
        assert got[0] == 'args 1'
        want = brute_layout(W, S, k, lengths)
        assert got[1:-1] == want, (k, W, S, [(g, w) for g, w in zip(got[1:], want) if g != w][:5])
    for k, W, S in ((5, 4, 4), (4, 12, 0), (4, 12, 13), (4, 12, 5), (0, 12, 12)):
        r = subprocess.run([layout_program, str(W), str(S), str(k), '10'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert r.returncode == 0 and r.stdout.decode() == 'args 0\n', (k, W, S)


def kmers(seq, k, a, b, whole):
    """Multiset of the valid k-mers that BEGIN in [a, b) of seq; with ``whole`` only those that also end before b."""
    out = collections.Counter()
    for p in range(a, b):
        word = seq[p:p + k]
        if len(word) == k and all(c in 'ACGTacgt' for c in word) and (not whole or p + k <= b):
            out[word.upper()] += 1
    return out


def test_tile_decomposition_is_exact():
    """window j = sum of its tiles (k-mers by first base) - the k-mers that begin in its last k - 1 bases and run past its
    end, taken off only when the window ends before the record: what window_tiles / window_slide / window_trim compute."""
    rng = random.Random(5)
    for k, W, S in ((4, 12, 1), (9, 12, 3), (3, 6, 2), (8, 16, 2), (2, 8, 8), (5, 20, 5)):
        assert W % S == 0
        for L in (1, k - 1, k, W - 1, W, W + 1, W + S - 1, W + S, 3 * W + 5):
            seq = ''.join(rng.choice('ACGTacgtN\t' if rng.random() < 0.2 else 'ACGT') for _ in range(L))
            j = 0
            while True:
                a, b = j * S, min(j * S + W, L)
                tiles = collections.Counter()
                for t in range(j, j + W // S):
                    tiles.update(kmers(seq, k, min(t * S, L), min((t + 1) * S, L), False))
                if b < L:
                    tiles.subtract(kmers(seq, k, b - k + 1, b, False))
                assert +tiles == kmers(seq, k, a, b, True) and min(tiles.values(), default=0) >= 0, (k, W, S, L, j)
                if b == L:
                    break
                j += 1
