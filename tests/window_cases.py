"""Sliding-window cases PAST the first trip of every loop of kpal_amd/csrc/window_kernels.hpp and of fasta_windows_pass
(kpal_amd/csrc/kpal_records.hip), for tests/test_gpu_windows_trips.py.  No GPU in here: the plan numbers are restated from
the host code, the shapes are derived from them, and tests/test_window_cases_host.py asserts on the CPU -- for 256 and for 320
compute units -- that every case reaches what it is there for.

Sequences are drawn by a seeded numpy.random.RandomState over ACGTacgt with about one N per 3000 bases; every expected table
is ``oracle.from_sequences([seq[a:b]], k)`` of one window.  The stream the kernels walk is restated by ``stream``: record r is
one '\\n' at starts[r], then its bases."""
import collections
import functools

import numpy as np

import oracle

ALPHABET = np.frombuffer(b'ACGTacgt', dtype=np.uint8)
N_EVERY = 3000
CUS = (256, 320)

Case = collections.namedtuple('Case', 'name k W S records')


def thresholds(cus):
    """The five plan numbers the cases are sized by; a loop goes round again PAST each of them."""
    return {
        # kpal_records.hip:428  grid = min(groups, num_cu * 8), one group = kSmallTpw = 4 tiles for k <= 6 (window_kernels.hpp:51)
        'tiles_k6': 4 * 8 * cus,
        # kpal_records.hip:428  the same grid at k = 7, where kSmallTpw = 1: one tile a group
        'tiles_k7': 8 * cus,
        # kpal_records.hip:432  tiles of more than 2048 bases: grid = min(tiles, num_cu * 4)
        'tiles_long': 4 * cus,
        # count_plan.hpp:119    max_waves = num_cu * blocks_per_cu * waves_per_block, called with (8, 4) at kpal_records.hip:17 and :438
        'wave_steps': cus * 8 * 4,
        # kpal_records.hip:444  threads = num_cu * 2048; segment = max(m, ceil(n * bins / threads)) at :445
        'slide_threads': 2048 * cus,
    }


def ceil_div(a, b):
    return -(-a // b)


# ---- sequences, text, spans ------------------------------------------------------------------------------------------------------
def sequence(rs, n):
    """n bases over ACGTacgt, about one N per N_EVERY of them -> bytes"""
    seq = ALPHABET[rs.randint(0, 8, size=n)]
    if n >= N_EVERY:
        seq[rs.randint(0, n, size=n // N_EVERY)] = ord('N')
    return seq.tobytes()


def fasta_text(records, widths=(61, 10 ** 9, 70, 13)):
    """The records as FASTA text, LF, record r wrapped at widths[r % 4] (none divides a step of the cases)."""
    parts = []
    for r, (title, seq) in enumerate(records):
        parts.append(b'>' + title + b'\n')
        width = min(widths[r % len(widths)], max(len(seq), 1))
        full = len(seq) // width
        lines = np.empty((full, width + 1), dtype=np.uint8)
        lines[:, :width] = np.frombuffer(seq, dtype=np.uint8, count=full * width).reshape(full, width)
        lines[:, width] = ord('\n')
        parts.append(lines.tobytes())
        if len(seq) > full * width:
            parts.append(seq[full * width:] + b'\n')
    text = b''.join(parts)
    assert b'\t\n' not in text        # a tab that ends a line would be stripped
    return text


def win_count(L, W, S):
    """window_index.hpp: win_count"""
    return 0 if L == 0 else 1 if L <= W else ceil_div(L - W, S) + 1


def win_tiles(L, S):
    """window_index.hpp: win_tiles"""
    return ceil_div(L, S)


def window_spans(L, W, S):
    """[start, end) of every window of a record of L bases, enumerated one by one (as tests/test_gpu_windows.py)."""
    out, j = [], 0
    while L > 0:
        out.append((j * S, min(j * S + W, L)))
        if out[-1][1] == L:
            break
        j += 1
    return out


def n_windows(case):
    return sum(win_count(len(seq), case.W, case.S) for _, seq in case.records)


def n_tiles(case):
    return sum(win_tiles(len(seq), case.S) for _, seq in case.records)


def expected(case):
    """int64[n_windows, 4^k]: the oracle's table of every window, record-major.  Not cached: up to 768 MiB."""
    spans = [(seq, a, b) for _, seq in case.records for a, b in window_spans(len(seq), case.W, case.S)]
    assert len(spans) == n_windows(case)
    out = np.empty((len(spans), 4 ** case.k), dtype=np.int64)
    for i, (seq, a, b) in enumerate(spans):
        out[i] = oracle.from_sequences([seq[a:b]], case.k)
    return out


def expected_records(case, k):
    """int64[n_records, 4^k]: the oracle's table of every whole record."""
    return np.stack([oracle.from_sequences([seq], k) for _, seq in case.records])


def stream(case):
    """(the flattened stream as uint8, starts[R + 1]): one '\\n' before the bases of every record."""
    flat = np.frombuffer(b''.join(b'\n' + seq for _, seq in case.records), dtype=np.uint8)
    starts = np.concatenate([[0], np.cumsum([1 + len(seq) for _, seq in case.records])])
    return flat, starts


# ---- what the plans make of a case -----------------------------------------------------------------------------------------------
def lds_tile_members(case, group):
    """window_tiles_lds_kernel, tile by tile: (steps, per, [(member, first byte of its first step, st0, st1)] of the members
    that walk at least one step, e_lo, e_hi).  Restates window_kernels.hpp:77-85."""
    k, S = case.k, case.S
    _, starts = stream(case)
    out = []
    for r, (_, seq) in enumerate(case.records):
        rec_end = int(starts[r + 1])
        for t in range(win_tiles(len(seq), S)):
            a = int(starts[r]) + 1 + t * S
            b = min(a + S, rec_end)
            e_lo, e_hi = a + k - 1, min(b + k - 1, rec_end)
            if e_lo >= e_hi:
                out.append((0, 0, [], e_lo, e_hi))
                continue
            c_lo, c_hi = e_lo // 16, (e_hi + 15) // 16
            steps = ceil_div(c_hi - c_lo, 64)
            per = ceil_div(steps, group)
            walkers = [(mb, (c_lo + mb * per * 64) * 16, mb * per, min(mb * per + per, steps)) for mb in range(group) if mb * per < steps]
            out.append((steps, per, walkers, e_lo, e_hi))
    return out


def carried_kmers(case, group):
    """k-mers that begin in a member's last wave-step and end in the next member's first one, all of their bases in the
    alphabet and their end inside the tile's range: what only the carry loaded at c_lo + st0 * 64 - 1, st0 > 0, delivers."""
    flat, _ = stream(case)
    good = np.isin(flat, ALPHABET)
    found = 0
    for steps, per, walkers, e_lo, e_hi in lds_tile_members(case, group):
        for member, first_byte, st0, st1 in walkers:
            if st0 == 0:
                continue
            for e in range(max(first_byte, e_lo), min(first_byte + case.k - 1, e_hi)):      # ends in the step, begins before it
                found += bool(good[e - case.k + 1:e + 1].all())
    return found


def wave_steps(case):
    """wave-steps of 1024 bytes of the span window_tiles_atomic_kernel and count_records_kernel are fed for ALL windows /
    records of the case: the stream from byte 1 (byte 0 for the records) to its end, chunks counted from 16-byte aligned 0."""
    flat, _ = stream(case)
    return ceil_div(ceil_div(len(flat), 16), 64)


def steps_per_wave(steps, cus):
    """count_plan.hpp:117-123  wave_grid(steps, cus, 8, 4) -> (spw, waves)"""
    max_waves = thresholds(cus)['wave_steps']
    spw = ceil_div(steps, max_waves) if steps > max_waves else 1
    return spw, ceil_div(steps, spw)


def slide_plan(case, cus):
    """kpal_records.hip:444-448 for one call over all windows -> (segment, n_segments, segments a workgroup, workgroups)"""
    n, bins, m = n_windows(case), 4 ** case.k, case.W // case.S
    segment = max(m, ceil_div(n * bins, thresholds(cus)['slide_threads']))
    n_segments = ceil_div(n, segment)
    per_block = 256 // bins if bins < 256 else 1
    return segment, n_segments, per_block, ceil_div(n_segments, per_block) if bins < 256 else n_segments * (bins // 256)


def records_per_segment(case, cus):
    """per segment of the slide: how many records its windows belong to, and how many records WITHOUT windows it passes"""
    segment, n_segments, _, _ = slide_plan(case, cus)
    counts = np.array([win_count(len(seq), case.W, case.S) for _, seq in case.records])
    owner = np.repeat(np.arange(len(counts)), counts)
    held, passed = [], []
    for s in range(n_segments):
        mine = owner[s * segment:(s + 1) * segment]
        held.append(len(np.unique(mine)))
        passed.append(int((counts[mine[0]:mine[-1] + 1] == 0).sum()))
    return np.array(held), np.array(passed)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _records(seed, lengths):
    rs = np.random.RandomState(seed)
    return tuple((b'r%d' % i, sequence(rs, L)) for i, L in enumerate(lengths))


@functools.lru_cache(maxsize=None)
def case_a1():
    """k = 4, W = 4, S = 1: tiles of one base, four to a workgroup; past 32 * CUs tiles, the last group not full."""
    k = 4
    return Case('A1', k, 4, 1, _records(101, [10301, 0, k - 1, k, 9]))


@functools.lru_cache(maxsize=None)
def case_a2():
    """k = 7, W = S = 7: one tile a workgroup of four waves (TPW = 1); past 8 * CUs tiles."""
    k = 7
    return Case('A2', k, 7, 7, _records(102, [2700 * 7 + 3, 0, k - 1, k]))


@functools.lru_cache(maxsize=None)
def case_a3(m):
    """k = 2, S = 2049, W = m * S: the eight-wave kernel; past 4 * CUs tiles."""
    S = 2049
    return Case('A3m%d' % m, 2, m * S, S, _records(103, [1296 * S + 1000, 2 * S + 5, 1]))


@functools.lru_cache(maxsize=None)
def case_b(k):
    """S = 20000, W = 40000: twenty wave-steps a tile over eight member waves: three each, the last member idle."""
    return Case('Bk%d' % k, k, 40000, 20000, _records(104, [90000, 25000]))


@functools.lru_cache(maxsize=None)
def case_c():
    """k = 8, S = 1 MiB, W = 2 MiB: the atomic tile kernel and count_records_kernel at two wave-steps a wave."""
    k = 8
    return Case('C', k, 2 << 20, 1 << 20, _records(105, [(7 << 20) + 5345, 0, k - 1, k, (4 << 20) + 1101]))


# Long records of 50 000 and 25 000 bases, as first planned, give about 27 700 windows and segments of 4 (256 CUs) or 3 (320 CUs)
# windows, which cannot hold the windows of ten records.  A segment of ten needs more than 9 * 2048 * 320 / 64 = 92 160 windows.
D_LONG = (200000, 79000)
D_SHORT = 1500


@functools.lru_cache(maxsize=None)
def case_d():
    """k = 3, W = 6, S = 3: the slide with segments longer than m, four segments a workgroup, over 1500 short records."""
    rs = np.random.RandomState(106)
    # lengths 0 .. 13, three in four of them at most W (one window, or none for 0)
    short = np.where(rs.random_sample(D_SHORT) < 0.75, rs.randint(0, 7, size=D_SHORT), rs.randint(7, 14, size=D_SHORT))
    return Case('D', 3, 6, 3, _records(107, [D_LONG[0]] + short.tolist() + [D_LONG[1]]))


@functools.lru_cache(maxsize=None)
def case_e(k):
    """k = 10, 11, 12 at W = 24, S = 8: the DISPATCH_K_1_16 arms above 9, the trim's kmask and table + (i << 2k)."""
    W, S = 24, 8
    rs = np.random.RandomState(108 + k)
    seq = sequence(rs, W + 2 * S + k)
    pos = W - (k - 1)
    return Case('Ek%d' % k, k, W, S, ((b'tab', seq[:pos] + b'\t' + seq[pos + 1:]), (b'short', sequence(rs, k - 1))))


@functools.lru_cache(maxsize=None)
def case_f():
    """k = 2, W = S = 2049 again, 6001 tiles: every workgroup of the eight-wave kernel makes four trips or more.  Here
    for one reason: the barrier behind the dump orders a RACE (waves 1 .. 3 have nothing to dump at 16 bins and go on to zero h while
    wave 0 still reads it), which loses on about one trip in 500; A3's few hundred later trips are too few to show it."""
    S = 2049
    return Case('F', 2, S, S, _records(109, [6000 * S + 7]))


F_CALLS = 3


def all_cases():
    return [case_a1(), case_a2(), case_a3(1), case_a3(2), case_b(4), case_b(7), case_c(), case_d()] + [case_e(k) for k in (10, 11, 12)] + [case_f()]


# ---- what makes each case mean something: asserted by the host test for CUS and by every GPU test for the device's own count -----
def require_a1(cus):
    tiles = n_tiles(case_a1())
    assert tiles > thresholds(cus)['tiles_k6'], (tiles, cus)      # some workgroup zeroes, counts and dumps a second group
    assert tiles % 4 != 0, tiles                                  # the last group has dead slots


def require_a2(cus):
    case = case_a2()
    assert case.S <= 2048 and n_tiles(case) > thresholds(cus)['tiles_k7'], (n_tiles(case), cus)


def require_a3(m, cus):
    case = case_a3(m)
    assert case.S > 2048 and n_tiles(case) > thresholds(cus)['tiles_long'], (n_tiles(case), cus)


def require_b(k, cus):
    case = case_b(k)
    nominal = ceil_div(case.S + 15, 1024)
    assert ceil_div(nominal, 8) >= 2
    tiles = lds_tile_members(case, 8)
    full = [t for t in tiles if t[0] == nominal]
    assert len(full) >= 4
    for steps, per, walkers, _, _ in full:
        assert per >= 2 and len(walkers) < 8                                          # a member is idle: st0 >= steps
        assert any(st0 > 0 and st1 - st0 >= 2 for _, _, st0, st1 in walkers)          # mid-tile start, then a second step
    assert any(len(t[2]) > 1 and t[2][-1][3] - t[2][-1][2] < t[1] for t in tiles)     # a last walker cut short by `steps`


def require_c(cus):
    steps = wave_steps(case_c())
    assert steps > thresholds(cus)['wave_steps'], (steps, cus)
    spw, waves = steps_per_wave(steps, cus)
    assert spw >= 2 and steps % spw != 0, (spw, steps)            # the tail wave walks fewer steps than the others
    # a record border inside a wave's LATER step: the short records lie behind 7 MiB of the stream
    _, starts = stream(case_c())
    assert any((int(s) // 1024) % spw != 0 for s in starts[1:-1]), (spw, starts)


def require_d(cus):
    case = case_d()
    segment, n_segments, per_block, _ = slide_plan(case, cus)
    assert segment > case.W // case.S, (segment, cus)
    assert per_block == 4 and n_segments % 4 != 0, (per_block, n_segments)            # the last workgroup has segments past the end
    held, passed = records_per_segment(case, cus)
    assert held.max() >= 10, held.max()
    assert passed.max() >= 2, passed.max()                                            # `do ++r while` goes round more than once


def require_e(k):
    case = case_e(k)
    assert n_windows(case) <= 8 and case.records[0][1][case.W - (k - 1)] == 9 and len(case.records[1][1]) == k - 1


def require_f(cus):
    case = case_f()
    assert case.S > 2048 and n_tiles(case) >= 4 * thresholds(cus)['tiles_long'], (n_tiles(case), cus)
