"""The host decisions of the quad record pipelines without a GPU: kpal_amd/csrc/quad_plan.hpp -- the grid and the verdict of the
row-load sample, the tile sizes from the queue model, the tile sizes kept between feeds, the geometry of the launches --
driven by a stand-alone program built with the address and undefined-behaviour sanitizers.  Every expected integer is a
literal worked out by hand from the formulas (the working is in the comments), none is computed with the header; the
floating-point queue model is compared with a restatement in this file."""
import math
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'kpal_amd', 'csrc')
ONE_LEVEL = (8, 7, 6, 4, 3, 2, 1)   # kpal_quads.hip: candidates
TWO_LEVEL = (8, 7, 6, 3)            # kpal_quads2.hip: candidates
LEVEL2 = (8, 7, 6, 4, 3, 2)         # quad_plan.hpp: kQuadCandidates2


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('quad_plan') / 'quad_plan_check')
    b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-o', exe,
                        os.path.join(ROOT, 'tests', 'native', 'quad_plan_check.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0 and not b.stdout.strip(), b.stdout.decode()[-3000:]

    def ask(queries):
        """[query words] -> the answers, one list of numbers (int, or float where the program printed one) per query"""
        text = ''.join(' '.join(w if isinstance(w, str) else repr(w) for w in q) + '\n' for q in queries)
        r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0 and got[-2] == 'QUAD_PLAN_DONE %d' % len(queries), got[-20:]
        return [[int(w) if re.fullmatch(r'-?\d+', w) else float(w) for w in line.split()] for line in got[:len(queries)]]

    def check(cases):
        """[(query words, expected integers)]"""
        for (q, want), have in zip(cases, ask([q for q, _ in cases])):
            assert tuple(have) == tuple(want), (q, have, want)
    ask.check = check
    return ask


def test_constants_are_defined_once():
    """The kernels, the launchers and this file mean the same rows, records and candidates."""
    text = {f: open(os.path.join(CSRC, f)).read() for f in ('quad_plan.hpp', 'quad_kernels.hpp', 'kpal_host.hpp', 'kpal_quads.hip', 'kpal_quads2.hip')}
    for name, value in (('kQuadRowWords', '32768'), ('kQuadPackedRecordBytes', '192'), ('kQuadBacklogMax', '1500.0')):
        assert re.search(r'constexpr \w+ %s = %s;' % (name, re.escape(value)), text['quad_plan.hpp']), name
        assert not any(re.search(r'constexpr \w+ %s\b' % name, t) for f, t in text.items() if f != 'quad_plan.hpp'), name
    assert '#include "quad_plan.hpp"' in text['quad_kernels.hpp'] and '#include "quad_plan.hpp"' in text['kpal_host.hpp']
    assert 'hip' not in re.sub(r'//.*', '', text['quad_plan.hpp']).lower() and 'kpal_ctx' not in text['quad_plan.hpp']
    assert 'candidates[] = {%s}' % ', '.join(map(str, ONE_LEVEL)) in text['kpal_quads.hip']
    assert 'candidates[] = {%s}' % ', '.join(map(str, TWO_LEVEL)) in text['kpal_quads2.hip']
    assert 'kQuadCandidates2[] = {%s}' % ', '.join(map(str, LEVEL2)) in text['quad_plan.hpp']


def test_sample_grid(plan):
    # want = max(1, total / 2048) workgroups (8 waves x 4 steps x 64: 1/64 of the piece), at most 1024; stride = max(32, total / groups);
    # sampled = min(32 groups, total)
    plan.check([(('grid', 1000000), (488, 2049, 4, 15616)),        # 1e6 / 2048 = 488.3; 1e6 / 488 = 2049.2; 488 x 32
                (('grid', 10), (1, 32, 4, 10)),
                (('grid', 0), (1, 32, 4, 0)),                      # want = max(1, 0); stride = max(32, 0); min(32, 0)
                (('grid', 1), (1, 32, 4, 1)),
                (('grid', 2047), (1, 2047, 4, 32)),                # still one workgroup, the stride is the piece
                (('grid', 4096), (2, 2048, 4, 64)),
                (('grid', 2048 * 1024), (1024, 2048, 4, 32768)),
                (('grid', 4000000), (1024, 3906, 4, 32768))])      # 1953 wanted, 1024 at most; 4e6 / 1024 = 3906.25


def test_one_level_geometry(plan):
    # tiles = ceil(total / (16 steps)); G = min(CUs, tiles); tpb = ceil(tiles / G); pool = 128 KiB x G x tpb; too large: tpb > 0xFFFFFF
    plan.check([(('geo1', 1000000, 8, 256), (0, 7813, 256, 31, 1040187392)),     # 1e6 / 128 = 7812.5; 7813 / 256 = 30.5; 131072 x 256 x 31
                (('geo1', 5, 1, 256), (0, 1, 1, 1, 131072)),                     # a one-tile piece
                (('geo1', 1000000, 7, 256), (0, 8929, 256, 35, 1174405120)),     # 1e6 / 112 = 8928.6; 8929 / 256 = 34.9; 131072 x 256 x 35
                (('geo1', 1000, 8, 256), (0, 8, 8, 1, 1048576)),                 # fewer tiles than CUs
                # one CU, one step per tile: tpb = tiles = total / 16.  0xFFFFFF x 16 = 268435440; pool 2^17 x (2^24 - 1) = 2^41 - 2^17
                (('geo1', 268435440, 1, 1), (0, 16777215, 1, 16777215, 2199023124480)),
                (('geo1', 268435441, 1, 1), (1, 16777216, 1, 16777216, 2199023255552))])


def test_two_level_geometry(plan):
    # NB1 = 4^(k-11) coarse buckets, REP = 256 / NB1 replicas (at least 1), S1 = 32768 / (NB1 REP) slots; tiles1 = ceil(total / (16 steps1)),
    # G1 = min(CUs, 256, tiles1), tpb1 = ceil(tiles1 / G1), cap1 = tpb1 + 1 rounded up to 1024 / (4 S1) records, pool1 = 128 KiB x G1 x cap1;
    # units = REP G1, G2 = min(units, 4 CUs / NB1) (at least 1), upw = ceil(units / G2), G2 = ceil(units / upw), unit_cap = 4 S1 cap1,
    # tiles2 = ceil(upw unit_cap / (16 KiB x steps2)), cap2 = tiles2 + 1, pool2 = 512 x 192 x NB1 x G2 x cap2, nseg = G1 + G2 NB1 + 1
    plan.check([
        # k = 13: 1e6 / 112 = 8928.6; 8929 / 256 = 34.9; cap1 = 36 (pairs); 4096 units over 1024 / 16 = 64 workgroups; 36 x 512 = 18432;
        # 64 x 18432 / 98304 = 12; 98304 x 16 x 64 x 13
        (('geo2', 13, 1000000, 7, 6, 256), (0, 16, 16, 128, 8929, 256, 35, 36, 1207959552, 0, 4096, 64, 64, 18432, 12, 13, 1308622848, 1281)),
        # k = 14: 64 x 4 rows; 1024 units over 1024 / 64 = 16 workgroups
        (('geo2', 14, 1000000, 7, 6, 256), (0, 64, 4, 128, 8929, 256, 35, 36, 1207959552, 0, 1024, 16, 64, 18432, 12, 13, 1308622848, 1281)),
        # k = 15: 256 x 1 rows; 256 units over 4 workgroups
        (('geo2', 15, 1000000, 7, 6, 256), (0, 256, 1, 128, 8929, 256, 35, 36, 1207959552, 0, 256, 4, 64, 18432, 12, 13, 1308622848, 1281)),
        # k = 16: 1024 rows of 32 slots, eight records per KiB: cap1 = 36 -> 40; 256 units in one workgroup; 40 x 128 = 5120;
        # 256 x 5120 / 98304 = 13.3; 98304 x 1024 x 1 x 15
        (('geo2', 16, 1000000, 7, 6, 256), (0, 1024, 1, 32, 8929, 256, 35, 40, 1342177280, 0, 256, 1, 256, 5120, 14, 15, 1509949440, 1281)),
        # a one-tile piece: cap1 = 2; 16 units, one per workgroup; 2 x 512 = 1024 bytes are one tile of level 2; 98304 x 16 x 16 x 2
        (('geo2', 13, 5, 8, 8, 256), (0, 16, 16, 128, 1, 1, 1, 2, 262144, 0, 16, 16, 1, 1024, 1, 2, 50331648, 258)),
        # one CU, three steps per tile: tpb1 = tiles1 = total / 48.  0xFFFF x 48 = 3145680: cap1 = 65536, pool1 = 2^17 x 2^16; level 2: 16 units
        # in one workgroup (4 CUs / 16 = 0 -> 1), 65536 x 512 = 2^25 each, 2^29 / 32768 = 16384 tiles; 98304 x 16 x 16385; 1 + 16 + 1
        (('geo2', 13, 3145680, 3, 2, 1), (0, 16, 16, 128, 65535, 1, 65535, 65536, 8589934592, 0, 16, 1, 16, 33554432, 16384, 16385, 25771376640, 18)),
        # ... one tile more: too large.  cap1 = 65538; 16 x 65538 x 512 / 32768 = 16384.5
        (('geo2', 13, 3145681, 3, 2, 1), (1, 16, 16, 128, 65536, 1, 65536, 65538, 8590196736, 0, 16, 1, 16, 33555456, 16385, 16386, 25772949504, 18)),
        # upw x unit_cap >= 2^32: on 256 CUs upw = 64 and unit_cap = 512 cap1, so from cap1 = 131072 -- beyond the tpb1 bound, which the
        # launcher checks first (level 2 is a function of its own).  tpb1 = 131069: cap1 = 131070, 64 x 131070 x 512 = 2^32 - 65536;
        # tiles1 = 256 x 131069 = 33553664 = total / 48; 4294901760 / 131072 = 32767.5; 98304 x 16 x 64 x 32769
        (('geo2', 13, 1610575872, 3, 8, 256),
         (1, 16, 16, 128, 33553664, 256, 131069, 131070, 4397979402240, 0, 4096, 64, 64, 67107840, 32768, 32769, 3298635546624, 1281)),
        # ... one tile more: tpb1 = 131070, cap1 = 131072: exactly 2^32
        (('geo2', 13, 1610575920, 3, 8, 256),
         (1, 16, 16, 128, 33553665, 256, 131070, 131072, 4398046511104, 1, 4096, 64, 64, 67108864, 32768, 32769, 3298635546624, 1281))])


def _verdict(plan, rows, fine=(), repeat_items=0, sampled=1, is_auto=1):
    a, = plan([('verdict', len(rows), len(fine), repeat_items, sampled, is_auto) + tuple(rows) + tuple(fine)])
    return dict(zip(('use_chunked', 'budget', 'hot_rows', 'hot_percent', 'top3_percent', 'n', 'first', 'last', 'sorted', 'nfine', 'fine_first',
                     'fine_last', 'fine_sorted'), a))


def test_sample_verdict(plan):
    # counters are 16 x the load, 16 sampled steps: the loads are exact
    v = _verdict(plan, [16] * 512, sampled=16)
    assert (v['use_chunked'], v['budget'], v['hot_rows'], v['hot_percent'], v['top3_percent']) == (0, 1500, 0, 0, 0)
    assert (v['n'], v['first'], v['last'], v['sorted'], v['nfine']) == (480, 1, 1, 1, 0)
    # 500 rows at 1, twelve at 3: the excess over the median row is 12 x 2 = 24 of 536 items (4.48 % > 1.5 %), the top three hold 6 (25 % < 80 %)
    rows = [16] * 250 + [48] * 12 + [16] * 250
    for is_auto in (1, 0):
        v = _verdict(plan, rows, sampled=16, is_auto=is_auto)
        assert (v['use_chunked'], v['budget'], v['hot_rows']) == (is_auto, 375, 1)
        assert v['hot_percent'] == pytest.approx(100 * 24 / 536, rel=1e-12) and v['top3_percent'] == pytest.approx(25, rel=1e-12)
        assert (v['n'], v['first'], v['last'], v['sorted']) == (480, 1, 1, 1)      # the twelve are among the 32 left out
    # 509 rows at 1, three at 5: 12 of 524 (2.29 %), all of it in three rows: the quads keep the feed
    v = _verdict(plan, [80] + [16] * 509 + [80, 80], sampled=16)
    assert (v['use_chunked'], v['budget'], v['hot_rows'], v['top3_percent']) == (0, 375, 1, 100)
    assert v['hot_percent'] == pytest.approx(100 * 12 / 524, rel=1e-12)
    # all-zero counters; repeat lanes alone
    v = _verdict(plan, [0] * 512, sampled=16)
    assert (v['use_chunked'], v['budget'], v['hot_rows'], v['hot_percent'], v['top3_percent'], v['n'], v['first'], v['last']) == (0, 1500, 0, 0, 0, 480, 0, 0)
    assert _verdict(plan, [0] * 512, repeat_items=5, sampled=16)['hot_rows'] == 1
    # the k = 12 shape: 2048 rows at 1, forty of them at 3 -- 32 are left out, eight stay; excess 32 x 2 = 64 of 2008 + 120 = 2128 items (3 %)
    v = _verdict(plan, ([8] * 50 + [24]) * 40 + [8] * 8, sampled=8)
    assert (v['use_chunked'], v['budget'], v['hot_rows'], v['n'], v['first'], v['last'], v['sorted']) == (1, 375, 1, 2016, 1, 3, 1)
    assert v['hot_percent'] == pytest.approx(100 * 64 / 2128, rel=1e-12) and v['top3_percent'] == pytest.approx(100 * 6 / 64, rel=1e-12)
    # the two-level shape: 256 rows and the 512 fine rows, handed back sorted and whole
    v = _verdict(plan, [32] * 256, fine=[(7 * i) % 512 + 16 for i in range(512)], sampled=16)
    assert (v['use_chunked'], v['budget'], v['hot_rows'], v['n'], v['first'], v['last']) == (0, 1500, 0, 224, 2, 2)
    assert (v['nfine'], v['fine_first'], v['fine_last'], v['fine_sorted']) == (512, 1, 527 / 16, 1)


def test_sample_verdict_thresholds(plan):
    # 512 rows at 1000 (one sampled step), one of them e higher: the excess e sits in one row (concentrated: never handed over) and
    # passes 0.3 % when e > 0.003 (512000 + e), e > 1540.6
    for e, hot in ((1540, 0), (1541, 1)):
        v = _verdict(plan, [1000] * 511 + [1000 + e])
        assert (v['use_chunked'], v['budget'], v['hot_rows']) == (0, 375 if hot else 1500, hot), e
    # twelve rows e higher (the top three hold a quarter): 12 e > 0.015 (512000 + 12 e), e > 649.7
    for e, chunked in ((649, 0), (650, 1)):
        v = _verdict(plan, [1000] * 500 + [1000 + e] * 12)
        assert (v['use_chunked'], v['budget'], v['hot_rows']) == (chunked, 375, 1), e
        assert _verdict(plan, [1000] * 500 + [1000 + e] * 12, is_auto=0)['use_chunked'] == 0
    # repeat lanes: r > 0.001 (512000 + r), r > 512.5 -- REPEAT without a smaller budget
    for r, hot in ((512, 0), (513, 1)):
        v = _verdict(plan, [1000] * 512, repeat_items=r)
        assert (v['use_chunked'], v['budget'], v['hot_rows']) == (0, 1500, hot), r


def test_tile_cache(plan):
    # one run of the program, one cache: hit FEED_BYTES LEVELS -> 0 | 1; store / hot / clear -> steps1 steps2 uses bytes hot_rows
    plan.check([(('hit', 1000, 1), (0,)),                                    # nothing kept
                (('store', 7, 0, 1000), (7, 0, 0, 1000, 0)),                 # feed 1 is sampled
                (('hit', 2001, 1), (0,)), (('hit', 499, 1), (0,))]           # above twice, below half: a miss uses nothing up
               + [(('hit', 1000, 1), (1,))] * 16                             # feeds 2 .. 17
               + [(('hit', 1000, 1), (0,)),                                  # the 18th
                  (('store', 6, 0, 1000), (6, 0, 0, 1000, 0)),
                  (('hit', 2000, 1), (1,)), (('hit', 500, 1), (1,)), (('hit', 2001, 1), (0,)), (('hit', 499, 1), (0,)),
                  (('hit', 1000, 2), (0,)), (('hit', 1000, 1), (1,)),        # level 1 alone does not serve two levels
                  (('hot', 1), (6, 0, 3, 1000, 1)),
                  (('store', 7, 6, 3000), (7, 6, 0, 3000, 1)),               # the verdict is the last sample's, not the store's
                  (('hit', 3000, 2), (1,)), (('hit', 3000, 1), (1,)),
                  (('clear',), (0, 0, 0, 0, 0)),
                  (('hit', 3000, 1), (0,)), (('hit', 3000, 2), (0,)), (('hit', 0, 1), (0,))])


def test_forced_sizes_and_repeat(plan):
    plan.check([(('forced', 7, 4) + TWO_LEVEL, (7,)), (('forced', 4, 4) + TWO_LEVEL, (0,)), (('forced', 4, 7) + ONE_LEVEL, (4,)),
                (('forced', 0, 7) + ONE_LEVEL, (0,)), (('forced', 5, 7) + ONE_LEVEL, (0,)), (('forced', 1, 6) + LEVEL2, (0,)),
                # tile1 STEPS SAMPLED HOT_ROWS KPAL_QUAD_STEPS KPAL_QUAD_REPEAT -> steps, REPEAT, counted as a REPEAT piece
                (('tile1', 8, 0, 0, 8, -1), (8, 1, 1)),      # forced: no sample, REPEAT
                (('tile1', 8, 0, 0, 8, 0), (8, 0, 0)),       # ... unless KPAL_QUAD_REPEAT=0
                (('tile1', 7, 0, 1, 7, -1), (7, 1, 0)),      # forced seven stay seven (no REPEAT instantiation: not counted)
                (('tile1', 7, 1, 1, 0, -1), (6, 1, 1)),      # sampled seven with hot rows: six
                (('tile1', 7, 1, 0, 0, -1), (7, 0, 0)),
                (('tile1', 8, 1, 1, 0, -1), (8, 1, 1)),
                (('tile1', 7, 0, 1, 0, -1), (6, 1, 1)),      # kept seven, the kept verdict
                (('tile1', 8, 0, 0, 0, -1), (8, 0, 0)),
                (('tile1', 8, 0, 0, 5, -1), (8, 1, 1)),      # KPAL_QUAD_STEPS=5 forces no size, but a kept size then runs REPEAT
                (('tile1', 8, 1, 0, 5, -1), (8, 0, 0)),      # ... a sampled one goes by its sample
                (('tile1', 7, 1, 0, 0, 1), (6, 1, 1)),       # KPAL_QUAD_REPEAT=1
                (('tile1', 7, 1, 0, 5, 1), (7, 1, 0)),
                # tile2 FORCED1 CHOSEN HOT_ROWS KPAL_QUAD_REPEAT
                (('tile2', 0, 7, 1, -1), (7, 1, 0)), (('tile2', 0, 8, 1, -1), (8, 1, 1)), (('tile2', 6, 8, 0, -1), (6, 0, 0)),
                (('tile2', 0, 8, 0, 1), (8, 1, 1)), (('tile2', 0, 8, 1, 0), (8, 0, 0)), (('tile2', 3, 7, 1, -1), (3, 1, 1))])


# ---- the queue model, restated: same recurrence, same table (quad_plan.hpp: quad_expected_backlog)
RHO = (0.5, 0.6, 0.7, 0.75, 0.8, 0.85, 0.9, 0.925, 0.95, 0.975)
RATIO = ((1.02, 1.08, 1.25, 1.43, 1.70, 2.19, 3.21, 4.24, 6.34, 12.7),
         (1.00, 1.01, 1.08, 1.17, 1.33, 1.65, 2.34, 3.05, 4.52, 8.9),
         (1.00, 1.00, 1.01, 1.04, 1.12, 1.30, 1.75, 2.24, 3.25, 6.35),
         (1.00, 1.00, 1.00, 1.02, 1.02, 1.10, 1.36, 1.68, 2.37, 4.55))


def row_backlog(m, slots):
    """One row (a queue with Poisson(m) arrivals and `slots` departures per round): its expected backlog."""
    if m <= 0:
        return 0.0
    rho = m / slots
    if rho >= 0.995:
        return 1e6
    p, over = math.exp(-m), 0.0
    for x in range(1, int(m + 12 * math.sqrt(m) + 40) + 1):
        p *= m / x
        if x > slots:
            over += (x - slots) * p
    ratio = RATIO[0 if slots <= 24 else 1 if slots <= 32 else 2 if slots <= 64 else 3]
    if rho >= RHO[-1]:
        return max(over * ratio[-1], m / (2 * (slots - m)))
    if rho <= RHO[0]:
        return over
    j = max(i for i in range(9) if rho > RHO[i])
    return over * (ratio[j] + (rho - RHO[j]) / (RHO[j + 1] - RHO[j]) * (ratio[j + 1] - ratio[j]))


def backlog(mu, slots):
    """Sorted loads; rows within 1 % of the first of their group are evaluated once, at the group's mid-point."""
    total, at = 0.0, 0
    while at < len(mu):
        end = at + 1
        while end < len(mu) and mu[end] <= mu[at] * 1.01:
            end += 1
        total += row_backlog(0.5 * (mu[at] + mu[end - 1]), slots) * (end - at)
        at = end
    return total


FILLS = [0.3 + 0.05 * i for i in range(16)]   # 0.3 .. 1.05


def test_expected_backlog(plan):
    cases = []
    for slots in (16, 20, 32, 64, 128):
        for fill in FILLS:
            cases.append((slots, [fill * slots]))                                                # one row
            cases.append((slots, [fill * slots * (1 + 0.002 * j) for j in range(40)]))           # near-equal rows: groups of 1 %
        cases.append((slots, sorted([0.0, 0.0] + [f * slots for f in FILLS] * 3)))                # empty rows, every branch in one sum
        cases.append((slots, [0.99 * slots, 0.9949 * slots, 0.9951 * slots, 1.2 * slots]))       # either side of "cannot keep up"
    got = plan([('backlog', slots, len(mu)) + tuple(mu) for slots, mu in cases])
    saw_heavy = saw_full = 0
    for (slots, mu), (have,) in zip(cases, got):
        want = backlog(mu, slots)
        assert have == pytest.approx(want, rel=1e-9, abs=0), (slots, mu[:3], have, want)
        saw_heavy += any(0.975 <= m / slots < 0.995 for m in mu)
        saw_full += want >= 1e6
    assert saw_heavy and saw_full and backlog([], 16) == 0
    assert plan([('backlog', 64, 0)])[0] == [0]


def walk(loads, slots, candidates, budget):
    """-> (steps, the backlog of every candidate tried); every deciding figure at least 5 % away from the budget"""
    tried = []
    for c in candidates:
        tried.append(backlog([v * 16 * c for v in loads], slots))
        assert abs(tried[-1] - budget) >= 0.05 * budget, (c, tried[-1], budget)
        if tried[-1] <= budget:
            return c, tried
    return candidates[-1], tried


def walk2(fine, steps1):
    total = sum(fine)
    f1 = min(1.0, total * 16.0 * steps1 / 32768)
    for c in LEVEL2:
        b = backlog([v / total * (256.0 * f1) * 16 * c if total > 0 else 0.0 for v in fine[:-32]], 64)
        assert abs(b - 1500) >= 75, (c, b)
        if b <= 1500:
            return c
    return 2


# (loads per row and wave-step -- sorted, the 32 fullest rows already left out --, slots, candidates, budget, the size expected: the
# restatement's).  The uniform shapes were seen on an MI355X with 256 MiB of uniform 150-base reads, same sizes: k = 12 eight steps
# (backlog 698 logged, 731 here), k = 10 seven (4225 and 165 logged), k = 13 seven next to a 375 budget (580 and 11 logged), k = 15 eight.
WALKS = [
    ([0.119] * 2016, 20, ONE_LEVEL, 1500, 8),                       # k = 12, uniform reads: 0.119 x 16 x 8 = 15.2 of 20
    ([0.119] * 2016, 20, ONE_LEVEL, 375, 7),                        # ... next to hot rows
    ([0.476] * 480, 64, ONE_LEVEL, 1500, 7),                        # k <= 11, uniform: eight steps would bring 61 of 64
    ([0.95] * 224, 128, TWO_LEVEL, 1500, 8),                        # k = 13 .. 15, uniform: 122 of 128
    ([0.95] * 224, 128, TWO_LEVEL, 375, 7),
    ([0.2375] * 992, 32, TWO_LEVEL, 1500, 7),                       # k = 16
    ([0.2] * 380 + [2.5] * 100, 64, ONE_LEVEL, 1500, 1),            # skewed: 100 rows take 80 of 64 in two steps, 40 in one
    ([0.4] * 164 + [1.5] * 60, 128, TWO_LEVEL, 1500, 3),            # skewed: 144 of 128 in six steps, 72 in three
    ([0.4] * 164 + [3.0] * 60, 128, TWO_LEVEL, 1500, 3),            # ... 144 of 128 even in three: the smallest there is
]


def test_level1_walk(plan):
    got = plan([('walk1', slots, float(budget), len(cand)) + tuple(cand) + (len(loads),) + tuple(loads) for loads, slots, cand, budget, _ in WALKS])
    for (loads, slots, cand, budget, expected), have in zip(WALKS, got):
        steps, tried = walk(loads, slots, cand, budget)
        assert steps == expected == have[0] and have[1] == len(tried), (slots, cand, budget, have, steps, tried)
        assert have[2:] == pytest.approx(tried, rel=1e-9), (slots, have, tried)


# (items per fine row and wave-step of input -- sorted, all 512 --, steps1, the size expected: the restatement's; seen on an MI355X
# with uniform reads: k = 13 (7, 8), k = 15 (8, 8))
WALKS2 = [
    ([234 / 512] * 512, 7, 8),                                       # k = 13, uniform: f1 = 0.80, a fine row gets 51 of 64 in eight steps
    ([230.5 / 512] * 512, 8, 8),                                     # k = 15: f1 = 0.90, 58 of 64
    ([243 / 512] * 512, 8, 7),                                       # longer reads: f1 = 0.95, 61 of 64
    ([0.2 * 243 / 272] * 272 + [0.8 * 243 / 240] * 240, 8, 4),       # 240 fine rows share 80 % of the items
    ([0.015 * 243 / 332] * 332 + [0.985 * 243 / 180] * 180, 8, 2),   # 180 share 98.5 %: 64 of 64 in three steps, the smallest size
    ([0.0] * 512, 8, 8),                                             # an empty sample
]


def test_level2_walk(plan):
    got = plan([('walk2', steps1, len(fine)) + tuple(fine) for fine, steps1, _ in WALKS2])
    for (fine, steps1, expected), (have,) in zip(WALKS2, got):
        assert walk2(fine, steps1) == expected == have, (steps1, fine[0], fine[-1], have)
    assert plan([('walk2', 7, 0)])[0] == [8]                         # no fine loads at all
