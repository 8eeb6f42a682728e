"""The host decisions of the counting front end without a GPU: kpal_amd/csrc/count_plan.hpp -- which pipeline a piece of a
feed takes (the AUTO rule of DESIGN.md section 4), how large a piece is, the grid of a wave-per-range launch -- driven by a
stand-alone program built with the address and undefined-behaviour sanitizers.  Every expected value is a literal written
down from the rule, none is computed with the header."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'kpal_amd', 'csrc')

# include/kpal_hip.h: KPAL_STRATEGY_*
AUTO, ATOMIC, LDS, PART, PART2, CHUNKED, QUADS, QUADS2 = 0, 1, 2, 3, 4, 5, 6, 7
# count_plan.hpp: the strategy does not serve this k
NEEDS_LDS_K, NEEDS_ONE_LEVEL_K, NEEDS_TWO_LEVEL_K = -1, -2, -3
# chunk_kernels.hpp / partition_kernels.hpp: kChunkIdBits, kChunkKeys, kNumBuckets, kStepsPerBlockQuantum
LIMITS = (20, 4096, 512, 24)
KiB, MiB, GiB = 1 << 10, 1 << 20, 1 << 30


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('count_plan') / 'count_plan_check')
    b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-o', exe,
                        os.path.join(ROOT, 'tests', 'native', 'count_plan_check.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0 and not b.stdout.strip(), b.stdout.decode()[-3000:]

    def ask(queries):
        """[(query words, expected answer)] -> asserts every answer"""
        text = ''.join(' '.join(str(int(w)) if not isinstance(w, str) else w for w in q) + '\n' for q, _ in queries)
        r = subprocess.run([exe] + [str(v) for v in LIMITS], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0 and got[-2] == 'COUNT_PLAN_DONE %d' % len(queries), got[-20:]
        for (q, want), line in zip(queries, got):
            have = tuple(int(w) for w in line.split())
            assert have == (want if isinstance(want, tuple) else (want,)), (q, have, want)
    return ask


def test_limits_are_the_kernel_headers():
    """LIMITS above are what kpal_count.hip fills PlanLimits with: the constants of the kernel headers."""
    def const(header, name):
        m = re.search(r'constexpr \w+ %s = ([^;]+);' % name, open(os.path.join(CSRC, header)).read())
        assert m, name
        return m.group(1).strip()
    assert const('chunk_kernels.hpp', 'kChunkIdBits') == '20'
    assert (const('chunk_kernels.hpp', 'kChunkShift'), const('chunk_kernels.hpp', 'kChunkKeys')) == ('12', '1u << kChunkShift')
    assert (const('partition_kernels.hpp', 'kPartBits'), const('partition_kernels.hpp', 'kNumBuckets')) == ('9', '1 << kPartBits')
    assert (const('partition_kernels.hpp', 'kScatterThreads'), const('partition_kernels.hpp', 'kScatterWaves'),
            const('partition_kernels.hpp', 'kScatterSteps'), const('partition_kernels.hpp', 'kStepsPerBlockQuantum')) == \
        ('512', 'kScatterThreads / 64', '3', 'kScatterWaves * kScatterSteps')
    assert LIMITS == (20, 1 << 12, 1 << 9, 512 // 64 * 3)
    source = open(os.path.join(CSRC, 'kpal_count.hip')).read()
    assert 'kPlanLimits = {kChunkIdBits, kChunkKeys, kNumBuckets, kStepsPerBlockQuantum}' in source


def test_plan_resolve(plan):
    q = [(('resolve', AUTO, 1), LDS), (('resolve', AUTO, 7), LDS), (('resolve', AUTO, 8), QUADS), (('resolve', AUTO, 12), QUADS),
         (('resolve', AUTO, 13), QUADS2), (('resolve', AUTO, 16), QUADS2),
         (('resolve', LDS, 7), LDS), (('resolve', LDS, 8), NEEDS_LDS_K)]
    for s in (PART, CHUNKED, QUADS):
        q += [(('resolve', s, 7), NEEDS_ONE_LEVEL_K), (('resolve', s, 13), NEEDS_ONE_LEVEL_K), (('resolve', s, 8), s), (('resolve', s, 12), s)]
    for s in (PART2, QUADS2):
        q += [(('resolve', s, 12), NEEDS_TWO_LEVEL_K), (('resolve', s, 13), s), (('resolve', s, 16), s)]
    q += [(('resolve', ATOMIC, k), ATOMIC) for k in (1, 8, 16)]
    plan(q)


def test_plan_strategy_auto_one_level(plan):
    q = []
    for k in range(8, 13):   # resolved: quads
        q += [(('strategy', QUADS, 1, k, 1 << 18, 0), ATOMIC), (('strategy', QUADS, 1, k, (1 << 18) + 1, 0), CHUNKED),
              (('strategy', QUADS, 1, k, (1 << 25) - 1, 0), CHUNKED), (('strategy', QUADS, 1, k, 1 << 25, 0), QUADS),
              (('strategy', QUADS, 1, k, 1, 0), ATOMIC), (('strategy', QUADS, 1, k, 20 * GiB, 1), QUADS)]
    for k in (1, 7):         # resolved: LDS-direct at every size
        q += [(('strategy', LDS, 1, k, 1, 0), LDS), (('strategy', LDS, 1, k, 1 << 18, 0), LDS), (('strategy', LDS, 1, k, 1 << 30, 0), LDS)]
    plan(q)


def test_plan_strategy_explicit_is_kept(plan):
    q = []
    for n in (1, 16, 1 << 18, (1 << 18) + 1, 1 << 25, 64 * MiB - 1, 13 * GiB):
        for fresh in (0, 1):
            q += [(('strategy', QUADS, 0, 12, n, fresh), QUADS), (('strategy', CHUNKED, 0, 8, n, fresh), CHUNKED),
                  (('strategy', PART, 0, 9, n, fresh), PART), (('strategy', QUADS2, 0, 13, n, fresh), QUADS2),
                  (('strategy', QUADS2, 0, 16, n, fresh), QUADS2), (('strategy', PART2, 0, 14, n, fresh), PART2),
                  (('strategy', ATOMIC, 0, 16, n, fresh), ATOMIC), (('strategy', LDS, 0, 5, n, fresh), LDS)]
    plan(q)


def test_plan_strategy_auto_two_level(plan):
    q = []
    # (k, fresh candidate) -> the feed from which the two-level quads take it: max(64 MiB, 4^k / 8) or max(64 MiB, 3 * 4^k)
    thresholds = {(13, 0): 192 * MiB, (13, 1): 64 * MiB, (14, 0): 768 * MiB, (14, 1): 64 * MiB, (15, 0): 3 * GiB, (15, 1): 128 * MiB,
                  (16, 0): 12 * GiB, (16, 1): 512 * MiB}
    for (k, fresh), t in thresholds.items():
        q += [(('strategy', QUADS2, 1, k, t - 1, fresh), PART2), (('strategy', QUADS2, 1, k, t, fresh), QUADS2),
              (('strategy', QUADS2, 1, k, (1 << 18) + 1, fresh), PART2), (('strategy', QUADS2, 1, k, 20 * GiB, fresh), QUADS2),
              (('strategy', QUADS2, 1, k, 1 << 18, fresh), ATOMIC), (('strategy', QUADS2, 1, k, 16, fresh), ATOMIC)]
    plan(q)


def test_plan_piece_bytes(plan):
    n = 3 * GiB + 5   # (the feed: only a strategy without a bound of its own looks at it)
    q = [(('piece', QUADS, 12, n, 256, 1 * GiB, 0), 16 * GiB), (('piece', QUADS, 12, n, 256, 1 * MiB, 1), 1 * MiB),
         (('piece', QUADS, 12, n, 256, 20 * GiB, 1), 16 * GiB),
         (('piece', QUADS2, 14, n, 256, 1 * GiB, 0), 16 * GiB), (('piece', QUADS2, 14, n, 256, 1 * MiB, 1), 16 * MiB),
         (('piece', QUADS2, 14, n, 256, 2 * GiB, 1), 16 * GiB),
         # k = 13: min(4 batch_bytes, 0xF0000000) & ~15; k = 14..16: min(16 batch_bytes, 16 GiB); set or not
         (('piece', PART2, 13, n, 256, 1 * GiB, 0), 0xF0000000), (('piece', PART2, 13, n, 256, 1 * MiB, 1), 4 * MiB),
         (('piece', PART2, 13, n, 256, 1000, 1), 4000 - 4000 % 16), (('piece', PART2, 13, n, 256, 0x3C000000, 0), 0xF0000000),
         (('piece', PART2, 13, n, 256, 0x3BFFFFFF, 0), 0xEFFFFFF0),
         (('piece', PART, 10, n, 256, 1 * GiB, 0), 1 * GiB), (('piece', PART, 10, n, 256, 12345, 1), 12336), (('piece', PART, 10, n, 256, 7, 1), 16),
         (('piece', LDS, 5, n, 256, 1 * GiB, 0), 1 << 31), (('piece', LDS, 5, n, 256, 1 * MiB, 1), 1 << 31),
         # chunked on 256 CUs: G = 512 workgroups, r_max = (2^20 - 1) // 512 = 2047 chunks each, of which 2 * 512 + 64 = 1088 are fixed;
         # (2047 - 1088) * 4 = 3836 steps, less the margin of 48: 3788, down to a multiple of 24: 3768; a step is 1 KiB of input
         (('piece', CHUNKED, 12, n, 256, 1 * GiB, 0), 1975517184), (('piece', CHUNKED, 12, n, 256, 1 * MiB, 1), 1 * MiB),
         (('piece', CHUNKED, 12, n, 256, 4 * GiB, 1), 1975517184),
         # ... and on 8 CUs: G = 16, r_max = 65535, (65535 - 1088) * 4 = 257788, - 48 = 257740, to 24: 257736; x 16 KiB
         (('piece', CHUNKED, 8, n, 8, 1 * GiB, 0), 257736 * 16 * KiB),
         # global atomics: the feed itself, down to a multiple of 16 (at least 16)
         (('piece', ATOMIC, 9, 1 << 18, 256, 1 * GiB, 0), 1 << 18), (('piece', ATOMIC, 9, 100, 256, 1 * GiB, 0), 96), (('piece', ATOMIC, 9, 5, 256, 1 * GiB, 0), 16)]
    for k in (14, 15, 16):
        q += [(('piece', PART2, k, n, 256, 1 * GiB, 0), 16 * GiB), (('piece', PART2, k, n, 256, 1 * MiB, 1), 16 * MiB),
              (('piece', PART2, k, n, 256, 100, 1), 1600)]
    assert 3768 * 512 * 1024 == 1975517184
    plan(q)


def test_wave_grid(plan):
    plan([(('grid', 0, 256, 8, 4), (1, 0)), (('grid', 1, 256, 8, 4), (1, 1)), (('grid', 8192, 256, 8, 4), (1, 2048)),
          (('grid', 8193, 256, 8, 4), (2, 1025)), (('grid', 4097, 256, 2, 8), (2, 257)), (('grid', 4096, 256, 2, 8), (1, 512)),
          (('grid', 5, 256, 8, 4), (1, 2)), (('grid', 3 * 8192 + 1, 256, 8, 4), (4, 1537)), (('grid', 9, 1, 2, 8), (1, 2))])
