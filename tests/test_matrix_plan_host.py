"""The host decisions about the distances of sets of profiles without a GPU: kpal_amd/csrc/matrix_plan.hpp -- which kernel
family a triangle or a rectangle takes (and what the four KPAL_MATRIX_* switches change), the grids, the "too many for one
call" limit (which no GPU test can reach), where a pair lies in the reduced partials, the finishing arithmetic -- driven by a
stand-alone program built with the address and undefined-behaviour sanitizers.  Every expected value is a literal written
down from the rule, none is computed with the header.  256 CUs throughout."""
import math
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CU = 256
PROD, SUM, EUCLIDEAN, COSINE = 0, 1, 2, 3   # include/kpal_hip.h
NAN = float('nan')
ON = (1, 1, 1, 1)                           # MatrixSwitches: mfma, super_, all, rdiff
# matrix_route's answer: gram, all, all_wide, staged, recip
REGISTER_TILES = (0, 0, 0, 0, 0)
STAGED_RECIP = (0, 0, 0, 1, 1)              # the reciprocal form first, then cross_super
STAGED_ONLY = (0, 0, 0, 1, 0)
ALL_NARROW = (0, 1, 0, 1, 1)                # the *_all kernel first; behind it the staged forms
ALL_WIDE = (0, 1, 1, 1, 1)
GRAM_STAGED = (1, 0, 0, 1, 0)               # the Gram matrix first; behind it cross_super
GRAM_REGISTER = (1, 0, 0, 0, 0)


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('matrix_plan') / 'matrix_plan_check')
    b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-o', exe,
                        os.path.join(ROOT, 'tests', 'native', 'matrix_plan_check.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0 and not b.stdout.strip(), b.stdout.decode()[-3000:]

    def same(have, want):
        return len(have) == len(want) and all((math.isnan(h) and math.isnan(w)) or h == w for h, w in zip(have, want))

    def ask(queries):
        """[(query words, expected answer)] -> asserts every answer"""
        text = ''.join(' '.join(str(w) for w in q) + '\n' for q, _ in queries)
        r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0 and got[-2] == 'MATRIX_PLAN_DONE %d' % len(queries), got[-20:]
        for (q, want), line in zip(queries, got):
            have = tuple(float(w) for w in line.split())
            assert same(have, want if isinstance(want, tuple) else (want,)), (q, have, want)
    return ask


def route(P, n, metric, agreed=1, switches=ON):
    return ('route', P, n, metric, agreed) + tuple(switches)


def test_one_definition_each():
    """The header knows no GPU, and what moved into it is restated nowhere in the units and kernel headers that use it."""
    csrc = os.path.join(ROOT, 'kpal_amd', 'csrc')
    users = ('matrix_common.hpp', 'cross_kernels.hpp', 'cross_option_kernels.hpp', 'gram_kernels.hpp', 'matrix_all_kernels.hpp', 'vec_kernels.hpp',
             'kpal_host.hpp', 'kpal_vec.hip', 'kpal_pair.hip', 'kpal_cross.hip', 'kpal_multi.hip')
    text = {f: re.sub(r'//.*', '', open(os.path.join(csrc, f)).read()) for f in users + ('matrix_plan.hpp',)}
    header = text.pop('matrix_plan.hpp')
    assert not any(w in header for w in ('hip_runtime', 'hipLaunch', 'kpal_ctx', 'LAUNCH(', 'getenv'))
    assert '#include "matrix_plan.hpp"' in text['matrix_common.hpp'] and '#include "matrix_plan.hpp"' in text['kpal_host.hpp']
    for name in ('struct Partial {', 'struct CrossSets {', 'struct CrossGrid {', 'cross_tile_number(int', 'cross_slot(const', 'kSuperBins =', 'kGramBins ='):
        assert name in header and not any(name in t for t in text.values()), name
    for gone in ('PartialPod', 'cross_slot_host', 'struct Partial;', '% 64 == 0', '9007199254740992', '0x7fffffffu', 'std::sqrt', 'getenv("KPAL_MATRIX'):
        where = [f for f, t in text.items() if gone in t and not (gone == 'getenv("KPAL_MATRIX' and f == 'kpal_cross.hip')
                 and not (gone == 'std::sqrt' and f == 'kpal_vec.hip')]   # (kpal_stats_device: the standard deviation)
        assert not where, (gone, where)
    assert text['kpal_cross.hip'].count('getenv(name)') == 1   # the four switches are read in one place, once per process


def test_tiled_staged_plain(plan):
    plan([(('tiled', 4096), 1), (('tiled', 4160), 1), (('tiled', 4100), 0), (('tiled', 4032), 0), (('tiled', 1024), 0), (('tiled', 1 << 24), 1),
          (('staged', 5, 5, 4096), 1), (('staged', 4, 100, 4096), 0), (('staged', 100, 4, 4096), 0), (('staged', 5, 5, 1024), 0),
          (('plain', 0, 0, 0, PROD), 1), (('plain', 0, 0, 0, SUM), 1), (('plain', 0, 0, 0, EUCLIDEAN), 1), (('plain', 0, 0, 0, COSINE), 0),
          (('plain', 1, 0, 0, PROD), 0), (('plain', 0, 1, 0, PROD), 0), (('plain', 0, 0, 1, EUCLIDEAN), 0)])


def test_route_by_profiles(plan):
    n = 4096
    q = [(route(8, n, m), REGISTER_TILES) for m in (PROD, SUM, EUCLIDEAN)]
    q += [(route(9, n, PROD), STAGED_RECIP), (route(9, n, SUM), STAGED_RECIP), (route(9, n, EUCLIDEAN), GRAM_STAGED)]
    for m in (PROD, SUM):
        q += [(route(16, n, m), STAGED_RECIP), (route(17, n, m), ALL_NARROW), (route(32, n, m), ALL_NARROW), (route(33, n, m), ALL_WIDE),
              (route(64, n, m), ALL_WIDE), (route(65, n, m), STAGED_RECIP)]
    q += [(route(P, n, EUCLIDEAN), GRAM_STAGED) for P in (17, 40, 64, 65, 1000)]
    plan(q)


def test_route_by_bins_and_agreement(plan):
    plan([(route(40, 1024, PROD), REGISTER_TILES), (route(40, 1024, EUCLIDEAN), REGISTER_TILES),
          (route(40, 4160, PROD), ALL_WIDE), (route(40, 4100, PROD), REGISTER_TILES), (route(40, 4100, EUCLIDEAN), REGISTER_TILES),
          # a bin-range matrix whose ranks agreed not to take the staged kernels; -1 (one GPU) and 1 (agreed) decide by n
          (route(40, 4096, PROD, agreed=0), REGISTER_TILES), (route(40, 4096, EUCLIDEAN, agreed=0), REGISTER_TILES),
          (route(40, 4096, PROD, agreed=-1), ALL_WIDE), (route(40, 4096, PROD, agreed=1), ALL_WIDE),
          (route(40, 4096, EUCLIDEAN, agreed=-1), GRAM_STAGED)])


def test_route_switches(plan):
    n = 4096
    plan([(route(40, n, EUCLIDEAN, switches=(0, 1, 1, 1)), STAGED_ONLY),     # KPAL_MATRIX_MFMA=0
          (route(40, n, PROD, switches=(0, 1, 1, 1)), ALL_WIDE),
          (route(40, n, PROD, switches=(1, 1, 0, 1)), STAGED_RECIP),         # KPAL_MATRIX_ALL=0
          (route(40, n, PROD, switches=(1, 1, 1, 0)), STAGED_ONLY),          # KPAL_MATRIX_RDIFF=0: neither *_all nor the reciprocal form
          (route(40, n, SUM, switches=(1, 1, 1, 0)), STAGED_ONLY),
          (route(40, n, PROD, switches=(1, 0, 1, 1)), REGISTER_TILES),       # KPAL_MATRIX_SUPER=0
          (route(40, n, EUCLIDEAN, switches=(1, 0, 1, 1)), GRAM_REGISTER),   # ... the Gram matrix is still tried
          (route(40, n, EUCLIDEAN, switches=(0, 0, 0, 0)), REGISTER_TILES),
          (route(40, n, PROD, switches=(0, 0, 0, 0)), REGISTER_TILES)])


def test_cross_grid(plan):
    # ('grid', CUs, Q, R, n, tri, staged) -> (units, gx, slots, sideR, superR)
    plan([
        # triangle of 9: 1 super-tile, 3 * 4 / 2 = 6 tiles; gx = min(4096 / 64, 2048 / 1) = 64
        (('grid', CU, 9, 9, 4096, 1, 1), (1, 64, 96, 3, 1)),
        # 200: 13 * 14 / 2 = 91 super-tiles, 50 * 51 / 2 = 1275 tiles; 2048 // 91 = 22 -> 16
        (('grid', CU, 200, 200, 4096, 1, 1), (91, 16, 20400, 50, 13)),
        # 1000: 63 * 64 / 2 = 2016 super-tiles, 250 * 251 / 2 = 31375 tiles; 2048 // 2016 = 1 -> the floor of 8
        (('grid', CU, 1000, 1000, 4096, 1, 1), (2016, 8, 502000, 250, 63)),
        (('grid', CU, 5, 7, 4096, 0, 1), (1, 64, 64, 2, 1)),
        # register tiles: 1 x 25 tiles; gx = min(2^24 / 256, 4096 // 25) = 163
        (('grid', CU, 3, 100, 1 << 24, 0, 0), (25, 163, 400, 25, 7)),
        (('grid', CU, 8, 8, 4096, 1, 0), (3, 16, 48, 2, 1)),
        (('grid', CU, 2, 2, 4, 1, 0), (1, 1, 16, 1, 1))])


def test_too_many_for_one_call(plan):
    # 0x7fffffff // 8 = 268435455 slots at the staged grid's floor of 8 workgroups per slot
    plan([
        # side 5792: 5792 * 5793 / 2 = 16776528 tiles; 1448 * 1449 / 2 = 1049076 super-tiles
        (('grid', CU, 23168, 23168, 4096, 1, 1), (1049076, 8, 268424448, 5792, 1448)), (('toomany', 268424448, 8), 0),
        # side 5793: 5793 * 5794 / 2 = 16782321 tiles; 1449 * 1450 / 2 = 1050525 super-tiles
        (('grid', CU, 23169, 23169, 4096, 1, 1), (1050525, 8, 268517136, 5793, 1449)), (('toomany', 268517136, 8), 1),
        (('toomany', 268435455, 8), 0), (('toomany', 268435456, 8), 1), (('toomany', 0x7fffffff, 1), 0), (('toomany', 0x80000000, 1), 1),
        # an option set with three accumulators per pair reaches it at a third of the slots
        (('toomany', 3 * 89478485, 8), 0), (('toomany', 3 * 89478486, 8), 1)])


def test_gram_grids_and_indices(plan):
    blocks129 = (0, 0, 1, 1, 2, 2, 1, 0, 2, 0, 2, 1)   # the diagonal blocks, then (1,0), (2,0), (2,1)
    plan([(('gram', CU, 40, 4096), (1, 0, 64, 0, 0, 0)),
          (('gram', CU, 129, 4096), (3, 3, 64, 64) + blocks129),
          (('gram', CU, 129, 1 << 24), (3, 3, 170, 85) + blocks129),
          # pair (70, 3): block (1, 0) is the first off-diagonal one, number 3; tile 0; entry 6 * 16 + 3
          (('gramidx', CU, 129, 4096, 70, 3), 12387),
          (('gramidx', CU, 129, 4096, 70, 70), 4198),      # block 1, tile 0, entry 6 * 16 + 6
          (('gramidx', CU, 129, 4096, 128, 127), 21263),   # block (2, 1) = number 5, tile 0 * 4 + 3, entry 0 * 16 + 15
          (('gramidx', CU, 40, 4096, 39, 17), 2417),       # block 0, tile 2 * 4 + 1 = 9, entry 7 * 16 + 1
          # rectangle, two column blocks: (70, 100) is block 1 * 2 + 1, tile 0 * 4 + 2, entry 6 * 16 + 4
          (('xgramidx', 2, 70, 100), 12900), (('xgramidx', 1, 3, 5), 53),
          (('xgramgx', CU, 1, 4096), 64), (('xgramgx', CU, 4, 1 << 24), 64), (('xgramgx', CU, 300, 4096), 1)])


def test_other_grids(plan):
    plan([(('allgx', CU, 4096, 1), 32), (('allgx', CU, 4096, 0), 32), (('allgx', CU, 1 << 24, 1), 256), (('allgx', CU, 1 << 24, 0), 1024),
          (('allgx', CU, 64, 0), 1),
          (('gxt', CU, 12, 4096), 16), (('gxt', CU, 1000, 1 << 24), 2), (('gxt', CU, 3000, 4096), 1), (('gxt', CU, 12, 16), 1),
          (('nacc', PROD, 0, 0), (1, 1)), (('nacc', EUCLIDEAN, 1, 0), (1, 1)), (('nacc', SUM, 1, 1), (1, 2)), (('nacc', PROD, 0, 1), (1, 1)),
          (('nacc', COSINE, 0, 0), (3, 3)), (('nacc', COSINE, 1, 1), (3, 3))])


def test_slots(plan):
    plan([(('slot', 1, 0, 5, 2), 22),      # triangle: tile (1, 0) is number 1; 16 + 1 * 4 + 2
          (('slot', 1, 99, 5, 2), 22),     # ... whatever the side
          (('slot', 0, 3, 5, 6), 70),      # R = 9: three tiles a row; tile (1, 1) is number 4; 64 + 1 * 4 + 2
          (('slot', 1, 0, 0, 0), 0), (('slot', 1, 0, 11, 11), 95), (('slot', 0, 1, 7, 3), 31),
          (('tri', 5, 2), 12), (('tri', 1, 0), 0), (('tri', 2, 1), 2), (('tri', 65536, 65535), 2147516415)])


def test_finishing(plan):
    # ('finish', metric, scaled, s0, m0, s1, m1, s2, m2)
    plan([(('finish', PROD, 0, 3.0, 5, 0, 0, 0, 0), 0.5), (('finish', SUM, 1, 3.0, 5, 0, 0, 0, 0), 0.5),
          (('finish', PROD, 0, 0.0, 0, 0, 0, 0, 0), 0.0),
          (('finish', EUCLIDEAN, 0, 0.0, 25, 0, 0, 0, 0), 5.0),
          (('finish', EUCLIDEAN, 0, 0.0, (1 << 64) - 4, 0, 0, 0, 0), NAN),   # a wrapped, negative int64 dot
          (('finish', EUCLIDEAN, 1, 2.25, 25, 0, 0, 0, 0), 1.5),
          (('finish', COSINE, 0, 0.0, 6, 0.0, 4, 0.0, 9), 1.0), (('finish', COSINE, 1, 6.0, 0, 4.0, 0, 9.0, 0), 1.0),
          (('finish', COSINE, 0, 0.0, (1 << 64) - 6, 0.0, 4, 0.0, 9), -1.0)])


def test_gram_distance(plan):
    two53 = 1 << 53
    plan([(('gramdist', 25, 16, 20), (1.0, 1)),
          (('gramdist', two53 - 1, 1, (1 << 52) - 8), (4.0, 1)),   # 2^53 - 1 + 1 - 2 (2^52 - 8) = 16
          (('gramdist', two53, 1, 0), (0.0, 0)), (('gramdist', 1, two53, 0), (0.0, 0)), (('gramdist', 'nan', 1, 0), (0.0, 0)),
          (('gramdist', 0, 0, 0), (0.0, 1))])


def test_scale_factors(plan):
    # ('scale', total left, total right, down) -> (ls, rs)
    plan([(('scale', 10, 40, 0), (4.0, 1.0)), (('scale', 10, 40, 1), (1.0, 0.25)),
          (('scale', 40, 10, 0), (1.0, 4.0)), (('scale', 40, 10, 1), (0.25, 1.0)),
          (('scale', 7, 7, 0), (1.0, 1.0)), (('scale', 7, 7, 1), (1.0, 1.0)),
          # totals 0 and 0: 0 < 0 is false, so the right factor is 0 / 0 and the left one stays 1 -- until `down` divides both by it
          (('scale', 0, 0, 0), (1.0, NAN)), (('scale', 0, 0, 1), (NAN, NAN))])
