"""The host decisions of kpal_cross_nearest without a GPU: kpal_amd/csrc/nearest_plan.hpp -- the order of the candidates, the
kernel family of an option set, the tiles of a Q x R rectangle -- driven by a stand-alone program built with the address and
undefined-behaviour sanitizers (tests/native/nearest_plan_check.cpp).  256 CUs throughout."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CU = 256
PROD, SUM, EUCLIDEAN, COSINE = 0, 1, 2, 3          # include/kpal_hip.h
PLAIN, GRAM, OPTION, SMOOTH = 0, 1, 2, 3           # NearestRoute
GIB = 1 << 30
# (route, (s, m) groups per slot): plain, euclidean, scaled, positive + scale, cosine, smoothed prod, smoothed cosine
KINDS = [(PLAIN, 1), (GRAM, 1), (OPTION, 1), (OPTION, 2), (OPTION, 3), (SMOOTH, 2), (SMOOTH, 6)]


@pytest.fixture(scope='module')
def ask(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('nearest_plan') / 'nearest_plan_check')
    b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-o', exe,
                        os.path.join(ROOT, 'tests', 'native', 'nearest_plan_check.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0 and not b.stdout.strip(), b.stdout.decode()[-3000:]

    def run(queries):
        """[query words] -> [tuple of numbers] per query"""
        text = ''.join(' '.join(str(w) for w in q) + '\n' for q in queries)
        r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0 and got[-2] == 'NEAREST_PLAN_DONE %d' % len(queries), got[-20:]
        return [tuple(int(w) for w in line.split()) for line in got[:len(queries)]]
    return run


def plan(kind, Q, R, bins=4096, budget=4 * GIB, capq=0, capr=0):
    return ('plan', CU, bins, kind[0], kind[1], Q, R, budget, capq, capr)


# a plan's answer: tile_q, tile_r, tiles, then the five verdicts -- every pair covered once, ascending r0 within a band, every
# tile passes partials_too_many for every pass of its route, stays within the budget, and within the caller's caps
ALL_GOOD = (1, 1, 1, 1, 1)


def test_kinds(ask):
    # ('kind', balance, positive, smooth, scale, metric)
    got = ask([('kind', 0, 0, 0, 0, PROD), ('kind', 1, 0, 0, 0, SUM), ('kind', 0, 0, 0, 0, EUCLIDEAN), ('kind', 1, 0, 0, 0, EUCLIDEAN),
               ('kind', 0, 0, 0, 0, COSINE), ('kind', 0, 0, 0, 1, PROD), ('kind', 0, 1, 0, 0, EUCLIDEAN), ('kind', 0, 1, 0, 1, SUM),
               ('kind', 0, 1, 0, 1, COSINE), ('kind', 0, 0, 1, 0, PROD), ('kind', 0, 0, 1, 1, COSINE), ('default',)])
    assert got == [(PLAIN, 1), (PLAIN, 1), (GRAM, 1), (GRAM, 1), (OPTION, 3), (OPTION, 1), (OPTION, 1), (OPTION, 2), (OPTION, 3),
                   (SMOOTH, 2), (SMOOTH, 6), (4 * GIB,)]


def test_a_shape_one_call_refuses_is_tiled(ask):
    """20 000 x 16 384 at k = 6: 5000 * 4096 tiles of 16 slots at the staged floor of 8 workgroups pass 2^31 partials."""
    assert ask([('refused', CU, 20000, 16384, 4096)]) == [(1,)]
    assert ask([('refused', CU, 16000, 16384, 4096)]) == [(0,)]
    for kind, got in zip(KINDS, ask([plan(kind, 20000, 16384) for kind in KINDS])):
        assert got[3:8] == ALL_GOOD and got[2] > 1, (kind, got)


@pytest.mark.parametrize('bins', (64, 4096, 65536))
def test_tiles_cover_and_fit(ask, bins):
    shapes = [(1, 1), (3, 2), (9, 21), (64, 64), (65, 130), (1000, 1000), (4000, 64), (20000, 512), (60000, 8192), (1, 1 << 15),
              (1 << 20, 1), (1 << 20, 1 << 15), ((1 << 20) - 77, (1 << 15) - 5)]
    queries = [(kind, Q, R, budget) for kind in KINDS for Q, R in shapes for budget in (4 * GIB, 64 << 20)]
    for (kind, Q, R, budget), got in zip(queries, ask([plan(kind, Q, R, bins, budget) for kind, Q, R, budget in queries])):
        assert got[3:8] == ALL_GOOD and got[8] <= budget, (kind, Q, R, budget, got)
        assert 1 <= got[0] <= Q and 1 <= got[1] <= R and got[2] == -(-Q // got[0]) * -(-R // got[1]), (kind, Q, R, budget, got)


def test_small_shapes_are_one_tile(ask):
    got = ask([plan(kind, Q, R, bins) for kind in KINDS for Q, R, bins in ((9, 21, 4096), (4000, 64, 65536), (64, 64, 1 << 24))])
    want = [(Q, R, 1) for kind in KINDS for Q, R in ((9, 21), (4000, 64), (64, 64))]
    assert [g[:3] for g in got] == want and all(g[3:8] == ALL_GOOD for g in got)
    # 20 000 x 512 at k = 6: 5000 * 128 tiles of 16 slots, 8 partials of 16 bytes each -- 1.3 GB with one group per slot
    got = ask([plan(kind, 20000, 512) for kind in KINDS if kind[1] == 1])
    assert all(g[:8] == (20000, 512, 1) + ALL_GOOD for g in got), got


def test_caps_only_shrink(ask):
    got = ask([plan(kind, 9, 21, capq=4, capr=8) for kind in KINDS])
    assert all(g[:8] == (4, 8, 9) + ALL_GOOD for g in got), got
    got = ask([plan((PLAIN, 1), 9, 21, capq=100, capr=100), plan((PLAIN, 1), 9, 21, capq=9, capr=0), plan((PLAIN, 1), 9, 21, capq=0, capr=20),
               plan((PLAIN, 1), 9, 21, capq=1, capr=1)])
    assert [g[:8] for g in got] == [(9, 21, 1) + ALL_GOOD, (9, 21, 1) + ALL_GOOD, (9, 20, 2) + ALL_GOOD, (1, 1, 189) + ALL_GOOD]
    # a cap larger than what the budget admits does not enlarge a tile: 64 MiB hold fewer than 2^20 staged pairs of 152 bytes
    free, capped = ask([plan((PLAIN, 1), 4096, 4096, budget=64 << 20), plan((PLAIN, 1), 4096, 4096, budget=64 << 20, capq=4096, capr=4096)])
    assert free == capped and free[0] * free[1] < 1 << 20 and free[3:8] == ALL_GOOD


def test_budget_below_one_pair(ask):
    got, = ask([plan((OPTION, 3), 3, 2, budget=1)])
    assert got[:7] == (1, 1, 6, 1, 1, 1, 0)


SORTED = [('-inf', 9), (-1.0, 5), ('-0.0', 1), (0.0, 2), ('-0.0', 3), (0.25, 0), (0.25, 7), (0.25, 1 << 40), (1.0, 4), ('inf', 6), ('nan', 8),
          ('nan', 10), ('nan', 1 << 41)]


def order(entries):
    return ('order', len(entries)) + tuple(w for e in entries for w in e)


def test_order(ask):
    """Ascending distance; equal distances -- +0 and -0 are equal -- by the lower index; NaN behind every number, by index."""
    assert ask([order(SORTED)]) == [(0,)]
    for a in range(len(SORTED) - 1):   # the checker sees every neighbouring swap
        swapped = SORTED[:a] + [SORTED[a + 1], SORTED[a]] + SORTED[a + 2:]
        assert ask([order(swapped)]) == [(2,)], a


def test_host_merge(ask):
    # ('merge', n, have, count, first, have x (dist, index), count x dist) -> kept, indices
    got = ask([('merge', 3, 2, 4, 4, 0.25, 10, 0.5, 3, 0.25, 'nan', 0.5, 0.1),
               ('merge', 1, 1, 1, 5, 1.0, 20, 1.0),            # a carried candidate does not beat a lower index that arrives later
               ('merge', 2, 0, 3, 0, 'nan', 'nan', 'nan'),     # every candidate NaN: by index
               ('merge', 5, 1, 2, 7, 'nan', 2, 'nan', 3.0),    # fewer candidates than n
               ('merge', 2, 2, 1, 0, '-0.0', 4, 0.0, 6, 0.0)])
    assert got == [(3, 7, 4, 10), (1, 5), (2, 0, 1), (3, 8, 2, 7), (2, 0, 4)]
