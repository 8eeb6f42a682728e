"""The host decisions about dynamic smoothing over the linked pairs of two sets of profiles without a GPU:
kpal_amd/csrc/pair_smooth_plan.hpp -- the (pair, slice) items with their bin slices and node slices, the units and the persistent
grid, the layout of the partials, the chunks under the pyramid budget and the index of a pair's tables in the pyramid set --
driven by a stand-alone program built with the address and undefined-behaviour sanitizers.  Every expected value is a literal or
comes from the rule as it is written here, none is computed with the header.

The rule.  A pyramid has (4^k - 1) / 3 nodes, padded to a multiple of 64 elements (the stride).  A pair's slices are its
max(1, 4^k / 2^16) bin slices followed by ceil(stride / 2^16) node slices; up to k = 6 (the wave form) a wave adds both and a pair
has ONE partial per accumulator, a unit is four pairs; above, a unit is one (pair, slice) item.  Grid: 8 workgroups per CU, the
smallest grid that needs no more rounds.  Accumulator a of pair p, slice s lies at (a * N + p) * slices + s.  A chunk is that of
the unsmoothed entry, cut by the 32-bit index of these partials and so that ten bytes per element of the pyramids of its distinct
tables stay within 32 GiB: 2 * chunk tables, or chunk (the same range), or chunk + |lag| (a whole number of tables apart, more
pairs than |lag|); never below one pair."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'kpal_amd', 'csrc')
NS = (1, 2, 3, 4, 5, 255, 256, 257, 10 ** 5)
CUS = (1, 8, 256)
GIB = 1 << 30
DISJOINT, SAME, LAG, OTHER = 0, 1, 2, 3


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('pair_smooth_plan') / 'pair_smooth_plan_check')
    b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-o', exe,
                        os.path.join(ROOT, 'tests', 'native', 'pair_smooth_plan_check.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0 and not b.stdout.strip(), b.stdout.decode()[-3000:]

    def ask(queries):
        """[(query words, expected answer)] -> asserts every answer"""
        text = ''.join(' '.join(str(w) for w in q) + '\n' for q, _ in queries)
        r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0 and got[-2] == 'PAIR_SMOOTH_PLAN_DONE %d' % len(queries), got[-20:]
        for (q, want), line in zip(queries, got):
            have = tuple(int(w) for w in line.split())
            assert have == (want if isinstance(want, tuple) else (want,)), (q, have, want)
    return ask


def ceil_div(a, b):
    return -(-a // b)


def stride_of(k):
    return ceil_div((4 ** k - 1) // 3, 64) * 64


def bin_slices_of(k):
    return max(1, 4 ** k >> 16)


def node_slices_of(k):
    return ceil_div(stride_of(k), 1 << 16)


def slices_of(k):
    return 1 if k <= 6 else bin_slices_of(k) + node_slices_of(k)


def test_header_knows_no_gpu():
    header = re.sub(r'//.*', '', open(os.path.join(CSRC, 'pair_smooth_plan.hpp')).read())
    assert not any(w in header for w in ('hip', 'Hip', 'HIP', 'kpal_ctx', 'LAUNCH(', 'getenv', '__global__', '__device__', 'blockIdx'))
    assert '#include "pair_set_plan.hpp"' in header and '#include "smooth_plan.hpp"' in header
    for user, names in (('pair_smooth_kernels.hpp', ('kPairSetThreads', 'kPairSetWaves', 'kPairSetUnroll', 'pair_set_slice_begin(', 'pair_set_slice_end(',
                                                     'pair_set_partial(', 'pair_smooth_node_begin(', 'kPairSmoothSliceNodes', 'opt_term<', 'cross_opt_scale(')),
                        ('kpal_paired_smooth.hip', ('pair_smooth_chunk(', 'pair_set_union(', 'pair_smooth_left(', 'pair_smooth_right(', 'pair_smooth_units(',
                                                    'pair_smooth_workgroups(', 'pair_smooth_slices(', 'pair_smooth_batched(', 'pair_set_alias(',
                                                    'balanced_pair_chunk(', 'smooth_set_pyramids(', 'partials_too_many(')),
                        ('dist_host.hpp', ('pair_set_balance_bytes(', 'balance_set_launch('))):      # balanced_pair_chunk: shared with kpal_paired.hip
        text = re.sub(r'//.*', '', open(os.path.join(CSRC, user)).read())
        assert all(n in text for n in names), (user, [n for n in names if n not in text])
    unit = open(os.path.join(CSRC, 'kpal_paired_smooth.hip')).read()
    assert set(re.findall(r'LAUNCH\(ctx, "([a-z_]+)"', unit)) == {'pair_smooth', 'pair_smooth_apply'}
    # the two non-template kernels of the pyramids stay in one unit; both rectangle and linked pairs build them through one function
    assert 'smooth_set_kernels.hpp' not in unit
    cross = open(os.path.join(CSRC, 'kpal_cross.hip')).read()
    assert cross.count('smooth_set_level_kernel') == 1 and cross.count('smooth_set_pyramids(') == 2
    kernels = re.sub(r'//.*', '', open(os.path.join(CSRC, 'pair_smooth_kernels.hpp')).read())
    assert 'printf' not in kernels and not re.search(r'(?<!static_)assert\(', kernels) and 'asm' not in kernels and 'pw_prod' not in kernels


def test_sizes(plan):
    plan([(('sizes',), (65536, 32 * GIB, 10))])


def test_slices_depend_on_k_alone(plan):
    literal = {1: (1, 1, 1, 64), 6: (1, 1, 1, 1408), 7: (1, 1, 2, 5504), 8: (1, 1, 2, 21888), 9: (4, 2, 6, 87424), 12: (256, 86, 342, 5592448),
               16: (65536, 21846, 87382, 1431655808)}
    plan([(('slices', k), literal[k]) for k in sorted(literal)])
    plan([(('slices', k), (bin_slices_of(k), node_slices_of(k), slices_of(k), stride_of(k))) for k in range(1, 17)])
    assert all(node_slices_of(k) == 1 for k in range(1, 9)) and node_slices_of(9) == 2


def test_node_slices_tile_the_pyramid(plan):
    """... and at k = 9 the second node slice begins with node 0 of height 1: height 0 has 4^8 = 2^16 nodes."""
    queries = []
    for k in range(1, 17):
        last = node_slices_of(k) - 1
        first = last << 16
        height, at = 0, first
        while height < k and at >= 4 ** (k - 1 - height):
            at -= 4 ** (k - 1 - height)
            height += 1
        queries.append((('nodes', k), (1, height if height < k else -1, stride_of(k) - first)))
    plan(queries)
    plan([(('nodes', 8), (1, 0, 21888)), (('nodes', 9), (1, 1, 21888)), (('nodes', 1), (1, 0, 64))])


def test_units_and_grid(plan):
    queries = []
    for k in range(1, 17):
        for n in NS:
            units = ceil_div(n, 4) if k <= 6 else n * slices_of(k)
            for cu in CUS:
                rounds = ceil_div(units, cu * 8)
                queries.append((('walk', k, n, cu), (units, ceil_div(units, rounds), 1)))
    plan(queries)
    plan([(('walk', 6, 5, 256), (2, 2, 1)), (('walk', 6, 65, 256), (17, 17, 1)), (('walk', 8, 4000, 256), (8000, 2000, 1)), (('walk', 9, 5, 256), (30, 30, 1)),
          (('walk', 12, 64, 256), (21888, 1990, 1))])


def test_partials_are_a_bijection(plan):
    queries = []
    for k in (1, 6, 7, 8, 9, 10, 12, 16):
        for n in NS:
            for nacc in (1, 3):
                queries.append((('partial', k, n, nacc), (1, nacc * n * slices_of(k))))
    plan(queries)


def test_chunks_under_the_pyramid_budget(plan):
    p12, p16 = 10 * 5592448, 10 * 1431655808
    assert 32 * GIB // p12 == 614 and 32 * GIB // p16 == 2
    plan([(('chunk', 6, 20000, 0, 0, DISJOINT, 0), (20000, 40000, 40000 * 14080)),
          (('chunk', 6, 20000, 0, 7, DISJOINT, 0), (7, 14, 14 * 14080)),               # chunk_pairs lowers it
          (('chunk', 6, 20000, 0, 30000, LAG, 1), (20000, 20001, 20001 * 14080)),      # ... and never raises it
          (('chunk', 12, 1000, 0, 0, DISJOINT, 0), (307, 614, 614 * p12)),             # 614 pyramids fit 32 GiB
          (('chunk', 12, 1000, 0, 0, SAME, 0), (614, 614, 614 * p12)),
          (('chunk', 12, 1000, 0, 0, LAG, 1), (613, 614, 614 * p12)),                  # successive windows: N pyramids, not 2 (N - lag)
          (('chunk', 12, 1000, 0, 0, LAG, -3), (611, 614, 614 * p12)),
          (('chunk', 12, 1000, 0, 0, LAG, 400), (307, 614, 614 * p12)),                # no room for more pairs than the lag: two sides
          (('chunk', 12, 1000, 0, 0, OTHER, 0), (307, 614, 614 * p12)),
          (('chunk', 12, 1000, 1, 0, DISJOINT, 0), (128, 256, 256 * p12)),             # the balanced copies cut it first
          (('chunk', 12, 1000, 0, 7, LAG, 1), (7, 8, 8 * p12)),
          (('chunk', 16, 5, 0, 0, DISJOINT, 0), (1, 2, 2 * p16)),                      # two k = 16 pyramids fit: one pair
          (('chunk', 16, 5, 1, 0, DISJOINT, 0), (1, 2, 2 * p16)),
          (('chunk', 16, 5, 0, 0, LAG, 1), (1, 2, 2 * p16)),
          (('chunk', 16, 5, 0, 0, SAME, 0), (2, 2, 2 * p16)),
          (('chunk', 1, 1, 1, 0, DISJOINT, 0), (1, 2, 1280)),
          # (the pyramids bind long before the 32-bit index of the partials does)
          (('chunk', 7, 10 ** 9, 0, 0, SAME, 0), (624268, 624268, 624268 * 55040)),
          (('chunk', 6, 10 ** 9, 0, 0, LAG, 1), (2440321, 2440322, 2440322 * 14080))])
    queries = []
    for k in range(1, 17):
        pyramid = 10 * stride_of(k)
        fit = 32 * GIB // pyramid
        for n in NS:
            base = max(1, min(n, ((1 << 31) - 1) // bin_slices_of(k) // 3, ((1 << 31) - 1) // slices_of(k) // 3))
            chunk = max(1, min(base, fit // 2))
            assert chunk == 1 or 2 * chunk * pyramid <= 32 * GIB
            queries.append((('chunk', k, n, 0, 0, DISJOINT, 0), (chunk, 2 * chunk, 2 * chunk * pyramid)))
            queries.append((('chunk', k, n, 0, 0, SAME, 0), (min(base, fit), min(base, fit), min(base, fit) * pyramid)))
    plan(queries)


def test_table_indices(plan):
    """(union tables, pyramids, left of pair p, right of pair p)."""
    plan([(('tables', 10, DISJOINT, 0, 4), (0, 20, 4, 14)),             # two sides: p and N + p
          (('tables', 10, OTHER, 0, 9), (0, 20, 9, 19)),
          (('tables', 10, SAME, 0, 4), (10, 10, 4, 4)),
          (('tables', 10, LAG, 1, 4), (11, 11, 4, 5)), (('tables', 10, LAG, -1, 4), (11, 11, 5, 4)),
          (('tables', 10, LAG, 3, 0), (13, 13, 0, 3)), (('tables', 10, LAG, -3, 0), (13, 13, 3, 0)),
          (('tables', 10, LAG, 3, 9), (13, 13, 9, 12)), (('tables', 10, LAG, -3, 9), (13, 13, 12, 9)),
          (('tables', 10, LAG, 10, 4), (0, 20, 4, 14)),                  # the sides of the chunk do not meet
          (('tables', 1, LAG, 1, 0), (0, 2, 0, 1)), (('tables', 1, SAME, 0, 0), (1, 1, 0, 0))])


def test_positive_keeps_the_pair_pipeline(plan):
    plan([(('batched', 1, 0), 1), (('batched', 1, 1), 0), (('batched', 0, 0), 0), (('batched', 0, 1), 0)])
