"""The host decisions about the distances of the linked pairs of two sets of profiles without a GPU:
kpal_amd/csrc/pair_set_plan.hpp -- the flat list of (pair, slice) items, the units a workgroup of the persistent grid takes,
the layout of the partials, the chunks of a call with balanced copies and the test of the two input ranges against each other --
driven by a stand-alone program built with the address and undefined-behaviour sanitizers.  Every expected value is a literal or
comes from the rule as it is written here, none is computed with the header.

The rule.  A slice is 2^16 bins: a table of 4^k bins has max(1, 4^k / 2^16) of them, whatever N, the device or the chunking.  Up
to 4^6 bins a wave takes a whole table and a unit is four consecutive pairs; above, a unit is one (pair, slice) item.  `slots` = 8
workgroups per CU; the grid is the smallest that needs no more rounds than `slots` workgroups would (rounds = ceil(units /
slots), grid = ceil(units / rounds)), workgroup g takes units g, g + grid, ...  Accumulator a of pair p, slice s lies at
(a * N + p) * slices + s.  A chunk is N pairs, cut by the 32-bit index of the partials (2^31 - 1 groups over 3 accumulators), with
balance by 32 GiB of copies at two tables a pair (never below one pair), and by the caller's chunk_pairs."""
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


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('pair_set_plan') / 'pair_set_plan_check')
    b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-o', exe,
                        os.path.join(ROOT, 'tests', 'native', 'pair_set_plan_check.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0 and not b.stdout.strip(), b.stdout.decode()[-3000:]

    def ask(queries):
        """[(query words, expected answer)] -> asserts every answer"""
        text = ''.join(' '.join(str(w) for w in q) + '\n' for q, _ in queries)
        r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0 and got[-2] == 'PAIR_SET_PLAN_DONE %d' % len(queries), got[-20:]
        for (q, want), line in zip(queries, got):
            have = tuple(int(w) for w in line.split())
            assert have == (want if isinstance(want, tuple) else (want,)), (q, have, want)
    return ask


def slices_of(k):
    return max(1, 4 ** k >> 16)


def ceil_div(a, b):
    return -(-a // b)


def test_header_knows_no_gpu():
    header = re.sub(r'//.*', '', open(os.path.join(CSRC, 'pair_set_plan.hpp')).read())
    assert not any(w in header for w in ('hip', 'Hip', 'HIP', 'kpal_ctx', 'LAUNCH(', 'getenv', '__global__', '__device__', 'blockIdx'))
    # the kernels and the host take their numbers from it
    for user, names in (('pair_set_kernels.hpp', ('kPairSetThreads', 'kPairSetWaves', 'kPairSetUnroll', 'pair_set_slice_begin(', 'pair_set_slice_end(',
                                                  'pair_set_partial(')),
                        ('kpal_paired.hip', ('pair_set_wave_form(', 'pair_set_slices(', 'pair_set_units(', 'pair_set_workgroups(', 'pair_set_chunk(',
                                             'pair_set_alias(', 'pair_set_union(', 'balanced_pair_chunk(', 'partials_too_many(')),
                        ('pair_set_plan.hpp', ('pair_set_union_tables(', 'kPairSetSame', 'kPairSetLag')),      # pair_set_union: the union of a chunk
                        ('dist_host.hpp', ('pair_set_balance_bytes(', 'balance_set_launch('))):                # balanced_pair_chunk: shared with kpal_paired_smooth.hip
        text = re.sub(r'//.*', '', open(os.path.join(CSRC, user)).read())
        assert all(n in text for n in names), user
    # the term of a bin is defined once, for the rectangle kernels and these
    for user in ('pair_set_kernels.hpp', 'cross_option_kernels.hpp'):
        text = re.sub(r'//.*', '', open(os.path.join(CSRC, user)).read())
        assert '#include "option_term.hpp"' in text and 'opt_term<' in text and 'pw_prod' not in text, user
    unit = open(os.path.join(CSRC, 'kpal_paired.hip')).read()
    assert set(re.findall(r'LAUNCH\(ctx, "([a-z_]+)"', unit)) == {'pair_set', 'pair_set_totals'}
    # the kernels stay quiet
    kernels = re.sub(r'//.*', '', open(os.path.join(CSRC, 'pair_set_kernels.hpp')).read())
    assert 'printf' not in kernels and not re.search(r'(?<!static_)assert\(', kernels) and 'asm' not in kernels


def test_sizes(plan):
    plan([(('sizes',), (256, 4, 4, 65536, 4096, 8, 32 * GIB, 3))])


def test_slices_depend_on_k_alone_and_tile_the_table(plan):
    want = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1, 8: 1, 9: 4, 10: 16, 11: 64, 12: 256, 13: 1024, 14: 4096, 15: 16384, 16: 65536}
    plan([(('slices', k), (want[k], 1 if k <= 6 else 0)) for k in range(1, 17)])
    plan([(('tile', k), (1, min(4 ** k, 65536), min(4 ** k, 65536))) for k in range(1, 17)])


def test_every_item_is_reached_once(plan):
    """k = 1 .. 16, every N, three devices: units and grid by the rule, the walk complete, shares equal to within one -- and
    the number of slices (units / N in the slice form) the same for every N and every device."""
    queries = []
    for k in range(1, 17):
        for n in NS:
            units = ceil_div(n, 4) if k <= 6 else n * slices_of(k)
            for cu in CUS:
                rounds = ceil_div(units, cu * 8)
                grid = ceil_div(units, rounds)
                queries.append((('walk', k, n, cu), (units, grid, 1, units // grid, ceil_div(units, grid))))
    plan(queries)


def test_grid_literals(plan):
    plan([(('walk', 6, 20000, 256), (5000, 1667, 1, 2, 3)),      # 5000 units over 2048 slots: 3 rounds, ceil(5000 / 3)
          (('walk', 8, 4000, 256), (4000, 2000, 1, 2, 2)),
          (('walk', 12, 64, 256), (16384, 2048, 1, 8, 8)),
          (('walk', 6, 5, 256), (2, 2, 1, 1, 1)),                 # a ragged last unit: pair 4 alone
          (('walk', 7, 5, 1), (5, 5, 1, 1, 1)),
          (('walk', 7, 9, 1), (9, 5, 1, 1, 2))])                  # 9 units on 8 slots: two rounds, five workgroups


def test_partials_are_a_bijection(plan):
    queries = []
    for k in (1, 6, 7, 8, 9, 10, 12, 16):
        for n in NS:
            for nacc in (1, 2, 3):
                queries.append((('partial', k, n, nacc), (1, nacc * n * slices_of(k))))
    plan(queries)


def test_chunks(plan):
    plan([(('chunk', 6, 20000, 0, 0), (20000, 1)),
          (('chunk', 6, 20000, 0, 7), (7, 2858)),                 # chunk_pairs lowers it
          (('chunk', 6, 20000, 0, 30000), (20000, 1)),            # ... and never raises it
          (('chunk', 6, 20000, 1, 0), (20000, 1)),                # 2 x 20000 x 32 KiB = 1.2 GiB of copies
          (('chunk', 8, 40000, 1, 0), (32768, 2)),                # 2 x 512 KiB a pair: 32 GiB / 1 MiB
          (('chunk', 8, 40000, 1, 100), (100, 400)),
          (('chunk', 8, 40000, 1, 50000), (32768, 2)),
          (('chunk', 12, 64, 1, 0), (64, 1)),                     # 2 x 128 MiB a pair: 128 pairs fit
          (('chunk', 12, 300, 1, 0), (128, 3)),
          (('chunk', 15, 5, 1, 0), (2, 3)),                       # 8 GiB a table
          (('chunk', 16, 5, 1, 0), (1, 5)),                       # 64 GiB a pair: one pair, over the budget
          (('chunk', 16, 5, 0, 0), (5, 1)),
          (('chunk', 1, 1, 1, 0), (1, 1)),
          # the 32-bit index of the partials: (2^31 - 1) / slices groups over three accumulators
          (('chunk', 6, 10 ** 9, 0, 0), (715827882, 2)),
          (('chunk', 12, 10 ** 7, 0, 0), (2796202, 4)),
          (('chunk', 16, 10 ** 5, 0, 0), (10922, 10))])


def test_chunk_budget_is_kept_but_for_a_single_pair(plan):
    queries = []
    for k in range(1, 17):
        table = 8 * 4 ** k
        for n in NS:
            chunk = max(1, min(n, 32 * GIB // (2 * table), ((1 << 31) - 1) // slices_of(k) // 3))
            assert chunk == 1 or 2 * chunk * table <= 32 * GIB
            queries.append((('chunk', k, n, 1, 0), (chunk, ceil_div(n, chunk))))
            queries.append((('bbytes', chunk, 4 ** k, 0), 2 * chunk * table))
    plan(queries)


def test_alias(plan):
    bins, n, table = 4096, 10, 4096 * 8
    left = 1 << 20
    plan([(('alias', left, left + n * table, n, bins), (0, 0)),             # the right side begins where the left one ends
          (('alias', left + n * table, left, n, bins), (0, 0)),
          (('alias', left, left + 50 * table + 8, n, bins), (0, 0)),
          (('alias', left, left, n, bins), (1, 0)),                          # the same range
          (('alias', left, left + table, n, bins), (2, 1)),                  # a whole number of tables apart
          (('alias', left + table, left, n, bins), (2, -1)),
          (('alias', left, left + 3 * table, n, bins), (2, 3)),
          (('alias', left + 3 * table, left, n, bins), (2, -3)),
          (('alias', left, left + 9 * table, n, bins), (2, 9)),
          (('alias', left, left + table // 2, n, bins), (3, 0)),             # half a table: no shortcut
          (('alias', left + table // 2, left, n, bins), (3, 0)),
          (('alias', left, left + 3 * table + 16, n, bins), (3, 0)),
          (('alias', left, left + 16, 1, 4), (3, 0)), (('alias', left, left + 32, 1, 4), (0, 0)), (('alias', left, left + 32, 2, 4), (2, 1)),
          # the union of a chunk's two sides: chunk + |lag| tables, none when the sides of the chunk do not meet
          (('union', 10, 1), 11), (('union', 10, -1), 11), (('union', 10, 3), 13), (('union', 10, 9), 19), (('union', 10, 10), 0),
          (('union', 10, -10), 0), (('union', 1, 1), 0), (('union', 10, 0), 10), (('union', 7, -3), 10),
          (('bbytes', 10, bins, 11), 11 * table), (('bbytes', 10, bins, 0), 20 * table), (('bbytes', 10, bins, 10), 10 * table)])
