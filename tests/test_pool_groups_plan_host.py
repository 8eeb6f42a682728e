"""The host decisions about the pool of a set of tables by label without a GPU: kpal_amd/csrc/pool_groups_plan.hpp -- the
inverted index of the labels, the cut of long member lists into chunks, the packing of small tables and the sizes it refuses --
driven by a stand-alone program built with the address and undefined-behaviour sanitizers.  Every expected value is a literal
written down from the rule, none is computed with the header.

The rule: a column group is 256 threads with one pair of columns each (512 bins).  chunk_tables = max(16, ceil(tables / ceil(8 x
CUs / column groups))), the whole set from 2^20 bins on; a list of L tables is cut into ceil(L / chunk_tables) chunks, the first
L % chunks of them one table longer.  Without a cut the items are the groups (one launch, no scratch); with one the items are
the chunks in group order, one partial row of bins x 8 bytes each.  The index is members | begin[items + 1] | with a cut
group_begin[groups + 1], 4 bytes a word.  An item takes the power of two of threads that holds its column pairs, 256 at most."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'kpal_amd', 'csrc')


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('pool_groups_plan') / 'pool_groups_plan_check')
    b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-o', exe,
                        os.path.join(ROOT, 'tests', 'native', 'pool_groups_plan_check.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0 and not b.stdout.strip(), b.stdout.decode()[-3000:]

    def ask(queries):
        """[(query words, expected answer)] -> asserts every answer"""
        text = ''.join(' '.join(str(w) for w in q) + '\n' for q, _ in queries)
        r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0 and got[-2] == 'POOL_GROUPS_PLAN_DONE %d' % len(queries), got[-20:]
        for (q, want), line in zip(queries, got):
            have = tuple(int(w) for w in line.split())
            assert have == (want if isinstance(want, tuple) else (want,)), (q, have, want)
    return ask


def test_header_knows_no_gpu_and_the_unit_has_two_launch_names():
    header = re.sub(r'//.*', '', open(os.path.join(CSRC, 'pool_groups_plan.hpp')).read())
    assert not any(w in header for w in ('hip', 'Hip', 'HIP', 'kpal_ctx', 'LAUNCH(', 'getenv', '__global__', '__device__', 'blockIdx'))
    # the kernels and the host take their numbers from it, and the cut from the pool of a whole set
    for user, names in (('pool_groups_plan.hpp', ('transform_plan.hpp', 'kPoolGroupsPerCu', 'kPoolMinSliceTables', 'kPoolOneSliceBins', 'pool_column_groups(',
                                                  'transform_bytes_fit(')),
                        ('pool_groups_kernels.hpp', ('pool_groups_plan.hpp', 'kPoolThreads', 'kPoolUnroll', 'kPoolGroupsFinalUnroll', 'pool_column_pairs(')),
                        ('kpal_pool_groups.hip', ('pool_groups_plan(', 'pool_groups_fit(', 'pool_groups_lane_shift(', 'pool_groups_item_workgroups(',
                                                  'pool_column_groups(', 'tables_overlap(', 'kTransformDisjoint', 'kPoolGroupsMaxGridY',
                                                  '#include "table_host.hpp"')),
                        ('table_host.hpp', ('transform_overlap(',))):
        text = re.sub(r'//.*', '', open(os.path.join(CSRC, user)).read())
        assert all(n in text for n in names), user
    unit = open(os.path.join(CSRC, 'kpal_pool_groups.hip')).read()
    assert set(re.findall(r'"([a-z_]+)"', unit)) == {'pool_groups', 'pool_groups_final'}
    assert unit.count('LAUNCH(') == 4      # the four forms of one kernel, in the one function both passes go through
    # the kernels stay quiet
    kernels = re.sub(r'//.*', '', open(os.path.join(CSRC, 'pool_groups_kernels.hpp')).read())
    assert 'printf' not in kernels and not re.search(r'(?<!static_)assert\(', kernels) and 'asm' not in kernels


def test_sizes(plan):
    plan([(('sizes',), (2147483647, 65535, 16))])


def test_chunk_tables(plan):
    plan([(('ct', 3000, 64, 256), 16),                 # one column group, 2048 wanted: 3000 / 2048 -> 2, never below 16
          (('ct', 1, 64, 256), 16),
          (('ct', 20000, 4096, 256), 79),              # 8 column groups: 256 chunks wanted, 20000 / 256 = 78.1
          (('ct', 100000, 256, 256), 49),              # 100000 / 2048 = 48.8
          (('ct', 4000, 65536, 256), 250),             # 128 column groups: 16 chunks wanted
          (('ct', 3000, 64, 0), 375),                  # no CU count: one CU, 8 chunks wanted
          (('ct', 1000, 1048574, 304), 500),           # 2048 column groups against 2432 wanted: 2 chunks
          # from 2^20 bins on the column groups fill the device: the whole set, whatever the device
          (('ct', 1000, 1048576, 304), 1000), (('ct', 5, 1048576, 256), 5), (('ct', 64, 4 ** 12, 256), 64), (('ct', 100000, 4 ** 10, 10000), 100000)])


def test_chunks_of_a_list(plan):
    plan([(('chunks', 0, 16), 0), (('chunks', 1, 16), 1), (('chunks', 16, 16), 1), (('chunks', 17, 16), 2), (('chunks', 3000, 16), 188),
          (('chunks', 2700, 16), 169), (('chunks', 18000, 79), 228), (('chunks', 312, 79), 4)])


def test_small_tables_share_a_workgroup(plan):
    plan([(('lanes', 1), (0, 256)), (('lanes', 3), (1, 128)), (('lanes', 4), (1, 128)), (('lanes', 16), (3, 32)), (('lanes', 64), (5, 8)),
          (('lanes', 128), (6, 4)), (('lanes', 256), (7, 2)), (('lanes', 258), (8, 1)), (('lanes', 1001), (8, 1)), (('lanes', 1024), (8, 1)),
          (('lanes', 4 ** 12), (8, 1)),
          (('iwg', 3000, 64), 375), (('iwg', 3001, 64), 376), (('iwg', 200, 256), 100), (('iwg', 7, 4096), 7), (('iwg', 0, 64), 0)])


def test_every_lane_shift_below_a_wave_and_the_first_two_of_whole_waves(plan):
    """The bins tests/test_gpu_pool_groups.py launches to reach the shifts 0 to 4, 6 and 7 (PACKED_BINS)."""
    plan([(('lanes', 1), (0, 256)), (('lanes', 2), (0, 256)), (('lanes', 3), (1, 128)), (('lanes', 4), (1, 128)), (('lanes', 5), (2, 64)),
          (('lanes', 16), (3, 32)), (('lanes', 17), (4, 16)), (('lanes', 32), (4, 16)), (('lanes', 100), (6, 4)), (('lanes', 128), (6, 4)),
          (('lanes', 129), (7, 2)), (('lanes', 512), (8, 1)),
          (('iwg', 3000, 1), 12), (('iwg', 3000, 17), 188), (('iwg', 3000, 100), 750), (('iwg', 291, 100), 73), (('iwg', 65605, 512), 65605)])


def test_member_lists_keep_table_order(plan):
    #                bins CUs groups labels ...           status bad cut items members ct scratch | members | begin
    plan([(('labels', 64, 256, 3, 1, 0, 1, -1, 2, 0, 1), (0, -1, 0, 3, 6, 16, 0, 1, 5, 0, 2, 6, 4, 0, 2, 5, 6)),
          # negative labels are dropped, groups without a table keep their (empty) item
          (('labels', 64, 256, 4, 2, -5, 2), (0, -1, 0, 4, 2, 16, 0, 0, 2, 0, 0, 0, 2, 2)),
          (('labels', 64, 256, 2, -1, -1), (0, -1, 0, 2, 0, 16, 0, 0, 0, 0)),
          # a label == groups is refused, with the table that carries it
          (('labels', 64, 256, 2, 0, 1, 2, 0), (1, 2, 0, 0, 0, 16, 0)),
          (('pattern', 'last', 40, 3, 64, 256), (1, 39, 0, 0, 0, 16, 0, 0, 0, 0, 0, 0)),
          # 17 tables of group 0 around one of group 1: chunks of 9 and 8, the single table a chunk of its own; then the groups' chunks
          (('labels', 64, 256, 2, 0, 0, 0, 1) + (0,) * 14,
           (0, -1, 1, 3, 18, 16, 1536, 0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 3, 0, 9, 17, 18, 0, 2, 3))])


def test_cuts(plan):
    #      status bad cut items members ct scratch index_bytes shortest longest empty sound
    plan([(('pattern', 'one', 3000, 1, 64, 256), (0, -1, 1, 188, 3000, 16, 96256, 12764, 15, 16, 0, 1)),       # 3000 = 188 x 15 + 180
          (('pattern', 'each', 3000, 3000, 64, 256), (0, -1, 0, 3000, 3000, 16, 0, 24004, 1, 1, 0, 1)),        # one launch
          # 2700 tables in group 0, 300 groups of one: only the long list is cut, into 169 chunks of 15 or 16
          (('pattern', 'skew', 3000, 301, 64, 256), (0, -1, 1, 469, 3000, 16, 240128, 15088, 1, 16, 0, 1)),
          (('pattern', 'one', 2700, 1, 64, 256), (0, -1, 1, 169, 2700, 16, 86528, 11488, 15, 16, 0, 1)),
          # interleaved labels, 64 groups of 312 or 313 at k = 6: 4 chunks each
          (('pattern', 'mod', 20000, 64, 4096, 256), (0, -1, 1, 256, 20000, 79, 8388608, 81288, 78, 79, 0, 1)),
          # groups nobody is in: 40 tables over 100 groups
          (('pattern', 'mod', 40, 100, 64, 256), (0, -1, 0, 100, 40, 16, 0, 564, 1, 1, 60, 1)),
          # never cut from 2^20 bins on
          (('pattern', 'one', 3000, 1, 1 << 20, 256), (0, -1, 0, 1, 3000, 3000, 0, 12008, 3000, 3000, 0, 1)),
          (('pattern', 'skew', 3000, 301, 1 << 22, 8), (0, -1, 0, 301, 3000, 3000, 0, 13208, 1, 2700, 0, 1))])


def test_scratch_and_refusals(plan):
    plan([(('pscratch', 0, 188, 64), 0), (('pscratch', 1, 188, 64), 96256), (('pscratch', 1, 256, 4096), 8388608),
          (('fit', 1, 1, 1), 1), (('fit', 5, 2, 1 << 20), 1),
          (('fit', (1 << 31) - 1, 1, 1), 1), (('fit', 1 << 31, 1, 1), 0),              # tables are 32-bit words of the index
          (('fit', 1, (1 << 31) - 1, 1), 1), (('fit', 1, 1 << 31, 1), 0),              # and so are groups
          (('fit', 1, 1, 1 << 39), 1), (('fit', 1, 1, 1 << 40), 0),                    # 2^31 column groups
          (('fit', 1 << 22, 1, 1 << 39), 0), (('fit', 1, 1 << 22, 1 << 39), 0),        # 2^64 bytes of tables, of output
          (('fit', 1 << 21, 1 << 21, 1 << 39), 1)])
