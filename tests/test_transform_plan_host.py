"""The host decisions about the balance, the shrink and the pool of whole sets of tables without a GPU:
kpal_amd/csrc/transform_plan.hpp -- the persistent grid over the flat list of (table, canonical tile pair) items of a balance,
the column groups and the table slices of a pool, and the test of an output range against an input range -- driven by a
stand-alone program built with the address and undefined-behaviour sanitizers.  Every expected value is a literal written
down from the rule, none is computed with the header.

Balance: `slots` = 2 workgroups per CU; the grid is the smallest that needs no more rounds than `slots` workgroups would
(rounds = ceil(items / slots), grid = ceil(items / rounds)), workgroup g takes items g, g + grid, ...  Pool: a column group is
256 threads with one pair of columns each (512 bins); the tables are cut into min(ceil(8 x CUs / column groups), ceil(tables /
16)) slices, one from 2^20 bins on, the first tables % slices of them one table longer."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'kpal_amd', 'csrc')
SLOTS = 512            # 256 CUs
T64 = 1 << 64


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('transform_plan') / 'transform_plan_check')
    b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-o', exe,
                        os.path.join(ROOT, 'tests', 'native', 'transform_plan_check.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0 and not b.stdout.strip(), b.stdout.decode()[-3000:]

    def ask(queries):
        """[(query words, expected answer)] -> asserts every answer"""
        text = ''.join(' '.join(str(w) for w in q) + '\n' for q, _ in queries)
        r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0 and got[-2] == 'TRANSFORM_PLAN_DONE %d' % len(queries), got[-20:]
        for (q, want), line in zip(queries, got):
            have = tuple(int(w) for w in line.split())
            assert have == (want if isinstance(want, tuple) else (want,)), (q, have, want)
    return ask


def test_header_knows_no_gpu():
    header = re.sub(r'//.*', '', open(os.path.join(CSRC, 'transform_plan.hpp')).read())
    assert not any(w in header for w in ('hip', 'Hip', 'HIP', 'kpal_ctx', 'LAUNCH(', 'getenv', '__global__', '__device__', 'blockIdx'))
    # the kernels and the host take their numbers from it
    for user, names in (('transform_set_kernels.hpp', ('kBalanceSetThreads', 'kPoolThreads', 'kPoolUnroll', 'pool_column_pairs(', 'pool_slice_begin(',
                                                       'pool_slice_end(')),
                        ('kpal_transform.hip', ('balance_set_items(', 'balance_set_slots(', 'balance_set_workgroups(', 'kBalanceSetSmallMaxK',
                                                'kBalanceSetSlotsPerCu', 'kBalanceSetThreads', 'pool_column_groups(', 'pool_slices(',
                                                'pool_scratch_bytes(', 'shrink_set_launches(', 'tables_overlap(', 'transform_bytes_fit(', 'kTransformPartial',
                                                'kTransformDisjoint', 'check_bytes_at_k(', '#include "table_host.hpp"')),
                        # the host front end of the table units: the overlap test and the bytes of a set behind the rungs the entries share
                        ('table_host.hpp', ('transform_overlap(', 'transform_bytes_fit('))):
        text = re.sub(r'//.*', '', open(os.path.join(CSRC, user)).read())
        assert all(n in text for n in names), user
    # the launch names are the set's own: existing tests count the single-table ones
    unit = open(os.path.join(CSRC, 'kpal_transform.hip')).read()
    names = set(re.findall(r'"([a-z_]+)"', unit))
    assert names == {'balance_set', 'balance_tiled_set', 'shrink_set', 'pool_set', 'pool_set_final'}, names
    # the kernels stay quiet
    kernels = re.sub(r'//.*', '', open(os.path.join(CSRC, 'transform_set_kernels.hpp')).read())
    assert 'printf' not in kernels and not re.search(r'(?<!static_)assert\(', kernels) and 'asm' not in kernels


def test_both_shrink_entries_look_at_the_alignment_of_their_input():
    """The shuffle form of the shrink reads 16 bytes at a time, and the hardware may serve such a load from an address aligned
    to 8 bytes only: a result cannot tell which form ran (tests/test_gpu_transform_sets.py compares the results).  So the text
    is looked at: shrink_launch has no default for `in_aligned_16`, and each of its two callers passes what its input has."""
    header = re.sub(r'//.*', '', open(os.path.join(CSRC, 'table_host.hpp')).read())
    declaration = re.search(r'int shrink_launch\(([^;]*)\);', header).group(1)
    assert declaration.rstrip().endswith('bool in_aligned_16') and '=' not in declaration, declaration
    for unit, entry, pointer in (('kpal_vec.hip', 'kpal_shrink_device', 'dev_counts'), ('kpal_transform.hip', 'kpal_shrink_set_device', 'dev_in')):
        text = re.sub(r'//.*', '', open(os.path.join(CSRC, unit)).read())
        body = text[text.index('KPAL_API int %s(' % entry):]
        body = body[:body.index('\n}\n')]
        calls = [line for line in body.split('\n') if 'shrink_launch(' in line]
        assert len(calls) == 1 and re.search(r', \(uintptr_t\)%s %% 16 == 0\)\)?;$' % pointer, calls[0]), (entry, calls)
    launch = re.sub(r'//.*', '', open(os.path.join(CSRC, 'kpal_vec.hip')).read())
    assert 'if (m <= 64 && in_aligned_16) LAUNCH(ctx, name, shrink_small_kernel,' in launch


def test_sizes(plan):
    plan([(('sizes',), (2, 1024, 5, 256, 4, 8, 16, 1048576))])


def test_balance_items_and_slots(plan):
    plan([(('items', 20000, 1), 20000),            # k = 6: a table is one self pair
          (('items', 4000, 10), 40000),            # k = 8: 16 tiles, 4 of them their own partner
          (('items', 64, 2080), 133120),           # k = 12: (4096 + 64) / 2
          (('items', 1, 1), 1),
          (('slots', 256), 512), (('slots', 304), 608), (('slots', 1), 2), (('slots', 0), 2)])


def test_balance_grid(plan):
    plan([(('grid', 1, SLOTS), (1, 1)),
          (('grid', SLOTS - 1, SLOTS), (1, 511)),
          (('grid', SLOTS, SLOTS), (1, 512)),
          (('grid', SLOTS + 1, SLOTS), (2, 257)),            # two rounds: 257 workgroups, not 512 of which 511 have one item
          (('grid', 2 * SLOTS + 1, SLOTS), (3, 342)),        # 1025 / 3 = 341.7
          (('grid', 4400000, SLOTS), (8594, 512)),           # 4400000 / 512 = 8593.75
          (('grid', 0, SLOTS), (0, 0)),
          (('grid', 70, 608), (1, 70)), (('grid', 700, 608), (2, 350))])


def test_balance_shares_differ_by_one_at_most_and_sum_to_the_items(plan):
    plan([(('shares', 1, SLOTS), (1, 1, 1)),
          (('shares', SLOTS - 1, SLOTS), (1, 1, 511)),
          (('shares', SLOTS, SLOTS), (1, 1, 512)),
          (('shares', SLOTS + 1, SLOTS), (1, 2, 513)),       # 256 workgroups with two items, one with one
          (('shares', 2 * SLOTS + 1, SLOTS), (2, 3, 1025)),  # 1025 = 341 x 3 + 2
          (('shares', 4400000, SLOTS), (8593, 8594, 4400000)),   # 4400000 = 512 x 8593 + 384
          (('share', 513, 257, 0), 2), (('share', 513, 257, 255), 2), (('share', 513, 257, 256), 1), (('share', 513, 257, 600), 0),
          (('share', 4400000, 512, 383), 8594), (('share', 4400000, 512, 384), 8593), (('share', 5, 0, 0), 0)])


def test_shrink_launches(plan):
    """One launch over all entries up to k = 11; from k = 12 on, where the one launch was measured to lose, one per table."""
    plan([(('shrinkl', 2, 1), (12, 1)), (('shrinkl', 6, 20000), (12, 1)), (('shrinkl', 8, 4000), (12, 1)), (('shrinkl', 11, 70), (12, 1)),
          (('shrinkl', 12, 1), (12, 1)), (('shrinkl', 12, 64), (12, 64)), (('shrinkl', 16, 3), (12, 3)), (('shrinkl', 6, 0), (12, 0))])


def test_pool_columns(plan):
    plan([(('cols', 4), (2, 1)), (('cols', 64), (32, 1)), (('cols', 512), (256, 1)), (('cols', 513), (257, 2)), (('cols', 4096), (2048, 8)),
          (('cols', 65536), (32768, 128)), (('cols', 1), (1, 1)), (('cols', 1001), (501, 2))])


def test_pool_slices(plan):
    plan([(('slices', 1, 64, 256), 1),
          (('slices', 2, 64, 256), 1),                       # a slice is 16 tables at least
          (('slices', 3, 64, 256), 1), (('slices', 16, 64, 256), 1), (('slices', 17, 64, 256), 2),
          (('slices', 40, 4, 256), 3),
          (('slices', 257, 64, 256), 17),
          (('slices', 3000, 64, 256), 188),                  # 3000 / 16 = 187.5: the tables decide
          (('slices', 20000, 4096, 256), 256),               # 8 column groups: 2048 / 8, the device decides
          (('slices', 4000, 65536, 256), 16),                # 128 column groups
          (('slices', 1000, 262144, 256), 4),                # 512 column groups
          # one slice from the threshold on, whatever the device
          (('slices', 1000, 1048574, 304), 2),               # 2048 column groups against 2432 wanted
          (('slices', 1000, 1048576, 304), 1),
          (('slices', 64, 4 ** 12, 256), 1), (('slices', 100000, 4 ** 10, 10000), 1),
          # never more slices than tables
          (('slices', 5, 4, 100000), 1), (('slices', 33, 4, 100000), 3)])


def test_pool_slices_cover_every_table_once(plan):
    plan([(('slice', 3000, 188, 0), (0, 16)),                # 3000 = 188 x 15 + 180: the first 180 slices have 16 tables
          (('slice', 3000, 188, 179), (2864, 2880)), (('slice', 3000, 188, 180), (2880, 2895)), (('slice', 3000, 188, 187), (2985, 3000)),
          (('slice', 257, 1, 0), (0, 257)),
          (('cover', 3000, 188), (1, 15, 16)), (('cover', 257, 17), (1, 15, 16)), (('cover', 7, 7), (1, 1, 1)),
          (('cover', 20000, 256), (1, 78, 79)), (('cover', 4000, 16), (1, 250, 250)), (('cover', 1, 1), (1, 1, 1)),
          (('pscratch', 1, 64), 0), (('pscratch', 188, 64), 96256), (('pscratch', 256, 4096), 8388608)])


def test_overlap(plan):
    plan([(('overlap', 1000, 800, 1000, 800), 1),            # the same range
          (('overlap', 1000, 800, 1800, 800), 0),            # the output begins where the input ends
          (('overlap', 1800, 800, 1000, 800), 0),
          (('overlap', 1000, 800, 1792, 800), 2),            # one entry of overlap, on either side
          (('overlap', 1792, 800, 1000, 800), 2),
          (('overlap', 1000, 800, 1000, 100), 2),            # the same start is not the same range
          (('overlap', 1000, 800, 1400, 100), 2),            # inside
          (('overlap', 1400, 100, 1000, 800), 2),
          (('overlap', 1000, 800, 200, 800), 0), (('overlap', 1000, 800, 208, 800), 2),
          (('overlap', T64 - 800, 800, 0, 8), 0)])


def test_bytes_fit(plan):
    plan([(('fit', 1, 1), 1), (('fit', 20000, 4096), 1), (('fit', 1 << 60, 1), 1), (('fit', 1 << 61, 1), 0), (('fit', 1 << 32, 1 << 32), 0),
          (('fit', 1 << 29, 1 << 32), 0), (('fit', (1 << 29) - 1, 1 << 32), 1)])
