"""The host decisions about the summaries and the strand balance of whole sets of profiles without a GPU:
kpal_amd/csrc/stat_plan.hpp -- the slices one table is cut into (a function of its bins alone), the scratch of a profile, the
profiles of a pass and the bounds of the passes, the grid of the strand balance, and the arithmetic the single-profile and
the set entry share (the mean of a 128-bit sum, the digits a radix select runs) -- driven by a stand-alone program built with
the address and undefined-behaviour sanitizers.  Every expected value is a literal written down from the rule, none is
computed with the header.

A slice is 8192 bins: 256 threads of a workgroup, 32 entries each.  Scratch of a profile: 40 bytes per slice (128-bit sum,
non-zero count, min, max), 2048 of histogram, 48 of select state, 56 of finished summary.  A pass: 256 MiB of scratch, at most
65535 profiles (the second dimension of a grid), at most the caller's cap, never less than one."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'kpal_amd', 'csrc')
BUDGET = 256 << 20


def bits(value):
    return struct.unpack('<Q', struct.pack('<d', value))[0]


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('stat_plan') / 'stat_plan_check')
    b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-o', exe,
                        os.path.join(ROOT, 'tests', 'native', 'stat_plan_check.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0 and not b.stdout.strip(), b.stdout.decode()[-3000:]

    def ask(queries):
        """[(query words, expected answer)] -> asserts every answer"""
        text = ''.join(' '.join(str(w) for w in q) + '\n' for q, _ in queries)
        r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0 and got[-2] == 'STAT_PLAN_DONE %d' % len(queries), got[-20:]
        for (q, want), line in zip(queries, got):
            have = tuple(int(w) for w in line.split())
            assert have == (want if isinstance(want, tuple) else (want,)), (q, have, want)
    return ask


def test_header_knows_no_gpu():
    header = re.sub(r'//.*', '', open(os.path.join(CSRC, 'stat_plan.hpp')).read())
    assert not any(w in header for w in ('hip', 'Hip', 'HIP', 'kpal_ctx', 'LAUNCH(', 'getenv', '__global__', '__device__', 'blockIdx'))
    # the kernels and the host take their numbers from it
    for user, names in (('stat_set_kernels.hpp', ('stat_slice_begin(', 'stat_slice_end(', 'stat_mean(', 'stat_top_byte(', 'stat_mask_above(',
                                                  'StatSetState', 'kStatSetThreads', 'kStatHistBins', 'kStatPartialBytes')),
                        ('kpal_sets.hip', ('stat_slices(', 'stat_scratch_bytes(', 'stat_profiles_per_pass(', 'stat_chunks(', 'balance_set_grid(',
                                           'balance_set_scratch_bytes(', 'kStatSetBudgetBytes', 'stat_set_cap()', 'for_uploaded_chunks(',
                                           '#include "table_host.hpp"')),
                        # the host front end of the table units: the cap of a pass and the tables of an upload
                        ('table_host.hpp', ('getenv("KPAL_STAT_SET_PROFILES")', 'stat_chunks(', 'stat_upload_tables(')),
                        ('kpal_vec.hip', ('stat_mean(',))):
        text = re.sub(r'//.*', '', open(os.path.join(CSRC, user)).read())
        assert all(n in text for n in names), user
    # one conversion of the 128-bit sum for the single-profile and the set entry, and no slice size restated
    sources = {f: re.sub(r'//.*', '', open(os.path.join(CSRC, f)).read()) for f in os.listdir(CSRC)}
    assert [f for f, t in sources.items() if '18446744073709551616.0' in t or 'ldexp' in t] == ['stat_plan.hpp']
    # one reader of the cap's environment variable, one upload budget
    assert [(f, t.count('"KPAL_STAT_SET_PROFILES"')) for f, t in sources.items() if 'KPAL_STAT_SET_PROFILES' in t] == [('table_host.hpp', 1)]
    assert [(f, len(re.findall(r'=\s*1ULL << 30', t))) for f, t in sources.items() if 'UploadBytes' in t] == [('stat_plan.hpp', 1)]
    assert not any('8192' in sources[f] for f in ('stat_set_kernels.hpp', 'kpal_sets.hip'))
    # the set kernels stay quiet
    assert 'printf' not in sources['stat_set_kernels.hpp'] and not re.search(r'(?<!static_)assert\(', sources['stat_set_kernels.hpp'])


def test_sizes_and_limits(plan):
    plan([(('sizes',), (256, 8192, 40, 2048, 48, 56)), (('limits',), (BUDGET, 65535))])


def test_slices(plan):
    plan([(('slices', 1), 1), (('slices', 4), 1), (('slices', 16), 1), (('slices', 64), 1), (('slices', 255), 1), (('slices', 256), 1),
          (('slices', 257), 1), (('slices', 1001), 1), (('slices', 4 ** 6), 1), (('slices', 8191), 1), (('slices', 8192), 1),
          (('slices', 8193), 2), (('slices', 4 ** 7), 2), (('slices', 24576), 3), (('slices', 24577), 4), (('slices', 4 ** 8), 8),
          (('slices', 4 ** 12), 2048), (('slices', 4 ** 16), 524288),
          # bounds: the last slice is short when the bins are no multiple
          (('slice', 1, 0), (0, 1)), (('slice', 1001, 0), (0, 1001)), (('slice', 8192, 0), (0, 8192)), (('slice', 8193, 0), (0, 8192)),
          (('slice', 8193, 1), (8192, 8193)), (('slice', 4 ** 8, 7), (57344, 65536)), (('slice', 4 ** 16, 524287), (4294959104, 4294967296))])


def test_scratch_bytes(plan):
    plan([(('scratch', 1), 2192),                  # 40 + 2048 + 48 + 56
          (('scratch', 4 ** 6), 2192),
          (('scratch', 8193), 2232),               # two slices
          (('scratch', 4 ** 8), 2472),             # 8 x 40 + 2152
          (('scratch', 4 ** 12), 84072),           # 2048 x 40 + 2152
          (('scratch', 4 ** 16), 20973672)])       # 524288 x 40 + 2152


def test_profiles_per_pass(plan):
    plan([(('per', 2192, BUDGET, 0), 65535),       # 122461 fit: the grid's limit
          (('per', 84072, BUDGET, 0), 3192),       # k = 12: 268435456 / 84072 = 3192.9
          (('per', 20973672, BUDGET, 0), 12),      # k = 16
          (('per', 2192, BUDGET, 7), 7), (('per', 2192, BUDGET, 1), 1), (('per', 2192, BUDGET, 100000), 65535),
          (('per', 84072, BUDGET, 5000), 3192),    # a cap can only lower it
          (('per', 2192, 2191, 0), 1), (('per', 2192, 0, 0), 1), (('per', 20973672, 1000, 9), 1),   # a budget below one profile's scratch
          (('per', 2192, 2192, 0), 1), (('per', 2192, 4384, 0), 2), (('per', 0, BUDGET, 0), 65535),
          (('per', 16, BUDGET, 0), 65535), (('per', 16777216, BUDGET, 0), 16)])                 # strand balance: k <= 6, k = 16


def test_chunks(plan):
    plan([(('chunks', 1, 7), (0, 1)), (('chunks', 7, 7), (0, 7)), (('chunks', 8, 7), (0, 7, 7, 1)), (('chunks', 20, 7), (0, 7, 7, 7, 14, 6)),
          (('chunks', 65535, 65535), (0, 65535)), (('chunks', 65536, 65535), (0, 65535, 65535, 1)),
          (('chunks', 3, 1), (0, 1, 1, 1, 2, 1)), (('chunks', 3, 0), (0, 1, 1, 1, 2, 1)), (('chunks', 0, 7), ())])


def test_upload_tables(plan):
    """Host tables go up max(1, 1 GiB / (bins * 8)) at a time: a table larger than the budget still goes alone."""
    gib = 1 << 30
    plan([(('upload', 256), (524288, gib)), (('upload', 4 ** 12), (8, gib)), (('upload', 4 ** 13), (2, gib)), (('upload', 4 ** 14), (1, gib)),
          (('upload', 4 ** 16), (1, gib)), (('upload', 1), (134217728, gib)), (('upload', 3), (44739242, gib)), (('upload', 4 ** 13 + 1), (1, gib))])


def test_balance_grid(plan):
    plan([(('bgrid', 1), (1, 16)), (('bgrid', 2), (1, 16)), (('bgrid', 3), (1, 16)), (('bgrid', 4), (1, 16)), (('bgrid', 5), (4, 64)),
          (('bgrid', 6), (1, 16)), (('bgrid', 7), (4, 64)), (('bgrid', 8), (16, 256)), (('bgrid', 12), (4096, 65536)),
          (('bgrid', 16), (1048576, 16777216))])


def test_shared_arithmetic(plan):
    two64 = 1 << 64
    plan([(('sum128', 10, 0), bits(10.0)), (('sum128', 0, 1), bits(2.0 ** 64)), (('sum128', two64 - 3, two64 - 1), bits(-3.0)),
          (('sum128', 0, two64 - 1), bits(-2.0 ** 64)), (('sum128', 0, 0), bits(0.0)), (('sum128', 1 << 63, 0), bits(2.0 ** 63)),
          (('sum128', 1, 1), bits(2.0 ** 64)),                      # 2^64 + 1 rounds to 2^64
          (('mean', 10, 0, 4), bits(2.5)), (('mean', two64 - 3, two64 - 1, 2), bits(-1.5)), (('mean', 0, 1, 1 << 20), bits(2.0 ** 44)),
          (('mean', 1, 0, 3), bits(1.0 / 3.0)),
          # keys are values with the sign bit flipped
          (('top', 1 << 63, 1 << 63), -1), (('top', 1 << 63, (1 << 63) + 5), 0), (('top', 1 << 63, (1 << 63) + 256), 1),
          (('top', (1 << 63) - 1, 1 << 63), 7), (('top', 0, two64 - 1), 7), (('top', 1 << 63, (1 << 63) + 10 ** 12), 4),
          (('top', (1 << 63) + 255, (1 << 63) + 256), 1), (('top', (1 << 63) + 65535, (1 << 63) + 65536), 2),
          (('mask', 7), 0), (('mask', 6), 0xFF00000000000000), (('mask', 3), 0xFFFFFFFF00000000), (('mask', 0), 0xFFFFFFFFFFFFFF00)])
