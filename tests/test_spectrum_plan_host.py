"""The host decisions about the count-of-counts spectra of whole sets of tables without a GPU: kpal_amd/csrc/spectrum_plan.hpp
-- the window of a pass from its widest spread, the counters kept in LDS, the window slices of the compaction, the scratch of
a table, the tables of a pass, and the key arithmetic host and kernels share -- driven by a stand-alone program built with the
address and undefined-behaviour sanitizers.  Every expected value is a literal written down from the rule, none is computed
with the header.

Values are compared as keys: the two's complement word with the sign bit flipped.  The window of a pass is
min(widest (max - min + 1), bins, 2^20) counters; the first min(W, 4096) of them are kept in LDS.  Scratch of a table: 40 bytes
per slice of 8192 bins (the min/max partials), 16 of range, 8 per window counter, 8 per window slice of 2048 counters, 8 of
overflow count.  A pass: 256 MiB of scratch at the widest window the bins allow, at most 65535 tables, at most the caller's
cap, never less than one."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'kpal_amd', 'csrc')
BUDGET = 256 << 20
T63, T64 = 1 << 63, 1 << 64


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('spectrum_plan') / 'spectrum_plan_check')
    b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-o', exe,
                        os.path.join(ROOT, 'tests', 'native', 'spectrum_plan_check.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0 and not b.stdout.strip(), b.stdout.decode()[-3000:]

    def ask(queries):
        """[(query words, expected answer)] -> asserts every answer"""
        text = ''.join(' '.join(str(w) for w in q) + '\n' for q, _ in queries)
        r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0 and got[-2] == 'SPECTRUM_PLAN_DONE %d' % len(queries), got[-20:]
        for (q, want), line in zip(queries, got):
            have = tuple(int(w) for w in line.split())
            assert have == (want if isinstance(want, tuple) else (want,)), (q, have, want)
    return ask


def test_header_knows_no_gpu():
    header = re.sub(r'//.*', '', open(os.path.join(CSRC, 'spectrum_plan.hpp')).read())
    assert not any(w in header for w in ('hip', 'Hip', 'HIP', 'kpal_ctx', 'LAUNCH(', 'getenv', '__global__', '__device__', 'blockIdx'))
    # the kernels and the host take their numbers from it
    for user, names in (('spectrum_kernels.hpp', ('spectrum_key(', 'spectrum_value(', 'spectrum_offset(', 'spectrum_in_window(', 'spectrum_lds_bins(',
                                                  'kSpectrumLdsBins', 'kSpectrumPeels', 'kSpectrumWindowSlice', 'kSpectrumCompactPerThread',
                                                  'kSpectrumScanThreads', 'SpectrumRange', 'SpectrumOverflow', 'stat_slice_begin(', 'stat_slice_end(')),
                        ('kpal_spectrum.hip', ('spectrum_window(', 'spectrum_window_slices(', 'spectrum_scratch_bytes(', 'spectrum_tables_per_pass(',
                                               'spectrum_value(', 'stat_slices(', 'stat_chunks(', 'kStatSetBudgetBytes', 'kSpectrumOverflowBytes',
                                               'stat_set_cap()', 'for_uploaded_chunks(', '#include "table_host.hpp"')),
                        # the cap of a pass is read by the host front end of the table units, there alone
                        ('table_host.hpp', ('getenv("KPAL_STAT_SET_PROFILES")',))):
        text = re.sub(r'//.*', '', open(os.path.join(CSRC, user)).read())
        assert all(n in text for n in names), user
    # no size of the plan restated, one key mapping
    sources = {f: re.sub(r'//.*', '', open(os.path.join(CSRC, f)).read()) for f in ('spectrum_kernels.hpp', 'kpal_spectrum.hip')}
    assert not any(re.search(r'\b(4096|2048|8192|1048576)\b|<< 20', t) for t in sources.values())
    assert not any('0x8000000000000000' in t for t in sources.values())
    # the kernels stay quiet
    assert 'printf' not in sources['spectrum_kernels.hpp'] and not re.search(r'(?<!static_)assert\(', sources['spectrum_kernels.hpp'])


def test_sizes(plan):
    plan([(('sizes',), (1048576, 4096, 1, 2048, 1024, 16, 16, 16, 16))])


def test_key_mapping(plan):
    plan([(('key', T63), 0),                       # INT64_MIN
          (('key', T64 - 1), T63 - 1),             # -1
          (('key', 0), T63),
          (('key', 1), T63 + 1),
          (('key', T63 - 1), T64 - 1),             # INT64_MAX
          (('value', 0), T63), (('value', T63 - 1), T64 - 1), (('value', T63), 0), (('value', T64 - 1), T63 - 1),
          # INT64_MIN and INT64_MAX in one table: the whole range, no wrap
          (('offset', T64 - 1, 0), T64 - 1), (('offset', T63, T63 - 1), 1), (('offset', 5, 5), 0)])


def test_window_test_at_both_edges(plan):
    plan([(('inside', T63, T63, 4096), 1),                  # the smallest key is the window's first counter
          (('inside', T63 + 4095, T63, 4096), 1),           # the last key inside
          (('inside', T63 + 4096, T63, 4096), 0),           # the first key outside
          (('inside', T63, T63, 1), 1), (('inside', T63 + 1, T63, 1), 0),
          (('inside', T64 - 1, 0, 1048576), 0),             # INT64_MAX from a window at INT64_MIN
          (('inside', 1048575, 0, 1048576), 1), (('inside', 1048576, 0, 1048576), 0),
          (('inside', T64 - 1, T64 - 5, 5), 1),             # a window that ends at the top of the range does not wrap
          (('inside', T64 - 1, T64 - 5, 4), 0)])


def test_window_from_a_spread(plan):
    plan([(('window', 0, 100), 1),                          # a constant table
          (('window', 29, 4096), 30),                       # counts 0 .. 29
          (('window', 4095, 4096), 4096), (('window', 4096, 4096), 4096),
          (('window', 5000, 64), 64),                       # never more counters than bins
          (('window', 62, 64), 63), (('window', 63, 64), 64), (('window', 64, 64), 64),
          (('window', 1048574, 4 ** 12), 1048575), (('window', 1048575, 4 ** 12), 1048576), (('window', 1048576, 4 ** 12), 1048576),   # the cap
          (('window', T64 - 1, 4 ** 16), 1048576),          # INT64_MIN with INT64_MAX: the spread itself does not fit a word
          (('window', T64 - 1, 1), 1), (('window', T64 - 2, 4 ** 7), 16384)])


def test_lds_bins_and_window_slices(plan):
    plan([(('lds', 1), 1), (('lds', 30), 30), (('lds', 4095), 4095), (('lds', 4096), 4096), (('lds', 4097), 4096), (('lds', 1048576), 4096),
          (('wslices', 1), 1), (('wslices', 2048), 1), (('wslices', 2049), 2), (('wslices', 4096), 2), (('wslices', 16384), 8),
          (('wslices', 1048576), 512)])


def test_scratch_bytes(plan):
    plan([(('scratch', 1, 1), 80),                          # 40 + 16 + 8 + 8 + 8
          (('scratch', 4096, 30), 312),                     # 40 + 16 + 240 + 8 + 8
          (('scratch', 4096, 4096), 32848),                 # 40 + 16 + 32768 + 2 x 8 + 8
          (('scratch', 8193, 8193), 65688),                 # two slices, five window slices: 80 + 16 + 65544 + 40 + 8
          (('scratch', 4 ** 8, 4 ** 8), 524888),            # 320 + 16 + 524288 + 256 + 8
          (('scratch', 1 << 20, 1 << 20), 8397848),         # 128 slices: 5120 + 16 + 8388608 + 4096 + 8
          (('scratch', 4 ** 12, 1048576), 8474648),         # 81920 + 16 + 8388608 + 4096 + 8
          (('scratch', 4 ** 16, 1048576), 29364248)])       # 20971520 + 16 + 8388608 + 4096 + 8


def test_tables_per_pass(plan):
    plan([(('per', 1, BUDGET, 0), 65535),                   # 80 bytes a table: the grid's limit
          (('per', 4096, BUDGET, 0), 8172),                 # 268435456 / 32848 = 8172.05
          (('per', 4 ** 8, BUDGET, 0), 511),                # / 524888 = 511.4
          (('per', 1 << 20, 256 << 20, 0), 31),             # / 8397848 = 31.96: the seam tests/test_gpu_table_set_seams.py crosses
          (('per', (1 << 20) + 1, BUDGET, 0), 31),
          (('per', 4 ** 12, BUDGET, 0), 31),                # / 8474648 = 31.7
          (('per', 4 ** 16, BUDGET, 0), 9),                 # / 29364248 = 9.1
          (('per', 4096, BUDGET, 2), 2), (('per', 4096, BUDGET, 100000), 8172), (('per', 4 ** 16, 1000, 0), 1), (('per', 4 ** 16, 1000, 5), 1)])
