"""The host decisions about dynamic smoothing over whole sets of profiles without a GPU: kpal_amd/csrc/smooth_plan.hpp -- the
layout of one profile's pyramid of node sums and codes (bottom height first, padded with dead elements to a multiple of the 64
elements a staged rectangle kernel takes at a time), the scratch a set of pyramids needs, and the one rule that says whether a
call is batched -- driven by a stand-alone program built with the address and undefined-behaviour sanitizers.  Every expected
value is a literal written down from the rule, none is computed with the header.

Height h = 0 .. k-1 has 4^(k-1-h) nodes and starts 4^(k-1) + ... + 4^(k-h) elements into the pyramid; (4^k - 1) / 3 nodes in
all; ten bytes of scratch per element (an int64 sum, a code, a flag).

The last rows hold tests/smooth_cases.py -- the Python restatement of the grid rules that the GPU tests of multi-trip shapes
(tests/test_gpu_smooth_sets_trips.py) take their preconditions from -- against this program and matrix_plan_check at 256
compute units, and its trip counts against the literals of smooth_cases.TABLE."""
import os
import re
import shutil
import subprocess

import pytest

import smooth_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PADDING = -1
GIB = 1 << 30


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('smooth_plan') / 'smooth_plan_check')
    b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-o', exe,
                        os.path.join(ROOT, 'tests', 'native', 'smooth_plan_check.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0 and not b.stdout.strip(), b.stdout.decode()[-3000:]

    def ask(queries):
        """[(query words, expected answer)] -> asserts every answer"""
        text = ''.join(' '.join(str(w) for w in q) + '\n' for q, _ in queries)
        r = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0 and got[-2] == 'SMOOTH_PLAN_DONE %d' % len(queries), got[-20:]
        for (q, want), line in zip(queries, got):
            have = tuple(int(w) for w in line.split())
            assert have == (want if isinstance(want, tuple) else (want,)), (q, have, want)
    return ask


def test_header_knows_no_gpu():
    csrc = os.path.join(ROOT, 'kpal_amd', 'csrc')
    header = re.sub(r'//.*', '', open(os.path.join(csrc, 'smooth_plan.hpp')).read())
    assert not any(w in header for w in ('hip', 'Hip', 'HIP', 'kpal_ctx', 'LAUNCH(', 'getenv', '__global__', '__device__', 'blockIdx'))
    # the kernels and the host take the layout from it
    for user, names in (('smooth_set_kernels.hpp', ('smooth_level_offset(', 'smooth_level_nodes(', 'smooth_element(')),
                        ('kpal_cross.hip', ('smooth_stride(', 'smooth_scratch_bytes(', 'smooth_batched('))):
        text = open(os.path.join(csrc, user)).read()
        assert all(n in text for n in names), user
    # one summarise4 for the pair pipeline and the pyramids
    assert sum('double summarise4(' in open(os.path.join(csrc, f)).read() for f in os.listdir(csrc)) == 1


def test_levels_and_stride(plan):
    plan([
        # k = 1: the root alone
        (('nodes', 1), 1), (('stride', 1), 64), (('level', 1, 0), (0, 1)),
        # k = 2: four nodes of four bins, then the root
        (('nodes', 2), 5), (('stride', 2), 64), (('level', 2, 0), (0, 4)), (('level', 2, 1), (4, 1)),
        # k = 6: 1024 + 256 + 64 + 16 + 4 + 1 = 1365 -> 22 x 64 = 1408
        (('nodes', 6), 1365), (('stride', 6), 1408),
        (('level', 6, 0), (0, 1024)), (('level', 6, 1), (1024, 256)), (('level', 6, 2), (1280, 64)), (('level', 6, 3), (1344, 16)),
        (('level', 6, 4), (1360, 4)), (('level', 6, 5), (1364, 1)),
        # k = 7: 4096 + 1024 + 256 + 64 + 16 + 4 + 1 = 5461 -> 86 x 64 = 5504
        (('nodes', 7), 5461), (('stride', 7), 5504),
        (('level', 7, 0), (0, 4096)), (('level', 7, 1), (4096, 1024)), (('level', 7, 2), (5120, 256)), (('level', 7, 3), (5376, 64)),
        (('level', 7, 4), (5440, 16)), (('level', 7, 5), (5456, 4)), (('level', 7, 6), (5460, 1)),
        # a sum that is a multiple of 64 needs a whole chunk more?  no: k = 4 has 85 nodes -> 128
        (('nodes', 4), 85), (('stride', 4), 128),
        # k = 16: (2^32 - 1) / 3 nodes; the root is the last one
        (('nodes', 16), 1431655765), (('stride', 16), 1431655808), (('level', 16, 15), (1431655764, 1)), (('level', 16, 0), (0, 1 << 30))])


def test_elements(plan):
    q = [(('element', 1, 0), (0, 0)), (('element', 1, 1), (PADDING, 0)), (('element', 1, 63), (PADDING, 62)),
         (('element', 2, 0), (0, 0)), (('element', 2, 3), (0, 3)), (('element', 2, 4), (1, 0)), (('element', 2, 5), (PADDING, 0))]
    # first and last element of every height of k = 6 and k = 7, and the padding behind the root
    for k, starts in ((6, (0, 1024, 1280, 1344, 1360, 1364)), (7, (0, 4096, 5120, 5376, 5440, 5456, 5460))):
        for h, at in enumerate(starts):
            count = 4 ** (k - 1 - h)
            q += [(('element', k, at), (h, 0)), (('element', k, at + count - 1), (h, count - 1))]
    q += [(('element', 6, 1365), (PADDING, 0)), (('element', 6, 1407), (PADDING, 42)), (('element', 7, 5461), (PADDING, 0)),
          (('element', 7, 5503), (PADDING, 42)), (('element', 6, 1100), (1, 76))]
    plan(q)


def test_scratch_bytes(plan):
    plan([(('scratch', 1, 2), 1280),                   # 2 x 64 x 10
          (('scratch', 6, 50), 704000),                # 50 x 1408 x 10
          (('scratch', 7, 35), 1926400),               # 35 x 5504 x 10
          (('scratch', 12, 128), 7158333440),          # 128 x 5592448 x 10 (5592405 nodes -> 87382 x 64)
          (('scratch', 15, 1), 3579139840)])           # 357913941 nodes -> 357913984: 2.7 GiB of sums, 3.3 GiB with the bytes


def test_batched(plan):
    plan([(('budget',), 32 * GIB),
          # exactly at the budget, one byte under it
          (('batched', 6, 17, 33, 0, 704000), 1), (('batched', 6, 17, 33, 0, 703999), 0),
          # a triangle counts its one set
          (('batched', 6, 50, 0, 0, 704000), 1), (('batched', 6, 51, 0, 0, 704000), 0),
          # positive masks come before the smoothing: never batched
          (('batched', 6, 17, 33, 1, 704000), 0), (('batched', 1, 1, 1, 1, 32 * GIB), 0),
          # k = 15 at 32 GiB: 9 pyramids of 3579139840 bytes fit, 10 do not; k = 16: 2 fit, 3 do not
          (('batched', 15, 4, 5, 0, 32 * GIB), 1), (('batched', 15, 5, 5, 0, 32 * GIB), 0),
          (('batched', 16, 1, 1, 0, 32 * GIB), 1), (('batched', 16, 2, 1, 0, 32 * GIB), 0),
          (('batched', 12, 64, 64, 0, 32 * GIB), 1)])


@pytest.fixture(scope='module')
def answers(tmp_path_factory):
    """ask(program, [query words]) -> [tuple of ints]: the answers of matrix_plan_check / smooth_plan_check, nothing asserted"""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exes = {}
    for name in ('matrix_plan_check', 'smooth_plan_check'):
        exes[name] = str(tmp_path_factory.mktemp(name) / name)
        b = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-o', exes[name],
                            os.path.join(ROOT, 'tests', 'native', name + '.cpp')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert b.returncode == 0 and not b.stdout.strip(), b.stdout.decode()[-3000:]

    def ask(name, queries):
        text = ''.join(' '.join(str(int(w)) if not isinstance(w, str) else w for w in q) + '\n' for q in queries)
        r = subprocess.run([exes[name]], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        got = r.stdout.decode().split('\n')
        assert r.returncode == 0 and got[-2].endswith('_PLAN_DONE %d' % len(queries)), got[-20:]
        return [tuple(int(w) for w in line.split()) for line in got[:len(queries)]]
    return ask


@pytest.mark.parametrize('shape', sorted(smooth_cases.TABLE), ids=lambda s: 'k%d_%dx%d%s' % (s[0], s[1], s[2], '_tri' if s[3] else ''))
def test_trips_restatement_is_the_headers(answers, shape):
    """smooth_cases' cross_staged, cross_grid, option_totals_gx, smooth_stride and smooth_level_* give what the headers give,
    at every shape of the table and every height."""
    k, Q, R, tri = shape
    cu, n = smooth_cases.TABLE_CU, 4 ** k
    nprof = Q if tri else Q + R
    staged = smooth_cases.cross_staged(Q, R, n)
    units, gx = smooth_cases.cross_grid(cu, Q, R, n, tri, staged)
    stride = smooth_cases.smooth_stride(k)
    ntiles = ((Q + 3) // 4) * ((Q + 3) // 4 + 1) // 2 if tri else ((Q + 3) // 4) * ((R + 3) // 4)
    got = answers('matrix_plan_check', [('staged', Q, R, n), ('grid', cu, Q, R, n, tri, staged), ('grid', cu, Q, R, stride, tri, staged), ('gxt', cu, nprof, stride)]
                  + [('gxt', cu, nprof, smooth_cases.smooth_level_nodes(k, h)) for h in range(k)])
    assert got[0] == (int(staged),)
    assert got[1] == (units, gx, 16 * ntiles, (R + 3) // 4, (R + 15) // 16)
    assert got[3] == (smooth_cases.option_totals_gx(cu, nprof, stride),)
    assert got[4:] == [(smooth_cases.option_totals_gx(cu, nprof, smooth_cases.smooth_level_nodes(k, h)),) for h in range(k)]
    # the pyramid pass is launched with the grid of the bins, whatever cross_grid would make of the pyramids' own length
    assert got[2][1] <= gx
    got = answers('smooth_plan_check', [('stride', k), ('nodes', k)] + [('level', k, h) for h in range(k)])
    assert got[0] == (stride,) and got[1] == (smooth_cases.smooth_nodes(k),) and stride % smooth_cases.SUPER_BINS == 0
    assert got[2:] == [(smooth_cases.smooth_level_offset(k, h), smooth_cases.smooth_level_nodes(k, h)) for h in range(k)]


@pytest.mark.parametrize('shape', sorted(smooth_cases.TABLE), ids=lambda s: 'k%d_%dx%d%s' % (s[0], s[1], s[2], '_tri' if s[3] else ''))
def test_trips_of_the_table(shape):
    """The trip counts at 256 compute units are the literals of the table, and every shape has a loop that goes round twice."""
    k, Q, R, tri = shape
    want = smooth_cases.TABLE[shape]
    t = smooth_cases.trips(smooth_cases.TABLE_CU, k, Q, R, tri)
    assert (t['staged'], t['units'], t['gx'], t['bins'], t['pyramid']) == (want['staged'], want['units'], want['gx'], want['bins'], want['pyramid']), t
    assert t['first'] == want['gx'] * (64 if want['staged'] else 256)
    if want['level0'] is not None:
        assert (t['levels'][0], t['codes']) == (want['level0'], want['codes']), t
    assert len(t['levels']) == k and t['levels'][k - 1] == (1, 1)
    assert t['bins'][1] >= 2


def test_trips_by_hand():
    """_span and last_trip_chunk on ranges small enough to count on one's fingers."""
    span, last = smooth_cases._span, smooth_cases.last_trip_chunk
    assert span(10, 4) == (2, 3)          # walkers 0, 1 take three items (0 4 8, 1 5 9), walkers 2, 3 two
    assert span(8, 4) == (2, 2) and span(3, 4) == (1, 1) and span(4, 4) == (1, 1) and span(5, 4) == (1, 2) and span(1, 256) == (1, 1)
    assert last(10, 4, 0) == (8, 2) and last(10, 4, 1) == (9, 2) and last(10, 4, 3) == (7, 1) and last(4096, 1024, 5) == (3077, 3)
    # one-trip shapes of tests/test_gpu_smooth_sets.py: what the new module is for
    for k, Q, R in ((6, 17, 33), (7, 17, 18), (6, 3, 40), (6, 5, 7)):
        t = smooth_cases.trips(256, k, Q, R)
        assert t['bins'] == (1, 1) and t['pyramid'] == (1, 1) and t['codes'][1] == 1 and all(l == (1, 1) for l in t['levels']), (k, Q, R, t)


def test_codes_reference_by_hand():
    """k = 2: sixteen bins, four height-0 nodes, the root -- codes written down from the definitions."""
    table = [5, 5, 5, 5, 0, 9, 9, 9, 5, 5, 5, 5, 1, 1, 1, 1]
    r = smooth_cases.codes_reference(table, 2, 'min', 0)                 # node 1 has a zero quarter; the root's quarters are 20, 27, 20, 4
    assert [s.tolist() for s in r['sums']] == [[20, 27, 20, 4], [71]]
    assert [c.tolist() for c in r['codes']] == [[0, 1, 0, 0], [0]] and r['dead_bins'].tolist() == [False] * 4 + [True] * 4 + [False] * 8
    assert r['pyramid'].tolist() == [0, 1, 0, 0, 0] + [2] * 59
    r = smooth_cases.codes_reference(table, 2, 'average', 17.75)        # the root's average is 17.75: a tie collapses; node 3's is 1
    assert [f.tolist() for f in r['flags']] == [[True, True, True, True], [True]]
    assert [c.tolist() for c in r['codes']] == [[2, 2, 2, 2], [1]] and r['dead_bins'].all()
    r = smooth_cases.codes_reference(table, 2, 'median', 5)              # medians 5, 9, 5, 1 and (20 + 20) / 2
    assert [c.tolist() for c in r['codes']] == [[1, 0, 1, 1], [0]]
