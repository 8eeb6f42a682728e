"""The rectangle of distances between two sets of profiles (kpal_cross_distance, kdistlib.cross_distances, ``kpal cross``):
what can be checked without a GPU -- the ABI, the command line, the text format, ``nearest``, the chunk plan, and that the
boundary profile sets of the GPU tests sit where they say when they are split into a left and a right set."""
import io
import os

import numpy as np
import pytest

import matrix_cases
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cross_symbols():
    import re
    from kpal_amd import _native
    header = open(os.path.join(ROOT, 'include', 'kpal_hip.h')).read()
    declared = set(re.findall(r'\b(kpal_[a-z0-9_]+)\s*\(', header))
    L = _native.load()
    for name in ('kpal_cross_distance', 'kpal_cross_distance_device'):
        assert name in declared and name in _native.SIGNATURES and hasattr(L, name), name
    assert hasattr(_native.Context, 'cross_distance') and hasattr(_native.Context, 'cross_distance_device')


def test_cross_command_parses(tmp_path, monkeypatch):
    import memh5
    from kpal_amd import files, kmer
    store = memh5.Store()
    monkeypatch.setattr(files, 'open_profile_file', store.open)
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'a_1.fa').write_text('>r\nACGT\n')
    for name in ('counted.k8', 'merged.k8'):
        files.ProfileFileType('w')(name)
    parser = kmer.build_parser()
    args = parser.parse_args(['cross', 'counted.k8', 'merged.k8', 'x.txt'])
    ref = parser.parse_args(['matrix', 'counted.k8', 'm.txt'])
    for key in ('precision', 'pairwise', 'distance_function', 'summary', 'threshold', 'do_balance', 'do_positive', 'do_scale',
                'do_smooth', 'down', 'custom_pairwise', 'custom_summary'):
        assert getattr(args, key) == getattr(ref, key), key
    assert (args.nearest, args.names_left, args.names_right, args.func) == (None, None, None, kmer.cross)
    args = parser.parse_args(['cross', 'counted.k8', 'merged.k8', 'y.txt', '--nearest', '3', '-l', 'a', '-r', 'b', 'c', '-b', '-P', 'sum'])
    assert (args.nearest, args.names_left, args.names_right, args.do_balance, args.pairwise) == (3, ['a'], ['b', 'c'], True, 'sum')
    with pytest.raises(SystemExit) as exc:
        parser.parse_args(['cross', 'counted.k8', 'merged.k8'])      # no OUTPUT
    assert exc.value.code == 2
    # the seventeen sub-commands of the reference still parse what they parsed
    args = parser.parse_args(['count', 'a_1.fa', 'out.k9'])
    assert (args.size, args.by_record, args.names) == (9, False, None)
    assert parser.parse_args(['shrink', 'counted.k8', 's.k7']).factor == 1
    args = parser.parse_args(['merge', 'counted.k8', 'merged.k8', 'mm.k8'])
    assert (args.merger, args.custom_merger) == ('sum', None)
    assert parser.parse_args(['distance', 'counted.k8', 'merged.k8']).precision == 10
    sub = [a for a in parser._actions if a.dest == 'subcommand'][0]
    assert sorted(sub.choices) == sorted(['convert', 'cat', 'count', 'merge', 'balance', 'showbalance', 'stats', 'distr', 'info',
                                          'getcount', 'positive', 'scale', 'shrink', 'shuffle', 'smooth', 'distance', 'matrix',
                                          'cross'])


class FakeProfile(object):
    def __init__(self, value, name, length=2):
        self.counts, self.name, self.length = np.array([value], dtype=np.float64), name, length


TABLE = np.array([[0.5, 0.25, 0.25, 2.0],
                  [1.0, float('nan'), 0.125, 0.125],
                  [3.0, 3.0, 3.0, 3.0]])


def _fake_sets():
    from kpal_amd import kdistlib
    left = [FakeProfile(q, 'left%d' % q) for q in range(3)]
    right = [FakeProfile(r, 'right%d' % r) for r in range(4)]
    dist = kdistlib.ProfileDistance(distance_function=lambda l, r: TABLE[int(l[0]), int(r[0])])   # a user callable: no device
    return left, right, dist


def test_text_format_and_per_pair_fallback():
    from kpal_amd import kdistlib
    left, right, dist = _fake_sets()
    for p in left + right:
        p.copy = lambda p=p: p
    values = kdistlib.cross_distances(left, (p for p in right), dist)
    assert values.shape == (3, 4) and values.dtype == np.float64
    np.testing.assert_array_equal(values, TABLE)
    out = io.StringIO()
    kdistlib.cross_distance_matrix(left, (p for p in right), out, 3, dist)
    assert out.getvalue() == ('3 4\nleft0\nleft1\nleft2\nright0\nright1\nright2\nright3\n'
                              '0.500 0.250 0.250 2.000\n1.000 nan 0.125 0.125\n3.000 3.000 3.000 3.000\n')


def test_nearest():
    from kpal_amd import kdistlib
    np.testing.assert_array_equal(kdistlib.nearest(TABLE, 2), [[1, 2], [2, 3], [0, 1]])       # ties by the lower index
    np.testing.assert_array_equal(kdistlib.nearest(TABLE, 4)[1], [2, 3, 0, 1])                # NaN last
    assert kdistlib.nearest(TABLE, 9).shape == (3, 4)                                         # n > R
    np.testing.assert_array_equal(kdistlib.nearest(TABLE, 9)[0], [1, 2, 0, 3])
    assert kdistlib.nearest(TABLE, 0).shape == (3, 0)


def test_chunk_plan():
    from kpal_amd import kdistlib
    t = 8 * 4 ** 6
    assert kdistlib.cross_chunks(t, 1, kdistlib.CROSS_MAX_BYTES) == [(0, 1)]
    assert kdistlib.cross_chunks(t, 12, 4 * t) == [(0, 4), (4, 8), (8, 12)]                   # an exact multiple
    assert kdistlib.cross_chunks(t, 13, 4 * t + t - 1) == [(0, 4), (4, 8), (8, 12), (12, 13)]   # a remainder
    assert kdistlib.cross_chunks(t, 3, t - 1) == [(0, 1), (1, 2), (2, 3)]                     # never less than one table
    assert kdistlib.cross_chunks(t, 3, 0) == [(0, 1), (1, 2), (2, 3)]
    assert kdistlib.CROSS_MAX_BYTES == 32 << 30


@pytest.mark.parametrize('kind', ('plain', 'max_511', 'max_512', 'max_65535', 'max_65536', 'max_2p31m1', 'max_2p31', 'norm_2p53m1',
                                  'norm_2p53', 'neg_small', 'neg_large', 'int64_extreme'))
def test_boundary_sets_keep_their_edge_when_split(kind):
    """tests/test_gpu_cross.py splits these sets into even and odd profiles: the set has what its label says, the boundary
    profiles P // 2 and P // 2 + 1 land on different sides, and the oracle is finite / infinite where the case says."""
    for P in (12, 41):
        case = matrix_cases.build(kind, 6, P)
        matrix_cases.check_label(case)
        h = P // 2
        assert h % 2 != (h + 1) % 2
        if kind == 'int64_extreme':
            matrix_cases.wrap_visible(case)
            with np.errstate(all='ignore'):
                for i, j in ((h, 0), (h + 1, 0), (h + 1, h)):
                    assert np.isfinite(oracle.multiset(case.profiles[i], case.profiles[j], 'prod'))
                    assert np.isfinite(oracle.multiset(case.profiles[i], case.profiles[j], 'sum'))
                assert np.isinf(oracle.multiset(case.profiles[P - 1], case.profiles[0], 'prod'))
        elif kind.startswith('max_') or kind == 'plain':
            with np.errstate(all='ignore'):
                assert np.isfinite(oracle.multiset(case.profiles[h], case.profiles[h + 1], 'prod'))
