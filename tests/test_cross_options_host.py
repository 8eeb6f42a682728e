"""The rectangle and the triangle of distances for a ProfileDistance with options (kpal_cross_profile_distance[_device],
kpal_profile_distance_matrix_device): what can be checked without a GPU -- the ABI, the Python methods, and that
``cross_distances`` keeps the per-pair fallback for what cannot enter a kernel (a user callable, non-integer counts)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ('kpal_cross_profile_distance', 'kpal_cross_profile_distance_device', 'kpal_profile_distance_matrix_device')


def test_option_rectangle_symbols():
    from kpal_amd import _native
    header = open(os.path.join(ROOT, 'include', 'kpal_hip.h')).read()
    declared = set(re.findall(r'\b(kpal_[a-z0-9_]+)\s*\(', header))
    L = _native.load()
    for name in ENTRIES:
        assert name in declared and name in _native.SIGNATURES and hasattr(L, name), name
    for method in ('cross_profile_distance', 'cross_profile_distance_device', 'profile_distance_matrix_device'):
        assert hasattr(_native.Context, method), method
    # every declaration says which lines of the reference it replaces
    for name in ENTRIES[1:]:
        comment = header[:header.index('int %s(' % name)].rsplit('/*', 1)[1]
        assert 'kdistlib.py:' in comment, name


class FakeProfile(object):
    def __init__(self, value, name, length=2):
        self.counts, self.name, self.length = np.array([value], dtype=np.float64), name, length

    def copy(self):
        return self


TABLE = np.array([[0.5, 0.25, 0.25, 2.0],
                  [1.0, float('nan'), 0.125, 0.125],
                  [3.0, 3.0, 3.0, 3.0]])


def test_user_callable_keeps_the_per_pair_fallback():
    """A callable of the user's cannot enter a kernel: with and without option steps that alone could."""
    from kpal_amd import kdistlib
    left = [FakeProfile(q, 'left%d' % q) for q in range(3)]
    right = [FakeProfile(r, 'right%d' % r) for r in range(4)]
    calls = []

    def lookup(l, r):
        calls.append((int(l[0]), int(r[0])))
        return TABLE[int(l[0]), int(r[0])]

    dist = kdistlib.ProfileDistance(distance_function=lookup)
    assert dist._native_options() is None
    values = kdistlib.cross_distances(left, (p for p in right), dist)
    assert values.shape == (3, 4) and values.dtype == np.float64
    np.testing.assert_array_equal(values, TABLE)
    assert calls == [(q, r) for q in range(3) for r in range(4)]
    # a custom summary function with smoothing requested: no native options either
    custom = kdistlib.ProfileDistance(do_smooth=True, summary=lambda v: np.min(v), distance_function=lookup)
    assert custom._native_options() is None
    # a non-numeric threshold keeps a built-in summary in Python
    assert kdistlib.ProfileDistance(do_smooth=True, threshold='1')._native_options() is None


def test_float_counts_keep_the_per_pair_fallback(monkeypatch):
    """Built-in options over non-integer counts (profiles scaled beforehand): dist.distance pair by pair, and no device set
    is ever made."""
    from kpal_amd import kdistlib
    left = [FakeProfile(q, 'left%d' % q) for q in range(3)]
    right = [FakeProfile(r, 'right%d' % r) for r in range(4)]
    dist = kdistlib.ProfileDistance(do_scale=True, do_positive=True)
    assert dist._native_options() is not None
    seen = []
    monkeypatch.setattr(dist, 'distance', lambda l, r: seen.append((l.name, r.name)) or TABLE[int(l.counts[0]), int(r.counts[0])])

    def no_device(*a, **kw):
        raise AssertionError('float counts must not reach the device route')

    monkeypatch.setattr(kdistlib, '_DeviceSet', no_device)
    monkeypatch.setattr(kdistlib, '_cross_context', no_device)
    values = kdistlib.cross_distances(left, (p for p in right), dist)
    np.testing.assert_array_equal(values, TABLE)
    assert seen == [('left%d' % q, 'right%d' % r) for q in range(3) for r in range(4)]
