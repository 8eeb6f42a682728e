"""kdistlib.nearest_chunks / nearest_profiles without a GPU: a user callable keeps the distances in Python, so what is checked
is the chunking of both sides, the merge of the right side's chunks, the order (ties by the lower index, NaN last) and how far
the left iterable is read ahead."""
import gc
import weakref

import numpy as np
import pytest

# rows: ties inside a chunk and across chunks of the right side, a NaN, a row of equal values, a row with +0 and -0
TABLE = np.array([[0.5, 0.25, 0.25, 2.0, 0.25, 0.125, 2.0],
                  [1.0, float('nan'), 0.125, 0.125, 3.0, float('nan'), 0.125],
                  [3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0],
                  [0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 7.0],
                  [7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0]])
Q, R = TABLE.shape


class FakeProfile(object):
    def __init__(self, value, name, length=2):
        self.counts, self.name, self.length = np.array([value], dtype=np.float64), name, length

    def copy(self):
        return self


def fake_sets():
    from kpal_amd import kdistlib
    left = [FakeProfile(q, 'left%d' % q) for q in range(Q)]
    right = [FakeProfile(r, 'right%d' % r) for r in range(R)]
    dist = kdistlib.ProfileDistance(distance_function=lambda l, r: TABLE[int(l[0]), int(r[0])])   # a user callable: no device
    return left, right, dist


TABLE_BYTES = 8 * 4 ** 2   # of a FakeProfile


@pytest.mark.parametrize('n', (1, 2, 3, R, R + 5))
@pytest.mark.parametrize('max_tables', (None, R, 3, 2, 1))
def test_nearest_profiles_is_nearest_of_the_table(n, max_tables):
    from kpal_amd import kdistlib
    left, right, dist = fake_sets()
    max_bytes = None if max_tables is None else max_tables * TABLE_BYTES
    indices, distances = kdistlib.nearest_profiles((p for p in left), right, dist, n, max_bytes=max_bytes)
    want = kdistlib.nearest(TABLE, n)
    assert indices.dtype == np.int64 and distances.dtype == np.float64 and indices.shape == distances.shape == (Q, min(n, R))
    np.testing.assert_array_equal(indices, want)
    np.testing.assert_array_equal(distances, np.take_along_axis(TABLE, want, axis=1))   # (NaN equals NaN here)
    for q in range(Q):
        for j in range(indices.shape[1]):
            d, t = distances[q, j], TABLE[q, indices[q, j]]
            assert (np.isnan(d) and np.isnan(t)) or (d == t and np.signbit(d) == np.signbit(t)), (q, j)


def test_chunks_partition_the_left_side():
    from kpal_amd import kdistlib
    left, right, dist = fake_sets()
    chunks = list(kdistlib.nearest_chunks(iter(left), right, dist, 2, max_bytes=2 * TABLE_BYTES))
    assert [[p.name for p in chunk] for chunk, _, _ in chunks] == [['left0', 'left1'], ['left2', 'left3'], ['left4']]
    np.testing.assert_array_equal(np.concatenate([i for _, i, _ in chunks]), kdistlib.nearest(TABLE, 2))
    # a right side that is no sequence is read once into one
    indices, _ = kdistlib.nearest_profiles(left, (p for p in right), dist, 3)
    np.testing.assert_array_equal(indices, kdistlib.nearest(TABLE, 3))


def test_left_is_read_one_chunk_ahead_and_let_go():
    from kpal_amd import kdistlib
    _, right, dist = fake_sets()
    pulled, alive = [], []

    def left():
        for q in range(Q):
            p = FakeProfile(q, 'left%d' % q)
            pulled.append(q)
            alive.append(weakref.ref(p))
            yield p

    yielded = 0
    gen = kdistlib.nearest_chunks(left(), right, dist, 1, max_bytes=2 * TABLE_BYTES)
    assert pulled == []                                   # nothing is read before the first chunk is asked for
    for chunk, indices, _ in gen:
        # the chunk in hand and at most the one profile that told the generator where it ends
        assert len(pulled) <= yielded + len(chunk) + 1, (pulled, yielded)
        np.testing.assert_array_equal(indices[:, 0], kdistlib.nearest(TABLE, 1)[yielded:yielded + len(chunk), 0])
        first = yielded
        yielded += len(chunk)
        del chunk
        gc.collect()
        if first:   # the chunk before this one is referenced by nobody any more
            assert all(alive[q]() is None for q in range(first)), first
    assert yielded == Q and pulled == list(range(Q))


def test_edges():
    from kpal_amd import kdistlib
    left, right, dist = fake_sets()
    for n in (0, -3):
        with pytest.raises(ValueError):
            kdistlib.nearest_chunks(left, right, dist, n)
        with pytest.raises(ValueError):
            kdistlib.nearest_profiles(left, right, dist, n)
    indices, distances = kdistlib.nearest_profiles([], right, dist, 3)
    assert indices.shape == distances.shape == (0, 3) and indices.dtype == np.int64 and distances.dtype == np.float64
    assert list(kdistlib.nearest_chunks(iter(()), right, dist, 3)) == []
    indices, distances = kdistlib.nearest_profiles(left, [], dist, 3)
    assert indices.shape == distances.shape == (Q, 0)
    # n past what the device selects keeps the Python route; nothing else changes
    from kpal_amd import _native
    big = _native.NEAREST_MAX + 1
    indices, _ = kdistlib.nearest_profiles(left, right, dist, big)
    np.testing.assert_array_equal(indices, kdistlib.nearest(TABLE, big))
