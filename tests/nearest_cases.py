"""Inputs of tests/test_gpu_nearest_rows.py, built without a GPU: rows of thousands of candidates for nearest_select_kernel
(kpal_amd/csrc/nearest_kernels.hpp), which walks a row of a tile in chunks of THREADS * PER candidates, candidate r of a chunk
in register r // THREADS of thread r % THREADS.  tests/test_nearest_cases_host.py asserts from the oracle alone what the GPU
tests rely on, so that another seed or shape fails there.

wide_sets(): k = 3 (64 bins), Q = 6 left and R = 4500 right Poisson tables -- a one-tile row is chunks of 2048, 2048 and 404
candidates -- with planted tables written over the right side.  near(l, j) is l with bins [0, j] raised by one each: its
euclidean distance to l is exactly sqrt(j + 1), below every random table's.

    row 0  late winners    near(left[0], j) at 4499 - j, j < 64: the 64 best in the last chunk, in descending position
    row 1  early winners   near(left[1], j) at (37 j + 11) % 2048, j < 64: the 64 best in chunk 0, over every wave and register
    row 2  edges           near(left[2], j) at EDGES[j]: first and last slot of a lane range, a wave, a register, a chunk
    row 3  ties            near(left[3], 0) at TIES: six copies at distance 1 in different lanes, waves, registers, chunks
    row 4                  random tables only
    row 5                  left[5] = 0: every distance NaN under cosine and under scale

sparse_sets(): the first two left tables against R = 2300 right tables that are all zero but ten: under cosine a row is ten
numbers and then NaN by index, and the NaN that filled the list in chunk 0 give way to the numbers of chunk 1.
"""
import numpy as np

import oracle

K = 3
BINS = 4 ** K
Q, R = 6, 4500
THREADS, PER = 256, 8           # kNearestThreads, kNearestPer
CHUNK = THREADS * PER
NMAX = 64                       # KPAL_NEAREST_MAX
SEED = 71

LATE = [R - 1 - j for j in range(NMAX)]
EARLY = [(37 * j + 11) % CHUNK for j in range(NMAX)]
EDGES = [2047, 2048, 4095, 4096, 4435, 0, 255, 256, 63, 64, 1, 2049]
TIES = [5, 69, 261, 2053, 4101, 4400]
PLANTED = {0: LATE, 1: EARLY, 2: EDGES, 3: TIES}

SPARSE_R = 2300
SPARSE_AT = [2049, 7, 2100, 300, 2047, 2048, 1000, 64, 255, 2299]
SPARSE_SEED = 72


def near(l, j):
    t = l.copy()
    t[:j + 1] += 1
    return t


def where(r, tile=R):
    """(chunk, register, wave, lane) of column r of a row of a tile of ``tile`` columns that begins at column 0."""
    r = np.asarray(r) % tile
    tid = r % THREADS
    return r // CHUNK, r % CHUNK // THREADS, tid // 64, tid % 64


_SETS = {}


def _frozen(name, make):
    if name not in _SETS:
        _SETS[name] = make()
        for a in _SETS[name]:
            a.setflags(write=False)
    return _SETS[name]


def _wide():
    rs = np.random.RandomState(SEED)
    rates = rs.uniform(2, 40, Q + R)
    prof = np.stack([rs.poisson(rate, BINS) for rate in rates]).astype(np.int64)
    left, right = prof[:Q].copy(), prof[Q:].copy()
    left[5] = 0
    for j in range(NMAX):
        right[LATE[j]] = near(left[0], j)
        right[EARLY[j]] = near(left[1], j)
    for j, at in enumerate(EDGES):
        right[at] = near(left[2], j)
    for at in TIES:
        right[at] = near(left[3], 0)
    return left, right


def wide_sets():
    """(left int64[6, 64], right int64[4500, 64]), built once, read-only."""
    return _frozen('wide', _wide)


def _sparse():
    left = wide_sets()[0][:2].copy()
    rs = np.random.RandomState(SPARSE_SEED)
    right = np.zeros((SPARSE_R, BINS), dtype=np.int64)
    for at, rate in zip(SPARSE_AT, rs.uniform(2, 40, len(SPARSE_AT))):
        right[at] = rs.poisson(rate, BINS)
    return left, right


def sparse_sets():
    """(left int64[2, 64], right int64[2300, 64]), built once, read-only."""
    return _frozen('sparse', _sparse)


_RECT = {}


def oracle_rect(key, left, right, k, kwargs):
    """oracle.profile_distance over the rectangle left x right, computed once per ``key``, shared, never written."""
    if key not in _RECT:
        with np.errstate(all='ignore'):
            rect = np.array([[oracle.profile_distance(l, r, k, **kwargs) for r in right] for l in left], dtype=np.float64)
        rect.setflags(write=False)
        _RECT[key] = rect
    return _RECT[key]


def gaps(want, n, tables=None):
    """Per row the smallest relative difference of neighbours among the first n + 1 sorted values (which must be finite).
    ``tables``: the right tables of the columns -- neighbours whose tables are the same table are one candidate twice and are
    left out (see copies)."""
    order = np.argsort(want, axis=1, kind='stable')[:, :n + 1]
    s = np.take_along_axis(want, order, axis=1)
    assert np.isfinite(s).all()
    gap = (s[:, 1:] - s[:, :-1]) / np.maximum(np.abs(s[:, 1:]), np.abs(s[:, :-1]))
    if tables is not None:
        first = copies(tables)[order]
        gap = np.where(first[:, 1:] == first[:, :-1], np.inf, gap)
    return gap.min(axis=1)


def copies(tables):
    """For every table the lowest index of a table equal to it."""
    seen, out = {}, np.empty(len(tables), dtype=np.int64)
    for i, t in enumerate(tables):
        out[i] = seen.setdefault(t.tobytes(), i)
    return out
