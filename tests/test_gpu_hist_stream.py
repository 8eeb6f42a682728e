"""The record stream of the quad histogram (quad_kernels.hpp: quad_hist_kernel), bit for bit against the oracle.

A histogram wave reads the runs it takes -- run g = what scatter workgroup g wrote for the bucket -- as one stream of
256-vector batches: what a run leaves over after its whole batches rides in one batch with the head of the wave's next run,
and the next batch is requested before the current one is counted, across runs.  So the shapes that matter are run LENGTHS
(in batches and what they leave over), how many runs a wave has, and runs of unequal length.  Run lengths come from tile
counts: the tile size is forced (KPAL_QUAD_STEPS / KPAL_QUAD_STEPS2), the number of scatter workgroups is held down with
KPAL_QUAD_WORKGROUPS (the quad plans are then made for that many CUs), and tile j goes to workgroup j % G, so an input of
T tiles gives T % G workgroups one round more than the others.

  * one level (k <= 12): a round of a run is 4 vectors at k = 12, 16 at k <= 11, so what a run leaves over is a multiple of
    that: the smallest (4 / 16) and the largest (252 / 240) stand in for 1 and 255.
  * two levels (k >= 13): a level-2 workgroup writes one round per tile of its stream and one tail round, 16 vectors each.
  * a scatter never has more workgroups than tiles (quad_plan.hpp), so no run of a launch is ever empty: the histogram's skip
    of empty runs cannot be reached through the library and is not covered here.
  * k = 16 (a 32 GiB table) is left to the full-size tests; k = 15 runs the packed histogram with four waves to a run.
"""
import os

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')   # (imported before any HIP work of this process: see test_gpu_count.py)

READ = 151                              # bytes per read of oracle.synth_reads, newline included
_cache = {}


def reads(kind):
    """48 MiB of noisy reads; 'low': every fourth read poly-A, every fifth (AC)n -- items that repeat across the lanes of a load."""
    if kind not in _cache:
        buf = oracle.synth_reads(1207, 0, (48 << 20) // READ + 1, 150, noisy=True)
        if kind == 'low':
            buf = buf.copy()
            rows = buf.reshape(-1, READ)
            rows[::4, :150] = ord('A')
            rows[::5, :150] = np.resize(np.frombuffer(b'AC', dtype=np.uint8), 150)
        _cache[kind] = buf
    return _cache[kind]


def prefix(kind, tiles, tile_kib):
    """Whole reads that fill `tiles` tiles of tile_kib KiB: the last tile lacks 200 to 350 bytes."""
    n = (tiles * tile_kib * 1024 - 200) // READ
    assert n * READ > (tiles - 1) * tile_kib * 1024 + 200
    return reads(kind)[:n * READ]


def want(kind, tiles, tile_kib, k):
    key = (kind, tiles, tile_kib, k)
    if key not in _cache:
        _cache[key] = oracle.count_flat(prefix(kind, tiles, tile_kib), k, threads=8)
    return _cache[key]


def context(**env):
    from kpal_amd import _native
    key = tuple(sorted(env.items()))
    if key not in _cache:
        os.environ.update({n: str(v) for n, v in env.items()})
        try:
            _cache[key] = _native.Context(_native.default_device())
        finally:
            for n in env:
                del os.environ[n]
    return _cache[key]


@pytest.fixture(scope='module', autouse=True)
def _close_contexts():
    yield
    for key, value in list(_cache.items()):
        if hasattr(value, 'close') and hasattr(value, 'count_begin'):
            value.close()
    _cache.clear()


def check(ctx, k, strategy, kind, tiles, tile_kib, steps):
    data = prefix(kind, tiles, tile_kib)
    got = ctx.count_bytes(k, data, strategy)
    plan = ctx.count_last_plan()
    assert plan[0] == strategy and plan[1] == steps, plan
    assert np.array_equal(got, want(kind, tiles, tile_kib, k)), (k, strategy, kind, tiles)


# ---- one level, one-step tiles of 16 KiB.  (workgroups G, rounds per run) -> tiles = G x rounds (+ a few: unequal runs)
ONE_LEVEL = [
    # k = 12: 4 vectors per round.  G = 17: wave 0 takes runs 0 and 16, every other wave one run
    (12, 17, 17 * 63, 'runs of 252 vectors: shorter than a batch, two of them do not fit one'),
    (12, 17, 17 * 64, 'runs of exactly one batch: nothing left over'),
    (12, 17, 17 * 64 + 5, 'five runs of 260 vectors, twelve of 256: run 0 leaves 4 over, run 16 none'),
    (12, 17, 17 * 65, 'runs of 260 vectors: 4 left over, riding with the head of run 16'),
    (12, 16, 16 * 65, 'G = 16: one run per wave, what it leaves over has no next run'),
    (12, 16, 16 * 64 + 3, 'G = 16, unequal runs'),
    (12, 48, 48 * 2 + 5, 'three runs of 12 or 8 vectors per wave: a batch ends inside the second, the third gets its own'),
    (12, 33, 33 * 39 + 20, 'runs of 160 and 156 vectors, three for wave 0: the second lies in two batches'),
    # k <= 11: 16 vectors per round, rows not paired
    (11, 17, 17 * 16, 'k = 11: runs of exactly one batch'),
    (11, 17, 17 * 17, 'k = 11: 16 vectors left over'),
    (11, 17, 17 * 31, 'k = 11: 240 vectors left over'),
    (11, 17, 17 * 16 + 5, 'k = 11: runs of 272 and 256 vectors'),
    (9, 32, 32 * 17 + 9, 'k = 9: two runs per wave, 288 and 272 vectors'),
]


@pytest.mark.parametrize('k,G,tiles,what', ONE_LEVEL, ids=['k%d-G%d-T%d' % c[:3] for c in ONE_LEVEL])
def test_one_level_run_lengths(k, G, tiles, what):
    check(context(KPAL_QUAD_STEPS=1, KPAL_QUAD_WORKGROUPS=G), k, 'partition_quads', 'noisy', tiles, 16, 1)


@pytest.mark.parametrize('tiles', [17 * 64 + 5, 17 * 65])
def test_k12_atomic_merge(tiles):
    """KPAL_K12_STAGED=0: the same stream, the planes merged into the table with atomic adds instead of staged."""
    check(context(KPAL_QUAD_STEPS=1, KPAL_QUAD_WORKGROUPS=17, KPAL_K12_STAGED=0), 12, 'partition_quads', 'noisy', tiles, 16, 1)


@pytest.mark.parametrize('G,tiles', [(17, 17 * 64 + 5), (48, 48 * 2 + 5)])
def test_k12_low_complexity(G, tiles):
    """Poly-A and (AC)n reads among the noisy ones: batches that take the guarded adds, also where a batch holds two runs."""
    check(context(KPAL_QUAD_STEPS=1, KPAL_QUAD_WORKGROUPS=G), 12, 'partition_quads', 'low', tiles, 16, 1)


# ---- two levels at k = 13 (16 coarse buckets x 16 replicas; level-1 tiles of three steps = 48 KiB, level-2 tiles of two).  Planned for
# C CUs: G1 = C level-1 workgroups, G2 = C / 4 level-2 workgroups per coarse bucket taking 64 units each; a level-1 workgroup with t tiles
# writes units of t + 1 rounds (rounded up to even) = cap1, a level-2 stream is cap1 tiles: runs of 16 x (cap1 + 1) vectors.
TWO_LEVEL = [
    (68, 68 * 15, 'G2 = 17: runs of 272 vectors, 16 left over riding with run 16'),
    (64, 64 * 2, 'G2 = 16: one run of 80 vectors per wave'),
    (68, 68 * 2, 'G2 = 17: two runs of 80 vectors in one batch'),
    (16, 16 * 18, 'G2 = 4: four waves share a run of 336 vectors -- one whole batch, one of 80 vectors, two waves without'),
    (16, 16 * 40, 'G2 = 4: 688 vectors -- two whole batches and 176'),
    (4, 4 * 18, 'G2 = 1: sixteen waves share one run'),
]


@pytest.mark.parametrize('C,tiles,what', TWO_LEVEL, ids=['C%d-T%d' % c[:2] for c in TWO_LEVEL])
def test_two_level_run_lengths(C, tiles, what):
    check(context(KPAL_QUAD_STEPS=3, KPAL_QUAD_STEPS2=2, KPAL_QUAD_WORKGROUPS=C), 13, 'partition2_quads', 'noisy', tiles, 48, 3)


def test_k15_shared_runs_packed_bins():
    """k = 15 on a small input: four level-2 workgroups per coarse bucket, so four waves share a run, and the packed bins."""
    check(context(KPAL_QUAD_STEPS=3, KPAL_QUAD_STEPS2=2), 15, 'partition2_quads', 'noisy', 40, 48, 3)
    _cache.pop(('noisy', 40, 48, 15))   # (8 GiB)
