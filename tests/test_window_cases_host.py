"""What tests/test_gpu_windows_trips.py relies on, asserted on the CPU from tests/window_cases.py and the oracle alone, for a
part of 256 compute units (MI355X) and for one of 320: every case is past the plan number it is there for, its expected tables
say something, and case B holds k-mers that only a member wave's carry from the step before its first one delivers."""
import numpy as np
import pytest

import window_cases as wc

CASES = dict((case.name, case) for case in wc.all_cases())


@pytest.mark.parametrize('cus', wc.CUS)
def test_thresholds_restate_the_plans(cus):
    """The numbers against the source text they restate (the line a comment in thresholds() names may move; the text may not)."""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'kpal_amd', 'csrc')
    records = open(os.path.join(csrc, 'kpal_records.hip')).read()
    plan = open(os.path.join(csrc, 'count_plan.hpp')).read()
    kernels = open(os.path.join(csrc, 'window_kernels.hpp')).read()
    t = wc.thresholds(cus)
    assert 'std::min<uint64_t>((ntiles + TPW - 1) / TPW, (uint64_t)ctx->num_cu * 8)' in records
    assert 'kSmallTpw = K <= 6 ? 4 : 1' in kernels
    assert (t['tiles_k6'], t['tiles_k7']) == (4 * 8 * cus, 1 * 8 * cus)
    assert 'if (S <= 2048)' in records and 'std::min<uint64_t>(ntiles, (uint64_t)ctx->num_cu * 4)' in records
    assert t['tiles_long'] == 4 * cus
    assert records.count('wave_grid((s.nchunks + 63) / 64, ctx->num_cu, 8, 4)') == 2
    assert 'max_waves = (uint64_t)num_cu * blocks_per_cu * waves_per_block' in plan
    assert t['wave_steps'] == cus * 8 * 4
    assert 'threads = (uint64_t)ctx->num_cu * 2048' in records and 'std::max<uint64_t>(m, (n * bins + threads - 1) / threads)' in records
    assert t['slide_threads'] == cus * 2048


@pytest.mark.parametrize('cus', wc.CUS)
def test_every_precondition(cus):
    wc.require_a1(cus)
    wc.require_a2(cus)
    for m in (1, 2):
        wc.require_a3(m, cus)
    for k in (4, 7):
        wc.require_b(k, cus)
    wc.require_c(cus)
    wc.require_d(cus)
    for k in (10, 11, 12):
        wc.require_e(k)
    wc.require_f(cus)


def test_case_shapes():
    """(k, W, S) and the record lengths of every case, pinned; why D's two long records are as long as they are, window_cases.py says."""
    shapes = dict((name, (c.k, c.W, c.S)) for name, c in CASES.items())
    assert shapes == {'A1': (4, 4, 1), 'A2': (7, 7, 7), 'A3m1': (2, 2049, 2049), 'A3m2': (2, 4098, 2049), 'Bk4': (4, 40000, 20000),
                      'Bk7': (7, 40000, 20000), 'C': (8, 2 << 20, 1 << 20), 'D': (3, 6, 3), 'Ek10': (10, 24, 8), 'Ek11': (11, 24, 8),
                      'Ek12': (12, 24, 8), 'F': (2, 2049, 2049)}
    lengths = dict((name, [len(seq) for _, seq in c.records]) for name, c in CASES.items())
    assert lengths['A1'] == [10301, 0, 3, 4, 9] and lengths['A2'][1:] == [0, 6, 7] and lengths['Bk4'] == lengths['Bk7'] == [90000, 25000]
    assert lengths['C'][1:4] == [0, 7, 8] and lengths['C'][0] >= 7 << 20 and lengths['C'][4] >= 4 << 20
    short = lengths['D'][1:-1]
    assert len(short) == 1500 and sorted(set(short)) == list(range(14)) and sum(L <= 6 for L in short) > 1000
    for k in (10, 11, 12):
        assert lengths['Ek%d' % k] == [24 + 16 + k, k - 1]
    # about one N per few thousand bases, in every case with a long record
    for name in ('A1', 'A2', 'A3m1', 'Bk4', 'C', 'D', 'F'):
        flat, _ = wc.stream(CASES[name])
        n = int((flat == ord('N')).sum())
        assert 1 <= n and len(flat) / 6000 <= n <= len(flat) / 2000 + 1, (name, n)


def valid_kmers(case):
    """k-mers of every window, counted without the oracle: runs of k bytes of the alphabet inside [a, b)."""
    out = []
    for _, seq in case.records:
        good = np.isin(np.frombuffer(seq, dtype=np.uint8), wc.ALPHABET).astype(np.int64)
        run = np.concatenate([[0], np.cumsum(good)])
        whole = (run[case.k:] - run[:-case.k] == case.k) if len(seq) >= case.k else np.zeros(0, dtype=bool)     # k-mer begins at i
        begins = np.concatenate([[0], np.cumsum(whole)])
        for a, b in wc.window_spans(len(seq), case.W, case.S):
            out.append(int(begins[max(b - case.k + 1, a)] - begins[a]) if b - a >= case.k else 0)
    return np.array(out)


@pytest.mark.parametrize('name', sorted(CASES))
def test_expected_tables_say_something(name):
    """Every window's table sums to its k-mers counted another way; most windows hold k-mers, some are cut short by an N or
    a tab or hold none, and the tables differ from window to window."""
    case = CASES[name]
    want = wc.expected(case)
    assert want.shape == (wc.n_windows(case), 4 ** case.k) and want.min() >= 0
    totals = want.sum(axis=1)
    np.testing.assert_array_equal(totals, valid_kmers(case))
    assert (totals > 0).sum() >= 0.75 * len(totals) or name.startswith('E')
    assert (totals > 0).sum() >= 4
    full = min(case.W, max(len(seq) for _, seq in case.records)) - case.k + 1
    assert 0.99 * full <= totals.max() <= full        # a whole window of bases, but for an N in a few thousand
    assert (totals < totals.max()).any()              # and a window that is shorter, or holds an N or a tab
    some = want[np.linspace(0, len(want) - 1, min(len(want), 64)).astype(int)]
    assert (some[1:] != some[:-1]).any(axis=1).sum() >= min(len(some) - 1, 3)
    if name in ('A1', 'A2', 'D', 'C') or name.startswith('E'):
        assert (totals == 0).any()                    # the record of k - 1 bases, or a window of N


@pytest.mark.parametrize('k', (4, 7))
def test_case_b_needs_the_carry(k):
    """Some k-mer begins in a member's last 1024-byte step and ends in the next member's first: a carry loaded at c_lo - 1 for
    every member, or left zero, loses or miscounts it."""
    case = wc.case_b(k)
    assert wc.carried_kmers(case, 8) >= 8 * (k - 1)
    # and the same geometry gives none at GROUP = 4 for tiles of 2048 bases: per = 1 there, which is where the old tests stop
    old = wc.Case('old', k, 4112, 4112, case.records)
    assert all(per <= 1 for _, per, _, _, _ in wc.lds_tile_members(old, 8))
