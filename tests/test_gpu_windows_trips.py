"""Sliding windows PAST one grid trip, one wave-step a member and one segment (kpal_amd/csrc/window_kernels.hpp, fasta_windows_pass
in kpal_amd/csrc/kpal_records.hip).  tests/test_gpu_windows.py is careful about the text; its shapes are small enough that every
loop of the three kernels runs its first trip only.  The cases here come from tests/window_cases.py, which restates the plan
numbers; tests/test_window_cases_host.py asserts on the CPU, for 256 and 320 compute units, what they rely on.

Every case is indexed by ONE ctx.fasta_records_begin(text) and counted by ONE ctx.fasta_windows_count over all of its windows
(kpal_fasta_records_begin stages a text of any length through the pinned buffers, 64 MiB at a time; the klib generators would
cut the scan into batches that never reach these shapes).  Every test first ASSERTS, at the device's own number of compute
units, the precondition that makes it mean something.  Every expected table is ``oracle.from_sequences([seq[a:b]], k)``; every
comparison is exact.

    case   k        W, S              what it reaches
    A1     4        4, 1              window_tiles_lds_kernel<4, 4, 4>: more than 32 * CUs tiles -> a workgroup zeroes h, counts and
                                      dumps a second group of four tiles; tiles % 4 = 1 -> three dead slots in the last group
    A2     7        7, 7              <7, 1, 4>: one tile a workgroup, more than 8 * CUs tiles; m = 1 (tiles are the windows)
    A3     2        2049 | 4098, 2049 <2, 1, 8>: tiles past 2048 bases, more than 4 * CUs of them; m = 1 and m = 2
    B      4, 7     40000, 20000      <K, 1, 8>: 20 wave-steps a tile, per = 3: members 1 .. 6 load their carry in mid-tile and walk on,
                                      member 6 is cut short by `steps`, member 7 is idle; tiles of 10 and 5 steps beside them
    C      8        2 MiB, 1 MiB      window_tiles_atomic_kernel and count_records_kernel with steps_per_wave = 2: a wave from step0 > 0
                                      that carries into a second step, record borders inside a later step, a tail wave of one step
    D      3        6, 3              window_slide_kernel with segment = 12 > m = 2 (256 CUs), four segments a workgroup, segments over the
                                      windows of up to 12 records and over records without windows, n_segments % 4 = 2
    E      10 - 12  24, 8             the DISPATCH_K_1_16 arms above 9; the trim's kmask and table + (i << 2k) up to 128 MiB a window

    F      2        2049, 2049        <2, 1, 8> again with 6001 tiles, four trips or more of every workgroup, counted three times: see slip 2

Case D departs from the sizes first written down for it: 50 000 and 25 000 bases give 27 700 windows and segments of 4 windows,
which cannot hold the windows of ten records.  The long records are 200 000 and 79 000 bases (95 016 windows).

Measured on an MI355X (256 compute units): 12 tests, 14.2 s for this file run alone (16.6 s wall with the interpreter) -- 11.8 s of it the first test's
fixtures (the context, and torch's query of the device), 2.1 s in the tests; the slowest is E at k = 12 with 0.72 s (805 MB of
tables down and compared), then D 0.40 s, A2 0.32 s, A1 0.20 s; F, with its three calls, 0.08 s.  No kernel needed a change.

Checked once by hand, not part of the suite: scratch builds of the library with one slip each in window_kernels.hpp (all give
wrong tables, none a fault), tests/test_gpu_windows.py (16 tests, with the oracle comparison this change adds to
test_launch_structure_and_determinism) and this file (12 tests) against each:
    1  h zeroed before the grid-stride loop only            test_gpu_windows.py green; 6 fail here: A1, A2, A3 twice, D (95 894
                                                              tiles: its tile kernel goes round too) and F
    2  the barrier behind the dump removed                  test_gpu_windows.py green; F fails here (20 of 96 016 bins wrong in its
       (a race: at 16 bins waves 1 .. 3 have nothing to       first call), A1 .. A3 pass: in separate calls of 6001 such tiles 5, 23
       dump and zero h while wave 0 still reads it)           and 8 tiles came out wrong, of A3's 1301 tiles none -- which is why F exists
    3  the LDS kernel's carry loaded at c_lo - 1 for        5 of test_gpu_windows.py fail ALREADY: the grid at k = 2, 4, 6, 7 (tiles of
       every member                                           4112 bases: per = 1, members 1 .. 4 start in mid-tile) and the comparison
                                                              added to test_launch_structure_and_determinism; 5 fail here: A3 twice, B twice, F
    4  the atomic kernel's carry loaded at -1 for           2 of test_gpu_windows.py fail ALREADY (the grid at k = 8 and 9: a stream of a few
       every wave                                             kilobytes is several waves of one step); C fails here
    5  `fresh` not set again at a new record in the slide   12 of test_gpu_windows.py fail ALREADY; 6 fail here: A1, C, D, E three times
"""
import numpy as np
import pytest

import window_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from kpal_amd import _native
    return _native.context()


@pytest.fixture(scope='module')
def cu():
    """Compute units of the part: the device property kpal_ctx sizes its grids with."""
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def index(ctx, case):
    """One kpal_fasta_records_begin over the whole text; the layout against the enumeration -> number of windows."""
    flat, starts = wc.stream(case)
    n_records, flat_bytes = ctx.fasta_records_begin(wc.fasta_text(case.records))
    assert (n_records, flat_bytes) == (len(case.records), len(flat))
    n, first_window = ctx.fasta_windows_layout(case.W, case.S)
    counts = [wc.win_count(len(seq), case.W, case.S) for _, seq in case.records]
    assert n == wc.n_windows(case) and first_window.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    return n


def hold(ctx, case):
    """ONE kpal_fasta_windows_count over all windows of the case, against the oracle."""
    n = index(ctx, case)
    got = ctx.fasta_windows_count(case.k, case.W, case.S, 0, n)
    np.testing.assert_array_equal(got, wc.expected(case), err_msg='case %s' % case.name)


def test_a1_second_group_of_four_tiles(ctx, cu):
    wc.require_a1(cu)
    hold(ctx, wc.case_a1())


def test_a2_second_tile_of_a_workgroup_at_k7(ctx, cu):
    wc.require_a2(cu)
    hold(ctx, wc.case_a2())


@pytest.mark.parametrize('m', (1, 2))
def test_a3_second_long_tile_of_a_workgroup(ctx, cu, m):
    wc.require_a3(m, cu)
    hold(ctx, wc.case_a3(m))


@pytest.mark.parametrize('k', (4, 7))
def test_b_members_walk_three_steps_from_mid_tile(ctx, cu, k):
    wc.require_b(k, cu)
    assert wc.carried_kmers(wc.case_b(k), 8) > 0
    hold(ctx, wc.case_b(k))


def launched(ctx, call):
    """-> (result of call(), {kernel: launches})"""
    try:
        ctx.prof_enable(True)
        ctx.prof_reset()
        out = call()
        ctx.sync()
        return out, dict((name, count) for name, (_, count) in ctx.prof_get().items() if count)
    finally:
        ctx.prof_enable(False)


def test_c_two_steps_a_wave_windows_and_records(ctx, cu):
    wc.require_c(cu)
    case = wc.case_c()
    n = index(ctx, case)
    got, names = launched(ctx, lambda: ctx.fasta_windows_count(case.k, case.W, case.S, 0, n))
    assert names == {'window_tiles_atomic': 1, 'window_slide': 1, 'window_trim': 1}
    np.testing.assert_array_equal(got, wc.expected(case), err_msg='windows')
    by_record, names = launched(ctx, lambda: ctx.fasta_records_count(case.k, 0, len(case.records)))
    assert names == {'fa_rebase': 1, 'count_records': 1}
    np.testing.assert_array_equal(by_record, wc.expected_records(case, case.k), err_msg='records')


def test_d_segments_over_many_records(ctx, cu):
    wc.require_d(cu)
    hold(ctx, wc.case_d())


@pytest.mark.parametrize('k', (10, 11, 12))
def test_e_k_above_nine(ctx, k):
    wc.require_e(k)
    hold(ctx, wc.case_e(k))


def test_f_four_trips_of_every_workgroup(ctx, cu):
    """The call is made F_CALLS times and every result is held: what a missing barrier behind the dump loses, it loses on
    one trip in some hundreds, another one each time."""
    wc.require_f(cu)
    case = wc.case_f()
    n = index(ctx, case)
    want = wc.expected(case)
    for call in range(wc.F_CALLS):
        np.testing.assert_array_equal(ctx.fasta_windows_count(case.k, case.W, case.S, 0, n), want, err_msg='case F, call %d' % call)
