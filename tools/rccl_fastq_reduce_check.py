#!/usr/bin/env python
"""The in-library reduces end an open FASTQ text (tests/test_gpu_dist.py::test_library_rccl_world_1_ends_a_fastq_text; run on
the GPU box): on a communicator of world size 1, a FASTQ text whose last line lacks its '\\n' is fed, so that its last record
is still carried, and kpal_comm_reduce_table (serial and pipelined) and kpal_comm_reduce_scatter_table run with balance = 1
-- the merged table is oracle.balance(oracle.from_sequences(reads)), the carried read counted before the reduce; a text that
ends in a cut-off record makes the reduce raise ValueError naming the record."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np

import oracle
from fastq_cases import fastq_reads, random_fastq
from kpal_amd import _native

ctx = _native.Context(_native.default_device())
ctx.comm_init(0, 1, _native.comm_unique_id())
text = random_fastq(random.Random(14), 300, noise=False) + b'@last\nACGTTGACCAGTAGGCATCAAGTCAG\n+\nIIIIIIII#IIIIIIIIIIIIIIIII'
reads = fastq_reads(text)
assert reads[-1] == b'ACGTTGACCAGTAGGCATCAAGTCAG'
for k in (8, 13):
    want = oracle.balance(oracle.from_sequences(reads, k), k)
    late = oracle.balance(oracle.from_sequences(reads[:-1], k), k) + oracle.from_sequences(reads[-1:], k)
    assert not np.array_equal(late, want)              # a reduce that leaves the carried read to kpal_count_finish is visible
    for how in ('serial', 'pipelined', 'scatter'):
        ctx.count_begin(k, 'partition2_quads' if k == 13 else 'auto')
        ctx.count_feed_fastq(text[:1000])
        ctx.count_feed_fastq(text[1000:])
        if how == 'scatter':
            ctx.comm_reduce_scatter_table(balance=True)
            ctx.sync()
            ptr, first, bins = ctx.comm_merged_range()
            assert (first, bins) == (0, 4 ** k)
        else:
            ctx.comm_reduce_table(0, balance=True, pipelined=how == 'pipelined')
            ctx.sync()
            ptr, bins = ctx.comm_merged_table()
        got = np.empty(bins, dtype=np.int64)
        ctx.d2h(got, ptr)
        assert np.array_equal(got, want), (k, how)
        if how != 'pipelined':                         # (serial forms: the merged table is the count table)
            assert np.array_equal(ctx.count_finish(), want), (k, how)
cut_off = text[:text.rindex(b'@last')] + b'@cut\nACGT\n+'
for how in ('serial', 'pipelined', 'scatter'):
    ctx.count_begin(8)
    ctx.count_feed_fastq(cut_off)
    try:
        if how == 'scatter':
            ctx.comm_reduce_scatter_table(balance=True)
        else:
            ctx.comm_reduce_table(0, balance=True, pipelined=how == 'pipelined')
    except ValueError as e:
        assert 'record 301:' in str(e), str(e)
    else:
        raise AssertionError('a reduce over a text that ends in a cut-off record must fail (%s)' % how)
ctx.count_begin(8)
ctx.count_feed_fastq(text)
assert np.array_equal(ctx.count_finish(), oracle.from_sequences(reads, 8))
ctx.comm_destroy()
ctx.close()
print('RCCL_FASTQ_REDUCE_OK')
