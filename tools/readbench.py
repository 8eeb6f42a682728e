"""One profile per read of generated long reads: Profile.from_fastq_by_record on a FASTQ file against the only device route
there was before it -- the same reads written as FASTA records and read by Profile.from_fasta_by_record -- in one process, on
the same reads.  Three runs of either route, alternating, host clock around the whole scan and a device synchronise; Gbases/s
of each run, the byte counts of the two files, the FASTA figure scaled by the ratio of text bytes (ingest cost follows text
bytes: what the FASTQ route is expected to reach), the per-kernel times of one profiled scan of either route and the time of
indexing the pieces alone.  Needs a GPU.

Usage: python tools/readbench.py [--out DIR] [--reads N] [--length N] [--runs N]   (writes DIR/readbench.json; default profiles/reads)"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 8


def kernel_times(ctx, call):
    ctx.prof_enable(True)
    ctx.prof_reset()
    call()
    ctx.sync()
    got = dict((name, {'ms': ms, 'launches': n}) for name, (ms, n) in ctx.prof_get().items() if n)
    ctx.prof_enable(False)
    return got


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reads'))
    ap.add_argument('--reads', type=int, default=4000)
    ap.add_argument('--length', type=int, default=10000)
    ap.add_argument('--runs', type=int, default=3)
    args = ap.parse_args()
    from kpal_amd import _native, klib
    ctx = _native.context()
    rng = np.random.default_rng(29)
    bases = args.reads * args.length
    seqs = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, (args.reads, args.length))]
    quals = rng.integers(33 + 5, 33 + 41, (args.reads, args.length)).astype(np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        fastq, fasta = os.path.join(tmp, 'reads.fq'), os.path.join(tmp, 'reads.fa')
        with open(fastq, 'wb') as fq, open(fasta, 'wb') as fa:
            for i in range(args.reads):
                seq = seqs[i].tobytes()
                fq.write(b'@read%d\n%s\n+\n%s\n' % (i, seq, quals[i].tobytes()))
                fa.write(b'>read%d\n%s\n' % (i, seq))
        sizes = {'fastq': os.path.getsize(fastq), 'fasta': os.path.getsize(fasta)}

        def by_read():
            with open(fastq, 'rb') as fh:
                return list(klib.Profile.from_fastq_by_record(fh, K))

        def by_record():
            with open(fasta, 'rb') as fh:
                return list(klib.Profile.from_fasta_by_record(fh, K))

        new, old = by_read(), by_record()             # warm-up: code objects, buffers; and the two routes agree
        assert [p.name for p in new] == [p.name for p in old] and len(new) == args.reads
        for i in range(0, args.reads, max(1, args.reads // 20)):
            assert np.array_equal(new[i].counts, old[i].counts), i
        del new, old
        ctx.sync()
        runs = {'fastq': [], 'fasta': []}
        for _ in range(args.runs):
            for route, call in (('fastq', by_read), ('fasta', by_record)):
                t0 = time.perf_counter()
                profiles = call()
                ctx.sync()
                runs[route].append(time.perf_counter() - t0)
                del profiles
        kernels = {'fastq': kernel_times(ctx, by_read), 'fasta': kernel_times(ctx, by_record)}

        # where a scan's time goes: the pieces indexed and nothing else (read, upload, tokenise, index; no table, no profile)
        def index_only(path, open_scan):
            t0, resume = time.perf_counter(), 0
            while True:
                open_scan(path, resume, 0)
                piece = ctx.fasta_records_file_next()
                resume = ctx.fasta_records_file_tell() if piece is not None else 0
                ctx.fasta_records_file_close()
                if piece is None:
                    return time.perf_counter() - t0

        index_seconds = {'fastq': [index_only(fastq, ctx.fastq_records_file_open) for _ in range(args.runs)],
                         'fasta': [index_only(fasta, ctx.fasta_records_file_open) for _ in range(args.runs)]}
    rates = dict((route, [bases / t / 1e9 for t in times]) for route, times in runs.items())

    def middle(values):
        return sorted(values)[len(values) // 2]

    result = {'device': 'MI355X (gfx950)', 'k': K, 'reads': args.reads, 'read_length': args.length, 'bases': bases, 'text_bytes': sizes,
              'seconds': runs, 'index_only_seconds': index_seconds, 'gbases_per_s': rates,
              'median_gbases_per_s': dict((route, middle(r)) for route, r in rates.items()),
              'spread_gbases_per_s': dict((route, max(r) - min(r)) for route, r in rates.items()),
              'fasta_scaled_by_text_bytes': middle(rates['fasta']) * sizes['fasta'] / sizes['fastq'],
              'kernels': kernels}
    for route in ('fastq', 'fasta'):
        print('%s: %d text bytes, %s Gbases/s (median %.3f, spread %.3f)' % (route, sizes[route], ' '.join('%.3f' % r for r in rates[route]),
                                                                            result['median_gbases_per_s'][route], result['spread_gbases_per_s'][route]))
    print('index only (s): fastq %s, fasta %s' % (' '.join('%.4f' % t for t in index_seconds['fastq']), ' '.join('%.4f' % t for t in index_seconds['fasta'])))
    print('fasta scaled by text bytes (%.3f): %.3f Gbases/s' % (sizes['fasta'] / sizes['fastq'], result['fasta_scaled_by_text_bytes']))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'readbench.json'), 'w') as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
