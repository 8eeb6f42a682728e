"""Sliding-window profiles of one generated 5 Mb record: Profile.from_fasta_by_window against the only device route there
was before it -- the same windows written out as FASTA records and read by Profile.from_fasta_by_record -- in one process, on
the same sequence.  Per shape (k, window, step): ten repeats of either route, host clock around the call and a device
synchronise (min / median / max), end to end from the file and for the counting call alone (records indexed once), and the
per-kernel times of one profiled counting call.  Needs a GPU.

Usage: python tools/winbench.py [--out DIR] [--bases N] [--repeats N]      (writes DIR/winbench.json; default profiles/windows)"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(k, W, S) for k in (4, 6) for W, S in ((5000, 500), (1000, 1000))]


def spread(times):
    t = sorted(times)
    return {'min_ms': 1e3 * t[0], 'median_ms': 1e3 * t[len(t) // 2], 'max_ms': 1e3 * t[-1]}


def timed(ctx, repeats, call):
    call()                          # warm-up: code objects, buffers
    ctx.sync()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ctx.sync()
        out.append(time.perf_counter() - t0)
    return spread(out)


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'windows'))
    ap.add_argument('--bases', type=int, default=5000000)
    ap.add_argument('--repeats', type=int, default=10)
    args = ap.parse_args()
    from kpal_amd import _native, klib
    ctx = _native.context()
    rng = np.random.default_rng(17)
    seq = np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, args.bases)].tobytes().decode()
    lines = '\n'.join(seq[i:i + 70] for i in range(0, len(seq), 70))
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        genome = os.path.join(tmp, 'genome.fa')
        with open(genome, 'w') as fh:
            fh.write('>g\n' + lines + '\n')
        for k, W, S in SHAPES:
            spans = [(j * S, min(j * S + W, len(seq))) for j in range(klib._window_count(len(seq), W, S))]
            as_records = os.path.join(tmp, 'windows_%d_%d.fa' % (W, S))
            with open(as_records, 'w') as fh:
                for a, b in spans:
                    fh.write('>g:%d-%d\n%s\n' % (a + 1, b, seq[a:b]))

            def by_window():
                with open(genome) as fh:
                    return list(klib.Profile.from_fasta_by_window(fh, k, W, S))

            def by_record():
                with open(as_records) as fh:
                    return list(klib.Profile.from_fasta_by_record(fh, k))

            new, old = by_window(), by_record()
            assert [p.name for p in new] == [p.name for p in old] and len(new) == len(spans)
            for i in range(0, len(new), max(1, len(new) // 50)):
                assert np.array_equal(new[i].counts, old[i].counts), (k, W, S, i)
            del new, old
            row = {'k': k, 'window': W, 'step': S, 'bases': len(seq), 'windows': len(spans), 'repeats': args.repeats,
                   'end_to_end': {'by_window': timed(ctx, args.repeats, by_window), 'by_record': timed(ctx, args.repeats, by_record)}}
            # the counting call alone: records indexed once, the tables written into one allocation
            n = len(spans)
            dev = ctx.alloc(n * 8 * 4 ** k)
            try:
                with open(genome, 'rb') as fh:
                    ctx.fasta_records_begin(fh.read())
                call = lambda: ctx.fasta_windows_count_device(k, W, S, 0, n, dev)
                row['count_only'] = {'by_window': timed(ctx, args.repeats, call)}
                row['kernels'] = {'by_window': kernel_times(ctx, call)}
                with open(as_records, 'rb') as fh:
                    n_records, _ = ctx.fasta_records_begin(fh.read())
                assert n_records == n
                call = lambda: ctx.fasta_records_count_device(k, 0, n, dev)
                row['count_only']['by_record'] = timed(ctx, args.repeats, call)
                row['kernels']['by_record'] = kernel_times(ctx, call)
            finally:
                ctx.free(dev)
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, 'winbench.json'), 'w') as fh:
        json.dump({'device': 'MI355X (gfx950)', 'rows': rows}, fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
