/*
 * kpal_hip.h -- C-ABI of libkpal_hip.so: the MI355X (gfx950) k-mer counting and
 * profile-distance hot path of kPAL.
 *
 * The reference (kPAL 2.1.2.dev, pure Python) has no FFI for this path; its boundary is
 * the Python API of kpal/klib.py, kpal/metrics.py and kpal/kdistlib.py.  Each entry point
 * below names the reference interface it replaces (file:line into the reference tree).
 * kpal_amd/_native.py is the ctypes binding; INTEGRATION.md shows the stub a kPAL
 * maintainer would add.
 *
 * Conventions
 *  - every function returns an int status: 0 = ok, <0 = error (KPAL_E_*);
 *    kpal_last_error() returns a thread-local, NUL-terminated description.
 *  - the caller owns every host pointer; the library owns device memory behind kpal_ctx
 *    (or borrows caller-provided device pointers in the *_device variants).
 *  - calls are blocking unless stated otherwise; a ctx is bound to one GPU and one HIP
 *    stream and must not be used from two threads at once.
 *  - count vectors are int64, length 4^k, index = big-endian 2-bit packing of the k-mer
 *    with A/a=0 C/c=1 G/g=2 T/t=3 (klib.py:43-48, doc/method.rst:23-45).
 *  - 1 <= k <= KPAL_MAX_K = 16.  The reference takes any length and is bounded by memory alone (klib.py:149-151: a Python list
 *    of 4^k integers, then an int64 array); here the bound is the encoder's window -- a lane sees its own 16 bases and the 16
 *    before them -- and 4^16 int64 counts are 32 GiB of the 288 GB of one MI355X; k = 17 (128 GiB per profile, two of them
 *    for any distance) is refused with KPAL_E_INVALID -- ValueError in the Python face -- not miscounted.
 */
#ifndef KPAL_HIP_H
#define KPAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KPAL_MAX_K 16

#define KPAL_OK 0
#define KPAL_E_INVALID (-1) /* bad argument (-> ValueError) */
#define KPAL_E_NOMEM (-2)   /* host or device allocation failed (-> MemoryError) */
#define KPAL_E_HIP (-3)     /* HIP runtime error (-> RuntimeError) */
#define KPAL_E_STATE (-4)   /* call sequence error, e.g. feed before begin (-> RuntimeError) */
#define KPAL_E_IO (-5)      /* a file could not be opened or read (-> OSError) */

/* metric selectors */
#define KPAL_PAIRWISE_PROD 0 /* metrics.pairwise['prod'], metrics.py:160 */
#define KPAL_PAIRWISE_SUM 1  /* metrics.pairwise['sum'],  metrics.py:161 */
#define KPAL_EUCLIDEAN 2     /* metrics.euclidean,        metrics.py:126-135 */

#define KPAL_COSINE 3        /* metrics.cosine_similarity, metrics.py:138-147 (kpal_profile_distance only) */

/* summary functions of dynamic smoothing: the keys of metrics.summary, metrics.py:165-170 */
#define KPAL_SUMMARY_MIN 0
#define KPAL_SUMMARY_AVERAGE 1
#define KPAL_SUMMARY_MEDIAN 2

/* counting strategies (kpal_count_set_strategy) */
#define KPAL_STRATEGY_AUTO 0
#define KPAL_STRATEGY_GLOBAL_ATOMIC 1 /* one 64-bit global atomic per k-mer; any k (AUTO only for feeds <= 256 KiB; cross-check of the other pipelines) */
#define KPAL_STRATEGY_LDS_DIRECT 2    /* whole 4^k table privatised in LDS; k <= 7 */
#define KPAL_STRATEGY_PARTITION 3     /* exact-offset radix partition (count, scan, scatter, histogram); 8 <= k <= 12 */
#define KPAL_STRATEGY_PARTITION_CHUNKED 5 /* one-pass partition into chunked bucket lists (no counting pass); 8 <= k <= 12; AUTO */
#define KPAL_STRATEGY_PARTITION2 4    /* two-level radix partition; 13 <= k <= 16 */
#define KPAL_STRATEGY_PARTITION2_QUADS 7 /* two-level partition of 4-k-mer items (quad_kernels.hpp); 13 <= k <= 16; AUTO for feeds >= 64 MiB that hold 1/8 byte per table entry (first piece of a count, a whole device buffer) or 3 bytes (any other) */
#define KPAL_STRATEGY_PARTITION_QUADS 6 /* partition of 4-k-mer items into aligned records (quad_kernels.hpp); 8 <= k <= 12; AUTO for feeds >= 32 MiB */

typedef struct kpal_ctx kpal_ctx;

const char *kpal_last_error(void);
const char *kpal_version(void);

int kpal_device_count(int *n);
int kpal_ctx_create(int device, kpal_ctx **out);
void kpal_ctx_destroy(kpal_ctx *ctx);
int kpal_sync(kpal_ctx *ctx);

/* ---- device memory helpers (bench / tests keep inputs resident in HBM without torch) ---- */
int kpal_dev_alloc(kpal_ctx *ctx, size_t nbytes, void **dev_out);
int kpal_dev_free(kpal_ctx *ctx, void *dev);
int kpal_memcpy_h2d(kpal_ctx *ctx, void *dev_dst, const void *host_src, size_t nbytes);
int kpal_memcpy_d2h(kpal_ctx *ctx, void *host_dst, const void *dev_src, size_t nbytes);
int kpal_memcpy_d2d(kpal_ctx *ctx, void *dev_dst, const void *dev_src, size_t nbytes);   /* asynchronous, ordered on the context's stream */

/* ---- counting: replaces Profile.from_sequences / from_fasta inner loops, klib.py:149-170 ----
 * Input is a flat byte stream; every byte outside AaCcGgTt separates sequences (klib.py:152,
 * the regex '[^AaCcGgTt]'); windows never span a separator or two feeds.  The host side joins
 * the sequences of one from_sequences() call with a single '\n'. */
int kpal_count_begin(kpal_ctx *ctx, int k);            /* klib.py:149-151: zeroed 4^k table */
int kpal_count_set_strategy(kpal_ctx *ctx, int strategy);
int kpal_count_feed(kpal_ctx *ctx, const uint8_t *host_buf, size_t nbytes);        /* klib.py:154-168 */
/* Page-locked host memory for the caller's own staging (the host side of Profile.from_sequences gathers a list of reads into
 * it): kpal_count_feed_pinned lets the DMA engine read it in place -- no staging copy inside the library -- and returns when the
 * buffer may be refilled (the counting kernels may still run). */
int kpal_host_alloc(kpal_ctx *ctx, size_t nbytes, void **host_out);
int kpal_host_free(kpal_ctx *ctx, void *host);
int kpal_count_feed_pinned(kpal_ctx *ctx, const uint8_t *pinned_buf, size_t nbytes);   /* klib.py:154-168, as kpal_count_feed */
/* The same with the input already in HBM.  Stream-ordered: work queued on the context afterwards (kpal_memcpy_*,
 * kpal_synth_reads_device, the next feed) may reuse dev_buf; anything outside the context's stream waits for kpal_sync first.
 * The call does not wait for the GPU, with one exception: the FIRST whole-buffer feed of a k >= 13 count (FRESH mode of the
 * two-level quad pipeline) reads one word back before it returns -- whether a bypass list overflowed, in which case the piece is
 * counted again the classic way from the same buffer -- so that the buffer is the caller's again when the call is back. */
int kpal_count_feed_device(kpal_ctx *ctx, const void *dev_buf, size_t nbytes);
/* FASTA text of whole records (Profile.from_fasta, klib.py:97-112; tokenising the reference
 * delegates to Bio.SeqIO.parse, klib.py:111): header lines dropped, the lines of a record joined
 * with all ASCII whitespace removed, records separated; anything before the first header is
 * ignored.  The text goes to the device in 64 MiB chunks cut anywhere (pinned staging), is flattened there and counted; chunk
 * i + 1 is read, copied and flattened while chunk i is counted; k-mer windows span the chunk seams (never a record boundary).
 * Windows never span two CALLS: a call holds whole records -- or a record's tail / middle / head when the caller cuts one
 * giant record into ranges and hands every range but the first the k - 1 bases before it as `prefix` (below). */
int kpal_count_feed_fasta(kpal_ctx *ctx, const uint8_t *host_buf, size_t nbytes);
/* The same for the bytes [begin, end) of a FILE (end = 0: to its end), read by the library itself: parallel preads straight
 * into the pinned staging buffers (KPAL_READ_THREADS, default 16) -- the path of `kpal count` on a FASTA file (kmer.py:112-146
 * -> klib.py:97-112) and of one rank's shard of the input (byte ranges cut at record boundaries; for one giant
 * record, ranges with a (k-1)-base read-only halo).  `prefix` (may be NULL): text that logically precedes the range -- for a
 * range that begins inside a record: ">\n" + the last k - 1 sequence bytes before `begin`; the range itself must begin at a
 * line start.  Without a prefix, text before the first header of the range is ignored, as at the start of a file. */
int kpal_count_feed_fasta_file(kpal_ctx *ctx, const char *path, uint64_t begin, uint64_t end, const uint8_t *prefix, size_t prefix_len);
/* The flattening alone (tests): host_out needs nbytes bytes; records are each preceded by '\n'. */
int kpal_fasta_flatten(kpal_ctx *ctx, const uint8_t *host_buf, size_t nbytes, uint8_t *host_out, uint64_t *n_out);
/* FASTQ reads (Profile.from_fastq; beyond the reference, which reads FASTA only).  Four-line records: a title line beginning
 * with '@', the sequence line, a separator line beginning with '+' (the rest of it is ignored), the quality line; lines end at
 * '\n', a '\r' just before it is dropped; the role of a line follows from its index mod 4 alone (a quality line may begin with
 * '@' or '+').  Every record contributes '\n' + its sequence bytes, verbatim, to the stream the counters see (k-mers never span
 * two reads).  len(quality) must equal len(sequence).  Empty lines at the very end of the text are ignored; the last line may lack
 * its '\n'; an empty read (empty sequence and quality lines) is legal.  Wrapped (multi-line) FASTQ is malformed.
 * min_quality >= 0 masks bases: base i becomes 'N' (a byte outside the alphabet: it breaks windows) when
 * qual[i] - quality_offset < min_quality, and a quality byte below quality_offset or above '~' is malformed; min_quality < 0
 * (no mask) only length-checks the quality line.  quality_offset is 33 or 64; min_quality <= 93.
 * The text of one count may be cut ANYWHERE between the feeds of kpal_count_begin .. kpal_count_finish: the library carries the
 * unfinished record (in host memory) into the next FASTQ feed -- feeds of other kinds in between leave it alone -- and every call
 * that takes the table for complete ENDS the text first: kpal_count_finish, kpal_count_balance, kpal_comm_reduce_table,
 * kpal_comm_reduce_table_async and kpal_comm_reduce_scatter_table.  Ending the text tokenises and counts what is left with the
 * options of the last FASTQ feed (the carried record takes the options of the later feed, not of the feed it began in), and
 * returns KPAL_E_INVALID if that is a cut-off record.  A FASTQ feed after such a call begins a NEW text (nothing carried, records
 * numbered from 1 again).  kpal_count_table is a plain accessor: it does not end the text, and the table it hands out lacks a
 * record that is still carried.  A malformed record makes the feed (or the call that ends the text) return KPAL_E_INVALID with
 * "malformed FASTQ record N: ..." (N 1-based over the count's text) in kpal_last_error(); the count is abandoned then (the next
 * call that needs it is KPAL_E_STATE until kpal_count_begin).
 * The text goes to the device in 64 MiB chunks (KPAL_FASTA_CHUNK) by the pinned staging of the FASTA path; every chunk is
 * tokenised on the device (fastq_kernels.hpp) behind the carried rest of the chunk before, its status read back once, and counted
 * while the next chunk is copied and tokenised. */
typedef struct kpal_fastq_options {
    int min_quality;     /* < 0: no mask */
    int quality_offset;  /* 33 (Sanger / Illumina 1.8+) or 64 (Illumina 1.3-1.7) */
} kpal_fastq_options;
int kpal_count_feed_fastq(kpal_ctx *ctx, const uint8_t *host_buf, size_t nbytes, const kpal_fastq_options *opt /* NULL: no mask, 33 */);
/* The same for the bytes [begin, end) of a FILE (end = 0: to its end), read by the library's parallel preads straight into the
 * pinned staging buffers, as kpal_count_feed_fasta_file does; the range continues the text of the FASTQ feeds before it. */
int kpal_count_feed_fastq_file(kpal_ctx *ctx, const char *path, uint64_t begin, uint64_t end, const kpal_fastq_options *opt);
/* The tokenising alone (tests): the whole text in one call, ended; host_out needs nbytes bytes and receives the exact stream
 * the counters would see.  Independent of the begin / feed / finish state. */
int kpal_fastq_flatten(kpal_ctx *ctx, const uint8_t *host_buf, size_t nbytes, const kpal_fastq_options *opt, uint8_t *host_out,
                       uint64_t *n_out);
/* Profile.from_fasta_by_record, klib.py:114-133, batched: host_flat holds n_records records,
 * record r = bytes [starts[r], starts[r+1]) (starts ascending, starts[n_records] = nbytes; put a
 * separator byte such as '\n' between records so that no window spans two of them).  host_out
 * receives n_records tables of 4^k int64, record-major.  Independent of the begin/feed/finish state. */
int kpal_count_records(kpal_ctx *ctx, int k, const uint8_t *host_flat, size_t nbytes, const uint64_t *host_starts,
                       size_t n_records, int64_t *host_out);
/* Profile.from_fasta_by_record, klib.py:114-133, with the records found on the device (what the reference leaves to
 * Bio.SeqIO.parse, klib.py:131).  kpal_fasta_records_begin takes FASTA text that holds whole records (text before its first
 * header line is ignored, as at the start of a file), flattens it and indexes its records: *n_records, *flat_bytes.
 * kpal_fasta_records_index copies out, per record, the offset of its header line ('>') in host_text (n_records values: the
 * caller reads the name there, klib.py:132) and its start in the flattened stream (n_records + 1 values, the last = flat_bytes);
 * either pointer may be NULL.  kpal_fasta_records_count counts records [first, first + n) of that text into host_out: n tables of
 * 4^k int64, record-major -- as many records per call as the caller has room for.  The index lives until the next
 * kpal_fasta_records_begin of the context.  Independent of the begin / feed / finish state. */
int kpal_fasta_records_begin(kpal_ctx *ctx, const uint8_t *host_text, size_t nbytes, uint64_t *n_records, uint64_t *flat_bytes);
int kpal_fasta_records_index(kpal_ctx *ctx, uint64_t *header_off, uint64_t *flat_start);
int kpal_fasta_records_count(kpal_ctx *ctx, int k, uint64_t first, uint64_t n, int64_t *host_out);
int kpal_fasta_records_count_device(kpal_ctx *ctx, int k, uint64_t first, uint64_t n, int64_t *dev_out);   /* the same into n x 4^k int64 of the caller's device memory (kpal_dev_alloc): profiles that stay in HBM */
/* The same over a FILE the library reads itself (bytes [begin, end) of path; end = 0: to its end): after _open, every _next
 * indexes the next piece of whole records (as kpal_fasta_records_begin does for text) -- *text_offset = the file offset of the
 * piece's first byte (header offsets of kpal_fasta_records_index are relative to it), *done = 1 (and no records) after the last
 * piece.  Between two _next calls kpal_fasta_records_index / _count serve the current piece. */
int kpal_fasta_records_file_open(kpal_ctx *ctx, const char *path, uint64_t begin, uint64_t end);
int kpal_fasta_records_file_next(kpal_ctx *ctx, uint64_t *n_records, uint64_t *flat_bytes, uint64_t *text_offset, int *done);
int kpal_fasta_records_file_tell(kpal_ctx *ctx, uint64_t *offset);   /* file offset of the first byte no piece has covered yet: where a closed scan is opened again */
int kpal_fasta_records_file_close(kpal_ctx *ctx);
/* The same index over four-line FASTQ text, one record per READ (beyond the reference; the rules of kpal_count_feed_fastq:
 * validation, the quality mask and the flattening are the count path's own tokeniser).  kpal_fastq_records_begin fills the
 * index that kpal_fasta_records_begin fills -- header_off is the offset of the read's title line ('@') in host_text, flat_start
 * the start of '\n' + its sequence line, masked bases as 'N', in the flattened stream; an empty read is a record of no bases --
 * and kpal_fasta_records_index / _count / _count_device and kpal_fasta_windows_layout / _count / _count_device serve whichever
 * format indexed the context last.  Window coordinates count masked bases: a masked base is a base that breaks k-mers.
 * FASTQ text, indexed by read.  The text may be cut anywhere.
 * *consumed = bytes of host_text that the indexed records cover;
 *   the caller carries the rest into its next call.
 * final != 0: the text ends here.
 *   consumed = nbytes, trailing empty lines are no record,
 *   a record cut off is malformed.
 * records_before: records of the same text indexed by earlier calls
 *   (used only to number a malformed record, 1-based over the whole text).
 * Malformed text is KPAL_E_INVALID, "malformed FASTQ record N: ..." with N = records_before + 1 + the record's index in the
 * text; after any error the context holds no index.  A text of 4 GiB is refused.  Independent of the begin / feed / finish
 * state: the open FASTQ text of a count is neither read nor disturbed. */
int kpal_fastq_records_begin(kpal_ctx *ctx, const uint8_t *host_text, size_t nbytes, const kpal_fastq_options *opt,
                             int final, uint64_t records_before, uint64_t *n_records, uint64_t *flat_bytes, uint64_t *consumed);
/* ... over a FILE: the scan that kpal_fasta_records_file_next / _tell / _close then serve is one of FASTQ reads.  Every _next
 * indexes the next piece of whole reads -- the carried rest + a staging buffer's worth of the file (64 MiB, KPAL_FASTA_CHUNK),
 * cut behind the last read it finishes; a piece that finishes none gathers further -- _tell is the file offset of the carried
 * read's title line, and the piece that reaches `end` ends the text. */
int kpal_fastq_records_file_open(kpal_ctx *ctx, const char *path, uint64_t begin, uint64_t end,
                                 const kpal_fastq_options *opt, uint64_t records_before);
/* One profile per sliding window of each record (beyond the reference), over the records indexed by the last
 * kpal_fasta_records_begin / kpal_fasta_records_file_next.  Coordinates are bases of the flattened record; for a record of L
 * bases window j covers bases [j * step, min(j * step + window, L)): none for L = 0, one for L <= window, else
 * ceil((L - window) / step) + 1, the last one possibly truncated; windows never span records and are numbered record-major.
 * Each window restates Profile.from_sequences, klib.py:135-170, on those bases: exactly the k-mers lying wholly inside it.
 * Accepted: 1 <= step <= window, window % step == 0, k <= window; anything else is KPAL_E_INVALID.
 * kpal_fasta_windows_layout: *n_windows of the piece and, unless NULL, first_window[r] = number of record r's first window
 * (n_records + 1 values, the last = *n_windows).  kpal_fasta_windows_count counts windows [first, first + n) into host_out,
 * n tables of 4^k int64; the range may begin and end inside a record.  The cost per base does not grow with window / step.
 * The records are those of the last index, FASTA records or FASTQ reads (kpal_fastq_records_begin). */
int kpal_fasta_windows_layout(kpal_ctx *ctx, uint64_t window, uint64_t step, uint64_t *n_windows, uint64_t *first_window);
int kpal_fasta_windows_count(kpal_ctx *ctx, int k, uint64_t window, uint64_t step, uint64_t first, uint64_t n, int64_t *host_out);
int kpal_fasta_windows_count_device(kpal_ctx *ctx, int k, uint64_t window, uint64_t step, uint64_t first, uint64_t n, int64_t *dev_out);   /* the same into the caller's device memory (kpal_dev_alloc) */
int kpal_count_finish(kpal_ctx *ctx, int64_t *host_out /* 4^k, or NULL to keep the result on the device */); /* klib.py:170 */
/* Profile.balance (klib.py:285-298) on the count table in place, on the device: count + balance is the unit the
 * north-star metric is quoted on.  Call after the last feed, before kpal_count_finish (which then returns the balanced
 * counts).  An open FASTQ text is ended first, exactly as kpal_count_finish ends it (the carried last record is counted before
 * the balance; a cut-off record is KPAL_E_INVALID and the count is abandoned).  For k >= 13 on the two-level quad pipeline the balance is fused into the pass that finalises the table
 * (one read and one write of the 4^k entries instead of two each); otherwise it is kpal_balance_device on the table. */
int kpal_count_balance(kpal_ctx *ctx);
/* Diagnostics (tests, A/B timing): the pipeline the last piece of the last feed actually took (a KPAL_STRATEGY_* value: AUTO
 * resolves per feed size and input composition) and the tile sizes of the quad scatters (wave-steps per wave and tile of level 1 /
 * level 2; 0 where not applicable).  The environment variables KPAL_QUAD_STEPS / KPAL_QUAD_STEPS2, read when the context is
 * created, force those tile sizes. */
int kpal_count_last_plan(kpal_ctx *ctx, int *strategy, int *steps1, int *steps2);
/* Diagnostics: how often the slow paths of the quad pipelines ran since the context was created (cumulative; tests assert that
 * skewed inputs -- poly-A, (AC)n, adapter prefixes: every k-mer still counted once, klib.py:157-168 -- really exercised them).
 * out[0] entries of the per-workgroup hot-item tables in use at kernel ends, out[1] items that rode in a spill list,
 * out[2] items a spill list could not hold (counted on the spot), out[3] pieces finalised FRESH (k >= 13: table written, not
 * added to), out[4] FRESH pieces run again the classic way (a bypass list overflowed), out[5] pieces through a quad pipeline,
 * out[6] pieces through the chunked / round-1 pipelines, out[7] pieces halved (pool or offset limits), out[8] quad pieces whose
 * scatter ran as the REPEAT instantiation (hot rows in the sample: repeat lanes straight to the hot-item table).  n <= KPAL_COUNT_STATS
 * values are written.  Synchronises the context's stream. */
#define KPAL_COUNT_STATS 9
int kpal_count_stats(kpal_ctx *ctx, uint64_t *out, int n);
int kpal_count_table(kpal_ctx *ctx, void **dev_table, uint64_t *n_bins); /* device pointer of the int64 table (for the RCCL reduce); a plain accessor: an open FASTQ text is NOT ended */

/* Deterministic synthetic reads (same bytes as oracle/kpal_oracle.c
 * kpal_oracle_synth_reads): n_reads*(read_len+1) bytes, each read followed by '\n'. */
int kpal_synth_reads_device(kpal_ctx *ctx, uint64_t seed, uint64_t first_read, uint64_t n_reads,
                            int read_len, int noisy, void *dev_out);

/* ---- multi-GPU: one process per GPU, the per-rank count tables merged by ONE RCCL reduce over xGMI ----
 * Replaces nothing the reference has (it is single-threaded); mirrors Profile.merge with the 'sum' merger, klib.py:269-283 /
 * metrics.py:175: every rank counts its shard of the reads into its own table (begin / feed), the tables add -- int64 sums,
 * bit-exact for any reduction order.  RCCL is bound at run time: rccl_library names the librccl.so to load (NULL: the
 * KPAL_RCCL_LIBRARY environment variable, then the loader's search path); inside a PyTorch process pass PyTorch's copy.
 *   rank 0:      kpal_comm_unique_id(lib, id)          -> hand the 128 bytes to the other ranks (MPI, a file, torch.distributed ...)
 *   other ranks: kpal_comm_probe(lib)                  -> can RCCL be bound here?  (no id, no bootstrap listener; agree on the answer
 *                                                         BEFORE the collective kpal_comm_init: a rank that cannot join leaves the others waiting)
 *   every rank:  kpal_comm_init(ctx, lib, rank, world, id)
 *   per job:     kpal_count_begin / feed ...; kpal_comm_reduce_table(ctx, root, balance); kpal_count_finish(root's host buffer)
 * kpal_comm_reduce_table: ncclReduce(int64, sum) of the count table onto `root` and, if balance != 0, Profile.balance there -- all
 * queued on the context's stream, no host synchronisation (except that a count fed FASTQ text has that text ended first, as by
 * kpal_count_finish: the record still carried is counted, which reads one status word back; a cut-off record is KPAL_E_INVALID on
 * that rank and nothing is reduced -- the same holds for the two calls below).  kpal_comm_reduce_table_async: the same on a copy of the table and on a
 * second stream, so that the next kpal_count_begin / feed overlaps it (throughput pipelines; two extra tables of HBM); the merged table
 * is then read with kpal_comm_merged_table (valid until the reduce after next, or until a kpal_count_begin that changes k or -- serial
 * form, where the merged table IS the count table -- starts the next count) after kpal_sync. */
#define KPAL_COMM_ID_BYTES 128
int kpal_comm_probe(const char *rccl_library);
int kpal_comm_unique_id(const char *rccl_library, uint8_t *id_out /* KPAL_COMM_ID_BYTES */);
int kpal_comm_init(kpal_ctx *ctx, const char *rccl_library, int rank, int world, const uint8_t *id);
int kpal_comm_destroy(kpal_ctx *ctx);
int kpal_comm_reduce_table(kpal_ctx *ctx, int root, int balance);
int kpal_comm_reduce_table_async(kpal_ctx *ctx, int root, int balance);
int kpal_comm_merged_table(kpal_ctx *ctx, void **dev_table, uint64_t *n_bins);
/* The bin-range merge (k >= 13, where one rank cannot usefully hold and balance the whole merged vector): ONE ncclReduceScatter
 * (int64 sum) leaves rank r the merged bins [r * 4^k / W, (r + 1) * 4^k / W) in place in its count table; with balance,
 * Profile.balance (klib.py:285-298) of that range -- the entries rc(i) it needs lie 1 / W on every rank: one all-to-all of
 * 4^k / W^2 entries per pair of ranks between two permutation kernels (csrc/range_index.hpp).  W must be a power of two with
 * W^2 <= 4^k.  kpal_comm_merged_range tells where a rank's part lies (first_bin, n_bins; after the whole-table reduces: 0, 4^k);
 * kpal_comm_gather_table (collective, after the range merge) completes every rank's table by one ncclAllGather. */
int kpal_comm_reduce_scatter_table(kpal_ctx *ctx, int balance);
int kpal_comm_gather_table(kpal_ctx *ctx);
int kpal_comm_merged_range(kpal_ctx *ctx, void **dev_table, uint64_t *first_bin, uint64_t *n_bins);
/* The two permutation kernels of that exchange for callers that move the blocks themselves (kpal_amd.dist over torch.distributed):
 * dev_send / dev_recv hold 4^k / W entries, block q = what goes to / came from rank q; dev_table is the whole table, of which only
 * the rank's range is read (pack) or balanced in place (unpack). */
int kpal_range_pack_device(kpal_ctx *ctx, int k, int rank, int world, const int64_t *dev_table, int64_t *dev_send);
int kpal_range_unpack_device(kpal_ctx *ctx, int k, int rank, int world, int64_t *dev_table, const int64_t *dev_recv);
/* kdistlib.distance_matrix (kdistlib.py:164-186) over several GPUs, sharded by BIN RANGE: every rank holds the same bins
 * [first, first + bin_count) of all P profiles (dev_slices: int64[P][bin_count] on the device, profile-major; ranges of different
 * ranks tile 0 .. 4^k; the LDS-staged and matrix-core kernels run when EVERY rank's range is a multiple of 64 bins and >= 4096 -- the
 * ranks agree on that with one 4-byte all-reduce before anything else, a ragged range anywhere puts all of them on the plain kernels), computes every pair's partial sum / term count / dot
 * product over its bins, and ONE all-reduce (two calls: fp64 sums, 64-bit counts -- 32 KB at P = 64) gives every rank the finished lower
 * triangle.  metric: prod / sum / euclidean; balancing needs whole profiles (kpal_balance_device before slicing). */
int kpal_comm_distance_matrix_device(kpal_ctx *ctx, int P, uint64_t bin_count, const int64_t *dev_slices, int metric,
                                     double *out_lower /* P(P-1)/2, kdistlib.py:179-186 order */);
int kpal_comm_max_f64(kpal_ctx *ctx, double *inout);   /* max of a host scalar over the ranks (timing: the slowest rank) */

/* ---- vector operations on 4^k int64 count vectors ---- */
/* Profile.balance, klib.py:285-298: c[i] += c[rc(i)] (palindromes doubled), in place. */
int kpal_balance(kpal_ctx *ctx, int k, int64_t *host_inout);
int kpal_balance_device(kpal_ctx *ctx, int k, int64_t *dev_inout);
/* Profile.reverse_complement, klib.py:394-412 (host helper, no GPU). */
uint64_t kpal_reverse_complement(uint64_t number, int k);
/* Profile.split, klib.py:300-327: forward/reverse each need (4^k + 4^(k/2))/2 entries when k is
 * even, 4^k/2 when odd; *n_out receives that length. */
int kpal_split(kpal_ctx *ctx, int k, const int64_t *host_counts, int64_t *host_forward,
               int64_t *host_reverse, uint64_t *n_out);
/* kmer.get_balance score, kmer.py:243-245: multiset(*split(), pairwise) fused in one pass.  This is
 * kpal_strand_balance_set (below) with one table: the same kernels, the same bits.  KPAL_E_INVALID: k outside
 * 1..KPAL_MAX_K, a NULL pointer, a pairwise other than prod or sum, host_counts not 8-byte aligned (the last was
 * undefined behaviour before it was checked). */
int kpal_strand_balance(kpal_ctx *ctx, int k, const int64_t *host_counts, int pairwise, double *out);

/* metrics.multiset (metrics.py:101-123) with pairwise prod/sum, and metrics.euclidean
 * (metrics.py:126-135), on two int64 vectors of n entries.  If do_balance != 0 both vectors are
 * balanced copies first (kdistlib.py:136-141; n must equal 4^k); inputs are never modified.
 * aux_out (optional): multiset -> number of bins with l!=0 or r!=0 (len(distances));
 * euclidean -> the exact int64 dot product (np.dot wraps like int64). */
int kpal_pair_distance(kpal_ctx *ctx, size_t n, const int64_t *host_left, const int64_t *host_right,
                       int metric, int do_balance, int k, double *out, int64_t *aux_out);
int kpal_pair_distance_device(kpal_ctx *ctx, size_t n, const int64_t *dev_left, const int64_t *dev_right,
                              int metric, int do_balance, int k, double *out, int64_t *aux_out);
/* float64 inputs (profiles after do_scale, kdistlib.py:149-157); multiset only. */
int kpal_pair_distance_f64(kpal_ctx *ctx, size_t n, const double *host_left, const double *host_right,
                           int pairwise, double *out, int64_t *aux_out);

/* kdistlib.distance_matrix values, kdistlib.py:179-186: out_lower[i*(i-1)/2 + j] =
 * distance(profiles[i], profiles[j]) for 0 <= j < i < P (row = left, column = right). */
int kpal_distance_matrix(kpal_ctx *ctx, int P, int k, const int64_t *const *host_profiles, int metric,
                         int do_balance, double *out_lower);
int kpal_distance_matrix_device(kpal_ctx *ctx, int P, int k, const int64_t *dev_profiles /* P x 4^k */,
                                int metric, int do_balance, double *out_lower);

/* The rectangle of distances between two sets of profiles (no counterpart in kPAL: a sample against a panel):
 * out[q * R + r] = distance(left[q], right[r]) for 0 <= q < Q, 0 <= r < R (row = left, column = right), metric and
 * do_balance as for kpal_distance_matrix.  The sets are separate allocations and may alias or overlap (a set against
 * itself gives the full symmetric square with a zero diagonal); no pair inside one set is evaluated.  The host variant
 * uploads both sets through the context's scratch. */
int kpal_cross_distance(kpal_ctx *ctx, int k, int Q, const int64_t *const *host_left, int R,
                        const int64_t *const *host_right, int metric, int do_balance, double *out);
int kpal_cross_distance_device(kpal_ctx *ctx, int k, int Q, const int64_t *dev_left /* Q x 4^k */, int R,
                               const int64_t *dev_right /* R x 4^k */, int metric, int do_balance,
                               double *out /* host, Q x R */);

/* ---- ProfileDistance with its full option set, kdistlib.py:25-51,126-161 ----
 * The constructor arguments of kdistlib.ProfileDistance that select built-in behaviour; a
 * user-supplied summary / pairwise / distance callable cannot enter a kernel and stays in Python. */
typedef struct kpal_distance_options {
    int do_balance;   /* kdistlib.py:139-141: balance copies of both profiles */
    int do_positive;  /* kdistlib.py:143-145: zero every bin that is zero in either profile */
    int do_smooth;    /* kdistlib.py:147-148: dynamic smoothing */
    int summary;      /* KPAL_SUMMARY_*: the `summary` function of the smoothing test */
    double threshold; /* collapse iff min(summary(left quarters), summary(right quarters)) <= threshold */
    int do_scale;     /* kdistlib.py:149-157: scale by the totals (metrics.get_scale) -> float64 profiles */
    int down;         /* metrics.scale_down: both factors <= 1 */
    int metric;       /* KPAL_PAIRWISE_PROD / _SUM (multiset), KPAL_EUCLIDEAN, KPAL_COSINE */
} kpal_distance_options;

/* ProfileDistance.distance(left, right), kdistlib.py:126-161; inputs are never modified. */
int kpal_profile_distance(kpal_ctx *ctx, int k, const int64_t *host_left, const int64_t *host_right,
                          const kpal_distance_options *opt, double *out);
int kpal_profile_distance_device(kpal_ctx *ctx, int k, const int64_t *dev_left, const int64_t *dev_right,
                                 const kpal_distance_options *opt, double *out);
/* ProfileDistance.dynamic_smooth(left, right), kdistlib.py:112-124: both vectors smoothed in place. */
int kpal_dynamic_smooth(kpal_ctx *ctx, int k, int64_t *host_left_inout, int64_t *host_right_inout,
                        int summary, double threshold);
/* kdistlib.distance_matrix values (kdistlib.py:179-186) for any option set: profiles are uploaded once and handed to
 * kpal_profile_distance_matrix_device. */
int kpal_profile_distance_matrix(kpal_ctx *ctx, int P, int k, const int64_t *const *host_profiles,
                                 const kpal_distance_options *opt, double *out_lower);
/* The same values from P consecutive 16-byte aligned tables on the device, replacing the loop of dist.distance calls of
 * kdistlib.py:179-186 (and the per-pair balance / get_scale / scale_down of kdistlib.py:136-157, metrics.py:49-86): every
 * profile is balanced once; positive, scale (+- down) and prod / sum / euclidean / cosine run as rectangle kernels over the
 * tiles on or below the diagonal, a number of launches that does not grow with P; plain options are
 * kpal_distance_matrix_device.  With do_smooth the pair pipeline of kpal_profile_distance_device runs once per pair on the
 * balanced tables (smoothed tables depend on both partners, kdistlib.py:53-124). */
int kpal_profile_distance_matrix_device(kpal_ctx *ctx, int P, int k, const int64_t *dev_profiles /* P x 4^k */,
                                        const kpal_distance_options *opt, double *out_lower);
/* The rectangle of kpal_cross_distance for any option set: out[q * R + r] = ProfileDistance.distance(left[q], right[r])
 * (kdistlib.py:126-161 per pair, with metrics.get_scale / scale_down of metrics.py:49-86 and the masks of metrics.positive,
 * kdistlib.py:143-145, applied per pair on the device).  Launches as for kpal_profile_distance_matrix_device; plain options
 * are kpal_cross_distance_device.  The sets may alias; the host variant uploads both through the context's scratch. */
int kpal_cross_profile_distance(kpal_ctx *ctx, int k, int Q, const int64_t *const *host_left, int R,
                                const int64_t *const *host_right, const kpal_distance_options *opt, double *out);
int kpal_cross_profile_distance_device(kpal_ctx *ctx, int k, int Q, const int64_t *dev_left /* Q x 4^k */, int R,
                                       const int64_t *dev_right /* R x 4^k */, const kpal_distance_options *opt,
                                       double *out /* host, Q x R, row-major */);
/* The n nearest right profiles of every left profile under the distance of kpal_cross_profile_distance: for row q the n
 * smallest of out[q, :] in the order of kdistlib.nearest -- ascending distance, equal distances by the lower index, NaN last,
 * NaNs by index -- without the Q x R rectangle ever existing on the host.  The rectangle is cut into tiles over both sides
 * (nearest_plan.hpp: every tile passes the 32-bit limit of the partials and keeps its workspace within 4 GiB), so no Q and R
 * is refused for its size; a tile is the launches of kpal_cross_profile_distance_device, a kernel that finishes its distances
 * on the device (the doubles that entry returns, bit for bit) and one that merges them into the n best of every row, which
 * stay on the device over a band of tiles: a number of launches per tile that does not grow with the tile, and Q x n values
 * downloaded.  1 <= n <= KPAL_NEAREST_MAX.
 *   dist_inout / index_inout (host, Q x n, row-major): columns [0, have) hold the running best of earlier calls over earlier
 * chunks of the right side, in order; on return columns [0, min(n, have + R)) are the best of those and of this call's
 * right_first + r, in order, and the other columns NaN / -1.  The indices of one row must be distinct.  have = 0 starts.
 *   tile_q / tile_r > 0 cap the sides of a tile (0: the plan's choice); they only shrink tiles.
 * Option sets with do_smooth compute every tile with kpal_cross_smooth_distance_device into a host buffer of one tile and
 * select on the host, under the same order.  Inputs are not written; the workspace is the context's.  KPAL_E_INVALID: what
 * kpal_cross_profile_distance_device refuses, n < 1, n > KPAL_NEAREST_MAX, have < 0, have > n, a negative tile cap. */
#define KPAL_NEAREST_MAX 64
int kpal_cross_nearest(kpal_ctx *ctx, int k, int Q, const int64_t *const *host_left, int R,
                       const int64_t *const *host_right, const kpal_distance_options *opt, int n, int64_t right_first,
                       int have, int tile_q, int tile_r, double *dist_inout, int64_t *index_inout);
int kpal_cross_nearest_device(kpal_ctx *ctx, int k, int Q, const int64_t *dev_left /* Q x 4^k */, int R,
                              const int64_t *dev_right /* R x 4^k */, const kpal_distance_options *opt, int n,
                              int64_t right_first, int have, int tile_q, int tile_r,
                              double *dist_inout /* host, Q x n */, int64_t *index_inout /* host, Q x n */);
/* kpal_profile_distance_matrix_device and kpal_cross_profile_distance_device for an option set WITH dynamic smoothing in a number of launches that does not grow with the
 * number of pairs.  The reference collapses a node iff min(f(left quarters), f(right quarters)) <= threshold (kdistlib.py:
 * 99-100), that is iff f(left quarters) <= threshold OR f(right quarters) <= threshold: a flag per profile.  Every profile is
 * balanced once and gets one pyramid of node sums and node codes (k + 1 launches for all profiles); a pair's distance is the
 * option arithmetic over the bins and nodes that are live for that pair, two passes of the rectangle kernels and one
 * reduction.  Same arguments, checks and values (1e-9; unscaled euclidean and cosine bit for bit) as those entries, to which
 * an option set without do_smooth is handed.  With do_positive (the masks come first: node sums depend on the partner), or
 * when the pyramids -- ten bytes per node, a third of the tables' bins -- exceed 32 GiB, the pair pipeline per pair of those
 * entries runs instead.  Inputs are never modified; all workspace is the context's. */
int kpal_cross_smooth_distance_device(kpal_ctx *ctx, int k, int Q, const int64_t *dev_left /* Q x 4^k */, int R,
                                      const int64_t *dev_right /* R x 4^k */, const kpal_distance_options *opt,
                                      double *out /* host, Q x R, row-major */);
int kpal_smooth_distance_matrix_device(kpal_ctx *ctx, int P, int k, const int64_t *dev_profiles /* P x 4^k */,
                                       const kpal_distance_options *opt, double *out_lower);
/* The distances of the LINKED pairs of two sets: out[i] = ProfileDistance.distance(left[i], right[i]) (kdistlib.py:126-161)
 * for all i -- the loop of `kpal distance` (kmer.py:541-620) over two files, or over one set against itself shifted by a lag.
 * N consecutive 16-byte aligned tables a side.  A chunk of pairs is a fixed number of launches whatever N is: one metric
 * kernel over all (pair, slice) items and one reduction; with scale a totals kernel (masked under positive) and its
 * reduction before them, the pairs' factors derived on the device; with do_balance one launch of the set balance per
 * distinct input range before those, into the context's scratch.  The two ranges may alias or overlap in any way and are
 * never written: when they are the same range, or lie a whole number of tables apart (right == left +- lag * 4^k * 8
 * bytes: successive windows), the union of the two ranges is balanced once and both sides point into it.  A set against
 * itself gives zeros (NaN where the pair entry gives NaN).
 *   A slice is a fixed run of bins and a pair's slices are added in slice order: the value of a pair depends on its two
 * tables and the options alone -- the same bits in a set of 1 or of 10^5, at any position, under any chunk_pairs.  Unscaled
 * euclidean and cosine are int64 sums, bit for bit what kpal_profile_distance_device returns; everything else is within 1e-9
 * relative of the reference (exactly 0, the same NaN and the same infinity where it gives them).
 *   chunk_pairs: 0 takes the plan's chunk (with do_balance: as many pairs as keep the balanced copies within 32 GiB, never
 * less than one); > 0 only lowers it.
 *   With do_smooth the pair pipeline of kpal_profile_distance_device runs once per pair on the once-balanced tables -- exactly
 * what kpal_cross_profile_distance_device does for its pairs; the smoothed pair kernel over per-profile pyramids is
 * kpal_paired_smooth_distance_device, below.
 *   The host variant uploads both sides through the context's scratch, as kpal_cross_profile_distance does.
 * KPAL_E_INVALID, before anything is launched: N < 1, k outside 1 .. KPAL_MAX_K, a NULL pointer, tables not 16-byte aligned,
 * options kpal_profile_distance refuses, chunk_pairs < 0, byte sizes that do not fit. */
int kpal_paired_distance_device(kpal_ctx *ctx, int k, int64_t N, const int64_t *dev_left /* N x 4^k */,
                                const int64_t *dev_right /* N x 4^k */, const kpal_distance_options *opt,
                                int64_t chunk_pairs /* 0: the plan's; > 0 only lowers it */, double *out /* host, N */);
int kpal_paired_distance(kpal_ctx *ctx, int k, int64_t N, const int64_t *const *host_left,
                         const int64_t *const *host_right, const kpal_distance_options *opt, double *out /* host, N */);
/* kpal_paired_distance[_device] for an option set WITH dynamic smoothing in a number of launches that does not grow with N:
 * same arguments, same checks with the same messages, same values.  Without do_smooth, and with do_positive (the masks come
 * first: node sums depend on the partner), the call is handed to kpal_paired_distance_device.  Otherwise, per chunk of pairs:
 * with do_balance the set balance exactly as that entry runs it; the pyramids of node sums and codes of the chunk's DISTINCT
 * tables (kpal_cross_smooth_distance_device) -- when the ranges are the same range or lie a whole number of tables apart,
 * of their union once, so successive windows build N pyramids; ranges that alias in any other way are read as they lie --
 * in k + 1 launches; ONE metric kernel over all (pair, slice) items -- a pair's bin slices, then the slices of its two
 * pyramids -- and ONE reduction.  No totals pass under scale: smoothing conserves totals and the roots are the totals.
 *   A pair's slices depend on k alone and are added in slice order: the bits of a pair depend on its two tables and the
 * options, not on N, its position, chunk_pairs or the aliasing.  Unscaled euclidean and cosine are int64 sums, bit for bit
 * what kpal_profile_distance_device returns; everything else within 1e-9 relative of the reference (exactly 0, the same NaN
 * and infinity).  chunk_pairs: the chunk of kpal_paired_distance_device, cut further so that the pyramids of a chunk stay
 * within 32 GiB (never below one pair); > 0 only lowers it. */
int kpal_paired_smooth_distance_device(kpal_ctx *ctx, int k, int64_t N, const int64_t *dev_left /* N x 4^k */,
                                       const int64_t *dev_right /* N x 4^k */, const kpal_distance_options *opt,
                                       int64_t chunk_pairs, double *out /* host, N */);
int kpal_paired_smooth_distance(kpal_ctx *ctx, int k, int64_t N, const int64_t *const *host_left,
                                const int64_t *const *host_right, const kpal_distance_options *opt,
                                double *out /* host, N */);
/* The effect of ProfileDistance.dynamic_smooth(left[i], right[i]) (kdistlib.py:53-124) on copies, for all i: the pyramids
 * as above, then ONE kernel that writes both smoothed sets -- a bin no node above which collapses keeps its count, the first
 * bin of a collapsed node holds the node's sum (wrapping int64), every other bin is 0.  The inputs may alias in any way and
 * are never written (table j under a lag is smoothed differently as the left of pair j and as the right of pair j - lag:
 * hence two whole output sets).  Queued on the context's stream.  KPAL_E_INVALID before any launch: what
 * kpal_paired_distance_device refuses, summary outside KPAL_SUMMARY_*, outputs that are not 16-byte aligned or that overlap
 * each other or an input. */
int kpal_paired_smooth_device(kpal_ctx *ctx, int k, int64_t N, const int64_t *dev_left /* N x 4^k */,
                              const int64_t *dev_right /* N x 4^k */, int summary, double threshold, int64_t chunk_pairs,
                              int64_t *dev_out_left /* N x 4^k */, int64_t *dev_out_right /* N x 4^k */);

/* ---- profile summaries, merge, shrink ---- */
/* Profile.total / non_zero / mean / median / std (kpal/klib.py:193-225) of one int64 vector in two
 * streaming passes plus a radix select for the median.  total wraps like ndarray.sum(); mean and std
 * follow NumPy's float64 formulation (an exact 128-bit sum, then sum((x - mean)^2) / n), <= 1e-9
 * relative; median, min and max are exact. */
typedef struct kpal_profile_stats {
    int64_t total;     /* counts.sum(), int64 wrap */
    int64_t non_zero;  /* np.count_nonzero(counts) */
    int64_t min, max;
    double mean;       /* counts.mean() */
    double median;     /* np.median(counts): mean of the two middle elements for even n */
    double std;        /* counts.std(), population standard deviation */
} kpal_profile_stats;
int kpal_stats(kpal_ctx *ctx, size_t n, const int64_t *host_counts, kpal_profile_stats *out);
int kpal_stats_device(kpal_ctx *ctx, size_t n, const int64_t *dev_counts, kpal_profile_stats *out);

/* The same summaries (kpal/klib.py:193-225) for every one of n_tables vectors of `bins` entries lying one behind the other,
 * replacing a loop of kpal_stats calls (one per profile of `kpal count --by-record`, `kpal info`, `kpal stats`): a number of
 * launches and two synchronisations per pass that do not grow with n_tables -- six launches and two per 8-bit digit of the
 * radix select, as many digits as the widest value range of the pass needs.  A vector's summary does not depend on the set it is
 * in nor on its place there, bit for bit; values as kpal_stats (total, non_zero, min, max and median exact; mean and std
 * <= 1e-9 relative).  Passes are cut inside (stat_plan.hpp: scratch budget, 65535 profiles); KPAL_STAT_SET_PROFILES, read on
 * every call, lowers the profiles of a pass.  KPAL_E_INVALID: a NULL pointer, n_tables == 0, bins == 0, tables not 8-byte
 * aligned.  The host variant uploads through the context's scratch. */
int kpal_stats_set_device(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *dev_tables /* n_tables x bins */,
                          kpal_profile_stats *host_out /* n_tables */);
int kpal_stats_set(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *host_tables,
                   kpal_profile_stats *host_out);
/* kmer.get_balance scores (kpal/kmer.py:243-245) of n_tables consecutive 4^k tables, replacing a loop of kpal_strand_balance
 * calls (each of which is this entry with n_tables = 1): the fused split + multiset kernel over tiles x profiles and one
 * reduction per pass.  KPAL_E_INVALID: k outside
 * 1..KPAL_MAX_K, a NULL pointer, n_tables == 0, a pairwise other than prod or sum, tables not 8-byte aligned. */
int kpal_strand_balance_set_device(kpal_ctx *ctx, int k, size_t n_tables, const int64_t *dev_tables /* n_tables x 4^k */,
                                   int pairwise, double *host_out /* n_tables */);
int kpal_strand_balance_set(kpal_ctx *ctx, int k, size_t n_tables, const int64_t *host_tables, int pairwise,
                            double *host_out);
/* metrics.distribution (kpal/metrics.py:22-33) of every one of n_tables int64 vectors of `bins` entries lying one behind the
 * other -- the count-of-counts spectrum: for table t the pairs offsets[t] .. offsets[t+1]-1, values ascending (signed order),
 * number >= 1, the numbers of a table summing to bins.  Exact for every int64 input (values are compared as order-preserving
 * uint64 keys, every counter is 64-bit).  Without a sort: per pass six launches, one more if any entry lies past its table's
 * dense window (spectrum_plan.hpp: the keys [min, min + W) of a table, W = min(widest spread of the pass, bins, 2^20)), and
 * three synchronisations, whatever n_tables is; the entries past the window are sorted on the host.  A table's pairs do not
 * depend on the set it is in, on its place there, or on where the passes are cut (scratch budget, 65535 tables;
 * KPAL_STAT_SET_PROFILES, read on every call, lowers the tables of a pass).  The pairs stay with the context until the next
 * distribution call or kpal_ctx_destroy; kpal_distribution_fetch copies pairs [first_pair, first_pair + n_pairs) out, in
 * as many pieces as the caller likes.  KPAL_E_INVALID: a NULL pointer, n_tables == 0, bins == 0, tables not 8-byte aligned;
 * fetch with no distribution pending or with a range past the last pair.  The host variant uploads through the context's
 * scratch.  One table is a set of one. */
int kpal_distribution_set_device(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *dev_tables /* n_tables x bins */,
                                 uint64_t *host_offsets /* n_tables + 1 */);
int kpal_distribution_set(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *host_tables, uint64_t *host_offsets);
int kpal_distribution_fetch(kpal_ctx *ctx, uint64_t first_pair, uint64_t n_pairs, int64_t *host_values, uint64_t *host_numbers);

/* Profile.merge(profile, merger) for the built-in metrics.mergers (kpal/metrics.py:174-179,
 * kpal/klib.py:269-283): out = merger(left, right); out may be left or right. */
#define KPAL_MERGE_SUM 0   /* x + y */
#define KPAL_MERGE_XOR 1   /* (x + y) * logical_xor(x, y) */
#define KPAL_MERGE_INT 2   /* x * bool(y) */
#define KPAL_MERGE_NINT 3  /* x * logical_not(y) */
int kpal_merge(kpal_ctx *ctx, size_t n, const int64_t *host_left, const int64_t *host_right, int merger,
               int64_t *host_out);
int kpal_merge_device(kpal_ctx *ctx, size_t n, const int64_t *dev_left, const int64_t *dev_right, int merger,
                      int64_t *dev_out);

/* Profile.shrink(factor), kpal/klib.py:329-352: out[j] = sum of the 4^factor counts that share the
 * (k - factor)-mer prefix j; 1 <= factor < k (else KPAL_E_INVALID, the reference's ValueError);
 * out has 4^(k - factor) entries and must not overlap the input.  8-byte alignment of both is enough: the
 * device entry reads 16 bytes at a time only where dev_counts is 16-byte aligned. */
int kpal_shrink(kpal_ctx *ctx, int k, int factor, const int64_t *host_counts, int64_t *host_out);
int kpal_shrink_device(kpal_ctx *ctx, int k, int factor, const int64_t *dev_counts, int64_t *dev_out);

/* ---- new tables out of whole sets of tables in HBM: balance, shrink, pool ---- */
/* Every entry takes n_tables tables lying one behind the other on the device, queues its launches on the context's stream
 * and returns without waiting, like kpal_balance_device.  KPAL_E_INVALID, with nothing launched: a NULL pointer, n_tables == 0,
 * k outside 1..KPAL_MAX_K, bins == 0, a pointer that is not 8-byte aligned, more bytes than a size_t counts, and an output that
 * overlaps the input in a way the entry does not allow.  (The merge of two sets is kpal_merge_device over all their entries.)
 *
 * Profile.balance (kpal/klib.py:285-298) of every table: out[t][i] = in[t][i] + in[t][rc(i)], replacing a loop of
 * kpal_balance_device calls by ONE launch -- for k >= 6 persistent workgroups over the flat list of (table, canonical tile
 * pair), for k <= 5 one index over all bins.  dev_out == dev_in is allowed; any other overlap is KPAL_E_INVALID.  A table's
 * result does not depend on the set it is in. */
int kpal_balance_set_device(kpal_ctx *ctx, int k, size_t n_tables, const int64_t *dev_in /* n_tables x 4^k */,
                            int64_t *dev_out /* n_tables x 4^k */);
/* Profile.shrink(factor) (kpal/klib.py:329-352) of every table in one launch (from k = 12 on, where one launch over the whole
 * set was measured to lose, in one per table: transform_plan.hpp): 1 <= factor < k (else KPAL_E_INVALID with the reference's
 * ValueError text); dev_out has n_tables x 4^(k - factor) entries and must not overlap the input. */
int kpal_shrink_set_device(kpal_ctx *ctx, int k, int factor, size_t n_tables, const int64_t *dev_in /* n_tables x 4^k */,
                           int64_t *dev_out);
/* Profile.merge with the sum merger (kpal/klib.py:269-283; kpal/metrics.py:174) folded over the set: out[j] = the sum over t
 * of tables[t][j], int64 wrap; accumulate != 0: added onto what dev_out holds.  At most two launches whatever n_tables is: the
 * tables are cut into slices (transform_plan.hpp) whose partial rows, in the context's scratch, a second launch adds.  dev_out
 * has `bins` entries and must not overlap the tables. */
int kpal_pool_set_device(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *dev_tables /* n_tables x bins */,
                         int accumulate, int64_t *dev_out /* bins */);
/* The pool BY LABEL: out[g][j] = (accumulate ? out[g][j] : 0) + the sum over the tables t with labels[t] == g of tables[t][j],
 * int64 wrap.  `labels` is a HOST array: a label in [0, n_groups) names the group of a table, a negative one no group, a label
 * >= n_groups is KPAL_E_INVALID.  The host inverts the labels into one member list per group and cuts long lists into chunks
 * (pool_groups_plan.hpp); that index goes up in one copy, which the call waits for.  Then every table is read once, where it
 * lies: ONE launch ("pool_groups") when no list is cut, exactly TWO otherwise ("pool_groups", whose partial rows go to the
 * context's scratch, and "pool_groups_final"), whatever n_tables and n_groups are.  A group without a table becomes zeros, or
 * with accumulate != 0 keeps what it holds.  dev_out has n_groups x bins entries and must not overlap the tables; the other
 * refusals are those of kpal_pool_set_device, and n_groups == 0. */
int kpal_pool_groups_device(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *dev_tables /* n_tables x bins */,
                            const int64_t *labels /* HOST, n_tables */, size_t n_groups, int accumulate,
                            int64_t *dev_out /* n_groups x bins */);

/* ---- per-kernel timing with HIP events on the ctx stream (bench.py roofline leg) ---- */
int kpal_prof_enable(kpal_ctx *ctx, int on);
int kpal_prof_reset(kpal_ctx *ctx);
int kpal_prof_count(kpal_ctx *ctx, int *n_kernels);
int kpal_prof_get(kpal_ctx *ctx, int index, char *name_out, size_t name_cap, double *total_ms,
                  uint64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* KPAL_HIP_H */
