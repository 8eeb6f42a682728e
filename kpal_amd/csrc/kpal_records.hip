// kpal_records.hip -- one profile per record or per sliding window of a FASTA text, per read or per window of a read of a FASTQ
// text: kpal_count_records, the record index over memory and over a file the library reads itself (kpal_fasta_records_*,
// kpal_fastq_records_*: one index, filled by either format), the sliding windows (kpal_fasta_windows_*).  The scan of a file
// -- gather, cut, index, carry -- is RecordScan (record_scan.hpp: free of HIP, driven under sanitizers by
// tests/native/record_scan_check.cpp); this unit gives it the pinned staging buffer and the device index of either format.
#include "kpal_host.hpp"

#include "count_kernels.hpp"
#include "count_plan.hpp"
#include "fasta_kernels.hpp"
#include "record_scan.hpp"
#include "window_kernels.hpp"

// one table per record: the k-mers of `s` into out[r], r the record (of the n that begin at starts[0 .. n]) their last byte lies in
static int launch_count_records(kpal_ctx *ctx, int k, const Span &s, const uint64_t *starts, uint32_t n, unsigned long long *out)
{
    const WaveGrid w = wave_grid((s.nchunks + 63) / 64, ctx->num_cu, 8, 4);
    DISPATCH_K_1_16(k, LAUNCH(ctx, "count_records", (count_records_kernel<K>), dim3(w.grid), dim3(256), s, w.spw, starts, n, out));
    return KPAL_OK;
}

KPAL_API int kpal_count_records(kpal_ctx *ctx, int k, const uint8_t *host_flat, size_t nbytes, const uint64_t *host_starts,
                                size_t n_records, int64_t *host_out)
{
    CTX_ENTER(ctx);
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range 1..%d", k, KPAL_MAX_K);
    if (n_records == 0) return KPAL_OK;
    if (!host_starts || !host_out || (nbytes && !host_flat)) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (n_records >= 0xFFFFFFFFull) return set_err(KPAL_E_INVALID, "too many records in one batch");
    if (host_starts[0] != 0 || host_starts[n_records] != nbytes) return set_err(KPAL_E_INVALID, "starts must run from 0 to nbytes");
    for (size_t r = 0; r < n_records; ++r)
        if (host_starts[r] > host_starts[r + 1]) return set_err(KPAL_E_INVALID, "starts must be ascending");
    const uint64_t bins = 1ULL << (2 * k);
    const size_t out_bytes = n_records * bins * sizeof(int64_t);
    CHK(ensure(ctx, ctx->scratch[0], out_bytes));
    CHK(ensure(ctx, ctx->scratch[1], nbytes + 64));
    CHK(ensure(ctx, ctx->scratch[2], (n_records + 1) * sizeof(uint64_t)));
    HIPCHK(hipMemsetAsync(ctx->scratch[0].p, 0, out_bytes, ctx->stream));
    if (nbytes) {
        HIPCHK(hipMemcpyAsync(ctx->scratch[1].p, host_flat, nbytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->scratch[2].p, host_starts, (n_records + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        const Span s = make_span((const uint8_t *)ctx->scratch[1].p, nbytes, 0);
        CHK(launch_count_records(ctx, k, s, (const uint64_t *)ctx->scratch[2].p, (uint32_t)n_records, (unsigned long long *)ctx->scratch[0].p));
    }
    HIPCHK(hipMemcpyAsync(host_out, ctx->scratch[0].p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return KPAL_OK;
}

// ----------------------------------------------------------------------------------------------
// Profile.from_fasta_by_record (kpal/klib.py:114-133) with the records tokenised on the device: the text (whole records; the
// caller cuts at record boundaries) is flattened by the kernels of the FASTA ingest, and two compactions list where every record
// starts in the flattened stream and where its header line starts in the text -- the host reads the header lines only (names).
// kpal_fasta_records_count then counts batches of records into one table each (count_records_kernel), as many as the caller has
// room for.
// ----------------------------------------------------------------------------------------------
// text[0, m) -> raw on the device through the pinned staging buffers (host threads copy piece i + 1 while the DMA takes piece i)
// in_pinned0: the text lies in ctx->pinned[0] (the file reader put it there): the DMA engine reads it in place
static int records_upload(kpal_ctx *ctx, uint8_t *raw, const uint8_t *text, size_t m, bool in_pinned0)
{
    CHK(ensure_pinned(ctx));
    if (in_pinned0) {
        CHK(pinned_wait(ctx, 0));   // (an earlier DMA out of the buffer: long done, the caller has refilled it)
        CHK(pinned_h2d(ctx, 0, raw, text, m));
    } else {
        const size_t stage = kpal_ctx::kStage;
        int slot = 0;
        for (size_t off = 0; off < m; off += stage, slot ^= 1) {
            const size_t len = std::min(stage, m - off);
            CHK(pinned_wait(ctx, slot));
            staged_memcpy(ctx->pinned[slot], text + off, len);
            CHK(pinned_h2d(ctx, slot, raw + off, ctx->pinned[slot], len));
        }
    }
    return KPAL_OK;
}

// the context holds no index
static void records_index_clear(kpal_ctx *ctx)
{
    ctx->rec_n = ctx->rec_nf = 0;
    ctx->win_window = ctx->win_step = 0;
    ctx->rec_starts_host.clear();
    ctx->rec_hdr_host.clear();
}

// The end of both record indexes.  The caller has flattened the text into flat[0, nf), found R records in it and queued their R
// header offsets into rec_hdr.  Here the record starts of the stream -- its '\n' bytes -- are counted, compared with R and only
// then listed (the list has room for R of them and nf behind them); both lists come to the host and the index is the
// context's.  offs, marks: scratch of one offset (+ 1) and one mark per kFaBlockBytes of the stream.  kIndexMismatch: the
// stream holds *seps record starts, not R -- the caller says so in its own words; the context holds no index then.
constexpr int kIndexMismatch = 1;
static int records_index_finish(kpal_ctx *ctx, const uint8_t *flat, uint64_t nf, uint64_t R, uint64_t *offs, uint32_t *marks, uint64_t *seps)
{
    CHK(ensure(ctx, ctx->rec_starts, (size_t)(R + 1) * 8));
    const uint32_t fblocks = (uint32_t)((nf + kFaBlockBytes - 1) / kFaBlockBytes);
    LAUNCH(ctx, "fa_mark_count", (fa_mark_count_kernel<0>), dim3(fblocks), dim3(kFaThreads), flat, nf, marks);
    LAUNCH(ctx, "fa_offset", fa_offset_kernel, dim3(1), dim3(256), (const uint32_t *)marks, fblocks, offs);
    *seps = 0;
    HIPCHK(hipMemcpyAsync(seps, offs + fblocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (*seps != R) return kIndexMismatch;
    LAUNCH(ctx, "fa_mark_scatter", (fa_mark_scatter_kernel<0>), dim3(fblocks), dim3(kFaThreads), flat, nf, (const uint64_t *)offs,
           (uint64_t *)ctx->rec_starts.p);
    HIPCHK(hipMemcpyAsync((uint64_t *)ctx->rec_starts.p + R, &nf, sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    ctx->rec_hdr_host.resize((size_t)R);
    ctx->rec_starts_host.resize((size_t)R + 1);
    HIPCHK(hipMemcpyAsync(ctx->rec_hdr_host.data(), ctx->rec_hdr.p, (size_t)R * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->rec_starts_host.data(), ctx->rec_starts.p, (size_t)R * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->rec_starts_host[(size_t)R] = nf;
    ctx->rec_n = R;
    ctx->rec_nf = nf;
    return KPAL_OK;
}

// in_pinned0: host_text lies in ctx->pinned[0] (records_upload)
static int fasta_records_index_text(kpal_ctx *ctx, const uint8_t *host_text, size_t nbytes, bool in_pinned0, uint64_t *n_records, uint64_t *flat_bytes)
{
    *n_records = *flat_bytes = 0;
    records_index_clear(ctx);
    const size_t first = nbytes ? fasta_first_header(host_text, nbytes, true) : 0;   // text before the first header is no record (klib.py:131: SeqIO)
    if (first >= nbytes) return KPAL_OK;
    const uint8_t *text = host_text + first;
    const size_t m = nbytes - first;
    const size_t pad = kpal_ctx::kStagePad;
    const uint32_t nblocks = (uint32_t)((m + kFaBlockBytes - 1) / kFaBlockBytes);
    CHK(ensure(ctx, ctx->rec_raw, m + 64));
    CHK(ensure(ctx, ctx->rec_flat, m + pad + 64));
    CHK(ensure(ctx, ctx->rec_meta, (size_t)nblocks * (8 + 8 + 4 + 4) + 2 * (size_t)(nblocks + 1) * 8 + 128));
    uint8_t *raw = (uint8_t *)ctx->rec_raw.p;
    uint8_t *flat = (uint8_t *)ctx->rec_flat.p + pad;
    CHK(records_upload(ctx, raw, text, m, in_pinned0));
    // the flattening; behind its scratch the header lines' offsets (offs2) and the marks of both compactions
    uint64_t *offs, *offs2;
    CHK(fa_flatten(ctx, raw, m, 0, 1, flat, ctx->rec_meta.p, &offs, (void **)&offs2));
    uint32_t *marks = (uint32_t *)(offs2 + nblocks + 1);
    // header lines of the text
    LAUNCH(ctx, "fa_mark_count", (fa_mark_count_kernel<1>), dim3(nblocks), dim3(kFaThreads), (const uint8_t *)raw, (uint64_t)m, marks);
    LAUNCH(ctx, "fa_offset", fa_offset_kernel, dim3(1), dim3(256), (const uint32_t *)marks, nblocks, offs2);
    uint64_t sizes[2] = {0, 0};   // flattened bytes, records
    HIPCHK(hipMemcpyAsync(&sizes[0], offs + nblocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&sizes[1], offs2 + nblocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const uint64_t nf = sizes[0], R = sizes[1];
    if (R == 0 || nf < R) return set_err(KPAL_E_HIP, "record index: %llu records in %llu flattened bytes", (unsigned long long)R, (unsigned long long)nf);
    CHK(ensure(ctx, ctx->rec_hdr, (size_t)R * 8));
    LAUNCH(ctx, "fa_mark_scatter", (fa_mark_scatter_kernel<1>), dim3(nblocks), dim3(kFaThreads), (const uint8_t *)raw, (uint64_t)m, (const uint64_t *)offs2,
           (uint64_t *)ctx->rec_hdr.p);
    // (offs / marks are free again: the flattening is done; the stream is no longer than the text)
    uint64_t seps;
    const int rc = records_index_finish(ctx, flat, nf, R, offs, marks, &seps);
    if (rc == kIndexMismatch)
        return set_err(KPAL_E_HIP, "record index: %llu header lines but %llu separators", (unsigned long long)R, (unsigned long long)seps);
    CHK(rc);
    for (uint64_t &h : ctx->rec_hdr_host) h += first;
    *n_records = R;
    *flat_bytes = nf;
    return KPAL_OK;
}

KPAL_API int kpal_fasta_records_begin(kpal_ctx *ctx, const uint8_t *host_text, size_t nbytes, uint64_t *n_records, uint64_t *flat_bytes)
{
    CTX_ENTER(ctx);
    if (!n_records || !flat_bytes || (nbytes && !host_text)) return set_err(KPAL_E_INVALID, "NULL pointer");
    return fasta_records_index_text(ctx, host_text, nbytes, false, n_records, flat_bytes);
}

// ----------------------------------------------------------------------------------------------
// Profile.from_fastq_by_record / _by_window: the same index over FASTQ text.  The piece -- it begins at a title line; it may end
// anywhere unless `fin` -- is tokenised by the count path's own function (fq_tokenise: validation, mask, flattening), which
// leaves the newline positions and the status words behind: the records the piece finishes (R), the byte where the unfinished
// rest begins (*consumed), the flattened size.  Title offsets come from the newline positions (fq_title_offsets_kernel), flat
// starts from the '\n' bytes of the stream (fastq_kernels.hpp says why).  Everything that counts reads the index only.
// ----------------------------------------------------------------------------------------------
static int fastq_records_index_text(kpal_ctx *ctx, const uint8_t *host_text, size_t nbytes, bool in_pinned0, FqMask mask, bool fin,
                                    uint64_t records_before, uint64_t *n_records, uint64_t *flat_bytes, uint64_t *consumed)
{
    *n_records = *flat_bytes = *consumed = 0;
    records_index_clear(ctx);
    if (nbytes == 0) return KPAL_OK;
    const uint64_t n = nbytes;
    if (n >= ((uint64_t)1 << 32) - 64) return fq_chunk_too_long(records_before);
    const size_t pad = kpal_ctx::kStagePad;
    const uint32_t nblocks = (uint32_t)((n + kFaBlockBytes - 1) / kFaBlockBytes);
    CHK(ensure(ctx, ctx->rec_raw, n + 64));
    CHK(ensure(ctx, ctx->rec_flat, n + pad + 64));
    CHK(ensure(ctx, ctx->rec_meta, (size_t)(nblocks + 1) * 8 + (size_t)nblocks * 4 + 64));
    uint8_t *raw = (uint8_t *)ctx->rec_raw.p;
    uint8_t *flat = (uint8_t *)ctx->rec_flat.p + pad;
    uint64_t *offs = (uint64_t *)ctx->rec_meta.p;
    uint32_t *marks = (uint32_t *)(offs + nblocks + 1);
    CHK(records_upload(ctx, raw, host_text, n, in_pinned0));
    CHK(fq_tokenise(ctx, raw, n, fin, mask, flat));
    const unsigned long long *hs;
    CHK(fq_tokenise_wait(ctx, records_before, &hs));
    const uint64_t R = hs[2], nf = hs[4], used = fin ? n : hs[3];
    if (used > n || nf > n || nf < R)
        return set_err(KPAL_E_HIP, "FASTQ record index: %llu records, %llu flattened bytes, rest at %llu of %llu bytes", (unsigned long long)R,
                       (unsigned long long)nf, (unsigned long long)used, (unsigned long long)n);
    *consumed = used;
    if (R == 0) return KPAL_OK;
    CHK(ensure(ctx, ctx->rec_hdr, (size_t)R * 8));
    CHK(fq_title_offsets(ctx, R, (uint64_t *)ctx->rec_hdr.p));
    uint64_t seps;
    const int rc = records_index_finish(ctx, flat, nf, R, offs, marks, &seps);
    if (rc == kIndexMismatch)
        return set_err(KPAL_E_HIP, "FASTQ record index: the tokeniser reports %llu records but the stream holds %llu record starts",
                       (unsigned long long)R, (unsigned long long)seps);
    CHK(rc);
    *n_records = R;
    *flat_bytes = nf;
    return KPAL_OK;
}

KPAL_API int kpal_fastq_records_begin(kpal_ctx *ctx, const uint8_t *host_text, size_t nbytes, const kpal_fastq_options *opt, int final,
                                      uint64_t records_before, uint64_t *n_records, uint64_t *flat_bytes, uint64_t *consumed)
{
    CTX_ENTER(ctx);
    if (!n_records || !flat_bytes || !consumed || (nbytes && !host_text)) return set_err(KPAL_E_INVALID, "NULL pointer");
    FqMask mask;
    if (int rc = fq_mask_options(opt, mask)) {   // (every other error leaves through fastq_records_index_text, which has cleared both by then)
        *n_records = *flat_bytes = *consumed = 0;
        records_index_clear(ctx);
        return rc;
    }
    return fastq_records_index_text(ctx, host_text, nbytes, false, mask, final != 0, records_before, n_records, flat_bytes, consumed);
}

// ---- the same over a FILE the library reads itself (no byte of the text passes through Python): every
// kpal_fasta_records_file_next indexes the next piece of WHOLE records, or reads.  The scan -- what is gathered into the pinned
// staging buffer, where either format is cut, what is carried to the next piece, how a record longer than the buffer is
// gathered -- is RecordScan (record_scan.hpp, GPU-free; tests/native/record_scan_check.cpp drives it under sanitizers); here it
// is given the buffer, its guard and the index of the scan's format.
static int records_file_open(kpal_ctx *ctx, const char *path, uint64_t begin, uint64_t end)
{
    ctx->rec_scan.scan.close();
    FaSource src;
    CHK(open_text_range(path, begin, end, src));
    ctx->rec_scan.scan.open(src);
    ctx->rec_scan.fastq = false;
    ctx->rec_scan.records = 0;
    return KPAL_OK;
}

KPAL_API int kpal_fasta_records_file_open(kpal_ctx *ctx, const char *path, uint64_t begin, uint64_t end)
{
    CTX_ENTER(ctx);
    if (!path) return set_err(KPAL_E_INVALID, "path is NULL");
    return records_file_open(ctx, path, begin, end);
}

// ... of FASTQ reads: kpal_fasta_records_file_next / _tell / _close serve the scan, piece by piece of whole reads
KPAL_API int kpal_fastq_records_file_open(kpal_ctx *ctx, const char *path, uint64_t begin, uint64_t end, const kpal_fastq_options *opt,
                                          uint64_t records_before)
{
    CTX_ENTER(ctx);
    if (!path) return set_err(KPAL_E_INVALID, "path is NULL");
    FqMask mask;
    CHK(fq_mask_options(opt, mask));
    CHK(records_file_open(ctx, path, begin, end));
    ctx->rec_scan.fastq = true;
    ctx->rec_scan.mask = mask;
    ctx->rec_scan.records = records_before;
    return KPAL_OK;
}

KPAL_API int kpal_fasta_records_file_next(kpal_ctx *ctx, uint64_t *n_records, uint64_t *flat_bytes, uint64_t *text_offset, int *done)
{
    CTX_ENTER(ctx);
    if (!n_records || !flat_bytes || !text_offset || !done) return set_err(KPAL_E_INVALID, "NULL pointer");
    *n_records = *flat_bytes = *text_offset = 0;
    *done = 1;
    RecordFileScan &rs = ctx->rec_scan;
    if (!rs.scan.is_open()) return set_err(KPAL_E_STATE, "kpal_fasta_records_file_next without kpal_fasta_records_file_open");
    CHK(ensure_pinned(ctx));
    const size_t stage = std::min<size_t>(kpal_ctx::kStage, ctx->fa_chunk);   // (KPAL_FASTA_CHUNK: tests put the seams everywhere)
    // the index of one piece: a FASTA piece is whole records, all of it; of a FASTQ piece the tokeniser says what its reads cover
    const RecordScan::Index index = [&](const uint8_t *piece, size_t n, bool in_stage, bool at_end, uint64_t *records, size_t *used) {
        if (!rs.fastq) {
            *used = n;
            return fasta_records_index_text(ctx, piece, n, in_stage, records, flat_bytes);
        }
        uint64_t consumed = 0;
        const int rc = fastq_records_index_text(ctx, piece, n, in_stage, rs.mask, at_end, rs.records, records, flat_bytes, &consumed);
        *used = (size_t)consumed;
        return rc;
    };
    ScanPiece piece;
    const int got = rs.scan.next((uint8_t *)ctx->pinned[0], stage, [ctx] { return pinned_wait(ctx, 0); },
                                 rs.fastq ? fastq_record_cut : fasta_record_cut, index, piece);
    if (got == -1) return set_err(KPAL_E_IO, "reading the %s input failed: %s", rs.fastq ? "FASTQ" : "FASTA", strerror(rs.scan.io_errno()));
    if (got == -2) return rs.scan.user_error();
    if (got == 0) {   // the end: the scan is closed
        *flat_bytes = 0;
        return KPAL_OK;
    }
    rs.records += piece.records;
    *n_records = piece.records;
    *text_offset = piece.text_offset;
    *done = 0;
    return KPAL_OK;
}

// Where the scan stands: the file offset of the first byte that no piece has covered yet (the start of the carried,
// unfinished record).  A caller that lets other work use the context between two pieces keeps THIS, closes the scan and
// opens it again there: the scan state of the context -- descriptor, position, carried bytes -- then never outlives a call.
KPAL_API int kpal_fasta_records_file_tell(kpal_ctx *ctx, uint64_t *offset)
{
    CTX_ENTER(ctx);
    if (!offset) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (!ctx->rec_scan.scan.is_open()) return set_err(KPAL_E_STATE, "kpal_fasta_records_file_tell without an open scan");
    *offset = ctx->rec_scan.scan.tell();
    return KPAL_OK;
}

KPAL_API int kpal_fasta_records_file_close(kpal_ctx *ctx)
{
    CTX_ENTER(ctx);
    ctx->rec_scan.scan.close();
    return KPAL_OK;
}

KPAL_API int kpal_fasta_records_index(kpal_ctx *ctx, uint64_t *header_off, uint64_t *flat_start)
{
    CTX_ENTER(ctx);
    if (ctx->rec_n == 0) return set_err(KPAL_E_STATE, "kpal_fasta_records_index without records (kpal_fasta_records_begin)");
    if (header_off) memcpy(header_off, ctx->rec_hdr_host.data(), (size_t)ctx->rec_n * 8);
    if (flat_start) memcpy(flat_start, ctx->rec_starts_host.data(), (size_t)(ctx->rec_n + 1) * 8);
    return KPAL_OK;
}

// the tables of records [first, first + n) of the indexed text into n x 4^k int64 of DEVICE memory (queued on the context's stream)
static int fasta_records_count_into(kpal_ctx *ctx, int k, uint64_t first, uint64_t n, unsigned long long *dev_out)
{
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range 1..%d", k, KPAL_MAX_K);
    if (first > ctx->rec_n || n > ctx->rec_n - first) return set_err(KPAL_E_INVALID, "records %llu..%llu of %llu", (unsigned long long)first,
                                                                      (unsigned long long)(first + n), (unsigned long long)ctx->rec_n);
    if (n >= 0xFFFFFFFFull) return set_err(KPAL_E_INVALID, "too many records in one batch");
    const uint64_t bins = 1ULL << (2 * k);
    const size_t out_bytes = (size_t)n * bins * sizeof(int64_t);
    const uint64_t b0 = ctx->rec_starts_host[(size_t)first], b1 = ctx->rec_starts_host[(size_t)(first + n)];
    CHK(ensure(ctx, ctx->scratch[2], (size_t)(n + 1) * sizeof(uint64_t)));
    HIPCHK(hipMemsetAsync(dev_out, 0, out_bytes, ctx->stream));
    if (b1 > b0) {
        LAUNCH(ctx, "fa_rebase", fa_rebase_kernel, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), (const uint64_t *)ctx->rec_starts.p + first, n + 1, b0,
               (uint64_t *)ctx->scratch[2].p);
        const Span s = make_span((const uint8_t *)ctx->rec_flat.p + kpal_ctx::kStagePad + b0, (size_t)(b1 - b0), 0);
        CHK(launch_count_records(ctx, k, s, (const uint64_t *)ctx->scratch[2].p, (uint32_t)n, dev_out));
    }
    return KPAL_OK;
}

KPAL_API int kpal_fasta_records_count(kpal_ctx *ctx, int k, uint64_t first, uint64_t n, int64_t *host_out)
{
    CTX_ENTER(ctx);
    if (n == 0) return KPAL_OK;
    if (!host_out) return set_err(KPAL_E_INVALID, "host_out is NULL");
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range 1..%d", k, KPAL_MAX_K);
    const size_t out_bytes = (size_t)n * ((size_t)1 << (2 * k)) * sizeof(int64_t);
    CHK(ensure(ctx, ctx->scratch[0], out_bytes));
    CHK(fasta_records_count_into(ctx, k, first, n, (unsigned long long *)ctx->scratch[0].p));
    HIPCHK(hipMemcpyAsync(host_out, ctx->scratch[0].p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return KPAL_OK;
}

// ... into the CALLER's device memory (kpal_dev_alloc): the profiles of a by-record scan that stay in HBM until something on the
// host asks for their counts (kpal_amd/klib.py: Profile.counts is materialised lazily; distances and matrices of such profiles
// read the device copies)
KPAL_API int kpal_fasta_records_count_device(kpal_ctx *ctx, int k, uint64_t first, uint64_t n, int64_t *dev_out)
{
    CTX_ENTER(ctx);
    if (n == 0) return KPAL_OK;
    if (!dev_out) return set_err(KPAL_E_INVALID, "dev_out is NULL");
    CHK(fasta_records_count_into(ctx, k, first, n, (unsigned long long *)dev_out));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // (the index may be overwritten by the caller's next piece)
    return KPAL_OK;
}

// ----------------------------------------------------------------------------------------------
// Profile.from_fasta_by_window: one profile per sliding window of every indexed record (window_kernels.hpp; the layout
// arithmetic is window_index.hpp).  Tile tables, running sum along the tiles, trim of the windows that end inside their
// record: three launches per call (two when window == step), whatever window / step is.
// ----------------------------------------------------------------------------------------------
constexpr size_t kWinTileBytes = (size_t)2 << 30;   // tile tables of one pass (a longer range of windows is counted in several)

// first window / first tile of every indexed record for (window, step), on the host and on the device
static int fasta_windows_prepare(kpal_ctx *ctx, uint64_t W, uint64_t S)
{
    if (S < 1 || S > W || W % S != 0)
        return set_err(KPAL_E_INVALID, "window=%llu step=%llu: need 1 <= step <= window and window %% step == 0", (unsigned long long)W, (unsigned long long)S);
    if (W > (1ULL << 62)) return set_err(KPAL_E_INVALID, "window=%llu is too large", (unsigned long long)W);
    if (ctx->rec_n == 0) return set_err(KPAL_E_STATE, "kpal_fasta_windows_* without records (kpal_fasta_records_begin)");
    if (ctx->win_window == W && ctx->win_step == S) return KPAL_OK;
    const size_t R = (size_t)ctx->rec_n;
    ctx->win_window = ctx->win_step = 0;
    ctx->win_first_host.resize(R + 1);
    ctx->win_tile_host.resize(R + 1);
    win_layout(ctx->rec_starts_host.data(), R, W, S, ctx->win_first_host.data(), ctx->win_tile_host.data());
    CHK(ensure(ctx, ctx->win_index, 2 * (R + 1) * sizeof(uint64_t)));
    HIPCHK(hipMemcpyAsync(ctx->win_index.p, ctx->win_first_host.data(), (R + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync((uint64_t *)ctx->win_index.p + R + 1, ctx->win_tile_host.data(), (R + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->win_window = W;
    ctx->win_step = S;
    return KPAL_OK;
}

// windows [first, first + n) -- made from the tiles and bytes of `rg` -- into n x 4^k int64 of device memory
static int fasta_windows_pass(kpal_ctx *ctx, int k, uint64_t W, uint64_t S, uint64_t first, uint64_t n, const WinRange &rg, unsigned long long *dev_out)
{
    const uint64_t bins = 1ULL << (2 * k), m = W / S;
    const uint64_t R = ctx->rec_n, ntiles = rg.tile1 - rg.tile0;
    const uint64_t *index = (const uint64_t *)ctx->win_index.p;
    const WinGeom g = {(const uint64_t *)ctx->rec_starts.p, index, index + R + 1, R, W, S, first, n, rg.tile0, rg.tile1};
    const uint8_t *flat = (const uint8_t *)ctx->rec_flat.p + kpal_ctx::kStagePad;
    unsigned long long *tiles = dev_out;   // window == step: the tiles are the windows
    if (m > 1) {
        CHK(ensure(ctx, ctx->win_tiles, (size_t)ntiles * bins * sizeof(int64_t)));
        tiles = (unsigned long long *)ctx->win_tiles.p;
    }
    if (k <= 7 && S < (1ULL << 32)) {   // histograms in LDS (u32 bins: a tile holds fewer than 2^32 k-mers)
        const Span s = make_span(flat, (size_t)ctx->rec_nf, 0);
        if (S <= 2048) {
            DISPATCH_K_1_7(k, {
                constexpr int TPW = WinTileCfg<K>::kSmallTpw;
                const unsigned grid = (unsigned)std::min<uint64_t>((ntiles + TPW - 1) / TPW, (uint64_t)ctx->num_cu * 8);
                LAUNCH(ctx, "window_tiles", (window_tiles_lds_kernel<K, TPW, 4>), dim3(grid), dim3(256), s, g, tiles);
            });
        } else {
            const unsigned grid = (unsigned)std::min<uint64_t>(ntiles, (uint64_t)ctx->num_cu * 4);
            DISPATCH_K_1_7(k, LAUNCH(ctx, "window_tiles", (window_tiles_lds_kernel<K, 1, 8>), dim3(grid), dim3(512), s, g, tiles));
        }
    } else {
        HIPCHK(hipMemsetAsync(tiles, 0, (size_t)ntiles * bins * sizeof(int64_t), ctx->stream));
        const Span s = make_span(flat + rg.byte0, (size_t)(rg.byte1 - rg.byte0), 0);
        const WaveGrid w = wave_grid((s.nchunks + 63) / 64, ctx->num_cu, 8, 4);
        DISPATCH_K_1_16(k, LAUNCH(ctx, "window_tiles_atomic", (window_tiles_atomic_kernel<K>), dim3(w.grid), dim3(256), s, w.spw, rg.byte0, g, tiles));
    }
    if (m > 1) {
        // segments of at least m windows (the m loads of a segment's first sum then cost no more than one per window),
        // longer ones once the device is full
        const uint64_t threads = (uint64_t)ctx->num_cu * 2048;
        const uint64_t segment = std::max<uint64_t>(m, (n * bins + threads - 1) / threads);
        const uint64_t n_segments = (n + segment - 1) / segment;
        const uint64_t blocks = bins < (uint64_t)kWinSlideThreads ? (n_segments + kWinSlideThreads / bins - 1) / (kWinSlideThreads / bins)
                                                                   : n_segments * (bins / kWinSlideThreads);
        if (blocks > 0x7FFFFFFFull) return set_err(KPAL_E_INVALID, "too many windows in one batch");
        LAUNCH(ctx, "window_slide", window_slide_kernel, dim3((unsigned)blocks), dim3(kWinSlideThreads), g, bins, segment, n_segments,
               (const unsigned long long *)tiles, dev_out);
    }
    LAUNCH(ctx, "window_trim", window_trim_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), g, k, flat, dev_out);
    return KPAL_OK;
}

static int fasta_windows_count_into(kpal_ctx *ctx, int k, uint64_t W, uint64_t S, uint64_t first, uint64_t n, unsigned long long *dev_out)
{
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range 1..%d", k, KPAL_MAX_K);
    CHK(fasta_windows_prepare(ctx, W, S));
    if ((uint64_t)k > W) return set_err(KPAL_E_INVALID, "k=%d is longer than the window (%llu)", k, (unsigned long long)W);
    const uint64_t R = ctx->rec_n, total = ctx->win_first_host[(size_t)R];
    if (first > total || n > total - first) return set_err(KPAL_E_INVALID, "windows %llu..%llu of %llu", (unsigned long long)first,
                                                           (unsigned long long)(first + n), (unsigned long long)total);
    if (n >= 0x7FFFFFFFull * 256) return set_err(KPAL_E_INVALID, "too many windows in one batch");
    const uint64_t bins = 1ULL << (2 * k);
    const uint64_t cap = std::max<uint64_t>(1, kWinTileBytes / (bins * sizeof(int64_t)));
    const uint64_t *starts = ctx->rec_starts_host.data(), *fw = ctx->win_first_host.data(), *ft = ctx->win_tile_host.data();
    for (uint64_t done = 0; done < n;) {
        uint64_t c = n - done;
        WinRange rg = win_range(starts, fw, ft, R, k, W, S, first + done, c);
        while (W != S && rg.tile1 - rg.tile0 > cap && c > 1) {   // (the tile tables of a pass stay within kWinTileBytes)
            c = (c + 1) / 2;
            rg = win_range(starts, fw, ft, R, k, W, S, first + done, c);
        }
        CHK(fasta_windows_pass(ctx, k, W, S, first + done, c, rg, dev_out + done * bins));
        done += c;
    }
    return KPAL_OK;
}

KPAL_API int kpal_fasta_windows_layout(kpal_ctx *ctx, uint64_t window, uint64_t step, uint64_t *n_windows, uint64_t *first_window)
{
    CTX_ENTER(ctx);
    if (!n_windows) return set_err(KPAL_E_INVALID, "NULL pointer");
    *n_windows = 0;
    CHK(fasta_windows_prepare(ctx, window, step));
    *n_windows = ctx->win_first_host[(size_t)ctx->rec_n];
    if (first_window) memcpy(first_window, ctx->win_first_host.data(), (size_t)(ctx->rec_n + 1) * 8);
    return KPAL_OK;
}

KPAL_API int kpal_fasta_windows_count(kpal_ctx *ctx, int k, uint64_t window, uint64_t step, uint64_t first, uint64_t n, int64_t *host_out)
{
    CTX_ENTER(ctx);
    if (n && !host_out) return set_err(KPAL_E_INVALID, "host_out is NULL");
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range 1..%d", k, KPAL_MAX_K);
    const size_t out_bytes = (size_t)n * ((size_t)1 << (2 * k)) * sizeof(int64_t);
    if (n) CHK(ensure(ctx, ctx->scratch[0], out_bytes));
    CHK(fasta_windows_count_into(ctx, k, window, step, first, n, (unsigned long long *)ctx->scratch[0].p));
    if (n == 0) return KPAL_OK;
    HIPCHK(hipMemcpyAsync(host_out, ctx->scratch[0].p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return KPAL_OK;
}

KPAL_API int kpal_fasta_windows_count_device(kpal_ctx *ctx, int k, uint64_t window, uint64_t step, uint64_t first, uint64_t n, int64_t *dev_out)
{
    CTX_ENTER(ctx);
    if (n && !dev_out) return set_err(KPAL_E_INVALID, "dev_out is NULL");
    CHK(fasta_windows_count_into(ctx, k, window, step, first, n, (unsigned long long *)dev_out));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // (the index may be overwritten by the caller's next piece)
    return KPAL_OK;
}
