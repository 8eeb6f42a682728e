// kpal_text.hip -- the text ingests of a count: FASTA and FASTQ, from host memory or a byte range of a file, flattened /
// tokenised on the device (fasta_kernels.hpp, fastq_kernels.hpp) and counted chunk by chunk (kpal_count.hip: count_device_range).
#include "kpal_host.hpp"

#include "fasta_kernels.hpp"
#include "fasta_host.hpp"
#include "fastq_kernels.hpp"

#include <cerrno>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

// ----------------------------------------------------------------------------------------------
// FASTA ingest: text (a byte range of a file, or host memory) -> pinned staging -> device -> flattened on the device -> counted,
// chunk i+1 being read, copied and flattened while chunk i is counted.  Nothing in the loop waits for the GPU except for the
// flattened SIZE of the chunk before (read back asynchronously, needed on the host to launch its count), which is one whole
// chunk old by then.  The text ingests share their host side: open_text_range opens a file's range, the reader of
// fasta_host.hpp (StagedReader; FaChunker on top of it for FASTA; fa_read for one range) fills the pinned buffers, pinned_wait /
// pinned_h2d guard their reuse, and fa_flatten is the FASTA flattening of the stream and of the by-record index.
// ----------------------------------------------------------------------------------------------
// The flattening of raw[0, m) into flat (fasta_kernels.hpp): `state` says what raw[0] continues, `tail` whether blanks at its end
// trail their line (FaChunk).  Its scratch in meta: last_eol, eol_before, offs, kept.  Returns offs (offs[nblocks]: the flattened
// size) and in *rest the first 8-byte aligned byte of meta behind the scratch.
int fa_flatten(kpal_ctx *ctx, const uint8_t *raw, uint64_t m, int state, int tail, uint8_t *flat, void *meta, uint64_t **offs_out,
               void **rest)
{
    const uint32_t nblocks = (uint32_t)((m + kFaBlockBytes - 1) / kFaBlockBytes);
    long long *last_eol = (long long *)meta;
    long long *eol_before = last_eol + nblocks;
    uint64_t *offs = (uint64_t *)(eol_before + nblocks);
    uint32_t *kept = (uint32_t *)(offs + nblocks + 1);
    LAUNCH(ctx, "fa_last_eol", fa_last_eol_kernel, dim3(nblocks), dim3(kFaThreads), raw, m, last_eol);
    LAUNCH(ctx, "fa_carry", fa_carry_kernel, dim3(1), dim3(256), (const long long *)last_eol, nblocks, eol_before);
    LAUNCH(ctx, "fa_count", fa_count_kernel, dim3(nblocks), dim3(kFaThreads), raw, m, (const long long *)eol_before, state, tail, kept);
    LAUNCH(ctx, "fa_offset", fa_offset_kernel, dim3(1), dim3(256), (const uint32_t *)kept, nblocks, offs);
    LAUNCH(ctx, "fa_scatter", fa_scatter_kernel, dim3(nblocks), dim3(kFaThreads), raw, m, (const long long *)eol_before, state, tail,
           (const uint64_t *)offs, flat);
    *offs_out = offs;
    if (rest) *rest = (void *)(((uintptr_t)(kept + nblocks) + 7) & ~(uintptr_t)7);
    return KPAL_OK;
}

// The pipeline.  count: the flattened chunks are counted into the running count (windows span chunk seams through the saved
// tail of the chunk before, never a record boundary: every header leaves a '\n' in the stream); else they are copied to host_out.
static int fasta_pipeline(kpal_ctx *ctx, FaSource &src, bool count, uint8_t *host_out, uint64_t *n_out)
{
    const size_t stage = ctx->fa_chunk, pad = kpal_ctx::kStagePad;
    const size_t km1 = count ? (size_t)ctx->k - 1 : 0;
    CHK(ensure_pinned(ctx));
    if (!ctx->fa_nflat_host) {
        hipError_t e = hipHostMalloc((void **)&ctx->fa_nflat_host, 64, hipHostMallocDefault);
        if (e != hipSuccess) return set_err(KPAL_E_NOMEM, "hipHostMalloc failed: %s", hipGetErrorString(e));
    }
    CHK(ensure(ctx, ctx->fa_tail, 64));
    const uint32_t max_blocks = (uint32_t)((stage + kFaBlockBytes - 1) / kFaBlockBytes);
    for (int i = 0; i < 2; ++i) {
        CHK(ensure(ctx, ctx->fa_raw[i], stage + 64));
        CHK(ensure(ctx, ctx->fa_flat[i], stage + pad + 64));
        CHK(ensure(ctx, ctx->fa_meta[i], (size_t)max_blocks * (8 + 8 + 4) + (size_t)(max_blocks + 1) * 8 + 64));
    }
    int prev_slot = -1;          // the chunk that has been flattened but not consumed yet
    uint64_t flat_total = 0;     // flattened bytes of the chunks consumed so far (this feed)
    uint64_t out_total = 0;

    auto consume = [&](int slot) -> int {
        HIPCHK(hipEventSynchronize(ctx->ev_done[slot]));   // (its flattening finished about one chunk ago)
        const uint64_t nf = ctx->fa_nflat_host[slot];
        uint8_t *flat = (uint8_t *)ctx->fa_flat[slot].p + pad;
        if (!count) {
            if (nf) HIPCHK(hipMemcpyAsync(host_out + out_total, flat, nf, hipMemcpyDeviceToHost, ctx->stream));
            out_total += nf;
            return KPAL_OK;
        }
        const size_t h = (size_t)std::min<uint64_t>(km1, flat_total);    // flattened bytes of this feed that precede the chunk
        if (h) HIPCHK(hipMemcpyAsync(flat - h, ctx->fa_tail.p, h, hipMemcpyDeviceToDevice, ctx->stream));
        const size_t h2 = (size_t)std::min<uint64_t>(km1, h + nf);       // ... and the next one: the last bytes of [flat - h, flat + nf)
        if (h2) HIPCHK(hipMemcpyAsync(ctx->fa_tail.p, flat + nf - h2, h2, hipMemcpyDeviceToDevice, ctx->stream));
        if (nf) CHK(count_device_range(ctx, flat, (size_t)nf, h));
        flat_total += nf;
        return KPAL_OK;
    };

    // The chunker (fasta_host.hpp) reads chunk i + 1 into the other pinned buffer while the launches of chunk i are issued; a
    // pinned buffer is written again only after the DMA out of it has finished.
    FaChunker chunker(src, (uint8_t *)ctx->pinned[0], (uint8_t *)ctx->pinned[1], stage, [ctx](int slot) { return pinned_wait(ctx, slot); });
    FaChunk ck;
    for (;;) {
        const int got = chunker.next(ck);
        if (got == 0) break;
        if (got == -1) return set_err(KPAL_E_IO, "reading the FASTA input failed: %s", strerror(chunker.io_errno()));
        if (got < 0) return set_err(KPAL_E_HIP, "hipEventSynchronize failed while reading the FASTA input");
        const int slot = ck.slot;
        const uint32_t nblocks = (uint32_t)((ck.n + kFaBlockBytes - 1) / kFaBlockBytes);
        uint8_t *raw = (uint8_t *)ctx->fa_raw[slot].p;
        // the device copy of the raw text is free once the flattening that read it is done (two chunks ago)
        if (ctx->stage_used[slot]) HIPCHK(hipStreamWaitEvent(ctx->copy_stream, ctx->ev_done[slot], 0));
        CHK(pinned_h2d(ctx, slot, raw, ck.data, ck.n));
        uint64_t *offs;
        CHK(fa_flatten(ctx, raw, ck.n, ck.state, ck.tail_trailing ? 1 : 0, (uint8_t *)ctx->fa_flat[slot].p + pad, ctx->fa_meta[slot].p, &offs));
        HIPCHK(hipMemcpyAsync(&ctx->fa_nflat_host[slot], offs + nblocks, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipEventRecord(ctx->ev_done[slot], ctx->stream));
        // the chunk before: its flattened size has long arrived; its count is queued behind this chunk's flattening
        if (prev_slot >= 0) CHK(consume(prev_slot));
        prev_slot = slot;
    }
    if (prev_slot >= 0) CHK(consume(prev_slot));
    if (!count) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        *n_out = out_total;
    }
    return KPAL_OK;
}

KPAL_API int kpal_count_feed_fasta(kpal_ctx *ctx, const uint8_t *host_buf, size_t nbytes)
{
    CTX_ENTER(ctx);
    if (!ctx->counting) return set_err(KPAL_E_STATE, "kpal_count_feed_fasta before kpal_count_begin");
    if (nbytes == 0) return KPAL_OK;
    if (!host_buf) return set_err(KPAL_E_INVALID, "host_buf is NULL");
    FaSource src;
    src.mem = host_buf;
    src.end = nbytes;
    return fasta_pipeline(ctx, src, true, nullptr, nullptr);
}

// [begin, end) of the regular file `path` (end 0: up to its end) as src's range, opened for sequential reading; the caller
// closes src.fd.
int open_text_range(const char *path, uint64_t begin, uint64_t end, FaSource &src)
{
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return set_err(KPAL_E_IO, "cannot open %s: %s", path, strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
        close(fd);
        return set_err(KPAL_E_IO, "%s is not a regular file", path);
    }
    const uint64_t size = (uint64_t)st.st_size;
    if (end == 0) end = size;
    if (begin > end || end > size) {
        close(fd);
        return set_err(KPAL_E_INVALID, "byte range %llu..%llu outside %s (%llu bytes)", (unsigned long long)begin, (unsigned long long)end, path,
                       (unsigned long long)size);
    }
    (void)posix_fadvise(fd, (off_t)begin, (off_t)(end - begin), POSIX_FADV_SEQUENTIAL);
    src.fd = fd;
    src.pos = begin;
    src.end = end;
    return KPAL_OK;
}

KPAL_API int kpal_count_feed_fasta_file(kpal_ctx *ctx, const char *path, uint64_t begin, uint64_t end, const uint8_t *prefix, size_t prefix_len)
{
    CTX_ENTER(ctx);
    if (!ctx->counting) return set_err(KPAL_E_STATE, "kpal_count_feed_fasta_file before kpal_count_begin");
    if (!path) return set_err(KPAL_E_INVALID, "path is NULL");
    if (prefix_len && !prefix) return set_err(KPAL_E_INVALID, "prefix is NULL");
    if (prefix_len > ((size_t)1 << 20)) return set_err(KPAL_E_INVALID, "prefix longer than 1 MiB");
    FaSource src;
    CHK(open_text_range(path, begin, end, src));
    src.prefix = prefix;
    src.prefix_left = prefix_len;
    const int rc = fasta_pipeline(ctx, src, true, nullptr, nullptr);
    close(src.fd);
    return rc;
}

KPAL_API int kpal_fasta_flatten(kpal_ctx *ctx, const uint8_t *host_buf, size_t nbytes, uint8_t *host_out, uint64_t *n_out)
{
    CTX_ENTER(ctx);
    if (!n_out || (nbytes && (!host_buf || !host_out))) return set_err(KPAL_E_INVALID, "NULL pointer");
    *n_out = 0;
    if (nbytes == 0) return KPAL_OK;
    FaSource src;
    src.mem = host_buf;
    src.end = nbytes;
    return fasta_pipeline(ctx, src, false, host_out, n_out);
}

// ----------------------------------------------------------------------------------------------
// FASTQ ingest: text (a byte range of a file, or host memory) -> pinned staging -> device, behind the rest of the chunk before
// that no record finished -> tokenised on the device (fastq_kernels.hpp) -> counted.  Unlike a FASTA chunk, a FASTQ chunk cannot
// tell from its own bytes where its records begin (a quality line may begin with '@'), so every chunk begins at a record: the
// status of a chunk (where its unfinished rest begins, its flattened size, its first bad record) is read back once, and the next
// chunk is tokenised behind that rest.  The count of chunk i is queued behind the tokenising of chunk i + 1, and the reader
// (StagedReader) reads chunk i + 1 while chunk i is copied and tokenised.
// ----------------------------------------------------------------------------------------------
static const char *fq_error_text(unsigned kind)
{
    switch (kind) {
    case kFqNoAt: return "the title line does not begin with '@'";
    case kFqNoPlus: return "the separator line does not begin with '+'";
    case kFqLength: return "the quality line is not as long as the sequence line";
    case kFqCutOff: return "the record is cut off at the end of the text";
    default: return "a quality byte outside the range of the quality offset";
    }
}

int fq_mask_options(const kpal_fastq_options *opt, FqMask &m)
{
    m.min_quality = opt ? opt->min_quality : -1;
    m.offset = opt ? opt->quality_offset : 33;
    if (m.offset != 33 && m.offset != 64) return set_err(KPAL_E_INVALID, "quality_offset must be 33 or 64 (got %d)", m.offset);
    if (m.min_quality > 93) return set_err(KPAL_E_INVALID, "min_quality must be at most 93 (got %d)", m.min_quality);
    if (m.min_quality < 0) m.min_quality = -1;
    return KPAL_OK;
}

// The tokenising of ONE chunk, shared by the count path (fastq_pipeline) and the record index (kpal_records.hip): raw[0, n) on
// the device, beginning at a title line, n < 4 GiB - 64 -> flat; fin: the text ends with the chunk.  Queued on the context's
// stream: the newline positions stay in fq_pos, the status words go to fq_status and from there to fq_status_host, and fq_ev is
// recorded behind that copy -- the caller waits for it (fq_tokenise_wait) when it needs the words.
int fq_tokenise(kpal_ctx *ctx, const uint8_t *raw, uint64_t n, bool fin, FqMask m, uint8_t *flat)
{
    if (!ctx->fq_status_host) {
        hipError_t e = hipHostMalloc((void **)&ctx->fq_status_host, kFqStatusWords * sizeof(unsigned long long), hipHostMallocDefault);
        if (e != hipSuccess) {
            ctx->fq_status_host = nullptr;
            return set_err(KPAL_E_NOMEM, "hipHostMalloc failed: %s", hipGetErrorString(e));
        }
    }
    if (!ctx->fq_ev) HIPCHK(hipEventCreateWithFlags(&ctx->fq_ev, hipEventDisableTiming));
    CHK(ensure(ctx, ctx->fq_status, kFqStatusWords * sizeof(unsigned long long)));
    const uint32_t nb = (uint32_t)((n + kFaBlockBytes - 1) / kFaBlockBytes);
    CHK(ensure(ctx, ctx->fq_pos, n * sizeof(uint32_t) + 64));
    CHK(ensure(ctx, ctx->fq_meta, (size_t)(nb + 1) * 16 + (size_t)nb * 8 + 64));
    uint64_t *line_offs = (uint64_t *)ctx->fq_meta.p;
    uint64_t *kept_offs = line_offs + nb + 1;
    uint32_t *nl_cnt = (uint32_t *)(kept_offs + nb + 1);
    uint32_t *kept = nl_cnt + nb;
    uint32_t *pos = (uint32_t *)ctx->fq_pos.p;
    unsigned long long *st = (unsigned long long *)ctx->fq_status.p;
    HIPCHK(hipMemsetAsync(st, 0xFF, 2 * sizeof(unsigned long long), ctx->stream));
    HIPCHK(hipMemsetAsync(st + 2, 0, (kFqStatusWords - 2) * sizeof(unsigned long long), ctx->stream));
    const unsigned rec_grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n / 4 / 256 + 1, (uint64_t)ctx->num_cu * 4));
    LAUNCH(ctx, "fq_newlines", (fa_mark_count_kernel<0>), dim3(nb), dim3(kFaThreads), raw, n, nl_cnt);
    LAUNCH(ctx, "fq_line_scan", fa_offset_kernel, dim3(1), dim3(256), (const uint32_t *)nl_cnt, nb, line_offs);
    LAUNCH(ctx, "fq_newline_pos", fq_newline_pos_kernel, dim3(nb), dim3(kFaThreads), raw, n, (const uint64_t *)line_offs, pos);
    LAUNCH(ctx, "fq_records", fq_record_kernel, dim3(rec_grid), dim3(256), raw, n, (const uint32_t *)pos, (const uint64_t *)(line_offs + nb),
           fin ? 1 : 0, st);
    LAUNCH(ctx, "fq_carry", fq_carry_kernel, dim3(1), dim3(1), (const uint32_t *)pos, (const uint64_t *)(line_offs + nb), n, st);
    LAUNCH(ctx, "fq_count", fq_count_kernel, dim3(nb), dim3(kFaThreads), raw, n, (const uint64_t *)line_offs, nb, (const uint32_t *)pos, m, st, kept);
    LAUNCH(ctx, "fq_offset", fa_offset_kernel, dim3(1), dim3(256), (const uint32_t *)kept, nb, kept_offs);
    LAUNCH(ctx, "fq_scatter", fq_scatter_kernel, dim3(nb), dim3(kFaThreads), raw, n, (const uint64_t *)line_offs, nb, (const uint32_t *)pos, m, st,
           (const uint64_t *)kept_offs, flat);
    HIPCHK(hipMemcpyAsync(ctx->fq_status_host, st, kFqStatusWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipEventRecord(ctx->fq_ev, ctx->stream));
    return KPAL_OK;
}

// ... and its status words, once they have arrived (fastq_kernels.hpp: kFqStatusWords); a malformed record is the error, numbered
// behind the `records` records of the same text that earlier chunks finished
int fq_tokenise_wait(kpal_ctx *ctx, uint64_t records, const unsigned long long **status)
{
    HIPCHK(hipEventSynchronize(ctx->fq_ev));
    const unsigned long long *hs = ctx->fq_status_host;
    if (hs[0] != ~0ull)
        return set_err(KPAL_E_INVALID, "malformed FASTQ record %llu: %s", (unsigned long long)(records + (hs[0] >> 3) + 1),
                       fq_error_text((unsigned)(hs[0] & 7)));
    *status = hs;
    return KPAL_OK;
}

// The title lines of the R records the chunk tokenised last finishes (its newline positions are still in fq_pos): their offsets
// in the chunk, R values of device memory, queued on the context's stream.
int fq_title_offsets(kpal_ctx *ctx, uint64_t R, uint64_t *dev_title)
{
    LAUNCH(ctx, "fq_title_offsets", fq_title_offsets_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), (const uint32_t *)ctx->fq_pos.p, R, dev_title);
    return KPAL_OK;
}

int fq_chunk_too_long(uint64_t records)
{
    return set_err(KPAL_E_INVALID, "FASTQ record %llu: a record (or a run of empty lines) longer than 4 GiB", (unsigned long long)records + 1);
}

// The text = carry_in, then the source.  final_text: the text ends with the source (a record still open there is cut off); else
// the unfinished rest goes to *carry_out (which may be carry_in).  records: records finished before, advanced.  count: the stream
// is counted into the running count; else it is copied to host_out (*n_out bytes).
static int fastq_pipeline(kpal_ctx *ctx, FaSource &src, const std::vector<uint8_t> &carry_in, bool final_text, FqMask m,
                          uint64_t &records, bool count, uint8_t *host_out, uint64_t *n_out, std::vector<uint8_t> *carry_out)
{
    const size_t stage = ctx->fa_chunk, pad = kpal_ctx::kStagePad;
    CHK(ensure_pinned(ctx));

    // the carried text: fq_raw[cslot][cstart, cstart + clen)
    int cslot = 1;
    uint64_t cstart = 0, clen = carry_in.size();
    if (clen) {
        CHK(ensure(ctx, ctx->fq_raw[1], clen + 64));
        HIPCHK(hipMemcpyAsync(ctx->fq_raw[1].p, carry_in.data(), clen, hipMemcpyHostToDevice, ctx->stream));
    }
    // the reader (fasta_host.hpp) reads chunk i + 1 into the other pinned buffer while chunk i is copied and tokenised
    StagedReader reader(src, (uint8_t *)ctx->pinned[0], (uint8_t *)ctx->pinned[1], stage, [ctx](int slot) { return pinned_wait(ctx, slot); });
    int pend_slot = -1;            // tokenised, not consumed yet: fq_flat[pend_slot], pend_n bytes
    uint64_t pend_n = 0, out_total = 0;
    auto consume = [&]() -> int {
        if (pend_slot < 0) return KPAL_OK;
        uint8_t *flat = (uint8_t *)ctx->fq_flat[pend_slot].p + pad;
        if (pend_n) {
            if (count) CHK(count_device_range(ctx, flat, (size_t)pend_n, 0));   // (whole records: no window crosses the seam)
            else HIPCHK(hipMemcpyAsync(host_out + out_total, flat, pend_n, hipMemcpyDeviceToHost, ctx->stream));
        }
        out_total += pend_n;
        pend_slot = -1;
        return KPAL_OK;
    };

    for (bool first = true;; first = false) {
        StagedChunk ck;   // (none: the carry alone, slot 0)
        const int got = reader.next(ck);
        if (got == -1) return set_err(KPAL_E_IO, "reading the FASTQ input failed: %s", strerror(reader.io_errno()));
        if (got < 0) return set_err(KPAL_E_HIP, "hipEventSynchronize failed while reading the FASTQ input");
        if (got == 0 && !(first && clen)) break;
        const int slot = ck.slot;
        const size_t m_bytes = ck.n;
        const bool fin = final_text && src.pos >= src.end;
        const uint64_t n = clen + m_bytes;
        if (n >= ((uint64_t)1 << 32) - 64) return fq_chunk_too_long(records);
        CHK(ensure(ctx, ctx->fq_raw[slot], n + 64));   // (never the carry's buffer: cslot != slot)
        CHK(ensure(ctx, ctx->fq_flat[slot], n + pad + 64));
        uint8_t *raw = (uint8_t *)ctx->fq_raw[slot].p;
        if (clen) HIPCHK(hipMemcpyAsync(raw, (const uint8_t *)ctx->fq_raw[cslot].p + cstart, clen, hipMemcpyDeviceToDevice, ctx->stream));
        if (m_bytes) CHK(pinned_h2d(ctx, slot, raw + clen, ck.data, m_bytes));
        CHK(fq_tokenise(ctx, raw, n, fin, m, (uint8_t *)ctx->fq_flat[slot].p + pad));
        CHK(consume());                          // the chunk before: its count runs behind this chunk's tokenising
        const unsigned long long *hs;
        CHK(fq_tokenise_wait(ctx, records, &hs));
        records += hs[2];
        cslot = slot;
        cstart = fin ? n : hs[3];
        clen = n - cstart;
        pend_slot = slot;
        pend_n = hs[4];
    }
    if (carry_out) {
        carry_out->resize((size_t)clen);
        if (clen) {
            HIPCHK(hipMemcpyAsync(carry_out->data(), (const uint8_t *)ctx->fq_raw[cslot].p + cstart, clen, hipMemcpyDeviceToHost, ctx->copy_stream));
            HIPCHK(hipStreamSynchronize(ctx->copy_stream));
        }
    }
    CHK(consume());
    if (!count) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        *n_out = out_total;
    }
    return KPAL_OK;
}

void fq_reset(kpal_ctx *ctx)
{
    ctx->fq_carry.clear();
    ctx->fq_records = 0;
    ctx->fq_open = false;
}

// One FASTQ feed of a count; a malformed record abandons the count.
static int fastq_feed(kpal_ctx *ctx, FaSource &src, const FqMask &m)
{
    ctx->fq_open = true;
    ctx->fq_mask = m;
    const int rc = fastq_pipeline(ctx, src, ctx->fq_carry, false, m, ctx->fq_records, true, nullptr, nullptr, &ctx->fq_carry);
    if (rc != KPAL_OK) {
        fq_reset(ctx);
        ctx->counting = false;
    }
    return rc;
}

// The end of the count's text (kpal_count_finish, kpal_count_balance, the kpal_comm_reduce_* calls: everything that takes the table
// for complete): the record the last FASTQ feed left unfinished is tokenised and counted, or is an error that abandons the count.
// A no-op without a FASTQ feed since kpal_count_begin (or since the last end); a FASTQ feed afterwards begins a new text.
int count_end_text(kpal_ctx *ctx)
{
    if (!ctx->fq_open) return KPAL_OK;
    int rc = KPAL_OK;
    if (!ctx->fq_carry.empty()) {
        FaSource src;
        rc = fastq_pipeline(ctx, src, ctx->fq_carry, true, ctx->fq_mask, ctx->fq_records, true, nullptr, nullptr, nullptr);
    }
    fq_reset(ctx);
    if (rc != KPAL_OK) ctx->counting = false;
    return rc;
}

KPAL_API int kpal_count_feed_fastq(kpal_ctx *ctx, const uint8_t *host_buf, size_t nbytes, const kpal_fastq_options *opt)
{
    CTX_ENTER(ctx);
    if (!ctx->counting) return set_err(KPAL_E_STATE, "kpal_count_feed_fastq before kpal_count_begin");
    FqMask m;
    CHK(fq_mask_options(opt, m));
    if (nbytes == 0) return KPAL_OK;
    if (!host_buf) return set_err(KPAL_E_INVALID, "host_buf is NULL");
    FaSource src;
    src.mem = host_buf;
    src.end = nbytes;
    return fastq_feed(ctx, src, m);
}

KPAL_API int kpal_count_feed_fastq_file(kpal_ctx *ctx, const char *path, uint64_t begin, uint64_t end, const kpal_fastq_options *opt)
{
    CTX_ENTER(ctx);
    if (!ctx->counting) return set_err(KPAL_E_STATE, "kpal_count_feed_fastq_file before kpal_count_begin");
    if (!path) return set_err(KPAL_E_INVALID, "path is NULL");
    FqMask m;
    CHK(fq_mask_options(opt, m));
    FaSource src;
    CHK(open_text_range(path, begin, end, src));
    const int rc = src.pos < src.end ? fastq_feed(ctx, src, m) : KPAL_OK;
    close(src.fd);
    return rc;
}

KPAL_API int kpal_fastq_flatten(kpal_ctx *ctx, const uint8_t *host_buf, size_t nbytes, const kpal_fastq_options *opt, uint8_t *host_out,
                                uint64_t *n_out)
{
    CTX_ENTER(ctx);
    if (!n_out || (nbytes && (!host_buf || !host_out))) return set_err(KPAL_E_INVALID, "NULL pointer");
    *n_out = 0;
    FqMask m;
    CHK(fq_mask_options(opt, m));
    if (nbytes == 0) return KPAL_OK;
    FaSource src;
    src.mem = host_buf;
    src.end = nbytes;
    const std::vector<uint8_t> none;
    uint64_t records = 0;
    return fastq_pipeline(ctx, src, none, true, m, records, false, host_out, n_out, nullptr);
}
