// fastq_kernels.hpp -- FASTQ text -> flat sequence stream on the device (gfx950).
//
// The reference reads FASTA only; this is the sibling of fasta_kernels.hpp for four-line FASTQ, the format reads come off a
// sequencer in.  Output is the same flat stream the counting kernels consume: every record contributes '\n' + its sequence line.
//
// Rules (kpal_hip.h, kpal_count_feed_fastq):
//   * a record is four lines: title ('@...'), sequence, separator ('+...'), quality; lines end at '\n', a '\r' just before the
//     '\n' is dropped; the role of a line follows from its index mod 4 only (a quality line may begin with '@' or '+');
//   * sequence bytes are taken verbatim; with the mask on (min_quality >= 0) base c becomes 'N' when qual[c] - offset <
//     min_quality, and a quality byte outside [offset, '~'] is malformed;
//   * len(quality) == len(sequence); a record cut off at the end of the text is malformed; empty lines at the very end are not
//     a record.
// A chunk handed to these kernels always begins at a record's title line (the host carries an unfinished record into the next
// chunk).  The passes: newlines per 4 KiB block (fa_mark_count_kernel<0>), their scan (fa_offset_kernel), their positions
// (fq_newline_pos_kernel) -> line bounds; one thread per record validates it (fq_record_kernel: errors, blank records, how many
// records this chunk finishes); fq_carry_kernel says where the unfinished rest begins; kept bytes per block (fq_count_kernel, which
// also checks the quality bytes under the mask), their scan (fa_offset_kernel) and the scatter (fq_scatter_kernel, staged through
// LDS so the output is written with contiguous stores).  Byte c of a sequence line reads byte c of its quality line, so every pass
// is parallel over bytes or records.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fasta_kernels.hpp"
#include "fastq_mask.hpp"

namespace kpal {

// Error word of a chunk: (record << 3) | kind, the smallest wins (atomicMin) -- the first bad record and, for it, the first kind.
enum FqErrorKind : uint32_t { kFqNoAt = 1, kFqNoPlus = 2, kFqLength = 3, kFqCutOff = 4, kFqQuality = 5 };

// Status words of one chunk (device, read back once per chunk):
//   [0] error word (~0: none)          [1] first blank record (four empty lines; ~0: none)
//   [2] 1 + last non-blank record (0: none): the records the chunk finishes    [3] byte where the carried rest begins
//   [4] flattened bytes (copied from the kept-byte scan)
constexpr int kFqStatusWords = 8;

// Bounds of line `li` of a chunk: [s, e), the '\r' before its '\n' dropped.  Line T (T = newlines in the chunk) is the text
// after the last '\n'; there is none beyond it.
__device__ __forceinline__ void fq_line(const uint8_t *__restrict__ in, uint64_t n, const uint32_t *__restrict__ pos, uint64_t T, uint64_t li,
                                        uint64_t &s, uint64_t &e)
{
    s = li == 0 ? 0 : (uint64_t)pos[li - 1] + 1;
    if (li < T) {
        e = pos[li];
        if (e > s && in[e - 1] == '\r') --e;
    } else {
        e = n;
    }
}

// Positions of the newlines of the chunk in order (32-bit: the host keeps a chunk below 4 GiB); offs = fa_offset_kernel over
// fa_mark_count_kernel<0>.
__global__ __launch_bounds__(kFaThreads) void fq_newline_pos_kernel(const uint8_t *__restrict__ in, uint64_t n, const uint64_t *__restrict__ offs,
                                                                    uint32_t *__restrict__ pos)
{
    __shared__ uint32_t wsum[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kFaBlockBytes + (uint64_t)threadIdx.x * kFaPerThread;
    uint32_t mask = 0;
    for (int j = 0; j < kFaPerThread; ++j)
        if (i0 + j < n && in[i0 + j] == '\n') mask |= 1u << j;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t c = __popc(mask);
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint64_t at = offs[blockIdx.x] + (incl - c);
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (w < wave) at += wsum[w];
    for (int j = 0; j < kFaPerThread; ++j)
        if (mask & (1u << j)) pos[at++] = (uint32_t)(i0 + (uint64_t)j);
}

// One thread per candidate record (grid-stride).  final: the chunk ends the text -- line T exists (possibly empty) and a record
// may be partial; otherwise only the records whose four lines all end inside the chunk are looked at.
__global__ __launch_bounds__(256) void fq_record_kernel(const uint8_t *__restrict__ in, uint64_t n, const uint32_t *__restrict__ pos,
                                                        const uint64_t *__restrict__ line_total, int final_chunk,
                                                        unsigned long long *__restrict__ status)
{
    const uint64_t T = *line_total;
    const uint64_t lines = final_chunk ? T + 1 : T;
    const uint64_t nrec = final_chunk ? (lines + 3) / 4 : lines / 4;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nrec; r += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t s[4], e[4];
        bool blank = true;
        int present = 0;
        for (int j = 0; j < 4; ++j) {
            const uint64_t li = 4 * r + j;
            if (li >= lines) break;
            fq_line(in, n, pos, T, li, s[j], e[j]);
            if (e[j] > s[j]) blank = false;
            ++present;
        }
        if (blank) {
            atomicMin(&status[1], (unsigned long long)r);
            continue;
        }
        atomicMax(&status[2], (unsigned long long)(r + 1));
        uint32_t kind = 0;
        if (e[0] == s[0] || in[s[0]] != '@') kind = kFqNoAt;
        else if (present < 4) kind = kFqCutOff;
        else if (e[2] == s[2] || in[s[2]] != '+') kind = kFqNoPlus;
        else if (e[3] - s[3] != e[1] - s[1]) kind = kFqLength;
        if (kind) atomicMin(&status[0], ((unsigned long long)r << 3) | kind);
    }
}

// One thread: where the rest the chunk does not finish begins (the title line of record status[2]).  A blank record before the
// last non-blank one is a record without its '@'.
// (Line 4R - 1 may be missing at the end of the text: then the record is cut off and nothing is carried.)
__global__ void fq_carry_kernel(const uint32_t *__restrict__ pos, const uint64_t *__restrict__ line_total, uint64_t n,
                                unsigned long long *__restrict__ status)
{
    const unsigned long long R = status[2];
    status[3] = R == 0 ? 0 : 4 * R - 1 < *line_total ? (unsigned long long)pos[4 * R - 1] + 1 : n;
    if (status[1] < R) status[0] = min(status[0], (status[1] << 3) | kFqNoAt);
}

// ---- record index (Profile.from_fastq_by_record / _by_window: one profile per read, per window of a read) ----
// Title offsets: for each of the R records the chunk finishes, the byte of the chunk its title line begins at -- the start of
// line 4r, the counterpart of the FASTA index's header offsets (the host reads the read's name there and nowhere else).  One
// thread per record; pos[4r - 1] exists for every r < R (record R - 1 is not blank, so line 4R - 4 begins inside the chunk).
//
// The other half of the index, the records' starts in the flattened stream, is NOT derived from these line bounds: the host
// compacts the '\n' bytes of the stream itself (fa_mark_count_kernel<0> / fa_offset_kernel / fa_mark_scatter_kernel<0>, as the
// FASTA index does).  fq_scatter_kernel writes exactly one '\n' per record it keeps and none inside a sequence line, so the r-th
// '\n' IS where record r starts, whatever the scatter decided about a '\r' at a line's end -- a scan of line lengths would have to
// restate that rule and could disagree with it -- and the number of '\n' bytes checks the record count of the status words
// against what was really written.  It costs one more read of the stream, at most half the text, in HBM.
__global__ __launch_bounds__(256) void fq_title_offsets_kernel(const uint32_t *__restrict__ pos, uint64_t R, uint64_t *__restrict__ title)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) title[r] = r == 0 ? 0 : (uint64_t)pos[4 * r - 1] + 1;
}

// Exclusive sum of one value per thread over the 256-thread workgroup (plus `seed`).
__device__ __forceinline__ uint64_t fq_block_exclusive_sum(uint32_t v, uint64_t seed, uint32_t *sh /* [4] */)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    uint64_t before = seed + (incl - v);
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (w < wave) before += sh[w];
    __syncthreads();
    return before;
}

// Classify the thread's 16 bytes: bit j of `keep` set iff byte j is emitted, out[j] its value.  line0: the line byte i0 is in.
// err != nullptr: report quality bytes outside [offset, '~'] under the mask (the first pass does, the scatter does not).
__device__ __forceinline__ void fq_classify(const uint8_t *__restrict__ in, uint64_t n, uint64_t i0, uint64_t line0,
                                            const uint32_t *__restrict__ pos, uint64_t T, uint64_t R, FqMask m,
                                            unsigned long long *err, uint32_t &keep, uint8_t (&out)[kFaPerThread])
{
    keep = 0;
    uint64_t li = line0;
    bool known = false, active = false;
    int role = 0;
    uint64_t s = 0, e = 0, qs = 0, qe = 0;
    for (int j = 0; j < kFaPerThread; ++j) {
        const uint64_t i = i0 + j;
        if (i >= n) break;
        const uint8_t c = in[i];
        if (!known) {
            known = true;
            role = (int)(li & 3);
            active = (li >> 2) < R && role < 2;
            if (active) {
                fq_line(in, n, pos, T, li, s, e);
                if (role == 1 && m.min_quality >= 0) {
                    if (li + 2 <= T) fq_line(in, n, pos, T, li + 2, qs, qe);
                    else qs = qe = n;   // (a record cut off: an error the record pass reports)
                }
            }
        }
        if (active) {
            if (role == 0) {
                if (i == s) {
                    keep |= 1u << j;
                    out[j] = '\n';
                }
            } else if (i < e) {
                uint8_t v = c;
                if (m.min_quality >= 0) {
                    const uint64_t q = qs + (i - s);
                    if (q < qe) {
                        const int qc = in[q];
                        if (qc < m.offset || qc > '~') {
                            if (err) atomicMin(err, ((unsigned long long)(li >> 2) << 3) | kFqQuality);
                        } else if (qc - m.offset < m.min_quality) {
                            v = 'N';
                        }
                    }
                }
                keep |= 1u << j;
                out[j] = v;
            }
        }
        if (c == '\n') {
            ++li;
            known = false;
        }
    }
}

// Newlines among the thread's 16 bytes, and the line its first byte is in.
__device__ __forceinline__ uint64_t fq_thread_line(const uint8_t *__restrict__ in, uint64_t n, uint64_t i0, uint64_t block_line, uint32_t *sh)
{
    uint32_t nl = 0;
    for (int j = 0; j < kFaPerThread; ++j)
        if (i0 + j < n && in[i0 + j] == '\n') ++nl;
    return fq_block_exclusive_sum(nl, block_line, sh);
}

// Kept bytes per block.  line_offs: fa_offset_kernel over the newline counts (line of each block's first byte; [nblocks] = T).
__global__ __launch_bounds__(kFaThreads) void fq_count_kernel(const uint8_t *__restrict__ in, uint64_t n, const uint64_t *__restrict__ line_offs,
                                                              uint32_t nblocks, const uint32_t *__restrict__ pos, FqMask m,
                                                              unsigned long long *__restrict__ status, uint32_t *__restrict__ kept)
{
    __shared__ uint32_t sh[4];
    __shared__ uint32_t shc[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kFaBlockBytes + (uint64_t)threadIdx.x * kFaPerThread;
    const uint64_t line0 = fq_thread_line(in, n, i0, line_offs[blockIdx.x], sh);
    uint32_t keep;
    uint8_t out[kFaPerThread];
    fq_classify(in, n, i0, line0, pos, line_offs[nblocks], status[2], m, &status[0], keep, out);
    uint32_t c = __popc(keep);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63) == 0) shc[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) kept[blockIdx.x] = shc[0] + shc[1] + shc[2] + shc[3];
}

// Write the kept bytes of each block contiguously at offs[block].
__global__ __launch_bounds__(kFaThreads) void fq_scatter_kernel(const uint8_t *__restrict__ in, uint64_t n, const uint64_t *__restrict__ line_offs,
                                                                uint32_t nblocks, const uint32_t *__restrict__ pos, FqMask m,
                                                                unsigned long long *__restrict__ status, const uint64_t *__restrict__ offs,
                                                                uint8_t *__restrict__ flat)
{
    __shared__ uint32_t sh[4];
    __shared__ uint32_t wsum[4];
    __shared__ uint8_t stage[kFaBlockBytes];
    const uint64_t i0 = (uint64_t)blockIdx.x * kFaBlockBytes + (uint64_t)threadIdx.x * kFaPerThread;
    const uint64_t line0 = fq_thread_line(in, n, i0, line_offs[blockIdx.x], sh);
    uint32_t keep;
    uint8_t out[kFaPerThread];
    fq_classify(in, n, i0, line0, pos, line_offs[nblocks], status[2], m, nullptr, keep, out);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t c = __popc(keep);
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t at = incl - c;
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (w < wave) at += wsum[w];
    const uint32_t total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    for (int j = 0; j < kFaPerThread; ++j)
        if (keep & (1u << j)) stage[at++] = out[j];
    __syncthreads();
    uint8_t *dst = flat + offs[blockIdx.x];
    for (uint32_t t = threadIdx.x; t < total; t += kFaThreads) dst[t] = stage[t];
    if (blockIdx.x == 0 && threadIdx.x == 0) status[4] = offs[nblocks];
}

}  // namespace kpal
