// record_scan.hpp -- the by-record scan of a FASTA or FASTQ file, free of HIP like fasta_host.hpp, whose source and reader it
// uses: RecordScan hands a byte range of a file out in pieces of WHOLE records.  One loop serves both formats: gather the bytes
// carried from the piece before + the next bytes of the range into the caller's staging buffer, let the format say where to
// cut, let the caller index the cut, carry what the index did not cover.  Bytes that finish no record are gathered further --
// in the staging buffer while they fit, in pageable memory, one staging size per round, once they do not (a record longer than
// the buffer).  kpal_records.hip drives it with the pinned staging buffer and the device index of either format;
// tests/native/record_scan_check.cpp drives it with a malloc'ed buffer and host tokenisers under AddressSanitizer /
// ThreadSanitizer and compares the pieces with the file.
#pragma once
#include "fasta_host.hpp"

namespace kpal {

// index of the end-of-line byte before the LAST header line of buf[0, n) that begins at or after `from` (a '>' behind an
// end of line), or n when there is none
static inline size_t fasta_last_boundary(const uint8_t *buf, size_t n, size_t from)
{
    size_t i = n;
    while (i > from + 1) {
        const void *p = memrchr(buf + from + 1, '>', i - from - 1);
        if (!p) break;
        const size_t at = (size_t)((const uint8_t *)p - buf);
        if (fa_host_is_eol(buf[at - 1])) return at - 1;
        i = at;
    }
    return n;
}

// whether buf[0, n) holds the four line ends a FASTQ record needs
static inline bool fastq_four_line_ends(const uint8_t *buf, size_t n)
{
    const uint8_t *p = buf, *const end = buf + n;
    for (int i = 0; i < 4; ++i) {
        p = (const uint8_t *)memchr(p, '\n', (size_t)(end - p));
        if (!p) return false;
        ++p;
    }
    return true;
}

// The cut of either format (RecordScan::Cut): how many bytes of buf[0, n) -- its first `carried` bytes have been looked at
// before -- to index now; 0: nothing yet, keep gathering.  The text that reaches the end of the range is indexed whole.
// FASTA is cut on the host: whole records end with the end of line before the last header line, which is searched in the new
// bytes only (a boundary is two bytes: from carried - 1 on).
static inline size_t fasta_record_cut(const uint8_t *buf, size_t n, size_t carried, bool at_end)
{
    if (at_end) return n;
    const size_t eol = fasta_last_boundary(buf, n, carried ? carried - 1 : 0);
    return eol < n ? eol + 1 : 0;
}

// FASTQ cannot be cut on the host (a quality line may begin with '@'): the text is tokenised as it is, and the tokeniser says
// where the reads it finishes end -- but not before the text holds the four line ends a read needs.
static inline size_t fastq_record_cut(const uint8_t *buf, size_t n, size_t, bool at_end) { return at_end || fastq_four_line_ends(buf, n) ? n : 0; }

struct ScanPiece {
    uint64_t records = 0;       // > 0: a piece without records is never handed out
    uint64_t text_offset = 0;   // file offset of the piece's first byte
};

class RecordScan {
public:
    using Wait = std::function<int()>;
    using Cut = size_t (*)(const uint8_t *buf, size_t n, size_t carried, bool at_end);   // fasta_record_cut, fastq_record_cut
    // Index piece[0, n): -> 0, *records and *used, the bytes those records cover (FASTA: n; FASTQ: what the tokeniser says,
    // possibly 0), or an error code that ends the call.  in_stage: the piece lies in the staging buffer (else in pageable
    // memory).  at_end: the text ends with the piece, which is then covered whole whatever *used says.  The buffer stays the
    // scan's when the function has returned: what the records do not cover is carried out of it.
    using Index = std::function<int(const uint8_t *piece, size_t n, bool in_stage, bool at_end, uint64_t *records, size_t *used)>;

    RecordScan() = default;
    ~RecordScan() { close(); }
    RecordScan(const RecordScan &) = delete;
    RecordScan &operator=(const RecordScan &) = delete;

    // the range [src.pos, src.end) of src.fd, whose descriptor the scan owns from now on (an open scan is closed first).
    // split: see fa_copy_start (tests make it tiny)
    void open(const FaSource &src, size_t split = (size_t)4 << 20)
    {
        close();
        src_ = src;
        split_ = split;
        piece_at_ = src.pos;
        open_ = true;
    }
    void close()
    {
        if (open_ && src_.fd >= 0) ::close(src_.fd);
        src_ = FaSource();
        piece_at_ = 0;
        open_ = false;
        carry_.clear();
        carry_.shrink_to_fit();
    }
    bool is_open() const { return open_; }
    uint64_t tell() const { return piece_at_; }      // file offset of the first byte that no piece has covered
    int io_errno() const { return io_errno_; }       // after next() returned -1
    int user_error() const { return user_error_; }   // after next() returned -2: what wait or index returned

    // 1: `out` is the next piece with records, indexed by `index`; 0: the end of the range -- the scan is closed; -1: a read
    // failed (io_errno()); -2: wait or index failed (user_error()).  stage_buf: `stage` bytes; wait() is called before they
    // are written: it returns 0 once whatever the caller queued on their previous contents is done.  `cut` and `index` are
    // not called while the other's answer makes them pointless: no index without a cut, so none (no device call) while a
    // FASTA text has no boundary or a FASTQ text fewer than four line ends.
    int next(uint8_t *stage_buf, size_t stage, const Wait &wait, Cut cut, const Index &index, ScanPiece &out)
    {
        for (;;) {
            if (!open_ || (carry_.empty() && src_.pos >= src_.end)) {   // the end
                close();
                return 0;
            }
            const size_t c = carry_.size();
            const bool fits = c < stage;
            const size_t want = (size_t)std::min<uint64_t>(fits ? stage - c : stage, src_.end - src_.pos);
            uint8_t *buf;
            if (fits) {   // the carried bytes + the next bytes of the range into the staging buffer
                if (int rc = wait()) return fail(rc);
                buf = stage_buf;
                if (c) memcpy(buf, carry_.data(), c);
            } else {      // a record longer than the staging buffer: gathered in pageable memory, one staging size at a time
                carry_.resize(c + want);
                buf = carry_.data();
            }
            if (want) {
                if (int e = fa_read(src_, buf + c, src_.pos, want, split_)) {
                    if (!fits) carry_.resize(c);
                    io_errno_ = e;
                    return -1;
                }
                src_.pos += want;
            }
            const size_t n = c + want;
            const bool at_end = src_.pos >= src_.end;
            const size_t piece = cut(buf, n, c, at_end);
            uint64_t records = 0;
            size_t used = 0;
            if (piece)
                if (int rc = index(buf, piece, fits, at_end, &records, &used)) return fail(rc);
            if (at_end) used = n;          // the piece that reaches the end of the range is final
            if (used == 0) {               // no record ends in this text: keep gathering
                if (fits) carry_.assign(buf, buf + n);
                continue;
            }
            // the unfinished record behind the piece is carried (`index` is done with the buffer)
            std::vector<uint8_t> tail(buf + used, buf + n);
            carry_.swap(tail);
            out.records = records;
            out.text_offset = piece_at_;
            piece_at_ += used;
            if (records == 0) continue;    // text before the first header, empty lines at the end: the next piece
            return 1;
        }
    }

private:
    int fail(int rc)
    {
        user_error_ = rc;
        return -2;
    }

    FaSource src_;
    size_t split_ = (size_t)4 << 20;
    bool open_ = false;
    uint64_t piece_at_ = 0;
    std::vector<uint8_t> carry_;   // the unfinished record behind the last piece
    int io_errno_ = 0, user_error_ = 0;
};

}  // namespace kpal
