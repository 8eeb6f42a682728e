// record_scan_check.cpp -- AddressSanitizer / ThreadSanitizer harness of kpal_amd/csrc/record_scan.hpp, the by-record scan of a
// FASTA or FASTQ file (RecordScan: gather the carried bytes + the next bytes of the range, cut, index, carry), driven the way
// kpal_records.hip drives it -- with the cuts of the header itself (fasta_record_cut, fastq_record_cut) -- but with a malloc'ed
// staging buffer of EXACTLY the staging size (a byte written past it is an ASan finding), a temporary file, and index functions
// written here: FASTA counts the header lines of the piece, FASTQ is a sequential four-line tokeniser that says how many bytes
// its reads cover.  Staging sizes of 64, 257 and 5000 bytes; LF and CRLF; text before the first header; a record, and a read,
// longer than three staging buffers (gathered in pageable memory); a file that ends without an end of line; a range
// [begin, end) between record starts; an empty range.  What is checked: the pieces, concatenated, are the range; every
// text_offset is the running sum and tell() the next one; FASTA pieces begin at '>' (the first may begin before it) and end
// behind an end of line that precedes a '>' or at the end of the range; FASTQ pieces begin at a title line and are never
// indexed with fewer than four '\n' before the end; no piece without records is handed out; the records sum to what one pass
// over the whole text counts; after the end the scan is closed and so is its descriptor.  The reads go through fa_read with a
// split of 1 KiB, so the pool's threads (KPAL_READ_THREADS from the test) read the larger ones.  Test infrastructure; run by
// tests/test_native_sanitized.py.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

#include <fcntl.h>

#include "../../kpal_amd/csrc/record_scan.hpp"

using namespace kpal;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static int failures = 0;
#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            if (++failures <= 20) std::printf("line %d: %s -- %s\n", __LINE__, #cond, what.c_str()); \
        }                                                                              \
    } while (0)

struct Text {
    std::string text;
    std::vector<size_t> starts;   // where every record begins: its header / title line
};

// `records` FASTA records, number `long_at` of `long_len` bases; '>' inside titles and inside sequence lines (never at a line start)
static Text make_fasta(size_t records, size_t long_at, size_t long_len, const char *eol, bool junk, bool final_eol)
{
    Text t;
    if (junk) t.text += std::string("text before the first header") + eol + "ACGT>ACGT" + eol;
    for (size_t r = 0; r < records; ++r) {
        t.starts.push_back(t.text.size());
        t.text += ">rec" + std::to_string(r) + (rnd() & 1 ? " a > in the title" : "") + eol;
        const size_t len = r == long_at ? long_len : (size_t)(rnd() % 200);
        const size_t width = r == long_at && (rnd() & 1) ? len : 60;
        for (size_t i = 0; i < len; ++i) {
            t.text.push_back(i % width != 0 && rnd() % 50 == 0 ? '>' : "ACGTN"[rnd() % 5]);
            if ((i + 1) % width == 0 || i + 1 == len) t.text += eol;
        }
    }
    if (!final_eol)
        while (!t.text.empty() && fa_host_is_eol((uint8_t)t.text.back())) t.text.pop_back();
    return t;
}

// `reads` FASTQ reads, number `long_at` of `long_len` bases; quality lines over the whole range ('@', '+' and '>' at their start too)
static Text make_fastq(size_t reads, size_t long_at, size_t long_len, const char *eol, bool final_eol)
{
    Text t;
    for (size_t r = 0; r < reads; ++r) {
        t.starts.push_back(t.text.size());
        const size_t len = r == long_at ? long_len : (size_t)(rnd() % 120);
        t.text += "@read" + std::to_string(r) + eol;
        for (size_t i = 0; i < len; ++i) t.text.push_back("ACGTN"[rnd() % 5]);
        t.text += eol;
        t.text += rnd() & 1 ? "+" : "+read" + std::to_string(r);
        t.text += eol;
        for (size_t i = 0; i < len; ++i) t.text.push_back((char)(33 + (i == 0 && (rnd() & 1) ? '@' - 33 : rnd() % 94)));
        t.text += eol;
    }
    if (!final_eol) t.text.resize(t.text.size() - std::strlen(eol));
    return t;
}

// the records of text[b, e), in one pass over it: header lines ('>' at a line start) / four lines to a read
static uint64_t count_fasta(const std::string &s, size_t b, size_t e)
{
    uint64_t n = 0;
    for (size_t i = b; i < e; ++i)
        if (s[i] == '>' && (i == b || fa_host_is_eol((uint8_t)s[i - 1]))) ++n;
    return n;
}

static uint64_t count_fastq(const std::string &s, size_t b, size_t e)
{
    uint64_t lines = 0;
    for (size_t i = b; i < e; ++i)
        if (s[i] == '\n') ++lines;
    if (e > b && s[e - 1] != '\n') ++lines;
    if (lines % 4) ++failures;   // (the generator's own mistake)
    return lines / 4;
}

static size_t cases = 0;

// one scan of text[begin, end) of the file at `path` with a staging buffer of `stage` bytes
static void scan(const char *path, const Text &t, size_t begin, size_t end, size_t stage, bool fastq, const std::string &what)
{
    ++cases;
    const std::string &text = t.text;
    const std::set<size_t> starts(t.starts.begin(), t.starts.end());
    FaSource src;
    src.fd = open(path, O_RDONLY);
    src.pos = begin;
    src.end = end;
    const int fd = src.fd;
    EXPECT(fd >= 0);
    if (fd < 0) return;
    uint8_t *const stage_buf = (uint8_t *)malloc(stage);   // exactly `stage` bytes
    std::string seen;              // what the index calls covered, one behind the other
    size_t at = begin;             // the running sum: where the next covered byte lies in the file
    size_t last_at = begin;        // ... and where the piece covered last began
    int waits = 0, indexes = 0;
    bool waited = false, outside = false;

    const RecordScan::Wait wait = [&]() {
        ++waits;
        waited = true;
        return 0;
    };
    // what both formats share: the piece is text[at, at + n), in the staging buffer or outside it, at_end exactly at the end
    auto common = [&](const uint8_t *piece, size_t n, bool in_stage, bool at_end) {
        ++indexes;
        EXPECT(n > 0 && at + n <= end && text.compare(at, n, (const char *)piece, n) == 0);
        EXPECT(at_end == (at + n == end));
        if (in_stage) EXPECT(piece == stage_buf && n <= stage && waited);
        else EXPECT(n >= stage && piece != stage_buf);
        outside |= !in_stage;
        waited = false;
    };
    auto covered = [&](const uint8_t *piece, size_t used) {
        if (used == 0) return;
        seen.append((const char *)piece, used);
        last_at = at;
        at += used;
    };
    const RecordScan::Index fasta_index = [&](const uint8_t *piece, size_t n, bool in_stage, bool at_end, uint64_t *records, size_t *used) {
        common(piece, n, in_stage, at_end);
        EXPECT(piece[0] == '>' || at == begin);
        EXPECT(fa_host_is_eol(piece[n - 1]) ? (at + n == end || text[at + n] == '>') : at + n == end);
        *records = count_fasta(text, at, at + n);
        *used = n;
        covered(piece, n);
        return 0;
    };
    const RecordScan::Index fastq_index = [&](const uint8_t *piece, size_t n, bool in_stage, bool at_end, uint64_t *records, size_t *used) {
        common(piece, n, in_stage, at_end);
        EXPECT(starts.count(at) == 1 && piece[0] == '@');
        // four line ends to a read, one after the other; at the end of the text the last line needs none
        size_t lines = 0, done = 0;
        for (size_t i = 0; i < n; ++i)
            if (piece[i] == '\n' && ++lines % 4 == 0) done = i + 1;
        EXPECT(lines >= 4 || at_end);
        *records = lines / 4;
        if (at_end && piece[n - 1] != '\n' && ++lines % 4 == 0) ++*records;
        *used = at_end ? 0 : done;   // (at the end the scan takes the whole piece whatever this says)
        covered(piece, at_end ? n : done);
        return 0;
    };

    RecordScan rs;
    EXPECT(!rs.is_open());
    rs.open(src, 1024);
    EXPECT(rs.is_open() && rs.tell() == begin);
    uint64_t records = 0;
    size_t pieces = 0;
    for (;;) {
        ScanPiece piece;
        const size_t told = (size_t)rs.tell();
        const int got = rs.next(stage_buf, stage, wait, fastq ? fastq_record_cut : fasta_record_cut,
                                fastq ? fastq_index : fasta_index, piece);
        if (got != 1) {
            EXPECT(got == 0);
            break;
        }
        ++pieces;
        EXPECT(piece.records > 0);
        EXPECT(piece.text_offset == last_at && rs.tell() == at);
        // the piece begins where the scan said it stood, unless a piece without records (text before the first header) lay between
        EXPECT(piece.text_offset == told || (!fastq && told == begin && count_fasta(text, begin, piece.text_offset) == 0));
        records += piece.records;
        if (pieces > text.size() + 2) {   // (a scan that does not advance)
            EXPECT(false);
            break;
        }
    }
    EXPECT(!rs.is_open());
    EXPECT(fcntl(fd, F_GETFD) == -1 && errno == EBADF);
    EXPECT(seen == text.substr(begin, end - begin) && at == end);
    EXPECT(records == (fastq ? count_fastq(text, begin, end) : count_fasta(text, begin, end)));
    // a record longer than the staging buffer has been gathered, and indexed, outside it
    size_t longest = 0;
    for (size_t r = 0; r < t.starts.size(); ++r)
        if (t.starts[r] >= begin && t.starts[r] < end) longest = std::max(longest, std::min(r + 1 < t.starts.size() ? t.starts[r + 1] : text.size(), end) - t.starts[r]);
    EXPECT(outside == (longest > stage));
    if (begin == end) EXPECT(pieces == 0 && indexes == 0 && waits == 0);
    {   // a call after the end: still the end
        ScanPiece piece;
        EXPECT(rs.next(stage_buf, stage, wait, fasta_record_cut, fasta_index, piece) == 0);
    }
    free(stage_buf);
}

int main()
{
    char path[] = "/tmp/kpal_record_scan_check_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) {
        perror("mkstemp");
        return 2;
    }
    const size_t stages[] = {64, 257, 5000};
    for (int round = 0; round < 8; ++round) {
        const char *eol = round & 1 ? "\r\n" : "\n";
        const bool final_eol = (round & 2) == 0, junk = (round & 4) != 0;
        for (int fastq = 0; fastq < 2; ++fastq) {
            // the long record: more than three times the largest staging buffer, in the middle or at the very end
            const size_t n = 40, long_at = round % 3 == 0 ? n - 1 : 17, long_len = 16000 + (size_t)(rnd() % 3000);
            const Text t = fastq ? make_fastq(n, long_at, long_len / 2, eol, final_eol) : make_fasta(n, long_at, long_len, eol, junk, final_eol);
            if (pwrite(fd, t.text.data(), t.text.size(), 0) != (ssize_t)t.text.size() || ftruncate(fd, (off_t)t.text.size()) != 0) {
                perror("pwrite");
                return 2;
            }
            for (size_t stage : stages) {
                const std::string what = std::string(fastq ? "FASTQ" : "FASTA") + " round " + std::to_string(round) + " stage " + std::to_string(stage);
                scan(path, t, 0, t.text.size(), stage, fastq != 0, what + " whole");
                scan(path, t, t.starts[3], t.starts[30], stage, fastq != 0, what + " range with the long record");
                scan(path, t, t.starts[20], t.starts[21], stage, fastq != 0, what + " one record");
                scan(path, t, t.starts[5], t.starts[5], stage, fastq != 0, what + " empty range");
                scan(path, t, t.text.size(), t.text.size(), stage, fastq != 0, what + " empty range at the end");
            }
        }
    }
    // a file of text without any header: one piece, no record, nothing handed out; an empty file
    {
        Text none;
        none.text = "no header at all\nACGT\n";
        if (pwrite(fd, none.text.data(), none.text.size(), 0) != (ssize_t)none.text.size() || ftruncate(fd, (off_t)none.text.size()) != 0) return 2;
        for (size_t stage : stages) scan(path, none, 0, none.text.size(), stage, false, "no header, stage " + std::to_string(stage));
        if (ftruncate(fd, 0) != 0) return 2;
        none.text.clear();
        scan(path, none, 0, 0, 64, false, "empty file");
        scan(path, none, 0, 0, 64, true, "empty file");
    }
    // a read error is -1 with the errno, and leaves the scan open: a range beyond the end of the file
    {
        const std::string what = "read error";
        FaSource bad;
        bad.fd = open(path, O_RDONLY);
        bad.end = (uint64_t)1 << 40;
        uint8_t *buf = (uint8_t *)malloc(4096);
        RecordScan rs;
        rs.open(bad, 1024);
        ScanPiece piece;
        const int got = rs.next(buf, 4096, [] { return 0; }, fasta_record_cut,
                                [](const uint8_t *, size_t n, bool, bool, uint64_t *records, size_t *used) {
                                    *records = 1;
                                    *used = n;
                                    return 0;
                                }, piece);
        EXPECT(got == -1 && rs.io_errno() != 0 && rs.is_open());
        // ... and an index that fails is -2 with its code (the destructor closes the descriptor)
        RecordScan rs2;
        FaSource one;
        one.fd = open(path, O_RDONLY);
        if (pwrite(fd, ">a\nAC\n", 6, 0) != 6) return 2;
        one.end = 6;
        rs2.open(one);
        const int got2 = rs2.next(buf, 4096, [] { return 0; }, fasta_record_cut,
                                  [](const uint8_t *, size_t, bool, bool, uint64_t *, size_t *) { return -7; }, piece);
        EXPECT(got2 == -2 && rs2.user_error() == -7);
        RecordScan rs3;
        one.fd = open(path, O_RDONLY);
        rs3.open(one);
        EXPECT(rs3.next(buf, 4096, [] { return -9; }, fasta_record_cut, nullptr, piece) == -2 && rs3.user_error() == -9);
        free(buf);
        cases += 3;
    }
    close(fd);
    unlink(path);
    if (failures) {
        std::printf("record_scan_check: %d failure(s) in %zu cases\n", failures, cases);
        return 1;
    }
    std::printf("record_scan_check: %zu cases, pool of %d\nSANITIZE_OK\n", cases, HostPool::instance().size());
    return 0;
}
