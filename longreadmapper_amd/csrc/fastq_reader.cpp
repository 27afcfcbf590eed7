// fastq_reader.cpp -- FASTA / FASTQ batches (lrm_reader_*, include/lrm_io_host.h): a pool of large host blocks, the
// buffered byte source, the parallel 4-line FASTQ parser and the general parser behind it.  Host-side C++.
#include <zlib.h>
#include <fcntl.h>
#include <unistd.h>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>
#include "../../include/lrm_io_host.h"
#include "lrm_internal.h"

// ------------------------------------------------------------------------------------------
// FASTA / FASTQ batches (reads_load + refactor_reads_seq, accaln.c:45-58, alnmain.c:87-103)
//
// Two parsers over one buffered byte source:
//   fast   4-line FASTQ records (what every long-read basecaller writes): the buffered block is cut at arbitrary byte
//          offsets into one piece per host thread, every piece resynchronises to a record boundary (a line that starts
//          with '@' whose line-after-next starts with '+': a quality line may start with '@', but then the line after
//          next is a sequence, and a sequence never starts with '+'), the pieces are indexed in parallel and the
//          sequences / names / qualities are copied into the dense batch in parallel.  Plain files are read with
//          parallel preads, gzip streams are inflated by zlib (one thread) into the same buffer.
//   slow   the general kseq-like parser (multi-line records, FASTA, CR LF): taken for the rest of the file as soon as
//          the fast parser meets a record that is not four LF-terminated lines.
//
// Both hand their records to batch_fill, which builds the batch: one allocation rule, one layout.
// ------------------------------------------------------------------------------------------
// Large host buffers (the reader's block, a batch's sequences and its name / quality arenas) are recycled through a small
// pool instead of going back to the allocator: a freed gigabyte is unmapped by malloc and the next batch pays for its
// page faults again -- with every thread of a copy loop faulting on one address space that is seconds per gigabyte on
// some kernels (tools/io_probe.py: 0.4 GB/s the first time, 7-25 GB/s on warm pages).
namespace bigmem {
struct Hdr { size_t cap; size_t pad[7]; };
static_assert(sizeof(Hdr) == 64, "header keeps the payload 64-byte aligned");
std::mutex mu;
std::vector<Hdr *> pool;                 // free blocks (at most 12, largest kept)
void *alloc(size_t n) {
    if (n == 0) n = 1;
    {
        std::lock_guard<std::mutex> g(mu);
        size_t best = pool.size();
        for (size_t i = 0; i < pool.size(); ++i)
            if (pool[i]->cap >= n && pool[i]->cap <= 2 * n + (1u << 20) && (best == pool.size() || pool[i]->cap < pool[best]->cap)) best = i;
        if (best != pool.size()) { Hdr *h = pool[best]; pool.erase(pool.begin() + (long) best); return h + 1; }
    }
    const size_t cap = n + n / 8;
    Hdr *h = (Hdr *) malloc(sizeof(Hdr) + cap);
    if (!h) return nullptr;
    h->cap = cap;
    return h + 1;
}
size_t capacity(void *p) { return p ? ((Hdr *) p - 1)->cap : 0; }
void release(void *p) {
    if (!p) return;
    Hdr *h = (Hdr *) p - 1;
    Hdr *drop = nullptr;
    {
        std::lock_guard<std::mutex> g(mu);
        pool.push_back(h);
        if (pool.size() > 12) {                                    // too many: the smallest goes back to the allocator
            size_t sm = 0;
            for (size_t i = 1; i < pool.size(); ++i) if (pool[i]->cap < pool[sm]->cap) sm = i;
            drop = pool[sm];
            pool.erase(pool.begin() + (long) sm);
        }
    }
    free(drop);
}
}  // namespace bigmem

struct lrm_reader {
    gzFile fp = nullptr;
    int fd = -1;             // plain file: read with pread (fp is null then)
    uint64_t file_off = 0;
    struct RawBuf {          // grows without initialising (a std::vector would clear every gigabyte it grows by)
        char *p = nullptr; size_t cap = 0;
        char *data() { return p; }
        const char *data() const { return p; }
        size_t size() const { return cap; }
        char &operator[](size_t i) { return p[i]; }
        void resize(size_t n, size_t keep) {        // keeps the first `keep` bytes
            if (n <= cap) return;
            char *q = (char *) bigmem::alloc(n);
            if (!q) throw std::bad_alloc();
            if (keep) memcpy(q, p, keep);
            bigmem::release(p);
            p = q; cap = bigmem::capacity(q);
        }
        ~RawBuf() { bigmem::release(p); }
    } buf;
    size_t pos = 0, end = 0;
    int last = 0;            // slow parser: header character already consumed ('>' or '@'), 0 = none
    bool eof = false;
    bool fast = true;        // the 4-line FASTQ fast parser is still viable
    size_t rec_bytes = 0;    // bytes per record seen so far (sizes the next block)

    // appends up to `want` bytes at buf[end..): returns the number read (0 at end of input)
    size_t read_more(size_t want) {
        if (eof || want == 0) return 0;
        if (buf.size() < end + want) buf.resize(end + want, end);
        size_t got = 0;
        if (fd >= 0) {
            const size_t piece = 8u << 20, np = (want + piece - 1) / piece;
            std::vector<ssize_t> gotp(np, 0);
            const int nt = (int) (np < (size_t) lrm_host_threads() ? np : (size_t) lrm_host_threads());
#pragma omp parallel for schedule(dynamic, 1) num_threads(nt > 1 ? nt : 1)
            for (size_t i = 0; i < np; ++i) {
                const size_t o = i * piece, l = want - o < piece ? want - o : piece;
                size_t done = 0;
                while (done < l) {
                    const ssize_t k = pread(fd, buf.data() + end + o + done, l - done, (off_t) (file_off + o + done));
                    if (k <= 0) break;
                    done += (size_t) k;
                }
                gotp[i] = (ssize_t) done;
            }
            for (size_t i = 0; i < np; ++i) {
                got += (size_t) gotp[i];
                if ((size_t) gotp[i] < (want - i * piece < piece ? want - i * piece : piece)) break;      // short piece: end of file
            }
            file_off += got;
        } else {
            while (got < want) {
                const unsigned ask = (unsigned) (want - got < (1u << 30) ? want - got : (1u << 30));
                const int k = gzread(fp, buf.data() + end + got, ask);
                if (k <= 0) break;
                got += (size_t) k;
            }
        }
        if (got < want) eof = true;
        end += got;
        return got;
    }
    void compact() {
        if (pos == 0) return;
        if (end > pos) memmove(buf.data(), buf.data() + pos, end - pos);
        end -= pos;
        pos = 0;
    }
    // ---- slow parser primitives ----
    int getc_() {
        if (pos == end) {
            pos = end = 0;
            if (read_more(1u << 20) == 0) return -1;
        }
        return (unsigned char) buf[pos++];
    }
    // appends the rest of the current line (without the newline) to s; returns false at EOF before any byte.
    // Whole buffer spans at a time (memchr + one append): a 10 kbp sequence line is one or two appends.
    bool line_(std::string &s) {
        bool any = false;
        while (true) {
            if (pos == end) {
                pos = end = 0;
                if (read_more(1u << 20) == 0) return any;
            }
            any = true;
            const char *b = buf.data() + pos;
            const char *nl = (const char *) memchr(b, '\n', end - pos);
            size_t len = nl ? (size_t) (nl - b) : end - pos;
            pos += len + (nl ? 1 : 0);
            const size_t at = s.size();
            s.append(b, len);
            if (len && memchr(b, '\r', len)) {                     // CR LF files: carriage returns are dropped wherever they are
                size_t w = at;
                for (size_t i = at; i < s.size(); ++i) if (s[i] != '\r') s[w++] = s[i];
                s.resize(w);
            }
            if (nl) return true;
        }
    }
};

extern "C" int lrm_reader_open(lrm_reader **out, const char *path) {
    int fd = open(path, O_RDONLY);
    if (fd < 0) { lrm_set_error("cannot open: %s", path); return -1; }
    unsigned char magic[2] = {0, 0};
    const ssize_t k = pread(fd, magic, 2, 0);
    lrm_reader *r = new lrm_reader;
    if (k == 2 && magic[0] == 0x1f && magic[1] == 0x8b) {          // gzip: inflate through zlib
        r->fp = gzdopen(fd, "rb");
        if (!r->fp) { close(fd); delete r; lrm_set_error("cannot open: %s", path); return -1; }
        gzbuffer(r->fp, 1u << 20);
    } else {
        r->fd = fd;
    }
    *out = r;
    return 0;
}

extern "C" void lrm_reader_close(lrm_reader *r) {
    if (!r) return;
    if (r->fp) gzclose(r->fp);
    if (r->fd >= 0) close(r->fd);
    delete r;
}

extern "C" void lrm_read_batch_free(lrm_read_batch *b) {
    if (!b) return;
    if (!b->seqs_borrowed) bigmem::release(b->seqs);           // the large buffers go back to the pool (batch_fill took them there)
    bigmem::release(b->name_arena); bigmem::release(b->qual_arena);
    free(b->lens); free(b->names); free(b->quals);
    memset(b, 0, sizeof(*b));
}

namespace {

struct RecView { const char *name; size_t name_len; const char *seq; size_t seq_len; const char *qual; };   // qual null: a FASTA record

// The batch of the n records at(0) .. at(n - 1) in the layout refactor_reads_seq builds (alnmain.c:87-103): rows NUL
// padded to stride = max_len + 1, in the caller's seq_buf when they fit there; names and qualities back to back in two
// arenas (serial prefix sums, then the copies in parallel).  Returns n, -1 without memory or for a record too long.
template <typename At>
int64_t batch_fill(lrm_read_batch *out, uint64_t n, char *seq_buf, uint64_t seq_cap, At at) {
    uint32_t max_len = 0;
    uint64_t name_bytes = 0, qual_bytes = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const RecView v = at(i);
        if (v.seq_len > 0xffffffffull) { lrm_set_error("record longer than 2^32 bases"); return -1; }
        max_len = v.seq_len > max_len ? (uint32_t) v.seq_len : max_len;
        name_bytes += v.name_len + 1;
        if (v.qual) qual_bytes += v.seq_len + 1;
    }
    out->n = n; out->max_len = max_len; out->stride = (uint64_t) max_len + 1;
    if (seq_buf && n * out->stride <= seq_cap) { out->seqs = seq_buf; out->seqs_borrowed = 1; }
    else out->seqs = (char *) bigmem::alloc(n * out->stride);
    out->lens = (uint32_t *) malloc(n * sizeof(uint32_t));
    out->names = (char **) malloc(n * sizeof(char *));
    out->quals = (char **) malloc(n * sizeof(char *));
    out->name_arena = (char *) bigmem::alloc(name_bytes);
    out->qual_arena = (char *) bigmem::alloc(qual_bytes);
    if (!out->seqs || !out->lens || !out->names || !out->quals || !out->name_arena || !out->qual_arena) {
        lrm_read_batch_free(out);
        lrm_set_error("out of memory");
        return -1;
    }
    uint64_t no = 0, qo = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const RecView v = at(i);
        out->names[i] = out->name_arena + no; no += v.name_len + 1;
        out->quals[i] = v.qual ? out->qual_arena + qo : nullptr;
        if (v.qual) qo += v.seq_len + 1;
    }
    const uint64_t stride = out->stride;
#pragma omp parallel for schedule(static) num_threads(lrm_host_threads())
    for (uint64_t i = 0; i < n; ++i) {
        const RecView v = at(i);
        char *row = out->seqs + i * stride;
        memcpy(row, v.seq, v.seq_len);
        memset(row + v.seq_len, 0, stride - v.seq_len);                           // NUL padded (alnmain.c:94 callocs)
        out->lens[i] = (uint32_t) v.seq_len;
        memcpy(out->names[i], v.name, v.name_len); out->names[i][v.name_len] = 0;
        if (v.qual) { memcpy(out->quals[i], v.qual, v.seq_len); out->quals[i][v.seq_len] = 0; }
    }
    return (int64_t) n;
}

struct FqRec { size_t name, name_len, seq, seq_len, qual; };

// One 4-line record at buf[p..e): returns the offset behind it, 0 if it is incomplete (needs more input), SIZE_MAX if it
// is not a plain 4-line record (the caller falls back to the general parser).  `final`: e is the end of the input, a
// missing last newline is fine.
inline size_t fq_record(const char *buf, size_t p, size_t e, bool final, FqRec *out) {
    if (buf[p] != '@') return SIZE_MAX;
    const char *l0 = (const char *) memchr(buf + p, '\n', e - p);
    if (!l0) return final ? SIZE_MAX : 0;
    const size_t s0 = (size_t) (l0 - buf) + 1;
    const char *l1 = s0 < e ? (const char *) memchr(buf + s0, '\n', e - s0) : nullptr;
    if (!l1) return final ? SIZE_MAX : 0;
    const size_t p0 = (size_t) (l1 - buf) + 1;
    if (p0 >= e) return final ? SIZE_MAX : 0;
    if (buf[p0] != '+') return SIZE_MAX;
    const char *l2 = (const char *) memchr(buf + p0, '\n', e - p0);
    if (!l2) return final ? SIZE_MAX : 0;
    const size_t q0 = (size_t) (l2 - buf) + 1, slen = p0 - 1 - s0;
    size_t q1;                                                       // end of the quality line
    if (q0 + slen < e) { if (buf[q0 + slen] != '\n') return SIZE_MAX; q1 = q0 + slen + 1; }
    else if (q0 + slen == e && final) q1 = e;
    else return final ? SIZE_MAX : 0;
    if ((slen && buf[s0 + slen - 1] == '\r') || buf[s0 - 2] == '\r') return SIZE_MAX;     // CR LF: general parser
    size_t nl = 0;
    while (p + 1 + nl < s0 - 1 && buf[p + 1 + nl] != ' ' && buf[p + 1 + nl] != '\t') ++nl;     // name ends at the first blank
    out->name = p + 1; out->name_len = nl; out->seq = s0; out->seq_len = slen; out->qual = q0;
    return q1;
}

// Indexes the complete 4-line records of buf[from..e) in parallel.  Returns the offset behind the last one (== from if
// none), or SIZE_MAX if the region is not 4-line FASTQ.
size_t fq_index(const char *buf, size_t from, size_t e, bool final, std::vector<FqRec> &recs) {
    const int T = lrm_host_threads();
    const size_t len = e - from;
    int nt = (int) (len / (1u << 20));
    nt = nt < 1 ? 1 : (nt > T ? T : nt);
    std::vector<size_t> start((size_t) nt + 1, e);
    start[0] = from;
    bool bad = false;
#pragma omp parallel for schedule(static, 1) num_threads(nt) reduction(|| : bad)
    for (int t = 1; t < nt; ++t) {
        // first record boundary at or after the cut: a line that starts with '@' whose line-after-next starts with '+'
        size_t c = from + len * (size_t) t / (size_t) nt;
        size_t found = e;
        for (int tries = 0; tries < 8 && c < e; ++tries) {
            const char *nl = (const char *) memchr(buf + c - 1, '\n', e - (c - 1));
            if (!nl) break;
            const size_t q = (size_t) (nl - buf) + 1;
            if (q >= e) break;
            if (buf[q] == '@') {
                const char *a = (const char *) memchr(buf + q, '\n', e - q);
                const char *b = a && (size_t) (a - buf) + 1 < e ? (const char *) memchr(a + 1, '\n', e - (size_t) (a + 1 - buf)) : nullptr;
                if (!b || (size_t) (b - buf) + 1 >= e) break;                 // runs out of the region: no boundary in this piece
                if (b[1] == '+') { found = q; break; }
            }
            c = q + 1;
        }
        start[(size_t) t] = found;
    }
    for (int t = 1; t < nt; ++t) if (start[(size_t) t] < start[(size_t) t - 1]) start[(size_t) t] = start[(size_t) t - 1];   // (pieces shorter than a record)
    std::vector<std::vector<FqRec>> part((size_t) nt);
    std::vector<size_t> stop((size_t) nt, 0);
#pragma omp parallel for schedule(static, 1) num_threads(nt) reduction(|| : bad)
    for (int t = 0; t < nt; ++t) {
        size_t p = start[(size_t) t];
        const size_t lim = start[(size_t) t + 1];
        const bool last_piece = lim == e;
        auto &v = part[(size_t) t];
        while (p < lim) {
            FqRec r;
            const size_t nx = fq_record(buf, p, e, final, &r);
            if (nx == SIZE_MAX) { bad = true; break; }
            if (nx == 0) { if (!last_piece) bad = true; break; }              // incomplete: only the tail of the region may be
            v.push_back(r);
            p = nx;
        }
        if (!bad && !last_piece && p != lim) bad = true;                      // the piece must end exactly where the next one starts
        stop[(size_t) t] = p;
    }
    if (bad) return SIZE_MAX;
    size_t behind = from;
    for (int t = 0; t < nt; ++t) {
        recs.insert(recs.end(), part[(size_t) t].begin(), part[(size_t) t].end());
        if (!part[(size_t) t].empty() || stop[(size_t) t] > behind) behind = stop[(size_t) t] > behind ? stop[(size_t) t] : behind;
    }
    return behind;
}

// the general parser (multi-line FASTA / FASTQ, CR LF): one record after the other
int64_t reader_next_slow(lrm_reader *r, uint64_t batch_size, lrm_read_batch *out, char *seq_buf, uint64_t seq_cap) {
    std::vector<std::string> names, seqs, quals;
    std::vector<char> has_qual;
    int rc = 0;
    while (names.size() < batch_size) {                      // reads_load, accaln.c:45-58
        int c = r->last;
        if (c == 0) {
            while ((c = r->getc_()) != -1 && c != '>' && c != '@') {}
            if (c == -1) break;
        }
        r->last = 0;
        std::string header, seq, qual;
        r->line_(header);
        size_t sp = header.find_first_of(" \t");
        if (sp != std::string::npos) header.resize(sp);       // name ends at the first blank
        bool plus = false;
        while ((c = r->getc_()) != -1) {
            if (c == '>' || c == '@') { r->last = c; break; }
            if (c == '+') { plus = true; break; }
            if (c == '\n' || c == '\r') continue;
            seq.push_back((char) c);
            r->line_(seq);
        }
        if (plus) {
            std::string skip;
            r->line_(skip);
            while (qual.size() < seq.size()) { if (!r->line_(qual)) break; }
            if (qual.size() != seq.size()) { rc = -2; lrm_set_error("record %s: quality length differs from sequence length", header.c_str()); break; }
        }
        names.push_back(header); seqs.push_back(seq); quals.push_back(qual); has_qual.push_back(plus ? 1 : 0);
    }
    if (rc < 0) return rc;
    const uint64_t n = names.size();
    if (n == 0) return 0;
    return batch_fill(out, n, seq_buf, seq_cap, [&](uint64_t i) {
        return RecView{names[i].data(), names[i].size(), seqs[i].data(), seqs[i].size(), has_qual[i] ? quals[i].data() : nullptr};
    });
}

}  // namespace

static int64_t reader_next_impl(lrm_reader *r, uint64_t batch_size, lrm_read_batch *out, void *seq_buf, uint64_t seq_cap);
extern "C" int64_t lrm_reader_next_into(lrm_reader *r, uint64_t batch_size, lrm_read_batch *out, void *seq_buf, uint64_t seq_cap) {
    try { return reader_next_impl(r, batch_size, out, seq_buf, seq_cap); }
    catch (const std::exception &e) { lrm_set_error("reader: %s", e.what()); return -1; }
}
static int64_t reader_next_impl(lrm_reader *r, uint64_t batch_size, lrm_read_batch *out, void *seq_buf, uint64_t seq_cap) {
    memset(out, 0, sizeof(*out));
    if (!r || batch_size == 0) return 0;
    if (!r->fast) return reader_next_slow(r, batch_size, out, (char *) seq_buf, seq_cap);
    // ---- fast parser: index at least batch_size records of the buffered block ----
    r->compact();
    std::vector<FqRec> recs;
    size_t scanned = 0;                                       // records of buf[0..scanned) are in `recs`
    for (;;) {
        if (r->end == scanned && r->eof) break;
        if (recs.size() >= batch_size) break;
        const size_t per = r->rec_bytes ? r->rec_bytes : 1024;
        size_t want = (size_t) ((batch_size - recs.size()) * (double) per * 1.05) + (1u << 20);
        if (want > (1ull << 32)) want = 1ull << 32;
        const size_t have = r->end - scanned;
        if (have < want && !r->eof) r->read_more(want - have);
        if (r->end == scanned) break;
        if (recs.empty() && scanned == 0 && r->buf[0] != '@') { r->fast = false; break; }      // FASTA or leading junk: general parser
        const size_t before = recs.size();
        const size_t behind = fq_index(r->buf.data(), scanned, r->end, r->eof, recs);
        if (behind == SIZE_MAX) { recs.resize(before); r->fast = false; break; }
        if (behind == scanned) {
            if (r->eof) { if (scanned < r->end) { r->fast = false; } break; }       // trailing bytes that are no record: let the general parser judge
            r->rec_bytes = (r->end - scanned) * 2;                                  // one record is longer than the block: read more
            continue;
        }
        scanned = behind;
        if (recs.size() > before) r->rec_bytes = (scanned) / recs.size() + 1;
    }
    if (recs.empty()) {
        if (!r->fast) return reader_next_slow(r, batch_size, out, (char *) seq_buf, seq_cap);
        return 0;
    }
    const uint64_t n = recs.size() < batch_size ? recs.size() : batch_size;
    const char *buf = r->buf.data();
    const int64_t rc = batch_fill(out, n, (char *) seq_buf, seq_cap, [&](uint64_t i) {
        const FqRec &q = recs[i];
        return RecView{buf + q.name, q.name_len, buf + q.seq, q.seq_len, buf + q.qual};
    });
    if (rc < 0) return rc;
    // behind the last record taken: the start of the next one, or what was scanned
    r->pos = n < recs.size() ? recs[n].name - 1 : scanned;
    return (int64_t) n;
}

extern "C" int64_t lrm_reader_next(lrm_reader *r, uint64_t batch_size, lrm_read_batch *out) {
    return lrm_reader_next_into(r, batch_size, out, nullptr, 0);
}
