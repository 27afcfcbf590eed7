// index_image.hip -- the index image (layout: lrm_internal.h) and the handle over it: packing from the reference's
// arrays into a host blob or straight into device memory, upload / adopt, lrm_index_get_tables, lrm_index_free.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>
#include <algorithm>
#include <omp.h>
#include "lrm_hip_util.h"
#include "extend_stage.h"

static inline uint64_t align256(uint64_t x) { return (x + 255ull) & ~255ull; }
#define LRM_LCX_MAX 4096    // capacity of the long-interval side table

// THE sections of the image behind the header, in image order: where the header keeps the offset, the bytes of one element,
// the number of elements.  The layout, the packer's pieces (whole elements, BlobPacker::fill) and the gaps to clear all
// come from this table.
enum { S_OCC, S_LC, S_LCX, S_SA, S_CONTENT, S_MTA, N_SECTIONS };
struct Section { uint64_t LrmBlobHeader::*off; uint64_t elem; uint64_t (*count)(const LrmBlobHeader &); };
static const Section k_sections[N_SECTIONS] = {
    {&LrmBlobHeader::off_occ, sizeof(LrmOccBlock), [](const LrmBlobHeader &h) { return h.n_blocks; }},
    {&LrmBlobHeader::off_lc, 8, [](const LrmBlobHeader &h) { return h.lc_entries; }},
    {&LrmBlobHeader::off_lcx, 24, [](const LrmBlobHeader &) { return (uint64_t) LRM_LCX_MAX; }},
    {&LrmBlobHeader::off_sa, 8, [](const LrmBlobHeader &h) { return h.sa_len; }},
    {&LrmBlobHeader::off_content, 1, [](const LrmBlobHeader &h) { return h.con_len + 1; }},                 // the text and a NUL
    {&LrmBlobHeader::off_mta, sizeof(LrmMtaDev), [](const LrmBlobHeader &h) { return (uint64_t) (h.mta_len > 0 ? h.mta_len : 1); }},
};
static inline uint64_t section_bytes(const LrmBlobHeader &h, int s) { return k_sections[s].elem * k_sections[s].count(h); }

static void blob_layout(uint64_t length, int hlen, int mta_len, int sa_ratio, LrmBlobHeader *h) {
    memset(h, 0, sizeof(*h));
    h->magic = LRM_BLOB_MAGIC;
    h->version = LRM_ABI_VERSION;
    h->length = length;
    h->hlen = hlen;
    h->mta_len = mta_len;
    h->n_blocks = (length + LRM_OCC_ROWS - 1) / LRM_OCC_ROWS + 1;   // +1: rank(loc) may touch the block of L-1 only; spare block keeps gathers in bounds
    h->lc_entries = 1ull << (2 * hlen);
    h->sa_ratio = (uint64_t) sa_ratio;
    h->sa_len = sa_ratio > 1 ? (length + sa_ratio - 1) / sa_ratio : length;
    h->con_len = length;
    uint64_t off = sizeof(LrmBlobHeader);
    for (int s = 0; s < N_SECTIONS; ++s) { h->*k_sections[s].off = off; off = align256(off + section_bytes(*h, s)); }
    h->total_bytes = off;
}

static void tune_of(const lrm_index_options *opt, LrmIndexTune *t) {
    LrmEnv env;
    lrm_env_snapshot(&env);
    lrm_resolve_index_tune(opt, env, t);
}

extern "C" uint64_t lrm_index_blob_bytes_opt(uint64_t length, int hlen, int mta_len, const lrm_index_options *opt) {
    LrmIndexTune t;
    tune_of(opt, &t);
    LrmBlobHeader h;
    blob_layout(length, hlen, mta_len, t.sa_ratio, &h);
    return h.total_bytes;
}
extern "C" uint64_t lrm_index_blob_bytes(uint64_t length, int hlen, int mta_len) {
    return lrm_index_blob_bytes_opt(length, hlen, mta_len, nullptr);
}

// The image is produced SECTION BY SECTION in pieces of <= LRM_PACK_PIECE bytes, every piece by all host
// threads, so that the same code fills a host blob (lrm_index_pack_blob) or a pair of pinned chunks whose DMA
// overlaps the packing of the next piece (lrm_index_upload: no host copy of the image -- GRCh38 is a 63 GB
// image next to 75 GB of reference-layout arrays).
#define LRM_PACK_PIECE (64ull << 20)
struct BlobPacker {
    const lrm_dna_fmi *fmi; const lrm_lc_hash *lch; const lrm_sa_mem *sa; const char *content;
    const lrm_mta_entry *mta; int mta_len;
    LrmBlobHeader h;
    uint64_t L;
    static constexpr uint64_t SEG = 1ull << 20;          // rows per segment of the bwt prefix counts
    std::vector<uint64_t> seg_cnt;                       // [seg][4]: # of A,C,G,T in bwt[0 .. seg*SEG)
    uint64_t total[4];
    std::vector<uint64_t> lcx;                           // side table, sorted {code, k, l}

    int init(const lrm_dna_fmi *fmi_, const lrm_lc_hash *lch_, const lrm_sa_mem *sa_, const char *content_,
             uint64_t con_len, const lrm_mta_entry *mta_, int mta_len_, const lrm_index_options *opt) {
        LrmIndexTune tune;
        tune_of(opt, &tune);
        fmi = fmi_; lch = lch_; sa = sa_; content = content_; mta = mta_; mta_len = mta_len_;
        if (!fmi || !lch || !sa || !content) { lrm_set_error("null argument"); return -1; }
        L = fmi->length;
        if (L < 2 || L >= (1ull << 40)) { lrm_set_error("text length %llu outside [2, 2^40)", (unsigned long long) L); return -1; }
        if (con_len != L) { lrm_set_error("content length %llu != fm length %llu", (unsigned long long) con_len, (unsigned long long) L); return -1; }
        if (sa->len < L) { lrm_set_error("suffix array has %llu rows, need %llu", (unsigned long long) sa->len, (unsigned long long) L); return -1; }
        if (lch->hlen < 1 || lch->hlen > 15) { lrm_set_error("hlen %d outside [1,15] (lchash.c:75-77)", lch->hlen); return -1; }
        if (lch->len != 2ull << (2 * lch->hlen)) { lrm_set_error("lc table length %llu != 2*4^hlen", (unsigned long long) lch->len); return -1; }
        if (mta_len < 0 || (mta_len > 0 && !mta)) { lrm_set_error("bad mta"); return -1; }
        if ((uint64_t) mta_len * sizeof(LrmMtaDev) > LRM_PACK_PIECE) { lrm_set_error("too many sequences"); return -1; }      // [mta] is one piece
        blob_layout(L, lch->hlen, mta_len, tune.sa_ratio, &h);
        h.c4[0] = fmi->c[(unsigned char) 'A']; h.c4[1] = fmi->c[(unsigned char) 'C'];
        h.c4[2] = fmi->c[(unsigned char) 'G']; h.c4[3] = fmi->c[(unsigned char) 'T'];

        // pass 1 over the bwt: per-segment symbol counts (parallel), the '$' row, alphabet check
        const uint64_t nseg = (L + SEG - 1) / SEG;
        seg_cnt.assign((nseg + 1) * 4, 0);
        uint64_t dollar = ~0ull, n_dollar = 0, bad_row = ~0ull;
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(dynamic, 4) reduction(+ : n_dollar) reduction(min : dollar, bad_row)
        for (uint64_t sg = 0; sg < nseg; ++sg) {
            const uint64_t lo = sg * SEG, hi = lo + SEG < L ? lo + SEG : L;
            uint64_t c[4] = {0, 0, 0, 0};
            for (uint64_t i = lo; i < hi; ++i) {
                const char ch = fmi->bwt[i];
                const int code = base_code(ch);
                if (code >= 0) c[code]++;
                else if (ch == '$') { n_dollar++; if (i < dollar) dollar = i; }
                else if (i < bad_row) bad_row = i;
            }
            for (int x = 0; x < 4; ++x) seg_cnt[(sg + 1) * 4 + x] = c[x];
        }
        if (bad_row != ~0ull || n_dollar > 1) {
            const uint64_t r = bad_row != ~0ull ? bad_row : dollar;
            lrm_set_error("bwt row %llu holds byte 0x%02x (only upper-case ACGT and one '$' supported)", (unsigned long long) r, (unsigned) (unsigned char) fmi->bwt[r]);
            return -1;
        }
        if (n_dollar == 0) { lrm_set_error("bwt has no '$' row"); return -1; }
        h.dollar_row = dollar;
        for (uint64_t sg = 1; sg <= nseg; ++sg)
            for (int x = 0; x < 4; ++x) seg_cnt[sg * 4 + x] += seg_cnt[(sg - 1) * 4 + x];
        for (int x = 0; x < 4; ++x) total[x] = seg_cnt[nseg * 4 + x];

        // side table of the lc intervals that do not fit 24 bits of length
        const uint64_t long_thr = tune.lcx_threshold;           // (tests send shorter intervals through the side table too)
        lcx_thr = long_thr;
        std::vector<uint64_t> over;
        const uint64_t ne = h.lc_entries;
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static)
        for (uint64_t num = 0; num < ne; ++num) {
            const uint64_t k = lch->lc[2 * num], l = lch->lc[2 * num + 1];
            if (k == 0 && l == 0) continue;
            const uint64_t cnt = l >= k ? l - k + 1 : 0;
            if (cnt == 0 || cnt >= long_thr || k >= (1ull << 40)) {
                const uint64_t code = rev_groups(num, lch->hlen);
#pragma omp critical
                { over.push_back(code); over.push_back(k); over.push_back(l); }
            }
        }
        if (over.size() / 3 > LRM_LCX_MAX) { lrm_set_error("too many long lchash intervals (%zu)", over.size() / 3); return -1; }
        std::vector<size_t> ord(over.size() / 3);
        for (size_t i = 0; i < ord.size(); ++i) ord[i] = i;
        std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return over[3 * a] < over[3 * b]; });
        lcx.assign(3 * (size_t) LRM_LCX_MAX, ~0ull);
        for (size_t i = 0; i < ord.size(); ++i)
            for (int f = 0; f < 3; ++f) lcx[3 * i + f] = over[3 * ord[i] + f];
        h.n_lcx = ord.size();
        return 0;
    }

    uint64_t lcx_thr = 0xFFFFFFull;
    static inline uint64_t rev_groups(uint64_t v, int hl) {          // reverse the order of the 2-bit groups
        uint64_t code = 0;
        for (int i = 0; i < hl; ++i) { code = (code << 2) | (v & 3); v >>= 2; }
        return code;
    }

    // occ blocks [b0, b0 + nb): one {C[sym] + prefix count, occurrence mask} pair per symbol and 64 bwt rows;
    // cross-checked against the reference's sampled O table (fmidx.c:128-150)
    int fill_occ(uint64_t b0, uint64_t nb, LrmOccBlock *dst) const {
        const uint64_t ratio = (uint64_t) fmi->o_ratio;
        const uint64_t bps = SEG / LRM_OCC_ROWS;           // blocks per segment
        uint64_t bad = ~0ull;
        const uint64_t s0 = b0 / bps, s1 = (b0 + nb + bps - 1) / bps;
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(dynamic, 1) reduction(min : bad)
        for (uint64_t sg = s0; sg < s1; ++sg) {
            uint64_t run[4];
            const uint64_t nseg = (L + SEG - 1) / SEG;
            const uint64_t sgc = sg < nseg ? sg : nseg;
            for (int x = 0; x < 4; ++x) run[x] = seg_cnt[sgc * 4 + x];
            const uint64_t blo = sg * bps > b0 ? sg * bps : b0, bhi = (sg + 1) * bps < b0 + nb ? (sg + 1) * bps : b0 + nb;
            // rows of the segment before blo (a piece boundary inside a segment): count them
            for (uint64_t i = sg * SEG; i < blo * LRM_OCC_ROWS && i < L; ++i) { const int c = base_code(fmi->bwt[i]); if (c >= 0) run[c]++; }
            for (uint64_t b = blo; b < bhi; ++b) {
                LrmOccBlock blk;
                for (int x = 0; x < 4; ++x) { blk.sym[x].cnt = h.c4[x] + run[x]; blk.sym[x].mask = 0; }
                const uint64_t r0 = b * LRM_OCC_ROWS, r1 = r0 + LRM_OCC_ROWS < L ? r0 + LRM_OCC_ROWS : L;
                for (uint64_t i = r0; i < r1; ++i) {
                    if (fmi->o && ratio > 0 && i % ratio == 0) {
                        const uint64_t *o = fmi->o + 4 * (i / ratio);
                        if ((o[0] != run[0] || o[1] != run[1] || o[2] != run[2] || o[3] != run[3]) && i < bad) bad = i;
                    }
                    const int c = base_code(fmi->bwt[i]);
                    if (c >= 0) { run[c]++; blk.sym[c].mask |= 1ull << (i & 63); }
                }
                dst[b - b0] = blk;
            }
        }
        if (bad != ~0ull) { lrm_set_error("O table disagrees with bwt at row %llu", (unsigned long long) bad); return -1; }
        return 0;
    }

    // lc entries [c0, c0 + n) in device order (LSB-first code): gathered from the reference's table
    void fill_lc(uint64_t c0, uint64_t n, uint64_t *dst) const {
        const int hl = lch->hlen;
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static)
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t num = rev_groups(c0 + i, hl);               // the permutation is an involution
            const uint64_t k = lch->lc[2 * num], l = lch->lc[2 * num + 1];
            uint64_t e = 0;
            if (!(k == 0 && l == 0)) {
                uint64_t cnt = l >= k ? l - k + 1 : 0;
                if (cnt == 0 || cnt >= lcx_thr || k >= (1ull << 40)) cnt = 0xFFFFFFull;
                e = (k & ((1ull << 40) - 1ull)) | (cnt << 40);
            }
            dst[i] = e;
        }
    }

    // SA entries [e0, e0 + n) of the image: rows e*sa_ratio, as u64 (sa_use.h:27-29)
    void fill_sa(uint64_t e0, uint64_t n, uint64_t *dst) const {
        const uint64_t r = h.sa_ratio;
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static)
        for (uint64_t i = 0; i < n; ++i) dst[i] = ui40_get(sa->mem[(e0 + i) * r]);
    }

    // text bytes [o, o + n) and the NUL behind the text
    void fill_content(uint64_t o, uint64_t n, uint8_t *b) const {
        const uint64_t nc = o + n > L ? L - o : n;
        const uint64_t piece = 1ull << 20, np = (nc + piece - 1) / piece;
#pragma omp parallel for num_threads(lrm_host_threads()) schedule(static)
        for (uint64_t i = 0; i < np; ++i) {
            const uint64_t po = i * piece, pl = nc - po < piece ? nc - po : piece;
            memcpy(b + po, content + o + po, pl);
        }
        if (nc < n) b[nc] = 0;
    }

    // elements [lo, lo + n) of section s
    int fill(int s, uint64_t lo, uint64_t n, uint8_t *b) const {
        switch (s) {
        case S_OCC: return fill_occ(lo, n, (LrmOccBlock *) b);
        case S_LC: fill_lc(lo, n, (uint64_t *) b); return 0;
        case S_LCX: memcpy(b, lcx.data() + 3 * lo, n * 24); return 0;
        case S_SA: fill_sa(lo, n, (uint64_t *) b); return 0;
        case S_CONTENT: fill_content(lo, n, b); return 0;
        default: {                                                     // S_MTA; an image without sequences holds one zero entry
            LrmMtaDev *md = (LrmMtaDev *) b;
            for (uint64_t i = lo; i < lo + n; ++i)
                md[i - lo] = i < (uint64_t) mta_len ? LrmMtaDev{mta[i].offset, (uint64_t) mta[i].seq_len} : LrmMtaDev{0, 0};
            return 0;
        }
        }
    }

    // Emits the image in order as (offset, bytes) pieces through `sink`, which may consume the buffer asynchronously:
    // next_buf(offset) hands out the buffer for the piece that goes to `offset` (>= LRM_PACK_PIECE bytes, or the piece's
    // own place in a host blob).
    template <typename NextBuf, typename Sink>
    int emit(NextBuf next_buf, Sink sink) const {
        {   // header
            uint8_t *b = next_buf(0);
            if (!b) return -1;
            memcpy(b, &h, sizeof(h));
            if (sink(0, sizeof(h), b)) return -1;
        }
        for (int s = 0; s < N_SECTIONS; ++s) {
            const Section &sec = k_sections[s];
            const uint64_t count = sec.count(h), per = LRM_PACK_PIECE / sec.elem;
            for (uint64_t lo = 0; lo < count; lo += per) {
                const uint64_t n = count - lo < per ? count - lo : per, off = h.*sec.off + lo * sec.elem;
                uint8_t *b = next_buf(off);
                if (!b) return -1;
                if (fill(s, lo, n, b) || sink(off, n * sec.elem, b)) return -1;
            }
        }
        return 0;
    }
};

extern "C" int lrm_index_pack_blob(const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa,
                                   const char *content, uint64_t con_len, const lrm_mta_entry *mta, int mta_len,
                                   void *blob, uint64_t blob_bytes) {
    return lrm_index_pack_blob_opt(fmi, lch, sa, content, con_len, mta, mta_len, blob, blob_bytes, nullptr);
}
extern "C" int lrm_index_pack_blob_opt(const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa,
                                       const char *content, uint64_t con_len, const lrm_mta_entry *mta, int mta_len,
                                       void *blob, uint64_t blob_bytes, const lrm_index_options *opt) {
    if (!blob) { lrm_set_error("null argument"); return -1; }
    BlobPacker pk;
    if (pk.init(fmi, lch, sa, content, con_len, mta, mta_len, opt)) return -1;
    const LrmBlobHeader &h = pk.h;
    if (blob_bytes < h.total_bytes) { lrm_set_error("blob buffer too small"); return -1; }
    // pieces are written in place: the buffer of a piece is its own position in the blob, so there is nothing left for the
    // sink to do; the gaps between the 256-byte aligned sections (and the spare tail) are cleared first, so that images of
    // equal inputs are byte-identical
    uint8_t *base = (uint8_t *) blob;
    for (int s = 0; s < N_SECTIONS; ++s) {
        const uint64_t end = h.*k_sections[s].off + section_bytes(h, s), next = s + 1 < N_SECTIONS ? h.*k_sections[s + 1].off : h.total_bytes;
        if (next > end) memset(base + end, 0, next - end);
    }
    return pk.emit([&](uint64_t off) -> uint8_t * { return base + off; }, [](uint64_t, uint64_t, const uint8_t *) -> int { return 0; });
}

int lrm_index_make_handle(lrm_index **out, void *d_blob, uint64_t bytes, int device, int owns, const LrmBlobHeader &h,
                          const lrm_index_options *opt) {
    if (h.magic != LRM_BLOB_MAGIC || h.version != LRM_ABI_VERSION) { lrm_set_error("not an lrm index image (magic/version)"); return -1; }
    if (h.total_bytes > bytes) { lrm_set_error("index image truncated"); return -1; }
    lrm_index *ix = new (std::nothrow) lrm_index;
    if (!ix) { lrm_set_error("out of memory"); return -1; }
    memset(ix, 0, sizeof(*ix));
    ix->d_blob = d_blob; ix->blob_bytes = bytes; ix->owns_blob = owns; ix->device = device; ix->hdr = h;
    uint8_t *b = (uint8_t *) d_blob;
    ix->view.occ = (const LrmOccBlock *) (b + h.off_occ);
    ix->view.lc = (const uint64_t *) (b + h.off_lc);
    ix->view.lcx = (const uint64_t *) (b + h.off_lcx);
    ix->view.n_lcx = h.n_lcx;
    ix->view.sa = (const uint64_t *) (b + h.off_sa);
    ix->view.content = (const char *) (b + h.off_content);
    ix->view.mta = (const LrmMtaDev *) (b + h.off_mta);
    ix->view.length = h.length; ix->view.dollar_row = h.dollar_row;
    ix->view.sa_len = h.sa_len; ix->view.con_len = h.con_len;
    for (int i = 0; i < 4; ++i) ix->view.c4[i] = h.c4[i];
    ix->view.hlen = h.hlen; ix->view.mta_len = h.mta_len;
    // (the derived tables of the view -- core, sd, lcl -- and sa_shift start out null / 0: the memset above)
    for (uint64_t r = h.sa_ratio > 1 ? h.sa_ratio : 1; r > 1; r >>= 1) ix->view.sa_shift++;
    ix->n_peers = 1;
    lrm_env_snapshot(&ix->env);                          // the LRM_* overrides are read here, once per handle
    lrm_resolve_index_tune(opt, ix->env, &ix->itune);
    lrm_resolve_map_tune(nullptr, ix->env, &ix->mtune);
    if (lrm_bs_prepare_index(ix)) { delete ix; return -1; }
    if (lrm_lcl_prepare_index(ix)) { lrm_bs_free_index(ix); delete ix; return -1; }
    *out = ix;
    return 0;
}

extern "C" int lrm_index_upload_blob(lrm_index **out, const void *blob, uint64_t blob_bytes, int device) {
    return lrm_index_upload_blob_opt(out, blob, blob_bytes, device, nullptr);
}
extern "C" int lrm_index_upload_blob_opt(lrm_index **out, const void *blob, uint64_t blob_bytes, int device,
                                         const lrm_index_options *opt) {
    if (!out || !blob || blob_bytes < sizeof(LrmBlobHeader)) { lrm_set_error("bad blob"); return -1; }
    if (lrm_require_device(device)) return -1;
    LrmBlobHeader h;
    memcpy(&h, blob, sizeof(h));
    void *d = nullptr;
    HIPCHK(hipMalloc(&d, blob_bytes));
    if (hipMemcpy(d, blob, blob_bytes, hipMemcpyHostToDevice) != hipSuccess) { (void) hipFree(d); lrm_set_error("index upload failed"); return -1; }
    if (lrm_index_make_handle(out, d, blob_bytes, device, 1, h, opt)) { (void) hipFree(d); return -1; }
    return 0;
}

extern "C" int lrm_index_adopt_device(lrm_index **out, void *d_blob, uint64_t blob_bytes, int device) {
    return lrm_index_adopt_device_opt(out, d_blob, blob_bytes, device, nullptr);
}
extern "C" int lrm_index_adopt_device_opt(lrm_index **out, void *d_blob, uint64_t blob_bytes, int device,
                                          const lrm_index_options *opt) {
    if (!out || !d_blob || blob_bytes < sizeof(LrmBlobHeader)) { lrm_set_error("bad blob"); return -1; }
    if (lrm_require_device(device)) return -1;
    LrmBlobHeader h;
    HIPCHK(hipMemcpy(&h, d_blob, sizeof(h), hipMemcpyDeviceToHost));
    return lrm_index_make_handle(out, d_blob, blob_bytes, device, 0, h, opt);
}

// pack + upload without a host copy of the image: two pinned chunks, the DMA of one overlaps the packing of the other
static int stream_image(const BlobPacker &pk, void *d_dst) {
    struct Res {
        void *pin[2] = {nullptr, nullptr}; hipEvent_t ev[2] = {nullptr, nullptr}; hipStream_t st = nullptr;
        ~Res() {
            if (st) { (void) hipStreamSynchronize(st); (void) hipStreamDestroy(st); }
            for (int i = 0; i < 2; ++i) { if (pin[i]) (void) hipHostFree(pin[i]); if (ev[i]) (void) hipEventDestroy(ev[i]); }
        }
    } r;
    HIPCHK(hipStreamCreateWithFlags(&r.st, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        HIPCHK(hipHostMalloc(&r.pin[i], LRM_PACK_PIECE, hipHostMallocDefault));
        HIPCHK(hipEventCreateWithFlags(&r.ev[i], hipEventDisableTiming));
    }
    HIPCHK(hipMemsetAsync(d_dst, 0, pk.h.total_bytes, r.st));          // alignment gaps: images of equal inputs are byte-identical
    uint64_t seq = 0;
    bool used[2] = {false, false};
    int rc = pk.emit(
        [&](uint64_t) -> uint8_t * {
            const int b = (int) (seq & 1);
            if (used[b] && hipEventSynchronize(r.ev[b]) != hipSuccess) { lrm_set_error("index upload: event wait failed"); return nullptr; }
            return (uint8_t *) r.pin[b];
        },
        [&](uint64_t off, uint64_t n, const uint8_t *buf) -> int {
            const int b = (int) (seq & 1);
            HIPCHK(hipMemcpyAsync((uint8_t *) d_dst + off, buf, n, hipMemcpyHostToDevice, r.st));
            HIPCHK(hipEventRecord(r.ev[b], r.st));
            used[b] = true;
            ++seq;
            return 0;
        });
    if (rc) return -1;
    HIPCHK(hipStreamSynchronize(r.st));
    return 0;
}

int lrm_index_upload_one(lrm_index **out, const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa,
                      const char *content, uint64_t con_len, const lrm_mta_entry *mta, int mta_len, int device,
                      const lrm_index_options *opt) {
    if (!out || !fmi || !lch) { lrm_set_error("null argument"); return -1; }
    if (lrm_require_device(device)) return -1;
    BlobPacker pk;
    if (pk.init(fmi, lch, sa, content, con_len, mta, mta_len, opt)) return -1;
    const uint64_t bytes = pk.h.total_bytes;
    void *d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) { (void) hipGetLastError(); lrm_set_error("hipMalloc of the %llu-byte index image failed", (unsigned long long) bytes); return -1; }
    if (stream_image(pk, d) || lrm_index_make_handle(out, d, bytes, device, 1, pk.h, opt)) { (void) hipFree(d); return -1; }
    return 0;
}

extern "C" int lrm_index_upload(lrm_index **out, const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa,
                                const char *content, uint64_t con_len, const lrm_mta_entry *mta, int mta_len, int device) {
    return lrm_index_upload_one(out, fmi, lch, sa, content, con_len, mta, mta_len, device, nullptr);
}

// the same into device memory the caller owns (e.g. a buffer that is then broadcast to the other ranks and
// adopted with lrm_index_adopt_device on every rank)
extern "C" int lrm_index_pack_device(const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa,
                                     const char *content, uint64_t con_len, const lrm_mta_entry *mta, int mta_len,
                                     void *d_blob, uint64_t blob_bytes, int device) {
    return lrm_index_pack_device_opt(fmi, lch, sa, content, con_len, mta, mta_len, d_blob, blob_bytes, device, nullptr);
}
extern "C" int lrm_index_pack_device_opt(const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa,
                                         const char *content, uint64_t con_len, const lrm_mta_entry *mta, int mta_len,
                                         void *d_blob, uint64_t blob_bytes, int device, const lrm_index_options *opt) {
    if (!fmi || !lch || !d_blob) { lrm_set_error("null argument"); return -1; }
    if (lrm_require_device(device)) return -1;
    BlobPacker pk;
    if (pk.init(fmi, lch, sa, content, con_len, mta, mta_len, opt)) return -1;
    if (blob_bytes < pk.h.total_bytes) { lrm_set_error("device buffer too small for the image"); return -1; }
    return stream_image(pk, d_blob);
}

extern "C" int lrm_index_get_tables(const lrm_index *idx, lrm_index_tables *out) {
    if (!idx || !out) { lrm_set_error("lrm_index_get_tables: null argument"); return -1; }
    memset(out, 0, sizeof(*out));
    const LrmIndexView &v = idx->view;
    uint64_t bytes = 0;
    if (v.lcl) {
        out->lc_long = v.hl; out->lc_pair = v.lcl_pair; out->lc_entry_bytes = v.lcl_kbits ? 5 : 8;
        bytes += ((v.lcl_pair ? 2ull : 1ull) << (2 * v.hl)) * (uint64_t) out->lc_entry_bytes;
        if (v.lclx) bytes += (v.lclx_mask + 1) * 16;
    }
    if (v.core) { out->lc_core = 1; bytes += 64ull << 26; }
    if (v.sd) {
        out->seed_table_len = v.sd_len; out->seed_table_share = v.sd_f; out->seed_table_bits = v.sd_bits;
        out->seed_table_slot_bytes = v.sd_slot; out->seed_table_count_bits = v.sd_cbits;
        out->seed_table_side_entries = idx->sd_side_entries;
        bytes += (64ull << v.sd_bits) + (v.sdx_mask + 1) * 16;
    }
    out->derived_bytes = bytes;
    return 0;
}

extern "C" void lrm_index_free(lrm_index *idx) {
    if (!idx) return;
    for (int r = 1; r < idx->n_peers && idx->peers; ++r) lrm_index_free(idx->peers[r]);     // replicas of a multi-GPU group
    delete[] idx->peers;
    (void) hipSetDevice(idx->device);
    lrm_host_ctx_free(idx);                      // workspace, device mirrors, pinned staging, streams of the host-buffer calls
    lrm_bs_free_index(idx);
    if (idx->d_lcl) (void) hipFree(idx->d_lcl);
    if (idx->d_lclx) (void) hipFree(idx->d_lclx);
    if (idx->d_core) (void) hipFree(idx->d_core);
    if (idx->d_sd) (void) hipFree(idx->d_sd);
    if (idx->d_sdx) (void) hipFree(idx->d_sdx);
    if (idx->d_sd_filt) (void) hipFree(idx->d_sd_filt);
    if (idx->owns_blob && idx->d_blob) (void) hipFree(idx->d_blob);
    delete idx;
}
