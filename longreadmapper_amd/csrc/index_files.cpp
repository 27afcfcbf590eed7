// index_files.cpp -- the index on disk (include/lrm_index_host.h; Notes.txt:6-29): genome.mta, genome.cat, genome.cat.mfi,
// genome.cat.lch, genome.cat.sa5 as the reference writes and reads them, the FASTA reader, and lrm_accidx (FASTA -> files).
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/lrm_index_host.h"
#include "lrm_internal.h"

namespace {

// A FILE that closes itself and knows its path for the error text.  A failed open has set the message; test with ok().
class File {
    FILE *fp;
    std::string path;
public:
    File(const std::string &p, const char *mode) : fp(fopen(p.c_str(), mode)), path(p) {
        if (!fp) lrm_set_error("%s: %s", mode[0] == 'r' ? "cannot open" : "cannot create", p.c_str());
    }
    ~File() { if (fp) fclose(fp); }
    File(const File &) = delete;
    File &operator=(const File &) = delete;
    bool ok() const { return fp != nullptr; }
    bool fail(const char *what, const char *field = nullptr) const {           // "<what> (<field>): <path>", false
        if (field) lrm_set_error("%s (%s): %s", what, field, path.c_str());
        else lrm_set_error("%s: %s", what, path.c_str());
        return false;
    }
    size_t read_some(void *p, size_t n) { return fread(p, 1, n, fp); }         // the bytes it got, no message
    char *read_line(char *buf, int n) { return fgets(buf, n, fp); }
    bool read_exact(void *p, size_t n, const char *field = nullptr) { return read_some(p, n) == n || fail("short read", field); }
    bool write_exact(const void *p, size_t n) { return fwrite(p, 1, n, fp) == n || fail("write failed"); }
    // a whole file from a buffer / into a malloc'd buffer with a NUL behind it
    static bool write_all(const std::string &p, const char *buf, uint64_t n) {
        File f(p, "wb");
        return f.ok() && f.write_exact(buf, n);
    }
    static bool read_all(const std::string &p, char *&buf, uint64_t &n) {
        File f(p, "rb");
        if (!f.ok()) return false;
        fseek(f.fp, 0, SEEK_END);
        const long l = ftell(f.fp);
        fseek(f.fp, 0, SEEK_SET);
        if (l < 0) return f.fail("cannot tell the size");
        if (!lrm_alloc(buf, (uint64_t) l + 1, "text") || !f.read_exact(buf, (size_t) l)) return false;
        buf[l] = 0;
        n = (uint64_t) l;
        return true;
    }
};

// ---- ONE description per format: the fields in file order, visited by a FieldWriter or a FieldReader -------------------------
// scalar(x): sizeof(x) bytes.  array(p, n, name, nul): n elements; the reader allocates them (one more, zeroed, with nul).
struct FieldWriter {
    File &f;
    template <typename T> bool scalar(const T &x) { return f.write_exact(&x, sizeof(T)); }
    template <typename T> bool array(const T *p, uint64_t n, const char *, bool = false) { return f.write_exact(p, n * sizeof(T)); }
};
struct FieldReader {
    File &f;
    bool quiet;              // a record that ends early is the end of the list, not an error (.mta): no message
    template <typename T> bool scalar(T &x) { return get(&x, sizeof(T), nullptr); }
    template <typename T> bool array(T *&p, uint64_t n, const char *name, bool nul = false) {
        const size_t bytes = (size_t) n * sizeof(T);
        p = (T *) malloc(bytes + sizeof(T));
        if (!p) return f.fail("out of memory", name);
        if (!get(p, bytes, name)) return false;
        if (nul) p[n] = T();
        return true;
    }
    bool get(void *p, size_t n, const char *name) { return quiet ? f.read_some(p, n) == n : f.read_exact(p, n, name); }
};

template <typename V, typename F>
bool fmi_fields(V &v, F &f) {                                      // .mfi (fmidx.c:221-275)
    return v.array(f.c, 256, "C") && v.scalar(f.o_ratio) && v.scalar(f.o_len) && v.array(f.o, f.o_len, "O") &&
           v.scalar(f.length) && v.array(f.bwt, f.length, "bwt", true) &&
           v.scalar(f.csa_ratio) && v.scalar(f.csa_len) && v.array(f.csa, f.csa_len, "csa");
}
template <typename V, typename H>
bool lc_fields(V &v, H &h) {                                       // .lch (lchash.c:106-127)
    return v.scalar(h.hlen) && v.scalar(h.len) && v.array(h.lc, h.len, "lc");
}
template <typename V, typename E>
bool mta_fields(V &v, E &e) {                                      // one .mta record (asindex.c:89-93, mutils.c:53-68): mstring, offset, size_t
    return v.scalar(e.name_len) && v.array(e.name, e.name_len, "name", true) && v.scalar(e.offset) && v.scalar(e.seq_len);
}

// a reader that failed leaves nothing behind: its allocations freed, the struct zeroed
int fmi_read_failed(lrm_dna_fmi *f) { free(f->c); free(f->o); free(f->csa); free(f->bwt); memset(f, 0, sizeof(*f)); return -1; }
int lc_read_failed(lrm_lc_hash *h) { free(h->lc); memset(h, 0, sizeof(*h)); return -1; }

constexpr uint64_t SA5_CHUNK = 1 << 20;      // entries per read / write of .sa5

}  // namespace

extern "C" int lrm_fmi_write(const lrm_dna_fmi *fmi, const char *prefix) {
    File f(std::string(prefix) + ".mfi", "wb");
    FieldWriter w{f};
    return f.ok() && fmi_fields(w, *fmi) ? 0 : -1;
}

extern "C" int lrm_fmi_read(lrm_dna_fmi *fmi, const char *prefix) {
    memset(fmi, 0, sizeof(*fmi));
    File f(std::string(prefix) + ".mfi", "rb");
    FieldReader r{f, false};
    return f.ok() && fmi_fields(r, *fmi) ? 0 : fmi_read_failed(fmi);
}

extern "C" int lrm_lc_write(const char *path, const lrm_lc_hash *h) {
    File f(path, "wb");
    FieldWriter w{f};
    return f.ok() && lc_fields(w, *h) ? 0 : -1;
}

extern "C" int lrm_lc_read(const char *path, lrm_lc_hash *h) {
    memset(h, 0, sizeof(*h));
    File f(path, "rb");
    FieldReader r{f, false};
    return f.ok() && lc_fields(r, *h) ? 0 : lc_read_failed(h);
}

extern "C" int lrm_sa5_write(const char *path, const lrm_ui40 *mem, uint64_t n) {    // 5-byte little-endian entries (uint40.h)
    File f(path, "wb");
    if (!f.ok()) return -1;
    std::vector<uint8_t> buf(SA5_CHUNK * 5);
    for (uint64_t i = 0; i < n; i += SA5_CHUNK) {
        const uint64_t m = n - i < SA5_CHUNK ? n - i : SA5_CHUNK;
        for (uint64_t j = 0; j < m; ++j) { const uint64_t v = ui40_get(mem[i + j]); memcpy(&buf[j * 5], &v, 5); }
        if (!f.write_exact(buf.data(), m * 5)) return -1;
    }
    return 0;
}

// ui40_fread (sa_use.h:31-46): the entries it got, which may be fewer than asked for
extern "C" int64_t lrm_sa5_read(const char *path, lrm_ui40 *mem, uint64_t nitems) {
    File f(path, "rb");
    if (!f.ok()) return -1;
    std::vector<uint8_t> buf(SA5_CHUNK * 5);
    uint64_t got = 0;
    while (got < nitems) {
        const uint64_t want = nitems - got < SA5_CHUNK ? nitems - got : SA5_CHUNK;
        const uint64_t m = f.read_some(buf.data(), want * 5) / 5;
        for (uint64_t j = 0; j < m; ++j) { uint64_t v = 0; memcpy(&v, &buf[j * 5], 5); ui40_put(&mem[got + j], v); }
        got += m;
        if (m < want) break;
    }
    return (int64_t) got;
}

extern "C" int lrm_mta_write(const char *path, const lrm_mta_entry *mta, int n) {
    File f(path, "wb");
    if (!f.ok()) return -1;
    FieldWriter w{f};
    for (int i = 0; i < n; ++i) if (!mta_fields(w, mta[i])) return -1;
    return 0;
}

// load_mta (alnmain.c:125-140): records until the file ends, inside a record or not, 65535 at most (alnmain.c:127)
extern "C" int lrm_mta_read(const char *path, lrm_mta_entry **mta_out) {
    File f(path, "rb");
    if (!f.ok()) return -1;
    FieldReader r{f, true};
    std::vector<lrm_mta_entry> v;
    while (v.size() < 65535) {
        lrm_mta_entry e;
        memset(&e, 0, sizeof(e));
        e.name_own = 1;
        if (!mta_fields(r, e)) { free(e.name); break; }
        v.push_back(e);
    }
    lrm_mta_entry *out;
    if (!lrm_alloc(out, v.size(), "mta", true)) { for (lrm_mta_entry &e : v) free(e.name); return -1; }
    for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
    *mta_out = out;
    return (int) v.size();
}

extern "C" int lrm_host_index_write(const lrm_host_index *idx, const char *genome) {
    const std::string g = genome, cat = g + ".cat";
    const bool ok = lrm_mta_write((g + ".mta").c_str(), idx->mta, idx->mta_len) == 0 && File::write_all(cat, idx->content, idx->con_len) &&
                    lrm_fmi_write(&idx->fmi, cat.c_str()) == 0 && lrm_lc_write((cat + ".lch").c_str(), &idx->lch) == 0 &&
                    lrm_sa5_write((cat + ".sa5").c_str(), idx->sa.mem, idx->sa.len) == 0;
    return ok ? 0 : -1;
}

extern "C" int lrm_host_index_read(const char *genome, lrm_host_index *out) {      // alnmain.c:179-256 (init)
    memset(out, 0, sizeof(*out));
    const std::string g = genome, cat = g + ".cat";
    int64_t n_sa = 0;
    const bool ok = lrm_fmi_read(&out->fmi, cat.c_str()) == 0 && lrm_lc_read((cat + ".lch").c_str(), &out->lch) == 0 &&
                    (out->mta_len = lrm_mta_read((g + ".mta").c_str(), &out->mta)) >= 0 &&
                    File::read_all(cat, out->content, out->con_len) &&
                    lrm_alloc(out->sa.mem, out->con_len, "suffix array") &&
                    (n_sa = lrm_sa5_read((cat + ".sa5").c_str(), out->sa.mem, out->con_len)) >= 0;    // a short .sa5 is accepted
    if (!ok) { lrm_host_index_free(out); return -1; }
    out->sa.start = 0;
    out->sa.len = (uint64_t) n_sa;
    return 0;
}

// FASTA (plain text) records -> names/sequences
static int read_fasta(const char *path, std::vector<std::string> &names, std::vector<std::string> &seqs) {
    File f(path, "rb");
    if (!f.ok()) return -1;
    std::vector<char> line(1 << 16);
    bool have = false;
    while (f.read_line(line.data(), (int) line.size())) {
        size_t l = strlen(line.data());
        bool full = l > 0 && line[l - 1] == '\n';
        while (l > 0 && (line[l - 1] == '\n' || line[l - 1] == '\r')) line[--l] = 0;
        if (line[0] == '>') {
            std::string nm(line.data() + 1);
            size_t sp = nm.find_first_of(" \t");                      // kseq: name ends at first whitespace
            if (sp != std::string::npos) nm.resize(sp);
            names.push_back(nm);
            seqs.emplace_back();
            have = true;
            while (!full && f.read_line(line.data(), (int) line.size())) {  // swallow the rest of a long header
                size_t k = strlen(line.data());
                full = k > 0 && line[k - 1] == '\n';
            }
        } else if (have) {
            seqs.back().append(line.data(), l);
        }
    }
    return 0;
}

extern "C" int lrm_accidx(const char *genome, int o_ratio, int hlen, uint64_t n_seed) {   // asindex.c:129-153
    std::vector<std::string> names, seqs;
    if (read_fasta(genome, names, seqs)) return -1;
    if (seqs.empty()) { lrm_set_error("no FASTA records in %s", genome); return -1; }
    std::vector<const char *> np, sp;
    std::vector<uint64_t> lens;
    for (size_t i = 0; i < seqs.size(); ++i) { np.push_back(names[i].c_str()); sp.push_back(seqs[i].c_str()); lens.push_back(seqs[i].size()); }
    char *cat = nullptr;
    uint64_t L = 0;
    lrm_mta_entry *mta = nullptr;
    if (lrm_cat_from_seqs(np.data(), sp.data(), lens.data(), (int) seqs.size(), n_seed, &cat, &L, &mta)) return -1;
    lrm_host_index idx;
    int rc = lrm_host_index_build(cat, L, mta, (int) seqs.size(), o_ratio, hlen, &idx);
    free(cat);
    lrm_mta_free(mta, (int) seqs.size());
    if (rc) return -1;
    rc = lrm_host_index_write(&idx, genome);
    lrm_host_index_free(&idx);
    return rc;
}
