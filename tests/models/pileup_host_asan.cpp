// pileup_host_asan.cpp -- a stand-alone program (its own main, never loaded into Python) over the host code of the pileup on
// the host-buffer path (docs/GACT_SPEC.md, "Pileup on the host-buffer path and across replicas"): lrm_pileup_sites_format_ins on
// tables and output buffers that sit in heap blocks of exactly their size, for every buffer size from one byte up to the
// text's own, and the refusals of lrm_accaln_pileup, which return before a device is touched.  It needs no GPU.  Build the
// library and the program with the sanitizers and run the program directly:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -shared -fopenmp -Xarch_host -fsanitize=address,undefined -Iinclude \
//         longreadmapper_amd/csrc/*.hip longreadmapper_amd/csrc/{suffix_sort,index_build,index_files,fastq_reader,sam_text,paf_text,pileup_text,accaln_flow}.cpp \
//         -lz -ldl -o <dir>/liblrm_accel_asan.so
//   <the clang++ that hipcc drives> -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude tests/models/pileup_host_asan.cpp \
//         -L<dir> -llrm_accel_asan -Wl,-rpath,<dir> -o <dir>/pileup_host_asan        (one compiler: one sanitizer runtime)
//   LSAN_OPTIONS=suppressions=<a file with the line "leak:libomp.so"> <dir>/pileup_host_asan <an empty scratch directory>
//
// Exit status 0 and "ok" on the last line: every check held and no sanitizer spoke.  (The suppression: the OpenMP runtime
// keeps 128 bytes of its own until the process ends.)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <sys/stat.h>
#include "lrm_accel.h"
#include "lrm_index_host.h"
#include "lrm_io_host.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, lrm_last_error()); ++failures; } } while (0)

// a heap block of exactly n elements (one stands for none: nothing of it is touched)
template <typename T>
static T *exact(const std::vector<T> &v) {
    T *p = (T *) malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

static bool exists(const std::string &path) { struct stat st; return stat(path.c_str(), &st) == 0; }

static void format_checks() {
    char name0[] = "first sequence", name1[] = "b";
    lrm_mta_entry mta[2];
    memset(mta, 0, sizeof(mta));
    mta[0].name = name0; mta[0].name_len = strlen(name0); mta[0].offset = 7; mta[0].seq_len = 700;
    mta[1].name = name1; mta[1].name_len = 1; mta[1].offset = 1000; mta[1].seq_len = 61;
    const uint64_t pos[] = {7, 8, 350, 706, 1000, 1030, 1060};                  // the first and the last base of either sequence
    const uint8_t lens[] = {0, 1, 8, 3};
    std::vector<lrm_pileup_site> sites;
    std::vector<lrm_pileup_ins_allele> alleles;
    std::string want;
    for (unsigned k = 0; k < sizeof(pos) / sizeof(pos[0]); ++k) {
        lrm_pileup_site s;
        memset(&s, 0, sizeof(s));
        s.pos = pos[k]; s.depth = 4000000000u - k; s.n_ref = 30 + k; s.n_alt = k; s.n_del = 2 * k; s.n_ins = 4294967295u;
        s.ref = "ACGTn"[k % 5]; s.alt = "TGCA."[k % 5]; s.cons = "ACGT-N"[k % 6]; s.kinds = (uint8_t) (1 + k % 7);
        sites.push_back(s);
        lrm_pileup_ins_allele a;
        memset(&a, 0, sizeof(a));
        a.len = lens[k % 4]; a.n_col0 = 7 * k; a.flags = (uint8_t) (k % 4);
        memcpy(a.bases, "GATTACAT", a.len);
        alleles.push_back(a);
        // the line, spelled out here
        const lrm_mta_entry &m = pos[k] >= 1000 ? mta[1] : mta[0];
        char head[256];
        std::string kinds;
        if (s.kinds & LRM_CALL_SNV) kinds += 'S';
        if (s.kinds & LRM_CALL_DEL) kinds += 'D';
        if (s.kinds & LRM_CALL_INS) kinds += 'I';
        snprintf(head, sizeof(head), "%s\t%llu\t%c\t%c\t%s\t%u\t%u\t%u\t%u\t%u\t%c\t", m.name, (unsigned long long) (pos[k] - m.offset + 1), s.ref, s.alt,
                 kinds.c_str(), s.depth, s.n_ref, s.n_alt, s.n_del, s.n_ins, s.cons);
        want += head;
        want += a.len ? std::string("GATTACAT", a.len) : std::string(".");
        want += '\n';
    }
    lrm_pileup_site *hs = exact(sites);
    lrm_pileup_ins_allele *ha = exact(alleles);
    const uint64_t n = sites.size();
    // every buffer size: the text, or -2 with nothing behind the buffer touched
    int fitted = 0, refused = 0;
    for (int64_t room = 1; room <= (int64_t) want.size() + 200; ++room) {
        char *buf = (char *) malloc((size_t) room);
        const int64_t k = lrm_pileup_sites_format_ins(mta, 2, hs, ha, n, buf, room);
        if (k >= 0) { CHECK(k == (int64_t) want.size() && k < room && memcmp(buf, want.data(), (size_t) k) == 0 && buf[k] == '\0'); ++fitted; }
        else { CHECK(k == -2 && room <= (int64_t) want.size() + 200); ++refused; }
        free(buf);
    }
    CHECK(fitted > 0 && refused > 0);
    // NULL alleles: lrm_pileup_sites_format, byte for byte
    std::vector<char> a(want.size() + 256), b(want.size() + 256);
    const int64_t ka = lrm_pileup_sites_format_ins(mta, 2, hs, nullptr, n, a.data(), (int64_t) a.size());
    const int64_t kb = lrm_pileup_sites_format(mta, 2, hs, n, b.data(), (int64_t) b.size());
    CHECK(ka > 0 && ka == kb && memcmp(a.data(), b.data(), (size_t) ka) == 0 && ka < (int64_t) want.size());
    // no record, a position in no sequence, null arguments
    CHECK(lrm_pileup_sites_format_ins(mta, 2, nullptr, nullptr, 0, a.data(), 1) == 0 && a[0] == '\0');
    hs[n - 1].pos = 5000;
    CHECK(lrm_pileup_sites_format_ins(mta, 2, hs, ha, n, a.data(), (int64_t) a.size()) == -1);
    CHECK(lrm_pileup_sites_format_ins(mta, 2, nullptr, ha, n, a.data(), (int64_t) a.size()) == -1);
    CHECK(lrm_pileup_sites_format_ins(nullptr, 2, hs, ha, n, a.data(), (int64_t) a.size()) == -1);
    free(hs);
    free(ha);
}

static void refusal_checks(const std::string &dir) {
    const std::string fa = dir + "/ref.fa", fq = dir + "/reads.fq", sam = dir + "/out.sam", tsv = dir + "/sites.tsv", cfa = dir + "/cons.fa";
    FILE *f = fopen(fa.c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write into %s\n", dir.c_str()); ++failures; return; }
    uint32_t x = 12345;
    for (int s = 0; s < 2; ++s) {
        fprintf(f, ">seq%d\n", s);
        for (int i = 0; i < 3000; ++i) { x = x * 1664525u + 1013904223u; fputc("ACGT"[x >> 30], f); if (i % 60 == 59) fputc('\n', f); }
    }
    fclose(f);
    f = fopen(fq.c_str(), "wb");
    fprintf(f, "@r0\nACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIII\n");
    fclose(f);
    CHECK(lrm_accidx(fa.c_str(), 32, 6, 1) == 0);
    const lrm_params p = {64, 20, 300};
    const lrm_gact_params gp = {0, 0, 0};
    struct Case { const char *what; uint32_t struct_size, ins_cols, min_mapq, reserved, min_pct, call_reserved; int32_t seq; uint32_t reserved2; int mapq; const char *text; };
    const uint32_t full = (uint32_t) sizeof(lrm_accaln_pileup_options);
    const Case cases[] = {
        {"min_mapq without mapq", full, 0, 1, 0, 0, 0, -1, 0, 0, "min_mapq needs mapq"},
        {"reserved", full, 0, 0, 1, 0, 0, -1, 0, 1, "reserved"},
        {"reserved2", full, 0, 0, 0, 0, 0, -1, 9, 1, "reserved"},
        {"call.reserved", full, 0, 0, 0, 0, 3, -1, 0, 1, "reserved"},
        {"seq == mta_len", full, 0, 0, 0, 0, 0, 2, 0, 1, "seq 2"},
        {"seq == -2", full, 0, 0, 0, 0, 0, -2, 0, 0, "seq -2"},
        {"ins_cols", full, 9, 0, 0, 0, 0, 0, 0, 0, "insertion columns"},
        {"min_pct", full, 0, 0, 0, 101, 0, 0, 0, 0, "min_pct"},
        {"struct_size", full - 8, 0, 0, 0, 0, 0, 0, 0, 0, "struct_size"},
    };
    for (const Case &c : cases) {
        for (int with_sam = 0; with_sam < 2; ++with_sam) {
            lrm_accaln_pileup_options po;
            memset(&po, 0, sizeof(po));
            po.struct_size = c.struct_size; po.ins_cols = c.ins_cols; po.min_mapq = c.min_mapq; po.reserved = c.reserved;
            po.call.min_pct = c.min_pct; po.call.reserved = c.call_reserved; po.seq = c.seq; po.reserved2 = c.reserved2;
            po.sites_path = tsv.c_str(); po.fasta_path = cfa.c_str();
            uint64_t total = 77, valid = 77;
            const int rc = lrm_accaln_pileup(fa.c_str(), fq.c_str(), with_sam ? sam.c_str() : nullptr, p, gp, 0, 1, &total, &valid, nullptr, c.mapq, &po);
            if (rc != -1 || !strstr(lrm_last_error(), c.text)) { fprintf(stderr, "%s: rc %d, \"%s\"\n", c.what, rc, lrm_last_error()); ++failures; }
            CHECK(!exists(sam) && !exists(tsv) && !exists(cfa));
        }
    }
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]); return 2; }
    format_checks();
    refusal_checks(argv[1]);
    if (failures) printf("%d checks failed\n", failures);
    else printf("ok\n");
    return failures ? 1 : 0;
}
