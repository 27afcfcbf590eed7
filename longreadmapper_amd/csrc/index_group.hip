// index_group.hip -- one handle over several devices (lrm_index_upload_multi / _opt, lrm_index_replicas / _replica)
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <new>
#include <vector>
#include <dlfcn.h>
#include "lrm_hip_util.h"

// ------------------------------------------------------------------------------------------
// multi-GPU group: the image is packed and uploaded once (device devices[0]) and replicated to the other
// devices over xGMI -- one RCCL broadcast when the devices are distinct and librccl is loadable, else
// hipMemcpyPeer (or a plain device copy when a device is listed twice: a logical replica, used by tests on a
// one-GPU box).  Every replica derives its own planar text / long seed table on its device.
// ------------------------------------------------------------------------------------------
namespace {
struct Rccl {
    typedef int (*init_all_t)(void **, int, const int *);
    typedef int (*bcast_t)(const void *, void *, size_t, int, int, void *, hipStream_t);
    typedef int (*group_t)(void);
    typedef int (*destroy_t)(void *);
    typedef const char *(*errstr_t)(int);
    void *lib = nullptr;
    init_all_t init_all = nullptr; bcast_t bcast = nullptr; group_t gstart = nullptr, gend = nullptr; destroy_t destroy = nullptr;
    errstr_t errstr = nullptr;
    bool load() {
        if (getenv("LRM_NO_RCCL")) return false;
        for (const char *name : {"librccl.so.1", "librccl.so"}) { lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
        if (!lib) return false;
        init_all = (init_all_t) dlsym(lib, "ncclCommInitAll"); bcast = (bcast_t) dlsym(lib, "ncclBroadcast");
        gstart = (group_t) dlsym(lib, "ncclGroupStart"); gend = (group_t) dlsym(lib, "ncclGroupEnd");
        destroy = (destroy_t) dlsym(lib, "ncclCommDestroy"); errstr = (errstr_t) dlsym(lib, "ncclGetErrorString");
        return init_all && bcast && gstart && gend && destroy;
    }
};

// ncclBroadcast of the image from devs[0] into bufs[1..] (rccl.h:591; ncclUint8 = 1), in pieces of 256 MiB so
// that RCCL pipelines across the xGMI links.  Returns 1 if RCCL is unavailable (caller falls back), -1 on error.
int rccl_broadcast(const std::vector<int> &devs, const std::vector<void *> &bufs, uint64_t bytes) {
    Rccl r;
    if (!r.load()) return 1;
    const int n = (int) devs.size();
    std::vector<void *> comms((size_t) n, nullptr);
    int rc = r.init_all(comms.data(), n, devs.data());
    if (rc != 0) { lrm_set_error("ncclCommInitAll failed: %s", r.errstr ? r.errstr(rc) : "?"); return -1; }
    std::vector<hipStream_t> st((size_t) n, nullptr);
    int out = 0;
    for (int i = 0; i < n && !out; ++i)
        if (hipSetDevice(devs[i]) != hipSuccess || hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking) != hipSuccess) out = -1;
    const uint64_t piece = 256ull << 20;
    for (uint64_t o = 0; o < bytes && !out; o += piece) {
        const uint64_t l = bytes - o < piece ? bytes - o : piece;
        r.gstart();
        for (int i = 0; i < n; ++i) {
            rc = r.bcast((const char *) bufs[i] + o, (char *) bufs[i] + o, (size_t) l, 1 /* ncclUint8 */, 0, comms[i], st[i]);
            if (rc != 0) out = -1;
        }
        rc = r.gend();
        if (rc != 0) out = -1;
    }
    for (int i = 0; i < n; ++i) {
        if (st[i]) { (void) hipSetDevice(devs[i]); if (hipStreamSynchronize(st[i]) != hipSuccess) out = -1; (void) hipStreamDestroy(st[i]); }
        if (comms[i]) r.destroy(comms[i]);
    }
    if (out) lrm_set_error("RCCL broadcast of the index image failed%s%s", rc ? ": " : "", rc && r.errstr ? r.errstr(rc) : "");
    return out;
}
}  // namespace

extern "C" int lrm_index_upload_multi(lrm_index **out, const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa,
                                      const char *content, uint64_t con_len, const lrm_mta_entry *mta, int mta_len,
                                      const int *devices, int ngpus) {
    return lrm_index_upload_opt(out, fmi, lch, sa, content, con_len, mta, mta_len, devices, ngpus, nullptr);
}
extern "C" int lrm_index_upload_opt(lrm_index **out, const lrm_dna_fmi *fmi, const lrm_lc_hash *lch, const lrm_sa_mem *sa,
                                    const char *content, uint64_t con_len, const lrm_mta_entry *mta, int mta_len,
                                    const int *devices, int ngpus, const lrm_index_options *opt) {
    if (!out || ngpus < 1 || ngpus > 64) { lrm_set_error("bad argument (1 <= ngpus <= 64)"); return -1; }
    std::vector<int> devs((size_t) ngpus);
    for (int i = 0; i < ngpus; ++i) devs[i] = devices ? devices[i] : i;
    lrm_index *root = nullptr;
    if (lrm_index_upload_one(&root, fmi, lch, sa, content, con_len, mta, mta_len, devs[0], opt)) return -1;
    if (ngpus == 1) { *out = root; return 0; }
    const uint64_t bytes = root->blob_bytes;
    std::vector<void *> bufs((size_t) ngpus, nullptr);
    bufs[0] = root->d_blob;
    bool distinct = true;
    for (int i = 0; i < ngpus; ++i) for (int k = 0; k < i; ++k) distinct &= devs[i] != devs[k];
    auto cleanup = [&](int upto) { for (int i = 1; i < upto; ++i) if (bufs[i]) { (void) hipSetDevice(devs[i]); (void) hipFree(bufs[i]); } lrm_index_free(root); };
    for (int i = 1; i < ngpus; ++i) {
        if (lrm_require_device(devs[i]) || hipMalloc(&bufs[i], bytes) != hipSuccess) {
            if (!bufs[i]) lrm_set_error("device %d: cannot allocate the %llu-byte index image", devs[i], (unsigned long long) bytes);
            cleanup(i + 1);
            return -1;
        }
    }
    int rc = distinct ? rccl_broadcast(devs, bufs, bytes) : 1;
    if (rc == 1) {                                     // no RCCL (or logical replicas on one device): peer copies
        rc = 0;
        for (int i = 1; i < ngpus && !rc; ++i) {
            (void) hipSetDevice(devs[i]);
            const hipError_t e = devs[i] == devs[0] ? hipMemcpy(bufs[i], bufs[0], bytes, hipMemcpyDeviceToDevice)
                                                     : hipMemcpyPeer(bufs[i], devs[i], bufs[0], devs[0], bytes);
            if (e != hipSuccess) { lrm_set_error("replication of the index image to device %d failed: %s", devs[i], hipGetErrorString(e)); rc = -1; }
        }
    }
    if (rc) { cleanup(ngpus); return -1; }
    root->peers = new (std::nothrow) lrm_index *[(size_t) ngpus];
    if (!root->peers) { cleanup(ngpus); lrm_set_error("out of memory"); return -1; }
    root->peers[0] = root;
    root->n_peers = 1;
    for (int i = 1; i < ngpus; ++i) {
        lrm_index *rep = nullptr;
        if (lrm_require_device(devs[i]) || lrm_index_make_handle(&rep, bufs[i], bytes, devs[i], 1, root->hdr, opt)) {
            for (int k = i; k < ngpus; ++k) { (void) hipSetDevice(devs[k]); (void) hipFree(bufs[k]); }
            lrm_index_free(root);                  // frees the replicas made so far
            return -1;
        }
        root->peers[i] = rep;
        root->n_peers = i + 1;
    }
    *out = root;
    return 0;
}

// Test tap: the RCCL path of lrm_index_upload_multi on ONE device -- dlopen of librccl, ncclCommInitAll, a grouped
// ncclBroadcast of `bytes` bytes on a 1-rank communicator, teardown.  A one-GPU box cannot run the multi-device
// broadcast itself; this checks that the library loads and that the calls are bound with the right signatures.
// Returns 0 ok, 1 RCCL not loadable (the multi-GPU upload then falls back to hipMemcpyPeer), -1 error.
extern "C" int lrm_debug_rccl_selftest(int device, uint64_t bytes) {
    if (lrm_require_device(device)) return -1;
    void *d = nullptr;
    if (hipMalloc(&d, bytes ? bytes : 1) != hipSuccess) { lrm_set_error("hipMalloc failed"); return -1; }
    std::vector<uint8_t> h(bytes ? bytes : 1);
    for (size_t i = 0; i < h.size(); ++i) h[i] = (uint8_t) (i * 131u + 7u);
    int rc = hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
    if (rc == 0) rc = rccl_broadcast(std::vector<int>{device}, std::vector<void *>{d}, (uint64_t) h.size());
    std::vector<uint8_t> back(h.size());
    if (rc == 0 && hipMemcpy(back.data(), d, h.size(), hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
    if (rc == 0 && back != h) { lrm_set_error("RCCL self-test: buffer changed by a 1-rank broadcast"); rc = -1; }
    (void) hipFree(d);
    return rc;
}

extern "C" int lrm_index_replicas(const lrm_index *idx) { return idx ? idx->n_peers : 0; }
extern "C" lrm_index *lrm_index_replica(lrm_index *idx, int r) {
    if (!idx || r < 0 || r >= idx->n_peers) return nullptr;
    return idx->peers ? idx->peers[r] : idx;
}
