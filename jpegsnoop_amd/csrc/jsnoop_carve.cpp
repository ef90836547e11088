// jsnoop_carve.cpp -- jsnoop_carve_*: every embedded JPEG of a byte blob as a table of frames (kernels: jsnoop_carve.hip; checks, sizes, the walk and the
// parent pass: jsnoop_carve_check.h).  A carve owns its stream, its page-locked staging and its scratch; it is independent of batches and jobs.
#include <stdio.h>
#include <vector>
#include "jsnoop_host.h"
#include "jsnoop_launch.h"
#include "jsnoop_carve_check.h"

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    js_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

#define CARVE_STAGE_HALF ((size_t)8 << 20)     /* bytes of one half of the page-locked staging: a copy into one half runs under the transfer of the other */

struct JsnoopCarve {
    int device = 0; hipStream_t stream = nullptr; hipEvent_t ev[2] = { nullptr, nullptr };
    uint8_t* h_stage = nullptr; unsigned long long* h_tot = nullptr;
    uint8_t* d_copy = nullptr;  size_t d_copy_cap = 0;             // a host blob's copy
    uint8_t* d_counts = nullptr; size_t d_counts_cap = 0;
    uint8_t* d_term = nullptr;  size_t d_term_cap = 0;
    uint8_t* d_cand = nullptr;  size_t d_cand_cap = 0;
    uint8_t* d_recs = nullptr;  size_t d_recs_cap = 0;
    std::vector<JsCarveRec> recs; std::vector<int32_t> parent; uint64_t nterm = 0, ncand = 0;

    int run(const JsnoopCarveSpec& spec, const void* blob, uint64_t len, int where);
    int upload(const uint8_t* src, size_t len);
    int download(void* dst, const uint8_t* src, size_t len);
};

static int carve_grow(uint8_t** p, size_t* cap, size_t need)
{
    if (need <= *cap) return 0;                                  // (hipFree waits for the device: no earlier call still uses the old block)
    if (*p) hipFree(*p);
    *p = nullptr; *cap = 0;
    HIP_TRY(hipMalloc((void**)p, need + 256));
    *cap = need + 256;
    return 0;
}

int JsnoopCarve::upload(const uint8_t* src, size_t len)
{
    size_t k = 0;
    for (size_t off = 0; off < len; off += CARVE_STAGE_HALF, k++) {
        const size_t m = len - off < CARVE_STAGE_HALF ? len - off : CARVE_STAGE_HALF; const int half = (int)(k & 1u);
        if (k >= 2) HIP_TRY(hipEventSynchronize(ev[half]));
        memcpy(h_stage + half * CARVE_STAGE_HALF, src + off, m);
        HIP_TRY(hipMemcpyAsync(d_copy + off, h_stage + half * CARVE_STAGE_HALF, m, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(ev[half], stream));
    }
    return 0;
}
int JsnoopCarve::download(void* dst, const uint8_t* src, size_t len)
{
    for (size_t off = 0; off < len; off += 2 * CARVE_STAGE_HALF) {
        const size_t m = len - off < 2 * CARVE_STAGE_HALF ? len - off : 2 * CARVE_STAGE_HALF;
        HIP_TRY(hipMemcpyAsync(h_stage, src + off, m, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        memcpy(static_cast<uint8_t*>(dst) + off, h_stage, m);
    }
    return 0;
}

// Two waits: behind k_carve_count + k_carve_scan the totals come back (wait 1) and size the lists; behind k_carve_emit + k_carve_walk the records come back (wait 2).
int JsnoopCarve::run(const JsnoopCarveSpec& spec, const void* blob, uint64_t len, int where)
{
    HIP_TRY(hipSetDevice(device));
    if (where == 1 && len) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, blob) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != device) {
            (void)hipGetLastError(); js_set_error("carve: where = 1, but the blob is not memory of device %d", device); return -1; }
    }
    uint64_t budget = spec.max_scratch_bytes;
    if (!budget) { size_t free_b = 0, total_b = 0; HIP_TRY(hipMemGetInfo(&free_b, &total_b)); budget = (uint64_t)free_b / 2; }
    const uint32_t head = where == 1 ? (uint32_t)(reinterpret_cast<uintptr_t>(blob) & 15u) : 0u;
    const uint32_t tiles = (uint32_t)js_carve_tiles(len, head);
    if (js_carve_check_budget(js_carve_sizes(len, head, 0, 0, where), budget)) return -1;
    const uint8_t* base = static_cast<const uint8_t*>(blob) - head;
    if (where == 0 && len) {
        if (carve_grow(&d_copy, &d_copy_cap, (size_t)len) || upload(static_cast<const uint8_t*>(blob), (size_t)len)) return -1;
        base = d_copy;
    }
    if (carve_grow(&d_counts, &d_counts_cap, (size_t)tiles * 16u + 16u)) return -1;
    uint32_t* counts = reinterpret_cast<uint32_t*>(d_counts);
    if (js_launch_carve_count(stream, base, head, len, tiles, counts)) { js_set_error("carve: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    HIP_TRY(hipMemcpyAsync(h_tot, counts + 4u * (size_t)tiles, 16, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));                                                           // ---- wait 1
    const uint64_t nt = h_tot[0], nc = h_tot[1];
    if (nt > len || nc > nt) { js_set_error("carve: the count came back with %llu terminators and %llu candidates in %llu bytes", (unsigned long long)nt, (unsigned long long)nc, (unsigned long long)len); return -1; }
    const JsCarveSizes sz = js_carve_sizes(len, head, nt, nc, where);
    if (js_carve_check_budget(sz, budget)) return -1;
    std::vector<JsCarveRec> got((size_t)nc);
    if (nt) {
        if (carve_grow(&d_term, &d_term_cap, (size_t)sz.term_list) || carve_grow(&d_cand, &d_cand_cap, (size_t)sz.cand_list) || carve_grow(&d_recs, &d_recs_cap, (size_t)sz.recs)) return -1;
        if (js_launch_carve_walk(stream, base, head, len, tiles, counts, (uint32_t)nt, (uint32_t)nc, spec.max_markers, reinterpret_cast<uint32_t*>(d_term),
                                 reinterpret_cast<uint32_t*>(d_cand), reinterpret_cast<uint32_t*>(d_recs))) {
            js_set_error("carve: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
        if (nc) { if (download(got.data(), d_recs, (size_t)sz.recs)) return -1; }                    // ---- wait 2
        else HIP_TRY(hipStreamSynchronize(stream));
    }
    recs.swap(got); nterm = nt; ncand = nc;
    js_carve_parents(recs.data(), recs.size(), &parent);
    return 0;
}

extern "C" {

void jsnoop_carve_spec_defaults(JsnoopCarveSpec* out) { if (out) js_carve_spec_defaults(out); }

JsnoopCarve* jsnoop_carve_create(int device)
{
    const int n = jsnoop_device_count();
    if (n <= 0) { js_set_error("no HIP device visible: libjsnoop_gpu has no CPU fallback"); return nullptr; }
    if (device < 0 || device >= n) { js_set_error("jsnoop_carve_create: device %d not available (%d visible)", device, n); return nullptr; }
    JsnoopCarve* c = new JsnoopCarve; c->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipEventCreateWithFlags(&c->ev[k], hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_stage, 2 * CARVE_STAGE_HALF, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void**)&c->h_tot, 64, hipHostMallocDefault);
    if (e != hipSuccess) { js_set_error("jsnoop_carve_create: %s", hipGetErrorString(e)); jsnoop_carve_destroy(c); return nullptr; }
    return c;
}
void jsnoop_carve_destroy(JsnoopCarve* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (uint8_t* p : { c->d_copy, c->d_counts, c->d_term, c->d_cand, c->d_recs }) if (p) (void)hipFree(p);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->h_tot) (void)hipHostFree(c->h_tot);
    for (hipEvent_t e : c->ev) if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}
int jsnoop_carve_run(JsnoopCarve* c, const JsnoopCarveSpec* spec_in, const void* blob, uint64_t len, int where)
{
    if (!c) { js_set_error("carve: carve is NULL"); return -1; }
    JsnoopCarveSpec spec;
    if (js_carve_import_spec(spec_in, &spec) || js_carve_check_blob(blob, len, where)) return -1;
    return c->run(spec, blob, len, where);
}
int64_t jsnoop_carve_host(const JsnoopCarveSpec* spec_in, const void* blob, uint64_t len, JsnoopCarveFrame* frames, uint64_t cap)
{
    JsnoopCarveSpec spec;
    if (js_carve_import_spec(spec_in, &spec) || js_carve_check_blob(blob, len, 0)) return -1;
    if (cap && !frames) { js_set_error("carve_host: frames is NULL"); return -1; }
    std::vector<uint32_t> term, cand; std::vector<JsCarveRec> recs; std::vector<int32_t> parent;
    js_carve_host_table(static_cast<const uint8_t*>(blob), len, spec.max_markers, &term, &cand, &recs);
    js_carve_parents(recs.data(), recs.size(), &parent);
    for (size_t k = 0; k < recs.size() && k < cap; k++) js_carve_frame_of(recs[k], parent[k], &frames[k]);
    return (int64_t)recs.size();
}
int64_t jsnoop_carve_count(const JsnoopCarve* c) { return c ? (int64_t)c->recs.size() : 0; }
int jsnoop_carve_frame(const JsnoopCarve* c, int64_t k, JsnoopCarveFrame* out)
{
    if (!c) { js_set_error("carve_frame: carve is NULL"); return -1; }
    if (k < 0 || (uint64_t)k >= c->recs.size()) { js_set_error("carve_frame: frame %lld out of range, the last run found %zu", (long long)k, c->recs.size()); return -1; }
    return js_carve_export_frame(c->recs[(size_t)k], c->parent[(size_t)k], out);
}
int64_t jsnoop_carve_frames(const JsnoopCarve* c, JsnoopCarveFrame* out, uint64_t cap)
{
    if (!c) { js_set_error("carve_frames: carve is NULL"); return -1; }
    if (cap && !out) { js_set_error("carve_frames: out is NULL"); return -1; }
    size_t k = 0;
    for (; k < c->recs.size() && k < cap; k++) js_carve_frame_of(c->recs[k], c->parent[k], &out[k]);
    return (int64_t)k;
}
const void* jsnoop_carve_frames_dev(const JsnoopCarve* c) { return c && c->ncand ? c->d_recs : nullptr; }
int jsnoop_carve_lists_dev(const JsnoopCarve* c, const uint32_t** terminators, const uint32_t** candidates)
{
    if (!c) { js_set_error("carve_lists_dev: carve is NULL"); return -1; }
    if (terminators) *terminators = c->nterm ? reinterpret_cast<const uint32_t*>(c->d_term) : nullptr;
    if (candidates) *candidates = c->ncand ? reinterpret_cast<const uint32_t*>(c->d_cand) : nullptr;
    return 0;
}
int jsnoop_carve_totals(const JsnoopCarve* c, uint64_t* terminators, uint64_t* candidates)
{
    if (!c) { js_set_error("carve_totals: carve is NULL"); return -1; }
    if (terminators) *terminators = c->nterm;
    if (candidates) *candidates = c->ncand;
    return 0;
}
int64_t jsnoop_carve_copy(JsnoopCarve* c, int what, void* dev_dst, uint64_t cap)
{
    if (!c) { js_set_error("carve_copy: carve is NULL"); return -1; }
    if (what < 0 || what > 2) { js_set_error("carve_copy: what = %d, 0 records, 1 terminators, 2 candidates", what); return -1; }
    const uint8_t* src = what == 0 ? c->d_recs : (what == 1 ? c->d_term : c->d_cand);
    const uint64_t bytes = what == 0 ? c->ncand * sizeof(JsCarveRec) : (what == 1 ? c->nterm : c->ncand) * 4u;
    if (!bytes) return 0;
    if (!dev_dst) { js_set_error("carve_copy: dev_dst is NULL"); return -1; }
    if (cap < bytes) { js_set_error("carve_copy: cap %llu is below the %llu bytes to copy", (unsigned long long)cap, (unsigned long long)bytes); return -1; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(dev_dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return (int64_t)bytes;
}

} // extern "C"
