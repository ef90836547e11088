// jsnoop_pack.cpp -- jsnoop_batch_pack and jsnoop_batch_pack_resized: the last stage, DIBs of a decoded batch into caller-owned device memory
// (kernels: jsnoop_pack.hip, jsnoop_pack_resize.hip).
#include "jsnoop_host.h"
#include "jsnoop_launch.h"
#include "jsnoop_pack_check.h"

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    js_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

// h_pack may be rewritten once the copy of the call before this one has read it; it grows by a quarter beyond what is asked for
int JsnoopBatch::pack_block(size_t total)
{
    if (!ev_pack) HIP_TRY(hipEventCreateWithFlags(&ev_pack, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(ev_pack));
    if (total > h_pack_cap) {
        if (h_pack) hipHostFree(h_pack);
        h_pack = nullptr; h_pack_cap = 0;
        HIP_TRY(hipHostMalloc((void**)&h_pack, total + total / 4 + 4096, hipHostMallocDefault));
        h_pack_cap = total + total / 4 + 4096;
    }
    return 0;
}
int JsnoopBatch::pack_send(size_t total)
{
    if (total > d_pack_cap) {                                    // (hipFree waits for the device: no earlier pack still reads the old block)
        if (d_pack) hipFree(d_pack);
        d_pack = nullptr; d_pack_cap = 0;
        HIP_TRY(hipMalloc((void**)&d_pack, h_pack_cap));
        d_pack_cap = h_pack_cap;
    }
    HIP_TRY(hipMemcpyAsync(d_pack, h_pack, total, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(ev_pack, stream));
    return 0;
}

// One H2D copy of the call's records, one launch, both on the batch stream: behind whatever decode was enqueued last (a two-stream decode joins this
// stream before decode() returns; a progressive one runs on it).  Nothing waits.
int JsnoopBatch::pack(const JsnoopPackSpec* spec_in, const int* images, int n, const JsnoopPackDst* dst)
{
    if (!uploaded || last_form == 0 || !dev.dib || !dev.imgs) { js_set_error("pack: the batch has not been decoded"); return -1; }
    JsnoopPackSpec spec;
    if (js_pack_import_spec(spec_in, &spec)) return -1;
    if (n < 0) { js_set_error("pack: n = %d", n); return -1; }
    if (n == 0) return 0;
    if (!dst) { js_set_error("pack: dst is NULL"); return -1; }
    HIP_TRY(hipSetDevice(device));
    const size_t rec_bytes = ((size_t)n * sizeof(JsPackRec) + 15) & ~(size_t)15, total = rec_bytes + ((size_t)n + 1) * 4;
    if (pack_block(total)) return -1;
    JsPackRec* recs = reinterpret_cast<JsPackRec*>(h_pack); uint32_t* base = reinterpret_cast<uint32_t*>(h_pack + rec_bytes);
    if (js_pack_plan(imgs.data(), imgs.size(), spec, images, n, dst, recs, base)) return -1;
    if (pack_send(total)) return -1;
    JsPackArgs a; a.bgr = spec.bgr != 0;
    for (int c = 0; c < 3; c++) { a.scale[c] = spec.scale[c]; a.bias[c] = spec.bias[c]; }
    if (js_launch_pack_rgb(stream, dev.imgs, dev.dib, reinterpret_cast<const JsPackRec*>(d_pack), reinterpret_cast<const uint32_t*>(d_pack + rec_bytes),
                           (uint32_t)n, base[n], spec.layout, spec.dtype, a)) {
        js_set_error("pack: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    return 0;
}

// The same block, the same event, the same place on the batch stream; the records carry output size and ROI, the kernel is k_pack_resize.
int JsnoopBatch::pack_resized(const JsnoopPackSpec* spec_in, int filter, const int* images, int n, const JsnoopResizeDst* dst)
{
    if (!uploaded || last_form == 0 || !dev.dib || !dev.imgs) { js_set_error("pack_resized: the batch has not been decoded"); return -1; }
    JsnoopPackSpec spec;
    if (js_pack_import_spec(spec_in, &spec, "pack_resized") || js_resize_check_filter(filter)) return -1;
    if (n < 0) { js_set_error("pack_resized: n = %d", n); return -1; }
    if (n == 0) return 0;
    if (!dst) { js_set_error("pack_resized: dst is NULL"); return -1; }
    HIP_TRY(hipSetDevice(device));
    const size_t rec_bytes = ((size_t)n * sizeof(JsResizeRec) + 15) & ~(size_t)15, total = rec_bytes + ((size_t)n + 1) * 4;
    if (pack_block(total)) return -1;
    JsResizeRec* recs = reinterpret_cast<JsResizeRec*>(h_pack); uint32_t* base = reinterpret_cast<uint32_t*>(h_pack + rec_bytes);
    if (js_resize_plan(imgs.data(), imgs.size(), spec, images, n, dst, recs, base)) return -1;
    if (pack_send(total)) return -1;
    JsPackArgs a; a.bgr = spec.bgr != 0;
    for (int c = 0; c < 3; c++) { a.scale[c] = spec.scale[c]; a.bias[c] = spec.bias[c]; }
    if (js_launch_pack_resize(stream, dev.imgs, dev.dib, reinterpret_cast<const JsResizeRec*>(d_pack), reinterpret_cast<const uint32_t*>(d_pack + rec_bytes),
                              (uint32_t)n, base[n], filter, spec.layout, spec.dtype, a)) {
        js_set_error("pack_resized: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    return 0;
}

extern "C" {

void jsnoop_pack_spec_defaults(JsnoopPackSpec* out) { if (out) js_pack_spec_defaults(out); }
uint64_t jsnoop_batch_pack_bytes(const JsnoopBatch* b, const JsnoopPackSpec* spec_in, int i)
{
    JsnoopPackSpec spec;
    if (!b) { js_set_error("pack: batch is NULL"); return 0; }
    if (js_pack_import_spec(spec_in, &spec)) return 0;
    if (i < 0 || (size_t)i >= b->imgs.size()) { js_set_error("pack: image index %d out of range, the batch holds %zu", i, b->imgs.size()); return 0; }
    return js_pack_dense_bytes(b->imgs[i], spec);
}
int jsnoop_batch_device(const JsnoopBatch* b) { return b ? b->device : -1; }
int jsnoop_batch_pack(JsnoopBatch* b, const JsnoopPackSpec* spec, const int* images, int n, const JsnoopPackDst* dst)
{
    if (!b) { js_set_error("pack: batch is NULL"); return -1; }
    return b->pack(spec, images, n, dst);
}
int jsnoop_batch_pack_resized(JsnoopBatch* b, const JsnoopPackSpec* spec, int filter, const int* images, int n, const JsnoopResizeDst* dst)
{
    if (!b) { js_set_error("pack_resized: batch is NULL"); return -1; }
    return b->pack_resized(spec, filter, images, n, dst);
}

} // extern "C"
