// jsnoop_planes.cpp -- jsnoop_batch_pack_planes and its helpers: the retained int16 planes of a decoded batch into caller-owned device memory, one tensor per
// component (kernel: jsnoop_planes.hip; checks and records: jsnoop_plane_check.h).
#include "jsnoop_host.h"
#include "jsnoop_launch.h"
#include "jsnoop_plane_check.h"

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    js_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

// The pack's block, event and place on the batch stream: one H2D copy of the call's records, one launch, nothing waited for.
// Never decodes: the planes are what the decode enqueued last left, whichever form it took.
int JsnoopBatch::pack_planes(const JsnoopPlaneSpec* spec_in, const int* images, int n, const JsnoopPlaneDst* dst)
{
    if (!uploaded || last_form == 0 || !dev.imgs) { js_set_error("pack_planes: the batch has not been decoded"); return -1; }
    if (!opt_want_planes || !dev.planes) { js_set_error("pack_planes: the batch keeps no planes (want_planes)"); return -1; }
    JsnoopPlaneSpec spec;
    if (js_plane_import_spec(spec_in, &spec)) return -1;
    if (n < 0) { js_set_error("pack_planes: n = %d", n); return -1; }
    if (n == 0) return 0;
    if (!dst) { js_set_error("pack_planes: dst is NULL"); return -1; }
    HIP_TRY(hipSetDevice(device));
    const size_t rec_bytes = ((size_t)n * sizeof(JsPlaneRec) + 15) & ~(size_t)15, total = rec_bytes + ((size_t)n + 1) * 4;
    if (pack_block(total)) return -1;
    JsPlaneRec* recs = reinterpret_cast<JsPlaneRec*>(h_pack); uint32_t* base = reinterpret_cast<uint32_t*>(h_pack + rec_bytes);
    if (js_plane_plan(imgs.data(), imgs.size(), spec, images, n, dst, recs, base)) return -1;
    if (pack_send(total)) return -1;
    JsPlaneArgs a;
    for (int c = 0; c < 3; c++) { a.scale[c] = spec.scale[c]; a.bias[c] = spec.bias[c]; }
    if (js_launch_pack_planes(stream, dev.planes, reinterpret_cast<const JsPlaneRec*>(d_pack), reinterpret_cast<const uint32_t*>(d_pack + rec_bytes),
                              (uint32_t)n, base[n], spec.dtype, a)) {
        js_set_error("pack_planes: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    return 0;
}

extern "C" {

void jsnoop_plane_spec_defaults(JsnoopPlaneSpec* out) { if (out) js_plane_spec_defaults(out); }
int jsnoop_batch_plane_size(const JsnoopBatch* b, const JsnoopPlaneSpec* spec_in, int i, int comp, unsigned* w, unsigned* h)
{
    JsnoopPlaneSpec spec;
    if (!b) { js_set_error("pack_planes: batch is NULL"); return -1; }
    if (js_plane_import_spec(spec_in, &spec)) return -1;
    if (i < 0 || (size_t)i >= b->imgs.size()) { js_set_error("pack_planes: image index %d out of range, the batch holds %zu", i, b->imgs.size()); return -1; }
    uint32_t ow = 0, oh = 0;
    if (js_plane_size(b->imgs[i], spec, comp, &ow, &oh, nullptr, nullptr)) return -1;
    if (w) *w = ow;
    if (h) *h = oh;
    return 0;
}
uint64_t jsnoop_batch_plane_bytes(const JsnoopBatch* b, const JsnoopPlaneSpec* spec_in, int i, int comp)
{
    JsnoopPlaneSpec spec; unsigned w = 0, h = 0;
    if (!b) { js_set_error("pack_planes: batch is NULL"); return 0; }
    if (js_plane_import_spec(spec_in, &spec) || jsnoop_batch_plane_size(b, spec_in, i, comp, &w, &h)) return 0;
    return js_plane_dense_bytes(w, h, spec);
}
int jsnoop_batch_pack_planes(JsnoopBatch* b, const JsnoopPlaneSpec* spec, const int* images, int n, const JsnoopPlaneDst* dst)
{
    if (!b) { js_set_error("pack_planes: batch is NULL"); return -1; }
    return b->pack_planes(spec, images, n, dst);
}

} // extern "C"
