// jsnoop_render.cpp -- jsnoop_batch_pack_ijg and jsnoop_batch_ijg_renderable: the coefficient arena of a decoded batch rendered as libjpeg's pixels into
// caller-owned device memory (kernel: jsnoop_render.hip; checks, records and the arithmetic: jsnoop_render_check.h).
#include "jsnoop_host.h"
#include "jsnoop_launch.h"
#include "jsnoop_render_check.h"

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    js_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

// The pack's block, event and place on the batch stream: one H2D copy of the call's records, one launch, nothing waited for -- except behind a DC-only fast-form
// decode, whose arena does not hold the blocks: the batch is then decoded once more in the generic form (ensure_generic, as jsnoop_batch_pack_coefs does), after
// every argument has passed its checks.  No other decode-side state is touched.
int JsnoopBatch::pack_ijg(const JsnoopPackSpec* spec_in, const int* images, int n, const JsnoopPackDst* dst)
{
    if (!uploaded || last_form == 0 || !dev.coef || !dev.dccum || !dev.imgs) { js_set_error("pack_ijg: the batch has not been decoded"); return -1; }
    JsnoopPackSpec spec;
    if (js_pack_import_spec(spec_in, &spec, "pack_ijg")) return -1;
    if (n < 0) { js_set_error("pack_ijg: n = %d", n); return -1; }
    if (n == 0) return 0;
    if (!dst) { js_set_error("pack_ijg: dst is NULL"); return -1; }
    HIP_TRY(hipSetDevice(device));
    const size_t rec_bytes = ((size_t)n * sizeof(JsRenRec) + 15) & ~(size_t)15, total = rec_bytes + ((size_t)n + 1) * 4;
    if (pack_block(total)) return -1;
    JsRenRec* recs = reinterpret_cast<JsRenRec*>(h_pack); uint32_t* base = reinterpret_cast<uint32_t*>(h_pack + rec_bytes);
    if (js_ren_plan(imgs.data(), imgs.size(), spec, images, n, dst, recs, base)) return -1;
    if (ensure_generic()) return -1;
    if (pack_send(total)) return -1;
    JsPackArgs a; a.bgr = spec.bgr != 0;
    for (int c = 0; c < 3; c++) { a.scale[c] = spec.scale[c]; a.bias[c] = spec.bias[c]; }
    if (js_launch_render_ijg(stream, dev.coef, dev.dccum, reinterpret_cast<const JsRenRec*>(d_pack), reinterpret_cast<const uint32_t*>(d_pack + rec_bytes),
                             (uint32_t)n, base[n], spec.layout, spec.dtype, a)) {
        js_set_error("pack_ijg: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    return 0;
}

extern "C" {

int jsnoop_batch_ijg_renderable(const JsnoopBatch* b, int i)
{
    if (!b) { js_set_error("pack_ijg: batch is NULL"); return 0; }
    if (i < 0 || (size_t)i >= b->imgs.size()) { js_set_error("pack_ijg: image index %d out of range, the batch holds %zu", i, b->imgs.size()); return 0; }
    return js_ren_renderable(b->imgs[i], i) == 0 ? 1 : 0;
}
int jsnoop_batch_pack_ijg(JsnoopBatch* b, const JsnoopPackSpec* spec, const int* images, int n, const JsnoopPackDst* dst)
{
    if (!b) { js_set_error("pack_ijg: batch is NULL"); return -1; }
    return b->pack_ijg(spec, images, n, dst);
}

} // extern "C"
