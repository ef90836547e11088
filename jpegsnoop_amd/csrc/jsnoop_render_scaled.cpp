// jsnoop_render_scaled.cpp -- jsnoop_batch_pack_ijg_scaled, jsnoop_batch_ijg_scaled_size and jsnoop_batch_pack_ijg_scaled_bytes: the coefficient arena of a decoded
// batch rendered as libjpeg's reduced-size pixels into caller-owned device memory (kernel: jsnoop_render_scaled.hip; checks, records and the arithmetic:
// jsnoop_render_scaled_check.h).  denom 1 is jsnoop_batch_pack_ijg itself.
#include "jsnoop_host.h"
#include "jsnoop_launch.h"
#include "jsnoop_render_scaled_check.h"

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    js_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

// jsnoop_batch_pack_ijg's place on the batch stream, block and event: one H2D copy of the call's records, one launch, nothing waited for -- except behind a DC-only
// fast-form decode (ensure_generic, after every argument has passed its checks).
int JsnoopBatch::pack_ijg_scaled(const JsnoopPackSpec* spec_in, unsigned denom, const int* images, int n, const JsnoopPackDst* dst)
{
    if (js_rs_denom(denom, "pack_ijg_scaled")) return -1;
    if (denom == 1u) return pack_ijg(spec_in, images, n, dst);
    if (!uploaded || last_form == 0 || !dev.coef || !dev.dccum || !dev.imgs) { js_set_error("pack_ijg_scaled: the batch has not been decoded"); return -1; }
    JsnoopPackSpec spec;
    if (js_pack_import_spec(spec_in, &spec, "pack_ijg_scaled")) return -1;
    if (n < 0) { js_set_error("pack_ijg_scaled: n = %d", n); return -1; }
    if (n == 0) return 0;
    if (!dst) { js_set_error("pack_ijg_scaled: dst is NULL"); return -1; }
    HIP_TRY(hipSetDevice(device));
    const size_t rec_bytes = ((size_t)n * sizeof(JsRsRec) + 15) & ~(size_t)15, total = rec_bytes + ((size_t)n + 1) * 4;
    if (pack_block(total)) return -1;
    JsRsRec* recs = reinterpret_cast<JsRsRec*>(h_pack); uint32_t* base = reinterpret_cast<uint32_t*>(h_pack + rec_bytes);
    if (js_rs_plan(imgs.data(), imgs.size(), spec, denom, images, n, dst, recs, base)) return -1;
    if (ensure_generic()) return -1;
    if (pack_send(total)) return -1;
    JsPackArgs a; a.bgr = spec.bgr != 0;
    for (int c = 0; c < 3; c++) { a.scale[c] = spec.scale[c]; a.bias[c] = spec.bias[c]; }
    if (js_launch_render_ijg_scaled(stream, dev.coef, dev.dccum, reinterpret_cast<const JsRsRec*>(d_pack), reinterpret_cast<const uint32_t*>(d_pack + rec_bytes),
                                    (uint32_t)n, base[n], spec.layout, spec.dtype, a)) {
        js_set_error("pack_ijg_scaled: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    return 0;
}

extern "C" {

int jsnoop_batch_ijg_scaled_size(const JsnoopBatch* b, int i, unsigned denom, unsigned* w, unsigned* h)
{
    if (!b) { js_set_error("pack_ijg_scaled: batch is NULL"); return -1; }
    if (js_rs_denom(denom, "pack_ijg_scaled")) return -1;
    if (i < 0 || (size_t)i >= b->imgs.size()) { js_set_error("pack_ijg_scaled: image index %d out of range, the batch holds %zu", i, b->imgs.size()); return -1; }
    if (js_ren_renderable(b->imgs[i], i)) return -1;
    if (w) *w = js_rs_out(b->imgs[i].dim_x, denom);
    if (h) *h = js_rs_out(b->imgs[i].dim_y, denom);
    return 0;
}
uint64_t jsnoop_batch_pack_ijg_scaled_bytes(const JsnoopBatch* b, const JsnoopPackSpec* spec_in, unsigned denom, int i)
{
    JsnoopPackSpec spec;
    if (!b) { js_set_error("pack_ijg_scaled: batch is NULL"); return 0; }
    if (js_pack_import_spec(spec_in, &spec, "pack_ijg_scaled") || js_rs_denom(denom, "pack_ijg_scaled")) return 0;
    if (i < 0 || (size_t)i >= b->imgs.size()) { js_set_error("pack_ijg_scaled: image index %d out of range, the batch holds %zu", i, b->imgs.size()); return 0; }
    if (js_ren_renderable(b->imgs[i], i)) return 0;
    return js_rs_dense_bytes(b->imgs[i], spec, denom);
}
int jsnoop_batch_pack_ijg_scaled(JsnoopBatch* b, const JsnoopPackSpec* spec, unsigned denom, const int* images, int n, const JsnoopPackDst* dst)
{
    if (!b) { js_set_error("pack_ijg_scaled: batch is NULL"); return -1; }
    return b->pack_ijg_scaled(spec, denom, images, n, dst);
}

} // extern "C"
