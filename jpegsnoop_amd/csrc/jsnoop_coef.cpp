// jsnoop_coef.cpp -- jsnoop_batch_pack_coefs and its helpers: the coefficient arena of a decoded batch into caller-owned device memory, one tensor per
// component (kernel: jsnoop_coef.hip; checks and records: jsnoop_coef_check.h).
#include "jsnoop_host.h"
#include "jsnoop_launch.h"
#include "jsnoop_coef_check.h"

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    js_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

// The pack's block, event and place on the batch stream: one H2D copy of the call's records, one launch, nothing waited for -- except behind a DC-only fast-form
// decode, whose arena does not hold the blocks: the batch is then decoded once more in the generic form (ensure_generic, as jsnoop_batch_read_coefs does), after
// every argument has passed its checks.
int JsnoopBatch::pack_coefs(const JsnoopCoefSpec* spec_in, const int* images, int n, const JsnoopCoefDst* dst)
{
    if (!uploaded || last_form == 0 || !dev.coef || !dev.dccum) { js_set_error("pack_coefs: the batch has not been decoded"); return -1; }
    JsnoopCoefSpec spec;
    if (js_coef_import_spec(spec_in, &spec)) return -1;
    if (n < 0) { js_set_error("pack_coefs: n = %d", n); return -1; }
    if (n == 0) return 0;
    if (!dst) { js_set_error("pack_coefs: dst is NULL"); return -1; }
    HIP_TRY(hipSetDevice(device));
    const size_t rec_bytes = (size_t)n * sizeof(JsCoefRec), total = rec_bytes + ((size_t)n + 1) * 4;
    if (pack_block(total)) return -1;
    JsCoefRec* recs = reinterpret_cast<JsCoefRec*>(h_pack); uint32_t* base = reinterpret_cast<uint32_t*>(h_pack + rec_bytes);
    if (js_coef_plan(imgs.data(), imgs.size(), spec, images, n, dst, recs, base)) return -1;
    if (ensure_generic()) return -1;
    if (pack_send(total)) return -1;
    if (js_launch_pack_coefs(stream, dev.coef, dev.dccum, reinterpret_cast<const JsCoefRec*>(d_pack), reinterpret_cast<const uint32_t*>(d_pack + rec_bytes),
                             (uint32_t)n, base[n], spec.layout, spec.dtype, spec.order)) {
        js_set_error("pack_coefs: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    return 0;
}

extern "C" {

void jsnoop_coef_spec_defaults(JsnoopCoefSpec* out) { if (out) js_coef_spec_defaults(out); }
int jsnoop_batch_coef_grid(const JsnoopBatch* b, int i, int comp, unsigned* bw, unsigned* bh)
{
    if (!b) { js_set_error("pack_coefs: batch is NULL"); return -1; }
    if (i < 0 || (size_t)i >= b->imgs.size()) { js_set_error("pack_coefs: image index %d out of range, the batch holds %zu", i, b->imgs.size()); return -1; }
    uint32_t w = 0, h = 0;
    if (js_coef_grid(b->imgs[i], comp, &w, &h, nullptr)) return -1;
    if (bw) *bw = w;
    if (bh) *bh = h;
    return 0;
}
uint64_t jsnoop_batch_coef_bytes(const JsnoopBatch* b, const JsnoopCoefSpec* spec_in, int i, int comp)
{
    JsnoopCoefSpec spec; unsigned bw = 0, bh = 0;
    if (!b) { js_set_error("pack_coefs: batch is NULL"); return 0; }
    if (js_coef_import_spec(spec_in, &spec) || jsnoop_batch_coef_grid(b, i, comp, &bw, &bh)) return 0;
    return js_coef_dense_bytes(bw, bh, spec);
}
int jsnoop_batch_pack_coefs(JsnoopBatch* b, const JsnoopCoefSpec* spec, const int* images, int n, const JsnoopCoefDst* dst)
{
    if (!b) { js_set_error("pack_coefs: batch is NULL"); return -1; }
    return b->pack_coefs(spec, images, n, dst);
}
int jsnoop_batch_image_dqt(const JsnoopBatch* b, int i, int comp, uint16_t* out64)
{
    if (!b) { js_set_error("image_dqt: batch is NULL"); return -1; }
    if (!out64) { js_set_error("image_dqt: out64 is NULL"); return -1; }
    if (i < 0 || (size_t)i >= b->imgs.size()) { js_set_error("image_dqt: image index %d out of range, the batch holds %zu", i, b->imgs.size()); return -1; }
    const JsImage& im = b->imgs[i];
    if (comp < 0 || (uint32_t)comp >= im.ncomp || comp > 2) { js_set_error("image_dqt: component %d, the image has %u", comp, im.ncomp); return -1; }
    if ((size_t)i < js_prog_count(b)) return js_prog_dqt(b, (uint32_t)i, (uint32_t)comp, out64);
    if (im.tableset >= b->tables.size()) { js_set_error("image_dqt: image %d has no table set", i); return -1; }
    js_coef_dqt_natural(b->tables[im.tableset].qzz[comp], out64);
    return 0;
}

} // extern "C"
