// jsnoop_transform.cpp -- jsnoop_transform_* : the DCT blocks of a decoded batch rearranged on the device into the coefficient arena and the cumulative-DC array
// of flipped, rotated, transposed, cropped or grey pictures (kernel: jsnoop_transform.hip; checks, geometry, block map and plan: jsnoop_transform_check.h), and
// that arena written as files by the export of jsnoop_export.cpp.
#include <array>
#include <map>
#include "jsnoop_host.h"
#include "jsnoop_launch.h"
#include "jsnoop_transform_check.h"
#include "jsnoop_export_prog_check.h"

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    js_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

// where the pieces of one call lie in the private batch's page-locked block (and in its device copy)
struct JsXfBlock { size_t recs, unit_base, total; };
static JsXfBlock js_xf_block(size_t n)
{
    JsXfBlock b; size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 15u) & ~(size_t)15u; return o; };
    b.recs = take(n * sizeof(JsXfRec)); b.unit_base = take((n + 1) * 4); b.total = at;
    return b;
}
static int js_xf_grow(int16_t** p, size_t* cap, size_t need)
{
    if (need <= *cap && *p) return 0;                            // (hipFree waits for the device: no earlier call still uses the old block)
    if (*p) hipFree(*p);
    *p = nullptr; *cap = 0;
    HIP_TRY(hipMalloc((void**)p, need + need / 16 + 256));
    *cap = need + need / 16 + 256;
    return 0;
}

JsnoopTransform::~JsnoopTransform() { if (ev_src) hipEventDestroy(ev_src); delete b; }

// Every check first (a refused call leaves entries, images, arena and files of the call before it); then the arena grows where it must, the records and the prefix
// table go through the private batch's page-locked block behind its event (pack_block / pack_send), and k_transform is launched on the object's stream -- behind
// an event on the source batch's stream where that is another one.  Nothing waits, except the generic re-decode behind a DC-only fast decode of the source.
int JsnoopTransform::run(JsnoopBatch* src, const JsnoopTransformSpec* spec_in, const int* images, int n)
{
    if (!src) { js_set_error("transform: batch is NULL"); return -1; }
    JsnoopTransformSpec spec;
    if (js_transform_import_spec(spec_in, &spec)) return -1;
    if (n < 0) { js_set_error("transform: n = %d", n); return -1; }
    if (src == b) { js_set_error("transform: the source is the object's own arena"); return -1; }
    if (!src->uploaded || src->last_form == 0 || !src->dev.coef || !src->dev.dccum) { js_set_error("transform: the batch has not been decoded"); return -1; }
    if (src->device != b->device) { js_set_error("transform: the batch lives on device %d, the object on device %d", src->device, b->device); return -1; }
    std::vector<int> res((size_t)n), image_of_((size_t)n);
    std::vector<JsXfRec> recs((size_t)n); std::vector<JsImage> descs((size_t)n); std::vector<uint32_t> unit_base((size_t)n + 1);
    uint32_t nout = 0; uint64_t blocks = 0;
    if (js_transform_plan(src->imgs.data(), src->imgs.size(), spec, images, n, res.data(), image_of_.data(), recs.data(), descs.data(), unit_base.data(), &nout, &blocks)) return -1;
    // the destination's table sets: one per distinct content, which is at most one per (source set, transposed or not) pair the call uses
    const uint32_t flags = (uint32_t)js_xf_flags(spec.op);
    std::vector<JsTableSet> sets; std::map<std::array<uint16_t, 192>, uint32_t> seen;
    for (int k = 0; k < n; k++) {
        if (image_of_[(size_t)k] < 0) continue;
        JsImage& d = descs[(size_t)image_of_[(size_t)k]];
        std::array<uint16_t, 192> key; key.fill(0);
        for (uint32_t c = 0; c < d.ncomp; c++) {
            uint16_t nat[64];
            if (jsnoop_batch_image_dqt(src, images ? images[k] : k, (int)c, nat)) return -1;
            js_xf_table(nat, flags & JS_XF_T, &key[c * 64]);
        }
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (uint32_t)sets.size()).first;
            sets.emplace_back(); memset(&sets.back(), 0, sizeof(JsTableSet)); memcpy(sets.back().qzz, key.data(), sizeof key);
        }
        d.tableset = it->second;
    }
    HIP_TRY(hipSetDevice(b->device));
    const JsXfBlock blk = js_xf_block(nout);
    if (nout) {
        if (b->pack_block(blk.total)) return -1;
        if (src->ensure_generic()) return -1;                     // (a DC-only fast-form decode left the source's arena untouched)
        if (src->stream != b->stream && !ev_src) HIP_TRY(hipEventCreateWithFlags(&ev_src, hipEventDisableTiming));
        if (js_xf_grow(&b->dev.coef, &b->cap.coef, (size_t)blocks * 128) || js_xf_grow(&b->dev.dccum, &b->cap.dccum, (size_t)blocks * 2 + 64)) { b->clear(); results.clear(); image_of.clear(); return -1; }
    }
    // ---- from here on the object holds this call
    b->clear();
    b->export_opt = false; b->export_prog = false; b->export_scans.clear(); b->export_scan_base.clear();
    results.swap(res); image_of.swap(image_of_);
    if (nout == 0) return 0;
    b->tables.swap(sets);
    b->imgs.assign(descs.begin(), descs.begin() + nout);
    memcpy(b->h_pack + blk.recs, recs.data(), (size_t)nout * sizeof(JsXfRec));
    memcpy(b->h_pack + blk.unit_base, unit_base.data(), ((size_t)nout + 1) * 4);
    auto fail = [&]() { b->clear(); results.clear(); image_of.clear(); return -1; };
    if (b->pack_send(blk.total)) return fail();
    if (src->stream != b->stream) {
        if (hipEventRecord(ev_src, src->stream) != hipSuccess || hipStreamWaitEvent(b->stream, ev_src, 0) != hipSuccess) { js_set_error("transform: the event behind the source batch's stream failed: %s", hipGetErrorString(hipGetLastError())); return fail(); }
    }
    if (js_launch_transform(b->stream, reinterpret_cast<const JsXfRec*>(b->d_pack + blk.recs), reinterpret_cast<const uint32_t*>(b->d_pack + blk.unit_base), nout, unit_base[nout], flags,
                            src->dev.coef, src->dev.dccum, b->dev.coef, b->dev.dccum)) {
        js_set_error("transform: launch failed: %s", hipGetErrorString(hipGetLastError())); return fail(); }
    b->uploaded = true; b->last_form = 1;
    return 0;
}

// jsnoop_batch_export_jpeg_prog on the private batch.  What that call refuses only after it has dropped the previous export (an index out of range) is
// refused here first.
int JsnoopTransform::export_jpeg(const JsnoopExportSpec* spec, const JsnoopExportCoding* coding, const JsnoopExportRestart* restart, const JsnoopExportProgressive* prog,
                                 const int* images, int n)
{
    if (!b->uploaded || b->last_form == 0) { js_set_error("transform_export: nothing has been transformed"); return -1; }
    JsnoopExportSpec s; JsnoopExportCoding c; JsnoopExportRestart r; JsnoopExportProgressive p;
    if (js_export_import_spec(spec, &s) || js_export_import_coding(coding, &c) || js_export_import_restart(restart, &r) || js_export_import_progressive(prog, &p)) return -1;
    if (n < 0) { js_set_error("transform_export: n = %d", n); return -1; }
    if (!images && (size_t)n > b->imgs.size()) { js_set_error("transform_export: n = %d without a list, the object holds %zu", n, b->imgs.size()); return -1; }
    for (int k = 0; images && k < n; k++)
        if (images[k] < 0 || (size_t)images[k] >= b->imgs.size()) { js_set_error("transform_export: image index %d (entry %d) out of range, the object holds %zu", images[k], k, b->imgs.size()); return -1; }
    return b->export_jpeg_prog(spec, coding, restart, prog, images, n);
}

static JsnoopTransform* js_xf_obj(const JsnoopTransform* t, const char* what)
{
    if (!t || !t->b) { js_set_error("%s: transform object is NULL", what); return nullptr; }
    return const_cast<JsnoopTransform*>(t);
}

extern "C" {

void* jsnoop_batch_stream(const JsnoopBatch* b) { return b ? (void*)b->stream : nullptr; }
JsnoopTransform* jsnoop_transform_create(void* stream)
{
    JsnoopBatch* b = jsnoop_batch_create(stream);
    if (!b) return nullptr;
    JsnoopTransform* t = new JsnoopTransform; t->b = b;
    return t;
}
void jsnoop_transform_destroy(JsnoopTransform* t) { delete t; }
void jsnoop_transform_spec_defaults(JsnoopTransformSpec* out) { if (out) js_transform_spec_defaults(out); }
int jsnoop_transform_run(JsnoopTransform* t, JsnoopBatch* src, const JsnoopTransformSpec* spec, const int* images, int n)
{
    if (!js_xf_obj(t, "transform")) return -1;
    return t->run(src, spec, images, n);
}
int jsnoop_transform_entry_count(const JsnoopTransform* t) { return t && t->b ? (int)t->results.size() : 0; }
int jsnoop_transform_entry(const JsnoopTransform* t, int k, int* result, int* image)
{
    if (!js_xf_obj(t, "transform_entry")) return -1;
    if (k < 0 || (size_t)k >= t->results.size()) { js_set_error("transform_entry: entry %d out of range, the last run had %zu", k, t->results.size()); return -1; }
    if (result) *result = t->results[(size_t)k];
    if (image) *image = t->image_of[(size_t)k];
    return 0;
}
int jsnoop_transform_count(const JsnoopTransform* t) { return t && t->b ? (int)t->b->imgs.size() : 0; }
int jsnoop_transform_image_info(const JsnoopTransform* t, int i, unsigned* out16)
{
    if (!js_xf_obj(t, "transform_image_info")) return -1;
    if (!out16) { js_set_error("transform_image_info: out16 is NULL"); return -1; }
    if (i < 0 || (size_t)i >= t->b->imgs.size()) { js_set_error("transform_image_info: image index %d out of range, the object holds %zu", i, t->b->imgs.size()); return -1; }
    return jsnoop_batch_image_info(t->b, i, out16);
}
int jsnoop_transform_image_dqt(const JsnoopTransform* t, int i, int comp, uint16_t* out64)
{
    if (!js_xf_obj(t, "transform_image_dqt")) return -1;
    return jsnoop_batch_image_dqt(t->b, i, comp, out64);
}
int jsnoop_transform_read_coefs(JsnoopTransform* t, int i, int16_t* coefs, int16_t* dccum, size_t max_blocks)
{
    if (!js_xf_obj(t, "transform_read_coefs")) return -1;
    JsnoopBatch* b = t->b;
    if (i < 0 || (size_t)i >= b->imgs.size()) { js_set_error("transform_read_coefs: image index %d out of range, the object holds %zu", i, b->imgs.size()); return -1; }
    const JsImage& im = b->imgs[(size_t)i]; const size_t nb = std::min<size_t>(max_blocks, im.total_blocks);
    HIP_TRY(hipSetDevice(b->device));
    if (coefs && nb && b->d2h_staged(coefs, b->dev.coef + im.coef_off * 64, nb * 128)) return -1;
    if (dccum && nb && b->d2h_staged(dccum, b->dev.dccum + im.coef_off, nb * 2)) return -1;
    return (int)nb;
}
int jsnoop_transform_export(JsnoopTransform* t, const JsnoopExportSpec* spec, const JsnoopExportCoding* coding, const JsnoopExportRestart* restart, const JsnoopExportProgressive* prog,
                            const int* images, int n)
{
    if (!js_xf_obj(t, "transform_export")) return -1;
    return t->export_jpeg(spec, coding, restart, prog, images, n);
}
int jsnoop_transform_export_count(const JsnoopTransform* t) { return t && t->b ? jsnoop_batch_export_count(t->b) : 0; }
int jsnoop_transform_export_file(const JsnoopTransform* t, int k, const void** dev_ptr, uint64_t* len, int* result, uint32_t* detail, int* image)
{
    if (!js_xf_obj(t, "transform_export_file")) return -1;
    return jsnoop_batch_export_file(t->b, k, dev_ptr, len, result, detail, image);
}
int64_t jsnoop_transform_read_export(JsnoopTransform* t, int k, void* host_dst, uint64_t cap)
{
    if (!js_xf_obj(t, "transform_read_export")) return -1;
    return jsnoop_batch_read_export(t->b, k, host_dst, cap);
}
int64_t jsnoop_transform_export_copy(JsnoopTransform* t, int k, void* dev_dst, uint64_t cap)
{
    if (!js_xf_obj(t, "transform_export_copy")) return -1;
    return jsnoop_batch_export_copy(t->b, k, dev_dst, cap);
}
int jsnoop_transform_export_scan_count(const JsnoopTransform* t, int k) { return t && t->b ? jsnoop_batch_export_scan_count(t->b, k) : 0; }
int jsnoop_transform_export_scan_info(const JsnoopTransform* t, int k, int scan, JsnoopExportScan* sc, uint32_t* ri, uint64_t* intervals, uint64_t* sos_offset, uint64_t* data_bytes)
{
    if (!js_xf_obj(t, "transform_export_scan_info")) return -1;
    return jsnoop_batch_export_scan_info(t->b, k, scan, sc, ri, intervals, sos_offset, data_bytes);
}

} // extern "C"
