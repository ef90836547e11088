// jsnoop_encode.cpp -- jsnoop_encode_* : 8-bit pictures in device memory encoded into a coefficient arena and a cumulative-DC array on the device (kernel:
// jsnoop_encode.hip; checks, tables, geometry and the unit plan: jsnoop_encode_check.h), and that arena written as files by the export of jsnoop_export.cpp.
#include "jsnoop_host.h"
#include "jsnoop_launch.h"
#include "jsnoop_encode_check.h"
#include "jsnoop_export_prog_check.h"

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    js_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

// where the pieces of one call lie in the private batch's page-locked block (and in its device copy)
struct JsEncBlock { size_t recs, unit_base, tabs, total; };
static JsEncBlock js_enc_block(size_t n)
{
    JsEncBlock b; size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 15u) & ~(size_t)15u; return o; };
    b.recs = take(n * sizeof(JsEncRec)); b.unit_base = take((n + 1) * 4); b.tabs = take(sizeof(JsEncTabs)); b.total = at;
    return b;
}
static int js_enc_grow(int16_t** p, size_t* cap, size_t need)
{
    if (need <= *cap && *p) return 0;                            // (hipFree waits for the device: no earlier call still uses the old block)
    if (*p) hipFree(*p);
    *p = nullptr; *cap = 0;
    HIP_TRY(hipMalloc((void**)p, need + need / 16 + 256));
    *cap = need + need / 16 + 256;
    return 0;
}

JsnoopEncode::~JsnoopEncode() { delete b; }

// Every check first (a refused call leaves images, arena and files of the call before it); then the arena grows where it must, the records, the prefix table and
// the tables go through the batch's page-locked block behind its event (pack_block / pack_send), and k_encode is launched on the stream.  Nothing waits.
int JsnoopEncode::run(const JsnoopEncodeSpec* spec_in, const JsnoopEncodeSrc* src, int n)
{
    JsnoopEncodeSpec spec;
    if (js_encode_import_spec(spec_in, &spec)) return -1;
    if (n < 0) { js_set_error("encode: n = %d", n); return -1; }
    if (n > 0 && !src) { js_set_error("encode: src is NULL"); return -1; }
    std::vector<JsEncRec> recs((size_t)n); std::vector<uint32_t> unit_base((size_t)n + 1);
    uint64_t blocks = 0;
    if (js_encode_plan(spec, src, n, recs.data(), unit_base.data(), &blocks)) return -1;
    uint8_t luma[64], chroma[64];
    js_encode_tables(spec, luma, chroma);
    HIP_TRY(hipSetDevice(b->device));
    const JsEncBlock blk = js_enc_block((size_t)n);
    if (n) {
        if (b->pack_block(blk.total)) return -1;
        if (js_enc_grow(&b->dev.coef, &b->cap.coef, (size_t)blocks * 128) || js_enc_grow(&b->dev.dccum, &b->cap.dccum, (size_t)blocks * 2 + 64)) { b->clear(); return -1; }
    }
    // ---- from here on the object holds this call
    b->clear();
    b->export_opt = false; b->export_prog = false; b->export_scans.clear(); b->export_scan_base.clear();
    if (n == 0) return 0;
    static const uint8_t zz[64] = JS_ZIGZAG_NATURAL;
    b->tables.resize(1);
    JsTableSet& ts = b->tables[0];
    memset(&ts, 0, sizeof ts);
    for (int z = 0; z < 64; z++) { ts.qzz[0][z] = luma[zz[z]]; ts.qzz[1][z] = ts.qzz[2][z] = chroma[zz[z]]; }
    b->imgs.resize((size_t)n);
    for (int k = 0; k < n; k++) js_encode_describe(recs[(size_t)k], &b->imgs[(size_t)k]);
    memcpy(b->h_pack + blk.recs, recs.data(), (size_t)n * sizeof(JsEncRec));
    memcpy(b->h_pack + blk.unit_base, unit_base.data(), ((size_t)n + 1) * 4);
    js_encode_fill_tabs(luma, chroma, reinterpret_cast<JsEncTabs*>(b->h_pack + blk.tabs));
    if (b->pack_send(blk.total)) { b->clear(); return -1; }
    if (js_launch_encode(b->stream, reinterpret_cast<const JsEncRec*>(b->d_pack + blk.recs), reinterpret_cast<const uint32_t*>(b->d_pack + blk.unit_base),
                         reinterpret_cast<const JsEncTabs*>(b->d_pack + blk.tabs), (uint32_t)n, unit_base[(size_t)n], b->dev.coef, b->dev.dccum)) {
        b->clear(); js_set_error("encode: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    b->uploaded = true; b->last_form = 1;
    return 0;
}

// jsnoop_batch_export_jpeg_prog on the private batch.  What that call refuses only after it has dropped the previous export (an index out of range) is
// refused here first.
int JsnoopEncode::export_jpeg(const JsnoopExportSpec* spec, const JsnoopExportCoding* coding, const JsnoopExportRestart* restart, const JsnoopExportProgressive* prog,
                              const int* images, int n)
{
    if (!b->uploaded || b->last_form == 0) { js_set_error("encode_export: nothing has been encoded"); return -1; }
    JsnoopExportSpec s; JsnoopExportCoding c; JsnoopExportRestart r; JsnoopExportProgressive p;
    if (js_export_import_spec(spec, &s) || js_export_import_coding(coding, &c) || js_export_import_restart(restart, &r) || js_export_import_progressive(prog, &p)) return -1;
    if (n < 0) { js_set_error("encode_export: n = %d", n); return -1; }
    if (!images && (size_t)n > b->imgs.size()) { js_set_error("encode_export: n = %d without a list, the object holds %zu", n, b->imgs.size()); return -1; }
    for (int k = 0; images && k < n; k++)
        if (images[k] < 0 || (size_t)images[k] >= b->imgs.size()) { js_set_error("encode_export: image index %d (entry %d) out of range, the object holds %zu", images[k], k, b->imgs.size()); return -1; }
    return b->export_jpeg_prog(spec, coding, restart, prog, images, n);
}

static JsnoopEncode* js_enc_obj(const JsnoopEncode* e, const char* what)
{
    if (!e || !e->b) { js_set_error("%s: encoder is NULL", what); return nullptr; }
    return const_cast<JsnoopEncode*>(e);
}

extern "C" {

JsnoopEncode* jsnoop_encode_create(void* stream)
{
    JsnoopBatch* b = jsnoop_batch_create(stream);
    if (!b) return nullptr;
    JsnoopEncode* e = new JsnoopEncode; e->b = b;
    return e;
}
void jsnoop_encode_destroy(JsnoopEncode* e) { delete e; }
void jsnoop_encode_spec_defaults(JsnoopEncodeSpec* out) { if (out) js_encode_spec_defaults(out); }
int jsnoop_encode_qtables(const JsnoopEncodeSpec* spec_in, uint8_t luma64[64], uint8_t chroma64[64])
{
    JsnoopEncodeSpec spec; uint8_t l[64], c[64];
    if (js_encode_import_spec(spec_in, &spec)) return -1;
    js_encode_tables(spec, l, c);
    if (luma64) memcpy(luma64, l, 64);
    if (chroma64) memcpy(chroma64, c, 64);
    return 0;
}
int jsnoop_encode_run(JsnoopEncode* e, const JsnoopEncodeSpec* spec, const JsnoopEncodeSrc* src, int n)
{
    if (!js_enc_obj(e, "encode")) return -1;
    return e->run(spec, src, n);
}
int jsnoop_encode_count(const JsnoopEncode* e) { return e && e->b ? (int)e->b->imgs.size() : 0; }
int jsnoop_encode_image_info(const JsnoopEncode* e, int i, unsigned* out16)
{
    if (!js_enc_obj(e, "encode_image_info")) return -1;
    if (!out16) { js_set_error("encode_image_info: out16 is NULL"); return -1; }
    if (i < 0 || (size_t)i >= e->b->imgs.size()) { js_set_error("encode_image_info: image index %d out of range, the object holds %zu", i, e->b->imgs.size()); return -1; }
    return jsnoop_batch_image_info(e->b, i, out16);
}
int jsnoop_encode_read_coefs(JsnoopEncode* e, int i, int16_t* coefs, int16_t* dccum, size_t max_blocks)
{
    if (!js_enc_obj(e, "encode_read_coefs")) return -1;
    JsnoopBatch* b = e->b;
    if (i < 0 || (size_t)i >= b->imgs.size()) { js_set_error("encode_read_coefs: image index %d out of range, the object holds %zu", i, b->imgs.size()); return -1; }
    const JsImage& im = b->imgs[(size_t)i]; const size_t nb = std::min<size_t>(max_blocks, im.total_blocks);
    HIP_TRY(hipSetDevice(b->device));
    if (coefs && nb && b->d2h_staged(coefs, b->dev.coef + im.coef_off * 64, nb * 128)) return -1;
    if (dccum && nb && b->d2h_staged(dccum, b->dev.dccum + im.coef_off, nb * 2)) return -1;
    return (int)nb;
}
int jsnoop_encode_export(JsnoopEncode* e, const JsnoopExportSpec* spec, const JsnoopExportCoding* coding, const JsnoopExportRestart* restart, const JsnoopExportProgressive* prog,
                         const int* images, int n)
{
    if (!js_enc_obj(e, "encode_export")) return -1;
    return e->export_jpeg(spec, coding, restart, prog, images, n);
}
int jsnoop_encode_export_count(const JsnoopEncode* e) { return e && e->b ? jsnoop_batch_export_count(e->b) : 0; }
int jsnoop_encode_export_file(const JsnoopEncode* e, int k, const void** dev_ptr, uint64_t* len, int* result, uint32_t* detail, int* image)
{
    if (!js_enc_obj(e, "encode_export_file")) return -1;
    return jsnoop_batch_export_file(e->b, k, dev_ptr, len, result, detail, image);
}
int64_t jsnoop_encode_read_export(JsnoopEncode* e, int k, void* host_dst, uint64_t cap)
{
    if (!js_enc_obj(e, "encode_read_export")) return -1;
    return jsnoop_batch_read_export(e->b, k, host_dst, cap);
}
int64_t jsnoop_encode_export_copy(JsnoopEncode* e, int k, void* dev_dst, uint64_t cap)
{
    if (!js_enc_obj(e, "encode_export_copy")) return -1;
    return jsnoop_batch_export_copy(e->b, k, dev_dst, cap);
}
int jsnoop_encode_export_scan_count(const JsnoopEncode* e, int k) { return e && e->b ? jsnoop_batch_export_scan_count(e->b, k) : 0; }
int jsnoop_encode_export_scan_info(const JsnoopEncode* e, int k, int scan, JsnoopExportScan* sc, uint32_t* ri, uint64_t* intervals, uint64_t* sos_offset, uint64_t* data_bytes)
{
    if (!js_enc_obj(e, "encode_export_scan_info")) return -1;
    return jsnoop_batch_export_scan_info(e->b, k, scan, sc, ri, intervals, sos_offset, data_bytes);
}

} // extern "C"
