// jsnoop_export.cpp -- jsnoop_batch_export_jpeg and its helpers: what a decoded batch holds (coefficient arena, cumulative DC) written back as baseline JPEG
// files, entropy-coded on the device into memory the batch owns (kernels: jsnoop_export.hip; checks, header and sizes: jsnoop_export_check.h).
#include <stdio.h>
#include "jsnoop_host.h"
#include "jsnoop_launch.h"
#include "jsnoop_export_check.h"

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    js_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

static_assert(JS_EXPORT_TAB_WORDS == JS_EXPORT_TABS, "one table layout");
typedef JsnoopBatch::JsExportEntry JsExportEntry;

static int js_export_grow(uint8_t** p, size_t* cap, size_t need)
{
    if (need <= *cap) return 0;                                  // (hipFree waits for the device: no earlier call still uses the old block)
    if (*p) hipFree(*p);
    *p = nullptr; *cap = 0;
    HIP_TRY(hipMalloc((void**)p, need + need / 4 + 4096));
    *cap = need + need / 4 + 4096;
    return 0;
}
static int js_export_q(void* user, int i, int comp, uint16_t* out64) { return jsnoop_batch_image_dqt(static_cast<const JsnoopBatch*>(user), i, comp, out64); }

// Two phases on the batch stream, each behind one H2D copy of the call's block (the packs' page-locked block and event), each ended by ONE wait:
//   1. k_export_measure + k_export_scan; the result words and the bit length of every entry come back (wait 1): the host sizes the un-stuffed streams and the files.
//   2. the streams zeroed, k_export_bits, k_export_ffcount, k_export_scan, k_export_stuff; the file lengths come back (wait 2).
// (pack_block's wait for the event of the first copy, in front of phase 2, finds it complete: wait 1 was behind it.)
int JsnoopBatch::export_jpeg(const JsnoopExportSpec* spec_in, const int* images, int n)
{
    if (!uploaded || last_form == 0 || !dev.coef || !dev.dccum) { js_set_error("export_jpeg: the batch has not been decoded"); return -1; }
    JsnoopExportSpec spec;
    if (js_export_import_spec(spec_in, &spec)) return -1;
    if (n < 0) { js_set_error("export_jpeg: n = %d", n); return -1; }
    if (!images && (size_t)n > imgs.size()) { js_set_error("export_jpeg: n = %d without a list, the batch holds %zu", n, imgs.size()); return -1; }
    exports.clear();
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    const JsExportBlock blk = js_export_block((size_t)n);
    if (pack_block(blk.total)) return -1;
    JsExportRec* recs = reinterpret_cast<JsExportRec*>(h_pack + blk.recs);
    uint32_t* unit_base = reinterpret_cast<uint32_t*>(h_pack + blk.unit_base); uint32_t* chunk_base = reinterpret_cast<uint32_t*>(h_pack + blk.chunk_base);
    std::vector<uint8_t> unsupported((size_t)n);
    uint64_t blocks = 0;
    if (js_export_plan(imgs.data(), imgs.size(), spec, images, n, js_export_q, this, recs, unit_base, h_pack + blk.hdrs, unsupported.data(), &blocks)) return -1;
    memset(chunk_base, 0, ((size_t)n + 1) * 4);
    js_export_code_tabs(reinterpret_cast<uint32_t*>(h_pack + blk.tabs));
    if (ensure_generic()) return -1;
    const uint32_t units = unit_base[n];
    const JsExportScratch sc = js_export_scratch((size_t)n, units, blocks);
    if (js_export_grow(&d_export_tmp, &d_export_tmp_cap, sc.total)) return -1;
    if (pack_send(blk.total)) return -1;
    HIP_TRY(hipMemsetAsync(d_export_tmp + sc.res, 0, (size_t)n * 4, stream));
    HIP_TRY(hipMemsetAsync(d_export_tmp + sc.res + (size_t)n * 4, 0xFF, (size_t)n * 8, stream));
    HIP_TRY(hipMemsetAsync(d_export_tmp + sc.len, 0, (size_t)n * 8, stream));
    const JsExportRec* d_recs = reinterpret_cast<const JsExportRec*>(d_pack + blk.recs);
    const uint32_t* d_unit_base = reinterpret_cast<const uint32_t*>(d_pack + blk.unit_base); const uint32_t* d_tabs = reinterpret_cast<const uint32_t*>(d_pack + blk.tabs);
    uint16_t* d_blk_bits = reinterpret_cast<uint16_t*>(d_export_tmp + sc.blk_bits); uint64_t* d_unit_off = reinterpret_cast<uint64_t*>(d_export_tmp + sc.unit_off);
    if (js_launch_export_measure(stream, dev.coef, dev.dccum, d_recs, d_unit_base, (uint32_t)n, units, d_tabs, d_blk_bits, reinterpret_cast<uint32_t*>(d_export_tmp + sc.unit_bits),
                                 d_unit_off, reinterpret_cast<uint32_t*>(d_export_tmp + sc.res), reinterpret_cast<uint64_t*>(d_export_tmp + sc.ent_bits))) {
        js_set_error("export_jpeg: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    std::vector<uint8_t> back(sc.len);
    if (d2h_staged(back.data(), d_export_tmp, sc.len)) return -1;                                    // ---- wait 1
    std::vector<int> result((size_t)n); std::vector<uint32_t> detail((size_t)n);
    uint64_t u_bytes = 0, out_bytes = 0;
    if (pack_block(blk.total)) return -1;
    if (js_export_layout(recs, n, unsupported.data(), reinterpret_cast<const uint32_t*>(back.data() + sc.res), reinterpret_cast<const uint64_t*>(back.data() + sc.ent_bits),
                         chunk_base, result.data(), detail.data(), &u_bytes, &out_bytes)) return -1;
    const uint32_t chunks = chunk_base[n];
    std::vector<uint64_t> len((size_t)n, 0);
    if (chunks) {
        const size_t ff_at = 0, off_at = ((size_t)chunks * 4 + 15u) & ~(size_t)15u, u_at = (off_at + (size_t)chunks * 8 + 15u) & ~(size_t)15u;      // the chunk tables in front of the streams (which start on 16 bytes)
        if (js_export_grow(&d_export_u, &d_export_u_cap, u_at + u_bytes) || js_export_grow(&d_export_out, &d_export_out_cap, out_bytes)) return -1;
        if (pack_send(blk.total)) return -1;
        HIP_TRY(hipMemsetAsync(d_export_u + u_at, 0, u_bytes, stream));
        if (js_launch_export_write(stream, dev.coef, dev.dccum, d_recs, d_unit_base, reinterpret_cast<const uint32_t*>(d_pack + blk.chunk_base), (uint32_t)n, units, chunks, d_tabs,
                                   d_blk_bits, d_unit_off, d_export_u + u_at, reinterpret_cast<uint32_t*>(d_export_u + ff_at), reinterpret_cast<uint64_t*>(d_export_u + off_at),
                                   reinterpret_cast<uint64_t*>(d_export_tmp + sc.ent_ff), d_pack + blk.hdrs, d_export_out, reinterpret_cast<uint64_t*>(d_export_tmp + sc.len))) {
            js_set_error("export_jpeg: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
        if (d2h_staged(len.data(), d_export_tmp + sc.len, (size_t)n * 8)) return -1;                  // ---- wait 2
    }
    for (int k = 0; k < n; k++) {
        JsExportEntry e; e.off = recs[k].out_off; e.len = recs[k].live ? len[k] : 0; e.result = result[k]; e.detail = detail[k]; e.image = images ? images[k] : k;
        if (recs[k].live && (e.len < recs[k].hdr_len + 3u || e.len > recs[k].out_cap)) {
            exports.clear(); js_set_error("export_jpeg: entry %d came back with %llu bytes, its place holds %llu", k, (unsigned long long)e.len, (unsigned long long)recs[k].out_cap); return -1; }
        exports.push_back(e);
    }
    return 0;
}

static const char* js_export_reason(int result)
{
    switch (result) {
    case JSNOOP_EXPORT_INEXACT: return "a value is no multiple of its quantiser (INEXACT)";
    case JSNOOP_EXPORT_UNCODABLE: return "a level has no Annex K code (UNCODABLE)";
    case JSNOOP_EXPORT_UNSUPPORTED: return "the sample precision is not 8 (UNSUPPORTED)";
    default: return "ok";
    }
}
static const JsExportEntry* js_export_entry(const JsnoopBatch* b, int k, const char* what)
{
    if (!b) { js_set_error("%s: batch is NULL", what); return nullptr; }
    if (k < 0 || (size_t)k >= b->exports.size()) { js_set_error("%s: entry %d out of range, the last export holds %zu", what, k, b->exports.size()); return nullptr; }
    return &b->exports[(size_t)k];
}

extern "C" {

void jsnoop_export_spec_defaults(JsnoopExportSpec* out) { if (out) js_export_spec_defaults(out); }
int jsnoop_batch_export_jpeg(JsnoopBatch* b, const JsnoopExportSpec* spec, const int* images, int n)
{
    if (!b) { js_set_error("export_jpeg: batch is NULL"); return -1; }
    return b->export_jpeg(spec, images, n);
}
int jsnoop_batch_export_count(const JsnoopBatch* b) { return b ? (int)b->exports.size() : 0; }
int jsnoop_batch_export_file(const JsnoopBatch* b, int k, const void** dev_ptr, uint64_t* len, int* result, uint32_t* detail, int* image)
{
    const JsExportEntry* e = js_export_entry(b, k, "export_file");
    if (!e) return -1;
    if (dev_ptr) *dev_ptr = e->len ? b->d_export_out + e->off : nullptr;
    if (len) *len = e->len;
    if (result) *result = e->result;
    if (detail) *detail = e->detail;
    if (image) *image = e->image;
    return 0;
}
int64_t jsnoop_batch_read_export(JsnoopBatch* b, int k, void* host_dst, uint64_t cap)
{
    const JsExportEntry* e = js_export_entry(b, k, "read_export");
    if (!e) return -1;
    if (!e->len) return 0;
    if (!host_dst) { js_set_error("read_export: host_dst is NULL"); return -1; }
    if (cap < e->len) { js_set_error("read_export: cap %llu is below the file's %llu bytes", (unsigned long long)cap, (unsigned long long)e->len); return -1; }
    if (hipSetDevice(b->device) != hipSuccess) { js_set_error("read_export: device error"); return -1; }
    if (b->d2h_staged(host_dst, b->d_export_out + e->off, (size_t)e->len)) return -1;
    return (int64_t)e->len;
}
int64_t jsnoop_batch_export_copy(JsnoopBatch* b, int k, void* dev_dst, uint64_t cap)
{
    const JsExportEntry* e = js_export_entry(b, k, "export_copy");
    if (!e) return -1;
    if (!e->len) return 0;
    if (!dev_dst) { js_set_error("export_copy: dev_dst is NULL"); return -1; }
    if (cap < e->len) { js_set_error("export_copy: cap %llu is below the file's %llu bytes", (unsigned long long)cap, (unsigned long long)e->len); return -1; }
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemcpyAsync(dev_dst, b->d_export_out + e->off, (size_t)e->len, hipMemcpyDeviceToDevice, b->stream));
    return (int64_t)e->len;
}
int jsnoop_export_jpeg(JsnoopDecoder* d, const char* path)
{
    if (!d || !path) { js_set_error("jsnoop_export_jpeg: bad argument"); return -1; }
    if (!d->have_image || !d->preview_is_jpeg || !d->batch) { js_set_error("jsnoop_export_jpeg: no decoded image"); return -1; }
    d->arena_generic();
    JsnoopBatch* b = d->batch;
    JsnoopExportSpec spec; js_export_spec_defaults(&spec);
    const int img = d->img;
    if (b->export_jpeg(&spec, &img, 1)) return -1;
    const JsExportEntry e = b->exports[0];
    if (e.result != JSNOOP_EXPORT_OK) { js_set_error("jsnoop_export_jpeg: not exported: %s, block %u", js_export_reason(e.result), e.detail); return -1; }
    std::vector<uint8_t> host((size_t)e.len);
    if (jsnoop_batch_read_export(b, 0, host.data(), e.len) < 0) return -1;
    FILE* f = fopen(path, "wb");
    if (!f) { js_set_error("ERROR: Couldn't open file for write [%s]", path); return -1; }
    const bool ok = fwrite(host.data(), 1, host.size(), f) == host.size();
    fclose(f);
    if (!ok) { js_set_error("jsnoop_export_jpeg: short write to [%s]", path); return -1; }
    return 0;
}

} // extern "C"
