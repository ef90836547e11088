// jsnoop_export.cpp -- jsnoop_batch_export_jpeg and its helpers: what a decoded batch holds (coefficient arena, cumulative DC) written back as baseline JPEG
// files, entropy-coded on the device into memory the batch owns (kernels: jsnoop_export.hip; checks, header and sizes: jsnoop_export_check.h).
#include <stdio.h>
#include "jsnoop_host.h"
#include "jsnoop_launch.h"
#include "jsnoop_export_prog_check.h"

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
// With JSNOOP_HUFFMAN_OPTIMAL (jsnoop_export_opt_check.h has the arithmetic) phase 1 is k_export_symbols, k_export_huff, k_export_measure with every entry's own
// tables, k_export_scan; the header lengths come back with wait 1, and phase 2 reads tables and headers from d_export_opt, where the device built them (the second
// copy of the call's block rewrites d_pack, so nothing the device made lives there).
int JsnoopBatch::export_jpeg(const JsnoopExportSpec* spec_in, const int* images, int n)
{
    JsnoopExportCoding coding; js_export_coding_defaults(&coding);
    return export_jpeg_coded(spec_in, &coding, images, n);
}
int JsnoopBatch::export_jpeg_coded(const JsnoopExportSpec* spec_in, const JsnoopExportCoding* coding_in, const int* images, int n)
{
    return export_jpeg_rst(spec_in, coding_in, nullptr, images, n);
}
// With restart intervals (jsnoop_export_rst_check.h has the arithmetic) the plan gains the side records and DRI in the headers, phase 1 measures with the restart forms
// (k_export_rst_scan in place of k_export_scan over the units) and phase 2 runs k_export_bits in its restart form, which fills the interval tables, and
// k_export_stuff_rst; the interval tables live behind the first phase's scratch.  A call in which no entry has an interval takes none of this.
int JsnoopBatch::export_jpeg_rst(const JsnoopExportSpec* spec_in, const JsnoopExportCoding* coding_in, const JsnoopExportRestart* restart_in, const int* images, int n)
{
    JsnoopExportCoding coding;
    if (js_export_import_coding(coding_in, &coding)) return -1;
    JsnoopExportRestart restart;
    if (js_export_import_restart(restart_in, &restart)) return -1;
    const bool opt = coding.huffman == JSNOOP_HUFFMAN_OPTIMAL;
    if (!uploaded || last_form == 0 || !dev.coef || !dev.dccum) { js_set_error("export_jpeg: the batch has not been decoded"); return -1; }
    JsnoopExportSpec spec;
    if (js_export_import_spec(spec_in, &spec)) return -1;
    if (n < 0) { js_set_error("export_jpeg: n = %d", n); return -1; }
    if (!images && (size_t)n > imgs.size()) { js_set_error("export_jpeg: n = %d without a list, the batch holds %zu", n, imgs.size()); return -1; }
    exports.clear(); export_opt = false; export_prog = false;
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    bool rst = false;                                            // some listed entry is written with a restart interval (or refused for one too large)
    if (restart.mode != JSNOOP_RESTART_NONE) for (int k = 0; k < n && !rst; k++) {
        const int i = images ? images[k] : k;
        if (i < 0 || (size_t)i >= imgs.size()) break;                // (the plan names it)
        rst = js_export_rst_ri(restart, imgs[(size_t)i]) != 0u;
    }
    const JsExportRstBlock rblk = js_export_rst_block((size_t)n, opt);
    const JsExportOptBlock oblk = rst ? rblk.o : js_export_opt_block((size_t)n);
    const JsExportBlock blk = rst ? rblk.o.b : (opt ? oblk.b : js_export_block((size_t)n));
    if (pack_block(blk.total)) return -1;
    JsExportRec* recs = reinterpret_cast<JsExportRec*>(h_pack + blk.recs);
    uint32_t* unit_base = reinterpret_cast<uint32_t*>(h_pack + blk.unit_base); uint32_t* chunk_base = reinterpret_cast<uint32_t*>(h_pack + blk.chunk_base);
    std::vector<uint8_t> unsupported((size_t)n);
    uint64_t blocks = 0;
    JsExportOptRec* orecs = opt ? reinterpret_cast<JsExportOptRec*>(h_pack + oblk.orecs) : nullptr;
    if (opt ? js_export_opt_plan(imgs.data(), imgs.size(), spec, images, n, js_export_q, this, recs, orecs, unit_base, h_pack + blk.hdrs, unsupported.data(), &blocks)
            : js_export_plan(imgs.data(), imgs.size(), spec, images, n, js_export_q, this, recs, unit_base, h_pack + blk.hdrs, unsupported.data(), &blocks)) return -1;
    JsExportRstRec* rrecs = rst ? reinterpret_cast<JsExportRstRec*>(h_pack + rblk.rrecs) : nullptr;
    std::vector<uint64_t> ri((size_t)n, 0); uint64_t intervals = 0;
    if (rst && js_export_rst_plan(imgs.data(), restart, images, n, recs, orecs, rrecs, unit_base, h_pack + blk.hdrs, unsupported.data(), ri.data(), &blocks, &intervals)) return -1;
    memset(chunk_base, 0, ((size_t)n + 1) * 4);
    js_export_code_tabs(reinterpret_cast<uint32_t*>(h_pack + blk.tabs));
    if (ensure_generic()) return -1;
    const uint32_t units = unit_base[n];
    const JsExportRstScratch rsc = js_export_rst_scratch((size_t)n, units, blocks, intervals, opt);
    const JsExportOptScratch osc = rst ? rsc.o : js_export_opt_scratch((size_t)n, units, blocks);
    const JsExportScratch sc = rst ? rsc.o.s : (opt ? osc.s : js_export_scratch((size_t)n, units, blocks));
    const JsExportOptKeep keep = js_export_opt_keep((size_t)n);
    if (js_export_grow(&d_export_tmp, &d_export_tmp_cap, sc.total)) return -1;
    if (opt && js_export_grow(&d_export_opt, &d_export_opt_cap, keep.total)) return -1;
    if (pack_send(blk.total)) return -1;
    HIP_TRY(hipMemsetAsync(d_export_tmp + sc.res, 0, (size_t)n * 4, stream));
    HIP_TRY(hipMemsetAsync(d_export_tmp + sc.res + (size_t)n * 4, 0xFF, (size_t)n * 8, stream));
    HIP_TRY(hipMemsetAsync(d_export_tmp + sc.len, 0, (size_t)n * 8, stream));
    const JsExportRec* d_recs = reinterpret_cast<const JsExportRec*>(d_pack + blk.recs);
    const uint32_t* d_unit_base = reinterpret_cast<const uint32_t*>(d_pack + blk.unit_base); const uint32_t* d_tabs = reinterpret_cast<const uint32_t*>(d_pack + blk.tabs);
    uint16_t* d_blk_bits = reinterpret_cast<uint16_t*>(d_export_tmp + sc.blk_bits); uint64_t* d_unit_off = reinterpret_cast<uint64_t*>(d_export_tmp + sc.unit_off);
    const JsExportRstRec* d_rrecs = rst ? reinterpret_cast<const JsExportRstRec*>(d_pack + rblk.rrecs) : nullptr;
    if (opt) HIP_TRY(hipMemsetAsync(d_export_opt + keep.stats, 0, (size_t)n * sizeof(JsExportOptStat), stream));
    if (rst) {
        if (js_launch_export_measure_rst(stream, dev.coef, dev.dccum, d_recs, opt ? reinterpret_cast<const JsExportOptRec*>(d_pack + oblk.orecs) : nullptr, d_rrecs, d_unit_base, (uint32_t)n, units,
                                         d_tabs, d_pack + blk.hdrs, opt ? reinterpret_cast<JsExportOptStat*>(d_export_opt + keep.stats) : nullptr,
                                         opt ? reinterpret_cast<uint32_t*>(d_export_opt + keep.tabs) : nullptr, opt ? d_export_opt + keep.hdrs : nullptr,
                                         opt ? reinterpret_cast<uint32_t*>(d_export_tmp + osc.hdr_len) : nullptr, d_blk_bits, reinterpret_cast<JsRstSum*>(d_export_tmp + rsc.sums), d_unit_off,
                                         reinterpret_cast<uint32_t*>(d_export_tmp + sc.res), reinterpret_cast<uint64_t*>(d_export_tmp + sc.ent_bits))) {
            js_set_error("export_jpeg: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    } else if (opt) {
        if (js_launch_export_measure_opt(stream, dev.coef, dev.dccum, d_recs, reinterpret_cast<const JsExportOptRec*>(d_pack + oblk.orecs), d_unit_base, (uint32_t)n, units, d_tabs,
                                         d_pack + blk.hdrs, reinterpret_cast<JsExportOptStat*>(d_export_opt + keep.stats), reinterpret_cast<uint32_t*>(d_export_opt + keep.tabs),
                                         d_export_opt + keep.hdrs, reinterpret_cast<uint32_t*>(d_export_tmp + osc.hdr_len), d_blk_bits, reinterpret_cast<uint32_t*>(d_export_tmp + sc.unit_bits),
                                         d_unit_off, reinterpret_cast<uint32_t*>(d_export_tmp + sc.res), reinterpret_cast<uint64_t*>(d_export_tmp + sc.ent_bits))) {
            js_set_error("export_jpeg: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    } else if (js_launch_export_measure(stream, dev.coef, dev.dccum, d_recs, d_unit_base, (uint32_t)n, units, d_tabs, d_blk_bits, reinterpret_cast<uint32_t*>(d_export_tmp + sc.unit_bits),
                                 d_unit_off, reinterpret_cast<uint32_t*>(d_export_tmp + sc.res), reinterpret_cast<uint64_t*>(d_export_tmp + sc.ent_bits))) {
        js_set_error("export_jpeg: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    std::vector<uint8_t> back(sc.len);
    if (d2h_staged(back.data(), d_export_tmp, sc.len)) return -1;                                    // ---- wait 1
    std::vector<int> result((size_t)n); std::vector<uint32_t> detail((size_t)n);
    uint64_t u_bytes = 0, out_bytes = 0;
    if (pack_block(blk.total)) return -1;
    if (rst ? js_export_rst_layout(recs, orecs, rrecs, n, unsupported.data(), reinterpret_cast<const uint32_t*>(back.data() + sc.res), reinterpret_cast<const uint64_t*>(back.data() + sc.ent_bits),
                                   opt ? reinterpret_cast<const uint32_t*>(back.data() + osc.hdr_len) : nullptr, chunk_base, result.data(), detail.data(), &u_bytes, &out_bytes)
      : opt ? js_export_opt_layout(recs, orecs, n, unsupported.data(), reinterpret_cast<const uint32_t*>(back.data() + sc.res), reinterpret_cast<const uint64_t*>(back.data() + sc.ent_bits),
                                   reinterpret_cast<const uint32_t*>(back.data() + osc.hdr_len), chunk_base, result.data(), detail.data(), &u_bytes, &out_bytes)
            : js_export_layout(recs, n, unsupported.data(), reinterpret_cast<const uint32_t*>(back.data() + sc.res), reinterpret_cast<const uint64_t*>(back.data() + sc.ent_bits),
                               chunk_base, result.data(), detail.data(), &u_bytes, &out_bytes)) return -1;
    const uint32_t chunks = chunk_base[n];
    std::vector<uint64_t> len((size_t)n, 0);
    if (chunks) {
        const size_t ff_at = 0, off_at = ((size_t)chunks * 4 + 15u) & ~(size_t)15u, u_at = (off_at + (size_t)chunks * 8 + 15u) & ~(size_t)15u;      // the chunk tables in front of the streams (which start on 16 bytes)
        if (js_export_grow(&d_export_u, &d_export_u_cap, u_at + u_bytes) || js_export_grow(&d_export_out, &d_export_out_cap, out_bytes)) return -1;
        if (pack_send(blk.total)) return -1;
        HIP_TRY(hipMemsetAsync(d_export_u + u_at, 0, u_bytes, stream));
        if (rst ? js_launch_export_write_rst(stream, dev.coef, dev.dccum, d_recs, d_rrecs, d_unit_base, reinterpret_cast<const uint32_t*>(d_pack + blk.chunk_base), (uint32_t)n, units, chunks,
                                             opt ? reinterpret_cast<const uint32_t*>(d_export_opt + keep.tabs) : d_tabs, opt ? JS_EXPORT_TAB_WORDS : 0u, d_blk_bits, d_unit_off,
                                             reinterpret_cast<uint64_t*>(d_export_tmp + rsc.itab), d_export_u + u_at, reinterpret_cast<uint32_t*>(d_export_u + ff_at),
                                             reinterpret_cast<uint64_t*>(d_export_u + off_at), reinterpret_cast<uint64_t*>(d_export_tmp + sc.ent_ff), opt ? d_export_opt + keep.hdrs : d_pack + blk.hdrs,
                                             d_export_out, reinterpret_cast<uint64_t*>(d_export_tmp + sc.len))
          : opt ? js_launch_export_write_opt(stream, dev.coef, dev.dccum, d_recs, d_unit_base, reinterpret_cast<const uint32_t*>(d_pack + blk.chunk_base), (uint32_t)n, units, chunks,
                                             reinterpret_cast<const uint32_t*>(d_export_opt + keep.tabs), d_blk_bits, d_unit_off, d_export_u + u_at, reinterpret_cast<uint32_t*>(d_export_u + ff_at),
                                             reinterpret_cast<uint64_t*>(d_export_u + off_at), reinterpret_cast<uint64_t*>(d_export_tmp + sc.ent_ff), d_export_opt + keep.hdrs, d_export_out,
                                             reinterpret_cast<uint64_t*>(d_export_tmp + sc.len))
                : js_launch_export_write(stream, dev.coef, dev.dccum, d_recs, d_unit_base, reinterpret_cast<const uint32_t*>(d_pack + blk.chunk_base), (uint32_t)n, units, chunks, d_tabs,
                                   d_blk_bits, d_unit_off, d_export_u + u_at, reinterpret_cast<uint32_t*>(d_export_u + ff_at), reinterpret_cast<uint64_t*>(d_export_u + off_at),
                                   reinterpret_cast<uint64_t*>(d_export_tmp + sc.ent_ff), d_pack + blk.hdrs, d_export_out, reinterpret_cast<uint64_t*>(d_export_tmp + sc.len))) {
            js_set_error("export_jpeg: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
        if (d2h_staged(len.data(), d_export_tmp + sc.len, (size_t)n * 8)) return -1;                  // ---- wait 2
    }
    for (int k = 0; k < n; k++) {
        JsExportEntry e; e.off = recs[k].out_off; e.len = recs[k].live ? len[k] : 0; e.result = result[k]; e.detail = detail[k]; e.image = images ? images[k] : k;
        e.ri = (uint32_t)ri[(size_t)k]; e.intervals = recs[k].live ? (rst ? rrecs[k].ni : 1u) : 0u;
        if (recs[k].live && (e.len < recs[k].hdr_len + 3u || e.len > recs[k].out_cap)) {
            exports.clear(); js_set_error("export_jpeg: entry %d came back with %llu bytes, its place holds %llu", k, (unsigned long long)e.len, (unsigned long long)recs[k].out_cap); return -1; }
        exports.push_back(e);
    }
    export_opt = opt;
    return 0;
}

int JsnoopBatch::export_tables(int k, int slot, uint8_t* counts, uint8_t* symbols, uint32_t* nsym, uint32_t* freq)
{
    if (k < 0 || (size_t)k >= exports.size()) { js_set_error("export_tables: entry %d out of range, the last export holds %zu", k, exports.size()); return -1; }
    if (export_prog) { js_set_error("export_tables: the last export wrote progressive files, whose tables belong to scans: jsnoop_batch_export_scan_tables returns them"); return -1; }
    if (!export_opt || !d_export_opt) { js_set_error("export_tables: the last export wrote the Annex K tables (huffman = 0): it built none"); return -1; }
    const JsExportEntry& e = exports[(size_t)k];
    if (e.result != JSNOOP_EXPORT_OK) { js_set_error("export_tables: entry %d was not exported (result %d): it has no tables", k, e.result); return -1; }
    const int nslots = imgs[(size_t)e.image].ncomp == 1u ? 2 : 4;
    if (slot < 0 || slot >= nslots) { js_set_error("export_tables: slot %d, image %d has slots 0 .. %d", slot, e.image, nslots - 1); return -1; }
    HIP_TRY(hipSetDevice(device));
    const JsExportOptKeep keep = js_export_opt_keep(exports.size());
    std::vector<JsExportOptStat> st(1);
    if (d2h_staged(st.data(), d_export_opt + keep.stats + (size_t)k * sizeof(JsExportOptStat), sizeof(JsExportOptStat))) return -1;
    const JsExportOptSlot& s = st[0].slot[slot];
    if (s.nsym > 256u) { js_set_error("export_tables: entry %d, slot %d came back with %u symbols", k, slot, s.nsym); return -1; }
    if (counts) memcpy(counts, s.counts, 16);
    if (symbols) memcpy(symbols, s.syms, 256);
    if (nsym) *nsym = s.nsym;
    if (freq) {
        memset(freq, 0, 256 * 4);
        if (slot & 1) memcpy(freq, st[0].freq + 32 + (slot >> 1) * 256, 256 * 4); else memcpy(freq, st[0].freq + (slot >> 1) * 16, 16 * 4);
    }
    return 0;
}

// Progressive files (jsnoop_export_prog_check.h has the arithmetic, DESIGN.md 4.17 the contract).  The same two phases and two waits with a record per (entry, scan):
//   1. k_prog_classify, k_prog_runs, k_prog_symbols, k_prog_huff, k_prog_measure, k_export_rst_scan; result words, the scans' stream lengths and header-piece
//      lengths come back (wait 1): the host sizes the un-stuffed streams and the files.
//   2. the streams zeroed, k_prog_bits, k_prog_ffcount, k_export_scan, k_prog_place, k_prog_stuff; the file lengths, the scans' places and FF counts come back (wait 2).
int JsnoopBatch::export_jpeg_prog(const JsnoopExportSpec* spec_in, const JsnoopExportCoding* coding_in, const JsnoopExportRestart* restart_in, const JsnoopExportProgressive* prog_in,
                                  const int* images, int n)
{
    JsnoopExportProgressive prog;
    if (js_export_import_progressive(prog_in, &prog)) return -1;
    if (prog.mode == JSNOOP_PROGRESSIVE_OFF) return export_jpeg_rst(spec_in, coding_in, restart_in, images, n);
    JsnoopExportCoding coding;
    if (js_export_import_coding(coding_in, &coding)) return -1;      // (validated; both values write the scans' own tables)
    JsnoopExportRestart restart;
    if (js_export_import_restart(restart_in, &restart)) return -1;
    std::vector<JsnoopExportScan> script3, script1;
    if (prog.mode == JSNOOP_PROGRESSIVE_DEFAULT) {
        script3.resize(6); script1.resize(4);
        js_export_prog_default(3u, script3.data()); js_export_prog_default(1u, script1.data());
    } else {
        uint32_t nc = 0;
        if (js_export_prog_validate(prog.scans, prog.nscans, &nc)) return -1;
        (nc == 1u ? script1 : script3).assign(prog.scans, prog.scans + prog.nscans);
    }
    if (!uploaded || last_form == 0 || !dev.coef || !dev.dccum) { js_set_error("export_jpeg: the batch has not been decoded"); return -1; }
    JsnoopExportSpec spec;
    if (js_export_import_spec(spec_in, &spec)) return -1;
    if (n < 0) { js_set_error("export_jpeg: n = %d", n); return -1; }
    if (!images && (size_t)n > imgs.size()) { js_set_error("export_jpeg: n = %d without a list, the batch holds %zu", n, imgs.size()); return -1; }
    const JsnoopExportScan* s3 = script3.empty() ? nullptr : script3.data(); const JsnoopExportScan* s1 = script1.empty() ? nullptr : script1.data();
    const uint32_t n3 = (uint32_t)script3.size(), n1 = (uint32_t)script1.size();
    std::vector<uint8_t> refused((size_t)n), unsupported((size_t)n);
    size_t nrec = 0;
    if (js_export_prog_count(imgs.data(), imgs.size(), images, n, restart, s3, n3, s1, n1, refused.data(), &nrec)) return -1;      // (an index out of range too leaves the previous export)
    exports.clear(); export_opt = false; export_prog = false; export_scans.clear(); export_scan_base.clear();
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    const JsExportProgBlock blk = js_export_prog_block((size_t)n, nrec);
    if (pack_block(blk.b.total)) return -1;
    JsExportRec* recs = reinterpret_cast<JsExportRec*>(h_pack + blk.b.recs);
    uint32_t* rec_base = reinterpret_cast<uint32_t*>(h_pack + blk.b.unit_base);
    JsExportScanRec* srecs = reinterpret_cast<JsExportScanRec*>(h_pack + blk.srecs);
    uint32_t* tile_base = reinterpret_cast<uint32_t*>(h_pack + blk.tile_base); uint32_t* chunk_base = reinterpret_cast<uint32_t*>(h_pack + blk.chunk_base);
    uint64_t blocks = 0, units = 0, intervals = 0;
    if (js_export_plan(imgs.data(), imgs.size(), spec, images, n, js_export_q, this, recs, rec_base, h_pack + blk.b.hdrs, unsupported.data(), &blocks)) return -1;
    for (int k = 0; k < n; k++) unsupported[(size_t)k] |= refused[(size_t)k];
    if (js_export_prog_plan(imgs.data(), images, n, restart, s3, n3, s1, n1, recs, unsupported.data(), h_pack + blk.b.hdrs, (uint32_t)(blk.posts - blk.b.hdrs), srecs, rec_base, tile_base,
                            &units, &intervals)) return -1;
    if (rec_base[n] != nrec) { js_set_error("export_jpeg: %u scan records planned, %zu counted", rec_base[n], nrec); return -1; }
    memset(chunk_base, 0, (nrec + 1) * 4);
    if (ensure_generic()) return -1;
    const uint32_t tiles = tile_base[nrec];
    const JsExportProgScratch sc = js_export_prog_scratch((size_t)n, nrec, tiles, units, intervals);
    const JsExportProgKeep keep = js_export_prog_keep(nrec);
    if (js_export_grow(&d_export_tmp, &d_export_tmp_cap, sc.total) || js_export_grow(&d_export_opt, &d_export_opt_cap, keep.total)) return -1;
    if (pack_send(blk.b.total)) return -1;
    HIP_TRY(hipMemsetAsync(d_export_tmp + sc.res, 0, (size_t)n * 4, stream));
    HIP_TRY(hipMemsetAsync(d_export_tmp + sc.res + (size_t)n * 4, 0xFF, (size_t)n * 8, stream));
    HIP_TRY(hipMemsetAsync(d_export_tmp + sc.rec_bits, 0, sc.back2 - sc.rec_bits, stream));
    if (nrec) HIP_TRY(hipMemsetAsync(d_export_opt + keep.stats, 0, nrec * sizeof(JsExportScanStat), stream));      // (a call in which every entry is unsupported has no record)
    const JsExportRec* d_recs = reinterpret_cast<const JsExportRec*>(d_pack + blk.b.recs); const JsExportScanRec* d_srecs = reinterpret_cast<const JsExportScanRec*>(d_pack + blk.srecs);
    const uint32_t* d_tile_base = reinterpret_cast<const uint32_t*>(d_pack + blk.tile_base);
    uint32_t* d_tabs = reinterpret_cast<uint32_t*>(d_export_opt + keep.tabs); uint32_t* d_hdr_len = reinterpret_cast<uint32_t*>(d_export_tmp + sc.hdr_len);
    uint16_t* d_eob = reinterpret_cast<uint16_t*>(d_export_tmp + sc.eob); uint16_t* d_blk_bits = reinterpret_cast<uint16_t*>(d_export_tmp + sc.blk_bits);
    uint64_t* d_tile_off = reinterpret_cast<uint64_t*>(d_export_tmp + sc.tile_off);
    if (js_launch_export_prog_measure(stream, dev.coef, dev.dccum, d_recs, d_srecs, d_tile_base, (uint32_t)n, (uint32_t)nrec, tiles, d_pack + blk.b.hdrs,
                                      reinterpret_cast<JsExportScanStat*>(d_export_opt + keep.stats), d_tabs, d_export_opt + keep.hdrs, d_hdr_len, d_export_tmp + sc.cls, d_eob, d_blk_bits,
                                      reinterpret_cast<JsRstSum*>(d_export_tmp + sc.sums), d_tile_off, reinterpret_cast<uint32_t*>(d_export_tmp + sc.res),
                                      reinterpret_cast<uint64_t*>(d_export_tmp + sc.rec_bits))) {
        js_set_error("export_jpeg: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    std::vector<uint8_t> back(sc.back2);
    if (d2h_staged(back.data(), d_export_tmp, sc.back1)) return -1;                                  // ---- wait 1
    const uint32_t* hdr_len = reinterpret_cast<const uint32_t*>(back.data() + sc.hdr_len);
    std::vector<int> result((size_t)n); std::vector<uint32_t> detail((size_t)n);
    uint64_t u_bytes = 0, out_bytes = 0;
    if (pack_block(blk.b.total)) return -1;
    if (js_export_prog_layout(recs, srecs, rec_base, n, unsupported.data(), reinterpret_cast<const uint32_t*>(back.data() + sc.res), reinterpret_cast<const uint64_t*>(back.data() + sc.rec_bits),
                              hdr_len, chunk_base, result.data(), detail.data(), &u_bytes, &out_bytes)) return -1;
    const uint32_t chunks = chunk_base[nrec];
    if (chunks) {
        const size_t ff_at = 0, off_at = ((size_t)chunks * 4 + 15u) & ~(size_t)15u, u_at = (off_at + (size_t)chunks * 8 + 15u) & ~(size_t)15u;
        if (js_export_grow(&d_export_u, &d_export_u_cap, u_at + u_bytes) || js_export_grow(&d_export_out, &d_export_out_cap, out_bytes)) return -1;
        if (pack_send(blk.b.total)) return -1;
        HIP_TRY(hipMemsetAsync(d_export_u + u_at, 0, u_bytes, stream));
        if (js_launch_export_prog_write(stream, dev.coef, dev.dccum, d_recs, d_srecs, reinterpret_cast<const uint32_t*>(d_pack + blk.b.unit_base), d_tile_base,
                                        reinterpret_cast<const uint32_t*>(d_pack + blk.chunk_base), (uint32_t)n, (uint32_t)nrec, tiles, chunks, d_tabs, d_eob, d_blk_bits, d_tile_off,
                                        reinterpret_cast<uint64_t*>(d_export_tmp + sc.itab), d_export_u + u_at, reinterpret_cast<uint32_t*>(d_export_u + ff_at),
                                        reinterpret_cast<uint64_t*>(d_export_u + off_at), reinterpret_cast<uint64_t*>(d_export_tmp + sc.rec_ff), d_export_opt + keep.hdrs, d_hdr_len,
                                        reinterpret_cast<uint64_t*>(d_export_tmp + sc.scan_out), d_export_out, reinterpret_cast<uint64_t*>(d_export_tmp + sc.len))) {
            js_set_error("export_jpeg: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
        if (d2h_staged(back.data() + sc.len, d_export_tmp + sc.len, sc.back2 - sc.len)) return -1;     // ---- wait 2
    } else memset(back.data() + sc.len, 0, sc.back2 - sc.len);
    const uint64_t* len = reinterpret_cast<const uint64_t*>(back.data() + sc.len); const uint64_t* scan_out = reinterpret_cast<const uint64_t*>(back.data() + sc.scan_out);
    const uint64_t* rec_ff = reinterpret_cast<const uint64_t*>(back.data() + sc.rec_ff);
    for (int k = 0; k < n; k++) {
        const JsImage& im = imgs[(size_t)(images ? images[k] : k)];
        const std::vector<JsnoopExportScan>& script = im.ncomp == 1u ? script1 : script3;
        JsExportEntry e; e.off = recs[k].out_off; e.len = recs[k].live ? len[k] : 0; e.result = result[(size_t)k]; e.detail = detail[(size_t)k]; e.image = images ? images[k] : k;
        if (recs[k].live && (e.len < 4u || e.len > recs[k].out_cap)) {
            exports.clear(); export_scans.clear(); export_scan_base.clear();
            js_set_error("export_jpeg: entry %d came back with %llu bytes, its place holds %llu", k, (unsigned long long)e.len, (unsigned long long)recs[k].out_cap); return -1; }
        export_scan_base.push_back((uint32_t)export_scans.size());
        for (uint32_t i = rec_base[k]; recs[k].live && i < rec_base[k + 1]; i++) {
            const JsExportScanRec& p = srecs[i];
            JsExportScanInfo si; si.sc = script[p.scan]; si.ri = p.ri / p.spm; si.rec = i; si.ntab = p.ntab; si.kind = p.kind; si.intervals = p.ni;
            si.sos_offset = scan_out[i] + hdr_len[i] - (8u + 2u * (uint32_t)__builtin_popcount(si.sc.comps)); si.data_bytes = (p.bits >> 3) + rec_ff[i] + 2u * (uint64_t)(p.ni - 1u);
            export_scans.push_back(si);
        }
        if (recs[k].live) { const JsExportScanRec& p = srecs[rec_base[k]]; e.ri = p.ri / p.spm; e.intervals = p.ni; }
        exports.push_back(e);
    }
    export_scan_base.push_back((uint32_t)export_scans.size());
    export_prog = true; export_prog_nrec = nrec;
    return 0;
}

int JsnoopBatch::export_scan_tables(int k, int scan, int slot, uint8_t* counts, uint8_t* symbols, uint32_t* nsym, uint32_t* freq)
{
    if (k < 0 || (size_t)k >= exports.size()) { js_set_error("export_scan_tables: entry %d out of range, the last export holds %zu", k, exports.size()); return -1; }
    if (!export_prog || !d_export_opt || export_scan_base.size() != exports.size() + 1) { js_set_error("export_scan_tables: the last export wrote no progressive files"); return -1; }
    const int ns = (int)(export_scan_base[(size_t)k + 1] - export_scan_base[(size_t)k]);
    if (!ns) { js_set_error("export_scan_tables: entry %d was not exported (result %d): it has no tables", k, exports[(size_t)k].result); return -1; }
    if (scan < 0 || scan >= ns) { js_set_error("export_scan_tables: scan %d, entry %d has scans 0 .. %d", scan, k, ns - 1); return -1; }
    const JsExportScanInfo& si = export_scans[export_scan_base[(size_t)k] + (size_t)scan];
    if (slot < 0 || (uint32_t)slot >= si.ntab) { js_set_error("export_scan_tables: slot %d, scan %d of entry %d has %u tables", slot, scan, k, si.ntab); return -1; }
    HIP_TRY(hipSetDevice(device));
    const JsExportProgKeep keep = js_export_prog_keep(export_prog_nrec);
    std::vector<JsExportScanStat> st(1);
    if (d2h_staged(st.data(), d_export_opt + keep.stats + (size_t)si.rec * sizeof(JsExportScanStat), sizeof(JsExportScanStat))) return -1;
    const JsExportOptSlot& s = st[0].slot[slot];
    if (s.nsym > 256u) { js_set_error("export_scan_tables: entry %d, scan %d, slot %d came back with %u symbols", k, scan, slot, s.nsym); return -1; }
    if (counts) memcpy(counts, s.counts, 16);
    if (symbols) memcpy(symbols, s.syms, 256);
    if (nsym) *nsym = s.nsym;
    if (freq) {
        memset(freq, 0, 256 * 4);
        if (si.kind == JS_PROG_AC_FIRST) memcpy(freq, st[0].freq + 48, 256 * 4); else memcpy(freq, st[0].freq + slot * 16, 16 * 4);
    }
    return 0;
}

static const char* js_export_reason(int result)
{
    switch (result) {
    case JSNOOP_EXPORT_INEXACT: return "a value is no multiple of its quantiser (INEXACT)";
    case JSNOOP_EXPORT_UNCODABLE: return "a level has no Annex K code (UNCODABLE)";
    case JSNOOP_EXPORT_UNSUPPORTED: return "the sample precision is not 8, or the restart interval is above 65535 (UNSUPPORTED)";
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
void jsnoop_export_coding_defaults(JsnoopExportCoding* out) { if (out) js_export_coding_defaults(out); }
int jsnoop_batch_export_jpeg_coded(JsnoopBatch* b, const JsnoopExportSpec* spec, const JsnoopExportCoding* coding, const int* images, int n)
{
    if (!b) { js_set_error("export_jpeg: batch is NULL"); return -1; }
    if (!coding) { js_set_error("export_jpeg: coding is NULL"); return -1; }
    return b->export_jpeg_coded(spec, coding, images, n);
}
int jsnoop_batch_export_tables(JsnoopBatch* b, int k, int slot, uint8_t counts[16], uint8_t symbols[256], uint32_t* nsym, uint32_t freq[256])
{
    if (!b) { js_set_error("export_tables: batch is NULL"); return -1; }
    return b->export_tables(k, slot, counts, symbols, nsym, freq);
}
void jsnoop_export_restart_defaults(JsnoopExportRestart* out) { if (out) js_export_restart_defaults(out); }
int jsnoop_batch_export_jpeg_rst(JsnoopBatch* b, const JsnoopExportSpec* spec, const JsnoopExportCoding* coding, const JsnoopExportRestart* restart, const int* images, int n)
{
    if (!b) { js_set_error("export_jpeg: batch is NULL"); return -1; }
    return b->export_jpeg_rst(spec, coding, restart, images, n);
}
int jsnoop_batch_export_restart(const JsnoopBatch* b, int k, uint32_t* ri, uint64_t* intervals)
{
    const JsExportEntry* e = js_export_entry(b, k, "export_restart");
    if (!e) return -1;
    if (ri) *ri = e->ri;
    if (intervals) *intervals = e->intervals;
    return 0;
}
void jsnoop_export_progressive_defaults(JsnoopExportProgressive* out) { if (out) js_export_progressive_defaults(out); }
int jsnoop_batch_export_jpeg_prog(JsnoopBatch* b, const JsnoopExportSpec* spec, const JsnoopExportCoding* coding, const JsnoopExportRestart* restart, const JsnoopExportProgressive* prog,
                                  const int* images, int n)
{
    if (!b) { js_set_error("export_jpeg: batch is NULL"); return -1; }
    return b->export_jpeg_prog(spec, coding, restart, prog, images, n);
}
int jsnoop_batch_export_scan_count(const JsnoopBatch* b, int k)
{
    if (!b || !b->export_prog || k < 0 || (size_t)k >= b->exports.size() || b->export_scan_base.size() != b->exports.size() + 1) return 0;
    return (int)(b->export_scan_base[(size_t)k + 1] - b->export_scan_base[(size_t)k]);
}
int jsnoop_batch_export_scan_info(const JsnoopBatch* b, int k, int scan, JsnoopExportScan* sc, uint32_t* ri, uint64_t* intervals, uint64_t* sos_offset, uint64_t* data_bytes)
{
    if (!js_export_entry(b, k, "export_scan_info")) return -1;
    const int ns = jsnoop_batch_export_scan_count(b, k);
    if (scan < 0 || scan >= ns) { js_set_error("export_scan_info: scan %d, entry %d has %d scans", scan, k, ns); return -1; }
    const JsnoopBatch::JsExportScanInfo& si = b->export_scans[b->export_scan_base[(size_t)k] + (size_t)scan];
    if (sc) *sc = si.sc;
    if (ri) *ri = si.ri;
    if (intervals) *intervals = si.intervals;
    if (sos_offset) *sos_offset = si.sos_offset;
    if (data_bytes) *data_bytes = si.data_bytes;
    return 0;
}
int jsnoop_batch_export_scan_tables(JsnoopBatch* b, int k, int scan, int slot, uint8_t counts[16], uint8_t symbols[256], uint32_t* nsym, uint32_t freq[256])
{
    if (!b) { js_set_error("export_scan_tables: batch is NULL"); return -1; }
    return b->export_scan_tables(k, scan, slot, counts, symbols, nsym, freq);
}
int jsnoop_export_jpeg(JsnoopDecoder* d, const char* path) { return jsnoop_export_jpeg_rst(d, path, nullptr, nullptr); }
int jsnoop_export_jpeg_coded(JsnoopDecoder* d, const char* path, const JsnoopExportCoding* coding) { return jsnoop_export_jpeg_rst(d, path, coding, nullptr); }
int jsnoop_export_jpeg_rst(JsnoopDecoder* d, const char* path, const JsnoopExportCoding* coding, const JsnoopExportRestart* restart) { return jsnoop_export_jpeg_prog(d, path, coding, restart, nullptr); }
int jsnoop_export_jpeg_prog(JsnoopDecoder* d, const char* path, const JsnoopExportCoding* coding, const JsnoopExportRestart* restart, const JsnoopExportProgressive* prog)
{
    if (!d || !path) { js_set_error("jsnoop_export_jpeg: bad argument"); return -1; }
    if (!d->have_image || !d->preview_is_jpeg || !d->batch) { js_set_error("jsnoop_export_jpeg: no decoded image"); return -1; }
    d->arena_generic();
    JsnoopBatch* b = d->batch;
    JsnoopExportSpec spec; js_export_spec_defaults(&spec);
    const int img = d->img;
    if (b->export_jpeg_prog(&spec, coding, restart, prog, &img, 1)) return -1;
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
