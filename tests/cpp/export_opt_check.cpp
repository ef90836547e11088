// Host-only program: the host arithmetic jsnoop_batch_export_jpeg_coded adds for JSNOOP_HUFFMAN_OPTIMAL (jpegsnoop_amd/csrc/jsnoop_export_opt_check.h) on
// hand-made image descriptors -- the coding spec and its refusals, the 2^26-block refusal, the side records (where a header splits around its DHT segments),
// the call's block and scratch, and the second phase's layout with the header lengths the device returns.  tests/test_export_opt_abi.py builds it with the
// address and undefined-behaviour sanitizers and runs it.  Prints "ok" and returns 0, or the line that failed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#ifndef __HIPCC__
#define __host__
#define __device__
#endif
#include "../../jpegsnoop_amd/csrc/jsnoop_export_opt_check.h"

static std::string g_err;
void js_set_error(const char* fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)

static JsImage image(uint32_t ncomp, const uint32_t (*hv)[2], uint32_t dim_x, uint32_t dim_y, uint64_t coef_off = 0)
{
    JsImage im; memset(&im, 0, sizeof im);
    im.ncomp = ncomp; im.dim_x = dim_x; im.dim_y = dim_y; im.coef_off = coef_off; im.precision = 8;
    uint32_t hmax = 0, vmax = 0, nb = 0;
    for (uint32_t c = 1; c <= ncomp; c++) {
        im.samp_h[c] = hv[c - 1][0]; im.samp_v[c] = hv[c - 1][1];
        if (im.samp_h[c] > hmax) hmax = im.samp_h[c];
        if (im.samp_v[c] > vmax) vmax = im.samp_v[c];
        for (uint32_t v = 0; v < im.samp_v[c]; v++) for (uint32_t h = 0; h < im.samp_h[c]; h++) { im.blk_comp[nb] = (uint8_t)c; im.blk_ch[nb] = (uint8_t)h; im.blk_cv[nb] = (uint8_t)v; nb++; }
    }
    im.blk_per_mcu = nb; im.mcu_w = hmax * 8; im.mcu_h = vmax * 8;
    im.mcu_xmax = (dim_x + im.mcu_w - 1) / im.mcu_w; im.mcu_ymax = (dim_y + im.mcu_h - 1) / im.mcu_h;
    im.total_blocks = im.mcu_xmax * im.mcu_ymax * nb;
    return im;
}
static uint16_t g_q[3] = { 3, 5, 7 };
static int qfn(void*, int, int comp, uint16_t* out64) { for (int k = 0; k < 64; k++) out64[k] = g_q[comp]; return 0; }

int main()
{
    static const uint32_t k420[3][2] = { { 2, 2 }, { 1, 1 }, { 1, 1 } }, kGrey[1][2] = { { 1, 1 } };
    // image 2: 8192 x 8192 grey blocks = 2^26 exactly; image 3: one block row fewer
    std::vector<JsImage> imgs = { image(3, k420, 333, 217, 64), image(1, kGrey, 1, 1, 1 << 20), image(1, kGrey, 65535, 65535, 128), image(1, kGrey, 65535, 65528, 256) };
    CHECK(imgs[2].total_blocks == JS_EXPORT_OPT_MAX_BLOCKS && imgs[3].total_blocks == JS_EXPORT_OPT_MAX_BLOCKS - 8192u);
    CHECK(sizeof(JsnoopExportCoding) == 8 && sizeof(JsExportOptRec) == 16 && sizeof(JsExportOptSlot) == 276 && sizeof(JsExportOptStat) == 544 * 4 + 4 * 276 && sizeof(JsExportOptStat) % 4 == 0);
    CHECK(63ull * (JS_EXPORT_OPT_MAX_BLOCKS - 1u) < (1ull << 32));

    // coding spec: defaults, NULL, shorter accepted, longer and an unknown mode refused
    JsnoopExportCoding def; memset(&def, 0xEE, sizeof def); js_export_coding_defaults(&def);
    CHECK(def.struct_size == 8 && def.huffman == JSNOOP_HUFFMAN_ANNEX_K);
    JsnoopExportCoding in = def, c;
    CHECK(js_export_import_coding(nullptr, &c) == 0 && c.huffman == 0 && c.struct_size == 8);
    in.huffman = JSNOOP_HUFFMAN_OPTIMAL; CHECK(js_export_import_coding(&in, &c) == 0 && c.huffman == 1);
    in.struct_size = 4; CHECK(js_export_import_coding(&in, &c) == 0 && c.huffman == 0 && c.struct_size == 8);
    in.struct_size = 12; CHECK(js_export_import_coding(&in, &c) == -1 && g_err.find("struct_size") != std::string::npos);
    in.struct_size = 0; CHECK(js_export_import_coding(&in, &c) == -1);
    in.struct_size = 8; in.huffman = 2; CHECK(js_export_import_coding(&in, &c) == -1 && g_err.find("huffman = 2") != std::string::npos);
    in.huffman = -1; CHECK(js_export_import_coding(&in, &c) == -1 && g_err.find("huffman = -1") != std::string::npos);

    // the plan: side records split every header at its first DHT and at SOS; 2^26 blocks are refused on the host and own no unit
    JsnoopExportSpec spec; js_export_spec_defaults(&spec);
    const int list[] = { 0, 2, 1, 3, 0 }; const int n = 5;
    const JsExportOptBlock ob = js_export_opt_block((size_t)n); const JsExportBlock plain = js_export_block((size_t)n);
    CHECK(ob.orecs == plain.total && ob.b.total >= ob.orecs + n * sizeof(JsExportOptRec) && !(ob.b.total % 16) && ob.b.hdrs == plain.hdrs && ob.b.recs == plain.recs);
    std::vector<JsExportRec> recs((size_t)n); std::vector<JsExportOptRec> orecs((size_t)n); std::vector<uint32_t> base((size_t)n + 1, 0xA5A5A5A5u);
    std::vector<uint8_t> hdrs((size_t)n * JS_EXPORT_HDR_MAX, 0xA5), uns((size_t)n, 0xA5); uint64_t blocks = 0;
    CHECK(js_export_opt_plan(imgs.data(), imgs.size(), spec, list, n, qfn, nullptr, recs.data(), orecs.data(), base.data(), hdrs.data(), uns.data(), &blocks) == 0);
    CHECK(!uns[0] && uns[1] == 1 && !uns[2] && !uns[3] && !uns[4]);
    const uint32_t u0 = (imgs[0].total_blocks + JS_EXPORT_TILE - 1) / JS_EXPORT_TILE, u3 = imgs[3].total_blocks / JS_EXPORT_TILE;
    CHECK(base[0] == 0 && base[1] == u0 && base[2] == u0 && base[3] == u0 + 1 && base[4] == u0 + 1 + u3 && base[5] == 2 * u0 + 1 + u3);
    CHECK(recs[2].blk_base == imgs[0].total_blocks && recs[3].blk_base == imgs[0].total_blocks + 1 && blocks == 2ull * imgs[0].total_blocks + 1 + imgs[3].total_blocks);
    for (int k = 0; k < n; k++) {
        const JsExportRec& r = recs[k]; const JsExportOptRec& o = orecs[k]; const uint8_t* h = hdrs.data() + r.hdr_off;
        const uint32_t nc = imgs[list[k]].ncomp;
        CHECK(o.nslots == (nc == 1 ? 2u : 4u) && o.sos_len == 8 + 2 * nc && o.sos_off + o.sos_len == r.hdr_len && o.sos_off - o.pre_len == (nc == 1 ? 1u : 2u) * 216u);
        CHECK(h[o.pre_len] == 0xFF && h[o.pre_len + 1] == 0xC4 && h[o.sos_off] == 0xFF && h[o.sos_off + 1] == 0xDA);
        CHECK(h[o.pre_len - 3 * nc - 10] == 0xFF && h[o.pre_len - 3 * nc - 9] == 0xC0);                 // what ends at pre_len is the SOF segment
    }
    {   // a header that does not hold the markers where they must be is refused
        JsExportOptRec o; std::vector<uint8_t> h(hdrs.begin(), hdrs.begin() + recs[0].hdr_len);
        CHECK(js_export_opt_split(h.data(), recs[0].hdr_len, 3, &o) == 0);
        h[o.sos_off + 1] = 0xDB; CHECK(js_export_opt_split(h.data(), recs[0].hdr_len, 3, &o) == -1 && g_err.find("split") != std::string::npos);
        CHECK(js_export_opt_split(h.data(), 100, 3, &o) == -1 && js_export_opt_split(h.data(), JS_EXPORT_HDR_MAX + 1, 3, &o) == -1);
    }

    // scratch: the header lengths lie in front of `len`, inside what the first wait copies back
    {
        const JsExportOptScratch s = js_export_opt_scratch(3, 1000, 70000); const JsExportScratch p = js_export_scratch(3, 1000, 70000);
        CHECK(s.s.res == 0 && s.s.ent_bits == p.ent_bits && s.hdr_len >= s.s.ent_bits + 24 && s.s.len >= s.hdr_len + 12 && s.s.back_bytes >= s.s.len + 24 && s.s.ent_ff >= s.s.back_bytes);
        CHECK(s.s.unit_bits >= s.s.ent_ff + 24 && s.s.unit_off >= s.s.unit_bits + 4000 && s.s.blk_bits >= s.s.unit_off + 8000 && s.s.total >= s.s.blk_bits + 140000);
        CHECK(!(s.hdr_len % 16) && !(s.s.len % 16) && !(s.s.unit_off % 16) && !(s.s.blk_bits % 16));
        const JsExportOptKeep k = js_export_opt_keep(3);
        CHECK(k.stats == 0 && k.tabs >= 3 * sizeof(JsExportOptStat) && k.hdrs >= k.tabs + 3 * JS_EXPORT_TABS * 4 && k.total >= k.hdrs + 3 * JS_EXPORT_OPT_HDR && !(k.tabs % 16) && !(k.hdrs % 16));
        CHECK(JS_EXPORT_OPT_HDR >= 438 + 2 * (21 + 16) + 2 * (21 + 256) + 14);
    }

    // second phase: the returned header lengths size the files and move the headers to the device's own place
    {
        std::vector<uint32_t> res(3 * n, 0xFFFFFFFFu), hl((size_t)n, 0), cb((size_t)n + 1, 0xA5A5A5A5u); std::vector<uint64_t> bits((size_t)n, 0);
        std::vector<int> result((size_t)n, -7); std::vector<uint32_t> detail((size_t)n, 77);
        for (int k = 0; k < n; k++) { res[k] = 0; bits[k] = (uint64_t)recs[k].nblk * 2u; hl[k] = orecs[k].pre_len + orecs[k].sos_len + orecs[k].nslots * 22u; }
        res[4] = JSNOOP_EXPORT_INEXACT; res[n + 8] = 17; hl[4] = 0;
        hl[1] = 12345;                                                                            // (unsupported: not looked at)
        uint64_t ub = 0, obytes = 0;
        auto layout = [&]() { std::vector<JsExportRec> r2 = recs; g_err.clear();
            const int rc = js_export_opt_layout(r2.data(), orecs.data(), n, uns.data(), res.data(), bits.data(), hl.data(), cb.data(), result.data(), detail.data(), &ub, &obytes);
            if (!rc) recs = r2;
            return rc; };
        const std::vector<JsExportRec> before = recs;
        CHECK(layout() == 0);
        CHECK(result[0] == 0 && result[1] == 3 && result[2] == 0 && result[3] == 0 && result[4] == 1 && detail[4] == 17 && detail[0] == 0);
        CHECK(recs[0].live && !recs[1].live && recs[2].live && recs[3].live && !recs[4].live);
        CHECK(recs[0].hdr_len == hl[0] && recs[0].hdr_off == 0 && recs[2].hdr_len == hl[2] && recs[2].hdr_off == 2 * JS_EXPORT_OPT_HDR && recs[3].hdr_off == 3 * JS_EXPORT_OPT_HDR);
        CHECK(recs[4].hdr_len == before[4].hdr_len && recs[4].hdr_off == before[4].hdr_off);          // an entry that is not written keeps the host's
        const uint64_t nb0 = (bits[0] + 7) / 8;
        CHECK(recs[0].out_off == 0 && recs[0].out_cap == ((hl[0] + 2 * nb0 + 2 + 15) & ~15ull) && recs[2].out_off == recs[0].out_cap && recs[2].out_cap == ((hl[2] + 2 * 1 + 2 + 15) & ~15ull));
        CHECK(cb[0] == 0 && cb[1] == 1 && cb[2] == 1 && cb[3] == 2 && cb[5] == cb[4] && obytes == recs[3].out_off + recs[3].out_cap && ub == recs[3].u_off + (((bits[3] + 7) / 8 + 15) & ~15ull) + 16);
        recs = before;
        // lengths and bit counts the kernels cannot have produced are refused
        hl[0]--; CHECK(layout() == -1 && g_err.find("header") != std::string::npos); hl[0]++;
        hl[0] = orecs[0].sos_off + orecs[0].sos_len + 1; CHECK(layout() == -1 && g_err.find("header") != std::string::npos);
        hl[0] = orecs[0].sos_off + orecs[0].sos_len; CHECK(layout() == 0); recs = before;
        bits[0]--; CHECK(layout() == -1 && g_err.find("bits") != std::string::npos);
        bits[0] = (uint64_t)recs[0].nblk * 1665u; CHECK(layout() == 0); recs = before;
        bits[0]++; CHECK(layout() == -1);
        bits[0] = 100; res[0] = 4; CHECK(layout() == -1 && g_err.find("result") != std::string::npos);
    }
    printf("ok\n");
    return 0;
}
