// Host-only program: the host arithmetic of jsnoop_batch_export_jpeg (jpegsnoop_amd/csrc/jsnoop_export_check.h) on hand-made image descriptors --
// spec import, the Annex K code tables, the header bytes for Pq 0 / 1 and one / three components, every refusal of the plan, the records (component and
// predecessor of every block of an MCU), the prefix tables and the second phase's sizes, past 2^32 bits.  tests/test_export_abi.py builds it with the
// address and undefined-behaviour sanitizers and runs it.  Prints "ok" and returns 0, or the line that failed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#ifndef __HIPCC__              // (a plain host compiler: the descriptors' header marks one helper for both sides)
#define __host__
#define __device__
#endif
#include "../../jpegsnoop_amd/csrc/jsnoop_export_check.h"

static std::string g_err;
void js_set_error(const char* fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)

// the descriptor js_geometry makes for these sampling factors (ncomp 1: a lone component is 1 x 1) and these SOF dimensions
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

static uint16_t g_q[3] = { 3, 5, 7 };                  // multiplier of every index, by component
static int g_q_fail = -1;
static int qfn(void*, int i, int comp, uint16_t* out64)
{
    if (i == g_q_fail) { js_set_error("image_dqt: image %d has no table set", i); return -1; }
    for (int k = 0; k < 64; k++) out64[k] = (uint16_t)(g_q[comp] + (comp == 1 ? k : 0));
    return 0;
}
static uint32_t be16(const uint8_t* p) { return (uint32_t)p[0] << 8 | p[1]; }

int main(int argc, char** argv)
{
    static const uint32_t k420[3][2] = { { 2, 2 }, { 1, 1 }, { 1, 1 } }, kGrey[1][2] = { { 1, 1 } }, k411[3][2] = { { 4, 1 }, { 1, 1 }, { 1, 1 } }, kOdd[3][2] = { { 1, 2 }, { 2, 1 }, { 1, 1 } };
    std::vector<JsImage> imgs = { image(3, k420, 333, 217, 64), image(1, kGrey, 1, 1, 1 << 20), image(3, k411, 1025, 9, 128), image(3, kOdd, 100, 50, 8), image(3, k420, 65535, 65535, 1u << 24) };
    CHECK(imgs[1].blk_per_mcu == 1 && imgs[1].total_blocks == 1);
    if (argc > 1) {                                    // "header <image> <jfif>": the header's bytes in hex, for the comparison with tests/export_model.py
        const int i = argc > 2 ? atoi(argv[2]) : 0; uint16_t q[3][64]; uint8_t h[JS_EXPORT_HDR_MAX];
        if (i < 0 || i > 3) return 2;
        for (int c = 0; c < 3; c++) qfn(nullptr, i, c, q[c]);
        if (argc > 4) q[1][63] = (uint16_t)atoi(argv[4]);
        const uint32_t n = js_export_header(imgs[(size_t)i], q, argc > 3 ? atoi(argv[3]) : 1, h);
        for (uint32_t k = 0; k < n; k++) printf("%02x", h[k]);
        printf("\n");
        return 0;
    }
    CHECK(sizeof(JsnoopExportSpec) == 8 && sizeof(JsExportRec) == 552 && sizeof(JsExportRec) % 8 == 0);

    // spec: defaults, shorter accepted, longer and NULL refused
    JsnoopExportSpec def; memset(&def, 0xEE, sizeof def); js_export_spec_defaults(&def);
    CHECK(def.struct_size == 8 && def.jfif == 1);
    JsnoopExportSpec in = def, s;
    in.jfif = 0; CHECK(js_export_import_spec(&in, &s) == 0 && s.jfif == 0);
    in.struct_size = 4; CHECK(js_export_import_spec(&in, &s) == 0 && s.jfif == 1 && s.struct_size == 8);
    in.struct_size = 12; CHECK(js_export_import_spec(&in, &s) == -1 && g_err.find("struct_size") != std::string::npos);
    in.struct_size = 0; CHECK(js_export_import_spec(&in, &s) == -1);
    CHECK(js_export_import_spec(nullptr, &s) == -1 && g_err.find("spec is NULL") != std::string::npos);

    // code tables: Annex K's known corners, a prefix code of 12 + 162 symbols per table
    std::vector<uint32_t> tabs(JS_EXPORT_TABS, 0xA5A5A5A5u);
    js_export_code_tabs(tabs.data());
    CHECK(tabs[0] == (2u << 16 | 0u) && tabs[11] == (9u << 16 | 0x1FEu) && tabs[12] == 0 && tabs[16 + 0] == (2u << 16 | 0u) && tabs[16 + 11] == (11u << 16 | 0x7FEu));
    CHECK(tabs[32 + 0x00] == (4u << 16 | 0xAu) && tabs[32 + 0xF0] == (11u << 16 | 0x7F9u) && tabs[32 + 0x0A] == (16u << 16 | 0xFF83u) && tabs[32 + 0xFA] == (16u << 16 | 0xFFFEu));
    CHECK(tabs[288 + 0x00] == (2u << 16 | 0u) && tabs[288 + 0xF0] == (10u << 16 | 0x3FAu) && tabs[288 + 0xFA] == (16u << 16 | 0xFFFEu) && tabs[32 + 0x0B] == 0);
    for (int t = 0; t < 2; t++) { int n = 0; for (int k = 0; k < 256; k++) n += tabs[32 + t * 256 + k] != 0; CHECK(n == 162); }

    // the plan: records, unit prefix, headers
    auto plan = [&](const JsnoopExportSpec& sp, const int* images, int n, std::vector<JsExportRec>* recs_out = nullptr, std::vector<uint32_t>* base_out = nullptr,
                    std::vector<uint8_t>* hdr_out = nullptr, std::vector<uint8_t>* uns_out = nullptr, uint64_t* blocks_out = nullptr) {
        std::vector<JsExportRec> recs((size_t)n); std::vector<uint32_t> base((size_t)n + 1, 0xA5A5A5A5u); std::vector<uint8_t> hdrs((size_t)n * JS_EXPORT_HDR_MAX, 0xA5), uns((size_t)n, 0xA5);
        uint64_t blocks = 0;
        g_err.clear();
        const int rc = js_export_plan(imgs.data(), imgs.size(), sp, images, n, qfn, nullptr, recs.data(), base.data(), hdrs.data(), uns.data(), &blocks);
        if (recs_out) *recs_out = recs;
        if (base_out) *base_out = base;
        if (hdr_out) *hdr_out = hdrs;
        if (uns_out) *uns_out = uns;
        if (blocks_out) *blocks_out = blocks;
        return rc;
    };
    std::vector<JsExportRec> recs; std::vector<uint32_t> base; std::vector<uint8_t> hdrs, uns; uint64_t blocks = 0;
    const int list[] = { 3, 0, 1, 0, 2 };
    CHECK(plan(def, list, 5, &recs, &base, &hdrs, &uns, &blocks) == 0);
    uint64_t want_blocks = 0, want_units = 0;
    for (int k = 0; k < 5; k++) {
        const JsImage& im = imgs[list[k]]; const JsExportRec& r = recs[k];
        CHECK(r.coef_off == im.coef_off && r.nblk == im.total_blocks && r.bpm == im.blk_per_mcu && r.blk_base == want_blocks && base[k] == want_units && !uns[k]);
        want_blocks += im.total_blocks; want_units += (im.total_blocks + JS_EXPORT_TILE - 1) / JS_EXPORT_TILE;
        // the predecessor of every block of two MCUs, found the slow way
        for (uint32_t j = im.blk_per_mcu; j < 2 * im.blk_per_mcu; j++) {
            const uint32_t pos = j % im.blk_per_mcu; uint32_t p = j;
            do p--; while (im.blk_comp[p % im.blk_per_mcu] != im.blk_comp[pos]);
            CHECK(r.comp[pos] == im.blk_comp[pos] - 1u && r.back[pos] == j - p);
        }
        for (uint32_t c = 0; c < im.ncomp; c++) CHECK(r.q[c][0] == g_q[c] && r.q[c][63] == g_q[c] + (c == 1 ? 63 : 0));
        CHECK(r.hdr_off == (uint32_t)k * JS_EXPORT_HDR_MAX && r.hdr_len <= JS_EXPORT_HDR_MAX && hdrs[r.hdr_off + r.hdr_len] == 0xA5);
    }
    CHECK(base[5] == want_units && blocks == want_blocks);
    {   // 4:2:0: Y Y Y Y Cb Cr
        const JsExportRec& r = recs[1];
        const uint8_t comp[6] = { 0, 0, 0, 0, 1, 2 }, back[6] = { 3, 1, 1, 1, 6, 6 };
        CHECK(!memcmp(r.comp, comp, 6) && !memcmp(r.back, back, 6));
    }
    {   // header of the three-component 4:2:0 image, 8-bit tables: walk the segments
        const JsExportRec& r = recs[1]; const uint8_t* h = hdrs.data() + r.hdr_off;
        CHECK(r.hdr_len == 2 + 18 + 3 * 69 + 19 + 2 * 33 + 2 * 183 + 14);
        CHECK(h[0] == 0xFF && h[1] == 0xD8 && h[2] == 0xFF && h[3] == 0xE0 && be16(h + 4) == 16 && !memcmp(h + 6, "JFIF\0\1\1\0\0\1\0\1\0\0", 14));
        const uint8_t* p = h + 20;
        for (uint32_t c = 0; c < 3; c++) { CHECK(p[0] == 0xFF && p[1] == 0xDB && be16(p + 2) == 67 && p[4] == c && p[5] == g_q[c] && p[5 + 2] == g_q[c] + (c == 1 ? 8 : 0)); p += 69; }   // zig-zag position 2 = natural 8
        CHECK(p[0] == 0xFF && p[1] == 0xC0 && be16(p + 2) == 17 && p[4] == 8 && be16(p + 5) == 217 && be16(p + 7) == 333 && p[9] == 3);
        CHECK(p[10] == 1 && p[11] == 0x22 && p[12] == 0 && p[13] == 2 && p[14] == 0x11 && p[15] == 1 && p[16] == 3 && p[17] == 0x11 && p[18] == 2);
        p += 19;
        const uint8_t th[4] = { 0x00, 0x10, 0x01, 0x11 }; const uint32_t ln[4] = { 31, 181, 31, 181 };
        for (int t = 0; t < 4; t++) { CHECK(p[0] == 0xFF && p[1] == 0xC4 && be16(p + 2) == ln[t] && p[4] == th[t]); uint32_t n = 0; for (int i = 0; i < 16; i++) n += p[5 + i]; CHECK(n + 19 == ln[t]); p += 2 + ln[t]; }
        CHECK(p[0] == 0xFF && p[1] == 0xDA && be16(p + 2) == 12 && p[4] == 3 && p[5] == 1 && p[6] == 0x00 && p[7] == 2 && p[8] == 0x11 && p[9] == 3 && p[10] == 0x11 && p[11] == 0 && p[12] == 63 && p[13] == 0);
        CHECK(p + 14 == h + r.hdr_len);
    }
    {   // one component, no APP0: two tables, 1 x 1 whatever the SOF said
        JsnoopExportSpec nj = def; nj.jfif = 0;
        const int one[] = { 1 };
        CHECK(plan(nj, one, 1, &recs, &base, &hdrs) == 0);
        const uint8_t* h = hdrs.data();
        CHECK(recs[0].hdr_len == 2 + 69 + 13 + 33 + 183 + 10 && h[2] == 0xFF && h[3] == 0xDB);
        const uint8_t* p = h + 2 + 69;
        CHECK(p[1] == 0xC0 && be16(p + 2) == 11 && p[9] == 1 && p[10] == 1 && p[11] == 0x11 && p[12] == 0);
        p += 13 + 33 + 183;
        CHECK(p[1] == 0xDA && be16(p + 2) == 8 && p[4] == 1 && p[5] == 1 && p[6] == 0 && p[7] == 0 && p[8] == 63 && p[9] == 0);
        CHECK(recs[0].comp[0] == 0 && recs[0].back[0] == 1 && base[1] == 1);
    }
    {   // a 16-bit multiplier in component 1: its DQT has Pq 1 and 128 bytes, the frame is SOF1, the others stay 8-bit
        g_q[1] = 300;
        const int one[] = { 0 };
        CHECK(plan(def, one, 1, &recs, &base, &hdrs) == 0);
        const uint8_t* p = hdrs.data() + 20;
        CHECK(be16(p + 2) == 67 && p[4] == 0x00); p += 69;
        CHECK(be16(p + 2) == 131 && p[4] == 0x11 && be16(p + 5) == 300 && be16(p + 5 + 4) == 308); p += 133;
        CHECK(be16(p + 2) == 67 && p[4] == 0x02); p += 69;
        CHECK(p[0] == 0xFF && p[1] == 0xC1);
        CHECK(recs[0].hdr_len == 2 + 18 + 69 + 133 + 69 + 19 + 2 * 33 + 2 * 183 + 14 && recs[0].hdr_len <= JS_EXPORT_HDR_MAX);
        g_q[0] = g_q[2] = 65535; g_q[1] = 65000;                   // the longest header there is
        CHECK(plan(def, one, 1, &recs) == 0 && recs[0].hdr_len == 884);
        g_q[0] = 3; g_q[1] = 5; g_q[2] = 7;
    }

    // refusals: nothing usable is promised, the text names the reason
    const int bad_hi[] = { 0, 5 }, bad_lo[] = { -1 };
    CHECK(plan(def, bad_hi, 2) == -1 && g_err.find("out of range") != std::string::npos);
    CHECK(plan(def, bad_lo, 1) == -1 && g_err.find("out of range") != std::string::npos);
    CHECK(plan(def, nullptr, 6) == -1 && g_err.find("out of range") != std::string::npos);          // images == NULL: 0 .. n - 1
    CHECK(plan(def, nullptr, 5) == 0);
    { JsImage keep = imgs[2]; imgs[2].total_blocks++; CHECK(plan(def, nullptr, 3) == -1 && g_err.find("geometry") != std::string::npos); imgs[2] = keep; }
    { JsImage keep = imgs[2]; imgs[2].blk_per_mcu = 0; CHECK(plan(def, nullptr, 3) == -1 && g_err.find("geometry") != std::string::npos); imgs[2] = keep; }
    { JsImage keep = imgs[2]; imgs[2].ncomp = 2; CHECK(plan(def, nullptr, 3) == -1 && g_err.find("components") != std::string::npos); imgs[2] = keep; }
    { JsImage keep = imgs[0]; imgs[0].blk_comp[1] = 2; imgs[0].blk_comp[4] = 1; CHECK(plan(def, nullptr, 1) == -1 && g_err.find("block order") != std::string::npos); imgs[0] = keep; }
    { JsImage keep = imgs[0]; imgs[0].blk_comp[5] = 4; CHECK(plan(def, nullptr, 1) == -1 && g_err.find("block order") != std::string::npos); imgs[0] = keep; }
    g_q_fail = 1; CHECK(plan(def, nullptr, 2) == -1 && g_err.find("table set") != std::string::npos); g_q_fail = -1;
    {   // precision 12: the host's word, no unit, no block
        imgs[1].precision = 12;
        CHECK(plan(def, list, 5, &recs, &base, &hdrs, &uns, &blocks) == 0);
        CHECK(uns[2] == 1 && base[3] == base[2] && !uns[0] && !uns[1] && !uns[3] && blocks == want_blocks - 1 && recs[3].blk_base == recs[2].blk_base);
        imgs[1].precision = 8;
    }
    {   // more tiles than a grid holds
        const std::vector<int> big(6000, 4);                                                     // 393 216 tiles each
        CHECK(imgs[4].total_blocks == 4096u * 4096u * 6u);
        CHECK(plan(def, big.data(), 5000) == 0 && plan(def, big.data(), 6000) == -1 && g_err.find("2^31") != std::string::npos);
    }

    // second phase: sizes from result words and bit lengths
    CHECK(plan(def, list, 5, &recs, &base, &hdrs, &uns) == 0);
    {
        const int n = 5;
        std::vector<uint32_t> res(3 * n, 0xFFFFFFFFu); std::vector<uint64_t> bits(n, 0); std::vector<uint32_t> cb((size_t)n + 1, 0xA5A5A5A5u);
        std::vector<int> result(n, -7); std::vector<uint32_t> detail(n, 77);
        for (int k = 0; k < n; k++) { res[k] = 0; bits[k] = (uint64_t)recs[k].nblk * 6u; }
        res[1] = JSNOOP_EXPORT_INEXACT; res[n + 2] = 17; res[n + 3] = 99;                       // entry 1: inexact at 17 (the uncodable slot is not its word)
        res[3] = JSNOOP_EXPORT_UNCODABLE; res[n + 6] = 5; res[n + 7] = 9;                       // entry 3: uncodable at 9, though a block in front of it is inexact
        uns[2] = 1;
        bits[4] = 8u * JS_EXPORT_CHUNK + 1u;                                                    // one bit into the second chunk
        uint64_t ub = 0, ob = 0;
        g_err.clear();
        CHECK(js_export_layout(recs.data(), n, uns.data(), res.data(), bits.data(), cb.data(), result.data(), detail.data(), &ub, &ob) == 0);
        CHECK(result[0] == 0 && result[1] == 1 && result[2] == 3 && result[3] == 2 && result[4] == 0 && detail[0] == 0 && detail[1] == 17 && detail[2] == 0 && detail[3] == 9 && detail[4] == 0);
        CHECK(recs[0].live && !recs[1].live && !recs[2].live && !recs[3].live && recs[4].live && recs[1].bits == 0 && recs[1].out_cap == 0);
        const uint64_t nb0 = (bits[0] + 7) / 8, nb4 = JS_EXPORT_CHUNK + 1u;
        CHECK(cb[0] == 0 && cb[1] == (nb0 + JS_EXPORT_CHUNK - 1) / JS_EXPORT_CHUNK && cb[2] == cb[1] && cb[3] == cb[1] && cb[4] == cb[1] && cb[5] == cb[1] + 2);
        CHECK(recs[0].u_off == 0 && recs[4].u_off == ((nb0 + 15) & ~15ull) + 16 && ub == recs[4].u_off + ((nb4 + 15) & ~15ull) + 16 && recs[4].u_off % 16 == 0);
        CHECK(recs[0].out_off == 0 && recs[0].out_cap >= recs[0].hdr_len + 2 * nb0 + 2 && recs[0].out_cap % 16 == 0 && recs[4].out_off == recs[0].out_cap && ob == recs[4].out_off + recs[4].out_cap);
        // bit lengths the kernels cannot have produced are refused
        bits[0] = 5; CHECK(js_export_layout(recs.data(), n, uns.data(), res.data(), bits.data(), cb.data(), result.data(), detail.data(), &ub, &ob) == -1);
        bits[0] = (uint64_t)recs[0].nblk * 1658u + 1u; CHECK(js_export_layout(recs.data(), n, uns.data(), res.data(), bits.data(), cb.data(), result.data(), detail.data(), &ub, &ob) == -1);
        bits[0] = 6; res[0] = 4; CHECK(js_export_layout(recs.data(), n, uns.data(), res.data(), bits.data(), cb.data(), result.data(), detail.data(), &ub, &ob) == -1 && g_err.find("result") != std::string::npos);
    }
    {   // past 2^32 bits in one entry, past 2^32 bytes in one call: 64-bit throughout
        const int big[] = { 4, 4 };
        CHECK(plan(def, big, 2, &recs, &base, &hdrs, &uns) == 0);
        std::vector<uint32_t> res(6, 0xFFFFFFFFu); res[0] = res[1] = 0;
        std::vector<uint64_t> bits = { (uint64_t)recs[0].nblk * 400u, (1ull << 32) + 8u }; std::vector<uint32_t> cb(3); std::vector<int> result(2); std::vector<uint32_t> detail(2);
        uint64_t ub = 0, ob = 0;
        CHECK(bits[0] > (1ull << 35));
        CHECK(js_export_layout(recs.data(), 2, uns.data(), res.data(), bits.data(), cb.data(), result.data(), detail.data(), &ub, &ob) == 0);
        const uint64_t nb0 = bits[0] / 8, nb1 = (1ull << 29) + 1;
        CHECK(recs[0].bits == bits[0] && cb[1] == nb0 / JS_EXPORT_CHUNK && cb[2] == cb[1] + (1u << 17) + 1u);
        CHECK(recs[1].u_off == nb0 + 16 && recs[1].out_off >= 2 * nb0 && ub > (1ull << 32) && ob == recs[1].out_off + recs[1].out_cap && recs[1].out_cap >= 2 * nb1 + 2);
        bits[0] = (uint64_t)recs[0].nblk * 1658u; bits[1] = bits[0];                            // 2 x 20 GB of stream: more chunks than a grid holds
        CHECK(js_export_layout(recs.data(), 2, uns.data(), res.data(), bits.data(), cb.data(), result.data(), detail.data(), &ub, &ob) == 0 && cb[2] == 2u * (uint32_t)((bits[0] / 8 + 4095) / 4096));
    }
    // the blocks of the batch's page-locked memory and of the device scratch do not overlap and keep 16-byte starts
    {
        const JsExportBlock b = js_export_block(3); const JsExportScratch sc = js_export_scratch(3, 1000, 70000);
        CHECK(b.recs == 0 && b.unit_base >= 3 * sizeof(JsExportRec) && b.chunk_base >= b.unit_base + 16 && b.tabs >= b.chunk_base + 16 && b.hdrs >= b.tabs + JS_EXPORT_TABS * 4 && b.total >= b.hdrs + 3 * JS_EXPORT_HDR_MAX);
        CHECK(!(b.unit_base % 16) && !(b.chunk_base % 16) && !(b.tabs % 16) && !(b.hdrs % 16) && !(b.total % 16));
        CHECK(sc.res == 0 && sc.ent_bits >= 36 && sc.len >= sc.ent_bits + 24 && sc.ent_ff >= sc.len + 24 && sc.unit_bits >= sc.ent_ff + 24 && sc.unit_off >= sc.unit_bits + 4000 && sc.blk_bits >= sc.unit_off + 8000 && sc.total >= sc.blk_bits + 140000);
        CHECK(!(sc.ent_bits % 16) && !(sc.len % 16) && !(sc.unit_off % 16) && !(sc.blk_bits % 16));
    }
    printf("ok\n");
    return 0;
}
