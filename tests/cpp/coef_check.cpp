// Host-only program: the argument checks and the grid / record / prefix-table arithmetic of jsnoop_batch_pack_coefs (jpegsnoop_amd/csrc/jsnoop_coef_check.h)
// on hand-made image descriptors.  tests/test_coef_abi.py builds it with the address and undefined-behaviour sanitizers and runs it: every refusal the
// header lists must come back as -1 with a text, every accepted call must fill exactly n records and n + 1 prefix entries, and the grid of every
// component of every sampling layout from 1 to 48 blocks per MCU must address each block of the arena exactly once.  Prints "ok" and returns 0, or the
// line that failed.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#ifndef __HIPCC__              // (a plain host compiler: the descriptors' header marks one helper for both sides)
#define __host__
#define __device__
#endif
#include "../../jpegsnoop_amd/csrc/jsnoop_coef_check.h"

static std::string g_err;
void js_set_error(const char* fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)

// the descriptor js_geometry makes for these sampling factors (ncomp 1: a lone component is 1 x 1) and this many MCUs
static JsImage image(uint32_t ncomp, const uint32_t (*hv)[2], uint32_t mcu_x, uint32_t mcu_y, uint64_t coef_off = 0)
{
    JsImage im; memset(&im, 0, sizeof im);
    im.ncomp = ncomp; im.mcu_xmax = mcu_x; im.mcu_ymax = mcu_y; im.coef_off = coef_off;
    uint32_t hmax = 0, vmax = 0, nb = 0;
    for (uint32_t c = 1; c <= ncomp; c++) {
        im.samp_h[c] = hv[c - 1][0]; im.samp_v[c] = hv[c - 1][1];
        if (im.samp_h[c] > hmax) hmax = im.samp_h[c];
        if (im.samp_v[c] > vmax) vmax = im.samp_v[c];
        for (uint32_t v = 0; v < im.samp_v[c]; v++) for (uint32_t h = 0; h < im.samp_h[c]; h++) { im.blk_comp[nb] = (uint8_t)c; im.blk_ch[nb] = (uint8_t)h; im.blk_cv[nb] = (uint8_t)v; nb++; }
    }
    im.blk_per_mcu = nb; im.mcu_w = hmax * 8; im.mcu_h = vmax * 8; im.blk_xmax = mcu_x * hmax; im.blk_ymax = mcu_y * vmax;
    im.img_x = im.dim_x = mcu_x * im.mcu_w; im.img_y = im.dim_y = mcu_y * im.mcu_h; im.total_blocks = mcu_x * mcu_y * nb;
    return im;
}

int main()
{
    static const uint32_t k420[3][2] = { { 2, 2 }, { 1, 1 }, { 1, 1 } }, kGrey[1][2] = { { 1, 1 } }, k48[3][2] = { { 4, 4 }, { 4, 4 }, { 4, 4 } }, kOdd[3][2] = { { 3, 1 }, { 1, 2 }, { 2, 3 } };
    std::vector<JsImage> imgs = { image(3, k420, 21, 14, 1000), image(1, kGrey, 1, 1, 7), image(3, k48, 3, 2, 50), image(3, kOdd, 5, 4, 0), image(3, k420, 120, 68, 1u << 20) };
    alignas(16) static unsigned char mem[64];
    auto plan = [&](const JsnoopCoefSpec& s, const int* images, int n, const JsnoopCoefDst* dst, std::vector<JsCoefRec>* recs_out = nullptr, std::vector<uint32_t>* base_out = nullptr) {
        std::vector<JsCoefRec> recs((size_t)n); std::vector<uint32_t> base((size_t)n + 1, 0xA5A5A5A5u);      // to the byte: a write past either is the sanitizer's to report
        g_err.clear();
        const int rc = js_coef_plan(imgs.data(), imgs.size(), s, images, n, dst, recs.data(), base.data());
        if (recs_out) *recs_out = recs;
        if (base_out) *base_out = base;
        return rc;
    };
    CHECK(sizeof(JsnoopCoefSpec) == 16 && sizeof(JsnoopCoefDst) == 32 && sizeof(JsCoefRec) == 64);
    JsnoopCoefSpec def; memset(&def, 0xEE, sizeof def); js_coef_spec_defaults(&def);
    CHECK(def.struct_size == sizeof(JsnoopCoefSpec) && def.layout == JSNOOP_COEF_BLOCKS && def.dtype == JSNOOP_COEF_I16 && def.order == JSNOOP_COEF_NATURAL);

    // spec import: shorter accepted with the lacking fields default, longer refused, unknown layout / dtype / order refused
    JsnoopCoefSpec in = def, s;
    in.struct_size = 12; in.layout = JSNOOP_COEF_FREQ; in.dtype = JSNOOP_COEF_F32; in.order = JSNOOP_COEF_ZIGZAG;
    CHECK(js_coef_import_spec(&in, &s) == 0 && s.layout == JSNOOP_COEF_FREQ && s.dtype == JSNOOP_COEF_F32 && s.order == JSNOOP_COEF_NATURAL && s.struct_size == sizeof s);
    in.struct_size = 4; CHECK(js_coef_import_spec(&in, &s) == 0 && s.layout == 0 && s.dtype == 0 && s.order == 0);
    in.struct_size = 16; CHECK(js_coef_import_spec(&in, &s) == 0 && s.order == JSNOOP_COEF_ZIGZAG);
    in.struct_size = sizeof in + 4; CHECK(js_coef_import_spec(&in, &s) == -1 && g_err.find("struct_size") != std::string::npos);
    in.struct_size = 0; CHECK(js_coef_import_spec(&in, &s) == -1);
    in = def; in.layout = 2;  CHECK(js_coef_import_spec(&in, &s) == -1 && g_err.find("layout") != std::string::npos);
    in = def; in.dtype = -1;  CHECK(js_coef_import_spec(&in, &s) == -1 && g_err.find("dtype") != std::string::npos);
    in = def; in.order = 7;   CHECK(js_coef_import_spec(&in, &s) == -1 && g_err.find("order") != std::string::npos);
    CHECK(js_coef_import_spec(nullptr, &s) == -1);

    JsnoopCoefSpec bi = def, bf = def, fi = def, ff = def;
    bf.dtype = JSNOOP_COEF_F32; fi.layout = JSNOOP_COEF_FREQ; ff.layout = JSNOOP_COEF_FREQ; ff.dtype = JSNOOP_COEF_F32;

    // grids and dense sizes of every sampling layout from 1 to 48 blocks per MCU; every arena block addressed exactly once
    {
        unsigned layouts = 0; bool seen[49] = { false };
        for (uint32_t code = 0; code < 4096 * 16; code++) {                       // six factors 1 .. 4: all 4096 three-component layouts (the low bits vary the MCU counts)
            uint32_t hv[3][2]; for (int k = 0; k < 6; k++) hv[k / 2][k % 2] = 1u + ((code >> (4 + 2 * k)) & 3u);
            if (code & 15u) continue;
            const uint32_t mx = 1u + (code >> 4) % 5u, my = 1u + (code >> 7) % 3u;
            const JsImage im = image(3, hv, mx, my);
            std::vector<int> hits(im.total_blocks, 0);
            for (int c = 0; c < 3; c++) {
                uint32_t bw = 0, bh = 0, first = 99;
                CHECK(js_coef_grid(im, c, &bw, &bh, &first) == 0);
                CHECK(bw == mx * hv[c][0] && bh == my * hv[c][1]);
                CHECK(js_coef_dense_bytes(bw, bh, bi) == (uint64_t)bw * bh * 128 && js_coef_dense_bytes(bw, bh, ff) == (uint64_t)bw * bh * 256);
                CHECK(js_coef_dense_row(bw, bi) == bw * 128ull && js_coef_dense_row(bw, bf) == bw * 256ull && js_coef_dense_row(bw, fi) == bw * 2ull && js_coef_dense_row(bw, ff) == bw * 4ull);
                CHECK(js_coef_units(bw, bh) == (uint64_t)bh * ((bw + 63) / 64));
                const uint32_t sh = hv[c][0], sv = hv[c][1];
                for (uint32_t by = 0; by < bh; by++) for (uint32_t bx = 0; bx < bw; bx++) {
                    const uint32_t blk = ((by / sv) * mx + bx / sh) * im.blk_per_mcu + first + (by % sv) * sh + bx % sh;   // the kernel's address
                    CHECK(blk < im.total_blocks && im.blk_comp[blk % im.blk_per_mcu] == c + 1 && im.blk_ch[blk % im.blk_per_mcu] == bx % sh && im.blk_cv[blk % im.blk_per_mcu] == by % sv);
                    hits[blk]++;
                }
            }
            for (int h : hits) CHECK(h == 1);
            seen[im.blk_per_mcu] = true; layouts++;
        }
        CHECK(layouts == 4096 && seen[3] && seen[48] && !seen[2]);
        uint32_t bw = 0, bh = 0, first = 99;
        CHECK(js_coef_grid(imgs[1], 0, &bw, &bh, &first) == 0 && bw == 1 && bh == 1 && first == 0);       // 1 block per MCU
        CHECK(js_coef_grid(imgs[0], 2, &bw, &bh, &first) == 0 && bw == 21 && bh == 14 && first == 5);
        CHECK(js_coef_grid(imgs[0], 0, &bw, &bh, nullptr) == 0 && bw == 42 && bh == 28);
        CHECK(js_coef_grid(imgs[0], 3, &bw, &bh, &first) == -1 && js_coef_grid(imgs[0], -1, &bw, &bh, &first) == -1 && js_coef_grid(imgs[1], 1, &bw, &bh, &first) == -1);
        JsImage bad = imgs[0]; bad.blk_ch[1] = 0; CHECK(js_coef_grid(bad, 0, &bw, &bh, &first) == -1 && g_err.find("block order") != std::string::npos);
    }
    // an accepted call: components in any order, an image listed twice, dense and pitched destinations
    {
        const int which[4] = { 0, 0, 3, 1 };
        JsnoopCoefDst dst[4] = { { mem + 2, 0, 0, 2, 0 }, { mem + 4, 42 * 128 + 6, 0, 0, 0 }, { mem + 6, 0, 0, 2, 0 }, { mem, 0, 0, 0, 0 } };
        std::vector<JsCoefRec> r; std::vector<uint32_t> b;
        CHECK(plan(bi, which, 4, dst, &r, &b) == 0);
        CHECK(b[0] == 0 && b[1] == 14 && b[2] == 14 + 28 && b[3] == 42 + 12 && b[4] == 55);
        CHECK(r[0].bw == 21 && r[0].bh == 14 && r[0].sh == 1 && r[0].sv == 1 && r[0].first == 5 && r[0].bpm == 6 && r[0].mcu_xmax == 21 && r[0].tiles == 1 && r[0].coef_off == 1000 && r[0].row_pitch == 21 * 128);
        CHECK(r[1].bw == 42 && r[1].sh == 2 && r[1].sv == 2 && r[1].first == 0 && r[1].row_pitch == 42 * 128 + 6 && r[1].ptr == (uint64_t)(uintptr_t)(mem + 4));
        CHECK(r[2].bw == 10 && r[2].bh == 12 && r[2].sh == 2 && r[2].sv == 3 && r[2].first == 5 && r[2].bpm == 11);
        CHECK(r[3].bw == 1 && r[3].bh == 1 && r[3].coef_off == 7);
        JsnoopCoefDst d2[2] = { { mem, 0, 0, 0, 0 }, { mem + 16, 8, 8 * 3, 0, 0 } };
        CHECK(plan(ff, nullptr, 2, d2, &r, &b) == 0);                    // images == NULL: 0 .. n - 1
        CHECK(r[0].row_pitch == 42 * 4 && r[0].plane_pitch == 42ull * 4 * 28 && r[1].row_pitch == 8 && r[1].plane_pitch == 24 && b[2] == 29);
        const int big = 4; JsnoopCoefDst d3 = { mem, 0, 0, 0, 0 };
        CHECK(plan(fi, &big, 1, &d3, &r, &b) == 0 && r[0].bw == 240 && r[0].tiles == 4 && b[1] == 136 * 4 && r[0].coef_off == (1u << 20));
    }
    // the refusals
    {
        JsnoopCoefDst d = { mem, 0, 0, 0, 0 }; int i;
        i = 5;  CHECK(plan(bi, &i, 1, &d) == -1 && g_err.find("out of range") != std::string::npos);
        i = -1; CHECK(plan(bi, &i, 1, &d) == -1 && g_err.find("out of range") != std::string::npos);
        i = 0;
        d = { nullptr, 0, 0, 0, 0 };          CHECK(plan(bi, &i, 1, &d) == -1 && g_err.find("NULL") != std::string::npos);
        d = { mem, 0, 0, 0, 1 };              CHECK(plan(bi, &i, 1, &d) == -1 && g_err.find("reserved") != std::string::npos);
        d = { mem, 0, 0, 3, 0 };              CHECK(plan(bi, &i, 1, &d) == -1 && g_err.find("component") != std::string::npos);
        i = 1; d = { mem, 0, 0, 1, 0 };       CHECK(plan(bi, &i, 1, &d) == -1 && g_err.find("component") != std::string::npos);
        i = 0;
        d = { mem, 42 * 128 - 2, 0, 0, 0 };   CHECK(plan(bi, &i, 1, &d) == -1 && g_err.find("row_pitch") != std::string::npos);
        d = { mem, 42 * 128, 0, 0, 0 };       CHECK(plan(bi, &i, 1, &d) == 0);
        d = { mem, 42 * 128, 5, 0, 0 };       CHECK(plan(bi, &i, 1, &d) == 0);                       // BLOCKS ignores plane_pitch
        d = { mem, 42 * 128 + 1, 0, 0, 0 };   CHECK(plan(bi, &i, 1, &d) == -1 && g_err.find("multiples of 2") != std::string::npos);
        d = { mem + 1, 0, 0, 0, 0 };          CHECK(plan(bi, &i, 1, &d) == -1 && g_err.find("multiples of 2") != std::string::npos);
        d = { mem + 2, 0, 0, 0, 0 };          CHECK(plan(bi, &i, 1, &d) == 0);
        d = { mem + 2, 0, 0, 0, 0 };          CHECK(plan(bf, &i, 1, &d) == -1 && g_err.find("multiples of 4") != std::string::npos);
        d = { mem, 42 * 256 + 2, 0, 0, 0 };   CHECK(plan(bf, &i, 1, &d) == -1 && g_err.find("multiples of 4") != std::string::npos);
        d = { mem, 82, 0, 0, 0 };             CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("row_pitch") != std::string::npos);
        d = { mem, 86, 86 * 28 - 2, 0, 0 };   CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("plane_pitch") != std::string::npos);
        d = { mem, 86, 86 * 28, 0, 0 };       CHECK(plan(fi, &i, 1, &d) == 0);
        d = { mem, 86, 86 * 28 + 1, 0, 0 };   CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("multiples of 2") != std::string::npos);
        d = { mem, 168, 168 * 28 + 2, 0, 0 }; CHECK(plan(ff, &i, 1, &d) == -1 && g_err.find("multiples of 4") != std::string::npos);
        d = { mem + 4, 172, 172 * 28 + 4, 0, 0 }; CHECK(plan(ff, &i, 1, &d) == 0);
        const int two[2] = { 0, 9 }; JsnoopCoefDst d2[2] = { { mem, 0, 0, 0, 0 }, { mem, 0, 0, 0, 0 } };   // the second entry bad: still -1
        CHECK(plan(bi, two, 2, d2) == -1);
    }
    // a prefix table whose unit count passes 2^32
    {
        static const uint32_t k444[3][2] = { { 1, 1 }, { 1, 1 }, { 1, 1 } };
        imgs.push_back(image(3, k444, 1, 0x40000000u));                  // 2^30 block rows of one block: 2^30 units a component
        std::vector<int> many(5, 5); std::vector<JsnoopCoefDst> d(5, JsnoopCoefDst{ mem, 0, 0, 1, 0 });
        CHECK(plan(bi, many.data(), 5, d.data()) == -1 && g_err.find("block runs") != std::string::npos);
        std::vector<uint32_t> b;
        CHECK(plan(bi, many.data(), 3, d.data(), nullptr, &b) == 0 && b[3] == 0xC0000000u);
    }
    // the quantisation table back in natural order
    {
        static const uint8_t zz[64] = JS_ZIGZAG_NATURAL;
        uint16_t q[64], out[64]; for (int z = 0; z < 64; z++) q[z] = (uint16_t)(1000 + z);
        js_coef_dqt_natural(q, out);
        for (int z = 0; z < 64; z++) CHECK(out[zz[z]] == 1000 + z);
        CHECK(out[0] == 1000 && out[1] == 1001 && out[8] == 1002 && out[63] == 1063);
    }
    printf("ok\n");
    return 0;
}
