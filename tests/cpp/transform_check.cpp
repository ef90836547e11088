// Host-only program: the host arithmetic of jsnoop_transform_run (jpegsnoop_amd/csrc/jsnoop_transform_check.h) and the block map k_transform runs, which that
// header compiles for both sides -- every refusal of the spec, defaults and a shorter struct, the multiply-high divisions against plain division, the entry
// geometry and the map against a brute-force walk over the component grids (the table of DESIGN.md 4.19 transcribed op by op) for seven layouts x 8 ops x
// crops x grayscale x both edge modes, that the map is a bijection onto the region's blocks and never leaves the source, result words, the plan of a mixed
// call, and 2^31 blocks.  tests/test_transform_abi.py builds it with the address and undefined-behaviour sanitizers and runs it.  Prints "ok" and returns 0,
// or the line that failed.
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
#include "../../jpegsnoop_amd/csrc/jsnoop_transform_check.h"

static std::string g_err;
void js_set_error(const char* fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)
#define REFUSED(call, word) do { g_err.clear(); CHECK((call) == -1); CHECK(g_err.find(word) != std::string::npos); } while (0)

struct HV { uint32_t h, v; };
// the descriptor a decode makes of a w x h picture of ncomp components (js_geometry's rules)
static JsImage image(uint32_t w, uint32_t h, uint32_t ncomp, const HV* hv, uint64_t coef_off)
{
    JsImage im; memset(&im, 0, sizeof im);
    uint32_t hmax = 1, vmax = 1, nb = 0;
    for (uint32_t c = 0; c < ncomp && ncomp > 1; c++) { if (hv[c].h > hmax) hmax = hv[c].h; if (hv[c].v > vmax) vmax = hv[c].v; }
    im.dim_x = w; im.dim_y = h; im.ncomp = ncomp; im.precision = 8; im.mcu_w = 8 * hmax; im.mcu_h = 8 * vmax;
    im.mcu_xmax = (w + im.mcu_w - 1) / im.mcu_w; im.mcu_ymax = (h + im.mcu_h - 1) / im.mcu_h;
    for (uint32_t c = 1; c <= ncomp; c++) {
        const uint32_t H = ncomp > 1 ? hv[c - 1].h : 1, V = ncomp > 1 ? hv[c - 1].v : 1;
        im.samp_h[c] = H; im.samp_v[c] = V;
        for (uint32_t y = 0; y < V; y++) for (uint32_t x = 0; x < H; x++) { im.blk_comp[nb] = (uint8_t)c; im.blk_ch[nb] = (uint8_t)x; im.blk_cv[nb] = (uint8_t)y; nb++; }
    }
    im.blk_per_mcu = nb; im.total_blocks = im.mcu_xmax * im.mcu_ymax * nb; im.coef_off = coef_off;
    return im;
}

// One entry against brute force.  0 = fine, else the line that failed.
static int walk(const JsImage& im, const JsnoopTransformSpec& s, int* result_out)
{
    JsXfRec r; JsImage out; uint32_t reg[4] = { 0, 0, 0, 0 };
    const int res = js_xf_entry(im, s, &r, &out, reg);
    *result_out = res;
    const uint32_t nc = s.grayscale ? 1u : im.ncomp;
    uint32_t wH[3] = { 1, 1, 1 }, wV[3] = { 1, 1, 1 }, hmax = 1, vmax = 1;
    for (uint32_t c = 0; c < nc && nc == 3; c++) { wH[c] = im.samp_h[c + 1]; wV[c] = im.samp_v[c + 1]; if (wH[c] > hmax) hmax = wH[c]; if (wV[c] > vmax) vmax = wV[c]; }
    const uint32_t mw = 8 * hmax, mh = 8 * vmax;
    const bool revx = s.op == JSNOOP_XFORM_FLIP_H || s.op == JSNOOP_XFORM_ROT_180 || s.op == JSNOOP_XFORM_TRANSVERSE || s.op == JSNOOP_XFORM_ROT_270;
    const bool revy = s.op == JSNOOP_XFORM_FLIP_V || s.op == JSNOOP_XFORM_ROT_180 || s.op == JSNOOP_XFORM_TRANSVERSE || s.op == JSNOOP_XFORM_ROT_90;
    const bool T = s.op == JSNOOP_XFORM_TRANSPOSE || s.op == JSNOOP_XFORM_TRANSVERSE || s.op == JSNOOP_XFORM_ROT_90 || s.op == JSNOOP_XFORM_ROT_270;
    // the region, in the contract's words
    uint64_t x0 = 0, y0 = 0, w = im.dim_x, h = im.dim_y;
    int want = JSNOOP_XFORM_OK;
    if (s.crop) {
        if (s.crop_x >= im.dim_x || s.crop_y >= im.dim_y) want = JSNOOP_XFORM_EMPTY;
        else {
            x0 = s.crop_x / mw * mw; y0 = s.crop_y / mh * mh;
            w = (uint64_t)s.crop_x + s.crop_w; if (w > im.dim_x) w = im.dim_x; w -= x0;
            h = (uint64_t)s.crop_y + s.crop_h; if (h > im.dim_y) h = im.dim_y; h -= y0;
        }
    }
    if (want == JSNOOP_XFORM_OK && ((revx && w % mw) || (revy && h % mh))) {
        if (s.edge == JSNOOP_XFORM_EDGE_PERFECT) want = JSNOOP_XFORM_IMPERFECT;
        else { if (revx) w = w / mw * mw; if (revy) h = h / mh * mh; if (!w || !h) want = JSNOOP_XFORM_EMPTY; }
    }
    CHECK(res == want);
    if (res != JSNOOP_XFORM_OK) return 0;
    CHECK(reg[0] == x0 && reg[1] == y0 && reg[2] == w && reg[3] == h);
    const uint32_t rw = (uint32_t)((w + mw - 1) / mw), rh = (uint32_t)((h + mh - 1) / mh);
    // the destination's descriptor
    CHECK(out.dim_x == (T ? h : w) && out.dim_y == (T ? w : h) && out.ncomp == nc && out.precision == im.precision);
    CHECK(out.mcu_w == 8 * (T ? vmax : hmax) && out.mcu_h == 8 * (T ? hmax : vmax));
    CHECK(out.mcu_xmax == (out.dim_x + out.mcu_w - 1) / out.mcu_w && out.mcu_ymax == (out.dim_y + out.mcu_h - 1) / out.mcu_h);      // what a decode of the file would find
    CHECK(out.mcu_xmax == (T ? rh : rw) && out.mcu_ymax == (T ? rw : rh));
    uint32_t nb = 0, dfirst[3] = { 0, 0, 0 }, sfirst[3] = { 0, 0, 0 }, sb = 0;
    for (uint32_t c = 0; c < im.ncomp; c++) { sfirst[c] = sb; sb += im.samp_h[c + 1] * im.samp_v[c + 1]; }
    for (uint32_t c = 0; c < nc; c++) {
        CHECK(out.samp_h[c + 1] == (T ? wV[c] : wH[c]) && out.samp_v[c + 1] == (T ? wH[c] : wV[c]));
        dfirst[c] = nb;
        for (uint32_t y = 0; y < out.samp_v[c + 1]; y++) for (uint32_t x = 0; x < out.samp_h[c + 1]; x++, nb++) CHECK(out.blk_comp[nb] == c + 1 && out.blk_ch[nb] == x && out.blk_cv[nb] == y);
    }
    CHECK(out.blk_per_mcu == nb && out.total_blocks == out.mcu_xmax * out.mcu_ymax * nb && r.nblk == out.total_blocks && r.d_bpm == nb && r.d_mcu_x == out.mcu_xmax);
    // the map: every block of every component's destination grid, by the table of the contract
    const uint32_t flags = (uint32_t)js_xf_flags(s.op);
    std::vector<uint8_t> hit(im.total_blocks, 0); uint64_t expected_hits = 0;
    for (uint32_t c = 0; c < nc; c++) {
        const uint32_t sH = im.samp_h[c + 1], sV = im.samp_v[c + 1];
        const uint32_t BW = rw * wH[c], BH = rh * wV[c], ox = (uint32_t)(x0 / mw) * wH[c], oy = (uint32_t)(y0 / mh) * wV[c];
        const uint32_t DW = T ? BH : BW, DH = T ? BW : BH, dH = out.samp_h[c + 1], dV = out.samp_v[c + 1];
        CHECK(DW == out.mcu_xmax * dH && DH == out.mcu_ymax * dV);
        for (uint32_t by = 0; by < DH; by++) for (uint32_t bx = 0; bx < DW; bx++) {
            uint32_t sy = 0, sx = 0;
            switch (s.op) {
            case JSNOOP_XFORM_NONE:       sy = by;          sx = bx;          break;
            case JSNOOP_XFORM_FLIP_H:     sy = by;          sx = BW - 1 - bx; break;
            case JSNOOP_XFORM_FLIP_V:     sy = BH - 1 - by; sx = bx;          break;
            case JSNOOP_XFORM_ROT_180:    sy = BH - 1 - by; sx = BW - 1 - bx; break;
            case JSNOOP_XFORM_TRANSPOSE:  sy = bx;          sx = by;          break;
            case JSNOOP_XFORM_ROT_90:     sy = BH - 1 - bx; sx = by;          break;
            case JSNOOP_XFORM_ROT_270:    sy = bx;          sx = BW - 1 - by; break;
            case JSNOOP_XFORM_TRANSVERSE: sy = BH - 1 - bx; sx = BW - 1 - by; break;
            }
            CHECK(sx < BW && sy < BH);
            sx += ox; sy += oy;
            CHECK(sx < im.mcu_xmax * sH && sy < im.mcu_ymax * sV);
            const uint64_t src = ((uint64_t)(sy / sV) * im.mcu_xmax + sx / sH) * im.blk_per_mcu + sfirst[c] + (sy % sV) * sH + sx % sH;
            const uint32_t j = ((by / dV) * out.mcu_xmax + bx / dH) * nb + dfirst[c] + (by % dV) * dH + bx % dH;
            const uint64_t got = js_xf_map(r, flags, j);
            if (got != src) printf("layout %ux%u comp %u op %d block (%u, %u): map %llu, walk %llu\n", sH, sV, c, s.op, bx, by, (unsigned long long)got, (unsigned long long)src);
            CHECK(got == src && got < im.total_blocks);
            CHECK(!hit[got]); hit[got] = 1; expected_hits++;
        }
    }
    CHECK(expected_hits == r.nblk);                                   // a bijection: every destination block once, no source block twice
    CHECK(r.src_off == im.coef_off);
    return 0;
}

int main()
{
    // ---- spec: defaults, struct_size, every refusal
    JsnoopTransformSpec d, got;
    memset(&d, 0xEE, sizeof d); js_transform_spec_defaults(&d);
    CHECK(sizeof d == 40 && d.struct_size == 40 && d.op == JSNOOP_XFORM_NONE && d.edge == JSNOOP_XFORM_EDGE_TRIM && !d.grayscale && !d.crop && !d.crop_x && !d.crop_y && !d.crop_w && !d.crop_h && !d.reserved);
    CHECK(js_transform_import_spec(&d, &got) == 0 && !memcmp(&d, &got, sizeof d));
    REFUSED(js_transform_import_spec(nullptr, &got), "spec is NULL");
    { JsnoopTransformSpec s = d; s.struct_size = 3; REFUSED(js_transform_import_spec(&s, &got), "struct_size"); s.struct_size = 44; REFUSED(js_transform_import_spec(&s, &got), "struct_size"); }
    {   // a shorter struct: op and edge alone; what lies behind is not read
        JsnoopTransformSpec s; memset(&s, 0xEE, sizeof s); s.struct_size = 12; s.op = JSNOOP_XFORM_ROT_90; s.edge = JSNOOP_XFORM_EDGE_PERFECT;
        CHECK(js_transform_import_spec(&s, &got) == 0 && got.struct_size == 40 && got.op == JSNOOP_XFORM_ROT_90 && got.edge == JSNOOP_XFORM_EDGE_PERFECT && !got.grayscale && !got.crop && !got.crop_w && !got.reserved);
        s.struct_size = 4; CHECK(js_transform_import_spec(&s, &got) == 0 && got.op == JSNOOP_XFORM_NONE);
    }
    { JsnoopTransformSpec s = d; s.op = 8; REFUSED(js_transform_import_spec(&s, &got), "unknown op"); s.op = -1; REFUSED(js_transform_import_spec(&s, &got), "unknown op"); }
    { JsnoopTransformSpec s = d; s.edge = 2; REFUSED(js_transform_import_spec(&s, &got), "unknown edge"); s.edge = -1; REFUSED(js_transform_import_spec(&s, &got), "unknown edge"); }
    { JsnoopTransformSpec s = d; s.grayscale = 2; REFUSED(js_transform_import_spec(&s, &got), "grayscale"); }
    { JsnoopTransformSpec s = d; s.crop = 2; REFUSED(js_transform_import_spec(&s, &got), "crop is 2"); }
    { JsnoopTransformSpec s = d; s.crop_x = 1; REFUSED(js_transform_import_spec(&s, &got), "while crop is 0"); s = d; s.crop_h = 8; REFUSED(js_transform_import_spec(&s, &got), "while crop is 0"); }
    { JsnoopTransformSpec s = d; s.crop = 1; s.crop_w = 0; s.crop_h = 5; REFUSED(js_transform_import_spec(&s, &got), "crop size"); s.crop_w = 5; s.crop_h = 0; REFUSED(js_transform_import_spec(&s, &got), "crop size"); }
    { JsnoopTransformSpec s = d; s.reserved = 1; REFUSED(js_transform_import_spec(&s, &got), "reserved"); }
    for (int op = 0; op < 8; op++) CHECK(js_xf_flags(op) >= 0);
    CHECK(js_xf_flags(8) < 0 && js_xf_flags(-1) < 0);

    // ---- the multiply-high divisions against plain division: every divisor the map can meet at the dividends around every multiple, and at both ends
    {
        const uint32_t ds[] = { 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 18, 24, 32, 47, 48, 63, 64, 100, 1000, 4095, 4096, 8191, 8192, 65535, 65536, 1000003 };
        for (uint32_t d0 : ds) {
            const JsXfDiv m = js_xf_magic(d0);
            for (uint64_t x = 0; x < 70000; x++) CHECK(js_xf_div((uint32_t)x, m) == x / d0);
            for (uint64_t q = 1; q * d0 < 0x80000000ull; q = q * 3 + 1) for (int e = -2; e <= 2; e++) { const uint64_t x = q * d0 + e; if (x < 0x80000000ull) CHECK(js_xf_div((uint32_t)x, m) == x / d0); }
            for (uint64_t x = 0x7FFFFFFFull - 5000; x <= 0x7FFFFFFFull; x++) CHECK(js_xf_div((uint32_t)x, m) == x / d0);
        }
    }

    // ---- entry geometry and the block map against the brute-force walk
    const HV layouts[7][3] = { { { 1, 1 }, { 1, 1 }, { 1, 1 } }, { { 1, 1 }, { 1, 1 }, { 1, 1 } }, { { 2, 1 }, { 1, 1 }, { 1, 1 } }, { { 1, 2 }, { 1, 1 }, { 1, 1 } },
                               { { 2, 2 }, { 1, 1 }, { 1, 1 } }, { { 4, 1 }, { 1, 1 }, { 1, 1 } }, { { 1, 4 }, { 1, 1 }, { 1, 1 } } };
    const uint32_t sizes[][2] = { { 8, 8 }, { 17, 9 }, { 33, 31 }, { 48, 32 }, { 50, 70 }, { 1, 1 }, { 100, 7 }, { 7, 100 }, { 64, 64 } };
    const uint32_t crops[][4] = { { 0, 0, 16, 16 }, { 16, 16, 16, 8 }, { 5, 3, 20, 11 }, { 9, 17, 1000, 1000 }, { 32, 0, 7, 9 }, { 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu }, { 49, 69, 1, 1 }, { 50, 0, 1, 1 }, { 0, 70, 1, 1 } };
    int counts[4] = { 0, 0, 0, 0 };
    for (int L = 0; L < 7; L++) for (auto& sz : sizes) {
        const JsImage im = image(sz[0], sz[1], L == 0 ? 1 : 3, layouts[L], 12345u + L);
        for (int op = 0; op < 8; op++) for (int edge = 0; edge < 2; edge++) for (uint32_t gray = 0; gray < 2; gray++) for (int k = -1; k < 9; k++) {
            JsnoopTransformSpec s = d; s.op = op; s.edge = edge; s.grayscale = gray;
            if (k >= 0) { s.crop = 1; s.crop_x = crops[k][0]; s.crop_y = crops[k][1]; s.crop_w = crops[k][2]; s.crop_h = crops[k][3]; }
            int res = -1;
            if (walk(im, s, &res)) { printf("  in layout %d, %u x %u, op %d, edge %d, grayscale %u, crop %d\n", L, sz[0], sz[1], op, edge, gray, k); return 1; }
            counts[res]++;
        }
    }
    CHECK(counts[JSNOOP_XFORM_OK] > 5000 && counts[JSNOOP_XFORM_IMPERFECT] > 500 && counts[JSNOOP_XFORM_EMPTY] > 500);

    // ---- result words
    {
        JsXfRec r; JsImage out; JsnoopTransformSpec s = d;
        const JsImage a = image(15, 40, 3, layouts[4], 0);
        s.op = JSNOOP_XFORM_FLIP_H; CHECK(js_xf_entry(a, s, &r, &out, nullptr) == JSNOOP_XFORM_EMPTY);
        s.edge = JSNOOP_XFORM_EDGE_PERFECT; CHECK(js_xf_entry(a, s, &r, &out, nullptr) == JSNOOP_XFORM_IMPERFECT);
        s = d; s.op = JSNOOP_XFORM_ROT_180; CHECK(js_xf_entry(image(17, 9, 3, layouts[4], 0), s, &r, &out, nullptr) == JSNOOP_XFORM_EMPTY);
        JsImage two = image(8, 8, 3, layouts[1], 0); two.ncomp = 2; s = d; CHECK(js_xf_entry(two, s, &r, &out, nullptr) == JSNOOP_XFORM_UNSUPPORTED);
        JsImage odd = image(8, 8, 3, layouts[1], 0); odd.blk_per_mcu = 4; CHECK(js_xf_entry(odd, s, &r, &out, nullptr) == JSNOOP_XFORM_UNSUPPORTED);
        JsImage p12 = image(16, 16, 1, layouts[0], 0); p12.precision = 12; CHECK(js_xf_entry(p12, s, &r, &out, nullptr) == JSNOOP_XFORM_OK && out.precision == 12);
    }

    // ---- the plan of a mixed call: order, images of the object, offsets, units
    {
        std::vector<JsImage> imgs = { image(50, 70, 3, layouts[4], 0), image(15, 40, 3, layouts[4], 1000), image(33, 31, 1, layouts[0], 2000), image(8, 8, 3, layouts[1], 3000) };
        imgs[3].ncomp = 2;
        const int list[6] = { 2, 1, 0, 3, 0, 2 };
        int results[6], image_of[6]; JsXfRec recs[6]; JsImage descs[6]; uint32_t unit_base[7], nout = 0; uint64_t blocks = 0;
        JsnoopTransformSpec s = d; s.op = JSNOOP_XFORM_FLIP_H;
        CHECK(js_transform_plan(imgs.data(), imgs.size(), s, list, 6, results, image_of, recs, descs, unit_base, &nout, &blocks) == 0);
        CHECK(results[0] == 0 && results[1] == JSNOOP_XFORM_EMPTY && results[2] == 0 && results[3] == JSNOOP_XFORM_UNSUPPORTED && results[4] == 0 && results[5] == 0);
        CHECK(nout == 4 && image_of[0] == 0 && image_of[1] == -1 && image_of[2] == 1 && image_of[3] == -1 && image_of[4] == 2 && image_of[5] == 3);
        uint64_t at = 0, units = 0;
        for (uint32_t k = 0; k < nout; k++) { CHECK(recs[k].dst_off == at && descs[k].coef_off == at && unit_base[k] == units); at += recs[k].nblk; units += (recs[k].nblk + JS_XF_RUN - 1) / JS_XF_RUN; }
        CHECK(blocks == at && unit_base[nout] == units && recs[0].nblk == 4 * 4 && recs[1].nblk == 3 * 5 * 6 && recs[1].src_off == 0 && recs[0].src_off == 2000);
        CHECK(js_transform_plan(imgs.data(), imgs.size(), s, nullptr, 3, results, image_of, recs, descs, unit_base, &nout, &blocks) == 0 && nout == 2);
        CHECK(js_transform_plan(imgs.data(), imgs.size(), s, nullptr, 0, results, image_of, recs, descs, unit_base, &nout, &blocks) == 0 && nout == 0 && blocks == 0);
        REFUSED(js_transform_plan(imgs.data(), imgs.size(), s, list, -1, results, image_of, recs, descs, unit_base, &nout, &blocks), "n = -1");
        REFUSED(js_transform_plan(imgs.data(), imgs.size(), s, nullptr, 5, results, image_of, recs, descs, unit_base, &nout, &blocks), "without a list");
        const int bad1[2] = { 0, 4 }, bad2[2] = { -1, 0 };
        REFUSED(js_transform_plan(imgs.data(), imgs.size(), s, bad1, 2, results, image_of, recs, descs, unit_base, &nout, &blocks), "out of range");
        REFUSED(js_transform_plan(imgs.data(), imgs.size(), s, bad2, 2, results, image_of, recs, descs, unit_base, &nout, &blocks), "out of range");
    }
    // ---- 2^31 blocks: 32 grey pictures of 65535 x 65535 are 32 x 8192 x 8192 blocks; 31 of them pass
    {
        const JsImage big = image(65535, 65535, 1, layouts[0], 0);
        std::vector<int> list(32, 0), results(32), image_of(32); std::vector<JsXfRec> recs(32); std::vector<JsImage> descs(32); std::vector<uint32_t> unit_base(33); uint32_t nout = 0; uint64_t blocks = 0;
        CHECK(js_transform_plan(&big, 1, d, list.data(), 31, results.data(), image_of.data(), recs.data(), descs.data(), unit_base.data(), &nout, &blocks) == 0 && blocks == 31ull << 26 && unit_base[31] == 31u << 23);
        REFUSED(js_transform_plan(&big, 1, d, list.data(), 32, results.data(), image_of.data(), recs.data(), descs.data(), unit_base.data(), &nout, &blocks), "2^31 blocks");
    }
    // ---- a table into the set's zig-zag order, transposed or not
    {
        static const uint8_t zz[64] = JS_ZIGZAG_NATURAL;
        uint16_t nat[64], q[64];
        for (int n = 0; n < 64; n++) nat[n] = (uint16_t)(1000 + n);
        js_xf_table(nat, false, q); for (int z = 0; z < 64; z++) CHECK(q[z] == 1000 + zz[z]);
        js_xf_table(nat, true, q);  for (int z = 0; z < 64; z++) CHECK(q[z] == 1000 + (zz[z] & 7) * 8 + (zz[z] >> 3));
    }
    printf("ok\n");
    return 0;
}
