// Host-only program: the argument checks and the size / record / prefix-table arithmetic of jsnoop_batch_pack_planes (jpegsnoop_amd/csrc/jsnoop_plane_check.h)
// on hand-made image descriptors.  tests/test_plane_abi.py builds it with the address and undefined-behaviour sanitizers and runs it: every refusal the
// header lists must come back as -1 with a text, every accepted call must fill exactly n records and n + 1 prefix entries, and every element a record
// addresses must lie inside its plane and in front of dim_x x dim_y.  Prints "ok" and returns 0, or the line that failed.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#ifndef __HIPCC__              // (a plain host compiler: the descriptors' header marks one helper for both sides)
#define __host__
#define __device__
#endif
#include "../../jpegsnoop_amd/csrc/jsnoop_plane_check.h"

static std::string g_err;
void js_set_error(const char* fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)

// the descriptor js_geometry makes for these sampling factors (ncomp 1: a lone component is 1 x 1) and these SOF dimensions
static JsImage image(uint32_t ncomp, const uint32_t (*hv)[2], uint32_t dim_x, uint32_t dim_y, uint64_t plane_off = 0)
{
    JsImage im; memset(&im, 0, sizeof im);
    im.ncomp = ncomp; im.dim_x = dim_x; im.dim_y = dim_y; im.plane_off = plane_off; im.want_planes = 1;
    uint32_t hmax = 0, vmax = 0;
    for (uint32_t c = 1; c <= ncomp; c++) {
        im.samp_h[c] = hv[c - 1][0]; im.samp_v[c] = hv[c - 1][1];
        if (im.samp_h[c] > hmax) hmax = im.samp_h[c];
        if (im.samp_v[c] > vmax) vmax = im.samp_v[c];
    }
    for (uint32_t c = 1; c <= ncomp; c++) { im.expand_h[c] = hmax / im.samp_h[c]; im.expand_v[c] = vmax / im.samp_v[c]; }
    im.mcu_w = hmax * 8; im.mcu_h = vmax * 8;
    im.mcu_xmax = (dim_x + im.mcu_w - 1) / im.mcu_w; im.mcu_ymax = (dim_y + im.mcu_h - 1) / im.mcu_h;
    im.blk_xmax = im.mcu_xmax * hmax; im.blk_ymax = im.mcu_ymax * vmax; im.img_x = im.mcu_xmax * im.mcu_w; im.img_y = im.mcu_ymax * im.mcu_h;
    return im;
}

int main()
{
    static const uint32_t k420[3][2] = { { 2, 2 }, { 1, 1 }, { 1, 1 } }, kGrey[1][2] = { { 1, 1 } }, k411[3][2] = { { 4, 1 }, { 1, 1 }, { 1, 1 } }, k440[3][2] = { { 1, 2 }, { 1, 1 }, { 1, 1 } },
                          kOdd[3][2] = { { 3, 1 }, { 1, 2 }, { 2, 3 } };
    std::vector<JsImage> imgs = { image(3, k420, 333, 217, 64), image(1, kGrey, 1, 1, 1 << 20), image(3, k411, 1025, 9, 128), image(3, k440, 513, 17, 0), image(3, kOdd, 100, 50, 8),
                                  image(3, k420, 1920, 1080, 1u << 24) };
    alignas(16) static unsigned char mem[64];
    auto plan = [&](const JsnoopPlaneSpec& s, const int* images, int n, const JsnoopPlaneDst* dst, std::vector<JsPlaneRec>* recs_out = nullptr, std::vector<uint32_t>* base_out = nullptr) {
        std::vector<JsPlaneRec> recs((size_t)n); std::vector<uint32_t> base((size_t)n + 1, 0xA5A5A5A5u);      // to the byte: a write past either is the sanitizer's to report
        g_err.clear();
        const int rc = js_plane_plan(imgs.data(), imgs.size(), s, images, n, dst, recs.data(), base.data());
        if (recs_out) *recs_out = recs;
        if (base_out) *base_out = base;
        return rc;
    };
    CHECK(sizeof(JsnoopPlaneSpec) == 36 && sizeof(JsnoopPlaneDst) == 24 && sizeof(JsPlaneRec) == 56 && sizeof(JsPlaneArgs) == 24);
    JsnoopPlaneSpec def; memset(&def, 0xEE, sizeof def); js_plane_spec_defaults(&def);
    CHECK(def.struct_size == sizeof(JsnoopPlaneSpec) && def.res == JSNOOP_PLANE_FULL && def.dtype == JSNOOP_PLANE_I16);
    for (int c = 0; c < 3; c++) CHECK(def.scale[c] == 1.0f && def.bias[c] == 0.0f);

    // spec import: shorter accepted with the lacking fields default, longer refused, unknown res / dtype refused
    JsnoopPlaneSpec in = def, s;
    in.res = JSNOOP_PLANE_NATIVE; in.dtype = JSNOOP_PLANE_F32; in.scale[0] = 9.0f; in.bias[2] = 5.0f;
    in.struct_size = 8;  CHECK(js_plane_import_spec(&in, &s) == 0 && s.res == JSNOOP_PLANE_NATIVE && s.dtype == JSNOOP_PLANE_I16 && s.scale[0] == 1.0f && s.struct_size == sizeof s);
    in.struct_size = 4;  CHECK(js_plane_import_spec(&in, &s) == 0 && s.res == JSNOOP_PLANE_FULL && s.dtype == JSNOOP_PLANE_I16);
    in.struct_size = 24; CHECK(js_plane_import_spec(&in, &s) == 0 && s.dtype == JSNOOP_PLANE_F32 && s.scale[0] == 9.0f && s.scale[2] == 1.0f && s.bias[2] == 0.0f);
    in.struct_size = 36; CHECK(js_plane_import_spec(&in, &s) == 0 && s.bias[2] == 5.0f);
    in.struct_size = sizeof in + 4; CHECK(js_plane_import_spec(&in, &s) == -1 && g_err.find("struct_size") != std::string::npos);
    in.struct_size = 0;  CHECK(js_plane_import_spec(&in, &s) == -1);
    in = def; in.res = 2;    CHECK(js_plane_import_spec(&in, &s) == -1 && g_err.find("res") != std::string::npos);
    in = def; in.res = -1;   CHECK(js_plane_import_spec(&in, &s) == -1);
    in = def; in.dtype = 3;  CHECK(js_plane_import_spec(&in, &s) == -1 && g_err.find("dtype") != std::string::npos);
    in = def; in.dtype = -1; CHECK(js_plane_import_spec(&in, &s) == -1);
    CHECK(js_plane_import_spec(nullptr, &s) == -1);

    JsnoopPlaneSpec fi = def, fu = def, ff = def, ni = def, nu = def, nf = def;
    fu.dtype = JSNOOP_PLANE_U8; ff.dtype = JSNOOP_PLANE_F32; ni.res = nu.res = nf.res = JSNOOP_PLANE_NATIVE; nu.dtype = JSNOOP_PLANE_U8; nf.dtype = JSNOOP_PLANE_F32;
    CHECK(js_plane_elem(fi) == 2 && js_plane_elem(fu) == 1 && js_plane_elem(ff) == 4);

    // sizes: every layout of factors 1 .. 4, dimensions 1, eh, eh + 1 (and the same for rows): FULL is the SOF size, NATIVE ceil(dim / factor); the last
    // element a record addresses is in front of dim_x x dim_y, hence inside the plane
    {
        unsigned layouts = 0;
        for (uint32_t code = 0; code < 4096; code++) {
            uint32_t hv[3][2]; for (int k = 0; k < 6; k++) hv[k / 2][k % 2] = 1u + ((code >> (2 * k)) & 3u);
            uint32_t hmax = 0, vmax = 0; for (int c = 0; c < 3; c++) { if (hv[c][0] > hmax) hmax = hv[c][0]; if (hv[c][1] > vmax) vmax = hv[c][1]; }
            for (int c = 0; c < 3; c++) {
                const uint32_t eh = hmax / hv[c][0], ev = vmax / hv[c][1];
                const uint32_t dxs[4] = { 1, eh, eh + 1, 97 }, dys[4] = { 1, ev, ev + 1, 41 };
                for (int a = 0; a < 4; a++) {
                    const JsImage im = image(3, hv, dxs[a], dys[a]);
                    uint32_t w = 0, h = 0, sx = 0, sy = 0;
                    CHECK(js_plane_size(im, def, c, &w, &h, &sx, &sy) == 0 && w == dxs[a] && h == dys[a] && sx == 1 && sy == 1);
                    CHECK(js_plane_size(im, ni, c, &w, &h, &sx, &sy) == 0 && sx == eh && sy == ev);
                    CHECK(w == (dxs[a] + eh - 1) / eh && h == (dys[a] + ev - 1) / ev && w >= 1 && h >= 1);
                    CHECK((w - 1) * sx < im.dim_x && (h - 1) * sy < im.dim_y && w * sx >= im.dim_x && h * sy >= im.dim_y);
                    CHECK(im.dim_x <= im.blk_xmax * 8 && im.dim_y <= im.blk_ymax * 8);
                    CHECK(js_plane_size(im, ni, c, &w, &h, nullptr, nullptr) == 0);
                    CHECK(js_plane_dense_bytes(w, h, nf) == (uint64_t)w * h * 4 && js_plane_dense_row(w, nu) == w && js_plane_dense_row(w, ni) == 2ull * w);
                    CHECK(js_plane_units(w, h) == (uint64_t)h * ((w + 511) / 512));
                }
            }
            layouts++;
        }
        CHECK(layouts == 4096);
        uint32_t w = 0, h = 0, sx = 0, sy = 0;
        CHECK(js_plane_size(imgs[1], ni, 0, &w, &h, &sx, &sy) == 0 && w == 1 && h == 1 && sx == 1 && sy == 1);       // one component: 1 x 1
        CHECK(js_plane_size(imgs[0], ni, 2, &w, &h, &sx, &sy) == 0 && w == 167 && h == 109 && sx == 2 && sy == 2);
        CHECK(js_plane_size(imgs[0], ni, 0, &w, &h, &sx, &sy) == 0 && w == 333 && h == 217 && sx == 1 && sy == 1);
        CHECK(js_plane_size(imgs[2], ni, 1, &w, &h, &sx, &sy) == 0 && w == 257 && h == 9 && sx == 4 && sy == 1);
        CHECK(js_plane_size(imgs[3], ni, 2, &w, &h, &sx, &sy) == 0 && w == 513 && h == 9 && sx == 1 && sy == 2);
        CHECK(js_plane_size(imgs[4], ni, 0, &w, &h, &sx, &sy) == 0 && w == 100 && h == 17 && sx == 1 && sy == 3);   // luma is not always the finest grid
        CHECK(js_plane_size(imgs[4], ni, 1, &w, &h, &sx, &sy) == 0 && w == 34 && h == 50 && sx == 3 && sy == 1);
        CHECK(js_plane_size(imgs[0], def, 3, &w, &h, &sx, &sy) == -1 && js_plane_size(imgs[0], def, -1, &w, &h, &sx, &sy) == -1 && js_plane_size(imgs[1], def, 1, &w, &h, &sx, &sy) == -1);
        JsImage bad = imgs[0]; bad.expand_h[2] = 0; CHECK(js_plane_size(bad, def, 1, &w, &h, &sx, &sy) == -1 && g_err.find("geometry") != std::string::npos);
        bad = imgs[0]; bad.blk_xmax = 41;            CHECK(js_plane_size(bad, def, 0, &w, &h, &sx, &sy) == -1);          // a plane narrower than dim_x
        bad = imgs[0]; bad.plane_off = 4;            CHECK(js_plane_size(bad, def, 0, &w, &h, &sx, &sy) == -1);          // rows must start on 16 bytes
    }
    // an accepted call: components in any order, an image listed twice, dense and pitched destinations
    {
        const int which[5] = { 0, 0, 2, 1, 3 };
        JsnoopPlaneDst dst[5] = { { mem + 1, 0, 2, 0 }, { mem + 3, 333 + 1, 0, 0 }, { mem + 7, 0, 1, 0 }, { mem, 0, 0, 0 }, { mem + 5, 600, 2, 0 } };
        std::vector<JsPlaneRec> r; std::vector<uint32_t> b;
        CHECK(plan(fu, which, 5, dst, &r, &b) == 0);
        CHECK(b[0] == 0 && b[1] == 217 && b[2] == 434 && b[3] == 434 + 9 * 3 && b[4] == 462 && b[5] == 462 + 17 * 2);
        const uint64_t psz0 = 336ull * 224;
        CHECK(r[0].w == 333 && r[0].h == 217 && r[0].eh == 1 && r[0].ev == 1 && r[0].pw == 336 && r[0].src_off == 64 + 2 * psz0 && r[0].xlim == 333 && r[0].comp == 2 && r[0].segs == 1);
        CHECK(r[0].row_pitch == 333 && r[0].ptr == (uint64_t)(uintptr_t)(mem + 1) && r[1].row_pitch == 334 && r[1].src_off == 64 && r[1].comp == 0);
        CHECK(r[2].w == 1025 && r[2].segs == 3 && r[2].pw == 1056 && r[2].src_off == 128 + 1056ull * 16 && r[2].row_pitch == 1025);
        CHECK(r[3].w == 1 && r[3].h == 1 && r[3].pw == 8 && r[3].src_off == (1u << 20) && r[3].segs == 1);
        CHECK(r[4].w == 513 && r[4].h == 17 && r[4].segs == 2 && r[4].row_pitch == 600 && r[4].pw == 520);
        CHECK(plan(nu, which, 5, dst, &r, &b) == 0);
        CHECK(r[0].w == 167 && r[0].h == 109 && r[0].eh == 2 && r[0].ev == 2 && r[0].row_pitch == 167 && r[0].xlim == 333 && r[0].src_off == 64 + 2 * psz0);
        CHECK(r[1].w == 333 && r[1].eh == 1 && r[2].w == 257 && r[2].eh == 4 && r[2].ev == 1 && r[2].segs == 1 && r[4].w == 513 && r[4].h == 9 && r[4].ev == 2);
        CHECK(b[1] == 109 && b[2] == 109 + 217 && b[3] == 326 + 9 && b[4] == 336 && b[5] == 336 + 18);
        JsnoopPlaneDst d2[2] = { { mem, 0, 1, 0 }, { mem + 16, 8, 0, 0 } };
        CHECK(plan(nf, nullptr, 2, d2, &r, &b) == 0);                    // images == NULL: 0 .. n - 1
        CHECK(r[0].row_pitch == 167 * 4 && r[1].row_pitch == 8 && b[2] == 110);
        const int big = 5; JsnoopPlaneDst d3 = { mem, 0, 0, 0 };
        CHECK(plan(fi, &big, 1, &d3, &r, &b) == 0 && r[0].w == 1920 && r[0].segs == 4 && b[1] == 1080 * 4 && r[0].src_off == (1u << 24) && r[0].row_pitch == 3840);
    }
    // the refusals, and pitches at their limits
    {
        JsnoopPlaneDst d = { mem, 0, 0, 0 }; int i;
        i = 6;  CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("out of range") != std::string::npos);
        i = -1; CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("out of range") != std::string::npos);
        i = 0;
        d = { nullptr, 0, 0, 0 };      CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("NULL") != std::string::npos);
        d = { mem, 0, 0, 1 };          CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("reserved") != std::string::npos);
        d = { mem, 0, 3, 0 };          CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("component") != std::string::npos);
        d = { mem, 0, 0xFFFFFFFFu, 0 }; CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("component") != std::string::npos);
        i = 1; d = { mem, 0, 1, 0 };   CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("component") != std::string::npos);
        i = 0;
        d = { mem, 664, 0, 0 };        CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("row_pitch") != std::string::npos);
        d = { mem, 666, 0, 0 };        CHECK(plan(fi, &i, 1, &d) == 0);
        d = { mem, 667, 0, 0 };        CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("multiples of 2") != std::string::npos);
        d = { mem + 1, 0, 0, 0 };      CHECK(plan(fi, &i, 1, &d) == -1 && g_err.find("multiples of 2") != std::string::npos);
        d = { mem + 2, 668, 0, 0 };    CHECK(plan(fi, &i, 1, &d) == 0);
        d = { mem, 332, 0, 0 };        CHECK(plan(fu, &i, 1, &d) == -1 && g_err.find("row_pitch") != std::string::npos);
        d = { mem + 1, 333, 0, 0 };    CHECK(plan(fu, &i, 1, &d) == 0);
        d = { mem + 15, 334, 0, 0 };   CHECK(plan(fu, &i, 1, &d) == 0);
        d = { mem + 2, 0, 0, 0 };      CHECK(plan(ff, &i, 1, &d) == -1 && g_err.find("multiples of 4") != std::string::npos);
        d = { mem, 1334, 0, 0 };       CHECK(plan(ff, &i, 1, &d) == -1 && g_err.find("multiples of 4") != std::string::npos);
        d = { mem, 1328, 0, 0 };       CHECK(plan(ff, &i, 1, &d) == -1 && g_err.find("row_pitch") != std::string::npos);
        d = { mem + 4, 1332, 0, 0 };   CHECK(plan(ff, &i, 1, &d) == 0);
        d = { mem, 166, 1, 0 };        CHECK(plan(nu, &i, 1, &d) == -1 && g_err.find("row_pitch") != std::string::npos);       // NATIVE: the dense row is the decimated one
        d = { mem, 167, 1, 0 };        CHECK(plan(nu, &i, 1, &d) == 0);
        d = { mem, 1ull << 40, 1, 0 }; CHECK(plan(nu, &i, 1, &d) == 0);
        const int two[2] = { 0, 9 }; JsnoopPlaneDst d2[2] = { { mem, 0, 0, 0 }, { mem, 0, 0, 0 } };   // the second entry bad: still -1
        CHECK(plan(fi, two, 2, d2) == -1);
    }
    // a prefix table whose unit count passes 2^32
    {
        imgs.push_back(image(1, kGrey, 65535, 65535));                   // 128 segments a row: 2^23 units a listing
        std::vector<int> many(512, 6); std::vector<JsnoopPlaneDst> d(512, JsnoopPlaneDst{ mem, 0, 0, 0 });
        CHECK(plan(fu, many.data(), 512, d.data()) == -1 && g_err.find("row segments") != std::string::npos);
        std::vector<uint32_t> b;
        CHECK(plan(fu, many.data(), 500, d.data(), nullptr, &b) == 0 && b[500] == 500u * 65535u * 128u);
        JsImage big = imgs[6]; big.dim_x = 65536; big.blk_xmax = 8192;
        uint32_t w = 0, h = 0; CHECK(js_plane_size(big, def, 0, &w, &h, nullptr, nullptr) == -1);
    }
    printf("ok\n");
    return 0;
}
