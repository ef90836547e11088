// Host-only program: the argument checks and the record / prefix-table arithmetic of jsnoop_batch_pack_resized (jpegsnoop_amd/csrc/jsnoop_pack_check.h)
// on hand-made image descriptors.  tests/test_resize_abi.py builds it with the address and undefined-behaviour sanitizers and runs it: every
// refusal the header lists must come back as -1 with a text that names the entry and the image, every accepted call must fill exactly n records and
// n + 1 prefix entries, and js_pack_plan must behave as before.  Prints "ok" and returns 0, or the line that failed.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#ifndef __HIPCC__              // (a plain host compiler: the descriptors' header marks one helper for both sides)
#define __host__
#define __device__
#endif
#include "../../jpegsnoop_amd/csrc/jsnoop_pack_check.h"

static std::string g_err;
void js_set_error(const char* fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)
static bool said(const char* w) { return g_err.find(w) != std::string::npos; }

static JsImage image(uint32_t dx, uint32_t dy, uint32_t mcu)
{
    JsImage im; memset(&im, 0, sizeof im);
    im.dim_x = dx; im.dim_y = dy; im.img_x = (dx + mcu - 1) / mcu * mcu; im.img_y = (dy + mcu - 1) / mcu * mcu;
    return im;
}
static JsnoopResizeDst dst_of(void* p, uint64_t rp, uint64_t pp, uint32_t ow, uint32_t oh, uint32_t x = 0, uint32_t y = 0, uint32_t w = 0, uint32_t h = 0)
{
    JsnoopResizeDst d; memset(&d, 0, sizeof d);
    d.ptr = p; d.row_pitch = rp; d.plane_pitch = pp; d.out_w = ow; d.out_h = oh; d.roi_x = x; d.roi_y = y; d.roi_w = w; d.roi_h = h;
    return d;
}

int main()
{
    static_assert(sizeof(JsnoopResizeDst) == 48 && sizeof(JsResizeRec) == 56, "records");
    std::vector<JsImage> imgs = { image(333, 217, 16), image(1, 1, 8), image(1920, 1080, 16), image(65535, 2, 8) };
    JsImage undecoded = image(8, 8, 8); undecoded.dim_x = 0; imgs.push_back(undecoded);
    alignas(16) static unsigned char mem[64];
    // exactly n records and n + 1 prefix entries, allocated to the byte: a write past either is the sanitizer's to report
    auto plan = [&](const JsnoopPackSpec& s, const int* images, int n, const JsnoopResizeDst* dst, std::vector<JsResizeRec>* recs_out = nullptr, std::vector<uint32_t>* base_out = nullptr) {
        std::vector<JsResizeRec> recs((size_t)n); std::vector<uint32_t> base((size_t)n + 1, 0xA5A5A5A5u);
        g_err.clear();
        const int rc = js_resize_plan(imgs.data(), imgs.size(), s, images, n, dst, recs.data(), base.data());
        if (recs_out) *recs_out = recs;
        if (base_out) *base_out = base;
        return rc;
    };
    JsnoopPackSpec hwc8; js_pack_spec_defaults(&hwc8);
    JsnoopPackSpec chw8 = hwc8, hwcf = hwc8, chwf = hwc8;
    chw8.layout = JSNOOP_PACK_CHW; hwcf.dtype = JSNOOP_PACK_F32; chwf.layout = JSNOOP_PACK_CHW; chwf.dtype = JSNOOP_PACK_F32;

    // the spec's refusals name this entry point
    { JsnoopPackSpec bad = hwc8, got; bad.layout = 2; CHECK(js_pack_import_spec(&bad, &got, "pack_resized") == -1 && said("pack_resized: unknown layout 2"));
      CHECK(js_pack_import_spec(&bad, &got) == -1 && g_err == "pack: unknown layout 2"); }
    // filters
    CHECK(js_resize_check_filter(JSNOOP_RESIZE_NEAREST) == 0 && js_resize_check_filter(JSNOOP_RESIZE_BILINEAR) == 0 && js_resize_check_filter(JSNOOP_RESIZE_AREA) == 0);
    CHECK(js_resize_check_filter(3) == -1 && said("filter 3"));
    CHECK(js_resize_check_filter(-1) == -1 && said("filter"));
    // units: out_h * ceil(out_w / 256)
    CHECK(js_resize_units(1, 1) == 1 && js_resize_units(256, 3) == 3 && js_resize_units(257, 3) == 6 && js_resize_units(32767, 32767) == 32767ull * 128);

    // an accepted call: one image three times with different rectangles, another one whole; dense and pitched destinations
    {
        const int which[4] = { 0, 2, 0, 0 };
        JsnoopResizeDst dst[4] = { dst_of(mem + 1, 0, 0, 48, 32, 10, 20, 100, 50), dst_of(mem + 2, 700, 0, 224, 224), dst_of(mem + 3, 0, 0, 300, 2, 332, 216, 1, 1),
                                   dst_of(mem + 5, 0, 0, 7, 9, 0, 0, 333, 217) };
        std::vector<JsResizeRec> r; std::vector<uint32_t> b;
        CHECK(plan(hwc8, which, 4, dst, &r, &b) == 0);
        CHECK(b[0] == 0 && b[1] == 32 && b[2] == 32 + 224 && b[3] == 32 + 224 + 4 && b[4] == 32 + 224 + 4 + 9);
        CHECK(r[0].img == 0 && r[0].out_w == 48 && r[0].out_h == 32 && r[0].roi_x == 10 && r[0].roi_y == 20 && r[0].roi_w == 100 && r[0].roi_h == 50 && r[0].row_pitch == 144);
        CHECK(r[1].img == 2 && r[1].roi_x == 0 && r[1].roi_y == 0 && r[1].roi_w == 1920 && r[1].roi_h == 1080 && r[1].row_pitch == 700 && r[1].ptr == (uint64_t)(uintptr_t)(mem + 2));
        CHECK(r[2].roi_x == 332 && r[2].roi_w == 1 && r[2].row_pitch == 900 && r[3].roi_w == 333 && r[3].roi_h == 217);
        JsnoopResizeDst d2[2] = { dst_of(mem, 0, 0, 224, 100), dst_of(mem + 16, 240 * 4, 240 * 4 * 104, 224, 100) };
        CHECK(plan(chwf, nullptr, 2, d2, &r, &b) == 0);                  // images == NULL: 0 .. n - 1
        CHECK(r[0].img == 0 && r[0].row_pitch == 896 && r[0].plane_pitch == 89600 && r[1].img == 1 && r[1].row_pitch == 960 && r[1].plane_pitch == 960ull * 104 && r[1].roi_w == 1 && r[1].roi_h == 1);
        CHECK(b[2] == 200);
        // the widest rectangle and the largest output a call can name
        const int wide = 3; JsnoopResizeDst dw = dst_of(mem, 0, 0, 32767, 32767);
        CHECK(plan(chw8, &wide, 1, &dw, &r, &b) == 0 && r[0].roi_w == 65535 && b[1] == 32767u * 128u);
    }
    // the refusals
    {
        JsnoopResizeDst d = dst_of(mem, 0, 0, 8, 8); int i;
        i = 5;  CHECK(plan(hwc8, &i, 1, &d) == -1 && said("out of range") && said("entry 0"));
        i = -1; CHECK(plan(hwc8, &i, 1, &d) == -1 && said("out of range"));
        i = 4;  CHECK(plan(hwc8, &i, 1, &d) == -1 && said("image 4 has no decoded DIB"));
        i = 0;
        d = dst_of(nullptr, 0, 0, 8, 8);        CHECK(plan(hwc8, &i, 1, &d) == -1 && said("NULL") && said("destination 0 (image 0)"));
        d = dst_of(mem, 0, 0, 0, 8);            CHECK(plan(hwc8, &i, 1, &d) == -1 && said("output size") && said("destination 0 (image 0)"));
        d = dst_of(mem, 0, 0, 8, 0);            CHECK(plan(hwc8, &i, 1, &d) == -1 && said("output size"));
        d = dst_of(mem, 0, 0, 32768, 8);        CHECK(plan(hwc8, &i, 1, &d) == -1 && said("output size"));
        d = dst_of(mem, 0, 0, 8, 0xFFFFFFFFu);  CHECK(plan(hwc8, &i, 1, &d) == -1 && said("output size"));
        d = dst_of(mem, 0, 0, 32767, 32767);    CHECK(plan(hwc8, &i, 1, &d) == 0);
        d = dst_of(mem, 0, 0, 8, 8, 0, 0, 5, 0); CHECK(plan(hwc8, &i, 1, &d) == -1 && said("ROI") && said("(image 0)"));
        d = dst_of(mem, 0, 0, 8, 8, 0, 0, 0, 5); CHECK(plan(hwc8, &i, 1, &d) == -1 && said("ROI"));
        d = dst_of(mem, 0, 0, 8, 8, 1, 0, 0, 0); CHECK(plan(hwc8, &i, 1, &d) == -1 && said("ROI"));
        d = dst_of(mem, 0, 0, 8, 8, 0, 2, 0, 0); CHECK(plan(hwc8, &i, 1, &d) == -1 && said("ROI"));
        d = dst_of(mem, 0, 0, 8, 8, 0, 0, 334, 217); CHECK(plan(hwc8, &i, 1, &d) == -1 && said("leaves image 0"));
        d = dst_of(mem, 0, 0, 8, 8, 1, 0, 333, 217); CHECK(plan(hwc8, &i, 1, &d) == -1 && said("leaves image 0"));
        d = dst_of(mem, 0, 0, 8, 8, 0, 217, 1, 1);   CHECK(plan(hwc8, &i, 1, &d) == -1 && said("leaves image 0"));
        d = dst_of(mem, 0, 0, 8, 8, 0xFFFFFFFFu, 0, 2, 1); CHECK(plan(hwc8, &i, 1, &d) == -1 && said("leaves image 0"));    // (x + w wraps in 32 bits)
        d = dst_of(mem, 0, 0, 8, 8, 332, 216, 1, 1); CHECK(plan(hwc8, &i, 1, &d) == 0);
        // "dense" is the OUTPUT's size
        d = dst_of(mem, 23, 0, 8, 8);           CHECK(plan(hwc8, &i, 1, &d) == -1 && said("row_pitch") && said("destination 0 (image 0)"));
        d = dst_of(mem, 24, 0, 8, 8);           CHECK(plan(hwc8, &i, 1, &d) == 0);
        d = dst_of(mem, 24, 5, 8, 8);           CHECK(plan(hwc8, &i, 1, &d) == 0);                       // HWC ignores plane_pitch
        d = dst_of(mem, 7, 0, 8, 8);            CHECK(plan(chw8, &i, 1, &d) == -1 && said("row_pitch"));
        d = dst_of(mem, 9, 71, 8, 8);           CHECK(plan(chw8, &i, 1, &d) == -1 && said("plane_pitch"));
        d = dst_of(mem, 9, 72, 8, 8);           CHECK(plan(chw8, &i, 1, &d) == 0);
        d = dst_of(mem + 2, 0, 0, 8, 8);        CHECK(plan(chwf, &i, 1, &d) == -1 && said("multiples of 4"));
        d = dst_of(mem, 34, 0, 8, 8);           CHECK(plan(chwf, &i, 1, &d) == -1 && said("multiples of 4"));
        d = dst_of(mem, 36, 36 * 8 + 2, 8, 8);  CHECK(plan(chwf, &i, 1, &d) == -1 && said("multiples of 4"));
        d = dst_of(mem, 94, 0, 8, 8);           CHECK(plan(hwcf, &i, 1, &d) == -1);
        d = dst_of(mem + 4, 100, 0, 8, 8);      CHECK(plan(hwcf, &i, 1, &d) == 0);
        // the second entry bad: still -1, and the text names it
        const int two[2] = { 0, 2 }; JsnoopResizeDst d2[2] = { dst_of(mem, 0, 0, 8, 8), dst_of(mem, 0, 0, 8, 8, 1900, 0, 21, 5) };
        CHECK(plan(hwc8, two, 2, d2) == -1 && said("destination 1") && said("image 2"));
    }
    // more row segments than the 32-bit prefix holds: 32767 * 128 per destination
    {
        std::vector<int> many(1100, 0); std::vector<JsnoopResizeDst> d(1100, dst_of(mem, 0, 0, 32767, 32767));
        CHECK(plan(hwc8, many.data(), 1100, d.data()) == -1 && said("row segments"));
        CHECK(plan(hwc8, many.data(), 1000, d.data()) == 0);
    }
    // js_pack_plan is what it was
    {
        const int which[3] = { 3, 0, 1 };
        JsnoopPackDst dst[3] = { { mem + 1, 0, 0 }, { mem + 2, 1012, 0 }, { mem + 3, 0, 0 } };
        std::vector<JsPackRec> r(3); std::vector<uint32_t> b(4);
        CHECK(js_pack_plan(imgs.data(), imgs.size(), hwc8, which, 3, dst, r.data(), b.data()) == 0);
        CHECK(b[0] == 0 && b[1] == 2 * 128 && b[2] == 256 + 217 && b[3] == 256 + 217 + 1 && r[1].row_pitch == 1012 && r[0].row_pitch == 65535ull * 3);
    }
    printf("ok\n");
    return 0;
}
