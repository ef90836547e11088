// Host-only program: the argument checks and the record / prefix-table arithmetic of jsnoop_batch_pack (jpegsnoop_amd/csrc/jsnoop_pack_check.h)
// on hand-made image descriptors.  tests/test_pack_abi.py builds it with the address and undefined-behaviour sanitizers and runs it: every
// refusal the header lists must come back as -1 with a text and leave the outputs alone, every accepted call must fill exactly n records and
// n + 1 prefix entries.  Prints "ok" and returns 0, or the line that failed.
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

static JsImage image(uint32_t dx, uint32_t dy, uint32_t mcu)
{
    JsImage im; memset(&im, 0, sizeof im);
    im.dim_x = dx; im.dim_y = dy; im.img_x = (dx + mcu - 1) / mcu * mcu; im.img_y = (dy + mcu - 1) / mcu * mcu;
    return im;
}

int main()
{
    std::vector<JsImage> imgs = { image(333, 217, 16), image(1, 1, 8), image(1920, 1080, 16), image(513, 2, 8) };
    JsImage undecoded = image(8, 8, 8); undecoded.dim_x = 0; imgs.push_back(undecoded);
    alignas(16) static unsigned char mem[64];
    // exactly n records and n + 1 prefix entries, allocated to the byte: a write past either is the sanitizer's to report
    auto plan = [&](const JsnoopPackSpec& s, const int* images, int n, const JsnoopPackDst* dst, std::vector<JsPackRec>* recs_out = nullptr, std::vector<uint32_t>* base_out = nullptr) {
        std::vector<JsPackRec> recs((size_t)n); std::vector<uint32_t> base((size_t)n + 1, 0xA5A5A5A5u);
        g_err.clear();
        const int rc = js_pack_plan(imgs.data(), imgs.size(), s, images, n, dst, recs.data(), base.data());
        if (recs_out) *recs_out = recs;
        if (base_out) *base_out = base;
        return rc;
    };
    JsnoopPackSpec def; js_pack_spec_defaults(&def);
    CHECK(def.struct_size == sizeof(JsnoopPackSpec) && def.layout == 0 && def.dtype == 0 && def.bgr == 0);
    for (int c = 0; c < 3; c++) CHECK(def.scale[c] == 1.0f && def.bias[c] == 0.0f);

    // spec import: shorter accepted with defaults, longer refused, unknown layout / dtype refused
    JsnoopPackSpec in = def, s;
    in.struct_size = 16; in.layout = JSNOOP_PACK_CHW; in.dtype = JSNOOP_PACK_F32; in.scale[0] = 7.0f;
    CHECK(js_pack_import_spec(&in, &s) == 0 && s.layout == JSNOOP_PACK_CHW && s.dtype == JSNOOP_PACK_F32 && s.scale[0] == 1.0f && s.struct_size == sizeof s);
    in.struct_size = sizeof in + 4; CHECK(js_pack_import_spec(&in, &s) == -1 && !g_err.empty());
    in.struct_size = 0; CHECK(js_pack_import_spec(&in, &s) == -1);
    in = def; in.layout = 2; CHECK(js_pack_import_spec(&in, &s) == -1 && g_err.find("layout") != std::string::npos);
    in = def; in.dtype = -1; CHECK(js_pack_import_spec(&in, &s) == -1 && g_err.find("dtype") != std::string::npos);
    CHECK(js_pack_import_spec(nullptr, &s) == -1);

    // dense sizes and units
    JsnoopPackSpec hwc8 = def, chw8 = def, hwcf = def, chwf = def;
    chw8.layout = JSNOOP_PACK_CHW; hwcf.dtype = JSNOOP_PACK_F32; chwf.layout = JSNOOP_PACK_CHW; chwf.dtype = JSNOOP_PACK_F32;
    CHECK(js_pack_dense_bytes(imgs[0], hwc8) == 333ull * 217 * 3 && js_pack_dense_bytes(imgs[0], chwf) == 333ull * 217 * 12);
    CHECK(js_pack_dense_row(imgs[0], hwc8) == 999 && js_pack_dense_row(imgs[0], chw8) == 333 && js_pack_dense_row(imgs[0], hwcf) == 3996 && js_pack_dense_row(imgs[0], chwf) == 1332);
    CHECK(js_pack_units(imgs[0]) == 217 && js_pack_units(imgs[1]) == 1 && js_pack_units(imgs[2]) == 1080 * 4 && js_pack_units(imgs[3]) == 4);

    // an accepted call: a subset in non-ascending order, dense and pitched destinations
    {
        const int which[3] = { 3, 0, 1 };
        JsnoopPackDst dst[3] = { { mem + 1, 0, 0 }, { mem + 2, 1012, 0 }, { mem + 3, 0, 0 } };
        std::vector<JsPackRec> r; std::vector<uint32_t> b;
        CHECK(plan(hwc8, which, 3, dst, &r, &b) == 0);
        CHECK(b[0] == 0 && b[1] == 4 && b[2] == 4 + 217 && b[3] == 4 + 217 + 1);
        CHECK(r[0].img == 3 && r[0].row_pitch == 513 * 3 && r[1].img == 0 && r[1].row_pitch == 1012 && r[2].img == 1 && r[2].ptr == (uint64_t)(uintptr_t)(mem + 3));
        JsnoopPackDst d2[2] = { { mem, 0, 0 }, { mem + 16, 336 * 4, 336 * 4 * 224 } };
        CHECK(plan(chwf, nullptr, 2, d2, &r, &b) == 0);                  // images == NULL: 0 .. n - 1
        CHECK(r[0].img == 0 && r[0].row_pitch == 1332 && r[0].plane_pitch == 1332ull * 217 && r[1].img == 1 && r[1].row_pitch == 1344 && r[1].plane_pitch == 1344ull * 224);
        CHECK(b[2] == 218);
    }
    // the refusals
    {
        JsnoopPackDst d = { mem, 0, 0 }; int i;
        i = 5;  CHECK(plan(hwc8, &i, 1, &d) == -1 && g_err.find("out of range") != std::string::npos);
        i = -1; CHECK(plan(hwc8, &i, 1, &d) == -1 && g_err.find("out of range") != std::string::npos);
        i = 4;  CHECK(plan(hwc8, &i, 1, &d) == -1 && g_err.find("image 4 has no decoded DIB") != std::string::npos);
        i = 0;
        d = { nullptr, 0, 0 };          CHECK(plan(hwc8, &i, 1, &d) == -1 && g_err.find("NULL") != std::string::npos);
        d = { mem, 998, 0 };            CHECK(plan(hwc8, &i, 1, &d) == -1 && g_err.find("row_pitch") != std::string::npos);
        d = { mem, 999, 0 };            CHECK(plan(hwc8, &i, 1, &d) == 0);
        d = { mem, 999, 5 };            CHECK(plan(hwc8, &i, 1, &d) == 0);                       // HWC ignores plane_pitch
        d = { mem, 332, 0 };            CHECK(plan(chw8, &i, 1, &d) == -1 && g_err.find("row_pitch") != std::string::npos);
        d = { mem, 340, 340 * 217 - 1 }; CHECK(plan(chw8, &i, 1, &d) == -1 && g_err.find("plane_pitch") != std::string::npos);
        d = { mem, 340, 340 * 217 };    CHECK(plan(chw8, &i, 1, &d) == 0);
        d = { mem + 2, 0, 0 };          CHECK(plan(chwf, &i, 1, &d) == -1 && g_err.find("multiples of 4") != std::string::npos);
        d = { mem, 1334, 0 };           CHECK(plan(chwf, &i, 1, &d) == -1 && g_err.find("multiples of 4") != std::string::npos);
        d = { mem, 1336, 1336 * 217 + 2 }; CHECK(plan(chwf, &i, 1, &d) == -1 && g_err.find("multiples of 4") != std::string::npos);
        d = { mem, 3998, 0 };           CHECK(plan(hwcf, &i, 1, &d) == -1);
        d = { mem + 4, 4000, 0 };       CHECK(plan(hwcf, &i, 1, &d) == 0);
        // the second entry bad: still -1
        const int two[2] = { 0, 9 }; JsnoopPackDst d2[2] = { { mem, 0, 0 }, { mem, 0, 0 } };
        CHECK(plan(hwc8, two, 2, d2) == -1);
    }
    // more row segments than the 32-bit prefix holds
    {
        imgs.push_back(image(1, 0x40000000u, 8));
        std::vector<int> many(5, 5); std::vector<JsnoopPackDst> d(5, JsnoopPackDst{ mem, 0, 0 });
        CHECK(plan(hwc8, many.data(), 5, d.data()) == -1 && g_err.find("row segments") != std::string::npos);
        CHECK(plan(hwc8, many.data(), 3, d.data()) == 0);
    }
    printf("ok\n");
    return 0;
}
