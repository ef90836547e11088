// Host-only program: the argument checks and the record / prefix-table arithmetic of jsnoop_batch_pack_stats (jpegsnoop_amd/csrc/jsnoop_stats_check.h) on
// hand-made image descriptors.  tests/test_stats_abi.py builds it with the address and undefined-behaviour sanitizers and runs it: every refusal the header
// lists that host arithmetic decides must come back as -1 with a text, every accepted call must fill exactly n records and n + 1 prefix entries, repeated and
// permuted lists must address their own rows and their own event-count words, and the prefix table must pass 2^32 units.  Prints "ok" and returns 0, or the
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
#include "../../jpegsnoop_amd/csrc/jsnoop_stats_check.h"

static std::string g_err;
void js_set_error(const char* fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)

// the geometry js_geometry makes for a picture of mcu_x x mcu_y MCUs of hmax x vmax blocks
static JsImage image(uint32_t ncomp, uint32_t hmax, uint32_t vmax, uint32_t mcu_x, uint32_t mcu_y, uint64_t plane_off)
{
    JsImage im; memset(&im, 0, sizeof im);
    im.ncomp = ncomp; im.mcu_xmax = mcu_x; im.mcu_ymax = mcu_y; im.mcu_w = hmax * 8; im.mcu_h = vmax * 8; im.blk_xmax = mcu_x * hmax; im.blk_ymax = mcu_y * vmax;
    im.img_x = im.dim_x = mcu_x * im.mcu_w; im.img_y = im.dim_y = mcu_y * im.mcu_h; im.plane_off = plane_off; im.want_planes = 1;
    return im;
}

int main()
{
    std::vector<JsImage> imgs = { image(3, 2, 2, 120, 68, 0), image(1, 1, 1, 1, 1, 6266880), image(3, 1, 1, 65, 2, 6267072), image(3, 2, 1, 33, 3, 6270000 + 48) };
    alignas(16) static uint32_t mem[16];
    auto plan = [&](const int* images, int n, const void* dst, uint64_t pitch, std::vector<JsStatRec>* recs_out = nullptr, std::vector<uint64_t>* base_out = nullptr, uint64_t* rows_out = nullptr) {
        std::vector<JsStatRec> recs((size_t)n); std::vector<uint64_t> base((size_t)n + 1, 0xA5A5A5A5A5A5A5A5ull);      // to the byte: a write past either is the sanitizer's to report
        uint64_t rows = 77;
        g_err.clear();
        const int rc = js_stats_plan(imgs.data(), imgs.size(), images, n, dst, pitch, recs.data(), base.data(), &rows);
        if (recs_out) *recs_out = recs;
        if (base_out) *base_out = base;
        if (rows_out) *rows_out = rows;
        return rc;
    };
    CHECK(sizeof(JsStatRec) == 80 && JSNOOP_STATS_WORDS == 2482 && JS_STATS_UNIT == 512 && JS_STATS_UNIT % 8 == 0);
    CHECK(js_stats_units(imgs[0]) == 1088ull * 4 && js_stats_units(imgs[1]) == 8 && js_stats_units(imgs[2]) == 16ull * 2 && js_stats_units(imgs[3]) == 24ull * 2);
    CHECK(js_stats_pitch(0) == 2482 && js_stats_pitch(2482) == 2482 && js_stats_pitch(4096) == 4096);
    CHECK(js_stats_pitch(2481) == 0 && g_err.find("row_pitch_words") != std::string::npos && js_stats_pitch(1) == 0);
    CHECK(js_stats_scratch_bytes(3, 100) == (3 * 8 + 100) * 4);

    // an accepted call: a permuted subset with a repeat, dense
    {
        const int which[5] = { 2, 0, 2, 1, 3 };
        std::vector<JsStatRec> r; std::vector<uint64_t> b; uint64_t rows = 0;
        CHECK(plan(which, 5, mem, 0, &r, &b, &rows) == 0);
        CHECK(b[0] == 0 && b[1] == 32 && b[2] == 32 + 4352 && b[3] == 64 + 4352 && b[4] == 72 + 4352 && b[5] == 120 + 4352);
        CHECK(rows == 16 + 1088 + 16 + 8 + 24);
        for (int k = 0; k < 5; k++) CHECK(r[k].dst == (uint64_t)(uintptr_t)mem + (uint64_t)k * 2482 * 4);
        CHECK(r[0].row_base == 0 && r[1].row_base == 16 && r[2].row_base == 16 + 1088 && r[3].row_base == 32 + 1088 && r[4].row_base == 40 + 1088);
        CHECK(r[0].img_x == 520 && r[0].img_y == 16 && r[0].pw == 520 && r[0].psz == 520ull * 16 && r[0].tiles == 2 && r[0].ncomp == 3 && r[0].mcu_w == 8 && r[0].across == 65 && r[0].plane_off == 6267072);
        CHECK(r[2].plane_off == r[0].plane_off && r[2].img_x == r[0].img_x && r[2].dst != r[0].dst && r[2].row_base != r[0].row_base);     // the repeat: its own row, its own counts
        CHECK(r[1].img_x == 1920 && r[1].img_y == 1088 && r[1].tiles == 4 && r[1].mcu_w == 16 && r[1].mcu_h == 16 && r[1].across == 120 && r[1].psz == 1920ull * 1088);
        CHECK(r[3].ncomp == 1 && r[3].img_x == 8 && r[3].tiles == 1 && r[4].img_x == 528 && r[4].tiles == 2 && r[4].mcu_w == 16 && r[4].mcu_h == 8 && r[4].across == 33);
        CHECK(r[0].shift_ind == 0 && r[0].shift_y == 0 && r[0].shift_cb == 0 && r[0].shift_cr == 0);
        // images == NULL: 0 .. n - 1; a pitch above the row
        CHECK(plan(nullptr, 3, mem + 1, 3000, &r, &b, &rows) == 0);
        CHECK(r[0].img_x == 1920 && r[1].img_x == 8 && r[2].img_x == 520 && b[3] == 4352 + 8 + 32 && rows == 1088 + 8 + 16);
        CHECK(r[1].dst == (uint64_t)(uintptr_t)(mem + 1) + 3000ull * 4 && r[2].dst == (uint64_t)(uintptr_t)(mem + 1) + 6000ull * 4);
        // the preview shift is carried along
        imgs[2].shift_mcu_x = 3; imgs[2].shift_mcu_y = 1; imgs[2].shift_y = -5; imgs[2].shift_cb = 6; imgs[2].shift_cr = 7;
        const int two = 2;
        CHECK(plan(&two, 1, mem, 0, &r) == 0 && r[0].shift_ind == 68 && r[0].shift_y == -5 && r[0].shift_cb == 6 && r[0].shift_cr == 7);
        imgs[2].shift_mcu_x = imgs[2].shift_mcu_y = 0; imgs[2].shift_y = imgs[2].shift_cb = imgs[2].shift_cr = 0;
    }
    // the refusals
    {
        int i;
        i = 4;  CHECK(plan(&i, 1, mem, 0) == -1 && g_err.find("out of range") != std::string::npos);
        i = -1; CHECK(plan(&i, 1, mem, 0) == -1 && g_err.find("out of range") != std::string::npos);
        i = 0;
        CHECK(plan(&i, 1, nullptr, 0) == -1 && g_err.find("NULL") != std::string::npos);
        CHECK(plan(&i, 1, (const unsigned char*)mem + 2, 0) == -1 && g_err.find("multiple of 4") != std::string::npos);
        CHECK(plan(&i, 1, (const unsigned char*)mem + 1, 0) == -1);
        CHECK(plan(&i, 1, mem, 2481) == -1 && g_err.find("row_pitch_words") != std::string::npos);
        CHECK(plan(&i, 1, mem, 1) == -1);
        CHECK(plan(&i, 1, mem, 2482) == 0 && plan(&i, 1, mem, 2483) == 0);
        const int two[2] = { 0, 9 };                                       // the second entry bad: still -1
        CHECK(plan(two, 2, mem, 0) == -1);
        CHECK(plan(nullptr, 5, mem, 0) == -1 && g_err.find("out of range") != std::string::npos);      // NULL list, n past the batch
        JsImage keep = imgs[1];
        imgs[1].img_x = 0;   CHECK(plan(nullptr, 2, mem, 0) == -1 && g_err.find("geometry") != std::string::npos);
        imgs[1] = keep; imgs[1].plane_off += 4; CHECK(plan(nullptr, 2, mem, 0) == -1 && g_err.find("geometry") != std::string::npos);
        imgs[1] = keep; imgs[1].blk_xmax = 0;   CHECK(plan(nullptr, 2, mem, 0) == -1);
        imgs[1] = keep; CHECK(plan(nullptr, 2, mem, 0) == 0);
    }
    // a prefix table whose unit count passes 2^32: 64-bit entries, nothing refused
    {
        imgs.push_back(image(3, 1, 1, 8000, 8000, 1ull << 33));             // 64 000 rows of 125 units: 8 000 000 units an entry
        std::vector<int> many(600, 4); std::vector<JsStatRec> r; std::vector<uint64_t> b; uint64_t rows = 0;
        CHECK(plan(many.data(), 600, mem, 0, &r, &b, &rows) == 0);
        CHECK(b[600] == 600ull * 8000000ull && b[600] > (1ull << 32) && b[537] == 537ull * 8000000ull && rows == 600ull * 64000);
        CHECK(r[599].row_base == 599ull * 64000 && r[599].tiles == 125 && r[599].plane_off == (1ull << 33) && r[599].psz == 64000ull * 64000);
    }
    printf("ok\n");
    return 0;
}
