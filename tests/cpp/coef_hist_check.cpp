// Host-only program: the argument checks and the record / prefix-table arithmetic of jsnoop_batch_pack_coef_hist (jpegsnoop_amd/csrc/jsnoop_coef_hist_check.h)
// on hand-made image descriptors.  tests/test_coef_hist_abi.py builds it with the address and undefined-behaviour sanitizers and runs it: every refusal the
// header lists that host arithmetic decides must come back as -1 with a text, every accepted call must fill exactly n records and n + 1 prefix entries,
// repeated and permuted pairs must address their own rows, the row length must be right for every R, and the prefix table must pass 2^32 units.
// Prints "ok" and returns 0, or the line that failed.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#ifndef __HIPCC__              // (a plain host compiler: the descriptors' header marks one helper for both sides)
#define __host__
#define __device__
#endif
#include "../../jpegsnoop_amd/csrc/jsnoop_coef_hist_check.h"

static std::string g_err;
void js_set_error(const char* fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)

// the geometry js_geometry makes: ncomp components, the first sampled h x v, the others 1 x 1
static JsImage image(uint32_t ncomp, uint32_t h, uint32_t v, uint32_t mcu_x, uint32_t mcu_y, uint64_t coef_off)
{
    JsImage im; memset(&im, 0, sizeof im);
    im.ncomp = ncomp; im.mcu_xmax = mcu_x; im.mcu_ymax = mcu_y; im.coef_off = coef_off;
    uint32_t n = 0;
    for (uint32_t c = 1; c <= ncomp; c++) {
        im.samp_h[c] = c == 1 ? h : 1; im.samp_v[c] = c == 1 ? v : 1;
        for (uint32_t y = 0; y < im.samp_v[c]; y++) for (uint32_t x = 0; x < im.samp_h[c]; x++) { im.blk_comp[n] = (uint8_t)c; im.blk_ch[n] = (uint8_t)x; im.blk_cv[n] = (uint8_t)y; n++; }
    }
    im.blk_per_mcu = n; im.total_blocks = n * mcu_x * mcu_y;
    return im;
}
static int g_dqt_calls = 0;
static int dqt(void*, int image, int comp, uint16_t* out64)
{
    g_dqt_calls++;
    for (int k = 0; k < 64; k++) out64[k] = (uint16_t)(k == 5 ? 0 : (k == 6 ? 65535 : 1 + image * 100 + comp * 10 + k));
    return 0;
}

int main()
{
    std::vector<JsImage> imgs = { image(3, 2, 2, 120, 68, 0), image(1, 1, 1, 1, 1, 48960), image(3, 1, 1, 65, 2, 48961), image(3, 2, 1, 33, 3, 49351) };
    alignas(16) static uint32_t mem[16];
    JsnoopCoefHistSpec spec; js_coef_hist_spec_defaults(&spec);
    auto plan = [&](const JsnoopCoefHistSpec& s, const int* images, const int* comps, int n, const void* dst, uint64_t pitch, std::vector<JsCoefHistRec>* recs_out = nullptr, std::vector<uint64_t>* base_out = nullptr) {
        std::vector<JsCoefHistRec> recs((size_t)n); std::vector<uint64_t> base((size_t)n + 1, 0xA5A5A5A5A5A5A5A5ull);      // to the byte: a write past either is the sanitizer's to report
        g_err.clear();
        const int rc = js_coef_hist_plan(imgs.data(), imgs.size(), s, images, comps, n, dst, pitch, dqt, nullptr, recs.data(), base.data());
        if (recs_out) *recs_out = recs;
        if (base_out) *base_out = base;
        return rc;
    };
    CHECK(sizeof(JsCoefHistRec) == 304 && sizeof(JsCoefHistRec) % 16 == 0 && offsetof(JsCoefHistRec, recip) % 16 == 0 && JS_COEF_HIST_UNIT == 64 && JS_COEF_HIST_WAVES == 8 && JS_COEF_HIST_WG_PER_CU == 2);
    CHECK(spec.struct_size == 16 && spec.order == JSNOOP_COEF_NATURAL && spec.quantised == 1 && spec.range == 127);
    { const uint8_t zz[64] = JS_ZIGZAG_NATURAL, pos[64] = JS_ZIGZAG_POSITION; for (int k = 0; k < 64; k++) CHECK(zz[pos[k]] == k && pos[zz[k]] == k); }
    // the row length for every R, through the spec
    for (uint32_t r = 0; r <= 130; r++) {
        JsnoopCoefHistSpec s = spec, out; s.range = r;
        const int rc = js_coef_hist_import_spec(&s, &out);
        if (r >= 1 && r <= 127) { CHECK(rc == 0 && js_chist_words(out.range) == 64 * (2 * r + 1) + 128); }
        else CHECK(rc == -1 && g_err.find("range") != std::string::npos);
    }
    CHECK(js_coef_hist_units(1) == 1 && js_coef_hist_units(63) == 1 && js_coef_hist_units(64) == 1 && js_coef_hist_units(65) == 2 && js_coef_hist_units(0xFFFFFFFFu) == 67108864ull);
    CHECK(js_coef_hist_pitch(0, 448) == 448 && js_coef_hist_pitch(448, 448) == 448 && js_coef_hist_pitch(500, 448) == 500 && js_coef_hist_pitch(447, 448) == 0 && g_err.find("row_pitch_words") != std::string::npos);
    // struct_size: shorter accepted with the lacking fields at their defaults, longer refused
    {
        JsnoopCoefHistSpec s, out; memset(&s, 0xEE, sizeof s);
        s.struct_size = 4;  CHECK(js_coef_hist_import_spec(&s, &out) == 0 && out.order == 0 && out.quantised == 1 && out.range == 127 && out.struct_size == sizeof out);
        s.struct_size = 8; s.order = JSNOOP_COEF_ZIGZAG; CHECK(js_coef_hist_import_spec(&s, &out) == 0 && out.order == 1 && out.quantised == 1 && out.range == 127);
        s.struct_size = 12; s.quantised = 0; CHECK(js_coef_hist_import_spec(&s, &out) == 0 && out.quantised == 0 && out.range == 127);
        s.struct_size = 16; s.range = 16; CHECK(js_coef_hist_import_spec(&s, &out) == 0 && out.range == 16);
        s.struct_size = 20; CHECK(js_coef_hist_import_spec(&s, &out) == -1 && g_err.find("struct_size") != std::string::npos);
        s.struct_size = 3;  CHECK(js_coef_hist_import_spec(&s, &out) == -1);
        s.struct_size = 0;  CHECK(js_coef_hist_import_spec(&s, &out) == -1);
        s.struct_size = 16; s.order = 2; CHECK(js_coef_hist_import_spec(&s, &out) == -1 && g_err.find("order") != std::string::npos);
        s.order = -1; CHECK(js_coef_hist_import_spec(&s, &out) == -1);
        CHECK(js_coef_hist_import_spec(nullptr, &out) == -1 && g_err.find("NULL") != std::string::npos);
    }
    // an accepted call: permuted pairs with a repeat, dense
    {
        const int which[6] = { 2, 0, 0, 2, 1, 3 }, comps[6] = { 1, 0, 2, 1, 0, 0 };
        std::vector<JsCoefHistRec> r; std::vector<uint64_t> b;
        CHECK(plan(spec, which, comps, 6, mem, 0, &r, &b) == 0);
        // blocks: 130; 240 * 136 = 32640; 8160; 130; 1; 66 * 3 = 198
        CHECK(b[0] == 0 && b[1] == 3 && b[2] == 3 + 510 && b[3] == 513 + 128 && b[4] == 641 + 3 && b[5] == 644 + 1 && b[6] == 645 + 4);
        const uint32_t words = js_chist_words(127);
        for (int k = 0; k < 6; k++) CHECK(r[k].dst == (uint64_t)(uintptr_t)mem + (uint64_t)k * words * 4);
        CHECK(r[0].nblk == 130 && r[0].hv == 1 && r[0].first == 1 && r[0].bpm == 3 && r[0].coef_off == 48961 && r[0].hv_magic == 65537);
        CHECK(r[1].nblk == 32640 && r[1].hv == 4 && r[1].first == 0 && r[1].bpm == 6 && r[1].coef_off == 0 && r[1].hv_magic == 16385);
        CHECK(r[2].nblk == 8160 && r[2].hv == 1 && r[2].first == 5 && r[2].bpm == 6);
        CHECK(r[3].nblk == r[0].nblk && r[3].first == r[0].first && r[3].dst != r[0].dst);                            // the repeat: its own row
        CHECK(r[4].nblk == 1 && r[4].bpm == 1 && r[4].first == 0 && r[5].nblk == 198 && r[5].hv == 2 && r[5].bpm == 4 && r[5].hv_magic == 32769);
        // the divisors: reciprocals of the table of (image, comp); a 0 entry counts as 1; quantised == 0 takes no table at all
        CHECK(r[0].recip[0] == js_chist_recip(1 + 200 + 10) && r[0].recip[63] == js_chist_recip(1 + 200 + 10 + 63) && r[0].recip[5] == js_chist_recip(1) && r[0].recip[6] == js_chist_recip(65535));
        CHECK(r[1].recip[0] == js_chist_recip(1) && r[2].recip[1] == js_chist_recip(22));
        JsnoopCoefHistSpec raw = spec; raw.quantised = 0; raw.range = 2; g_dqt_calls = 0;
        CHECK(plan(raw, which, comps, 6, mem + 1, 1000, &r, &b) == 0 && g_dqt_calls == 0);
        for (int k = 0; k < 6; k++) { CHECK(r[k].dst == (uint64_t)(uintptr_t)(mem + 1) + (uint64_t)k * 4000); for (int f = 0; f < 64; f++) CHECK(r[k].recip[f] == 0x80000001u); }
        CHECK(b[6] == 649);
    }
    // the refusals
    {
        int i = 0, c = 0;
        i = 4;  CHECK(plan(spec, &i, &c, 1, mem, 0) == -1 && g_err.find("out of range") != std::string::npos);
        i = -1; CHECK(plan(spec, &i, &c, 1, mem, 0) == -1 && g_err.find("out of range") != std::string::npos);
        i = 0; c = 3;  CHECK(plan(spec, &i, &c, 1, mem, 0) == -1 && g_err.find("component") != std::string::npos);
        c = -1; CHECK(plan(spec, &i, &c, 1, mem, 0) == -1 && g_err.find("component") != std::string::npos);
        i = 1; c = 1;  CHECK(plan(spec, &i, &c, 1, mem, 0) == -1 && g_err.find("component") != std::string::npos);      // comp 1 of a grey image
        i = 0; c = 0;
        CHECK(plan(spec, nullptr, &c, 1, mem, 0) == -1 && g_err.find("images is NULL") != std::string::npos);
        CHECK(plan(spec, &i, nullptr, 1, mem, 0) == -1 && g_err.find("comps is NULL") != std::string::npos);
        CHECK(plan(spec, &i, &c, 1, nullptr, 0) == -1 && g_err.find("NULL") != std::string::npos);
        CHECK(plan(spec, &i, &c, 1, (const unsigned char*)mem + 2, 0) == -1 && g_err.find("multiple of 4") != std::string::npos);
        CHECK(plan(spec, &i, &c, 1, (const unsigned char*)mem + 1, 0) == -1);
        CHECK(plan(spec, &i, &c, 1, mem, js_chist_words(127) - 1) == -1 && g_err.find("row_pitch_words") != std::string::npos);
        CHECK(plan(spec, &i, &c, 1, mem, 1) == -1);
        CHECK(plan(spec, &i, &c, 1, mem, js_chist_words(127)) == 0 && plan(spec, &i, &c, 1, mem, js_chist_words(127) + 1) == 0);
        const int two[2] = { 0, 9 }, cc[2] = { 0, 0 };                         // the second entry bad: still -1
        CHECK(plan(spec, two, cc, 2, mem, 0) == -1);
        JsImage keep = imgs[1];
        imgs[1].mcu_xmax = 0; i = 1; CHECK(plan(spec, &i, &c, 1, mem, 0) == -1 && g_err.find("geometry") != std::string::npos);
        imgs[1] = keep; CHECK(plan(spec, &i, &c, 1, mem, 0) == 0);
    }
    // a prefix table whose unit count passes 2^32: 64-bit entries, nothing refused
    {
        imgs.push_back(image(1, 1, 1, 60000, 60000, 1ull << 33));             // 3 600 000 000 blocks: 56 250 000 units an entry
        std::vector<int> many(100, 4), cc(100, 0); std::vector<JsCoefHistRec> r; std::vector<uint64_t> b;
        CHECK(plan(spec, many.data(), cc.data(), 100, mem, 0, &r, &b) == 0);
        CHECK(b[100] == 100ull * 56250000ull && b[100] > (1ull << 32) && b[77] == 77ull * 56250000ull);
        CHECK(r[99].nblk == 3600000000u && r[99].coef_off == (1ull << 33));
        imgs.push_back(image(1, 1, 1, 65536, 65536, 0));                      // 2^32 blocks: one too many for a record
        int i = 5, c = 0;
        CHECK(plan(spec, &i, &c, 1, mem, 0) == -1 && g_err.find("2^32") != std::string::npos);
    }
    printf("ok\n");
    return 0;
}
