// Host-only program: the host arithmetic of jsnoop_encode_run (jpegsnoop_amd/csrc/jsnoop_encode_check.h) and the integer transform k_encode runs, which
// that header compiles for both sides -- every refusal of spec and source, the tables of every quality, records, geometry and the unit plan against a
// brute-force walk for the four layouts, edge sizes, the exhaustive proof of the quantiser's reciprocal, and the bounds the header states (pass 1 in int16,
// no int16 product wraps).  tests/test_encode_abi.py builds it with the address and undefined-behaviour sanitizers and runs it.  Prints "ok" and returns 0,
// or the line that failed.  `encode_check block q s0 .. s63` prints level * q of the 64 coefficients of one block of samples (natural order) under the
// multiplier q: the test compares them with tests/encode_model.py.
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
#include "../../jpegsnoop_amd/csrc/jsnoop_encode_check.h"

static std::string g_err;
void js_set_error(const char* fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)
#define REFUSED(call, word) do { g_err.clear(); CHECK((call) == -1); CHECK(g_err.find(word) != std::string::npos); } while (0)

// samples 0..255 [8 rows][8 columns] -> out[64]: 8 x the coefficients, natural order; *p1max: the largest |value| between the passes
static void fdct_block(const int* s, int* out, int* p1max)
{
    int t[8][8];
    for (int r = 0; r < 8; r++) {
        int d[8]; for (int c = 0; c < 8; c++) d[c] = s[r * 8 + c] - 128;
        js_enc_fdct_pass<true>(d);
        for (int c = 0; c < 8; c++) { t[r][c] = d[c]; if (abs(d[c]) > *p1max) *p1max = abs(d[c]); }
    }
    for (int c = 0; c < 8; c++) {
        int d[8]; for (int r = 0; r < 8; r++) d[r] = t[r][c];
        js_enc_fdct_pass<false>(d);
        for (int r = 0; r < 8; r++) out[r * 8 + c] = d[r];
    }
}

static JsnoopEncodeSrc source(uint32_t w, uint32_t h, uint32_t ch)
{
    JsnoopEncodeSrc s; memset(&s, 0, sizeof s);
    s.ptr = (const void*)(uintptr_t)0x10000; s.width = w; s.height = h; s.channels = ch;
    return s;
}

int main(int argc, char** argv)
{
    if (argc == 67 && !strcmp(argv[1], "block")) {
        const uint32_t q = (uint32_t)atoi(argv[2]); int s[64], o[64], p1 = 0;
        for (int k = 0; k < 64; k++) s[k] = atoi(argv[3 + k]);
        fdct_block(s, o, &p1);
        for (int k = 0; k < 64; k++) printf("%d ", js_enc_quant(o[k], q, js_enc_recip(q)));
        printf("\n");
        return 0;
    }
    // ---- spec: defaults, struct_size, every refusal
    JsnoopEncodeSpec d, got;
    memset(&d, 0xEE, sizeof d); js_encode_spec_defaults(&d);
    CHECK(d.struct_size == sizeof(JsnoopEncodeSpec) && d.quality == 75 && d.subsampling == JSNOOP_ENCODE_420 && d.reserved == 0 && d.qtables == nullptr);
    CHECK(js_encode_import_spec(&d, &got) == 0 && got.quality == 75);
    REFUSED(js_encode_import_spec(nullptr, &got), "spec is NULL");
    { JsnoopEncodeSpec s = d; s.struct_size = 3; REFUSED(js_encode_import_spec(&s, &got), "struct_size"); s.struct_size = sizeof s + 4; REFUSED(js_encode_import_spec(&s, &got), "struct_size"); }
    { JsnoopEncodeSpec s = d; s.quality = 33; s.struct_size = 8; s.subsampling = 77; CHECK(js_encode_import_spec(&s, &got) == 0 && got.quality == 33 && got.subsampling == JSNOOP_ENCODE_420); }   // a shorter struct: the rest at its defaults
    { JsnoopEncodeSpec s = d; s.quality = 0; REFUSED(js_encode_import_spec(&s, &got), "quality"); s.quality = 101; REFUSED(js_encode_import_spec(&s, &got), "quality"); }
    { JsnoopEncodeSpec s = d; s.subsampling = 3; REFUSED(js_encode_import_spec(&s, &got), "subsampling"); s.subsampling = -1; REFUSED(js_encode_import_spec(&s, &got), "subsampling"); }
    { JsnoopEncodeSpec s = d; s.reserved = 1; REFUSED(js_encode_import_spec(&s, &got), "reserved"); }
    {
        uint8_t t[128]; for (int k = 0; k < 128; k++) t[k] = (uint8_t)(1 + k);
        JsnoopEncodeSpec s = d; s.qtables = t; s.quality = 0;             // (quality is not read with tables)
        CHECK(js_encode_import_spec(&s, &got) == 0);
        uint8_t l[64], c[64]; js_encode_tables(got, l, c);
        CHECK(!memcmp(l, t, 64) && !memcmp(c, t + 64, 64));
        t[64 + 9] = 0; REFUSED(js_encode_import_spec(&s, &got), "entry 9 of the chroma table");
        t[64 + 9] = 1; t[0] = 0; REFUSED(js_encode_import_spec(&s, &got), "entry 0 of the luma table");
    }
    // ---- tables: every quality, against the formula written out once more; the ends of the range
    for (int q = 1; q <= 100; q++) {
        JsnoopEncodeSpec s = d; s.quality = q; uint8_t l[64], c[64];
        CHECK(js_encode_import_spec(&s, &got) == 0); js_encode_tables(got, l, c);
        const long scale = q < 50 ? 5000 / q : 200 - 2 * q;
        for (int k = 0; k < 64; k++) {
            long a = (kEncK1[k] * scale + 50) / 100, b = (kEncK2[k] * scale + 50) / 100;
            a = a < 1 ? 1 : a > 255 ? 255 : a; b = b < 1 ? 1 : b > 255 ? 255 : b;
            CHECK(l[k] == a && c[k] == b && l[k] >= 1 && c[k] >= 1);
        }
        if (q == 100) for (int k = 0; k < 64; k++) CHECK(l[k] == 1 && c[k] == 1);
        if (q == 50) CHECK(!memcmp(l, kEncK1, 64) && !memcmp(c, kEncK2, 64));
        if (q == 1) for (int k = 0; k < 64; k++) CHECK(l[k] == 255 && c[k] == 255);
    }
    // ---- sources: every refusal, the defaults of stride and pitches, the four address forms
    JsEncRec r;
    CHECK(js_encode_resolve_src(source(17, 9, 3), 0, JSNOOP_ENCODE_420, &r) == 0);
    CHECK(r.base[0] == 0x10000 && r.base[1] == 0x10001 && r.base[2] == 0x10002 && r.row_step == 51 && r.px_step == 3 && r.mcu_xmax == 2 && r.mcu_ymax == 1 && r.bpm == 6 && r.runs == 1 && r.sub == 2);
    { JsnoopEncodeSrc s = source(17, 9, 3); s.ptr = nullptr; REFUSED(js_encode_resolve_src(s, 4, 0, &r), "source 4: ptr is NULL"); }
    { JsnoopEncodeSrc s = source(17, 9, 3); s.reserved = 2; REFUSED(js_encode_resolve_src(s, 0, 0, &r), "reserved"); }
    { JsnoopEncodeSrc s = source(0, 9, 3); REFUSED(js_encode_resolve_src(s, 0, 0, &r), "1..65535"); s = source(9, 0, 3); REFUSED(js_encode_resolve_src(s, 0, 0, &r), "1..65535"); }
    { JsnoopEncodeSrc s = source(65536, 9, 3); REFUSED(js_encode_resolve_src(s, 0, 0, &r), "1..65535"); s = source(9, 65536, 3); REFUSED(js_encode_resolve_src(s, 0, 0, &r), "1..65535"); }
    for (uint32_t ch : { 0u, 2u, 4u }) REFUSED(js_encode_resolve_src(source(8, 8, ch), 0, 0, &r), "channels");
    { JsnoopEncodeSrc s = source(8, 8, 3); s.layout = 2; REFUSED(js_encode_resolve_src(s, 0, 0, &r), "layout"); s.layout = -1; REFUSED(js_encode_resolve_src(s, 0, 0, &r), "layout"); }
    { JsnoopEncodeSrc s = source(8, 8, 3); s.order = 2; REFUSED(js_encode_resolve_src(s, 0, 0, &r), "order"); }
    { JsnoopEncodeSrc s = source(8, 8, 3); s.bottom_up = 2; REFUSED(js_encode_resolve_src(s, 0, 0, &r), "bottom_up"); }
    { JsnoopEncodeSrc s = source(8, 8, 3); s.pixel_stride = 2; REFUSED(js_encode_resolve_src(s, 0, 0, &r), "pixel_stride"); }
    { JsnoopEncodeSrc s = source(8, 8, 3); s.row_pitch = 23; REFUSED(js_encode_resolve_src(s, 0, 0, &r), "row_pitch"); s.pixel_stride = 4; s.row_pitch = 31; REFUSED(js_encode_resolve_src(s, 0, 0, &r), "row_pitch"); }
    { JsnoopEncodeSrc s = source(8, 8, 3); s.row_pitch = (1ull << 40) + 1; REFUSED(js_encode_resolve_src(s, 0, 0, &r), "2^40"); }
    { JsnoopEncodeSrc s = source(8, 8, 3); s.layout = JSNOOP_ENCODE_PLANAR; s.row_pitch = 10; s.plane_pitch = 79; REFUSED(js_encode_resolve_src(s, 0, 0, &r), "plane_pitch"); }
    {   // a DIB: interleaved B, G, R, stride 4, bottom-up
        JsnoopEncodeSrc s = source(10, 6, 3); s.order = JSNOOP_ENCODE_BGR; s.pixel_stride = 4; s.bottom_up = 1;
        CHECK(js_encode_resolve_src(s, 0, JSNOOP_ENCODE_444, &r) == 0);
        CHECK(r.row_step == -40 && r.base[0] == 0x10000 + 5 * 40 + 2 && r.base[1] == 0x10000 + 5 * 40 + 1 && r.base[2] == 0x10000 + 5 * 40 && r.px_step == 4 && r.bpm == 3 && r.sub == 0);
    }
    {   // planar with pitches above the dense ones
        JsnoopEncodeSrc s = source(10, 6, 3); s.layout = JSNOOP_ENCODE_PLANAR; s.row_pitch = 16; s.plane_pitch = 100; s.order = JSNOOP_ENCODE_BGR;
        CHECK(js_encode_resolve_src(s, 0, JSNOOP_ENCODE_422, &r) == 0);
        CHECK(r.row_step == 16 && r.base[0] == 0x10000 + 200 && r.base[1] == 0x10000 + 100 && r.base[2] == 0x10000 && r.px_step == 1 && r.bpm == 4 && r.sub == 1);
        s.plane_pitch = 0; CHECK(js_encode_resolve_src(s, 0, 0, &r) == 0 && r.base[0] == 0x10000 + 2 * 96);
    }
    {   // grey ignores the subsampling and the order
        JsnoopEncodeSrc s = source(65535, 65535, 1); s.order = JSNOOP_ENCODE_BGR;
        CHECK(js_encode_resolve_src(s, 0, JSNOOP_ENCODE_420, &r) == 0);
        CHECK(r.sub == 0 && r.bpm == 1 && r.mcu_xmax == 8192 && r.mcu_ymax == 8192 && r.runs == 1024 && r.base[0] == 0x10000 && r.row_step == 65535);
    }
    // ---- geometry and the unit plan against a brute-force walk: four layouts, edge sizes, a mixed call
    {
        const uint32_t sizes[][2] = { { 1, 1 }, { 8, 8 }, { 17, 9 }, { 9, 17 }, { 33, 31 }, { 50, 70 }, { 130, 21 }, { 64, 48 }, { 127, 16 }, { 128, 16 }, { 129, 17 }, { 448, 33 }, { 65535, 3 }, { 3, 65535 } };
        std::vector<JsnoopEncodeSrc> src; std::vector<int> sub_of;
        for (int lay = 0; lay < 4; lay++) for (const auto& wh : sizes) {
            JsnoopEncodeSpec s = d; s.subsampling = lay == 0 ? 0 : lay - 1;
            const JsnoopEncodeSrc one = source(wh[0], wh[1], lay == 0 ? 1 : 3);
            JsEncRec rec; uint32_t ub[2]; uint64_t blocks = 0;
            CHECK(js_encode_plan(s, &one, 1, &rec, ub, &blocks) == 0);
            const uint32_t H = lay >= 2 ? 2 : 1, V = lay == 3 ? 2 : 1, mx = (wh[0] + 8 * H - 1) / (8 * H), my = (wh[1] + 8 * V - 1) / (8 * V), bpm = lay == 0 ? 1 : H * V + 2;
            CHECK(rec.mcu_xmax == mx && rec.mcu_ymax == my && rec.bpm == bpm && blocks == (uint64_t)mx * my * bpm && ub[0] == 0);
            // every MCU lies in exactly one unit; units follow each other in decode order, straddle no MCU row and hold at most JS_ENC_RUN MCUs
            uint64_t next = 0;
            for (uint32_t u = 0; u < ub[1]; u++) {
                const uint32_t row = u / rec.runs, m0 = (u - row * rec.runs) * JS_ENC_RUN;
                CHECK(row < my && m0 < mx);
                const uint32_t nm = mx - m0 < JS_ENC_RUN ? mx - m0 : JS_ENC_RUN;
                CHECK((uint64_t)row * mx + m0 == next && nm >= 1);
                next += nm;
            }
            CHECK(next == (uint64_t)mx * my);
            JsImage im; js_encode_describe(rec, &im);
            CHECK(im.dim_x == wh[0] && im.dim_y == wh[1] && im.blk_per_mcu == bpm && im.total_blocks == blocks && im.mcu_w == 8 * H && im.mcu_h == 8 * V && im.precision == 8);
            CHECK(im.samp_h[1] == (lay ? H : 1) && im.samp_v[1] == (lay ? V : 1) && im.img_x == mx * 8 * H && im.blk_ymax == my * V);
            uint32_t j = 0;
            for (uint32_t c = 1; c <= im.ncomp; c++) for (uint32_t y = 0; y < im.samp_v[c]; y++) for (uint32_t x = 0; x < im.samp_h[c]; x++, j++)
                CHECK(im.blk_comp[j] == c && im.blk_ch[j] == x && im.blk_cv[j] == y);
            CHECK(j == bpm);
            CHECK(js_enc_coded(wh[0], H, H) == (wh[0] + 7) / 8 && js_enc_coded(wh[0], 1, H) == ((wh[0] + H - 1) / H + 7) / 8 && js_enc_coded(wh[0], 1, H) == mx);   // chroma has no dummy block
            src.push_back(one); sub_of.push_back(lay);
        }
        // the mixed call: prefix sums of units and blocks over all of them (one subsampling: the three-channel ones at 4:2:0)
        std::vector<JsEncRec> recs(src.size()); std::vector<uint32_t> ub(src.size() + 1); uint64_t blocks = 0, want_blocks = 0, want_units = 0;
        JsnoopEncodeSpec s = d;
        CHECK(js_encode_plan(s, src.data(), (int)src.size(), recs.data(), ub.data(), &blocks) == 0);
        for (size_t k = 0; k < src.size(); k++) {
            CHECK(recs[k].coef_off == want_blocks && ub[k] == want_units);
            want_blocks += (uint64_t)recs[k].mcu_xmax * recs[k].mcu_ymax * recs[k].bpm; want_units += (uint64_t)recs[k].mcu_ymax * recs[k].runs;
        }
        CHECK(blocks == want_blocks && ub[src.size()] == want_units);
        src[3].channels = 2; REFUSED(js_encode_plan(s, src.data(), (int)src.size(), recs.data(), ub.data(), &blocks), "source 3");
        // 2^31 units: 65535 x 65535 grey pictures of 8192 x 1024 units each
        std::vector<JsnoopEncodeSrc> big(257, source(65535, 65535, 1)); std::vector<JsEncRec> brecs(big.size()); std::vector<uint32_t> bub(big.size() + 1);
        REFUSED(js_encode_plan(s, big.data(), (int)big.size(), brecs.data(), bub.data(), &blocks), "2^31 units");
        CHECK(js_encode_plan(s, big.data(), 255, brecs.data(), bub.data(), &blocks) == 0 && blocks == 255ull * 8192 * 8192);
    }
    // ---- the reciprocal: every q against every numerator below JS_ENC_NUM_MAX, and the quantiser's rounding on both signs
    for (uint32_t q = 1; q <= 255; q++) {
        const uint32_t m = js_enc_recip(q), dv = 8 * q;
        for (uint32_t n = 0; n < JS_ENC_NUM_MAX; n++) if ((uint32_t)(((uint64_t)n * m) >> 32) != n / dv) { printf("FAILED reciprocal q %u n %u\n", q, n); return 1; }
        for (int c : { 0, 1, (int)(4 * q) - 1, (int)(4 * q), (int)(12 * q) - 1, (int)(12 * q), JS_ENC_COEF_MAX }) {
            const int lv = (int)((c + 4 * q) / (8 * q));
            CHECK(js_enc_quant(c, q, m) == lv * (int)q && js_enc_quant(-c, q, m) == -lv * (int)q);
        }
        CHECK(JS_ENC_COEF_MAX + 4 * q < JS_ENC_NUM_MAX && (JS_ENC_COEF_MAX + 4 * q) / 8 <= JS_ENC_PROD_MAX);
    }
    // ---- bounds: pass 1 over every corner of a row of samples; both passes and the products on extreme blocks
    {
        int p1 = 0;
        for (int k = 0; k < 256; k++) { int v[8]; for (int i = 0; i < 8; i++) v[i] = (k >> i & 1) ? 127 : -128; js_enc_fdct_pass<true>(v); for (int i = 0; i < 8; i++) if (abs(v[i]) > p1) p1 = abs(v[i]); }
        CHECK(p1 <= JS_ENC_PASS1_MAX && JS_ENC_PASS1_MAX < 32768);
        int cmax = 0, s[64], o[64];
        for (int pat = 0; pat < 64 + 6; pat++) {
            for (int k = 0; k < 64; k++) {
                const int x = k & 7, y = k >> 3;
                if (pat < 64) { const int u = pat & 7, v = pat >> 3; s[k] = ((((2 * x + 1) * u) % 32 < 16) != (((2 * y + 1) * v) % 32 < 16)) ? 0 : 255; }   // the sign pattern of basis function (u, v)
                else s[k] = pat == 64 ? 0 : pat == 65 ? 255 : pat == 66 ? ((x + y) & 1) * 255 : pat == 67 ? (x & 1) * 255 : pat == 68 ? (y & 1) * 255 : ((x >> 1) & 1) * 255;
            }
            fdct_block(s, o, &p1);
            for (int k = 0; k < 64; k++) { if (abs(o[k]) > cmax) cmax = abs(o[k]); for (uint32_t q : { 1u, 2u, 255u }) CHECK(abs(js_enc_quant(o[k], q, js_enc_recip(q))) <= JS_ENC_PROD_MAX); }
        }
        CHECK(p1 <= JS_ENC_PASS1_MAX && cmax <= JS_ENC_COEF_MAX && cmax >= 8 * 1016);
        int y, cb, cr;
        js_enc_ycc(0, 0, 0, &y, &cb, &cr); CHECK(y == 0 && cb == 128 && cr == 128);
        js_enc_ycc(255, 255, 255, &y, &cb, &cr); CHECK(y == 255 && cb == 128 && cr == 128);
        js_enc_ycc(255, 0, 0, &y, &cb, &cr); CHECK(y == 76 && cb == 85 && cr == 255);
        js_enc_ycc(0, 0, 255, &y, &cb, &cr); CHECK(y == 29 && cb == 255 && cr == 107);
        for (int rr = 0; rr < 256; rr += 5) for (int gg = 0; gg < 256; gg += 3) for (int bb = 0; bb < 256; bb += 7) { js_enc_ycc(rr, gg, bb, &y, &cb, &cr); CHECK(y >= 0 && y <= 255 && cb >= 0 && cb <= 255 && cr >= 0 && cr <= 255); }
    }
    // ---- struct sizes the records are copied with
    CHECK(sizeof(JsEncRec) == 80 && sizeof(JsEncTabs) == 768 && sizeof(JsnoopEncodeSpec) == 24 && sizeof(JsnoopEncodeSrc) == 56);
    printf("ok\n");
    return 0;
}
