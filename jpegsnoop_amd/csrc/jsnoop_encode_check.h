// jsnoop_encode_check.h -- the arithmetic of jsnoop_encode_run that is not a device call: spec import, the tables a quality comes to, the checks of a source,
// geometry, records and the unit plan -- and the integer kernels of the transform itself (colour, one jfdctint pass, the quantiser), compiled for host AND
// device: k_encode (jsnoop_encode.hip) calls the very functions tests/cpp/encode_check.cpp runs as a plain host program.  Errors go through js_set_error.
//
// Bounds (tests/cpp/encode_check.cpp proves the ones marked *):
//   samples are 0..255, level-shifted -128..127.
//   pass 1 (rows) leaves |value| <= JS_ENC_PASS1_MAX = 5793 *(every corner of the sample cube; the pass is linear up to its rounding) -- int16 holds it.
//   pass 2 leaves 8 x the coefficient: |c| <= 8 * 1024 + 8 = JS_ENC_COEF_MAX (an orthonormal 8 x 8 basis function has absolute sum <= 8, samples |s| <= 128; the
//   two roundings add less than 8).
//   quantiser: n = |c| + 4 q <= 8200 + 1020 < 2^17, level = n / (8 q) = mulhi32(n, js_enc_recip(q)) *(every q 1..255 against every n below 2^17).
//   products: |level * q| <= (|c| + 4 q) / 8 <= 1025 + 127 = 1152 < 1154 *(re-stated on extreme blocks): no int16 value of the arena or of dccum wraps.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_types.h"

#if defined(__HIPCC__)
#define JS_ENC_HD __host__ __device__ __forceinline__
#else
#define JS_ENC_HD inline
#endif

void js_set_error(const char* fmt, ...);

static_assert(JS_ENC_RUN == JSNOOP_ENCODE_RUN, "the public seam constant is the kernel's");
#define JS_ENC_PASS1_MAX 5793
#define JS_ENC_COEF_MAX  8200
#define JS_ENC_NUM_MAX   (1u << 17)      /* the quantiser's numerators stay below this */
#define JS_ENC_PROD_MAX  1153

// ---------------------------------------------------------------------------------------------- the transform (host and device)
// R, G, B 0..255 -> Y, Cb, Cr 0..255 (libjpeg's rgb_ycc tables, SCALEBITS 16; >> is arithmetic, every sum here is non-negative)
JS_ENC_HD void js_enc_ycc(int r, int g, int b, int* y, int* cb, int* cr)
{
    *y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    *cb = (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
    *cr = (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
}
JS_ENC_HD int js_enc_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// One 1-D pass of jfdctint (CONST_BITS 13, PASS1_BITS 2) over d[0..7], in place.  FIRST: the row pass (outputs 0 and 4 shifted left by 2, the others descaled by
// 11); else the column pass (0 and 4 descaled by 2, the others by 15).
template <bool FIRST>
JS_ENC_HD void js_enc_fdct_pass(int d[8])
{
    const int n = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6], t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) { d[0] = (t10 + t11) * 4; d[4] = (t10 - t11) * 4; }
    else { d[0] = js_enc_descale(t10 + t11, 2); d[4] = js_enc_descale(t10 - t11, 2); }
    int z1 = (t12 + t13) * 4433;
    d[2] = js_enc_descale(z1 + t13 * 6270, n); d[6] = js_enc_descale(z1 - t12 * 15137, n);
    z1 = t4 + t7; int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7; const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    d[7] = js_enc_descale(a4 + z1 + z3, n); d[5] = js_enc_descale(a5 + z2 + z4, n); d[3] = js_enc_descale(a6 + z2 + z3, n); d[1] = js_enc_descale(a7 + z1 + z4, n);
}
// ceil(2^32 / (8 q)): floor(n * recip / 2^32) = n / (8 q) for every n < JS_ENC_NUM_MAX (e = recip * 8 q - 2^32 < 8 q, so n * e < 2^17 * 2^11 < 2^32)
JS_ENC_HD uint32_t js_enc_recip(uint32_t q) { return (uint32_t)(((1ull << 32) + 8u * q - 1u) / (8u * q)); }
// c = 8 x the coefficient -> level * q (what the arena holds): level = sign(c) * ((|c| + 4 q) / (8 q))
JS_ENC_HD int js_enc_quant(int c, uint32_t q, uint32_t recip)
{
    const uint32_t n = (uint32_t)(c < 0 ? -c : c) + 4u * q;
    const int p = (int)((uint32_t)(((uint64_t)n * recip) >> 32) * q);
    return c < 0 ? -p : p;
}

// ---------------------------------------------------------------------------------------------- spec and tables (host)
// ITU-T T.81 Annex K, Tables K.1 and K.2, natural order
static const uint8_t kEncK1[64] = { 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 };
static const uint8_t kEncK2[64] = { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 };

inline void js_encode_spec_defaults(JsnoopEncodeSpec* s) { memset(s, 0, sizeof *s); s->struct_size = (uint32_t)sizeof *s; s->quality = 75; s->subsampling = JSNOOP_ENCODE_420; }
// struct_size is the caller's sizeof(JsnoopEncodeSpec), read like JsnoopPackSpec's: a shorter struct leaves the fields it lacks at their defaults, a longer one is refused
inline int js_encode_import_spec(const JsnoopEncodeSpec* in, JsnoopEncodeSpec* out)
{
    if (!in) { js_set_error("encode: spec is NULL"); return -1; }
    const uint32_t sz = in->struct_size;
    if (sz < sizeof(uint32_t) || sz > sizeof(JsnoopEncodeSpec)) { js_set_error("encode: struct_size %u, this library has %zu", sz, sizeof(JsnoopEncodeSpec)); return -1; }
    js_encode_spec_defaults(out); memcpy(out, in, sz); out->struct_size = (uint32_t)sizeof(JsnoopEncodeSpec);
    if (out->reserved) { js_set_error("encode: reserved is %u, not 0", out->reserved); return -1; }
    if (out->subsampling < JSNOOP_ENCODE_444 || out->subsampling > JSNOOP_ENCODE_420) { js_set_error("encode: subsampling %d is none of 4:4:4 (0), 4:2:2 (1), 4:2:0 (2)", out->subsampling); return -1; }
    if (!out->qtables && (out->quality < 1 || out->quality > 100)) { js_set_error("encode: quality %d outside 1..100", out->quality); return -1; }
    if (out->qtables) for (int k = 0; k < 128; k++) if (!out->qtables[k]) { js_set_error("encode: entry %d of the %s table is 0", k & 63, k < 64 ? "luma" : "chroma"); return -1; }
    return 0;
}
// the tables of an imported spec, natural order
inline void js_encode_tables(const JsnoopEncodeSpec& s, uint8_t luma[64], uint8_t chroma[64])
{
    if (s.qtables) { memcpy(luma, s.qtables, 64); memcpy(chroma, s.qtables + 64, 64); return; }
    const int scale = s.quality < 50 ? 5000 / s.quality : 200 - 2 * s.quality;
    for (int k = 0; k < 64; k++) {
        const int a = (kEncK1[k] * scale + 50) / 100, b = (kEncK2[k] * scale + 50) / 100;
        luma[k] = (uint8_t)(a < 1 ? 1 : (a > 255 ? 255 : a)); chroma[k] = (uint8_t)(b < 1 ? 1 : (b > 255 ? 255 : b));
    }
}
inline void js_encode_fill_tabs(const uint8_t luma[64], const uint8_t chroma[64], JsEncTabs* t)
{
    for (int k = 0; k < 64; k++) { t->q[0][k] = luma[k]; t->q[1][k] = chroma[k]; t->recip[0][k] = js_enc_recip(luma[k]); t->recip[1][k] = js_enc_recip(chroma[k]); }
}

// ---------------------------------------------------------------------------------------------- sources, geometry, plan (host)
// One source checked and resolved into its record (coef_off left to the plan).  0, or -1 + error text.
inline int js_encode_resolve_src(const JsnoopEncodeSrc& s, int k, int subsampling, JsEncRec* r)
{
    if (!s.ptr) { js_set_error("encode: source %d: ptr is NULL", k); return -1; }
    if (s.reserved) { js_set_error("encode: source %d: reserved is %u, not 0", k, s.reserved); return -1; }
    if (s.width < 1u || s.width > 65535u || s.height < 1u || s.height > 65535u) { js_set_error("encode: source %d: %u x %u, each side must be 1..65535", k, s.width, s.height); return -1; }
    if (s.channels != 1u && s.channels != 3u) { js_set_error("encode: source %d: %u channels, 1 or 3 are encoded", k, s.channels); return -1; }
    if (s.layout != JSNOOP_ENCODE_INTERLEAVED && s.layout != JSNOOP_ENCODE_PLANAR) { js_set_error("encode: source %d: unknown layout %d", k, s.layout); return -1; }
    if (s.order != JSNOOP_ENCODE_RGB && s.order != JSNOOP_ENCODE_BGR) { js_set_error("encode: source %d: unknown channel order %d", k, s.order); return -1; }
    if (s.bottom_up > 1u) { js_set_error("encode: source %d: bottom_up is %u, not 0 or 1", k, s.bottom_up); return -1; }
    const bool planar = s.layout == JSNOOP_ENCODE_PLANAR;
    const uint32_t least = planar ? 1u : s.channels, px = s.pixel_stride ? s.pixel_stride : least;
    if (px < least) { js_set_error("encode: source %d: pixel_stride %u is below %u", k, px, least); return -1; }
    const uint64_t dense_row = (uint64_t)s.width * px, row = s.row_pitch ? s.row_pitch : dense_row;
    if (row < dense_row) { js_set_error("encode: source %d: row_pitch %llu is below the row's %llu bytes", k, (unsigned long long)row, (unsigned long long)dense_row); return -1; }
    if (row > (1ull << 40)) { js_set_error("encode: source %d: row_pitch %llu is beyond 2^40", k, (unsigned long long)row); return -1; }
    const uint64_t dense_plane = (uint64_t)s.height * row, plane = s.plane_pitch ? s.plane_pitch : dense_plane;
    if (planar && s.channels == 3u && plane < dense_plane) { js_set_error("encode: source %d: plane_pitch %llu is below the plane's %llu bytes", k, (unsigned long long)plane, (unsigned long long)dense_plane); return -1; }
    memset(r, 0, sizeof *r);
    const uint64_t p0 = (uint64_t)(uintptr_t)s.ptr + (s.bottom_up ? (uint64_t)(s.height - 1u) * row : 0u);
    for (uint32_t c = 0; c < s.channels; c++) {
        const uint32_t cc = s.channels == 3u && s.order == JSNOOP_ENCODE_BGR ? 2u - c : c;
        r->base[c] = p0 + (planar ? (uint64_t)cc * plane : (uint64_t)cc);
    }
    r->row_step = s.bottom_up ? -(int64_t)row : (int64_t)row;
    r->px_step = px; r->width = s.width; r->height = s.height; r->ncomp = s.channels; r->sub = s.channels == 1u ? 0u : (uint32_t)subsampling;
    const uint32_t mw = r->sub ? 16u : 8u, mh = r->sub == 2u ? 16u : 8u;
    r->mcu_xmax = (s.width + mw - 1u) / mw; r->mcu_ymax = (s.height + mh - 1u) / mh;
    r->runs = (r->mcu_xmax + JS_ENC_RUN - 1u) / JS_ENC_RUN;
    r->bpm = s.channels == 1u ? 1u : (r->sub == 0u ? 3u : (r->sub == 1u ? 4u : 6u));
    return 0;
}
// The image descriptor the export reads for a record: frame, geometry and block order of a decode of the same file (js_geometry), no stream, no preview state.
inline void js_encode_describe(const JsEncRec& r, JsImage* im)
{
    memset(im, 0, sizeof *im);
    const uint32_t hmax = r.sub ? 2u : 1u, vmax = r.sub == 2u ? 2u : 1u;
    im->dim_x = r.width; im->dim_y = r.height; im->ncomp = r.ncomp; im->precision = 8; im->decode_ac = 1;
    im->mcu_w = hmax * 8u; im->mcu_h = vmax * 8u; im->mcu_xmax = r.mcu_xmax; im->mcu_ymax = r.mcu_ymax;
    im->blk_xmax = r.mcu_xmax * hmax; im->blk_ymax = r.mcu_ymax * vmax; im->img_x = r.mcu_xmax * im->mcu_w; im->img_y = r.mcu_ymax * im->mcu_h;
    uint32_t nb = 0;
    for (uint32_t c = 1; c <= r.ncomp; c++) {
        const uint32_t h = c == 1u ? hmax : 1u, v = c == 1u ? vmax : 1u;
        im->samp_h[c] = h; im->samp_v[c] = v; im->expand_h[c] = hmax / h; im->expand_v[c] = vmax / v;
        for (uint32_t y = 0; y < v; y++) for (uint32_t x = 0; x < h; x++) { im->blk_comp[nb] = (uint8_t)c; im->blk_ch[nb] = (uint8_t)x; im->blk_cv[nb] = (uint8_t)y; nb++; }
    }
    im->blk_per_mcu = nb; im->total_blocks = r.mcu_xmax * r.mcu_ymax * nb; im->coef_off = r.coef_off; im->preview_mode = 1;
}
// Checks every source of one call and fills recs[n] and unit_base[n + 1]; *total_blocks: the arena rows of the call.  0, or -1 + error text.
inline int js_encode_plan(const JsnoopEncodeSpec& spec, const JsnoopEncodeSrc* src, int n, JsEncRec* recs, uint32_t* unit_base, uint64_t* total_blocks)
{
    uint64_t units = 0, blocks = 0;
    for (int k = 0; k < n; k++) {
        if (js_encode_resolve_src(src[k], k, spec.subsampling, &recs[k])) return -1;
        recs[k].coef_off = blocks; unit_base[k] = (uint32_t)units;
        units += (uint64_t)recs[k].mcu_ymax * recs[k].runs; blocks += (uint64_t)recs[k].mcu_xmax * recs[k].mcu_ymax * recs[k].bpm;
        if (units >= 0x7FFFFFFFull) { js_set_error("encode: more than 2^31 units of work in one call"); return -1; }
    }
    unit_base[n] = (uint32_t)units; *total_blocks = blocks;
    return 0;
}
// the component's coded part in blocks (T.81 A.2.3): a block of the MCU-padded grid at or beyond it is a dummy block
JS_ENC_HD uint32_t js_enc_coded(uint32_t dim, uint32_t samp, uint32_t smax) { return ((dim * samp + smax - 1u) / smax + 7u) / 8u; }
