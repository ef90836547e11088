// jsnoop_transform_check.h -- the arithmetic of jsnoop_transform_run that is not a device call: spec import, what an op comes to, the geometry of an entry
// (grayscale, crop, edge), its record and destination descriptor, the plan of a call -- and the block map itself, compiled for host AND device: k_transform
// (jsnoop_transform.hip) calls the very js_xf_map that tests/cpp/transform_check.cpp walks against brute force as a plain host program.  DESIGN.md section 4.19
// is the contract, tests/transform_model.py its definition.  Errors go through js_set_error.
//
// Divisions.  The map divides by four numbers that are fixed per entry (blocks per destination MCU, destination MCUs per row, gsh, gsv).  The host turns each
// into a multiply-high word (js_xf_magic): for a divisor d >= 2 with s = ceil(log2 d), mul = ceil(2^(31 + s) / d) lies in [2^31, 2^32) and
// floor(x * mul / 2^(31 + s)) = x / d for every x < 2^31: e = mul * d - 2^(31 + s) < d <= 2^s, so x * e < 2^(31 + s).  Every dividend of the map is a block
// count or a block coordinate of one call, below 2^31 by the plan's check.  transform_check.cpp holds the words against plain division.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_types.h"

#if defined(__HIPCC__)
#define JS_XF_HD __host__ __device__ __forceinline__
#else
#define JS_XF_HD inline
#endif

void js_set_error(const char* fmt, ...);

static_assert(JS_XF_RUN == JSNOOP_TRANSFORM_RUN, "the public seam constant is the kernel's");

// ---------------------------------------------------------------------------------------------- the block map (host and device)
JS_XF_HD uint32_t js_xf_div(uint32_t x, const JsXfDiv& d) { return d.mul ? (uint32_t)(((uint64_t)x * d.mul) >> 32) >> d.shift : x; }
// Destination block j of the entry (decode order of the new geometry) -> its source block, counted from the source image's first block.  Everything but j and
// the table entry is uniform over a wave that works on one entry.
JS_XF_HD uint64_t js_xf_map(const JsXfRec& r, uint32_t flags, uint32_t j)
{
    const uint32_t m = js_xf_div(j, r.m_bpm), kb = j - m * r.d_bpm;                  // destination MCU, block inside it
    const uint32_t dmy = js_xf_div(m, r.m_mcu_x), dmx = m - dmy * r.d_mcu_x;
    const uint32_t a = flags & JS_XF_T ? dmy : dmx, b = flags & JS_XF_T ? dmx : dmy;
    const uint32_t sx = (flags & JS_XF_REVX ? r.rw - 1u - a : a) + r.ox, sy = (flags & JS_XF_REVY ? r.rh - 1u - b : b) + r.oy;   // the working MCU it comes from
    const uint32_t mx = js_xf_div(sx, r.m_gsh), my = js_xf_div(sy, r.m_gsv);          // ... which lies in this MCU of the source
    return ((uint64_t)my * r.s_mcu_x + mx) * r.s_bpm + (sy - my * r.gsv) * r.gsh + (sx - mx * r.gsh) + r.tab[kb];
}

// ---------------------------------------------------------------------------------------------- spec, geometry, plan (host)
inline JsXfDiv js_xf_magic(uint32_t d)
{
    JsXfDiv m = { 0u, 0u };
    if (d < 2u) return m;
    uint32_t s = 0; while ((1u << s) < d) s++;
    m.mul = (uint32_t)(((1ull << (31u + s)) + d - 1u) / d); m.shift = s - 1u;
    return m;
}
// what an op comes to: JS_XF_* bits, or -1 for an unknown op
inline int js_xf_flags(int op)
{
    switch (op) {
    case JSNOOP_XFORM_NONE:       return 0;
    case JSNOOP_XFORM_FLIP_H:     return JS_XF_REVX | JS_XF_NEGU;
    case JSNOOP_XFORM_FLIP_V:     return JS_XF_REVY | JS_XF_NEGV;
    case JSNOOP_XFORM_TRANSPOSE:  return JS_XF_T;
    case JSNOOP_XFORM_TRANSVERSE: return JS_XF_T | JS_XF_REVX | JS_XF_REVY | JS_XF_NEGU | JS_XF_NEGV;
    case JSNOOP_XFORM_ROT_90:     return JS_XF_T | JS_XF_REVY | JS_XF_NEGU;
    case JSNOOP_XFORM_ROT_180:    return JS_XF_REVX | JS_XF_REVY | JS_XF_NEGU | JS_XF_NEGV;
    case JSNOOP_XFORM_ROT_270:    return JS_XF_T | JS_XF_REVX | JS_XF_NEGV;
    }
    return -1;
}
inline void js_transform_spec_defaults(JsnoopTransformSpec* s) { memset(s, 0, sizeof *s); s->struct_size = (uint32_t)sizeof *s; }
// struct_size is the caller's sizeof(JsnoopTransformSpec), read like JsnoopPackSpec's: a shorter struct leaves the fields it lacks at their defaults, a longer one is refused
inline int js_transform_import_spec(const JsnoopTransformSpec* in, JsnoopTransformSpec* out)
{
    if (!in) { js_set_error("transform: spec is NULL"); return -1; }
    const uint32_t sz = in->struct_size;
    if (sz < sizeof(uint32_t) || sz > sizeof(JsnoopTransformSpec)) { js_set_error("transform: struct_size %u, this library has %zu", sz, sizeof(JsnoopTransformSpec)); return -1; }
    js_transform_spec_defaults(out); memcpy(out, in, sz); out->struct_size = (uint32_t)sizeof(JsnoopTransformSpec);
    if (out->reserved) { js_set_error("transform: reserved is %u, not 0", out->reserved); return -1; }
    if (js_xf_flags(out->op) < 0) { js_set_error("transform: unknown op %d", out->op); return -1; }
    if (out->edge != JSNOOP_XFORM_EDGE_TRIM && out->edge != JSNOOP_XFORM_EDGE_PERFECT) { js_set_error("transform: unknown edge mode %d", out->edge); return -1; }
    if (out->grayscale > 1u) { js_set_error("transform: grayscale is %u, not 0 or 1", out->grayscale); return -1; }
    if (out->crop > 1u) { js_set_error("transform: crop is %u, not 0 or 1", out->crop); return -1; }
    if (!out->crop && (out->crop_x | out->crop_y | out->crop_w | out->crop_h)) { js_set_error("transform: crop fields are set while crop is 0"); return -1; }
    if (out->crop && (!out->crop_w || !out->crop_h)) { js_set_error("transform: crop size %u x %u, each side must be at least 1", out->crop_w, out->crop_h); return -1; }
    return 0;
}

// One entry: source descriptor + imported spec -> result word; for JSNOOP_XFORM_OK the record (src_off set, dst_off left to the plan) and the destination's
// descriptor (coef_off and tableset left to the caller).  region4: x0, y0, width, height of what is kept, in source pixels (filled where the result is OK).
inline int js_xf_entry(const JsImage& im, const JsnoopTransformSpec& s, JsXfRec* r, JsImage* out, uint32_t* region4)
{
    if (im.ncomp != 1u && im.ncomp != 3u) return JSNOOP_XFORM_UNSUPPORTED;
    uint32_t sH[3] = { 1, 1, 1 }, sV[3] = { 1, 1, 1 }, sfirst[3] = { 0, 0, 0 }, bpm = 0;
    for (uint32_t c = 0; c < im.ncomp; c++) {
        if (im.ncomp == 3u) { sH[c] = im.samp_h[c + 1]; sV[c] = im.samp_v[c + 1]; }
        if (sH[c] < 1u || sH[c] > 4u || sV[c] < 1u || sV[c] > 4u) return JSNOOP_XFORM_UNSUPPORTED;
        sfirst[c] = bpm; bpm += sH[c] * sV[c];
    }
    if (bpm != im.blk_per_mcu || !im.mcu_xmax || !im.mcu_ymax || !im.dim_x || !im.dim_y) return JSNOOP_XFORM_UNSUPPORTED;
    const int flags = js_xf_flags(s.op);
    // 1. grayscale: the working layout, in the source's orientation
    const uint32_t nc = s.grayscale ? 1u : im.ncomp;
    uint32_t wH[3] = { 1, 1, 1 }, wV[3] = { 1, 1, 1 }, hmax = 1, vmax = 1;
    for (uint32_t c = 0; c < nc && nc == 3u; c++) { wH[c] = sH[c]; wV[c] = sV[c]; if (wH[c] > hmax) hmax = wH[c]; if (wV[c] > vmax) vmax = wV[c]; }
    const uint32_t mw = 8u * hmax, mh = 8u * vmax;
    // 2. crop
    uint32_t x0 = 0, y0 = 0, w = im.dim_x, h = im.dim_y;
    if (s.crop) {
        if (s.crop_x >= im.dim_x || s.crop_y >= im.dim_y) return JSNOOP_XFORM_EMPTY;
        x0 = s.crop_x - s.crop_x % mw; y0 = s.crop_y - s.crop_y % mh;
        const uint64_t gw = (uint64_t)s.crop_w + (s.crop_x - x0), gh = (uint64_t)s.crop_h + (s.crop_y - y0);
        w = gw < im.dim_x - x0 ? (uint32_t)gw : im.dim_x - x0; h = gh < im.dim_y - y0 ? (uint32_t)gh : im.dim_y - y0;
    }
    // 3. edge
    const bool revx = flags & JS_XF_REVX, revy = flags & JS_XF_REVY;
    if ((revx && w % mw) || (revy && h % mh)) {
        if (s.edge == JSNOOP_XFORM_EDGE_PERFECT) return JSNOOP_XFORM_IMPERFECT;
        if (revx) w -= w % mw;
        if (revy) h -= h % mh;
        if (!w || !h) return JSNOOP_XFORM_EMPTY;
    }
    const uint32_t rw = (w + mw - 1u) / mw, rh = (h + mh - 1u) / mh;       // the region in MCUs (exact on a reversed axis)
    if (region4) { region4[0] = x0; region4[1] = y0; region4[2] = w; region4[3] = h; }
    // 4. record and destination
    const bool T = flags & JS_XF_T, gray = nc == 1u && im.ncomp == 3u;
    memset(r, 0, sizeof *r); memset(out, 0, sizeof *out);
    r->src_off = im.coef_off; r->s_mcu_x = im.mcu_xmax; r->s_bpm = im.blk_per_mcu;
    r->rw = rw; r->rh = rh; r->ox = x0 / mw; r->oy = y0 / mh; r->gsh = gray ? sH[0] : 1u; r->gsv = gray ? sV[0] : 1u;
    r->d_mcu_x = T ? rh : rw; const uint32_t d_mcu_y = T ? rw : rh;
    uint32_t nb = 0;
    for (uint32_t c = 0; c < nc; c++) {
        const uint32_t dh = T ? wV[c] : wH[c], dv = T ? wH[c] : wV[c];
        out->samp_h[c + 1] = dh; out->samp_v[c + 1] = dv;
        for (uint32_t y = 0; y < dv; y++) for (uint32_t x = 0; x < dh; x++) {
            const uint32_t a = T ? y : x, b = T ? x : y, hs = revx ? wH[c] - 1u - a : a, vs = revy ? wV[c] - 1u - b : b;      // the block of the source's MCU
            r->tab[nb] = (uint8_t)(gray ? 0u : sfirst[c] + vs * sH[c] + hs);
            out->blk_comp[nb] = (uint8_t)(c + 1u); out->blk_ch[nb] = (uint8_t)x; out->blk_cv[nb] = (uint8_t)y; nb++;
        }
    }
    r->d_bpm = nb; r->m_bpm = js_xf_magic(nb); r->m_mcu_x = js_xf_magic(r->d_mcu_x); r->m_gsh = js_xf_magic(r->gsh); r->m_gsv = js_xf_magic(r->gsv);
    const uint64_t nblk = (uint64_t)r->d_mcu_x * d_mcu_y * nb;             // (at most 8192 x 8192 MCUs of 48 blocks: the plan holds the call below 2^31)
    r->nblk = nblk < 0x80000000ull ? (uint32_t)nblk : 0x80000000u;
    const uint32_t dhmax = T ? vmax : hmax, dvmax = T ? hmax : vmax;
    out->dim_x = T ? h : w; out->dim_y = T ? w : h; out->ncomp = nc; out->precision = im.precision; out->decode_ac = 1; out->preview_mode = 1;
    out->mcu_w = 8u * dhmax; out->mcu_h = 8u * dvmax; out->mcu_xmax = r->d_mcu_x; out->mcu_ymax = d_mcu_y;
    out->blk_xmax = out->mcu_xmax * dhmax; out->blk_ymax = out->mcu_ymax * dvmax; out->img_x = out->mcu_xmax * out->mcu_w; out->img_y = out->mcu_ymax * out->mcu_h;
    for (uint32_t c = 1; c <= nc; c++) { out->expand_h[c] = dhmax / out->samp_h[c]; out->expand_v[c] = dvmax / out->samp_v[c]; }
    out->blk_per_mcu = nb; out->total_blocks = r->nblk;
    return JSNOOP_XFORM_OK;
}

// The plan of one call: every listed image through js_xf_entry.  results[n]: the result words; image_of[n]: the entry's image in the object, -1 where it has
// none; recs / descs / unit_base: one per WRITTEN entry (unit_base one more), in the order of the call; *nout their number, *total_blocks the arena rows of the
// call.  The index list is checked before anything else.  0, or -1 + error text.
inline int js_transform_plan(const JsImage* imgs, size_t nimg, const JsnoopTransformSpec& spec, const int* images, int n, int* results, int* image_of,
                             JsXfRec* recs, JsImage* descs, uint32_t* unit_base, uint32_t* nout, uint64_t* total_blocks)
{
    if (n < 0) { js_set_error("transform: n = %d", n); return -1; }
    if (!images && (size_t)n > nimg) { js_set_error("transform: n = %d without a list, the batch holds %zu", n, nimg); return -1; }
    for (int k = 0; images && k < n; k++)
        if (images[k] < 0 || (size_t)images[k] >= nimg) { js_set_error("transform: image index %d (entry %d) out of range, the batch holds %zu", images[k], k, nimg); return -1; }
    uint64_t blocks = 0, units = 0; uint32_t m = 0;
    for (int k = 0; k < n; k++) {
        const JsImage& im = imgs[images ? images[k] : k];
        results[k] = js_xf_entry(im, spec, &recs[m], &descs[m], nullptr); image_of[k] = -1;
        if (results[k] != JSNOOP_XFORM_OK) continue;
        recs[m].dst_off = blocks; descs[m].coef_off = blocks; unit_base[m] = (uint32_t)units;
        blocks += recs[m].nblk; units += (recs[m].nblk + JS_XF_RUN - 1u) / JS_XF_RUN;
        if (blocks >= 0x80000000ull) { js_set_error("transform: 2^31 blocks or more in one call"); return -1; }
        image_of[k] = (int)m++;
    }
    unit_base[m] = (uint32_t)units; *nout = m; *total_blocks = blocks;
    return 0;
}
// a table in natural order, transposed (cell [v][u] takes [u][v]) or as it is, into the zig-zag order a table set holds
inline void js_xf_table(const uint16_t nat[64], bool transposed, uint16_t qzz[64])
{
    static const uint8_t zz[64] = JS_ZIGZAG_NATURAL;
    for (int z = 0; z < 64; z++) { const int n = zz[z]; qzz[z] = nat[transposed ? (n & 7) * 8 + (n >> 3) : n]; }
}
