// jsnoop_coef_check.h -- the host arithmetic of jsnoop_batch_pack_coefs: spec import, block grids, dense sizes, argument checks, records and prefix table.
// No device call in here (tests/cpp/coef_check.cpp runs it as a plain host program); errors go through js_set_error.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_types.h"

void js_set_error(const char* fmt, ...);

inline void js_coef_spec_defaults(JsnoopCoefSpec* s) { memset(s, 0, sizeof *s); s->struct_size = (uint32_t)sizeof *s; }
// struct_size is the caller's sizeof(JsnoopCoefSpec), read like JsnoopPackSpec's: a shorter struct leaves the fields it lacks at their defaults, a longer one is refused
inline int js_coef_import_spec(const JsnoopCoefSpec* in, JsnoopCoefSpec* out)
{
    if (!in) { js_set_error("pack_coefs: spec is NULL"); return -1; }
    const uint32_t sz = in->struct_size;
    if (sz < sizeof(uint32_t) || sz > sizeof(JsnoopCoefSpec)) { js_set_error("pack_coefs: struct_size %u, this library has %zu", sz, sizeof(JsnoopCoefSpec)); return -1; }
    js_coef_spec_defaults(out); memcpy(out, in, sz); out->struct_size = (uint32_t)sizeof(JsnoopCoefSpec);
    if (out->layout != JSNOOP_COEF_BLOCKS && out->layout != JSNOOP_COEF_FREQ) { js_set_error("pack_coefs: unknown layout %d", out->layout); return -1; }
    if (out->dtype != JSNOOP_COEF_I16 && out->dtype != JSNOOP_COEF_F32) { js_set_error("pack_coefs: unknown dtype %d", out->dtype); return -1; }
    if (out->order != JSNOOP_COEF_NATURAL && out->order != JSNOOP_COEF_ZIGZAG) { js_set_error("pack_coefs: unknown order %d", out->order); return -1; }
    return 0;
}
inline uint64_t js_coef_elem(const JsnoopCoefSpec& s) { return s.dtype == JSNOOP_COEF_F32 ? 4u : 2u; }

// The block grid of component `comp` (0 = Y) and where its blocks sit inside an MCU, from the descriptor's block list (blk_comp / blk_ch / blk_cv, js_geometry):
// *first = the MCU's block of that component with (ch, cv) = (0, 0).  -1 when the component's blocks are not samp_v rows of samp_h consecutive blocks.
inline int js_coef_grid(const JsImage& im, int comp, uint32_t* bw, uint32_t* bh, uint32_t* first)
{
    if (comp < 0 || (uint32_t)comp >= im.ncomp || im.ncomp > 3u) { js_set_error("pack_coefs: component %d, the image has %u", comp, im.ncomp); return -1; }
    const uint32_t c = (uint32_t)comp + 1u, sh = im.samp_h[c], sv = im.samp_v[c];
    if (!sh || !sv || sh > 4u || sv > 4u || !im.mcu_xmax || !im.mcu_ymax || !im.blk_per_mcu || im.blk_per_mcu > JS_MAX_BLK_PER_MCU) {
        js_set_error("pack_coefs: the image has no decoded geometry"); return -1; }
    uint32_t f = 0; while (f < im.blk_per_mcu && im.blk_comp[f] != c) f++;
    if (f + sh * sv > im.blk_per_mcu) { js_set_error("pack_coefs: component %d has no blocks in the MCU", comp); return -1; }
    for (uint32_t v = 0; v < sv; v++) for (uint32_t h = 0; h < sh; h++) {
        const uint32_t j = f + v * sh + h;
        if (im.blk_comp[j] != c || im.blk_ch[j] != h || im.blk_cv[j] != v) { js_set_error("pack_coefs: unexpected block order inside the MCU"); return -1; }
    }
    *bw = im.mcu_xmax * sh; *bh = im.mcu_ymax * sv; if (first) *first = f;
    return 0;
}
inline uint64_t js_coef_dense_row(uint32_t bw, const JsnoopCoefSpec& s) { return (uint64_t)bw * js_coef_elem(s) * (s.layout == JSNOOP_COEF_BLOCKS ? 64u : 1u); }
inline uint64_t js_coef_dense_bytes(uint32_t bw, uint32_t bh, const JsnoopCoefSpec& s) { return (uint64_t)bw * bh * 64u * js_coef_elem(s); }
inline uint64_t js_coef_units(uint32_t bw, uint32_t bh) { return (uint64_t)bh * ((bw + JS_COEF_TILE - 1u) / JS_COEF_TILE); }

// Checks every argument of one call and fills recs[n] and unit_base[n + 1].  0, or -1 + error text with nothing usable in the outputs.
// `s` has been through js_coef_import_spec.
inline int js_coef_plan(const JsImage* imgs, size_t nimg, const JsnoopCoefSpec& s, const int* images, int n, const JsnoopCoefDst* dst,
                        JsCoefRec* recs, uint32_t* unit_base)
{
    uint64_t units = 0;
    const uint64_t elem = js_coef_elem(s);
    for (int k = 0; k < n; k++) {
        const int i = images ? images[k] : k;
        if (i < 0 || (size_t)i >= nimg) { js_set_error("pack_coefs: image index %d (entry %d) out of range, the batch holds %zu", i, k, nimg); return -1; }
        const JsImage& im = imgs[i];
        const JsnoopCoefDst& d = dst[k];
        if (!d.ptr) { js_set_error("pack_coefs: destination %d (image %d) is NULL", k, i); return -1; }
        if (d.reserved) { js_set_error("pack_coefs: destination %d (image %d): reserved is %u, must be 0", k, i, d.reserved); return -1; }
        if (d.comp >= im.ncomp) { js_set_error("pack_coefs: destination %d names component %u, image %d has %u", k, d.comp, i, im.ncomp); return -1; }
        uint32_t bw = 0, bh = 0, first = 0;
        if (js_coef_grid(im, (int)d.comp, &bw, &bh, &first)) return -1;
        const uint64_t dense_row = js_coef_dense_row(bw, s), row_pitch = d.row_pitch ? d.row_pitch : dense_row;
        if (row_pitch < dense_row) { js_set_error("pack_coefs: row_pitch %llu of destination %d (image %d) is below the dense row of %llu bytes", (unsigned long long)d.row_pitch, k, i, (unsigned long long)dense_row); return -1; }
        const uint64_t dense_plane = (uint64_t)bh * row_pitch;
        uint64_t plane_pitch = dense_plane;
        if (s.layout == JSNOOP_COEF_FREQ) {
            if (d.plane_pitch) plane_pitch = d.plane_pitch;
            if (plane_pitch < dense_plane) { js_set_error("pack_coefs: plane_pitch %llu of destination %d (image %d) is below the dense plane of %llu bytes", (unsigned long long)d.plane_pitch, k, i, (unsigned long long)dense_plane); return -1; }
        }
        if (((uint64_t)(uintptr_t)d.ptr | row_pitch | plane_pitch) & (elem - 1u)) {
            js_set_error("pack_coefs: destination %d (image %d): pointer and pitches must be multiples of %u", k, i, (unsigned)elem); return -1; }
        JsCoefRec& r = recs[k];
        r.ptr = (uint64_t)(uintptr_t)d.ptr; r.row_pitch = row_pitch; r.plane_pitch = plane_pitch; r.coef_off = im.coef_off;
        r.bw = bw; r.bh = bh; r.sh = im.samp_h[d.comp + 1u]; r.sv = im.samp_v[d.comp + 1u]; r.first = first; r.bpm = im.blk_per_mcu; r.mcu_xmax = im.mcu_xmax;
        r.tiles = (bw + JS_COEF_TILE - 1u) / JS_COEF_TILE;
        unit_base[k] = (uint32_t)units; units += js_coef_units(bw, bh);
        if (units >= 0xFFFF0000ull) { js_set_error("pack_coefs: more than 2^32 block runs in one call"); return -1; }
    }
    unit_base[n] = (uint32_t)units;
    return 0;
}

// zig-zag table (position z of a DQT segment) -> natural order
inline void js_coef_dqt_natural(const uint16_t* qzz, uint16_t* out64)
{
    static const uint8_t zz[64] = JS_ZIGZAG_NATURAL;
    for (int z = 0; z < 64; z++) out64[zz[z]] = qzz[z];
}
