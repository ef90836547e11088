// jsnoop_plane_check.h -- the host arithmetic of jsnoop_batch_pack_planes: spec import, output sizes, dense sizes, argument checks, records and prefix table.
// No device call in here (tests/cpp/plane_check.cpp runs it as a plain host program); errors go through js_set_error.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_types.h"

void js_set_error(const char* fmt, ...);

inline void js_plane_spec_defaults(JsnoopPlaneSpec* s)
{
    memset(s, 0, sizeof *s); s->struct_size = (uint32_t)sizeof *s;
    for (int c = 0; c < 3; c++) { s->scale[c] = 1.0f; s->bias[c] = 0.0f; }
}
// struct_size is the caller's sizeof(JsnoopPlaneSpec), read like JsnoopPackSpec's: a shorter struct leaves the fields it lacks at their defaults, a longer one is refused
inline int js_plane_import_spec(const JsnoopPlaneSpec* in, JsnoopPlaneSpec* out)
{
    if (!in) { js_set_error("pack_planes: spec is NULL"); return -1; }
    const uint32_t sz = in->struct_size;
    if (sz < sizeof(uint32_t) || sz > sizeof(JsnoopPlaneSpec)) { js_set_error("pack_planes: struct_size %u, this library has %zu", sz, sizeof(JsnoopPlaneSpec)); return -1; }
    js_plane_spec_defaults(out); memcpy(out, in, sz); out->struct_size = (uint32_t)sizeof(JsnoopPlaneSpec);
    if (out->res != JSNOOP_PLANE_FULL && out->res != JSNOOP_PLANE_NATIVE) { js_set_error("pack_planes: unknown res %d", out->res); return -1; }
    if (out->dtype != JSNOOP_PLANE_I16 && out->dtype != JSNOOP_PLANE_U8 && out->dtype != JSNOOP_PLANE_F32) { js_set_error("pack_planes: unknown dtype %d", out->dtype); return -1; }
    return 0;
}
inline uint64_t js_plane_elem(const JsnoopPlaneSpec& s) { return s.dtype == JSNOOP_PLANE_F32 ? 4u : s.dtype == JSNOOP_PLANE_U8 ? 1u : 2u; }

// Output size of component `comp` (0 = Y) under `s`, and the steps (eh, ev) through the retained plane that give it: FULL walks every sample of dim_x x dim_y,
// NATIVE every expand_h-th column and every expand_v-th row.  -1 for a component the image lacks or a descriptor without a decoded geometry.
inline int js_plane_size(const JsImage& im, const JsnoopPlaneSpec& s, int comp, uint32_t* w, uint32_t* h, uint32_t* eh, uint32_t* ev)
{
    if (comp < 0 || comp > 2 || (uint32_t)comp >= im.ncomp) { js_set_error("pack_planes: component %d, the image has %u", comp, im.ncomp); return -1; }
    const uint32_t c = (uint32_t)comp + 1u, xh = im.expand_h[c], xv = im.expand_v[c];
    if (!im.dim_x || !im.dim_y || !xh || !xv || xh > 4u || xv > 4u || (uint64_t)im.blk_xmax * 8u < im.dim_x || (uint64_t)im.blk_ymax * 8u < im.dim_y ||
        im.dim_x > 65535u || im.dim_y > 65535u || (im.plane_off & 7u)) {
        js_set_error("pack_planes: the image has no decoded geometry"); return -1; }
    const uint32_t sx = s.res == JSNOOP_PLANE_NATIVE ? xh : 1u, sy = s.res == JSNOOP_PLANE_NATIVE ? xv : 1u;
    *w = (im.dim_x + sx - 1u) / sx; *h = (im.dim_y + sy - 1u) / sy;
    if (eh) *eh = sx;
    if (ev) *ev = sy;
    return 0;
}
inline uint64_t js_plane_dense_row(uint32_t w, const JsnoopPlaneSpec& s) { return (uint64_t)w * js_plane_elem(s); }
inline uint64_t js_plane_dense_bytes(uint32_t w, uint32_t h, const JsnoopPlaneSpec& s) { return (uint64_t)w * h * js_plane_elem(s); }
inline uint64_t js_plane_units(uint32_t w, uint32_t h) { return (uint64_t)h * ((w + JS_PLANE_SEG - 1u) / JS_PLANE_SEG); }

// Checks every argument of one call and fills recs[n] and unit_base[n + 1].  0, or -1 + error text with nothing usable in the outputs.
// `s` has been through js_plane_import_spec.
inline int js_plane_plan(const JsImage* imgs, size_t nimg, const JsnoopPlaneSpec& s, const int* images, int n, const JsnoopPlaneDst* dst,
                         JsPlaneRec* recs, uint32_t* unit_base)
{
    uint64_t units = 0;
    const uint64_t elem = js_plane_elem(s);
    for (int k = 0; k < n; k++) {
        const int i = images ? images[k] : k;
        if (i < 0 || (size_t)i >= nimg) { js_set_error("pack_planes: image index %d (entry %d) out of range, the batch holds %zu", i, k, nimg); return -1; }
        const JsImage& im = imgs[i];
        const JsnoopPlaneDst& d = dst[k];
        if (!d.ptr) { js_set_error("pack_planes: destination %d (image %d) is NULL", k, i); return -1; }
        if (d.reserved) { js_set_error("pack_planes: destination %d (image %d): reserved is %u, must be 0", k, i, d.reserved); return -1; }
        if (d.comp > 2u || d.comp >= im.ncomp) { js_set_error("pack_planes: destination %d names component %u, image %d has %u", k, d.comp, i, im.ncomp); return -1; }
        uint32_t w = 0, h = 0, eh = 1, ev = 1;
        if (js_plane_size(im, s, (int)d.comp, &w, &h, &eh, &ev)) return -1;
        const uint64_t dense_row = js_plane_dense_row(w, s), row_pitch = d.row_pitch ? d.row_pitch : dense_row;
        if (row_pitch < dense_row) { js_set_error("pack_planes: row_pitch %llu of destination %d (image %d) is below the dense row of %llu bytes", (unsigned long long)d.row_pitch, k, i, (unsigned long long)dense_row); return -1; }
        if (((uint64_t)(uintptr_t)d.ptr | row_pitch) & (elem - 1u)) {
            js_set_error("pack_planes: destination %d (image %d): pointer and pitch must be multiples of %u", k, i, (unsigned)elem); return -1; }
        JsPlaneRec& r = recs[k];
        r.ptr = (uint64_t)(uintptr_t)d.ptr; r.row_pitch = row_pitch;
        r.pw = im.blk_xmax * 8u; r.src_off = im.plane_off + (uint64_t)d.comp * r.pw * im.blk_ymax * 8u;
        r.w = w; r.h = h; r.eh = eh; r.ev = ev; r.xlim = im.dim_x; r.comp = d.comp; r.segs = (w + JS_PLANE_SEG - 1u) / JS_PLANE_SEG;
        unit_base[k] = (uint32_t)units; units += js_plane_units(w, h);
        if (units >= 0xFFFF0000ull) { js_set_error("pack_planes: more than 2^32 row segments in one call"); return -1; }
    }
    unit_base[n] = (uint32_t)units;
    return 0;
}
