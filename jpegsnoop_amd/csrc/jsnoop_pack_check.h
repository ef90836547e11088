// jsnoop_pack_check.h -- the host arithmetic of jsnoop_batch_pack and jsnoop_batch_pack_resized: spec import, dense sizes, argument checks, records and prefix tables.
// No device call in here (tests/cpp/pack_check.cpp and resize_check.cpp run it as plain host programs); errors go through js_set_error.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_types.h"

void js_set_error(const char* fmt, ...);

inline void js_pack_spec_defaults(JsnoopPackSpec* s)
{
    memset(s, 0, sizeof *s); s->struct_size = (uint32_t)sizeof *s;
    for (int c = 0; c < 3; c++) { s->scale[c] = 1.0f; s->bias[c] = 0.0f; }
}
// struct_size is the caller's sizeof(JsnoopPackSpec), read like JsnoopTuning's: a shorter struct leaves the fields it lacks at their defaults, a longer one is refused
// (`who`: the entry point the error text names)
inline int js_pack_import_spec(const JsnoopPackSpec* in, JsnoopPackSpec* out, const char* who = "pack")
{
    if (!in) { js_set_error("%s: spec is NULL", who); return -1; }
    const uint32_t sz = in->struct_size;
    if (sz < sizeof(uint32_t) || sz > sizeof(JsnoopPackSpec)) { js_set_error("%s: struct_size %u, this library has %zu", who, sz, sizeof(JsnoopPackSpec)); return -1; }
    js_pack_spec_defaults(out); memcpy(out, in, sz); out->struct_size = (uint32_t)sizeof(JsnoopPackSpec);
    if (out->layout != JSNOOP_PACK_HWC && out->layout != JSNOOP_PACK_CHW) { js_set_error("%s: unknown layout %d", who, out->layout); return -1; }
    if (out->dtype != JSNOOP_PACK_U8 && out->dtype != JSNOOP_PACK_F32) { js_set_error("%s: unknown dtype %d", who, out->dtype); return -1; }
    return 0;
}
inline uint64_t js_pack_elem(const JsnoopPackSpec& s) { return s.dtype == JSNOOP_PACK_F32 ? 4u : 1u; }
inline uint64_t js_pack_dense_row(const JsImage& im, const JsnoopPackSpec& s) { return (uint64_t)im.dim_x * js_pack_elem(s) * (s.layout == JSNOOP_PACK_HWC ? 3u : 1u); }
inline uint64_t js_pack_dense_bytes(const JsImage& im, const JsnoopPackSpec& s) { return (uint64_t)im.dim_x * im.dim_y * 3u * js_pack_elem(s); }
inline uint64_t js_pack_units(const JsImage& im) { return (uint64_t)im.dim_y * ((im.dim_x + JS_PACK_SEG - 1u) / JS_PACK_SEG); }

// Checks every argument of one call and fills recs[n] and unit_base[n + 1].  0, or -1 + error text with nothing usable in the outputs.
// `s` has been through js_pack_import_spec.
inline int js_pack_plan(const JsImage* imgs, size_t nimg, const JsnoopPackSpec& s, const int* images, int n, const JsnoopPackDst* dst,
                        JsPackRec* recs, uint32_t* unit_base)
{
    uint64_t units = 0;
    for (int k = 0; k < n; k++) {
        const int i = images ? images[k] : k;
        if (i < 0 || (size_t)i >= nimg) { js_set_error("pack: image index %d (entry %d) out of range, the batch holds %zu", i, k, nimg); return -1; }
        const JsImage& im = imgs[i];
        // (every image a batch accepted has a geometry, and a decoded batch holds a DIB for each of them: this guards a descriptor that is not one of those)
        if (!im.dim_x || !im.dim_y || im.img_x < im.dim_x || im.img_y < im.dim_y) { js_set_error("pack: image %d has no decoded DIB", i); return -1; }
        const JsnoopPackDst& d = dst[k];
        if (!d.ptr) { js_set_error("pack: destination %d (image %d) is NULL", k, i); return -1; }
        const uint64_t dense_row = js_pack_dense_row(im, s), row_pitch = d.row_pitch ? d.row_pitch : dense_row;
        if (row_pitch < dense_row) { js_set_error("pack: row_pitch %llu of destination %d (image %d) is below the dense row of %llu bytes", (unsigned long long)d.row_pitch, k, i, (unsigned long long)dense_row); return -1; }
        const uint64_t dense_plane = (uint64_t)im.dim_y * row_pitch;
        uint64_t plane_pitch = dense_plane;
        if (s.layout == JSNOOP_PACK_CHW) {
            if (d.plane_pitch) plane_pitch = d.plane_pitch;
            if (plane_pitch < dense_plane) { js_set_error("pack: plane_pitch %llu of destination %d (image %d) is below the dense plane of %llu bytes", (unsigned long long)d.plane_pitch, k, i, (unsigned long long)dense_plane); return -1; }
        }
        if (s.dtype == JSNOOP_PACK_F32 && (((uint64_t)(uintptr_t)d.ptr | row_pitch | plane_pitch) & 3u)) {
            js_set_error("pack: float32 destination %d (image %d): pointer and pitches must be multiples of 4", k, i); return -1; }
        JsPackRec& r = recs[k];
        r.img = (uint32_t)i; r.reserved = 0; r.ptr = (uint64_t)(uintptr_t)d.ptr; r.row_pitch = row_pitch; r.plane_pitch = plane_pitch;
        unit_base[k] = (uint32_t)units; units += js_pack_units(im);
        if (units >= 0xFFFF0000ull) { js_set_error("pack: more than 2^32 row segments in one call"); return -1; }
    }
    unit_base[n] = (uint32_t)units;
    return 0;
}

// ---- jsnoop_batch_pack_resized: the same checks for an out_w x out_h destination, plus filter, output size and ROI ----
inline int js_resize_check_filter(int filter)
{
    if (filter != JSNOOP_RESIZE_NEAREST && filter != JSNOOP_RESIZE_BILINEAR && filter != JSNOOP_RESIZE_AREA) { js_set_error("pack_resized: unknown filter %d", filter); return -1; }
    return 0;
}
inline uint64_t js_resize_units(uint32_t out_w, uint32_t out_h) { return (uint64_t)out_h * ((out_w + JS_RESIZE_SEG - 1u) / JS_RESIZE_SEG); }

// Checks every argument of one call and fills recs[n] and unit_base[n + 1].  0, or -1 + error text with nothing usable in the outputs.
// `s` has been through js_pack_import_spec, the filter through js_resize_check_filter.
inline int js_resize_plan(const JsImage* imgs, size_t nimg, const JsnoopPackSpec& s, const int* images, int n, const JsnoopResizeDst* dst,
                          JsResizeRec* recs, uint32_t* unit_base)
{
    uint64_t units = 0;
    for (int k = 0; k < n; k++) {
        const int i = images ? images[k] : k;
        if (i < 0 || (size_t)i >= nimg) { js_set_error("pack_resized: image index %d (entry %d) out of range, the batch holds %zu", i, k, nimg); return -1; }
        const JsImage& im = imgs[i];
        if (!im.dim_x || !im.dim_y || im.img_x < im.dim_x || im.img_y < im.dim_y) { js_set_error("pack_resized: image %d has no decoded DIB", i); return -1; }
        const JsnoopResizeDst& d = dst[k];
        if (!d.ptr) { js_set_error("pack_resized: destination %d (image %d) is NULL", k, i); return -1; }
        if (!d.out_w || !d.out_h || d.out_w > 32767u || d.out_h > 32767u) {
            js_set_error("pack_resized: output size %u x %u of destination %d (image %d): each of 1 .. 32767", d.out_w, d.out_h, k, i); return -1; }
        uint32_t rx = d.roi_x, ry = d.roi_y, rw = d.roi_w, rh = d.roi_h;
        if (!rw != !rh || (!rw && (rx || ry))) {
            js_set_error("pack_resized: ROI %u,%u %u x %u of destination %d (image %d): width and height are both 0 (the whole image, at 0,0) or both positive", rx, ry, rw, rh, k, i); return -1; }
        if (!rw) { rw = im.dim_x; rh = im.dim_y; }
        if ((uint64_t)rx + rw > im.dim_x || (uint64_t)ry + rh > im.dim_y) {
            js_set_error("pack_resized: ROI %u,%u %u x %u of destination %d leaves image %d of %u x %u", rx, ry, rw, rh, k, i, im.dim_x, im.dim_y); return -1; }
        // (the kernel's 32-bit products: (2 * out - 1) * roi and out * roi stay below 2^32 for roi <= 65535, the largest dimension a SOF can carry)
        if (rw > 65535u || rh > 65535u) { js_set_error("pack_resized: ROI %u x %u of destination %d (image %d) is above 65535", rw, rh, k, i); return -1; }
        const uint64_t dense_row = (uint64_t)d.out_w * js_pack_elem(s) * (s.layout == JSNOOP_PACK_HWC ? 3u : 1u), row_pitch = d.row_pitch ? d.row_pitch : dense_row;
        if (row_pitch < dense_row) { js_set_error("pack_resized: row_pitch %llu of destination %d (image %d) is below the dense row of %llu bytes", (unsigned long long)d.row_pitch, k, i, (unsigned long long)dense_row); return -1; }
        const uint64_t dense_plane = (uint64_t)d.out_h * row_pitch;
        uint64_t plane_pitch = dense_plane;
        if (s.layout == JSNOOP_PACK_CHW) {
            if (d.plane_pitch) plane_pitch = d.plane_pitch;
            if (plane_pitch < dense_plane) { js_set_error("pack_resized: plane_pitch %llu of destination %d (image %d) is below the dense plane of %llu bytes", (unsigned long long)d.plane_pitch, k, i, (unsigned long long)dense_plane); return -1; }
        }
        if (s.dtype == JSNOOP_PACK_F32 && (((uint64_t)(uintptr_t)d.ptr | row_pitch | plane_pitch) & 3u)) {
            js_set_error("pack_resized: float32 destination %d (image %d): pointer and pitches must be multiples of 4", k, i); return -1; }
        JsResizeRec& r = recs[k];
        r.img = (uint32_t)i; r.out_w = d.out_w; r.out_h = d.out_h; r.roi_x = rx; r.roi_y = ry; r.roi_w = rw; r.roi_h = rh; r.reserved = 0;
        r.ptr = (uint64_t)(uintptr_t)d.ptr; r.row_pitch = row_pitch; r.plane_pitch = plane_pitch;
        unit_base[k] = (uint32_t)units; units += js_resize_units(d.out_w, d.out_h);
        if (units >= 0xFFFF0000ull) { js_set_error("pack_resized: more than 2^32 row segments in one call"); return -1; }
    }
    unit_base[n] = (uint32_t)units;
    return 0;
}
