// jsnoop_stats_check.h -- the host arithmetic of jsnoop_batch_pack_stats / _read_stats: argument checks, records, the 64-bit prefix table and scratch sizes.
// No device call in here (tests/cpp/stats_check.cpp runs it as a plain host program); errors go through js_set_error.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_types.h"

void js_set_error(const char* fmt, ...);

inline uint64_t js_stats_units(const JsImage& im) { return (uint64_t)im.img_y * ((im.img_x + JS_STATS_UNIT - 1u) / JS_STATS_UNIT); }
// the pitch the call works with (0 = dense), or 0 + error text
inline uint64_t js_stats_pitch(uint64_t row_pitch_words)
{
    if (!row_pitch_words) return JSNOOP_STATS_WORDS;
    if (row_pitch_words < JSNOOP_STATS_WORDS) { js_set_error("pack_stats: row_pitch_words %llu is below the row of %d words", (unsigned long long)row_pitch_words, JSNOOP_STATS_WORDS); return 0; }
    if (row_pitch_words > (1ull << 40)) { js_set_error("pack_stats: row_pitch_words %llu is not a pitch", (unsigned long long)row_pitch_words); return 0; }
    return row_pitch_words;
}
// bytes of batch scratch behind one call: JS_STATS_TOT_WORDS words of totals per listed row, then one range-event count per picture row of every listed row
inline uint64_t js_stats_scratch_bytes(int n, uint64_t row_words) { return ((uint64_t)n * JS_STATS_TOT_WORDS + row_words) * 4u; }

// Checks every argument of one call and fills recs[n] and unit_base[n + 1]; *row_words = picture rows of all listed rows together.
// 0, or -1 + error text with nothing usable in the outputs.  The statistics walk the MCU-padded picture img_x x img_y at the planes' pitch blk_xmax * 8.
inline int js_stats_plan(const JsImage* imgs, size_t nimg, const int* images, int n, const void* dst, uint64_t row_pitch_words,
                         JsStatRec* recs, uint64_t* unit_base, uint64_t* row_words)
{
    if (!dst) { js_set_error("pack_stats: destination is NULL"); return -1; }
    if ((uint64_t)(uintptr_t)dst & 3u) { js_set_error("pack_stats: the destination must be a multiple of 4"); return -1; }
    const uint64_t pitch = js_stats_pitch(row_pitch_words);
    if (!pitch) return -1;
    uint64_t units = 0, rows = 0;
    for (int k = 0; k < n; k++) {
        const int i = images ? images[k] : k;
        if (i < 0 || (size_t)i >= nimg) { js_set_error("pack_stats: image index %d (entry %d) out of range, the batch holds %zu", i, k, nimg); return -1; }
        const JsImage& im = imgs[i];
        if (!im.img_x || !im.img_y || !im.mcu_w || !im.mcu_h || (im.mcu_w & 7u) || (im.img_x & 7u) || im.img_x % im.mcu_w || im.blk_xmax * 8u < im.img_x ||
            im.blk_ymax * 8u < im.img_y || (im.plane_off & 7u) || im.img_x > 0xFFFF8u || im.img_y > 0xFFFF8u) {
            js_set_error("pack_stats: image %d (entry %d) has no decoded geometry", i, k); return -1; }
        JsStatRec& r = recs[k];
        r.dst = (uint64_t)(uintptr_t)dst + (uint64_t)k * pitch * 4u; r.plane_off = im.plane_off;
        r.pw = im.blk_xmax * 8u; r.psz = (uint64_t)r.pw * im.blk_ymax * 8u; r.row_base = rows;
        r.img_x = im.img_x; r.img_y = im.img_y; r.ncomp = im.ncomp; r.mcu_w = im.mcu_w; r.mcu_h = im.mcu_h; r.across = im.img_x / im.mcu_w;
        r.shift_ind = im.shift_mcu_y * r.across + im.shift_mcu_x; r.shift_y = im.shift_y; r.shift_cb = im.shift_cb; r.shift_cr = im.shift_cr;
        r.tiles = (im.img_x + JS_STATS_UNIT - 1u) / JS_STATS_UNIT;
        unit_base[k] = units; units += js_stats_units(im); rows += im.img_y;
    }
    unit_base[n] = units; *row_words = rows;
    return 0;
}
