// jsnoop_coef_hist_check.h -- the host arithmetic of jsnoop_batch_pack_coef_hist / _read_coef_hist: spec import, row length, argument checks, records and the
// 64-bit prefix table.  No device call in here (tests/cpp/coef_hist_check.cpp runs it as a plain host program); errors go through js_set_error.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_types.h"
#include "jsnoop_coef_check.h"
#include "jsnoop_coef_bin.h"

inline void js_coef_hist_spec_defaults(JsnoopCoefHistSpec* s) { memset(s, 0, sizeof *s); s->struct_size = (uint32_t)sizeof *s; s->order = JSNOOP_COEF_NATURAL; s->quantised = 1; s->range = 127u; }
// struct_size is the caller's sizeof(JsnoopCoefHistSpec), read like JsnoopCoefSpec's: a shorter struct leaves the fields it lacks at their defaults, a longer one is refused
inline int js_coef_hist_import_spec(const JsnoopCoefHistSpec* in, JsnoopCoefHistSpec* out)
{
    if (!in) { js_set_error("pack_coef_hist: spec is NULL"); return -1; }
    const uint32_t sz = in->struct_size;
    if (sz < sizeof(uint32_t) || sz > sizeof(JsnoopCoefHistSpec)) { js_set_error("pack_coef_hist: struct_size %u, this library has %zu", sz, sizeof(JsnoopCoefHistSpec)); return -1; }
    js_coef_hist_spec_defaults(out); memcpy(out, in, sz); out->struct_size = (uint32_t)sizeof(JsnoopCoefHistSpec);
    if (out->order != JSNOOP_COEF_NATURAL && out->order != JSNOOP_COEF_ZIGZAG) { js_set_error("pack_coef_hist: unknown order %d", out->order); return -1; }
    if (out->range < 1u || out->range > 127u) { js_set_error("pack_coef_hist: range %u is outside 1..127", out->range); return -1; }
    return 0;
}
inline uint64_t js_coef_hist_units(uint32_t nblk) { return ((uint64_t)nblk + JS_COEF_HIST_UNIT - 1u) / JS_COEF_HIST_UNIT; }
// the pitch the call works with (0 = dense), or 0 + error text
inline uint64_t js_coef_hist_pitch(uint64_t row_pitch_words, uint32_t words)
{
    if (!row_pitch_words) return words;
    if (row_pitch_words < words) { js_set_error("pack_coef_hist: row_pitch_words %llu is below the row of %u words", (unsigned long long)row_pitch_words, words); return 0; }
    if (row_pitch_words > (1ull << 40)) { js_set_error("pack_coef_hist: row_pitch_words %llu is not a pitch", (unsigned long long)row_pitch_words); return 0; }
    return row_pitch_words;
}

// the 64 DQT entries of (image, comp) in natural order; 0 / -1 + error text
typedef int (*js_coef_hist_dqt_fn)(void* ctx, int image, int comp, uint16_t* out64);

// Checks every argument of one call and fills recs[n] and unit_base[n + 1].  0, or -1 + error text with nothing usable in the outputs.
// `s` has been through js_coef_hist_import_spec.
inline int js_coef_hist_plan(const JsImage* imgs, size_t nimg, const JsnoopCoefHistSpec& s, const int* images, const int* comps, int n, const void* dst, uint64_t row_pitch_words,
                             js_coef_hist_dqt_fn dqt, void* ctx, JsCoefHistRec* recs, uint64_t* unit_base)
{
    if (!images) { js_set_error("pack_coef_hist: images is NULL"); return -1; }
    if (!comps) { js_set_error("pack_coef_hist: comps is NULL"); return -1; }
    if (!dst) { js_set_error("pack_coef_hist: destination is NULL"); return -1; }
    if ((uint64_t)(uintptr_t)dst & 3u) { js_set_error("pack_coef_hist: the destination must be a multiple of 4"); return -1; }
    const uint32_t words = js_chist_words(s.range);
    const uint64_t pitch = js_coef_hist_pitch(row_pitch_words, words);
    if (!pitch) return -1;
    uint64_t units = 0;
    for (int k = 0; k < n; k++) {
        const int i = images[k], c = comps[k];
        if (i < 0 || (size_t)i >= nimg) { js_set_error("pack_coef_hist: image index %d (entry %d) out of range, the batch holds %zu", i, k, nimg); return -1; }
        const JsImage& im = imgs[i];
        if (c < 0 || (uint32_t)c >= im.ncomp) { js_set_error("pack_coef_hist: entry %d names component %d, image %d has %u", k, c, i, im.ncomp); return -1; }
        uint32_t bw = 0, bh = 0, first = 0;
        if (js_coef_grid(im, c, &bw, &bh, &first)) return -1;
        if ((uint64_t)bw * bh > 0xFFFFFFFFull) { js_set_error("pack_coef_hist: image %d (entry %d) has more than 2^32 blocks", i, k); return -1; }
        JsCoefHistRec& r = recs[k];
        memset(&r, 0, sizeof r);
        r.dst = (uint64_t)(uintptr_t)dst + (uint64_t)k * pitch * 4u; r.coef_off = im.coef_off;
        r.nblk = bw * bh; r.hv = im.samp_h[c + 1] * im.samp_v[c + 1]; r.first = first; r.bpm = im.blk_per_mcu; r.hv_magic = 65536u / r.hv + 1u;
        uint16_t q[64];
        if (s.quantised) { if (dqt(ctx, i, c, q)) return -1; }
        for (int f = 0; f < 64; f++) r.recip[f] = js_chist_recip(s.quantised ? q[f] : 1u);
        unit_base[k] = units; units += js_coef_hist_units(r.nblk);
    }
    unit_base[n] = units;
    return 0;
}
