// jsnoop_export_rst_check.h -- the host arithmetic jsnoop_batch_export_jpeg_rst adds to jsnoop_export_check.h / jsnoop_export_opt_check.h: the restart spec and
// its refusals, the effective interval of an entry, the side records and interval tables, DRI in the header, the second phase's layout with the worst-case size
// of a file, and the scan operator the kernels place blocks with (the same functions, compiled for the device too).  No device call in here
// (tests/cpp/export_rst_check.cpp runs it as a plain host program).
#pragma once
#include "jsnoop_export_opt_check.h"

#if defined(__HIPCC__)
#define JS_RST_HD __host__ __device__ __forceinline__
#else
#define JS_RST_HD inline
#endif

// ---- the scan operator.  In the un-stuffed stream every interval starts on a byte, so the bit position of a block is 8 x (bytes of all earlier intervals, each
// rounded up) + the bits in front of it inside its own interval.  A run of blocks is summarised by JsRstSum (jsnoop_types.h); a block of n bits is (0, n, 0, 0),
// or (1, n, 0, 0) when it is the last of its interval.  Two runs that follow each other combine associatively:
JS_RST_HD JsRstSum js_rst_identity() { JsRstSum s; s.has = 0u; s.head = 0u; s.mid = 0u; s.tail = 0u; return s; }
JS_RST_HD JsRstSum js_rst_leaf(uint32_t bits, bool ends) { JsRstSum s; s.has = ends ? 1u : 0u; s.head = bits; s.mid = 0u; s.tail = 0u; return s; }
JS_RST_HD JsRstSum js_rst_combine(const JsRstSum& a, const JsRstSum& b)
{
    JsRstSum s;
    if (!a.has) { s.has = b.has; s.head = a.head + b.head; s.mid = b.mid; s.tail = b.tail; }
    else if (!b.has) { s.has = 1u; s.head = a.head; s.mid = a.mid; s.tail = a.tail + b.head; }
    else { s.has = 1u; s.head = a.head; s.mid = a.mid + ((a.tail + b.head + 7u) >> 3) + b.mid; s.tail = b.tail; }
    return s;
}
// the bit position behind a run that starts at bit position pos (pos counts from the entry's start; the interval pos lies in started on a byte)
JS_RST_HD uint64_t js_rst_apply(uint64_t pos, const JsRstSum& s)
{
    if (!s.has) return pos + s.head;
    return ((((pos + s.head + 7u) >> 3) + s.mid) << 3) + s.tail;
}

inline void js_export_restart_defaults(JsnoopExportRestart* r) { memset(r, 0, sizeof *r); r->struct_size = (uint32_t)sizeof *r; r->mode = JSNOOP_RESTART_NONE; }
// struct_size read like JsnoopExportSpec's; NULL: the defaults.  Refused: an unknown mode, an interval of 0 or above 65535 with MCUS / ROWS, a non-zero interval with
// NONE / SOURCE, non-zero reserved.
inline int js_export_import_restart(const JsnoopExportRestart* in, JsnoopExportRestart* out)
{
    js_export_restart_defaults(out);
    if (!in) return 0;
    const uint32_t sz = in->struct_size;
    if (sz < sizeof(uint32_t) || sz > sizeof(JsnoopExportRestart)) { js_set_error("export_jpeg: restart struct_size %u, this library has %zu", sz, sizeof(JsnoopExportRestart)); return -1; }
    memcpy(out, in, sz); out->struct_size = (uint32_t)sizeof(JsnoopExportRestart);
    if (out->mode < JSNOOP_RESTART_NONE || out->mode > JSNOOP_RESTART_SOURCE) { js_set_error("export_jpeg: restart mode = %d (0: none, 1: MCUs, 2: MCU rows, 3: the source's)", out->mode); return -1; }
    if (out->reserved) { js_set_error("export_jpeg: restart reserved = %u, must be 0", out->reserved); return -1; }
    const bool counted = out->mode == JSNOOP_RESTART_MCUS || out->mode == JSNOOP_RESTART_ROWS;
    if (counted && (out->interval == 0u || out->interval > 65535u)) { js_set_error("export_jpeg: restart interval = %u with mode %d (1 .. 65535)", out->interval, out->mode); return -1; }
    if (!counted && out->interval) { js_set_error("export_jpeg: restart interval = %u with mode %d, which takes none", out->interval, out->mode); return -1; }
    return 0;
}
// the Ri an image is written with under an imported spec (above 65535: the entry is JSNOOP_EXPORT_UNSUPPORTED)
inline uint64_t js_export_rst_ri(const JsnoopExportRestart& r, const JsImage& im)
{
    switch (r.mode) {
    case JSNOOP_RESTART_MCUS: return r.interval;
    case JSNOOP_RESTART_ROWS: return (uint64_t)r.interval * im.mcu_xmax;
    case JSNOOP_RESTART_SOURCE: return im.rst_en ? im.rst_interval : 0u;
    default: return 0u;
    }
}

// the call's page-locked block: js_export_block's (or js_export_opt_block's) pieces, the restart side records behind them
struct JsExportRstBlock { JsExportOptBlock o; size_t rrecs; };
inline JsExportRstBlock js_export_rst_block(size_t n, bool opt)
{
    JsExportRstBlock b;
    if (opt) b.o = js_export_opt_block(n); else { b.o.b = js_export_block(n); b.o.orecs = 0; }
    b.rrecs = b.o.b.total; b.o.b.total = (b.o.b.total + n * sizeof(JsExportRstRec) + 15u) & ~(size_t)15u;
    return b;
}
// the first phase's scratch: js_export_scratch's (js_export_opt_scratch's) pieces, one JsRstSum per unit and the interval tables behind them
struct JsExportRstScratch { JsExportOptScratch o; size_t sums, itab; };
inline JsExportRstScratch js_export_rst_scratch(size_t n, uint64_t units, uint64_t blocks, uint64_t intervals, bool opt)
{
    JsExportRstScratch s;
    if (opt) s.o = js_export_opt_scratch(n, units, blocks); else { s.o.s = js_export_scratch(n, units, blocks); s.o.hdr_len = 0; }
    size_t at = s.o.s.total;
    auto take = [&](size_t bytes) { const size_t p = at; at = (at + bytes + 15u) & ~(size_t)15u; return p; };
    s.sums = take((size_t)units * sizeof(JsRstSum)); s.itab = take((size_t)intervals * 8u); s.o.s.total = at;
    return s;
}

// Behind js_export_plan / js_export_opt_plan: the effective interval of every entry (ri[k]; above 65535: unsupported, the entry owns no unit, so the prefix table
// and the block bases are made again), the side records with the places of the interval tables, and for Ri != 0 the DRI segment in the host's header directly in
// front of SOS -- which makes it the first bytes of the "SOS piece" of the optimal mode's side record (orecs may be NULL).  0, or -1 + error text.
inline int js_export_rst_plan(const JsImage* imgs, const JsnoopExportRestart& rs, const int* images, int n, JsExportRec* recs, JsExportOptRec* orecs, JsExportRstRec* rrecs,
                              uint32_t* unit_base, uint8_t* hdrs, uint8_t* unsupported, uint64_t* ri, uint64_t* total_blocks, uint64_t* total_intervals)
{
    uint64_t units = 0, blocks = 0, ivs = 0;
    for (int k = 0; k < n; k++) {
        const JsImage& im = imgs[images ? images[k] : k];
        JsExportRec& r = recs[k]; JsExportRstRec& rr = rrecs[k];
        ri[k] = js_export_rst_ri(rs, im);
        if (ri[k] > 65535u) unsupported[k] = 1;
        const uint64_t nmcu = (uint64_t)r.nblk / r.bpm;
        rr.itab_off = ivs; rr.ri_blocks = 0u; rr.ni = 1u;
        if (ri[k] && ri[k] <= 65535u) {
            rr.ri_blocks = (uint32_t)ri[k] * r.bpm; rr.ni = (uint32_t)((nmcu + ri[k] - 1u) / ri[k]);
            const uint32_t sos_len = 4u + 1u + 2u * r.ncomp + 3u;
            if (r.hdr_len < sos_len + 2u || r.hdr_len + 6u > JS_EXPORT_HDR_MAX) { js_set_error("export_jpeg: a header of %u bytes", r.hdr_len); return -1; }
            uint8_t* h = hdrs + r.hdr_off; const uint32_t sos = r.hdr_len - sos_len;
            if (h[sos] != 0xFFu || h[sos + 1u] != 0xDAu) { js_set_error("export_jpeg: the header has no SOS at %u", sos); return -1; }
            memmove(h + sos + 6u, h + sos, sos_len);
            h[sos] = 0xFFu; h[sos + 1u] = 0xDDu; h[sos + 2u] = 0u; h[sos + 3u] = 4u; h[sos + 4u] = (uint8_t)(ri[k] >> 8); h[sos + 5u] = (uint8_t)(ri[k] & 255u);
            r.hdr_len += 6u;
            if (orecs) { if (orecs[k].sos_off != sos || orecs[k].sos_len != sos_len) { js_set_error("export_jpeg: the header does not split at %u", sos); return -1; } orecs[k].sos_len += 6u; }
        }
        unit_base[k] = (uint32_t)units; r.blk_base = blocks;
        if (!unsupported[k]) { units += ((uint64_t)r.nblk + JS_EXPORT_TILE - 1u) / JS_EXPORT_TILE; blocks += r.nblk; ivs += rr.ni; }
    }
    unit_base[n] = (uint32_t)units; *total_blocks = blocks; *total_intervals = ivs;
    return 0;
}

// The largest file an entry can become.  Every byte of the un-stuffed stream leaves as itself, an FF with a 00 behind it, and the last byte of an interval but the
// last with a marker of two bytes behind it: header + 2 x bytes + 2 x (NI - 1) + EOI.  (A stuffing chunk of JS_EXPORT_CHUNK bytes by the same count: at most
// 4 x JS_EXPORT_CHUNK, what k_export_stuff_rst stages.)
inline uint64_t js_export_rst_out_cap(uint32_t hdr_len, uint64_t nbytes, uint32_t ni) { return (((uint64_t)hdr_len + 2u * nbytes + 2u * (uint64_t)(ni ? ni - 1u : 0u) + 2u) + 15u) & ~(uint64_t)15u; }

// js_export_layout / js_export_opt_layout for a call with restart intervals.  ent_bits[k]: the length of the entry's un-stuffed stream in bits, every interval
// padded: a multiple of 8, at least one byte an interval and at most the blocks' bits (1658 a block at most, 1665 with own tables) + 7 an interval.
// orecs / hdr_len: NULL without own tables.
inline int js_export_rst_layout(JsExportRec* recs, const JsExportOptRec* orecs, const JsExportRstRec* rrecs, int n, const uint8_t* unsupported, const uint32_t* res, const uint64_t* ent_bits,
                                const uint32_t* hdr_len, uint32_t* chunk_base, int* result, uint32_t* detail, uint64_t* u_bytes, uint64_t* out_bytes)
{
    uint64_t u = 0, o = 0, chunks = 0;
    for (int k = 0; k < n; k++) {
        JsExportRec& r = recs[k];
        result[k] = unsupported[k] ? JSNOOP_EXPORT_UNSUPPORTED : (int)res[k];
        detail[k] = result[k] == JSNOOP_EXPORT_INEXACT ? res[n + 2 * k] : (result[k] == JSNOOP_EXPORT_UNCODABLE ? res[n + 2 * k + 1] : 0u);
        if (result[k] < 0 || result[k] > JSNOOP_EXPORT_UNSUPPORTED) { js_set_error("export_jpeg: entry %d came back with result %d", k, result[k]); return -1; }
        r.live = result[k] == JSNOOP_EXPORT_OK; r.bits = r.live ? ent_bits[k] : 0u;
        chunk_base[k] = (uint32_t)chunks;
        r.u_off = u; r.out_off = o; r.out_cap = 0;
        if (!r.live) continue;
        if (orecs) {
            const uint32_t least = orecs[k].pre_len + orecs[k].sos_len + orecs[k].nslots * 22u, most = orecs[k].pre_len + orecs[k].sos_len + (orecs[k].nslots / 2u) * (33u + 183u);
            if (hdr_len[k] < least || hdr_len[k] > most || most > JS_EXPORT_HDR_MAX) { js_set_error("export_jpeg: entry %d came back with a header of %u bytes (%u .. %u)", k, hdr_len[k], least, most); return -1; }
            r.hdr_len = hdr_len[k]; r.hdr_off = (uint32_t)((size_t)k * JS_EXPORT_OPT_HDR);
        }
        const uint64_t ni = rrecs[k].ni, most_bits = (uint64_t)r.nblk * (orecs ? 1665u : 1658u) + 7u * ni;
        if ((r.bits & 7u) || r.bits < 8u * ni || r.bits > most_bits) { js_set_error("export_jpeg: entry %d came back with %llu bits for %u blocks in %llu intervals", k, (unsigned long long)r.bits, r.nblk, (unsigned long long)ni); return -1; }
        const uint64_t nbytes = r.bits >> 3;
        u += ((nbytes + 15u) & ~(uint64_t)15u) + 16u;
        r.out_cap = js_export_rst_out_cap(r.hdr_len, nbytes, rrecs[k].ni);
        o += r.out_cap;
        chunks += (nbytes + JS_EXPORT_CHUNK - 1u) / JS_EXPORT_CHUNK;
        if (chunks >= 0x7FFFFFFFull) { js_set_error("export_jpeg: more than 2^31 stuffing chunks in one call"); return -1; }
    }
    chunk_base[n] = (uint32_t)chunks; *u_bytes = u; *out_bytes = o;
    return 0;
}
