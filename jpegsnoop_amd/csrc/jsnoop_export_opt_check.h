// jsnoop_export_opt_check.h -- the host arithmetic jsnoop_batch_export_jpeg_coded adds to jsnoop_export_check.h for JSNOOP_HUFFMAN_OPTIMAL: the coding spec, the
// 2^26-block refusal, the side records (how a header splits around its DHT segments), the call's block and scratch with the pieces the device fills, and the
// second phase's layout with the header lengths the device returned.  No device call in here (tests/cpp/export_opt_check.cpp runs it as a plain host program).
#pragma once
#include "jsnoop_export_check.h"

inline void js_export_coding_defaults(JsnoopExportCoding* c) { memset(c, 0, sizeof *c); c->struct_size = (uint32_t)sizeof *c; c->huffman = JSNOOP_HUFFMAN_ANNEX_K; }
// struct_size read like JsnoopExportSpec's; NULL: the defaults; a huffman value outside the two known ones is refused
inline int js_export_import_coding(const JsnoopExportCoding* in, JsnoopExportCoding* out)
{
    js_export_coding_defaults(out);
    if (!in) return 0;
    const uint32_t sz = in->struct_size;
    if (sz < sizeof(uint32_t) || sz > sizeof(JsnoopExportCoding)) { js_set_error("export_jpeg: coding struct_size %u, this library has %zu", sz, sizeof(JsnoopExportCoding)); return -1; }
    memcpy(out, in, sz); out->struct_size = (uint32_t)sizeof(JsnoopExportCoding);
    if (out->huffman != JSNOOP_HUFFMAN_ANNEX_K && out->huffman != JSNOOP_HUFFMAN_OPTIMAL) { js_set_error("export_jpeg: huffman = %d (0: Annex K, 1: optimal)", out->huffman); return -1; }
    return 0;
}

// A header of js_export_header around its DHT segments: [0, pre_len) ends behind SOF, [sos_off, sos_off + sos_len) is the SOS segment.  0, or -1 + error text
// where the bytes at those places are not the markers they must be.
inline int js_export_opt_split(const uint8_t* hdr, uint32_t hdr_len, uint32_t ncomp, JsExportOptRec* o)
{
    const uint32_t sos_len = 4u + 1u + 2u * ncomp + 3u, dht = (ncomp == 1u ? 1u : 2u) * (33u + 183u);
    if (hdr_len < sos_len + dht + 4u || hdr_len > JS_EXPORT_HDR_MAX) { js_set_error("export_jpeg: a header of %u bytes", hdr_len); return -1; }
    o->sos_len = sos_len; o->sos_off = hdr_len - sos_len; o->pre_len = o->sos_off - dht; o->nslots = ncomp == 1u ? 2u : 4u;
    if (hdr[o->pre_len] != 0xFFu || hdr[o->pre_len + 1u] != 0xC4u || hdr[o->sos_off] != 0xFFu || hdr[o->sos_off + 1u] != 0xDAu) {
        js_set_error("export_jpeg: the header does not split at %u / %u", o->pre_len, o->sos_off); return -1; }
    return 0;
}

// the call's page-locked block: js_export_block's pieces, the side records behind them
struct JsExportOptBlock { JsExportBlock b; size_t orecs; };
inline JsExportOptBlock js_export_opt_block(size_t n)
{
    JsExportOptBlock o; o.b = js_export_block(n);
    o.orecs = o.b.total; o.b.total = (o.b.total + n * sizeof(JsExportOptRec) + 15u) & ~(size_t)15u;
    return o;
}
// the first phase's scratch: js_export_scratch's pieces with the header lengths (one uint32 per entry) among what the first wait brings back
struct JsExportOptScratch { JsExportScratch s; size_t hdr_len; };
inline JsExportOptScratch js_export_opt_scratch(size_t n, uint64_t units, uint64_t blocks)
{
    JsExportOptScratch o; JsExportScratch& s = o.s; size_t at = 0;
    auto take = [&](size_t bytes) { const size_t p = at; at = (at + bytes + 15u) & ~(size_t)15u; return p; };
    s.res = take(n * 12); s.ent_bits = take(n * 8); o.hdr_len = take(n * 4); s.len = take(n * 8); s.back_bytes = at; s.ent_ff = take(n * 8);
    s.unit_bits = take((size_t)units * 4); s.unit_off = take((size_t)units * 8); s.blk_bits = take((size_t)blocks * 2); s.total = at;
    return o;
}
// what the device keeps per entry beside that scratch: the statistics and tables (JsExportOptStat), the code words, the headers
struct JsExportOptKeep { size_t stats, tabs, hdrs, total; };
inline JsExportOptKeep js_export_opt_keep(size_t n)
{
    JsExportOptKeep k; size_t at = 0;
    auto take = [&](size_t bytes) { const size_t p = at; at = (at + bytes + 15u) & ~(size_t)15u; return p; };
    k.stats = take(n * sizeof(JsExportOptStat)); k.tabs = take(n * JS_EXPORT_TABS * 4u); k.hdrs = take(n * JS_EXPORT_OPT_HDR); k.total = at;
    return k;
}

// js_export_plan, then what the mode adds: an entry of JS_EXPORT_OPT_MAX_BLOCKS blocks or more is unsupported (it owns no unit, so the prefix table and the block
// bases are made again), and every entry gets its side record
inline int js_export_opt_plan(const JsImage* imgs, size_t nimg, const JsnoopExportSpec& s, const int* images, int n, js_export_q_fn qfn, void* user,
                              JsExportRec* recs, JsExportOptRec* orecs, uint32_t* unit_base, uint8_t* hdrs, uint8_t* unsupported, uint64_t* total_blocks)
{
    if (js_export_plan(imgs, nimg, s, images, n, qfn, user, recs, unit_base, hdrs, unsupported, total_blocks)) return -1;
    uint64_t units = 0, blocks = 0;
    for (int k = 0; k < n; k++) {
        JsExportRec& r = recs[k];
        if (r.nblk >= JS_EXPORT_OPT_MAX_BLOCKS) unsupported[k] = 1;
        if (js_export_opt_split(hdrs + r.hdr_off, r.hdr_len, r.ncomp, orecs + k)) return -1;
        unit_base[k] = (uint32_t)units; r.blk_base = blocks;
        if (!unsupported[k]) { units += ((uint64_t)r.nblk + JS_EXPORT_TILE - 1u) / JS_EXPORT_TILE; blocks += r.nblk; }
    }
    unit_base[n] = (uint32_t)units; *total_blocks = blocks;
    return 0;
}

// js_export_layout with the header lengths the device returned: an entry that will be written takes its header from the device's own place (entry k:
// JS_EXPORT_OPT_HDR bytes at k * JS_EXPORT_OPT_HDR), its length between the shortest possible (every table one symbol) and the Annex K header's.  A block has at
// least two bits here (a table of one symbol has the code '0') and at most 16 + 11 + 63 * 26.
inline int js_export_opt_layout(JsExportRec* recs, const JsExportOptRec* orecs, int n, const uint8_t* unsupported, const uint32_t* res, const uint64_t* ent_bits, const uint32_t* hdr_len,
                                uint32_t* chunk_base, int* result, uint32_t* detail, uint64_t* u_bytes, uint64_t* out_bytes)
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
        const uint32_t least = orecs[k].pre_len + orecs[k].sos_len + orecs[k].nslots * 22u, most = orecs[k].pre_len + orecs[k].sos_len + (orecs[k].nslots / 2u) * (33u + 183u);
        if (hdr_len[k] < least || hdr_len[k] > most || most > JS_EXPORT_HDR_MAX) { js_set_error("export_jpeg: entry %d came back with a header of %u bytes (%u .. %u)", k, hdr_len[k], least, most); return -1; }
        r.hdr_len = hdr_len[k]; r.hdr_off = (uint32_t)((size_t)k * JS_EXPORT_OPT_HDR);
        if (r.bits < 2u * (uint64_t)r.nblk || r.bits > (uint64_t)r.nblk * 1665u) { js_set_error("export_jpeg: entry %d came back with %llu bits for %u blocks", k, (unsigned long long)r.bits, r.nblk); return -1; }
        const uint64_t nbytes = (r.bits + 7u) >> 3;
        u += ((nbytes + 15u) & ~(uint64_t)15u) + 16u;
        r.out_cap = (((uint64_t)r.hdr_len + 2u * nbytes + 2u) + 15u) & ~(uint64_t)15u;
        o += r.out_cap;
        chunks += (nbytes + JS_EXPORT_CHUNK - 1u) / JS_EXPORT_CHUNK;
        if (chunks >= 0x7FFFFFFFull) { js_set_error("export_jpeg: more than 2^31 stuffing chunks in one call"); return -1; }
    }
    chunk_base[n] = (uint32_t)chunks; *u_bytes = u; *out_bytes = o;
    return 0;
}
