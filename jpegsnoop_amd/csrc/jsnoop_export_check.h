// jsnoop_export_check.h -- the host arithmetic of jsnoop_batch_export_jpeg: spec import, the Annex K code tables, the file header, argument checks, records,
// prefix tables and the sizes of the second phase.  No device call in here (tests/cpp/export_check.cpp runs it as a plain host program); errors go through js_set_error.
#pragma once
#include <stdint.h>
#include <string.h>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_types.h"

void js_set_error(const char* fmt, ...);

static_assert(JS_EXPORT_TILE == JSNOOP_EXPORT_TILE && JS_EXPORT_SCAN == JSNOOP_EXPORT_SCAN && JS_EXPORT_CHUNK == JSNOOP_EXPORT_CHUNK && JS_EXPORT_WINDOW == JSNOOP_EXPORT_WINDOW,
              "the public seam constants are the kernels'");
#define JS_EXPORT_HDR_MAX 1024u      /* SOI 2, APP0 18, 3 x DQT 133, SOF 19, 2 x DHT 33, 2 x DHT 183, SOS 14: 884 at most */
#define JS_EXPORT_TABS 544u          /* words of the code tables: DC0[16] DC1[16] AC0[256] AC1[256] (JS_EXPORT_TAB_WORDS of jsnoop_launch.h) */

// ITU-T T.81 Annex K.3.3, Tables K.3 - K.6: code counts per length and symbols in code order
static const uint8_t kExDcBits[2][16] = { { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 }, { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 } };
static const uint8_t kExAcBits[2][16] = { { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D }, { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77 } };
static const uint8_t kExAcVals[2][162] = { {
    0x01,0x02,0x03,0x00,0x04,0x11,0x05,0x12,0x21,0x31,0x41,0x06,0x13,0x51,0x61,0x07,0x22,0x71,0x14,0x32,0x81,0x91,0xA1,0x08,0x23,0x42,0xB1,0xC1,0x15,0x52,0xD1,0xF0,
    0x24,0x33,0x62,0x72,0x82,0x09,0x0A,0x16,0x17,0x18,0x19,0x1A,0x25,0x26,0x27,0x28,0x29,0x2A,0x34,0x35,0x36,0x37,0x38,0x39,0x3A,0x43,0x44,0x45,0x46,0x47,0x48,0x49,
    0x4A,0x53,0x54,0x55,0x56,0x57,0x58,0x59,0x5A,0x63,0x64,0x65,0x66,0x67,0x68,0x69,0x6A,0x73,0x74,0x75,0x76,0x77,0x78,0x79,0x7A,0x83,0x84,0x85,0x86,0x87,0x88,0x89,
    0x8A,0x92,0x93,0x94,0x95,0x96,0x97,0x98,0x99,0x9A,0xA2,0xA3,0xA4,0xA5,0xA6,0xA7,0xA8,0xA9,0xAA,0xB2,0xB3,0xB4,0xB5,0xB6,0xB7,0xB8,0xB9,0xBA,0xC2,0xC3,0xC4,0xC5,
    0xC6,0xC7,0xC8,0xC9,0xCA,0xD2,0xD3,0xD4,0xD5,0xD6,0xD7,0xD8,0xD9,0xDA,0xE1,0xE2,0xE3,0xE4,0xE5,0xE6,0xE7,0xE8,0xE9,0xEA,0xF1,0xF2,0xF3,0xF4,0xF5,0xF6,0xF7,0xF8,
    0xF9,0xFA }, {
    0x00,0x01,0x02,0x03,0x11,0x04,0x05,0x21,0x31,0x06,0x12,0x41,0x51,0x07,0x61,0x71,0x13,0x22,0x32,0x81,0x08,0x14,0x42,0x91,0xA1,0xB1,0xC1,0x09,0x23,0x33,0x52,0xF0,
    0x15,0x62,0x72,0xD1,0x0A,0x16,0x24,0x34,0xE1,0x25,0xF1,0x17,0x18,0x19,0x1A,0x26,0x27,0x28,0x29,0x2A,0x35,0x36,0x37,0x38,0x39,0x3A,0x43,0x44,0x45,0x46,0x47,0x48,
    0x49,0x4A,0x53,0x54,0x55,0x56,0x57,0x58,0x59,0x5A,0x63,0x64,0x65,0x66,0x67,0x68,0x69,0x6A,0x73,0x74,0x75,0x76,0x77,0x78,0x79,0x7A,0x82,0x83,0x84,0x85,0x86,0x87,
    0x88,0x89,0x8A,0x92,0x93,0x94,0x95,0x96,0x97,0x98,0x99,0x9A,0xA2,0xA3,0xA4,0xA5,0xA6,0xA7,0xA8,0xA9,0xAA,0xB2,0xB3,0xB4,0xB5,0xB6,0xB7,0xB8,0xB9,0xBA,0xC2,0xC3,
    0xC4,0xC5,0xC6,0xC7,0xC8,0xC9,0xCA,0xD2,0xD3,0xD4,0xD5,0xD6,0xD7,0xD8,0xD9,0xDA,0xE2,0xE3,0xE4,0xE5,0xE6,0xE7,0xE8,0xE9,0xEA,0xF2,0xF3,0xF4,0xF5,0xF6,0xF7,0xF8,
    0xF9,0xFA } };

inline void js_export_spec_defaults(JsnoopExportSpec* s) { memset(s, 0, sizeof *s); s->struct_size = (uint32_t)sizeof *s; s->jfif = 1; }
// struct_size is the caller's sizeof(JsnoopExportSpec), read like JsnoopPackSpec's: a shorter struct leaves the fields it lacks at their defaults, a longer one is refused
inline int js_export_import_spec(const JsnoopExportSpec* in, JsnoopExportSpec* out)
{
    if (!in) { js_set_error("export_jpeg: spec is NULL"); return -1; }
    const uint32_t sz = in->struct_size;
    if (sz < sizeof(uint32_t) || sz > sizeof(JsnoopExportSpec)) { js_set_error("export_jpeg: struct_size %u, this library has %zu", sz, sizeof(JsnoopExportSpec)); return -1; }
    js_export_spec_defaults(out); memcpy(out, in, sz); out->struct_size = (uint32_t)sizeof(JsnoopExportSpec);
    return 0;
}

// (length << 16 | code) by symbol (Annex C from the counts): DC0[16] DC1[16] AC0[256] AC1[256]; a symbol without a code stays 0
inline void js_export_code_tabs(uint32_t* tabs)
{
    memset(tabs, 0, JS_EXPORT_TABS * 4u);
    for (int t = 0; t < 2; t++) {
        uint32_t code = 0, k = 0;
        for (uint32_t ln = 1; ln <= 16; ln++) { for (uint32_t i = 0; i < kExDcBits[t][ln - 1]; i++) { tabs[t * 16 + k] = ln << 16 | code; code++; k++; } code <<= 1; }
        code = 0; k = 0;
        for (uint32_t ln = 1; ln <= 16; ln++) { for (uint32_t i = 0; i < kExAcBits[t][ln - 1]; i++) { tabs[32 + t * 256 + kExAcVals[t][k]] = ln << 16 | code; code++; k++; } code <<= 1; }
    }
}

// Everything of the file in front of the entropy-coded data, for the image `im` and its multipliers q[c][natural index].  Returns the length (at most JS_EXPORT_HDR_MAX).
inline uint32_t js_export_header(const JsImage& im, const uint16_t q[3][64], int jfif, uint8_t* out)
{
    static const uint8_t zz[64] = JS_ZIGZAG_NATURAL;
    uint32_t n = 0;
    auto put = [&](uint32_t b) { out[n++] = (uint8_t)b; };
    auto seg = [&](uint32_t marker, uint32_t payload) { put(0xFF); put(marker); put((payload + 2u) >> 8); put((payload + 2u) & 255u); };
    const uint32_t nc = im.ncomp;
    put(0xFF); put(0xD8);
    if (jfif) { seg(0xE0, 14); const uint8_t a[14] = { 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0 }; for (uint8_t b : a) put(b); }
    bool any16 = false;
    for (uint32_t c = 0; c < nc; c++) {
        bool big = false; for (int k = 0; k < 64; k++) big |= q[c][k] > 255u;
        any16 |= big;
        seg(0xDB, big ? 129 : 65); put((big ? 16u : 0u) | c);
        for (int z = 0; z < 64; z++) { const uint32_t v = q[c][zz[z]]; if (big) put(v >> 8); put(v & 255u); }
    }
    seg(any16 ? 0xC1 : 0xC0, 6 + 3 * nc); put(8); put(im.dim_y >> 8); put(im.dim_y & 255u); put(im.dim_x >> 8); put(im.dim_x & 255u); put(nc);
    for (uint32_t c = 0; c < nc; c++) { put(c + 1); put(nc == 1 ? 0x11u : (im.samp_h[c + 1] << 4 | im.samp_v[c + 1])); put(c); }
    for (uint32_t t = 0; t < (nc == 1 ? 1u : 2u); t++) {
        seg(0xC4, 1 + 16 + 12); put(t); for (int i = 0; i < 16; i++) put(kExDcBits[t][i]); for (int i = 0; i < 12; i++) put(i);
        seg(0xC4, 1 + 16 + 162); put(0x10 | t); for (int i = 0; i < 16; i++) put(kExAcBits[t][i]); for (int i = 0; i < 162; i++) put(kExAcVals[t][i]);
    }
    seg(0xDA, 1 + 2 * nc + 3); put(nc);
    for (uint32_t c = 0; c < nc; c++) { put(c + 1); put(c ? 0x11 : 0x00); }
    put(0); put(63); put(0);
    return n;
}

// where the pieces of one call lie in the batch's page-locked block (and in its device copy): records, the two prefix tables, the code tables, the headers
struct JsExportBlock { size_t recs, unit_base, chunk_base, tabs, hdrs, total; };
inline JsExportBlock js_export_block(size_t n)
{
    JsExportBlock b; size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 15u) & ~(size_t)15u; return o; };
    b.recs = take(n * sizeof(JsExportRec)); b.unit_base = take((n + 1) * 4); b.chunk_base = take((n + 1) * 4); b.tabs = take(JS_EXPORT_TABS * 4u);
    b.hdrs = take(n * JS_EXPORT_HDR_MAX); b.total = at;
    return b;
}
// ... and the device scratch of the first phase: what comes back to the host in front ([n] result, [n][2] lowest block per kind, [n] bits, [n] file lengths)
struct JsExportScratch { size_t res, ent_bits, len, ent_ff, back_bytes, unit_bits, unit_off, blk_bits, total; };
inline JsExportScratch js_export_scratch(size_t n, uint64_t units, uint64_t blocks)
{
    JsExportScratch s; size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 15u) & ~(size_t)15u; return o; };
    s.res = take(n * 12); s.ent_bits = take(n * 8); s.len = take(n * 8); s.back_bytes = at; s.ent_ff = take(n * 8);
    s.unit_bits = take((size_t)units * 4); s.unit_off = take((size_t)units * 8); s.blk_bits = take((size_t)blocks * 2); s.total = at;
    return s;
}

// q of component comp of image i, natural order -> out64; 0 / -1 + error text
typedef int (*js_export_q_fn)(void* user, int i, int comp, uint16_t* out64);

// Checks every argument of one call and fills recs[n], unit_base[n + 1] and the headers (entry k: JS_EXPORT_HDR_MAX bytes at hdrs + k * JS_EXPORT_HDR_MAX).
// unsupported[k] = 1 where the host decides JSNOOP_EXPORT_UNSUPPORTED (such an entry owns no unit).  0, or -1 + error text.
inline int js_export_plan(const JsImage* imgs, size_t nimg, const JsnoopExportSpec& s, const int* images, int n, js_export_q_fn qfn, void* user,
                          JsExportRec* recs, uint32_t* unit_base, uint8_t* hdrs, uint8_t* unsupported, uint64_t* total_blocks)
{
    uint64_t units = 0, blocks = 0;
    for (int k = 0; k < n; k++) {
        const int i = images ? images[k] : k;
        if (i < 0 || (size_t)i >= nimg) { js_set_error("export_jpeg: image index %d (entry %d) out of range, the batch holds %zu", i, k, nimg); return -1; }
        const JsImage& im = imgs[i];
        if (im.ncomp != 1u && im.ncomp != 3u) { js_set_error("export_jpeg: image %d has %u components", i, im.ncomp); return -1; }
        if (!im.blk_per_mcu || im.blk_per_mcu > JS_MAX_BLK_PER_MCU || !im.mcu_xmax || !im.mcu_ymax || (uint64_t)im.mcu_xmax * im.mcu_ymax * im.blk_per_mcu != im.total_blocks) {
            js_set_error("export_jpeg: image %d has no decoded geometry", i); return -1; }
        JsExportRec& r = recs[k];
        memset(&r, 0, sizeof r);
        r.coef_off = im.coef_off; r.blk_base = blocks; r.nblk = im.total_blocks; r.bpm = im.blk_per_mcu; r.ncomp = im.ncomp;
        uint32_t count[4] = { 0, 0, 0, 0 }, seen[4] = { 0, 0, 0, 0 };
        for (uint32_t j = 0; j < im.blk_per_mcu; j++) {
            if (im.blk_comp[j] < 1u || im.blk_comp[j] > im.ncomp) { js_set_error("export_jpeg: unexpected block order inside the MCU of image %d", i); return -1; }
            count[im.blk_comp[j]]++;
        }
        for (uint32_t j = 0; j < im.blk_per_mcu; j++) {
            const uint32_t c = im.blk_comp[j];
            r.comp[j] = (uint8_t)(c - 1u);
            if (seen[c]) { if (im.blk_comp[j - 1] != c) { js_set_error("export_jpeg: unexpected block order inside the MCU of image %d", i); return -1; } r.back[j] = 1; }
            else r.back[j] = (uint8_t)(im.blk_per_mcu - (count[c] - 1u));
            seen[c]++;
        }
        for (uint32_t c = 0; c < im.ncomp; c++) if (qfn(user, i, (int)c, r.q[c])) return -1;
        unsupported[k] = im.precision != 8u;
        r.hdr_off = (uint32_t)((size_t)k * JS_EXPORT_HDR_MAX);
        r.hdr_len = js_export_header(im, r.q, s.jfif != 0, hdrs + r.hdr_off);
        unit_base[k] = (uint32_t)units;
        if (!unsupported[k]) { units += ((uint64_t)r.nblk + JS_EXPORT_TILE - 1u) / JS_EXPORT_TILE; blocks += r.nblk; }
        if (units >= 0x7FFFFFFFull) { js_set_error("export_jpeg: more than 2^31 tiles of blocks in one call"); return -1; }
    }
    unit_base[n] = (uint32_t)units; *total_blocks = blocks;
    return 0;
}

// Second phase: from the result words and the bit lengths of the first, which entries are written (live), where their un-stuffed streams and their files lie
// and how many stuffing chunks each owns.  A file's place is sized for the worst case of the stuffing (every byte FF): header + 2 x stream + EOI.
// result[k] / detail[k]: what jsnoop_batch_export_file reports.  0, or -1 + error text.
inline int js_export_layout(JsExportRec* recs, int n, const uint8_t* unsupported, const uint32_t* res /*[n] result, [n][2] lowest block*/, const uint64_t* ent_bits,
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
        if (r.bits < 6u || r.bits > (uint64_t)r.nblk * 1658u) { js_set_error("export_jpeg: entry %d came back with %llu bits for %u blocks", k, (unsigned long long)r.bits, r.nblk); return -1; }
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
