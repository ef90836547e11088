// jsnoop_carve_check.h -- the host side of jsnoop_carve_run that needs no device: spec import, argument checks, the sizes of lists and scratch, the marker walk
// of the carve contract (ONE function over two callables, "byte at" and "next terminator": k_carve_walk, the host entry jsnoop_carve_host and
// tests/cpp/carve_check.cpp all run this one), records <-> frames and the parent pass.  No device call in here; errors go through js_set_error.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/jsnoop_gpu.h"

void js_set_error(const char* fmt, ...);

#define JS_CARVE_LANE 16u            /* public: JSNOOP_CARVE_LANE */
#define JS_CARVE_WAVE 1024u          /* public: JSNOOP_CARVE_WAVE */
#define JS_CARVE_TILE 16384u         /* public: JSNOOP_CARVE_TILE */
#define JS_CARVE_WALK 256u           /* public: JSNOOP_CARVE_WALK */
#define JS_CARVE_REC_WORDS 16u       /* public: JSNOOP_CARVE_REC_WORDS */
static_assert(JS_CARVE_LANE == JSNOOP_CARVE_LANE && JS_CARVE_WAVE == JSNOOP_CARVE_WAVE && JS_CARVE_TILE == JSNOOP_CARVE_TILE && JS_CARVE_WALK == JSNOOP_CARVE_WALK &&
              JS_CARVE_REC_WORDS == JSNOOP_CARVE_REC_WORDS, "the public seam constants are the kernels'");
#define JS_CARVE_MAX_MARKERS 4096u
#if defined(__HIPCC__)                 /* the walk below is also what k_carve_walk runs */
#define JS_CARVE_HD __host__ __device__
#else
#define JS_CARVE_HD
#endif

struct JsCarveRec { uint32_t w[JS_CARVE_REC_WORDS]; };
static_assert(sizeof(JsCarveRec) == 64, "a record is 64 bytes");

inline void js_carve_spec_defaults(JsnoopCarveSpec* s) { memset(s, 0, sizeof *s); s->struct_size = (uint32_t)sizeof *s; s->max_markers = JS_CARVE_MAX_MARKERS; }
// struct_size is the caller's sizeof(JsnoopCarveSpec), read like JsnoopTuning's: a shorter struct leaves the fields it lacks at their defaults, a longer one is refused
inline int js_carve_import_spec(const JsnoopCarveSpec* in, JsnoopCarveSpec* out)
{
    if (!in) { js_set_error("carve: spec is NULL"); return -1; }
    const uint32_t sz = in->struct_size;
    if (sz < sizeof(uint32_t) || sz > sizeof(JsnoopCarveSpec)) { js_set_error("carve: struct_size %u, this library has %zu", sz, sizeof(JsnoopCarveSpec)); return -1; }
    js_carve_spec_defaults(out); memcpy(out, in, sz); out->struct_size = (uint32_t)sizeof(JsnoopCarveSpec);
    if (!out->max_markers) out->max_markers = JS_CARVE_MAX_MARKERS;
    return 0;
}
inline int js_carve_check_blob(const void* blob, uint64_t len, int where)
{
    if (!blob && len) { js_set_error("carve: blob is NULL"); return -1; }
    if (len >= (1ull << 32)) { js_set_error("carve: a blob of %llu bytes, positions are 32 bits (the reference refuses 4 GB and more too)", (unsigned long long)len); return -1; }
    if (where != 0 && where != 1) { js_set_error("carve: where = %d, 0 is host memory and 1 device memory", where); return -1; }
    return 0;
}

// Tiles are counted from the 16-byte boundary at or below the blob's first byte (head = the bytes between the two): the kernels load whole aligned 16-byte pieces.
// An empty blob has no tile: nothing is read.
inline uint64_t js_carve_tiles(uint64_t len, uint32_t head) { return len ? (len + head + JS_CARVE_TILE - 1u) / JS_CARVE_TILE : 0u; }
// the scratch of one call: counts (two words a tile, then their prefix sums, then the two totals), the lists, the records, and for a host blob its copy
struct JsCarveSizes { uint64_t counts, term_list, cand_list, recs, copy, total; };
inline JsCarveSizes js_carve_sizes(uint64_t len, uint32_t head, uint64_t nterm, uint64_t ncand, int where)
{
    JsCarveSizes s; const uint64_t tiles = js_carve_tiles(len, head);
    s.counts = tiles * 16u + 16u; s.term_list = nterm * 4u; s.cand_list = ncand * 4u; s.recs = ncand * (uint64_t)sizeof(JsCarveRec); s.copy = where == 0 ? len : 0u;
    s.total = s.counts + s.term_list + s.cand_list + s.recs + s.copy;
    return s;
}
inline int js_carve_check_budget(const JsCarveSizes& s, uint64_t budget)
{
    if (s.total > budget) {
        js_set_error("carve: %llu bytes of scratch (lists %llu, records %llu, counts %llu, copy %llu) exceed max_scratch_bytes %llu",
                     (unsigned long long)s.total, (unsigned long long)(s.term_list + s.cand_list), (unsigned long long)s.recs, (unsigned long long)s.counts,
                     (unsigned long long)s.copy, (unsigned long long)budget);
        return -1;
    }
    return 0;
}

JS_CARVE_HD inline bool js_carve_is_sof(uint32_t c) { return c >= 0xC0u && c <= 0xCFu && c != 0xC4u && c != 0xC8u && c != 0xCCu; }

// The walk of one candidate.  at(i): B(i), 0 past the end; next_term(pos): the least terminator >= pos, or UINT64_MAX.  Fills every word of the record.
template <class At, class Next>
JS_CARVE_HD inline void js_carve_walk(uint64_t n, uint32_t p, uint32_t max_markers, At at, Next next_term, JsCarveRec* out)
{
    uint64_t pos = p, end = n, dpos = 0;
    uint32_t markers = 0, scans = 0, seen = 0, status = JSNOOP_CARVE_NO_EOI, reason = 0, dbyte = 0, sof = 0, prec = 0, ncomp = 0, width = 0, height = 0, sos_pos = 0, scan_start = 0;
    for (;;) {
        if (pos >= n) break;
        if (at(pos) != 0xFFu) { status = JSNOOP_CARVE_STOPPED; reason = JSNOOP_CARVE_NOT_A_MARKER; dpos = pos; dbyte = at(pos); break; }
        pos++;
        uint32_t code = at(pos++);
        while (code == 0xFFu) code = at(pos++);
        if (pos > n) break;
        const uint64_t cpos = pos - 1;
        markers++;
        if (markers > max_markers) { status = JSNOOP_CARVE_LIMIT; dpos = cpos; dbyte = code; break; }
        if (code == 0xD8u) { if (markers > 1u) seen |= JSNOOP_CARVE_SEEN_SOI_AGAIN; continue; }
        if (code == 0xD9u) { end = pos; status = scans ? JSNOOP_CARVE_OK : JSNOOP_CARVE_NO_SOS; break; }
        if (code >= 0xD0u && code <= 0xD7u) { status = JSNOOP_CARVE_STOPPED; reason = JSNOOP_CARVE_RST_OUTSIDE_SCAN; dpos = cpos; dbyte = code; break; }
        if (code >= 0xC0u || code == 0x01u) {
            const uint32_t len = at(pos) * 256u + at(pos + 1);
            if (len < 2u) { status = JSNOOP_CARVE_STOPPED; reason = JSNOOP_CARVE_BAD_LENGTH; dpos = pos; dbyte = len; break; }
            if (pos + len > n) break;
            if (!sof && js_carve_is_sof(code)) { sof = code; prec = at(pos + 2); height = at(pos + 3) * 256u + at(pos + 4); width = at(pos + 5) * 256u + at(pos + 6); ncomp = at(pos + 7); }
            if (code == 0xDBu) seen |= JSNOOP_CARVE_SEEN_DQT;
            if (code == 0xC4u) seen |= JSNOOP_CARVE_SEEN_DHT;
            if (code == 0xDDu) seen |= JSNOOP_CARVE_SEEN_DRI;
            if (code == 0xE0u && at(pos + 2) == 'A' && at(pos + 3) == 'V' && at(pos + 4) == 'I' && at(pos + 5) == '1') seen |= JSNOOP_CARVE_SEEN_AVI1;
            pos += len;
            if (code == 0xDAu) {
                if (!scans) { sos_pos = (uint32_t)(cpos - 1); scan_start = (uint32_t)pos; }
                scans++;
                pos = next_term(pos);
                if (pos >= n) break;
            }
            continue;
        }
        status = JSNOOP_CARVE_STOPPED; reason = JSNOOP_CARVE_UNKNOWN_MARKER; dpos = cpos; dbyte = code; break;
    }
    if (status == JSNOOP_CARVE_STOPPED || status == JSNOOP_CARVE_LIMIT) end = dpos;
    uint32_t* w = out->w;
    w[0] = p; w[1] = (uint32_t)end; w[2] = status | reason << 8 | (dbyte & 255u) << 16 | seen << 24; w[3] = (uint32_t)dpos;
    w[4] = sof | prec << 8 | ncomp << 16; w[5] = width | height << 16; w[6] = sos_pos; w[7] = scan_start; w[8] = scans; w[9] = markers;
    for (uint32_t k = 10; k < JS_CARVE_REC_WORDS; k++) w[k] = 0;
}

inline bool js_carve_is_term(const uint8_t* b, uint64_t n, uint64_t i)
{
    if (b[i] != 0xFFu || i + 1 >= n) return false;
    const uint32_t x = b[i + 1];
    return x != 0u && (x & 0xF8u) != 0xD0u;
}
// The two lists and the records of a whole blob, on the host (positions ascending).
inline void js_carve_host_table(const uint8_t* b, uint64_t n, uint32_t max_markers, std::vector<uint32_t>* term, std::vector<uint32_t>* cand, std::vector<JsCarveRec>* recs)
{
    term->clear(); cand->clear();
    for (uint64_t i = 0; i + 1 < n; i++) if (js_carve_is_term(b, n, i)) {
        term->push_back((uint32_t)i);
        if (i + 3 <= n && b[i + 1] == 0xD8u && b[i + 2] == 0xFFu) cand->push_back((uint32_t)i);
    }
    auto at = [&](uint64_t i) -> uint32_t { return i < n ? b[i] : 0u; };
    auto next_term = [&](uint64_t pos) -> uint64_t {
        size_t lo = 0, hi = term->size();
        while (lo < hi) { const size_t mid = (lo + hi) / 2; if ((*term)[mid] < pos) lo = mid + 1; else hi = mid; }
        return lo < term->size() ? (uint64_t)(*term)[lo] : UINT64_MAX;
    };
    recs->resize(cand->size());
    for (size_t k = 0; k < cand->size(); k++) js_carve_walk(n, (*cand)[k], max_markers, at, next_term, &(*recs)[k]);
}

inline void js_carve_frame_of(const JsCarveRec& r, int32_t parent, JsnoopCarveFrame* f)
{
    const uint32_t* w = r.w;
    f->struct_size = (uint32_t)sizeof *f; f->start = w[0]; f->end = w[1]; f->status = (int32_t)(w[2] & 255u); f->reason = (int32_t)(w[2] >> 8 & 255u);
    f->detail_pos = w[3]; f->detail_byte = w[2] >> 16 & 255u; f->seen = w[2] >> 24;
    f->sof_code = w[4] & 255u; f->precision = w[4] >> 8 & 255u; f->components = w[4] >> 16 & 255u; f->width = w[5] & 65535u; f->height = w[5] >> 16;
    f->sos_pos = w[6]; f->scan_start = w[7]; f->scans = w[8]; f->markers = w[9]; f->parent = parent;
}
// parent[k]: the innermost earlier frame with status OK whose [start, end) holds frame k's start, or -1.  Starts ascend, so the OK frames that can still hold a
// later start form a stack: whatever ends at or before this start holds no later one either.
inline void js_carve_parents(const JsCarveRec* recs, size_t n, std::vector<int32_t>* parent)
{
    parent->assign(n, -1);
    std::vector<size_t> open;
    for (size_t k = 0; k < n; k++) {
        const uint32_t start = recs[k].w[0];
        while (!open.empty() && recs[open.back()].w[1] <= start) open.pop_back();
        if (!open.empty()) (*parent)[k] = (int32_t)open.back();
        if ((recs[k].w[2] & 255u) == JSNOOP_CARVE_OK) open.push_back(k);
    }
}
// jsnoop_carve_frame's guarded copy: struct_size 0 = this header's, shorter accepted (no byte past it written), longer refused
inline int js_carve_export_frame(const JsCarveRec& r, int32_t parent, JsnoopCarveFrame* out)
{
    if (!out) { js_set_error("carve_frame: out is NULL"); return -1; }
    const uint32_t want = out->struct_size ? out->struct_size : (uint32_t)sizeof(JsnoopCarveFrame);
    if (want < 8u || want > sizeof(JsnoopCarveFrame)) { js_set_error("carve_frame: struct_size %u, this library has %zu", want, sizeof(JsnoopCarveFrame)); return -1; }
    JsnoopCarveFrame f; js_carve_frame_of(r, parent, &f); f.struct_size = want;
    memcpy(out, &f, want);
    return 0;
}
// which frames jsnoop_job_add_carved adds: -1 + text for a frame outside the blob
inline int js_carve_pick(const JsnoopCarveFrame* frames, int64_t nframes, uint64_t len, int include_no_eoi, std::vector<int64_t>* pick)
{
    pick->clear();
    if (nframes < 0 || (nframes && !frames)) { js_set_error("jsnoop_job_add_carved: bad frame table"); return -1; }
    for (int64_t k = 0; k < nframes; k++) {
        const JsnoopCarveFrame& f = frames[k];
        if (!(f.status == JSNOOP_CARVE_OK || (include_no_eoi && f.status == JSNOOP_CARVE_NO_EOI))) continue;
        if (f.start >= f.end || f.end > len) { js_set_error("jsnoop_job_add_carved: frame %lld [%u, %u) lies outside the blob of %llu bytes", (long long)k, f.start, f.end, (unsigned long long)len); return -1; }
        pick->push_back(k);
    }
    return 0;
}
