// jsnoop_export_prog_check.h -- the host arithmetic jsnoop_batch_export_jpeg_prog adds to the export's other check headers: the progressive spec and its
// refusals, the scan script's rules, the default scripts, the record of every (entry, scan) with the map from a unit to its arena block, the header pieces, the
// prefix tables over (entry, scan, tile), the second phase's layout with the worst-case size of a file, and the two operators that resolve end-of-band runs
// (the same functions, compiled for the device too).  No device call in here (tests/cpp/export_prog_check.cpp runs it as a plain host program).
// The definition of the file: tests/export_prog_model.py; the contract: DESIGN.md section 4.17.
#pragma once
#include "jsnoop_export_rst_check.h"

// ---- end-of-band runs.  In an AC scan a unit is EMPTY (no level in its band), TAIL (symbols, and the band ends in zeros) or FULL.  A run is a TAIL unit or an
// EMPTY unit at an interval start or behind a FULL unit, and the EMPTY units that follow it inside the interval.  The unit with index i in its run carries an
// EOBn when i % 32767 == 0, of min(32767, length - i).  Index and length come from two segmented scans:
//   forward   JsRunFwd (cnt, cut, tail): a cut is a unit with symbols (the cut lies AT it, it counts 0) or an interval start (the cut lies in FRONT of the unit,
//             it counts 1).  combine(a, b) = b where b has a cut, else (a.cnt + b.cnt, a.cut, a.tail).  The index of an EMPTY unit is cnt - 1 + tail of the
//             inclusive scan; of a TAIL unit 0.  Associative: in (a b) c and a (b c) alike the result is c where c has a cut; else b's with c.cnt added where b
//             has one; else a's with b.cnt + c.cnt added -- the last cut wins and counts add behind it.
//   backward  JsRunBwd (lead, open): the EMPTY units at the front of a stretch up to its first stop -- a unit with symbols (lead 0) or the last unit of an
//             interval (lead 1 where EMPTY) --, open where there is no stop.  combine(a, b) = (a.lead + b.lead, b.open) where a is open, else a.  The EMPTY units
//             that follow unit u are the lead of the stretch behind u, or 0 where u ends an interval.  Associative: the result is a's where a is not open; else
//             b's with a.lead added where b is not open; else (a.lead + b.lead + c.lead, c.open) -- the first stop wins and counts add in front of it.
#define JS_PROG_EMPTY 0u
#define JS_PROG_TAIL  1u
#define JS_PROG_FULL  2u
#define JS_PROG_EOB_MAX 32767u
JS_RST_HD JsRunFwd js_run_fwd_identity() { JsRunFwd s; s.cnt = 0u; s.cut = 0u; s.tail = 0u; return s; }
JS_RST_HD JsRunFwd js_run_fwd_leaf(uint32_t cls, bool starts)
{
    JsRunFwd s; s.cnt = cls == JS_PROG_EMPTY ? 1u : 0u; s.cut = (cls != JS_PROG_EMPTY || starts) ? 1u : 0u; s.tail = cls == JS_PROG_TAIL ? 1u : 0u;
    return s;
}
JS_RST_HD JsRunFwd js_run_fwd_combine(const JsRunFwd& a, const JsRunFwd& b)
{
    JsRunFwd s; s.cnt = b.cut ? b.cnt : a.cnt + b.cnt; s.cut = b.cut ? 1u : a.cut; s.tail = b.cut ? b.tail : a.tail;
    return s;
}
JS_RST_HD JsRunBwd js_run_bwd_identity() { JsRunBwd s; s.lead = 0u; s.open = 1u; return s; }
JS_RST_HD JsRunBwd js_run_bwd_leaf(uint32_t cls, bool ends)
{
    JsRunBwd s; s.lead = cls == JS_PROG_EMPTY ? 1u : 0u; s.open = (cls == JS_PROG_EMPTY && !ends) ? 1u : 0u;
    return s;
}
JS_RST_HD JsRunBwd js_run_bwd_combine(const JsRunBwd& a, const JsRunBwd& b)
{
    JsRunBwd s; s.lead = a.open ? a.lead + b.lead : a.lead; s.open = a.open ? b.open : 0u;
    return s;
}
// does the unit carry an EOBn (incl: the inclusive forward scan at the unit)
JS_RST_HD bool js_run_carries(uint32_t cls, const JsRunFwd& incl) { return cls == JS_PROG_TAIL || (cls == JS_PROG_EMPTY && (incl.cnt - 1u + incl.tail) % JS_PROG_EOB_MAX == 0u); }
// ... and of how many blocks (behind: the backward scan of everything behind the unit)
JS_RST_HD uint32_t js_run_length(bool ends, const JsRunBwd& behind) { const uint32_t n = 1u + (ends ? 0u : behind.lead); return n < JS_PROG_EOB_MAX ? n : JS_PROG_EOB_MAX; }

// unit u of a scan -> the block of the entry's arena
JS_RST_HD uint32_t js_prog_block(const JsExportScanRec& r, uint32_t u)
{
    if (!r.single) return (u / r.spm) * r.bpm + r.pos[u % r.spm];
    const uint32_t by = u / r.w, bx = u % r.w;
    return ((by / r.V) * r.mcu_x + bx / r.H) * r.bpm + r.base + (by % r.V) * r.H + bx % r.H;
}
JS_RST_HD bool js_prog_ends(const JsExportScanRec& r, uint32_t u) { return u + 1u == r.nunits || (r.ri && (u + 1u) % r.ri == 0u); }
JS_RST_HD bool js_prog_starts(const JsExportScanRec& r, uint32_t u) { return u == 0u || (r.ri && u % r.ri == 0u); }

// ---- the spec
inline void js_export_progressive_defaults(JsnoopExportProgressive* p) { memset(p, 0, sizeof *p); p->struct_size = (uint32_t)sizeof *p; p->mode = JSNOOP_PROGRESSIVE_OFF; }
// struct_size read like JsnoopExportSpec's; NULL: the defaults
inline int js_export_import_progressive(const JsnoopExportProgressive* in, JsnoopExportProgressive* out)
{
    js_export_progressive_defaults(out);
    if (!in) return 0;
    const uint32_t sz = in->struct_size;
    if (sz < sizeof(uint32_t) || sz > sizeof(JsnoopExportProgressive)) { js_set_error("export_jpeg: progressive struct_size %u, this library has %zu", sz, sizeof(JsnoopExportProgressive)); return -1; }
    memcpy(out, in, sz); out->struct_size = (uint32_t)sizeof(JsnoopExportProgressive);
    if (out->mode < JSNOOP_PROGRESSIVE_OFF || out->mode > JSNOOP_PROGRESSIVE_SCRIPT) { js_set_error("export_jpeg: progressive mode = %d (0: off, 1: the default script, 2: a script)", out->mode); return -1; }
    if (out->reserved) { js_set_error("export_jpeg: progressive reserved = %u, must be 0", out->reserved); return -1; }
    if (out->mode != JSNOOP_PROGRESSIVE_SCRIPT && (out->nscans || out->scans)) { js_set_error("export_jpeg: progressive mode %d takes no script", out->mode); return -1; }
    if (out->mode == JSNOOP_PROGRESSIVE_SCRIPT && (!out->scans || !out->nscans || out->nscans > JSNOOP_EXPORT_MAX_SCANS)) {
        js_set_error("export_jpeg: a script of %u scans at %s (1 .. %u)", out->nscans, out->scans ? "its place" : "NULL", JSNOOP_EXPORT_MAX_SCANS); return -1; }
    return 0;
}
inline uint32_t js_prog_kind(const JsnoopExportScan& s) { return s.ss ? JS_PROG_AC_FIRST : (s.ah ? JS_PROG_DC_REFINE : JS_PROG_DC_FIRST); }
// The rules of a script (structure, then progression).  *ncomp: 1 or 3, the images it can write.  0, or -1 + error text naming scan and rule.
inline int js_export_prog_validate(const JsnoopExportScan* s, uint32_t n, uint32_t* ncomp)
{
    if (!s || !n || n > JSNOOP_EXPORT_MAX_SCANS) { js_set_error("export_jpeg: a script of %u scans (1 .. %u)", n, JSNOOP_EXPORT_MAX_SCANS); return -1; }
    uint32_t all = 0;
    for (uint32_t i = 0; i < n; i++) {
        const JsnoopExportScan& c = s[i];
        if (c.reserved[0] || c.reserved[1] || c.reserved[2]) { js_set_error("export_jpeg: scan %u: reserved bytes must be 0", i); return -1; }
        if (!c.comps || (c.comps & 0xF8u)) { js_set_error("export_jpeg: scan %u: comps = 0x%02X (bits 0 .. 2, at least one)", i, c.comps); return -1; }
        if (c.ss > c.se || c.se > 63u) { js_set_error("export_jpeg: scan %u: Ss %u, Se %u (Ss <= Se <= 63)", i, c.ss, c.se); return -1; }
        if (c.al > 13u) { js_set_error("export_jpeg: scan %u: Al %u (0 .. 13)", i, c.al); return -1; }
        if (c.ss == 0u && c.se != 0u) { js_set_error("export_jpeg: scan %u: a DC scan has Ss = Se = 0, not Se %u", i, c.se); return -1; }
        if (c.ss != 0u && (c.comps & (c.comps - 1u))) { js_set_error("export_jpeg: scan %u: an AC scan names exactly one component", i); return -1; }
        if (c.ss != 0u && (c.ah || c.al)) { js_set_error("export_jpeg: scan %u: AC successive approximation (Ah %u, Al %u) is not written", i, c.ah, c.al); return -1; }
        if (c.ss == 0u && c.ah && c.al + 1u != c.ah) { js_set_error("export_jpeg: scan %u: a DC refinement has Al = Ah - 1, not Ah %u, Al %u", i, c.ah, c.al); return -1; }
        all |= c.comps;
    }
    if (all != 1u && all != 7u) { js_set_error("export_jpeg: the script names components 0x%02X (component 0, or 0, 1 and 2)", all); return -1; }
    int al[3] = { -1, -1, -1 }; uint64_t seen[3] = { 0, 0, 0 };
    for (uint32_t i = 0; i < n; i++) {
        const JsnoopExportScan& c = s[i];
        for (uint32_t k = 0; k < 3u; k++) if (c.comps >> k & 1u) {
            if (c.ss == 0u) {
                if (al[k] < 0 ? c.ah != 0u : (al[k] == 0 || (int)c.ah != al[k])) { js_set_error("export_jpeg: scan %u: component %u's DC has Ah %u where %d is next", i, k, c.ah, al[k] < 0 ? 0 : al[k]); return -1; }
                al[k] = (int)c.al;
            } else {
                if (al[k] < 0) { js_set_error("export_jpeg: scan %u: an AC scan of component %u in front of its first DC scan", i, k); return -1; }
                const uint64_t band = ((c.se == 63u ? 0ull : 1ull << (c.se + 1u)) - (1ull << c.ss));
                if (seen[k] & band) { js_set_error("export_jpeg: scan %u: component %u's band %u .. %u is coded twice", i, k, c.ss, c.se); return -1; }
                seen[k] |= band;
            }
        }
    }
    for (uint32_t k = 0; k < (all == 1u ? 1u : 3u); k++) {
        if (al[k] != 0) { js_set_error("export_jpeg: component %u's DC ends at Al %d, not 0", k, al[k]); return -1; }
        if (seen[k] != 0xFFFFFFFFFFFFFFFEull) { js_set_error("export_jpeg: component %u's AC indices are not all coded (0x%016llX)", k, (unsigned long long)seen[k]); return -1; }
    }
    *ncomp = all == 1u ? 1u : 3u;
    return 0;
}
// the built-in script for images of ncomp components (6 or 4 scans) -> out; returns their number
inline uint32_t js_export_prog_default(uint32_t ncomp, JsnoopExportScan* out)
{
    static const uint8_t three[6][5] = { { 7, 0, 0, 0, 1 }, { 1, 1, 5, 0, 0 }, { 2, 1, 63, 0, 0 }, { 4, 1, 63, 0, 0 }, { 1, 6, 63, 0, 0 }, { 7, 0, 0, 1, 0 } };
    static const uint8_t one[4][5] = { { 1, 0, 0, 0, 1 }, { 1, 1, 5, 0, 0 }, { 1, 6, 63, 0, 0 }, { 1, 0, 0, 1, 0 } };
    const uint32_t n = ncomp == 1u ? 4u : 6u;
    for (uint32_t i = 0; i < n; i++) {
        const uint8_t* v = ncomp == 1u ? one[i] : three[i];
        memset(out + i, 0, sizeof out[i]); out[i].comps = v[0]; out[i].ss = v[1]; out[i].se = v[2]; out[i].ah = v[3]; out[i].al = v[4];
    }
    return n;
}

// The record of scan `sc` (number si) of an image: geometry, units, the map.  ri_mode / interval: the imported restart spec.  Returns the scan's Ri in units of
// its own (above 65535: the entry is unsupported; the record's ri / ni are then not set).
inline uint64_t js_export_prog_scan_rec(const JsImage& im, const JsnoopExportScan& sc, uint32_t si, const JsnoopExportRestart& rs, JsExportScanRec* r)
{
    memset(r, 0, sizeof *r);
    r->scan = si; r->kind = js_prog_kind(sc); r->ss = sc.ss; r->se = sc.se; r->al = sc.al; r->bpm = im.blk_per_mcu;
    uint32_t per_row;
    const bool one = (sc.comps & (sc.comps - 1u)) == 0u;
    uint32_t c0 = 0; while (!(sc.comps >> c0 & 1u)) c0++;
    r->comp0 = c0;
    if (one && im.ncomp == 3u) {
        uint32_t hmax = 1, vmax = 1;
        for (uint32_t c = 1; c <= 3u; c++) { hmax = im.samp_h[c] > hmax ? im.samp_h[c] : hmax; vmax = im.samp_v[c] > vmax ? im.samp_v[c] : vmax; }
        r->single = 1u; r->H = im.samp_h[c0 + 1u]; r->V = im.samp_v[c0 + 1u]; r->mcu_x = im.mcu_xmax;
        r->w = ((im.dim_x * r->H + hmax - 1u) / hmax + 7u) / 8u; const uint32_t h = ((im.dim_y * r->V + vmax - 1u) / vmax + 7u) / 8u;
        while (r->base < im.blk_per_mcu && im.blk_comp[r->base] != c0 + 1u) r->base++;
        r->spm = 1u; r->nunits = r->w * h; r->comp[0] = (uint8_t)c0; r->slot[0] = 0; r->back[0] = 1; per_row = r->w;
    } else {
        uint32_t count[3] = { 0, 0, 0 }, rank[3] = { 0, 0, 0 }, k = 0;
        for (uint32_t c = 0; c < 3u; c++) if (sc.comps >> c & 1u) rank[c] = k++;
        for (uint32_t j = 0; j < im.blk_per_mcu; j++) { const uint32_t c = im.blk_comp[j] - 1u; if (sc.comps >> c & 1u) count[c]++; }
        uint32_t seen[3] = { 0, 0, 0 };
        for (uint32_t j = 0; j < im.blk_per_mcu; j++) {
            const uint32_t c = im.blk_comp[j] - 1u;
            if (!(sc.comps >> c & 1u)) continue;
            r->pos[r->spm] = (uint8_t)j; r->comp[r->spm] = (uint8_t)c; r->slot[r->spm] = (uint8_t)rank[c];
            r->spm++;
        }
        for (uint32_t p = 0; p < r->spm; p++) { const uint32_t c = r->comp[p]; r->back[p] = (uint8_t)(seen[c] ? 1u : r->spm - (count[c] - 1u)); seen[c]++; }
        r->nunits = im.mcu_xmax * im.mcu_ymax * r->spm; per_row = im.mcu_xmax;
    }
    r->ntab = r->kind == JS_PROG_DC_FIRST ? (one ? 1u : (uint32_t)__builtin_popcount(sc.comps)) : (r->kind == JS_PROG_AC_FIRST ? 1u : 0u);
    uint64_t ri = 0;
    switch (rs.mode) {
    case JSNOOP_RESTART_MCUS: ri = rs.interval; break;
    case JSNOOP_RESTART_ROWS: ri = (uint64_t)rs.interval * per_row; break;
    case JSNOOP_RESTART_SOURCE: ri = im.rst_en ? im.rst_interval : 0u; break;
    default: break;
    }
    if (ri <= 65535u) {
        const uint64_t groups = r->nunits / r->spm;
        r->ri = (uint32_t)ri * r->spm; r->ni = ri ? (uint32_t)((groups + ri - 1u) / ri) : 1u;
    }
    return ri;
}
// the SOS segment of a scan (and DRI in front of it where `dri`): at most JS_PROG_POST bytes -> out; returns the length
inline uint32_t js_export_prog_post(const JsnoopExportScan& sc, bool dri, uint32_t ri, uint8_t* out)
{
    uint32_t n = 0, ns = (uint32_t)__builtin_popcount(sc.comps), k = 0;
    if (dri) { out[n++] = 0xFF; out[n++] = 0xDD; out[n++] = 0; out[n++] = 4; out[n++] = (uint8_t)(ri >> 8); out[n++] = (uint8_t)ri; }
    out[n++] = 0xFF; out[n++] = 0xDA; out[n++] = 0; out[n++] = (uint8_t)(6u + 2u * ns); out[n++] = (uint8_t)ns;
    for (uint32_t c = 0; c < 3u; c++) if (sc.comps >> c & 1u) { out[n++] = (uint8_t)(c + 1u); out[n++] = (uint8_t)((sc.ss == 0u && sc.ah == 0u) ? k << 4 : 0u); k++; }
    out[n++] = sc.ss; out[n++] = sc.se; out[n++] = (uint8_t)(sc.ah << 4 | sc.al);
    return n;
}

// the call's page-locked block: js_export_block's pieces (the entries' records, the entries' prefix table over SCAN RECORDS in unit_base, the headers up to SOF),
// then the scan records, their prefix tables over tiles and chunks, the entry of every scan record, and the post pieces
struct JsExportProgBlock { JsExportBlock b; size_t srecs, tile_base, chunk_base, posts; };
inline JsExportProgBlock js_export_prog_block(size_t n, size_t nrec)
{
    JsExportProgBlock p; p.b = js_export_block(n);
    size_t at = p.b.total;
    auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 15u) & ~(size_t)15u; return o; };
    p.srecs = take(nrec * sizeof(JsExportScanRec)); p.tile_base = take((nrec + 1) * 4); p.chunk_base = take((nrec + 1) * 4); p.posts = take(nrec * JS_PROG_POST); p.b.total = at;
    return p;
}
// the device scratch: what the first wait brings back in front ([n] result, [n][2] lowest block, [nrec] stream bits, [nrec] header lengths), what the second brings
// back behind it ([n] file lengths, [nrec] where the scan's piece starts in the file, [nrec] FF bytes of the scan), then per-tile, per-unit and per-interval pieces
struct JsExportProgScratch { size_t res, rec_bits, hdr_len, back1, len, scan_out, rec_ff, back2, sums, tile_off, blk_bits, eob, cls, itab, total; };
inline JsExportProgScratch js_export_prog_scratch(size_t n, size_t nrec, uint64_t tiles, uint64_t units, uint64_t intervals)
{
    JsExportProgScratch s; size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at = (at + bytes + 15u) & ~(size_t)15u; return o; };
    s.res = take(n * 12); s.rec_bits = take(nrec * 8); s.hdr_len = take(nrec * 4); s.back1 = at;
    s.len = take(n * 8); s.scan_out = take(nrec * 8); s.rec_ff = take(nrec * 8); s.back2 = at;
    s.sums = take((size_t)tiles * sizeof(JsRstSum)); s.tile_off = take((size_t)tiles * 8); s.blk_bits = take((size_t)units * 2); s.eob = take((size_t)units * 2);
    s.cls = take((size_t)units); s.itab = take((size_t)intervals * 8); s.total = at;
    return s;
}
// what the device keeps per scan record: counts and tables (JsExportScanStat), code words, header pieces
struct JsExportProgKeep { size_t stats, tabs, hdrs, total; };
inline JsExportProgKeep js_export_prog_keep(size_t nrec)
{
    JsExportProgKeep k; size_t at = 0;
    auto take = [&](size_t bytes) { const size_t p = at; at = (at + bytes + 15u) & ~(size_t)15u; return p; };
    k.stats = take(nrec * sizeof(JsExportScanStat)); k.tabs = take(nrec * JS_PROG_TAB_WORDS * 4u); k.hdrs = take(nrec * JS_PROG_HDR); k.total = at;
    return k;
}

// How many scan records a call needs (an unsupported entry owns none), and which entries this mode refuses beyond js_export_plan's precision test (flags[k] = 1):
// the script's component count differs from the image's, 2^26 blocks or more, an Ri above 65535 in some scan.  script3 / script1: the script for images of
// three / one component (NULL: none fits).  0, or -1 + error text for an image index out of range.
inline int js_export_prog_count(const JsImage* imgs, size_t nimg, const int* images, int n, const JsnoopExportRestart& rs, const JsnoopExportScan* script3, uint32_t n3,
                                const JsnoopExportScan* script1, uint32_t n1, uint8_t* flags, size_t* nrec_out)
{
    size_t nrec = 0; JsExportScanRec tmp;
    for (int k = 0; k < n; k++) {
        const int i = images ? images[k] : k;
        if (i < 0 || (size_t)i >= nimg) { js_set_error("export_jpeg: image index %d (entry %d) out of range, the batch holds %zu", i, k, nimg); return -1; }
        const JsImage& im = imgs[i];
        const JsnoopExportScan* s = im.ncomp == 1u ? script1 : script3; const uint32_t ns = im.ncomp == 1u ? n1 : n3;
        flags[k] = (!s || (im.ncomp != 1u && im.ncomp != 3u) || im.total_blocks >= JS_EXPORT_OPT_MAX_BLOCKS || !im.blk_per_mcu || im.blk_per_mcu > JS_MAX_BLK_PER_MCU) ? 1 : 0;
        for (uint32_t j = 0; j < ns && !flags[k]; j++) if (js_export_prog_scan_rec(im, s[j], j, rs, &tmp) > 65535u) flags[k] = 1;
        if (!flags[k] && im.precision == 8u) nrec += ns;
    }
    *nrec_out = nrec;
    return 0;
}
// Fills the scan records, the prefix tables (recs' table over scan records in rec_base[n + 1], tiles in tile_base[nrec + 1]), the pre pieces (the entry's header
// of js_export_plan cut behind SOF, its marker turned into FF C2) and the post pieces.  0, or -1 + error text.
inline int js_export_prog_plan(const JsImage* imgs, const int* images, int n, const JsnoopExportRestart& rs, const JsnoopExportScan* script3, uint32_t n3,
                               const JsnoopExportScan* script1, uint32_t n1, JsExportRec* recs, const uint8_t* unsupported, uint8_t* hdrs, uint32_t posts_off /*from hdrs' base*/,
                               JsExportScanRec* srecs, uint32_t* rec_base, uint32_t* tile_base, uint64_t* total_units, uint64_t* total_intervals)
{
    uint64_t tiles = 0, units = 0, ivs = 0; uint32_t nrec = 0;
    for (int k = 0; k < n; k++) {
        const JsImage& im = imgs[images ? images[k] : k];
        JsExportRec& r = recs[k];
        rec_base[k] = nrec;
        if (unsupported[k]) continue;
        const JsnoopExportScan* s = im.ncomp == 1u ? script1 : script3; const uint32_t ns = im.ncomp == 1u ? n1 : n3;
        JsExportOptRec split;
        if (js_export_opt_split(hdrs + r.hdr_off, r.hdr_len, r.ncomp, &split)) return -1;
        const uint32_t sof = split.pre_len - (10u + 3u * r.ncomp);
        uint8_t* h = hdrs + r.hdr_off;
        if (h[sof] != 0xFFu || (h[sof + 1u] != 0xC0u && h[sof + 1u] != 0xC1u)) { js_set_error("export_jpeg: the header has no SOF at %u", sof); return -1; }
        h[sof + 1u] = 0xC2u;
        uint64_t prev_ri = 0;
        for (uint32_t i = 0; i < ns; i++, nrec++) {
            JsExportScanRec& p = srecs[nrec];
            const uint64_t ri = js_export_prog_scan_rec(im, s[i], i, rs, &p);
            p.entry = (uint32_t)k; p.ubase = units; p.itab_off = ivs;
            p.pre_off = r.hdr_off; p.pre_len = i ? 0u : split.pre_len;
            p.post_off = posts_off + nrec * JS_PROG_POST; p.post_len = js_export_prog_post(s[i], ri != prev_ri, (uint32_t)ri, hdrs + p.post_off);
            prev_ri = ri;
            tile_base[nrec] = (uint32_t)tiles;
            tiles += ((uint64_t)p.nunits + JS_EXPORT_TILE - 1u) / JS_EXPORT_TILE; units += p.nunits; ivs += p.ni;
            if (tiles >= 0x7FFFFFFFull) { js_set_error("export_jpeg: more than 2^31 tiles of blocks in one call"); return -1; }
        }
    }
    rec_base[n] = nrec; tile_base[nrec] = (uint32_t)tiles; *total_units = units; *total_intervals = ivs;
    return 0;
}

// The largest file an entry can become: per scan its header piece, and of its un-stuffed stream every byte as itself, an FF with a 00 behind it, the last byte of
// an interval but the last with a marker behind it (js_export_rst_out_cap's count, without its EOI and rounding); then EOI.
inline uint64_t js_export_prog_scan_cap(uint32_t hdr_len, uint64_t nbytes, uint32_t ni) { return (uint64_t)hdr_len + 2u * nbytes + 2u * (uint64_t)(ni ? ni - 1u : 0u); }

// The second phase's layout from what the first wait brought back.  An entry is live where its result is OK; its scans' streams follow each other in the
// un-stuffed memory (each starts on 16 bytes), chunk_base[nrec + 1] counts stuffing chunks per scan record.  A scan's stream is a multiple of 8 bits, at least a
// byte an interval, at most 1668 bits a unit (63 x 26 and an EOB14 of 30) + 7 an interval; its header piece at most JS_PROG_HDR.
inline int js_export_prog_layout(JsExportRec* recs, JsExportScanRec* srecs, const uint32_t* rec_base, int n, const uint8_t* unsupported, const uint32_t* res, const uint64_t* rec_bits,
                                 const uint32_t* hdr_len, uint32_t* chunk_base, int* result, uint32_t* detail, uint64_t* u_bytes, uint64_t* out_bytes)
{
    uint64_t u = 0, o = 0, chunks = 0;
    for (int k = 0; k < n; k++) {
        JsExportRec& r = recs[k];
        result[k] = unsupported[k] ? JSNOOP_EXPORT_UNSUPPORTED : (int)res[k];
        detail[k] = result[k] == JSNOOP_EXPORT_INEXACT ? res[n + 2 * k] : (result[k] == JSNOOP_EXPORT_UNCODABLE ? res[n + 2 * k + 1] : 0u);
        if (result[k] < 0 || result[k] > JSNOOP_EXPORT_UNSUPPORTED) { js_set_error("export_jpeg: entry %d came back with result %d", k, result[k]); return -1; }
        r.live = result[k] == JSNOOP_EXPORT_OK; r.bits = 0; r.u_off = u; r.out_off = o; r.out_cap = 0;
        uint64_t cap = 2;
        for (uint32_t i = rec_base[k]; i < rec_base[k + 1]; i++) {
            JsExportScanRec& p = srecs[i];
            chunk_base[i] = (uint32_t)chunks;
            p.live = r.live; p.bits = r.live ? rec_bits[i] : 0u; p.u_off = u;
            if (!r.live) continue;
            const uint32_t most_hdr = p.pre_len + p.post_len + (p.kind == JS_PROG_AC_FIRST ? 277u : p.ntab * 37u);
            if (hdr_len[i] < p.pre_len + p.post_len + p.ntab * 22u || hdr_len[i] > most_hdr || most_hdr > JS_PROG_HDR) {
                js_set_error("export_jpeg: entry %d, scan %u came back with a header piece of %u bytes", k, p.scan, hdr_len[i]); return -1; }
            if ((p.bits & 7u) || p.bits < 8u * (uint64_t)p.ni || p.bits > (uint64_t)p.nunits * 1668u + 7u * (uint64_t)p.ni) {
                js_set_error("export_jpeg: entry %d, scan %u came back with %llu bits for %u blocks in %u intervals", k, p.scan, (unsigned long long)p.bits, p.nunits, p.ni); return -1; }
            const uint64_t nbytes = p.bits >> 3;
            u += ((nbytes + 15u) & ~(uint64_t)15u) + 16u;
            cap += js_export_prog_scan_cap(hdr_len[i], nbytes, p.ni);
            chunks += (nbytes + JS_EXPORT_CHUNK - 1u) / JS_EXPORT_CHUNK;
            if (chunks >= 0x7FFFFFFFull) { js_set_error("export_jpeg: more than 2^31 stuffing chunks in one call"); return -1; }
        }
        if (r.live) { r.out_cap = (cap + 15u) & ~(uint64_t)15u; o += r.out_cap; }
    }
    chunk_base[rec_base[n]] = (uint32_t)chunks; *u_bytes = u; *out_bytes = o;
    return 0;
}
