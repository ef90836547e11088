// jsnoop_export_prog.hip -- the kernels of jsnoop_batch_export_jpeg_prog: a decoded batch written as progressive (SOF2) files along a scan script (the definition:
// tests/export_prog_model.py; host side: jsnoop_export.cpp; arithmetic and the run operators: jsnoop_export_prog_check.h).
//
// The unit of work is a tile of up to JS_EXPORT_TILE consecutive units of one (entry, scan) record: a thread owns a unit, one block of the scan in the scan's own
// order (js_prog_block maps it to the arena: an interleaved scan walks the arena itself, a one-component scan of a three-component image gathers the coded part
// of its component row by row).  Tiles never straddle scans or entries; the record of a tile comes from a prefix table by one search.
//
//   k_prog_classify   AC scans: every unit EMPTY / TAIL / FULL from the levels of its band.
//   k_prog_runs       AC scans, a workgroup a scan: the two segmented scans of jsnoop_export_prog_check.h over the classes, JS_EXPORT_SCAN units a step with the
//                     summary of everything before (behind) as the carry; every unit gets the length of the end-of-band run whose EOBn it carries (uint16; 0: none).
//   k_prog_symbols    ONE walk (pg_walk: DC first / DC refinement / AC first over Ss..Se with the point transform) with a sink that counts symbols ...
//   k_prog_huff       ... T.81 K.2 per (scan, table), a wave a table -- k_export_huff's procedure on this call's records: up to three DC tables or one AC table
//                     a scan -- and the scan's header piece: the host's bytes in front, the DHT segments, the host's DRI / SOS.
//   k_prog_measure    the walk with a sink that sums bits: a length per unit, a JsRstSum per tile (a scan starts on a byte and so does every interval of it), the
//                     result words of the entry (atomicMax) and its lowest offending block per kind in the IMAGE's decode order (atomicMin).
//   (k_export_rst_scan over the tiles of every scan record: jsnoop_export.hip)
//   k_prog_bits       the walk with a sink that writes, k_export_bits' scheme: an LDS window, interior words stored, edge words ORed into zeroed memory; a tile
//                     of nothing but empty blocks writes nothing.  The thread of an interval's last unit pads and writes the interval's end into the table.
//   k_prog_ffcount, (k_export_scan,) k_prog_place, k_prog_stuff
//                     FF bytes per chunk and scan; where every scan's piece starts in its file (a thread an entry adds up header pieces, stream bytes, FF bytes
//                     and markers scan by scan), EOI and the file's length; k_export_stuff_rst's stuffing with the scan's header piece in front of its first chunk.
// Words of the bit stream are kept MSB-first as numbers and byte-swapped when they leave for memory.  A bit group is at most 32 bits (an EOB14: 16 + 14).
#include <hip/hip_runtime.h>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_launch.h"
#include "jsnoop_export_prog_check.h"

#define PG_THREADS 256
#define PG_ROW_HALVES 66u                             /* 132 bytes: 33 dwords, as jsnoop_export.hip lays its rows */
#define PG_WIN_WORDS (JS_EXPORT_WINDOW / 4u)
#define PG_AC 48u                                     /* where the AC table starts in a scan's JS_PROG_TAB_WORDS */
static_assert(JS_EXPORT_TILE == PG_THREADS && JS_EXPORT_SCAN == PG_THREADS && JS_EXPORT_CHUNK == PG_THREADS * 16u, "a thread owns a unit / 16 bytes");

typedef uint32_t pg_u32x4 __attribute__((ext_vector_type(4)));
__constant__ uint8_t c_pg_zigzag[64] = JS_ZIGZAG_NATURAL;
__constant__ uint8_t c_pg_zzpos[64] = JS_ZIGZAG_POSITION;

// the last k with base[k] <= u (base[0] = 0, base[n] > u)
__device__ __forceinline__ uint32_t pg_find(const uint32_t* __restrict__ base, uint32_t n, uint32_t u)
{
    uint32_t k = 0;
    for (uint32_t top = n; top - k > 1u; ) { const uint32_t mid = (k + top) >> 1; if (base[mid] <= u) k = mid; else top = mid; }
    return k;
}
// exclusive prefix sum over the workgroup; *total = the sum.  s: PG_THREADS words of LDS (free to reuse behind the call).
__device__ __forceinline__ uint32_t pg_scan(uint32_t v, uint32_t* s, uint32_t* total)
{
    const uint32_t t = threadIdx.x;
    s[t] = v; __syncthreads();
    for (uint32_t d = 1; d < PG_THREADS; d <<= 1) {
        const uint32_t a = t >= d ? s[t - d] : 0u; __syncthreads();
        s[t] += a; __syncthreads();
    }
    const uint32_t incl = s[t]; *total = s[PG_THREADS - 1]; __syncthreads();
    return incl - v;
}
// exclusive scan of run summaries over the workgroup with js_rst_combine; *total = the summary of all
__device__ __forceinline__ JsRstSum pg_rst_scan(JsRstSum v, JsRstSum* s, JsRstSum* total)
{
    const uint32_t t = threadIdx.x;
    s[t] = v; __syncthreads();
    for (uint32_t d = 1; d < PG_THREADS; d <<= 1) {
        JsRstSum a = s[t];
        if (t >= d) a = js_rst_combine(s[t - d], a);
        __syncthreads();
        s[t] = a; __syncthreads();
    }
    const JsRstSum ex = t ? s[t - 1u] : js_rst_identity();
    *total = s[PG_THREADS - 1]; __syncthreads();
    return ex;
}

// The sinks of pg_walk see every symbol twice: sym(index into the scan's JS_PROG_TAB_WORDS) and put(bits, count) with its code and value bits.
struct PgCount { uint32_t bits = 0; __device__ __forceinline__ void put(uint32_t, uint32_t n) { bits += n; } __device__ __forceinline__ void sym(uint32_t) {} };
struct PgSymbols { uint32_t* hist; __device__ __forceinline__ void put(uint32_t, uint32_t) {} __device__ __forceinline__ void sym(uint32_t i) { atomicAdd(hist + i, 1u); } };
struct PgEmit {
    uint32_t* win; uint32_t* mem; uint64_t w0, pos;
    __device__ __forceinline__ void word(uint64_t w, uint32_t v) {
        if (!v) return;
        const uint64_t rel = w - w0;
        if (rel < PG_WIN_WORDS) atomicOr(win + (uint32_t)rel, v); else atomicOr(mem + w, __builtin_bswap32(v));
    }
    __device__ __forceinline__ void put(uint32_t v, uint32_t n) {
        if (!n) return;
        const uint32_t off = (uint32_t)pos & 31u; const uint64_t w = pos >> 5;
        if (off + n <= 32u) word(w, v << (32u - off - n));
        else { const uint32_t k = off + n - 32u; word(w, v >> k); word(w + 1u, v << (32u - k)); }
        pos += n;
    }
    __device__ __forceinline__ void sym(uint32_t) {}
};

struct PgShared {
    union { uint16_t rows[JS_EXPORT_TILE * PG_ROW_HALVES]; JsRstSum sums[PG_THREADS]; };      // sums: behind the walks
    uint32_t blk[PG_THREADS];                                                               // the arena block of every thread's unit
    uint16_t q[64];                                                                         // AC: the component's multipliers, zig-zag order
    uint32_t tab[JS_PROG_TAB_WORDS];
};
// The tile into LDS: the arena block of every unit, the scan's code words (tabs == NULL: zeros) and, for an AC scan, the units' rows -- gathered by the map, 16-byte
// loads of whole 128-byte rows written in ZIG-ZAG order -- and the component's multipliers.  Ends with a barrier.
__device__ __forceinline__ void pg_stage(PgShared& s, const int16_t* __restrict__ coef, const JsExportScanRec& r, const JsExportRec& e, uint32_t u0, uint32_t nb, const uint32_t* __restrict__ tabs)
{
    const uint32_t t = threadIdx.x, ch = t & 7u;
    s.blk[t] = t < nb ? js_prog_block(r, u0 + t) : 0xFFFFFFFFu;
    for (uint32_t i = t; i < JS_PROG_TAB_WORDS; i += PG_THREADS) s.tab[i] = tabs ? tabs[i] : 0u;
    const bool ac = r.kind == JS_PROG_AC_FIRST;
    if (ac && t < 64u) s.q[t] = e.q[r.comp0][c_pg_zigzag[t]];
    __syncthreads();
    if (ac) {
        uint32_t zp[8];
        #pragma unroll
        for (uint32_t k = 0; k < 8u; k++) zp[k] = c_pg_zzpos[ch * 8u + k];
        #pragma unroll
        for (uint32_t p = 0; p < 8u; p++) {
            const uint32_t i = p * PG_THREADS + t, b = i >> 3;
            if (b < nb) {
                const pg_u32x4 v = reinterpret_cast<const pg_u32x4*>(coef + (e.coef_off + s.blk[b]) * 64u)[ch]; uint16_t* o = s.rows + b * PG_ROW_HALVES;
                o[zp[0]] = (uint16_t)v.x; o[zp[1]] = (uint16_t)(v.x >> 16); o[zp[2]] = (uint16_t)v.y; o[zp[3]] = (uint16_t)(v.y >> 16);
                o[zp[4]] = (uint16_t)v.z; o[zp[5]] = (uint16_t)(v.z >> 16); o[zp[6]] = (uint16_t)v.w; o[zp[7]] = (uint16_t)(v.w >> 16);
            }
        }
        __syncthreads();
    }
}
// the level of an AC value (C division; no multiplier: level 0 and inexact)
__device__ __forceinline__ int32_t pg_level(int32_t v, int32_t qz, bool& inexact)
{
    if (!qz) { inexact = true; return 0; }
    const int32_t lv = v / qz; inexact |= lv * qz != v;
    return lv;
}
// the absolute DC level of arena block j: (int16)dccum / q[0]
__device__ __forceinline__ int32_t pg_dc(const int16_t* __restrict__ dccum, uint64_t coef_off, uint32_t j, int32_t q0, bool& inexact)
{
    const int32_t d = dccum[coef_off + j];
    if (!q0) { inexact |= d != 0; return 0; }
    const int32_t lv = d / q0; inexact |= lv * q0 != d;
    return lv;
}
// the class of a unit of an AC scan from its row (zig-zag order)
__device__ __forceinline__ uint32_t pg_class(const uint16_t* row, const uint16_t* q, uint32_t ss, uint32_t se)
{
    bool any = false, last = false, ix = false;
    for (uint32_t z = ss; z <= se; z++) {
        const int32_t v = (int16_t)row[z];
        last = v && pg_level(v, q[z], ix) != 0;
        any |= last;
    }
    return any ? (last ? JS_PROG_FULL : JS_PROG_TAIL) : JS_PROG_EMPTY;
}
// One unit through `sink`.  u: the unit, j: its arena block; row / q: AC only; tab: the scan's code words (length << 16 | code by symbol); eob: the length of the
// end-of-band run whose EOBn the unit carries (AC; 0: none).  Returns the unit's result (JSNOOP_EXPORT_OK / _INEXACT / _UNCODABLE).
template <class SINK>
__device__ __forceinline__ uint32_t pg_walk(const JsExportScanRec& r, const JsExportRec& e, const int16_t* __restrict__ dccum, uint32_t u, uint32_t j, const uint16_t* row, const uint16_t* q,
                                            const uint32_t* tab, uint32_t eob, SINK& sink)
{
    bool inexact = false, uncodable = false;
    const uint32_t al = r.al;
    if (r.kind != JS_PROG_AC_FIRST) {
        const uint32_t p = u % r.spm, c = r.comp[p], slot = r.slot[p], back = r.back[p];
        const int32_t q0 = e.q[c][0], v = pg_dc(dccum, e.coef_off, j, q0, inexact);
        if (r.kind == JS_PROG_DC_REFINE) sink.put((uint32_t)(v >> al) & 1u, 1u);
        else {
            int32_t pv = 0;
            if (u >= back && (r.ri == 0u || u % r.ri >= back)) { bool other = false; pv = pg_dc(dccum, e.coef_off, js_prog_block(r, u - back), q0, other) >> al; }
            const int32_t d = (v >> al) - pv;
            const uint32_t a = (uint32_t)(d < 0 ? -d : d), cat = 32u - (uint32_t)__clz((int)a);
            uncodable |= a > 2047u;
            const uint32_t i = slot * 16u + (cat & 15u), w = tab[i], bits = (uint32_t)(d < 0 ? d - 1 : d) & ((1u << cat) - 1u);
            sink.sym(i);
            sink.put(((w & 0xFFFFu) << cat) | bits, (w >> 16) + cat);
        }
    } else {
        const uint32_t* ac = tab + PG_AC;
        uint32_t run = 0;
        for (uint32_t z = r.ss; z <= r.se; z++) {
            const int32_t v = (int16_t)row[z];
            if (!v) { run++; continue; }
            const int32_t lv = pg_level(v, q[z], inexact);
            if (!lv) { run++; continue; }
            const uint32_t a = (uint32_t)(lv < 0 ? -lv : lv), cat = 32u - (uint32_t)__clz((int)a);
            uncodable |= a > 1023u;
            while (run > 15u) { const uint32_t w = ac[0xF0]; sink.sym(PG_AC + 0xF0u); sink.put(w & 0xFFFFu, w >> 16); run -= 16u; }
            const uint32_t sy = ((run << 4) | cat) & 255u, w = ac[sy], bits = (uint32_t)(lv < 0 ? lv - 1 : lv) & ((1u << cat) - 1u);
            sink.sym(PG_AC + sy);
            sink.put(((w & 0xFFFFu) << cat) | bits, (w >> 16) + cat);
            run = 0;
        }
        if (eob) {
            const uint32_t n = 31u - (uint32_t)__clz((int)eob), w = ac[n << 4];
            sink.sym(PG_AC + (n << 4));
            sink.put(((w & 0xFFFFu) << n) | (eob - (1u << n)), (w >> 16) + n);
        }
    }
    return uncodable ? JSNOOP_EXPORT_UNCODABLE : (inexact ? JSNOOP_EXPORT_INEXACT : JSNOOP_EXPORT_OK);
}

__global__ void __launch_bounds__(PG_THREADS) k_prog_classify(const int16_t* __restrict__ coef, const JsExportRec* __restrict__ recs, const JsExportScanRec* __restrict__ srecs,
                                                              const uint32_t* __restrict__ tile_base, uint32_t nrec, uint8_t* __restrict__ cls)
{
    __shared__ PgShared s;
    const uint32_t t = threadIdx.x, tile = blockIdx.x, i = pg_find(tile_base, nrec, tile);
    const JsExportScanRec& r = srecs[i];
    if (r.kind != JS_PROG_AC_FIRST) return;
    const uint32_t u0 = (tile - tile_base[i]) * JS_EXPORT_TILE, nb = min(JS_EXPORT_TILE, r.nunits - u0);
    pg_stage(s, coef, r, recs[r.entry], u0, nb, nullptr);
    if (t < nb) cls[r.ubase + u0 + t] = (uint8_t)pg_class(s.rows + t * PG_ROW_HALVES, s.q, r.ss, r.se);
}

// A workgroup a scan record.  Forward: the inclusive scan of JsRunFwd decides which units carry an EOBn (eob[u] = 1); backward, over the units in reverse: the
// scan of JsRunBwd over everything behind a unit gives every carrier its run length.
__global__ void __launch_bounds__(PG_THREADS) k_prog_runs(const JsExportScanRec* __restrict__ srecs, const uint8_t* __restrict__ cls_all, uint16_t* __restrict__ eob_all)
{
    __shared__ JsRunFwd sf[PG_THREADS];
    __shared__ JsRunBwd sb[PG_THREADS];
    const JsExportScanRec& r = srecs[blockIdx.x];
    if (r.kind != JS_PROG_AC_FIRST) return;
    const uint32_t t = threadIdx.x, n = r.nunits;
    const uint8_t* cls = cls_all + r.ubase; uint16_t* eob = eob_all + r.ubase;
    JsRunFwd cf = js_run_fwd_identity();
    for (uint32_t i0 = 0; i0 < n; i0 += JS_EXPORT_SCAN) {              // (n, i0: the same in every thread -- every barrier is met by all; n < 2^26)
        const uint32_t u = i0 + t; const bool mine = u < n;
        const uint32_t c = mine ? cls[u] : JS_PROG_FULL;
        sf[t] = mine ? js_run_fwd_leaf(c, js_prog_starts(r, u)) : js_run_fwd_identity(); __syncthreads();
        for (uint32_t d = 1; d < PG_THREADS; d <<= 1) {
            JsRunFwd a = sf[t];
            if (t >= d) a = js_run_fwd_combine(sf[t - d], a);
            __syncthreads();
            sf[t] = a; __syncthreads();
        }
        if (mine) eob[u] = js_run_carries(c, js_run_fwd_combine(cf, sf[t])) ? (uint16_t)1u : (uint16_t)0u;
        cf = js_run_fwd_combine(cf, sf[PG_THREADS - 1]); __syncthreads();
    }
    JsRunBwd cb = js_run_bwd_identity();
    for (uint32_t hi = n; hi > 0u; ) {
        const uint32_t lo = (hi - 1u) / JS_EXPORT_SCAN * JS_EXPORT_SCAN, u = hi - 1u - t; const bool mine = t < hi - lo;      // thread t: the t-th unit from the back
        const bool ends = mine && js_prog_ends(r, u);
        sb[t] = mine ? js_run_bwd_leaf(cls[u], ends) : js_run_bwd_identity(); __syncthreads();
        for (uint32_t d = 1; d < PG_THREADS; d <<= 1) {
            JsRunBwd a = sb[t];
            if (t >= d) a = js_run_bwd_combine(a, sb[t - d]);           // (sb[t - d] summarises units BEHIND those of sb[t])
            __syncthreads();
            sb[t] = a; __syncthreads();
        }
        if (mine && eob[u]) eob[u] = (uint16_t)js_run_length(ends, js_run_bwd_combine(t ? sb[t - 1u] : js_run_bwd_identity(), cb));
        cb = js_run_bwd_combine(sb[PG_THREADS - 1], cb); __syncthreads();
        hi = lo;
    }
}

__global__ void __launch_bounds__(PG_THREADS) k_prog_symbols(const int16_t* __restrict__ coef, const int16_t* __restrict__ dccum, const JsExportRec* __restrict__ recs,
                                                             const JsExportScanRec* __restrict__ srecs, const uint32_t* __restrict__ tile_base, uint32_t nrec,
                                                             const uint16_t* __restrict__ eob, JsExportScanStat* __restrict__ stats)
{
    __shared__ PgShared s;
    __shared__ uint32_t s_hist[JS_PROG_TAB_WORDS];
    const uint32_t t = threadIdx.x, tile = blockIdx.x, i = pg_find(tile_base, nrec, tile);
    const JsExportScanRec& r = srecs[i];
    if (r.kind == JS_PROG_DC_REFINE) return;
    const JsExportRec& e = recs[r.entry];
    const uint32_t u0 = (tile - tile_base[i]) * JS_EXPORT_TILE, nb = min(JS_EXPORT_TILE, r.nunits - u0);
    for (uint32_t k = t; k < JS_PROG_TAB_WORDS; k += PG_THREADS) s_hist[k] = 0u;
    pg_stage(s, coef, r, e, u0, nb, nullptr);
    if (t < nb) {
        PgSymbols sink{ s_hist };
        pg_walk(r, e, dccum, u0 + t, s.blk[t], s.rows + t * PG_ROW_HALVES, s.q, s.tab, r.kind == JS_PROG_AC_FIRST ? (uint32_t)eob[r.ubase + u0 + t] : 0u, sink);
    }
    __syncthreads();
    uint32_t* freq = stats[i].freq;
    for (uint32_t k = t; k < JS_PROG_TAB_WORDS; k += PG_THREADS) { const uint32_t v = s_hist[k]; if (v) atomicAdd(freq + k, v); }
}

#define PG_HUFF_DEAD 0xFFFFFFFFFFFFFFFFull
__device__ __forceinline__ uint64_t pg_wave_min(uint64_t v)
{
    #pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const uint64_t o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
// One workgroup per scan record, wave w builds table w of the scan (a DC first scan: the table of the scan's w-th component, class 0, id w; an AC scan: wave 0,
// class 1, id 0).  The procedure is k_export_huff's (jsnoop_export.hip), to which the comments there apply: keys (frequency << 9 | 511 - symbol) of live group
// heads, a merge as two wave-wide minima, Adjust_BITS and the reserved code point by one lane, ranks by (code size, symbol), Annex C codes.  The whole workgroup
// then puts the scan's header piece together.  Every barrier is met by all four waves: a wave without a table runs along with nothing but the reserved symbol.
// (The procedure is REPEATED here, not shared: called as one inline function from both kernels it changed k_export_huff's register count.  A fix to either belongs in both.)
__global__ void __launch_bounds__(PG_THREADS) k_prog_huff(const JsExportScanRec* __restrict__ srecs, const uint8_t* __restrict__ hdrs, JsExportScanStat* __restrict__ stats, uint32_t* __restrict__ tabs,
                                                          uint8_t* __restrict__ hdr_out, uint32_t* __restrict__ hdr_len)
{
    __shared__ uint16_t s_size[4][264];
    __shared__ uint32_t s_bits[4][264];
    __shared__ uint8_t s_syms[4][256];
    __shared__ uint32_t s_start[4][18], s_first[4][18];
    const uint32_t t = threadIdx.x, k = blockIdx.x, w = t >> 6, lane = t & 63u;
    const JsExportScanRec& r = srecs[k];
    const uint32_t ntab = r.ntab, cls = r.kind == JS_PROG_AC_FIRST ? 1u : 0u, nsymbols = cls ? 256u : 16u, at0 = cls ? PG_AC : (w < 3u ? w * 16u : 0u);
    const bool have = w < ntab;
    const uint32_t* freq = stats[k].freq + at0;
    uint64_t key[5]; uint32_t size[5], group[5];
    #pragma unroll
    for (uint32_t e = 0; e < 5u; e++) {
        const uint32_t sy = lane * 5u + e;
        const uint64_t f = sy == 256u ? 1u : (have && sy < nsymbols ? (uint64_t)freq[sy] : 0u);
        key[e] = f ? (f << 9 | (511u - sy)) : PG_HUFF_DEAD; size[e] = 0u; group[e] = f ? sy : 0xFFFFu;
    }
    for (;;) {
        uint64_t m = key[0];
        #pragma unroll
        for (uint32_t e = 1; e < 5u; e++) m = key[e] < m ? key[e] : m;
        const uint64_t m1 = pg_wave_min(m);
        m = PG_HUFF_DEAD;
        #pragma unroll
        for (uint32_t e = 0; e < 5u; e++) m = key[e] != m1 && key[e] < m ? key[e] : m;
        const uint64_t m2 = pg_wave_min(m);
        if (m2 == PG_HUFF_DEAD) break;
        const uint32_t c1 = 511u - (uint32_t)(m1 & 511u), c2 = 511u - (uint32_t)(m2 & 511u);
        const uint64_t merged = ((m1 >> 9) + (m2 >> 9)) << 9 | (511u - c1);
        #pragma unroll
        for (uint32_t e = 0; e < 5u; e++) {
            if (key[e] == m1) key[e] = merged; else if (key[e] == m2) key[e] = PG_HUFF_DEAD;
            if (group[e] == c1 || group[e] == c2) { size[e]++; group[e] = c1; }
        }
    }
    for (uint32_t i = lane; i < 264u; i += 64u) s_bits[w][i] = 0u;
    #pragma unroll
    for (uint32_t e = 0; e < 5u; e++) { const uint32_t sy = lane * 5u + e; if (sy < 264u) s_size[w][sy] = group[e] != 0xFFFFu ? (uint16_t)size[e] : (uint16_t)0xFFFFu; }
    __syncthreads();
    #pragma unroll
    for (uint32_t e = 0; e < 5u; e++) if (group[e] != 0xFFFFu) atomicAdd(&s_bits[w][size[e] < 263u ? size[e] : 263u], 1u);
    __syncthreads();
    if (lane == 0u) {
        uint32_t* bits = s_bits[w];
        uint32_t i = 263u;
        while (i > 0u && !bits[i]) i--;
        bool sound = true;
        while (i > 16u && sound) {                                  // Figure K.3
            while (bits[i] > 0u) {
                uint32_t j = i - 2u;
                while (j > 0u && !bits[j]) j--;
                if (!j || bits[i] < 2u) { sound = false; break; }
                bits[i] -= 2u; bits[i - 1u] += 1u; bits[j + 1u] += 2u; bits[j] -= 1u;
            }
            i--;
        }
        while (i > 0u && !bits[i]) i--;
        if (i) bits[i] -= 1u;                                       // the reserved code point
        uint32_t code = 0u, at = 0u;
        for (uint32_t ln = 1; ln <= 16u; ln++) { s_start[w][ln] = at; s_first[w][ln] = code; at += bits[ln]; code = (code + bits[ln]) << 1; }
        s_start[w][17] = at < 256u ? at : 256u;
    }
    for (uint32_t i = lane; i < 256u; i += 64u) s_syms[w][i] = 0u;
    __syncthreads();
    uint32_t* my_tabs = tabs + (size_t)k * JS_PROG_TAB_WORDS + at0;
    #pragma unroll
    for (uint32_t e = 0; e < 5u; e++) {
        const uint32_t sy = lane * 5u + e;
        if (sy >= nsymbols || !have) continue;
        uint32_t word = 0u;
        if (group[e] != 0xFFFFu) {
            uint32_t rank = 0u;
            for (uint32_t u = 0; u < nsymbols; u++) { const uint32_t su = s_size[w][u]; rank += (su < size[e] || (su == size[e] && u < sy)) ? 1u : 0u; }
            uint32_t ln = 1u;
            while (ln < 16u && s_start[w][ln + 1u] <= rank) ln++;
            word = ln << 16 | ((s_first[w][ln] + rank - s_start[w][ln]) & 0xFFFFu);
            s_syms[w][rank & 255u] = (uint8_t)sy;
        }
        my_tabs[sy] = word;
    }
    __syncthreads();
    if (w < 3u) {
        JsExportOptSlot* slot = stats[k].slot + w;
        if (lane == 0u) slot->nsym = have ? s_start[w][17] : 0u;
        if (lane < 16u) slot->counts[lane] = have ? (uint8_t)s_bits[w][lane + 1u] : (uint8_t)0u;
        for (uint32_t i = lane; i < 256u; i += 64u) slot->syms[i] = have ? s_syms[w][i] : (uint8_t)0u;
    }
    // the header piece: the host's bytes in front, a DHT segment per table, the host's DRI / SOS
    uint32_t seg_at[4]; seg_at[0] = r.pre_len;
    #pragma unroll
    for (uint32_t q = 0; q < 3u; q++) seg_at[q + 1u] = seg_at[q] + (q < ntab ? 21u + s_start[q][17] : 0u);
    const uint32_t total = min(seg_at[3] + r.post_len, JS_PROG_HDR);
    const uint8_t* pre = hdrs + r.pre_off; const uint8_t* post = hdrs + r.post_off; uint8_t* out = hdr_out + (size_t)k * JS_PROG_HDR;
    for (uint32_t i = t; i < total; i += PG_THREADS) {
        uint32_t b;
        if (i < r.pre_len) b = pre[i];
        else if (i >= seg_at[3]) b = post[i - seg_at[3]];
        else {
            uint32_t q = 0u;
            #pragma unroll
            for (uint32_t x = 1; x < 3u; x++) q += i >= seg_at[x] ? 1u : 0u;
            const uint32_t rel = i - seg_at[q], n = s_start[q][17];
            b = rel == 0u ? 0xFFu : rel == 1u ? 0xC4u : rel == 2u ? (19u + n) >> 8 : rel == 3u ? (19u + n) & 255u : rel == 4u ? (cls ? 0x10u : q)
              : rel < 21u ? s_bits[q][rel - 4u] : (uint32_t)s_syms[q][(rel - 21u) & 255u];
        }
        out[i] = (uint8_t)b;
    }
    if (t == 0u) hdr_len[k] = total;
}

__global__ void __launch_bounds__(PG_THREADS) k_prog_measure(const int16_t* __restrict__ coef, const int16_t* __restrict__ dccum, const JsExportRec* __restrict__ recs,
                                                             const JsExportScanRec* __restrict__ srecs, const uint32_t* __restrict__ tile_base, uint32_t nrec, const uint32_t* __restrict__ tabs,
                                                             const uint16_t* __restrict__ eob, uint16_t* __restrict__ blk_bits, JsRstSum* __restrict__ tile_sum,
                                                             uint32_t* __restrict__ res /*[nent] result, then [nent][2] lowest block per kind*/, uint32_t nent)
{
    __shared__ PgShared s;
    __shared__ uint32_t s_red[3];                                   // result, lowest inexact block, lowest uncodable block
    const uint32_t t = threadIdx.x, tile = blockIdx.x, i = pg_find(tile_base, nrec, tile);
    const JsExportScanRec& r = srecs[i];
    const JsExportRec& e = recs[r.entry];
    const uint32_t u0 = (tile - tile_base[i]) * JS_EXPORT_TILE, nb = min(JS_EXPORT_TILE, r.nunits - u0);
    uint32_t my_bits = 0u; bool my_end = false;
    if (t == 0) { s_red[0] = 0u; s_red[1] = 0xFFFFFFFFu; s_red[2] = 0xFFFFFFFFu; }
    pg_stage(s, coef, r, e, u0, nb, tabs + (size_t)i * JS_PROG_TAB_WORDS);
    if (t < nb) {
        const uint32_t u = u0 + t, j = s.blk[t];
        PgCount sink;
        const uint32_t st = pg_walk(r, e, dccum, u, j, s.rows + t * PG_ROW_HALVES, s.q, s.tab, r.kind == JS_PROG_AC_FIRST ? (uint32_t)eob[r.ubase + u] : 0u, sink);
        blk_bits[r.ubase + u] = (uint16_t)sink.bits;
        my_bits = sink.bits & 0xFFFFu; my_end = js_prog_ends(r, u);
        if (st) { atomicMax(&s_red[0], st); atomicMin(&s_red[st], j); }
    }
    __syncthreads();                                                // every walk is done: the summaries are scanned where the tile's rows lay
    JsRstSum all;
    pg_rst_scan(t < nb ? js_rst_leaf(my_bits, my_end) : js_rst_identity(), s.sums, &all);
    if (t == 0) {
        JsRstSum* o = tile_sum + tile; o->has = all.has; o->head = all.head; o->mid = all.mid; o->tail = all.tail;
        if (s_red[0]) {
            const uint32_t k = r.entry;
            atomicMax(res + k, s_red[0]);
            if (s_red[1] != 0xFFFFFFFFu) atomicMin(res + nent + 2u * k, s_red[1]);
            if (s_red[2] != 0xFFFFFFFFu) atomicMin(res + nent + 2u * k + 1u, s_red[2]);
        }
    }
}

__global__ void __launch_bounds__(PG_THREADS) k_prog_bits(const int16_t* __restrict__ coef, const int16_t* __restrict__ dccum, const JsExportRec* __restrict__ recs,
                                                          const JsExportScanRec* __restrict__ srecs, const uint32_t* __restrict__ tile_base, uint32_t nrec, const uint32_t* __restrict__ tabs,
                                                          const uint16_t* __restrict__ eob, const uint16_t* __restrict__ blk_bits, const uint64_t* __restrict__ tile_off,
                                                          uint8_t* __restrict__ ustream, uint64_t* __restrict__ itab)
{
    __shared__ PgShared s;
    __shared__ uint32_t s_win[PG_WIN_WORDS];
    __shared__ JsRstSum s_sum[PG_THREADS];
    const uint32_t t = threadIdx.x, tile = blockIdx.x, i = pg_find(tile_base, nrec, tile);
    const JsExportScanRec& r = srecs[i];
    if (!r.live) return;
    const JsExportRec& e = recs[r.entry];
    const uint32_t u0 = (tile - tile_base[i]) * JS_EXPORT_TILE, nb = min(JS_EXPORT_TILE, r.nunits - u0);
    uint32_t* mem = reinterpret_cast<uint32_t*>(ustream + r.u_off);
    for (uint32_t k = t; k < PG_WIN_WORDS; k += PG_THREADS) s_win[k] = 0u;
    pg_stage(s, coef, r, e, u0, nb, tabs + (size_t)i * JS_PROG_TAB_WORDS);
    const uint32_t mine = t < nb ? (uint32_t)blk_bits[r.ubase + u0 + t] : 0u;
    const bool ends = t < nb && js_prog_ends(r, u0 + t);
    const uint64_t b0 = tile_off[tile];
    JsRstSum all;
    const JsRstSum ex = pg_rst_scan(t < nb ? js_rst_leaf(mine, ends) : js_rst_identity(), s_sum, &all);
    const uint64_t at = js_rst_apply(b0, ex), b1 = js_rst_apply(b0, all);      // the range this workgroup writes: [b0, b1), possibly empty
    const uint32_t pad = (uint32_t)(0u - (at + mine)) & 7u;                    // ones behind this thread's unit, where it ends an interval
    const uint64_t w0 = b0 >> 5;
    if (t < nb) {
        const uint32_t u = u0 + t;
        PgEmit sink{ s_win, mem, w0, at };
        pg_walk(r, e, dccum, u, s.blk[t], s.rows + t * PG_ROW_HALVES, s.q, s.tab, r.kind == JS_PROG_AC_FIRST ? (uint32_t)eob[r.ubase + u] : 0u, sink);
        if (ends) { if (pad) sink.put((1u << pad) - 1u, pad); itab[r.itab_off + (r.ri ? u / r.ri : 0u)] = (at + mine + pad) >> 3; }
    }
    __syncthreads();
    if (b1 == b0) return;
    const uint64_t wl = (b1 - 1u) >> 5, nw = wl - w0 + 1u;
    const uint32_t in_win = nw < PG_WIN_WORDS ? (uint32_t)nw : PG_WIN_WORDS;
    for (uint32_t k = t; k < in_win; k += PG_THREADS) {
        const uint32_t v = __builtin_bswap32(s_win[k]);
        if (k == 0u || w0 + k == wl) { if (v) atomicOr(mem + w0 + k, v); }      // shared with the neighbouring range
        else mem[w0 + k] = v;
    }
}

__device__ __forceinline__ uint32_t pg_ff16(pg_u32x4 v, uint32_t valid /*bytes that count, from the first*/)
{
    uint32_t n = 0; const uint32_t w[4] = { v.x, v.y, v.z, v.w };
    #pragma unroll
    for (uint32_t i = 0; i < 16u; i++) n += (i < valid && ((w[i >> 2] >> ((i & 3u) * 8u)) & 255u) == 255u) ? 1u : 0u;
    return n;
}
__global__ void __launch_bounds__(PG_THREADS) k_prog_ffcount(const JsExportScanRec* __restrict__ srecs, const uint32_t* __restrict__ chunk_base, uint32_t nrec,
                                                             const uint8_t* __restrict__ ustream, uint32_t* __restrict__ chunk_ff)
{
    __shared__ uint32_t s_n;
    const uint32_t t = threadIdx.x, chunk = blockIdx.x, i = pg_find(chunk_base, nrec, chunk);
    const JsExportScanRec& r = srecs[i];
    const uint64_t nbytes = r.bits >> 3, c0 = (uint64_t)(chunk - chunk_base[i]) * JS_EXPORT_CHUNK, at = c0 + t * 16u;
    if (t == 0) s_n = 0u;
    __syncthreads();
    if (at < nbytes) {
        const pg_u32x4 v = *reinterpret_cast<const pg_u32x4*>(ustream + r.u_off + at);
        const uint32_t n = pg_ff16(v, (uint32_t)min((uint64_t)16u, nbytes - at));
        if (n) atomicAdd(&s_n, n);
    }
    __syncthreads();
    if (t == 0) chunk_ff[chunk] = s_n;
}

// Where every scan's piece starts in its file, EOI and the file's length: one thread an entry walks its scan records.  A piece is the header piece, the stream's
// bytes, a 00 per FF and a marker per interval but the last.
__global__ void k_prog_place(const JsExportRec* __restrict__ recs, const JsExportScanRec* __restrict__ srecs, const uint32_t* __restrict__ rec_base, uint32_t nent,
                             const uint32_t* __restrict__ hdr_len, const uint64_t* __restrict__ rec_ff, uint64_t* __restrict__ scan_out, uint8_t* __restrict__ out, uint64_t* __restrict__ len)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nent || !recs[k].live) return;
    uint64_t pos = 0;
    for (uint32_t i = rec_base[k]; i < rec_base[k + 1u]; i++) { scan_out[i] = pos; pos += (uint64_t)hdr_len[i] + (srecs[i].bits >> 3) + rec_ff[i] + 2u * (uint64_t)(srecs[i].ni - 1u); }
    uint8_t* file = out + recs[k].out_off;
    file[pos] = 0xFFu; file[pos + 1u] = 0xD9u; len[k] = pos + 2u;
}

// k_export_stuff_rst (jsnoop_export.hip) per scan record: byte p of interval r of the scan goes to (the piece's start) + header piece + p + (FFs in front of p) + 2 r,
// and FF D0+(r & 7) follows the last byte of every interval but the scan's last.  The first chunk's workgroup also copies the header piece the device built.
__global__ void __launch_bounds__(PG_THREADS) k_prog_stuff(const JsExportRec* __restrict__ recs, const JsExportScanRec* __restrict__ srecs, const uint32_t* __restrict__ chunk_base, uint32_t nrec,
                                                           const uint8_t* __restrict__ ustream, const uint64_t* __restrict__ chunk_off, const uint64_t* __restrict__ itab_all,
                                                           const uint8_t* __restrict__ hdrs, const uint32_t* __restrict__ hdr_lens, const uint64_t* __restrict__ scan_out, uint8_t* __restrict__ out)
{
    __shared__ uint32_t s_scan[PG_THREADS];
    __shared__ uint8_t s_out[4u * JS_EXPORT_CHUNK];
    __shared__ uint32_t s_r0, s_n;
    const uint32_t t = threadIdx.x, chunk = blockIdx.x, k = pg_find(chunk_base, nrec, chunk);
    const JsExportScanRec& r = srecs[k];
    const uint32_t lc = chunk - chunk_base[k], hdr_len = hdr_lens[k], ni = r.ni;
    const uint64_t* itab = itab_all + r.itab_off;
    const uint64_t nbytes = r.bits >> 3, c0 = (uint64_t)lc * JS_EXPORT_CHUNK, at = c0 + t * 16u;
    const uint32_t here = (uint32_t)min((uint64_t)JS_EXPORT_CHUNK, nbytes - c0);
    uint8_t* file = out + recs[r.entry].out_off + scan_out[k];
    pg_u32x4 v = { 0u, 0u, 0u, 0u }; uint32_t valid = 0, iv = 0;
    if (at < nbytes) {
        v = *reinterpret_cast<const pg_u32x4*>(ustream + r.u_off + at); valid = (uint32_t)min((uint64_t)16u, nbytes - at);
        for (uint32_t top = ni - 1u; iv < top; ) { const uint32_t mid = (iv + top) >> 1; if (itab[mid] > at) top = mid; else iv = mid + 1u; }      // the first interval that ends behind `at`
    }
    if (t == 0) s_r0 = iv;
    uint32_t ff_here;
    const uint32_t before = pg_scan(pg_ff16(v, valid), s_scan, &ff_here);
    const uint32_t r0 = s_r0;
    if (valid) {
        uint32_t o = t * 16u + before + 2u * (iv - r0); const uint32_t w[4] = { v.x, v.y, v.z, v.w };
        uint64_t end = itab[iv];
        #pragma unroll
        for (uint32_t i = 0; i < 16u; i++) if (i < valid) {
            const uint32_t b = (w[i >> 2] >> ((i & 3u) * 8u)) & 255u;
            s_out[o++] = (uint8_t)b;
            if (b == 255u) s_out[o++] = 0u;
            if (at + i + 1u == end) {
                if (iv + 1u < ni) { s_out[o++] = 0xFFu; s_out[o++] = (uint8_t)(0xD0u + (iv & 7u)); end = itab[iv + 1u]; }
                iv++;
            }
        }
        if (t * 16u + valid == here) s_n = o;                       // the thread with the chunk's last byte: everything the chunk writes
    }
    __syncthreads();
    uint8_t* dst = file + (uint64_t)hdr_len + c0 + chunk_off[chunk] + 2u * (uint64_t)r0;
    const uint32_t n_out = s_n;
    for (uint32_t i = t; i < n_out; i += PG_THREADS) dst[i] = s_out[i];
    if (lc == 0u) { const uint8_t* h = hdrs + (size_t)k * JS_PROG_HDR; for (uint32_t i = t; i < hdr_len; i += PG_THREADS) file[i] = h[i]; }
}

int js_launch_export_prog_measure(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const JsExportScanRec* srecs, const uint32_t* tile_base, uint32_t nent,
                                  uint32_t nrec, uint32_t tiles, const uint8_t* hdrs, JsExportScanStat* stats, uint32_t* tabs, uint8_t* hdr_out, uint32_t* hdr_len, uint8_t* cls, uint16_t* eob,
                                  uint16_t* blk_bits, JsRstSum* tile_sum, uint64_t* tile_off, uint32_t* res, uint64_t* rec_bits)
{
    if (!nrec || !tiles) return 0;
    hipLaunchKernelGGL(k_prog_classify, dim3(tiles), dim3(PG_THREADS), 0, st, coef, recs, srecs, tile_base, nrec, cls);
    hipLaunchKernelGGL(k_prog_runs, dim3(nrec), dim3(PG_THREADS), 0, st, srecs, (const uint8_t*)cls, eob);
    hipLaunchKernelGGL(k_prog_symbols, dim3(tiles), dim3(PG_THREADS), 0, st, coef, dccum, recs, srecs, tile_base, nrec, (const uint16_t*)eob, stats);
    hipLaunchKernelGGL(k_prog_huff, dim3(nrec), dim3(PG_THREADS), 0, st, srecs, hdrs, stats, tabs, hdr_out, hdr_len);
    hipLaunchKernelGGL(k_prog_measure, dim3(tiles), dim3(PG_THREADS), 0, st, coef, dccum, recs, srecs, tile_base, nrec, (const uint32_t*)tabs, (const uint16_t*)eob, blk_bits, tile_sum, res, nent);
    if (hipGetLastError() != hipSuccess) return -1;
    return js_launch_export_rst_scan(st, tile_sum, tile_off, tile_base, nrec, rec_bits);
}
int js_launch_export_prog_write(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const JsExportScanRec* srecs, const uint32_t* rec_base, const uint32_t* tile_base,
                                const uint32_t* chunk_base, uint32_t nent, uint32_t nrec, uint32_t tiles, uint32_t chunks, const uint32_t* tabs, const uint16_t* eob, const uint16_t* blk_bits,
                                const uint64_t* tile_off, uint64_t* itab, uint8_t* ustream, uint32_t* chunk_ff, uint64_t* chunk_off, uint64_t* rec_ff, const uint8_t* hdrs,
                                const uint32_t* hdr_len, uint64_t* scan_out, uint8_t* out, uint64_t* len)
{
    if (!nrec || !tiles || !chunks) return 0;
    hipLaunchKernelGGL(k_prog_bits, dim3(tiles), dim3(PG_THREADS), 0, st, coef, dccum, recs, srecs, tile_base, nrec, tabs, eob, blk_bits, tile_off, ustream, itab);
    hipLaunchKernelGGL(k_prog_ffcount, dim3(chunks), dim3(PG_THREADS), 0, st, srecs, chunk_base, nrec, (const uint8_t*)ustream, chunk_ff);
    if (hipGetLastError() != hipSuccess) return -1;
    if (js_launch_export_scan(st, chunk_ff, chunk_off, chunk_base, nrec, rec_ff)) return -1;
    hipLaunchKernelGGL(k_prog_place, dim3((nent + 63u) / 64u), dim3(64), 0, st, recs, srecs, rec_base, nent, hdr_len, (const uint64_t*)rec_ff, scan_out, out, len);
    hipLaunchKernelGGL(k_prog_stuff, dim3(chunks), dim3(PG_THREADS), 0, st, recs, srecs, chunk_base, nrec, (const uint8_t*)ustream, (const uint64_t*)chunk_off, (const uint64_t*)itab, hdrs, hdr_len,
                       (const uint64_t*)scan_out, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
