// jsnoop_export.hip -- the kernels of jsnoop_batch_export_jpeg: the coefficient arena and the cumulative DC of a decoded batch entropy-coded as baseline JPEG
// files (the definition: tests/export_model.py; host side: jsnoop_export.cpp, jsnoop_export_check.h).
//
// A unit is a tile of up to JS_EXPORT_TILE blocks of one listed entry, consecutive in the arena (decode order IS arena order), the work of one workgroup of
// 256 threads: a thread owns a block.  Units never straddle two entries; the entry of a unit comes from a prefix table by one search.
//
//   k_export_measure  stages the tile in LDS (16-byte loads of whole 128-byte rows, written in ZIG-ZAG order; rows 132 bytes apart, so the per-thread walks below
//                     read 32 different banks).  A thread walks its block two positions a dword -- a zero dword is two more of the run, and most are zero --,
//                     divides, tests remainders and ranges, sums code and value bits: one bit length per block (uint16: a block has at most 20 + 63 * 26 bits),
//                     one sum per unit, and per entry the result word (atomicMax) and the lowest offending block per kind (atomicMin).
//   k_export_scan     exclusive prefix sums inside every entry, one workgroup per entry walking its units JS_EXPORT_SCAN at a time with a 64-bit carry;
//                     used a second time for the FF counts of the stuffing chunks.
//   k_export_bits     the same walk (ONE function, ex_walk, with a sink that either counts or writes), now writing: a workgroup owns the contiguous bit range of
//                     its unit, assembles it in a JS_EXPORT_WINDOW-byte LDS window by LDS atomic OR, stores the interior words coalesced and ORs the first
//                     and the last word, which neighbours share, into zeroed memory.  Bit groups past the window go to memory one atomic OR each: the run
//                     length does not assume the typical block (a tile of worst-case blocks has 52 KiB of bits).
//   k_export_ffcount  FF bytes of every JS_EXPORT_CHUNK-byte chunk of the un-stuffed streams.
//   k_export_stuff    per chunk: an exclusive sum of the FF counts of 16-byte pieces, the stuffed bytes assembled in LDS, written out byte-coalesced at the
//                     file's place; the first chunk's workgroup also copies the header the host built, the last one writes EOI and the file length.
// With the images' own Huffman tables (jsnoop_batch_export_jpeg_coded, JSNOOP_HUFFMAN_OPTIMAL; the definition: tests/export_opt_model.py) two kernels run in front:
//   k_export_symbols  the same walk with a sink that counts symbols: a tile histogram in LDS, added to the entry's 544 counters.
//   k_export_huff     per entry, a wave per table: T.81 Annex K.2 (code sizes by merging groups, Adjust_BITS, the reserved code point, the symbol order, Annex C
//                     codes), the entry's own code words and its header with the DHT segments it built.
// and k_export_measure / k_export_bits read every entry's own code words (tab_stride words apart; 0: one set for all, the Annex K export).
// With restart intervals (jsnoop_batch_export_jpeg_rst; the definition: tests/export_rst_model.py; arithmetic and the scan operator: jsnoop_export_rst_check.h)
// k_export_measure, k_export_symbols and k_export_bits run in their RST form -- a template parameter: the plain instantiations are the code they were -- and two kernels
// take the place of their plain siblings:
//   the RST forms      the DC predecessor is 0 at every interval start (ex_dc_diff); an interval starts on a byte, so blocks are placed by a segmented scan of run
//                      summaries (JsRstSum, js_rst_combine) in place of the plain sums; the thread of an interval's last block appends its padding ones and writes the
//                      interval's end into the entry's interval table.
//   k_export_rst_scan  k_export_scan over the tiles' summaries, a 64-bit bit position as the carry.
//   k_export_stuff_rst k_export_stuff that finds the interval of its bytes in the interval table and writes FF D0+(r & 7) behind the last byte of interval r.
// Words of the bit stream are kept MSB-first as numbers and byte-swapped when they leave for memory.
#include <hip/hip_runtime.h>
#include "../../include/jsnoop_gpu.h"
#include "jsnoop_launch.h"
#include "jsnoop_export_rst_check.h"

#define EX_THREADS 256
#define EX_ROW_HALVES 66u                             /* 132 bytes: 33 dwords */
#define EX_WIN_WORDS (JS_EXPORT_WINDOW / 4u)
static_assert(JS_EXPORT_TILE == EX_THREADS && JS_EXPORT_SCAN == EX_THREADS && JS_EXPORT_CHUNK == EX_THREADS * 16u, "a thread owns a block / a unit / 16 bytes");

typedef uint32_t ex_u32x4 __attribute__((ext_vector_type(4)));
__constant__ uint8_t c_ex_zigzag[64] = JS_ZIGZAG_NATURAL;
__constant__ uint8_t c_ex_zzpos[64] = JS_ZIGZAG_POSITION;

// the last k with base[k] <= u (base[0] = 0, base[n] > u)
__device__ __forceinline__ uint32_t ex_find(const uint32_t* __restrict__ base, uint32_t n, uint32_t u)
{
    uint32_t k = 0;
    for (uint32_t top = n; top - k > 1u; ) { const uint32_t mid = (k + top) >> 1; if (base[mid] <= u) k = mid; else top = mid; }
    return k;
}
// exclusive prefix sum over the workgroup; *total = the sum.  s: EX_THREADS words of LDS (free to reuse behind the call).
__device__ __forceinline__ uint32_t ex_scan(uint32_t v, uint32_t* s, uint32_t* total)
{
    const uint32_t t = threadIdx.x;
    s[t] = v; __syncthreads();
    for (uint32_t d = 1; d < EX_THREADS; d <<= 1) {
        const uint32_t a = t >= d ? s[t - d] : 0u; __syncthreads();
        s[t] += a; __syncthreads();
    }
    const uint32_t incl = s[t]; *total = s[EX_THREADS - 1]; __syncthreads();
    return incl - v;
}

// A sink of ex_walk sees every symbol twice: sym(class, symbol) -- class 0 DC, 1 AC -- and put(bits, count) with its code and value bits.
struct ExCount { uint32_t bits = 0; __device__ __forceinline__ void put(uint32_t, uint32_t n) { bits += n; } __device__ __forceinline__ void sym(uint32_t, uint32_t) {} };
// counts symbols into the tile's histogram in LDS (dc: 16 words, ac: 256 words of the block's table id)
struct ExSymbols {
    uint32_t* dc; uint32_t* ac;
    __device__ __forceinline__ void put(uint32_t, uint32_t) {}
    __device__ __forceinline__ void sym(uint32_t cls, uint32_t s) { atomicAdd(cls ? ac + s : dc + s, 1u); }
};
// writes bit groups of at most 27 bits at a running position: into the LDS window where the word lies inside it, else into memory
struct ExEmit {
    uint32_t* win; uint32_t* mem; uint64_t w0, pos;
    __device__ __forceinline__ void word(uint64_t w, uint32_t v) {
        if (!v) return;
        const uint64_t rel = w - w0;
        if (rel < EX_WIN_WORDS) atomicOr(win + (uint32_t)rel, v); else atomicOr(mem + w, __builtin_bswap32(v));
    }
    __device__ __forceinline__ void put(uint32_t v, uint32_t n) {
        const uint32_t off = (uint32_t)pos & 31u; const uint64_t w = pos >> 5;
        if (off + n <= 32u) word(w, v << (32u - off - n));
        else { const uint32_t k = off + n - 32u; word(w, v >> k); word(w + 1u, v << (32u - k)); }
        pos += n;
    }
    __device__ __forceinline__ void sym(uint32_t, uint32_t) {}
};

// One AC value of a block: nothing but a longer run where its level is 0, else the ZRLs the run needs and the symbol (run, category) with the value bits
template <class SINK>
__device__ __forceinline__ void ex_coef(int32_t v, int32_t qz, uint32_t& run, bool& inexact, bool& uncodable, const uint32_t* ac, SINK& sink)
{
    if (!v) { run++; return; }
    int32_t lv = 0;
    if (qz) { lv = v / qz; inexact |= lv * qz != v; } else inexact = true;
    if (!lv) { run++; return; }                                                     // (|v| < q: inexact, and no symbol)
    const uint32_t a = (uint32_t)(lv < 0 ? -lv : lv), cat = 32u - (uint32_t)__clz((int)a);
    uncodable |= a > 1023u;
    while (run > 15u) { const uint32_t e = ac[0xF0]; sink.sym(1u, 0xF0u); sink.put(e & 0xFFFFu, e >> 16); run -= 16u; }
    sink.sym(1u, ((run << 4) | cat) & 255u);
    const uint32_t e = ac[((run << 4) | cat) & 255u], bits = (uint32_t)(lv < 0 ? lv - 1 : lv) & ((1u << cat) - 1u);
    sink.put(((e & 0xFFFFu) << cat) | bits, (e >> 16) + cat);
    run = 0;
}
// One block: Annex F symbols of the DC difference level and the AC levels through `sink`.  row: the block's 64 int16 in LDS in ZIG-ZAG order (ex_stage put them so),
// read two positions a dword, a zero dword being two more of the run; q: the component's multipliers, zig-zag order; dc / ac: (length << 16 | code) by symbol.
// Returns the block's result (JSNOOP_EXPORT_OK / _INEXACT / _UNCODABLE).
template <class SINK>
__device__ __forceinline__ uint32_t ex_walk(const uint16_t* row, int32_t d, const uint16_t* q, const uint32_t* dc, const uint32_t* ac, SINK& sink)
{
    bool inexact = false, uncodable = false;
    {
        const int32_t q0 = q[0]; int32_t lv = 0;
        if (q0) { lv = d / q0; inexact |= lv * q0 != d; } else inexact |= d != 0;
        const uint32_t a = (uint32_t)(lv < 0 ? -lv : lv), cat = 32u - (uint32_t)__clz((int)a);
        uncodable |= a > 2047u;
        sink.sym(0u, cat & 15u);
        const uint32_t e = dc[cat & 15u], bits = (uint32_t)(lv < 0 ? lv - 1 : lv) & ((1u << cat) - 1u);
        sink.put(((e & 0xFFFFu) << cat) | bits, (e >> 16) + cat);
    }
    const uint32_t* row32 = reinterpret_cast<const uint32_t*>(row);                    // (a row starts on a multiple of 132 bytes)
    uint32_t run = 0;
    ex_coef((int32_t)row32[0] >> 16, q[1], run, inexact, uncodable, ac, sink);          // position 1; position 0, the arena's slot 0, is not read
    for (uint32_t w = 1; w < 32u; w++) {
        const uint32_t two = row32[w];
        if (!two) { run += 2u; continue; }
        ex_coef((int32_t)(int16_t)(two & 0xFFFFu), q[2u * w], run, inexact, uncodable, ac, sink);
        ex_coef((int32_t)two >> 16, q[2u * w + 1u], run, inexact, uncodable, ac, sink);
    }
    if (run) { const uint32_t e = ac[0]; sink.sym(1u, 0u); sink.put(e & 0xFFFFu, e >> 16); }
    return uncodable ? JSNOOP_EXPORT_UNCODABLE : (inexact ? JSNOOP_EXPORT_INEXACT : JSNOOP_EXPORT_OK);
}

struct ExShared {
    union { uint16_t rows[JS_EXPORT_TILE * EX_ROW_HALVES]; JsRstSum sums[EX_THREADS]; };      // sums: k_export_measure's restart form, behind the walks
    uint16_t q[3][64];
    uint32_t dc[2][16], ac[2][256];
    uint32_t scan[EX_THREADS];
};
// the tile's rows -- turned into zig-zag order on the way: a thread always holds the same eight natural indices, so it looks their positions up once --, the entry's
// multipliers (zig-zag order too) and the code tables into LDS; ends with a barrier
__device__ __forceinline__ void ex_stage(ExShared& s, const int16_t* __restrict__ coef, const JsExportRec& r, uint32_t t0, uint32_t nb, const uint32_t* __restrict__ tabs)
{
    const uint32_t t = threadIdx.x, ch = t & 7u;                                       // (p * EX_THREADS + t) & 7 for every p
    const ex_u32x4* src = reinterpret_cast<const ex_u32x4*>(coef + (r.coef_off + t0) * 64u);
    uint32_t zp[8];
    #pragma unroll
    for (uint32_t e = 0; e < 8u; e++) zp[e] = c_ex_zzpos[ch * 8u + e];
    #pragma unroll
    for (uint32_t p = 0; p < 8u; p++) {
        const uint32_t i = p * EX_THREADS + t, blk = i >> 3;
        if (blk < nb) {
            const ex_u32x4 v = src[i]; uint16_t* o = s.rows + blk * EX_ROW_HALVES;
            o[zp[0]] = (uint16_t)v.x; o[zp[1]] = (uint16_t)(v.x >> 16); o[zp[2]] = (uint16_t)v.y; o[zp[3]] = (uint16_t)(v.y >> 16);
            o[zp[4]] = (uint16_t)v.z; o[zp[5]] = (uint16_t)(v.z >> 16); o[zp[6]] = (uint16_t)v.w; o[zp[7]] = (uint16_t)(v.w >> 16);
        }
    }
    if (t < 192u) s.q[t >> 6][t & 63u] = r.q[t >> 6][c_ex_zigzag[t & 63u]];
    if (t < 32u) s.dc[t >> 4][t & 15u] = tabs[t];
    s.ac[0][t] = tabs[32u + t]; s.ac[1][t] = tabs[288u + t];
    __syncthreads();
}
// what block j of the entry is: its component (0-based) and its DC difference.  rb: the entry's restart interval in blocks (0: none) -- a predecessor in an
// earlier interval counts as 0, so the first block of a component in an interval codes its cumulative value itself
__device__ __forceinline__ int32_t ex_dc_diff(const int16_t* __restrict__ dccum, const JsExportRec* __restrict__ rp, uint64_t coef_off, uint32_t bpm, uint32_t j, uint32_t rb, uint32_t* comp)
{
    const uint32_t pos = j % bpm, back = rp->back[pos];
    *comp = rp->comp[pos];
    const bool have = j >= back && (rb == 0u || j % rb >= back);
    const int32_t cur = dccum[coef_off + j], prev = have ? (int32_t)dccum[coef_off + j - back] : 0;
    return (int32_t)(int16_t)(cur - prev);
}
// exclusive scan of run summaries over the workgroup with js_rst_combine; *total = the summary of all.  s: EX_THREADS summaries of LDS (free to reuse behind the call).
__device__ __forceinline__ JsRstSum ex_rst_scan(JsRstSum v, JsRstSum* s, JsRstSum* total)
{
    const uint32_t t = threadIdx.x;
    s[t] = v; __syncthreads();
    for (uint32_t d = 1; d < EX_THREADS; d <<= 1) {
        JsRstSum a = s[t];
        if (t >= d) a = js_rst_combine(s[t - d], a);
        __syncthreads();
        s[t] = a; __syncthreads();
    }
    const JsRstSum ex = t ? s[t - 1u] : js_rst_identity();
    *total = s[EX_THREADS - 1]; __syncthreads();
    return ex;
}
// block j is the last of its interval (the entry's last block always is)
__device__ __forceinline__ bool ex_rst_ends(uint32_t j, uint32_t nblk, uint32_t rb) { return j + 1u == nblk || (rb && (j + 1u) % rb == 0u); }

// RST (jsnoop_batch_export_jpeg_rst; the definition: tests/export_rst_model.py): the DC predecessor is 0 at every interval start, and a unit's sum is a JsRstSum
template <bool RST>
__global__ void __launch_bounds__(EX_THREADS) k_export_measure(const int16_t* __restrict__ coef, const int16_t* __restrict__ dccum, const JsExportRec* __restrict__ recs,
                                                               const uint32_t* __restrict__ unit_base, uint32_t nrec, const uint32_t* __restrict__ tabs, uint32_t tab_stride /*words from an entry's tables to the next's; 0: one set for all*/,
                                                               uint16_t* __restrict__ blk_bits, uint32_t* __restrict__ unit_bits, uint32_t* __restrict__ res /*[nrec] result, then [nrec][2] lowest block per kind*/,
                                                               const JsExportRstRec* __restrict__ rrecs, JsRstSum* __restrict__ unit_sum /*both: RST only*/)
{
    __shared__ ExShared s;
    __shared__ uint32_t s_red[4];                                 // sum of bits, result, lowest inexact block, lowest uncodable block
    const uint32_t t = threadIdx.x, unit = blockIdx.x, k = ex_find(unit_base, nrec, unit);
    const JsExportRec* rp = recs + k;
    const uint32_t t0 = (unit - unit_base[k]) * JS_EXPORT_TILE, nblk = rp->nblk, nb = min(JS_EXPORT_TILE, nblk - t0), bpm = rp->bpm;
    const uint64_t coef_off = rp->coef_off;
    uint32_t rb = 0u;
    if constexpr (RST) rb = rrecs[k].ri_blocks;
    uint32_t my_bits = 0u; bool my_end = false;                      // (RST: this thread's leaf; a thread without a block has the identity)
    if (t == 0) { s_red[0] = 0u; s_red[1] = 0u; s_red[2] = 0xFFFFFFFFu; s_red[3] = 0xFFFFFFFFu; }
    ex_stage(s, coef, *rp, t0, nb, tabs + (size_t)k * tab_stride);
    if (t < nb) {
        const uint32_t j = t0 + t; uint32_t c;
        const int32_t d = ex_dc_diff(dccum, rp, coef_off, bpm, j, rb, &c);
        const uint32_t tb = c ? 1u : 0u;
        ExCount sink;
        const uint32_t st = ex_walk(s.rows + t * EX_ROW_HALVES, d, s.q[c], s.dc[tb], s.ac[tb], sink);
        blk_bits[rp->blk_base + j] = (uint16_t)sink.bits;
        if constexpr (RST) { my_bits = sink.bits; my_end = ex_rst_ends(j, nblk, rb); } else atomicAdd(&s_red[0], sink.bits);
        if (st) { atomicMax(&s_red[1], st); atomicMin(&s_red[1u + st], j); }
    }
    if constexpr (RST) {
        __syncthreads();                                              // every walk is done: the summaries are scanned where the tile's rows lay
        JsRstSum all;
        ex_rst_scan(js_rst_leaf(my_bits, my_end), s.sums, &all);
        if (t == 0) { JsRstSum* o = unit_sum + unit; o->has = all.has; o->head = all.head; o->mid = all.mid; o->tail = all.tail; }
    }
    __syncthreads();
    if (t == 0) {
        if constexpr (!RST) unit_bits[unit] = s_red[0];
        if (s_red[1]) {
            atomicMax(res + k, s_red[1]);
            if (s_red[2] != 0xFFFFFFFFu) atomicMin(res + nrec + 2u * k, s_red[2]);
            if (s_red[3] != 0xFFFFFFFFu) atomicMin(res + nrec + 2u * k + 1u, s_red[3]);
        }
    }
}

// off[i] = the sum of cnt[base[k] .. i) for every i of entry k; total[k] = the entry's sum
__global__ void __launch_bounds__(EX_THREADS) k_export_scan(const uint32_t* __restrict__ cnt, uint64_t* __restrict__ off, const uint32_t* __restrict__ base, uint64_t* __restrict__ total)
{
    __shared__ uint32_t s[EX_THREADS];
    const uint32_t t = threadIdx.x, k = blockIdx.x, a = base[k], e = base[k + 1];
    uint64_t carry = 0;
    for (uint32_t i0 = a; i0 < e; i0 += JS_EXPORT_SCAN) {           // (a, e, i0: the same in every thread -- the barriers inside ex_scan are met by all)
        const uint32_t i = i0 + t, v = i < e && i >= i0 ? cnt[i] : 0u;
        uint32_t step;
        const uint32_t ex = ex_scan(v, s, &step);
        if (i < e && i >= i0) off[i] = carry + ex;
        carry += step;
        if (e - i0 <= JS_EXPORT_SCAN) break;                        // (i0 + JS_EXPORT_SCAN must not wrap)
    }
    if (t == 0) total[k] = carry;
}

// k_export_scan for the units of a call with restart intervals: the bit position of every unit's first block (off[i]) from the units' summaries, JS_EXPORT_SCAN at a
// time with js_rst_combine in place of the sum and a 64-bit position as the carry; total[k]: the length of the entry's stream in bits (every interval padded, so
// a multiple of 8: the entry's last block ends an interval)
__global__ void __launch_bounds__(EX_THREADS) k_export_rst_scan(const JsRstSum* __restrict__ sum, uint64_t* __restrict__ off, const uint32_t* __restrict__ base, uint64_t* __restrict__ total)
{
    __shared__ JsRstSum s[EX_THREADS];
    const uint32_t t = threadIdx.x, k = blockIdx.x, a = base[k], e = base[k + 1];
    uint64_t carry = 0;
    for (uint32_t i0 = a; i0 < e; i0 += JS_EXPORT_SCAN) {           // (a, e, i0: the same in every thread -- the barriers inside ex_rst_scan are met by all)
        const uint32_t i = i0 + t; const bool mine = i < e && i >= i0;
        JsRstSum step;
        const JsRstSum ex = ex_rst_scan(mine ? sum[i] : js_rst_identity(), s, &step);
        if (mine) off[i] = js_rst_apply(carry, ex);
        carry = js_rst_apply(carry, step);
        if (e - i0 <= JS_EXPORT_SCAN) break;                        // (i0 + JS_EXPORT_SCAN must not wrap)
    }
    if (t == 0) total[k] = carry;
}

// RST: blocks are placed by the summaries (an interval starts on a byte), the thread that owns the last block of an interval appends its padding ones and writes the
// interval's end, in bytes, into the entry's interval table -- the entry's end is the last case of that rule
template <bool RST>
__global__ void __launch_bounds__(EX_THREADS) k_export_bits(const int16_t* __restrict__ coef, const int16_t* __restrict__ dccum, const JsExportRec* __restrict__ recs,
                                                            const uint32_t* __restrict__ unit_base, uint32_t nrec, const uint32_t* __restrict__ tabs, uint32_t tab_stride,
                                                            const uint16_t* __restrict__ blk_bits, const uint64_t* __restrict__ unit_off, uint8_t* __restrict__ ustream,
                                                            const JsExportRstRec* __restrict__ rrecs, uint64_t* __restrict__ itab /*both: RST only*/)
{
    __shared__ ExShared s;
    __shared__ uint32_t s_win[EX_WIN_WORDS];
    const uint32_t t = threadIdx.x, unit = blockIdx.x, k = ex_find(unit_base, nrec, unit);
    const JsExportRec* rp = recs + k;
    if (!rp->live) return;
    const uint32_t t0 = (unit - unit_base[k]) * JS_EXPORT_TILE, nblk = rp->nblk, nb = min(JS_EXPORT_TILE, nblk - t0), bpm = rp->bpm;
    const uint64_t coef_off = rp->coef_off, total_bits = rp->bits;
    uint32_t* mem = reinterpret_cast<uint32_t*>(ustream + rp->u_off);
    for (uint32_t i = t; i < EX_WIN_WORDS; i += EX_THREADS) s_win[i] = 0u;
    ex_stage(s, coef, *rp, t0, nb, tabs + (size_t)k * tab_stride);
    const uint32_t mine = t < nb ? (uint32_t)blk_bits[rp->blk_base + t0 + t] : 0u;
    const uint64_t b0 = unit_off[unit];
    uint64_t b1, at;                                                // the range this workgroup writes: [b0, b1); where this thread's block starts
    uint32_t pad, rb = 0u; bool pads;                               // ones behind this thread's block, up to a whole byte
    if constexpr (RST) {
        __shared__ JsRstSum s_sum[EX_THREADS];
        rb = rrecs[k].ri_blocks;
        const bool ends = t < nb && ex_rst_ends(t0 + t, nblk, rb);
        JsRstSum all;
        const JsRstSum ex = ex_rst_scan(t < nb ? js_rst_leaf(mine, ends) : js_rst_identity(), s_sum, &all);
        at = js_rst_apply(b0, ex); b1 = js_rst_apply(b0, all);
        pads = ends; pad = (uint32_t)(0u - (at + mine)) & 7u;
    } else {
        uint32_t run_bits;
        const uint32_t before = ex_scan(mine, s.scan, &run_bits);
        at = b0 + before; b1 = b0 + run_bits;
        pad = (uint32_t)(0u - total_bits) & 7u;                     // behind the entry's last block
        if (t0 + nb == nblk) b1 += pad;
        pads = t0 + t + 1u == nblk;
    }
    const uint64_t w0 = b0 >> 5, wl = (b1 - 1u) >> 5;               // first and last word of the range (every block has bits: b1 > b0)
    if (t < nb) {
        const uint32_t j = t0 + t; uint32_t c;
        const int32_t d = ex_dc_diff(dccum, rp, coef_off, bpm, j, rb, &c);
        const uint32_t tb = c ? 1u : 0u;
        ExEmit sink{ s_win, mem, w0, at };
        ex_walk(s.rows + t * EX_ROW_HALVES, d, s.q[c], s.dc[tb], s.ac[tb], sink);
        if (pads && pad) sink.put((1u << pad) - 1u, pad);
        if constexpr (RST) { if (pads) itab[rrecs[k].itab_off + (rb ? j / rb : 0u)] = (at + mine + pad) >> 3; }
    }
    __syncthreads();
    const uint64_t nw = wl - w0 + 1u;
    const uint32_t in_win = nw < EX_WIN_WORDS ? (uint32_t)nw : EX_WIN_WORDS;
    for (uint32_t i = t; i < in_win; i += EX_THREADS) {
        const uint32_t v = __builtin_bswap32(s_win[i]);
        if (i == 0u || w0 + i == wl) { if (v) atomicOr(mem + w0 + i, v); }      // shared with the neighbouring range
        else mem[w0 + i] = v;
    }
}

__device__ __forceinline__ uint32_t ex_ff16(ex_u32x4 v, uint32_t valid /*bytes that count, from the first*/)
{
    uint32_t n = 0; const uint32_t w[4] = { v.x, v.y, v.z, v.w };
    #pragma unroll
    for (uint32_t i = 0; i < 16u; i++) n += (i < valid && ((w[i >> 2] >> ((i & 3u) * 8u)) & 255u) == 255u) ? 1u : 0u;
    return n;
}

__global__ void __launch_bounds__(EX_THREADS) k_export_ffcount(const JsExportRec* __restrict__ recs, const uint32_t* __restrict__ chunk_base, uint32_t nrec,
                                                               const uint8_t* __restrict__ ustream, uint32_t* __restrict__ chunk_ff)
{
    __shared__ uint32_t s_n;
    const uint32_t t = threadIdx.x, chunk = blockIdx.x, k = ex_find(chunk_base, nrec, chunk);
    const JsExportRec* rp = recs + k;
    const uint64_t nbytes = (rp->bits + 7u) >> 3, c0 = (uint64_t)(chunk - chunk_base[k]) * JS_EXPORT_CHUNK, at = c0 + t * 16u;
    if (t == 0) s_n = 0u;
    __syncthreads();
    if (at < nbytes) {
        const ex_u32x4 v = *reinterpret_cast<const ex_u32x4*>(ustream + rp->u_off + at);
        const uint32_t n = ex_ff16(v, (uint32_t)min((uint64_t)16u, nbytes - at));
        if (n) atomicAdd(&s_n, n);
    }
    __syncthreads();
    if (t == 0) chunk_ff[chunk] = s_n;
}

__global__ void __launch_bounds__(EX_THREADS) k_export_stuff(const JsExportRec* __restrict__ recs, const uint32_t* __restrict__ chunk_base, uint32_t nrec,
                                                             const uint8_t* __restrict__ ustream, const uint64_t* __restrict__ chunk_off, const uint8_t* __restrict__ hdrs,
                                                             uint8_t* __restrict__ out, uint64_t* __restrict__ len)
{
    __shared__ uint32_t s_scan[EX_THREADS];
    __shared__ uint8_t s_out[2u * JS_EXPORT_CHUNK];
    const uint32_t t = threadIdx.x, chunk = blockIdx.x, k = ex_find(chunk_base, nrec, chunk);
    const JsExportRec* rp = recs + k;
    const uint32_t lc = chunk - chunk_base[k], nchunks = chunk_base[k + 1] - chunk_base[k], hdr_len = rp->hdr_len;
    const uint64_t nbytes = (rp->bits + 7u) >> 3, c0 = (uint64_t)lc * JS_EXPORT_CHUNK, at = c0 + t * 16u;
    const uint32_t here = (uint32_t)min((uint64_t)JS_EXPORT_CHUNK, nbytes - c0);
    uint8_t* file = out + rp->out_off;
    ex_u32x4 v = { 0u, 0u, 0u, 0u }; uint32_t valid = 0;
    if (at < nbytes) { v = *reinterpret_cast<const ex_u32x4*>(ustream + rp->u_off + at); valid = (uint32_t)min((uint64_t)16u, nbytes - at); }
    uint32_t ff_here;
    const uint32_t before = ex_scan(ex_ff16(v, valid), s_scan, &ff_here);
    {
        uint32_t o = t * 16u + before; const uint32_t w[4] = { v.x, v.y, v.z, v.w };
        #pragma unroll
        for (uint32_t i = 0; i < 16u; i++) if (i < valid) {
            const uint32_t b = (w[i >> 2] >> ((i & 3u) * 8u)) & 255u;
            s_out[o++] = (uint8_t)b;
            if (b == 255u) s_out[o++] = 0u;
        }
    }
    __syncthreads();
    uint8_t* dst = file + hdr_len + c0 + chunk_off[chunk];
    const uint32_t n_out = here + ff_here;
    for (uint32_t i = t; i < n_out; i += EX_THREADS) dst[i] = s_out[i];
    if (lc == 0u) { const uint8_t* h = hdrs + rp->hdr_off; for (uint32_t i = t; i < hdr_len; i += EX_THREADS) file[i] = h[i]; }
    if (lc + 1u == nchunks && t == 0u) { dst[n_out] = 0xFFu; dst[n_out + 1u] = 0xD9u; len[k] = (uint64_t)hdr_len + c0 + chunk_off[chunk] + n_out + 2u; }
}

// k_export_stuff for a call with restart intervals.  The un-stuffed stream holds the padded intervals and no marker; byte p of interval r goes to header + p +
// (FFs in front of p) + 2 r, and FF D0+(r & 7) follows the last byte of every interval but the last -- written by the workgroup that owns that byte.  A thread finds
// the interval of its first byte by one search in the entry's interval table (ends in bytes) and advances from there; an interval has at least one byte.
// s_out: every byte leaves as at most four (itself, 00 behind an FF, a marker behind the last of an interval).
__global__ void __launch_bounds__(EX_THREADS) k_export_stuff_rst(const JsExportRec* __restrict__ recs, const JsExportRstRec* __restrict__ rrecs, const uint32_t* __restrict__ chunk_base, uint32_t nrec,
                                                                 const uint8_t* __restrict__ ustream, const uint64_t* __restrict__ chunk_off, const uint64_t* __restrict__ itab_all,
                                                                 const uint8_t* __restrict__ hdrs, uint8_t* __restrict__ out, uint64_t* __restrict__ len)
{
    __shared__ uint32_t s_scan[EX_THREADS];
    __shared__ uint8_t s_out[4u * JS_EXPORT_CHUNK];
    __shared__ uint32_t s_r0, s_n;
    const uint32_t t = threadIdx.x, chunk = blockIdx.x, k = ex_find(chunk_base, nrec, chunk);
    const JsExportRec* rp = recs + k;
    const uint32_t lc = chunk - chunk_base[k], nchunks = chunk_base[k + 1] - chunk_base[k], hdr_len = rp->hdr_len, ni = rrecs[k].ni;
    const uint64_t* itab = itab_all + rrecs[k].itab_off;
    const uint64_t nbytes = rp->bits >> 3, c0 = (uint64_t)lc * JS_EXPORT_CHUNK, at = c0 + t * 16u;
    const uint32_t here = (uint32_t)min((uint64_t)JS_EXPORT_CHUNK, nbytes - c0);
    uint8_t* file = out + rp->out_off;
    ex_u32x4 v = { 0u, 0u, 0u, 0u }; uint32_t valid = 0, r = 0;
    if (at < nbytes) {
        v = *reinterpret_cast<const ex_u32x4*>(ustream + rp->u_off + at); valid = (uint32_t)min((uint64_t)16u, nbytes - at);
        for (uint32_t top = ni - 1u; r < top; ) { const uint32_t mid = (r + top) >> 1; if (itab[mid] > at) top = mid; else r = mid + 1u; }      // the first interval that ends behind `at` (the last ends at nbytes)
    }
    if (t == 0) s_r0 = r;                                           // (the chunk's first byte exists: thread 0 searched)
    uint32_t ff_here;
    const uint32_t before = ex_scan(ex_ff16(v, valid), s_scan, &ff_here);
    const uint32_t r0 = s_r0;
    if (valid) {
        uint32_t o = t * 16u + before + 2u * (r - r0); const uint32_t w[4] = { v.x, v.y, v.z, v.w };
        uint64_t end = itab[r];
        #pragma unroll
        for (uint32_t i = 0; i < 16u; i++) if (i < valid) {
            const uint32_t b = (w[i >> 2] >> ((i & 3u) * 8u)) & 255u;
            s_out[o++] = (uint8_t)b;
            if (b == 255u) s_out[o++] = 0u;
            if (at + i + 1u == end) {
                if (r + 1u < ni) { s_out[o++] = 0xFFu; s_out[o++] = (uint8_t)(0xD0u + (r & 7u)); end = itab[r + 1u]; }
                r++;
            }
        }
        if (t * 16u + valid == here) s_n = o;                       // the thread with the chunk's last byte: everything the chunk writes
    }
    __syncthreads();
    const uint64_t first = (uint64_t)hdr_len + c0 + chunk_off[chunk] + 2u * (uint64_t)r0;
    uint8_t* dst = file + first;
    const uint32_t n_out = s_n;
    for (uint32_t i = t; i < n_out; i += EX_THREADS) dst[i] = s_out[i];
    if (lc == 0u) { const uint8_t* h = hdrs + rp->hdr_off; for (uint32_t i = t; i < hdr_len; i += EX_THREADS) file[i] = h[i]; }
    if (lc + 1u == nchunks && t == 0u) { dst[n_out] = 0xFFu; dst[n_out + 1u] = 0xD9u; len[k] = first + n_out + 2u; }
}

// ---- JSNOOP_HUFFMAN_OPTIMAL: the symbol counts of every entry, and T.81 Annex K.2 per entry and table (the definition: tests/export_opt_model.py) ----
// k_export_symbols: k_export_measure's geometry, the same walk with a sink that counts: LDS atomics into a tile histogram laid out like the code tables, the words
// that are not zero added to the entry's (indices masked in ex_walk: an uncodable entry stays inside its 544 words).
template <bool RST>
__global__ void __launch_bounds__(EX_THREADS) k_export_symbols(const int16_t* __restrict__ coef, const int16_t* __restrict__ dccum, const JsExportRec* __restrict__ recs,
                                                               const uint32_t* __restrict__ unit_base, uint32_t nrec, const uint32_t* __restrict__ tabs, JsExportOptStat* __restrict__ stats,
                                                               const JsExportRstRec* __restrict__ rrecs /*RST only*/)
{
    __shared__ ExShared s;
    __shared__ uint32_t s_hist[JS_EXPORT_TAB_WORDS];
    const uint32_t t = threadIdx.x, unit = blockIdx.x, k = ex_find(unit_base, nrec, unit);
    const JsExportRec* rp = recs + k;
    const uint32_t t0 = (unit - unit_base[k]) * JS_EXPORT_TILE, nblk = rp->nblk, nb = min(JS_EXPORT_TILE, nblk - t0), bpm = rp->bpm;
    const uint64_t coef_off = rp->coef_off;
    for (uint32_t i = t; i < JS_EXPORT_TAB_WORDS; i += EX_THREADS) s_hist[i] = 0u;
    ex_stage(s, coef, *rp, t0, nb, tabs);
    if (t < nb) {
        uint32_t c;
        uint32_t rb = 0u;
        if constexpr (RST) rb = rrecs[k].ri_blocks;
        const int32_t d = ex_dc_diff(dccum, rp, coef_off, bpm, t0 + t, rb, &c);
        const uint32_t tb = c ? 1u : 0u;
        ExSymbols sink{ s_hist + tb * 16u, s_hist + 32u + tb * 256u };
        ex_walk(s.rows + t * EX_ROW_HALVES, d, s.q[c], s.dc[tb], s.ac[tb], sink);
    }
    __syncthreads();
    uint32_t* freq = stats[k].freq;
    for (uint32_t i = t; i < JS_EXPORT_TAB_WORDS; i += EX_THREADS) { const uint32_t v = s_hist[i]; if (v) atomicAdd(freq + i, v); }
}

#define EX_HUFF_DEAD 0xFFFFFFFFFFFFFFFFull
__device__ __forceinline__ uint64_t ex_wave_min(uint64_t v)
{
    #pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const uint64_t o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
// k_export_huff: one workgroup per entry, wave w builds the table of slot w (2 * table id + class).  A lane holds symbols 5 * lane .. 5 * lane + 4 of the 257 (256: the
// reserved one, frequency 1) in registers: the key (frequency << 9 | 511 - symbol) of a live group head -- the least key is the least frequency and, among equals,
// the LARGEST symbol --, the code size and the group id.  A merge is two wave-wide minima and one step over the five: every symbol of group c1 or c2 gets one more
// bit and the id c1 (what K.2's OTHERS chains do one link at a time).  Then lengths are counted, one lane runs Adjust_BITS (Figure K.3) and takes the reserved
// code point off the longest length, the symbols are ranked by (code size, symbol) and get their Annex C codes.  The whole workgroup then puts the entry's header
// together.  Every barrier is met by all four waves: a slot the image does not have runs along with nothing but the reserved symbol.
// (k_prog_huff of jsnoop_export_prog.hip REPEATS this procedure for the progressive export's records: a fix to either belongs in both.)
__global__ void __launch_bounds__(EX_THREADS) k_export_huff(const JsExportRec* __restrict__ recs, const JsExportOptRec* __restrict__ orecs, const uint32_t* __restrict__ unit_base,
                                                            const uint8_t* __restrict__ hdrs, JsExportOptStat* __restrict__ stats, uint32_t* __restrict__ tabs,
                                                            uint8_t* __restrict__ hdr_out, uint32_t* __restrict__ hdr_len)
{
    __shared__ uint16_t s_size[4][264];                 // code size by symbol; 0xFFFF: the symbol does not occur
    __shared__ uint32_t s_bits[4][264];                 // symbols by code size (0 .. 257)
    __shared__ uint8_t s_syms[4][256];                  // symbols in code order
    __shared__ uint32_t s_start[4][18], s_first[4][18]; // rank and code of the first symbol of every length 1 .. 16; s_start[w][17] = the number of symbols
    const uint32_t t = threadIdx.x, k = blockIdx.x, w = t >> 6, lane = t & 63u;
    if (unit_base[k + 1] == unit_base[k]) { if (t == 0) hdr_len[k] = 0u; return; }      // (an unsupported entry: nothing was counted)
    const JsExportOptRec o = orecs[k];
    const bool have = w < o.nslots;
    const uint32_t cls = w & 1u, tb = w >> 1, nsymbols = cls ? 256u : 16u;
    const uint32_t* freq = stats[k].freq + (cls ? 32u + tb * 256u : tb * 16u);
    uint64_t key[5]; uint32_t size[5], group[5];
    #pragma unroll
    for (uint32_t e = 0; e < 5u; e++) {
        const uint32_t sy = lane * 5u + e;
        const uint64_t f = sy == 256u ? 1u : (have && sy < nsymbols ? (uint64_t)freq[sy] : 0u);
        key[e] = f ? (f << 9 | (511u - sy)) : EX_HUFF_DEAD; size[e] = 0u; group[e] = f ? sy : 0xFFFFu;
    }
    for (;;) {
        uint64_t m = key[0];
        #pragma unroll
        for (uint32_t e = 1; e < 5u; e++) m = key[e] < m ? key[e] : m;
        const uint64_t m1 = ex_wave_min(m);
        m = EX_HUFF_DEAD;
        #pragma unroll
        for (uint32_t e = 0; e < 5u; e++) m = key[e] != m1 && key[e] < m ? key[e] : m;
        const uint64_t m2 = ex_wave_min(m);
        if (m2 == EX_HUFF_DEAD) break;                              // one group left (the same in every lane)
        const uint32_t c1 = 511u - (uint32_t)(m1 & 511u), c2 = 511u - (uint32_t)(m2 & 511u);
        const uint64_t merged = ((m1 >> 9) + (m2 >> 9)) << 9 | (511u - c1);      // (sums in 64 bits: below 2^33)
        #pragma unroll
        for (uint32_t e = 0; e < 5u; e++) {
            if (key[e] == m1) key[e] = merged; else if (key[e] == m2) key[e] = EX_HUFF_DEAD;
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
                if (!j || bits[i] < 2u) { sound = false; break; }   // (no code tree has such counts)
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
    uint32_t* my_tabs = tabs + (size_t)k * JS_EXPORT_TAB_WORDS + (cls ? 32u + tb * 256u : tb * 16u);
    #pragma unroll
    for (uint32_t e = 0; e < 5u; e++) {
        const uint32_t sy = lane * 5u + e;
        if (sy >= nsymbols) continue;
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
    JsExportOptSlot* slot = stats[k].slot + w;
    if (lane == 0u) slot->nsym = have ? s_start[w][17] : 0u;
    if (lane < 16u) slot->counts[lane] = have ? (uint8_t)s_bits[w][lane + 1u] : (uint8_t)0u;
    for (uint32_t i = lane; i < 256u; i += 64u) slot->syms[i] = have ? s_syms[w][i] : (uint8_t)0u;
    // the header: the host's bytes up to SOF, a DHT segment per slot, the host's SOS
    uint32_t seg_at[5]; seg_at[0] = o.pre_len;
    #pragma unroll
    for (uint32_t q = 0; q < 4u; q++) seg_at[q + 1u] = seg_at[q] + (q < o.nslots ? 21u + s_start[q][17] : 0u);
    const uint32_t total = min(seg_at[4] + o.sos_len, JS_EXPORT_OPT_HDR);
    const uint8_t* h = hdrs + recs[k].hdr_off; uint8_t* out = hdr_out + (size_t)k * JS_EXPORT_OPT_HDR;
    for (uint32_t i = t; i < total; i += EX_THREADS) {
        uint32_t b;
        if (i < o.pre_len) b = h[i];
        else if (i >= seg_at[4]) b = h[o.sos_off + (i - seg_at[4])];
        else {
            uint32_t q = 0u;
            #pragma unroll
            for (uint32_t r = 1; r < 4u; r++) q += i >= seg_at[r] ? 1u : 0u;
            const uint32_t rel = i - seg_at[q], n = s_start[q][17];
            b = rel == 0u ? 0xFFu : rel == 1u ? 0xC4u : rel == 2u ? (19u + n) >> 8 : rel == 3u ? (19u + n) & 255u : rel == 4u ? ((q & 1u) << 4 | q >> 1)
              : rel < 21u ? s_bits[q][rel - 4u] : (uint32_t)s_syms[q][(rel - 21u) & 255u];
        }
        out[i] = (uint8_t)b;
    }
    if (t == 0u) hdr_len[k] = total;
}

int js_launch_export_measure(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                             const uint32_t* tabs, uint16_t* blk_bits, uint32_t* unit_bits, uint64_t* unit_off, uint32_t* res, uint64_t* ent_bits)
{
    if (!nrec) return 0;
    if (total_units) hipLaunchKernelGGL(k_export_measure<false>, dim3(total_units), dim3(EX_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, tabs, 0u, blk_bits, unit_bits, res, (const JsExportRstRec*)nullptr, (JsRstSum*)nullptr);
    hipLaunchKernelGGL(k_export_scan, dim3(nrec), dim3(EX_THREADS), 0, st, unit_bits, unit_off, unit_base, ent_bits);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int js_launch_export_measure_opt(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const JsExportOptRec* orecs, const uint32_t* unit_base,
                                 uint32_t nrec, uint32_t total_units, const uint32_t* annex_tabs, const uint8_t* hdrs, JsExportOptStat* stats, uint32_t* tabs, uint8_t* hdr_out,
                                 uint32_t* hdr_len, uint16_t* blk_bits, uint32_t* unit_bits, uint64_t* unit_off, uint32_t* res, uint64_t* ent_bits)
{
    if (!nrec) return 0;
    if (total_units) hipLaunchKernelGGL(k_export_symbols<false>, dim3(total_units), dim3(EX_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, annex_tabs, stats, (const JsExportRstRec*)nullptr);
    hipLaunchKernelGGL(k_export_huff, dim3(nrec), dim3(EX_THREADS), 0, st, recs, orecs, unit_base, hdrs, stats, tabs, hdr_out, hdr_len);
    if (total_units) hipLaunchKernelGGL(k_export_measure<false>, dim3(total_units), dim3(EX_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, tabs, JS_EXPORT_TAB_WORDS, blk_bits, unit_bits, res, (const JsExportRstRec*)nullptr, (JsRstSum*)nullptr);
    hipLaunchKernelGGL(k_export_scan, dim3(nrec), dim3(EX_THREADS), 0, st, unit_bits, unit_off, unit_base, ent_bits);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
static int ex_launch_write(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const uint32_t* unit_base, const uint32_t* chunk_base, uint32_t nrec,
                           uint32_t total_units, uint32_t total_chunks, const uint32_t* tabs, uint32_t tab_stride, const uint16_t* blk_bits, const uint64_t* unit_off, uint8_t* ustream,
                           uint32_t* chunk_ff, uint64_t* chunk_off, uint64_t* ent_ff, const uint8_t* hdrs, uint8_t* out, uint64_t* len)
{
    if (!nrec || !total_units || !total_chunks) return 0;
    hipLaunchKernelGGL(k_export_bits<false>, dim3(total_units), dim3(EX_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, tabs, tab_stride, blk_bits, unit_off, ustream, (const JsExportRstRec*)nullptr, (uint64_t*)nullptr);
    hipLaunchKernelGGL(k_export_ffcount, dim3(total_chunks), dim3(EX_THREADS), 0, st, recs, chunk_base, nrec, ustream, chunk_ff);
    hipLaunchKernelGGL(k_export_scan, dim3(nrec), dim3(EX_THREADS), 0, st, chunk_ff, chunk_off, chunk_base, ent_ff);
    hipLaunchKernelGGL(k_export_stuff, dim3(total_chunks), dim3(EX_THREADS), 0, st, recs, chunk_base, nrec, ustream, chunk_off, hdrs, out, len);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int js_launch_export_write(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const uint32_t* unit_base, const uint32_t* chunk_base, uint32_t nrec,
                           uint32_t total_units, uint32_t total_chunks, const uint32_t* tabs, const uint16_t* blk_bits, const uint64_t* unit_off, uint8_t* ustream,
                           uint32_t* chunk_ff, uint64_t* chunk_off, uint64_t* ent_ff, const uint8_t* hdrs, uint8_t* out, uint64_t* len)
{
    return ex_launch_write(st, coef, dccum, recs, unit_base, chunk_base, nrec, total_units, total_chunks, tabs, 0u, blk_bits, unit_off, ustream, chunk_ff, chunk_off, ent_ff, hdrs, out, len);
}
int js_launch_export_write_opt(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const uint32_t* unit_base, const uint32_t* chunk_base, uint32_t nrec,
                               uint32_t total_units, uint32_t total_chunks, const uint32_t* tabs, const uint16_t* blk_bits, const uint64_t* unit_off, uint8_t* ustream,
                               uint32_t* chunk_ff, uint64_t* chunk_off, uint64_t* ent_ff, const uint8_t* hdrs, uint8_t* out, uint64_t* len)
{
    return ex_launch_write(st, coef, dccum, recs, unit_base, chunk_base, nrec, total_units, total_chunks, tabs, JS_EXPORT_TAB_WORDS, blk_bits, unit_off, ustream, chunk_ff, chunk_off, ent_ff, hdrs, out, len);
}

// ---- jsnoop_batch_export_jpeg_rst: the two phases with the restart forms of the kernels.  orecs == NULL: the Annex K tables (annex_tabs: one set), else every entry's own.
int js_launch_export_measure_rst(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const JsExportOptRec* orecs, const JsExportRstRec* rrecs,
                                 const uint32_t* unit_base, uint32_t nrec, uint32_t total_units, const uint32_t* annex_tabs, const uint8_t* hdrs, JsExportOptStat* stats, uint32_t* tabs,
                                 uint8_t* hdr_out, uint32_t* hdr_len, uint16_t* blk_bits, JsRstSum* unit_sum, uint64_t* unit_off, uint32_t* res, uint64_t* ent_bits)
{
    if (!nrec) return 0;
    if (orecs) {
        if (total_units) hipLaunchKernelGGL(k_export_symbols<true>, dim3(total_units), dim3(EX_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, annex_tabs, stats, rrecs);
        hipLaunchKernelGGL(k_export_huff, dim3(nrec), dim3(EX_THREADS), 0, st, recs, orecs, unit_base, hdrs, stats, tabs, hdr_out, hdr_len);
    }
    if (total_units) hipLaunchKernelGGL(k_export_measure<true>, dim3(total_units), dim3(EX_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, orecs ? (const uint32_t*)tabs : annex_tabs,
                                        orecs ? JS_EXPORT_TAB_WORDS : 0u, blk_bits, (uint32_t*)nullptr, res, rrecs, unit_sum);
    hipLaunchKernelGGL(k_export_rst_scan, dim3(nrec), dim3(EX_THREADS), 0, st, (const JsRstSum*)unit_sum, unit_off, unit_base, ent_bits);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int js_launch_export_write_rst(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const JsExportRstRec* rrecs, const uint32_t* unit_base,
                               const uint32_t* chunk_base, uint32_t nrec, uint32_t total_units, uint32_t total_chunks, const uint32_t* tabs, uint32_t tab_stride, const uint16_t* blk_bits,
                               const uint64_t* unit_off, uint64_t* itab, uint8_t* ustream, uint32_t* chunk_ff, uint64_t* chunk_off, uint64_t* ent_ff, const uint8_t* hdrs, uint8_t* out, uint64_t* len)
{
    if (!nrec || !total_units || !total_chunks) return 0;
    hipLaunchKernelGGL(k_export_bits<true>, dim3(total_units), dim3(EX_THREADS), 0, st, coef, dccum, recs, unit_base, nrec, tabs, tab_stride, blk_bits, unit_off, ustream, rrecs, itab);
    hipLaunchKernelGGL(k_export_ffcount, dim3(total_chunks), dim3(EX_THREADS), 0, st, recs, chunk_base, nrec, (const uint8_t*)ustream, chunk_ff);
    hipLaunchKernelGGL(k_export_scan, dim3(nrec), dim3(EX_THREADS), 0, st, (const uint32_t*)chunk_ff, chunk_off, chunk_base, ent_ff);
    hipLaunchKernelGGL(k_export_stuff_rst, dim3(total_chunks), dim3(EX_THREADS), 0, st, recs, rrecs, chunk_base, nrec, (const uint8_t*)ustream, (const uint64_t*)chunk_off, (const uint64_t*)itab, hdrs, out, len);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- jsnoop_batch_export_jpeg_prog (jsnoop_export_prog.hip) places its tiles and chunks with the two scan kernels above, one "entry" per (entry, scan) record
int js_launch_export_scan(hipStream_t st, const uint32_t* cnt, uint64_t* off, const uint32_t* base, uint32_t nrec, uint64_t* total)
{
    if (!nrec) return 0;
    hipLaunchKernelGGL(k_export_scan, dim3(nrec), dim3(EX_THREADS), 0, st, cnt, off, base, total);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int js_launch_export_rst_scan(hipStream_t st, const JsRstSum* sum, uint64_t* off, const uint32_t* base, uint32_t nrec, uint64_t* total)
{
    if (!nrec) return 0;
    hipLaunchKernelGGL(k_export_rst_scan, dim3(nrec), dim3(EX_THREADS), 0, st, sum, off, base, total);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
