// jsnoop_progressive.hip -- progressive (SOF2) scan decode, SURVEY.md 8(f) rank 4 / BASELINE.json config 5
// ("progressive multi-scan 4:2:2 JPEG with RSTn restart intervals, per-interval parallel entropy decode").
//
// The reference refuses SOF2 (source/JfifDecode.cpp:4827-4833, :5272-5274), so there is no reference answer for these
// files; the contract is transitive: a progressive file that carries the same quantised coefficients as a baseline
// file must come out with the baseline file's pixels.  The scans therefore only rebuild the coefficient arena of the
// baseline path -- `coef` (natural order, one 64-entry row per block in decode order) and `dccum` -- and the unchanged
// back end (k_idct_color: the reference's fp32 IDCT, replication, colour conversion, DIB) runs on it.
//
// Entropy decoding follows ITU-T T.81 Annex G: DC first / refinement scans (G.1.2.1), AC first scans with EOBRUN
// (G.1.2.2) and AC refinement scans with correction bits (G.1.2.3), spectral selection and successive approximation.
// Parallelism is what the stream offers without speculation: restart intervals are independent, so every
// (scan, interval) pair is one wave with its own bit reader (one lane of it for the DC and AC-first scans, all 64 for AC
// refinement); scans that touch different coefficients run side by side (jsnoop_progressive.cpp orders them into levels).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "jsnoop_types.h"
#include "jsnoop_progressive.h"

__device__ __constant__ uint8_t c_zz_nat[64] = {       // zig-zag index -> natural index (T.81 Figure A.6)
     0, 1, 8,16, 9, 2, 3,10, 17,24,32,25,18,11, 4, 5, 12,19,26,33,40,48,41,34, 27,20,13, 6, 7,14,21,28,
    35,42,49,56,57,50,43,36, 29,22,15,23,30,37,44,51, 58,59,52,45,38,31,39,46, 53,60,61,54,47,55,62,63 };

// Active lanes (restart intervals) per wave of the sequential scan kinds: 1 for small jobs (lanes that share a wave serialise each
// other's branches, and a single file leaves most SIMDs idle anyway), more once a batch fills the chip with waves.

namespace {

// MSB-first bit reader over one restart interval of a scan (file bytes, stuffing removed on the fly).
struct PReader {
    static constexpr bool UNIFORM = false;
    const uint8_t* base; uint32_t pos, end; uint64_t acc; int n; uint32_t over; uint64_t win; uint32_t win_at;
    __device__ void init(const uint8_t* file, uint32_t s, uint32_t e) { base = file; pos = s; end = e; acc = 0; n = 0; over = 0; win = 0; win_at = 0xFFFFFFFFu; }
    // file byte `i` through an 8-byte register window (one aligned 64-bit load per 8 bytes instead of a load per byte)
    __device__ uint32_t byte_at(uint32_t i)
    {
        const uint32_t a = i & ~7u;
        if (a != win_at) { win = *reinterpret_cast<const uint64_t*>(base + a); win_at = a; }
        return (uint32_t)(win >> ((i & 7u) * 8)) & 255u;
    }
    __device__ void fill()
    {
        while (n <= 56) {
            uint32_t b = 0;
            if (pos < end) { b = byte_at(pos++); if (b == 0xFF && pos < end && byte_at(pos) == 0x00) pos++; }    // FF00 -> FF (B.1.1.5)
            else over++;                                                               // past the interval: zero bits, counted
            acc |= (uint64_t)b << (56 - n); n += 8;
        }
    }
    __device__ uint32_t peek(int k) { if (n < k) fill(); return (uint32_t)(acc >> (64 - k)); }
    __device__ void skip(int k) { acc <<= k; n -= k; }
    __device__ uint32_t bits(int k) { if (!k) return 0; const uint32_t v = peek(k); skip(k); return v; }
    __device__ uint32_t bit() { return bits(1); }
    __device__ bool overrun() const { return over * 8 > (uint32_t)(n > 0 ? n : 0); }      // consumed bits that were never in the interval
};

// A value every lane of the wave holds alike, handed to the compiler as such: what is computed from it is scalar work (one issue slot of the
// scalar unit instead of a four-cycle vector instruction -- a lone wave that decodes a chain of dependent symbols is bound by exactly that).
__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uni(uint64_t x) { return (uint64_t)uni((uint32_t)x) | ((uint64_t)uni((uint32_t)(x >> 32)) << 32); }
template <bool U> __device__ __forceinline__ uint32_t uni_if(uint32_t x) { return U ? uni(x) : x; }

// The same reader for a WAVE that decodes ONE interval (a scan without restart markers is a single interval: a 1080p scan is one chain of
// ~10^5 dependent symbols, and a lane that waits ~1 us for every eight file bytes and for every block it updates spends its time waiting).
// All 64 lanes run the decoder identically (same data, same branches: wave-uniform control flow); the file bytes come through a 2 KiB ring
// in LDS that the WAVE fills -- every lane fetches 16 bytes of a 1 KiB chunk, the chunk after the two in the ring is already in flight in
// registers when the reader gets there -- so a byte costs an LDS read instead of a trip to memory.
struct WReader {
    static constexpr bool UNIFORM = true;
    const uint8_t* base; uint4* ring; uint32_t pos, end, limit, ring_c, lane; uint64_t acc; int n; uint32_t over; uint64_t win; uint32_t win_at; uint4 nxt;
    __device__ __forceinline__ uint4 chunk(uint32_t c) const { const uint32_t o = (c << 10) + lane * 16u; return o < limit ? *reinterpret_cast<const uint4*>(base + o) : make_uint4(0u, 0u, 0u, 0u); }
    __device__ __forceinline__ void init(uint4* lds, const uint8_t* file, uint32_t s, uint32_t e, uint32_t file_len, uint32_t lane_)
    {
        base = file; ring = lds; pos = s; end = e; limit = (file_len + 15u) & ~15u; lane = lane_; acc = 0; n = 0; over = 0; win = 0; win_at = 0xFFFFFFFFu;   // (file images are 16-byte aligned and zero padded in the raw arena)
        ring_c = s >> 10;
        ring[(ring_c & 1u) * 64u + lane] = chunk(ring_c); ring[((ring_c + 1u) & 1u) * 64u + lane] = chunk(ring_c + 1u); nxt = chunk(ring_c + 2u);
        __syncthreads();
    }
    __device__ __forceinline__ uint32_t byte_at(uint32_t i)
    {
        const uint32_t a = i & ~7u;
        if (a != win_at) {
            while ((a >> 10) >= ring_c + 2u) {                     // (wave-uniform; the workgroup IS the wave)
                __syncthreads(); ring[(ring_c & 1u) * 64u + lane] = nxt; ring_c++; nxt = chunk(ring_c + 2u); __syncthreads();
            }
            win = uni(reinterpret_cast<const uint64_t*>(ring)[(a & 2047u) >> 3]); win_at = a;
        }
        return (uint32_t)(win >> ((i & 7u) * 8)) & 255u;
    }
    __device__ __forceinline__ void fill()
    {
        while (n <= 56) {
            uint32_t b = 0;
            if (pos < end) { b = byte_at(pos++); if (b == 0xFF && pos < end && byte_at(pos) == 0x00) pos++; }
            else over++;
            acc |= (uint64_t)b << (56 - n); n += 8;
        }
    }
    __device__ __forceinline__ uint32_t peek(int k) { if (n < k) fill(); return (uint32_t)(acc >> (64 - k)); }
    __device__ __forceinline__ void skip(int k) { acc <<= k; n -= k; }
    __device__ __forceinline__ uint32_t bits(int k) { if (!k) return 0; const uint32_t v = peek(k); skip(k); return v; }
    __device__ __forceinline__ uint32_t bit() { return bits(1); }
    __device__ __forceinline__ bool overrun() const { return over * 8 > (uint32_t)(n > 0 ? n : 0); }
};

// Canonical Huffman decode (T.81 F.2.2.3): 8-bit look-ahead table, then bit-serial through MAXCODE.
template <class R> __device__ __forceinline__ int huff(R& r, const JsProgTable& t)
{
    const uint32_t la = r.peek(16);
    const uint32_t e = uni_if<R::UNIFORM>(t.look[la >> 8]);
    if (e) { r.skip((int)(e >> 8)); return (int)(e & 255u); }
    for (int l = 9; l <= 16; l++) {
        const int32_t code = (int32_t)(la >> (16 - l));
        if (code <= (int32_t)uni_if<R::UNIFORM>((uint32_t)t.maxcode[l])) { r.skip(l); return (int)uni_if<R::UNIFORM>(t.sym[(code + (int32_t)uni_if<R::UNIFORM>((uint32_t)t.valoff[l])) & 255]); }
    }
    r.skip(16);
    return -1;                                                   // no code matches
}
__device__ __forceinline__ int extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int)v - (int)((1u << s) - 1) : (int)v; }   // F.2.2.1

// decode-order row of block (bx, by) of frame component `comp` (0-based) in the coefficient arena
__device__ __forceinline__ size_t block_row(const JsImage& im, const JsProgFrame& fr, uint32_t comp, uint32_t bx, uint32_t by)
{
    const uint32_t hs = fr.hs[comp], vs = fr.vs[comp];
    return ((size_t)(by / vs) * im.mcu_xmax + bx / hs) * im.blk_per_mcu + fr.first_blk[comp] + (by % vs) * hs + (bx % hs);
}

// The same with the geometry in registers (a sequential decoder must not wait for a descriptor word per block: the stores to the arena
// keep the compiler from holding what it reads through `im` / `fr`).
struct PGeo { uint32_t hs, vs, first, mcu_xmax, bpm; };
__device__ __forceinline__ PGeo geo_of(const JsImage& im, const JsProgFrame& fr, uint32_t comp) { PGeo g; g.hs = fr.hs[comp]; g.vs = fr.vs[comp]; g.first = fr.first_blk[comp]; g.mcu_xmax = im.mcu_xmax; g.bpm = im.blk_per_mcu; return g; }
__device__ __forceinline__ size_t block_row(const PGeo& g, uint32_t bx, uint32_t by) { return ((size_t)(by / g.vs) * g.mcu_xmax + bx / g.hs) * g.bpm + g.first + (by % g.vs) * g.hs + (bx % g.hs); }

// Block u of a non-interleaved scan (the component's nbx x nby grid in scan order, A.2.3) and its row in the arena WITHOUT a division per block
// (six of them -- ~200 vector instructions on a chip without an integer divider -- were most of what a block of a sparse scan cost): the block's
// place in its MCU row is carried along, a jump over an end-of-band run re-seeks.
struct PCursor {
    uint32_t nbx, hs, vs, mcu_xmax, bpm, first, u, bx, rx, mx, ry, my;                      // bx = mx * hs + rx; the block row by = my * vs + ry
    __device__ __forceinline__ void seek(uint32_t to) { u = to; bx = to % nbx; const uint32_t by = to / nbx; rx = bx % hs; mx = bx / hs; ry = by % vs; my = by / vs; }
    __device__ __forceinline__ void init(const PGeo& g, uint32_t nbx_, uint32_t to) { nbx = nbx_; hs = g.hs; vs = g.vs; mcu_xmax = g.mcu_xmax; bpm = g.bpm; first = g.first; seek(to); }
    __device__ __forceinline__ size_t row() const { return ((size_t)my * mcu_xmax + mx) * bpm + first + ry * hs + rx; }
    __device__ __forceinline__ void step()
    {
        u++; bx++; rx++;
        if (rx == hs) { rx = 0; mx++; }
        if (bx == nbx) { bx = 0; rx = 0; mx = 0; ry++; if (ry == vs) { ry = 0; my++; } }
    }
    __device__ __forceinline__ void skip(uint32_t n) { if (n <= 3u) { for (; n; n--) step(); } else seek(u + n); }
};

// The scan's description without arrays: every field a register (an indexed array in a by-value copy sends the whole copy to scratch, and
// then every `k <= se` of the symbol loop is a scratch load).
struct PScanR { uint32_t img, ncomp, c0, c1, c2, ntabs, t0, t1, t2, t3, dc0, dc1, dc2, ac0, ss, se, ah, al, seg_first, nseg, rst_interval, nbx, nby; };
__device__ __forceinline__ PScanR scan_regs(const JsProgScan& S)
{
    PScanR r; r.img = S.img; r.ncomp = S.ncomp; r.c0 = S.comp[0]; r.c1 = S.comp[1]; r.c2 = S.comp[2]; r.ntabs = S.ntabs; r.t0 = S.tab[0]; r.t1 = S.tab[1]; r.t2 = S.tab[2]; r.t3 = S.tab[3];
    r.dc0 = S.dc_slot[0]; r.dc1 = S.dc_slot[1]; r.dc2 = S.dc_slot[2]; r.ac0 = S.ac_slot[0]; r.ss = S.ss; r.se = S.se; r.ah = S.ah; r.al = S.al;
    r.seg_first = S.seg_first; r.nseg = S.nseg; r.rst_interval = S.rst_interval; r.nbx = S.nbx; r.nby = S.nby;
    return r;
}

// One restart interval of one scan, units [u0, u1), through reader `r`.  `writer`: this lane stores what the DC and AC-first kinds decode (the
// wave form runs them in every lane; AC refinement is a wave's work in either form: `lane` = the zig-zag position this lane holds).
template <class R>
__device__ __forceinline__ uint32_t prog_interval(R& r, const bool writer, const uint32_t lane, const PScanR& sc, const JsImage& im, const JsProgFrame& fr,
                                                  const JsProgTable* s_tab, const uint8_t* s_zz, int16_t* cbase, const uint32_t u0, const uint32_t u1)
{
    uint32_t bad = 0;
    const int al = (int)sc.al;
    if (sc.ss == 0) {
        // ---- DC scans (G.1.2.1): interleaved or not; first (Ah = 0): DIFF, point transform; refinement: one bit per block
        int p0 = 0, p1 = 0, p2 = 0;
        const PGeo g0 = geo_of(im, fr, sc.c0), g1 = geo_of(im, fr, sc.ncomp > 1 ? sc.c1 : sc.c0), g2 = geo_of(im, fr, sc.ncomp > 2 ? sc.c2 : sc.c0);
        PCursor cur; cur.init(g0, sc.nbx, sc.ncomp > 1 ? 0u : u0);
        const uint32_t ncomp = sc.ncomp, ah = sc.ah, dcpack = sc.dc0 | sc.dc1 << 8 | sc.dc2 << 16;       // (a select over dc0..dc2 comes back as an indexed load from a scratch copy of the scan)
        for (uint32_t u = u0; u < u1 && !bad; u++) {
            for (uint32_t ci = 0; ci < ncomp; ci++) {
                const PGeo& g = ci == 0 ? g0 : ci == 1 ? g1 : g2;                                                  // (selects, no indexed arrays)
                const JsProgTable& Tdc = s_tab[(dcpack >> (8u * ci)) & 255u];
                const uint32_t hs = ncomp > 1 ? g.hs : 1u, vs = ncomp > 1 ? g.vs : 1u;
                for (uint32_t v = 0; v < vs && !bad; v++) for (uint32_t h = 0; h < hs && !bad; h++) {     // (a stop ends the MCU at once: the `break` below leaves the h loop only)
                    // interleaved (A.2.2): block (v, h) of the component in MCU u -- the arena's rows ARE in that order; else the component's own grid
                    int16_t* blk = cbase + (ncomp > 1 ? (size_t)u * g.bpm + g.first + v * hs + h : cur.row()) * 64;
                    if (ah == 0) {
                        const int s = huff(r, Tdc);
                        if (s < 0 || s > 15) { bad = 1; break; }
                        const int diff = s ? extend(r.bits(s), s) : 0;
                        const int pv = (ci == 0 ? p0 : ci == 1 ? p1 : p2) + diff;
                        if (ci == 0) p0 = pv; else if (ci == 1) p1 = pv; else p2 = pv;
                        if (writer) blk[0] = (int16_t)(pv * (1 << al));
                    } else if (r.bit() && writer) atomicOr(reinterpret_cast<unsigned int*>(blk), 1u << al);      // (no value comes back: the decoder does not wait for the block)
                }
                if (bad) break;
            }
            if (ncomp == 1) cur.step();
        }
    } else if (sc.ah == 0) {
        // ---- AC first scan (G.1.2.2): one component, band Ss..Se, end-of-band runs
        const PGeo g = geo_of(im, fr, sc.c0); const JsProgTable& T = s_tab[sc.ac0];
        PCursor cur; cur.init(g, sc.nbx, u0);
        uint32_t eobrun = 0;
        for (uint32_t u = u0; u < u1 && !bad; u++, cur.step()) {
            if (eobrun) { const uint32_t hop = min(eobrun, u1 - u); eobrun -= hop; u += hop - 1u; cur.skip(hop - 1u); continue; }
            int16_t* blk = cbase + cur.row() * 64;
            for (uint32_t k = sc.ss; k <= sc.se; k++) {
                const int rs = huff(r, T);
                if (rs < 0) { bad = 1; break; }
                const uint32_t run = (uint32_t)rs >> 4, s = (uint32_t)rs & 15u;
                if (s) {
                    k += run;
                    if (k > sc.se) { bad = 1; break; }
                    const int val = extend(r.bits((int)s), (int)s) * (1 << al);
                    if (writer) blk[uni_if<R::UNIFORM>(s_zz[k])] = (int16_t)val;
                } else if (run == 15) k += 15;                                          // ZRL
                else { eobrun = (1u << run) + r.bits((int)run) - 1; break; }             // EOBn: this block ends here, eobrun more follow
            }
        }
    } else {
        // ---- AC refinement scan (G.1.2.3): new coefficients of magnitude 1 << Al, correction bits for the known non-zero ones.
        // The WAVE works on the block: lane l holds the coefficient at zig-zag position l; bit reader and Huffman decode run
        // identically in every lane.  A symbol (run, s) means "pass `run` coefficients with zero history; every non-zero one on
        // the way takes a correction bit; put the new value on the next zero one": the history is one 64-bit ballot, the target
        // position the (run+1)-th set bit of the zero mask (mbcnt + ballot), the correction bits of the whole stretch come out of
        // the reader at once and each lane picks its own by the rank of its position.  The blocks come in scan order whatever the
        // symbols say, so the coefficients of the next two are fetched while this one is worked on.
        const PGeo g = geo_of(im, fr, sc.c0); const JsProgTable& T = s_tab[sc.ac0];
        const int p1 = 1 << al, m1 = -(1 << al);
        const uint64_t below_ss = (1ull << sc.ss) - 1ull, upto_se = sc.se >= 63u ? ~0ull : ((1ull << (sc.se + 1u)) - 1ull);
        const uint64_t bandmask = upto_se & ~below_ss;
        const bool inband = lane >= sc.ss && lane <= sc.se;
        const uint32_t nat = s_zz[lane];
        PCursor cur, ahead; cur.init(g, sc.nbx, u0); ahead.init(g, sc.nbx, u0);            // ahead: the block whose coefficients are fetched next
        auto fetch = [&]() -> int { const int x = (inband && ahead.u < u1) ? (int)cbase[ahead.row() * 64 + nat] : 0; ahead.step(); return x; };
        uint32_t eobrun = 0;
        int v_1 = fetch(), v_2 = fetch();
        for (uint32_t u = u0; u < u1 && !bad; u++) {
            int v = v_1; v_1 = v_2; v_2 = fetch();
            int16_t* const mine = cbase + cur.row() * 64 + nat; cur.step();
            const uint64_t H = __ballot(v != 0) & bandmask;       // non-zero history (positions only grow inside a block: new values never re-enter)
            if (eobrun && !H) { eobrun--; continue; }             // inside an end-of-band run and nothing to correct: the block stays as it is
            const int v_in = v;
            // correction bits for the non-zero-history positions in [from, to): the first bit read belongs to the lowest position
            auto correct = [&](uint32_t from, uint32_t to) {
                const uint64_t range = (to >= 64u ? ~0ull : ((1ull << to) - 1ull)) & ~((1ull << from) - 1ull);
                const uint64_t C = H & range;
                const uint32_t nc = (uint32_t)__builtin_popcountll(C);
                uint64_t cb = 0;                                   // bit j = the j-th correction bit of the stretch
                for (uint32_t got = 0; got < nc; ) {
                    const uint32_t n = min(nc - got, 32u);
                    const uint32_t w = r.bits((int)n);             // MSB first
                    cb |= (uint64_t)(__brev(w) >> (32u - n)) << got; got += n;
                }
                if ((C >> lane) & 1ull) {
                    const uint32_t j = (uint32_t)__builtin_popcountll(C & ((1ull << lane) - 1ull));
                    if (((cb >> j) & 1ull) && !(v & p1)) v += (v >= 0 ? p1 : m1);
                }
            };
            uint32_t k = sc.ss;
            if (!eobrun) {
                while (k <= sc.se) {
                    const int rs = huff(r, T);
                    if (rs < 0) { bad = 1; break; }
                    const int run = rs >> 4; const uint32_t s = (uint32_t)rs & 15u;
                    int newv = 0;
                    if (s) { if (s != 1) { bad = 1; break; } newv = r.bit() ? p1 : m1; }
                    else if (run != 15) { eobrun = (1u << run) + r.bits(run); break; }     // EOBn (this block included)
                    const uint64_t Z = ~H & bandmask & ~((1ull << k) - 1ull);            // zero history from k on
                    const uint32_t zr = __builtin_amdgcn_mbcnt_hi((uint32_t)(Z >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)Z, 0u));
                    const uint64_t tb = __ballot(((Z >> lane) & 1ull) && zr == (uint32_t)run);
                    const uint32_t t = tb ? (uint32_t)__builtin_ctzll(tb) : sc.se + 1u;  // the (run+1)-th of them, or the band ends first
                    correct(k, t);
                    if (newv && t <= sc.se && lane == t) v = newv;
                    k = t + 1u;
                }
            }
            if (eobrun) { correct(k, sc.se + 1u); eobrun--; }      // rest of the band: correction bits only
            if (inband && v != v_in) *mine = (int16_t)v;            // the band only: other scans own the rest of the block
        }
    }
    return bad;
}

}  // namespace

// One wave per restart interval of one scan (pg_lanes == 1: the whole wave decodes it, WReader) or 2 / 4 / 8 intervals per wave, a lane each
// (mid-size batches: more decoders than SIMDs); one launch covers every scan of a dependency level of the batch.
__global__ void __launch_bounds__(64) k_prog_scan(const JsImage* __restrict__ imgs, const JsProgFrame* __restrict__ frames, const JsProgScan* __restrict__ scans,
                                                  const uint32_t* __restrict__ lvl_scans, const uint32_t* __restrict__ lvl_wg, uint32_t nsc, uint32_t pg_lanes,
                                                  const JsProgTable* __restrict__ tabs, const JsProgSeg* __restrict__ segs, const uint8_t* __restrict__ raw,
                                                  int16_t* __restrict__ coef, uint32_t* __restrict__ status_all)
{
    uint32_t lo = 0, hi = nsc;                                   // lvl_wg is an exclusive prefix, nsc + 1 entries
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (lvl_wg[mid] <= blockIdx.x) lo = mid; else hi = mid; }
    const PScanR sc = scan_regs(scans[lvl_scans[lo]]);          // wave-uniform
    const uint32_t wg_in_scan = blockIdx.x - lvl_wg[lo];
    const JsProgFrame& fr = frames[sc.img];
    uint32_t* status = status_all + sc.img * 4u;
    __shared__ JsProgTable s_tab[4];
    __shared__ uint8_t s_zz[64];
    __shared__ uint4 s_ring[128];
    if (threadIdx.x < 64) s_zz[threadIdx.x] = c_zz_nat[threadIdx.x];
    for (uint32_t t = 0; t < sc.ntabs; t++) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(tabs + (((t & 2u) ? (t & 1u ? sc.t3 : sc.t2) : (t & 1u ? sc.t1 : sc.t0)))); uint32_t* dst = reinterpret_cast<uint32_t*>(&s_tab[t]);
        for (uint32_t i = threadIdx.x; i < sizeof(JsProgTable) / 4; i += blockDim.x) dst[i] = src[i];
    }
    __syncthreads();
    const bool wave_coop = sc.ss != 0 && sc.ah != 0;             // AC refinement: the whole wave works on one interval's blocks
    const uint32_t per = wave_coop ? 1u : pg_lanes;                // intervals this wave carries
    const uint32_t lane = threadIdx.x & 63u;
    const JsImage& im = imgs[sc.img];
    int16_t* cbase = coef + im.coef_off * 64;
    const uint32_t units = sc.ncomp > 1 ? im.mcu_xmax * im.mcu_ymax : sc.nbx * sc.nby;     // MCUs of the scan (A.2.2 / A.2.3)
    const uint32_t ri = sc.rst_interval ? sc.rst_interval : units;
    if (per == 1u) {
        const uint32_t iv = wg_in_scan;
        if (iv >= sc.nseg) return;
        const JsProgSeg sg = segs[sc.seg_first + iv];
        WReader r; r.init(s_ring, raw + im.file_off, sg.start, sg.end, im.file_len, lane);
        const uint32_t u0 = iv * ri, u1 = min(units, u0 + ri);
        const uint32_t bad = prog_interval(r, lane == 0u, lane, sc, im, fr, s_tab, s_zz, cbase, u0, u1);
        if (lane == 0u) { if (bad) atomicOr(&status[0], 1u); if (r.overrun()) atomicOr(&status[0], 2u); }     // a code that matches nothing / the interval ended before its blocks did
        return;
    }
    // Lanes that share a wave serialise each other's branches, so only `per` lanes of the wave carry a decoder.
    if (threadIdx.x % (64u / per)) return;
    const uint32_t iv = wg_in_scan * per + threadIdx.x / (64u / per);
    if (iv >= sc.nseg) return;
    const JsProgSeg sg = segs[sc.seg_first + iv];
    PReader r; r.init(raw + im.file_off, sg.start, sg.end);      // file images are 16-byte aligned and zero padded in the raw arena
    const uint32_t u0 = iv * ri, u1 = min(units, u0 + ri);
    const uint32_t bad = prog_interval(r, true, lane, sc, im, fr, s_tab, s_zz, cbase, u0, u1);
    if (bad) atomicOr(&status[0], 1u);
    if (r.overrun()) atomicOr(&status[0], 2u);
}

// Quantised, point-transformed coefficients -> what the baseline path leaves behind: dequantised AC terms in place
// ((short)(val * Q), DecodeIdctSet :2278) and the dequantised DC in `dccum` (the reference's running DC sum equals
// Q * DC in wrapping int16 arithmetic, :3280); slot 0 of the block is cleared (the back end never reads it).
// A lane takes eight consecutive coefficients (16 bytes) of a block, a wave eight blocks per trip: 1 KiB read and 1 KiB written per wave
// instruction pair (the first form moved 2 bytes per lane: 4.3 ms per 512 images, a quarter of what the arena's bytes cost at HBM speed).
__global__ void __launch_bounds__(256) k_prog_finalize(const JsImage* __restrict__ imgs, const JsProgFrame* __restrict__ frames, uint32_t nimg,
                                                       const uint32_t* __restrict__ blk_base, uint32_t total_blocks, int16_t* __restrict__ coef, int16_t* __restrict__ dccum)
{
    __shared__ __attribute__((aligned(16))) int16_t s_q[3][64];
    const uint32_t lane = threadIdx.x & 63, sub = lane & 7u, boff = lane >> 3;
    (void)blk_base; (void)total_blocks;
    for (uint32_t img = blockIdx.y; img < nimg; img += gridDim.y) {                         // one grid row per image (rows wrap beyond the grid.y limit)
        const JsImage& im = imgs[img]; const JsProgFrame& fr = frames[img];
        __syncthreads();                                         // (the table of the image before is no longer read)
        if (threadIdx.x < 192) s_q[threadIdx.x >> 6][threadIdx.x & 63] = (int16_t)fr.qnat[(threadIdx.x >> 6) < im.ncomp ? (threadIdx.x >> 6) : 0][threadIdx.x & 63];
        __syncthreads();
        int16_t* cbase = coef + im.coef_off * 64; int16_t* dbase = dccum + im.coef_off;
        const uint32_t nb = im.blk_per_mcu, stride = gridDim.x * 32u, step = stride % nb;
        uint32_t b = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 8u + boff, r = b % nb;       // r = block-in-MCU index of b, carried along (no division in the loop)
        for (; b < im.total_blocks; b += stride) {
            const uint32_t comp = im.blk_comp[r] - 1u;
            uint4* p = reinterpret_cast<uint4*>(cbase + (size_t)b * 64 + sub * 8u);
            const uint4 v = *p, q = *reinterpret_cast<const uint4*>(&s_q[comp][sub * 8u]);
            const uint32_t vw[4] = { v.x, v.y, v.z, v.w }, qw[4] = { q.x, q.y, q.z, q.w }; uint32_t o[4];
            #pragma unroll
            for (int j = 0; j < 4; j++) {
                const int32_t lo = (int32_t)(int16_t)vw[j] * (int32_t)(int16_t)qw[j], hi = ((int32_t)vw[j] >> 16) * ((int32_t)qw[j] >> 16);
                o[j] = ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
            }
            if (sub == 0) { dbase[b] = (int16_t)o[0]; o[0] &= 0xFFFF0000u; }                // the dequantised DC goes to dccum, slot 0 is cleared
            *p = make_uint4(o[0], o[1], o[2], o[3]);
            r += step; if (r >= nb) r -= nb;
        }
    }
}

// =====================================================================================================================================
//  Lane-per-interval form of the scan kernels (pg_lanes == 64): one LANE per restart interval, the 64 lanes of a wave step through
//  64 intervals of ONE scan together.  The wave-per-interval kernel above spends a whole wave's issue slots on one to eight sequential
//  decoders (profiles/r03_prog_*: 3.7 G wave instructions per 64 images for one level of refinement scans, 1800 per block); here the
//  same decoders run 64 abreast in straight-line, predicated code:
//    * DC scans: a uniform loop over the units of the interval (every lane decodes "its" j-th unit in the same iteration);
//    * AC first scans: one symbol per lane and iteration, end-of-band runs skip whole blocks;
//    * AC refinement scans: a uniform loop over the blocks of the interval and, inside, over the band positions k = Ss..Se -- every lane
//      is at the SAME zig-zag position of its own block in every iteration (a position takes exactly one iteration whatever happens at
//      it: a correction bit for a non-zero history, a zero counted towards the run, the placement of the new value, or the tail of
//      an end-of-band run), so the position's natural index is wave-uniform; the block sits in LDS dword-interleaved across the lanes
//      (dword d of lane l at [d][l]: conflict-free), changes go through to HBM as 2-byte stores of the band positions only (other
//      scans of the level may own other bands of the same block).
//  The bit reader keeps 64 bits per lane and is topped up to >= 32 before every symbol (a code of <= 16 bits plus <= 15 value bits).
// =====================================================================================================================================
namespace {
// The file bytes come through a 64-byte ring per lane in LDS (dword-interleaved across the lanes), topped up in WAVE-UNIFORM code: a
// wave of sequential decoders has nothing else to run while a load is in flight, and a load issued inside a lane's own branch is waited
// for on the spot.  When some lane runs low, EVERY lane of the wave takes a 32-byte chunk if its ring has room for one -- one round of
// loads and one wait per few dozen steps.
struct LReader { const uint8_t* base; uint32_t pos, end, wr, limit; uint64_t acc; int n; uint32_t over; };
typedef uint32_t LRing[16][64];
__device__ __forceinline__ void lr_refill(LReader& r, bool live, LRing& ring, uint32_t lane)
{
    for (int c = 0; c < 2; c++) {
        const bool take = live && r.wr < r.limit && (r.wr - (r.pos & ~31u)) <= 32u;
        if (!__any(take)) break;
        if (take) {
            const uint4* p = reinterpret_cast<const uint4*>(r.base + r.wr);
            const uint4 a = p[0], b = p[1];
            const uint32_t d = (r.wr >> 2) & 15u;
            ring[d][lane] = a.x; ring[d + 1][lane] = a.y; ring[d + 2][lane] = a.z; ring[d + 3][lane] = a.w;
            ring[d + 4][lane] = b.x; ring[d + 5][lane] = b.y; ring[d + 6][lane] = b.z; ring[d + 7][lane] = b.w;
            r.wr += 32u;
        }
    }
}
__device__ __forceinline__ void lr_init(LReader& r, const uint8_t* file, uint32_t s, uint32_t e, uint32_t file_len, bool live, LRing& ring, uint32_t lane)
{
    r.base = file; r.pos = s; r.end = e; r.acc = 0; r.n = 0; r.over = 0; r.wr = s & ~31u; r.limit = (file_len + 31u) & ~31u;   // (file images are 16-byte aligned, padded, and the arena has slack)
    lr_refill(r, live, ring, lane);
}
__device__ __forceinline__ uint32_t lr_byte(const LReader& r, uint32_t i, const LRing& ring, uint32_t lane) { return (ring[(i >> 2) & 15u][lane] >> ((i & 3u) * 8u)) & 255u; }
// every live lane leaves with at least 32 bits; a pass appends one byte to every live lane that has room for it (a pass takes at most two
// file bytes from a lane's ring, which is topped up whenever some lane has fewer than eight left)
__device__ __forceinline__ void lr_fill(LReader& r, bool live, LRing& ring, uint32_t lane)
{
    while (__any(live && r.n < 32)) {          // (topping every lane up beyond 48 bits once some lane is short -- bursts of passes instead of one per step -- measured slower)
        if (__any(live && r.wr < r.limit && r.wr - r.pos < 8u)) lr_refill(r, live, ring, lane);
        if (live && r.n <= 56) {
            uint32_t b = 0;
            if (r.pos < r.end) { b = lr_byte(r, r.pos++, ring, lane); if (b == 0xFF && r.pos < r.end && lr_byte(r, r.pos, ring, lane) == 0x00) r.pos++; }    // FF00 -> FF (B.1.1.5)
            else r.over++;                                                                 // past the interval: zero bits, counted
            r.acc |= (uint64_t)b << (56 - r.n); r.n += 8;
        }
    }
}
__device__ __forceinline__ void lr_skip(LReader& r, int k) { r.acc <<= k; r.n -= k; }
__device__ __forceinline__ uint32_t lr_bits(LReader& r, int k) { if (!k) return 0u; const uint32_t v = (uint32_t)(r.acc >> (64 - k)); lr_skip(r, k); return v; }
__device__ __forceinline__ bool lr_overrun(const LReader& r) { return r.over * 8 > (uint32_t)(r.n > 0 ? r.n : 0); }
// canonical Huffman decode of the code at the top of the register (>= 16 bits present); consumes it for lanes in `take`
__device__ __forceinline__ int lr_huff(LReader& r, const JsProgTable& t, bool take)
{
    const uint32_t la = (uint32_t)(r.acc >> 48);
    const uint32_t e = t.look[la >> 8];
    int sym = -1, len = 16;
    if (e) { len = (int)(e >> 8); sym = (int)(e & 255u); }
    if (__any(take && !e)) {                                     // a code longer than eight bits in some lane
        if (!e) for (int l = 9; l <= 16; l++) {
            const int32_t code = (int32_t)(la >> (16 - l));
            if (code <= t.maxcode[l]) { len = l; sym = t.sym[(code + t.valoff[l]) & 255]; break; }
        }
    }
    if (take) lr_skip(r, len);
    return sym;
}
}  // namespace

#define PL_THREADS 256                                           // four waves per workgroup share the scan's tables (an LDS ring per wave): eight waves per SIMD fit
// zig-zag position -> natural index as compile-time constants (the mask builder below is unrolled over them)
__device__ constexpr uint8_t kZzNat[64] = {
     0, 1, 8,16, 9, 2, 3,10, 17,24,32,25,18,11, 4, 5, 12,19,26,33,40,48,41,34, 27,20,13, 6, 7,14,21,28,
    35,42,49,56,57,50,43,36, 29,22,15,23,30,37,44,51, 58,59,52,45,38,31,39,46, 53,60,61,54,47,55,62,63 };
// History of a block for a refinement scan, one bit per zig-zag position: coefficient non-zero / negative / bit `al` already set (a
// correction bit leaves such a coefficient alone: libjpeg's guard "(*thiscoef & p1) == 0", jdphuff.c decode_mcu_AC_refine -- a
// well-formed stream never sets the bit, a hostile one may, and the add would otherwise carry into the neighbouring coefficient).
__device__ __forceinline__ void history_masks(const int16_t* __restrict__ gblk, uint32_t al, uint64_t& nz, uint64_t& neg, uint64_t& set)
{
    uint32_t w[32];
    #pragma unroll
    for (int q = 0; q < 8; q++) { const uint4 x = reinterpret_cast<const uint4*>(gblk)[q]; w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w; }
    uint32_t nzl = 0, nzh = 0, ngl = 0, ngh = 0, stl = 0, sth = 0;
    #pragma unroll
    for (int k = 0; k < 64; k++) {
        const int nat = kZzNat[k];
        const uint32_t c = (nat & 1) ? w[nat >> 1] >> 16 : w[nat >> 1] & 0xFFFFu;
        const uint32_t one = min(c, 1u), sg = c >> 15, pb = (c >> al) & 1u;
        if (k < 32) { nzl |= one << k; ngl |= sg << k; stl |= pb << k; } else { nzh |= one << (k - 32); ngh |= sg << (k - 32); sth |= pb << (k - 32); }
    }
    nz = ((uint64_t)nzh << 32) | nzl; neg = ((uint64_t)ngh << 32) | ngl; set = ((uint64_t)sth << 32) | stl;
}

__global__ void __launch_bounds__(PL_THREADS) k_prog_scan_lanes(const JsImage* __restrict__ imgs, const JsProgFrame* __restrict__ frames, const JsProgScan* __restrict__ scans,
                                                        const uint32_t* __restrict__ lvl_scans, const uint32_t* __restrict__ lvl_wg, uint32_t nsc,
                                                        const JsProgTable* __restrict__ tabs, const JsProgSeg* __restrict__ segs, const uint8_t* __restrict__ raw,
                                                        int16_t* __restrict__ coef, uint32_t* __restrict__ status_all)
{
    uint32_t lo = 0, hi = nsc;                                   // lvl_wg is an exclusive prefix, nsc + 1 entries
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (lvl_wg[mid] <= blockIdx.x) lo = mid; else hi = mid; }
    const JsProgScan& sc = scans[lvl_scans[lo]];                 // wave-uniform, read through the scalar cache (a by-value copy of a struct that is
    const uint32_t wg_in_scan = blockIdx.x - lvl_wg[lo];          // indexed dynamically anywhere ends up in scratch memory, every field of it)
    const JsProgFrame& fr = frames[sc.img];
    uint32_t* status = status_all + sc.img * 4u;
    const uint32_t SS = sc.ss, SE = sc.se, AH = sc.ah, NBX = sc.nbx, NCOMP = sc.ncomp;      // the fields the loops live on, in registers
    __shared__ JsProgTable s_tab[4];
    __shared__ uint8_t s_zz[64];
    __shared__ LRing s_rings[PL_THREADS / 64];                   // the lanes' file bytes, one ring set per wave
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    LRing& s_ring = s_rings[wave];
    if (threadIdx.x < 64) s_zz[threadIdx.x] = c_zz_nat[threadIdx.x];
    for (uint32_t t = 0; t < sc.ntabs; t++) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(tabs + sc.tab[t]); uint32_t* dst = reinterpret_cast<uint32_t*>(&s_tab[t]);
        for (uint32_t i = threadIdx.x; i < sizeof(JsProgTable) / 4; i += PL_THREADS) dst[i] = src[i];
    }
    __syncthreads();
    // (from here on the waves of the workgroup go their own ways: no further barrier)
    const JsImage& im = imgs[sc.img];
    const uint32_t iv = wg_in_scan * PL_THREADS + threadIdx.x;
    const bool have = iv < sc.nseg;
    const JsProgSeg sg = segs[sc.seg_first + (have ? iv : 0u)];
    LReader r; lr_init(r, raw + im.file_off, sg.start, have ? sg.end : sg.start, im.file_len, have, s_ring, lane);
    int16_t* cbase = coef + im.coef_off * 64;
    const uint32_t units = sc.ncomp > 1 ? im.mcu_xmax * im.mcu_ymax : sc.nbx * sc.nby;     // MCUs of the scan (A.2.2 / A.2.3)
    const uint32_t ri = sc.rst_interval ? sc.rst_interval : units;
    const uint32_t u0 = min(units, iv * ri), u1 = have ? min(units, u0 + ri) : u0;
    const uint32_t nu = u1 - u0;
    uint32_t bad = 0;
    const int al = (int)sc.al;

    if (SS == 0) {
        // ---- DC scans (G.1.2.1): the j-th unit of every interval in the same iteration
        int pred[3] = { 0, 0, 0 };
        for (uint32_t j = 0; __any(j < nu && !bad); j++) {
            const bool live0 = j < nu;
            const uint32_t u = u0 + j;
            for (uint32_t ci = 0; ci < NCOMP; ci++) {
                const uint32_t comp = sc.comp[ci];
                const uint32_t hs = NCOMP > 1 ? fr.hs[comp] : 1u, vs = NCOMP > 1 ? fr.vs[comp] : 1u;
                for (uint32_t v = 0; v < vs; v++) for (uint32_t h = 0; h < hs; h++) {
                    const bool live = live0 && !bad;
                    const uint32_t bx = NCOMP > 1 ? (u % im.mcu_xmax) * hs + h : u % NBX;
                    const uint32_t by = NCOMP > 1 ? (u / im.mcu_xmax) * vs + v : u / NBX;
                    int16_t* blk = cbase + block_row(im, fr, comp, live ? bx : 0u, live ? by : 0u) * 64;
                    lr_fill(r, live, s_ring, lane);
                    if (AH == 0) {
                        const int s = lr_huff(r, s_tab[sc.dc_slot[ci]], live);
                        if (live) {
                            if (s < 0 || s > 15) bad = 1;
                            else { const int diff = s ? extend(lr_bits(r, s), s) : 0; pred[ci] += diff; blk[0] = (int16_t)(pred[ci] * (1 << al)); }
                        }
                    } else if (live) { if (lr_bits(r, 1)) blk[0] = (int16_t)(blk[0] | (1 << al)); }
                }
            }
        }
    } else if (AH == 0) {
        // ---- AC first scan (G.1.2.2): one symbol per lane and iteration; an end-of-band run skips whole blocks
        const uint32_t comp = sc.comp[0]; const JsProgTable& T = s_tab[sc.ac_slot[0]];
        uint32_t j = 0, k = SS, eobrun = 0;
        int16_t* blk = cbase; bool newblk = true;               // the block of unit j: its row is worked out when j moves, not per symbol
        while (__any(j < nu && !bad)) {
            if (j < nu && eobrun && k == SS) { const uint32_t sk = min(eobrun, nu - j); j += sk; eobrun -= sk; newblk = true; }
            const bool live = j < nu && !bad;
            if (__any(live && newblk)) {
                if (live && newblk) { const uint32_t u = u0 + j; blk = cbase + block_row(im, fr, comp, u % NBX, u / NBX) * 64; newblk = false; }
            }
            lr_fill(r, live, s_ring, lane);
            const int rs = lr_huff(r, T, live);
            if (live) {
                if (rs < 0) bad = 1;
                else {
                    const uint32_t run = (uint32_t)rs >> 4, s = (uint32_t)rs & 15u;
                    if (s) {
                        k += run;
                        if (k > SE) bad = 1;
                        else { blk[s_zz[k]] = (int16_t)(extend(lr_bits(r, (int)s), (int)s) * (1 << al)); k++; }
                    } else if (run == 15) k += 16;                                          // ZRL
                    else { eobrun = (1u << run) + lr_bits(r, (int)run) - 1u; k = SE + 1u; }    // EOBn: this block ends here, eobrun more follow
                    if (k > SE) { j++; k = SS; newblk = true; }
                }
            }
        }
    } else {
        // ---- AC refinement scan (G.1.2.3), the decoding procedure of libjpeg's decode_mcu_AC_refine position by position.
        // What the procedure needs of a block is its history -- which coefficients are non-zero, and their signs: two 64-bit masks per
        // lane, built when the block is entered.  A coefficient with history is a multiple of 2 << Al (every earlier scan of its band had
        // a larger point transform), so a correction bit adds +-(1 << Al) to it, and a new coefficient adds its value to a zero: both
        // leave as ONE 32-bit atomic add on the dword that holds the coefficient (no value comes back: nothing to wait for).  The low
        // half takes the addend sign-extended when the coefficient is non-zero (it grows away from zero: no carry, no borrow reaches
        // the neighbour) and as its 16-bit pattern when it is zero; other scans of the level may own the other half of the dword.
        const uint32_t comp = sc.comp[0]; const JsProgTable& T = s_tab[sc.ac_slot[0]];
        const int p1 = 1 << al, m1 = -(1 << al);
        uint32_t eobrun = 0;
        for (uint32_t j = 0; __any(j < nu && !bad); j++) {
            const bool inb = j < nu;
            const uint32_t u = u0 + (inb ? j : 0u);
            int16_t* gblk = cbase + block_row(im, fr, comp, u % NBX, u / NBX) * 64;
            uint64_t nz = 0, neg = 0, p1set = 0;
            if (__any(inb)) { if (inb) history_masks(gblk, (uint32_t)al, nz, neg, p1set); }
            uint32_t* gw = reinterpret_cast<uint32_t*>(gblk);
            bool adv = false, has_new = false; int newv = 0; uint32_t run = 0;
            for (uint32_t k = SS; k <= SE; k++) {                // k is wave-uniform
                const bool live = inb && !bad;
                const uint32_t nat = s_zz[k];
                lr_fill(r, live, s_ring, lane);
                const bool need = live && !eobrun && !adv;
                if (__any(need)) {
                    const int rs = lr_huff(r, T, need);
                    if (need) {
                        if (rs < 0) bad = 1;
                        else {
                            run = (uint32_t)rs >> 4; const uint32_t s = (uint32_t)rs & 15u;
                            if (s) { if (s != 1) bad = 1; newv = lr_bits(r, 1) ? p1 : m1; has_new = true; adv = true; }
                            else if (run == 15) { has_new = false; adv = true; }
                            else eobrun = (1u << run) + lr_bits(r, (int)run);                // EOBn (this block included): the rest of the band takes correction bits only
                        }
                    }
                }
                if (live && !bad) {
                    const bool hist = (nz >> k) & 1ull;
                    int delta = 0; bool was_zero = false;
                    if (hist) {                                  // a coefficient with history: one correction bit
                        if (lr_bits(r, 1) && !((p1set >> k) & 1ull)) delta = ((neg >> k) & 1ull) ? m1 : p1;
                    } else if (!eobrun && adv) {                 // a zero: counts towards the run, or takes the new value
                        if (run == 0) { if (has_new) { delta = newv; was_zero = true; } adv = false; }
                        else run--;
                    }
                    if (delta) {
                        const uint32_t add = (nat & 1u) ? (uint32_t)delta << 16 : (was_zero ? (uint32_t)delta & 0xFFFFu : (uint32_t)delta);
                        atomicAdd(gw + (nat >> 1), add);
                    }
                }
            }
            if (inb && eobrun) eobrun--;
        }
    }
    if (bad) atomicOr(&status[0], 1u);                              // a code that matches nothing / illegal symbol
    if (have && lr_overrun(r)) atomicOr(&status[0], 2u);            // the interval ended before its blocks did
}

uint32_t js_prog_wgs_of(const JsProgScan& sc, uint32_t pg_lanes) { const uint32_t per = pg_lanes >= 64u ? (uint32_t)PL_THREADS : ((sc.ss != 0 && sc.ah != 0) ? 1u : pg_lanes); return (sc.nseg + per - 1) / per; }
void js_launch_prog_level(hipStream_t st, const JsImage* imgs, const JsProgFrame* frames, const JsProgScan* scans, const uint32_t* lvl_scans, const uint32_t* lvl_wg,
                          uint32_t nsc, uint32_t total_wgs, uint32_t pg_lanes, const JsProgTable* tabs, const JsProgSeg* segs, const uint8_t* raw, int16_t* coef, uint32_t* status)
{
    if (!nsc || !total_wgs) return;
    if (pg_lanes >= 64u) { hipLaunchKernelGGL(k_prog_scan_lanes, dim3(total_wgs), dim3(PL_THREADS), 0, st, imgs, frames, scans, lvl_scans, lvl_wg, nsc, tabs, segs, raw, coef, status); return; }
    hipLaunchKernelGGL(k_prog_scan, dim3(total_wgs), dim3(64), 0, st, imgs, frames, scans, lvl_scans, lvl_wg, nsc, pg_lanes, tabs, segs, raw, coef, status);
}
void js_launch_prog_finalize(hipStream_t st, const JsImage* imgs, const JsProgFrame* frames, uint32_t nimg, const uint32_t* blk_base, uint32_t total_blocks,
                             int16_t* coef, int16_t* dccum)
{
    if (!nimg) return;
    const uint32_t per_img = (total_blocks / nimg + 3) / 4;           // workgroups of four blocks; each strides over its image
    const uint32_t gx = nimg >= 64 ? 64u : (per_img < 2048 ? (per_img ? per_img : 1u) : 2048u);
    hipLaunchKernelGGL(k_prog_finalize, dim3(gx, nimg < 65535u ? nimg : 65535u), dim3(256), 0, st, imgs, frames, nimg, blk_base, total_blocks, coef, dccum);
}
