// Host-only program: the host arithmetic jsnoop_batch_export_jpeg_prog adds (jpegsnoop_amd/csrc/jsnoop_export_prog_check.h) on hand-made image descriptors -- the
// progressive spec and every refusal, every rule of a script one by one, the default scripts, the scan records and the map from a unit to its arena block against a
// brute-force loop for six layouts, the two run operators (associativity on random summaries, and both scans against a sequential loop that flushes runs the way
// libjpeg does, the 32767 split included), plans of 1, 4, 190 and 231 scans, the layout and the worst-case size of a file.  With the argument "headers" it prints
// the header pieces of one plan in hex for tests/test_export_prog_abi.py to compare with the model's.  tests/test_export_prog_abi.py builds it with the address and
// undefined-behaviour sanitizers and runs it.  Prints "ok" and returns 0, or the line that failed.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#ifndef __HIPCC__
#define __host__
#define __device__
#endif
#include "../../jpegsnoop_amd/csrc/jsnoop_export_prog_check.h"

static std::string g_err;
void js_set_error(const char* fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)

static JsImage image(uint32_t ncomp, const uint32_t (*hv)[2], uint32_t dim_x, uint32_t dim_y, uint32_t rst_interval = 0)
{
    JsImage im; memset(&im, 0, sizeof im);
    im.ncomp = ncomp; im.dim_x = dim_x; im.dim_y = dim_y; im.precision = 8; im.rst_interval = rst_interval; im.rst_en = rst_interval != 0;
    uint32_t hmax = 0, vmax = 0, nb = 0;
    for (uint32_t c = 1; c <= ncomp; c++) {
        im.samp_h[c] = hv[c - 1][0]; im.samp_v[c] = hv[c - 1][1];
        if (im.samp_h[c] > hmax) hmax = im.samp_h[c];
        if (im.samp_v[c] > vmax) vmax = im.samp_v[c];
        for (uint32_t v = 0; v < im.samp_v[c]; v++) for (uint32_t h = 0; h < im.samp_h[c]; h++) { im.blk_comp[nb] = (uint8_t)c; im.blk_ch[nb] = (uint8_t)h; im.blk_cv[nb] = (uint8_t)v; nb++; }
    }
    im.blk_per_mcu = nb; im.mcu_w = hmax * 8; im.mcu_h = vmax * 8;
    im.mcu_xmax = (dim_x + im.mcu_w - 1) / im.mcu_w; im.mcu_ymax = (dim_y + im.mcu_h - 1) / im.mcu_h;
    im.total_blocks = im.mcu_xmax * im.mcu_ymax * nb;
    return im;
}
static int qfn(void*, int, int comp, uint16_t* out64) { for (int k = 0; k < 64; k++) out64[k] = (uint16_t)(3 + 2 * comp); return 0; }

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return (uint32_t)(g_seed >> 16); }
static JsnoopExportScan scan(uint8_t comps, uint8_t ss, uint8_t se, uint8_t ah, uint8_t al) { JsnoopExportScan s; memset(&s, 0, sizeof s); s.comps = comps; s.ss = ss; s.se = se; s.ah = ah; s.al = al; return s; }
typedef std::vector<JsnoopExportScan> Script;
static int valid(const Script& s, uint32_t* nc = nullptr) { uint32_t n = 0; const int r = js_export_prog_validate(s.data(), (uint32_t)s.size(), &n); if (nc) *nc = n; return r; }
static bool says(const char* word) { return g_err.find(word) != std::string::npos; }

// the carried run lengths of a sequence of classes by a sequential loop with libjpeg's flushing (the run is flushed in front of a block with symbols, at 32767, at an
// interval end, at the end): the length goes to the unit that STARTED the flushed piece
static std::vector<uint32_t> runs_by_loop(const std::vector<uint8_t>& cls, uint32_t ri)
{
    std::vector<uint32_t> out(cls.size(), 0); uint32_t run = 0; size_t first = 0;
    auto flush = [&]() { if (run) out[first] = run; run = 0; };
    for (size_t u = 0; u < cls.size(); u++) {
        if (ri && u && u % ri == 0) flush();
        if (cls[u] != JS_PROG_EMPTY) flush();
        if (cls[u] != JS_PROG_FULL) { if (!run) first = u; run++; if (run == JS_PROG_EOB_MAX) flush(); }
    }
    flush();
    return out;
}
// ... and by the two scans, folded in pieces of `piece` units the way the kernel carries summaries from step to step
static std::vector<uint32_t> runs_by_scans(const std::vector<uint8_t>& cls, uint32_t ri, size_t piece)
{
    const size_t n = cls.size(); std::vector<uint32_t> out(n, 0);
    JsExportScanRec r; memset(&r, 0, sizeof r); r.nunits = (uint32_t)n; r.ri = ri;
    JsRunFwd cf = js_run_fwd_identity();
    for (size_t i0 = 0; i0 < n; i0 += piece) {
        JsRunFwd in = js_run_fwd_identity();
        for (size_t u = i0; u < n && u < i0 + piece; u++) { in = js_run_fwd_combine(in, js_run_fwd_leaf(cls[u], js_prog_starts(r, (uint32_t)u))); out[u] = js_run_carries(cls[u], js_run_fwd_combine(cf, in)) ? 1u : 0u; }
        cf = js_run_fwd_combine(cf, in);
    }
    JsRunBwd cb = js_run_bwd_identity();
    for (size_t hi = n; hi > 0; ) {
        const size_t lo = (hi - 1) / piece * piece;
        JsRunBwd in = js_run_bwd_identity();
        for (size_t u = hi; u-- > lo; ) {
            const bool ends = js_prog_ends(r, (uint32_t)u);
            if (out[u]) out[u] = js_run_length(ends, js_run_bwd_combine(in, cb));
            in = js_run_bwd_combine(js_run_bwd_leaf(cls[u], ends), in);
        }
        cb = js_run_bwd_combine(in, cb); hi = lo;
    }
    return out;
}

int main(int argc, char** argv)
{
    static const uint32_t k444[3][2] = { { 1, 1 }, { 1, 1 }, { 1, 1 } }, k422[3][2] = { { 2, 1 }, { 1, 1 }, { 1, 1 } }, k420[3][2] = { { 2, 2 }, { 1, 1 }, { 1, 1 } },
                          k440[3][2] = { { 1, 2 }, { 1, 1 }, { 1, 1 } }, k411[3][2] = { { 4, 1 }, { 1, 1 }, { 1, 1 } }, kGrey[1][2] = { { 1, 1 } };
    std::vector<JsImage> imgs = { image(3, k420, 333, 217, 5), image(1, kGrey, 72, 40), image(3, k444, 17, 9), image(3, k422, 72, 40), image(3, k440, 17, 9), image(3, k411, 72, 40),
                                  image(1, kGrey, 8 * 300, 16), image(3, k420, 1, 1) };
    CHECK(sizeof(JsnoopExportScan) == 8 && sizeof(JsnoopExportProgressive) == 24 && sizeof(JsRunFwd) == 12 && sizeof(JsRunBwd) == 8 && sizeof(JsExportRec) == 552 && sizeof(JsExportScanRec) % 8 == 0);
    Script d3(6), d1(4);
    CHECK(js_export_prog_default(3, d3.data()) == 6 && js_export_prog_default(1, d1.data()) == 4);

    if (argc > 1 && !strcmp(argv[1], "headers")) {                   // the pieces of image 0 under the default script with ROWS 1, in hex: the pre piece, then a line per scan
        JsnoopExportSpec spec; js_export_spec_defaults(&spec);
        JsnoopExportRestart rs; js_export_restart_defaults(&rs); rs.mode = JSNOOP_RESTART_ROWS; rs.interval = 1;
        std::vector<uint8_t> flags(1), uns(1); size_t nrec = 0; const int list[1] = { 0 };
        CHECK(js_export_prog_count(imgs.data(), imgs.size(), list, 1, rs, d3.data(), 6, d1.data(), 4, flags.data(), &nrec) == 0 && nrec == 6 && !flags[0]);
        const JsExportProgBlock blk = js_export_prog_block(1, nrec);
        std::vector<uint8_t> mem(blk.b.total);
        JsExportRec* recs = reinterpret_cast<JsExportRec*>(mem.data() + blk.b.recs); uint32_t* rec_base = reinterpret_cast<uint32_t*>(mem.data() + blk.b.unit_base);
        JsExportScanRec* srecs = reinterpret_cast<JsExportScanRec*>(mem.data() + blk.srecs); uint32_t* tile_base = reinterpret_cast<uint32_t*>(mem.data() + blk.tile_base);
        uint64_t blocks = 0, units = 0, ivs = 0;
        CHECK(js_export_plan(imgs.data(), imgs.size(), spec, list, 1, qfn, nullptr, recs, rec_base, mem.data() + blk.b.hdrs, uns.data(), &blocks) == 0);
        CHECK(js_export_prog_plan(imgs.data(), list, 1, rs, d3.data(), 6, d1.data(), 4, recs, uns.data(), mem.data() + blk.b.hdrs, (uint32_t)(blk.posts - blk.b.hdrs), srecs, rec_base, tile_base, &units, &ivs) == 0);
        const uint8_t* h = mem.data() + blk.b.hdrs;
        for (uint32_t i = 0; i < srecs[0].pre_len; i++) printf("%02x", h[srecs[0].pre_off + i]);
        printf("\n");
        for (size_t s = 0; s < nrec; s++) { for (uint32_t i = 0; i < srecs[s].post_len; i++) printf("%02x", h[srecs[s].post_off + i]); printf(" %u %u %u\n", srecs[s].nunits, srecs[s].ri, srecs[s].ni); }
        return 0;
    }

    // ---- the spec: defaults, NULL, a shorter struct, and every refusal
    JsnoopExportProgressive def; memset(&def, 0xEE, sizeof def); js_export_progressive_defaults(&def);
    CHECK(def.struct_size == 24 && def.mode == JSNOOP_PROGRESSIVE_OFF && def.nscans == 0 && def.reserved == 0 && def.scans == nullptr);
    JsnoopExportProgressive in = def, p;
    CHECK(js_export_import_progressive(nullptr, &p) == 0 && p.mode == 0);
    in.mode = JSNOOP_PROGRESSIVE_DEFAULT; CHECK(js_export_import_progressive(&in, &p) == 0 && p.mode == 1);
    in.struct_size = 8; CHECK(js_export_import_progressive(&in, &p) == 0 && p.mode == 1 && p.struct_size == 24);
    in.struct_size = 32; CHECK(js_export_import_progressive(&in, &p) == -1 && says("struct_size"));
    in.struct_size = 0; CHECK(js_export_import_progressive(&in, &p) == -1);
    in = def; in.mode = 3; CHECK(js_export_import_progressive(&in, &p) == -1 && says("mode = 3"));
    in.mode = -1; CHECK(js_export_import_progressive(&in, &p) == -1 && says("mode = -1"));
    in = def; in.reserved = 1; CHECK(js_export_import_progressive(&in, &p) == -1 && says("reserved"));
    for (int mode : { JSNOOP_PROGRESSIVE_OFF, JSNOOP_PROGRESSIVE_DEFAULT }) {
        in = def; in.mode = mode; in.nscans = 6; CHECK(js_export_import_progressive(&in, &p) == -1 && says("no script"));
        in.nscans = 0; in.scans = d3.data(); CHECK(js_export_import_progressive(&in, &p) == -1 && says("no script"));
    }
    in = def; in.mode = JSNOOP_PROGRESSIVE_SCRIPT; in.scans = d3.data(); in.nscans = 6; CHECK(js_export_import_progressive(&in, &p) == 0 && p.nscans == 6 && p.scans == d3.data());
    in.scans = nullptr; CHECK(js_export_import_progressive(&in, &p) == -1 && says("NULL"));
    in.scans = d3.data(); in.nscans = 0; CHECK(js_export_import_progressive(&in, &p) == -1);
    in.nscans = JSNOOP_EXPORT_MAX_SCANS + 1; CHECK(js_export_import_progressive(&in, &p) == -1);

    // ---- the rules of a script, one by one
    uint32_t nc = 0;
    CHECK(valid(d3, &nc) == 0 && nc == 3 && valid(d1, &nc) == 0 && nc == 1);
    CHECK(d3[0].comps == 7 && d3[0].al == 1 && d3[1].comps == 1 && d3[1].ss == 1 && d3[1].se == 5 && d3[2].comps == 2 && d3[3].comps == 4 && d3[4].ss == 6 && d3[4].se == 63 && d3[5].ah == 1 && d3[5].al == 0);
    const Script ok1 = { scan(1, 0, 0, 0, 0), scan(1, 1, 63, 0, 0) };
    CHECK(valid(ok1) == 0);
    Script s;
    s = ok1; s[1].reserved[2] = 1; CHECK(valid(s) == -1 && says("reserved"));
    s = ok1; s[1].comps = 0; CHECK(valid(s) == -1 && says("comps"));
    s = ok1; s[1].comps = 9; CHECK(valid(s) == -1 && says("comps"));
    s = ok1; s[1].ss = 5; s[1].se = 4; CHECK(valid(s) == -1 && says("Ss <= Se"));
    s = ok1; s[1].se = 64; CHECK(valid(s) == -1 && says("Se 64"));
    s = ok1; s[0].al = 14; CHECK(valid(s) == -1 && says("Al 14"));
    s = ok1; s[0].se = 5; CHECK(valid(s) == -1 && says("DC scan"));
    s = { scan(7, 0, 0, 0, 0), scan(3, 1, 63, 0, 0) }; CHECK(valid(s) == -1 && says("exactly one component"));
    s = ok1; s[1].al = 1; CHECK(valid(s) == -1 && says("successive approximation"));
    s = { scan(1, 0, 0, 0, 0), scan(1, 1, 63, 0, 0), scan(1, 1, 63, 1, 0) }; CHECK(valid(s) == -1 && says("successive approximation"));
    s = { scan(1, 0, 0, 0, 2), scan(1, 0, 0, 2, 0), scan(1, 1, 63, 0, 0) }; CHECK(valid(s) == -1 && says("Al = Ah - 1"));
    s = { scan(3, 0, 0, 0, 0), scan(1, 1, 63, 0, 0), scan(2, 1, 63, 0, 0) }; CHECK(valid(s) == -1 && says("names components"));
    s = { scan(2, 0, 0, 0, 0), scan(2, 1, 63, 0, 0) }; CHECK(valid(s) == -1 && says("names components"));
    s = { scan(1, 0, 0, 1, 0), scan(1, 1, 63, 0, 0) }; CHECK(valid(s) == -1 && says("DC has Ah"));
    s = { scan(1, 0, 0, 0, 2), scan(1, 0, 0, 1, 0), scan(1, 1, 63, 0, 0) }; CHECK(valid(s) == -1 && says("DC has Ah"));
    s = { scan(1, 0, 0, 0, 0), scan(1, 0, 0, 0, 0), scan(1, 1, 63, 0, 0) }; CHECK(valid(s) == -1 && says("DC has Ah"));
    s = { scan(1, 0, 0, 0, 1), scan(1, 1, 63, 0, 0) }; CHECK(valid(s) == -1 && says("ends at Al 1"));
    s = { scan(1, 1, 63, 0, 0), scan(1, 0, 0, 0, 0) }; CHECK(valid(s) == -1 && says("in front of its first DC"));
    s = { scan(1, 0, 0, 0, 0), scan(1, 1, 10, 0, 0), scan(1, 10, 63, 0, 0) }; CHECK(valid(s) == -1 && says("coded twice"));
    s = { scan(1, 0, 0, 0, 0), scan(1, 1, 10, 0, 0), scan(1, 12, 63, 0, 0) }; CHECK(valid(s) == -1 && says("not all coded"));
    s = { scan(7, 0, 0, 0, 0), scan(1, 1, 63, 0, 0), scan(2, 1, 63, 0, 0) }; CHECK(valid(s) == -1 && says("component 2"));
    CHECK(js_export_prog_validate(nullptr, 1, &nc) == -1 && js_export_prog_validate(ok1.data(), 0, &nc) == -1 && js_export_prog_validate(ok1.data(), 257, &nc) == -1);
    Script big;                                                         // the largest legal script: 3 x 14 DC scans, 3 x 63 AC scans
    for (uint8_t c = 0; c < 3; c++) big.push_back(scan((uint8_t)(1u << c), 0, 0, 0, 13));
    for (uint8_t a = 13; a > 0; a--) for (uint8_t c = 0; c < 3; c++) big.push_back(scan((uint8_t)(1u << c), 0, 0, a, (uint8_t)(a - 1)));
    for (uint8_t k = 1; k < 64; k++) for (uint8_t c = 0; c < 3; c++) big.push_back(scan((uint8_t)(1u << c), k, k, 0, 0));
    CHECK(big.size() == 231 && valid(big, &nc) == 0 && nc == 3);
    Script each = { scan(7, 0, 0, 0, 0) };
    for (uint8_t k = 1; k < 64; k++) for (uint8_t c = 0; c < 3; c++) each.push_back(scan((uint8_t)(1u << c), k, k, 0, 0));
    CHECK(each.size() == 190 && valid(each) == 0);

    // ---- scan records and the map against a brute-force walk of the arena, six layouts
    JsnoopExportRestart none; js_export_restart_defaults(&none);
    for (size_t ii = 0; ii < 6; ii++) {
        const JsImage& im = imgs[ii];
        uint32_t hmax = 1, vmax = 1;
        for (uint32_t c = 1; c <= im.ncomp; c++) { if (im.samp_h[c] > hmax) hmax = im.samp_h[c]; if (im.samp_v[c] > vmax) vmax = im.samp_v[c]; }
        for (uint8_t comps = 1; comps < (im.ncomp == 1 ? 2 : 8); comps++) {
            JsExportScanRec r; const JsnoopExportScan sc = scan(comps, 0, 0, 0, 0);
            CHECK(js_export_prog_scan_rec(im, sc, 0, none, &r) == 0 && r.ri == 0 && r.ni == 1);
            std::vector<uint32_t> want; std::vector<uint32_t> prev;      // arena blocks in the scan's order; the unit of the same component before each (0xFFFFFFFF: none)
            const bool one = (comps & (comps - 1)) == 0;
            if (one && im.ncomp == 3) {
                uint32_t c = 0; while (!(comps >> c & 1)) c++;
                const uint32_t H = im.samp_h[c + 1], V = im.samp_v[c + 1], w = ((im.dim_x * H + hmax - 1) / hmax + 7) / 8, h = ((im.dim_y * V + vmax - 1) / vmax + 7) / 8;
                for (uint32_t by = 0; by < h; by++) for (uint32_t bx = 0; bx < w; bx++) {
                    const uint32_t m = (by / V) * im.mcu_xmax + bx / H; uint32_t found = 0xFFFFFFFFu;
                    for (uint32_t j = 0; j < im.blk_per_mcu; j++) if (im.blk_comp[j] == c + 1 && im.blk_ch[j] == bx % H && im.blk_cv[j] == by % V) found = m * im.blk_per_mcu + j;
                    prev.push_back(want.empty() ? 0xFFFFFFFFu : (uint32_t)want.size() - 1); want.push_back(found);
                }
                CHECK(r.single == 1 && r.w == w && r.ntab == 1);
            } else {
                uint32_t last[3] = { 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu };
                for (uint32_t j = 0; j < im.total_blocks; j++) { const uint32_t c = im.blk_comp[j % im.blk_per_mcu] - 1u; if (comps >> c & 1) { prev.push_back(last[c]); last[c] = (uint32_t)want.size(); want.push_back(j); } }
                CHECK(r.single == 0 && r.ntab == (uint32_t)__builtin_popcount(comps));
            }
            CHECK(r.nunits == want.size());
            for (uint32_t u = 0; u < r.nunits; u++) {
                CHECK(js_prog_block(r, u) == want[u] && want[u] < im.total_blocks);
                const uint32_t back = r.back[r.single ? 0 : u % r.spm];
                CHECK(prev[u] == 0xFFFFFFFFu ? u < back : u - back == prev[u]);
            }
        }
    }
    // Ri of the four modes in the scan's own units; above 65535 the entry is refused
    {
        JsExportScanRec r; JsnoopExportRestart rs = none;
        rs.mode = JSNOOP_RESTART_ROWS; rs.interval = 1;
        CHECK(js_export_prog_scan_rec(imgs[0], d3[0], 0, rs, &r) == 21 && r.ri == 21 * 6 && r.ni == 14 && r.nunits == 21 * 14 * 6);
        CHECK(js_export_prog_scan_rec(imgs[0], d3[1], 1, rs, &r) == 42 && r.ri == 42 && r.ni == 28 && r.nunits == 42 * 28);           // luma: 333 -> 42 blocks, 217 -> 28
        CHECK(js_export_prog_scan_rec(imgs[0], d3[2], 2, rs, &r) == 21 && r.ri == 21 && r.ni == 14);
        rs.mode = JSNOOP_RESTART_MCUS; rs.interval = 5; CHECK(js_export_prog_scan_rec(imgs[0], d3[1], 1, rs, &r) == 5 && r.ri == 5 && r.ni == (42 * 28 + 4) / 5);
        rs.mode = JSNOOP_RESTART_SOURCE; rs.interval = 0; CHECK(js_export_prog_scan_rec(imgs[0], d3[0], 0, rs, &r) == 5 && r.ri == 30 && js_export_prog_scan_rec(imgs[1], d1[0], 0, rs, &r) == 0 && r.ni == 1);
        rs.mode = JSNOOP_RESTART_ROWS; rs.interval = 219; CHECK(js_export_prog_scan_rec(imgs[6], d1[1], 1, rs, &r) == 65700);
        // above 65535 in ONE kind of scan: 2048 x 16 in 4:2:0 has 128 MCUs and 256 luma blocks a row
        const JsImage wide = image(3, k420, 2048, 16);
        rs.interval = 256; CHECK(js_export_prog_scan_rec(wide, d3[0], 0, rs, &r) == 32768 && js_export_prog_scan_rec(wide, d3[2], 2, rs, &r) == 32768 && js_export_prog_scan_rec(wide, d3[1], 1, rs, &r) == 65536);
        std::vector<JsImage> two = { wide, imgs[0] }; std::vector<uint8_t> fl(2); size_t nr = 0;
        CHECK(js_export_prog_count(two.data(), 2, nullptr, 2, rs, d3.data(), 6, d1.data(), 4, fl.data(), &nr) == 0 && fl[0] == 1 && fl[1] == 0 && nr == 6);
        rs.interval = 255; CHECK(js_export_prog_scan_rec(wide, d3[1], 1, rs, &r) == 65280 && r.ri == 65280 && r.ni == 1 && r.nunits == 512);
        CHECK(js_export_prog_count(two.data(), 2, nullptr, 2, rs, d3.data(), 6, d1.data(), 4, fl.data(), &nr) == 0 && fl[0] == 0 && nr == 12);
    }

    // ---- the run operators: associativity, and both scans against the sequential loop
    for (int it = 0; it < 20000; it++) {
        JsRunFwd f[3]; JsRunBwd b[3];
        for (int k = 0; k < 3; k++) { f[k].cnt = rnd() % 70000; f[k].cut = rnd() & 1; f[k].tail = f[k].cut ? rnd() & 1 : 0; b[k].lead = rnd() % 70000; b[k].open = rnd() & 1; }
        const JsRunFwd fl = js_run_fwd_combine(js_run_fwd_combine(f[0], f[1]), f[2]), fr = js_run_fwd_combine(f[0], js_run_fwd_combine(f[1], f[2]));
        const JsRunBwd bl = js_run_bwd_combine(js_run_bwd_combine(b[0], b[1]), b[2]), br = js_run_bwd_combine(b[0], js_run_bwd_combine(b[1], b[2]));
        CHECK(fl.cnt == fr.cnt && fl.cut == fr.cut && fl.tail == fr.tail && bl.lead == br.lead && bl.open == br.open);
        const JsRunFwd fi = js_run_fwd_combine(js_run_fwd_identity(), f[0]), fj = js_run_fwd_combine(f[0], js_run_fwd_identity());
        CHECK(fi.cnt == f[0].cnt && fi.cut == f[0].cut && fj.cnt == f[0].cnt && fj.cut == f[0].cut && fj.tail == f[0].tail);
        const JsRunBwd bi = js_run_bwd_combine(js_run_bwd_identity(), b[0]), bj = js_run_bwd_combine(b[0], js_run_bwd_identity());
        CHECK(bi.lead == b[0].lead && bi.open == b[0].open && bj.lead == b[0].lead && bj.open == b[0].open);
    }
    for (int it = 0; it < 300; it++) {
        const size_t n = 1 + rnd() % 3000; const uint32_t ri = (it & 1) ? 1 + rnd() % 700 : 0; const uint32_t dens = 1 + rnd() % 40;
        std::vector<uint8_t> cls(n);
        for (auto& c : cls) { const uint32_t x = rnd() % 100; c = x < dens ? (uint8_t)JS_PROG_TAIL : x < 2 * dens ? (uint8_t)JS_PROG_FULL : (uint8_t)JS_PROG_EMPTY; }
        const std::vector<uint32_t> want = runs_by_loop(cls, ri);
        CHECK(want == runs_by_scans(cls, ri, 256) && want == runs_by_scans(cls, ri, 1 + rnd() % 500));
    }
    for (uint32_t empty : { 32765u, 32766u, 32767u, 32768u, 65533u, 65534u, 65535u, 70000u }) for (uint8_t first : { (uint8_t)JS_PROG_TAIL, (uint8_t)JS_PROG_FULL }) {
        std::vector<uint8_t> cls(empty + 5, JS_PROG_EMPTY); cls[0] = first; cls[empty + 1] = JS_PROG_FULL; cls[empty + 2] = JS_PROG_FULL;
        const std::vector<uint32_t> want = runs_by_loop(cls, 0);
        const uint32_t len = empty + (first == JS_PROG_TAIL ? 1u : 0u);
        CHECK(want[first == JS_PROG_TAIL ? 0 : 1] == (len < 32767u ? len : 32767u) && want == runs_by_scans(cls, 0, 256));
        CHECK(runs_by_loop(cls, 1000) == runs_by_scans(cls, 1000, 256));
    }

    // ---- plans of 1 (refused: no script of one scan is complete), 4, 190 and 231 scans; what an entry is refused for; the layout and the size of a file
    JsnoopExportSpec spec; js_export_spec_defaults(&spec);
    struct Case { const Script* s3; const Script* s1; size_t per3, per1; } cases[] = { { &d3, &d1, 6, 4 }, { &each, nullptr, 190, 0 }, { &big, nullptr, 231, 0 } };
    CHECK(valid({ scan(1, 0, 0, 0, 0) }) == -1);
    for (const Case& cs : cases) {
        const int n = (int)imgs.size();
        std::vector<uint8_t> flags(n), uns(n); size_t nrec = 0;
        CHECK(js_export_prog_count(imgs.data(), imgs.size(), nullptr, n, none, cs.s3 ? cs.s3->data() : nullptr, (uint32_t)cs.per3, cs.s1 ? cs.s1->data() : nullptr, (uint32_t)cs.per1, flags.data(), &nrec) == 0);
        size_t want_rec = 0;
        for (int k = 0; k < n; k++) { const bool fits = imgs[k].ncomp == 1 ? cs.s1 != nullptr : true; CHECK(flags[k] == (fits ? 0 : 1)); if (fits) want_rec += imgs[k].ncomp == 1 ? cs.per1 : cs.per3; }
        CHECK(nrec == want_rec);
        const JsExportProgBlock blk = js_export_prog_block(n, nrec);
        std::vector<uint8_t> mem(blk.b.total);
        JsExportRec* recs = reinterpret_cast<JsExportRec*>(mem.data() + blk.b.recs); uint32_t* rec_base = reinterpret_cast<uint32_t*>(mem.data() + blk.b.unit_base);
        JsExportScanRec* srecs = reinterpret_cast<JsExportScanRec*>(mem.data() + blk.srecs); uint32_t* tile_base = reinterpret_cast<uint32_t*>(mem.data() + blk.tile_base);
        uint32_t* chunk_base = reinterpret_cast<uint32_t*>(mem.data() + blk.chunk_base);
        uint64_t blocks = 0, units = 0, ivs = 0;
        CHECK(js_export_plan(imgs.data(), imgs.size(), spec, nullptr, n, qfn, nullptr, recs, rec_base, mem.data() + blk.b.hdrs, uns.data(), &blocks) == 0);
        for (int k = 0; k < n; k++) uns[k] |= flags[k];
        CHECK(js_export_prog_plan(imgs.data(), nullptr, n, none, cs.s3 ? cs.s3->data() : nullptr, (uint32_t)cs.per3, cs.s1 ? cs.s1->data() : nullptr, (uint32_t)cs.per1, recs, uns.data(),
                                  mem.data() + blk.b.hdrs, (uint32_t)(blk.posts - blk.b.hdrs), srecs, rec_base, tile_base, &units, &ivs) == 0);
        CHECK(rec_base[n] == nrec && ivs == nrec);
        uint64_t u = 0, t = 0;
        for (size_t i = 0; i < nrec; i++) {
            CHECK(srecs[i].ubase == u && tile_base[i] == t && srecs[i].itab_off == i && srecs[i].nunits > 0 && (srecs[i].pre_len != 0) == (srecs[i].scan == 0));
            CHECK(srecs[i].post_off + srecs[i].post_len <= blk.b.total - blk.b.hdrs && srecs[i].post_len <= JS_PROG_POST);
            u += srecs[i].nunits; t += (srecs[i].nunits + 255) / 256;
        }
        CHECK(u == units && tile_base[nrec] == t);
        // the first wait's numbers, made up: every scan a byte an interval and the shortest header piece; entry 2 inexact at block 3
        std::vector<uint32_t> res(3 * n, 0), hdr_len(nrec); std::vector<uint64_t> bits(nrec, 8);
        for (int k = 0; k < n; k++) { res[n + 2 * k] = res[n + 2 * k + 1] = 0xFFFFFFFFu; }
        res[2] = JSNOOP_EXPORT_INEXACT; res[n + 4] = 3;
        for (size_t i = 0; i < nrec; i++) hdr_len[i] = srecs[i].pre_len + srecs[i].post_len + srecs[i].ntab * 22;
        std::vector<int> result(n); std::vector<uint32_t> detail(n); uint64_t ub = 0, ob = 0;
        CHECK(js_export_prog_layout(recs, srecs, rec_base, n, uns.data(), res.data(), bits.data(), hdr_len.data(), chunk_base, result.data(), detail.data(), &ub, &ob) == 0);
        CHECK(result[2] == JSNOOP_EXPORT_INEXACT && detail[2] == 3 && !recs[2].live && recs[2].out_cap == 0 && result[0] == JSNOOP_EXPORT_OK && recs[0].live);
        uint64_t cap = 2; for (uint32_t i = rec_base[0]; i < rec_base[1]; i++) cap += hdr_len[i] + 2;
        CHECK(recs[0].out_cap == ((cap + 15) & ~15ull) && chunk_base[rec_base[1]] == rec_base[1] - rec_base[0] && recs[1].out_off == recs[0].out_cap);
        bits[0] = 12; CHECK(js_export_prog_layout(recs, srecs, rec_base, n, uns.data(), res.data(), bits.data(), hdr_len.data(), chunk_base, result.data(), detail.data(), &ub, &ob) == -1 && says("bits"));
        bits[0] = 8; hdr_len[0] = JS_PROG_HDR + 1; CHECK(js_export_prog_layout(recs, srecs, rec_base, n, uns.data(), res.data(), bits.data(), hdr_len.data(), chunk_base, result.data(), detail.data(), &ub, &ob) == -1 && says("header piece"));
    }
    // every byte FF and a marker behind every interval: the count the stuffing kernel can reach
    CHECK(js_export_prog_scan_cap(100, 1000, 50) == 100 + 2000 + 98 && js_export_prog_scan_cap(0, 1, 1) == 2 && js_export_prog_scan_cap(7, 0, 0) == 7);
    {   // an entry the mode refuses: Ri above 65535 in one scan, another precision is js_export_plan's, an index out of range names the entry
        JsnoopExportRestart rs = none; rs.mode = JSNOOP_RESTART_ROWS; rs.interval = 219;
        std::vector<uint8_t> flags(imgs.size()); size_t nrec = 0;
        CHECK(js_export_prog_count(imgs.data(), imgs.size(), nullptr, (int)imgs.size(), rs, d3.data(), 6, d1.data(), 4, flags.data(), &nrec) == 0 && flags[6] == 1 && flags[0] == 0 && flags[1] == 0);
        const int bad[2] = { 0, 99 };
        CHECK(js_export_prog_count(imgs.data(), imgs.size(), bad, 2, rs, d3.data(), 6, d1.data(), 4, flags.data(), &nrec) == -1 && says("index 99 (entry 1)"));
    }
    printf("ok\n");
    return 0;
}
