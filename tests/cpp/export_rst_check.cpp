// Host-only program: the host arithmetic jsnoop_batch_export_jpeg_rst adds (jpegsnoop_amd/csrc/jsnoop_export_rst_check.h) on hand-made image descriptors -- the
// restart spec and every refusal, the effective interval of the four modes, the side records with DRI in the headers, interval-table sizes, the worst-case size of
// a file, the second phase's layout -- and the scan operator the kernels place blocks with: associativity on random summaries, and against a sequential loop over
// blocks.  tests/test_export_rst_abi.py builds it with the address and undefined-behaviour sanitizers and runs it.  Prints "ok" and returns 0, or the line that failed.
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
#include "../../jpegsnoop_amd/csrc/jsnoop_export_rst_check.h"

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
static bool same(const JsRstSum& a, const JsRstSum& b) { return a.has == b.has && a.head == b.head && a.mid == b.mid && a.tail == b.tail; }

int main()
{
    static const uint32_t k420[3][2] = { { 2, 2 }, { 1, 1 }, { 1, 1 } }, kGrey[1][2] = { { 1, 1 } };
    // 0: 4:2:0, 21 x 14 MCUs, decoded with DRI 5; 1: one grey block; 2: grey, 65535 blocks wide (ROWS 2 is 131070 MCUs); 3: grey 1024 x 1024 blocks = 2^20 MCUs; 4: grey 2048 x 2048 blocks
    std::vector<JsImage> imgs = { image(3, k420, 333, 217, 5), image(1, kGrey, 1, 1), image(1, kGrey, 65535 * 8, 16), image(1, kGrey, 8192, 8192), image(1, kGrey, 16384, 16384) };
    CHECK(sizeof(JsnoopExportRestart) == 16 && sizeof(JsExportRstRec) == 16 && sizeof(JsRstSum) == 16 && sizeof(JsExportRec) == 552);
    CHECK(imgs[0].mcu_xmax == 21 && imgs[0].mcu_ymax == 14 && imgs[3].total_blocks == 1u << 20);

    // the spec: defaults, NULL, a shorter struct accepted, a longer one and every bad combination refused
    JsnoopExportRestart def; memset(&def, 0xEE, sizeof def); js_export_restart_defaults(&def);
    CHECK(def.struct_size == 16 && def.mode == JSNOOP_RESTART_NONE && def.interval == 0 && def.reserved == 0);
    JsnoopExportRestart in = def, r;
    CHECK(js_export_import_restart(nullptr, &r) == 0 && r.mode == 0 && r.interval == 0 && r.struct_size == 16);
    in.mode = JSNOOP_RESTART_MCUS; in.interval = 7; CHECK(js_export_import_restart(&in, &r) == 0 && r.mode == 1 && r.interval == 7);
    in.struct_size = 8; CHECK(js_export_import_restart(&in, &r) == -1 && g_err.find("interval = 0") != std::string::npos);      // mode without its interval
    in.mode = JSNOOP_RESTART_SOURCE; CHECK(js_export_import_restart(&in, &r) == 0 && r.mode == 3 && r.interval == 0 && r.struct_size == 16);
    in.struct_size = 4; in.mode = 99; CHECK(js_export_import_restart(&in, &r) == 0 && r.mode == 0);
    in.struct_size = 20; CHECK(js_export_import_restart(&in, &r) == -1 && g_err.find("struct_size") != std::string::npos);
    in.struct_size = 0; CHECK(js_export_import_restart(&in, &r) == -1);
    in = def;
    in.mode = 4; CHECK(js_export_import_restart(&in, &r) == -1 && g_err.find("mode = 4") != std::string::npos);
    in.mode = -1; CHECK(js_export_import_restart(&in, &r) == -1 && g_err.find("mode = -1") != std::string::npos);
    for (int mode : { JSNOOP_RESTART_MCUS, JSNOOP_RESTART_ROWS }) {
        in = def; in.mode = mode;
        in.interval = 0; CHECK(js_export_import_restart(&in, &r) == -1 && g_err.find("interval = 0") != std::string::npos);
        in.interval = 65536; CHECK(js_export_import_restart(&in, &r) == -1 && g_err.find("interval = 65536") != std::string::npos);
        in.interval = 65535; CHECK(js_export_import_restart(&in, &r) == 0);
        in.reserved = 1; CHECK(js_export_import_restart(&in, &r) == -1 && g_err.find("reserved") != std::string::npos);
    }
    for (int mode : { JSNOOP_RESTART_NONE, JSNOOP_RESTART_SOURCE }) {
        in = def; in.mode = mode; in.interval = 1; CHECK(js_export_import_restart(&in, &r) == -1 && g_err.find("takes none") != std::string::npos);
        in.interval = 0; in.reserved = 5; CHECK(js_export_import_restart(&in, &r) == -1 && g_err.find("reserved") != std::string::npos);
    }

    // the effective interval of the four modes
    in = def; CHECK(js_export_rst_ri(in, imgs[0]) == 0);
    in.mode = JSNOOP_RESTART_MCUS; in.interval = 9; CHECK(js_export_rst_ri(in, imgs[0]) == 9 && js_export_rst_ri(in, imgs[2]) == 9);
    in.mode = JSNOOP_RESTART_ROWS; in.interval = 2; CHECK(js_export_rst_ri(in, imgs[0]) == 42 && js_export_rst_ri(in, imgs[2]) == 131070 && js_export_rst_ri(in, imgs[1]) == 2);
    in.interval = 65535; CHECK(js_export_rst_ri(in, imgs[2]) == 65535ull * 65535ull);
    in.mode = JSNOOP_RESTART_SOURCE; in.interval = 0; CHECK(js_export_rst_ri(in, imgs[0]) == 5 && js_export_rst_ri(in, imgs[1]) == 0);
    { JsImage odd = imgs[0]; odd.rst_en = 0; CHECK(js_export_rst_ri(in, odd) == 0); }

    // the plan, both Huffman modes: ROWS 2 over the list -- entry 1 (65535 blocks wide) is refused on the host and owns no unit
    JsnoopExportSpec spec; js_export_spec_defaults(&spec);
    const int list[] = { 0, 2, 1, 3, 0 }; const int n = 5;
    for (int opt = 0; opt < 2; opt++) {
        const JsExportRstBlock rb = js_export_rst_block((size_t)n, opt != 0);
        const size_t base_total = opt ? js_export_opt_block((size_t)n).b.total : js_export_block((size_t)n).total;
        CHECK(rb.rrecs == base_total && rb.o.b.total >= rb.rrecs + n * sizeof(JsExportRstRec) && !(rb.o.b.total % 16) && !(rb.rrecs % 16));
        std::vector<JsExportRec> recs((size_t)n); std::vector<JsExportOptRec> orecs((size_t)n); std::vector<JsExportRstRec> rrecs((size_t)n); std::vector<uint32_t> base((size_t)n + 1, 0xA5A5A5A5u);
        std::vector<uint8_t> hdrs((size_t)n * JS_EXPORT_HDR_MAX, 0xA5), uns((size_t)n, 0xA5); uint64_t blocks = 0, ivs = 0; std::vector<uint64_t> ri((size_t)n, 77);
        if (opt) CHECK(js_export_opt_plan(imgs.data(), imgs.size(), spec, list, n, qfn, nullptr, recs.data(), orecs.data(), base.data(), hdrs.data(), uns.data(), &blocks) == 0);
        else CHECK(js_export_plan(imgs.data(), imgs.size(), spec, list, n, qfn, nullptr, recs.data(), base.data(), hdrs.data(), uns.data(), &blocks) == 0);
        const std::vector<JsExportRec> plain = recs; const std::vector<uint8_t> plain_hdrs = hdrs;
        in = def; in.mode = JSNOOP_RESTART_ROWS; in.interval = 2;
        CHECK(js_export_rst_plan(imgs.data(), in, list, n, recs.data(), opt ? orecs.data() : nullptr, rrecs.data(), base.data(), hdrs.data(), uns.data(), ri.data(), &blocks, &ivs) == 0);
        CHECK(!uns[0] && uns[1] == 1 && !uns[2] && !uns[3] && !uns[4]);
        CHECK(ri[0] == 42 && ri[1] == 131070 && ri[2] == 2 && ri[3] == 2048 && ri[4] == 42);
        const uint32_t u0 = (imgs[0].total_blocks + JS_EXPORT_TILE - 1) / JS_EXPORT_TILE, u3 = imgs[3].total_blocks / JS_EXPORT_TILE;
        CHECK(base[0] == 0 && base[1] == u0 && base[2] == u0 && base[3] == u0 + 1 && base[4] == u0 + 1 + u3 && base[5] == 2 * u0 + 1 + u3);
        CHECK(recs[2].blk_base == imgs[0].total_blocks && recs[3].blk_base == imgs[0].total_blocks + 1 && blocks == 2ull * imgs[0].total_blocks + 1 + imgs[3].total_blocks);
        CHECK(rrecs[0].ri_blocks == 42 * 6 && rrecs[0].ni == 7 && rrecs[0].itab_off == 0 && rrecs[2].ri_blocks == 2 && rrecs[2].ni == 1 && rrecs[2].itab_off == 7);
        CHECK(rrecs[3].ri_blocks == 2048 && rrecs[3].ni == 512 && rrecs[3].itab_off == 8 && rrecs[4].itab_off == 520 && ivs == 527);
        for (int k = 0; k < n; k++) {
            if (uns[k]) { CHECK(recs[k].hdr_len == plain[k].hdr_len); continue; }
            const JsExportRec& rr = recs[k]; const uint8_t* h = hdrs.data() + rr.hdr_off; const uint8_t* p = plain_hdrs.data() + rr.hdr_off;
            const uint32_t sos_len = 8 + 2 * rr.ncomp, sos = plain[k].hdr_len - sos_len;
            CHECK(rr.hdr_len == plain[k].hdr_len + 6 && !memcmp(h, p, sos) && !memcmp(h + sos + 6, p + sos, sos_len));
            CHECK(h[sos] == 0xFF && h[sos + 1] == 0xDD && h[sos + 2] == 0 && h[sos + 3] == 4 && h[sos + 4] == (ri[k] >> 8) && h[sos + 5] == (ri[k] & 255));
            if (opt) CHECK(orecs[k].sos_off == sos && orecs[k].sos_len == sos_len + 6 && orecs[k].sos_off + orecs[k].sos_len == rr.hdr_len && h[orecs[k].sos_off + 6] == 0xFF && h[orecs[k].sos_off + 7] == 0xDA);
        }
        // SOURCE over the same list: only the image decoded with DRI gets one; the others are one interval and keep their headers
        recs = plain; hdrs = plain_hdrs; std::fill(uns.begin(), uns.end(), 0);
        if (opt) for (int k = 0; k < n; k++) CHECK(js_export_opt_split(hdrs.data() + recs[k].hdr_off, recs[k].hdr_len, recs[k].ncomp, &orecs[k]) == 0);
        in = def; in.mode = JSNOOP_RESTART_SOURCE;
        CHECK(js_export_rst_plan(imgs.data(), in, list, n, recs.data(), opt ? orecs.data() : nullptr, rrecs.data(), base.data(), hdrs.data(), uns.data(), ri.data(), &blocks, &ivs) == 0);
        CHECK(ri[0] == 5 && ri[1] == 0 && ri[2] == 0 && ri[3] == 0 && ri[4] == 5 && rrecs[0].ni == 59 && rrecs[0].ri_blocks == 30 && rrecs[1].ni == 1 && rrecs[1].ri_blocks == 0 && ivs == 59 + 3 + 59);
        CHECK(recs[1].hdr_len == plain[1].hdr_len && recs[0].hdr_len == plain[0].hdr_len + 6 && !uns[1]);

        // scratch: summaries and interval tables behind the plain pieces
        const JsExportRstScratch s = js_export_rst_scratch(3, 1000, 70000, 1u << 20, opt != 0);
        const size_t plain_total = opt ? js_export_opt_scratch(3, 1000, 70000).s.total : js_export_scratch(3, 1000, 70000).total;
        CHECK(s.sums == plain_total && s.itab >= s.sums + 16000 && s.o.s.total >= s.itab + (8u << 20) && !(s.sums % 16) && !(s.itab % 16));

        // second phase with ROWS 2 again: NI of 1, 512 and 7, the worst-case size of a file, bit counts the kernels cannot have produced
        recs = plain; hdrs = plain_hdrs; std::fill(uns.begin(), uns.end(), 0);
        if (opt) for (int k = 0; k < n; k++) CHECK(js_export_opt_split(hdrs.data() + recs[k].hdr_off, recs[k].hdr_len, recs[k].ncomp, &orecs[k]) == 0);
        in = def; in.mode = JSNOOP_RESTART_ROWS; in.interval = 2;
        CHECK(js_export_rst_plan(imgs.data(), in, list, n, recs.data(), opt ? orecs.data() : nullptr, rrecs.data(), base.data(), hdrs.data(), uns.data(), ri.data(), &blocks, &ivs) == 0);
        std::vector<uint32_t> res(3 * n, 0xFFFFFFFFu), hl((size_t)n, 0), cb((size_t)n + 1, 0xA5A5A5A5u); std::vector<uint64_t> bits((size_t)n, 0);
        std::vector<int> result((size_t)n, -7); std::vector<uint32_t> detail((size_t)n, 77);
        for (int k = 0; k < n; k++) { res[k] = 0; bits[k] = 8ull * ((uint64_t)recs[k].nblk + rrecs[k].ni); if (opt) hl[k] = orecs[k].pre_len + orecs[k].sos_len + orecs[k].nslots * 22u; }
        res[4] = JSNOOP_EXPORT_UNCODABLE; res[n + 9] = 252;
        uint64_t ub = 0, obytes = 0;
        const std::vector<JsExportRec> before = recs;
        auto layout = [&]() { std::vector<JsExportRec> r2 = before; g_err.clear();
            const int rc = js_export_rst_layout(r2.data(), opt ? orecs.data() : nullptr, rrecs.data(), n, uns.data(), res.data(), bits.data(), opt ? hl.data() : nullptr, cb.data(), result.data(), detail.data(), &ub, &obytes);
            if (!rc) recs = r2;
            return rc; };
        CHECK(layout() == 0);
        CHECK(result[0] == 0 && result[1] == 3 && result[2] == 0 && result[3] == 0 && result[4] == 2 && detail[4] == 252 && recs[0].live && !recs[1].live && !recs[4].live);
        const uint64_t nb0 = bits[0] / 8, nb3 = bits[3] / 8;
        CHECK(recs[0].out_cap == ((recs[0].hdr_len + 2 * nb0 + 2 * 6 + 2 + 15) & ~15ull) && recs[2].out_cap == ((recs[2].hdr_len + 2 * 2 + 0 + 2 + 15) & ~15ull));
        CHECK(recs[3].out_cap == ((recs[3].hdr_len + 2 * nb3 + 2 * 511 + 2 + 15) & ~15ull) && recs[2].out_off == recs[0].out_cap && obytes == recs[3].out_off + recs[3].out_cap);
        CHECK(cb[0] == 0 && cb[1] == (nb0 + 4095) / 4096 && cb[2] == cb[1] && cb[3] == cb[2] + 1 && cb[5] == cb[4]);
        if (opt) CHECK(recs[0].hdr_len == hl[0] && recs[3].hdr_off == 3 * JS_EXPORT_OPT_HDR);
        bits[0] += 4; CHECK(layout() == -1 && g_err.find("bits") != std::string::npos);                   // no multiple of 8
        bits[0] = 8ull * rrecs[0].ni - 8; CHECK(layout() == -1);                                          // an interval without a byte
        bits[0] = 8ull * rrecs[0].ni; CHECK(layout() == 0);
        const uint64_t top = (uint64_t)before[0].nblk * (opt ? 1665u : 1658u) + 7u * rrecs[0].ni;
        bits[0] = top & ~7ull; CHECK(layout() == 0);
        bits[0] = (top & ~7ull) + 8; CHECK(layout() == -1);
        bits[0] = 8ull * rrecs[0].ni; res[0] = 4; CHECK(layout() == -1 && g_err.find("result") != std::string::npos);
    }
    // NI = 2^20 (MCUS 4 on the 2^22-block grey image), and a stream past 2^32 bits: every block the longest there is
    {
        const int one[] = { 4 };
        std::vector<JsExportRec> recs(1); std::vector<JsExportRstRec> rrecs(1); uint32_t base[2]; std::vector<uint8_t> hdrs(JS_EXPORT_HDR_MAX), uns(1); uint64_t blocks = 0, ivs = 0, ri = 0;
        CHECK(js_export_plan(imgs.data(), imgs.size(), spec, one, 1, qfn, nullptr, recs.data(), base, hdrs.data(), uns.data(), &blocks) == 0);
        in = def; in.mode = JSNOOP_RESTART_MCUS; in.interval = 4;
        CHECK(js_export_rst_plan(imgs.data(), in, one, 1, recs.data(), nullptr, rrecs.data(), base, hdrs.data(), uns.data(), &ri, &blocks, &ivs) == 0);
        CHECK(rrecs[0].ni == 1u << 20 && ivs == 1u << 20 && rrecs[0].ri_blocks == 4 && ri == 4);
        CHECK(js_export_rst_scratch(1, base[1], blocks, ivs, false).o.s.total >= (8u << 20));
        uint32_t res[3] = { 0, 0, 0 }, cb[2]; uint64_t bits = 8ull * 829 * (1u << 20), ub, ob; int result; uint32_t detail;
        CHECK(bits > (1ull << 32));
        CHECK(js_export_rst_layout(recs.data(), nullptr, rrecs.data(), 1, uns.data(), res, &bits, nullptr, cb, &result, &detail, &ub, &ob) == 0);
        CHECK(recs[0].out_cap == ((recs[0].hdr_len + 2ull * 829 * (1u << 20) + 2ull * ((1u << 20) - 1) + 2 + 15) & ~15ull) && cb[1] == 829u * (1u << 20) / 4096u);
        CHECK(4 * 1658 == 8 * 829);
        CHECK(js_export_rst_out_cap(100, 1, 1) == 112 && js_export_rst_out_cap(100, 2, 2) == 112 && js_export_rst_out_cap(0, 4096, 4096) == ((8192 + 8190 + 2 + 15) & ~15ull));
    }

    // NI = 2: MCUS 1 on a picture of two MCUs, through the plan and the layout
    {
        std::vector<JsImage> two = { image(3, k420, 32, 16) };
        CHECK(two[0].mcu_xmax == 2 && two[0].mcu_ymax == 1 && two[0].total_blocks == 12);
        std::vector<JsExportRec> recs(1); std::vector<JsExportRstRec> rrecs(1); uint32_t base[2]; std::vector<uint8_t> hdrs(JS_EXPORT_HDR_MAX), uns(1); uint64_t blocks = 0, ivs = 0, ri = 0;
        CHECK(js_export_plan(two.data(), two.size(), spec, nullptr, 1, qfn, nullptr, recs.data(), base, hdrs.data(), uns.data(), &blocks) == 0);
        const uint32_t plain_len = recs[0].hdr_len;
        in = def; in.mode = JSNOOP_RESTART_MCUS; in.interval = 1;
        CHECK(js_export_rst_plan(two.data(), in, nullptr, 1, recs.data(), nullptr, rrecs.data(), base, hdrs.data(), uns.data(), &ri, &blocks, &ivs) == 0);
        CHECK(rrecs[0].ni == 2 && rrecs[0].ri_blocks == 6 && rrecs[0].itab_off == 0 && ivs == 2 && ri == 1 && recs[0].hdr_len == plain_len + 6 && base[1] == 1 && blocks == 12);
        const JsExportRstScratch s = js_export_rst_scratch(1, base[1], blocks, ivs, false);
        CHECK(s.itab >= s.sums + sizeof(JsRstSum) && s.o.s.total >= s.itab + 16);
        uint32_t res[3] = { 0, 0, 0 }, cb[2]; uint64_t bits = 8 * 9, ub, ob; int result; uint32_t detail;      // e.g. intervals of 4 and 5 bytes
        CHECK(js_export_rst_layout(recs.data(), nullptr, rrecs.data(), 1, uns.data(), res, &bits, nullptr, cb, &result, &detail, &ub, &ob) == 0);
        CHECK(result == 0 && recs[0].live && recs[0].out_cap == ((recs[0].hdr_len + 2 * 9 + 2 * 1 + 2 + 15) & ~15ull) && cb[1] == 1 && ob == recs[0].out_cap && ub == 16 + 16);
        bits = 8; CHECK(js_export_rst_layout(recs.data(), nullptr, rrecs.data(), 1, uns.data(), res, &bits, nullptr, cb, &result, &detail, &ub, &ob) == -1);      // two intervals, one byte
    }

    // the scan operator: identity, associativity on random summaries (runs made of blocks, so the summaries are ones that occur), and a scan by it against a
    // sequential loop that pads at every interval end
    {
        const JsRstSum id = js_rst_identity();
        for (int it = 0; it < 20000; it++) {
            JsRstSum s[3];
            for (JsRstSum& x : s) {
                x = id;
                const uint32_t nblocks = rnd() % 5;
                for (uint32_t b = 0; b < nblocks; b++) x = js_rst_combine(x, js_rst_leaf(2 + rnd() % 1664, rnd() % 3 == 0));
            }
            CHECK(same(js_rst_combine(js_rst_combine(s[0], s[1]), s[2]), js_rst_combine(s[0], js_rst_combine(s[1], s[2]))));
            CHECK(same(js_rst_combine(id, s[0]), s[0]) && same(js_rst_combine(s[0], id), s[0]));
            const uint64_t pos = 8ull * (rnd() % 1000) + rnd() % 8;
            CHECK(js_rst_apply(js_rst_apply(pos, s[0]), s[1]) == js_rst_apply(pos, js_rst_combine(s[0], s[1])));
        }
        for (uint32_t rbk : { 0u, 1u, 2u, 6u, 255u, 256u, 257u, 258u, 1000u }) {
            const uint32_t nblk = 3 * 256 + 77;
            std::vector<uint32_t> bits(nblk); for (uint32_t& b : bits) b = 2 + rnd() % 1664;
            // sequential
            std::vector<uint64_t> want(nblk); uint64_t pos = 0;
            for (uint32_t j = 0; j < nblk; j++) { want[j] = pos; pos += bits[j]; if (j + 1 == nblk || (rbk && (j + 1) % rbk == 0)) pos = (pos + 7) & ~7ull; }
            // tiles of 256 by the operator: a summary per tile, positions inside from the tile's
            uint64_t carry = 0;
            for (uint32_t t0 = 0; t0 < nblk; t0 += 256) {
                JsRstSum run = id;
                for (uint32_t j = t0; j < nblk && j < t0 + 256; j++) {
                    CHECK(js_rst_apply(carry, run) == want[j]);
                    run = js_rst_combine(run, js_rst_leaf(bits[j], j + 1 == nblk || (rbk && (j + 1) % rbk == 0)));
                }
                carry = js_rst_apply(carry, run);
            }
            CHECK(carry == pos && !(pos & 7));
        }
        // a position past 2^32 bits moves on exactly
        const uint64_t far = (1ull << 33) + 8; JsRstSum a = js_rst_leaf(13, true);
        CHECK(js_rst_apply(far, a) == far + 16 && js_rst_apply(far + 3, js_rst_leaf(5, false)) == far + 8);
    }
    printf("ok\n");
    return 0;
}
