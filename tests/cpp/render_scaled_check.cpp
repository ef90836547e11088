// Host-only program: the host arithmetic of jsnoop_batch_pack_ijg_scaled (jpegsnoop_amd/csrc/jsnoop_render_scaled_check.h) and the reduced render
// k_render_ijg_scaled runs, which that header compiles for both sides -- every refusal of denom, spec, destination and layout, the reduced sizes, the unit plan
// against a brute-force walk for the four layouts x three scales and edge sizes (1, 65535), the job list of every unit (every block inside the image's arena rows,
// every sample on a cell of the plane it belongs to, no cell written twice, no cell looked up that no job wrote, no workspace row past 63, a 1 x 1 component
// without an arena row).  tests/test_render_scaled_abi.py builds it with the address and undefined-behaviour sanitizers and runs it.  Prints "ok" and returns 0,
// or the line that failed.
//   render_scaled_check block N c0 .. c63   prints the N x N results of one block (before the + 128 and the clamp): the test compares them with the model
//   render_scaled_check render W H ncomp HS VS denom arena.bin out.bin
//                                        renders one image with the stages the kernel calls -- unit by unit, phase by phase, lanes 0 .. 63 in turn between the
//                                        barriers, through a copy of a wave's LDS that starts poisoned -- from int16 arena rows (slot 0 = cumulative DC) into
//                                        ceil(W / denom) x ceil(H / denom) x 3 bytes.  The DCs are handed over as dccum and every arena value the contract says
//                                        is not read (slot 0, row and column 4 of a 4 x 4, rows and columns 2, 4, 6 of a 2 x 2, all of a 1 x 1) is poisoned first.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#ifndef __HIPCC__              // (a plain host compiler: the descriptors' header marks one helper for both sides)
#define __host__
#define __device__
#endif
#include "../../jpegsnoop_amd/csrc/jsnoop_render_scaled_check.h"

static std::string g_err;
void js_set_error(const char* fmt, ...) { char buf[512]; va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap); g_err = buf; }

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, g_err.c_str()); return 1; } } while (0)
#define REFUSED(call, word) do { g_err.clear(); CHECK((call) == -1); CHECK(g_err.find(word) != std::string::npos); } while (0)

// the descriptor a decode leaves for a w x h image: lay 0 grey, 1 4:4:4, 2 4:2:2, 3 4:2:0
static JsImage image(uint32_t w, uint32_t h, int lay)
{
    JsImage im; memset(&im, 0, sizeof im);
    const uint32_t H = lay >= 2 ? 2 : 1, V = lay == 3 ? 2 : 1;
    im.dim_x = w; im.dim_y = h; im.ncomp = lay ? 3 : 1; im.precision = 8; im.mcu_w = 8 * H; im.mcu_h = 8 * V;
    im.mcu_xmax = (w + 8 * H - 1) / (8 * H); im.mcu_ymax = (h + 8 * V - 1) / (8 * V);
    uint32_t nb = 0;
    for (uint32_t c = 1; c <= im.ncomp; c++) {
        const uint32_t sh = c == 1 ? H : 1, sv = c == 1 ? V : 1;
        im.samp_h[c] = sh; im.samp_v[c] = sv; im.expand_h[c] = H / sh; im.expand_v[c] = V / sv;
        for (uint32_t y = 0; y < sv; y++) for (uint32_t x = 0; x < sh; x++) { im.blk_comp[nb] = (uint8_t)c; im.blk_ch[nb] = (uint8_t)x; im.blk_cv[nb] = (uint8_t)y; nb++; }
    }
    im.blk_per_mcu = nb; im.blk_xmax = im.mcu_xmax * H; im.blk_ymax = im.mcu_ymax * V; im.img_x = im.mcu_xmax * im.mcu_w; im.img_y = im.mcu_ymax * im.mcu_h;
    im.total_blocks = im.mcu_xmax * im.mcu_ymax * nb; im.preview_mode = 1;
    return im;
}

static int plan_one(const JsImage& im, unsigned denom, JsRsRec* rec, uint32_t ub[2])
{
    JsnoopPackSpec s; js_pack_spec_defaults(&s);
    JsnoopPackDst d; memset(&d, 0, sizeof d); d.ptr = (void*)(uintptr_t)0x10000;
    return js_rs_plan(&im, 1, s, denom, nullptr, 1, &d, rec, ub);
}

template <int N>
static void block_n(const int* c, int32_t* out)
{
    int32_t ws[N * 8];
    for (int x = 0; x < 8; x++) {
        int32_t v[8], o[8]; for (int k = 0; k < 8; k++) v[k] = c[k * 8 + x];
        if (N == 4) js_rs_step4<12>(v, o); else js_rs_step2<13>(v, o);
        for (int k = 0; k < N; k++) ws[k * 8 + x] = o[k];
    }
    for (int y = 0; y < N; y++) {
        int32_t o[8];
        if (N == 4) js_rs_step4<19>(ws + y * 8, o); else js_rs_step2<20>(ws + y * 8, o);
        for (int k = 0; k < N; k++) out[y * N + k] = o[k];
    }
}

// The job list of one unit, without an arena: where every job's block lies, which plane cells it writes, which cells the pixel stage looks up.
// -1: a bound of the header does not hold (the text says which).
static int walk_unit(const JsRsRec& r, uint32_t my, uint32_t m0, uint64_t nblocks)
{
    static uint8_t live[JS_RS_OFF_TILE];
    memset(live, 0, sizeof live);
    const uint32_t nm = r.mcu_xmax - m0 < r.run ? r.mcu_xmax - m0 : r.run;
    for (uint32_t phase = 0; phase < 2; phase++) {
        const uint32_t n = js_rs_n(r, phase), njobs = js_rs_jobs(r, nm, phase);
        if (!njobs) continue;
        if (n != 1u && n != 2u && n != 4u && n != 8u) { js_set_error("a transform size of %u", n); return -1; }
        const uint32_t group = 64u / n, padded = (njobs + group - 1u) / group * group;
        for (uint32_t jb = 0; jb < padded + 8u; jb++) {
            const JsRsJob j = js_rs_job(r, my, m0, nm, phase, jb);
            if (jb >= njobs && (j.exists || j.keep)) { js_set_error("a job past the phase's count exists"); return -1; }
            if (!j.exists) { if (j.keep) { js_set_error("a job that does not exist keeps samples"); return -1; } continue; }
            if (j.blk >= nblocks) { js_set_error("job %u of phase %u of unit (%u, %u) names block %llu of %llu", jb, phase, my, m0, (unsigned long long)j.blk, (unsigned long long)nblocks); return -1; }
            if ((jb % group) * n + (n - 1u) >= 64u) { js_set_error("a workspace row past 63"); return -1; }
            if (j.keep < 1u || j.keep > 3u) { js_set_error("a keep the kernel has no store for"); return -1; }
            if (n == 1u && j.keep != 1u) { js_set_error("a 1 x 1 halo job"); return -1; }
            const bool own_job = phase == 0u || jb < 2u * nm;
            if (own_job != (j.keep == 1u)) { js_set_error("own / halo mismatch of job %u", jb); return -1; }
            if (j.keep == 1u && (j.cell0 % n)) { js_set_error("an %u-byte write off its boundary", n); return -1; }
            const uint32_t plane = j.cell0 / JS_RS_PLANE_BYTES;
            if (plane != (phase ? 1u + ((own_job ? jb : jb - 2u * nm) & 1u) : 0u)) { js_set_error("job %u of phase %u writes plane %u", jb, phase, plane); return -1; }
            const uint32_t wown = phase && r.H == 2u && r.V == 1u ? nm * r.nc : nm * r.H * r.m;        // the component's own columns in this unit
            for (uint32_t k = 0; k < n; k++) for (uint32_t i = 0; i < (j.keep == 1u ? n : 1u); i++) {
                const uint32_t at = j.cell0 + k * JS_RS_PITCH + i;
                if (at >= JS_RS_OFF_TILE || at / JS_RS_PLANE_BYTES != plane) { js_set_error("a sample outside its plane"); return -1; }
                const uint32_t o = at % JS_RS_PLANE_BYTES, x = o % JS_RS_PITCH;
                if (x < 7u || x > 8u + wown) { js_set_error("a sample outside its row"); return -1; }
                const bool own_cell = x >= 8u && x < 8u + wown;
                if (own_cell != own_job) { js_set_error("job %u of phase %u: own / halo mismatch at cell %u", jb, phase, at); return -1; }
                if (live[at]) { js_set_error("cell %u written twice in unit (%u, %u)", at, my, m0); return -1; }
                live[at] = 1;
            }
        }
    }
    // the pixel stage: four pixels a lane
    const uint32_t ow = r.H * r.m, oh = r.V * r.m, x0 = m0 * ow, y0 = my * oh;
    if (x0 >= r.out_x || y0 >= r.out_y) { js_set_error("a unit outside the reduced picture"); return -1; }
    const uint32_t wpix = nm * ow < r.out_x - x0 ? nm * ow : r.out_x - x0, hpix = oh < r.out_y - y0 ? oh : r.out_y - y0;
    if (wpix > 64u || hpix > 8u) { js_set_error("a unit larger than its planes"); return -1; }
    for (uint32_t ly = 0; ly < hpix; ly++) for (uint32_t lx = 0; lx < wpix; lx += 4u) {
        const uint32_t n = wpix - lx < 4u ? wpix - lx : 4u;
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t at = ly * JS_RS_PITCH + 8u + lx + j;
            if (!live[at]) { js_set_error("a luma cell read that no job wrote"); return -1; }
            if (r.ncomp == 3u && !(r.H == 2u && r.V == 1u) && (!live[JS_RS_PLANE_BYTES + at] || !live[2u * JS_RS_PLANE_BYTES + at])) { js_set_error("a chroma cell read that no job wrote"); return -1; }
        }
        if (r.ncomp == 3u && r.H == 2u && r.V == 1u) {
            // the cells js_rs_chroma4 looks up
            const uint32_t i0 = (x0 + lx) >> 1, c0 = m0 * r.nc, wc = nm * r.nc, dw = r.dwc;
            if (dw <= c0) { js_set_error("a unit without a real chroma sample"); return -1; }
            int cols[4]; int ncols = 0;
            if (!js_rs_filtered(r) || dw <= 2u) {
                const uint32_t last = (dw < c0 + wc ? dw : c0 + wc) - 1u;
                cols[ncols++] = (int)((i0 > last ? last : i0) - c0); cols[ncols++] = (int)((i0 + 1u > last ? last : i0 + 1u) - c0);
            } else for (int k = 0; k < 4; k++) { const int i = (int)i0 - 1 + k; const uint32_t g = i < 0 ? 0u : ((uint32_t)i >= dw ? dw - 1u : (uint32_t)i); cols[ncols++] = (int)g - (int)c0; }
            for (int k = 0; k < ncols; k++) for (uint32_t c = 1; c <= 2; c++) {
                if (cols[k] < -1 || cols[k] > (int)wc) { js_set_error("a chroma look-up outside the plane"); return -1; }
                if (!live[c * JS_RS_PLANE_BYTES + ly * JS_RS_PITCH + 8u + cols[k]]) { js_set_error("unit (%u, %u): chroma column %d read at pixel (%u, %u), no job wrote it", my, m0, cols[k], x0 + lx, y0 + ly); return -1; }
            }
        }
    }
    return 0;
}

// One unit with the stages the kernel calls, lanes in turn where the kernel has a wave.
template <int N>
static void run_phase(const JsRsRec& r, const JsRsUnit& u, uint32_t phase, uint32_t njobs, const int16_t* coef, const int16_t* dccum, uint8_t* mem)
{
    for (uint32_t g0 = 0; g0 < njobs; g0 += 64u / N) {
        for (uint32_t q = 0; q < 8u / N && g0 + q * 8u < njobs; q++) {
            for (uint32_t lane = 0; lane < 64; lane++) js_rs_load<N>(r, u, phase, g0 + q * 8u, lane, coef, dccum, mem);
            for (uint32_t lane = 0; lane < 64; lane++) js_rs_pass1<N>(r, u, phase, g0 + q * 8u, q, lane, mem);
        }
        for (uint32_t lane = 0; lane < 64; lane++) js_rs_pass2<N>(r, u, phase, g0, lane, mem);
        memset(mem + JS_RS_OFF_TILE, 0xCD, JS_RS_WAVE_BYTES - JS_RS_OFF_TILE);             // (nothing of a group's tile or workspace serves the next)
    }
}
static void run_unit(const JsRsRec& r, uint32_t my, uint32_t m0, const int16_t* coef, const int16_t* dccum, uint8_t* out)
{
    alignas(16) static uint8_t mem[JS_RS_WAVE_BYTES];
    memset(mem, 0xCD, sizeof mem);
    JsRsUnit u; u.my = my; u.m0 = m0; u.nm = r.mcu_xmax - m0 < r.run ? r.mcu_xmax - m0 : r.run;
    for (uint32_t phase = 0; phase < 2; phase++) {
        const uint32_t njobs = js_rs_jobs(r, u.nm, phase), n = js_rs_n(r, phase);
        if (n == 8u) run_phase<8>(r, u, phase, njobs, coef, dccum, mem);
        else if (n == 4u) run_phase<4>(r, u, phase, njobs, coef, dccum, mem);
        else if (n == 2u) run_phase<2>(r, u, phase, njobs, coef, dccum, mem);
        else for (uint32_t lane = 0; lane < 64; lane++) for (uint32_t jb = lane; jb < njobs; jb += 64u) js_rs_dc_job(r, u, phase, jb, dccum, mem);
    }
    for (uint32_t ly0 = 0; ly0 < r.V * r.m; ly0 += 4u) for (uint32_t lane = 0; lane < 64; lane++) {
        uint32_t x = 0, y = 0, v[4];
        const uint32_t n = js_rs_pixels(r, u, lane, ly0, false, mem, &x, &y, v);
        for (uint32_t j = 0; j < n; j++) { uint8_t* o = out + ((size_t)y * r.out_x + x + j) * 3u; o[0] = (uint8_t)v[j]; o[1] = (uint8_t)(v[j] >> 8); o[2] = (uint8_t)(v[j] >> 16); }
    }
}

int main(int argc, char** argv)
{
    if (argc == 67 && !strcmp(argv[1], "block")) {
        const int n = atoi(argv[2]); int c[64]; int32_t o[64];
        for (int k = 0; k < 64; k++) c[k] = atoi(argv[3 + k]);
        if (n == 4) block_n<4>(c, o); else if (n == 2) block_n<2>(c, o); else if (n == 1) o[0] = js_rs_dc(c[0]); else return 2;
        for (int k = 0; k < n * n; k++) printf("%d ", o[k]);
        printf("\n");
        return 0;
    }
    if (argc == 10 && !strcmp(argv[1], "render")) {
        const uint32_t w = (uint32_t)atoi(argv[2]), h = (uint32_t)atoi(argv[3]), nc = (uint32_t)atoi(argv[4]), H = (uint32_t)atoi(argv[5]), V = (uint32_t)atoi(argv[6]);
        const unsigned denom = (unsigned)atoi(argv[7]);
        const int lay = nc == 1 ? 0 : (H == 1 ? 1 : (V == 1 ? 2 : 3));
        const JsImage im = image(w, h, lay);
        JsRsRec rec; uint32_t ub[2];
        CHECK(plan_one(im, denom, &rec, ub) == 0);
        std::vector<int16_t> arena((size_t)im.total_blocks * 64), dccum(im.total_blocks);
        FILE* f = fopen(argv[8], "rb"); CHECK(f != nullptr);
        CHECK(fread(arena.data(), 2, arena.size(), f) == arena.size()); fclose(f);
        for (uint32_t b = 0; b < im.total_blocks; b++) {
            dccum[b] = arena[(size_t)b * 64];
            const uint32_t n = b % rec.bpm < (nc == 1 ? 1u : H * V) ? rec.ny : rec.nc;
            for (uint32_t k = 0; k < 64; k++) if (k == 0 || n == 1u || !js_rs_needs(n, k >> 3) || !js_rs_needs(n, k & 7u)) arena[(size_t)b * 64 + k] = 0x5A5A;
        }
        // (where no component is transformed above 1 x 1 the arena pointer itself is poison: the sanitizer stops a read)
        const int16_t* coef = rec.ny == 1u && rec.nc <= 1u ? nullptr : arena.data();
        std::vector<uint8_t> out((size_t)rec.out_x * rec.out_y * 3, 0xEE);
        for (uint32_t u = 0; u < ub[1]; u++) run_unit(rec, u / rec.runs, (u % rec.runs) * rec.run, coef, dccum.data(), out.data());
        f = fopen(argv[9], "wb"); CHECK(f != nullptr);
        CHECK(fwrite(out.data(), 1, out.size(), f) == out.size()); fclose(f);
        printf("ok %u %u\n", rec.out_x, rec.out_y);
        return 0;
    }
    // ---- denominators, sizes, transform sizes
    REFUSED(js_rs_denom(0, "pack_ijg_scaled"), "denom = 0"); REFUSED(js_rs_denom(3, "pack_ijg_scaled"), "denom = 3"); REFUSED(js_rs_denom(16, "pack_ijg_scaled"), "pack_ijg_scaled: denom = 16");
    CHECK(js_rs_denom(1, "x") == 0 && js_rs_denom(2, "x") == 0 && js_rs_denom(4, "x") == 0 && js_rs_denom(8, "x") == 0);
    CHECK(js_rs_out(1, 8) == 1 && js_rs_out(8, 8) == 1 && js_rs_out(9, 8) == 2 && js_rs_out(65535, 2) == 32768 && js_rs_out(17, 4) == 5 && js_rs_out(16, 4) == 4);
    for (uint32_t m = 1; m <= 4; m *= 2) {
        CHECK(js_rs_size(m, 1, 1, 1, 1) == m && js_rs_size(m, 2, 1, 2, 1) == m && js_rs_size(m, 2, 1, 1, 1) == m && js_rs_size(m, 2, 2, 2, 2) == m && js_rs_size(m, 2, 2, 1, 1) == 2 * m);
        CHECK(js_rs_run(1, m) * m == 64 && js_rs_run(2, m) * 2 * m == 64);
    }
    for (uint32_t i = 0; i < 8; i++) CHECK(js_rs_needs(8, i) && js_rs_needs(4, i) == (i != 4) && js_rs_needs(2, i) == (i == 0 || i == 1 || i == 3 || i == 5 || i == 7));
    // ---- the call: every refusal of jsnoop_batch_pack_ijg, under this entry point's name and against the reduced size
    {
        JsnoopPackSpec d, got; js_pack_spec_defaults(&d);
        REFUSED(js_pack_import_spec(nullptr, &got, "pack_ijg_scaled"), "pack_ijg_scaled: spec is NULL");
        { JsnoopPackSpec s = d; s.struct_size = 3; REFUSED(js_pack_import_spec(&s, &got, "pack_ijg_scaled"), "struct_size"); }
        { JsnoopPackSpec s = d; s.layout = 2; REFUSED(js_pack_import_spec(&s, &got, "pack_ijg_scaled"), "pack_ijg_scaled: unknown layout"); s = d; s.dtype = 2; REFUSED(js_pack_import_spec(&s, &got, "pack_ijg_scaled"), "pack_ijg_scaled: unknown dtype"); }
        JsImage imgs[3] = { image(17, 9, 3), image(5, 4, 0), image(16, 16, 3) };
        imgs[2].samp_h[1] = 1; imgs[2].samp_v[1] = 2;                                   // (not renderable)
        imgs[1].coef_off = 12;
        JsRsRec recs[3]; uint32_t ub[4]; JsnoopPackDst dst[3]; memset(dst, 0, sizeof dst);
        for (int k = 0; k < 3; k++) dst[k].ptr = (void*)(uintptr_t)(0x10000 + k);
        const int two[2] = { 1, 0 };
        CHECK(js_rs_plan(imgs, 3, d, 2, two, 2, dst, recs, ub) == 0);
        CHECK(ub[0] == 0 && ub[1] == 1 && ub[2] == 2 && recs[0].ncomp == 1 && recs[0].bpm == 1 && recs[0].coef_off == 12 && recs[0].out_x == 3 && recs[0].out_y == 2 && recs[0].row_pitch == 9 && recs[0].plane_pitch == 18);
        CHECK(recs[0].m == 4 && recs[0].ny == 4 && recs[0].nc == 0 && recs[0].run == 16 && recs[0].runs == 1);
        CHECK(recs[1].H == 2 && recs[1].V == 2 && recs[1].bpm == 6 && recs[1].runs == 1 && recs[1].run == 8 && recs[1].mcu_xmax == 2 && recs[1].out_x == 9 && recs[1].out_y == 5 && recs[1].row_pitch == 27 && recs[1].ptr == 0x10001);
        CHECK(recs[1].ny == 4 && recs[1].nc == 8 && recs[1].dwc == 9);
        CHECK(js_rs_plan(imgs, 3, d, 8, two, 2, dst, recs, ub) == 0 && recs[1].out_x == 3 && recs[1].out_y == 2 && recs[1].ny == 1 && recs[1].nc == 2 && recs[1].run == 32 && recs[1].dwc == 3 && recs[0].ny == 1 && recs[0].run == 64);
        REFUSED(js_rs_plan(imgs, 3, d, 1, two, 2, dst, recs, ub), "denom = 1"); REFUSED(js_rs_plan(imgs, 3, d, 3, two, 2, dst, recs, ub), "denom = 3");
        REFUSED(js_rs_plan(imgs, 3, d, 2, nullptr, 3, dst, recs, ub), "image 2: luma sampling 1 x 2");
        const int bad[2] = { 0, 3 }; REFUSED(js_rs_plan(imgs, 3, d, 4, bad, 2, dst, recs, ub), "image index 3 (entry 1) out of range");
        const int neg[1] = { -1 }; REFUSED(js_rs_plan(imgs, 3, d, 4, neg, 1, dst, recs, ub), "out of range");
        { JsnoopPackDst x[2] = { dst[0], dst[1] }; x[1].ptr = nullptr; REFUSED(js_rs_plan(imgs, 3, d, 2, two, 2, x, recs, ub), "destination 1 (image 0) is NULL"); }
        { JsnoopPackDst x[2] = { dst[0], dst[1] }; x[0].row_pitch = 8; REFUSED(js_rs_plan(imgs, 3, d, 2, two, 2, x, recs, ub), "row_pitch 8"); x[0].row_pitch = 9; CHECK(js_rs_plan(imgs, 3, d, 2, two, 2, x, recs, ub) == 0); }
        { JsnoopPackSpec s = d; s.layout = JSNOOP_PACK_CHW; JsnoopPackDst x[2] = { dst[0], dst[1] }; x[0].row_pitch = 8; x[0].plane_pitch = 15; REFUSED(js_rs_plan(imgs, 3, s, 2, two, 2, x, recs, ub), "plane_pitch 15");
          x[0].plane_pitch = 16; CHECK(js_rs_plan(imgs, 3, s, 2, two, 2, x, recs, ub) == 0 && recs[0].plane_pitch == 16 && recs[0].row_pitch == 8); }
        { JsnoopPackSpec s = d; s.dtype = JSNOOP_PACK_F32; REFUSED(js_rs_plan(imgs, 3, s, 2, two, 2, dst, recs, ub), "multiples of 4");
          JsnoopPackDst x[2] = { dst[0], dst[1] }; x[0].ptr = (void*)(uintptr_t)0x10000; x[1].ptr = (void*)(uintptr_t)0x20000; x[1].row_pitch = 110; REFUSED(js_rs_plan(imgs, 3, s, 2, two, 2, x, recs, ub), "multiples of 4");
          x[1].row_pitch = 108; CHECK(js_rs_plan(imgs, 3, s, 2, two, 2, x, recs, ub) == 0 && recs[0].row_pitch == 36); }
        CHECK(js_rs_dense_bytes(imgs[0], d, 2) == 9 * 5 * 3 && js_rs_dense_bytes(imgs[0], d, 8) == 3 * 2 * 3 && js_rs_dense_row(imgs[1], d, 4) == 6);
        // 2^31 units: 65535 x 65535 grey images at denom 2 are 512 x 8192 units each
        std::vector<JsImage> big(513, image(65535, 65535, 0)); std::vector<JsRsRec> brecs(big.size()); std::vector<uint32_t> bub(big.size() + 1); std::vector<JsnoopPackDst> bd(big.size(), dst[0]);
        REFUSED(js_rs_plan(big.data(), big.size(), d, 2, nullptr, 513, bd.data(), brecs.data(), bub.data()), "2^31 units");
        CHECK(js_rs_plan(big.data(), big.size(), d, 2, nullptr, 511, bd.data(), brecs.data(), bub.data()) == 0 && bub[511] == 511u * 512u * 8192u);
    }
    // ---- the unit plan against a brute-force walk, and the job list of every unit: four layouts, three scales, edge sizes
    {
        const uint32_t sizes[][2] = { { 1, 1 }, { 2, 2 }, { 3, 3 }, { 4, 5 }, { 5, 4 }, { 8, 8 }, { 9, 7 }, { 16, 16 }, { 17, 9 }, { 9, 17 }, { 15, 17 }, { 25, 25 }, { 33, 31 }, { 50, 70 }, { 130, 21 }, { 64, 48 }, { 6, 40 },
                                      { 40, 6 }, { 127, 16 }, { 128, 16 }, { 129, 17 }, { 255, 33 }, { 256, 48 }, { 257, 33 }, { 511, 9 }, { 512, 16 }, { 513, 17 }, { 1025, 47 }, { 65535, 3 }, { 3, 65535 }, { 65535, 33 }, { 17, 65535 } };
        for (int lay = 0; lay < 4; lay++) for (unsigned denom = 2; denom <= 8; denom *= 2) for (const auto& wh : sizes) {
            const JsImage im = image(wh[0], wh[1], lay);
            JsRsRec rec; uint32_t ub[2];
            CHECK(plan_one(im, denom, &rec, ub) == 0);
            const uint32_t H = lay >= 2 ? 2 : 1, V = lay == 3 ? 2 : 1, mx = (wh[0] + 8 * H - 1) / (8 * H), my = (wh[1] + 8 * V - 1) / (8 * V), m = 8 / denom;
            CHECK(rec.mcu_xmax == mx && rec.mcu_ymax == my && rec.bpm == (lay ? H * V + 2 : 1) && rec.H == H && rec.V == V && ub[0] == 0 && ub[1] == js_rs_units(im, H, denom));
            CHECK(rec.out_x == (wh[0] + denom - 1) / denom && rec.out_y == (wh[1] + denom - 1) / denom && rec.m == m && rec.ny == m && rec.nc == (lay == 0 ? 0 : lay == 3 ? 2 * m : m) && rec.run * H * m == 64);
            // every MCU lies in exactly one unit; units follow each other in decode order, straddle no MCU row and hold at most `run` MCUs
            uint64_t next = 0;
            for (uint32_t u = 0; u < ub[1]; u++) {
                const uint32_t row = u / rec.runs, m0 = (u - row * rec.runs) * rec.run;
                CHECK(row < my && m0 < mx);
                const uint32_t nm = mx - m0 < rec.run ? mx - m0 : rec.run;
                CHECK((uint64_t)row * mx + m0 == next && nm >= 1);
                next += nm;
                // (the long thin pictures: the first and last units of a row, the first two and last two rows)
                if (ub[1] > 4096 && !(u < 2 * rec.runs || u >= ub[1] - 2 * rec.runs || m0 < 2 * rec.run || m0 + 2 * rec.run >= mx)) continue;
                CHECK(walk_unit(rec, row, m0, im.total_blocks) == 0);
            }
            CHECK(next == (uint64_t)mx * my);
        }
    }
    // ---- the reduced steps: DC alone is flat at every size, nothing is undefined on wild blocks (the sanitizers watch), results fit the saturation
    {
        int c[64]; int32_t o[64];
        memset(c, 0, sizeof c); c[0] = 8 * 100;
        block_n<4>(c, o); for (int k = 0; k < 16; k++) CHECK(o[k] == 100);
        block_n<2>(c, o); for (int k = 0; k < 4; k++) CHECK(o[k] == 100);
        CHECK(js_rs_dc(800) == 100 && js_rs_dc(-1) == 0 && js_rs_dc(-4) == 0 && js_rs_dc(-5) == -1 && js_rs_dc(3) == 0 && js_rs_dc(4) == 1 && js_rs_dc(-32768) == -4096 && js_rs_dc(32767) == 4096);
        c[4] = 32767; c[32] = -32768; c[36] = 1;                                        // (row and column 4 do not reach the 4 x 4; 2, 4, 6 not the 2 x 2)
        block_n<4>(c, o); for (int k = 0; k < 16; k++) CHECK(o[k] == 100);
        c[2] = 9; c[6] = -9; c[16] = 77; c[48] = -77; c[18] = 5;
        block_n<2>(c, o); for (int k = 0; k < 4; k++) CHECK(o[k] == 100);
        unsigned s = 12345; int32_t peak = 0;
        for (int it = 0; it < 2000; it++) {
            for (int k = 0; k < 64; k++) { s = s * 1664525u + 1013904223u; c[k] = it < 1000 ? (int)(s >> 16) - 32768 : ((s >> 20 & 1) ? 32767 : -32768); }
            block_n<4>(c, o); for (int k = 0; k < 16; k++) if (abs(o[k]) > peak) peak = abs(o[k]);
            block_n<2>(c, o); for (int k = 0; k < 4; k++) if (abs(o[k]) > peak) peak = abs(o[k]);
        }
        CHECK(peak <= 4096);                                                           // (js_ren_sample's + 128 cannot wrap)
    }
    // ---- struct sizes the records are copied with; the LDS layout
    CHECK(sizeof(JsRsRec) == 96 && sizeof(JsnoopPackSpec) == 40 && sizeof(JsnoopPackDst) == 24 && JS_RS_WAVE_BYTES == 6528 && JS_RS_OFF_TILE == 1920 && JS_RS_OFF_WS == 4224);
    for (uint32_t q = 0; q < 64; q++) CHECK(js_rs_ws_row(q) % 8 == 0 && js_rs_ws_row(q) + 8 <= JS_RS_WS_DWORDS && (q == 0 || js_rs_ws_row(q) >= js_rs_ws_row(q - 1) + 8));
    printf("ok\n");
    return 0;
}
