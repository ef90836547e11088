// Host-only program: the host arithmetic of jsnoop_batch_pack_ijg (jpegsnoop_amd/csrc/jsnoop_render_check.h) and the integer render k_render_ijg runs, which
// that header compiles for both sides -- every refusal of spec, destination and layout, the unit plan against a brute-force walk for the four layouts and edge
// sizes (1, 65535), the job list of every unit (every block inside the image's arena rows, every sample on a cell of the plane it belongs to, no cell written
// twice, no halo cell read that no job wrote), and the colour lines over all 2^24 (Y, Cb, Cr) against the contract written out once more.
// tests/test_render_abi.py builds it with the address and undefined-behaviour sanitizers and runs it.  Prints "ok" and returns 0, or the line that failed.
//   render_check block c0 .. c63        prints the 64 results of one block (before the + 128 and the clamp): the test compares them with tests/ijg_model.py
//   render_check render W H ncomp HS VS arena.bin out.bin
//                                        renders one image the way the kernel does -- unit by unit, job by job through a copy of a wave's LDS that starts
//                                        poisoned, four pixels a lane -- from int16 arena rows (slot 0 = cumulative DC) into W x H x 3 bytes
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
#include "../../jpegsnoop_amd/csrc/jsnoop_render_check.h"

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

static void idct_block(const int* c, int32_t* out)
{
    int32_t ws[64];
    for (int x = 0; x < 8; x++) { int32_t v[8]; for (int k = 0; k < 8; k++) v[k] = c[k * 8 + x]; js_ren_idct_step<11>(v); for (int k = 0; k < 8; k++) ws[k * 8 + x] = v[k]; }
    for (int y = 0; y < 8; y++) { int32_t v[8]; for (int k = 0; k < 8; k++) v[k] = ws[y * 8 + k]; js_ren_idct_step<18>(v); for (int k = 0; k < 8; k++) out[y * 8 + k] = v[k]; }
}

// One unit as the kernel runs it; `live` marks the LDS bytes a job wrote.  With out == nullptr only the job list is walked (no arena is read).
// -1: a bound of the header does not hold (the text says which).
static int run_unit(const JsRenRec& r, uint32_t my, uint32_t m0, const int16_t* arena, uint64_t nblocks, uint8_t* out)
{
    static uint8_t mem[JS_REN_WAVE_BYTES]; static uint8_t live[JS_REN_WAVE_BYTES];
    memset(mem, 0xCD, sizeof mem); memset(live, 0, sizeof live);
    const uint32_t nm = r.mcu_xmax - m0 < JS_REN_RUN ? r.mcu_xmax - m0 : JS_REN_RUN, njobs = js_ren_jobs(r, nm);
    if (njobs > JS_REN_MAX_JOBS) { js_set_error("more jobs than JS_REN_MAX_JOBS"); return -1; }
    for (uint32_t jb = 0; jb < ((njobs + 7u) & ~7u); jb++) {
        int32_t res[64]; bool have = false;
        for (uint32_t r8 = 0; r8 < 8; r8++) {
            const JsRenJob j = js_ren_job(r, my, m0, nm, jb, r8);
            if (jb >= njobs && (j.exists || j.mask)) { js_set_error("a job past the unit's count exists"); return -1; }
            if (!j.exists) { if (j.mask) { js_set_error("a job that does not exist keeps samples"); return -1; } continue; }
            if (j.blk >= nblocks) { js_set_error("job %u of unit (%u, %u) names block %llu of %llu", jb, my, m0, (unsigned long long)j.blk, (unsigned long long)nblocks); return -1; }
            if (j.mask != 0u && j.mask != 0xFFu && j.mask != 0x80u && j.mask != 0x01u) { js_set_error("a mask the kernel has no store for"); return -1; }
            if (j.mask == 0xFFu && (j.dst0 & 7u)) { js_set_error("an 8-byte write off its boundary"); return -1; }
            if (out && !have) { int c[64]; for (int k = 0; k < 64; k++) c[k] = arena[j.blk * 64 + k]; idct_block(c, res); have = true; }
            for (uint32_t i = 0; i < 8; i++) if (j.mask >> i & 1u) {
                const uint32_t at = j.dst0 + i;
                if (at >= JS_REN_OFF_TILE) { js_set_error("a sample outside the planes"); return -1; }
                if (live[at]) { js_set_error("cell %u written twice in unit (%u, %u)", at, my, m0); return -1; }
                // own cells and halo cells, each where the header says
                const bool own_job = jb < nm * r.bpm;
                bool own_cell;
                if (at < JS_REN_OFF_C) own_cell = (at % JS_REN_Y_PITCH) < nm * 8u * r.H && at / JS_REN_Y_PITCH < 8u * r.V;
                else {
                    const uint32_t o = (at - JS_REN_OFF_C) % JS_REN_C_BYTES, lr = o / JS_REN_C_PITCH, x = o % JS_REN_C_PITCH;
                    if (x < 7u || x - 7u > nm * 8u + 1u) { js_set_error("a chroma sample outside its row"); return -1; }
                    own_cell = lr >= 1u && lr <= 8u && x - 7u >= 1u && x - 7u <= nm * 8u;
                }
                if (own_job != own_cell) { js_set_error("job %u of unit (%u, %u): own / halo mismatch at cell %u", jb, my, m0, at); return -1; }
                live[at] = 1; if (out) mem[at] = (uint8_t)js_ren_sample(res[r8 * 8 + i]);
            }
        }
    }
    // step 2, lane = four pixels
    const uint32_t mcu_w = 8u * r.H, mcu_h = 8u * r.V, x0 = m0 * mcu_w, y0 = my * mcu_h;
    const uint32_t wpix = nm * mcu_w < r.dim_x - x0 ? nm * mcu_w : r.dim_x - x0, hpix = mcu_h < r.dim_y - y0 ? mcu_h : r.dim_y - y0;
    const uint32_t dw = (r.dim_x + r.H - 1u) / r.H, dh = (r.dim_y + r.V - 1u) / r.V;
    for (uint32_t ly = 0; ly < hpix; ly++) for (uint32_t lx = 0; lx < wpix; lx += 4u) {
        const uint32_t n = wpix - lx < 4u ? wpix - lx : 4u;
        uint32_t cb[4] = { 128, 128, 128, 128 }, cr[4] = { 128, 128, 128, 128 };
        for (uint32_t j = 0; j < 4; j++) if (!live[ly * JS_REN_Y_PITCH + lx + j]) { js_set_error("a luma cell read that no job wrote"); return -1; }
        if (r.ncomp == 3u) {
            if (r.H == 1u) for (uint32_t j = 0; j < 4; j++) {
                const uint32_t at = (1u + ly) * JS_REN_C_PITCH + 8u + lx + j;
                if (!live[JS_REN_OFF_C + at] || !live[JS_REN_OFF_C + JS_REN_C_BYTES + at]) { js_set_error("a chroma cell read that no job wrote"); return -1; }
                cb[j] = mem[JS_REN_OFF_C + at]; cr[j] = mem[JS_REN_OFF_C + JS_REN_C_BYTES + at];
            } else {
                // the cells js_ren_chroma4 looks up: columns i0 - 1 .. i0 + 2, this row and its neighbour
                const uint32_t i0 = (x0 + lx) >> 1, y = y0 + ly; const int jrow = (int)(r.V == 2u ? y >> 1 : y);
                for (int kk = -1; kk <= 2; kk++) for (int far = 0; far < 2; far++) {
                    if (dw <= 2u && (kk < 0 || kk > 1 || far)) continue;
                    if (far && r.V == 1u) continue;
                    const uint32_t lc = js_ren_clamp_col((int)i0 + kk, dw, m0), lr = js_ren_clamp_row(far ? ((y & 1u) ? jrow + 1 : jrow - 1) : jrow, dh, my);
                    if (lc > nm * 8u + 1u || lr > 9u) { js_set_error("a chroma look-up outside the plane"); return -1; }
                    for (uint32_t c = 1; c <= 2; c++) if (!live[js_ren_c_cell(c, lr, lc)]) { js_set_error("unit (%u, %u): chroma cell (%u, %u) read at pixel (%u, %u), no job wrote it", my, m0, lr, lc, x0 + lx, y); return -1; }
                }
                js_ren_chroma4(mem + JS_REN_OFF_C, r.V, y, i0, dw, dh, my, m0, cb);
                js_ren_chroma4(mem + JS_REN_OFF_C + JS_REN_C_BYTES, r.V, y, i0, dw, dh, my, m0, cr);
            }
        }
        if (out) for (uint32_t j = 0; j < n; j++) {
            const uint32_t yv = mem[ly * JS_REN_Y_PITCH + lx + j], rgb = r.ncomp == 1u ? yv * 0x010101u : js_ren_rgb(yv, cb[j], cr[j]);
            uint8_t* o = out + ((size_t)(y0 + ly) * r.dim_x + x0 + lx + j) * 3u;
            o[0] = (uint8_t)rgb; o[1] = (uint8_t)(rgb >> 8); o[2] = (uint8_t)(rgb >> 16);
        }
    }
    return 0;
}

static int plan_one(const JsImage& im, JsRenRec* rec, uint32_t ub[2])
{
    JsnoopPackSpec s; js_pack_spec_defaults(&s);
    JsnoopPackDst d; memset(&d, 0, sizeof d); d.ptr = (void*)(uintptr_t)0x10000;
    return js_ren_plan(&im, 1, s, nullptr, 1, &d, rec, ub);
}

int main(int argc, char** argv)
{
    if (argc == 66 && !strcmp(argv[1], "block")) {
        int c[64]; int32_t o[64];
        for (int k = 0; k < 64; k++) c[k] = atoi(argv[2 + k]);
        idct_block(c, o);
        for (int k = 0; k < 64; k++) printf("%d ", o[k]);
        printf("\n");
        return 0;
    }
    if (argc == 9 && !strcmp(argv[1], "render")) {
        const uint32_t w = (uint32_t)atoi(argv[2]), h = (uint32_t)atoi(argv[3]), nc = (uint32_t)atoi(argv[4]), H = (uint32_t)atoi(argv[5]), V = (uint32_t)atoi(argv[6]);
        const int lay = nc == 1 ? 0 : (H == 1 ? 1 : (V == 1 ? 2 : 3));
        const JsImage im = image(w, h, lay);
        JsRenRec rec; uint32_t ub[2];
        CHECK(plan_one(im, &rec, ub) == 0);
        std::vector<int16_t> arena((size_t)im.total_blocks * 64);
        FILE* f = fopen(argv[7], "rb"); CHECK(f != nullptr);
        CHECK(fread(arena.data(), 2, arena.size(), f) == arena.size()); fclose(f);
        std::vector<uint8_t> out((size_t)w * h * 3, 0xEE);
        for (uint32_t u = 0; u < ub[1]; u++) CHECK(run_unit(rec, u / rec.runs, (u % rec.runs) * JS_REN_RUN, arena.data(), im.total_blocks, out.data()) == 0);
        f = fopen(argv[8], "wb"); CHECK(f != nullptr);
        CHECK(fwrite(out.data(), 1, out.size(), f) == out.size()); fclose(f);
        printf("ok\n");
        return 0;
    }
    // ---- renderable: the four layouts, and every refusal
    for (int lay = 0; lay < 4; lay++) { uint32_t H = 9, V = 9; CHECK(js_ren_renderable(image(33, 31, lay), 0, &H, &V) == 0 && H == (lay >= 2 ? 2u : 1u) && V == (lay == 3 ? 2u : 1u)); }
    { JsImage im = image(16, 16, 3); im.precision = 12; REFUSED(js_ren_renderable(im, 5), "image 5 has a sample precision of 12"); }
    { JsImage im = image(16, 16, 3); im.ncomp = 2; REFUSED(js_ren_renderable(im, 0), "2 components"); im.ncomp = 4; REFUSED(js_ren_renderable(im, 0), "4 components"); }
    { JsImage im = image(16, 16, 3); im.samp_h[1] = 1; im.samp_v[1] = 2; REFUSED(js_ren_renderable(im, 0), "luma sampling 1 x 2"); }               // 4:4:0
    { JsImage im = image(16, 16, 3); im.samp_h[1] = 4; im.samp_v[1] = 1; REFUSED(js_ren_renderable(im, 0), "luma sampling 4 x 1"); }               // 4:1:1
    { JsImage im = image(16, 16, 3); im.samp_h[2] = 2; REFUSED(js_ren_renderable(im, 0), "chroma sampling 2 x 1 / 1 x 1"); }
    { JsImage im = image(16, 16, 3); im.samp_v[3] = 2; REFUSED(js_ren_renderable(im, 0), "chroma sampling"); }
    { JsImage im = image(16, 16, 3); im.blk_per_mcu = 5; REFUSED(js_ren_renderable(im, 0), "blocks per MCU"); }
    { JsImage im = image(16, 16, 3); im.blk_comp[1] = 2; REFUSED(js_ren_renderable(im, 0), "block order"); im = image(16, 16, 3); im.blk_comp[5] = 2; REFUSED(js_ren_renderable(im, 0), "block order"); }
    { JsImage im = image(16, 16, 0); im.blk_per_mcu = 4; REFUSED(js_ren_renderable(im, 0), "one component"); }
    { JsImage im = image(16, 16, 2); im.dim_x = 0; REFUSED(js_ren_renderable(im, 0), "no decoded geometry"); }
    { JsImage im = image(16, 16, 2); im.mcu_xmax = 2; REFUSED(js_ren_renderable(im, 0), "MCU grid"); im = image(16, 16, 2); im.total_blocks++; REFUSED(js_ren_renderable(im, 0), "MCU grid"); }
    // ---- the call: every refusal of jsnoop_batch_pack, under this entry point's name
    {
        JsnoopPackSpec d, got; js_pack_spec_defaults(&d);
        REFUSED(js_pack_import_spec(nullptr, &got, "pack_ijg"), "pack_ijg: spec is NULL");
        { JsnoopPackSpec s = d; s.struct_size = 3; REFUSED(js_pack_import_spec(&s, &got, "pack_ijg"), "struct_size"); s.struct_size = sizeof s + 4; REFUSED(js_pack_import_spec(&s, &got, "pack_ijg"), "struct_size"); }
        { JsnoopPackSpec s = d; s.layout = 2; REFUSED(js_pack_import_spec(&s, &got, "pack_ijg"), "pack_ijg: unknown layout"); s = d; s.dtype = 2; REFUSED(js_pack_import_spec(&s, &got, "pack_ijg"), "pack_ijg: unknown dtype"); }
        JsImage imgs[3] = { image(17, 9, 3), image(5, 4, 0), image(16, 16, 3) };
        imgs[2].samp_h[1] = 1; imgs[2].samp_v[1] = 2;                                   // (not renderable)
        imgs[1].coef_off = 12;
        JsRenRec recs[3]; uint32_t ub[4]; JsnoopPackDst dst[3]; memset(dst, 0, sizeof dst);
        for (int k = 0; k < 3; k++) dst[k].ptr = (void*)(uintptr_t)(0x10000 + k);
        const int two[2] = { 1, 0 };
        CHECK(js_ren_plan(imgs, 3, d, two, 2, dst, recs, ub) == 0);
        CHECK(ub[0] == 0 && ub[1] == 1 && ub[2] == 2 && recs[0].ncomp == 1 && recs[0].bpm == 1 && recs[0].coef_off == 12 && recs[0].row_pitch == 15 && recs[0].plane_pitch == 60);
        CHECK(recs[1].H == 2 && recs[1].V == 2 && recs[1].bpm == 6 && recs[1].runs == 1 && recs[1].mcu_xmax == 2 && recs[1].row_pitch == 51 && recs[1].ptr == 0x10001);
        REFUSED(js_ren_plan(imgs, 3, d, nullptr, 3, dst, recs, ub), "image 2: luma sampling 1 x 2");
        const int bad[2] = { 0, 3 }; REFUSED(js_ren_plan(imgs, 3, d, bad, 2, dst, recs, ub), "image index 3 (entry 1) out of range");
        const int neg[1] = { -1 }; REFUSED(js_ren_plan(imgs, 3, d, neg, 1, dst, recs, ub), "out of range");
        { JsnoopPackDst x[2] = { dst[0], dst[1] }; x[1].ptr = nullptr; REFUSED(js_ren_plan(imgs, 3, d, two, 2, x, recs, ub), "destination 1 (image 0) is NULL"); }
        { JsnoopPackDst x[2] = { dst[0], dst[1] }; x[0].row_pitch = 14; REFUSED(js_ren_plan(imgs, 3, d, two, 2, x, recs, ub), "row_pitch 14"); x[0].row_pitch = 15; CHECK(js_ren_plan(imgs, 3, d, two, 2, x, recs, ub) == 0); }
        { JsnoopPackSpec s = d; s.layout = JSNOOP_PACK_CHW; JsnoopPackDst x[2] = { dst[0], dst[1] }; x[0].row_pitch = 8; x[0].plane_pitch = 31; REFUSED(js_ren_plan(imgs, 3, s, two, 2, x, recs, ub), "plane_pitch 31");
          x[0].plane_pitch = 32; CHECK(js_ren_plan(imgs, 3, s, two, 2, x, recs, ub) == 0 && recs[0].plane_pitch == 32 && recs[0].row_pitch == 8); }
        { JsnoopPackSpec s = d; s.dtype = JSNOOP_PACK_F32; REFUSED(js_ren_plan(imgs, 3, s, two, 2, dst, recs, ub), "multiples of 4");
          JsnoopPackDst x[2] = { dst[0], dst[1] }; x[0].ptr = (void*)(uintptr_t)0x10000; x[1].ptr = (void*)(uintptr_t)0x20000; x[1].row_pitch = 206; REFUSED(js_ren_plan(imgs, 3, s, two, 2, x, recs, ub), "multiples of 4");
          x[1].row_pitch = 208; CHECK(js_ren_plan(imgs, 3, s, two, 2, x, recs, ub) == 0 && recs[0].row_pitch == 60); }
        // 2^31 units: 65535 x 65535 grey images of 8192 x 1024 units each
        std::vector<JsImage> big(257, image(65535, 65535, 0)); std::vector<JsRenRec> brecs(big.size()); std::vector<uint32_t> bub(big.size() + 1); std::vector<JsnoopPackDst> bd(big.size(), dst[0]);
        REFUSED(js_ren_plan(big.data(), big.size(), d, nullptr, 257, bd.data(), brecs.data(), bub.data()), "2^31 units");
        CHECK(js_ren_plan(big.data(), big.size(), d, nullptr, 255, bd.data(), brecs.data(), bub.data()) == 0 && bub[255] == 255u * 8192u * 1024u);
    }
    // ---- the unit plan against a brute-force walk, and the job list of every unit: four layouts, edge sizes
    {
        const uint32_t sizes[][2] = { { 1, 1 }, { 2, 2 }, { 3, 3 }, { 4, 5 }, { 5, 4 }, { 8, 8 }, { 16, 16 }, { 17, 9 }, { 9, 17 }, { 33, 31 }, { 50, 70 }, { 130, 21 }, { 64, 48 }, { 6, 40 }, { 40, 6 },
                                      { 127, 16 }, { 128, 16 }, { 129, 17 }, { 112, 33 }, { 144, 48 }, { 448, 33 }, { 449, 47 }, { 65535, 3 }, { 3, 65535 }, { 65535, 33 }, { 17, 65535 } };
        for (int lay = 0; lay < 4; lay++) for (const auto& wh : sizes) {
            const JsImage im = image(wh[0], wh[1], lay);
            JsRenRec rec; uint32_t ub[2];
            CHECK(plan_one(im, &rec, ub) == 0);
            const uint32_t H = lay >= 2 ? 2 : 1, V = lay == 3 ? 2 : 1, mx = (wh[0] + 8 * H - 1) / (8 * H), my = (wh[1] + 8 * V - 1) / (8 * V);
            CHECK(rec.mcu_xmax == mx && rec.mcu_ymax == my && rec.bpm == (lay ? H * V + 2 : 1) && rec.H == H && rec.V == V && ub[0] == 0 && ub[1] == js_ren_units(im));
            // every MCU lies in exactly one unit; units follow each other in decode order, straddle no MCU row and hold at most JS_REN_RUN MCUs
            uint64_t next = 0;
            for (uint32_t u = 0; u < ub[1]; u++) {
                const uint32_t row = u / rec.runs, m0 = (u - row * rec.runs) * JS_REN_RUN;
                CHECK(row < my && m0 < mx);
                const uint32_t nm = mx - m0 < JS_REN_RUN ? mx - m0 : JS_REN_RUN;
                CHECK((uint64_t)row * mx + m0 == next && nm >= 1);
                next += nm;
                // (the long thin pictures: the first and last units of a row, the first two and last two rows)
                if (ub[1] > 4096 && !(u < 2 * rec.runs || u >= ub[1] - 2 * rec.runs || m0 < 2 * JS_REN_RUN || m0 + 2 * JS_REN_RUN >= mx)) continue;
                CHECK(run_unit(rec, row, m0, nullptr, im.total_blocks, nullptr) == 0);
            }
            CHECK(next == (uint64_t)mx * my);
        }
    }
    // ---- the transform: DC alone is flat, nothing is undefined on wild blocks (the sanitizers watch), results stay 32-bit clean
    {
        int c[64]; int32_t o[64];
        memset(c, 0, sizeof c); c[0] = 8 * 100; idct_block(c, o); for (int k = 0; k < 64; k++) CHECK(o[k] == 100);
        c[0] = -1024 * 8; idct_block(c, o); for (int k = 0; k < 64; k++) CHECK(o[k] == -1024 && js_ren_sample(o[k]) == 0);
        unsigned s = 12345; int32_t peak = 0;
        for (int it = 0; it < 2000; it++) {
            for (int k = 0; k < 64; k++) { s = s * 1664525u + 1013904223u; c[k] = it < 1000 ? (int)(s >> 16) - 32768 : ((s >> 20 & 1) ? 32767 : -32768); }
            idct_block(c, o);
            for (int k = 0; k < 64; k++) { CHECK(js_ren_sample(o[k]) <= 255u); if (abs(o[k]) > peak) peak = abs(o[k]); }
        }
        CHECK(peak < (1 << 14));
        CHECK(js_ren_sample(-129) == 0 && js_ren_sample(-128) == 0 && js_ren_sample(0) == 128 && js_ren_sample(127) == 255 && js_ren_sample(128) == 255 && js_ren_sample(8191) == 255 && js_ren_sample(-8192) == 0);
    }
    // ---- upsampling formulas at their corners, and the colour lines over all 2^24 (Y, Cb, Cr) against the contract written out once more
    {
        uint32_t e, o;
        js_ren_h2v1(0, 1, 2, &e, &o); CHECK(e == 1 && o == 1); js_ren_h2v1(255, 255, 255, &e, &o); CHECK(e == 255 && o == 255); js_ren_h2v1(2, 1, 0, &e, &o); CHECK(e == 1 && o == 1);
        js_ren_h2v1(0, 0, 2, &e, &o); CHECK(e == 0 && o == 1); js_ren_h2v1(1, 0, 1, &e, &o); CHECK(e == 0 && o == 0); js_ren_h2v1(3, 0, 2, &e, &o); CHECK(e == 1 && o == 1);
        CHECK(js_ren_h2v2_sum(255, 255) == 1020 && js_ren_h2v2_sum(1, 0) == 3);
        js_ren_h2v2(1020, 1020, 1020, &e, &o); CHECK(e == 255 && o == 255); js_ren_h2v2(0, 0, 9, &e, &o); CHECK(e == 0 && o == 1); js_ren_h2v2(8, 0, 8, &e, &o); CHECK(e == 1 && o == 0);
        for (int y = 0; y < 256; y++) for (int cb = 0; cb < 256; cb++) for (int cr = 0; cr < 256; cr++) {
            const long long b0 = cb - 128, r0 = cr - 128;
            long long R = y + ((91881 * r0 + 32768) >> 16), G = y + ((-22554 * b0 - 46802 * r0 + 32768) >> 16), B = y + ((116130 * b0 + 32768) >> 16);
            R = R < 0 ? 0 : R > 255 ? 255 : R; G = G < 0 ? 0 : G > 255 ? 255 : G; B = B < 0 ? 0 : B > 255 ? 255 : B;
            if (js_ren_rgb((uint32_t)y, (uint32_t)cb, (uint32_t)cr) != (uint32_t)(R | G << 8 | B << 16)) { printf("FAILED colour %d %d %d\n", y, cb, cr); return 1; }
        }
        CHECK(js_ren_rgb(128, 128, 128) == 0x808080u && js_ren_rgb(255, 128, 255) == 0xFFA4FFu);
    }
    // ---- struct sizes the records are copied with; the LDS layout
    CHECK(sizeof(JsRenRec) == 72 && sizeof(JsnoopPackSpec) == 40 && sizeof(JsnoopPackDst) == 24 && JS_REN_WAVE_BYTES == 5952 && JS_REN_MAX_JOBS == 92);
    printf("ok\n");
    return 0;
}
