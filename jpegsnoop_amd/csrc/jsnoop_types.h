// jsnoop_types.h -- device-visible descriptors shared by the host code and the HIP kernels.
//
// HBM layout of one batch (all arenas are single hipMalloc blocks; offsets are per image):
//
//   raw    u8   file bytes of every image, 16-byte aligned starts     (read once by the entropy front end)
//   ustr   u8   un-stuffed entropy segment of every image (FF00->FF, RSTn removed) + interval table
//   coef   i16  [total_blocks][64] dequantised coefficients, NATURAL order, blocks in decode order
//               (mcu * blocks_per_mcu + block_in_mcu); slot 0 = dequantised DC difference
//   dccum  i16  [total_blocks] cumulative (predicted) DC per block = CimgDecode's m_nDcLum/Cb/Cr at that block
//   dib    u8   [img_y][img_x][4] bottom-up BGRA per image                (written once)
//   planes i16  3 x [blk_ymax*8][blk_xmax*8] per image (optional; m_pPixValY/Cb/Cr)
//   side   u32  per image: MCU file map, block-DC maps, Huffman histogram, status words
//
// Names follow the reference (MCU, block, restart interval, DIB), see SURVEY.md section 8.
#pragma once
#include <stdint.h>

#define JS_MAX_BLK_PER_MCU 48      // 3 components x (4 x 4) sampling factors (MAX_SAMP_FACT_H/V, ImgDecode.h:79-80)
#define JS_DHT_CODES       260     // MAX_DHT_CODES, ImgDecode.h:68
#define JS_FAST_BITS       9       // DHT_FAST_SIZE, ImgDecode.h:96
#define JS_CODE_UNUSED     0xFFFFFFFFu
#define JS_L1_BITS         9       // first-level index width of the parallel path's decode tables (1 KiB rows: four workgroups of the write pass fit a CU)
#define JS_LUT2_MAX        2048    // second-level entries (all tables together) in the parallel path's LUT form
#define JS_MAX_DEVICES     64      // devices one process may drive (per-device state of the launch wrappers)
#define JS_SUBSEQ_BYTES    128     // bytes of un-stuffed stream per sub-sequence (parallel entropy path)

// One distinct set of Huffman + quantisation tables, resolved per scan component
// (index t = (comp-1)*2 + class, class 0 = DC, 1 = AC).  De-duplicated across a batch.
struct JsTableSet {
    // --- exact-mirror form: the arrays CimgDecode::SetDhtEntry fills (ImgDecode.cpp:748-820)
    uint32_t fast[6][1 << JS_FAST_BITS];    // m_anDhtLookupfast: (len<<8)+code, 0xFFFFFFFF = miss
    uint32_t size[6];                       // m_anDhtLookupSize
    uint32_t bitlen[6][JS_DHT_CODES], bits[6][JS_DHT_CODES], mask[6][JS_DHT_CODES], code[6][JS_DHT_CODES];
    uint32_t dest_id[6];                    // DHT destination id behind each slot (histogram index)
    uint16_t qzz[3][64];                    // m_anDqtCoeffZz of the table selected for each component
    // --- parallel-path form: JS_L1_BITS-bit first level + second level for the longer codes (a few % of symbols).
    //     Identical tables share one row (Cb and Cr normally do): slot_row[slot] says which.
    //     entry: bit15 = 0 : [12:8] = code length (0 = invalid), [7:0] = symbol (run<<4 | size)
    //            bit15 = 1 : [14:12] = extra index bits nb (1..5), [11:0] = base into lut2
    uint16_t lut1[6][1 << JS_L1_BITS];
    uint16_t lut2[JS_LUT2_MAX];
    // --- state-only form for the synchronisation walks (k_sync needs positions and coefficient indices, not values): one entry
    //     covers the symbol at the window AND, for AC rows, the next one when its code also lies inside the JS_L1_BITS window.
    //     byte 0 = bits of symbol 1 (code + value), byte 1 = its advance of the coefficient index (DC rows: 1; EOB: 64, which ends
    //     the block from any index), byte 2 = bits of both symbols (0 = no second symbol described), byte 3 = index advance of both
    //     (a second symbol that is EOB adds 64).  Bit 31 = escape: the code is longer than the window, [14:12] extra index bits and
    //     [11:0] base of its second level (as in lut1), whose entries (lut2p, parallel to lut2) are single-symbol entries of the
    //     same form; bits 31 and 30: no code starts with these bits.
    uint32_t lutp[6][1 << JS_L1_BITS];
    uint32_t lut2p[JS_LUT2_MAX];
    // --- value form for the write pass (DC tables: single-symbol entries, [3:0] code length, [7:4] size): the symbol at the window and, when its
    //     code is visible in the same window, the AC symbol behind it -- [3:0] code length, [7:4] size, [11:8] run of symbol 1,
    //     [15:12] / [19:16] / [23:20] the same of symbol 2, [24] a second symbol is described.  Bit 31 = escape as in lutp.
    uint32_t lutw[6][1 << JS_L1_BITS];
    uint32_t row_sub[6];                    // index of a lut1 row among the rows of its class (DC tables / AC tables)
    uint32_t n_dc_rows, n_ac_rows;
    uint32_t slot_row[6];                   // row of lut1 holding the table of slot (comp-1)*2 + class
    uint32_t n_rows, lut2_used;
    uint32_t lut_ok;                        // 1 when every table fits the LUT form and is a canonical prefix code
};

struct JsImage {
    // frame / scan description (SetImageDetails :590, SetSofSampFactors :619, SetPrecision :564)
    uint32_t dim_x, dim_y, ncomp, precision, rst_en, rst_interval, decode_ac, want_planes;
    // geometry (DecodeScanImg :2831-2872)
    uint32_t mcu_w, mcu_h, mcu_xmax, mcu_ymax, blk_xmax, blk_ymax, img_x, img_y;
    uint32_t samp_h[4], samp_v[4], expand_h[4], expand_v[4];       // index 1..3 = Y, Cb, Cr
    uint32_t blk_per_mcu, total_blocks;
    uint8_t  blk_comp[JS_MAX_BLK_PER_MCU], blk_ch[JS_MAX_BLK_PER_MCU], blk_cv[JS_MAX_BLK_PER_MCU];
    // inputs
    uint64_t file_off;  uint32_t file_len, scan_start, scan_len;    // scan_len = bytes up to the terminating marker
    uint64_t ustr_off;  uint32_t ustr_cap;                          // un-stuffed stream capacity (= scan_len + slack)
    uint32_t tableset;
    // outputs
    uint64_t coef_off;      // in blocks
    uint64_t dib_off;       // in bytes
    uint64_t plane_off;     // in samples (3 planes of blk_xmax*8 x blk_ymax*8 follow each other)
    uint64_t side_off;      // in u32 words, see JS_SIDE_*
    uint64_t subseq_off;    // first sub-sequence slot of this image
    uint32_t n_subseq;      // capacity in sub-sequences
    uint64_t seg_off;       // first entry of this image's restart-interval table (u32 start bytes + end sentinel)
    uint32_t seg_cap;       // entries available
    uint64_t mcu_off;       // first byte of this image's per-MCU restart flags
    // preview controls (SetPreviewMode :633, SetPreviewYccOffset :650)
    uint32_t preview_mode; int32_t shift_y, shift_cb, shift_cr; uint32_t shift_mcu_x, shift_mcu_y;
    uint32_t err_max;
    // event log of the exact-mirror reader (what the reference writes to CDocLog while it decodes); 0 capacity = off
    uint64_t ev_off; uint32_t ev_cap;
    uint32_t rec_off;       // first word of this image's MCU-top positions in an arena that holds every image's (number of MCUs + 2 each; the batched side pass)
};

// Event records (6 u32 each, preceded by one count word per image): what the reference logs during the scan decode.
#define JS_ANOM_MAX 1024           // coefficient-index overflows the side pass records per image (beyond that: the mirror's side-only pass)
#define JS_EV_WORDS 6
#define JS_EV_MAX   1024
enum { JS_EV_OVERREAD_BEFORE = 1, JS_EV_OVERREAD_CODE, JS_EV_OVERREAD_BITS, JS_EV_CANT_FIND, JS_EV_RST_INDEX, JS_EV_MARKER,
       JS_EV_BAD_MARKER, JS_EV_BAD_HUFF, JS_EV_NUMCOEF, JS_EV_BAD_SCAN_MCU, JS_EV_RST_NOT_DETECTED };

// Per-image side block (u32 words, in this order):
//   [0..15]   status: 0 scan_bad, 1 scan_end, 2 #RST read, 3 num_pixels, 4 pos0, 5 align, 6 warn_bad, 7 first,
//             8 flags (JSNOOP_FLAG_*), 9 path, 10 un-stuffed length, 11 #intervals,
//             12-13 brightest-pixel key (64-bit: Y+32768 high, ~raster index low), 14 blocks decoded, 15 sum of final Y
//   [16..151] Huffman code-length histogram [2][4][17]
//   [152..]   MCU file map [mcu_ymax*mcu_xmax], then three block-DC maps (i16 packed as u16 pairs, each
//             padded to a whole word count), sized by the image
#define JS_SIDE_STATUS 0
#define JS_SIDE_HISTO  16
#define JS_SIDE_MCUMAP 152

// Layouts the back end converts without a replicated LDS tile (k_idct_color, mcu_to_dib_fast): three components, Y un-expanded,
// Cb and Cr one block each and both expanded eh x ev with eh, ev in {1, 2} (4:4:4, 4:2:2, 4:4:0, 4:2:0), default preview, no YCC shift.
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline bool js_fast_layout(const JsImage& im)
{
    const uint32_t eh = im.expand_h[2], ev = im.expand_v[2];
    return im.ncomp == 3 && im.preview_mode == 1 && (im.shift_y | im.shift_cb | im.shift_cr) == 0 &&
           im.expand_h[1] == 1 && im.expand_v[1] == 1 && im.samp_h[1] == eh && im.samp_v[1] == ev &&
           im.samp_h[2] == 1 && im.samp_v[2] == 1 && im.samp_h[3] == 1 && im.samp_v[3] == 1 && im.expand_h[3] == eh && im.expand_v[3] == ev &&
           eh >= 1 && eh <= 2 && ev >= 1 && ev <= 2;
}
// ... whose blocks come in the order k_dc_color computes with: luma block (ch, cv) is number cv * eh + ch of the MCU, Cb and Cr follow
static inline bool js_dc_fast_order(const JsImage& im)
{
    const uint32_t eh = im.expand_h[2], ev = im.expand_v[2];
    if (!js_fast_layout(im) || im.blk_per_mcu != eh * ev + 2u) return false;
    for (uint32_t cv = 0; cv < ev; cv++) for (uint32_t ch = 0; ch < eh; ch++) {
        const uint32_t j = cv * eh + ch;
        if (im.blk_comp[j] != 1 || im.blk_ch[j] != ch || im.blk_cv[j] != cv) return false;
    }
    return im.blk_comp[eh * ev] == 2 && im.blk_comp[eh * ev + 1u] == 3;
}
// bytes of the back end's per-wave LDS tile for this image: Y plane + two bare chroma blocks (fast layouts), else three replicated planes
static inline uint32_t js_tile_bytes(const JsImage& im)
{
    const uint32_t b = js_fast_layout(im) ? im.mcu_h * (im.mcu_w + 8u) * 2u + 256u : 3u * im.mcu_h * (im.mcu_w + 8u) * 2u;
    return (b + 15u) & ~15u;
}

static inline __host__ __device__ uint32_t js_side_words(uint32_t nmcu, uint32_t nblk) { return JS_SIDE_MCUMAP + nmcu + 3 * ((nblk + 1) / 2); }

// jsnoop_batch_pack (k_pack_rgb): one record per listed image, and a prefix table unit_base[nrec + 1] over the records in which image k owns
// dim_y * ceil(dim_x / JS_PACK_SEG) units -- a unit is one segment of one output row, the work of one wave at a time.
#define JS_PACK_SEG 512u             /* pixels per unit: two 16-byte loads per lane */
struct JsPackRec  { uint32_t img, reserved; uint64_t ptr, row_pitch, plane_pitch; };   // destination of image `img`; pitches in bytes, resolved (never 0)
struct JsPackArgs { int32_t bgr; float scale[3], bias[3]; };

// jsnoop_batch_pack_resized (k_pack_resize, jsnoop_pack_resize.hip): one record per listed destination, resolved like JsPackRec's (pitches never 0, the ROI
// never empty), and a prefix table in which destination k owns out_h * ceil(out_w / JS_RESIZE_SEG) units -- a unit is one segment of one OUTPUT row.
#define JS_RESIZE_SEG   256u         /* output pixels per unit: four per lane, the store shapes of the plain pack */
#define JS_RESIZE_CHUNK 1024u        /* AREA: source pixels of one row a wave stages in LDS at a time (4 KiB per wave) */
struct JsResizeRec { uint32_t img, out_w, out_h, roi_x, roi_y, roi_w, roi_h, reserved; uint64_t ptr, row_pitch, plane_pitch; };

// jsnoop_batch_pack_coefs (k_pack_coefs, jsnoop_coef.hip): one record per listed destination -- one component of one image, everything the kernel needs of it
// resolved on the host -- and a prefix table in which destination k owns bh * ceil(bw / JS_COEF_TILE) units: a unit is a run of up to JS_COEF_TILE blocks,
// consecutive in bx, of one row of the component's block grid -- the work of one wave at a time.  Block (bx, by) of the component is block
// coef_off + ((by / sv) * mcu_xmax + bx / sh) * bpm + first + (by % sv) * sh + bx % sh of the arena.
#define JS_COEF_TILE 64u             /* blocks per unit: eight 16-byte loads per lane; one frequency of a full tile is 128 contiguous int16 bytes */
struct JsCoefRec { uint64_t ptr, row_pitch, plane_pitch, coef_off; uint32_t bw, bh, sh, sv, first, bpm, mcu_xmax, tiles; };   // pitches in bytes, resolved (never 0); tiles = ceil(bw / JS_COEF_TILE)
// jsnoop_batch_pack_stats (k_stats_batch / k_stats_order, jsnoop_stats.hip): one record per listed row -- one image, everything the kernels need of it resolved
// on the host -- and a 64-bit prefix table in which row k owns img_y * ceil(img_x / JS_STATS_UNIT) units: a unit is a run of up to JS_STATS_UNIT pixels of one
// row of the MCU-padded picture, the work of one wave at a time (a lane owns eight consecutive samples).  row_base: the row's first word in the per-call
// arena of range-event counts per picture row.
#define JS_STATS_UNIT 512u           /* pixels per unit: one 16-byte load per lane and plane */
#define JS_STATS_TOT_WORDS 8u        /* per listed row in scratch: the six range-event totals, padded */
struct JsStatRec { uint64_t dst, plane_off, psz, row_base; uint32_t img_x, img_y, pw, ncomp, mcu_w, mcu_h, across, shift_ind; int32_t shift_y, shift_cb, shift_cr; uint32_t tiles; };
// jsnoop_batch_pack_coef_hist (k_coef_hist, jsnoop_coef_hist.hip): one record per listed row -- one component of one image, everything the kernel needs of it
// resolved on the host -- and a 64-bit prefix table in which row k owns ceil(nblk / JS_COEF_HIST_UNIT) units: a unit is a run of up to JS_COEF_HIST_UNIT of
// the component's blocks in ARENA order (a histogram does not care about raster order), the work of one wave at a time.  Block n of the component is block
// coef_off + (n / hv) * bpm + first + n % hv of the arena; hv_magic = 65536 / hv + 1 divides the small sums the kernel meets (below 96) by hv exactly.
// recip[k]: the reciprocal (js_chist_recip, jsnoop_coef_bin.h) of the divisor of natural index k -- the DQT entry, or 1 where the row holds dequantised values.
#define JS_COEF_HIST_UNIT 64u        /* blocks per unit: eight 16-byte loads per lane */
#define JS_COEF_HIST_WAVES 8u        /* waves of a workgroup: they share one histogram in LDS and deal the units of a share among themselves */
#define JS_COEF_HIST_WG_PER_CU 2u    /* workgroups per compute unit: sixteen waves, four a SIMD at 128 VGPRs; two histograms of up to 65 280 bytes fit the 160 KiB of LDS */
struct JsCoefHistRec { uint64_t dst, coef_off; uint32_t nblk, hv, first, bpm, hv_magic, pad0, pad1, pad2; uint32_t recip[64]; };
// jsnoop_batch_pack_planes (k_pack_planes, jsnoop_planes.hip): one record per listed destination -- one component of one image, everything the kernel needs of it
// resolved on the host -- and a prefix table in which destination k owns h * ceil(w / JS_PLANE_SEG) units: a unit is a segment of up to JS_PLANE_SEG elements of
// one OUTPUT row, the work of one wave at a time (a lane owns eight consecutive elements).  Output element (x, y) is sample src_off + (y * ev) * pw + x * eh of
// the plane arena; FULL is eh = ev = 1 with w x h = dim_x x dim_y.  xlim = the first source column the kernel must not read (dim_x).
#define JS_PLANE_SEG 512u            /* output elements per unit: one (eh = 1) or two (eh = 2) 16-byte loads per lane */
struct JsPlaneRec { uint64_t ptr, row_pitch, src_off; uint32_t pw, w, h, eh, ev, xlim, comp, segs; };   // row_pitch in bytes, resolved (never 0); src_off in samples; segs = ceil(w / JS_PLANE_SEG)
struct JsPlaneArgs { float scale[3], bias[3]; };
// jsnoop_batch_export_jpeg (k_export_*, jsnoop_export.hip): one record per listed entry -- one image, everything the kernels need of it resolved on the host --
// and prefix tables over the entries: unit_base (a unit is a tile of up to JS_EXPORT_TILE blocks of the image, consecutive in the arena, the work of one
// workgroup; an entry that is not encoded owns none) and, in the second phase, chunk_base (a chunk is JS_EXPORT_CHUNK bytes of the entry's un-stuffed stream).
// comp[j] / back[j]: the component of block j of an MCU, and how many blocks back the block of the same component before it lies (in the MCU, or the
// component's last block of the MCU before); q: the multipliers by component, natural order.  Phase 2 fills live, bits, u_off, out_off, out_cap.
#define JS_EXPORT_TILE   256u        /* public: JSNOOP_EXPORT_TILE */
#define JS_EXPORT_SCAN   256u        /* public: JSNOOP_EXPORT_SCAN */
#define JS_EXPORT_CHUNK  4096u       /* public: JSNOOP_EXPORT_CHUNK */
#define JS_EXPORT_WINDOW 8192u       /* public: JSNOOP_EXPORT_WINDOW */
struct JsExportRec { uint64_t coef_off, blk_base, bits, u_off, out_off, out_cap; uint32_t nblk, bpm, hdr_off, hdr_len, live, ncomp;
                     uint8_t comp[JS_MAX_BLK_PER_MCU], back[JS_MAX_BLK_PER_MCU]; uint16_t q[3][64]; };
// jsnoop_batch_export_jpeg_coded with JSNOOP_HUFFMAN_OPTIMAL (k_export_symbols, k_export_huff): a side record per entry beside JsExportRec -- how the header the
// host built splits around its DHT segments: [0, pre_len) ends behind SOF, [sos_off, sos_off + sos_len) is SOS; nslots: 2 (grey) or 4 tables -- and what the
// device keeps per entry: the symbol counts (laid out like the code tables: DC0[16] DC1[16] AC0[256] AC1[256]) and, per slot (2 * table id + class), the
// table it built (counts per length 1..16, symbols in code order, zero behind nsym).  The device assembles the entry's header in JS_EXPORT_OPT_HDR bytes of
// its own: 438 bytes up to SOF at most, four DHT segments of at most 21 + 16 / 21 + 256 bytes (every counter of an uncodable entry), SOS 14.
#define JS_EXPORT_OPT_HDR 1280u
#define JS_EXPORT_OPT_MAX_BLOCKS (1u << 26)      /* at most 63 counts a block: uint32 counters hold below this many blocks */
struct JsExportOptRec { uint32_t pre_len, sos_off, sos_len, nslots; };
struct JsExportOptSlot { uint32_t nsym; uint8_t counts[16]; uint8_t syms[256]; };
struct JsExportOptStat { uint32_t freq[544]; JsExportOptSlot slot[4]; };
// jsnoop_batch_export_jpeg_rst (restart intervals in the written files; arithmetic: jsnoop_export_rst_check.h): a side record per entry beside JsExportRec.
// ri_blocks: the entry's restart interval in BLOCKS (Ri x blocks per MCU; 0: the entry is written without restart markers, one interval), ni: its intervals,
// itab_off: where its interval table lies in the call's table (one uint64 per interval: the interval's end in bytes of the un-stuffed stream, in which every
// interval is padded to a whole byte and no marker stands).
struct JsExportRstRec { uint64_t itab_off; uint32_t ri_blocks, ni; };
// The summary of a run of blocks under that rule: has -- an interval ends inside the run; head -- the bits in front of the first such end (all bits where has
// is 0); mid -- whole bytes between the first and the last end; tail -- the bits behind the last end.  js_rst_combine (jsnoop_export_rst_check.h) is associative.
struct JsRstSum { uint32_t has, head, mid, tail; };
// jsnoop_batch_export_jpeg_prog (progressive files; arithmetic: jsnoop_export_prog_check.h, kernels: jsnoop_export_prog.hip): one record per (entry, scan) of the
// entries that are coded, beside the entry's JsExportRec (which holds the arena's place and the multipliers).  A unit is one block of the scan in the scan's own
// order; unit u is arena block (u / spm) * bpm + pos[u % spm] of the entry in an interleaved scan (and in every scan of a one-component image: spm = bpm = 1),
// and block (bx, by) = (u % w, u / w) of the component's coded part in a one-component scan of a three-component image (single = 1):
// ((by / V) * mcu_x + bx / H) * bpm + base + (by % V) * H + bx % H.  back[p]: how many units back the unit of the same component before position p lies.
// kind: JS_PROG_DC_FIRST / _DC_REFINE / _AC_FIRST; ri: the scan's restart interval in UNITS (0: one interval), ni its intervals; ubase: the scan's first unit in
// the call's per-unit arrays; ntab tables (a DC first scan: one per scan component, slot = position in the scan; an AC scan: one); the scan's header piece is
// pre (hdrs + pre_off, pre_len bytes: the file up to SOF2 for the first scan, else nothing), the DHT segments the device builds, post (DRI where Ri changes, SOS).
// Phase 2 fills live, bits (the scan's un-stuffed stream: every interval padded), u_off.
#define JS_PROG_DC_FIRST  0u
#define JS_PROG_DC_REFINE 1u
#define JS_PROG_AC_FIRST  2u
#define JS_PROG_TAB_WORDS 304u       /* DC slot 0..2 [16] each, AC [256] */
#define JS_PROG_HDR       768u       /* a scan's header piece on the device: 438 up to SOF at most, 3 x (21 + 16) or 21 + 256 of DHT, DRI 6, SOS 14 */
#define JS_PROG_POST      32u
struct JsExportScanRec { uint64_t ubase, itab_off, bits, u_off; uint32_t entry, scan, nunits, ri, ni, kind, ss, se, al, single, w, H, V, mcu_x, bpm, base, spm, ntab,
                    pre_off, pre_len, post_off, post_len, live, comp0;
                    uint8_t pos[JS_MAX_BLK_PER_MCU], comp[JS_MAX_BLK_PER_MCU], slot[JS_MAX_BLK_PER_MCU], back[JS_MAX_BLK_PER_MCU]; };
struct JsExportScanStat { uint32_t freq[JS_PROG_TAB_WORDS]; JsExportOptSlot slot[3]; };
// The summaries of the two segmented scans that resolve end-of-band runs (operators and proofs: jsnoop_export_prog_check.h).
struct JsRunFwd { uint32_t cnt, cut, tail; };    // units behind the last cut (all where cut is 0); a cut lies inside; the last cut was a block with symbols whose band ends in zeros
struct JsRunBwd { uint32_t lead, open; };        // empty units from the front up to the first stop; no stop inside
// jsnoop_encode_run (k_encode, jsnoop_encode.hip; arithmetic: jsnoop_encode_check.h): one record per source picture, everything the kernel needs of it resolved on
// the host, and a prefix table in which picture k owns mcu_ymax * runs units -- a unit is a run of up to JS_ENC_RUN consecutive MCUs of one MCU row, the work
// of one wave at a time (runs = ceil(mcu_xmax / JS_ENC_RUN); a unit straddles neither a picture nor an MCU row, and an MCU never spans units).  Sample (x, y) of
// channel c (0, 1, 2 = R, G, B; a grey picture has channel 0 alone) is the byte at base[c] + y * row_step + x * px_step: the host has folded layout, channel
// order, plane pitch and the bottom-up flag into the three addresses and the signed row step.  sub: 0 = 4:4:4 (and grey), 1 = 4:2:2, 2 = 4:2:0.
// JsEncTabs: the call's two tables (0 luma, 1 chroma), natural order, and per entry the reciprocal js_enc_recip(q) the quantiser multiplies by.
#define JS_ENC_RUN 8u                /* public: JSNOOP_ENCODE_RUN */
struct JsEncRec  { uint64_t base[3]; int64_t row_step; uint64_t coef_off; uint32_t px_step, width, height, ncomp, sub, mcu_xmax, mcu_ymax, runs, bpm, reserved; };
struct JsEncTabs { uint32_t recip[2][64]; uint16_t q[2][64]; };
// jsnoop_transform_run (k_transform, jsnoop_transform.hip; geometry, block map and plan: jsnoop_transform_check.h): one record per entry that is written --
// everything the kernel needs of it resolved on the host -- and a prefix table in which entry k owns ceil(nblk / JS_XF_RUN) units: a unit is a run of up to
// JS_XF_RUN consecutive DESTINATION blocks (decode order of the new geometry), the work of one wave at a time.  An op maps MCUs onto MCUs: the region is rw x rh
// MCUs of the layout the entry works in (the source's; 8 x 8 single blocks under grayscale), its origin (ox, oy) counted in such MCUs, and block kb of a
// destination MCU is block tab[kb] of the source MCU it comes from.  Under grayscale a working MCU is one of the gsh x gsv blocks component 0 has in a source MCU
// (gsh = gsv = 1 otherwise).  m_*: the divisions by the destination's blocks per MCU and MCUs per row and by gsh and gsv as multiply-high words (js_xf_magic).
// What the op comes to is call-wide (JS_XF_* flag bits).
#define JS_XF_RUN 8u                 /* public: JSNOOP_TRANSFORM_RUN */
#define JS_XF_T     1u               /* the 8 x 8 cells and the block grid are transposed */
#define JS_XF_REVX  2u               /* the source's x axis is reversed */
#define JS_XF_REVY  4u               /* the source's y axis is reversed */
#define JS_XF_NEGU  8u               /* destination cells of odd u change sign */
#define JS_XF_NEGV 16u               /* destination cells of odd v change sign */
struct JsXfDiv  { uint32_t mul, shift; };                        // mul 0: the divisor is 1
struct JsXfRec  { uint64_t src_off, dst_off; uint32_t nblk, s_mcu_x, s_bpm, d_mcu_x, d_bpm, rw, rh, ox, oy, gsh, gsv, reserved; JsXfDiv m_bpm, m_mcu_x, m_gsh, m_gsv;
                  uint8_t tab[JS_MAX_BLK_PER_MCU]; };
// zig-zag position of natural index k: the inverse of JS_ZIGZAG_NATURAL below
#define JS_ZIGZAG_POSITION { 0, 1, 5, 6,14,15,27,28,  2, 4, 7,13,16,26,29,42,  3, 8,12,17,25,30,41,43,  9,11,18,24,31,40,44,53, \
                            10,19,23,32,39,45,52,54, 20,22,33,38,46,51,55,60, 21,34,37,47,50,56,59,61, 35,36,48,49,57,58,62,63 }
// natural index of zig-zag position z (T.81 Figure A.6)
#define JS_ZIGZAG_NATURAL { 0, 1, 8,16, 9, 2, 3,10, 17,24,32,25,18,11, 4, 5, 12,19,26,33,40,48,41,34, 27,20,13, 6, 7,14,21,28, \
                           35,42,49,56,57,50,43,36, 29,22,15,23,30,37,44,51, 58,59,52,45,38,31,39,46, 53,60,61,54,47,55,62,63 }
