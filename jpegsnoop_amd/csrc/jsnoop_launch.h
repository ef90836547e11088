// jsnoop_launch.h -- host-callable launch wrappers of the kernels in jsnoop_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "jsnoop_types.h"

void js_launch_entropy_exact(hipStream_t st, const JsImage* imgs, const uint32_t* sel, uint32_t nsel, const JsTableSet* tables,
                             const uint8_t* raw, int16_t* coef, int16_t* dccum, uint32_t* side, int side_only, uint32_t* events);
int  js_launch_idct_color(hipStream_t st, const JsImage* imgs, const uint32_t* wg_base, uint32_t nimg, uint32_t total_wgs, uint32_t tile_bytes,
                          const float* lut_t, const int16_t* coef, const int16_t* dccum, uint8_t* dib, int16_t* planes, uint32_t* side,
                          int layout /* 0 = mixed; 1..4 = every image has the fast layout with chroma expansion (2,2) / (2,1) / (1,2) / (1,1) */,
                          unsigned long long* wg_part /* null, or 2 words per workgroup (indexed like wg_base): brightest-pixel / luminance records folded by a second kernel */);
void js_launch_unaligned_probe(hipStream_t st, void* buf48);    // one 16-byte store at byte offset 6 of buf48 (halves 1..8), see k_unaligned_probe
void js_launch_idct_probe(hipStream_t st, const float* lut_t, const int16_t* coef64, float* out64);
void js_launch_clear3(hipStream_t st, void* a, size_t a_bytes, void* b, size_t b_bytes, void* c, size_t c_bytes, const JsImage* imgs = nullptr, uint32_t nimg = 0);   // three arenas to zero in one launch (sizes rounded up to 16 bytes)
void js_launch_clear5(hipStream_t st, uint32_t* a, size_t na, uint32_t* b, size_t nb, uint32_t* c, size_t nc, uint32_t* d, size_t nd, uint32_t* e, size_t ne);   // five word ranges to zero in one launch
void js_launch_dib_checksum(hipStream_t st, const JsImage* imgs, uint32_t nimg, const uint8_t* dib, unsigned long long* sums);
void js_launch_color_probe(hipStream_t st, int y, int cb, int cr, uint32_t* out);
void js_launch_bright_probe(hipStream_t st, const JsImage* imgs, uint32_t img, const uint32_t* side, const int16_t* planes /*or null*/, uint32_t* out8);   // chroma + BGRA of the brightest pixel, and the key they belong to
#define JS_STATS_WORDS 2482          /* public layout, include/jsnoop_gpu.h JSNOOP_STATS_WORDS */
#define JS_STATS_DEV_WORDS 2496      /* + the six uncapped YCC range-event totals, padded */
void js_launch_color_stats(hipStream_t st, const JsImage* imgs, uint32_t img, const int16_t* planes, int hist_en, uint32_t* stats);
void js_launch_clip_order(hipStream_t st, const JsImage* imgs, uint32_t img, const int16_t* planes, uint32_t budget, uint32_t* out6);
void js_launch_tiff_pack(hipStream_t st, const JsImage* imgs, uint32_t img, const uint8_t* dib, const int16_t* planes, int mode, uint8_t* out);
void js_launch_color_sweep(hipStream_t st, uint32_t* out /*2^24 words*/);
void js_launch_color_offsets_sweep(hipStream_t st, uint32_t* out /*2^24 words*/);
void js_launch_unstuff(hipStream_t st, int wl, const JsImage* imgs, const uint32_t* us_base, uint32_t nimg, uint32_t total_chunks, const uint8_t* raw,
                       uint32_t* chunk_keep, uint32_t* chunk_rst, uint8_t* ustr_lin, uint8_t* ustr, uint32_t* seg_tab, uint32_t* side, uint32_t* flags,
                       const uint32_t* sy_base, uint32_t sy_wgs, unsigned long long* us_state /*nullptr: the three-pass form*/, uint32_t epoch,
                       const uint32_t* us4_base /*prefix over super-chunks of four chunks, or nullptr: linear output + transposition pass*/, uint32_t total_super,
                       uint32_t* ticket /*device counter the fused passes take their chunk from*/, uint32_t* ticket_base /*host: its value before the launch; advanced here*/);
void js_launch_sync(hipStream_t st, int wl, uint32_t tab_rows, uint32_t tab_lut2, const JsImage* imgs, const uint32_t* sy_base, uint32_t nimg, uint32_t total_wgs, const JsTableSet* tables,
                    const uint8_t* ustr, const uint32_t* seg_tab, const uint32_t* side, uint32_t* sub, uint64_t nsub, int first_pass, uint32_t it_max = 0 /* rounds at most; 0: to the fixed point */);
// the large-job form of the synchronisation stage: k_sync cut after two rounds, list rounds (k_sync_links / k_sync_round), k_sync's verification mode
#define JS_SYR_SLOTS 12                /* list counters per image */
#define JS_SYR_ROUNDS 8                /* list rounds of a large job (k_sync alone needs 4.8 rounds per workgroup on average, 7 at most in 834 workgroups read) */
size_t js_sync_list_words(uint64_t nsub, uint32_t nimg);
void js_launch_sync_rounds(hipStream_t st, int wl, uint32_t tab_rows, uint32_t tab_lut2, const JsImage* imgs, const uint32_t* sn_base, uint32_t sn_wgs, const uint32_t* sy_base, uint32_t sy_wgs,
                           uint32_t nimg, const JsTableSet* tables, const uint8_t* ustr, const uint32_t* seg_tab, const uint32_t* side, uint32_t* sub, uint64_t nsub,
                           uint32_t* lists /* js_sync_list_words(nsub, images of the BATCH) words */, uint32_t* rcnt /* this part's counters inside it */, int rounds);
#define JS_SY_THREADS 256
#define JS_SY_HALO    2            // lanes of a k_sync workgroup that walk in front of its first sub-sequence
// Candidate synchronisation (the small-job form of the synchronisation stage: k_cand_spec / _walk / _chain / _fill / _apply); leaves the
// sub-sequence arrays as js_launch_sync would, open links marked for a js_launch_sync(..., first_pass = 2) behind it.
#define JS_CAND_MAX_BLK 6            /* images with more blocks per MCU than this synchronise the classic way */
#define JS_CAND_REQ_WORDS 12         /* per image: diagnostics of the chain */
size_t js_cand_bytes(uint64_t nsub);
void js_launch_cand_sync(hipStream_t st, int wl, uint32_t tab_rows, uint32_t tab_lut2, const JsImage* imgs, const uint32_t* sy_base, uint32_t nimg, uint32_t sy_wgs, uint32_t max_blk,
                         const JsTableSet* tables, const uint8_t* ustr, const uint32_t* seg_tab, const uint32_t* side, uint32_t* sub, uint64_t nsub, uint32_t* cand, uint32_t* req, int fill_rounds,
                         int mid /* the memo walks report middle states for a two-lanes-per-sub-sequence write pass (js_launch_write with the same arena) */);
void js_launch_block_scan(hipStream_t st, int wl, const JsImage* imgs, uint32_t nimg, const JsTableSet* tables, uint32_t* sub, uint64_t nsub, uint32_t* side, uint32_t* flags);
void js_launch_write(hipStream_t st, int wl, uint32_t tab_rows, uint32_t tab_lut2, const JsImage* imgs, const uint32_t* sy_base, uint32_t nimg, uint32_t total_wgs, const JsTableSet* tables,
                     const uint8_t* ustr, const uint32_t* seg_tab, uint32_t* side, uint32_t* sub, uint64_t nsub,
                     int16_t* coef, int16_t* dccum, uint8_t* mcu_rst, uint32_t* flags,
                     uint32_t* cand_half /* null, or the candidate arena of a job that was synchronised by candidates: two lanes per sub-sequence (64-byte pieces only) */, bool v1,
                     uint32_t* rec_pos = nullptr /* 64-byte pieces, !v1: the pass records MCU-top bit positions here and the code-length histogram in the side block (the side walk's outputs) */);
// DC-only fast form (every image decode_ac == 0, fast layout): the write pass without the coefficient arena, and the back end straight from cumulative DC to DIB
void js_launch_write_dc(hipStream_t st, int wl, uint32_t tab_rows, uint32_t tab_lut2, const JsImage* imgs, const uint32_t* sy_base, uint32_t nimg, uint32_t total_wgs, const JsTableSet* tables,
                        const uint8_t* ustr, const uint32_t* seg_tab, uint32_t* side, uint32_t* sub, uint64_t nsub, int16_t* dccum, uint8_t* mcu_rst, uint32_t* flags);
int  js_launch_dc_color(hipStream_t st, const JsImage* imgs, const uint32_t* wg_base, uint32_t nimg, uint32_t total_wgs,
                        const int16_t* dccum, uint8_t* dib, int16_t* planes, uint32_t* side, unsigned long long* wg_part);
// side-output pass over one image the parallel path decoded (MCU file map, block-DC maps, code-length histogram, status words)
void js_launch_side_pass(hipStream_t st, int wl, uint32_t tab_rows, uint32_t tab_lut2, const JsImage* imgs, const uint32_t* us_base, const uint32_t* sy_base, uint32_t nimg,
                         uint32_t img, uint32_t us_wg0, uint32_t us_wgs, uint32_t sy_wg0, uint32_t sy_wgs, const JsTableSet* tables, const uint8_t* raw,
                         const uint32_t* chunk_keep, const uint32_t* chunk_rst, const uint8_t* ustr, uint32_t* seg_tab, uint32_t* side, uint32_t* sub, uint64_t nsub,
                         const int16_t* dccum, uint8_t* mcu_rst, uint32_t* mcu_pos, uint32_t* us_out, uint32_t* events,
                         uint32_t* anoms, uint32_t dead_blk = 0xFFFFFFFFu, uint32_t cut_mcu = 0xFFFFFFFFu /* [0] count, 4 words per record from [4]: block, bit position of the symbol, index it ran to, bit position behind the block; or null */, bool walked = false /* the decode's write pass recorded positions + histogram: no side walk */);
// ... of every image whose byte of img_mask is set, in four launches (pos_all: rec_off-indexed positions, zeroed by the caller; us_all: 256 words per chunk of the batch)
void js_launch_side_pass_all(hipStream_t st, int wl, uint32_t tab_rows, uint32_t tab_lut2, const JsImage* imgs, const uint32_t* us_base, const uint32_t* sy_base, uint32_t nimg,
                             uint32_t us_wgs, uint32_t sy_wgs, const JsTableSet* tables, const uint8_t* raw, const uint32_t* chunk_keep, const uint32_t* chunk_rst, const uint8_t* ustr,
                             uint32_t* seg_tab, uint32_t* side, uint32_t* sub, uint64_t nsub, const int16_t* dccum, uint8_t* mcu_rst, uint32_t* pos_all, uint32_t* us_all,
                             uint32_t* events, const uint8_t* img_mask);
#define JS_DC_PARTS_IMAGES 8         /* batches of up to this many images take the two-level DC scan */
#define JS_DC_PARTS_BYTES (JS_DC_PARTS_IMAGES * 64 * 16)
void js_launch_dead_fill(hipStream_t st, const JsImage* imgs, uint32_t img, uint32_t bstar, uint32_t kind /*ANOM_KEY's death kinds 1..8*/,
                         const JsTableSet* tables, int16_t* coef, int16_t* dccum, uint8_t* mcu_rst);
void js_launch_dc_scan(hipStream_t st, const JsImage* imgs, uint32_t nimg, const JsTableSet* tables, int16_t* dccum, const uint8_t* mcu_rst, void* parts_scratch /*JS_DC_PARTS_BYTES or null*/);
#define JS_US_CHUNK 4096
#define JS_SC_HDR 145                 // words of a chunk record in front of its events (k_side_chunks)
void js_launch_side_chunks(hipStream_t st, const JsImage* imgs, uint32_t img, const JsTableSet* tables, const uint8_t* raw, const uint32_t* seg_tab, const uint8_t* mcu_rst,
                           const uint32_t* mcu_pos, const uint32_t* us_out, uint32_t us_threads, uint32_t* side, const int16_t* dccum, uint32_t ch_mcus, uint32_t nchunks, uint32_t ev_cap,
                           const uint32_t* mcus_left0, uint32_t* recs, uint32_t* map_own, unsigned long long* map_beyond, uint32_t run_on_mcu /*~0: none*/, uint32_t* fill_desc /*64 words, zeroed*/);
void js_launch_tail_pass(hipStream_t st, int wl, uint32_t tab_rows, uint32_t tab_lut2, const JsImage* imgs, const uint32_t* us_base, const uint32_t* sy_base, uint32_t nimg,
                         uint32_t us_wg0, uint32_t us_wgs, uint32_t sy_wg0, uint32_t sy_wgs, const JsTableSet* tables, const uint8_t* raw,
                         const uint32_t* chunk_keep, const uint32_t* chunk_rst, const uint8_t* ustr, uint32_t* seg_tab, uint32_t* side, uint32_t* sub, uint64_t nsub,
                         int16_t* coef, int16_t* dccum, uint8_t* mcu_rst, uint32_t* mcu_pos, uint32_t* us_out, const uint32_t* flags /*the batch's flag arena*/, const uint32_t* sel1 /*device: the image index*/);
// k_pack_rgb (jsnoop_pack.hip): DIBs of a decoded batch -> caller-owned device memory, cropped top-down three-channel pixels, ONE launch for the whole list.
// recs / unit_base: JsPackRec and its prefix table (jsnoop_types.h), both in device memory.  0, -1 on a launch error.
int  js_launch_pack_rgb(hipStream_t st, const JsImage* imgs, const uint8_t* dib, const JsPackRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                        int layout /*JSNOOP_PACK_HWC / _CHW*/, int dtype /*JSNOOP_PACK_U8 / _F32*/, const JsPackArgs& a);
// k_pack_resize (jsnoop_pack_resize.hip): a rectangle of every listed DIB resampled to its destination's size, ONE launch for the whole list.
// recs / unit_base: JsResizeRec and its prefix table (jsnoop_types.h), both in device memory.  0, -1 on a launch error or an unknown filter / layout / dtype.
int  js_launch_pack_resize(hipStream_t st, const JsImage* imgs, const uint8_t* dib, const JsResizeRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                           int filter /*JSNOOP_RESIZE_**/, int layout, int dtype, const JsPackArgs& a);
// k_pack_coefs (jsnoop_coef.hip): the coefficient arena of a decoded batch -> caller-owned device memory, one tensor per listed component, ONE launch for the whole list.
// recs / unit_base: JsCoefRec and its prefix table (jsnoop_types.h), both in device memory.  0, -1 on a launch error or an unknown layout / dtype / order.
int  js_launch_pack_coefs(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsCoefRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                          int layout /*JSNOOP_COEF_BLOCKS / _FREQ*/, int dtype /*JSNOOP_COEF_I16 / _F32*/, int order /*JSNOOP_COEF_NATURAL / _ZIGZAG*/);
// k_stats_batch / k_stats_order (jsnoop_stats.hip): the colour statistics of every listed row from the retained planes, TWO launches for the whole list.
// recs / unit_base: JsStatRec and its 64-bit prefix table (jsnoop_types.h), both in device memory; tot (JS_STATS_TOT_WORDS words per row) and rowcnt (one word
// per picture row of every listed row) are scratch the caller zeroed on `st`, as it zeroed the rows; totals_out: null, or [nrec][6].  0, -1 on a launch error.
int  js_launch_stats_batch(hipStream_t st, const int16_t* planes, const JsStatRec* recs, const uint64_t* unit_base, uint32_t nrec, uint64_t total_units, int hist_en,
                           uint32_t* tot, uint32_t* rowcnt, uint32_t* totals_out);
// k_coef_hist_init / k_coef_hist (jsnoop_coef_hist.hip): the rows of jsnoop_batch_pack_coef_hist initialised, then filled in ONE launch for the whole list.
// recs / unit_base: JsCoefHistRec and its 64-bit prefix table (jsnoop_types.h), both in device memory; row k at dst + k * pitch_words words.
// 0, -1 on a launch error or an unknown order / range.
int  js_launch_coef_hist(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsCoefHistRec* recs, const uint64_t* unit_base, uint32_t nrec, uint64_t total_units,
                         int order /*JSNOOP_COEF_NATURAL / _ZIGZAG*/, uint32_t range /*1 .. 127*/, void* dst, uint64_t pitch_words);
// k_pack_planes (jsnoop_planes.hip): the retained planes of a decoded batch -> caller-owned device memory, one tensor per listed component, ONE launch for the whole list.
// recs / unit_base: JsPlaneRec and its prefix table (jsnoop_types.h), both in device memory.  0, -1 on a launch error or an unknown dtype.
int  js_launch_pack_planes(hipStream_t st, const int16_t* planes, const JsPlaneRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                           int dtype /*JSNOOP_PLANE_I16 / _U8 / _F32*/, const JsPlaneArgs& a);
// jsnoop_batch_export_jpeg (jsnoop_export.hip), first phase: k_export_measure over every unit, then k_export_scan over the units of every entry.
// recs / unit_base / tabs (JS_EXPORT_TAB_WORDS words: length << 16 | code by symbol, DC0 DC1 AC0 AC1) in device memory; blk_bits: one uint16 per listed block;
// unit_bits / unit_off: one entry per unit; res: [nrec] result words, then [nrec][2] lowest offending block (zeroed / set to all ones by the caller);
// ent_bits: bits of every entry.  0, -1 on a launch error.
#define JS_EXPORT_TAB_WORDS 544u
int  js_launch_export_measure(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                              const uint32_t* tabs, uint16_t* blk_bits, uint32_t* unit_bits, uint64_t* unit_off, uint32_t* res, uint64_t* ent_bits);
// ... second phase, the records now with live / bits / u_off / out_off: k_export_bits into the zeroed un-stuffed streams, k_export_ffcount, k_export_scan over the
// chunks of every entry, k_export_stuff into the files (hdrs: the headers the host built; len: one word per entry, zeroed by the caller).
int  js_launch_export_write(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const uint32_t* unit_base, const uint32_t* chunk_base, uint32_t nrec,
                            uint32_t total_units, uint32_t total_chunks, const uint32_t* tabs, const uint16_t* blk_bits, const uint64_t* unit_off, uint8_t* ustream,
                            uint32_t* chunk_ff, uint64_t* chunk_off, uint64_t* ent_ff, const uint8_t* hdrs, uint8_t* out, uint64_t* len);
// jsnoop_batch_export_jpeg_coded with JSNOOP_HUFFMAN_OPTIMAL, first phase: k_export_symbols over every unit (the symbol counts of every entry into stats[k].freq,
// zeroed by the caller), k_export_huff, one workgroup per entry (T.81 K.2 per slot: stats[k].slot, the entry's JS_EXPORT_TAB_WORDS code words at
// tabs + k * JS_EXPORT_TAB_WORDS, its header -- the host's bytes up to SOF, the built DHT segments, the host's SOS -- in JS_EXPORT_OPT_HDR bytes at
// hdr_out + k * JS_EXPORT_OPT_HDR and its length in hdr_len[k]; an entry without a unit gets length 0), then k_export_measure with the entry's own tables and
// k_export_scan.  0, -1 on a launch error.
int  js_launch_export_measure_opt(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const JsExportOptRec* orecs, const uint32_t* unit_base,
                                  uint32_t nrec, uint32_t total_units, const uint32_t* annex_tabs, const uint8_t* hdrs, JsExportOptStat* stats, uint32_t* tabs, uint8_t* hdr_out,
                                  uint32_t* hdr_len, uint16_t* blk_bits, uint32_t* unit_bits, uint64_t* unit_off, uint32_t* res, uint64_t* ent_bits);
// ... second phase: js_launch_export_write with every entry's own code tables (tabs + k * JS_EXPORT_TAB_WORDS)
int  js_launch_export_write_opt(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const uint32_t* unit_base, const uint32_t* chunk_base, uint32_t nrec,
                                uint32_t total_units, uint32_t total_chunks, const uint32_t* tabs, const uint16_t* blk_bits, const uint64_t* unit_off, uint8_t* ustream,
                                uint32_t* chunk_ff, uint64_t* chunk_off, uint64_t* ent_ff, const uint8_t* hdrs, uint8_t* out, uint64_t* len);
// jsnoop_batch_export_jpeg_rst (restart intervals): both phases with the restart forms of the kernels -- k_export_symbols / k_export_measure / k_export_bits with the DC
// predecessor reset at every interval start, k_export_rst_scan (positions from run summaries: an interval starts on a byte), k_export_stuff_rst (markers between the
// intervals).  rrecs: the side records; unit_sum: one JsRstSum per unit; itab: the call's interval tables (filled by k_export_bits, read by k_export_stuff_rst).
// orecs == NULL: the Annex K tables (annex_tabs), else every entry's own, built as in js_launch_export_measure_opt.  tabs / tab_stride of the second phase: the one set
// and 0, or the entries' own and JS_EXPORT_TAB_WORDS.
int  js_launch_export_measure_rst(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const JsExportOptRec* orecs, const JsExportRstRec* rrecs,
                                  const uint32_t* unit_base, uint32_t nrec, uint32_t total_units, const uint32_t* annex_tabs, const uint8_t* hdrs, JsExportOptStat* stats, uint32_t* tabs,
                                  uint8_t* hdr_out, uint32_t* hdr_len, uint16_t* blk_bits, JsRstSum* unit_sum, uint64_t* unit_off, uint32_t* res, uint64_t* ent_bits);
int  js_launch_export_write_rst(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const JsExportRstRec* rrecs, const uint32_t* unit_base,
                                const uint32_t* chunk_base, uint32_t nrec, uint32_t total_units, uint32_t total_chunks, const uint32_t* tabs, uint32_t tab_stride, const uint16_t* blk_bits,
                                const uint64_t* unit_off, uint64_t* itab, uint8_t* ustream, uint32_t* chunk_ff, uint64_t* chunk_off, uint64_t* ent_ff, const uint8_t* hdrs, uint8_t* out, uint64_t* len);
// jsnoop_batch_export_jpeg_prog (progressive files; jsnoop_export_prog.hip): a record per (entry, scan) of the coded entries (srecs, nrec of them; rec_base: the
// entries' prefix table over them, tile_base / chunk_base: theirs over tiles of JS_EXPORT_TILE units / chunks of the scans' un-stuffed streams).  First phase:
// k_prog_classify, k_prog_runs (the carried end-of-band run of every unit), k_prog_symbols, k_prog_huff (stats, zeroed by the caller; the scans' code words at
// tabs + i * JS_PROG_TAB_WORDS, header pieces at hdr_out + i * JS_PROG_HDR, their lengths), k_prog_measure, k_export_rst_scan over the tiles of every record.
// Second phase: k_prog_bits into the zeroed streams, k_prog_ffcount, k_export_scan, k_prog_place (scan_out: where a scan's piece starts in its file; len: zeroed
// by the caller), k_prog_stuff.  0, -1 on a launch error.  js_launch_export_scan / _rst_scan: the two scan kernels of jsnoop_export.hip over any prefix table.
int  js_launch_export_scan(hipStream_t st, const uint32_t* cnt, uint64_t* off, const uint32_t* base, uint32_t nrec, uint64_t* total);
int  js_launch_export_rst_scan(hipStream_t st, const JsRstSum* sum, uint64_t* off, const uint32_t* base, uint32_t nrec, uint64_t* total);
int  js_launch_export_prog_measure(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const JsExportScanRec* srecs, const uint32_t* tile_base, uint32_t nent,
                                   uint32_t nrec, uint32_t tiles, const uint8_t* hdrs, JsExportScanStat* stats, uint32_t* tabs, uint8_t* hdr_out, uint32_t* hdr_len, uint8_t* cls, uint16_t* eob,
                                   uint16_t* blk_bits, JsRstSum* tile_sum, uint64_t* tile_off, uint32_t* res, uint64_t* rec_bits);
int  js_launch_export_prog_write(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsExportRec* recs, const JsExportScanRec* srecs, const uint32_t* rec_base, const uint32_t* tile_base,
                                 const uint32_t* chunk_base, uint32_t nent, uint32_t nrec, uint32_t tiles, uint32_t chunks, const uint32_t* tabs, const uint16_t* eob, const uint16_t* blk_bits,
                                 const uint64_t* tile_off, uint64_t* itab, uint8_t* ustream, uint32_t* chunk_ff, uint64_t* chunk_off, uint64_t* rec_ff, const uint8_t* hdrs,
                                 const uint32_t* hdr_len, uint64_t* scan_out, uint8_t* out, uint64_t* len);
// jsnoop_encode_run (jsnoop_encode.hip): k_encode over every unit of the call's records (JsEncRec; unit_base: their prefix table over runs of JS_ENC_RUN MCUs; tabs:
// the call's two tables and their reciprocals) into the arena and the cumulative DC.  One launch, no scratch.  0, -1 on a launch error.
int  js_launch_encode(hipStream_t st, const JsEncRec* recs, const uint32_t* unit_base, const JsEncTabs* tabs, uint32_t nrec, uint32_t total_units, int16_t* coef, int16_t* dccum);
// jsnoop_transform_run (jsnoop_transform.hip): k_transform over every unit of the call's records (JsXfRec; unit_base: their prefix table over runs of JS_XF_RUN
// destination blocks; flags: what the call's op comes to, JS_XF_*) from the source batch's arena and cumulative DC into the object's.  One launch, no scratch.
// 0, -1 on a launch error.
int  js_launch_transform(hipStream_t st, const JsXfRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units, uint32_t flags,
                         const int16_t* src_coef, const int16_t* src_dccum, int16_t* coef, int16_t* dccum);
// jsnoop_carve_run (jsnoop_carve.hip), first phase: k_carve_count over every tile of the blob, then k_carve_scan.  base: the 16-byte boundary at or below the blob,
// head: the bytes between the two, n: the blob's length; counts: 4 * tiles + 4 words (per tile terminators and candidates, then their exclusive prefix sums, then
// the two totals as 64-bit words).  0, -1 on a launch error.
int  js_launch_carve_count(hipStream_t st, const uint8_t* base, uint32_t head, uint64_t n, uint32_t tiles, uint32_t* counts);
// ... second phase: k_carve_emit writes the two ascending position lists, k_carve_walk one 64-byte record per candidate.
int  js_launch_carve_walk(hipStream_t st, const uint8_t* base, uint32_t head, uint64_t n, uint32_t tiles, const uint32_t* counts, uint32_t nterm, uint32_t ncand,
                          uint32_t max_markers, uint32_t* term, uint32_t* cand, uint32_t* recs);
// k_render_ijg (jsnoop_render.hip): the coefficient arena of a decoded batch rendered as libjpeg's pixels -> caller-owned device memory, jsnoop_batch_pack's store
// forms, ONE launch for the whole list.  recs / unit_base: JsRenRec and its prefix table (jsnoop_render_check.h), both in device memory.  0, -1 on a launch error
// or an unknown layout / dtype.
struct JsRenRec;
int  js_launch_render_ijg(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsRenRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                          int layout /*JSNOOP_PACK_HWC / _CHW*/, int dtype /*JSNOOP_PACK_U8 / _F32*/, const JsPackArgs& a);
// k_render_ijg_scaled (jsnoop_render_scaled.hip): ... as libjpeg's reduced-size pixels (1/2, 1/4, 1/8; the scale is in the records), the same store forms, ONE launch
// for the whole list.  recs / unit_base: JsRsRec and its prefix table (jsnoop_render_scaled_check.h), both in device memory.  0, -1 on a launch error or an unknown
// layout / dtype.
struct JsRsRec;
int  js_launch_render_ijg_scaled(hipStream_t st, const int16_t* coef, const int16_t* dccum, const JsRsRec* recs, const uint32_t* unit_base, uint32_t nrec, uint32_t total_units,
                                 int layout /*JSNOOP_PACK_HWC / _CHW*/, int dtype /*JSNOOP_PACK_U8 / _F32*/, const JsPackArgs& a);
