/* jsnoop_gpu.h -- C ABI of libjsnoop_gpu.so, the MI355X-native scan-decode stage.
 *
 * This is the drop-in boundary for the reference's scan decoder.  The reference
 * has no FFI; its boundary is the public C++ method set of `CimgDecode`
 * (reference source/ImgDecode.h:286-356,384-385,407-425) as driven by
 * `CjfifDecode` and re-exported by `CJPEGsnoopCore::I_*` (source/JPEGsnoopCore.h:79-117).
 * One `JsnoopDecoder` handle == one `CimgDecode` object; each entry point cites the
 * method it replaces.  All pointers are plain host or device addresses, no C++ or
 * torch types cross this line.  INTEGRATION.md shows the `CimgDecode`-shaped C++
 * wrapper (jpegsnoop_amd/csrc/ImgDecodeGpu.h) a reference maintainer would bind.
 *
 * Threading: like the reference (single-threaded, non-re-entrant objects,
 * source/JPEGsnoopCore.cpp:46) a handle may be used from one host thread at a
 * time; different handles are independent.  Work is issued on the handle's own HIP
 * stream (or the caller's, see jsnoop_batch_create).
 *
 * Errors: setters return 0 / 1 like the reference's bool setters; decode entry
 * points return void like DecodeScanImg and report through jsnoop_is_preview_ready,
 * the status words and the log callback (the reference's CDocLog sink).  If the HIP
 * runtime or device is unavailable, jsnoop_create returns NULL and
 * jsnoop_last_error() says why -- there is no CPU fallback in this library.
 */
#ifndef JSNOOP_GPU_H
#define JSNOOP_GPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define JSNOOP_ABI_VERSION 1

typedef struct JsnoopDecoder JsnoopDecoder;
typedef struct JsnoopBatch   JsnoopBatch;

/* ---- library / device ------------------------------------------------------ */
int         jsnoop_abi_version(void);
/* Host-only self test (no device needed): `rounds` random canonical Huffman table sets through the builders of the parallel
 * path's decode tables (two-level tables, state-only pair entries of the sync pass, value-pair entries of the write pass), every
 * first-level window checked against a plain search through the code list.  Returns the number of disagreements (0 = pass). */
int         jsnoop_selftest_tables(unsigned seed, unsigned rounds);
/* Host-only self test: the marker searches of the staging code (scan end, next FF: sixteen bytes per step) against byte-at-a-time loops on
 * `rounds` random buffers dense in FF / 00 / RSTn / other markers, every alignment.  Returns the number of disagreements (0 = pass). */
int         jsnoop_selftest_bytes(unsigned seed, unsigned rounds);
const char* jsnoop_last_error(void);                /* thread-local text of the last failure      */
int         jsnoop_device_count(void);              /* number of visible HIP devices (0 = none)   */
int         jsnoop_set_device(int device);          /* device used by objects created afterwards  */

/* log sink: replaces CDocLog::AddLine / AddLineWarn / AddLineErr (source/DocLog.cpp:102-194).
 * level: 0 = info, 1 = warning, 2 = error.  NULL disables logging (default). */
typedef void (*jsnoop_log_fn)(void* user, int level, const char* text);

/* ---- lifecycle: CimgDecode ctor :142, dtor :239, Reset :49, ResetState :286 ---- */
JsnoopDecoder* jsnoop_create(void);
void           jsnoop_destroy(JsnoopDecoder*);
void           jsnoop_reset(JsnoopDecoder*);
void           jsnoop_reset_state(JsnoopDecoder*);
/* the two halves of ResetState the class also has on their own: ResetDqtTables :343 (table selection, coefficients, number of SOF components)
 * and ResetDhtLookup :373 (code lists, fast look-up, table selection, the code-length histogram)                                          */
void           jsnoop_reset_dqt_tables(JsnoopDecoder*);
void           jsnoop_reset_dht_lookup(JsnoopDecoder*);
void           jsnoop_set_log_callback(JsnoopDecoder*, jsnoop_log_fn fn, void* user);

/* ---- options: the CSnoopConfig fields read at ImgDecode.cpp:2730-2741 ---------
 * decode_ac = bDecodeScanImgAc ("Full IDCT"), histo_en = bHistoEn,
 * stat_clip_en = bStatClipEn, err_max = nErrMaxDecodeScan.                      */
void jsnoop_set_options(JsnoopDecoder*, int decode_ac, int histo_en, int stat_clip_en, unsigned err_max);

/* ---- tables (SetDqtEntry :424, SetDqtTables :505, GetDqtEntry :466, SetDhtEntry :748,
 *      SetDhtSize :834, SetDhtTables :536) -- same argument meaning and range checks */
int      jsnoop_set_dqt_entry(JsnoopDecoder*, unsigned tbl_dest_id, unsigned coeff_ind, unsigned coeff_ind_zz, unsigned value);
int      jsnoop_set_dqt_tables(JsnoopDecoder*, unsigned comp_ind, unsigned tbl);
unsigned jsnoop_get_dqt_entry(JsnoopDecoder*, unsigned tbl_dest_id, unsigned coeff_ind);
int      jsnoop_set_dht_entry(JsnoopDecoder*, unsigned dest_id, unsigned cls, unsigned ind, unsigned len,
                              unsigned bits_left_just, unsigned mask_left_just, unsigned code);
int      jsnoop_set_dht_size(JsnoopDecoder*, unsigned dest_id, unsigned cls, unsigned size);
int      jsnoop_set_dht_tables(JsnoopDecoder*, unsigned comp_ind, unsigned tbl_dc, unsigned tbl_ac);

/* ---- geometry (SetSofSampFactors :619, SetPrecision :564, SetImageDetails :590) */
void jsnoop_set_sof_samp_factors(JsnoopDecoder*, unsigned comp_ind, unsigned samp_h, unsigned samp_v);
void jsnoop_set_precision(JsnoopDecoder*, unsigned precision);
void jsnoop_set_image_details(JsnoopDecoder*, unsigned dim_x, unsigned dim_y, unsigned comps_sof, unsigned comps_sos,
                              int rst_en, unsigned rst_interval);

/* SetImageDimensions :2706 (the PSD path's way of sizing the preview, source/JfifDecode.cpp:7374): the base rectangle of the preview, which
 * DecodeScanImg sets to the MCU-rounded image size itself (:2874).  jsnoop_get_image_dimensions reads it back.                            */
void jsnoop_set_image_dimensions(JsnoopDecoder*, unsigned width, unsigned height);
void jsnoop_get_image_dimensions(JsnoopDecoder*, unsigned* width, unsigned* height);
/* The public members CjfifDecode pokes when the preview does NOT come from the scan decoder (source/ImgDecode.h:508-510, used at
 * source/JfifDecode.cpp:7369-7373: a Photoshop file's image decoded into m_pDibTemp): jsnoop_dib_temp_create is m_pDibTemp.Kill() +
 * CreateDIB(width, height, 32) + GetDIBBitArray() -- a zeroed bottom-up BGRA buffer owned by the decoder that the caller fills and
 * jsnoop_get_bitmap_ptr then hands out (GetBitmapPtr :4940 returns m_pDibTemp's bits whatever filled them) --, the two setters are the
 * members m_bDibTempReady and m_bPreviewIsJpeg (IsPreviewReady :3753 returns the latter).  Reset() drops the buffer (:80-83).             */
uint8_t* jsnoop_dib_temp_create(JsnoopDecoder*, unsigned width, unsigned height);
void     jsnoop_set_dib_temp_ready(JsnoopDecoder*, int ready);
int      jsnoop_get_dib_temp_ready(JsnoopDecoder*);
void     jsnoop_set_preview_is_jpeg(JsnoopDecoder*, int is_jpeg);

/* ---- minimal JFIF front end: walks SOI/DQT/SOF0-1/DHT/DRI up to the first SOS and
 *      issues the setter calls above exactly as CjfifDecode::DecodeMarker does (source/JfifDecode.cpp:3581,
 *      :3600, :4648, :5008-5025, :5161, :5291).  On success *scan_start is the nStart to pass to
 *      jsnoop_decode_scan_img.  Returns 0, or -1 with jsnoop_last_error() (e.g. SOF2: the reference
 *      refuses progressive files, :4827-4833).                                                    */
int  jsnoop_jfif_walk(JsnoopDecoder*, const uint8_t* file, size_t len, unsigned* scan_start);

/* ---- decode: DecodeScanImg(nStart,bDisplay,bQuiet) :2723 ------------------------
 * `file`/`len` is the whole file image that the reference reads through
 * CwindowBuf::Buf (source/WindowBuf.cpp:639; bytes past `len` read as 0).  The bytes are
 * staged through pinned host memory with hipMemcpyAsync, with the overlays installed through
 * jsnoop_overlay_install applied to the staged copy.  Blocks until the DIB is resident in HBM. */
void jsnoop_decode_scan_img(JsnoopDecoder*, const uint8_t* file, size_t len, unsigned start, int display, int quiet);

/* ---- results: IsPreviewReady :3753, GetImageSize :4929, GetBitmapPtr :4940,
 *      GetPixMapPtrs :4913, LookupFilePosMcu :5020, LookupFilePosPix :5001, LookupBlkYCC :5037.
 * Host pointers are owned by the decoder and stay valid until the next
 * Reset / DecodeScanImg / destroy (same ownership rule as the reference); they are
 * filled by a D2H copy on first request.  The *_dev variants return the HBM copies. */
int            jsnoop_is_preview_ready(JsnoopDecoder*);
void           jsnoop_get_image_size(JsnoopDecoder*, unsigned* x, unsigned* y);
const uint8_t* jsnoop_get_bitmap_ptr(JsnoopDecoder*);
const void*    jsnoop_get_bitmap_dev(JsnoopDecoder*);
void           jsnoop_get_pixmap_ptrs(JsnoopDecoder*, const int16_t** y, const int16_t** cb, const int16_t** cr);
void           jsnoop_lookup_file_pos_mcu(JsnoopDecoder*, unsigned mcu_x, unsigned mcu_y, unsigned* byte, unsigned* bit);
void           jsnoop_lookup_file_pos_pix(JsnoopDecoder*, unsigned pix_x, unsigned pix_y, unsigned* byte, unsigned* bit);
void           jsnoop_lookup_blk_ycc(JsnoopDecoder*, unsigned blk_x, unsigned blk_y, int* y, int* cb, int* cr);

/* PixelToMcu :5056, PixelToBlk :5071, McuXyToLinear :5088 (the hover / status-bar helpers of source/JPEGsnoopViewImg.cpp:294-334) */
void     jsnoop_pixel_to_mcu(JsnoopDecoder*, unsigned pix_x, unsigned pix_y, unsigned* mcu_x, unsigned* mcu_y);
void     jsnoop_pixel_to_blk(JsnoopDecoder*, unsigned pix_x, unsigned pix_y, unsigned* blk_x, unsigned* blk_y);
unsigned jsnoop_mcu_xy_to_linear(JsnoopDecoder*, unsigned mcu_x, unsigned mcu_y);

/* bDumpHistoY (CSnoopConfig, read at ImgDecode.cpp:2730): with bHistoEn and bDisplay the decode log ends with
 * ReportHistogramY's 256 lines of the 2048-bin Y histogram (:3740-3741, :3845-3868).                          */
void jsnoop_set_dump_histo_y(JsnoopDecoder*, int on);

/* ---- byte overlays: CwindowBuf::OverlayInstall / OverlayRemoveAll / OverlayGet / OverlayGetNum
 *      (source/WindowBuf.cpp:516-620).  The reference's fault-injection tool: Buf() (:639-660) returns an overlay's
 *      byte instead of the file's wherever an enabled overlay covers the offset, the LAST installed one winning.
 *      jsnoop_decode_scan_img applies the installed overlays to its staged copy of the file image (offsets inside the
 *      file), so a re-decode after an install shows the patched stream exactly as the reference's would.
 *      At most 500 overlays of fewer than 500 bytes (NUM_OVERLAYS / MAX_OVERLAY, WindowBuf.h:42-43).           */
int      jsnoop_overlay_install(JsnoopDecoder*, const uint8_t* data, unsigned len, unsigned begin);   /* 1 = installed, 0 = refused */
void     jsnoop_overlay_remove_all(JsnoopDecoder*);
unsigned jsnoop_overlay_get_num(JsnoopDecoder*);
int      jsnoop_overlay_get(JsnoopDecoder*, unsigned ind, const uint8_t** data, unsigned* len, unsigned* begin);

/* ---- preview re-render on the retained planes: SetPreviewMode :633,
 *      SetPreviewYccOffset :650 (each re-runs the colour kernel only)            */
void     jsnoop_set_preview_mode(JsnoopDecoder*, unsigned mode);
unsigned jsnoop_get_preview_mode(JsnoopDecoder*);
void     jsnoop_set_preview_ycc_offset(JsnoopDecoder*, unsigned mcu_x, unsigned mcu_y, int y, int cb, int cr);
void     jsnoop_get_preview_ycc_offset(JsnoopDecoder*, unsigned* mcu_x, unsigned* mcu_y, int* y, int* cb, int* cr);   /* :670 */
/* SetPreviewMcuInsert :682 / GetPreviewMcuInsert :693 ("UNUSED" in the reference: stored, triggers a re-render, no pixel effect) */
void     jsnoop_set_preview_mcu_insert(JsnoopDecoder*, unsigned mcu_x, unsigned mcu_y, int len);
void     jsnoop_get_preview_mcu_insert(JsnoopDecoder*, unsigned* mcu_x, unsigned* mcu_y, unsigned* len);

/* ---- Progressive (SOF2) files -- beyond the reference, which refuses them (source/JfifDecode.cpp:4827-4833; the two
 *      entry points above refuse them the same way).  Walks ALL scans of the file (spectral selection and successive
 *      approximation, T.81 Annex G; tables may change between scans), decodes every restart interval of every scan as an
 *      independent lane, and hands the coefficient arena to the same back end as the baseline path, so a progressive
 *      file carrying the coefficients of a baseline file yields that file's DIB.  Results through the getters above
 *      (jsnoop_last_path() == 3; no MCU file map / block-DC maps).  Returns the number of scans, or -1.            */
int jsnoop_decode_progressive(JsnoopDecoder*, const uint8_t* file, size_t len);

/* ---- Export to TIFF (CJPEGsnoopDoc::OnToolsExporttiff, source/JPEGsnoopDoc.cpp:2008-2190, FileTiff::WriteFile
 *      source/FileTiff.cpp:436): mode 0 = RGB 8 bit, 1 = RGB 16 bit, 2 = YCC 8 bit (three-component images); byte-identical
 *      to the reference's file.  The pixel strip is arranged on the device.  0 on success, -1 + jsnoop_last_error().  */
int jsnoop_export_tiff(JsnoopDecoder*, const char* path, int mode);

/* ---- decoder internals that the reference keeps in public/inspectable members and
 *      that the log / hover UI consume (side outputs).
 *      Layouts match oracle/ref_shim/ref_driver.cpp so the same parity script runs
 *      against reference, oracle and this library.                                  */
void            jsnoop_get_geometry(JsnoopDecoder*, unsigned* out8);   /* McuW,McuH,McuXMax,McuYMax,BlkXMax,BlkYMax,ImgSizeX,ImgSizeY */
const uint32_t* jsnoop_mcu_file_map(JsnoopDecoder*);                   /* m_pMcuFileMap [McuYMax][McuXMax], PackFileOffset :5104 */
void            jsnoop_blk_dc_ptrs(JsnoopDecoder*, const int16_t** y, const int16_t** cb, const int16_t** cr);
const uint32_t* jsnoop_dht_histo(JsnoopDecoder*);                      /* m_anDhtHisto [2][4][17] */
void            jsnoop_scan_status(JsnoopDecoder*, unsigned* out8);    /* scan_bad, scan_end, #RST, num_pixels, pos0, align, warn_bad, first */
void            jsnoop_bright_avg(JsnoopDecoder*, int* out10);         /* brightest pixel + average Y (:4722-4730, :4802-4819) */
/* Statistics of the bHistoEn / bStatClipEn colour path (ConvertYCCtoRGB :4229, CapYccRange :4341, CapRgbRange :4495;
 * enable with jsnoop_set_options before DecodeScanImg).  As in the reference they are cleared by DecodeScanImg
 * (:3145-3155) and accumulated by every CalcChannelPreview, i.e. also by the preview re-renders below.  Layout,
 * JSNOOP_STATS_WORDS 32-bit words: [0..35] PixelCcHisto (ImgDecode.h:238-279: min,max,sum as int for PreclipY/Cb/Cr,
 * ClipY/Cb/Cr, ClipR/G/B, PreclipR/G/B), [36] nCount, [37..49] PixelCcClip (ImgDecode.h:220-234), [50..433]
 * m_anCcHisto_r/g/b[128], [434..2481] m_anHistoYFull[2048].                                                      */
#define JSNOOP_STATS_WORDS 2482
void            jsnoop_get_color_stats(JsnoopDecoder*, uint32_t* out);
const float*    jsnoop_idct_lut(JsnoopDecoder*);                       /* m_afIdctLookup [64][64] as uploaded to the device */
const uint32_t* jsnoop_dht_lookupfast(JsnoopDecoder*);                 /* m_anDhtLookupfast [2][4][1024] */
void            jsnoop_idct_block(JsnoopDecoder*, const int16_t* coef64, float* out64);   /* one block through the device IDCT */
/* every (Y, Cb, Cr) in [-128,127]^3 through the device ConvertYCCtoRGBFastFloat (ImgDecode.cpp:4086):
 * out_bgra[(Y+128)<<16 | (Cb+128)<<8 | (Cr+128)] = B | G<<8 | R<<16; 2^24 words; 0 on success */
int             jsnoop_color_sweep(JsnoopDecoder*, uint32_t* out_bgra);
/* the same sweep, same layout, through the offset form the 4:2:0 back end converts with (one evaluation per chroma
 * sample, a pixel = saturating adds, the listed exceptions of jsnoop_color_exc.h applied) */
int             jsnoop_color_offsets_sweep(JsnoopDecoder*, uint32_t* out_bgra);
/* which device path decoded the last image: 1 = parallel (self-synchronising) entropy
 * decode, 2 = sequential exact-mirror entropy kernel (taken for streams the parallel
 * path flags as malformed), 0 = nothing decoded */
int             jsnoop_last_path(JsnoopDecoder*);
uint32_t        jsnoop_last_flags(JsnoopDecoder*);                     /* JSNOOP_FLAG_* raised by the parallel path */
/* who produced the side outputs (MCU file map, histogram, status words, messages: what GetPixMapPtrs / LookupFilePosMcu and the log of
 * DecodeScanImg, ImgDecode.cpp:2723, show) of the last image: 0 = not asked for yet, 1 = the parallel side pass, 2 = the sequential
 * exact-mirror reader, 3 = the parallel side pass plus exact readers on chunks of a few MCUs (flagged files, in milliseconds) */
int             jsnoop_last_side_mode(JsnoopDecoder*);

#define JSNOOP_FLAG_BAD_CODE      0x0001u  /* no Huffman code matches (alone: decoded the reference's way by the parallel path) */
#define JSNOOP_FLAG_OVERRUN       0x0002u  /* code or extra bits run past the interval / scan end       */
#define JSNOOP_FLAG_COEF_OVERFLOW 0x0004u  /* coefficient index > 63                                    */
#define JSNOOP_FLAG_RST_MISALIGN  0x0008u  /* RSTn not on an MCU boundary (alone: followed the reference's way) */
#define JSNOOP_FLAG_SHORT         0x0010u  /* entropy data ends before all MCUs are decoded             */
#define JSNOOP_FLAG_TABLES        0x0020u  /* tables not expressible in the parallel path's LUT form    */
#define JSNOOP_FLAG_MARKER        0x0040u  /* non-RST marker or FFFF inside the scan                    */
#define JSNOOP_FLAG_NOSYNC        0x0080u  /* sub-sequence chain failed to converge                     */
#define JSNOOP_FLAG_BAD_EDGE      0x0100u  /* an anomaly whose outcome depends on the reader's look-ahead: mirror */
#define JSNOOP_FLAG_FORCED        0x8000u  /* caller forced the exact path                              */

/* ---- batch submit: N files -> N DIBs, all resident in HBM --------------------------
 * The batched analogue of CJPEGsnoopCore::DoBatchFileProcess (source/JPEGsnoopCore.cpp:765),
 * whose per-file semantics are preserved: every image is decoded exactly as a fresh
 * CimgDecode would.  `stream` is a hipStream_t (NULL = the batch creates its own).  */
JsnoopBatch* jsnoop_batch_create(void* stream);
void         jsnoop_batch_destroy(JsnoopBatch*);
void         jsnoop_batch_clear(JsnoopBatch*);
void         jsnoop_batch_set_options(JsnoopBatch*, int decode_ac, int want_planes, int force_exact_path);
/* Adds one image using the table/geometry state currently held by `tables`
 * (i.e. after the SetDqt/SetDht/SetSof/SetImageDetails calls of its header).
 * The file bytes are copied into the batch's pinned staging arena.
 * Returns the image index, or -1 with jsnoop_last_error() set.                      */
int          jsnoop_batch_add(JsnoopBatch*, const JsnoopDecoder* tables, const uint8_t* file, size_t len, unsigned scan_start);
/* Adds one JPEG file image, walking its header with the built-in minimal JFIF front
 * end (the subset of CjfifDecode::DecodeMarker that feeds CimgDecode).               */
int          jsnoop_batch_add_jpeg(JsnoopBatch*, const uint8_t* file, size_t len);
/* A progressive (SOF2) file into a batch -- jsnoop_batch_add_jpeg routes such files here by itself.  A batch holds either
 * baseline or progressive files; all scans of all its images then decode together, one launch per dependency level
 * (every restart interval of every scan of every image is one lane), then one finalize pass and the common back end.      */
int          jsnoop_batch_add_progressive(JsnoopBatch*, const uint8_t* file, size_t len);
/* Tiles already-added images so the batch holds `total` images (image i reuses the
 * bytes of image i % n): the bench's "N distinct seeds tiled to 1024".               */
int          jsnoop_batch_tile(JsnoopBatch*, int total);
/* Beyond the reference: the decodes of a batch may run its two halves on two streams side by side (same arenas, same results; the
   kernels of one half fill the thinly populated phases of the other: about 4 % more throughput on 1024 x 1080p).  parts = 0: the
   library decides (two streams from 8 MB of scan data in the batch -- the default), 1: one stream (profiling: per-kernel timings
   are then those of whole-batch launches), 2: two streams whenever the batch has two images.  0 / -1.                            */
int          jsnoop_batch_set_split(JsnoopBatch*, int parts);
int          jsnoop_batch_split_parts(const JsnoopBatch*);              /* what the setting comes to for the images the batch holds now: 1 or 2 */
/* ---- tuning: how the library decodes, never what it produces.  Every field has an automatic setting (0); the environment variables
 *      of tools/README.md are read ONCE per process and only supply the defaults jsnoop_tuning_defaults returns -- nothing on the
 *      decode path reads the environment.  A batch takes a copy at jsnoop_batch_set_tuning (call before upload; -1 + last_error on a
 *      value out of range); jsnoop_set_tuning does the same for the private batch behind a single-image decoder.                      */
typedef struct JsnoopTuning {
    uint32_t struct_size;     /* sizeof(JsnoopTuning) of the caller: a shorter (older) struct is accepted, the fields it lacks are automatic, and
                                 jsnoop_batch_get_tuning writes no byte past it; a longer one than the library knows is refused              */
    int32_t  sub_wl;          /* log2(32-bit words) of a sub-sequence: 4..8 = 64 B .. 1 KiB; 0 = by job size (4 / 5 / 6 / 7)              */
    int32_t  cand_rounds;     /* synchronisation form: -1 = rounds of k_sync only, n > 0 = candidates with at most n walk rounds (<= 64),
                                 0 = automatic (candidates with 16 rounds while the job is small enough, see cand_max_walks)          */
    uint64_t cand_max_walks;  /* largest job (64-byte pieces x blocks per MCU) that synchronises by candidates; 0 = 2 600 000         */
    int32_t  sync_launches;   /* synchronisation by rounds: 0 = one cut launch of k_sync, then list rounds over the whole job
                                 (k_sync_links / k_sync_round); n > 0 = n plain launches of k_sync (the form before round 6)           */
    int32_t  write_lanes;     /* lanes per sub-sequence in the write pass of the smallest jobs: 1, 2; 0 = automatic (2 up to 40 960 pieces) */
    int32_t  split;           /* as jsnoop_batch_set_split: 0 automatic, 1 one stream, 2 two streams                                  */
    int32_t  mcus_per_wave;   /* MCUs per back-end wave; 0 = one round of workgroups over the chip, at most 64                        */
    int32_t  pg_lanes;        /* progressive: restart intervals per wave 1, 2, 4, 8, 16 or 64 (lane-per-interval kernel); 0 = by batch size */
    uint32_t cross_checks;    /* JSNOOP_XC_* bits: alternative code paths kept for cross-checking, same results                       */
    uint32_t debug;           /* JSNOOP_DBG_* bits: diagnostics on stderr                                                             */
} JsnoopTuning;
#define JSNOOP_XC_BACKEND_GENERIC 0x01u  /* the all-layouts back-end kernel for every launch                                          */
#define JSNOOP_XC_WRITE_V1        0x02u  /* the first form of the write pass                                                          */
#define JSNOOP_XC_NO_TAIL         0x04u  /* damaged files: no tail take-over / second attempt, the whole image through the mirror     */
#define JSNOOP_XC_SIDE_EXACT      0x08u  /* side outputs always from the exact-mirror reader                                          */
#define JSNOOP_XC_CAND_VERIFY     0x10u  /* k_sync's verification mode behind every candidate chain                                   */
#define JSNOOP_XC_UNSTUFF_3PASS   0x20u  /* un-stuffing as count / scan / write passes instead of the fused look-back pass            */
#define JSNOOP_XC_DC_GENERIC      0x40u  /* DC-only decodes through the Full-IDCT kernels instead of the DC-only fast form            */
#define JSNOOP_DBG_CAND           0x01u  /* candidate chain: rounds, queued walks                                                     */
#define JSNOOP_DBG_CAND_LINKS     0x02u  /* ... and the links left open per image (stops the stream)                                  */
#define JSNOOP_DBG_TAIL           0x04u  /* damaged files: tail take-over decisions                                                   */
#define JSNOOP_DBG_TIMING         0x08u  /* single-image calls: where the wall time goes                                              */
void         jsnoop_tuning_defaults(JsnoopTuning* out);                 /* struct_size set, everything else the process defaults: writes
                                                                          * sizeof(JsnoopTuning) of THIS header                       */
/* ... for a caller built against an older (shorter) JsnoopTuning: at most struct_size bytes are written, struct_size says how many.
 * jsnoop_batch_get_tuning reads out->struct_size the same way: set it to sizeof(your JsnoopTuning) (or 0: this header's) before the call. */
void         jsnoop_tuning_defaults_sized(JsnoopTuning* out, uint32_t struct_size);
int          jsnoop_batch_set_tuning(JsnoopBatch*, const JsnoopTuning*);
void         jsnoop_batch_get_tuning(const JsnoopBatch*, JsnoopTuning* out);
int          jsnoop_set_tuning(JsnoopDecoder*, const JsnoopTuning*);
int          jsnoop_batch_count(const JsnoopBatch*);
int          jsnoop_batch_upload(JsnoopBatch*);      /* pinned host -> HBM (async), builds device descriptors */
int          jsnoop_batch_decode(JsnoopBatch*);      /* HBM -> HBM, asynchronous on the batch stream          */
int          jsnoop_batch_sync(JsnoopBatch*);        /* waits; then re-decodes flagged images on the exact path */
/* DC-only fast form.  DC-only (decode_ac = 0, what a single-image call with bDisplay = FALSE forces) is the reference's default mode: it parses the AC
 * symbols without storing them and never runs the IDCT, so every sample of a block is its cumulative DC.  A decode takes a form of its own for that --
 * a write pass without the coefficient arena and a back end straight from cumulative DC to DIB -- when EVERY image of the batch is DC-only, has one of
 * the common layouts (three components, 4:4:4 / 4:2:2 / 4:4:0 / 4:2:0) in the default preview mode without YCC shift and decode tables the parallel
 * path takes, the exact path is not forced, and the decode records no events: a log callback (jsnoop_set_log_callback) and jsnoop_batch_enable_log keep a decode
 * on the Full-IDCT kernels, as do JSNOOP_XC_DC_GENERIC and the cross-checks that name one of those kernels (JSNOOP_XC_WRITE_V1, _BACKEND_GENERIC).
 * Results are the same bit for bit.  After such a decode the coefficient arena does not hold its blocks: whatever reads it (jsnoop_batch_read_coefs, a
 * preview re-render, the repair of a damaged file at jsnoop_batch_sync) first decodes the batch again through the Full-IDCT kernels.
 * jsnoop_batch_last_form: the form behind the results the batch holds NOW -- 0 = nothing decoded, 1 = Full-IDCT kernels, 2 = DC-only fast form (so 1
 * after such a second decode); jsnoop_last_form: the same for the private batch behind a single-image decoder.                                       */
int          jsnoop_batch_last_form(const JsnoopBatch*);
int          jsnoop_last_form(JsnoopDecoder*);
/* Timed decode: `reps` decodes bracketed by hipEvents on the batch stream; per-stage
 * average milliseconds into stage_ms[JSNOOP_NUM_STAGES] (may be NULL).  Returns the
 * average milliseconds per whole decode, < 0 on error.                              */
#define JSNOOP_NUM_STAGES 8
double       jsnoop_batch_decode_timed(JsnoopBatch*, int reps, double* stage_ms);
const char*  jsnoop_stage_name(int stage);
/* per-image results */
int          jsnoop_batch_image_info(const JsnoopBatch*, int i, unsigned* out16);  /* dim_x,dim_y,img_x,img_y,mcu_w,mcu_h,mcu_xmax,mcu_ymax,
                                                                                     blk_xmax,blk_ymax,scan_bytes,flags,path,ns,file_len,0 */
const void*  jsnoop_batch_dib_dev(const JsnoopBatch*, int i);                      /* bottom-up BGRA, img_x*img_y*4 bytes in HBM */
int          jsnoop_batch_read_dib(JsnoopBatch*, int i, uint8_t* host_dst);        /* D2H copy of one DIB */
int          jsnoop_batch_read_planes(JsnoopBatch*, int i, int16_t* y, int16_t* cb, int16_t* cr);
int          jsnoop_batch_read_coefs(JsnoopBatch*, int i, int16_t* dst, size_t max_blocks); /* dequantised blocks, decode order */
/* 64-bit FNV-1a of every DIB computed on the device (one word per image), for
 * whole-batch parity checks without moving 8 GB over PCIe.                          */
/* the same statistics for image i of a decoded batch (needs want_planes): one fresh pass, as a DecodeScanImg with
 * bHistoEn (histo_en != 0) or only bStatClipEn (histo_en == 0) would leave them */
int          jsnoop_batch_color_stats(JsnoopBatch*, int i, int histo_en, uint32_t* out);
int          jsnoop_batch_dib_hashes(JsnoopBatch*, uint64_t* host_dst);
/* ---- everything else DecodeScanImg leaves behind, per image of a decoded batch: what the per-file pass of the reference's batch loop
 *      produces (CJPEGsnoopCore::DoBatchFileProcess -> AnalyzeFile -> DoLogSave, source/JPEGsnoopCore.cpp:765-845; the log body of this
 *      path is source/ImgDecode.cpp:3021-3025, :3126-3135 and :3630-3745).  Same code as the single-image API, addressed at image i.
 *  jsnoop_batch_side_outputs: any pointer may be NULL.  mcu_map [mcu_ymax*mcu_xmax] (m_pMcuFileMap :3229), dc_* [blk_ymax*blk_xmax]
 *      (m_pBlkDcValY/Cb/Cr :3524-3608; Cb / Cr untouched for a one-component image), dht_histo [2][4][17] (m_anDhtHisto :1190), status8 as
 *      jsnoop_scan_status, bright_avg10 as jsnoop_bright_avg (three-component images: needs want_planes).  Produced on request by the
 *      parallel side pass (about 1 ms per image), without touching coefficients or pixels.
 *  jsnoop_batch_enable_log: keep the decoder's event records of every image (24 KiB of HBM each); call before upload.
 *  jsnoop_batch_log: the text DecodeScanImg(nStart, bDisplay = TRUE, bQuiet = quiet) of a fresh CimgDecode writes to CDocLog for image i
 *      under bHistoEn = histo_en / bStatClipEn = stat_clip_en, through `fn` (needs jsnoop_batch_enable_log, and want_planes for
 *      three-component images and the statistics).
 *  jsnoop_batch_export_tiff: jsnoop_export_tiff for image i.   All four: 0 on success, -1 + jsnoop_last_error().                    */
int          jsnoop_batch_enable_log(JsnoopBatch*, int on);
int          jsnoop_batch_side_outputs(JsnoopBatch*, int i, uint32_t* mcu_map, int16_t* dc_y, int16_t* dc_cb, int16_t* dc_cr, uint32_t* dht_histo,
                                       unsigned* status8, int* bright_avg10);
int          jsnoop_batch_log(JsnoopBatch*, int i, int histo_en, int stat_clip_en, int quiet, jsnoop_log_fn fn, void* user);
int          jsnoop_batch_export_tiff(JsnoopBatch*, int i, const char* path, int mode);
uint64_t     jsnoop_batch_algorithmic_bytes(const JsnoopBatch*);                   /* sum(scan bytes + DIB bytes), SURVEY.md 8(d) */
uint64_t     jsnoop_batch_pixels(const JsnoopBatch*);                              /* sum(SOF X*Y) */
/* HBM that jsnoop_batch_upload requests for the images the batch holds now (0 for an empty batch): every arena of the decode, the allocator's
 * slack included.  Where the library chooses a form by job size (sub-sequence length, candidate synchronisation) the largest candidate is counted:
 * the figure is never below the request and never falls when an image is added.  Scratch that only a later request allocates (side-output
 * passes, second attempts at damaged files) is not part of it.  Host arithmetic only.                                                        */
uint64_t     jsnoop_batch_device_bytes(const JsnoopBatch*);

/* ---- pack: DIBs of a decoded batch -> caller-owned DEVICE memory as cropped, top-down, three-channel pixels ----------------------
 * The DIB is the reference's CDIB: bottom-up, BGRA with A = 0, img_x x img_y rounded up to whole MCUs.  jsnoop_batch_pack rearranges
 * any subset of a decoded batch in ONE kernel launch: output pixel (x, y) of image i, 0 <= x < dim_x, 0 <= y < dim_y (the SOF
 * dimensions), is DIB pixel (x, img_y - 1 - y).  Channels in output order c = 0..2 are R, G, B, or B, G, R with bgr != 0.
 *   JSNOOP_PACK_HWC: element (x, y, c) at ptr + y * row_pitch + (x * 3 + c) * elem
 *   JSNOOP_PACK_CHW: element (x, y, c) at ptr + c * plane_pitch + y * row_pitch + x * elem
 *   JSNOOP_PACK_U8 : elem = 1, the DIB's byte as it is
 *   JSNOOP_PACK_F32: elem = 4, (float)byte * scale[c] + bias[c]: one rounded fp32 multiply, then one rounded fp32 add (no FMA)
 * Pitches are in bytes; 0 = dense (row_pitch: dim_x * 3 * elem for HWC, dim_x * elem for CHW; plane_pitch: dim_y * row_pitch; HWC
 * ignores plane_pitch).  Only the addressed elements are written: the bytes between the dense row and row_pitch keep their content.
 *
 * Ordering: the launch is enqueued on the batch's stream, behind the decode enqueued last (both halves of a two-stream decode
 * included), and the call returns without waiting: the destination is ready once that stream has passed the pack (jsnoop_batch_sync,
 * or the caller's own event on the stream it gave jsnoop_batch_create).  Damaged files are repaired at jsnoop_batch_sync: a pack
 * enqueued AFTER jsnoop_batch_sync sees the repaired DIB, one enqueued BEFORE it sees what the parallel path left.
 * The pack never decodes again: jsnoop_batch_last_form is the same before and after.
 *
 * Refused with -1 + jsnoop_last_error(), nothing launched, nothing written: a NULL or not yet decoded batch; an image index out of
 * range; an image without a decoded DIB (the text names it -- every image of a decoded batch has one, so for images a batch accepted
 * only the batch-level check can fire); a NULL destination pointer; a row_pitch or plane_pitch below the dense size; JSNOOP_PACK_F32
 * with a pointer or pitch that is not a multiple of 4; an unknown layout, dtype or struct_size.  n == 0 is 0.                        */
#define JSNOOP_PACK_HWC 0
#define JSNOOP_PACK_CHW 1
#define JSNOOP_PACK_U8  0
#define JSNOOP_PACK_F32 1
typedef struct JsnoopPackSpec {
    uint32_t struct_size;           /* sizeof(JsnoopPackSpec) of the caller, read like JsnoopTuning's: shorter is accepted (the fields it lacks
                                       are the defaults), longer is refused                                                               */
    int32_t  layout, dtype, bgr;    /* JSNOOP_PACK_HWC / _CHW, JSNOOP_PACK_U8 / _F32, 0 = R,G,B                                            */
    float    scale[3], bias[3];     /* JSNOOP_PACK_F32 only, by OUTPUT channel; defaults 1 and 0                                           */
} JsnoopPackSpec;
typedef struct JsnoopPackDst { void* ptr; uint64_t row_pitch, plane_pitch; } JsnoopPackDst;   /* device pointer; bytes; 0 = dense */
void         jsnoop_pack_spec_defaults(JsnoopPackSpec* out);
/* dense size in bytes of image i's output under `spec` (dim_x * dim_y * 3 * elem); host arithmetic; 0 for a bad argument */
uint64_t     jsnoop_batch_pack_bytes(const JsnoopBatch*, const JsnoopPackSpec* spec, int i);
/* images: n indices into the batch, in any order (NULL = images 0..n-1); dst: n destinations */
int          jsnoop_batch_pack(JsnoopBatch*, const JsnoopPackSpec* spec, const int* images, int n, const JsnoopPackDst* dst);
/* the device the batch lives on (jsnoop_set_device when it was created): where the destinations of jsnoop_batch_pack must be; -1 for NULL */
int          jsnoop_batch_device(const JsnoopBatch*);

/* ---- pack, cropped and resampled: a rectangle of every listed image at the size its destination asks for ------------------------------
 * jsnoop_batch_pack_resized is jsnoop_batch_pack with a source rectangle (ROI) and an output size per destination: layout, dtype, bgr,
 * scale and bias come from the same JsnoopPackSpec, pitches mean the same for an out_w x out_h image, and ONE kernel launch serves the
 * whole list -- 1024 crops into one [N,3,H,W] allocation, or a set of differently sized thumbnails.  `images` may name an image several
 * times (several crops of one file).  The ROI is given in the coordinates of the plain pack's output (top-down, cropped to dim_x x
 * dim_y); roi_w == roi_h == 0 with roi_x == roi_y == 0 is the whole image.
 *
 * What a pixel is.  R is the ROI as a top-down rh x rw x 3 array of the DIB's bytes (the plain pack, cropped).  Output pixel (ox, oy),
 * channel c, has the interpolant q = (float)((double)S / (double)D) with exact integers S and D (S < 2^53): one IEEE double division, one
 * rounding to float; nothing outside the ROI contributes.
 *   JSNOOP_RESIZE_NEAREST : x = ((2 ox + 1) rw) div (2 out_w), y likewise; S = R[y][x][c], D = 1.
 *   JSNOOP_RESIZE_BILINEAR: half-pixel centres, edge replication inside the ROI (torch's bilinear, align_corners=False, no antialias):
 *       Dx = 2 out_w, P = (2 ox + 1) rw - out_w; P < 0: x0 = 0, rx = 0; else x0 = P div Dx, rx = P mod Dx; x1 = min(x0 + 1, rw - 1);
 *       likewise Dy, y0, y1, ry;  S = (Dx-rx)(Dy-ry) R[y0][x0] + rx (Dy-ry) R[y0][x1] + (Dx-rx) ry R[y1][x0] + rx ry R[y1][x1], D = Dx Dy.
 *   JSNOOP_RESIZE_AREA    : box filter with fractional coverage.  In units of 1 / out_w source pixel output column ox covers
 *       [ox rw, (ox+1) rw) and source column j covers [j out_w, (j+1) out_w); wx(ox, j) is the length of their overlap, wy likewise;
 *       S = sum_j sum_i wy wx R[j][i][c], D = rw rh.
 *   JSNOOP_PACK_U8 : q rounded to nearest, ties to even.   JSNOOP_PACK_F32: q * scale[c] + bias[c], one rounded multiply, one rounded add.
 * With out_w == rw and out_h == rh every filter gives exactly the plain pack of the ROI.
 *
 * Ordering: jsnoop_batch_pack's -- enqueued on the batch's stream behind the decode enqueued last (both halves of a two-stream decode
 * included), not waited for; a call before jsnoop_batch_sync sees what the parallel path left; never decodes again
 * (jsnoop_batch_last_form is unchanged).
 *
 * Refused with -1 + jsnoop_last_error(), nothing launched, nothing written: everything jsnoop_batch_pack refuses ("dense" meaning the
 * output's out_w x out_h); an unknown filter; out_w or out_h of 0 or above 32767; an ROI with one of roi_w / roi_h zero and the other
 * not, or with both zero and roi_x or roi_y not; an ROI that leaves dim_x x dim_y.  n == 0 is 0.                                     */
#define JSNOOP_RESIZE_NEAREST  0
#define JSNOOP_RESIZE_BILINEAR 1
#define JSNOOP_RESIZE_AREA     2
typedef struct JsnoopResizeDst {
    void*    ptr; uint64_t row_pitch, plane_pitch;   /* as JsnoopPackDst, for an out_w x out_h image; 0 = dense */
    uint32_t out_w, out_h;                           /* 1 .. 32767 each */
    uint32_t roi_x, roi_y, roi_w, roi_h;             /* source rectangle in the coordinates of the plain pack's output (top-down, cropped
                                                        to dim_x x dim_y); roi_w == roi_h == 0 (then roi_x == roi_y == 0) = the whole image */
} JsnoopResizeDst;
int          jsnoop_batch_pack_resized(JsnoopBatch*, const JsnoopPackSpec* spec, int filter,
                                       const int* images, int n, const JsnoopResizeDst* dst);

/* ---- coefficient tensors: the DCT blocks of a decoded batch by component, in caller-owned device memory --------------------------------
 * The third sibling of the two packs, for the decode's other product.  The coefficient arena holds [blocks][64] dequantised int16 in
 * natural order and DECODE order (MCU after MCU, the components interleaved inside the MCU), with only the DC difference in slot 0.
 * jsnoop_batch_pack_coefs turns any subset of it into one tensor per destination -- one component of one image -- in ONE kernel launch:
 * blocks in raster order of that component's own block grid, the true (cumulative) DC in slot 0.
 *
 * Block grid.  `comp` counts the scan's components from 0 (0 = Y).  Component c has samp_h[c] x samp_v[c] blocks per MCU; its grid is
 * bw = mcu_xmax * samp_h[c] by bh = mcu_ymax * samp_v[c] blocks, MCU padding included (jsnoop_batch_coef_grid).  Block (bx, by) is block
 * (by % samp_v) * samp_h + (bx % samp_h) of that component in MCU (bx / samp_h, by / samp_v).
 *
 * What an element is.  Element (bx, by, k) for natural index k != 0 is the arena's value, bit for bit: (int16)(level * dqt[k]) with the
 * multipliers jsnoop_batch_image_dqt returns.  For natural index 0 it is the block's cumulative DC -- the running sum of the dequantised
 * differences in wrapping int16 arithmetic, restarted at every restart interval -- never the difference.  Baseline and progressive images
 * mean the same thing: a progressive file that carries a baseline file's coefficients gives that file's tensors.  An image decoded with
 * decode_ac = 0 gives what the Full-IDCT kernels leave for it: zeros in slots 1..63, the cumulative DC in slot 0.
 *
 * Forms.  JSNOOP_COEF_BLOCKS: [bh][bw][64], element (bx, by, k) at ptr + by * row_pitch + (bx * 64 + k) * elem; plane_pitch is ignored.
 * JSNOOP_COEF_FREQ: [64][bh][bw], element at ptr + k * plane_pitch + by * row_pitch + bx * elem.  JSNOOP_COEF_I16: elem 2, the arena's
 * int16 as it is; JSNOOP_COEF_F32: elem 4, (float)value, exact.  JSNOOP_COEF_NATURAL: k = row * 8 + column, the arena's order;
 * JSNOOP_COEF_ZIGZAG: position z holds natural index zigzag[z] (T.81 Figure A.6).  Dense pitches (what 0 means): BLOCKS row_pitch =
 * bw * 64 * elem; FREQ row_pitch = bw * elem, plane_pitch = bh * row_pitch.  Only addressed elements are written: pitch gaps and
 * everything around a destination keep their bytes.
 *
 * Ordering: jsnoop_batch_pack's -- enqueued on the batch's stream behind the decode enqueued last (both halves of a two-stream decode
 * included), not waited for; a call after jsnoop_batch_sync sees the repaired arena, a call before it sees what the parallel path left.
 * After a DC-only fast-form decode (jsnoop_batch_last_form == 2) the arena does not hold the blocks: the call then does what
 * jsnoop_batch_read_coefs does, decodes the batch once more through the Full-IDCT kernels and waits for it, and jsnoop_batch_last_form
 * goes 2 -> 1.  That is the one case in which this call decodes again.
 *
 * Refused with -1 + jsnoop_last_error(), nothing launched, nothing written: a NULL batch or one not yet decoded; an image index out of
 * range; comp at or past the image's component count; a NULL destination; a non-zero `reserved`; a pitch below the dense size; a pointer
 * or pitch that is not a multiple of elem; an unknown layout, dtype, order or struct_size (read like JsnoopPackSpec's: shorter accepted
 * with the lacking fields at their defaults, longer refused).  n == 0 is 0; images == NULL means images 0 .. n - 1; an image may be listed
 * several times (once per component is the normal use).
 *
 * jsnoop_batch_image_dqt: the 64 multipliers the decode used for that component, natural order, host arithmetic only.  The library keeps
 * ONE table per component: for a baseline image the table its component selects when the scan starts, for a progressive image the
 * definition of the selected destination the file's header walk ended with -- a file that redefines a table between scans is dequantised
 * with, and reports, that one table.                                                                                                 */
#define JSNOOP_COEF_BLOCKS  0
#define JSNOOP_COEF_FREQ    1
#define JSNOOP_COEF_I16     0
#define JSNOOP_COEF_F32     1
#define JSNOOP_COEF_NATURAL 0
#define JSNOOP_COEF_ZIGZAG  1
typedef struct JsnoopCoefSpec { uint32_t struct_size; int32_t layout, dtype, order; } JsnoopCoefSpec;
typedef struct JsnoopCoefDst  { void* ptr; uint64_t row_pitch, plane_pitch; uint32_t comp, reserved; } JsnoopCoefDst;   /* device pointer; pitches in bytes, 0 = dense */
void         jsnoop_coef_spec_defaults(JsnoopCoefSpec* out);                                   /* BLOCKS, I16, NATURAL; NULL tolerated */
int          jsnoop_batch_coef_grid(const JsnoopBatch*, int i, int comp, unsigned* bw, unsigned* bh);        /* host arithmetic; 0 / -1 */
uint64_t     jsnoop_batch_coef_bytes(const JsnoopBatch*, const JsnoopCoefSpec*, int i, int comp);            /* dense size; 0 = bad argument */
int          jsnoop_batch_pack_coefs(JsnoopBatch*, const JsnoopCoefSpec*, const int* images, int n, const JsnoopCoefDst* dst);
int          jsnoop_batch_image_dqt(const JsnoopBatch*, int i, int comp, uint16_t* out64);     /* natural order; host only; 0 / -1 */

/* ---- colour statistics of a whole batch: one row of JSNOOP_STATS_WORDS words per listed image, on the device ---------------------------
 * The fourth sibling: jsnoop_batch_color_stats(b, i, ...) costs a fill, a launch, a copy and a wait per image (and a second round for
 * an image with more than 10 range events).  jsnoop_batch_pack_stats computes the rows of any subset of a decoded batch in TWO kernel
 * launches, from the retained int16 planes (the batch needs want_planes), into caller-owned device memory.
 *
 * What a row is.  Row k holds exactly the words jsnoop_batch_color_stats(b, images[k], histo_en, out) writes: the layout above
 * (JSNOOP_STATS_WORDS), records seeded with 0, sums modulo 2^32, over the MCU-padded picture img_x x img_y; a fresh budget of 10 YCC
 * range events per image, counted in the reference's visiting order -- raster order, within a pixel Y over, Y under, Cb over, Cb under,
 * Cr over, Cr under; histo_en == 0 leaves only the clip counters (words 37..48).  Baseline and progressive images, images decoded by the
 * Full-IDCT kernels and by the DC-only fast form are treated alike: the call reads the planes and never decodes again
 * (jsnoop_batch_last_form is unchanged).  The preview shift of an image descriptor is part of the shared per-pixel arithmetic and is
 * carried along, but no public call sets it on a user batch: through this door it is always the default (no shift) and untested.
 *
 * dst: device memory, a multiple of 4; row k starts at word k * row_pitch_words (0 = dense, else at least JSNOOP_STATS_WORDS).  All
 * JSNOOP_STATS_WORDS words of every listed row are defined by the call (rows are zeroed on the stream first: a second call into the same
 * memory gives the same rows); words between JSNOOP_STATS_WORDS and the pitch keep their content.  totals: NULL, or device memory
 * [n][6]: how many range events of each kind image k has IN ALL, indexed like words 37..42 (Y<0, Y>255, Cb<0, Cb>255, Cr<0, Cr>255) --
 * the row's counters stop at 10 together, these do not.  images: n indices into the batch, any order, any subset, repeats allowed (NULL =
 * images 0..n-1).
 *
 * Ordering: jsnoop_batch_pack's -- enqueued on the batch's stream behind the decode enqueued last (both halves of a two-stream decode
 * included), not waited for; a call after jsnoop_batch_sync sees the repaired planes, a call before it what the parallel path left.
 * Scratch (a few words per listed image and per picture row) is batch-owned, grown on demand and not part of jsnoop_batch_device_bytes.
 *
 * Refused with -1 + jsnoop_last_error(), nothing launched, nothing written: a NULL batch or one not yet decoded; an image index out of
 * range; a batch without planes; a NULL destination or one that is not a multiple of 4 (totals likewise); a row_pitch_words below
 * JSNOOP_STATS_WORDS.  n == 0 is 0.
 *
 * jsnoop_batch_read_stats: the same rows, dense, into HOST memory through batch-owned device scratch: one D2H copy, one wait.          */
int          jsnoop_batch_pack_stats(JsnoopBatch*, int histo_en, const int* images, int n, void* dst, uint64_t row_pitch_words, uint32_t* totals);
int          jsnoop_batch_read_stats(JsnoopBatch*, int histo_en, const int* images, int n, uint32_t* host_dst);

/* ---- coefficient histograms: one row of counts per (image, component), by DCT frequency, on the device ---------------------------------
 * The fifth sibling, the reduction of the coefficient side: the histogram of every DCT frequency of one component of one image -- what
 * double-compression detection, quantiser estimation and first-digit statistics start from -- without the tensors ever being written.
 * jsnoop_batch_pack_coef_hist turns any list of (image, component) pairs of a decoded batch into one row per pair in caller-owned
 * device memory, in ONE kernel launch behind a small one that initialises the rows.
 *
 * What a row is.  Let T be the tensor jsnoop_batch_pack_coefs gives for (image, comp) in BLOCKS / I16 / NATURAL: [bh][bw][64], MCU padding
 * included, the cumulative DC in natural index 0 (baseline and progressive files mean the same thing; an image decoded with decode_ac = 0
 * has zeros in 1..63), and q[k] what jsnoop_batch_image_dqt returns.  For an element v at natural index k, x = v when quantised == 0 and
 * x = v / max(q[k], 1) otherwise: C integer division, truncating toward zero, of the int16 as it stands in the arena -- exact levels
 * whenever |level * q| <= 32767; where the product wrapped int16 the quotient is what it is.  Position p = 0..63 is natural index p
 * (JSNOOP_COEF_NATURAL) or natural index zigzag[p] (JSNOOP_COEF_ZIGZAG).  With range R (1..127) and NB = 2 R + 1 a row is 64 * NB + 128
 * words (jsnoop_coef_hist_words): hist[p][b], uint32 at word p * NB + b, the number of blocks whose x at position p has
 * clamp(x, -R, R) + R == b -- both end bins saturate; min[p], int32 at word 64 * NB + p, and max[p], int32 at word 64 * NB + 64 + p, the
 * smallest and largest UNCLAMPED x at that position (every grid has a block: no seed is ever visible).
 *
 * dst: device memory, a multiple of 4; row k belongs to (images[k], comps[k]) and starts at word k * row_pitch_words (0 = dense, else at
 * least the row length).  Any order, any subset, repeats allowed; each row stands alone.  All words of every listed row are defined by the
 * call (rows are initialised on the stream first: a second call into the same memory gives the same rows); words between the row length
 * and the pitch keep their bytes.
 *
 * Ordering: jsnoop_batch_pack_coefs', word for word -- enqueued on the batch's stream behind the decode enqueued last (both halves of a
 * two-stream decode included), not waited for; a call after jsnoop_batch_sync sees the repaired arena, a call before it sees what the
 * parallel path left.  After a DC-only fast-form decode (jsnoop_batch_last_form == 2) the call does what jsnoop_batch_read_coefs does,
 * decodes the batch once more through the Full-IDCT kernels and waits for it, and jsnoop_batch_last_form goes 2 -> 1.  That is the one
 * case in which this call decodes again.
 *
 * Refused with -1 + jsnoop_last_error(), nothing launched, nothing written: a NULL batch or one not yet decoded; NULL images, comps or
 * dst; an image index out of range; a comp at or past the image's component count; a dst that is not a multiple of 4; a pitch that is
 * non-zero and below the row length; a range outside 1..127; an unknown order or struct_size (read like JsnoopCoefSpec's: shorter
 * accepted with the lacking fields at their defaults, longer refused).  n == 0 is 0.
 *
 * jsnoop_batch_read_coef_hist: the same rows, dense, into HOST memory through batch-owned device scratch: one D2H copy, one wait.      */
typedef struct JsnoopCoefHistSpec { uint32_t struct_size; int32_t order, quantised; uint32_t range; } JsnoopCoefHistSpec;
void         jsnoop_coef_hist_spec_defaults(JsnoopCoefHistSpec* out);                          /* NATURAL, quantised 1, range 127; NULL tolerated */
uint32_t     jsnoop_coef_hist_words(const JsnoopCoefHistSpec*);                                /* row length in words; 0 = bad spec */
int          jsnoop_batch_pack_coef_hist(JsnoopBatch*, const JsnoopCoefHistSpec*, const int* images, const int* comps, int n, void* dst, uint64_t row_pitch_words);
int          jsnoop_batch_read_coef_hist(JsnoopBatch*, const JsnoopCoefHistSpec*, const int* images, const int* comps, int n, uint32_t* host_dst);

/* ---- plane tensors: the Y, Cb, Cr samples of a decoded batch by component, in caller-owned device memory --------------------------------
 * The sixth sibling, for the decode's third product.  A batch that keeps its planes (want_planes) holds, per image, the reference's
 * m_pPixValY / Cb / Cr: int16 samples before CapYccRange, three fractional bits, chroma replicated to the luma grid.  The DIB cannot give
 * them back (the clamp, the float colour lines and the replication are lossy) and jsnoop_batch_read_planes crosses PCIe.
 * jsnoop_batch_pack_planes turns any subset into one two-dimensional tensor per destination -- one component of one image -- in ONE kernel
 * launch.  Pure data movement: no sample is recomputed.
 *
 * What an element is.  `comp` counts the scan's components from 0 (0 = Y; a one-component image has component 0 only).  P_c is what
 * jsnoop_batch_read_planes gives for component c of image i: top-down, blk_xmax * 8 samples wide, MCU padding included.  eh = expand_h[c]
 * and ev = expand_v[c] are the replication factors the decode used: hmax / samp_h[c] and vmax / samp_v[c], integer division, hmax and vmax
 * the largest sampling factors of the scan (1 for a one-component scan).
 *   JSNOOP_PLANE_FULL  : dim_x x dim_y (the SOF dimensions); element (x, y) is P_c[y][x].
 *   JSNOOP_PLANE_NATIVE: ceil(dim_x / eh) x ceil(dim_y / ev); element (x, y) is P_c[y * ev][x * eh].  A decimation of the retained plane,
 *                        defined for every layout; where the plane is a pure replication it is the component's own sample grid.  For a
 *                        component with eh = ev = 1 (luma, normally) it equals FULL.
 *   JSNOOP_PLANE_I16   : elem 2, the plane's int16 as it is.
 *   JSNOOP_PLANE_U8    : elem 1, min(max((v + 1024) / 8, 0), 255) with C division, truncating toward zero: CapYccRange's value, the 8-bit
 *                        sample the colour conversion starts from.  After the clamp it equals clamp_s8(v >> 3) + 128 with an arithmetic
 *                        shift, the form the DIB path uses (a negative numerator differs between the two only below the clamp).
 *   JSNOOP_PLANE_F32   : elem 4, (float)v * scale[comp] + bias[comp]: one rounded fp32 multiply, then one rounded fp32 add (no FMA).
 * Element (x, y) lies at ptr + y * row_pitch + x * elem; row_pitch is in bytes, 0 = dense (w * elem).  Only addressed elements are
 * written: pitch gaps and everything around a destination keep their bytes.  U8 destinations may start at any byte, I16 at any even one.
 * The preview shift of an image descriptor is not part of the planes (they hold the un-shifted samples) and is not applied.
 *
 * Ordering: jsnoop_batch_pack_stats', word for word -- enqueued on the batch's stream behind the decode enqueued last (both halves of a
 * two-stream decode included), not waited for; a call after jsnoop_batch_sync sees the repaired planes, a call before it what the parallel
 * path left.  The call reads the planes and never decodes again: jsnoop_batch_last_form is unchanged, also after a DC-only fast-form
 * decode, whose kernels write the planes too.
 *
 * Refused with -1 + jsnoop_last_error(), nothing launched, nothing written: a NULL batch or one not yet decoded; a batch without planes
 * (want_planes); an image index out of range; comp at or past the image's component count, or above 2; a NULL destination; a non-zero
 * `reserved`; a row_pitch that is non-zero and below the dense row; a pointer or pitch that is not a multiple of elem; an unknown res,
 * dtype or struct_size (read like JsnoopPackSpec's: shorter accepted with the lacking fields at their defaults, longer refused).  n == 0
 * is 0; images == NULL means images 0 .. n - 1; an image may be listed several times (once per component is the normal use).           */
#define JSNOOP_PLANE_FULL   0
#define JSNOOP_PLANE_NATIVE 1
#define JSNOOP_PLANE_I16    0
#define JSNOOP_PLANE_U8     1
#define JSNOOP_PLANE_F32    2
typedef struct JsnoopPlaneSpec { uint32_t struct_size; int32_t res, dtype; float scale[3], bias[3]; } JsnoopPlaneSpec;   /* scale, bias: JSNOOP_PLANE_F32 only, by component */
typedef struct JsnoopPlaneDst  { void* ptr; uint64_t row_pitch; uint32_t comp, reserved; } JsnoopPlaneDst;               /* device pointer; pitch in bytes, 0 = dense */
void         jsnoop_plane_spec_defaults(JsnoopPlaneSpec* out);                                 /* FULL, I16, scale 1, bias 0; NULL tolerated */
int          jsnoop_batch_plane_size(const JsnoopBatch*, const JsnoopPlaneSpec*, int i, int comp, unsigned* w, unsigned* h);   /* host arithmetic; 0 / -1 */
uint64_t     jsnoop_batch_plane_bytes(const JsnoopBatch*, const JsnoopPlaneSpec*, int i, int comp);                           /* dense size; 0 = bad argument */
int          jsnoop_batch_pack_planes(JsnoopBatch*, const JsnoopPlaneSpec*, const int* images, int n, const JsnoopPlaneDst* dst);

/* ---- libjpeg's pixels: a decoded batch rendered with the integer IDCT, fancy upsampling and fixed-point colour, on the device -------------
 * The seventh sibling.  The DIB holds JPEGsnoop's pixels (fp32 IDCT, replicated chroma, fp32 colour lines); every other decoder a user can
 * compare with -- Pillow, OpenCV, torchvision, browsers, djpeg -- gives libjpeg's.  jsnoop_batch_pack_ijg renders any subset of a decoded
 * batch a second time, from the coefficient arena and the cumulative DC, in ONE kernel launch, and stores the result in the forms of
 * jsnoop_batch_pack: the same JsnoopPackSpec (HWC / CHW, uint8 / float32 with (float)v * scale[c] + bias[c] in two rounded operations,
 * bgr), the same JsnoopPackDst (dense or pitched rows at any byte alignment for uint8), the sizes of jsnoop_batch_pack_bytes, cropped to the
 * SOF dimensions, top-down.  Only addressed elements are written.
 *
 * What a pixel is (tests/ijg_model.py is the definition).  Per block libjpeg's jidctint ("islow", CONST_BITS 13,
 * PASS1_BITS 2: columns descaled by 11, then rows by 18, 32-bit wrapping sums), sample = clamp(result + 128, 0, 255) -- libjpeg's pixels
 * exactly while |result| <= 511, which every file an encoder wrote satisfies.  Chroma of a 2 x 1 / 2 x 2 subsampled image goes through
 * libjpeg's triangle filter (h2v1 / h2v2 "fancy" upsampling), its neighbours clamped to the component's real extent
 * ceil(dim_x / 2) x ceil(dim_y / 2 or 1); a chroma plane at most two samples wide is replicated instead, as libjpeg does it.  Colour:
 * R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16), clamped.  A
 * one-component image gives R = G = B = Y.  The preview mode and the YCC shift of an image descriptor are not applied.
 *
 * Renderable: precision 8, and one component, or three taken as Y, Cb, Cr with chroma sampled 1 x 1 and luma 1 x 1, 2 x 1 or 2 x 2
 * (4:4:4, 4:2:2, 4:2:0).  jsnoop_batch_ijg_renderable says 1, or 0 with the reason in jsnoop_last_error(); host arithmetic only.
 *
 * Ordering: jsnoop_batch_pack_coefs', word for word -- enqueued on the batch's stream behind the decode enqueued last (both halves of a
 * two-stream decode included), not waited for; a call after jsnoop_batch_sync renders the repaired blocks, a call before it what the
 * parallel path left.  After a DC-only fast-form decode (jsnoop_batch_last_form == 2) the call does what jsnoop_batch_read_coefs does,
 * decodes the batch once more through the Full-IDCT kernels and waits for it, and jsnoop_batch_last_form says 1 afterwards.
 *
 * Refused with -1 + jsnoop_last_error(), nothing launched, nothing written: everything jsnoop_batch_pack refuses, and a listed image that
 * is not renderable (the text names it and why).  n == 0 is 0; images == NULL means images 0 .. n - 1; any order, subsets and repeats.    */
int          jsnoop_batch_ijg_renderable(const JsnoopBatch*, int i);
int          jsnoop_batch_pack_ijg(JsnoopBatch*, const JsnoopPackSpec* spec, const int* images, int n, const JsnoopPackDst* dst);

/* ---- libjpeg's pixels at 1/2, 1/4, 1/8 size: the scaled IDCTs, on the device ----------------------------------------------------------------
 * What Image.draft / Image.thumbnail, cv2.IMREAD_REDUCED_COLOR_2/4/8 and djpeg -scale 1/N give: the blocks go through libjpeg's smaller
 * inverse transforms (jidctred.c: 4 x 4, 2 x 2, 1 x 1), full-size pixels are never made.  jsnoop_batch_pack_ijg_scaled is
 * jsnoop_batch_pack_ijg with a denominator: denom 1 IS that call (the same launch, the same bytes); denom 2, 4, 8 render image i as
 * ceil(dim_x / denom) x ceil(dim_y / denom) pixels, top-down, in ONE launch (k_render_ijg_scaled), through the same JsnoopPackSpec /
 * JsnoopPackDst with sizes and pitches taken against the reduced picture.  Any other denom is refused.
 *
 * What a pixel is (tests/ijg_scaled_model.py is the definition, equal to Pillow's draft()ed decode byte for byte).
 * m = 8 / denom.  A component is transformed at n = m, doubled while n < 8 and both (hmax m) % (h n 2) and (vmax m) % (v n 2) are 0
 * (jdmaster.c): grey, 4:4:4 and all of 4:2:2 at m; 4:2:0 luma at m and chroma at 2 m -- the MCU's output size, so 4:2:0 chroma is not
 * upsampled at all.  Pass 1 along the columns, pass 2 along the n rows, CONST_BITS 13, PASS1_BITS 2, 32-bit wrapping sums,
 * sample = clamp(result + 128, 0, 255); the 1 x 1 is DESCALE(dc, 3).  4:2:2 chroma goes through the h2v1 triangle filter on the reduced
 * plane at denom 2 and 4 (neighbours clamped to the plane's real width, a plane at most two samples wide replicated) and is replicated at
 * denom 8, where libjpeg has no filter.  The colour lines are jsnoop_batch_pack_ijg's.
 *
 * Ordering, the re-decode behind a DC-only fast form, the renderable layouts and every refusal (-1 + jsnoop_last_error(), nothing launched,
 * nothing written) are jsnoop_batch_pack_ijg's.  jsnoop_batch_ijg_scaled_size gives the reduced size of a renderable image (host arithmetic),
 * jsnoop_batch_pack_ijg_scaled_bytes the dense size of its destination.                                                                     */
int          jsnoop_batch_ijg_scaled_size(const JsnoopBatch*, int i, unsigned denom, unsigned* w, unsigned* h);                /* host arithmetic; 0 / -1 */
uint64_t     jsnoop_batch_pack_ijg_scaled_bytes(const JsnoopBatch*, const JsnoopPackSpec*, unsigned denom, int i);             /* dense size; 0 = bad argument */
int          jsnoop_batch_pack_ijg_scaled(JsnoopBatch*, const JsnoopPackSpec* spec, unsigned denom, const int* images, int n, const JsnoopPackDst* dst);

/* ---- export: a decoded batch written back as baseline JPEG files, entropy-coded on the device -------------------------------------------
 * The one product of a decode that is a FILE.  jsnoop_batch_export_jpeg encodes what the batch holds for every listed image -- the
 * coefficient arena and the cumulative DC, so the repaired blocks of a damaged file after jsnoop_batch_sync, the merged scans of a
 * progressive one -- as one sequential Huffman file per image (SOF0, or SOF1 where a multiplier needs 16 bits) with the Annex K tables, into
 * device memory the batch owns.  tests/export_model.py is the definition, byte for byte; DESIGN.md section 4.13 has the contract.
 *
 * Levels.  AC: level = arena[b][n] / q_c[n], C division, q_c the multipliers of jsnoop_batch_image_dqt.  DC: d = (int16)(dccum[b] - dccum[p]),
 * p the block of the same component before b in decode order (0 for the component's first block), level = d / q_c[0].  No restart markers
 * are written.  The result word of an image:
 *   JSNOOP_EXPORT_OK          the file was written.
 *   JSNOOP_EXPORT_INEXACT     a value leaves a remainder (its int16 product wrapped in the decode).
 *   JSNOOP_EXPORT_UNCODABLE   a DC difference level beyond +-2047 or an AC level beyond +-1023: Annex K has no code for it.
 *   JSNOOP_EXPORT_UNSUPPORTED the SOF precision is not 8 (host arithmetic; nothing is launched for the image).
 * The result is the largest of the image's blocks'; `detail` is the lowest block (counted inside the image, decode order) that has it, for
 * INEXACT and UNCODABLE.  An image that is not OK has length 0 and disturbs no other image of the call.
 *
 * The file: SOI; APP0 JFIF 1.01 (units 0, density 1 x 1, no thumbnail) unless spec.jfif == 0; one DQT per component (id = component index,
 * Pq = 1 when a multiplier is above 255); SOF0 / SOF1 (P 8, Y = dim_y, X = dim_x, ids 1..n, the image's H and V -- a one-component image
 * 1 x 1 --, Tq = component index); DHT DC0, AC0 and for three components DC1, AC1 (Annex K.3 - K.6, one table per segment); SOS (first component
 * tables 0/0, the others 1/1, Ss 0, Se 63, Ah/Al 0); the blocks of the MCU-padded grid in decode order (Annex F: ZRL for runs above 15,
 * EOB unless position 63 is non-zero; MSB first; the last byte padded with ones; every FF followed by 00, a padded last byte too); EOI.
 *
 * Ordering and waits.  The call encodes what the arena holds when it is made, on the batch's stream behind the decode enqueued last; behind
 * a DC-only fast-form decode the batch is first decoded once more in the generic form (jsnoop_batch_last_form goes 2 -> 1, as for
 * jsnoop_batch_pack_coefs); a decode_ac = 0 batch exports DC-only blocks.  File sizes depend on the data, so the call waits for the device
 * twice: once behind the measuring pass and its prefix sums (result words and bit lengths come back, the memory is sized), once at the
 * end (file lengths come back).  When it returns 0 every file is complete.  The files stay valid until the next export, clear, upload or
 * destroy of the batch.  -1 + jsnoop_last_error(): a NULL batch or one not decoded, an image index out of range, n < 0, a bad struct_size
 * (read like JsnoopPackSpec's), a device error.  images == NULL means images 0 .. n - 1; any order, subsets and repeats are allowed.
 *
 * jsnoop_batch_export_count: entries of the last export (0: none, or invalidated).  jsnoop_batch_export_file: entry k -- device pointer
 * (NULL when len is 0), length, result, detail, image index; any output pointer may be NULL.  jsnoop_batch_read_export: entry k to the host
 * (waits); jsnoop_batch_export_copy: entry k device-to-device on the batch's stream into caller memory, exactly len bytes, not waited for;
 * both refuse cap < len and return the length otherwise (0 for an entry that is not OK), -1 on error.
 * jsnoop_export_jpeg: the single-image call beside jsnoop_export_tiff: the image a decoder holds, to a file; an image that is not OK
 * writes no file and returns -1 with the reason.                                                                                        */
#define JSNOOP_EXPORT_OK          0
#define JSNOOP_EXPORT_INEXACT     1
#define JSNOOP_EXPORT_UNCODABLE   2
#define JSNOOP_EXPORT_UNSUPPORTED 3
/* units of work of the export kernels (jsnoop_export.hip), for tests that place block counts and stream lengths at their seams */
#define JSNOOP_EXPORT_TILE   256u      /* blocks of one image a workgroup measures, and later writes the bits of, at a time */
#define JSNOOP_EXPORT_SCAN   256u      /* tiles (or stuffing chunks) of one image a prefix-sum step covers */
#define JSNOOP_EXPORT_CHUNK  4096u     /* bytes of the un-stuffed stream a workgroup stuffs at a time */
#define JSNOOP_EXPORT_WINDOW 8192u     /* bytes of LDS in which a workgroup assembles its bit range; what does not fit goes to memory bit group by bit group */
typedef struct JsnoopExportSpec { uint32_t struct_size; int32_t jfif; } JsnoopExportSpec;
void         jsnoop_export_spec_defaults(JsnoopExportSpec* out);                               /* jfif 1; NULL tolerated */
int          jsnoop_batch_export_jpeg(JsnoopBatch*, const JsnoopExportSpec*, const int* images, int n);
int          jsnoop_batch_export_count(const JsnoopBatch*);
int          jsnoop_batch_export_file(const JsnoopBatch*, int k, const void** dev_ptr, uint64_t* len, int* result, uint32_t* detail, int* image);
int64_t      jsnoop_batch_read_export(JsnoopBatch*, int k, void* host_dst, uint64_t cap);
int64_t      jsnoop_batch_export_copy(JsnoopBatch*, int k, void* dev_dst, uint64_t cap);
int          jsnoop_export_jpeg(JsnoopDecoder*, const char* path);
/* Huffman tables of the export.  jsnoop_batch_export_jpeg_coded is jsnoop_batch_export_jpeg with a second spec: huffman = JSNOOP_HUFFMAN_ANNEX_K
 * gives the same bytes; JSNOOP_HUFFMAN_OPTIMAL counts the Annex F symbols of every listed entry and builds its own tables on the device
 * (T.81 Annex K.2 per table: the reserved 257th symbol, on equal counts the largest symbol first, Adjust_BITS, symbols in the order of
 * (code size before the adjustment, symbol value)) and writes them in place of the Annex K ones: DHT DC0, AC0 (DC1, AC1), one segment
 * each, Lh = 19 + symbols.  Everything else of the file, the result words, `detail`, the two waits and the accessors above are unchanged;
 * tests/export_opt_model.py is the definition, byte for byte, DESIGN.md section 4.15 the contract.  In this mode alone an image of 2^26
 * blocks or more is JSNOOP_EXPORT_UNSUPPORTED (32-bit symbol counters).  struct_size is read like JsnoopExportSpec's; a huffman value
 * other than the two is refused.
 * jsnoop_batch_export_tables: entry k of the last export and slot 0..3 (2 x table id + class; a grey image has 0 and 1): the symbol counts
 * (freq[256], zero where the symbol did not occur) and the table that was written (counts per length 1..16, symbols in code order, *nsym
 * of them; the rest of symbols[256] zero), by one staged copy from the device on demand; any output pointer may be NULL.  -1 with a text
 * for an entry that is not OK, a slot the image does not have, and a last export with huffman = JSNOOP_HUFFMAN_ANNEX_K.
 * jsnoop_export_jpeg_coded: jsnoop_export_jpeg with a coding spec (NULL: the defaults).                                                  */
#define JSNOOP_HUFFMAN_ANNEX_K 0
#define JSNOOP_HUFFMAN_OPTIMAL 1
typedef struct JsnoopExportCoding { uint32_t struct_size; int32_t huffman; } JsnoopExportCoding;
void         jsnoop_export_coding_defaults(JsnoopExportCoding* out);                           /* huffman 0; NULL tolerated */
int          jsnoop_batch_export_jpeg_coded(JsnoopBatch*, const JsnoopExportSpec*, const JsnoopExportCoding*, const int* images, int n);
int          jsnoop_batch_export_tables(JsnoopBatch*, int k, int slot, uint8_t counts[16], uint8_t symbols[256], uint32_t* nsym, uint32_t freq[256]);
int          jsnoop_export_jpeg_coded(JsnoopDecoder*, const char* path, const JsnoopExportCoding*);
/* Restart intervals in the written files.  jsnoop_batch_export_jpeg_rst is jsnoop_batch_export_jpeg_coded with a third spec that gives every entry a
 * restart interval Ri in MCUs (tests/export_rst_model.py is the definition, byte for byte; DESIGN.md section 4.16 the contract).  Ri = 0 writes the
 * file of jsnoop_batch_export_jpeg_coded.  For Ri in 1 .. 65535: interval r holds MCUs [r Ri, min((r + 1) Ri, MCUs)) in decode order; the DC predecessor
 * of every component is 0 at the start of every interval (the first block of a component in an interval codes (int16)dccum[b] itself), so a restart can
 * make an image UNCODABLE or INEXACT that is OK without one (a cumulative DC level beyond +-2047, or a cumulative DC that wrapped int16 and is no multiple
 * of its multiplier any more) -- the result word says so, it is no error of the call; the header carries FF DD 00 04 Ri directly in front of SOS (behind
 * the last DHT, also when there is one interval only); every interval is coded on its own (padded with ones to a whole byte, every FF followed by 00) and
 * FF D0+(r & 7) stands between interval r and r + 1, never stuffed.  With JSNOOP_HUFFMAN_OPTIMAL the symbol counts are those of the levels above.
 *   JSNOOP_RESTART_NONE    no DRI, no markers (interval must be 0).
 *   JSNOOP_RESTART_MCUS    Ri = interval (1 .. 65535).
 *   JSNOOP_RESTART_ROWS    Ri = interval x the image's MCUs per MCU row (interval 1 .. 65535); an entry whose Ri comes out above 65535 is
 *                          JSNOOP_EXPORT_UNSUPPORTED (host arithmetic: nothing is launched for it, no other entry is disturbed).
 *   JSNOOP_RESTART_SOURCE  Ri = the interval the image was decoded with, 0 where it had none (interval must be 0).  For a progressive image this is what
 *                          the header walk recorded: the DRI in force when the walk ended.
 * struct_size is read like JsnoopExportSpec's; NULL coding or restart: the defaults.  Refused with -1 and a text, nothing launched: an unknown mode, an
 * interval of 0 or above 65535 with MCUS or ROWS, a non-zero interval with NONE or SOURCE, non-zero reserved.  Accessors, waits, ownership and
 * invalidation are those of jsnoop_batch_export_jpeg.  jsnoop_batch_export_restart: the Ri entry k of the last export was written with and the number of
 * intervals of its file (0 where no file was written); either pointer may be NULL.  jsnoop_export_jpeg_rst: jsnoop_export_jpeg_coded with a restart spec. */
#define JSNOOP_RESTART_NONE   0   /* no DRI, no markers: jsnoop_batch_export_jpeg_coded byte for byte            */
#define JSNOOP_RESTART_MCUS   1   /* Ri = interval                                                               */
#define JSNOOP_RESTART_ROWS   2   /* Ri = interval * mcu_xmax of the image (interval MCU rows)                   */
#define JSNOOP_RESTART_SOURCE 3   /* Ri = the image's own rst_interval when it was decoded with one, else 0      */
typedef struct JsnoopExportRestart { uint32_t struct_size; int32_t mode; uint32_t interval; uint32_t reserved; } JsnoopExportRestart;
void         jsnoop_export_restart_defaults(JsnoopExportRestart* out);                         /* NONE, 0; NULL tolerated */
int          jsnoop_batch_export_jpeg_rst(JsnoopBatch*, const JsnoopExportSpec*, const JsnoopExportCoding*, const JsnoopExportRestart*, const int* images, int n);
int          jsnoop_batch_export_restart(const JsnoopBatch*, int k, uint32_t* ri, uint64_t* intervals);   /* what entry k of the last export was written with */
int          jsnoop_export_jpeg_rst(JsnoopDecoder*, const char* path, const JsnoopExportCoding*, const JsnoopExportRestart*);
/* Progressive (SOF2) files.  jsnoop_batch_export_jpeg_prog is jsnoop_batch_export_jpeg_rst with a fourth spec: mode JSNOOP_PROGRESSIVE_OFF is that call byte for
 * byte and launch for launch; DEFAULT writes the built-in scan script, SCRIPT the caller's (tests/export_prog_model.py is the definition, byte for byte; DESIGN.md
 * section 4.17 has the contract, the rules of a script and the default scripts).  A script is a list of scans (components as a bit mask, Ss, Se, Ah, Al): DC scans
 * (Ss = Se = 0) with successive approximation, AC scans of one component by spectral selection (Ah = Al = 0).  AC successive approximation is not written: a
 * script that asks for it, or breaks any other rule, is refused with -1 and a text before anything is launched or cleared (the previous export stays valid), and
 * so are an unknown mode, SCRIPT with NULL scans or nscans of 0 or above JSNOOP_EXPORT_MAX_SCANS, OFF / DEFAULT with a script, non-zero reserved fields, comps
 * bits 3..7 and a longer struct.  Every scan carries its own optimal Huffman tables, built on the device from the scan's symbol counts: coding.huffman is
 * validated as before, but BOTH values write own tables in a progressive mode, because Annex K has no codes for the end-of-band runs EOBn.
 * The restart spec counts in every scan's own units: MCUS n is Ri = n in every scan, ROWS r is Ri = r x the scan's units per row (mcu_xmax of an interleaved
 * scan, the width in blocks of the component's coded part in a one-component scan), SOURCE the image's recorded interval as MCUS.  DRI stands in front of the SOS
 * of every scan whose Ri differs from the one in force.  An entry whose component count differs from the script's, with a precision other than 8, with an Ri above
 * 65535 in some scan, or with 2^26 blocks or more is JSNOOP_EXPORT_UNSUPPORTED (host arithmetic; the other entries are written).  DC levels are the ABSOLUTE
 * values (int16)dccum / q[0] (a remainder is INEXACT), coded as differences of their point transforms inside every restart interval (beyond +-2047: UNCODABLE).
 * jsnoop_batch_export_file, _read_export, _export_copy, _export_count, ownership and invalidation are jsnoop_batch_export_jpeg's; jsnoop_batch_export_restart
 * returns the FIRST scan's values on a progressive entry; jsnoop_batch_export_tables refuses one (jsnoop_batch_export_scan_tables is its call).
 * jsnoop_batch_export_scan_count: the scans entry k was written with (0 for a baseline or absent file).  jsnoop_batch_export_scan_info: scan `scan` of entry k --
 * the script's scan, its Ri in its own units, its intervals, where its SOS marker stands in the file and the bytes of its entropy-coded data (stuffing and RSTn
 * included); any output pointer may be NULL.  jsnoop_batch_export_scan_tables: table `slot` of that scan (a DC first scan: one per scan component, in the scan's
 * order; an AC scan: slot 0; a refinement scan has none) as jsnoop_batch_export_tables returns a table.  jsnoop_export_jpeg_prog: jsnoop_export_jpeg_rst with a
 * progressive spec.  The call waits for the device twice, as every export does. */
#define JSNOOP_PROGRESSIVE_OFF     0
#define JSNOOP_PROGRESSIVE_DEFAULT 1
#define JSNOOP_PROGRESSIVE_SCRIPT  2
#define JSNOOP_EXPORT_MAX_SCANS    256u
typedef struct JsnoopExportScan { uint8_t comps /* bit c = component c */, ss, se, ah, al, reserved[3]; } JsnoopExportScan;
typedef struct JsnoopExportProgressive { uint32_t struct_size; int32_t mode; uint32_t nscans; uint32_t reserved; const JsnoopExportScan* scans; } JsnoopExportProgressive;
void         jsnoop_export_progressive_defaults(JsnoopExportProgressive* out);                 /* OFF; NULL tolerated */
int          jsnoop_batch_export_jpeg_prog(JsnoopBatch*, const JsnoopExportSpec*, const JsnoopExportCoding*, const JsnoopExportRestart*, const JsnoopExportProgressive*, const int* images, int n);
int          jsnoop_batch_export_scan_count(const JsnoopBatch*, int k);
int          jsnoop_batch_export_scan_info(const JsnoopBatch*, int k, int scan, JsnoopExportScan* sc, uint32_t* ri, uint64_t* intervals, uint64_t* sos_offset, uint64_t* data_bytes);
int          jsnoop_batch_export_scan_tables(JsnoopBatch*, int k, int scan, int slot, uint8_t counts[16], uint8_t symbols[256], uint32_t* nsym, uint32_t freq[256]);
int          jsnoop_export_jpeg_prog(JsnoopDecoder*, const char* path, const JsnoopExportCoding*, const JsnoopExportRestart*, const JsnoopExportProgressive*);

/* ---- encode: pixels in device memory to JPEG files, on the device ---------------------------------------------------------------------------
 * The forward path in front of the export: colour conversion, chroma downsampling, forward DCT and quantisation of 8-bit pictures that lie in
 * device memory -- what jsnoop_batch_pack wrote, a batch's own DIB, any tensor -- into a coefficient arena and a cumulative-DC array of the form a
 * decode leaves, which the export above then writes as files, unchanged.  The arithmetic is libjpeg's integer path ("islow" DCT), exactly:
 * tests/encode_model.py is the definition, value for value; DESIGN.md section 4.18 has the contract (colour constants, padding and downsampling rules,
 * the quantiser's rounding, the dummy-block rule).
 *
 * A JsnoopEncode owns its arena, its export memory and (unless the caller passes one) its stream; it lives on the device that was current when it
 * was created.  jsnoop_encode_run encodes n pictures in ONE launch on that stream, waits for nothing, and replaces what the object held:
 * picture i of the call is image i of the object until the next successful run.  A picture has 1 channel (grey: one component, 1 x 1) or 3; the
 * spec applies to the whole call:
 *   subsampling  JSNOOP_ENCODE_444 / _422 / _420: luma H x V = 1x1 / 2x1 / 2x2, chroma 1 x 1 (a grey picture ignores it).
 *   qtables      NULL: the tables come from `quality` (1..100): scale = quality < 50 ? 5000 / quality : 200 - 2 quality,
 *                v = clamp((base * scale + 50) / 100, 1, 255) over T.81 Tables K.1 / K.2.  Else 128 bytes, luma[64] then chroma[64], natural
 *                order, every value 1..255, taken as they are (quality is then not read).  jsnoop_encode_qtables: the tables a spec comes to.
 * A source: sample (x, y) of channel c lies at ptr + y' * row_pitch + x * pixel_stride + c' (INTERLEAVED) or ptr + c' * plane_pitch + y' * row_pitch +
 * x * pixel_stride (PLANAR); c' = c for JSNOOP_ENCODE_RGB and 2 - c for _BGR (a grey picture: 0); y' = y, or height - 1 - y with bottom_up (a DIB:
 * INTERLEAVED, BGR, pixel_stride 4, bottom_up 1).  0 stands for the dense value of pixel_stride (channels, or 1 when PLANAR), row_pitch
 * (width * pixel_stride) and plane_pitch (height * row_pitch).  Any byte alignment is accepted.  Only addressed bytes are read.
 *
 * What a run leaves: arena rows [blocks][64] int16 in decode order, natural order inside a row, slot n = level * q[n], slot 0 = 0; dccum[b] = DC
 * level * q[0].  No product wraps (|value| < 1154).  jsnoop_encode_image_info returns the words of jsnoop_batch_image_info; jsnoop_encode_read_coefs
 * copies up to max_blocks rows and dccum values to the host (waits; either pointer may be NULL) and returns the number copied.
 * jsnoop_encode_export is jsnoop_batch_export_jpeg_prog on the encoded arena: every mode, result word and limit of that call (NULL coding, restart
 * or progressive: the defaults; JSNOOP_RESTART_SOURCE finds no interval); jsnoop_encode_export_count, _export_file, _read_export, _export_copy,
 * _export_scan_count and _export_scan_info are the batch calls of the same name.  The files stay valid until the next export, run or destroy.
 *
 * Refused with -1 + jsnoop_last_error(), nothing launched, the previous result untouched: a NULL object, spec or (n > 0) source list; n < 0; a
 * struct_size that is too small or larger than this library's (read like JsnoopPackSpec's); quality outside 1..100 without tables; a table value
 * of 0; an unknown subsampling, layout or order; non-zero reserved fields; a NULL ptr; width or height outside 1..65535; channels other than 1 or
 * 3; a pixel_stride below the channel count (1 when PLANAR), a row_pitch below width * pixel_stride, a plane_pitch below height * row_pitch;
 * bottom_up other than 0 / 1; 2^31 units of work or more in one call.  An export refuses, before it touches the previous export, what
 * jsnoop_batch_export_jpeg_prog refuses, an object that has not run, and an image index out of range.                                        */
#define JSNOOP_ENCODE_444         0
#define JSNOOP_ENCODE_422         1
#define JSNOOP_ENCODE_420         2
#define JSNOOP_ENCODE_INTERLEAVED 0
#define JSNOOP_ENCODE_PLANAR      1
#define JSNOOP_ENCODE_RGB         0
#define JSNOOP_ENCODE_BGR         1
#define JSNOOP_ENCODE_RUN         8u       /* MCUs of one MCU row a wave encodes at a time (k_encode), for tests that place widths at its seams */
typedef struct JsnoopEncode JsnoopEncode;
typedef struct JsnoopEncodeSpec { uint32_t struct_size; int32_t quality, subsampling; uint32_t reserved; const uint8_t* qtables; } JsnoopEncodeSpec;
typedef struct JsnoopEncodeSrc  { const void* ptr; uint32_t width, height, channels; int32_t layout, order; uint32_t pixel_stride; uint64_t row_pitch, plane_pitch;
                                  uint32_t bottom_up, reserved; } JsnoopEncodeSrc;                 /* device pointer; pitches in bytes, 0 = dense */
JsnoopEncode* jsnoop_encode_create(void* stream);                                                 /* NULL stream: a stream of its own */
void         jsnoop_encode_destroy(JsnoopEncode*);
void         jsnoop_encode_spec_defaults(JsnoopEncodeSpec* out);                                   /* quality 75, 4:2:0, no tables; NULL tolerated */
int          jsnoop_encode_qtables(const JsnoopEncodeSpec*, uint8_t luma64[64], uint8_t chroma64[64]);   /* host arithmetic, natural order; 0 / -1 */
int          jsnoop_encode_run(JsnoopEncode*, const JsnoopEncodeSpec*, const JsnoopEncodeSrc* src, int n);
int          jsnoop_encode_count(const JsnoopEncode*);
int          jsnoop_encode_image_info(const JsnoopEncode*, int i, unsigned* out16);
int          jsnoop_encode_read_coefs(JsnoopEncode*, int i, int16_t* coefs, int16_t* dccum, size_t max_blocks);
int          jsnoop_encode_export(JsnoopEncode*, const JsnoopExportSpec*, const JsnoopExportCoding*, const JsnoopExportRestart*, const JsnoopExportProgressive*, const int* images, int n);
int          jsnoop_encode_export_count(const JsnoopEncode*);
int          jsnoop_encode_export_file(const JsnoopEncode*, int k, const void** dev_ptr, uint64_t* len, int* result, uint32_t* detail, int* image);
int64_t      jsnoop_encode_read_export(JsnoopEncode*, int k, void* host_dst, uint64_t cap);
int64_t      jsnoop_encode_export_copy(JsnoopEncode*, int k, void* dev_dst, uint64_t cap);
int          jsnoop_encode_export_scan_count(const JsnoopEncode*, int k);
int          jsnoop_encode_export_scan_info(const JsnoopEncode*, int k, int scan, JsnoopExportScan* sc, uint32_t* ri, uint64_t* intervals, uint64_t* sos_offset, uint64_t* data_bytes);

/* ---- transform: flip, rotate, transpose, crop and grayscale of a decoded batch without a second quantisation, on the device -----------------------
 * jpegtran's lossless transforms: the DCT blocks of every listed image are rearranged (and their cells transposed and sign-changed) into a coefficient
 * arena and a cumulative-DC array of the form a decode leaves, which the export above then writes as files, unchanged.  No cell is interpreted, none is
 * quantised again.  tests/transform_model.py is the definition, value for value; DESIGN.md section 4.19 has the contract (grayscale, crop, edge, block
 * map and signs, descriptor).
 *
 * A JsnoopTransform owns its arena, its export memory and (unless the caller passes one) its stream; it lives on the device that was current when it
 * was created.  jsnoop_transform_run transforms n images of `src` (images == NULL: images 0 .. n - 1) in ONE launch on the object's stream, waits for
 * nothing on the host, and replaces what the object held.  Where the object's stream is not the source batch's, the launch goes behind an event
 * recorded on the source batch's stream.  The source needs what jsnoop_batch_pack_coefs needs: decoded, and ensure_generic() after a DC-only fast
 * decode (the call makes it, as the pack does: that decode is waited for).  Baseline and progressive batches are both accepted.  The caller leaves the
 * source batch's arena alone (no decode, clear, upload or destroy) until the object's stream has passed the run.  What the arena holds when the
 * kernel runs is what is transformed: an image the parallel path flagged is final only behind jsnoop_batch_sync (a damaged file then arrives as repaired).
 *
 * The spec applies to the whole call; per entry, in this order, in source coordinates (the source MCU is mw = 8 Hmax by mh = 8 Vmax):
 *   grayscale 1  a three-component source keeps component 0 alone: one component, 1 x 1, ceil(W / 8) x ceil(H / 8) blocks, mw = mh = 8 from here on.
 *   crop 1       jpegtran's rule: the offset goes down to the MCU grid (x0 = crop_x - crop_x % mw), the size grows by what the offset lost and is
 *                clipped to the picture.  A rectangle that starts outside the picture: JSNOOP_XFORM_EMPTY.
 *   edge         an op that reverses the source's x axis (FLIP_H, ROT_180, TRANSVERSE, ROT_270) needs the width to be a multiple of mw, one that
 *                reverses y (FLIP_V, ROT_180, TRANSVERSE, ROT_90) the height a multiple of mh.  JSNOOP_XFORM_EDGE_TRIM cuts the dimension down to whole
 *                MCUs from the origin (below one MCU: EMPTY); _EDGE_PERFECT makes the entry JSNOOP_XFORM_IMPERFECT instead.
 * jsnoop_transform_entry: entry k's result word and its image in the object (-1 where the entry is not OK: it has none; the others are written, in the
 * order of the call).  JSNOOP_XFORM_UNSUPPORTED: a source whose component count is neither 1 nor 3.  The four transposing ops swap width and height,
 * H and V of every component, and transpose every quantiser table; precision is the source's; no restart interval is recorded.
 *
 * jsnoop_transform_image_info, _image_dqt and _read_coefs are jsnoop_batch_image_info, jsnoop_batch_image_dqt and jsnoop_encode_read_coefs on the
 * object's images; jsnoop_transform_export is jsnoop_batch_export_jpeg_prog on the object's arena, and _export_count, _export_file, _read_export,
 * _export_copy, _export_scan_count and _export_scan_info are the batch calls of the same name.  The files stay valid until the next export, run or destroy.
 *
 * Refused with -1 + jsnoop_last_error(), nothing launched, the previous result untouched: a NULL object, batch or spec; n < 0, or an index out of
 * range; an unknown op or edge; grayscale or crop other than 0 / 1; crop fields set while crop = 0; crop_w or crop_h of 0; non-zero reserved; a
 * struct_size that is too small or larger than this library's (read like JsnoopPackSpec's); a source that is not decoded; 2^31 or more blocks in one
 * call.                                                                                                                                        */
#define JSNOOP_XFORM_NONE         0        /* libjpeg's JXFORM codes */
#define JSNOOP_XFORM_FLIP_H       1
#define JSNOOP_XFORM_FLIP_V       2
#define JSNOOP_XFORM_TRANSPOSE    3
#define JSNOOP_XFORM_TRANSVERSE   4
#define JSNOOP_XFORM_ROT_90       5        /* clockwise */
#define JSNOOP_XFORM_ROT_180      6
#define JSNOOP_XFORM_ROT_270      7
#define JSNOOP_XFORM_EDGE_TRIM    0
#define JSNOOP_XFORM_EDGE_PERFECT 1
#define JSNOOP_XFORM_OK           0
#define JSNOOP_XFORM_IMPERFECT    1
#define JSNOOP_XFORM_EMPTY        2
#define JSNOOP_XFORM_UNSUPPORTED  3
#define JSNOOP_TRANSFORM_RUN      8u       /* destination blocks a wave moves at a time (k_transform), for tests that place pictures at its seams */
typedef struct JsnoopTransform JsnoopTransform;
typedef struct JsnoopTransformSpec { uint32_t struct_size; int32_t op, edge; uint32_t grayscale, crop, crop_x, crop_y, crop_w, crop_h, reserved; } JsnoopTransformSpec;
void*        jsnoop_batch_stream(const JsnoopBatch*);                                             /* the hipStream_t the batch enqueues on (its own or the caller's), to create a transform object on it */
JsnoopTransform* jsnoop_transform_create(void* stream);                                           /* NULL stream: a stream of its own */
void         jsnoop_transform_destroy(JsnoopTransform*);
void         jsnoop_transform_spec_defaults(JsnoopTransformSpec* out);                            /* NONE, TRIM, no crop; NULL tolerated */
int          jsnoop_transform_run(JsnoopTransform*, JsnoopBatch* src, const JsnoopTransformSpec*, const int* images, int n);
int          jsnoop_transform_entry(const JsnoopTransform*, int k, int* result, int* image);      /* image: index in the object, -1 where none */
int          jsnoop_transform_entry_count(const JsnoopTransform*);                                /* entries of the last run */
int          jsnoop_transform_count(const JsnoopTransform*);                                      /* images the object holds */
int          jsnoop_transform_image_info(const JsnoopTransform*, int i, unsigned* out16);
int          jsnoop_transform_image_dqt(const JsnoopTransform*, int i, int comp, uint16_t* out64);
int          jsnoop_transform_read_coefs(JsnoopTransform*, int i, int16_t* coefs, int16_t* dccum, size_t max_blocks);
int          jsnoop_transform_export(JsnoopTransform*, const JsnoopExportSpec*, const JsnoopExportCoding*, const JsnoopExportRestart*, const JsnoopExportProgressive*, const int* images, int n);
int          jsnoop_transform_export_count(const JsnoopTransform*);
int          jsnoop_transform_export_file(const JsnoopTransform*, int k, const void** dev_ptr, uint64_t* len, int* result, uint32_t* detail, int* image);
int64_t      jsnoop_transform_read_export(JsnoopTransform*, int k, void* host_dst, uint64_t cap);
int64_t      jsnoop_transform_export_copy(JsnoopTransform*, int k, void* dev_dst, uint64_t cap);
int          jsnoop_transform_export_scan_count(const JsnoopTransform*, int k);
int          jsnoop_transform_export_scan_info(const JsnoopTransform*, int k, int scan, JsnoopExportScan* sc, uint32_t* ri, uint64_t* intervals, uint64_t* sos_offset, uint64_t* data_bytes);

/* ---- staging pipeline: the CwindowBuf replacement at batch scale (source/WindowBuf.cpp:351-416 BufLoadWindow, :639-714 Buf) ----
 * `slots` batch slots, each with its own pinned staging area, HBM arenas and stream (fill them through jsnoop_pipeline_slot and
 * the jsnoop_batch_add* calls).  jsnoop_pipeline_run cycles `batches` batches through the slots: while one slot decodes, the next
 * slot's compressed bytes cross PCIe, and with d2h != 0 the previous slot's DIBs are copied back to pinned host memory meanwhile.
 * out_ms6: [0] wall ms per batch in steady state (timing scope T2 with d2h = 0, T3 with d2h = 1), then the pieces on their own:
 * [1] H2D ms, [2] decode ms (T1), [3] D2H ms (0 without d2h), [4] compressed bytes per batch, [5] DIB bytes per batch.       */
typedef struct JsnoopPipeline JsnoopPipeline;
JsnoopPipeline* jsnoop_pipeline_create(int slots);
void            jsnoop_pipeline_destroy(JsnoopPipeline*);
JsnoopBatch*    jsnoop_pipeline_slot(JsnoopPipeline*, int i);
int             jsnoop_pipeline_run(JsnoopPipeline*, int batches, int d2h, double* out_ms6);

/* ---- job: one call decodes a mixed file list over all devices --------------------------------------------------------------------
 * The reference's batch loop on the whole node: CJPEGsnoopCore::GenBatchFileList (source/JPEGsnoopCore.cpp:454) builds a file list and
 * DoBatchFileProcess (:765-845) works through it one file at a time, every file with a freshly reset decoder (CjfifDecode::Reset,
 * source/JfifDecode.cpp:7306-7308) -- files are independent, so the list shards with no exchange between devices.  A job takes files of
 * any kind the library decodes (baseline and progressive side by side), spreads them over shards -- one host thread with its own
 * batches per shard, a shard bound to one device; a device may carry several shards -- and decodes each shard in memory-bounded
 * rounds.  Every file gets a result; a file never fails the job:
 *   - what jsnoop_batch_add_jpeg / _add_progressive refuses (not a JPEG, SOF3, four components ...) is JSNOOP_JOB_REFUSED with the text
 *     jsnoop_last_error() held on the worker thread; the reference's loop notes such a file and moves on;
 *   - a path that cannot be opened is JSNOOP_JOB_UNREADABLE (the reference returns silently there, :794-798).
 * A file's pixels, flags, path and log are those of the same file alone in a plain JsnoopBatch, whatever the number of shards, rounds
 * or partition rule.
 *
 * Rounds: a shard fills a round until max_images_per_round is reached or jsnoop_batch_device_bytes of the round's two batches (one
 * baseline, one progressive, decoded on their own streams) would pass max_round_bytes; an image larger than the budget goes alone in a
 * round, it is never refused for size.  Each shard has two round slots: reading, header walk, pinned copy and H2D of round r + 1
 * overlap decode and callbacks of round r.  max_round_bytes = 0 takes HALF of the free HBM hipMemGetInfo reports for the device when
 * jsnoop_job_run starts, divided by the shards on that device and by the two slots.  The half is a choice, not a measurement: it leaves
 * room for the scratch jsnoop_batch_device_bytes does not count and for other users of the device.
 *
 * Threading: jsnoop_job_* calls on one job come from one thread.  on_file is called on the thread that called jsnoop_job_run, one call
 * at a time; workers hand finished rounds over through a queue, and a batch handed over is not touched by its worker until the callbacks
 * for its files have returned (the one-thread-per-handle rule above holds for `batch`).  Files of one round arrive in index order;
 * rounds of different shards arrive as they finish.
 *
 * Failure: the first HIP error on any shard cancels the job -- no shard starts another launch, nothing is retried, jsnoop_job_run
 * returns -1 and jsnoop_last_error() carries the text.  The multi-device path has been exercised with several shards on one device only. */
typedef struct JsnoopJob JsnoopJob;
#define JSNOOP_JOB_MAX_SHARDS 16
#define JSNOOP_JOB_PENDING    (-1)   /* no result (before jsnoop_job_run, or behind a cancelled / failed run) */
#define JSNOOP_JOB_OK           0
#define JSNOOP_JOB_REFUSED      1
#define JSNOOP_JOB_UNREADABLE   2
typedef struct JsnoopJobOptions {
    uint32_t struct_size;           /* sizeof(JsnoopJobOptions) of the caller, read like JsnoopTuning's: shorter is accepted, longer is refused */
    int32_t  decode_ac;             /* as jsnoop_batch_set_options (default 1)                                                          */
    int32_t  want_planes;           /* keep the int16 planes (default 0)                                                                */
    int32_t  enable_log;            /* jsnoop_batch_enable_log on every batch: jsnoop_batch_log works from inside the callback (default 0) */
    int32_t  max_images_per_round;  /* 0 = 1024                                                                                         */
    uint64_t max_round_bytes;       /* HBM budget of one round of one shard; 0 = automatic (above)                                       */
    int32_t  partition;             /* 0 = longest-processing-time by file bytes (jsnoop_partition_lpt), 1 = contiguous index ranges    */
    int32_t  keep_resident;         /* 1: one round per shard, and every result's batch / image stay valid until jsnoop_job_clear / _destroy:
                                       N DIBs resident across the devices.  jsnoop_job_run returns -1 before any decode if a shard needs more rounds */
} JsnoopJobOptions;
typedef struct JsnoopJobFile {
    uint32_t struct_size;           /* jsnoop_job_file_result: set to sizeof(your JsnoopJobFile) (or 0: this header's); no byte past it is written */
    int32_t  index;                 /* what jsnoop_job_add_file / _add_path returned                                                     */
    int32_t  status;                /* JSNOOP_JOB_*                                                                                      */
    int32_t  kind;                  /* 1 baseline, 2 progressive, 0 unknown (refused / unreadable)                                       */
    int32_t  shard, device, round;  /* where and when it was decoded (round counts per shard from 0)                                     */
    int32_t  image;                 /* index in `batch`                                                                                  */
    JsnoopBatch* batch;             /* valid during the callback (with keep_resident: until clear / destroy), NULL otherwise.  Every per-image
                                       jsnoop_batch_* call works on (batch, image): read_dib, dib_dev, log, side_outputs, export_tiff, color_stats */
    uint32_t info16[16];            /* as jsnoop_batch_image_info                                                                        */
    uint64_t dib_hash;              /* the word jsnoop_batch_dib_hashes gives for this image                                             */
    const char* message;            /* "" or why the file was refused / unreadable; owned by the job, valid until clear / destroy / the next run */
} JsnoopJobFile;
typedef struct JsnoopJobStats {
    uint32_t struct_size;           /* set by the caller like JsnoopJobFile's                                                            */
    int32_t  files, ok, refused, unreadable;   /* files reported; ok + refused + unreadable == files                                     */
    int32_t  flagged;               /* decoded files with any JSNOOP_FLAG_* raised                                                       */
    int32_t  rounds;                /* rounds decoded, all shards                                                                        */
    int32_t  nshards;
    uint64_t pixels;                /* sum(SOF X*Y) of the decoded files                                                                 */
    uint64_t dib_hash_sum;          /* sum of dib_hash mod 2^64: the same for every partition                                            */
    uint64_t max_round_device_bytes;/* largest jsnoop_batch_device_bytes of a round's two batches                                        */
    double   wall_ms;               /* jsnoop_job_run, start to return                                                                   */
    double   shard_ms[JSNOOP_JOB_MAX_SHARDS];  /* busy time of each shard's thread                                                       */
} JsnoopJobStats;
/* The greedy longest-processing-time rule on its own (host only, no device needed): files in the order (cost descending, index ascending),
 * each into the part with the least load so far, ties to the lowest part.  part_of[i] = part of file i.  0, or -1 for a bad argument.     */
int        jsnoop_partition_lpt(const uint64_t* costs, int n, int parts, int* part_of);
/* devices / nshards: the device of every shard (a device may be named more than once: logical shards on one GPU); NULL, 0 = one shard
 * per visible device.  At most JSNOOP_JOB_MAX_SHARDS.  NULL + jsnoop_last_error() without a device (no CPU fallback) or on a bad list.  */
JsnoopJob* jsnoop_job_create(const int* devices, int nshards);
void       jsnoop_job_destroy(JsnoopJob*);
void       jsnoop_job_options_defaults(JsnoopJobOptions* out);
int        jsnoop_job_set_options(JsnoopJob*, const JsnoopJobOptions*);
int        jsnoop_job_set_tuning(JsnoopJob*, const JsnoopTuning*);          /* handed to every batch the job creates                    */
int        jsnoop_job_add_file(JsnoopJob*, const uint8_t* file, size_t len); /* bytes copied; returns the file index; content is not judged here */
int        jsnoop_job_add_path(JsnoopJob*, const char* path);               /* read by the shard that owns it, in the round that decodes it */
int        jsnoop_job_count(const JsnoopJob*);
void       jsnoop_job_clear(JsnoopJob*);                                    /* drops files, results and resident batches                */
typedef int (*jsnoop_job_file_fn)(void* user, const JsnoopJobFile* f);      /* non-zero return cancels the job                          */
/* 0 = every file reported, 1 = cancelled by the callback (later files stay JSNOOP_JOB_PENDING), -1 = error.  on_file and stats may be NULL. */
int        jsnoop_job_run(JsnoopJob*, jsnoop_job_file_fn on_file, void* user, JsnoopJobStats* stats);
int        jsnoop_job_file_result(const JsnoopJob*, int index, JsnoopJobFile* out);

/* ---- carve: every embedded JPEG of a byte blob, found and walked on the device ------------------------------------------------------
 * The other half of the reference's batch loop: "extract all" (-ext_all / bExtractAll of DoBatchFileProcess, source/JPEGsnoopCore.cpp:765-845;
 * DoExtractEmbeddedJPEG :906-1091) takes any file -- a Motion-JPEG AVI, a RAW with previews, a JPEG with an EXIF thumbnail, a dump -- finds every
 * FF D8 FF in it and walks the markers of each hit to its EOI; the search restarts one byte behind the previous START (:1063-1066), so nested
 * thumbnails are frames of their own.  jsnoop_carve_run does that for a whole blob at once and leaves a table of frames; the frames go into a
 * job through jsnoop_job_add_carved.  tests/carve_model.py is the definition; DESIGN.md section 4.14 has the contract and its reasons.
 *
 * The contract is structural: marker codes and segment lengths as CjfifDecode::DecodeMarker reads them in its strict mode, no segment's content.
 * The blob is b[0..n), B(i) = b[i] for i < n and 0 past the end; n < 2^32.
 *   terminator  i < n with b[i] = FF and B(i + 1) not 00 and not D0..D7 (what ends the skip over scan data).
 *   candidate   p with b[p..p+3) = FF D8 FF and p + 3 <= n.  Every candidate gets a frame record; frames come in ascending start.
 *   walk        from the candidate, marker by marker (fill bytes FF skipped): SOI goes on; EOI ends the frame (OK with a scan, NO_SOS without);
 *               RST0-7 outside a scan, a code 00 / 02..BF, a byte that is not FF where a marker belongs and a length below 2 STOP it; C0..CF,
 *               DA..FE and 01 are segments with a big-endian length; a segment or a fill run passing the end of the blob is NO_EOI; behind an SOS
 *               segment the walk goes on at the next terminator (none: NO_EOI); more than max_markers markers is LIMIT.
 * A frame: start; end (one past the EOI; n for NO_EOI; the detail position for STOPPED and LIMIT); status; for STOPPED the reason, for STOPPED and LIMIT
 * the position and the byte found there (NOT_A_MARKER: the byte; RST_OUTSIDE_SCAN, UNKNOWN_MARKER and LIMIT: the marker code, at its own position;
 * BAD_LENGTH: the length, at the length field); seen (JSNOOP_CARVE_SEEN_*); of the first SOFn (C0-C3, C5-C7, C9-CB, CD-CF) its code, precision, height,
 * width and component count (0 without one); sos_pos (the FF of the first SOS), scan_start (behind its segment), scans, markers; parent: the
 * innermost earlier frame with status OK whose [start, end) holds this frame's start, or -1 -- what tells a thumbnail from the next video frame.
 *
 * jsnoop_carve_run: where = 0, blob is host memory and goes to the device through page-locked staging; where = 1, blob is memory of the carve's
 * device, read in place (any alignment).  Two waits: the totals of terminators and candidates come back and size the lists, then the records
 * come back.  Lists and records (4 bytes per terminator, 68 per candidate), the tile counts and for where = 0 the blob's copy are the scratch;
 * above max_scratch_bytes (0 = half of the device's free memory) the call is refused with a text before any of it is allocated beyond the counts.
 * -1 + jsnoop_last_error(): a NULL carve, spec or (with len > 0) blob, len >= 2^32, a bad struct_size (read like JsnoopTuning's), a where
 * other than 0 / 1, scratch over budget, a device error.  A refused call leaves the last table as it was.  max_markers = 0 means 4096.
 * A fill run is walked byte by byte: a blob of FF D8 followed by megabytes of FF costs one lane that many steps.
 * jsnoop_carve_host: the same table on the host alone, no device needed: the number of frames (frames[0 .. min(count, cap)) written), or -1.  */
typedef struct JsnoopCarve JsnoopCarve;
#define JSNOOP_CARVE_OK       0
#define JSNOOP_CARVE_NO_SOS   1
#define JSNOOP_CARVE_NO_EOI   2
#define JSNOOP_CARVE_STOPPED  3
#define JSNOOP_CARVE_LIMIT    4
#define JSNOOP_CARVE_NOT_A_MARKER      1
#define JSNOOP_CARVE_RST_OUTSIDE_SCAN  2
#define JSNOOP_CARVE_BAD_LENGTH        3
#define JSNOOP_CARVE_UNKNOWN_MARKER    4
#define JSNOOP_CARVE_SEEN_SOI_AGAIN 1u
#define JSNOOP_CARVE_SEEN_DQT       2u
#define JSNOOP_CARVE_SEEN_DHT       4u
#define JSNOOP_CARVE_SEEN_DRI       8u
#define JSNOOP_CARVE_SEEN_AVI1      16u
/* units of work of the carve kernels (jsnoop_carve.hip), for tests that slide patterns across their seams */
#define JSNOOP_CARVE_LANE   16u        /* bytes a lane classifies at a time, one 16-byte load */
#define JSNOOP_CARVE_WAVE   1024u      /* ... and a wave: 64 lanes */
#define JSNOOP_CARVE_TILE   16384u     /* bytes of a workgroup's tile: 4 waves, 4 loads a lane; tiles start at multiples of it counted from the 16-byte boundary at or below the blob */
#define JSNOOP_CARVE_WALK   256u       /* candidates of one workgroup of the walk kernel, one a lane */
#define JSNOOP_CARVE_REC_WORDS 16u     /* words of a record in device memory (jsnoop_carve_frames_dev): start, end, status | reason << 8 | byte << 16 | seen << 24,
                                          detail position, sof_code | precision << 8 | components << 16, width | height << 16, sos_pos, scan_start, scans, markers, 6 x 0 */
typedef struct JsnoopCarveSpec { uint32_t struct_size; uint32_t max_markers; uint64_t max_scratch_bytes; } JsnoopCarveSpec;
typedef struct JsnoopCarveFrame {
    uint32_t struct_size;           /* jsnoop_carve_frame: set to sizeof(your JsnoopCarveFrame) (or 0: this header's); no byte past it is written */
    uint32_t start, end;
    int32_t  status, reason;        /* JSNOOP_CARVE_*; reason 0 unless STOPPED */
    uint32_t detail_pos, detail_byte;
    uint32_t seen;
    uint32_t sof_code, precision, width, height, components;
    uint32_t sos_pos, scan_start, scans, markers;
    int32_t  parent;
} JsnoopCarveFrame;
JsnoopCarve* jsnoop_carve_create(int device);                                   /* NULL + jsnoop_last_error() without that device */
void         jsnoop_carve_destroy(JsnoopCarve*);
void         jsnoop_carve_spec_defaults(JsnoopCarveSpec* out);                  /* max_markers 4096, max_scratch_bytes 0; NULL tolerated */
int          jsnoop_carve_run(JsnoopCarve*, const JsnoopCarveSpec*, const void* blob, uint64_t len, int where);
int64_t      jsnoop_carve_host(const JsnoopCarveSpec*, const void* blob, uint64_t len, JsnoopCarveFrame* frames, uint64_t cap);
int64_t      jsnoop_carve_count(const JsnoopCarve*);                            /* frames of the last run */
int          jsnoop_carve_frame(const JsnoopCarve*, int64_t k, JsnoopCarveFrame* out);
int64_t      jsnoop_carve_frames(const JsnoopCarve*, JsnoopCarveFrame* out, uint64_t cap);   /* this header's struct, struct_size set; returns how many were written */
const void*  jsnoop_carve_frames_dev(const JsnoopCarve*);                       /* count x JSNOOP_CARVE_REC_WORDS words in device memory (no parent); valid until the next run / destroy */
int          jsnoop_carve_lists_dev(const JsnoopCarve*, const uint32_t** terminators, const uint32_t** candidates);   /* the two ascending position lists, device memory */
int          jsnoop_carve_totals(const JsnoopCarve*, uint64_t* terminators, uint64_t* candidates);
/* what = 0 the records, 1 the terminator list, 2 the candidate list: copied device-to-device into caller memory of the carve's device and waited for.
 * Returns the bytes copied (0 for an empty one); -1: a NULL carve or destination, an unknown `what`, cap below the size, a device error.             */
int64_t      jsnoop_carve_copy(JsnoopCarve*, int what, void* dev_dst, uint64_t cap);
/* Adds blob[start, end) of every frame with status OK (and NO_EOI if include_no_eoi) to the job, each with the copy jsnoop_job_add_file makes, in table order.
 * Returns how many it added, *first_index (may be NULL) = the file index of the first (-1: none); -1 on a bad argument or a frame outside the blob, nothing added. */
int          jsnoop_job_add_carved(JsnoopJob*, const uint8_t* blob, uint64_t len, const JsnoopCarveFrame* frames, int64_t nframes, int include_no_eoi, int* first_index);

#ifdef __cplusplus
}
#endif
#endif
