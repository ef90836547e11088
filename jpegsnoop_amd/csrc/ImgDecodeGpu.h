// ImgDecodeGpu.h -- the reference's scan-decoder interface on top of the C ABI (include/jsnoop_gpu.h).
//
// `CimgDecodeGpu` keeps the public method names, argument meaning and return conventions of the
// reference's `CimgDecode` (reference source/ImgDecode.h:286-356, :384-385, :407-425) for the
// scan-decode path, so that `CjfifDecode` / `CJPEGsnoopCore` code that drives a `CimgDecode*` can be
// pointed at this class (INTEGRATION.md shows the two-line change).  `CJPEGsnoopCoreGpu` carries the
// `I_*` pass-throughs of `CJPEGsnoopCore` (source/JPEGsnoopCore.h:79-117) that belong to this path,
// plus the batched submit that replaces the sequential DoBatchFileProcess loop
// (source/JPEGsnoopCore.cpp:765-845).
//
// Header-only, no MFC: CString/CDocLog/CwindowBuf are replaced by std::string, a log callback and a
// (pointer, length) view of the file bytes.  Everything below is a thin forwarding layer; the work
// happens in libjsnoop_gpu.so on the GPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <filesystem>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/jsnoop_gpu.h"

// What CwindowBuf hands the decoder: the whole file image (overlays already applied by the caller).
struct CwindowBufView {
    const uint8_t* pData = nullptr; size_t nLen = 0;
    uint8_t Buf(size_t nOffset) const { return nOffset < nLen ? pData[nOffset] : 0; }     // WindowBuf.cpp:639
};

// The slice of CDIB (source/Dib.h:33-55) that reaches the decoder: the preview DIB CjfifDecode lets the Photoshop decoder fill
// (m_pPsDec->DecodePsd(nStartPos, &m_pImgDec->m_pDibTemp, ...), source/JfifDecode.cpp:7369).  The bits live in the decoder
// (jsnoop_dib_temp_create), so GetBitmapPtr hands them out as the reference's would.
class CDibGpu {
public:
    void  Kill() { if (m_h) jsnoop_dib_temp_create(m_h, 0, 0); m_pBits = nullptr; m_nW = m_nH = 0; }                                     // Dib.cpp:88
    bool  CreateDIB(unsigned long dwWidth, unsigned long dwHeight, unsigned short nBits)                                               // Dib.cpp:53: 32 bits per pixel is what this path creates
    { if (!m_h || nBits != 32) return false; m_pBits = jsnoop_dib_temp_create(m_h, (unsigned)dwWidth, (unsigned)dwHeight); m_nW = (unsigned)dwWidth; m_nH = (unsigned)dwHeight; return m_pBits != nullptr; }
    void* GetDIBBitArray() const { return m_pBits; }                                                                                   // Dib.cpp:131
    unsigned GetWidth() const { return m_nW; }
    unsigned GetHeight() const { return m_nH; }
    void  Attach(JsnoopDecoder* h) { m_h = h; }
    void  Invalidate() { m_pBits = nullptr; m_nW = m_nH = 0; }                                                                         // the decoder dropped the bits (Reset, DecodeScanImg): GetDIBBitArray is NULL as after Kill
private:
    JsnoopDecoder* m_h = nullptr; uint8_t* m_pBits = nullptr; unsigned m_nW = 0, m_nH = 0;
};

// TDib: the type of the public member m_pDibTemp -- CDibGpu here; a build inside the reference's tree may name its own CDIB-shaped class
// (it needs Kill / CreateDIB / GetDIBBitArray, an Attach(JsnoopDecoder*) hook and Invalidate(): called when the decoder has dropped the bits).
template <class TDib>
class CimgDecodeGpuT {
public:
    using LogFn = std::function<void(int /*0 info, 1 warn, 2 err*/, const std::string&)>;

    explicit CimgDecodeGpuT(LogFn pLog = nullptr, const CwindowBufView* pWBuf = nullptr) : m_pWBuf(pWBuf), m_log(std::move(pLog))
    {
        m_h = jsnoop_create();                                   // CimgDecode ctor (ImgDecode.cpp:142)
        if (!m_h) throw std::runtime_error(std::string("jsnoop_create: ") + jsnoop_last_error());
        if (m_log) jsnoop_set_log_callback(m_h, &CimgDecodeGpuT::LogThunk, this);
        m_pDibTemp.Attach(m_h);
    }
    ~CimgDecodeGpuT() { jsnoop_destroy(m_h); }
    CimgDecodeGpuT(const CimgDecodeGpuT&) = delete;
    CimgDecodeGpuT& operator=(const CimgDecodeGpuT&) = delete;

    // ---- the three public members CjfifDecode writes for a preview that is not the scan decoder's (source/ImgDecode.h:507-510, "FIXME (workaround)"
    //      there too; set at source/JfifDecode.cpp:7369-7373).  Plain members like the reference's: SyncPreviewMembers() carries them into the
    //      library -- IsPreviewReady / GetBitmapPtr call it, so poking them and asking is all a caller does.
    bool m_bDibTempReady = false;
    TDib m_pDibTemp;
    bool m_bPreviewIsJpeg = false;
    void SyncPreviewMembers() { jsnoop_set_dib_temp_ready(m_h, m_bDibTempReady); jsnoop_set_preview_is_jpeg(m_h, m_bPreviewIsJpeg); }

    void SetWindowBuf(const CwindowBufView* pWBuf) { m_pWBuf = pWBuf; }

    // ---- lifecycle ------------------------------------------------------------------------------
    void Reset() { SyncPreviewMembers(); jsnoop_reset(m_h); m_bDibTempReady = false; m_pDibTemp.Invalidate(); }   // :49 (kills m_pDibTemp when it was ready, :80-83 -- "ready" is the member the caller may just have set)
    void ResetState() { jsnoop_reset_state(m_h); }              // :286
    void ResetDqtTables() { jsnoop_reset_dqt_tables(m_h); }     // :343 (private in the reference: ResetState calls it)
    void ResetDhtLookup() { jsnoop_reset_dht_lookup(m_h); }     // :373

    // ---- options: the CSnoopConfig fields DecodeScanImg reads (:2730-2741) -------------------------
    void SetConfig(bool bDecodeScanImgAc, bool bHistoEn = false, bool bStatClipEn = false, unsigned nErrMaxDecodeScan = 20, bool bDumpHistoY = false)
    { jsnoop_set_options(m_h, bDecodeScanImgAc, bHistoEn, bStatClipEn, nErrMaxDecodeScan); jsnoop_set_dump_histo_y(m_h, bDumpHistoY); }

    // ---- tables / geometry (same names, same bool returns) -------------------------------------------
    bool SetDqtEntry(unsigned nTblDestId, unsigned nCoeffInd, unsigned nCoeffIndZz, unsigned short nCoeffVal)
    { return jsnoop_set_dqt_entry(m_h, nTblDestId, nCoeffInd, nCoeffIndZz, nCoeffVal) != 0; }                 // :424
    bool SetDqtTables(unsigned nCompInd, unsigned nTbl) { return jsnoop_set_dqt_tables(m_h, nCompInd, nTbl) != 0; }          // :505
    unsigned GetDqtEntry(unsigned nTblDestId, unsigned nCoeffInd) { return jsnoop_get_dqt_entry(m_h, nTblDestId, nCoeffInd); } // :466
    bool SetDhtTables(unsigned nCompInd, unsigned nTblDc, unsigned nTblAc) { return jsnoop_set_dht_tables(m_h, nCompInd, nTblDc, nTblAc) != 0; } // :536
    bool SetDhtEntry(unsigned nDestId, unsigned nClass, unsigned nInd, unsigned nLen, unsigned nBits, unsigned nMask, unsigned nCode)
    { return jsnoop_set_dht_entry(m_h, nDestId, nClass, nInd, nLen, nBits, nMask, nCode) != 0; }                // :748
    bool SetDhtSize(unsigned nDestId, unsigned nClass, unsigned nSize) { return jsnoop_set_dht_size(m_h, nDestId, nClass, nSize) != 0; } // :834
    void SetPrecision(unsigned nPrecision) { jsnoop_set_precision(m_h, nPrecision); }                           // :564
    void SetSofSampFactors(unsigned nCompInd, unsigned nSampFactH, unsigned nSampFactV) { jsnoop_set_sof_samp_factors(m_h, nCompInd, nSampFactH, nSampFactV); } // :619
    void SetImageDetails(unsigned nDimX, unsigned nDimY, unsigned nCompsSOF, unsigned nCompsSOS, bool bRstEn, unsigned nRstInterval)
    { jsnoop_set_image_details(m_h, nDimX, nDimY, nCompsSOF, nCompsSOS, bRstEn, nRstInterval); }                // :590
    void SetImageDimensions(unsigned nWidth, unsigned nHeight) { jsnoop_set_image_dimensions(m_h, nWidth, nHeight); }          // :2706
    void GetImageDimensions(unsigned& nWidth, unsigned& nHeight) { jsnoop_get_image_dimensions(m_h, &nWidth, &nHeight); }      // (m_rectImgBase, read by the view code)

    // ---- minimal header walk: the subset of CjfifDecode::DecodeMarker that feeds this object --------------
    bool WalkJfifHeader(unsigned& nPosScanStart)
    { return m_pWBuf && jsnoop_jfif_walk(m_h, m_pWBuf->pData, m_pWBuf->nLen, &nPosScanStart) == 0; }

    // ---- the hot path -----------------------------------------------------------------------------------
    void DecodeScanImg(unsigned nStart, bool bDisplay, bool bQuiet)                                              // :2723
    {
        if (!m_pWBuf || !m_pWBuf->pData) { if (m_log) m_log(2, "*** ERROR: DecodeScanImg without a file buffer ***"); return; }
        jsnoop_decode_scan_img(m_h, m_pWBuf->pData, m_pWBuf->nLen, nStart, bDisplay, bQuiet);
        m_pDibTemp.Invalidate();                                                                                 // (the decode clears the temporary preview, :2976-2978)
        m_bPreviewIsJpeg = jsnoop_is_preview_ready(m_h) != 0; m_bDibTempReady = jsnoop_get_dib_temp_ready(m_h) != 0;     // :3647-3648
    }

    // ---- results (owned by the decoder, valid until the next Reset / DecodeScanImg / destruction) ------------
    bool IsPreviewReady() { SyncPreviewMembers(); return jsnoop_is_preview_ready(m_h) != 0; }                    // :3753 (returns m_bPreviewIsJpeg)
    void GetImageSize(unsigned& nX, unsigned& nY) { jsnoop_get_image_size(m_h, &nX, &nY); }                      // :4929
    void GetBitmapPtr(unsigned char*& pBitmap) { SyncPreviewMembers(); pBitmap = const_cast<unsigned char*>(jsnoop_get_bitmap_ptr(m_h)); } // :4940
    const void* GetBitmapDevicePtr() { return jsnoop_get_bitmap_dev(m_h); }                                      // HBM copy of the DIB
    void GetPixMapPtrs(short*& pMapY, short*& pMapCb, short*& pMapCr)                                            // :4913
    {
        const int16_t *y, *cb, *cr; jsnoop_get_pixmap_ptrs(m_h, &y, &cb, &cr);
        pMapY = const_cast<short*>(y); pMapCb = const_cast<short*>(cb); pMapCr = const_cast<short*>(cr);
    }
    void LookupFilePosPix(unsigned nPixX, unsigned nPixY, unsigned& nByte, unsigned& nBit) { jsnoop_lookup_file_pos_pix(m_h, nPixX, nPixY, &nByte, &nBit); } // :5001
    void LookupFilePosMcu(unsigned nMcuX, unsigned nMcuY, unsigned& nByte, unsigned& nBit) { jsnoop_lookup_file_pos_mcu(m_h, nMcuX, nMcuY, &nByte, &nBit); } // :5020
    void LookupBlkYCC(unsigned nBlkX, unsigned nBlkY, int& nY, int& nCb, int& nCr) { jsnoop_lookup_blk_ycc(m_h, nBlkX, nBlkY, &nY, &nCb, &nCr); }            // :5037
    // bHistoEn / bStatClipEn statistics (m_sHisto, m_sStatClip, m_anCcHisto_r/g/b, m_anHistoYFull; ImgDecode.h:220-279, :656-661)
    // as one JSNOOP_STATS_WORDS record, see include/jsnoop_gpu.h
    void GetColorStats(uint32_t* pStats) { jsnoop_get_color_stats(m_h, pStats); }
    // Export to TIFF (CJPEGsnoopDoc::OnToolsExporttiff + FileTiff::WriteFile): nMode 0 RGB8, 1 RGB16, 2 YCC8
    bool ExportTiff(const std::string& strFnameOut, int nMode) { return jsnoop_export_tiff(m_h, strFnameOut.c_str(), nMode) == 0; }
    bool ExportJpeg(const std::string& strFnameOut) { return jsnoop_export_jpeg(m_h, strFnameOut.c_str()) == 0; }   // the coefficients the decoder holds as a baseline JPEG file, coded on the device
    // ... with restart intervals (jsnoop_export_jpeg_rst): nMode JSNOOP_RESTART_*, nInterval in MCUs or MCU rows; bOptimal: the image's own Huffman tables
    bool ExportJpegRestart(const std::string& strFnameOut, bool bOptimal, int nMode, unsigned nInterval)
    { JsnoopExportCoding coding; jsnoop_export_coding_defaults(&coding); coding.huffman = bOptimal ? JSNOOP_HUFFMAN_OPTIMAL : JSNOOP_HUFFMAN_ANNEX_K;
      JsnoopExportRestart rst; jsnoop_export_restart_defaults(&rst); rst.mode = nMode; rst.interval = nInterval;
      return jsnoop_export_jpeg_rst(m_h, strFnameOut.c_str(), &coding, &rst) == 0; }
    // ... as a progressive file (jsnoop_export_jpeg_prog): scans empty: the built-in script, else the caller's (DESIGN.md 4.17 has the rules)
    bool ExportJpegProgressive(const std::string& strFnameOut, int nMode, unsigned nInterval, const std::vector<JsnoopExportScan>& scans = {})
    { JsnoopExportRestart rst; jsnoop_export_restart_defaults(&rst); rst.mode = nMode; rst.interval = nInterval;
      JsnoopExportProgressive prog; jsnoop_export_progressive_defaults(&prog); prog.mode = scans.empty() ? JSNOOP_PROGRESSIVE_DEFAULT : JSNOOP_PROGRESSIVE_SCRIPT;
      prog.nscans = (uint32_t)scans.size(); prog.scans = scans.empty() ? nullptr : scans.data();
      return jsnoop_export_jpeg_prog(m_h, strFnameOut.c_str(), nullptr, &rst, &prog) == 0; }
    // hover helpers next to LookupFilePosMcu (source/JPEGsnoopViewImg.cpp:294-334); CPoint is a pair of unsigned here
    void PixelToMcu(unsigned nPixX, unsigned nPixY, unsigned& nMcuX, unsigned& nMcuY) { jsnoop_pixel_to_mcu(m_h, nPixX, nPixY, &nMcuX, &nMcuY); }               // :5056
    void PixelToBlk(unsigned nPixX, unsigned nPixY, unsigned& nBlkX, unsigned& nBlkY) { jsnoop_pixel_to_blk(m_h, nPixX, nPixY, &nBlkX, &nBlkY); }               // :5071
    unsigned McuXyToLinear(unsigned nMcuX, unsigned nMcuY) { return jsnoop_mcu_xy_to_linear(m_h, nMcuX, nMcuY); }                                              // :5088
    // CwindowBuf overlays (source/WindowBuf.cpp:516-620): the next DecodeScanImg reads the patched bytes, as CwindowBuf::Buf would hand them out
    bool OverlayInstall(unsigned /*nOvrInd*/, const uint8_t* pOverlay, unsigned nLen, unsigned nBegin) { return jsnoop_overlay_install(m_h, pOverlay, nLen, nBegin) != 0; }
    void OverlayRemoveAll() { jsnoop_overlay_remove_all(m_h); }
    unsigned OverlayGetNum() { return jsnoop_overlay_get_num(m_h); }
    bool OverlayGet(unsigned nOvrInd, const uint8_t*& pOverlay, unsigned& nLen, unsigned& nBegin) { return jsnoop_overlay_get(m_h, nOvrInd, &pOverlay, &nLen, &nBegin) != 0; }
    unsigned PackFileOffset(unsigned nByte, unsigned nBit) const { return (nByte << 4) + nBit; }                 // :5104
    void UnpackFileOffset(unsigned nPacked, unsigned& nByte, unsigned& nBit) const { nBit = nPacked & 0x7; nByte = nPacked >> 4; } // :5123

    // ---- preview re-render on the retained data --------------------------------------------------------------
    void SetPreviewMode(unsigned nMode) { jsnoop_set_preview_mode(m_h, nMode); }                                 // :633
    unsigned GetPreviewMode() { return jsnoop_get_preview_mode(m_h); }
    void SetPreviewYccOffset(unsigned nMcuX, unsigned nMcuY, int nY, int nCb, int nCr) { jsnoop_set_preview_ycc_offset(m_h, nMcuX, nMcuY, nY, nCb, nCr); } // :650

    void GetPreviewYccOffset(unsigned& nMcuX, unsigned& nMcuY, int& nY, int& nCb, int& nCr) { jsnoop_get_preview_ycc_offset(m_h, &nMcuX, &nMcuY, &nY, &nCb, &nCr); }   // :670
    void SetPreviewMcuInsert(unsigned nMcuX, unsigned nMcuY, int nLen) { jsnoop_set_preview_mcu_insert(m_h, nMcuX, nMcuY, nLen); }                                        // :682
    void GetPreviewMcuInsert(unsigned& nMcuX, unsigned& nMcuY, unsigned& nLen) { jsnoop_get_preview_mcu_insert(m_h, &nMcuX, &nMcuY, &nLen); }                             // :693

    JsnoopDecoder* Handle() { return m_h; }

private:
    static void LogThunk(void* user, int level, const char* text) { auto* self = static_cast<CimgDecodeGpuT*>(user); if (self->m_log) self->m_log(level, text); }
    JsnoopDecoder* m_h = nullptr;
    const CwindowBufView* m_pWBuf;
    LogFn m_log;
};
using CimgDecodeGpu = CimgDecodeGpuT<CDibGpu>;

// The slice of CJPEGsnoopCore that belongs to the scan-decode path (source/JPEGsnoopCore.h:79-117, JPEGsnoopCore.cpp:1211-1399):
// the data-bearing I_* accessors over the core's one CimgDecode (source/JPEGsnoopCore.cpp:46), an AnalyzeFile-shaped entry
// (source/JPEGsnoopCore.cpp:325: open, analyse, close) fed from a file or from bytes, the B_Overlay* pass-throughs of its
// CwindowBuf, and a batched replacement for the strictly sequential per-file loop (DoBatchFileProcess :765-845).  Not carried:
// the status-bar / zoom / marker / GDI accessors (I_SetStatusBar, I_*Zoom*, I_*Marker*, I_ViewOnDraw, I_*StatusText) -- Windows
// GUI state that never reaches the decoder -- and the J_* metadata-report accessors (out of scope).
class CJPEGsnoopCoreGpu {
public:
    explicit CJPEGsnoopCoreGpu(CimgDecodeGpu::LogFn pLog = nullptr) : m_pImgDec(new CimgDecodeGpu(std::move(pLog), &m_view))
    { m_b = jsnoop_batch_create(nullptr); if (!m_b) { delete m_pImgDec; throw std::runtime_error(std::string("jsnoop_batch_create: ") + jsnoop_last_error()); } }
    ~CJPEGsnoopCoreGpu() { jsnoop_batch_destroy(m_b); delete m_pImgDec; }
    CJPEGsnoopCoreGpu(const CJPEGsnoopCoreGpu&) = delete;
    CJPEGsnoopCoreGpu& operator=(const CJPEGsnoopCoreGpu&) = delete;

    // ---- AnalyzeFile :325 (AnalyzeOpen, AnalyzeFileDo, AnalyzeClose): header walk with the built-in front end, then DecodeScanImg(nStart, true, false) as
    //      CjfifDecode::DecodeMarker issues it (source/JfifDecode.cpp:5299).  The file image stays owned by the core until the next Analyze*.
    bool AnalyzeBuffer(const uint8_t* pFile, size_t nLen)
    {
        m_file.assign(pFile, pFile + nLen); m_view.pData = m_file.data(); m_view.nLen = m_file.size(); m_bFileAnalyzed = false;
        if (nLen == 0) return false;                             // "ERROR: File length is zero, no decoding done." (:301)
        m_pImgDec->ResetState(); m_pImgDec->Reset();             // CjfifDecode::Reset (source/JfifDecode.cpp:7306-7308)
        unsigned nStart = 0;
        if (!m_pImgDec->WalkJfifHeader(nStart)) return false;
        m_pImgDec->DecodeScanImg(nStart, true, false);
        m_bFileAnalyzed = true;
        return true;
    }
    bool AnalyzeFile(const std::string& strFname)
    {
        FILE* f = fopen(strFname.c_str(), "rb");                 // AnalyzeOpen :157: FALSE when the file cannot be opened
        if (!f) return false;
        std::vector<uint8_t> buf; uint8_t tmp[65536]; size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
        fclose(f);
        m_strPathName = strFname;
        AnalyzeBuffer(buf.data(), buf.size());
        return true;                                             // the status of opening the file, like the reference
    }
    bool IsAnalyzed() const { return m_bFileAnalyzed; }          // :138

    // ---- I_* accessor wrappers for CimgDecode (:1211-1399) ---------------------------------------------------------------------
    unsigned I_GetDqtEntry(unsigned nTblDestId, unsigned nCoeffInd) { return m_pImgDec->GetDqtEntry(nTblDestId, nCoeffInd); }                       // :1216
    void     I_SetPreviewMode(unsigned nMode) { m_pImgDec->SetPreviewMode(nMode); }                                                                 // :1221
    unsigned I_GetPreviewMode() { return m_pImgDec->GetPreviewMode(); }                                                                             // :1226
    void     I_SetPreviewYccOffset(unsigned nMcuX, unsigned nMcuY, int nY, int nCb, int nCr) { m_pImgDec->SetPreviewYccOffset(nMcuX, nMcuY, nY, nCb, nCr); }   // :1231
    void     I_GetPreviewYccOffset(unsigned& nMcuX, unsigned& nMcuY, int& nY, int& nCb, int& nCr) { m_pImgDec->GetPreviewYccOffset(nMcuX, nMcuY, nY, nCb, nCr); } // :1236
    void     I_SetPreviewMcuInsert(unsigned nMcuX, unsigned nMcuY, int nLen) { m_pImgDec->SetPreviewMcuInsert(nMcuX, nMcuY, nLen); }               // :1241
    void     I_GetPreviewMcuInsert(unsigned& nMcuX, unsigned& nMcuY, unsigned& nLen) { m_pImgDec->GetPreviewMcuInsert(nMcuX, nMcuY, nLen); }       // :1246
    void     I_PixelToMcu(unsigned nPixX, unsigned nPixY, unsigned& nMcuX, unsigned& nMcuY) { m_pImgDec->PixelToMcu(nPixX, nPixY, nMcuX, nMcuY); } // :1276
    void     I_PixelToBlk(unsigned nPixX, unsigned nPixY, unsigned& nBlkX, unsigned& nBlkY) { m_pImgDec->PixelToBlk(nPixX, nPixY, nBlkX, nBlkY); } // :1281
    unsigned I_McuXyToLinear(unsigned nMcuX, unsigned nMcuY) { return m_pImgDec->McuXyToLinear(nMcuX, nMcuY); }                                    // :1286
    void     I_GetImageSize(unsigned& nX, unsigned& nY) { m_pImgDec->GetImageSize(nX, nY); }                                                       // :1291
    void     I_GetPixMapPtrs(short*& pMapY, short*& pMapCb, short*& pMapCr) { m_pImgDec->GetPixMapPtrs(pMapY, pMapCb, pMapCr); }                   // :1296
    void     I_GetBitmapPtr(unsigned char*& pBitmap) { m_pImgDec->GetBitmapPtr(pBitmap); }                                                         // :1361: the decoder-owned pointer, nothing copied
    void     I_LookupFilePosMcu(unsigned nMcuX, unsigned nMcuY, unsigned& nByte, unsigned& nBit) { m_pImgDec->LookupFilePosMcu(nMcuX, nMcuY, nByte, nBit); } // :1366
    void     I_LookupFilePosPix(unsigned nPixX, unsigned nPixY, unsigned& nByte, unsigned& nBit) { m_pImgDec->LookupFilePosPix(nPixX, nPixY, nByte, nBit); } // :1371
    void     I_LookupBlkYCC(unsigned nBlkX, unsigned nBlkY, int& nY, int& nCb, int& nCr) { m_pImgDec->LookupBlkYCC(nBlkX, nBlkY, nY, nCb, nCr); } // :1376
    bool     I_IsPreviewReady() { return m_pImgDec->IsPreviewReady(); }                                                                           // :1396
    const void* I_GetBitmapDevicePtr() { return m_pImgDec->GetBitmapDevicePtr(); }                                                                 // (HBM copy, no reference counterpart)

    // ---- B_* accessor wrappers for CwindowBuf that reach the decoder: byte fetch and overlays (:1180-1207) ------------------------
    uint8_t  B_Buf(unsigned long nOffset, bool bClean = false)                                                                                     // :1180 -> CwindowBuf::Buf (source/WindowBuf.cpp:639)
    {
        if (!bClean) {
            const uint8_t* p; unsigned n, b; uint8_t v = 0; bool hit = false;
            for (unsigned i = 0; i < m_pImgDec->OverlayGetNum(); i++)
                if (m_pImgDec->OverlayGet(i, p, n, b) && nOffset >= b && nOffset < (unsigned long)b + n) { v = p[nOffset - b]; hit = true; }
            if (hit) return v;
        }
        return m_view.Buf(nOffset);
    }
    bool     B_OverlayInstall(unsigned nOvrInd, const uint8_t* pOverlay, unsigned nLen, unsigned nBegin, unsigned /*nMcuX*/ = 0, unsigned /*nMcuY*/ = 0,
                              unsigned /*nMcuLen*/ = 0, unsigned /*nMcuLenIns*/ = 0, int /*nAdjY*/ = 0, int /*nAdjCb*/ = 0, int /*nAdjCr*/ = 0)
    { return m_pImgDec->OverlayInstall(nOvrInd, pOverlay, nLen, nBegin); }                                                                         // :1191
    void     B_OverlayRemoveAll() { m_pImgDec->OverlayRemoveAll(); }                                                                              // :1198
    bool     B_OverlayGet(unsigned nOvrInd, const uint8_t*& pOverlay, unsigned& nLen, unsigned& nBegin) { return m_pImgDec->OverlayGet(nOvrInd, pOverlay, nLen, nBegin); } // :1203
    // re-run the scan decode of the analysed file on the (re-)patched bytes: what the reference's "Tools -> File overlay" does after an install
    bool     ReprocessFile() { if (!m_bFileAnalyzed) return false; const std::vector<uint8_t> copy(m_file); return AnalyzeBuffer(copy.data(), copy.size()); }

    // ---- batch: N files -> N DIBs resident in HBM (per-file semantics of DoBatchFileProcess :765-845 preserved) -------------------
    void     BatchClear() { jsnoop_batch_clear(m_b); }
    int      BatchAddFile(const uint8_t* pFile, size_t nLen) { return jsnoop_batch_add_jpeg(m_b, pFile, nLen); }
    unsigned GetBatchFileCount() const { return (unsigned)jsnoop_batch_count(m_b); }                                                             // :680
    bool     DoBatchProcess() { return jsnoop_batch_upload(m_b) == 0 && jsnoop_batch_decode(m_b) == 0 && jsnoop_batch_sync(m_b) == 0; }
    int      BatchLastForm() const { return jsnoop_batch_last_form(m_b); }   // the form behind the results held now: 0 nothing decoded, 1 Full-IDCT kernels, 2 DC-only fast form
    bool     BatchSetSplit(int nParts) { return jsnoop_batch_set_split(m_b, nParts) == 0; }   // 0: the library decides (default), 1: one stream, 2: the halves of the batch on two streams side by side (same results)
    bool     BatchSetTuning(const JsnoopTuning& t) { return jsnoop_batch_set_tuning(m_b, &t) == 0; }   // how the batch decodes, never what it produces (jsnoop_tuning_defaults fills a struct)
    const void* BatchBitmapDevicePtr(int nFileInd) const { return jsnoop_batch_dib_dev(m_b, nFileInd); }
    // the DIBs of the listed files as cropped, top-down, three-channel pixels in the caller's device memory, one launch for the whole list
    // (jsnoop_batch_pack: enqueued on the batch's stream, not waited for; jsnoop_pack_spec_defaults fills a spec)
    bool     BatchPack(const JsnoopPackSpec& spec, const std::vector<int>& files, const std::vector<JsnoopPackDst>& dst)
    { return files.size() == dst.size() && jsnoop_batch_pack(m_b, &spec, files.data(), (int)files.size(), dst.data()) == 0; }
    // the listed files rendered as libjpeg's pixels (integer IDCT, fancy upsampling, fixed-point colour) from the coefficient arena, in BatchPack's store forms
    // (jsnoop_batch_pack_ijg: one launch for the whole list, same ordering; BatchIjgRenderable: whether a file's layout is rendered, host arithmetic)
    bool     BatchPackIjg(const JsnoopPackSpec& spec, const std::vector<int>& files, const std::vector<JsnoopPackDst>& dst)
    { return files.size() == dst.size() && jsnoop_batch_pack_ijg(m_b, &spec, files.data(), (int)files.size(), dst.data()) == 0; }
    bool     BatchIjgRenderable(int nFileInd) const { return jsnoop_batch_ijg_renderable(m_b, nFileInd) == 1; }
    // ... at 1 / nDenom of the size (nDenom 1, 2, 4, 8: libjpeg's scaled IDCTs, what djpeg -scale 1/N and Image.draft give; 1 is BatchPackIjg), into destinations of
    // BatchIjgScaledSize's dimensions (jsnoop_batch_pack_ijg_scaled: one launch for the whole list, same ordering)
    bool     BatchPackIjgScaled(const JsnoopPackSpec& spec, unsigned nDenom, const std::vector<int>& files, const std::vector<JsnoopPackDst>& dst)
    { return files.size() == dst.size() && jsnoop_batch_pack_ijg_scaled(m_b, &spec, nDenom, files.data(), (int)files.size(), dst.data()) == 0; }
    bool     BatchIjgScaledSize(int nFileInd, unsigned nDenom, unsigned& nW, unsigned& nH) const { return jsnoop_batch_ijg_scaled_size(m_b, nFileInd, nDenom, &nW, &nH) == 0; }
    // (jsnoop_batch_pack_resized: a rectangle of every listed file at its destination's size, filter = JSNOOP_RESIZE_*; same ordering)
    bool     BatchPackResized(const JsnoopPackSpec& spec, int filter, const std::vector<int>& files, const std::vector<JsnoopResizeDst>& dst)
    { return files.size() == dst.size() && jsnoop_batch_pack_resized(m_b, &spec, filter, files.data(), (int)files.size(), dst.data()) == 0; }
    // the DCT coefficients of the listed files, one destination per (file, dst[k].comp): blocks in raster order of the component's block grid, cumulative DC in
    // natural index 0 (jsnoop_batch_pack_coefs: one launch for the whole list, same ordering; jsnoop_coef_spec_defaults fills a spec)
    bool     BatchPackCoefs(const JsnoopCoefSpec& spec, const std::vector<int>& files, const std::vector<JsnoopCoefDst>& dst)
    { return files.size() == dst.size() && jsnoop_batch_pack_coefs(m_b, &spec, files.data(), (int)files.size(), dst.data()) == 0; }
    // the retained Y / Cb / Cr planes of the listed files, one two-dimensional destination per (file, dst[k].comp): cropped to the SOF dimensions or decimated to the
    // component's own grid, int16 / uint8 / float32 (jsnoop_batch_pack_planes: one launch for the whole list, same ordering; jsnoop_plane_spec_defaults fills a spec)
    bool     BatchPackPlanes(const JsnoopPlaneSpec& spec, const std::vector<int>& files, const std::vector<JsnoopPlaneDst>& dst)
    { return files.size() == dst.size() && jsnoop_batch_pack_planes(m_b, &spec, files.data(), (int)files.size(), dst.data()) == 0; }
    // the listed files (empty list: all) written back as baseline JPEG files, entropy-coded on the device into memory the batch owns (jsnoop_batch_export_jpeg: waits twice;
    // valid until the next export, clear, upload or destroy); entry k through BatchExportFile / BatchReadExport (false where the image could not be exported: nResult says why)
    // bOptimal: every file with its own Huffman tables, built on the device (jsnoop_batch_export_jpeg_coded, JSNOOP_HUFFMAN_OPTIMAL); BatchExportTables reads them back
    bool     BatchExportJpeg(const std::vector<int>& files = {}, bool bJfif = true, bool bOptimal = false)
    { JsnoopExportSpec spec; jsnoop_export_spec_defaults(&spec); spec.jfif = bJfif ? 1 : 0;
      const int* p = files.empty() ? nullptr : files.data(); const int n = files.empty() ? jsnoop_batch_count(m_b) : (int)files.size();
      if (!bOptimal) return jsnoop_batch_export_jpeg(m_b, &spec, p, n) == 0;
      JsnoopExportCoding coding; jsnoop_export_coding_defaults(&coding); coding.huffman = JSNOOP_HUFFMAN_OPTIMAL;
      return jsnoop_batch_export_jpeg_coded(m_b, &spec, &coding, p, n) == 0; }
    // the forward path: 8-bit pictures in device memory (what BatchPack wrote, a DIB, any buffer: JsnoopEncodeSrc) to JPEG files, transformed, quantised and
    // entropy-coded on the current device (jsnoop_encode_run + jsnoop_encode_export on an encoder object of its own; jsnoop_encode_spec_defaults fills a spec).
    // files[k]: the file of src[k], empty where it could not be written.  pCoding / pRestart / pProg: NULL = Annex K tables, no restart markers, baseline.
    static bool EncodeJpeg(const std::vector<JsnoopEncodeSrc>& src, const JsnoopEncodeSpec& spec, std::vector<std::vector<uint8_t>>& files, bool bJfif = true,
                           const JsnoopExportCoding* pCoding = nullptr, const JsnoopExportRestart* pRestart = nullptr, const JsnoopExportProgressive* pProg = nullptr)
    {
        files.clear();
        JsnoopEncode* e = jsnoop_encode_create(nullptr);
        if (!e) return false;
        JsnoopExportSpec ex; jsnoop_export_spec_defaults(&ex); ex.jfif = bJfif ? 1 : 0;
        bool ok = jsnoop_encode_run(e, &spec, src.data(), (int)src.size()) == 0 && jsnoop_encode_export(e, &ex, pCoding, pRestart, pProg, nullptr, (int)src.size()) == 0;
        for (int k = 0; ok && k < jsnoop_encode_export_count(e); k++) {
            uint64_t nLen = 0;
            ok = jsnoop_encode_export_file(e, k, nullptr, &nLen, nullptr, nullptr, nullptr) == 0;
            files.emplace_back((size_t)nLen);
            if (ok && nLen) ok = jsnoop_encode_read_export(e, k, files.back().data(), nLen) == (int64_t)nLen;
        }
        jsnoop_encode_destroy(e);
        return ok;
    }
    // jpegtran's lossless transforms of the decoded batch: the listed files (empty = all) flipped, rotated, transposed, cropped or made grey on the device without
    // a second quantisation and written as files (jsnoop_transform_run + jsnoop_transform_export on a transform object of its own, on the batch's stream;
    // jsnoop_transform_spec_defaults fills a spec).  results[k]: JSNOOP_XFORM_* of entry k; out[k]: its file, empty where the entry is not OK or could not be
    // written.  pCoding / pRestart / pProg: NULL = Annex K tables, no restart markers, baseline.  After DoBatchProcess.
    bool     TransformJpeg(const JsnoopTransformSpec& spec, const std::vector<int>& files, std::vector<int>& results, std::vector<std::vector<uint8_t>>& out, bool bJfif = true,
                           const JsnoopExportCoding* pCoding = nullptr, const JsnoopExportRestart* pRestart = nullptr, const JsnoopExportProgressive* pProg = nullptr)
    {
        results.clear(); out.clear();
        JsnoopTransform* t = jsnoop_transform_create(jsnoop_batch_stream(m_b));
        if (!t) return false;
        const int* p = files.empty() ? nullptr : files.data(); const int n = files.empty() ? jsnoop_batch_count(m_b) : (int)files.size();
        JsnoopExportSpec ex; jsnoop_export_spec_defaults(&ex); ex.jfif = bJfif ? 1 : 0;
        bool ok = jsnoop_transform_run(t, m_b, &spec, p, n) == 0;
        if (ok && jsnoop_transform_count(t)) ok = jsnoop_transform_export(t, &ex, pCoding, pRestart, pProg, nullptr, jsnoop_transform_count(t)) == 0;
        for (int k = 0; ok && k < n; k++) {
            int nResult = 0, nImage = -1; uint64_t nLen = 0;
            ok = jsnoop_transform_entry(t, k, &nResult, &nImage) == 0;
            results.push_back(nResult); out.emplace_back();
            if (ok && nImage >= 0) {
                ok = jsnoop_transform_export_file(t, nImage, nullptr, &nLen, nullptr, nullptr, nullptr) == 0;
                out.back().resize((size_t)nLen);
                if (ok && nLen) ok = jsnoop_transform_read_export(t, nImage, out.back().data(), nLen) == (int64_t)nLen;
            }
        }
        jsnoop_transform_destroy(t);
        return ok;
    }
    // BatchExportJpeg with a restart interval per file (jsnoop_batch_export_jpeg_rst): nMode JSNOOP_RESTART_*, nInterval in MCUs or MCU rows; BatchExportRestart: what entry k got
    bool     BatchExportJpegRestart(const std::vector<int>& files, bool bJfif, bool bOptimal, int nMode, unsigned nInterval)
    { JsnoopExportSpec spec; jsnoop_export_spec_defaults(&spec); spec.jfif = bJfif ? 1 : 0;
      JsnoopExportCoding coding; jsnoop_export_coding_defaults(&coding); coding.huffman = bOptimal ? JSNOOP_HUFFMAN_OPTIMAL : JSNOOP_HUFFMAN_ANNEX_K;
      JsnoopExportRestart rst; jsnoop_export_restart_defaults(&rst); rst.mode = nMode; rst.interval = nInterval;
      const int n = files.empty() ? jsnoop_batch_count(m_b) : (int)files.size();
      return jsnoop_batch_export_jpeg_rst(m_b, &spec, &coding, &rst, files.empty() ? nullptr : files.data(), n) == 0; }
    bool     BatchExportRestart(int k, uint32_t& nRi, uint64_t& nIntervals) const { return jsnoop_batch_export_restart(m_b, k, &nRi, &nIntervals) == 0; }
    // BatchExportJpegRestart as progressive files (jsnoop_batch_export_jpeg_prog): scans empty: the built-in script, else the caller's; every scan carries its own
    // optimal tables.  BatchExportScanCount / BatchExportScanInfo: the scans entry k was written with
    bool     BatchExportJpegProgressive(const std::vector<int>& files, bool bJfif, int nMode, unsigned nInterval, const std::vector<JsnoopExportScan>& scans = {})
    { JsnoopExportSpec spec; jsnoop_export_spec_defaults(&spec); spec.jfif = bJfif ? 1 : 0;
      JsnoopExportRestart rst; jsnoop_export_restart_defaults(&rst); rst.mode = nMode; rst.interval = nInterval;
      JsnoopExportProgressive prog; jsnoop_export_progressive_defaults(&prog); prog.mode = scans.empty() ? JSNOOP_PROGRESSIVE_DEFAULT : JSNOOP_PROGRESSIVE_SCRIPT;
      prog.nscans = (uint32_t)scans.size(); prog.scans = scans.empty() ? nullptr : scans.data();
      const int n = files.empty() ? jsnoop_batch_count(m_b) : (int)files.size();
      return jsnoop_batch_export_jpeg_prog(m_b, &spec, nullptr, &rst, &prog, files.empty() ? nullptr : files.data(), n) == 0; }
    int      BatchExportScanCount(int k) const { return jsnoop_batch_export_scan_count(m_b, k); }
    bool     BatchExportScanInfo(int k, int nScan, JsnoopExportScan& scan, uint32_t& nRi, uint64_t& nIntervals, uint64_t& nSosOffset, uint64_t& nDataBytes) const
    { return jsnoop_batch_export_scan_info(m_b, k, nScan, &scan, &nRi, &nIntervals, &nSosOffset, &nDataBytes) == 0; }
    bool     BatchExportTables(int k, int nSlot, uint8_t anCounts[16], uint8_t anSymbols[256], uint32_t& nSymbols, uint32_t anFreq[256])
    { return jsnoop_batch_export_tables(m_b, k, nSlot, anCounts, anSymbols, &nSymbols, anFreq) == 0; }
    int      BatchExportCount() const { return jsnoop_batch_export_count(m_b); }
    bool     BatchExportFile(int k, const void*& pDev, uint64_t& nLen, int& nResult, uint32_t& nDetail, int& nFileInd) const { return jsnoop_batch_export_file(m_b, k, &pDev, &nLen, &nResult, &nDetail, &nFileInd) == 0; }
    bool     BatchReadExport(int k, std::vector<uint8_t>& file)
    { uint64_t n = 0; if (jsnoop_batch_export_file(m_b, k, nullptr, &n, nullptr, nullptr, nullptr) || !n) return false; file.resize((size_t)n); return jsnoop_batch_read_export(m_b, k, file.data(), n) == (int64_t)n; }
    bool     BatchPlaneSize(const JsnoopPlaneSpec& spec, int nFileInd, int nComp, unsigned& nW, unsigned& nH) const { return jsnoop_batch_plane_size(m_b, &spec, nFileInd, nComp, &nW, &nH) == 0; }
    // the bHistoEn (bHistoEn = false: only bStatClipEn) statistics of the listed files, one row of JSNOOP_STATS_WORDS words each at pDst + k * nRowPitchWords (0 = dense)
    // in the caller's device memory, from the retained planes (jsnoop_batch_pack_stats: two launches for the whole list, same ordering; pTotals: NULL or [n][6])
    bool     BatchPackStats(bool bHistoEn, const std::vector<int>& files, void* pDst, uint64_t nRowPitchWords = 0, uint32_t* pTotals = nullptr)
    { return jsnoop_batch_pack_stats(m_b, bHistoEn ? 1 : 0, files.data(), (int)files.size(), pDst, nRowPitchWords, pTotals) == 0; }
    // the histogram of every DCT frequency of component comps[k] of file files[k], one row of jsnoop_coef_hist_words(&spec) words each at pDst + k * nRowPitchWords
    // (0 = dense) in the caller's device memory (jsnoop_batch_pack_coef_hist: one launch for the whole list, same ordering; jsnoop_coef_hist_spec_defaults fills a spec)
    bool     BatchPackCoefHist(const JsnoopCoefHistSpec& spec, const std::vector<int>& files, const std::vector<int>& comps, void* pDst, uint64_t nRowPitchWords = 0)
    { return files.size() == comps.size() && jsnoop_batch_pack_coef_hist(m_b, &spec, files.data(), comps.data(), (int)files.size(), pDst, nRowPitchWords) == 0; }
    bool     BatchCoefGrid(int nFileInd, int nComp, unsigned& nBlkW, unsigned& nBlkH) const { return jsnoop_batch_coef_grid(m_b, nFileInd, nComp, &nBlkW, &nBlkH) == 0; }
    bool     BatchImageDqt(int nFileInd, int nComp, uint16_t* anDqt64) const { return jsnoop_batch_image_dqt(m_b, nFileInd, nComp, anDqt64) == 0; }   // natural order
    bool     BatchGetBitmap(int nFileInd, std::vector<uint8_t>& dib, unsigned& nX, unsigned& nY)
    {
        unsigned info[16]; if (jsnoop_batch_image_info(m_b, nFileInd, info)) return false;
        nX = info[2]; nY = info[3]; dib.resize((size_t)nX * nY * 4);
        return jsnoop_batch_read_dib(m_b, nFileInd, dib.data()) == 0;
    }
    // ---- what the per-file pass of DoBatchFileProcess leaves behind besides pixels (:805-808 DoLogSave; log body ImgDecode.cpp:3021-3745)
    void     BatchSetOptions(bool bDecodeScanImgAc, bool bKeepPixMaps) { jsnoop_batch_set_options(m_b, bDecodeScanImgAc, bKeepPixMaps, 0); }   // before DoBatchProcess
    bool     BatchEnableLog(bool bOn = true) { return jsnoop_batch_enable_log(m_b, bOn) == 0; }                                               // before DoBatchProcess
    // the DecodeScanImg text of file nFileInd, one std::string per CDocLog line ("W:" / "E:" prefixed like AddLineWarn / AddLineErr colour them)
    bool     BatchGetLog(int nFileInd, std::vector<std::string>& lines, bool bHistoEn = false, bool bStatClipEn = false, bool bQuiet = false)
    {
        lines.clear();
        auto thunk = [](void* u, int lvl, const char* txt) { static_cast<std::vector<std::string>*>(u)->push_back(std::string(lvl == 2 ? "E:" : lvl == 1 ? "W:" : "") + txt); };
        return jsnoop_batch_log(m_b, nFileInd, bHistoEn, bStatClipEn, bQuiet, thunk, &lines) == 0;
    }
    // DoLogSave (:807 -> source/JPEGsnoopCore.cpp:150-220) for the scan-decode part of the report: the lines above into a text file
    bool     BatchLogSave(int nFileInd, const std::string& strLogName, bool bHistoEn = false)
    {
        std::vector<std::string> lines; if (!BatchGetLog(nFileInd, lines, bHistoEn)) return false;
        FILE* f = fopen(strLogName.c_str(), "w"); if (!f) return false;
        for (const std::string& l : lines) fprintf(f, "%s\n", l.c_str());
        return fclose(f) == 0;
    }
    // m_pMcuFileMap / m_pBlkDcVal* / m_anDhtHisto / scan status / brightest pixel + average Y of file nFileInd (any pointer may be null)
    bool     BatchGetSideOutputs(int nFileInd, uint32_t* pMcuFileMap, int16_t* pBlkDcY, int16_t* pBlkDcCb, int16_t* pBlkDcCr, uint32_t* pDhtHisto, unsigned* pStatus8, int* pBrightAvg10)
    { return jsnoop_batch_side_outputs(m_b, nFileInd, pMcuFileMap, pBlkDcY, pBlkDcCb, pBlkDcCr, pDhtHisto, pStatus8, pBrightAvg10) == 0; }
    bool     BatchExportTiff(int nFileInd, const std::string& strFname, int nMode = 0) { return jsnoop_batch_export_tiff(m_b, nFileInd, strFname.c_str(), nMode) == 0; }

    // ---- the whole batch loop on every device: GenBatchFileList :454 builds the list, DoBatchFileProcess :765-845 works through it -- here as ONE job
    //      (jsnoop_job_* of include/jsnoop_gpu.h): baseline and progressive files side by side, sharded over the devices, decoded in memory-bounded
    //      rounds; a file the front end refuses or that cannot be read is noted and the loop moves on, as the reference's does (:794-798).
    struct BatchFileInfo { std::string strSrc /*full path*/, strRel /*below dirSrc*/; };
    // The file list of dirSrc (sub-folders with bRecSubdir), sorted by relative path; GenBatchFileListSingle's filter (:608-622): only names whose
    // extension, lower-cased, is .jpg or .jpeg.  Returns the number of files listed.
    unsigned GenBatchFileList(const std::string& dirSrc, bool bRecSubdir)
    {
        namespace fs = std::filesystem;
        m_batchFiles.clear(); m_strBatchDirSrc = dirSrc;
        std::error_code ec;
        auto take = [&](const fs::directory_entry& de) {
            if (!de.is_regular_file(ec)) return;
            std::string ext = de.path().extension().string();
            std::transform(ext.begin(), ext.end(), ext.begin(), [](unsigned char c) { return (char)std::tolower(c); });
            if (ext != ".jpg" && ext != ".jpeg") return;
            m_batchFiles.push_back({ de.path().string(), de.path().lexically_relative(dirSrc).generic_string() });
        };
        if (bRecSubdir) { for (fs::recursive_directory_iterator it(dirSrc, fs::directory_options::skip_permission_denied, ec), end; !ec && it != end; it.increment(ec)) take(*it); }
        else { for (fs::directory_iterator it(dirSrc, ec), end; !ec && it != end; it.increment(ec)) take(*it); }
        std::sort(m_batchFiles.begin(), m_batchFiles.end(), [](const BatchFileInfo& a, const BatchFileInfo& b) { return a.strRel < b.strRel; });
        return (unsigned)m_batchFiles.size();
    }
    unsigned GetBatchFileListCount() const { return (unsigned)m_batchFiles.size(); }
    std::string GetBatchFileInfo(unsigned nFileInd) const { return nFileInd < m_batchFiles.size() ? m_batchFiles[nFileInd].strSrc : std::string(); }   // :686
    const BatchFileInfo* GetBatchFileEntry(unsigned nFileInd) const { return nFileInd < m_batchFiles.size() ? &m_batchFiles[nFileInd] : nullptr; }

    void     JobSetOptions(const JsnoopJobOptions& o) { m_jobOpt = o; m_bJobOpt = true; }
    // "Extract all" for one blob (DoExtractEmbeddedJPEG, source/JPEGsnoopCore.cpp:906-1091, for every hit at once): the frame table of every FF D8 FF in
    // [pBlob, pBlob + nLen), found and walked on `nDevice` (jsnoop_carve_* of include/jsnoop_gpu.h).  false + jsnoop_last_error() on a refusal.
    static bool CarveBlob(const uint8_t* pBlob, size_t nLen, std::vector<JsnoopCarveFrame>& frames, int nDevice = 0, const JsnoopCarveSpec* pSpec = nullptr)
    {
        frames.clear();
        JsnoopCarve* c = jsnoop_carve_create(nDevice);
        if (!c) return false;
        JsnoopCarveSpec spec; jsnoop_carve_spec_defaults(&spec);
        bool ok = jsnoop_carve_run(c, pSpec ? pSpec : &spec, pBlob, nLen, 0) == 0;
        if (ok) { frames.resize((size_t)jsnoop_carve_count(c)); ok = jsnoop_carve_frames(c, frames.data(), frames.size()) == (int64_t)frames.size(); }
        jsnoop_carve_destroy(c);
        return ok;
    }
    // With bExtractAll the job's files are the carved frames of the listed files: which listed file a job index came from, its frame number there (from 1, the
    // number in the reference's name.000001.jpg) and the frame's record.
    struct CarvedInfo { unsigned nFileInd; unsigned nFrame; JsnoopCarveFrame frame; };
    const CarvedInfo* GetCarvedEntry(unsigned nJobInd) const { return nJobInd < m_carved.size() ? &m_carved[nJobInd] : nullptr; }
    // Runs the listed files as one job over `devices` (empty: one shard per visible device); fn sees every file once, on this thread -- f.batch / f.image
    // take the per-image jsnoop_batch_* calls while it runs.  A false return cancels.  Returns jsnoop_job_run's value (0 done, 1 cancelled, -1 error).
    // With bExtractAll every listed file is carved (on the first device of the list) and its frames with status OK are the job's files, in place of the file:
    // f.index then counts carved frames, GetCarvedEntry(f.index) says where each came from.  A listed file that cannot be read yields no frame.
    int      JobRun(const std::function<bool(const JsnoopJobFile&)>& fn, const std::vector<int>& devices = {}, JsnoopJobStats* pStats = nullptr, bool bExtractAll = false)
    {
        JsnoopJob* j = jsnoop_job_create(devices.empty() ? nullptr : devices.data(), (int)devices.size());
        if (!j) return -1;
        int rc = (m_bJobOpt && jsnoop_job_set_options(j, &m_jobOpt)) ? -1 : 0;
        m_carved.clear();
        for (size_t i = 0; rc == 0 && i < m_batchFiles.size(); i++) {
            if (!bExtractAll) { if (jsnoop_job_add_path(j, m_batchFiles[i].strSrc.c_str()) < 0) rc = -1; continue; }
            std::vector<uint8_t> blob; std::vector<JsnoopCarveFrame> frames;
            if (FILE* fp = fopen(m_batchFiles[i].strSrc.c_str(), "rb")) {
                uint8_t tmp[65536]; size_t n;
                while ((n = fread(tmp, 1, sizeof tmp, fp)) > 0) blob.insert(blob.end(), tmp, tmp + n);
                fclose(fp);
            }
            if (!CarveBlob(blob.data(), blob.size(), frames, devices.empty() ? 0 : devices[0])) { rc = -1; break; }
            if (jsnoop_job_add_carved(j, blob.data(), blob.size(), frames.data(), (int64_t)frames.size(), 0, nullptr) < 0) { rc = -1; break; }
            for (size_t k = 0; k < frames.size(); k++) if (frames[k].status == JSNOOP_CARVE_OK) m_carved.push_back({ (unsigned)i, (unsigned)k + 1u, frames[k] });
        }
        if (rc == 0) {
            auto thunk = [](void* u, const JsnoopJobFile* f) -> int { return (*static_cast<const std::function<bool(const JsnoopJobFile&)>*>(u))(*f) ? 0 : 1; };
            rc = jsnoop_job_run(j, fn ? static_cast<jsnoop_job_file_fn>(thunk) : nullptr, const_cast<void*>(static_cast<const void*>(&fn)), pStats);
        }
        jsnoop_job_destroy(j);
        return rc;
    }
    // DoBatchFileProcess for every listed file at once.  With bWriteLog each file gets <dirDst>/<relative path>.txt, the name GenBatchFileListSingle derives
    // (:649-650), holding what BatchLogSave writes: the DecodeScanImg report.  A progressive file has no such report (the reference refuses SOF2): the
    // library's own wording of that goes in its place; a refused or unreadable file gets its message.  Returns the number of files decoded, or -1.
    // bExtractAll (the reference's parameter of the same name, :765): every listed file is carved and its frames are decoded in place of the file; the report
    // of frame k of a file goes to <dirDst>/<relative path>.<k, six digits>.txt beside the name the reference gives the extracted frame (:1052-1056).
    int      DoBatchFileProcessAll(bool bWriteLog, const std::string& dirDst, const std::vector<int>& devices = {}, JsnoopJobStats* pStats = nullptr, bool bExtractAll = false)
    {
        namespace fs = std::filesystem;
        JsnoopJobOptions o; if (m_bJobOpt) o = m_jobOpt; else jsnoop_job_options_defaults(&o);
        if (bWriteLog) { o.enable_log = 1; o.want_planes = 1; }                               // (the report quotes plane samples)
        const JsnoopJobOptions saved = m_jobOpt; const bool bSaved = m_bJobOpt;
        m_jobOpt = o; m_bJobOpt = true;
        int nOk = 0;
        const int rc = JobRun([&](const JsnoopJobFile& f) {
            if (f.status == JSNOOP_JOB_OK) nOk++;
            if (!bWriteLog || f.index < 0 || (size_t)f.index >= (bExtractAll ? m_carved.size() : m_batchFiles.size())) return true;
            std::string strName = bExtractAll ? m_batchFiles[m_carved[(size_t)f.index].nFileInd].strRel : m_batchFiles[(size_t)f.index].strRel;
            if (bExtractAll) { char num[16]; snprintf(num, sizeof num, ".%06u", m_carved[(size_t)f.index].nFrame); strName += num; }
            const fs::path log = fs::path(dirDst) / (strName + ".txt");
            std::error_code ec; fs::create_directories(log.parent_path(), ec);
            FILE* fp = fopen(log.string().c_str(), "w");
            if (!fp) return true;
            auto thunk = [](void* u, int lvl, const char* txt) { fprintf(static_cast<FILE*>(u), "%s%s\n", lvl == 2 ? "E:" : lvl == 1 ? "W:" : "", txt); };
            if (f.status != JSNOOP_JOB_OK) fprintf(fp, "E:%s\n", f.message);
            else if (jsnoop_batch_log(f.batch, f.image, 0, 0, 0, thunk, fp)) fprintf(fp, "W:%s\n", jsnoop_last_error());
            fclose(fp);
            return true;
        }, devices, pStats, bExtractAll);
        m_jobOpt = saved; m_bJobOpt = bSaved;
        return rc < 0 ? -1 : nOk;
    }
    CimgDecodeGpu* ImgDec() { return m_pImgDec; }
    JsnoopBatch* Handle() { return m_b; }
private:
    CwindowBufView m_view; std::vector<uint8_t> m_file; std::string m_strPathName; bool m_bFileAnalyzed = false;
    CimgDecodeGpu* m_pImgDec; JsnoopBatch* m_b = nullptr;
    std::vector<BatchFileInfo> m_batchFiles; std::string m_strBatchDirSrc; JsnoopJobOptions m_jobOpt{}; bool m_bJobOpt = false;
    std::vector<CarvedInfo> m_carved;
};
