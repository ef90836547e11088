"""Host-side mirror of the reference's operator interface for the scan-decode path.

`CimgDecode` keeps the reference's method names, argument meaning and error behaviour
(reference source/ImgDecode.h:286-356) on top of the C ABI; `JpegBatch` is the batched
submit that replaces the strictly sequential per-file loop of
CJPEGsnoopCore::DoBatchFileProcess (source/JPEGsnoopCore.cpp:765).  Python is only the
binding layer here: decode happens in libjsnoop_gpu.so on the GPU.
"""
from __future__ import annotations

import builtins
import ctypes as C

import numpy as np

from . import capi


class CimgDecode:
    """One decoder object == one `CimgDecode` of the reference."""

    PREVIEW_RGB, PREVIEW_YCC, PREVIEW_R, PREVIEW_G, PREVIEW_B, PREVIEW_Y, PREVIEW_CB, PREVIEW_CR = range(1, 9)

    def __init__(self, log=None):
        self._lib = capi.load()
        self._h = self._lib.jsnoop_create()
        if not self._h:
            raise RuntimeError("jsnoop_create failed: " + capi.last_error())
        self._log_cb = None
        if log is not None:
            self._log_cb = capi.LOG_FN(lambda _u, lvl, txt: log(lvl, txt.decode(errors="replace")))
            self._lib.jsnoop_set_log_callback(self._h, self._log_cb, None)
        self._buf = None

    def close(self):
        if self._h:
            self._lib.jsnoop_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- lifecycle / options -------------------------------------------------------
    def Reset(self): self._lib.jsnoop_reset(self._h)
    def ResetState(self): self._lib.jsnoop_reset_state(self._h)
    def SetOptions(self, bDecodeScanImgAc=True, bHistoEn=False, bStatClipEn=False, nErrMaxDecodeScan=20):
        self._lib.jsnoop_set_options(self._h, int(bDecodeScanImgAc), int(bHistoEn), int(bStatClipEn), nErrMaxDecodeScan)

    # --- tables / geometry ------------------------------------------------------------
    def SetDqtEntry(self, nTblDestId, nCoeffInd, nCoeffIndZz, nCoeffVal):
        return bool(self._lib.jsnoop_set_dqt_entry(self._h, nTblDestId, nCoeffInd, nCoeffIndZz, nCoeffVal))
    def SetDqtTables(self, nCompInd, nTbl): return bool(self._lib.jsnoop_set_dqt_tables(self._h, nCompInd, nTbl))
    def GetDqtEntry(self, nTblDestId, nCoeffInd): return self._lib.jsnoop_get_dqt_entry(self._h, nTblDestId, nCoeffInd)
    def SetDhtEntry(self, nDestId, nClass, nInd, nLen, nBits, nMask, nCode):
        return bool(self._lib.jsnoop_set_dht_entry(self._h, nDestId, nClass, nInd, nLen, nBits, nMask, nCode))
    def SetDhtSize(self, nDestId, nClass, nSize): return bool(self._lib.jsnoop_set_dht_size(self._h, nDestId, nClass, nSize))
    def SetDhtTables(self, nCompInd, nTblDc, nTblAc): return bool(self._lib.jsnoop_set_dht_tables(self._h, nCompInd, nTblDc, nTblAc))
    def SetSofSampFactors(self, nCompInd, nSampFactH, nSampFactV): self._lib.jsnoop_set_sof_samp_factors(self._h, nCompInd, nSampFactH, nSampFactV)
    def SetPrecision(self, nPrecision): self._lib.jsnoop_set_precision(self._h, nPrecision)
    def SetImageDetails(self, nDimX, nDimY, nCompsSOF, nCompsSOS, bRstEn, nRstInterval):
        self._lib.jsnoop_set_image_details(self._h, nDimX, nDimY, nCompsSOF, nCompsSOS, int(bRstEn), nRstInterval)

    # --- decode -------------------------------------------------------------------------
    def DecodeScanImg(self, file_bytes: bytes, nStart: int, bDisplay=True, bQuiet=False):
        """`file_bytes` stands for what the reference reads through CwindowBuf::Buf."""
        self._buf = (C.c_uint8 * len(file_bytes)).from_buffer_copy(file_bytes)
        self._lib.jsnoop_decode_scan_img(self._h, C.cast(self._buf, C.c_void_p), len(file_bytes), nStart, int(bDisplay), int(bQuiet))

    def DecodeProgressive(self, file_bytes: bytes) -> int:
        """Beyond the reference (it refuses SOF2): decode every scan of a progressive file; returns the number of scans."""
        self._buf = (C.c_uint8 * len(file_bytes)).from_buffer_copy(file_bytes)
        n = self._lib.jsnoop_decode_progressive(self._h, C.cast(self._buf, C.c_void_p), len(file_bytes))
        if n < 0:
            raise RuntimeError("jsnoop_decode_progressive: " + capi.last_error())
        return n
    def GetColorStats(self):
        out = np.zeros(2482, np.uint32)
        self._lib.jsnoop_get_color_stats(self._h, out.ctypes.data)
        return out
    def ExportTiff(self, path: str, nMode: int = 0) -> bool:
        return self._lib.jsnoop_export_tiff(self._h, path.encode(), nMode) == 0

    def export_jpeg(self, path: str, huffman: str = "annex_k", restart=0, progressive=False) -> bool:
        """The decoded image written back as a baseline JPEG file (jsnoop_export_jpeg): the coefficients the decoder holds, entropy-coded on the
        device.  False, and no file, where the image cannot be exported (capi.last_error() has the reason).  huffman="optimal": with the image's own
        Huffman tables (jsnoop_export_jpeg_coded).  restart: as in JpegBatch.export_jpeg (jsnoop_export_jpeg_rst).  progressive: False (the default) writes
        a baseline file; True a progressive (SOF2) file along the built-in scan script; a list of scans (components, ss, se, ah, al) along that script, as
        in JpegBatch.export_jpeg (jsnoop_export_jpeg_prog): every scan then has its own optimal tables whatever huffman says, and restart counts in each
        scan's own units."""
        rst = capi.export_restart(self._lib, restart)
        prog = capi.export_progressive(self._lib, progressive)
        if prog.mode != capi.PROGRESSIVE_OFF:
            return self._lib.jsnoop_export_jpeg_prog(self._h, path.encode(), C.byref(capi.export_coding(self._lib, huffman)), C.byref(rst), C.byref(prog)) == 0
        if rst.mode != capi.RESTART_NONE:
            return self._lib.jsnoop_export_jpeg_rst(self._h, path.encode(), C.byref(capi.export_coding(self._lib, huffman)), C.byref(rst)) == 0
        if huffman == "annex_k":
            return self._lib.jsnoop_export_jpeg(self._h, path.encode()) == 0
        return self._lib.jsnoop_export_jpeg_coded(self._h, path.encode(), C.byref(capi.export_coding(self._lib, huffman))) == 0

    # --- results ---------------------------------------------------------------------------
    def IsPreviewReady(self): return bool(self._lib.jsnoop_is_preview_ready(self._h))
    def GetImageSize(self):
        x, y = C.c_uint(), C.c_uint()
        self._lib.jsnoop_get_image_size(self._h, C.byref(x), C.byref(y))
        return x.value, y.value
    def GetBitmapPtr(self):
        x, y = self.GetImageSize()
        p = self._lib.jsnoop_get_bitmap_ptr(self._h)
        if not p:
            return None
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(y, x, 4))
    def GetPixMapPtrs(self):
        g = (C.c_uint * 8)()
        self._lib.jsnoop_get_geometry(self._h, g)
        ptrs = [C.c_void_p() for _ in range(3)]
        self._lib.jsnoop_get_pixmap_ptrs(self._h, *[C.byref(q) for q in ptrs])
        return [np.ctypeslib.as_array(C.cast(q, C.POINTER(C.c_int16)), shape=(g[5] * 8, g[4] * 8)) if q.value else None for q in ptrs]
    def LookupFilePosMcu(self, nMcuX, nMcuY):
        a, b = C.c_uint(), C.c_uint()
        self._lib.jsnoop_lookup_file_pos_mcu(self._h, nMcuX, nMcuY, C.byref(a), C.byref(b))
        return a.value, b.value
    def LookupFilePosPix(self, nPixX, nPixY):
        a, b = C.c_uint(), C.c_uint()
        self._lib.jsnoop_lookup_file_pos_pix(self._h, nPixX, nPixY, C.byref(a), C.byref(b))
        return a.value, b.value
    def LookupBlkYCC(self, nBlkX, nBlkY):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._lib.jsnoop_lookup_blk_ycc(self._h, nBlkX, nBlkY, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value
    def PixelToMcu(self, nPixX, nPixY):
        a, b = C.c_uint(), C.c_uint()
        self._lib.jsnoop_pixel_to_mcu(self._h, nPixX, nPixY, C.byref(a), C.byref(b))
        return a.value, b.value
    def PixelToBlk(self, nPixX, nPixY):
        a, b = C.c_uint(), C.c_uint()
        self._lib.jsnoop_pixel_to_blk(self._h, nPixX, nPixY, C.byref(a), C.byref(b))
        return a.value, b.value
    def McuXyToLinear(self, nMcuX, nMcuY): return self._lib.jsnoop_mcu_xy_to_linear(self._h, nMcuX, nMcuY)
    def SetDumpHistoY(self, bDumpHistoY): self._lib.jsnoop_set_dump_histo_y(self._h, int(bDumpHistoY))
    # CwindowBuf overlays (source/WindowBuf.cpp:516-620): patched bytes seen by the next DecodeScanImg
    def OverlayInstall(self, data: bytes, nBegin: int) -> bool:
        buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
        return bool(self._lib.jsnoop_overlay_install(self._h, C.cast(buf, C.c_void_p), len(data), nBegin))
    def OverlayRemoveAll(self): self._lib.jsnoop_overlay_remove_all(self._h)
    def OverlayGetNum(self): return self._lib.jsnoop_overlay_get_num(self._h)
    def OverlayGet(self, nOvrInd):
        p, n, b = C.c_void_p(), C.c_uint(), C.c_uint()
        if not self._lib.jsnoop_overlay_get(self._h, nOvrInd, C.byref(p), C.byref(n), C.byref(b)):
            return None
        return bytes((C.c_uint8 * n.value).from_address(p.value)), b.value
    def SetPreviewMode(self, nMode): self._lib.jsnoop_set_preview_mode(self._h, nMode)
    def GetPreviewMode(self): return self._lib.jsnoop_get_preview_mode(self._h)
    def SetPreviewYccOffset(self, nMcuX, nMcuY, nY, nCb, nCr): self._lib.jsnoop_set_preview_ycc_offset(self._h, nMcuX, nMcuY, nY, nCb, nCr)
    def LastPath(self): return self._lib.jsnoop_last_path(self._h)
    def LastFlags(self): return self._lib.jsnoop_last_flags(self._h)
    def LastSideMode(self): return self._lib.jsnoop_last_side_mode(self._h)
    def last_form(self) -> int:
        """Which form produced the results held now: 0 nothing decoded, 1 Full-IDCT kernels, 2 DC-only fast form (jsnoop_last_form)."""
        return int(self._lib.jsnoop_last_form(self._h))


class JpegBatch:
    """N JPEG files -> N DIBs resident in HBM (device-side batch)."""

    def __init__(self, stream=None, decode_ac=True, want_planes=False, force_exact=False):
        self._lib = capi.load()
        self._h = self._lib.jsnoop_batch_create(C.c_void_p(stream) if stream else None)
        if not self._h:
            raise RuntimeError("jsnoop_batch_create failed: " + capi.last_error())
        self._lib.jsnoop_batch_set_options(self._h, int(decode_ac), int(want_planes), int(force_exact))
        self.want_planes = want_planes
        self._borrowed = False                   # True: the handle belongs to a JpegPipeline, which destroys it
        self._stream = int(stream) if stream else None   # the caller's hipStream_t, or None: the batch runs on a stream of its own

    def close(self):
        if getattr(self, "_encoder", None) is not None:              # (encode_jpeg's encoder object)
            self._encoder.close(); self._encoder = None
        if self._h:
            if not getattr(self, "_borrowed", False):
                self._lib.jsnoop_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc < 0:
            raise RuntimeError(f"{what} failed: {capi.last_error()}")
        return rc

    def add_jpeg(self, data: bytes) -> int:
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        return self._chk(self._lib.jsnoop_batch_add_jpeg(self._h, C.cast(buf, C.c_void_p), len(data)), "batch_add_jpeg")

    def tile(self, total: int) -> int: return self._chk(self._lib.jsnoop_batch_tile(self._h, total), "batch_tile")
    def set_split(self, parts: int) -> None:
        """parts = 2: later decodes run the two halves of the batch on two streams side by side (same results); 1: one stream; 0: the library decides."""
        self._chk(self._lib.jsnoop_batch_set_split(self._h, parts), "batch_set_split")
    def split_parts(self) -> int: return int(self._lib.jsnoop_batch_split_parts(self._h))
    def tuning(self) -> "capi.Tuning":
        t = capi.Tuning(); self._lib.jsnoop_batch_get_tuning(self._h, C.byref(t)); return t
    def set_tuning(self, **fields) -> None:
        """Replaces fields of the batch's JsnoopTuning (e.g. sub_wl=5, cand_rounds=-1); call before upload()."""
        t = self.tuning()
        for k, v in fields.items():
            if not hasattr(t, k): raise AttributeError("JsnoopTuning has no field " + k)
            setattr(t, k, v)
        self._chk(self._lib.jsnoop_batch_set_tuning(self._h, C.byref(t)), "batch_set_tuning")
    def clear(self): self._lib.jsnoop_batch_clear(self._h)
    def __len__(self): return self._lib.jsnoop_batch_count(self._h)
    def upload(self): self._chk(self._lib.jsnoop_batch_upload(self._h), "batch_upload")
    def decode(self): self._chk(self._lib.jsnoop_batch_decode(self._h), "batch_decode")
    def sync(self): self._chk(self._lib.jsnoop_batch_sync(self._h), "batch_sync")
    def last_form(self) -> int:
        """Which form produced the results the batch holds now: 0 nothing decoded, 1 Full-IDCT kernels, 2 DC-only fast form (jsnoop_batch_last_form)."""
        return int(self._lib.jsnoop_batch_last_form(self._h))

    def decode_timed(self, reps=1):
        st = (C.c_double * capi.NUM_STAGES)()
        ms = self._lib.jsnoop_batch_decode_timed(self._h, reps, st)
        if ms < 0:
            raise RuntimeError("batch_decode_timed failed: " + capi.last_error())
        return ms, {self._lib.jsnoop_stage_name(i).decode(): st[i] for i in range(capi.NUM_STAGES)}

    def info(self, i):
        o = (C.c_uint * 16)()
        self._chk(self._lib.jsnoop_batch_image_info(self._h, i, o), "batch_image_info")
        keys = "dim_x dim_y img_x img_y mcu_w mcu_h mcu_xmax mcu_ymax blk_xmax blk_ymax scan_bytes flags path ncomp file_len total_blocks".split()
        return dict(zip(keys, o))

    def dib(self, i):
        inf = self.info(i)
        out = np.empty((inf["img_y"], inf["img_x"], 4), np.uint8)
        self._chk(self._lib.jsnoop_batch_read_dib(self._h, i, out.ctypes.data), "batch_read_dib")
        return out

    def device(self) -> int:
        """The device the batch lives on (jsnoop_batch_device)."""
        return int(self._lib.jsnoop_batch_device(self._h))

    def pack_bytes(self, i, layout="CHW", float32=False) -> int:
        """Dense size in bytes of image i's packed output (jsnoop_batch_pack_bytes)."""
        spec = _pack_spec(self._lib, layout, bool(float32), False, None, None)
        return int(self._lib.jsnoop_batch_pack_bytes(self._h, C.byref(spec), i))

    def to_torch(self, images=None, layout="CHW", dtype=None, bgr=False, scale=None, bias=None, stack=False, pad_to=None, out=None,
                 size=None, filter="bilinear", roi=None, pixels="jpegsnoop", reduce=1):
        """The decoded images as torch tensors on the batch's device: cropped to the SOF dimensions, top-down, three channels (R,G,B, or
        B,G,R with bgr), filled by ONE jsnoop_batch_pack -- no pixel crosses PCIe.

        images: indices into the batch, any order (None = all).  layout "CHW" -> [3, dim_y, dim_x], "HWC" -> [dim_y, dim_x, 3].
        dtype: torch.uint8 (default: the DIB's bytes) or torch.float32 (float(v) * scale[c] + bias[c], c the output channel; scale / bias a
        number or three, defaults 1 and 0; one rounded multiply, then one rounded add).
        Default: a list of tensors, one per image, carved out of one allocation.  stack=True: one [N, ...] tensor (ValueError if the dimensions
        differ).  pad_to=(H, W): one zero-filled [N, 3, H, W] / [N, H, W, 3] tensor, every image in its top-left corner.  out=: a tensor
        [N, ...] at least as large as every image, or a list of tensors of the images' exact shapes; inner dimensions contiguous; returned as it is.

        size=(H, W): every image -- or the rectangle roi names in it -- resampled to H x W by ONE jsnoop_batch_pack_resized: the result is one
        [N, 3, H, W] / [N, H, W, 3] tensor, or out= of exactly that shape (the outer dimension may be strided).  filter: "bilinear" (half-pixel
        centres, as torch's align_corners=False without antialiasing), "nearest" or "area" (a box filter with fractional coverage, the one for
        reducing).  roi: None (whole images), one (x, y, w, h) for all, or a list with one per image, in the coordinates of the cropped
        top-down image.  With H x W equal to the rectangle's size every filter returns its pixels unchanged.  size= excludes stack and pad_to;
        filter (other than the default) or roi without size= is a ValueError.

        pixels: "jpegsnoop" (default) -- the DIB's bytes: JPEGsnoop's fp32 IDCT, replicated chroma, fp32 colour lines; "libjpeg" -- the batch rendered a
        second time from its coefficients by ONE jsnoop_batch_pack_ijg: the integer "islow" IDCT, fancy chroma upsampling and 16-bit fixed-point
        colour, the pixels Pillow, OpenCV, torchvision and djpeg give for the same file.  Every image listed must be renderable
        (ijg_renderable); size= and roi= are refused with "libjpeg" for now.

        reduce: 1 (default), 2, 4 or 8 -- with pixels="libjpeg", libjpeg's reduced-size decode (the scaled IDCTs: what Image.draft, cv2.IMREAD_REDUCED_COLOR_*
        and djpeg -scale 1/N give): image i arrives as ceil(dim_y / reduce) x ceil(dim_x / reduce) (ijg_scaled_size), and every size above -- stack, pad_to,
        out -- is taken against that.  A sequence gives one value per listed image (reduce_for turns a target size into one); the list is then served by at
        most four jsnoop_batch_pack_ijg_scaled, one per value.  reduce other than 1 without pixels="libjpeg" is a ValueError.

        Calls sync() first (damaged files arrive repaired), synchronises torch's current stream before the pack unless the batch runs on it, and
        waits for the batch's stream -- sync() again, no other stream of the device is waited for -- before it returns: the tensors are ready."""
        import torch
        n_all = len(self)
        idx = list(range(n_all)) if images is None else [int(i) for i in images]
        for i in idx:
            if not 0 <= i < n_all:
                raise IndexError(f"to_torch: image index {i} out of range, the batch holds {n_all}")
        if dtype is None:
            dtype = torch.uint8
        if dtype not in (torch.uint8, torch.float32):
            raise ValueError("to_torch: dtype must be torch.uint8 or torch.float32")
        is_f32 = dtype == torch.float32
        if not is_f32 and (scale is not None or bias is not None):
            raise ValueError("to_torch: scale / bias belong to dtype=torch.float32")
        if bool(stack) + (pad_to is not None) + (out is not None) > 1:
            raise ValueError("to_torch: stack, pad_to and out exclude each other")
        if size is None and (roi is not None or filter != "bilinear"):
            raise ValueError("to_torch: filter and roi belong to size=(H, W)")
        if pixels not in ("jpegsnoop", "libjpeg"):
            raise ValueError("to_torch: pixels must be \"jpegsnoop\" or \"libjpeg\"")
        if pixels == "libjpeg" and (size is not None or roi is not None):
            raise ValueError("to_torch: size= and roi= are not available with pixels=\"libjpeg\"")
        if isinstance(reduce, (list, tuple)):
            red = [int(x) for x in reduce]
            if len(red) != len(idx):
                raise ValueError(f"to_torch: reduce holds {len(red)} values for {len(idx)} images")
        else:
            red = [int(reduce)] * len(idx)
        if any(x not in (1, 2, 4, 8) for x in red) or (not isinstance(reduce, (list, tuple)) and int(reduce) not in (1, 2, 4, 8)):
            raise ValueError("to_torch: reduce must be 1, 2, 4 or 8")
        if pixels != "libjpeg" and (isinstance(reduce, (list, tuple)) or int(reduce) != 1):
            raise ValueError("to_torch: reduce belongs to pixels=\"libjpeg\"")
        spec = _pack_spec(self._lib, layout, is_f32, bgr, scale, bias)
        chw = layout == "CHW"
        self.sync()
        dev = torch.device("cuda", self.device())
        if size is not None:
            return self._to_torch_resized(torch, idx, spec, chw, dtype, dev, stack, pad_to, out, size, filter, roi)
        dims = []
        for k, i in enumerate(idx):
            if red[k] != 1:
                dims.append(self.ijg_scaled_size(i, red[k]))
                continue
            inf = self.info(i)
            dims.append((inf["dim_y"], inf["dim_x"]))
        shape = (lambda h, w: (3, h, w)) if chw else (lambda h, w: (h, w, 3))
        crop = (lambda t, h, w: t[:, :h, :w]) if chw else (lambda t, h, w: t[:h, :w, :])
        if out is not None:
            if isinstance(out, torch.Tensor):
                if out.dim() != 4 or out.shape[0] != len(idx) or out.shape[1 if chw else 3] != 3:
                    raise ValueError(f"to_torch: out must be [{len(idx)}, " + ("3, H, W]" if chw else "H, W, 3]") + f", got {list(out.shape)}")
                H, W = (out.shape[2], out.shape[3]) if chw else (out.shape[1], out.shape[2])
                for k, (h, w) in enumerate(dims):
                    if h > H or w > W:
                        raise ValueError(f"to_torch: image {idx[k]} is {h} x {w}, larger than out's {H} x {W}")
                views, result = [crop(out[k], h, w) for k, (h, w) in enumerate(dims)], out
            else:
                views, result = list(out), out
                if len(views) != len(idx):
                    raise ValueError(f"to_torch: out holds {len(views)} tensors for {len(idx)} images")
                for k, (h, w) in enumerate(dims):
                    if not isinstance(views[k], torch.Tensor) or tuple(views[k].shape) != shape(h, w):
                        raise ValueError(f"to_torch: out[{k}] must be a tensor of shape {list(shape(h, w))} for image {idx[k]}")
            for k, t in enumerate(views):
                if t.device != dev:
                    raise ValueError(f"to_torch: out[{k}] is on {t.device}, the batch on {dev}")
                if t.dtype != dtype:
                    raise ValueError(f"to_torch: out[{k}] is {t.dtype}, asked for {dtype}")
        elif pad_to is not None:
            H, W = int(pad_to[0]), int(pad_to[1])
            for k, (h, w) in enumerate(dims):
                if h > H or w > W:
                    raise ValueError(f"to_torch: image {idx[k]} is {h} x {w}, larger than pad_to = ({H}, {W})")
            result = torch.zeros((len(idx),) + shape(H, W), dtype=dtype, device=dev)
            views = [crop(result[k], h, w) for k, (h, w) in enumerate(dims)]
        elif stack:
            for k, d in enumerate(dims):
                if d != dims[0]:
                    raise ValueError(f"to_torch: stack=True, but image {idx[k]} is {d[0]} x {d[1]} and image {idx[0]} is {dims[0][0]} x {dims[0][1]}")
            result = torch.empty((len(idx),) + (shape(*dims[0]) if dims else shape(0, 0)), dtype=dtype, device=dev)
            views = [result[k] for k in range(len(idx))]
        else:
            flat = torch.empty(sum(3 * h * w for h, w in dims), dtype=dtype, device=dev)
            views, off = [], 0
            for h, w in dims:
                views.append(flat[off:off + 3 * h * w].view(shape(h, w)))
                off += 3 * h * w
            result = views
        if not idx:
            return result
        elem = 4 if is_f32 else 1
        dst = (capi.PackDst * len(idx))()
        for k, t in enumerate(views):
            st = t.stride()
            if st[2] != 1 or (not chw and st[1] != 3) or min(st) < 1:
                raise ValueError(f"to_torch: destination {k}: the inner dimensions must be contiguous (strides {st})")
            dst[k].ptr = t.data_ptr()
            dst[k].row_pitch = (st[1] if chw else st[0]) * elem
            dst[k].plane_pitch = st[0] * elem if chw else 0
        # memory the allocator hands out may still have work pending on torch's current stream (the zero fill of pad_to among it)
        cur = torch.cuda.current_stream(dev)
        if self._stream != cur.cuda_stream:
            cur.synchronize()
        ind = (C.c_int * len(idx))(*idx)
        if pixels == "libjpeg" and any(x != 1 for x in red):
            for denom in sorted(set(red)):                        # one call per value: at most four
                ks = [k for k in range(len(idx)) if red[k] == denom]
                sub = (capi.PackDst * len(ks))()
                for j, k in enumerate(ks):
                    sub[j].ptr, sub[j].row_pitch, sub[j].plane_pitch = dst[k].ptr, dst[k].row_pitch, dst[k].plane_pitch
                self._chk(self._lib.jsnoop_batch_pack_ijg_scaled(self._h, C.byref(spec), denom, (C.c_int * len(ks))(*[idx[k] for k in ks]), len(ks), sub),
                          "batch_pack_ijg_scaled")
        elif pixels == "libjpeg":
            self._chk(self._lib.jsnoop_batch_pack_ijg(self._h, C.byref(spec), ind, len(idx), dst), "batch_pack_ijg")
        else:
            self._chk(self._lib.jsnoop_batch_pack(self._h, C.byref(spec), ind, len(idx), dst), "batch_pack")
        self.sync()                              # waits for the batch's stream alone
        return result

    def ijg_renderable(self, i) -> bool:
        """Whether to_torch(pixels="libjpeg") renders image i (jsnoop_batch_ijg_renderable: precision 8; one component, or Y Cb Cr as 4:4:4, 4:2:2
        or 4:2:0).  Host arithmetic; False leaves the reason in last_error()."""
        return int(self._lib.jsnoop_batch_ijg_renderable(self._h, int(i))) == 1

    def ijg_scaled_size(self, i, reduce):
        """(h, w) of image i as to_torch(pixels="libjpeg", reduce=reduce) gives it: ceil(dim_y / reduce), ceil(dim_x / reduce)
        (jsnoop_batch_ijg_scaled_size; host arithmetic).  RuntimeError for an image that is not renderable or a reduce other than 1, 2, 4, 8."""
        w, h = C.c_uint(0), C.c_uint(0)
        self._chk(self._lib.jsnoop_batch_ijg_scaled_size(self._h, int(i), int(reduce), C.byref(w), C.byref(h)), "batch_ijg_scaled_size")
        return int(h.value), int(w.value)

    def reduce_for(self, i, size) -> int:
        """The denominator Pillow's Image.draft chooses for image i and a target size=(H, W): the largest of 8, 4, 2, 1 not above
        min(dim_x // W, dim_y // H) -- the smallest reduced picture that is still at least as large as the target."""
        H, W = int(size[0]), int(size[1])
        if H < 1 or W < 1:
            raise ValueError("reduce_for: size must be (H, W), each at least 1")
        inf = self.info(int(i))
        q = min(inf["dim_x"] // W, inf["dim_y"] // H)
        return next(s for s in (8, 4, 2, 1) if q >= s or s == 1)

    def _to_torch_resized(self, torch, idx, spec, chw, dtype, dev, stack, pad_to, out, size, filter, roi):
        """to_torch(size=...): one [N, ...] tensor filled by one jsnoop_batch_pack_resized.  The batch has been synchronised."""
        if stack or pad_to is not None:
            raise ValueError("to_torch: size= excludes stack and pad_to (the result is one tensor already)")
        filters = {"nearest": capi.RESIZE_NEAREST, "bilinear": capi.RESIZE_BILINEAR, "area": capi.RESIZE_AREA}
        if filter not in filters:
            raise ValueError("to_torch: filter must be \"bilinear\", \"nearest\" or \"area\"")
        try:
            H, W = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError("to_torch: size must be (H, W)") from None
        if not (1 <= H <= 32767 and 1 <= W <= 32767):
            raise ValueError(f"to_torch: size = ({H}, {W}): each of 1 .. 32767")
        n = len(idx)
        if roi is None:
            rois = [(0, 0, 0, 0)] * n
        elif len(roi) == 4 and all(np.isscalar(v) for v in roi):
            rois = [tuple(int(v) for v in roi)] * n
        else:
            rois = [tuple(int(v) for v in r) for r in roi]
            if len(rois) != n or any(len(r) != 4 for r in rois):
                raise ValueError(f"to_torch: roi must be one (x, y, w, h) or a list of {n} of them")
        for k, (x, y, w, h) in enumerate(rois):
            inf = self.info(idx[k])
            if roi is not None and (min(x, y) < 0 or w < 1 or h < 1 or x + w > inf["dim_x"] or y + h > inf["dim_y"]):
                raise ValueError(f"to_torch: roi {(x, y, w, h)} leaves image {idx[k]} of {inf['dim_x']} x {inf['dim_y']}")
        shape = (n, 3, H, W) if chw else (n, H, W, 3)
        if out is not None:
            if not isinstance(out, torch.Tensor) or tuple(out.shape) != shape:
                raise ValueError(f"to_torch: with size= out must be one tensor of shape {list(shape)}")
            if out.device != dev:
                raise ValueError(f"to_torch: out is on {out.device}, the batch on {dev}")
            if out.dtype != dtype:
                raise ValueError(f"to_torch: out is {out.dtype}, asked for {dtype}")
            result = out
        else:
            result = torch.empty(shape, dtype=dtype, device=dev)
        if not n:
            return result
        elem = 4 if dtype == torch.float32 else 1
        dst = (capi.ResizeDst * n)()
        for k in range(n):
            t = result[k]
            st = t.stride()
            if st[2] != 1 or (not chw and st[1] != 3) or min(st) < 1:
                raise ValueError(f"to_torch: destination {k}: the inner dimensions must be contiguous (strides {st})")
            dst[k].ptr = t.data_ptr()
            dst[k].row_pitch = (st[1] if chw else st[0]) * elem
            dst[k].plane_pitch = st[0] * elem if chw else 0
            dst[k].out_w, dst[k].out_h = W, H
            dst[k].roi_x, dst[k].roi_y, dst[k].roi_w, dst[k].roi_h = rois[k]
        cur = torch.cuda.current_stream(dev)
        if self._stream != cur.cuda_stream:
            cur.synchronize()
        ind = (C.c_int * n)(*idx)
        self._chk(self._lib.jsnoop_batch_pack_resized(self._h, C.byref(spec), filters[filter], ind, n, dst), "batch_pack_resized")
        self.sync()                              # waits for the batch's stream alone
        return result

    def color_stats(self, i, histo_en=True):
        """bHistoEn (or only bStatClipEn) statistics of image i: the JSNOOP_STATS_WORDS record of include/jsnoop_gpu.h."""
        out = np.zeros(2482, np.uint32)
        self._chk(self._lib.jsnoop_batch_color_stats(self._h, i, int(histo_en), out.ctypes.data), "batch_color_stats")
        return out

    def planes(self, i):
        inf = self.info(i)
        shp = (inf["blk_ymax"] * 8, inf["blk_xmax"] * 8)
        ps = [np.zeros(shp, np.int16) for _ in range(3)]
        self._chk(self._lib.jsnoop_batch_read_planes(self._h, i, *[p.ctypes.data for p in ps]), "batch_read_planes")
        return ps[: inf["ncomp"]]

    def coefs(self, i):
        inf = self.info(i)
        out = np.empty((inf["total_blocks"], 64), np.int16)
        self._chk(self._lib.jsnoop_batch_read_coefs(self._h, i, out.ctypes.data, inf["total_blocks"]), "batch_read_coefs")
        return out

    def coef_grid(self, i, comp):
        """(bw, bh): the block grid of component comp (0 = Y) of image i, MCU padding included (jsnoop_batch_coef_grid)."""
        bw, bh = C.c_uint(), C.c_uint()
        self._chk(self._lib.jsnoop_batch_coef_grid(self._h, int(i), int(comp), C.byref(bw), C.byref(bh)), "batch_coef_grid")
        return int(bw.value), int(bh.value)

    def dqt(self, i, comp):
        """The 64 multipliers the decode used for component comp of image i, natural order (jsnoop_batch_image_dqt): every coefficient is
        int16(level * dqt[k])."""
        out = np.zeros(64, np.uint16)
        self._chk(self._lib.jsnoop_batch_image_dqt(self._h, int(i), int(comp), out.ctypes.data_as(C.POINTER(C.c_uint16))), "batch_image_dqt")
        return out

    def coefs_to_torch(self, images=None, comps=None, layout="blocks", dtype=None, zigzag=False, out=None):
        """The DCT coefficients of the decoded images as torch tensors on the batch's device, filled by ONE jsnoop_batch_pack_coefs -- no
        coefficient crosses PCIe.  Returns, per listed image, a list with one tensor per component.

        images: indices into the batch, any order (None = all).  comps: the components wanted of every image, counted from 0 = Y (None = all
        the image has).  layout "blocks" -> [bh, bw, 64], "freq" -> [64, bh, bw], (bw, bh) = coef_grid(i, comp): blocks in raster order of the
        component's own grid, MCU padding included.  Natural index 0 holds the cumulative DC, the others the dequantised values
        int16(level * dqt(i, comp)[k]).  dtype: torch.int16 (default) or torch.float32 (exact).  zigzag: position z holds natural index
        zigzag[z] instead of k = row * 8 + column.  out=: a list (per image) of lists (per component) of tensors of exactly these shapes, on the
        batch's device, of the dtype asked for, inner dimensions contiguous (the outer ones may be strided); returned as it is.

        Calls sync() first (damaged files arrive repaired; after a DC-only fast-form decode the call decodes once more, last_form() goes
        2 -> 1), synchronises torch's current stream before the launch unless the batch runs on it, and waits for the batch's stream before it
        returns: the tensors are ready."""
        import torch
        n_all = len(self)
        idx = list(range(n_all)) if images is None else [int(i) for i in images]
        for i in idx:
            if not 0 <= i < n_all:
                raise IndexError(f"coefs_to_torch: image index {i} out of range, the batch holds {n_all}")
        if layout not in ("blocks", "freq"):
            raise ValueError("coefs_to_torch: layout must be \"blocks\" or \"freq\"")
        if dtype is None:
            dtype = torch.int16
        if dtype not in (torch.int16, torch.float32):
            raise ValueError("coefs_to_torch: dtype must be torch.int16 or torch.float32")
        freq, elem = layout == "freq", 4 if dtype == torch.float32 else 2
        spec = capi.CoefSpec()
        self._lib.jsnoop_coef_spec_defaults(C.byref(spec))
        spec.layout = capi.COEF_FREQ if freq else capi.COEF_BLOCKS
        spec.dtype = capi.COEF_F32 if dtype == torch.float32 else capi.COEF_I16
        spec.order = capi.COEF_ZIGZAG if zigzag else capi.COEF_NATURAL
        self.sync()
        dev = torch.device("cuda", self.device())
        want, per_image = [], []                     # (image, component, shape) of every destination, in the order of the result; destinations per listed image
        for i in idx:
            ncomp = self.info(i)["ncomp"]
            cs = list(range(ncomp)) if comps is None else [int(c) for c in comps]
            per_image.append(len(cs))
            for c in cs:
                if not 0 <= c < ncomp:
                    raise IndexError(f"coefs_to_torch: component {c} of image {i}, which has {ncomp}")
                bw, bh = self.coef_grid(i, c)
                want.append((i, c, (64, bh, bw) if freq else (bh, bw, 64)))
        if out is not None:
            rows = [list(r) for r in out]
            if len(rows) != len(idx) or [len(r) for r in rows] != per_image:
                raise ValueError(f"coefs_to_torch: out must hold {len(idx)} lists of {per_image} tensors")
            views, result = [t for r in rows for t in r], out
            for k, t in enumerate(views):
                i, c, shp = want[k]
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != shp:
                    raise ValueError(f"coefs_to_torch: out for component {c} of image {i} must be a tensor of shape {list(shp)}")
                if t.device != dev:
                    raise ValueError(f"coefs_to_torch: out for component {c} of image {i} is on {t.device}, the batch on {dev}")
                if t.dtype != dtype:
                    raise ValueError(f"coefs_to_torch: out for component {c} of image {i} is {t.dtype}, asked for {dtype}")
        else:
            sizes = [shp[0] * shp[1] * shp[2] for _, _, shp in want]
            flat = torch.empty(sum(sizes), dtype=dtype, device=dev)
            views, off = [], 0
            for (_, _, shp), sz in zip(want, sizes):
                views.append(flat[off:off + sz].view(shp))
                off += sz
            result, k = [], 0
            for m in per_image:
                result.append(views[k:k + m])
                k += m
        if not want:
            return result
        dst = (capi.CoefDst * len(want))()
        for k, t in enumerate(views):
            st, shp = t.stride(), want[k][2]
            ok = (st[2] == 1 and st[1] >= shp[2] and st[0] >= st[1] * shp[1]) if freq else (st[2] == 1 and st[1] == 64 and st[0] >= 64 * shp[1])
            if not ok and t.numel():
                raise ValueError(f"coefs_to_torch: destination {k}: the inner dimensions must be contiguous (strides {st})")
            dst[k].ptr = t.data_ptr()
            dst[k].row_pitch = (st[1] if freq else st[0]) * elem
            dst[k].plane_pitch = st[0] * elem if freq else 0
            dst[k].comp, dst[k].reserved = want[k][1], 0
        cur = torch.cuda.current_stream(dev)
        if self._stream != cur.cuda_stream:
            cur.synchronize()
        ind = (C.c_int * len(want))(*[w[0] for w in want])
        self._chk(self._lib.jsnoop_batch_pack_coefs(self._h, C.byref(spec), ind, len(want), dst), "batch_pack_coefs")
        self.sync()                              # waits for the batch's stream alone
        return result

    def _plane_spec(self, torch, native, dtype, scale, bias, what):
        if dtype is None:
            dtype = torch.int16
        codes = {torch.int16: capi.PLANE_I16, torch.uint8: capi.PLANE_U8, torch.float32: capi.PLANE_F32}
        if dtype not in codes:
            raise ValueError(f"{what}: dtype must be torch.int16, torch.uint8 or torch.float32")
        if dtype != torch.float32 and (scale is not None or bias is not None):
            raise ValueError(f"{what}: scale / bias belong to dtype=torch.float32")
        spec = capi.PlaneSpec()
        self._lib.jsnoop_plane_spec_defaults(C.byref(spec))
        spec.res = capi.PLANE_NATIVE if native else capi.PLANE_FULL
        spec.dtype = codes[dtype]
        for name, v in (("scale", scale), ("bias", bias)):
            if v is None:
                continue
            vals = [float(v)] * 3 if np.isscalar(v) else [float(x) for x in v]
            if len(vals) != 3:
                raise ValueError(f"{what}: {name} must be a number or three, one per component")
            for c in range(3):
                getattr(spec, name)[c] = vals[c]
        return spec, dtype

    def plane_size(self, i, comp, native=False):
        """(h, w) of component comp (0 = Y) of image i as planes_to_torch gives it: the SOF dimensions, or with native=True the component's own
        grid, ceil(dim / replication factor) each way (jsnoop_batch_plane_size)."""
        spec = capi.PlaneSpec()
        self._lib.jsnoop_plane_spec_defaults(C.byref(spec))
        spec.res = capi.PLANE_NATIVE if native else capi.PLANE_FULL
        w, h = C.c_uint(), C.c_uint()
        self._chk(self._lib.jsnoop_batch_plane_size(self._h, C.byref(spec), int(i), int(comp), C.byref(w), C.byref(h)), "batch_plane_size")
        return int(h.value), int(w.value)

    def planes_to_torch(self, images=None, comps=None, native=False, dtype=None, scale=None, bias=None, stack=False, out=None):
        """The retained Y / Cb / Cr planes of the decoded images (want_planes) as torch tensors on the batch's device, filled by ONE
        jsnoop_batch_pack_planes -- no sample crosses PCIe.  Returns, per listed image, a list with one [h, w] tensor per component.

        images: indices into the batch, any order (None = all).  comps: the components wanted of every image, counted from 0 = Y (None = all
        the image has).  native=False: every plane cropped to the SOF dimensions, chroma replicated as the decode left it; native=True: every
        component on its own grid, (h, w) = plane_size(i, comp, native=True) -- 4:2:0 as three planes.  dtype: torch.int16 (default: the
        plane's samples, three fractional bits, un-clamped), torch.uint8 (min(max((v + 1024) / 8, 0), 255), the 8-bit sample the colour
        conversion starts from) or torch.float32 (float(v) * scale[comp] + bias[comp]; scale / bias a number or three, defaults 1 and 0; one
        rounded multiply, then one rounded add).  stack=True: one [N, C, H, W] tensor (ValueError naming the first plane whose shape
        differs).  out=: a list (per image) of lists (per component) of tensors of exactly these shapes -- or with stack=True one
        [N, C, H, W] tensor -- on the batch's device, of the dtype asked for, rows contiguous (the outer dimensions may be strided);
        returned as it is.

        Calls sync() first (damaged files arrive repaired; the call never decodes again), synchronises torch's current stream before the
        launch unless the batch runs on it, and waits for the batch's stream before it returns: the tensors are ready."""
        import torch
        n_all = len(self)
        idx = list(range(n_all)) if images is None else [int(i) for i in images]
        for i in idx:
            if not 0 <= i < n_all:
                raise IndexError(f"planes_to_torch: image index {i} out of range, the batch holds {n_all}")
        spec, dtype = self._plane_spec(torch, native, dtype, scale, bias, "planes_to_torch")
        elem = {torch.int16: 2, torch.uint8: 1, torch.float32: 4}[dtype]
        self.sync()
        dev = torch.device("cuda", self.device())
        want, per_image = [], []                     # (image, component, shape) of every destination, in the order of the result; destinations per listed image
        for i in idx:
            ncomp = self.info(i)["ncomp"]
            cs = list(range(ncomp)) if comps is None else [int(c) for c in comps]
            per_image.append(len(cs))
            for c in cs:
                if not 0 <= c < ncomp:
                    raise IndexError(f"planes_to_torch: component {c} of image {i}, which has {ncomp}")
                want.append((i, c, self.plane_size(i, c, native)))
        if stack:
            for i, c, shp in want:
                if shp != want[0][2]:
                    raise ValueError(f"planes_to_torch: stack=True, but component {c} of image {i} is {shp[0]} x {shp[1]} and component {want[0][1]} of "
                                     f"image {want[0][0]} is {want[0][2][0]} x {want[0][2][1]}")
            if len(set(per_image)) > 1:
                k = next(k for k, m in enumerate(per_image) if m != per_image[0])
                raise ValueError(f"planes_to_torch: stack=True, but image {idx[k]} gives {per_image[k]} planes and image {idx[0]} gives {per_image[0]}")
            full = (len(idx), per_image[0] if per_image else 0) + (want[0][2] if want else (0, 0))
            if out is not None:
                if not isinstance(out, torch.Tensor) or tuple(out.shape) != full:
                    raise ValueError(f"planes_to_torch: out must be a tensor of shape {list(full)}")
                result = out
            else:
                result = torch.empty(full, dtype=dtype, device=dev)
            views = [result[k][j] for k in range(full[0]) for j in range(full[1])]
        elif out is not None:
            rows = [list(r) for r in out]
            if len(rows) != len(idx) or [len(r) for r in rows] != per_image:
                raise ValueError(f"planes_to_torch: out must hold {len(idx)} lists of {per_image} tensors")
            views, result = [t for r in rows for t in r], out
            for k, t in enumerate(views):
                i, c, shp = want[k]
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != shp:
                    raise ValueError(f"planes_to_torch: out for component {c} of image {i} must be a tensor of shape {list(shp)}")
        else:
            # every plane starts at a multiple of 16 bytes of one allocation
            sizes = [-(-(shp[0] * shp[1] * elem) // 16) * 16 // elem for _, _, shp in want]
            flat = torch.empty(sum(sizes), dtype=dtype, device=dev)
            views, off = [], 0
            for (_, _, shp), sz in zip(want, sizes):
                views.append(flat[off:off + shp[0] * shp[1]].view(shp))
                off += sz
            result, k = [], 0
            for m in per_image:
                result.append(views[k:k + m])
                k += m
        if out is not None:
            for k, t in enumerate(views):
                i, c, _ = want[k]
                if t.device != dev:
                    raise ValueError(f"planes_to_torch: out for component {c} of image {i} is on {t.device}, the batch on {dev}")
                if t.dtype != dtype:
                    raise ValueError(f"planes_to_torch: out for component {c} of image {i} is {t.dtype}, asked for {dtype}")
        if not want:
            return result
        dst = (capi.PlaneDst * len(want))()
        for k, t in enumerate(views):
            st, shp = t.stride(), want[k][2]
            if not (st[1] == 1 and st[0] >= shp[1]) and t.numel():
                raise ValueError(f"planes_to_torch: destination {k}: the rows must be contiguous (strides {st})")
            dst[k].ptr = t.data_ptr()
            dst[k].row_pitch = st[0] * elem
            dst[k].comp, dst[k].reserved = want[k][1], 0
        cur = torch.cuda.current_stream(dev)
        if self._stream != cur.cuda_stream:
            cur.synchronize()
        ind = (C.c_int * len(want))(*[w[0] for w in want])
        self._chk(self._lib.jsnoop_batch_pack_planes(self._h, C.byref(spec), ind, len(want), dst), "batch_pack_planes")
        self.sync()                              # waits for the batch's stream alone
        return result

    def stats_to_torch(self, images=None, histo_en=True, out=None, totals=False):
        """The bHistoEn (histo_en=False: only bStatClipEn) colour statistics of the decoded images as ONE int32 [n, 2482] tensor on the batch's
        device: row k is what color_stats(images[k], histo_en) returns (view it with stats_fields), computed from the retained planes by one
        jsnoop_batch_pack_stats -- two launches for the whole list, no word crosses PCIe.  The batch needs want_planes.

        images: indices into the batch, any order, repeats allowed (None = all).  out=: an int32 tensor [n, >= 2482] on the batch's device whose
        rows are contiguous (the outer dimension may be strided; columns from 2482 on keep their content); returned as it is.  totals=True:
        returns (rows, totals), totals an int32 [n, 6] tensor: how many YCC range events of each kind the image has in all, indexed like words
        37..42 (the row's counters stop at 10 together).

        Calls sync() first (damaged files arrive repaired; never decodes again, last_form() is unchanged), synchronises torch's current stream
        before the launches unless the batch runs on it, and waits for the batch's stream before it returns: the tensors are ready."""
        import torch
        n_all = len(self)
        idx = list(range(n_all)) if images is None else [int(i) for i in images]
        for i in idx:
            if not 0 <= i < n_all:
                raise IndexError(f"stats_to_torch: image index {i} out of range, the batch holds {n_all}")
        n = len(idx)
        self.sync()
        dev = torch.device("cuda", self.device())
        if out is None:
            rows = torch.empty((n, capi.STATS_WORDS), dtype=torch.int32, device=dev)
        else:
            rows = out
            if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[0] != n or rows.shape[1] < capi.STATS_WORDS:
                raise ValueError(f"stats_to_torch: out must be a tensor of shape [{n}, >= {capi.STATS_WORDS}]")
            if rows.device != dev or rows.dtype != torch.int32:
                raise ValueError(f"stats_to_torch: out is {rows.dtype} on {rows.device}, wanted torch.int32 on {dev}")
            if n and (rows.stride(1) != 1 or (n > 1 and rows.stride(0) < capi.STATS_WORDS)):
                raise ValueError(f"stats_to_torch: the rows of out must be contiguous and not overlap (strides {rows.stride()})")
        tot = torch.empty((n, 6), dtype=torch.int32, device=dev) if totals else None
        if n:
            cur = torch.cuda.current_stream(dev)
            if self._stream != cur.cuda_stream:
                cur.synchronize()
            ind = (C.c_int * n)(*idx)
            pitch = rows.stride(0) if n > 1 else 0
            self._chk(self._lib.jsnoop_batch_pack_stats(self._h, int(bool(histo_en)), ind, n, rows.data_ptr(), pitch, tot.data_ptr() if totals else None), "batch_pack_stats")
            self.sync()                          # waits for the batch's stream alone
        return (rows, tot) if totals else rows

    def stats_all(self, images=None, histo_en=True):
        """The same rows as a numpy uint32 [n, 2482] array in host memory (jsnoop_batch_read_stats: one D2H copy, one wait)."""
        n_all = len(self)
        idx = list(range(n_all)) if images is None else [int(i) for i in images]
        for i in idx:
            if not 0 <= i < n_all:
                raise IndexError(f"stats_all: image index {i} out of range, the batch holds {n_all}")
        out = np.zeros((len(idx), capi.STATS_WORDS), np.uint32)
        if idx:
            self.sync()
            ind = (C.c_int * len(idx))(*idx)
            self._chk(self._lib.jsnoop_batch_read_stats(self._h, int(bool(histo_en)), ind, len(idx), out.ctypes.data), "batch_read_stats")
        return out

    def _coef_hist_pairs(self, images, comps, what):
        """The (image, component) pairs of one coefficient-histogram call, checked: images and comps both given -> the pairs (images[k], comps[k]);
        comps None -> every component of every listed image (images None = all); images None -> the listed components of every image."""
        n_all = len(self)
        if images is not None and comps is not None:
            im, cs = [int(i) for i in images], [int(c) for c in comps]
            if len(im) != len(cs):
                raise ValueError(f"{what}: images and comps name pairs and must be equally long ({len(im)} and {len(cs)})")
            pairs = list(zip(im, cs))
        else:
            idx = list(builtins.range(n_all)) if images is None else [int(i) for i in images]
            for i in idx:
                if not 0 <= i < n_all:
                    raise IndexError(f"{what}: image index {i} out of range, the batch holds {n_all}")
            pairs = [(i, c) for i in idx for c in (builtins.range(self.info(i)["ncomp"]) if comps is None else [int(c) for c in comps])]
        for i, c in pairs:
            if not 0 <= i < n_all:
                raise IndexError(f"{what}: image index {i} out of range, the batch holds {n_all}")
            if not 0 <= c < self.info(i)["ncomp"]:
                raise IndexError(f"{what}: component {c} of image {i}, which has {self.info(i)['ncomp']}")
        return pairs

    def _coef_hist_spec(self, range, quantised, zigzag, what):
        if not 1 <= int(range) <= capi.COEF_HIST_RANGE_MAX:
            raise ValueError(f"{what}: range must be 1 .. {capi.COEF_HIST_RANGE_MAX}")
        spec = capi.CoefHistSpec()
        self._lib.jsnoop_coef_hist_spec_defaults(C.byref(spec))
        spec.order = capi.COEF_ZIGZAG if zigzag else capi.COEF_NATURAL
        spec.quantised, spec.range = int(bool(quantised)), int(range)
        return spec

    def coef_hist_to_torch(self, images=None, comps=None, range=127, quantised=True, zigzag=False, out=None):
        """The histogram of every DCT frequency of the listed (image, component) pairs as ONE int32 [n, 64 * (2 * range + 1) + 128] tensor on the
        batch's device, filled by one jsnoop_batch_pack_coef_hist -- no coefficient tensor is written, no word crosses PCIe.  Returns
        (pairs, rows): row k belongs to pairs[k] = (image, component); view it with coef_hist_fields(row, range).

        images / comps: both given -> the pairs (images[k], comps[k]), any order, repeats allowed; comps None -> every component of every listed
        image (images None = all images); images None -> the listed components of every image.  A row counts, per position 0..63 (natural index, or
        zig-zag position with zigzag=True), the blocks of the component's grid (MCU padding included) by clamp(x, -range, range) + range, x the
        quantised level (the arena's int16 divided by dqt(i, comp)[k], truncating toward zero; natural index 0 is the cumulative DC) or with
        quantised=False the dequantised value itself; behind the histograms the smallest and the largest unclamped x of every position.
        out=: an int32 tensor [n, >= row length] on the batch's device whose rows are contiguous (the outer dimension may be strided; columns
        behind the row keep their content); returned as it is.

        Calls sync() first (damaged files arrive repaired; after a DC-only fast-form decode the call decodes once more, last_form() goes
        2 -> 1), synchronises torch's current stream before the launch unless the batch runs on it, and waits for the batch's stream before it
        returns: the tensor is ready."""
        import torch
        spec = self._coef_hist_spec(range, quantised, zigzag, "coef_hist_to_torch")
        pairs = self._coef_hist_pairs(images, comps, "coef_hist_to_torch")
        n, words = len(pairs), capi.coef_hist_words(int(range))
        self.sync()
        dev = torch.device("cuda", self.device())
        if out is None:
            rows = torch.empty((n, words), dtype=torch.int32, device=dev)
        else:
            rows = out
            if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.shape[0] != n or rows.shape[1] < words:
                raise ValueError(f"coef_hist_to_torch: out must be a tensor of shape [{n}, >= {words}]")
            if rows.device != dev or rows.dtype != torch.int32:
                raise ValueError(f"coef_hist_to_torch: out is {rows.dtype} on {rows.device}, wanted torch.int32 on {dev}")
            if n and (rows.stride(1) != 1 or (n > 1 and rows.stride(0) < words)):
                raise ValueError(f"coef_hist_to_torch: the rows of out must be contiguous and not overlap (strides {rows.stride()})")
        if n:
            cur = torch.cuda.current_stream(dev)
            if self._stream != cur.cuda_stream:
                cur.synchronize()
            ind, cmp_ = (C.c_int * n)(*[i for i, _ in pairs]), (C.c_int * n)(*[c for _, c in pairs])
            pitch = rows.stride(0) if n > 1 else 0
            self._chk(self._lib.jsnoop_batch_pack_coef_hist(self._h, C.byref(spec), ind, cmp_, n, rows.data_ptr(), pitch), "batch_pack_coef_hist")
            self.sync()                          # waits for the batch's stream alone
        return pairs, rows

    def coef_hist_all(self, images=None, comps=None, range=127, quantised=True, zigzag=False):
        """(pairs, rows): the same rows as a numpy uint32 [n, row length] array in host memory (jsnoop_batch_read_coef_hist: one D2H copy, one wait);
        minima and maxima are signed: view them as int32 (coef_hist_fields does)."""
        spec = self._coef_hist_spec(range, quantised, zigzag, "coef_hist_all")
        pairs = self._coef_hist_pairs(images, comps, "coef_hist_all")
        out = np.zeros((len(pairs), capi.coef_hist_words(int(range))), np.uint32)
        if pairs:
            self.sync()
            n = len(pairs)
            ind, cmp_ = (C.c_int * n)(*[i for i, _ in pairs]), (C.c_int * n)(*[c for _, c in pairs])
            self._chk(self._lib.jsnoop_batch_read_coef_hist(self._h, C.byref(spec), ind, cmp_, n, out.ctypes.data), "batch_read_coef_hist")
        return pairs, out

    def dib_checksums(self):
        out = np.zeros(len(self), np.uint64)
        self._chk(self._lib.jsnoop_batch_dib_hashes(self._h, out.ctypes.data), "batch_dib_hashes")
        return out

    # --- what DecodeScanImg leaves behind besides pixels, per image (the per-file pass of DoBatchFileProcess) -----------------
    def add(self, tables: "CimgDecode", data: bytes, scan_start: int) -> int:
        """Adds one image under the table / frame state `tables` holds (after the setter calls of its header), like jsnoop_batch_add."""
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        h = getattr(tables, "_h", None) or getattr(tables, "h", None) or tables
        return self._chk(self._lib.jsnoop_batch_add(self._h, h, C.cast(buf, C.c_void_p), len(data), scan_start), "batch_add")

    def enable_log(self, on=True): self._chk(self._lib.jsnoop_batch_enable_log(self._h, int(on)), "batch_enable_log")

    def side_outputs(self, i, bright=True):
        """MCU file map, block-DC maps, Huffman code-length histogram, status words, brightest pixel / average Y of image i."""
        inf = self.info(i)
        nmcu, nblk = inf["mcu_xmax"] * inf["mcu_ymax"], inf["blk_xmax"] * inf["blk_ymax"]
        mcu = np.zeros(nmcu, np.uint32)
        dcs = [np.zeros(nblk, np.int16) for _ in range(3)]
        histo = np.zeros(2 * 4 * 17, np.uint32)
        st, ba = (C.c_uint * 8)(), (C.c_int * 10)()
        self._chk(self._lib.jsnoop_batch_side_outputs(self._h, i, mcu.ctypes.data, dcs[0].ctypes.data, dcs[1].ctypes.data, dcs[2].ctypes.data, histo.ctypes.data,
                                                      st, ba if bright else None), "batch_side_outputs")
        keys = "scan_bad scan_end rst_count num_pixels pos0 align warn_bad first".split()
        return {"mcu_map": mcu.reshape(inf["mcu_ymax"], inf["mcu_xmax"]),
                "blk_dc": [d.reshape(inf["blk_ymax"], inf["blk_xmax"]) if (c == 0 or inf["ncomp"] == 3) else None for c, d in enumerate(dcs)],
                "dht_histo": histo.reshape(2, 4, 17), "status": dict(zip(keys, st)), "bright_avg": list(ba) if bright else None}

    def log_lines(self, i, histo_en=False, stat_clip_en=False, quiet=False):
        """The text DecodeScanImg writes to CDocLog for image i, as (level, line) pairs."""
        out = []
        cb = capi.LOG_FN(lambda _u, lvl, txt: out.append((lvl, txt.decode(errors="replace"))))
        self._chk(self._lib.jsnoop_batch_log(self._h, i, int(histo_en), int(stat_clip_en), int(quiet), cb, None), "batch_log")
        return out

    def _export(self, images, jfif, what, huffman="annex_k", restart=0, progressive=False):
        n_all = len(self)
        idx = list(range(n_all)) if images is None else [int(i) for i in images]
        for i in idx:
            if not 0 <= i < n_all:
                raise IndexError(f"{what}: image index {i} out of range, the batch holds {n_all}")
        rst = capi.export_restart(self._lib, restart)                 # (refuses what is no restart value before anything is done)
        prog = capi.export_progressive(self._lib, progressive)
        spec = capi.ExportSpec()
        self._lib.jsnoop_export_spec_defaults(C.byref(spec))
        spec.jfif = 1 if jfif else 0
        self.sync()
        ind = (C.c_int * max(len(idx), 1))(*idx)
        if prog.mode != capi.PROGRESSIVE_OFF:
            self._chk(self._lib.jsnoop_batch_export_jpeg_prog(self._h, C.byref(spec), C.byref(capi.export_coding(self._lib, huffman)), C.byref(rst), C.byref(prog), ind, len(idx)),
                      "batch_export_jpeg_prog")
        elif rst.mode != capi.RESTART_NONE:
            self._chk(self._lib.jsnoop_batch_export_jpeg_rst(self._h, C.byref(spec), C.byref(capi.export_coding(self._lib, huffman)), C.byref(rst), ind, len(idx)),
                      "batch_export_jpeg_rst")
        elif huffman == "annex_k":
            self._chk(self._lib.jsnoop_batch_export_jpeg(self._h, C.byref(spec), ind, len(idx)), "batch_export_jpeg")
        else:
            self._chk(self._lib.jsnoop_batch_export_jpeg_coded(self._h, C.byref(spec), C.byref(capi.export_coding(self._lib, huffman)), ind, len(idx)), "batch_export_jpeg_coded")
        return self.export_results()

    def export_tables(self, k):
        """Entry k of the last export_jpeg(huffman="optimal"): one dict per slot (2 * table id + class; two for a grey image, else four) with freq (256
        symbol counts), counts (codes per length 1..16) and symbols (in code order) of the table the device built and wrote (jsnoop_batch_export_tables)."""
        res = self.export_results()
        if not 0 <= k < len(res):
            raise IndexError(f"export_tables: entry {k} out of range, the last export holds {len(res)}")
        out = []
        for slot in range(2 if self.info(res[k]["image"])["ncomp"] == 1 else 4):
            counts, syms, freq, n = (C.c_uint8 * 16)(), (C.c_uint8 * 256)(), (C.c_uint32 * 256)(), C.c_uint32()
            self._chk(self._lib.jsnoop_batch_export_tables(self._h, k, slot, counts, syms, C.byref(n), freq), "batch_export_tables")
            out.append(dict(slot=slot, freq=list(freq), counts=list(counts), symbols=list(syms[:n.value])))
        return out

    def export_restart(self, k):
        """Entry k of the last export: (Ri, intervals) -- the restart interval in MCUs it was written with (0: none) and the number of intervals of its file
        (0 where no file was written) (jsnoop_batch_export_restart)."""
        ri, n = C.c_uint32(), C.c_uint64()
        self._chk(self._lib.jsnoop_batch_export_restart(self._h, int(k), C.byref(ri), C.byref(n)), "batch_export_restart")
        return int(ri.value), int(n.value)

    def export_scans(self, k):
        """Entry k of the last export_jpeg(progressive=...): one dict per scan of its file with comps (list of component indices), ss, se, ah, al, ri (the
        scan's restart interval in its own units), intervals, sos_offset (where its SOS marker stands in the file) and data_bytes (its entropy-coded
        data, stuffing and RSTn included); empty for a baseline or absent file (jsnoop_batch_export_scan_info)."""
        out = []
        for i in range(self._lib.jsnoop_batch_export_scan_count(self._h, int(k))):
            sc, ri, n, sos, nb = capi.ExportScan(), C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
            self._chk(self._lib.jsnoop_batch_export_scan_info(self._h, int(k), i, C.byref(sc), C.byref(ri), C.byref(n), C.byref(sos), C.byref(nb)), "batch_export_scan_info")
            out.append(dict(comps=[c for c in range(8) if sc.comps >> c & 1], ss=sc.ss, se=sc.se, ah=sc.ah, al=sc.al, ri=int(ri.value), intervals=int(n.value),
                            sos_offset=int(sos.value), data_bytes=int(nb.value)))
        return out

    def export_scan_tables(self, k, scan):
        """The Huffman tables the device built for scan `scan` of entry k of the last progressive export: one dict per table (a DC first scan: one per scan
        component, in the scan's order; an AC scan: one; a refinement scan: none) with freq, counts and symbols as export_tables returns them
        (jsnoop_batch_export_scan_tables)."""
        scans = self.export_scans(k)
        if not 0 <= scan < len(scans):
            raise IndexError(f"export_scan_tables: scan {scan}, entry {k} has {len(scans)} scans")
        sc = scans[scan]
        ntab = 1 if sc["ss"] else (len(sc["comps"]) if sc["ah"] == 0 else 0)
        out = []
        for slot in range(ntab):
            counts, syms, freq, n = (C.c_uint8 * 16)(), (C.c_uint8 * 256)(), (C.c_uint32 * 256)(), C.c_uint32()
            self._chk(self._lib.jsnoop_batch_export_scan_tables(self._h, int(k), int(scan), slot, counts, syms, C.byref(n), freq), "batch_export_scan_tables")
            out.append(dict(slot=slot, freq=list(freq), counts=list(counts), symbols=list(syms[:n.value])))
        return out

    def export_results(self):
        """The entries of the last export_jpeg / export_jpeg_to_torch, in the order of its list: dicts with image, result (capi.EXPORT_OK / _INEXACT /
        _UNCODABLE / _UNSUPPORTED), detail (the lowest offending block of the image, decode order; 0 where the result has none), len (0 unless OK)
        and ptr (device address of the file, 0 with len 0).  Empty after clear() / upload()."""
        out = []
        for k in range(self._lib.jsnoop_batch_export_count(self._h)):
            ptr, ln, res, det, img = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint32(), C.c_int()
            self._chk(self._lib.jsnoop_batch_export_file(self._h, k, C.byref(ptr), C.byref(ln), C.byref(res), C.byref(det), C.byref(img)), "batch_export_file")
            out.append(dict(image=img.value, result=res.value, detail=det.value, len=int(ln.value), ptr=int(ptr.value or 0)))
        return out

    def export_jpeg(self, images=None, jfif=True, huffman="annex_k", restart=0, progressive=False):
        """What the batch holds for the listed images (None = all; any order, repeats allowed) written back as baseline JPEG files, entropy-coded on
        the device by ONE jsnoop_batch_export_jpeg: a list with the file's bytes per entry, None where the image could not be exported
        (export_results() says why).  An exported file decodes to the same coefficients; where the source was a clean file, to the same pixels.
        jfif=False leaves the APP0 segment out.  Calls sync() first (a damaged file is exported as repaired); behind a DC-only fast-form decode the
        batch is decoded once more in the generic form.  huffman="optimal": every file with its own Huffman tables, built on the device from the
        image's symbol counts (export_tables(k) returns them); "annex_k" (the default): the tables of T.81 Annex K.  restart: 0 (the default) writes no
        restart markers; an int the interval in MCUs; ("rows", n) n MCU rows of each image; "source" the interval each image was decoded with (none where it
        had none).  With an interval the files carry DRI and FF D0..D7 between the intervals (jsnoop_batch_export_jpeg_rst; export_restart(k) says what entry
        k got); an image whose interval comes out above 65535 is not exported (capi.EXPORT_UNSUPPORTED).  progressive: False (the default) writes
        baseline files; True progressive (SOF2) files along the built-in scan script; a list of scans (components, ss, se, ah, al) along that script
        (jsnoop_batch_export_jpeg_prog; DESIGN.md 4.17 has the rules, a script that breaks one is refused).  Every scan then carries its own optimal
        tables whatever huffman says, restart counts in each scan's own units, and export_scans(k) / export_scan_tables(k, scan) describe the file."""
        files = []
        for k, e in enumerate(self._export(images, jfif, "export_jpeg", huffman, restart, progressive)):
            if not e["len"]:
                files.append(None); continue
            buf = (C.c_uint8 * e["len"])()
            got = self._lib.jsnoop_batch_read_export(self._h, k, buf, e["len"])
            if got != e["len"]:
                raise RuntimeError(f"batch_read_export failed: {capi.last_error()}")
            files.append(bytes(buf))
        return files

    def export_jpeg_to_torch(self, images=None, jfif=True, huffman="annex_k", restart=0, progressive=False):
        """export_jpeg, but the files stay on the device: a list with one uint8 tensor per entry (None where the image could not be exported), copied
        out of the batch's memory by jsnoop_batch_export_copy -- they outlive the next export."""
        import torch
        dev = torch.device("cuda", self.device())
        res = self._export(images, jfif, "export_jpeg_to_torch", huffman, restart, progressive)
        sizes = [-(-e["len"] // 16) * 16 for e in res]
        flat = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
        cur = torch.cuda.current_stream(dev)
        if self._stream != cur.cuda_stream:
            cur.synchronize()
        out, off = [], 0
        for k, (e, sz) in enumerate(zip(res, sizes)):
            if not e["len"]:
                out.append(None); continue
            t = flat[off:off + e["len"]]; off += sz
            if self._lib.jsnoop_batch_export_copy(self._h, k, t.data_ptr(), e["len"]) != e["len"]:
                raise RuntimeError(f"batch_export_copy failed: {capi.last_error()}")
            out.append(t)
        self.sync()
        return out

    def encode_jpeg(self, images=None, size=None, roi=None, filter="bilinear", **encode_options):
        """The decoded PIXELS of the listed images (None = all) encoded anew on the device: to_torch(layout="HWC") -- with size=(H, W), roi and filter
        resampled by one jsnoop_batch_pack_resized, the thumbnail sheet -- into scratch tensors, then JpegEncoder.encode on them with encode_options
        (quality, subsampling, qtables, huffman, restart, progressive, jfif).  A list of bytes, one file per image.  Unlike export_jpeg, which writes
        the coefficients the batch holds, this quantises again: with the preview mode and the YCC shift applied, at any size and quality.  The encoder
        object is kept with the batch (the library's current device becomes the batch's)."""
        if size is None:
            t = self.to_torch(images, layout="HWC")
        else:
            t = self.to_torch(images, layout="HWC", size=size, roi=roi, filter=filter)
        if getattr(self, "_encoder", None) is None:
            self._encoder = JpegEncoder(device=self.device())
        return self._encoder.encode(list(t), **encode_options)

    def transform(self, op, images=None, crop=None, edge="trim", grayscale=False):
        """The listed images (None = all) flipped, rotated, transposed, cropped or made grey WITHOUT a second quantisation: a JpegTransform on the batch's
        stream, run once (JpegTransform.run has the arguments; .entries() says what became of each image, .export() writes the files, .coefs(i) reads the
        arena).  The caller closes it.  Nothing is waited for: the batch must not be decoded, cleared or closed until the transform's stream has passed the run
        (any read through the object waits for it)."""
        t = JpegTransform(device=self.device(), stream=self._lib.jsnoop_batch_stream(self._h))
        try:
            t.run(self, op, images, crop, edge, grayscale)
        except Exception:
            t.close(); raise
        return t

    def export_tiff(self, i, path: str, mode: int = 0):
        self._chk(self._lib.jsnoop_batch_export_tiff(self._h, i, path.encode(), mode), "batch_export_tiff")

    def algorithmic_bytes(self): return int(self._lib.jsnoop_batch_algorithmic_bytes(self._h))
    def device_bytes(self):
        """HBM that upload() requests for the images the batch holds now (jsnoop_batch_device_bytes)."""
        return int(self._lib.jsnoop_batch_device_bytes(self._h))
    def pixels(self): return int(self._lib.jsnoop_batch_pixels(self._h))


class JpegEncoder:
    """8-bit pictures in device memory -> JPEG files, transformed, quantised and entropy-coded on the device (jsnoop_encode_* of include/jsnoop_gpu.h;
    libjpeg's integer arithmetic, value for value).  The object owns its arena, its export memory and -- unless stream is given -- its stream, on `device`
    (None: the library's current device)."""

    def __init__(self, device=None, stream=None):
        self._lib = capi.load()
        if device is not None and self._lib.jsnoop_set_device(int(device)) != 0:
            raise RuntimeError("jsnoop_set_device failed: " + capi.last_error())
        self._h = self._lib.jsnoop_encode_create(C.c_void_p(stream) if stream else None)
        if not self._h:
            raise RuntimeError("jsnoop_encode_create failed: " + capi.last_error())
        self._stream = int(stream) if stream else None
        self._device = None if device is None else int(device)

    def close(self):
        if self._h:
            self._lib.jsnoop_encode_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc < 0:
            raise RuntimeError(f"{what} failed: {capi.last_error()}")
        return rc

    def __len__(self): return self._lib.jsnoop_encode_count(self._h)

    def info(self, i):
        """Geometry of image i of the last run: the words of JpegBatch.info."""
        o = (C.c_uint * 16)()
        self._chk(self._lib.jsnoop_encode_image_info(self._h, i, o), "encode_image_info")
        keys = "dim_x dim_y img_x img_y mcu_w mcu_h mcu_xmax mcu_ymax blk_xmax blk_ymax scan_bytes flags path ncomp file_len total_blocks".split()
        return dict(zip(keys, o))

    @staticmethod
    def _describe(src, bgr, k):
        """One source -> (capi.EncodeSrc, the object that keeps its memory alive)."""
        d = capi.EncodeSrc()
        if isinstance(src, dict):
            layouts = {"interleaved": capi.ENCODE_INTERLEAVED, "planar": capi.ENCODE_PLANAR}; orders = {"rgb": capi.ENCODE_RGB, "bgr": capi.ENCODE_BGR}
            unknown = set(src) - {"ptr", "width", "height", "channels", "layout", "order", "pixel_stride", "row_pitch", "plane_pitch", "bottom_up"}
            if unknown or src.get("layout", "interleaved") not in layouts or src.get("order", "rgb") not in orders:
                raise ValueError(f"encode: source {k}: a description has ptr, width, height, channels, layout (\"interleaved\" | \"planar\"), order (\"rgb\" | \"bgr\"), "
                                 f"pixel_stride, row_pitch, plane_pitch, bottom_up; got {sorted(src)}")
            d.ptr = int(src["ptr"]); d.width = int(src["width"]); d.height = int(src["height"]); d.channels = int(src.get("channels", 3))
            d.layout = layouts[src.get("layout", "interleaved")]; d.order = orders[src.get("order", "rgb")]
            d.pixel_stride = int(src.get("pixel_stride", 0)); d.row_pitch = int(src.get("row_pitch", 0)); d.plane_pitch = int(src.get("plane_pitch", 0))
            d.bottom_up = 1 if src.get("bottom_up", False) else 0
            return d, src
        import torch
        if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8 or not src.is_cuda or src.dim() not in (2, 3):
            raise ValueError(f"encode: source {k} must be a uint8 tensor [H, W, 3], [3, H, W] or [H, W] on the device, or a description of device memory")
        st = src.stride()
        if src.numel() == 0 or min(st) < 1:
            raise ValueError(f"encode: source {k}: empty, or strides {st} below 1")
        d.ptr = src.data_ptr(); d.order = capi.ENCODE_BGR if bgr else capi.ENCODE_RGB
        if src.dim() == 2:
            d.height, d.width = src.shape; d.channels = 1; d.pixel_stride = st[1]; d.row_pitch = st[0]
        elif src.shape[2] == 3:
            if st[2] != 1:
                raise ValueError(f"encode: source {k}: the channels of an [H, W, 3] tensor must be adjacent (strides {st})")
            d.height, d.width = src.shape[:2]; d.channels = 3; d.layout = capi.ENCODE_INTERLEAVED; d.pixel_stride = st[1]; d.row_pitch = st[0]
        elif src.shape[0] == 3:
            d.height, d.width = src.shape[1:]; d.channels = 3; d.layout = capi.ENCODE_PLANAR; d.pixel_stride = st[2]; d.row_pitch = st[1]; d.plane_pitch = st[0]
        else:
            raise ValueError(f"encode: source {k} has shape {list(src.shape)}: [H, W, 3], [3, H, W] or [H, W]")
        return d, src

    def run(self, sources, quality=75, subsampling="4:2:0", qtables=None, bgr=False):
        """jsnoop_encode_run: the listed pictures into the object's arena, one launch, not waited for.  sources: uint8 device tensors [H, W, 3], [3, H, W]
        (channels R, G, B; B, G, R with bgr) or [H, W] (grey), any strides whose channel / column steps the library accepts; or dicts describing device
        memory (ptr, width, height, channels, layout, order, pixel_stride, row_pitch, plane_pitch, bottom_up -- JsnoopEncodeSrc).  quality 1..100, or
        qtables = (luma64, chroma64) in natural order, values 1..255, taken as they are."""
        sources = list(sources)
        spec = capi.encode_spec(self._lib, quality, subsampling, qtables)
        arr = (capi.EncodeSrc * max(len(sources), 1))(); keep = []
        dev = None
        for k, s in enumerate(sources):
            arr[k], alive = self._describe(s, bgr, k); keep.append(alive)
            if not isinstance(s, dict):
                dev = s.device if dev is None else dev
                if s.device != dev or (self._device is not None and s.device.index != self._device):
                    raise ValueError(f"encode: source {k} is on {s.device}, not on the encoder's device")
        if dev is not None:
            import torch
            cur = torch.cuda.current_stream(dev)                     # whatever filled the tensors was enqueued there
            if self._stream != cur.cuda_stream:
                cur.synchronize()
        self._chk(self._lib.jsnoop_encode_run(self._h, C.byref(spec), arr, len(sources)), "encode_run")
        self._keep = keep                                            # (until the next run: the launch reads them)
        return len(sources)

    def coefs(self, i):
        """Image i of the last run: (arena rows [blocks][64] int16 -- decode order, natural order inside a row, slot 0 zero --, dccum [blocks] int16)."""
        nb = self.info(i)["total_blocks"]
        a = np.empty((nb, 64), np.int16); d = np.empty(nb, np.int16)
        got = self._chk(self._lib.jsnoop_encode_read_coefs(self._h, i, a.ctypes.data_as(C.POINTER(C.c_int16)), d.ctypes.data_as(C.POINTER(C.c_int16)), nb), "encode_read_coefs")
        assert got == nb
        return a, d

    def _export(self, images, jfif, huffman, restart, progressive):
        rst = capi.export_restart(self._lib, restart)
        prog = capi.export_progressive(self._lib, progressive)
        coding = capi.export_coding(self._lib, huffman)
        spec = capi.ExportSpec()
        self._lib.jsnoop_export_spec_defaults(C.byref(spec))
        spec.jfif = 1 if jfif else 0
        idx = list(range(len(self))) if images is None else [int(i) for i in images]
        ind = (C.c_int * max(len(idx), 1))(*idx)
        self._chk(self._lib.jsnoop_encode_export(self._h, C.byref(spec), C.byref(coding), C.byref(rst), C.byref(prog), ind, len(idx)), "encode_export")
        return self.export_results()

    def export_results(self):
        """The entries of the last export, as JpegBatch.export_results returns them."""
        out = []
        for k in range(self._lib.jsnoop_encode_export_count(self._h)):
            ptr, ln, res, det, img = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint32(), C.c_int()
            self._chk(self._lib.jsnoop_encode_export_file(self._h, k, C.byref(ptr), C.byref(ln), C.byref(res), C.byref(det), C.byref(img)), "encode_export_file")
            out.append(dict(image=img.value, result=res.value, detail=det.value, len=int(ln.value), ptr=int(ptr.value or 0)))
        return out

    def export_scans(self, k):
        """Entry k of the last progressive export: one dict per scan, as JpegBatch.export_scans returns them."""
        out = []
        for i in range(self._lib.jsnoop_encode_export_scan_count(self._h, int(k))):
            sc, ri, n, sos, nb = capi.ExportScan(), C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
            self._chk(self._lib.jsnoop_encode_export_scan_info(self._h, int(k), i, C.byref(sc), C.byref(ri), C.byref(n), C.byref(sos), C.byref(nb)), "encode_export_scan_info")
            out.append(dict(comps=[c for c in range(8) if sc.comps >> c & 1], ss=sc.ss, se=sc.se, ah=sc.ah, al=sc.al, ri=int(ri.value), intervals=int(n.value),
                            sos_offset=int(sos.value), data_bytes=int(nb.value)))
        return out

    def export(self, images=None, jfif=True, huffman="annex_k", restart=0, progressive=False):
        """The images of the last run (None = all; any order, repeats allowed) as files: a list of bytes, None where an image could not be written
        (export_results() says why).  huffman, restart and progressive are JpegBatch.export_jpeg's."""
        files = []
        for k, e in enumerate(self._export(images, jfif, huffman, restart, progressive)):
            if not e["len"]:
                files.append(None); continue
            buf = (C.c_uint8 * e["len"])()
            if self._lib.jsnoop_encode_read_export(self._h, k, buf, e["len"]) != e["len"]:
                raise RuntimeError(f"encode_read_export failed: {capi.last_error()}")
            files.append(bytes(buf))
        return files

    def encode(self, sources, quality=75, subsampling="4:2:0", qtables=None, huffman="annex_k", restart=0, progressive=False, bgr=False, jfif=True):
        """run + export: one file (bytes) per source.  No pixel and no coefficient crosses PCIe; the files do."""
        self.run(sources, quality, subsampling, qtables, bgr)
        return self.export(None, jfif, huffman, restart, progressive)

    def encode_to_torch(self, sources, quality=75, subsampling="4:2:0", qtables=None, huffman="annex_k", restart=0, progressive=False, bgr=False, jfif=True):
        """encode, but the files stay on the device: a list with one uint8 tensor per source (None where it could not be written), copied out of the
        object's memory by jsnoop_encode_export_copy -- they outlive the next export."""
        import torch
        self.run(sources, quality, subsampling, qtables, bgr)
        res = self._export(None, jfif, huffman, restart, progressive)
        tens = [s for s in sources if isinstance(s, torch.Tensor)]
        dev = tens[0].device if tens else torch.device("cuda", self._device if self._device is not None else torch.cuda.current_device())
        sizes = [-(-e["len"] // 16) * 16 for e in res]
        flat = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
        cur = torch.cuda.current_stream(dev)
        if self._stream != cur.cuda_stream:
            cur.synchronize()
        out, off = [], 0
        for k, (e, sz) in enumerate(zip(res, sizes)):
            if not e["len"]:
                out.append(None); continue
            t = flat[off:off + e["len"]]; off += sz
            if self._lib.jsnoop_encode_export_copy(self._h, k, t.data_ptr(), e["len"]) != e["len"]:
                raise RuntimeError(f"encode_export_copy failed: {capi.last_error()}")
            out.append(t)
        if out and any(t is not None for t in out):                   # wait for the copies: one byte of the last entry read back is behind all of them on the stream
            last = max(k for k, t in enumerate(out) if t is not None)
            one = (C.c_uint8 * res[last]["len"])()
            self._lib.jsnoop_encode_read_export(self._h, last, one, res[last]["len"])
        return out


class JpegTransform:
    """jpegtran's lossless transforms of a decoded batch on the device: flip, rotate, transpose, transverse, crop and grayscale rearrange the DCT blocks
    the batch holds into an arena of this object's, without a second quantisation, and the export writes that arena as files (jsnoop_transform_* of
    include/jsnoop_gpu.h).  The object owns its arena, its export memory and -- unless stream is given -- its stream, on `device` (None:
    the library's current device).  JpegBatch.transform makes one on the batch's stream and runs it."""

    def __init__(self, device=None, stream=None):
        self._lib = capi.load()
        if device is not None and self._lib.jsnoop_set_device(int(device)) != 0:
            raise RuntimeError("jsnoop_set_device failed: " + capi.last_error())
        self._h = self._lib.jsnoop_transform_create(C.c_void_p(stream) if stream else None)
        if not self._h:
            raise RuntimeError("jsnoop_transform_create failed: " + capi.last_error())
        self._stream = int(stream) if stream else None
        self._device = None if device is None else int(device)

    def close(self):
        if self._h:
            self._lib.jsnoop_transform_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc < 0:
            raise RuntimeError(f"{what} failed: {capi.last_error()}")
        return rc

    def __len__(self): return self._lib.jsnoop_transform_count(self._h)

    def run(self, batch, op="none", images=None, crop=None, edge="trim", grayscale=False):
        """jsnoop_transform_run: the listed images of `batch` (a decoded JpegBatch; None = all, any order, repeats allowed) into the object's arena, one
        launch, not waited for.  op: "none" | "flip_h" | "flip_v" | "transpose" | "transverse" | "rot90" (clockwise) | "rot180" | "rot270" or a JXFORM
        code (capi.XFORM_EXIF maps an EXIF orientation to the op that sets the picture upright); crop = (x, y, w, h) by jpegtran's rule; edge "trim"
        cuts a reversed dimension down to whole MCUs, "perfect" refuses such an entry (IMPERFECT); grayscale keeps component 0 alone.  Returns
        entries().  The batch's arena must stay as it is until the object's stream has passed the run; call batch.sync() first where damaged files
        should be transformed as repaired."""
        spec = capi.transform_spec(self._lib, op, edge, grayscale, crop)
        idx = list(range(len(batch))) if images is None else [int(i) for i in images]
        ind = (C.c_int * max(len(idx), 1))(*idx)
        self._chk(self._lib.jsnoop_transform_run(self._h, batch._h, C.byref(spec), ind, len(idx)), "transform_run")
        return self.entries()

    def entries(self):
        """The entries of the last run: dict(result, image) each -- result capi.XFORM_OK / _IMPERFECT / _EMPTY / _UNSUPPORTED, image the entry's index in
        this object or -1 where it has none."""
        out = []
        for k in range(self._lib.jsnoop_transform_entry_count(self._h)):
            res, img = C.c_int(), C.c_int()
            self._chk(self._lib.jsnoop_transform_entry(self._h, k, C.byref(res), C.byref(img)), "transform_entry")
            out.append(dict(result=res.value, image=img.value))
        return out

    def info(self, i):
        """Geometry of image i of the last run: the words of JpegBatch.info."""
        o = (C.c_uint * 16)()
        self._chk(self._lib.jsnoop_transform_image_info(self._h, i, o), "transform_image_info")
        keys = "dim_x dim_y img_x img_y mcu_w mcu_h mcu_xmax mcu_ymax blk_xmax blk_ymax scan_bytes flags path ncomp file_len total_blocks".split()
        return dict(zip(keys, o))

    def dqt(self, i, comp):
        """The 64 multipliers of component comp of image i, natural order (transposed where the op transposes)."""
        q = (C.c_uint16 * 64)()
        self._chk(self._lib.jsnoop_transform_image_dqt(self._h, i, comp, q), "transform_image_dqt")
        return list(q)

    def coefs(self, i):
        """Image i of the last run: (arena rows [blocks][64] int16 -- decode order of the new geometry, natural order inside a row --, dccum [blocks] int16)."""
        nb = self.info(i)["total_blocks"]
        a = np.empty((nb, 64), np.int16); d = np.empty(nb, np.int16)
        got = self._chk(self._lib.jsnoop_transform_read_coefs(self._h, i, a.ctypes.data_as(C.POINTER(C.c_int16)), d.ctypes.data_as(C.POINTER(C.c_int16)), nb), "transform_read_coefs")
        assert got == nb
        return a, d

    def _export(self, images, jfif, huffman, restart, progressive):
        rst = capi.export_restart(self._lib, restart)
        prog = capi.export_progressive(self._lib, progressive)
        coding = capi.export_coding(self._lib, huffman)
        spec = capi.ExportSpec()
        self._lib.jsnoop_export_spec_defaults(C.byref(spec))
        spec.jfif = 1 if jfif else 0
        idx = list(range(len(self))) if images is None else [int(i) for i in images]
        ind = (C.c_int * max(len(idx), 1))(*idx)
        self._chk(self._lib.jsnoop_transform_export(self._h, C.byref(spec), C.byref(coding), C.byref(rst), C.byref(prog), ind, len(idx)), "transform_export")
        return self.export_results()

    def export_results(self):
        """The entries of the last export, as JpegBatch.export_results returns them."""
        out = []
        for k in range(self._lib.jsnoop_transform_export_count(self._h)):
            ptr, ln, res, det, img = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_uint32(), C.c_int()
            self._chk(self._lib.jsnoop_transform_export_file(self._h, k, C.byref(ptr), C.byref(ln), C.byref(res), C.byref(det), C.byref(img)), "transform_export_file")
            out.append(dict(image=img.value, result=res.value, detail=det.value, len=int(ln.value), ptr=int(ptr.value or 0)))
        return out

    def export_scans(self, k):
        """Entry k of the last progressive export: one dict per scan, as JpegBatch.export_scans returns them."""
        out = []
        for i in range(self._lib.jsnoop_transform_export_scan_count(self._h, int(k))):
            sc, ri, n, sos, nb = capi.ExportScan(), C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
            self._chk(self._lib.jsnoop_transform_export_scan_info(self._h, int(k), i, C.byref(sc), C.byref(ri), C.byref(n), C.byref(sos), C.byref(nb)), "transform_export_scan_info")
            out.append(dict(comps=[c for c in range(8) if sc.comps >> c & 1], ss=sc.ss, se=sc.se, ah=sc.ah, al=sc.al, ri=int(ri.value), intervals=int(n.value),
                            sos_offset=int(sos.value), data_bytes=int(nb.value)))
        return out

    def export(self, images=None, jfif=True, huffman="annex_k", restart=0, progressive=False):
        """The images of the last run (None = all; any order, repeats allowed) as files: a list of bytes, None where an image could not be written
        (export_results() says why).  huffman, restart and progressive are JpegBatch.export_jpeg's; "source" finds no restart interval."""
        files = []
        for k, e in enumerate(self._export(images, jfif, huffman, restart, progressive)):
            if not e["len"]:
                files.append(None); continue
            buf = (C.c_uint8 * e["len"])()
            if self._lib.jsnoop_transform_read_export(self._h, k, buf, e["len"]) != e["len"]:
                raise RuntimeError(f"transform_read_export failed: {capi.last_error()}")
            files.append(bytes(buf))
        return files

    def export_to_torch(self, images=None, jfif=True, huffman="annex_k", restart=0, progressive=False, device=None):
        """export, but the files stay on the device: a list with one uint8 tensor per entry (None where it could not be written), copied out of the
        object's memory by jsnoop_transform_export_copy -- they outlive the next export."""
        import torch
        res = self._export(images, jfif, huffman, restart, progressive)
        dev = torch.device("cuda", device if device is not None else (self._device if self._device is not None else torch.cuda.current_device()))
        sizes = [-(-e["len"] // 16) * 16 for e in res]
        flat = torch.empty(sum(sizes), dtype=torch.uint8, device=dev)
        cur = torch.cuda.current_stream(dev)
        if self._stream != cur.cuda_stream:
            cur.synchronize()
        out, off = [], 0
        for k, (e, sz) in enumerate(zip(res, sizes)):
            if not e["len"]:
                out.append(None); continue
            t = flat[off:off + e["len"]]; off += sz
            if self._lib.jsnoop_transform_export_copy(self._h, k, t.data_ptr(), e["len"]) != e["len"]:
                raise RuntimeError(f"transform_export_copy failed: {capi.last_error()}")
            out.append(t)
        if out and any(t is not None for t in out):                   # wait for the copies: the last entry read back is behind all of them on the stream
            last = max(k for k, t in enumerate(out) if t is not None)
            one = (C.c_uint8 * res[last]["len"])()
            self._lib.jsnoop_transform_read_export(self._h, last, one, res[last]["len"])
        return out


class JpegPipeline:
    """Overlapped staging (the CwindowBuf replacement at batch scale): `slots` JpegBatch slots cycled by jsnoop_pipeline_run --
    H2D of the next batch and, on request, D2H of the previous one overlap the decode of the current one."""

    def __init__(self, slots=2):
        self._lib = capi.load()
        self._h = self._lib.jsnoop_pipeline_create(slots)
        if not self._h:
            raise RuntimeError("jsnoop_pipeline_create failed: " + capi.last_error())
        self.slots = []
        for i in range(slots):
            b = JpegBatch.__new__(JpegBatch)
            b._lib, b._h, b.want_planes, b._borrowed, b._stream = self._lib, self._lib.jsnoop_pipeline_slot(self._h, i), False, True, None
            self.slots.append(b)

    def run(self, batches, d2h=False):
        out = (C.c_double * 6)()
        if self._lib.jsnoop_pipeline_run(self._h, batches, int(d2h), out) < 0:
            raise RuntimeError("jsnoop_pipeline_run failed: " + capi.last_error())
        return {"ms_per_batch": out[0], "h2d_ms": out[1], "decode_ms": out[2], "d2h_ms": out[3], "compressed_bytes": int(out[4]), "dib_bytes": int(out[5])}

    def close(self):
        if self._h:
            for b in self.slots:
                b._h = None                      # owned by the pipeline
            self._lib.jsnoop_pipeline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pack_spec(lib, layout, is_f32, bgr, scale, bias) -> "capi.PackSpec":
    if layout not in ("CHW", "HWC"):
        raise ValueError("layout must be \"CHW\" or \"HWC\"")
    spec = capi.PackSpec()
    lib.jsnoop_pack_spec_defaults(C.byref(spec))
    spec.layout = capi.PACK_CHW if layout == "CHW" else capi.PACK_HWC
    spec.dtype = capi.PACK_F32 if is_f32 else capi.PACK_U8
    spec.bgr = int(bool(bgr))
    for name, val in (("scale", scale), ("bias", bias)):
        if val is None:
            continue
        vals = [float(val)] * 3 if np.isscalar(val) else [float(v) for v in val]
        if len(vals) != 3:
            raise ValueError(f"{name} must be a number or three numbers")
        for c in range(3):
            getattr(spec, name)[c] = vals[c]
    return spec


_INFO_KEYS = "dim_x dim_y img_x img_y mcu_w mcu_h mcu_xmax mcu_ymax blk_xmax blk_ymax scan_bytes flags path ncomp file_len total_blocks".split()


def stats_fields(row):
    """Named views of one JSNOOP_STATS_WORDS row (numpy array or torch tensor, any integer dtype): "records" [12, 3] = (min, max, sum) of
    PreclipY/Cb/Cr, ClipY/Cb/Cr, ClipR/G/B, PreclipR/G/B (signed: view an unsigned row as int32 first), "count", "clip" [13] (Y<0, Y>255,
    Cb<0, Cb>255, Cr<0, Cr>255, R<0, R>255, G<0, G>255, B<0, B>255, White), "r" / "g" / "b" [128] and "y" [2048]."""
    if row.shape[-1] != capi.STATS_WORDS or len(row.shape) != 1:
        raise ValueError("stats_fields: a row of %d words" % capi.STATS_WORDS)
    return {"records": row[0:36].reshape(12, 3), "count": row[36], "clip": row[37:50], "r": row[50:178], "g": row[178:306], "b": row[306:434], "y": row[434:2482]}


def coef_hist_fields(row, range):
    """Views (not copies) of one row of coef_hist_to_torch / coef_hist_all (numpy array or torch tensor): (hist [64, 2 * range + 1], min [64], max [64]).
    A numpy row of an unsigned dtype gives its minima and maxima viewed as int32."""
    nb = 2 * int(range) + 1
    if len(row.shape) != 1 or row.shape[0] != 64 * nb + 128:
        raise ValueError("coef_hist_fields: a row of %d words for range %d" % (64 * nb + 128, int(range)))
    mn, mx = row[64 * nb:64 * nb + 64], row[64 * nb + 64:]
    if isinstance(row, np.ndarray) and row.dtype == np.uint32:
        mn, mx = mn.view(np.int32), mx.view(np.int32)
    return row[:64 * nb].reshape(64, nb), mn, mx


class JobFileResult:
    """One file of a JpegJob: status ("ok" / "refused" / "unreadable" / "pending"), kind ("baseline" / "progressive" / None), where it was
    decoded, info (as JpegBatch.info), dib_hash, message.  `batch` / `image` address the file in a borrowed JpegBatch: inside the callback,
    or until JpegJob.clear() / close() with keep_resident; None otherwise."""
    STATUS = {capi.JOB_PENDING: "pending", capi.JOB_OK: "ok", capi.JOB_REFUSED: "refused", capi.JOB_UNREADABLE: "unreadable"}
    KIND = {0: None, 1: "baseline", 2: "progressive"}

    def __init__(self, lib, f: "capi.JobFile", want_planes: bool):
        self.index, self.status, self.kind = f.index, self.STATUS[f.status], self.KIND[f.kind]
        self.shard, self.device, self.round, self.image = f.shard, f.device, f.round, f.image
        self.info = dict(zip(_INFO_KEYS, f.info16))
        self.dib_hash = int(f.dib_hash)
        self.message = (f.message or b"").decode(errors="replace")
        self.batch = None
        if f.batch:
            b = JpegBatch.__new__(JpegBatch)
            b._lib, b._h, b.want_planes, b._borrowed = lib, f.batch, want_planes, True
            b._stream = None
            self.batch = b

    def to_torch(self, **kw):
        """JpegBatch.to_torch for this file alone: one tensor ([3, dim_y, dim_x] / [dim_y, dim_x, 3]; with stack / pad_to / size / a tensor out,
        the [1, ...] tensor); pixels="libjpeg" and reduce= pass through like every keyword.  Valid inside the callback, or until JpegJob.clear() / close() with keep_resident."""
        if self.batch is None:
            raise RuntimeError("to_torch: this result holds no resident image (status %s)" % self.status)
        r = self.batch.to_torch(images=[self.image], **kw)
        return r[0] if isinstance(r, list) else r

    def coefs_to_torch(self, **kw):
        """JpegBatch.coefs_to_torch for this file alone: a list with one tensor per component.  Valid inside the callback, or until
        JpegJob.clear() / close() with keep_resident."""
        if self.batch is None:
            raise RuntimeError("coefs_to_torch: this result holds no resident image (status %s)" % self.status)
        out = kw.pop("out", None)
        r = self.batch.coefs_to_torch(images=[self.image], out=None if out is None else [out], **kw)
        return r[0]

    def stats_to_torch(self, **kw):
        """JpegBatch.stats_to_torch for this file alone: the [1, 2482] tensor (with totals=True also the [1, 6] one).  The job needs want_planes.
        Valid inside the callback, or until JpegJob.clear() / close() with keep_resident."""
        if self.batch is None:
            raise RuntimeError("stats_to_torch: this result holds no resident image (status %s)" % self.status)
        return self.batch.stats_to_torch(images=[self.image], **kw)

    def planes_to_torch(self, **kw):
        """JpegBatch.planes_to_torch for this file alone: a list with one [h, w] tensor per component (with stack=True the [1, C, H, W] tensor).  The
        job needs want_planes.  Valid inside the callback, or until JpegJob.clear() / close() with keep_resident."""
        if self.batch is None:
            raise RuntimeError("planes_to_torch: this result holds no resident image (status %s)" % self.status)
        out = kw.pop("out", None)
        if kw.get("stack"):
            return self.batch.planes_to_torch(images=[self.image], out=out, **kw)
        r = self.batch.planes_to_torch(images=[self.image], out=None if out is None else [out], **kw)
        return r[0]

    def coef_hist_to_torch(self, **kw):
        """JpegBatch.coef_hist_to_torch for this file alone: (pairs, rows), one row per component (comps= picks some).  Valid inside the callback, or
        until JpegJob.clear() / close() with keep_resident."""
        if self.batch is None:
            raise RuntimeError("coef_hist_to_torch: this result holds no resident image (status %s)" % self.status)
        comps = kw.pop("comps", None)
        if comps is not None:
            comps = [int(c) for c in comps]
            return self.batch.coef_hist_to_torch(images=[self.image] * len(comps), comps=comps, **kw)
        return self.batch.coef_hist_to_torch(images=[self.image], **kw)

    def export_jpeg(self, **kw):
        """JpegBatch.export_jpeg for this file alone: the file's bytes, or None where the image could not be exported (batch.export_results()[0] says
        why).  Valid inside the callback, or until JpegJob.clear() / close() with keep_resident."""
        if self.batch is None:
            raise RuntimeError("export_jpeg: this result holds no resident image (status %s)" % self.status)
        return self.batch.export_jpeg(images=[self.image], **kw)[0]

    def __repr__(self):
        return "JobFileResult(index=%d, status=%s, kind=%s, shard=%d, round=%d)" % (self.index, self.status, self.kind, self.shard, self.round)


class JpegJob:
    """One call decodes a mixed file list (baseline and progressive, good and bad) over all devices: jsnoop_job_* of include/jsnoop_gpu.h,
    the whole-node form of CJPEGsnoopCore::DoBatchFileProcess (source/JPEGsnoopCore.cpp:765-845).

    devices: the device of every shard (a device may appear more than once: logical shards on one GPU); None = one shard per visible device.
    Every file gets a result; a file the front end refuses or a path that cannot be read never fails the job."""

    def __init__(self, devices=None, decode_ac=True, want_planes=False, enable_log=False, max_images_per_round=0, max_round_bytes=0,
                 partition="lpt", keep_resident=False, tuning=None):
        self._lib = capi.load()
        if devices is None:
            self._h = self._lib.jsnoop_job_create(None, 0)
        else:
            devs = (C.c_int * len(devices))(*devices)
            self._h = self._lib.jsnoop_job_create(devs, len(devices))
        if not self._h:
            raise RuntimeError("jsnoop_job_create failed: " + capi.last_error())
        o = capi.JobOptions()
        self._lib.jsnoop_job_options_defaults(C.byref(o))
        o.decode_ac, o.want_planes, o.enable_log = int(decode_ac), int(want_planes), int(enable_log)
        o.max_images_per_round, o.max_round_bytes = int(max_images_per_round), int(max_round_bytes)
        o.partition, o.keep_resident = {"lpt": 0, "contiguous": 1}[partition], int(keep_resident)
        self._chk(self._lib.jsnoop_job_set_options(self._h, C.byref(o)), "job_set_options")
        if tuning:
            t = capi.Tuning(); self._lib.jsnoop_tuning_defaults(C.byref(t))
            for k, v in tuning.items():
                if not hasattr(t, k): raise AttributeError("JsnoopTuning has no field " + k)
                setattr(t, k, v)
            self._chk(self._lib.jsnoop_job_set_tuning(self._h, C.byref(t)), "job_set_tuning")
        self.want_planes = bool(want_planes)

    def _chk(self, rc, what):
        if rc < 0:
            raise RuntimeError(f"{what} failed: {capi.last_error()}")
        return rc

    def add(self, data: bytes) -> int:
        """Adds one file image (bytes copied; the content is judged when the job runs).  Returns the file index."""
        buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
        return self._chk(self._lib.jsnoop_job_add_file(self._h, C.cast(buf, C.c_void_p), len(data)), "job_add_file")

    def add_carved(self, data, frames, include_no_eoi=False) -> list:
        """Adds data[start:end] of every frame of a carve's table (Carve.frames / carve_host) with status OK -- and NO_EOI if asked -- as a file of its own
        (jsnoop_job_add_carved).  `data` is host bytes or a uint8 numpy array.  Returns the file indices, in table order."""
        buf = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
        first = C.c_int(-1)
        n = self._chk(self._lib.jsnoop_job_add_carved(self._h, buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, _carve_table(frames), len(frames),
                                                      int(bool(include_no_eoi)), C.byref(first)), "job_add_carved")
        return list(builtins.range(first.value, first.value + n))

    def add_path(self, path) -> int:
        """Adds a file by path: read by the shard that owns it, in the round that decodes it."""
        import os
        return self._chk(self._lib.jsnoop_job_add_path(self._h, os.fsencode(path)), "job_add_path")

    def __len__(self): return self._lib.jsnoop_job_count(self._h)
    def clear(self): self._lib.jsnoop_job_clear(self._h)

    def run(self, on_file=None) -> dict:
        """Decodes every file.  on_file(result) is called on this thread, once per file; a true return value cancels the job.
        Returns the job's statistics (JsnoopJobStats as a dict, plus "cancelled")."""
        err = []

        def thunk(_user, fp):
            try:
                return 1 if on_file(JobFileResult(self._lib, fp.contents, self.want_planes)) else 0
            except BaseException as e:                   # (no exception crosses the C ABI: cancel, re-raise behind the run)
                err.append(e)
                return 1
        cb = capi.JOB_FILE_FN(thunk) if on_file is not None else C.cast(None, capi.JOB_FILE_FN)
        st = capi.JobStats(); st.struct_size = C.sizeof(capi.JobStats)
        rc = self._lib.jsnoop_job_run(self._h, cb, None, C.byref(st))
        if err:
            raise err[0]
        self._chk(rc, "job_run")
        out = {k: getattr(st, k) for k in ("files", "ok", "refused", "unreadable", "flagged", "rounds", "nshards", "pixels", "dib_hash_sum",
                                           "max_round_device_bytes", "wall_ms")}
        out["shard_ms"] = list(st.shard_ms)[: st.nshards]
        out["cancelled"] = rc == 1
        return out

    def result(self, i) -> JobFileResult:
        f = capi.JobFile(); f.struct_size = C.sizeof(capi.JobFile)
        self._chk(self._lib.jsnoop_job_file_result(self._h, i, C.byref(f)), "job_file_result")
        return JobFileResult(self._lib, f, self.want_planes)

    def results(self) -> list:
        return [self.result(i) for i in range(len(self))]

    def close(self):
        if self._h:
            self._lib.jsnoop_job_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CARVE_FIELDS = tuple(name for name, _ in capi.CarveFrame._fields_[1:])


def _carve_spec(lib, max_markers, max_scratch_bytes) -> "capi.CarveSpec":
    s = capi.CarveSpec()
    lib.jsnoop_carve_spec_defaults(C.byref(s))
    if max_markers is not None:
        s.max_markers = int(max_markers)
    s.max_scratch_bytes = int(max_scratch_bytes)
    return s


def _carve_dicts(arr, n) -> list:
    return [{k: getattr(arr[i], k) for k in CARVE_FIELDS} for i in builtins.range(n)]


def _carve_table(frames):
    """A list of frame dicts (Carve.frames / carve_host) as a JsnoopCarveFrame array."""
    arr = (capi.CarveFrame * max(1, len(frames)))()
    for a, f in zip(arr, frames):
        a.struct_size = C.sizeof(capi.CarveFrame)
        for k in CARVE_FIELDS:
            setattr(a, k, f[k])
    return arr


def carve_host(data, max_markers=None) -> list:
    """The frame table of `data` (bytes or a uint8 numpy array) computed on the host alone (jsnoop_carve_host): no device needed."""
    lib = capi.load(require_device=False)
    buf = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8)
    spec = _carve_spec(lib, max_markers, 0)
    ptr = buf.ctypes.data_as(C.c_void_p) if buf.size else None
    n = lib.jsnoop_carve_host(C.byref(spec), ptr, buf.size, None, 0)
    if n < 0:
        raise RuntimeError("carve_host failed: " + capi.last_error())
    arr = (capi.CarveFrame * max(1, n))()
    if lib.jsnoop_carve_host(C.byref(spec), ptr, buf.size, arr, n) != n:
        raise RuntimeError("carve_host failed: " + capi.last_error())
    return _carve_dicts(arr, n)


class Carve:
    """Every embedded JPEG of a byte blob, found and walked on the device: jsnoop_carve_* of include/jsnoop_gpu.h, the reference's "extract all"
    (DoExtractEmbeddedJPEG, source/JPEGsnoopCore.cpp:906-1091) for a whole blob at once.  run() takes bytes or a numpy array (uploaded through the
    library's page-locked staging) or a uint8 torch tensor on the carve's device (read in place, any alignment)."""

    def __init__(self, device=0, max_markers=None, max_scratch_bytes=0):
        self._lib = capi.load()
        self._h = self._lib.jsnoop_carve_create(int(device))
        if not self._h:
            raise RuntimeError("jsnoop_carve_create failed: " + capi.last_error())
        self.device = int(device)
        self._spec = _carve_spec(self._lib, max_markers, max_scratch_bytes)

    def close(self):
        if self._h:
            self._lib.jsnoop_carve_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_spec(self, max_markers=None, max_scratch_bytes=0):
        """The marker cap of a walk (None: the library's 4096) and the scratch budget (0: half of the device's free memory) of the runs that follow."""
        self._spec = _carve_spec(self._lib, max_markers, max_scratch_bytes)

    def run(self, data) -> int:
        """Carves `data`; returns the number of frames (one per FF D8 FF).  A refused call (scratch over budget, ...) raises and leaves the last table."""
        if isinstance(data, (bytes, bytearray, memoryview, np.ndarray)):
            buf = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data, dtype=np.uint8)
            rc = self._lib.jsnoop_carve_run(self._h, C.byref(self._spec), buf.ctypes.data_as(C.c_void_p) if buf.size else None, buf.size, 0)
        else:
            import torch
            if not (isinstance(data, torch.Tensor) and data.dtype == torch.uint8 and data.is_cuda and data.device.index == self.device and data.is_contiguous()):
                raise TypeError("Carve.run takes bytes, a numpy array or a contiguous uint8 torch tensor on device %d" % self.device)
            torch.cuda.current_stream(data.device).synchronize()      # the carve runs on its own stream: the tensor's bytes must be there
            rc = self._lib.jsnoop_carve_run(self._h, C.byref(self._spec), data.data_ptr() if data.numel() else None, data.numel(), 1)
        if rc < 0:
            raise RuntimeError("carve_run failed: " + capi.last_error())
        return len(self)

    def __len__(self): return int(self._lib.jsnoop_carve_count(self._h))

    def totals(self):
        """(terminators, candidates) of the last run."""
        t, c = C.c_uint64(), C.c_uint64()
        self._lib.jsnoop_carve_totals(self._h, C.byref(t), C.byref(c))
        return t.value, c.value

    def frames(self) -> list:
        """The frame table of the last run: one dict per candidate, ascending start (fields: JsnoopCarveFrame's)."""
        n = len(self)
        arr = (capi.CarveFrame * max(1, n))()
        if self._lib.jsnoop_carve_frames(self._h, arr, n) != n:
            raise RuntimeError("carve_frames failed: " + capi.last_error())
        return _carve_dicts(arr, n)

    def _dev_words(self, what, words):
        import torch
        out = torch.empty(words, dtype=torch.int32, device=torch.device("cuda", self.device))
        if self._lib.jsnoop_carve_copy(self._h, what, out.data_ptr() if words else None, words * 4) != words * 4:
            raise RuntimeError("carve_copy failed: " + capi.last_error())
        return out

    def frames_to_torch(self):
        """The records as they lie in device memory: an int32 tensor [frames, CARVE_REC_WORDS] (a copy; words are unsigned, see include/jsnoop_gpu.h)."""
        n = len(self)
        return self._dev_words(0, n * capi.CARVE_REC_WORDS).view(n, capi.CARVE_REC_WORDS)

    def lists_to_torch(self):
        """(terminators, candidates): the two ascending position lists of the last run, int32 tensors holding unsigned positions (copies)."""
        nt, nc = self.totals()
        return self._dev_words(1, nt), self._dev_words(2, nc)


def dib_checksum_numpy(dib: np.ndarray) -> int:
    """The position-keyed checksum of k_dib_checksum, recomputed on the host from a DIB array
    (used by tests to compare a device DIB against the oracle's without a D2H copy)."""
    px = np.ascontiguousarray(dib).view(np.uint32).reshape(-1).astype(np.uint64)
    z = (np.arange(px.size, dtype=np.uint64) << np.uint64(32)) | px
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return int(z.sum(dtype=np.uint64))
