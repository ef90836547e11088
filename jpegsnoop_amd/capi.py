"""ctypes binding of libjsnoop_gpu.so (the C ABI declared in include/jsnoop_gpu.h).

Plumbing only: the product is the shared library.  Loading fails loudly when the
library has not been built or no HIP device is visible -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libjsnoop_gpu.so")

NUM_STAGES = 8
LOG_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p)

class Tuning(C.Structure):
    """JsnoopTuning of include/jsnoop_gpu.h: how the library decodes (0 = automatic everywhere), never what it produces."""
    _fields_ = [("struct_size", C.c_uint32), ("sub_wl", C.c_int32), ("cand_rounds", C.c_int32), ("cand_max_walks", C.c_uint64),
                ("sync_launches", C.c_int32), ("write_lanes", C.c_int32), ("split", C.c_int32), ("mcus_per_wave", C.c_int32),
                ("pg_lanes", C.c_int32), ("cross_checks", C.c_uint32), ("debug", C.c_uint32)]


JOB_MAX_SHARDS = 16
JOB_PENDING, JOB_OK, JOB_REFUSED, JOB_UNREADABLE = -1, 0, 1, 2


class JobOptions(C.Structure):
    """JsnoopJobOptions of include/jsnoop_gpu.h."""
    _fields_ = [("struct_size", C.c_uint32), ("decode_ac", C.c_int32), ("want_planes", C.c_int32), ("enable_log", C.c_int32),
                ("max_images_per_round", C.c_int32), ("max_round_bytes", C.c_uint64), ("partition", C.c_int32), ("keep_resident", C.c_int32)]


class JobFile(C.Structure):
    """JsnoopJobFile of include/jsnoop_gpu.h: the result of one file of a job."""
    _fields_ = [("struct_size", C.c_uint32), ("index", C.c_int32), ("status", C.c_int32), ("kind", C.c_int32), ("shard", C.c_int32),
                ("device", C.c_int32), ("round", C.c_int32), ("image", C.c_int32), ("batch", C.c_void_p), ("info16", C.c_uint32 * 16),
                ("dib_hash", C.c_uint64), ("message", C.c_char_p)]


class JobStats(C.Structure):
    """JsnoopJobStats of include/jsnoop_gpu.h."""
    _fields_ = [("struct_size", C.c_uint32), ("files", C.c_int32), ("ok", C.c_int32), ("refused", C.c_int32), ("unreadable", C.c_int32),
                ("flagged", C.c_int32), ("rounds", C.c_int32), ("nshards", C.c_int32), ("pixels", C.c_uint64), ("dib_hash_sum", C.c_uint64),
                ("max_round_device_bytes", C.c_uint64), ("wall_ms", C.c_double), ("shard_ms", C.c_double * JOB_MAX_SHARDS)]


PACK_HWC, PACK_CHW = 0, 1
PACK_U8, PACK_F32 = 0, 1


class PackSpec(C.Structure):
    """JsnoopPackSpec of include/jsnoop_gpu.h: what jsnoop_batch_pack writes (layout, element type, channel order, float scale / bias)."""
    _fields_ = [("struct_size", C.c_uint32), ("layout", C.c_int32), ("dtype", C.c_int32), ("bgr", C.c_int32),
                ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class PackDst(C.Structure):
    """JsnoopPackDst of include/jsnoop_gpu.h: one destination in device memory; pitches in bytes, 0 = dense."""
    _fields_ = [("ptr", C.c_void_p), ("row_pitch", C.c_uint64), ("plane_pitch", C.c_uint64)]


RESIZE_NEAREST, RESIZE_BILINEAR, RESIZE_AREA = 0, 1, 2


class ResizeDst(C.Structure):
    """JsnoopResizeDst of include/jsnoop_gpu.h: one destination of jsnoop_batch_pack_resized -- pointer and pitches as PackDst for an out_w x out_h
    image, the output size (1 .. 32767 each) and the source rectangle in the plain pack's coordinates (roi_w == roi_h == 0: the whole image)."""
    _fields_ = [("ptr", C.c_void_p), ("row_pitch", C.c_uint64), ("plane_pitch", C.c_uint64), ("out_w", C.c_uint32), ("out_h", C.c_uint32),
                ("roi_x", C.c_uint32), ("roi_y", C.c_uint32), ("roi_w", C.c_uint32), ("roi_h", C.c_uint32)]


COEF_BLOCKS, COEF_FREQ = 0, 1
COEF_I16, COEF_F32 = 0, 1
COEF_NATURAL, COEF_ZIGZAG = 0, 1
STATS_WORDS = 2482      # JSNOOP_STATS_WORDS of include/jsnoop_gpu.h: words of one row of colour statistics
STATS_UNIT = 512        # JS_STATS_UNIT of csrc/jsnoop_types.h: pixels of one picture row a wave takes at a time (k_stats_batch)
COEF_TILE = 64          # JS_COEF_TILE of csrc/jsnoop_types.h: blocks of one block row a wave moves at a time (the frequency-major form's transposition tile)


COEF_HIST_UNIT = 64     # JS_COEF_HIST_UNIT of csrc/jsnoop_types.h: blocks of one component, in arena order, a wave takes at a time (k_coef_hist)
COEF_HIST_WAVES = 8     # JS_COEF_HIST_WAVES: waves of a workgroup, which deal the units of one destination inside the workgroup's share among themselves
COEF_HIST_WG_PER_CU = 2 # JS_COEF_HIST_WG_PER_CU: workgroups per compute unit (fewer if 160 KiB of LDS held fewer histograms of 64 * (2 R + 1) words)
COEF_HIST_RANGE_MAX = 127


def coef_hist_words(range_):
    """Words of one row of jsnoop_batch_pack_coef_hist: 64 histograms of 2 R + 1 bins, 64 minima, 64 maxima."""
    return 64 * (2 * range_ + 1) + 128


def coef_hist_share(total_units, cus, range_):
    """Units of one workgroup's contiguous share, as js_launch_coef_hist sizes it for a device of `cus` compute units."""
    want = min(cus * min(COEF_HIST_WG_PER_CU, 163840 // (256 * (2 * range_ + 1))), -(-total_units // COEF_HIST_WAVES))
    return -(-total_units // want)


class CoefHistSpec(C.Structure):
    """JsnoopCoefHistSpec of include/jsnoop_gpu.h: what a row of jsnoop_batch_pack_coef_hist counts (natural or zig-zag positions, quantised levels or the arena's
    values, bins -range .. range)."""
    _fields_ = [("struct_size", C.c_uint32), ("order", C.c_int32), ("quantised", C.c_int32), ("range", C.c_uint32)]


class CoefSpec(C.Structure):
    """JsnoopCoefSpec of include/jsnoop_gpu.h: what jsnoop_batch_pack_coefs writes (block- or frequency-major, int16 or float32, natural or zig-zag order)."""
    _fields_ = [("struct_size", C.c_uint32), ("layout", C.c_int32), ("dtype", C.c_int32), ("order", C.c_int32)]


class CoefDst(C.Structure):
    """JsnoopCoefDst of include/jsnoop_gpu.h: one destination in device memory -- component `comp` of the image listed at the same place; pitches in bytes, 0 = dense."""
    _fields_ = [("ptr", C.c_void_p), ("row_pitch", C.c_uint64), ("plane_pitch", C.c_uint64), ("comp", C.c_uint32), ("reserved", C.c_uint32)]


PLANE_FULL, PLANE_NATIVE = 0, 1
PLANE_I16, PLANE_U8, PLANE_F32 = 0, 1, 2
PLANE_SEG = 512         # JS_PLANE_SEG of csrc/jsnoop_types.h: elements of one output row a wave moves at a time (k_pack_planes)


class PlaneSpec(C.Structure):
    """JsnoopPlaneSpec of include/jsnoop_gpu.h: what jsnoop_batch_pack_planes writes (cropped planes or the component's own grid; int16, uint8 or float32 with
    scale and bias by component)."""
    _fields_ = [("struct_size", C.c_uint32), ("res", C.c_int32), ("dtype", C.c_int32), ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class PlaneDst(C.Structure):
    """JsnoopPlaneDst of include/jsnoop_gpu.h: one destination in device memory -- component `comp` of the image listed at the same place; pitch in bytes, 0 = dense."""
    _fields_ = [("ptr", C.c_void_p), ("row_pitch", C.c_uint64), ("comp", C.c_uint32), ("reserved", C.c_uint32)]


EXPORT_OK, EXPORT_INEXACT, EXPORT_UNCODABLE, EXPORT_UNSUPPORTED = 0, 1, 2, 3
EXPORT_TILE = 256       # JSNOOP_EXPORT_TILE of include/jsnoop_gpu.h: blocks of one image a workgroup measures, and writes the bits of, at a time
EXPORT_SCAN = 256       # JSNOOP_EXPORT_SCAN: tiles (or stuffing chunks) of one image a prefix-sum step covers
EXPORT_CHUNK = 4096     # JSNOOP_EXPORT_CHUNK: bytes of the un-stuffed stream a workgroup stuffs at a time
EXPORT_WINDOW = 8192    # JSNOOP_EXPORT_WINDOW: bytes of LDS in which a workgroup assembles its bit range


class ExportSpec(C.Structure):
    """JsnoopExportSpec of include/jsnoop_gpu.h: what jsnoop_batch_export_jpeg writes besides the image (the APP0 JFIF segment or none)."""
    _fields_ = [("struct_size", C.c_uint32), ("jfif", C.c_int32)]


HUFFMAN_ANNEX_K, HUFFMAN_OPTIMAL = 0, 1
HUFFMAN_MODES = {"annex_k": HUFFMAN_ANNEX_K, "optimal": HUFFMAN_OPTIMAL}


class ExportCoding(C.Structure):
    """JsnoopExportCoding of include/jsnoop_gpu.h: which Huffman tables jsnoop_batch_export_jpeg_coded writes (Annex K's, or each image's own, built on the device)."""
    _fields_ = [("struct_size", C.c_uint32), ("huffman", C.c_int32)]


def export_coding(lib, huffman):
    """The JsnoopExportCoding of huffman = "annex_k" | "optimal"."""
    if huffman not in HUFFMAN_MODES:
        raise ValueError('huffman must be "annex_k" or "optimal", not %r' % (huffman,))
    c = ExportCoding()
    lib.jsnoop_export_coding_defaults(C.byref(c))
    c.huffman = HUFFMAN_MODES[huffman]
    return c


RESTART_NONE, RESTART_MCUS, RESTART_ROWS, RESTART_SOURCE = 0, 1, 2, 3


class ExportRestart(C.Structure):
    """JsnoopExportRestart of include/jsnoop_gpu.h: the restart interval jsnoop_batch_export_jpeg_rst writes every entry with."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("interval", C.c_uint32), ("reserved", C.c_uint32)]


def export_restart(lib, restart):
    """The JsnoopExportRestart of restart = 0 (none) | an int (MCUs) | ("rows", n) | "source".  Values are handed to the library as given: it refuses
    an interval above 65535."""
    r = ExportRestart()
    lib.jsnoop_export_restart_defaults(C.byref(r))
    if isinstance(restart, str) and restart == "source":
        r.mode = RESTART_SOURCE
    elif isinstance(restart, (tuple, list)) and len(restart) == 2 and restart[0] == "rows" and isinstance(restart[1], int) and not isinstance(restart[1], bool) and 0 <= restart[1] < 1 << 32:
        r.mode = RESTART_ROWS; r.interval = restart[1]
    elif isinstance(restart, int) and not isinstance(restart, bool) and 0 <= restart < 1 << 32:
        r.mode = RESTART_MCUS if restart else RESTART_NONE; r.interval = restart
    else:
        raise ValueError('restart must be 0, a number of MCUs, ("rows", n) or "source", not %r' % (restart,))
    return r


PROGRESSIVE_OFF, PROGRESSIVE_DEFAULT, PROGRESSIVE_SCRIPT = 0, 1, 2
EXPORT_MAX_SCANS = 256  # JSNOOP_EXPORT_MAX_SCANS of include/jsnoop_gpu.h


class ExportScan(C.Structure):
    """JsnoopExportScan of include/jsnoop_gpu.h: one scan of a progressive script (comps: bit c = component c)."""
    _fields_ = [("comps", C.c_uint8), ("ss", C.c_uint8), ("se", C.c_uint8), ("ah", C.c_uint8), ("al", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class ExportProgressive(C.Structure):
    """JsnoopExportProgressive of include/jsnoop_gpu.h: the scan script jsnoop_batch_export_jpeg_prog writes progressive files along."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("nscans", C.c_uint32), ("reserved", C.c_uint32), ("scans", C.POINTER(ExportScan))]


def export_progressive(lib, progressive):
    """The JsnoopExportProgressive of progressive = False (baseline) | True (the built-in script) | a list of scans (components, ss, se, ah, al),
    components an iterable of indices or one index.  The scans are handed to the library as given: it refuses a script that breaks a rule.  The struct
    keeps the scan array alive (._scans)."""
    p = ExportProgressive()
    lib.jsnoop_export_progressive_defaults(C.byref(p))
    if progressive is False or progressive is None:
        return p
    if progressive is True:
        p.mode = PROGRESSIVE_DEFAULT
        return p
    try:
        scans = [tuple(s) for s in progressive]
        arr = (ExportScan * max(len(scans), 1))()
        for i, (comps, ss, se, ah, al) in enumerate(scans):
            mask = 0
            for c in ([comps] if isinstance(comps, int) else comps):
                if not 0 <= int(c) < 8:
                    raise ValueError
                mask |= 1 << int(c)
            for v in (ss, se, ah, al):                                    # (a c_uint8 field would take 319 as 63 without a word)
                if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 255:
                    raise ValueError
            arr[i].comps = mask; arr[i].ss = ss; arr[i].se = se; arr[i].ah = ah; arr[i].al = al
    except (TypeError, ValueError):
        raise ValueError("progressive must be False, True or a list of scans (components, ss, se, ah, al) with values 0 .. 255, not %r" % (progressive,)) from None
    p.mode = PROGRESSIVE_SCRIPT; p.nscans = len(scans); p.scans = C.cast(arr, C.POINTER(ExportScan)); p._scans = arr
    return p


ENCODE_444, ENCODE_422, ENCODE_420 = 0, 1, 2
ENCODE_SUBSAMPLING = {"4:4:4": ENCODE_444, "4:2:2": ENCODE_422, "4:2:0": ENCODE_420, 0: ENCODE_444, 1: ENCODE_422, 2: ENCODE_420}
ENCODE_INTERLEAVED, ENCODE_PLANAR = 0, 1
ENCODE_RGB, ENCODE_BGR = 0, 1
ENCODE_RUN = 8          # JSNOOP_ENCODE_RUN of include/jsnoop_gpu.h: MCUs of one MCU row a wave encodes at a time


class EncodeSpec(C.Structure):
    """JsnoopEncodeSpec of include/jsnoop_gpu.h: quality or tables, and the chroma subsampling, of one jsnoop_encode_run."""
    _fields_ = [("struct_size", C.c_uint32), ("quality", C.c_int32), ("subsampling", C.c_int32), ("reserved", C.c_uint32), ("qtables", C.POINTER(C.c_uint8))]


class EncodeSrc(C.Structure):
    """JsnoopEncodeSrc of include/jsnoop_gpu.h: one 8-bit picture in device memory (pitches in bytes, 0 = dense)."""
    _fields_ = [("ptr", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("channels", C.c_uint32), ("layout", C.c_int32), ("order", C.c_int32),
                ("pixel_stride", C.c_uint32), ("row_pitch", C.c_uint64), ("plane_pitch", C.c_uint64), ("bottom_up", C.c_uint32), ("reserved", C.c_uint32)]


def encode_spec(lib, quality=75, subsampling="4:2:0", qtables=None):
    """The JsnoopEncodeSpec of quality 1..100 | qtables = (luma64, chroma64) in natural order, and subsampling "4:4:4" | "4:2:2" | "4:2:0" (or 0 | 1 | 2).
    Values are handed to the library as given: it refuses what is out of range.  The struct keeps the table bytes alive (._tables)."""
    if subsampling not in ENCODE_SUBSAMPLING:
        raise ValueError('subsampling must be "4:4:4", "4:2:2" or "4:2:0", not %r' % (subsampling,))
    s = EncodeSpec()
    lib.jsnoop_encode_spec_defaults(C.byref(s))
    s.quality = int(quality); s.subsampling = ENCODE_SUBSAMPLING[subsampling]
    if qtables is not None:
        try:
            luma, chroma = ([int(v) for v in t] for t in qtables)
            if len(luma) != 64 or len(chroma) != 64 or not all(0 <= v <= 255 for v in luma + chroma):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError("qtables must be two tables of 64 values 1..255 (luma, chroma), natural order") from None
        arr = (C.c_uint8 * 128)(*(luma + chroma))
        s.qtables = C.cast(arr, C.POINTER(C.c_uint8)); s._tables = arr
    return s


XFORM_NONE, XFORM_FLIP_H, XFORM_FLIP_V, XFORM_TRANSPOSE, XFORM_TRANSVERSE, XFORM_ROT_90, XFORM_ROT_180, XFORM_ROT_270 = range(8)      # libjpeg's JXFORM codes; ROT_90 is clockwise
XFORM_OPS = {"none": XFORM_NONE, "flip_h": XFORM_FLIP_H, "flip_v": XFORM_FLIP_V, "transpose": XFORM_TRANSPOSE, "transverse": XFORM_TRANSVERSE,
             "rot90": XFORM_ROT_90, "rot180": XFORM_ROT_180, "rot270": XFORM_ROT_270}
XFORM_EDGE_TRIM, XFORM_EDGE_PERFECT = 0, 1
XFORM_EDGES = {"trim": XFORM_EDGE_TRIM, "perfect": XFORM_EDGE_PERFECT}
XFORM_OK, XFORM_IMPERFECT, XFORM_EMPTY, XFORM_UNSUPPORTED = 0, 1, 2, 3
XFORM_EXIF = {1: XFORM_NONE, 2: XFORM_FLIP_H, 3: XFORM_ROT_180, 4: XFORM_FLIP_V, 5: XFORM_TRANSPOSE, 6: XFORM_ROT_90, 7: XFORM_TRANSVERSE, 8: XFORM_ROT_270}   # EXIF orientation -> the op that sets it upright
TRANSFORM_RUN = 8       # JSNOOP_TRANSFORM_RUN of include/jsnoop_gpu.h: destination blocks a wave moves at a time


class TransformSpec(C.Structure):
    """JsnoopTransformSpec of include/jsnoop_gpu.h: op, edge mode, grayscale and crop of one jsnoop_transform_run."""
    _fields_ = [("struct_size", C.c_uint32), ("op", C.c_int32), ("edge", C.c_int32), ("grayscale", C.c_uint32), ("crop", C.c_uint32), ("crop_x", C.c_uint32),
                ("crop_y", C.c_uint32), ("crop_w", C.c_uint32), ("crop_h", C.c_uint32), ("reserved", C.c_uint32)]


def transform_spec(lib, op="none", edge="trim", grayscale=False, crop=None):
    """The JsnoopTransformSpec of op (a name of XFORM_OPS or a JXFORM code), edge ("trim" | "perfect" or 0 | 1), grayscale and crop = (x, y, w, h) | None.
    Numbers are handed to the library as given: it refuses what is out of range."""
    s = TransformSpec()
    lib.jsnoop_transform_spec_defaults(C.byref(s))
    if isinstance(op, str) and op not in XFORM_OPS:
        raise ValueError("op must be one of %s or a JXFORM code, not %r" % (", ".join(XFORM_OPS), op))
    if isinstance(edge, str) and edge not in XFORM_EDGES:
        raise ValueError('edge must be "trim" or "perfect", not %r' % (edge,))
    s.op = XFORM_OPS[op] if isinstance(op, str) else int(op)
    s.edge = XFORM_EDGES[edge] if isinstance(edge, str) else int(edge)
    s.grayscale = int(grayscale)
    if crop is not None:
        try:
            x, y, w, h = (int(v) for v in crop)
        except (TypeError, ValueError):
            raise ValueError("crop must be (x, y, w, h)") from None
        s.crop = 1; s.crop_x, s.crop_y, s.crop_w, s.crop_h = x, y, w, h
    return s


CARVE_OK, CARVE_NO_SOS, CARVE_NO_EOI, CARVE_STOPPED, CARVE_LIMIT = 0, 1, 2, 3, 4
CARVE_NOT_A_MARKER, CARVE_RST_OUTSIDE_SCAN, CARVE_BAD_LENGTH, CARVE_UNKNOWN_MARKER = 1, 2, 3, 4
CARVE_SEEN_SOI_AGAIN, CARVE_SEEN_DQT, CARVE_SEEN_DHT, CARVE_SEEN_DRI, CARVE_SEEN_AVI1 = 1, 2, 4, 8, 16
CARVE_LANE = 16         # JSNOOP_CARVE_LANE of include/jsnoop_gpu.h: bytes a lane classifies at a time, one 16-byte load
CARVE_WAVE = 1024       # JSNOOP_CARVE_WAVE: ... and a wave
CARVE_TILE = 16384      # JSNOOP_CARVE_TILE: bytes of a workgroup's tile, counted from the 16-byte boundary at or below the blob
CARVE_WALK = 256        # JSNOOP_CARVE_WALK: candidates of one workgroup of the walk kernel
CARVE_REC_WORDS = 16    # JSNOOP_CARVE_REC_WORDS: words of a record in device memory


class CarveSpec(C.Structure):
    """JsnoopCarveSpec of include/jsnoop_gpu.h: the marker cap of one walk and the scratch budget of one call (0 = half of the device's free memory)."""
    _fields_ = [("struct_size", C.c_uint32), ("max_markers", C.c_uint32), ("max_scratch_bytes", C.c_uint64)]


class CarveFrame(C.Structure):
    """JsnoopCarveFrame of include/jsnoop_gpu.h: one candidate of a carved blob and how its marker walk ended."""
    _fields_ = [("struct_size", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("status", C.c_int32), ("reason", C.c_int32),
                ("detail_pos", C.c_uint32), ("detail_byte", C.c_uint32), ("seen", C.c_uint32), ("sof_code", C.c_uint32), ("precision", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("components", C.c_uint32), ("sos_pos", C.c_uint32), ("scan_start", C.c_uint32),
                ("scans", C.c_uint32), ("markers", C.c_uint32), ("parent", C.c_int32)]


JOB_FILE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(JobFile))

XC_BACKEND_GENERIC, XC_WRITE_V1, XC_NO_TAIL, XC_SIDE_EXACT, XC_CAND_VERIFY, XC_UNSTUFF_3PASS, XC_DC_GENERIC = 1, 2, 4, 8, 16, 32, 64
DBG_CAND, DBG_CAND_LINKS, DBG_TAIL, DBG_TIMING = 1, 2, 4, 8

_u, _i, _p, _sz = C.c_uint, C.c_int, C.c_void_p, C.c_size_t
_PU, _PI = C.POINTER(C.c_uint), C.POINTER(C.c_int)

# name -> (restype, argtypes); every symbol include/jsnoop_gpu.h declares
SIGNATURES = {
    "jsnoop_abi_version": (_i, []),
    "jsnoop_selftest_tables": (_i, [C.c_uint, C.c_uint]),
    "jsnoop_selftest_bytes": (_i, [C.c_uint, C.c_uint]),
    "jsnoop_last_error": (C.c_char_p, []),
    "jsnoop_device_count": (_i, []),
    "jsnoop_set_device": (_i, [_i]),
    "jsnoop_create": (_p, []),
    "jsnoop_destroy": (None, [_p]),
    "jsnoop_reset": (None, [_p]),
    "jsnoop_reset_state": (None, [_p]),
    "jsnoop_reset_dqt_tables": (None, [_p]),
    "jsnoop_reset_dht_lookup": (None, [_p]),
    "jsnoop_set_image_dimensions": (None, [_p, _u, _u]),
    "jsnoop_get_image_dimensions": (None, [_p, _PU, _PU]),
    "jsnoop_dib_temp_create": (_p, [_p, _u, _u]),
    "jsnoop_set_dib_temp_ready": (None, [_p, _i]),
    "jsnoop_get_dib_temp_ready": (_i, [_p]),
    "jsnoop_set_preview_is_jpeg": (None, [_p, _i]),
    "jsnoop_set_log_callback": (None, [_p, LOG_FN, _p]),
    "jsnoop_set_options": (None, [_p, _i, _i, _i, _u]),
    "jsnoop_set_dqt_entry": (_i, [_p, _u, _u, _u, _u]),
    "jsnoop_set_dqt_tables": (_i, [_p, _u, _u]),
    "jsnoop_get_dqt_entry": (_u, [_p, _u, _u]),
    "jsnoop_set_dht_entry": (_i, [_p, _u, _u, _u, _u, _u, _u, _u]),
    "jsnoop_set_dht_size": (_i, [_p, _u, _u, _u]),
    "jsnoop_set_dht_tables": (_i, [_p, _u, _u, _u]),
    "jsnoop_set_sof_samp_factors": (None, [_p, _u, _u, _u]),
    "jsnoop_set_precision": (None, [_p, _u]),
    "jsnoop_set_image_details": (None, [_p, _u, _u, _u, _u, _i, _u]),
    "jsnoop_jfif_walk": (_i, [_p, _p, _sz, _PU]),
    "jsnoop_decode_scan_img": (None, [_p, _p, _sz, _u, _i, _i]),
    "jsnoop_decode_progressive": (_i, [_p, _p, _sz]),
    "jsnoop_is_preview_ready": (_i, [_p]),
    "jsnoop_get_image_size": (None, [_p, _PU, _PU]),
    "jsnoop_get_bitmap_ptr": (_p, [_p]),
    "jsnoop_get_bitmap_dev": (_p, [_p]),
    "jsnoop_get_pixmap_ptrs": (None, [_p, C.POINTER(_p), C.POINTER(_p), C.POINTER(_p)]),
    "jsnoop_lookup_file_pos_mcu": (None, [_p, _u, _u, _PU, _PU]),
    "jsnoop_lookup_file_pos_pix": (None, [_p, _u, _u, _PU, _PU]),
    "jsnoop_lookup_blk_ycc": (None, [_p, _u, _u, _PI, _PI, _PI]),
    "jsnoop_pixel_to_mcu": (None, [_p, _u, _u, _PU, _PU]),
    "jsnoop_pixel_to_blk": (None, [_p, _u, _u, _PU, _PU]),
    "jsnoop_mcu_xy_to_linear": (_u, [_p, _u, _u]),
    "jsnoop_set_dump_histo_y": (None, [_p, _i]),
    "jsnoop_overlay_install": (_i, [_p, _p, _u, _u]),
    "jsnoop_overlay_remove_all": (None, [_p]),
    "jsnoop_overlay_get_num": (_u, [_p]),
    "jsnoop_overlay_get": (_i, [_p, _u, C.POINTER(_p), _PU, _PU]),
    "jsnoop_set_preview_mode": (None, [_p, _u]),
    "jsnoop_get_preview_mode": (_u, [_p]),
    "jsnoop_set_preview_ycc_offset": (None, [_p, _u, _u, _i, _i, _i]),
    "jsnoop_get_preview_ycc_offset": (None, [_p, _PU, _PU, _PI, _PI, _PI]),
    "jsnoop_set_preview_mcu_insert": (None, [_p, _u, _u, _i]),
    "jsnoop_get_preview_mcu_insert": (None, [_p, _PU, _PU, _PU]),
    "jsnoop_get_geometry": (None, [_p, _PU]),
    "jsnoop_mcu_file_map": (_p, [_p]),
    "jsnoop_blk_dc_ptrs": (None, [_p, C.POINTER(_p), C.POINTER(_p), C.POINTER(_p)]),
    "jsnoop_dht_histo": (_p, [_p]),
    "jsnoop_scan_status": (None, [_p, _PU]),
    "jsnoop_bright_avg": (None, [_p, _PI]),
    "jsnoop_get_color_stats": (None, [_p, _p]),
    "jsnoop_export_tiff": (_i, [_p, C.c_char_p, _i]),
    "jsnoop_idct_lut": (_p, [_p]),
    "jsnoop_dht_lookupfast": (_p, [_p]),
    "jsnoop_idct_block": (None, [_p, _p, _p]),
    "jsnoop_color_sweep": (C.c_int, [_p, _p]),
    "jsnoop_color_offsets_sweep": (C.c_int, [_p, _p]),
    "jsnoop_last_path": (_i, [_p]),
    "jsnoop_last_flags": (C.c_uint32, [_p]),
    "jsnoop_last_side_mode": (_i, [_p]),
    "jsnoop_batch_create": (_p, [_p]),
    "jsnoop_batch_destroy": (None, [_p]),
    "jsnoop_batch_clear": (None, [_p]),
    "jsnoop_batch_set_options": (None, [_p, _i, _i, _i]),
    "jsnoop_batch_add": (_i, [_p, _p, _p, _sz, _u]),
    "jsnoop_batch_add_jpeg": (_i, [_p, _p, _sz]),
    "jsnoop_batch_tile": (_i, [_p, _i]),
    "jsnoop_batch_set_split": (_i, [_p, _i]),
    "jsnoop_batch_split_parts": (_i, [_p]),
    "jsnoop_tuning_defaults": (None, [C.POINTER(Tuning)]),
    "jsnoop_tuning_defaults_sized": (None, [C.POINTER(Tuning), C.c_uint32]),
    "jsnoop_batch_set_tuning": (_i, [_p, C.POINTER(Tuning)]),
    "jsnoop_batch_get_tuning": (None, [_p, C.POINTER(Tuning)]),
    "jsnoop_set_tuning": (_i, [_p, C.POINTER(Tuning)]),
    "jsnoop_batch_count": (_i, [_p]),
    "jsnoop_batch_upload": (_i, [_p]),
    "jsnoop_batch_decode": (_i, [_p]),
    "jsnoop_batch_sync": (_i, [_p]),
    "jsnoop_batch_last_form": (_i, [_p]),
    "jsnoop_last_form": (_i, [_p]),
    "jsnoop_batch_decode_timed": (C.c_double, [_p, _i, C.POINTER(C.c_double)]),
    "jsnoop_stage_name": (C.c_char_p, [_i]),
    "jsnoop_batch_image_info": (_i, [_p, _i, _PU]),
    "jsnoop_batch_dib_dev": (_p, [_p, _i]),
    "jsnoop_batch_read_dib": (_i, [_p, _i, _p]),
    "jsnoop_batch_read_planes": (_i, [_p, _i, _p, _p, _p]),
    "jsnoop_batch_read_coefs": (_i, [_p, _i, _p, _sz]),
    "jsnoop_batch_color_stats": (_i, [_p, _i, _i, _p]),
    "jsnoop_batch_dib_hashes": (_i, [_p, _p]),
    "jsnoop_batch_enable_log": (_i, [_p, _i]),
    "jsnoop_batch_side_outputs": (_i, [_p, _i, _p, _p, _p, _p, _p, _PU, _PI]),
    "jsnoop_batch_log": (_i, [_p, _i, _i, _i, _i, LOG_FN, _p]),
    "jsnoop_batch_export_tiff": (_i, [_p, _i, C.c_char_p, _i]),
    "jsnoop_batch_algorithmic_bytes": (C.c_uint64, [_p]),
    "jsnoop_batch_add_progressive": (_i, [_p, _p, _sz]),
    "jsnoop_pipeline_create": (_p, [_i]),
    "jsnoop_pipeline_destroy": (None, [_p]),
    "jsnoop_pipeline_slot": (_p, [_p, _i]),
    "jsnoop_pipeline_run": (_i, [_p, _i, _i, C.POINTER(C.c_double)]),
    "jsnoop_batch_pixels": (C.c_uint64, [_p]),
    "jsnoop_batch_device_bytes": (C.c_uint64, [_p]),
    "jsnoop_pack_spec_defaults": (None, [C.POINTER(PackSpec)]),
    "jsnoop_batch_pack_bytes": (C.c_uint64, [_p, C.POINTER(PackSpec), _i]),
    "jsnoop_batch_pack": (_i, [_p, C.POINTER(PackSpec), _PI, _i, C.POINTER(PackDst)]),
    "jsnoop_batch_pack_resized": (_i, [_p, C.POINTER(PackSpec), _i, _PI, _i, C.POINTER(ResizeDst)]),
    "jsnoop_batch_device": (_i, [_p]),
    "jsnoop_coef_spec_defaults": (None, [C.POINTER(CoefSpec)]),
    "jsnoop_batch_coef_grid": (_i, [_p, _i, _i, _PU, _PU]),
    "jsnoop_batch_coef_bytes": (C.c_uint64, [_p, C.POINTER(CoefSpec), _i, _i]),
    "jsnoop_batch_pack_coefs": (_i, [_p, C.POINTER(CoefSpec), _PI, _i, C.POINTER(CoefDst)]),
    "jsnoop_batch_image_dqt": (_i, [_p, _i, _i, C.POINTER(C.c_uint16)]),
    "jsnoop_batch_pack_stats": (_i, [_p, _i, _PI, _i, _p, C.c_uint64, _p]),
    "jsnoop_batch_read_stats": (_i, [_p, _i, _PI, _i, _p]),
    "jsnoop_coef_hist_spec_defaults": (None, [C.POINTER(CoefHistSpec)]),
    "jsnoop_coef_hist_words": (C.c_uint32, [C.POINTER(CoefHistSpec)]),
    "jsnoop_batch_pack_coef_hist": (_i, [_p, C.POINTER(CoefHistSpec), _PI, _PI, _i, _p, C.c_uint64]),
    "jsnoop_batch_read_coef_hist": (_i, [_p, C.POINTER(CoefHistSpec), _PI, _PI, _i, _p]),
    "jsnoop_plane_spec_defaults": (None, [C.POINTER(PlaneSpec)]),
    "jsnoop_batch_plane_size": (_i, [_p, C.POINTER(PlaneSpec), _i, _i, _PU, _PU]),
    "jsnoop_batch_plane_bytes": (C.c_uint64, [_p, C.POINTER(PlaneSpec), _i, _i]),
    "jsnoop_batch_pack_planes": (_i, [_p, C.POINTER(PlaneSpec), _PI, _i, C.POINTER(PlaneDst)]),
    "jsnoop_batch_ijg_renderable": (_i, [_p, _i]),
    "jsnoop_batch_pack_ijg": (_i, [_p, C.POINTER(PackSpec), _PI, _i, C.POINTER(PackDst)]),
    "jsnoop_batch_ijg_scaled_size": (_i, [_p, _i, C.c_uint, _PU, _PU]),
    "jsnoop_batch_pack_ijg_scaled_bytes": (C.c_uint64, [_p, C.POINTER(PackSpec), C.c_uint, _i]),
    "jsnoop_batch_pack_ijg_scaled": (_i, [_p, C.POINTER(PackSpec), C.c_uint, _PI, _i, C.POINTER(PackDst)]),
    "jsnoop_export_spec_defaults": (None, [C.POINTER(ExportSpec)]),
    "jsnoop_batch_export_jpeg": (_i, [_p, C.POINTER(ExportSpec), _PI, _i]),
    "jsnoop_batch_export_count": (_i, [_p]),
    "jsnoop_batch_export_file": (_i, [_p, _i, C.POINTER(_p), C.POINTER(C.c_uint64), _PI, C.POINTER(C.c_uint32), _PI]),
    "jsnoop_batch_read_export": (C.c_int64, [_p, _i, _p, C.c_uint64]),
    "jsnoop_batch_export_copy": (C.c_int64, [_p, _i, _p, C.c_uint64]),
    "jsnoop_export_jpeg": (_i, [_p, C.c_char_p]),
    "jsnoop_export_coding_defaults": (None, [C.POINTER(ExportCoding)]),
    "jsnoop_batch_export_jpeg_coded": (_i, [_p, C.POINTER(ExportSpec), C.POINTER(ExportCoding), _PI, _i]),
    "jsnoop_batch_export_tables": (_i, [_p, _i, _i, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "jsnoop_export_jpeg_coded": (_i, [_p, C.c_char_p, C.POINTER(ExportCoding)]),
    "jsnoop_export_restart_defaults": (None, [C.POINTER(ExportRestart)]),
    "jsnoop_batch_export_jpeg_rst": (_i, [_p, C.POINTER(ExportSpec), C.POINTER(ExportCoding), C.POINTER(ExportRestart), _PI, _i]),
    "jsnoop_batch_export_restart": (_i, [_p, _i, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "jsnoop_export_jpeg_rst": (_i, [_p, C.c_char_p, C.POINTER(ExportCoding), C.POINTER(ExportRestart)]),
    "jsnoop_export_progressive_defaults": (None, [C.POINTER(ExportProgressive)]),
    "jsnoop_batch_export_jpeg_prog": (_i, [_p, C.POINTER(ExportSpec), C.POINTER(ExportCoding), C.POINTER(ExportRestart), C.POINTER(ExportProgressive), _PI, _i]),
    "jsnoop_batch_export_scan_count": (_i, [_p, _i]),
    "jsnoop_batch_export_scan_info": (_i, [_p, _i, _i, C.POINTER(ExportScan), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jsnoop_batch_export_scan_tables": (_i, [_p, _i, _i, _i, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "jsnoop_export_jpeg_prog": (_i, [_p, C.c_char_p, C.POINTER(ExportCoding), C.POINTER(ExportRestart), C.POINTER(ExportProgressive)]),
    "jsnoop_encode_create": (_p, [_p]),
    "jsnoop_encode_destroy": (None, [_p]),
    "jsnoop_encode_spec_defaults": (None, [C.POINTER(EncodeSpec)]),
    "jsnoop_encode_qtables": (_i, [C.POINTER(EncodeSpec), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "jsnoop_encode_run": (_i, [_p, C.POINTER(EncodeSpec), C.POINTER(EncodeSrc), _i]),
    "jsnoop_encode_count": (_i, [_p]),
    "jsnoop_encode_image_info": (_i, [_p, _i, _PU]),
    "jsnoop_encode_read_coefs": (_i, [_p, _i, C.POINTER(C.c_int16), C.POINTER(C.c_int16), _sz]),
    "jsnoop_encode_export": (_i, [_p, C.POINTER(ExportSpec), C.POINTER(ExportCoding), C.POINTER(ExportRestart), C.POINTER(ExportProgressive), _PI, _i]),
    "jsnoop_encode_export_count": (_i, [_p]),
    "jsnoop_encode_export_file": (_i, [_p, _i, C.POINTER(_p), C.POINTER(C.c_uint64), _PI, C.POINTER(C.c_uint32), _PI]),
    "jsnoop_encode_read_export": (C.c_int64, [_p, _i, _p, C.c_uint64]),
    "jsnoop_encode_export_copy": (C.c_int64, [_p, _i, _p, C.c_uint64]),
    "jsnoop_encode_export_scan_count": (_i, [_p, _i]),
    "jsnoop_encode_export_scan_info": (_i, [_p, _i, _i, C.POINTER(ExportScan), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jsnoop_batch_stream": (_p, [_p]),
    "jsnoop_transform_create": (_p, [_p]),
    "jsnoop_transform_destroy": (None, [_p]),
    "jsnoop_transform_spec_defaults": (None, [C.POINTER(TransformSpec)]),
    "jsnoop_transform_run": (_i, [_p, _p, C.POINTER(TransformSpec), _PI, _i]),
    "jsnoop_transform_entry": (_i, [_p, _i, _PI, _PI]),
    "jsnoop_transform_entry_count": (_i, [_p]),
    "jsnoop_transform_count": (_i, [_p]),
    "jsnoop_transform_image_info": (_i, [_p, _i, _PU]),
    "jsnoop_transform_image_dqt": (_i, [_p, _i, _i, C.POINTER(C.c_uint16)]),
    "jsnoop_transform_read_coefs": (_i, [_p, _i, C.POINTER(C.c_int16), C.POINTER(C.c_int16), _sz]),
    "jsnoop_transform_export": (_i, [_p, C.POINTER(ExportSpec), C.POINTER(ExportCoding), C.POINTER(ExportRestart), C.POINTER(ExportProgressive), _PI, _i]),
    "jsnoop_transform_export_count": (_i, [_p]),
    "jsnoop_transform_export_file": (_i, [_p, _i, C.POINTER(_p), C.POINTER(C.c_uint64), _PI, C.POINTER(C.c_uint32), _PI]),
    "jsnoop_transform_read_export": (C.c_int64, [_p, _i, _p, C.c_uint64]),
    "jsnoop_transform_export_copy": (C.c_int64, [_p, _i, _p, C.c_uint64]),
    "jsnoop_transform_export_scan_count": (_i, [_p, _i]),
    "jsnoop_transform_export_scan_info": (_i, [_p, _i, _i, C.POINTER(ExportScan), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jsnoop_partition_lpt": (_i, [C.POINTER(C.c_uint64), _i, _i, _PI]),
    "jsnoop_job_create": (_p, [_PI, _i]),
    "jsnoop_job_destroy": (None, [_p]),
    "jsnoop_job_options_defaults": (None, [C.POINTER(JobOptions)]),
    "jsnoop_job_set_options": (_i, [_p, C.POINTER(JobOptions)]),
    "jsnoop_job_set_tuning": (_i, [_p, C.POINTER(Tuning)]),
    "jsnoop_job_add_file": (_i, [_p, _p, _sz]),
    "jsnoop_job_add_path": (_i, [_p, C.c_char_p]),
    "jsnoop_job_count": (_i, [_p]),
    "jsnoop_job_clear": (None, [_p]),
    "jsnoop_job_run": (_i, [_p, JOB_FILE_FN, _p, C.POINTER(JobStats)]),
    "jsnoop_job_file_result": (_i, [_p, _i, C.POINTER(JobFile)]),
    "jsnoop_carve_create": (_p, [_i]),
    "jsnoop_carve_destroy": (None, [_p]),
    "jsnoop_carve_spec_defaults": (None, [C.POINTER(CarveSpec)]),
    "jsnoop_carve_run": (_i, [_p, C.POINTER(CarveSpec), _p, C.c_uint64, _i]),
    "jsnoop_carve_host": (C.c_int64, [C.POINTER(CarveSpec), _p, C.c_uint64, C.POINTER(CarveFrame), C.c_uint64]),
    "jsnoop_carve_count": (C.c_int64, [_p]),
    "jsnoop_carve_frame": (_i, [_p, C.c_int64, C.POINTER(CarveFrame)]),
    "jsnoop_carve_frames": (C.c_int64, [_p, C.POINTER(CarveFrame), C.c_uint64]),
    "jsnoop_carve_frames_dev": (_p, [_p]),
    "jsnoop_carve_lists_dev": (_i, [_p, C.POINTER(_p), C.POINTER(_p)]),
    "jsnoop_carve_totals": (_i, [_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "jsnoop_carve_copy": (C.c_int64, [_p, _i, _p, C.c_uint64]),
    "jsnoop_job_add_carved": (_i, [_p, _p, C.c_uint64, C.POINTER(CarveFrame), C.c_int64, _i, _PI]),
}

_lib = None


def load(require_device: bool = True) -> C.CDLL:
    """Loads the shared library and types every entry point.  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C jpegsnoop_amd/csrc` (or __graft_entry__.build()). "
                "jpegsnoop_amd has no CPU fallback.")
        # torch first, where it is installed (README.md, "torch and the HIP runtime"): a PyTorch-ROCm wheel brings a HIP runtime of its own, a process drives the
        # GPU through ONE runtime, the library binds to the one that is loaded first, and torch cannot initialise its device behind another one.  In this
        # order both use the same runtime -- what bench.py has always done -- and JpegBatch.to_torch can hand torch's memory to the library.
        # JSNOOP_TORCH_FIRST=0 opts out (the library then binds to the runtime it was linked against, and to_torch cannot be used in the process);
        # a torch that is absent or does not import leaves a load that works as before.
        if os.environ.get("JSNOOP_TORCH_FIRST", "1") != "0":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError here = header/library mismatch
            fn.restype, fn.argtypes = res, args
        _lib = lib
    if require_device and _lib.jsnoop_device_count() <= 0:
        raise RuntimeError("no HIP device visible: jpegsnoop_amd decodes on an AMD GPU only (no CPU fallback)")
    return _lib


def last_error() -> str:
    return (load(False).jsnoop_last_error() or b"").decode()
