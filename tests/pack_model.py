"""Plain numpy model of jsnoop_batch_pack (include/jsnoop_gpu.h): a DIB -- bottom-up rows of img_x B,G,R,0 pixels, img_x x img_y rounded up to
whole MCUs -- as cropped, top-down, three-channel pixels.  The tests of the pack kernel compare against this model and nothing else."""
import struct

import numpy as np


def pack_model(dib, dim_x, dim_y, layout="CHW", dtype="uint8", bgr=False, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """dib: (img_y, img_x, 4) uint8 as JpegBatch.dib(i) or the oracle's dib().  Returns (3, dim_y, dim_x) or (dim_y, dim_x, 3).
    dtype "float32": float32(v) * float32(scale[c]) + float32(bias[c]) as two separately rounded numpy operations, c the OUTPUT channel."""
    assert layout in ("CHW", "HWC") and dtype in ("uint8", "float32")
    top_down = dib[::-1]
    out = top_down[:dim_y, :dim_x, :3] if bgr else top_down[:dim_y, :dim_x, 2::-1]
    if dtype == "float32":
        s = np.asarray(scale, np.float32).reshape(1, 1, 3)
        b = np.asarray(bias, np.float32).reshape(1, 1, 3)
        prod = out.astype(np.float32) * s                     # rounded once
        out = prod + b                                        # rounded again
        assert out.dtype == np.float32
    out = np.ascontiguousarray(out)
    return np.ascontiguousarray(out.transpose(2, 0, 1)) if layout == "CHW" else out


def f32(x: float) -> float:
    """x rounded to the nearest float32 (ties to even), as a Python float."""
    return struct.unpack("f", struct.pack("f", x))[0]


def two_roundings(v: int, s: float, b: float) -> float:
    """float32(float32(v * s) + b) for float32 s, b computed through doubles: an 8-bit v times a 24-bit s is exact in a double, and so is the
    sum of two float32 of these magnitudes, so each step is ONE rounding to float32."""
    return f32(f32(v * f32(s)) + f32(b))


def one_rounding(v: int, s: float, b: float) -> float:
    """What a fused multiply-add would give: float32(v * s + b) with the product unrounded."""
    return f32(v * f32(s) + f32(b))


def tells_fma_apart(scale, bias):
    """Per channel: the inputs v in 0..255 on which the two-rounding result and the fused one differ."""
    return [[v for v in range(256) if two_roundings(v, s, b) != one_rounding(v, s, b)] for s, b in zip(scale, bias)]
