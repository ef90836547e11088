"""Plain numpy model of jsnoop_batch_pack_planes (include/jsnoop_gpu.h): one retained int16 plane -- top-down, blk_xmax * 8 samples wide, MCU padding
included, as JpegBatch.planes(i)[c] or the oracle's planes()[c] -- as the tensor one destination receives.  The tests of the plane kernel compare against
this model and nothing else."""
import numpy as np

from pack_model import f32, tells_fma_apart


def plane_dims(dim_x, dim_y, eh, ev, res):
    """(h, w) of the output: the SOF dimensions (FULL), or ceil(dim / replication factor) each way (NATIVE)."""
    assert res in ("full", "native")
    if res == "full":
        return dim_y, dim_x
    return -(-dim_y // ev), -(-dim_x // eh)


def u8_value(v):
    """CapYccRange's value of int16 samples: min(max((v + 1024) / 8, 0), 255) with C's division, which truncates toward zero."""
    n = np.asarray(v).astype(np.int64) + 1024
    q = np.where(n >= 0, n // 8, -((-n) // 8))                  # numpy's // floors: toward zero through the magnitude
    return np.clip(q, 0, 255).astype(np.uint8)


def plane_model(P, dim_x, dim_y, eh, ev, res="full", dtype="int16", scale=1.0, bias=0.0):
    """P: (blk_ymax * 8, blk_xmax * 8) int16.  eh, ev: the replication factors of the component (expand_h, expand_v).  scale, bias: the component's
    own (one number each).  dtype "float32": float32(v) * float32(scale) + float32(bias) as two separately rounded numpy operations."""
    assert dtype in ("int16", "uint8", "float32") and P.dtype == np.int16
    h, w = plane_dims(dim_x, dim_y, eh, ev, res)
    out = P[:dim_y, :dim_x] if res == "full" else P[0:dim_y:ev, 0:dim_x:eh]
    assert out.shape == (h, w), (out.shape, h, w)
    if dtype == "uint8":
        out = u8_value(out)
    elif dtype == "float32":
        prod = out.astype(np.float32) * np.float32(scale)        # rounded once
        out = prod + np.float32(bias)                            # rounded again
        assert out.dtype == np.float32
    return np.ascontiguousarray(out)


def two_roundings(v, s, b):
    """float32(float32(v * s) + b) through doubles: an int16 v times a 24-bit s is exact in a double, and so is the sum of two float32 of these
    magnitudes, so each step is ONE rounding to float32."""
    return f32(f32(v * f32(s)) + f32(b))


def one_rounding(v, s, b):
    """What a fused multiply-add would give: float32(v * s + b) with the product unrounded."""
    return f32(v * f32(s) + f32(b))


def expand_factors(hs, vs, gray=False):
    """(eh, ev) per component of a file whose luma has hs x vs blocks per MCU and whose chroma has one (what harness.synth_jpeg writes)."""
    return [(1, 1)] if gray else [(1, 1), (hs, vs), (hs, vs)]


def fma_telling_values(scale, bias):
    """Per component: the sample values (pack_model.tells_fma_apart looks at 0 .. 255, all of them values a plane can hold) on which the two-rounding
    result and a fused multiply-add differ under that component's scale and bias."""
    return tells_fma_apart(scale, bias)
