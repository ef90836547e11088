"""Plain numpy model of jsnoop_batch_pack_resized (include/jsnoop_gpu.h): a rectangle of a DIB resampled to out_w x out_h.  Every output is
q = float32(float64(S) / float64(D)) with exact integers S and D (uint64 sums, one float64 division, one rounding to float32); uint8 output is
np.rint(q) (ties to even), float32 output is q * scale[c] + bias[c] as two separately rounded operations.  Imports nothing from the library;
the tests of k_pack_resize compare against this model and nothing else."""
import numpy as np

NEAREST, BILINEAR, AREA = 0, 1, 2
FILTERS = {"nearest": NEAREST, "bilinear": BILINEAR, "area": AREA}


def nearest_index(r, out):
    """Source index of every output index along one axis: ((2 o + 1) r) div (2 out)."""
    o = np.arange(out, dtype=np.int64)
    return ((2 * o + 1) * r) // (2 * out)


def bilinear_axis(r, out):
    """(i0, i1, frac, D) along one axis: P = (2 o + 1) r - out; P < 0 -> i0 = 0, frac = 0; else i0 = P div D, frac = P mod D with D = 2 out;
    i1 = min(i0 + 1, r - 1)."""
    o = np.arange(out, dtype=np.int64)
    d = 2 * out
    p = (2 * o + 1) * r - out
    neg = p < 0
    i0 = np.where(neg, 0, p // d)
    frac = np.where(neg, 0, p % d)
    return i0, np.minimum(i0 + 1, r - 1), frac.astype(np.uint64), np.uint64(d)


def area_weights(o, r, out):
    """(j0, w): the source indices j0 .. j0 + len(w) - 1 that output index o overlaps and the integer lengths of the overlaps, in units of 1 / out
    source pixel: output o covers [o r, (o + 1) r), source j covers [j out, (j + 1) out)."""
    lo, hi = o * r, (o + 1) * r
    j0, j1 = lo // out, (hi - 1) // out
    j = np.arange(j0, j1 + 1, dtype=np.int64)
    w = np.minimum((j + 1) * out, hi) - np.maximum(j * out, lo)
    assert (w > 0).all()
    return j0, w.astype(np.uint64)


def _area_reduce(a, out):
    """Contracts axis 0 of the integer array a (r, ...) with the area weights: (out, ...) uint64."""
    r = a.shape[0]
    res = np.zeros((out,) + a.shape[1:], np.uint64)
    for o in range(out):
        j0, w = area_weights(o, r, out)
        for b in range(0, len(w), 512):                          # (bands, so that a footprint of thousands of rows is never widened to uint64 at once)
            res[o] += np.tensordot(w[b:b + 512], a[j0 + b:j0 + b + len(w[b:b + 512])].astype(np.uint64), axes=(0, 0))
    return res


def resize_sd(R, out_w, out_h, filt):
    """R: (rh, rw, C) uint8.  Returns (S, D): S (out_h, out_w, C) uint64, D a Python int."""
    rh, rw = R.shape[:2]
    assert R.dtype == np.uint8 and rh >= 1 and rw >= 1 and out_w >= 1 and out_h >= 1
    if filt == NEAREST:
        return R[nearest_index(rh, out_h)][:, nearest_index(rw, out_w)].astype(np.uint64), 1
    if filt == BILINEAR:
        x0, x1, fx, dx = bilinear_axis(rw, out_w)
        y0, y1, fy, dy = bilinear_axis(rh, out_h)
        r64 = R.astype(np.uint64)
        wx0, wx1 = (dx - fx)[None, :, None], fx[None, :, None]
        wy0, wy1 = (dy - fy)[:, None, None], fy[:, None, None]
        s = wx0 * wy0 * r64[y0][:, x0] + wx1 * wy0 * r64[y0][:, x1] + wx0 * wy1 * r64[y1][:, x0] + wx1 * wy1 * r64[y1][:, x1]
        return s, int(dx) * int(dy)
    assert filt == AREA
    rows = _area_reduce(R, out_h)                                  # (out_h, rw, C)
    s = _area_reduce(np.ascontiguousarray(rows.transpose(1, 0, 2)), out_w)   # (out_w, out_h, C)
    return np.ascontiguousarray(s.transpose(1, 0, 2)), rw * rh


def resize_q(R, out_w, out_h, filt):
    """The interpolant: float32(float64(S) / float64(D)), (out_h, out_w, C)."""
    s, d = resize_sd(R, out_w, out_h, filt)
    assert int(s.max()) < 2 ** 53 and d < 2 ** 53
    q = (s.astype(np.float64) / np.float64(d)).astype(np.float32)
    assert q.dtype == np.float32
    return q


def crop_of(dib, dim_x, dim_y, roi=None, bgr=False):
    """The ROI as a top-down (rh, rw, 3) array in OUTPUT channel order: the plain pack of the image, cropped.  roi = (x, y, w, h) or None."""
    x, y, w, h = roi if roi is not None and (roi[2] or roi[3]) else (0, 0, dim_x, dim_y)
    assert 0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= dim_x and y + h <= dim_y
    top_down = dib[::-1][:dim_y, :dim_x]
    c = top_down[y:y + h, x:x + w, :3] if bgr else top_down[y:y + h, x:x + w, 2::-1]
    return np.ascontiguousarray(c)


def finish(q, layout="CHW", dtype="uint8", scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """q (out_h, out_w, 3) float32 in output channel order -> the bytes / floats of the destination."""
    assert layout in ("CHW", "HWC") and dtype in ("uint8", "float32") and q.dtype == np.float32
    if dtype == "uint8":
        out = np.rint(q).astype(np.uint8)
    else:
        prod = q * np.asarray(scale, np.float32).reshape(1, 1, 3)          # rounded once
        out = prod + np.asarray(bias, np.float32).reshape(1, 1, 3)         # rounded again
        assert out.dtype == np.float32
    out = np.ascontiguousarray(out)
    return np.ascontiguousarray(out.transpose(2, 0, 1)) if layout == "CHW" else out


def resize_model(dib, dim_x, dim_y, roi, out_w, out_h, filt, layout="CHW", dtype="uint8", bgr=False, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
    """dib: (img_y, img_x, 4) uint8 as JpegBatch.dib(i).  Returns (3, out_h, out_w) or (out_h, out_w, 3)."""
    return finish(resize_q(crop_of(dib, dim_x, dim_y, roi, bgr), out_w, out_h, filt), layout, dtype, scale, bias)
