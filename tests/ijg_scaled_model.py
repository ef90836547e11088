"""The definition of jsnoop_batch_pack_ijg_scaled -- TEST INFRASTRUCTURE and the authority k_render_ijg_scaled is compared with, byte for byte.

libjpeg's reduced-size decode (djpeg -scale 1/s, Image.draft, IMREAD_REDUCED_COLOR_s), s in {2, 4, 8}, from the coefficient arena of one image as
tests/ijg_model.py reads it (rows of 64 dequantised int16 values, slot 0 = the cumulative DC).  Everything not said here is ijg_model's: integer
arithmetic, DESCALE(x, n) = (x + (1 << (n - 1))) >> n, a 32-bit workspace whose sums wrap, sample = clamp(result + 128, 0, 255), the colour lines, the
renderable layouts.  Whole planes at a time in plain numpy; nothing of the kernel's structure.  DESIGN.md section 4.22.

  m = 8 / s.  The picture is X' = ceil(X / s) by Y' = ceil(Y / s), top-down, top-left.
  Transform size of component c (jdmaster.c): n = m, doubled while n < 8 and (hmax m) % (h_c n 2) == 0 and (vmax m) % (v_c n 2) == 0.  Grey, 4:4:4 and
  all of 4:2:2: n = m.  4:2:0: luma m, chroma 2 m -- the full 8 x 8 of ijg_model at s = 2.  A block yields n x n samples; the component's plane is its
  blocks side by side, cropped to dw = ceil(X h_c n / (hmax 8)) by dh = ceil(Y v_c n / (vmax 8)).
  Reduced transforms (jidctred.c, CONST_BITS 13, PASS1_BITS 2): pass 1 along the columns into n rows x 8 columns, pass 2 along each of the n rows.
    4 x 4, the step on v[0..7]:  t0 = v0 << 14;  t2 = v2 15137 - v6 6270;  t10 = t0 + t2;  t12 = t0 - t2;
            a = -v7 1730 + v5 11893 - v3 17799 + v1 8697;  b = -v7 4176 - v5 4926 + v3 7373 + v1 20995;
            outputs DESCALE of t10 + b, t12 + a, t12 - a, t10 - b by 12 (pass 1) and 19 (pass 2).  v4 is never read.
    2 x 2:  t10 = v0 << 15;  t0 = -v7 5906 + v5 6967 - v3 10426 + v1 29692;  outputs DESCALE of t10 + t0, t10 - t0 by 13 and 20.  v2, v4, v6 never read.
    1 x 1:  DESCALE(dc, 3).
  Upsampling by eh = hmax m / (h_c n), ev likewise: 1 x 1 everywhere but 4:2:2 chroma (2 x 1).  For s = 2, 4 that is ijg_model's h2v1 triangle filter on
  the reduced plane (indices clamped to dw, dw <= 2 replicated); for s = 8 plain replication (libjpeg has no filter where the smallest transform is 1 x 1).

`wrong` names one deliberately WRONG reading (tests/test_ijg_scaled_model.py shows that a named case refuses each): 'chroma_at_luma_size' (4:2:0 chroma
transformed at luma's size and upsampled 2 x 2), 'triangle_at_8' (the filter kept at s = 8 in 4:2:2), 'floor_size' (floor for the output size),
'index4_fed' (column / row 4 fed into the 4 x 4 as the 8-point even part takes it), 'dc_shift' (the 1 x 1 as dc >> 3 without rounding)."""
import numpy as np

import coef_model as CM
import ijg_model as M

WRONG = ("chroma_at_luma_size", "triangle_at_8", "floor_size", "index4_fed", "dc_shift")
SCALES = (2, 4, 8)


def out_size(width, height, s, wrong=None):
    if wrong == "floor_size":
        return max(1, width // s), max(1, height // s)
    return -(-width // s), -(-height // s)


def transform_size(hv, c, s, wrong=None):
    hmax = max(h for h, _ in hv); vmax = max(v for _, v in hv)
    m = 8 // s; n = m
    if wrong == "chroma_at_luma_size":
        return n
    while n < 8 and (hmax * m) % (hv[c][0] * n * 2) == 0 and (vmax * m) % (hv[c][1] * n * 2) == 0:
        n *= 2
    return n


def _descale(outs, shift):
    return np.stack([M._wrap32(M._wrap32(o) + (1 << (shift - 1))) >> shift for o in outs], -1)


def s4(v, shift, wrong=None):
    v = v.astype(np.int64)
    v0, v1, v2, v3, v4, v5, v6, v7 = (v[..., k] for k in range(8))
    t0 = ((v0 + v4) if wrong == "index4_fed" else v0) << 14
    t2 = v2 * 15137 - v6 * 6270
    t10 = t0 + t2; t12 = t0 - t2
    a = -v7 * 1730 + v5 * 11893 - v3 * 17799 + v1 * 8697
    b = -v7 * 4176 - v5 * 4926 + v3 * 7373 + v1 * 20995
    return _descale([t10 + b, t12 + a, t12 - a, t10 - b], shift)


def s2(v, shift):
    v = v.astype(np.int64)
    t10 = v[..., 0] << 15
    t0 = -v[..., 7] * 5906 + v[..., 5] * 6967 - v[..., 3] * 10426 + v[..., 1] * 29692
    return _descale([t10 + t0, t10 - t0], shift)


def idct(blocks, n, wrong=None):
    """[..., 8 rows, 8 columns] dequantised coefficients -> [..., n, n] results before the + 128 and the clamp (32-bit values)."""
    b = np.asarray(blocks).astype(np.int64)
    if n == 8:
        return M.idct(b)
    if n == 1:
        dc = b[..., 0:1, 0:1]
        return dc >> 3 if wrong == "dc_shift" else (dc + 4) >> 3
    f, p1, p2 = ((lambda v, sh: s4(v, sh, wrong)), 12, 19) if n == 4 else (s2, 13, 20)
    ws = f(b.swapaxes(-1, -2), p1).swapaxes(-1, -2)                  # pass 1: along the columns -> n rows x 8 columns
    return f(ws, p2)                                                 # pass 2: along each row


def render(arena, width, height, hv, s, wrong=None):
    """arena [blocks][64] int16 (slot 0 = cumulative DC) -> (pixels [Y'][X'][3] uint8, R G B; the largest |result| of the transforms)."""
    hv = [tuple(int(x) for x in c) for c in hv]
    assert M.renderable(hv) and s in SCALES, (hv, s)
    arena = np.asarray(arena); assert arena.dtype == np.int16 and arena.ndim == 2 and arena.shape[1] == 64, (arena.dtype, arena.shape)
    hmax = max(h for h, _ in hv); vmax = max(v for _, v in hv); m = 8 // s
    geo = CM.Geometry(hv, -(-width // (8 * hmax)), -(-height // (8 * vmax)))
    assert arena.shape[0] == geo.nblocks, (arena.shape, geo.nblocks)
    ow, oh = out_size(width, height, s, wrong)
    planes = []; peak = 0
    for c, (h, v) in enumerate(hv):
        n = transform_size(hv, c, s, wrong)
        bw, bh = geo.grid(c)
        res = idct(arena[geo.arena_index(c)].reshape(bh, bw, 8, 8), n, wrong)
        peak = max(peak, int(np.abs(res).max()))
        full = np.clip(res + 128, 0, 255).transpose(0, 2, 1, 3).reshape(bh * n, bw * n)
        dw, dh = -(-width * h * n // (hmax * 8)), -(-height * v * n // (vmax * 8))
        p = full[:dh, :dw]
        eh, ev = hmax * m // (h * n), vmax * m // (v * n)
        if (eh, ev) == (2, 1) and s == 8 and wrong != "triangle_at_8":
            p = np.repeat(p, 2, 1)
        else:
            p = M.upsample(p, eh, ev)
        planes.append(p[:oh, :ow])
    y = planes[0]
    if len(hv) == 1:
        return np.stack([y, y, y], -1).astype(np.uint8), peak
    cb = planes[1] - 128; cr = planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8), peak


def pillow_reduced(data, s, by_hand=False):
    """Pillow's (libjpeg-turbo's) decode of a file at 1 / s -> pixels [Y'][X'][3].  draft() with the size (max(1, X // s), max(1, Y // s)) selects exactly s
    when X >= s and Y >= s (both quotients fall in [s, 2 s)); for smaller pictures -- or with by_hand -- the decoder's scale is set the way draft sets it."""
    import io
    from PIL import Image, ImageFile
    im = Image.open(io.BytesIO(data))
    X, Y = im.size
    mode = "L" if im.mode == "L" else "RGB"
    if not by_hand and X >= s and Y >= s:
        im.draft(mode, (max(1, X // s), max(1, Y // s)))
    else:
        d, e, o, a = im.tile[0]
        im.tile = [ImageFile._Tile(d, (e[0], e[1], (e[2] - e[0] + s - 1) // s + e[0], (e[3] - e[1] + s - 1) // s + e[1]), o, a)]
        im._size = ((X + s - 1) // s, (Y + s - 1) // s)
        im.decoderconfig = (s, 0)
    assert im.size == (-(-X // s), -(-Y // s)), (im.size, X, Y, s)
    return np.asarray(im.convert("RGB"))
