"""The definition of jsnoop_batch_pack_ijg -- TEST INFRASTRUCTURE and the authority k_render_ijg is compared with, byte for byte.

From the coefficient arena of one image (rows of 64 dequantised int16 values, natural order, decode order, slot 0 replaced by the block's cumulative
DC as jsnoop_batch_pack_coefs does it) and the frame geometry to the pixels libjpeg gives: the integer "islow" inverse DCT, the triangle-filter
("fancy") chroma upsampling and the 16-bit fixed-point colour conversion.  Written from DESIGN.md section 4.21 in plain numpy -- whole planes at a
time, no units, no tiles, no halo, nothing of the kernel's structure.  All arithmetic is on integers, >> is arithmetic,
DESCALE(x, n) = (x + (1 << (n - 1))) >> n.

  1. IDCT per block: jidctint, CONST_BITS 13, PASS1_BITS 2.  Pass 1 over the eight COLUMNS, descaled by 11; pass 2 over the eight rows of pass 1's
     result, descaled by 18.  The workspace is 32 bits wide and every sum wraps modulo 2^32 (an arena from a damaged file may hold anything); the
     sample is clamp(result + 128, 0, 255), a true saturation of the 32-bit result.  libjpeg masks to 10 bits where its SIMD code saturates: the two
     agree while |result| <= 511, which render() reports so that a comparison with Pillow can assert it.
  2. component c has dw = ceil(X h_c / hmax) by dh = ceil(Y v_c / vmax) real samples; what its blocks hold beyond is never used, and the
     upsampling clamps its neighbours to that extent.
  3. chroma upsampling, indices clamped to [0, dh - 1] and [0, dw - 1]:
       2 x 1:  out[y][2i] = (3 p[y][i] + p[y][i-1] + 1) >> 2        out[y][2i+1] = (3 p[y][i] + p[y][i+1] + 2) >> 2
       2 x 2:  s[2j][i] = 3 p[j][i] + p[j-1][i]                      s[2j+1][i] = 3 p[j][i] + p[j+1][i]
               out[r][2i] = (3 s[r][i] + s[r][i-1] + 8) >> 4         out[r][2i+1] = (3 s[r][i] + s[r][i+1] + 7) >> 4
       with dw <= 2 libjpeg does not interpolate at all: the sample is replicated 2 x 1 or 2 x 2.  1 x 1: p itself.
  4. colour, cb = Cb - 128, cr = Cr - 128:  R = Y + ((91881 cr + 32768) >> 16),  G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
     B = Y + ((116130 cb + 32768) >> 16), each clamped to 0..255.  One component: R = G = B = Y.  The picture is the top-left X x Y, top-down.

Renderable: one component (one block per MCU), or three treated as Y, Cb, Cr with chroma at 1 x 1 and luma at 1 x 1, 2 x 1 or 2 x 2.

`wrong` names one deliberately WRONG reading of the text above (tests/test_ijg_model.py shows that a named case refuses each): 'pad_neighbours'
(the filter reads its neighbours from the block padding instead of clamping at dw / dh), 'interp_small' (interpolation at dw <= 2), 'bias_swapped'
(the biases 8 / 7 and 1 / 2 exchanged), 'rows_first' (rows before columns in the IDCT), 'g_separate' (G's two products rounded separately)."""
import numpy as np

import coef_model as CM

WRONG = ("pad_neighbours", "interp_small", "bias_swapped", "rows_first", "g_separate")


def renderable(hv):
    hv = [tuple(x) for x in hv]
    return hv == [(1, 1)] or (len(hv) == 3 and hv[1] == (1, 1) and hv[2] == (1, 1) and hv[0] in ((1, 1), (2, 1), (2, 2)))


def _wrap32(x):
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _step(v, shift):
    """The one-dimensional step of jidctint along the last axis (eight values of at most 32 bits, int64 here: no int64 sum below overflows, and
    wrapping once in front of the shift is wrapping everywhere -- the integers modulo 2^32 are a ring)."""
    v = v.astype(np.int64)
    v0, v1, v2, v3, v4, v5, v6, v7 = (v[..., k] for k in range(8))
    z1 = (v2 + v6) * 4433; t2 = z1 - v6 * 15137; t3 = z1 + v2 * 6270
    t0 = (v0 + v4) << 13; t1 = (v0 - v4) << 13
    t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2
    a, b, c, d = v7, v5, v3, v1
    z1 = a + d; z2 = b + c; z3 = a + c; z4 = b + d; z5 = (z3 + z4) * 9633
    a = a * 2446; b = b * 16819; c = c * 25172; d = d * 12299
    z1 = z1 * -7373; z2 = z2 * -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5
    a = a + z1 + z3; b = b + z2 + z4; c = c + z2 + z3; d = d + z1 + z4
    out = [t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d]
    return np.stack([_wrap32(_wrap32(o) + (1 << (shift - 1))) >> shift for o in out], -1)


def idct(blocks, wrong=None):
    """[..., 8 rows, 8 columns] dequantised coefficients -> [..., 8, 8] results before the + 128 and the clamp (32-bit values)."""
    b = np.asarray(blocks).astype(np.int64)
    if wrong == "rows_first":
        return _step(_step(b, 11).swapaxes(-1, -2), 18).swapaxes(-1, -2)
    ws = _step(b.swapaxes(-1, -2), 11).swapaxes(-1, -2)              # pass 1: along the columns
    return _step(ws, 18)                                             # pass 2: along the rows


def _shift(p, axis, by):
    """p[.. i + by ..] with the index clamped to the plane."""
    n = p.shape[axis]
    return np.take(p, np.clip(np.arange(n) + by, 0, n - 1), axis=axis)


def upsample(p, eh, ev, wrong=None):
    """A chroma plane of dh x dw real samples (or, under 'pad_neighbours', the whole padded plane) -> ev dh x eh dw."""
    p = p.astype(np.int64)
    dh, dw = p.shape
    if (eh, ev) == (1, 1):
        return p
    assert eh == 2 and ev in (1, 2), (eh, ev)
    if dw <= 2 and wrong != "interp_small":
        return np.repeat(np.repeat(p, ev, 0), 2, 1)
    out = np.zeros((dh * ev, dw * 2), np.int64)
    if ev == 1:
        be, bo = (2, 1) if wrong == "bias_swapped" else (1, 2)
        out[:, 0::2] = (3 * p + _shift(p, 1, -1) + be) >> 2
        out[:, 1::2] = (3 * p + _shift(p, 1, 1) + bo) >> 2
        return out
    s = np.zeros((dh * 2, dw), np.int64)
    s[0::2] = 3 * p + _shift(p, 0, -1)
    s[1::2] = 3 * p + _shift(p, 0, 1)
    be, bo = (7, 8) if wrong == "bias_swapped" else (8, 7)
    out[:, 0::2] = (3 * s + _shift(s, 1, -1) + be) >> 4
    out[:, 1::2] = (3 * s + _shift(s, 1, 1) + bo) >> 4
    return out


def render(arena, width, height, hv, wrong=None):
    """arena [blocks][64] int16 (slot 0 = cumulative DC) -> (pixels [height][width][3] uint8, R G B; the largest |result| of the IDCT)."""
    hv = [tuple(int(x) for x in c) for c in hv]
    assert renderable(hv), hv
    arena = np.asarray(arena); assert arena.dtype == np.int16 and arena.ndim == 2 and arena.shape[1] == 64, (arena.dtype, arena.shape)
    hmax = max(h for h, _ in hv); vmax = max(v for _, v in hv)
    geo = CM.Geometry(hv, -(-width // (8 * hmax)), -(-height // (8 * vmax)))
    assert arena.shape[0] == geo.nblocks, (arena.shape, geo.nblocks)
    planes = []; peak = 0
    for c, (h, v) in enumerate(hv):
        bw, bh = geo.grid(c)
        res = idct(arena[geo.arena_index(c)].reshape(bh, bw, 8, 8), wrong)
        peak = max(peak, int(np.abs(res).max()))
        full = np.clip(res + 128, 0, 255).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        dw, dh = -(-width * h // hmax), -(-height * v // vmax)
        p = full if wrong == "pad_neighbours" else full[:dh, :dw]
        planes.append(upsample(p, hmax // h, vmax // v, wrong)[:height, :width])
    y = planes[0]
    if len(hv) == 1:
        return np.stack([y, y, y], -1).astype(np.uint8), peak
    cb = planes[1] - 128; cr = planes[2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    if wrong == "g_separate":
        g = y + ((-22554 * cb + 32768) >> 16) + ((-46802 * cr + 32768) >> 16)
    else:
        g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8), peak


def arena_of_file(data):
    """(arena with the DC in slot 0, width, height, hv) of a file prog_codec.decode reads: what a clean decode leaves, read as pack_coefs reads it."""
    import prog_codec as PC
    d = PC.decode(data)
    return PC.arena(d.frame, d.coefs, clear_dc=False), d.frame.width, d.frame.height, d.frame.hv
