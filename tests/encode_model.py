"""The definition of jsnoop_encode_run -- TEST INFRASTRUCTURE and the authority k_encode is compared with, value for value.

Pixels (8-bit, grey or R, G, B) to what jsnoop_batch_export_jpeg reads: the coefficient arena [blocks][64] (int16, natural order, decode order, slot 0
zero) and dccum[blocks] (the DC level times q[0]).  The arithmetic is libjpeg's integer path, written from DESIGN.md section 4.18 in plain numpy -- whole
planes at a time, no units, no tiles, nothing of the kernel's structure:

  1. colour      Y  = (19595 R + 38470 G +  7471 B + 32768) >> 16
                 Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
                 Cr = (32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16          (arithmetic shifts; a grey source is Y itself)
  2. every plane is extended to the MCU-padded width by replicating its last source column (before downsampling)
  3. source rows are replicated to a multiple of Vmax, and no further
  4. downsampling, the bias by OUTPUT column x:  2x2: (a + b + c + d + (1, 2, 1, 2 ..)) >> 2;  2x1: (a + b + (0, 1, 0, 1 ..)) >> 1
  5. every component's last sample row is replicated to its MCU-padded height
  6. level shift -128, then jfdctint ("islow", CONST_BITS 13, PASS1_BITS 2): rows, then columns; results are 8 x the coefficient
  7. level = sign(c) * ((|c| + 4 q) // (8 q))
  8. a block of the MCU-padded grid outside the component's coded part (prog_codec.Frame.coded) is a dummy block: AC levels 0, DC level that of the
     block before it in its MCU's own block order (the rule chains; such a block always has a predecessor in its MCU)

Tables are natural order, 1..255; from quality 1..100: scale = 5000 // q below 50, else 200 - 2 q; v = clamp((base * scale + 50) // 100, 1, 255) over
T.81 Tables K.1 / K.2.  With q <= 255 no int16 product wraps: |c| <= 8 * 1024 + 8, so |level * q| <= (|c| + 4 q) / 8 < 1154.

`wrong` names one deliberately WRONG reading of the text above (tests/test_encode_model.py shows that a named case refuses each):
'rows_to_mcu' (source rows replicated down to the MCU edge before downsampling), 'const_bias' (bias 2 / 1 in every column), 'chroma_offset' (the
chroma offset without its - 1: + 32768 in place of + 32767), 'dummy_dc0' (a dummy block's DC level is 0), 'trunc_div' (level = c / (8 q), truncating)."""
import numpy as np

import coef_model as CM

SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2, 0: 0, 1: 1, 2: 2}
_HV = {0: [(1, 1), (1, 1), (1, 1)], 1: [(2, 1), (1, 1), (1, 1)], 2: [(2, 2), (1, 1), (1, 1)]}

# ITU-T T.81 Annex K, Tables K.1 and K.2, as printed (row by row: natural order)
K1 = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K2 = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def quality_tables(quality):
    """-> (luma[64], chroma[64]), natural order."""
    q = int(quality); assert 1 <= q <= 100, q
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((b * scale + 50) // 100, 1), 255) for b in base] for base in (K1, K2))


def hv_of(channels, subsampling):
    return [(1, 1)] if channels == 1 else _HV[SUBSAMPLING[subsampling]]


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, first):
    """One 1-D pass of jfdctint along the last axis."""
    d = d.astype(np.int64)
    t0 = d[..., 0] + d[..., 7]; t7 = d[..., 0] - d[..., 7]; t1 = d[..., 1] + d[..., 6]; t6 = d[..., 1] - d[..., 6]
    t2 = d[..., 2] + d[..., 5]; t5 = d[..., 2] - d[..., 5]; t3 = d[..., 3] + d[..., 4]; t4 = d[..., 3] - d[..., 4]
    t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2
    o = [None] * 8
    if first:
        o[0] = (t10 + t11) << 2; o[4] = (t10 - t11) << 2; n = 11
    else:
        o[0] = _descale(t10 + t11, 2); o[4] = _descale(t10 - t11, 2); n = 15
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n); o[6] = _descale(z1 - t12 * 15137, n)
    z1 = t4 + t7; z2 = t5 + t6; z3 = t4 + t6; z4 = t5 + t7; z5 = (z3 + z4) * 9633
    t4 = t4 * 2446; t5 = t5 * 16819; t6 = t6 * 25172; t7 = t7 * 12299
    z1 = z1 * -7373; z2 = z2 * -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5
    o[7] = _descale(t4 + z1 + z3, n); o[5] = _descale(t5 + z2 + z4, n); o[3] = _descale(t6 + z2 + z3, n); o[1] = _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct(blocks):
    """[..., 8 rows, 8 columns] level-shifted samples -> [..., 8, 8], 8 x the coefficients."""
    a = _pass(blocks, True)
    return _pass(a.swapaxes(-1, -2), False).swapaxes(-1, -2)


def pass1_max():
    """The largest |value| pass 1 can leave, over every row of samples -128 .. 127 (the pass is linear up to its rounding: the corners decide)."""
    rows = np.array([[127 if k >> i & 1 else -128 for i in range(8)] for k in range(256)])
    return int(np.abs(_pass(rows, True)).max())


def component_planes(pixels, subsampling, wrong=None):
    """pixels [H][W] or [H][W][3] (R, G, B) uint8 -> (hv, mcu_x, mcu_y, [per component: samples of its MCU-padded grid, int64])."""
    pixels = np.asarray(pixels); assert pixels.dtype == np.uint8 and pixels.ndim in (2, 3), (pixels.dtype, pixels.shape)
    H, W = pixels.shape[:2]
    if pixels.ndim == 2:
        src = [pixels.astype(np.int64)]
    else:
        assert pixels.shape[2] == 3
        r, g, b = (pixels[..., i].astype(np.int64) for i in range(3))
        off = 8388608 + (32768 if wrong == "chroma_offset" else 32767)
        src = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16, (-11059 * r - 21709 * g + 32768 * b + off) >> 16, (32768 * r - 27439 * g - 5329 * b + off) >> 16]
    hv = hv_of(len(src), subsampling)
    hmax = max(h for h, _ in hv); vmax = max(v for _, v in hv)
    mcu_x = -(-W // (8 * hmax)); mcu_y = -(-H // (8 * vmax))
    out = []
    for p, (h, v) in zip(src, hv):
        rows = mcu_y * 8 * vmax if wrong == "rows_to_mcu" else -(-H // vmax) * vmax
        p = np.pad(p, ((0, rows - H), (0, mcu_x * 8 * hmax - W)), mode="edge")
        eh, ev = hmax // h, vmax // v
        if (eh, ev) == (2, 2):
            s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
            bias = np.full(s.shape[1], 2) if wrong == "const_bias" else 1 + (np.arange(s.shape[1]) & 1)
            p = (s + bias) >> 2
        elif (eh, ev) == (2, 1):
            s = p[:, 0::2] + p[:, 1::2]
            bias = np.full(s.shape[1], 1) if wrong == "const_bias" else np.arange(s.shape[1]) & 1
            p = (s + bias) >> 1
        else:
            assert (eh, ev) == (1, 1)
        out.append(np.pad(p, ((0, mcu_y * 8 * v - p.shape[0]), (0, 0)), mode="edge"))
    return hv, mcu_x, mcu_y, out


def levels(pixels, subsampling, qtables, wrong=None):
    """-> (hv, mcu_x, mcu_y, [per component: quantised levels [grid_y][grid_x][64], natural order, int64]).  qtables = (luma64, chroma64)."""
    hv, mcu_x, mcu_y, planes = component_planes(pixels, subsampling, wrong)
    H, W = np.asarray(pixels).shape[:2]
    hmax = max(h for h, _ in hv); vmax = max(v for _, v in hv)
    out = []
    for c, (p, (h, v)) in enumerate(zip(planes, hv)):
        nby, nbx = p.shape[0] // 8, p.shape[1] // 8
        co = fdct(p.reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3) - 128).reshape(nby, nbx, 64)
        q = np.asarray(qtables[0 if c == 0 else 1], np.int64); assert q.shape == (64,) and q.min() >= 1 and q.max() <= 255
        if wrong == "trunc_div":
            lev = np.sign(co) * (np.abs(co) // (8 * q))
        else:
            lev = np.sign(co) * ((np.abs(co) + 4 * q) // (8 * q))
        cy, cx = -(-(-(-H * v // vmax)) // 8), -(-(-(-W * h // hmax)) // 8)         # the coded part (Frame.coded)
        for my in range(mcu_y):
            for mx in range(mcu_x):
                prev = None
                for vv in range(v):
                    for hh in range(h):
                        by, bx = my * v + vv, mx * h + hh
                        if by >= cy or bx >= cx:
                            assert prev is not None
                            lev[by, bx, 1:] = 0; lev[by, bx, 0] = 0 if wrong == "dummy_dc0" else prev
                        prev = lev[by, bx, 0]
        out.append(lev)
    return hv, mcu_x, mcu_y, out


def encode(pixels, subsampling, qtables, wrong=None):
    """What jsnoop_encode_run leaves for one image: (arena [blocks][64] int16, dccum [blocks] int16, coef_model.Geometry, qnat per component)."""
    hv, mcu_x, mcu_y, lev = levels(pixels, subsampling, qtables, wrong)
    geo = CM.Geometry(hv, mcu_x, mcu_y)
    arena = np.zeros((geo.nblocks, 64), np.int64); dccum = np.zeros(geo.nblocks, np.int64)
    qnat = [[int(x) for x in qtables[0 if c == 0 else 1]] for c in range(len(hv))]
    for c in range(len(hv)):
        idx = geo.arena_index(c); prod = lev[c] * np.asarray(qnat[c], np.int64)
        arena[idx] = prod; dccum[idx] = prod[..., 0]
    arena[:, 0] = 0
    assert np.abs(arena).max(initial=0) < 1154 and np.abs(dccum).max(initial=0) < 1154, "an int16 product beyond the bound of the contract"
    return arena.astype(np.int16), dccum.astype(np.int16), geo, qnat
