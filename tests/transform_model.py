"""The definition of jsnoop_transform_run -- TEST INFRASTRUCTURE and the authority the kernel is compared with, value for value.

Input is what the library holds for one image after a decode: the coefficient arena [blocks][64] (int16, natural order inside a row, decode order: MCU
after MCU, the components interleaved inside the MCU), the cumulative DC of every block (dccum), the geometry (coef_model.Geometry), the SOF
dimensions and the multipliers per component (natural order).  Output is a Result: the result word and, where it is OK, the same five things of the
transformed picture plus the region of the source that was kept.

Plain numpy on the block grid of one component at a time; nothing of the kernel's structure (no MCU table, no prefix table, no divisions by magic).
Per entry, in this order, all in source coordinates; the source MCU is mw = 8 Hmax by mh = 8 Vmax:
  1. grayscale: a three-component source keeps component 0 alone, as a one-component 1 x 1 picture of ceil(W / 8) x ceil(H / 8) blocks; mw = mh = 8.
  2. crop (jpegtran's rule): x0 = crop_x - crop_x % mw, the width grows by what the offset lost and is clipped to the picture; y alike.  A rectangle
     that starts outside the picture: EMPTY.
  3. edge: an op that reverses the source's x axis needs the width to be a multiple of mw, one that reverses y the height a multiple of mh.  TRIM
     cuts the dimension down to whole MCUs from the origin (nothing left: EMPTY); PERFECT makes the entry IMPERFECT.
  4. blocks: S is component c's block grid over the region, BW x BH blocks -- the region's MCUs times H_c / V_c, whole MCUs on a reversed axis, the
     MCU-padded count otherwise (padding blocks as the source holds them).  D comes from S by the table in `_turn`.  Negation is int16 modulo 2^16;
     cell 0 and dccum move with their block and never change sign; no cell is interpreted.
  5. descriptor: the transposing ops swap width and height, H_c and V_c, and transpose every table; the arena is in decode order of the NEW geometry."""
import numpy as np

import coef_model as CM

NONE, FLIP_H, FLIP_V, TRANSPOSE, TRANSVERSE, ROT_90, ROT_180, ROT_270 = range(8)      # libjpeg's JXFORM codes; ROT_90 is clockwise
OPS = {"none": NONE, "flip_h": FLIP_H, "flip_v": FLIP_V, "transpose": TRANSPOSE, "transverse": TRANSVERSE, "rot90": ROT_90, "rot180": ROT_180, "rot270": ROT_270}
TRIM, PERFECT = 0, 1
OK, IMPERFECT, EMPTY, UNSUPPORTED = 0, 1, 2, 3
REVERSES_X = (FLIP_H, ROT_180, TRANSVERSE, ROT_270)
REVERSES_Y = (FLIP_V, ROT_180, TRANSVERSE, ROT_90)
TRANSPOSING = (TRANSPOSE, TRANSVERSE, ROT_90, ROT_270)


class Result:
    def __init__(self, result, arena=None, dccum=None, geo=None, dim_x=0, dim_y=0, qnat=None, region=None):
        self.result, self.arena, self.dccum, self.geo, self.dim_x, self.dim_y, self.qnat, self.region = result, arena, dccum, geo, dim_x, dim_y, qnat, region


def _turn(S, op):
    """S [BH][BW][8][8] (cell [v][u]) in int64 -> D, the table of the contract:
         NONE        S[by][bx][v][u]                      TRANSPOSE   S[bx][by][u][v]
         FLIP_H      (-1)^u S[by][BW-1-bx][v][u]          ROT_90      (-1)^u S[BH-1-bx][by][u][v]
         FLIP_V      (-1)^v S[BH-1-by][bx][v][u]          ROT_270     (-1)^v S[bx][BW-1-by][u][v]
         ROT_180     (-1)^(u+v) S[BH-1-by][BW-1-bx][v][u] TRANSVERSE  (-1)^(u+v) S[BH-1-bx][BW-1-by][u][v]"""
    su = np.array([1, -1] * 4).reshape(1, 1, 1, 8); sv = su.reshape(1, 1, 8, 1)
    t = lambda A: A.transpose(1, 0, 3, 2)                            # D[by][bx][v][u] = A[bx][by][u][v]
    return {NONE: lambda: S, FLIP_H: lambda: su * S[:, ::-1], FLIP_V: lambda: sv * S[::-1], ROT_180: lambda: su * sv * S[::-1, ::-1],
            TRANSPOSE: lambda: t(S), ROT_90: lambda: su * t(S[::-1]), ROT_270: lambda: sv * t(S[:, ::-1]), TRANSVERSE: lambda: su * sv * t(S[::-1, ::-1])}[op]()


def _move(C, op):
    """The block permutation of `_turn` alone, for one value per block (dccum)."""
    t = lambda A: A.transpose(1, 0)
    return {NONE: lambda: C, FLIP_H: lambda: C[:, ::-1], FLIP_V: lambda: C[::-1], ROT_180: lambda: C[::-1, ::-1],
            TRANSPOSE: lambda: t(C), ROT_90: lambda: t(C[::-1]), ROT_270: lambda: t(C[:, ::-1]), TRANSVERSE: lambda: t(C[::-1, ::-1])}[op]()


def region(dim_x, dim_y, mw, mh, op, edge=TRIM, crop=None):
    """Steps 2 and 3 -> (result, (x0, y0, w, h)): what is kept of a dim_x x dim_y picture whose MCU is mw x mh.  crop = (x, y, w, h) or None."""
    x0, y0, w, h = 0, 0, dim_x, dim_y
    if crop is not None:
        cx, cy, cw, ch = crop
        if cx >= dim_x or cy >= dim_y:
            return EMPTY, None
        x0 = cx - cx % mw; y0 = cy - cy % mh
        w = min(cw + (cx - x0), dim_x - x0); h = min(ch + (cy - y0), dim_y - y0)
    bad_x = op in REVERSES_X and w % mw != 0; bad_y = op in REVERSES_Y and h % mh != 0
    if bad_x or bad_y:
        if edge == PERFECT:
            return IMPERFECT, None
        if op in REVERSES_X:
            w -= w % mw
        if op in REVERSES_Y:
            h -= h % mh
        if w == 0 or h == 0:
            return EMPTY, None
    return OK, (x0, y0, w, h)


def transform(arena, dccum, geo, dim_x, dim_y, qnat, op, edge=TRIM, grayscale=False, crop=None):
    arena = np.asarray(arena); dccum = np.asarray(dccum)
    if geo.ncomp not in (1, 3):
        return Result(UNSUPPORTED)
    assert arena.shape == (geo.nblocks, 64) and dccum.shape == (geo.nblocks,) and arena.dtype == np.int16 and dccum.dtype == np.int16
    hv = [(1, 1)] if (grayscale or geo.ncomp == 1) else list(geo.hv)       # 1. the layout the entry works in
    hmax = max(h for h, _ in hv); vmax = max(v for _, v in hv); mw, mh = 8 * hmax, 8 * vmax
    res, reg = region(dim_x, dim_y, mw, mh, op, edge, crop)                # 2., 3.
    if res != OK:
        return Result(res)
    x0, y0, w, h = reg
    mx = w // mw if op in REVERSES_X else -(-w // mw); my = h // mh if op in REVERSES_Y else -(-h // mh)
    turned = op in TRANSPOSING
    out_geo = CM.Geometry([(v, h_) for h_, v in hv] if turned else hv, my if turned else mx, mx if turned else my)
    out_arena = np.zeros((out_geo.nblocks, 64), np.int16); out_cum = np.zeros(out_geo.nblocks, np.int16); filled = np.zeros(out_geo.nblocks, bool)
    for c, (H, V) in enumerate(hv):                                        # 4.
        at = geo.arena_index(c)                                            # [bh][bw] of the SOURCE's grid of component c
        ox, oy, BW, BH = x0 // mw * H, y0 // mh * V, mx * H, my * V
        S = arena[at[oy:oy + BH, ox:ox + BW]].reshape(BH, BW, 8, 8).astype(np.int64)
        assert S.shape[:2] == (BH, BW), "the region lies inside the source's grid"
        D = _turn(S, op); Cm = _move(dccum[at[oy:oy + BH, ox:ox + BW]], op)
        to = out_geo.arena_index(c)
        assert to.shape == D.shape[:2]
        out_arena[to] = (D.reshape(D.shape[0], D.shape[1], 64) & 0xFFFF).astype(np.uint16).view(np.int16)
        out_cum[to] = Cm; filled[to] = True
    assert filled.all()
    q = [np.asarray(qnat[c]).reshape(8, 8) for c in range(len(hv))]        # 5.
    out_q = [[int(x) for x in (t.T if turned else t).reshape(64)] for t in q]
    return Result(OK, out_arena, out_cum, out_geo, h if turned else w, w if turned else h, out_q, reg)
