"""CPU: tests/transform_model.py -- the definition of jsnoop_transform_run -- pinned by a derivation that shares none of its index rules.

1. The float64 IDCT identity: the samples of the model's output (orthonormal IDCT of every block, transform_cases.planes) equal numpy's own flip /
   rot90 / transpose of the source's samples over the cropped and trimmed region, to 1e-6 -- derived, not measured: 64 products below 2^15 in float64
   carry an error below 1e-9, and 1e-6 is far below one level.  Sources are coefficient noise with every cell occupied under tables that are not
   symmetric.  8 ops x 6 layouts x 5 sizes x both edge modes x crops on and off the MCU grid x grayscale.
2. Algebra on whole-MCU pictures.  3. Through the export model and prog_codec / Pillow.  4. Edge and result words.  5. Five wrong readings, each
   refused by a named case."""
import io

import numpy as np
import pytest

import coef_model as CM
import export_model as EM
import prog_codec as PC
import transform_cases as TC
import transform_model as M

ALL_OPS = sorted(M.OPS.values())
TOL = 1e-6


def second_region(W, H, mw, mh, op, edge, crop):
    """Steps 2 and 3 of the contract once more, in pixels and in other words: (result, x0, y0, w, h)."""
    xs, ys = (0, W), (0, H)
    if crop is not None:
        if crop[0] >= W or crop[1] >= H:
            return (M.EMPTY,)
        xs = (crop[0] // mw * mw, min(W, crop[0] + crop[2])); ys = (crop[1] // mh * mh, min(H, crop[1] + crop[3]))
    w, h = xs[1] - xs[0], ys[1] - ys[0]
    cut_x = op in M.REVERSES_X and w % mw; cut_y = op in M.REVERSES_Y and h % mh
    if (cut_x or cut_y) and edge == M.PERFECT:
        return (M.IMPERFECT,)
    w -= cut_x; h -= cut_y
    if w <= 0 or h <= 0:
        return (M.EMPTY,)
    return M.OK, xs[0], ys[0], w, h


def identity_error(src, src_planes, R, op, x0, y0, grayscale):
    """Largest |difference| between the samples of the model's output and numpy's op over the source's samples of the region (padding blocks included)."""
    _a, _d, geo, _W, _H, _q = src
    hv = [(1, 1)] if (grayscale or geo.ncomp == 1) else geo.hv
    hmax = max(a for a, _ in hv); vmax = max(b for _, b in hv)
    worst = 0.0
    for c, (Hc, Vc) in enumerate(hv):
        P = TC.planes(R.arena, R.dccum, R.geo, c)
        hh, ww = P.shape[::-1] if op in M.TRANSPOSING else P.shape
        px, py = x0 * Hc // hmax, y0 * Vc // vmax
        S = src_planes[c][py:py + hh, px:px + ww]
        if S.shape != (hh, ww):
            return float("inf")
        worst = max(worst, float(np.abs(TC.numpy_op(S, op) - P).max()))
    return worst


def check(src, src_planes, op, edge, grayscale, crop):
    arena, dccum, geo, W, H, qnat = src
    gray = grayscale and geo.ncomp == 3
    hv = [(1, 1)] if (gray or geo.ncomp == 1) else geo.hv
    mw = 8 * max(a for a, _ in hv); mh = 8 * max(b for _, b in hv)
    want = second_region(W, H, mw, mh, op, edge, crop)
    R = M.transform(arena, dccum, geo, W, H, qnat, op, edge, grayscale, crop)
    what = (geo.hv, W, H, op, edge, grayscale, crop)
    assert R.result == want[0], what
    if R.result != M.OK:
        assert R.arena is None
        return R
    _ok, x0, y0, w, h = want
    turned = op in M.TRANSPOSING
    assert R.region == (x0, y0, w, h) and (R.dim_x, R.dim_y) == ((h, w) if turned else (w, h)), what
    assert R.geo.ncomp == len(hv) and R.geo.hv == ([(b, a) for a, b in hv] if turned else list(hv)), what
    omw = 8 * R.geo.hmax; omh = 8 * R.geo.vmax
    assert (R.geo.mcu_x, R.geo.mcu_y) == (-(-R.dim_x // omw), -(-R.dim_y // omh)), what       # the decode geometry of the declared size
    assert R.qnat == [list(np.array(qnat[c]).reshape(8, 8).T.reshape(64)) if turned else list(qnat[c]) for c in range(len(hv))], what
    err = identity_error(src, src_planes, R, op, x0, y0, gray)
    assert err < TOL, (what, err)
    return R


def sources(layout, sizes=TC.SIZES):
    out = []
    for k, (w, h) in enumerate(sizes):
        s = TC.noise(layout, w, h, 100 * k + len(layout))
        out.append((s, [TC.planes(s[0], s[1], s[2], c) for c in range(s[2].ncomp)]))
    return out


# ------------------------------------------------------------------------------------------------------------------ 1: the IDCT identity
@pytest.mark.parametrize("layout", list(TC.LAYOUTS))
def test_idct_identity_every_op_size_edge_and_grayscale(layout):
    n = 0
    for src, pl in sources(layout):
        for op in ALL_OPS:
            for edge in (M.TRIM, M.PERFECT):
                for gray in ((False, True) if layout != "grey" else (False,)):
                    n += check(src, pl, op, edge, gray, None).result == M.OK
    assert n >= 40                                                    # (most of the sweep is written, not refused)


@pytest.mark.parametrize("layout", list(TC.LAYOUTS))
def test_idct_identity_under_crops_on_and_off_the_mcu_grid(layout):
    n = 0
    for src, pl in sources(layout, [(48, 32), (50, 70)]):
        for op in ALL_OPS:
            for crop in TC.CROPS[1:]:
                for edge, gray in ((M.TRIM, False), (M.PERFECT, False), (M.TRIM, layout != "grey")):
                    n += check(src, pl, op, edge, gray, crop).result == M.OK
    assert n >= 100


# ------------------------------------------------------------------------------------------------------------------ 2: algebra
def again(R, op, **kw):
    return M.transform(R.arena, R.dccum, R.geo, R.dim_x, R.dim_y, R.qnat, op, **kw)


def same(A, B):
    return (np.array_equal(A.arena, B.arena) and np.array_equal(A.dccum, B.dccum) and A.qnat == B.qnat and A.geo.hv == B.geo.hv
            and (A.geo.mcu_x, A.geo.mcu_y, A.dim_x, A.dim_y) == (B.geo.mcu_x, B.geo.mcu_y, B.dim_x, B.dim_y))


@pytest.mark.parametrize("layout", list(TC.LAYOUTS))
def test_algebra_on_whole_mcu_pictures(layout):
    hv = TC.LAYOUTS[layout]; m = 8 * max(max(a, b) for a, b in hv)
    arena, dccum, geo, W, H, qnat = TC.noise(layout, 3 * m, 2 * m, 7)
    I = M.transform(arena, dccum, geo, W, H, qnat, M.NONE)
    assert np.array_equal(I.arena, arena) and np.array_equal(I.dccum, dccum) and I.qnat == qnat and (I.dim_x, I.dim_y) == (W, H)
    assert same(again(again(I, M.FLIP_H), M.FLIP_H), I)
    assert same(again(again(I, M.TRANSPOSE), M.TRANSPOSE), I)
    assert same(again(again(again(again(I, M.ROT_90), M.ROT_90), M.ROT_90), M.ROT_90), I)
    assert same(again(again(I, M.ROT_270), M.ROT_90), I) and same(again(again(I, M.ROT_90), M.ROT_270), I)
    assert same(again(I, M.ROT_90), again(again(I, M.TRANSPOSE), M.FLIP_H))
    assert same(again(again(I, M.ROT_90), M.ROT_90), again(I, M.ROT_180)) and same(again(again(I, M.FLIP_H), M.FLIP_V), again(I, M.ROT_180))
    assert same(again(I, M.TRANSVERSE), again(again(I, M.ROT_180), M.TRANSPOSE))
    assert not same(again(I, M.FLIP_H), I) and not same(again(I, M.ROT_90), again(I, M.ROT_270))


# ------------------------------------------------------------------------------------------------------------------ 3: through the export
@pytest.mark.parametrize("layout,op", [("grey", M.ROT_90), ("4:4:4", M.FLIP_H), ("4:2:2", M.TRANSPOSE), ("4:4:0", M.ROT_270), ("4:2:0", M.TRANSVERSE), ("4:1:1", M.ROT_90),
                                       ("4:2:0", M.ROT_180), ("4:2:2", M.FLIP_V)])
def test_the_exported_file_decodes_to_the_models_coefficients(layout, op):
    arena, dccum, geo, W, H, qnat = TC.noise(layout, 50, 70, 11)
    R = M.transform(arena, dccum, geo, W, H, qnat, op)
    assert R.result == M.OK
    res, _det, f = EM.export_file(R.arena, R.dccum, R.geo, R.dim_x, R.dim_y, R.qnat)
    assert res == EM.OK
    D = PC.decode(f)
    assert (D.frame.width, D.frame.height, D.frame.hv) == (R.dim_x, R.dim_y, R.geo.hv)
    want = TC.levels_of(R.arena, R.dccum, R.geo, R.qnat)
    for c in range(R.geo.ncomp):
        assert np.array_equal(D.coefs[c], want[c]), c
        qz = D.frame.qtabs[D.frame.comps[c][2]]                        # the DQT in the file, zig-zag order
        assert [qz[z] for z in range(64)] == [R.qnat[c][PC.ZIGZAG[z]] for z in range(64)]
        if op in M.TRANSPOSING:
            assert [qz[z] for z in range(64)] != [qnat[c][PC.ZIGZAG[z]] for z in range(64)]
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(f)); im.load()
    assert im.size == (R.dim_x, R.dim_y) and im.mode == ("L" if R.geo.ncomp == 1 else "RGB")


# ------------------------------------------------------------------------------------------------------------------ 4: edge and result words
def test_edge_modes_and_result_words():
    a = TC.noise("4:2:0", 15, 40, 3)
    assert M.transform(*a, M.FLIP_H, edge=M.TRIM).result == M.EMPTY                       # 15 wide is below one MCU of 16
    assert M.transform(*a, M.FLIP_H, edge=M.PERFECT).result == M.IMPERFECT
    R = M.transform(*a, M.FLIP_V)                                                           # y alone is reversed: 40 -> 32, x keeps its partial MCU
    assert R.result == M.OK and (R.dim_x, R.dim_y, R.geo.mcu_x, R.geo.mcu_y) == (15, 32, 1, 2)
    b = TC.noise("4:2:0", 17, 9, 4)
    assert M.transform(*b, M.ROT_180).result == M.EMPTY                                    # x trims to 16, y (9 < 16) to nothing
    assert M.transform(*b, M.FLIP_H).region == (0, 0, 16, 9) and M.transform(*b, M.NONE).region == (0, 0, 17, 9)
    assert M.transform(*b, M.ROT_180, grayscale=True).region == (0, 0, 16, 8)              # grey: the MCU is 8 x 8
    assert M.transform(*b, M.TRANSPOSE, edge=M.PERFECT).result == M.OK                     # nothing reversed, nothing to trim
    assert M.transform(*b, M.NONE, crop=(17, 0, 1, 1)).result == M.EMPTY and M.transform(*b, M.NONE, crop=(0, 9, 1, 1)).result == M.EMPTY
    assert M.transform(*b, M.NONE, crop=(16, 8, 1, 1)).region == (16, 0, 1, 9)
    two = CM.Geometry([(1, 1), (1, 1)], 1, 1)
    assert M.transform(np.zeros((2, 64), np.int16), np.zeros(2, np.int16), two, 8, 8, [[1] * 64] * 2, M.NONE).result == M.UNSUPPORTED


def test_minus_32768_stays_and_cell_0_and_dccum_keep_their_sign():
    arena, dccum, geo, W, H, qnat = TC.noise("grey", 16, 8, 5)
    arena = arena.copy(); dccum = dccum.copy()
    arena[0, 1] = -32768; arena[0, 9] = -32768; arena[1, 0] = -32768; arena[1, 8] = 32767; dccum[0] = -32768; dccum[1] = -5
    for op in ALL_OPS:
        R = M.transform(arena, dccum, geo, W, H, qnat, op)
        to = {M.NONE: (0, 1), M.FLIP_V: (0, 1), M.FLIP_H: (1, 0), M.ROT_180: (1, 0)}.get(op)
        if to is None:                                                # transposing: 2 x 1 blocks become 1 x 2, block order by rows
            to = (0, 1) if op in (M.TRANSPOSE, M.ROT_90) else (1, 0)
        b0, b1 = to
        assert R.dccum[b0] == -32768 and R.dccum[b1] == -5 and R.arena[b1, 0] == -32768, op
        n1, n9 = ((8, 9) if op in M.TRANSPOSING else (1, 9))
        assert R.arena[b0, n1] == -32768 and R.arena[b0, n9] == -32768, op
        n8 = 1 if op in M.TRANSPOSING else 8
        assert abs(int(R.arena[b1, n8])) == 32767, op


# ------------------------------------------------------------------------------------------------------------------ 5: wrong readings
def _setup(layout, w, h, op, **kw):
    src = TC.noise(layout, w, h, 21)
    pl = [TC.planes(src[0], src[1], src[2], c) for c in range(src[2].ncomp)]
    R = M.transform(*src, op, **kw)
    assert R.result == M.OK
    return src, pl, R


def test_wrong_reading_signs_by_v_for_flip_h():
    src, pl, R = _setup("4:4:4", 16, 16, M.FLIP_H)
    assert identity_error(src, pl, R, M.FLIP_H, 0, 0, False) < TOL
    sv = np.repeat(np.array([1, -1] * 4), 8)                          # (-1)^v over natural index 8 v + u
    W = M.Result(M.OK, (R.arena * (np.array([1, -1] * 32) * sv)).astype(np.int16), R.dccum, R.geo, R.dim_x, R.dim_y, R.qnat, R.region)   # u-signs undone, v-signs applied
    assert identity_error(src, pl, W, M.FLIP_H, 0, 0, False) > 1.0


def test_wrong_reading_table_left_untransposed():
    src, _pl, R = _setup("4:2:0", 32, 32, M.ROT_90)
    assert EM.levels(R.arena, R.dccum, R.geo, R.qnat)[1] == EM.OK
    assert EM.levels(R.arena, R.dccum, R.geo, src[5])[1] == EM.INEXACT          # level * q no longer divides by the source's own table


def test_wrong_reading_h_and_v_left_unswapped():
    src, pl, R = _setup("4:2:2", 32, 16, M.TRANSPOSE)
    assert R.geo.hv == [(1, 2), (1, 1), (1, 1)] and (R.geo.mcu_x, R.geo.mcu_y) == (2, 2) and identity_error(src, pl, R, M.TRANSPOSE, 0, 0, False) < TOL
    W = M.Result(M.OK, R.arena, R.dccum, CM.Geometry(src[2].hv, 2, 2), R.dim_x, R.dim_y, R.qnat, R.region)
    assert identity_error(src, pl, W, M.TRANSPOSE, 0, 0, False) > 1.0


def test_wrong_reading_trim_taken_from_the_far_side():
    src, pl, R = _setup("4:4:4", 20, 8, M.FLIP_H)
    assert R.region == (0, 0, 16, 8) and identity_error(src, pl, R, M.FLIP_H, 0, 0, False) < TOL
    assert identity_error(src, pl, R, M.FLIP_H, 8, 0, False) > 1.0   # not the last two block columns


def test_wrong_reading_crop_offset_rounded_up():
    src, pl, R = _setup("4:2:0", 64, 48, M.NONE, crop=(5, 19, 20, 10))
    assert R.region == (0, 16, 25, 13) and identity_error(src, pl, R, M.NONE, 0, 16, False) < TOL
    assert identity_error(src, pl, R, M.NONE, 16, 32, False) > 1.0
