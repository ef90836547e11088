"""CPU: tests/encode_model.py -- the definition k_encode is compared with -- against Pillow (libjpeg-turbo's integer path), exactly.

Pillow encodes the same pixels; prog_codec.decode reads its quantised levels and its DQT.  Every block of the coded part must equal the model's
coefficient for coefficient, every padding block must obey the dummy-block rule, the tables a quality comes to must be Pillow's for every quality,
the entropy-coded segment of the model's arena written by export_model must be Pillow's, the extreme pictures must stay codable, and five wrong
readings of the contract must each be refused by a named case."""
import io

import numpy as np
import pytest

import encode_cases as EC
import encode_model as M
import export_model as EM
import prog_codec as PC

Image = pytest.importorskip("PIL.Image")

_SUB = {"grey": 0, "4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def pillow_file(pixels, layout, quality=None, qtables=None):
    bio = io.BytesIO()
    kw = dict(qtables=[list(t) for t in qtables]) if qtables is not None else dict(quality=quality)
    Image.fromarray(pixels).save(bio, "JPEG", subsampling=_SUB[layout], **kw)
    return bio.getvalue()


def file_tables(D):
    """(luma, chroma) in natural order, from the file's own DQT."""
    out = []
    for c in (0, D.frame.ncomp - 1):
        qz = D.frame.qtabs[D.frame.comps[c][2]]; nat = [0] * 64
        for z in range(64):
            nat[PC.ZIGZAG[z]] = qz[z]
        out.append(nat)
    return out


def compare(pixels, layout, D, wrong=None):
    """-> None, or a text saying where the model (read `wrong`) and the decoded file differ."""
    fr = D.frame
    hv, mcu_x, mcu_y, lev = M.levels(pixels, _SUB[layout], file_tables(D), wrong)
    if hv != fr.hv or (mcu_x, mcu_y) != (fr.mcu_x, fr.mcu_y):
        return "geometry %r %r" % (hv, fr.hv)
    for c in range(fr.ncomp):
        got = D.coefs[c].astype(np.int64); want = lev[c][..., PC.ZIGZAG]
        nby, nbx = fr.coded(c); h, v = fr.hv[c]
        if not np.array_equal(got[:nby, :nbx], want[:nby, :nbx]):
            return "component %d: a real block differs" % c
        for my in range(fr.mcu_y):                                     # the dummy blocks by the rule, on the FILE's own levels
            for mx in range(fr.mcu_x):
                prev = None
                for vv in range(v):
                    for hh in range(h):
                        by, bx = my * v + vv, mx * h + hh
                        if by >= nby or bx >= nbx:
                            if prev is None or got[by, bx, 0] != prev or got[by, bx, 1:].any():
                                return "component %d: the file's dummy block (%d, %d) breaks the rule" % (c, bx, by)
                            if not np.array_equal(want[by, bx], got[by, bx]):
                                return "component %d: dummy block (%d, %d) differs" % (c, bx, by)
                        prev = got[by, bx, 0]
    return None


@pytest.mark.parametrize("layout", EC.LAYOUTS)
@pytest.mark.parametrize("size", EC.SIZES, ids=lambda s: "%dx%d" % s)
def test_model_levels_are_pillows(layout, size):
    w, h = size
    px = EC.picture(w, h, seed=w + h + _SUB[layout], grey=layout == "grey")
    for q in EC.QUALITIES:
        D = PC.decode(pillow_file(px, layout, quality=q))
        assert compare(px, layout, D) is None, (q, compare(px, layout, D))
    D = PC.decode(pillow_file(px, layout, qtables=EC.CUSTOM[:1] if layout == "grey" else EC.CUSTOM))
    assert sorted(file_tables(D)[0]) == sorted(EC.CUSTOM[0])             # (whatever order Pillow takes them in, the file carries the custom values)
    assert compare(px, layout, D) is None, compare(px, layout, D)


def test_quality_tables_are_pillows_for_every_quality():
    px = EC.picture(8, 8, seed=3)
    for q in range(1, 101):
        D = PC.decode(pillow_file(px, "4:4:4", quality=q))
        assert [list(t) for t in M.quality_tables(q)] == file_tables(D), q
    for t in M.quality_tables(1):
        assert max(t) == 255                                             # the clamp is met below quality 25
    assert M.quality_tables(100) == ([1] * 64, [1] * 64)


def scan_bytes(f):
    D = PC.decode(f)
    return bytes(f[D.scans[0]["start"]:D.scans[0]["end"]])


@pytest.mark.parametrize("layout", EC.LAYOUTS)
@pytest.mark.parametrize("size,quality", [((50, 70), 85), ((17, 9), 100), ((130, 21), 10), ((1, 1), 50)], ids=lambda v: str(v))
def test_exported_scan_of_the_models_arena_is_pillows(layout, size, quality):
    w, h = size
    px = EC.picture(w, h, seed=11 + w, grey=layout == "grey")
    f = pillow_file(px, layout, quality=quality)
    arena, dccum, geo, qnat = M.encode(px, _SUB[layout], M.quality_tables(quality))
    res, _det, mine = EM.export_file(arena, dccum, geo, w, h, qnat)
    assert res == EM.OK
    assert scan_bytes(mine) == scan_bytes(f)
    D = PC.decode(mine)
    assert (D.frame.width, D.frame.height, D.frame.hv) == (w, h, PC.decode(f).frame.hv)


@pytest.mark.parametrize("layout", EC.LAYOUTS)
def test_extreme_pictures_stay_codable_and_wrap_nothing(layout):
    assert M.pass1_max() < 32768
    for name, px in EC.extremes().items():
        if layout == "grey":
            px = np.ascontiguousarray(px[..., 0])
        arena, dccum, geo, qnat = M.encode(px, _SUB[layout], M.quality_tables(100))      # (asserts the int16 bound of the contract)
        lev, res, _det = EM.levels(arena, dccum, geo, qnat)
        assert res == EM.OK, (name, res)
        assert np.abs(lev[:, 1:]).max() <= 1023 and np.abs(lev[:, 0]).max() <= 2047, name
        assert compare(px, layout, PC.decode(pillow_file(px, layout, quality=100))) is None, name
    arena, dccum, geo, qnat = M.encode(EC.extremes()["checker"], 2, ([255] * 64, [255] * 64))
    assert EM.levels(arena, dccum, geo, qnat)[1] == EM.OK


WRONG = [("rows_to_mcu", "4:2:0", (50, 70), 85), ("const_bias", "4:2:0", (33, 31), 95), ("const_bias", "4:2:2", (33, 31), 95),
         ("chroma_offset", "4:4:4", (33, 31), 100), ("dummy_dc0", "4:2:0", (17, 9), 85), ("trunc_div", "4:4:4", (17, 9), 50)]


@pytest.mark.parametrize("wrong,layout,size,quality", WRONG, ids=lambda v: str(v))
def test_wrong_readings_are_refused(wrong, layout, size, quality):
    w, h = size
    px = EC.picture(w, h, seed=w + h + _SUB[layout])
    D = PC.decode(pillow_file(px, layout, quality=quality))
    assert compare(px, layout, D) is None
    assert compare(px, layout, D, wrong=wrong) is not None, "the wrong reading %r passes" % wrong
