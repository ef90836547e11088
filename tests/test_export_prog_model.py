"""CPU: tests/export_prog_model.py, the definition of the progressive export, pinned before any kernel is compared with it:
against prog_codec.encode_progressive as a second derivation of every scan's token stream and tables, against prog_codec's strict decoder and
libjpeg (Pillow) as decoders that share nothing with it, against export_rst_model with the mode off, and on constructed inputs for the result words,
the arithmetic of the point transform and every way an end-of-band run begins, splits and ends."""
import io

import numpy as np
import pytest

import export_model as EM
import export_prog_model as PM
import export_rst_model as RM
import prog_codec as PC
from test_export_model import LAYOUTS, SIZES, random_frame


def scripts_for(ncomp):
    """name -> script: the built-in one, DC at Al 0, DC at Al 2 with two refinements, DC scans per component."""
    every = tuple(range(ncomp)); ac = [((c,), 1, 63, 0, 0) for c in range(ncomp)]
    return {"default": PM.DEFAULT[ncomp], "al0": [(every, 0, 0, 0, 0)] + ac, "al2": [(every, 0, 0, 0, 2)] + ac + [(every, 0, 0, 2, 1), (every, 0, 0, 1, 0)],
            "percomp": [((c,), 0, 0, 0, 0) for c in range(ncomp)] + ac}


def every_index(ncomp):
    return [(tuple(range(ncomp)), 0, 0, 0, 0)] + [((c,), k, k, 0, 0) for k in range(1, 64) for c in range(ncomp)]


RESTARTS = {"ri0": (PM.NONE, 0), "ri1": (PM.MCUS, 1), "ri3": (PM.MCUS, 3), "row": (PM.ROWS, 1)}


def reference(frame, coefs, script, restart):
    """prog_codec.encode_progressive on the same script with every scan's own Ri."""
    sc = []
    for comps, ss, se, ah, al in script:
        row = frame.mcu_x if len(comps) > 1 else frame.coded(comps[0])[1]
        sc.append(dict(comps=list(comps), ss=ss, se=se, ah=ah, al=al, dri=PM.scan_ri(restart[0], restart[1], row)))
    return PC.encode_progressive(frame, coefs, sc)


def expected_coefs(frame, coefs, script):
    """What a decoder holds: everything inside coded(c), DC also outside where an interleaved DC scan covered it, zero elsewhere."""
    out = []
    for c in range(frame.ncomp):
        a = np.where(frame.coded_mask(c)[..., None], coefs[c], 0).astype(np.int16)
        if any(ss == 0 and len(comps) > 1 and c in comps for comps, ss, _se, _ah, _al in script):
            a[..., 0] = coefs[c][..., 0]
        out.append(a)
    return out


def check_case(layout, w, h, script, restart, seed=5):
    f, coefs = random_frame(layout, w, h, seed)
    arena, dccum, geo, qnat = EM.frame_inputs(f, coefs)
    res, detail, data, scans = PM.export_parts(arena, dccum, geo, w, h, qnat, script, restart)
    assert (res, detail) == (PM.OK, 0)
    ref = reference(f, coefs, script, restart)
    R = PC.decode(ref)                                              # (encode_progressive writes DRI in front of a scan's DHT segments, the model behind them: piece by piece)
    assert len(scans) == len(R.scans)
    for i, (s, r) in enumerate(zip(scans, R.scans)):                 # two derivations of every scan: its data and its tables
        assert s["ecs"] == ref[r["start"]:r["end"]], (i, s["comps"], s["ss"])
        assert s["dht"] == b"" or s["dht"] in ref
    D = PC.decode(data)                                             # strict
    assert D.sof == 0xC2 and (D.frame.width, D.frame.height) == (w, h)
    for c, want in enumerate(expected_coefs(f, coefs, script)):
        assert np.array_equal(D.coefs[c], want), c
    return f, coefs, data, (arena, dccum, geo, qnat)


def pillow_pixels(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data)); im.load()
    return im.size, np.asarray(im)


@pytest.mark.parametrize("restart", list(RESTARTS))
@pytest.mark.parametrize("name", ["default", "al0", "al2", "percomp"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_the_model_is_encode_progressive_scan_by_scan_and_two_decoders_read_it(layout, size, name, restart):
    w, h = size
    script = scripts_for(1 if layout == "grey" else 3)[name]
    _f, _coefs, data, (arena, dccum, geo, qnat) = check_case(layout, w, h, script, RESTARTS[restart])
    pytest.importorskip("PIL")
    base = EM.export_file(arena, dccum, geo, w, h, qnat)[2]
    (size_p, pix_p), (size_b, pix_b) = pillow_pixels(data), pillow_pixels(base)          # libjpeg decodes the same coefficients twice
    assert size_p == (w, h) == size_b and np.array_equal(pix_p, pix_b)


@pytest.mark.parametrize("restart", ["ri0", "ri3"])
@pytest.mark.parametrize("layout", ["420", "grey"])
def test_every_ac_index_a_scan_of_its_own(layout, restart):
    script = every_index(1 if layout == "grey" else 3)
    assert len(script) == (64 if layout == "grey" else 190) and PM.validate(script) == (1 if layout == "grey" else 3)
    check_case(layout, 17, 9, script, RESTARTS[restart])


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_the_mode_off_is_export_rst_model(layout):
    f, coefs = random_frame(layout, 72, 40, seed=11)
    arena, dccum, geo, qnat = EM.frame_inputs(f, coefs)
    for restart, ri in (((PM.NONE, 0), 0), ((PM.MCUS, 3), 3), ((PM.ROWS, 1), geo.mcu_x)):
        for optimal in (False, True):
            assert PM.export_file(arena, dccum, geo, 72, 40, qnat, None, restart, optimal=optimal) == RM.export_file(arena, dccum, geo, 72, 40, qnat, ri, optimal)


# ------------------------------------------------------------------------------------------------ the rules of a script
BROKEN = {
    "no scan": [], "Ss > Se": [((0,), 0, 0, 0, 0), ((0,), 5, 4, 0, 0)], "Se 64": [((0,), 0, 0, 0, 0), ((0,), 1, 64, 0, 0)], "Al 14": [((0,), 0, 0, 0, 14)],
    "DC with Se": [((0,), 0, 5, 0, 0)], "AC of two": [((0, 1, 2), 0, 0, 0, 0), ((0, 1), 1, 63, 0, 0)], "AC with Al": [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1)],
    "AC refinement": [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((0,), 1, 63, 1, 0)], "DC Al not Ah - 1": [((0,), 0, 0, 0, 2), ((0,), 0, 0, 2, 0)],
    "components 0 and 1": [((0, 1), 0, 0, 0, 0), ((0,), 1, 63, 0, 0), ((1,), 1, 63, 0, 0)], "first DC with Ah": [((0,), 0, 0, 1, 0), ((0,), 1, 63, 0, 0)],
    "Ah not the last Al": [((0,), 0, 0, 0, 2), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 0, 0)], "DC ends at Al 1": [((0,), 0, 0, 0, 1), ((0,), 1, 63, 0, 0)],
    "DC coded twice": [((0,), 0, 0, 0, 0), ((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0)], "AC before DC": [((0,), 1, 63, 0, 0), ((0,), 0, 0, 0, 0)],
    "index twice": [((0,), 0, 0, 0, 0), ((0,), 1, 10, 0, 0), ((0,), 10, 63, 0, 0)], "index missing": [((0,), 0, 0, 0, 0), ((0,), 1, 10, 0, 0), ((0,), 12, 63, 0, 0)],
    "257 scans": [((0,), 0, 0, 0, 0)] * 257,
}


@pytest.mark.parametrize("name", list(BROKEN))
def test_a_script_that_breaks_a_rule_is_refused(name):
    with pytest.raises(ValueError):
        PM.validate(BROKEN[name])


def test_the_default_scripts_and_the_largest_script_are_legal():
    assert PM.validate(PM.DEFAULT[3]) == 3 and PM.validate(PM.DEFAULT[1]) == 1
    dc = [((c,), 0, 0, 0, 13) for c in range(3)] + [((c,), 0, 0, a, a - 1) for a in range(13, 0, -1) for c in range(3)]
    big = dc + [((c,), k, k, 0, 0) for k in range(1, 64) for c in range(3)]
    assert len(big) == 231 and PM.validate(big) == 3


# ------------------------------------------------------------------------------------------------ result words on constructed inputs
def grey_inputs(bw, bh, q0=1, qac=1):
    import coef_model as CM
    geo = CM.Geometry([(1, 1)], bw, bh)
    q = [qac] * 64; q[0] = q0
    return np.zeros((geo.nblocks, 64), np.int16), np.zeros(geo.nblocks, np.int16), geo, [q]


def run_grey(arena, dccum, geo, qnat, script=None, restart=(PM.NONE, 0), **kw):
    return PM.export_parts(arena, dccum, geo, geo.mcu_x * 8, geo.mcu_y * 8, qnat, script or PM.DEFAULT[1], restart, **kw)


def test_a_remainder_in_a_band_of_the_third_scan_names_its_block():
    arena, dccum, geo, qnat = grey_inputs(4, 3, qac=3)
    arena[7, PC.ZIGZAG[40]] = 7; arena[9, PC.ZIGZAG[2]] = 6
    assert run_grey(arena, dccum, geo, qnat)[:2] == (PM.INEXACT, 7)
    arena[7, PC.ZIGZAG[40]] = 9
    assert run_grey(arena, dccum, geo, qnat)[0] == PM.OK


def test_dc_differences_of_2047_and_2048_after_the_shift():
    al0 = scripts_for(1)["al0"]
    for d, want in ((2047, PM.OK), (2048, PM.UNCODABLE), (-2047, PM.OK), (-2048, PM.UNCODABLE)):
        arena, dccum, geo, qnat = grey_inputs(3, 1)
        dccum[1] = d
        r = run_grey(arena, dccum, geo, qnat, al0)
        assert r[0] == want and (want == PM.OK or r[1] in (1, 2))
    # codable at Al 1 and not at Al 0 ...
    arena, dccum, geo, qnat = grey_inputs(3, 1)
    dccum[1] = 4000
    assert run_grey(arena, dccum, geo, qnat, al0)[:2] == (PM.UNCODABLE, 1) and run_grey(arena, dccum, geo, qnat)[0] == PM.OK
    # ... and a restart undoes what the difference gained: 1000, 2500, 4000 differ by at most 1500 at Al 0; behind a restart 2500 stands for itself
    dccum[:] = (1000, 2500, 4000)
    assert run_grey(arena, dccum, geo, qnat, al0)[0] == PM.OK
    assert run_grey(arena, dccum, geo, qnat, al0, (PM.MCUS, 1))[:2] == (PM.UNCODABLE, 1)
    assert run_grey(arena, dccum, geo, qnat, None, (PM.MCUS, 1))[0] == PM.OK          # (Al 1: 500, 1250, 2000)
    dccum[2] = 5000
    assert run_grey(arena, dccum, geo, qnat, None, (PM.MCUS, 1))[:2] == (PM.UNCODABLE, 2)


def test_ac_levels_of_1023_and_1024():
    for v, want in ((1023, PM.OK), (-1023, PM.OK), (1024, PM.UNCODABLE), (-1024, PM.UNCODABLE)):
        arena, dccum, geo, qnat = grey_inputs(2, 2, qac=2)
        arena[2, PC.ZIGZAG[6]] = 2 * v
        assert run_grey(arena, dccum, geo, qnat)[:2] == (want, 2 if want else 0)


def test_a_wrapped_dccum_under_q0_3_is_inexact_as_an_absolute_value():
    arena, dccum, geo, qnat = grey_inputs(2, 1, q0=3)
    al3 = [((0,), 0, 0, 0, 3), ((0,), 1, 63, 0, 0), ((0,), 0, 0, 3, 2), ((0,), 0, 0, 2, 1), ((0,), 0, 0, 1, 0)]
    dccum[:] = (38998 - 65536, 39000 - 65536)                        # 3 x 13000 wrapped is -26536, no multiple of 3; its neighbour -26538 is one
    assert run_grey(arena, dccum, geo, qnat, al3)[:2] == (PM.INEXACT, 1)
    dccum[1] = -26535
    assert run_grey(arena, dccum, geo, qnat, al3)[0] == PM.OK


def test_the_point_transform_of_a_negative_dc_is_an_arithmetic_shift():
    arena, dccum, geo, qnat = grey_inputs(2, 1)
    dccum[:] = (-5, -1)
    res, _, data, scans = run_grey(arena, dccum, geo, qnat)
    assert res == PM.OK
    D = PC.decode(data)
    assert [int(v) for v in D.coefs[0][0, :, 0]] == [-5, -1]
    assert (1, -3 - 1, 2) in scans[0]["tokens"]                      # -5 >> 1 = -3, not -2
    # the reading that divides toward zero writes another file, and a decoder gets other values out of it
    wrong = run_grey(arena, dccum, geo, qnat, arithmetic=False)[2]
    assert wrong != data and [int(v) for v in PC.decode(wrong).coefs[0][0, :, 0]] != [-5, -1]


# ------------------------------------------------------------------------------------------------ end-of-band runs
BIG = (256, 129)                                                    # a grey 2048 x 1032 picture: 33 024 blocks
BIG2 = (256, 257)                                                   # 2048 x 2056: 65 792


def eob_census(tokens):
    """[(n, run)] of every EOBn of an AC scan's tokens."""
    out = []; i = 0
    while i < len(tokens):
        k, a, b = tokens[i]
        if k == 0 and a == 0 and (b & 15) == 0 and b != 0xF0:
            n = b >> 4
            out.append((n, (1 << n) + (tokens[i + 1][1] if n else 0))); i += 2 if n else 1
        else:
            i += 1
    return out


def big_run(empty, dims=BIG, restart=(PM.NONE, 0), tail=False):
    """Block 0 busy up to the band's end (or with a tail), then `empty` empty blocks, then a busy block; the rest of the scan full blocks."""
    arena, dccum, geo, qnat = grey_inputs(*dims)
    arena[:, PC.ZIGZAG[63]] = 1
    arena[1:1 + empty] = 0
    if tail:
        arena[0, PC.ZIGZAG[63]] = 0; arena[0, PC.ZIGZAG[7]] = 1
    res, _, data, scans = run_grey(arena, dccum, geo, qnat, None, restart)
    assert res == PM.OK
    f = PC.Frame(dims[0] * 8, dims[1] * 8, [(1, 1, 0)], {0: [1] * 64})
    D = PC.decode(data)
    want = np.zeros(geo.nblocks * 64, np.int16).reshape(geo.nblocks, 64); zz = np.array(PC.ZIGZAG); want[:] = arena[:, zz]
    assert np.array_equal(D.coefs[0].reshape(geo.nblocks, 64), want) and f.mcu_x == dims[0]
    return eob_census(scans[2]["tokens"]), data, (arena, dccum, geo, qnat)


@pytest.mark.parametrize("empty,want", [(32766, [(14, 32766)]), (32767, [(14, 32767)]), (32768, [(14, 32767), (0, 1)])])
def test_runs_around_32767_split_where_libjpeg_splits_them(empty, want):
    census, _data, _ = big_run(empty)
    assert census == want
    census, _data, _ = big_run(empty - 1, tail=True)                 # the tail block is the run's first
    assert census == want


def test_a_run_of_65535_is_two_full_eob14_and_one_block():
    census, _data, _ = big_run(65535, BIG2)
    assert census == [(14, 32767), (14, 32767), (0, 1)]


def test_what_ends_a_run_and_a_run_that_begins_at_an_interval_start():
    arena, dccum, geo, qnat = grey_inputs(8, 2)
    z = PC.ZIGZAG
    arena[0, z[6]] = 1                                               # tail; then 1, 2 empty; 3 a TAIL block ends the run of 3 and starts one
    arena[3, z[10]] = 2                                              # then 4 empty; 5 a FULL block ends the run of 2
    arena[5, z[63]] = 3                                              # 6, 7 empty: the run of 2 ends at the interval end (Ri 8); 8 .. 10 empty: begins at the interval start
    arena[11, z[63]] = 1                                             # 12 .. 15 empty: ended by the scan end
    res, _, data, scans = run_grey(arena, dccum, geo, qnat, None, (PM.MCUS, 8))
    assert res == PM.OK and eob_census(scans[2]["tokens"]) == [(1, 3), (1, 2), (1, 2), (1, 3), (2, 4)]
    f = PC.Frame(64, 16, [(1, 1, 0)], {0: [1] * 64})
    ref = PC.encode_progressive(f, [arena[:, np.array(z)].reshape(2, 8, 64)], [dict(comps=[0], ss=s[1], se=s[2], ah=s[3], al=s[4], dri=8) for s in PM.DEFAULT[1]])
    for s, r in zip(scans, PC.decode(ref).scans):
        assert s["ecs"] == ref[r["start"]:r["end"]]
