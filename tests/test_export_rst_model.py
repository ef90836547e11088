"""CPU: tests/export_rst_model.py, the definition of the export with restart intervals, pinned before any kernel is compared
with it: against libjpeg byte for byte (Pillow writes DRI files with the Annex K tables), against prog_codec.encode_baseline(frame, coefs, dri) as a
second derivation of the token stream, against export_model / export_opt_model at Ri = 0, against three decoders that share nothing with it, and
on constructed inputs for the result words a restart changes."""
import io

import numpy as np
import pytest

import coef_model as CM
import export_model as EM
import export_opt_model as OM
import export_rst_model as RM
import prog_codec as PC
from test_export_model import LAYOUTS, SIZES, random_frame


@pytest.fixture(scope="module")
def oracles(harness):
    full, dc = harness.oracle_backend(), harness.oracle_backend()
    full.set_options(decode_ac=1); dc.set_options(decode_ac=0)
    yield full, dc
    full.close(); dc.close()


# ------------------------------------------------------------------------------------------------ libjpeg, byte for byte
PIL_SIZES = [(40, 24), (17, 9), (72, 40), (129, 65)]
PIL_RESTARTS = [("blocks", 1), ("blocks", 3), ("blocks", 7), ("rows", 1)]
SUBSAMPLING = {"420": 2, "422": 1, "444": 0}


def pillow_file(layout, w, h, kind, n, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    rgb = np.stack([(xx * 5 + yy * 3) % 256, (xx * 2 + yy * 7) % 256, (xx * yy) % 256], -1) + rng.integers(-20, 21, (h, w, 3))
    im = Image.fromarray(np.clip(rgb, 0, 255).astype(np.uint8), "RGB")
    out = io.BytesIO()
    kw = {"restart_marker_blocks": n} if kind == "blocks" else {"restart_marker_rows": n}
    im.save(out, "JPEG", quality=88, subsampling=SUBSAMPLING[layout], optimize=False, **kw)
    return out.getvalue()


@pytest.mark.parametrize("restart", PIL_RESTARTS, ids=lambda r: "%s%d" % r)
@pytest.mark.parametrize("size", PIL_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", list(SUBSAMPLING))
def test_the_models_scan_is_libjpegs_byte_for_byte_and_dri_sits_where_libjpeg_puts_it(layout, size, restart):
    pytest.importorskip("PIL")
    w, h = size
    f = pillow_file(layout, w, h, restart[0], restart[1], seed=w * 131 + h)
    D = PC.decode(f)
    sc = D.scans[0]
    ri = sc["dri"]
    assert D.sof == 0xC0 and len(D.scans) == 1 and ri == (restart[1] if restart[0] == "blocks" else restart[1] * D.frame.mcu_x)
    arena, dccum, geo, qnat = EM.frame_inputs(D.frame, D.coefs)
    res, detail, data = RM.export_file(arena, dccum, geo, w, h, qnat, ri)
    assert (res, detail) == (RM.OK, 0)
    sos = data.rindex(b"\xFF\xDA"); start = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    assert data[start:-2] == f[sc["start"]:sc["end"]] and f[sc["end"]:] == b"\xFF\xD9" == data[-2:]
    ni = RM.intervals(geo, ri)
    assert len(sc["intervals"]) == ni and data[start:].count(b"\xFF\xD0") == (ni + 6) // 8
    # DRI: directly in front of SOS and behind the last DHT, in both files
    fsos = sc["start"] - (start - sos)
    want = b"\xFF\xDD\x00\x04" + ri.to_bytes(2, "big")
    assert f[fsos - 6:fsos] == want == data[sos - 6:sos] and f[fsos:fsos + 2] == b"\xFF\xDA"
    assert max(m for m in range(len(f) - 1) if f[m:m + 2] == b"\xFF\xC4" and m < fsos) < fsos - 6
    assert data.rindex(b"\xFF\xC4", 0, sos) < sos - 6 and data.count(want) >= 1


def test_the_libjpeg_grid_has_more_than_eight_intervals_and_a_single_one():
    pytest.importorskip("PIL")
    counts = []
    for layout, (w, h), (kind, n) in (("444", (129, 65), ("blocks", 1)), ("420", (17, 9), ("blocks", 3)), ("420", (17, 9), ("blocks", 7))):
        D = PC.decode(pillow_file(layout, w, h, kind, n, seed=w * 131 + h))
        counts.append(len(D.scans[0]["intervals"]))
    assert counts[0] == 17 * 9 and 1 in counts


# ------------------------------------------------------------------------------------------------ a second derivation, and Ri = 0
@pytest.mark.parametrize("ri", [1, 2, 5, 9, 45, 46])
@pytest.mark.parametrize("layout", ["420", "grey", "411", "440"])
def test_with_the_encoders_own_tables_the_file_behind_sof_is_encode_baselines(layout, ri):
    """prog_codec.encode_baseline from the coefficients with its own DRI, the model from arena, dccum and multipliers: the optimal mode's tables, DRI
    behind them (encode_baseline writes DRI in front of its DHT segments: compared piece by piece) and the entropy-coded segment."""
    f, coefs = random_frame(layout, 72, 40, seed=7)
    ref = PC.encode_baseline(f, coefs, dri=ri)
    sc = PC.decode(ref).scans[0]
    arena, dccum, geo, qnat = EM.frame_inputs(f, coefs)
    res, _, data, freq, tabs = RM.export_parts(arena, dccum, geo, 72, 40, qnat, ri, optimal=True)
    assert res == RM.OK and sc["dri"] == ri
    sos = data.rindex(b"\xFF\xDA"); start = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    assert data[start:] == ref[sc["start"]:]
    for s, t in enumerate(tabs):
        assert PC._dht(s & 1, s >> 1, t) in ref[:sc["start"]]
    # the Annex K mode handed those tables is the same stream
    lev, res, _ = RM.levels(arena, dccum, geo, qnat, ri)
    T = RM.tokens(lev, geo, ri)
    assert res == RM.OK and PC._emit(T, tabs) == ref[sc["start"]:sc["end"]]
    assert sum(1 for t in T if t[0] == 2) == RM.intervals(geo, ri) - 1


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_ri_0_is_the_export_without_restart_in_both_modes(layout):
    f, coefs = random_frame(layout, 72, 40, seed=11)
    arena, dccum, geo, qnat = EM.frame_inputs(f, coefs)
    for jfif in (True, False):
        assert RM.export_file(arena, dccum, geo, 72, 40, qnat, 0, jfif=jfif) == EM.export_file(arena, dccum, geo, 72, 40, qnat, jfif=jfif)
        assert RM.export_file(arena, dccum, geo, 72, 40, qnat, 0, optimal=True, jfif=jfif) == OM.export_file(arena, dccum, geo, 72, 40, qnat, jfif=jfif)
    # one interval that holds everything: the same entropy-coded bytes, and DRI in the header
    nmcu = geo.nblocks // geo.bpm
    for ri in (nmcu, nmcu + 1):
        one = RM.export_file(arena, dccum, geo, 72, 40, qnat, ri)[2]; plain = EM.export_file(arena, dccum, geo, 72, 40, qnat)[2]
        sos = plain.rindex(b"\xFF\xDA")
        assert one == plain[:sos] + b"\xFF\xDD\x00\x04" + ri.to_bytes(2, "big") + plain[sos:]


# ------------------------------------------------------------------------------------------------ decoders
@pytest.mark.parametrize("optimal", [False, True], ids=["annex_k", "optimal"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_three_decoders_read_the_models_file_as_the_same_coefficients(harness, oracles, layout, size, optimal):
    from PIL import Image
    w, h = size
    f, coefs = random_frame(layout, w, h, seed=int(layout, 10) + w if layout != "grey" else 9000 + w)
    arena, dccum, geo, qnat = EM.frame_inputs(f, coefs)
    nmcu = geo.nblocks // geo.bpm
    plain = Image.open(io.BytesIO(EM.export_file(arena, dccum, geo, w, h, qnat)[2])); plain.load()
    for ri in sorted({1, 2, geo.mcu_x, max(1, nmcu - 1), nmcu, nmcu + 1}):
        res, detail, data = RM.export_file(arena, dccum, geo, w, h, qnat, ri, optimal=optimal)
        assert (res, detail) == (RM.OK, 0), ri
        D = PC.decode(data)
        assert D.sof == 0xC0 and D.scans[0]["dri"] == ri and len(D.scans[0]["intervals"]) == RM.intervals(geo, ri)
        for c in range(f.ncomp):
            assert np.array_equal(D.coefs[c], coefs[c]), (ri, c)
        full, dc = oracles
        harness.drive(dc, data)
        assert np.array_equal(CM.cum_from_planes(dc.planes(), geo), dccum), ri
        harness.drive(full, data)
        assert np.array_equal(harness.oracle_coefs(full)[:, 1:], arena[:, 1:]), ri
        im = Image.open(io.BytesIO(data)); im.load()
        assert im.size == (w, h) and im.tobytes() == plain.tobytes(), ri


# ------------------------------------------------------------------------------------------------ result words
def test_result_words_a_restart_changes():
    geo = CM.Geometry([(1, 1)], 3, 1)
    z = np.zeros((3, 64), np.int16)

    def run(dccum, q0, ri, **kw):
        return RM.export_file(z, np.asarray(dccum, np.int16), geo, 24, 8, [[q0] + [1] * 63], ri, **kw)

    # differences +2000, +2000: fine in a row, but block 1 alone is a level of 4000
    assert run([2000, 4000, 4000], 1, 0)[0] == RM.OK
    assert run([2000, 4000, 4000], 1, 3)[0] == RM.OK
    assert run([2000, 4000, 4000], 1, 1)[:2] == (RM.UNCODABLE, 1) and run([2000, 4000, 4000], 1, 1)[2] is None
    assert run([2000, 4000, 4000], 1, 2)[:2] == (RM.UNCODABLE, 2)
    assert run([2000, 4000, 4000], 1, 1, optimal=True)[:2] == (RM.UNCODABLE, 1)
    # a cumulative DC that wrapped int16 under q[0] = 3: ten steps of 6000, then 65538 = 3 * 21846, which the arena holds as (int16) 2.  Every difference is
    # exact (the int16 difference un-wraps); an interval that starts at block 10 codes the wrapped value itself, and 2 is no multiple of 3.
    geo12 = CM.Geometry([(1, 1)], 12, 1)
    z12 = np.zeros((12, 64), np.int16)
    real = [6000 * (i + 1) for i in range(10)] + [65538, 65541]
    cum = np.asarray([EM._i16(v) for v in real], np.int16)
    assert int(cum[10]) == 2 and int(cum[11]) == 5
    q3 = [[3] + [1] * 63]
    assert RM.export_file(z12, cum, geo12, 96, 8, q3, 0)[0] == RM.OK
    assert RM.export_file(z12, cum, geo12, 96, 8, q3, 12)[0] == RM.OK
    assert RM.export_file(z12, cum, geo12, 96, 8, q3, 10)[:2] == (RM.INEXACT, 10)
    assert RM.export_file(z12, cum, geo12, 96, 8, q3, 10, optimal=True)[:2] == (RM.INEXACT, 10)
    assert RM.export_file(z12, cum, geo12, 96, 8, q3, 5)[:2] == (RM.UNCODABLE, 5)          # 36000 wrapped is -29536: 9845 levels
    # effective Ri = 65536: host arithmetic
    assert RM.effective_ri(RM.ROWS, 2, 32768) == 65536
    assert RM.export_file(z, [0, 0, 0], geo, 24, 8, [[1] * 64], 65536) == (RM.UNSUPPORTED, 0, None)
    assert RM.export_file(z, np.zeros(3, np.int16), geo, 24, 8, [[1] * 64], 65535)[0] == RM.OK
    assert [RM.effective_ri(m, i, 120, 7) for m, i in ((RM.NONE, 0), (RM.MCUS, 5), (RM.ROWS, 2), (RM.SOURCE, 0))] == [0, 5, 240, 7]
