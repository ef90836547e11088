"""CPU: tests/export_model.py, the definition of the exported JPEG, checked against three decoders that share nothing with it -- prog_codec.decode
(strict), the oracle (the reference's scan decoder in C) and Pillow / libjpeg -- and, as a second derivation of the token stream, against
prog_codec.encode_baseline when the model is handed that encoder's own optimal tables.  Then the result words on constructed inputs and the census
of every content case of tests/export_cases.py (what the GPU test runs the kernels on)."""
import io

import numpy as np
import pytest

import coef_model as CM
import export_cases as X
import export_model as EM
import prog_codec as PC

# 4:4:4, 4:2:2, 4:2:0, grey, 4:4:0, 4:1:1 (tests/test_gpu_planes.py's SAMPLINGS as frame components)
LAYOUTS = {"444": [(1, 1, 0), (1, 1, 1), (1, 1, 1)], "422": [(2, 1, 0), (1, 1, 1), (1, 1, 1)], "420": [(2, 2, 0), (1, 1, 1), (1, 1, 1)],
           "grey": [(1, 1, 0)], "440": [(1, 2, 0), (1, 1, 1), (1, 1, 1)], "411": [(4, 1, 0), (1, 1, 1), (1, 1, 1)]}
SIZES = [(1, 1), (17, 9), (72, 40)]
QTABS = {0: [1 + z % 7 for z in range(64)], 1: [2 + z % 5 for z in range(64)]}


def random_frame(layout, w, h, seed):
    """Sparse blocks with levels of every category: 1023 * 8 stays an int16, DC levels small enough for differences within +-2047."""
    rng = np.random.default_rng(seed)
    f = PC.Frame(w, h, LAYOUTS[layout], {k: v for k, v in QTABS.items() if k < (1 if layout == "grey" else 2)})
    coefs = f.zeros()
    for c in range(f.ncomp):
        a = coefs[c]
        a[..., 0] = rng.integers(-120, 121, a.shape[:2])
        mask = rng.random(a.shape[:2] + (63,)) < 0.12
        mag = (2 ** rng.integers(0, 11, mask.shape)).astype(np.int64)
        val = np.minimum(rng.integers(mag // 2 + (mag == 1), mag + 1), 1023) * rng.choice([-1, 1], mask.shape)
        a[..., 1:] = np.where(mask, val, 0)
        a[0, 0, 63] = 5                                              # one block without EOB
        if a.shape[1] > 1:
            a[0, 1, 1:] = 0; a[0, 1, 62] = -3                        # one run of 61
    return f, coefs


@pytest.fixture(scope="module")
def oracles(harness):
    full, dc = harness.oracle_backend(), harness.oracle_backend()
    full.set_options(decode_ac=1); dc.set_options(decode_ac=0)
    yield full, dc
    full.close(); dc.close()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_three_decoders_read_the_models_file_as_the_same_coefficients(harness, oracles, layout, size):
    from PIL import Image
    w, h = size
    f, coefs = random_frame(layout, w, h, seed=int(layout, 10) + w if layout != "grey" else 9000 + w)
    arena, dccum, geo, qnat = EM.frame_inputs(f, coefs)
    res, detail, data = EM.export_file(arena, dccum, geo, w, h, qnat)
    assert (res, detail) == (EM.OK, 0)
    # prog_codec, strict
    D = PC.decode(data)
    assert D.sof == 0xC0 and (D.frame.width, D.frame.height) == (w, h) and D.frame.hv == f.hv
    for c in range(f.ncomp):
        assert np.array_equal(D.coefs[c], coefs[c]), c
        assert D.frame.qtabs[c] == f.qtabs[f.comps[c][2]]
    # the oracle: blocks of its Full-IDCT decode, cumulative DC off the planes of its DC-only decode
    full, dc = oracles
    p = harness.drive(dc, data)
    assert CM.geometry_of(p).hv == geo.hv
    assert np.array_equal(CM.cum_from_planes(dc.planes(), geo), dccum)
    harness.drive(full, data)
    blocks = harness.oracle_coefs(full)
    assert np.array_equal(blocks[:, 1:], arena[:, 1:])
    # libjpeg
    im = Image.open(io.BytesIO(data)); im.load()
    assert im.size == (w, h) and im.mode == ("L" if layout == "grey" else "RGB")
    # without the APP0 segment the rest is the same, 18 bytes shorter
    _, _, bare = EM.export_file(arena, dccum, geo, w, h, qnat, jfif=False)
    assert bare == data[:2] + data[20:] and data[2:4] == b"\xFF\xE0"


@pytest.mark.parametrize("layout", ["420", "grey", "411"])
def test_with_the_encoders_own_tables_the_entropy_segment_is_encode_baselines(layout):
    """Two derivations of the token stream: prog_codec.encode_baseline from the coefficients, the model from arena, dccum and multipliers."""
    f, coefs = random_frame(layout, 72, 40, seed=7)
    ref = PC.encode_baseline(f, coefs)
    sc = PC.decode(ref).scans[0]
    arena, dccum, geo, qnat = EM.frame_inputs(f, coefs)
    lev, res, _ = EM.levels(arena, dccum, geo, qnat)
    assert res == EM.OK
    T = EM.tokens(lev, geo)
    tabs = [PC.optimal_table(fr) for fr in PC._freq(T, 4)]
    assert EM.entropy_bytes(T, tabs) == ref[sc["start"]:sc["end"]] and ref[sc["end"]:] == b"\xFF\xD9"


def test_result_words_on_constructed_inputs():
    geo = CM.Geometry([(1, 1)], 3, 1)
    q = [[2] * 64]

    def run(arena, dccum, **kw):
        return EM.export_file(np.asarray(arena, np.int16), np.asarray(dccum, np.int16), geo, 24, 8, kw.pop("q", q), **kw)

    z = np.zeros((3, 64), np.int16)
    assert run(z, [0, 0, 0])[0] == EM.OK
    a = z.copy(); a[1, 9] = 7                                        # 7 / 2 leaves a remainder
    assert run(a, [0, 0, 0])[:2] == (EM.INEXACT, 1) and run(a, [0, 0, 0])[2] is None
    assert run(z, [0, 0, 3])[:2] == (EM.INEXACT, 2)                  # a DC difference of 3
    assert run(z, [4094, 0, 0])[0] == EM.OK                          # DC difference levels 2047, -2047
    assert run(z, [4096, 0, 0])[:2] == (EM.UNCODABLE, 0)             # 2048
    assert run(z, [0, -4096, 0])[:2] == (EM.UNCODABLE, 1)
    assert run(z, [30000, -30000, 0], q=[[1] * 64])[:2] == (EM.UNCODABLE, 0)      # the difference wraps: (int16)(-60000) = 5536
    assert run(z, [20000, -20000, 0], q=[[16] * 64])[0] == EM.OK                   # ... and here to 25536 / 16 = 1596
    a = z.copy(); a[2, 63] = 2046
    assert run(a, [0, 0, 0])[0] == EM.OK                             # AC level 1023
    a[2, 63] = -2048
    assert run(a, [0, 0, 0])[:2] == (EM.UNCODABLE, 2)                # 1024
    a[0, 5] = 1                                                      # an inexact block in front of it does not take the detail
    assert run(a, [0, 0, 0])[:2] == (EM.UNCODABLE, 2)
    a[2, 63] = 0
    assert run(a, [0, 0, 0])[:2] == (EM.INEXACT, 0)
    assert run(z, [0, 0, 0], precision=12) == (EM.UNSUPPORTED, 0, None)
    a = z.copy(); a[:, 0] = 12345                                    # slot 0 of the arena is not read
    assert run(a, [0, 0, 0])[0] == EM.OK
    # a 16-bit multiplier whose product wrapped in the decode: level 3 * 30000 = 90000 -> (int16) 24464, no multiple of 30000
    a = z.copy(); a[0, 1] = np.int16(24464)
    q16 = [[1] + [30000] * 63]
    assert run(a, [0, 0, 0], q=q16)[:2] == (EM.INEXACT, 0)
    a[0, 1] = 30000
    res, _, data = run(a, [0, 0, 0], q=q16)
    D = PC.decode(data)
    assert res == EM.OK and D.sof == 0xC1 and D.coefs[0][0, 0, 1] == 1 and D.frame.qtabs[0][1] == 30000


CASES = X.cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_census_of_the_content_cases(case):
    """Every content case of the GPU test holds its event where it was meant to be; the strict decoder reads the model's file back."""
    X.check_census(case)
    _T, _u, _bits, _ends, f = case.model()
    if case.nblocks <= 400:
        D = PC.decode(f)
        assert np.array_equal(D.coefs[0], case.coefs[0])


def test_the_empty_cases_cover_every_padding_length():
    assert sorted(X.check_census(c) for c in CASES if c.name.startswith("empty_")) == list(range(8))
