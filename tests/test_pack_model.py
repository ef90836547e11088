"""CPU: tests/pack_model.py, the numpy model every test of jsnoop_batch_pack compares against, checked against an explicit per-pixel loop over
the oracle's DIB -- all pixels of a 17 x 9 grayscale image, a few hundred seeded positions of a 333 x 217 4:2:0 one -- and its float form
against the doubly rounded computation done in Python floats."""
import itertools

import numpy as np
import pytest

from pack_model import pack_model, two_roundings, one_rounding, tells_fma_apart

SCALE = (1 / 255, 1 / 255, 1 / 255)
BIAS = (-0.485, -0.456, -0.406)
SCALE2 = (0.1, 1 / 3, 0.7)                                       # none of them a float32
BIAS2 = (0.3, -1 / 7, 1e-3)


@pytest.fixture(scope="module")
def decoded(harness, oracle):
    out = {}
    for name, kw in (("small", dict(width=17, height=9, gray=1, seed=3)), ("large", dict(width=333, height=217, hs=2, vs=2, seed=4))):
        data = harness.synth_jpeg(**kw)
        harness.drive(oracle, data)
        dib = oracle.dib().copy()
        out[name] = (dib, kw["width"], kw["height"])
    assert out["small"][0].shape == (16, 24, 4) and out["large"][0].shape == (224, 336, 4)       # whole MCUs: the padding the pack crops
    return out


def pixel(dib, x, y, c, bgr):
    """Output channel c of output pixel (x, y): the DIB's dword at row img_y - 1 - y, bytes B, G, R, 0."""
    return int(dib[dib.shape[0] - 1 - y, x, c if bgr else 2 - c])


def positions(name, w, h):
    if name == "small":
        return list(itertools.product(range(w), range(h)))
    rng = np.random.default_rng(20261018)
    pts = {(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)}
    while len(pts) < 300:
        pts.add((int(rng.integers(w)), int(rng.integers(h))))
    return sorted(pts)


@pytest.mark.parametrize("name", ["small", "large"])
@pytest.mark.parametrize("layout", ["HWC", "CHW"])
@pytest.mark.parametrize("bgr", [False, True])
def test_uint8_model_is_the_per_pixel_loop(decoded, name, layout, bgr):
    dib, w, h = decoded[name]
    got = pack_model(dib, w, h, layout, "uint8", bgr)
    assert got.dtype == np.uint8 and got.shape == ((3, h, w) if layout == "CHW" else (h, w, 3)) and got.flags.c_contiguous
    for x, y in positions(name, w, h):
        for c in range(3):
            assert int(got[c, y, x] if layout == "CHW" else got[y, x, c]) == pixel(dib, x, y, c, bgr), (x, y, c)
    assert dib[..., 3].max() == 0                                # the DIB's fourth byte, which the pack drops


@pytest.mark.parametrize("name", ["small", "large"])
@pytest.mark.parametrize("layout", ["HWC", "CHW"])
@pytest.mark.parametrize("scale,bias", [(SCALE, BIAS), (SCALE2, BIAS2)])
def test_float_model_is_two_separate_roundings(decoded, name, layout, scale, bias):
    dib, w, h = decoded[name]
    for bgr in (False, True):
        got = pack_model(dib, w, h, layout, "float32", bgr, scale, bias)
        assert got.dtype == np.float32
        for x, y in positions(name, w, h):
            for c in range(3):
                want = two_roundings(pixel(dib, x, y, c, bgr), scale[c], bias[c])
                assert float(got[c, y, x] if layout == "CHW" else got[y, x, c]) == want, (x, y, c)


@pytest.mark.parametrize("scale,bias", [(SCALE, BIAS), (SCALE2, BIAS2)])
def test_the_constants_tell_a_fused_multiply_add_apart(scale, bias):
    """A condition on the inputs of the GPU test: for these constants a fused multiply-add differs from multiply-then-add on some of the 256 inputs
    in every channel, so a kernel that contracts the two operations cannot match the model."""
    apart = tells_fma_apart(scale, bias)
    assert all(len(a) > 0 for a in apart), apart
    v = apart[0][0]
    assert two_roundings(v, scale[0], bias[0]) != one_rounding(v, scale[0], bias[0])
    # ... and numpy's two operations are the two-rounding ones on all 256 inputs
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(4, axis=2)
    got = pack_model(ramp, 256, 1, "HWC", "float32", True, scale, bias)
    for c in range(3):
        assert [float(g) for g in got[0, :, c]] == [two_roundings(v, scale[c], bias[c]) for v in range(256)]
