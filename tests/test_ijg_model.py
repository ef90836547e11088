"""CPU: tests/ijg_model.py -- the definition of jsnoop_batch_pack_ijg -- against Pillow (libjpeg-turbo) on Pillow's own files, exactly: the model reads what
prog_codec.decode leaves of a file (dequantised as the arena holds it, the DC in slot 0) and must give Image.open(file).convert("RGB") byte for byte, over
every layout, the sizes around every block, MCU and clamp edge, four qualities, baseline and progressive, and pictures of extremes at quality 1, 3 and
100.  Every comparison also asserts the condition under which libjpeg's C and SIMD range limits agree: the largest |IDCT result| is at most 511.

Five deliberately wrong readings of the contract (ijg_model.WRONG) are each refused by a named case, and on a file of the largest levels the codes allow at
quantiser 255 -- where no decoder's pixels mean anything -- the model is deterministic and wraps as the contract says."""
import numpy as np
import pytest

import ijg_cases as IC
import ijg_model as M


def check(data, mode, what):
    a, w, h, hv = M.arena_of_file(data)
    assert hv == IC.HV[mode], (what, hv)
    got, peak = M.render(a, w, h, hv)
    assert peak <= 511, (what, peak)
    want = IC.pillow_pixels(data)
    assert got.shape == want.shape and np.array_equal(got, want), (what, int((got != want).sum()))
    return peak


@pytest.mark.parametrize("progressive", [False, True], ids=["baseline", "progressive"])
@pytest.mark.parametrize("mode", IC.MODES)
def test_the_model_gives_pillows_pixels_over_the_matrix(mode, progressive):
    for k, (w, h) in enumerate(IC.SIZES):
        for q in IC.QUALITIES:
            check(IC.pillow_file(IC.noise(w, h, 100 * k + q), mode, q, progressive), mode, (mode, w, h, q, progressive))


@pytest.mark.parametrize("mode", IC.MODES)
def test_pictures_of_extremes_at_the_ends_of_the_quality_range(mode):
    peak = 0
    for name, px in IC.extremes():
        for q in (1, 3, 100):
            peak = max(peak, check(IC.pillow_file(px, mode, q), mode, (mode, name, q)))
    assert peak > 128                                                # (these pictures do leave the sample range: the clamp is at work)


# the case that refuses each wrong reading: (mode, width, height, quality).  The padding is read only where the last chroma column has an odd output
# column inside the picture (an even width whose half is no multiple of 8); interpolation at dw <= 2 needs dw = 2; G's rounding needs unsubsampled chroma noise.
REFUSES = {"pad_neighbours": [("420", 50, 70, 85), ("422", 6, 40, 85)], "interp_small": [("420", 4, 5, 85), ("422", 3, 3, 85)],
           "bias_swapped": [("420", 16, 16, 85), ("422", 16, 16, 85)], "rows_first": [("grey", 16, 16, 100)], "g_separate": [("444", 16, 16, 100)]}


@pytest.mark.parametrize("wrong", M.WRONG)
def test_every_wrong_reading_is_refused_by_a_named_case(wrong):
    assert set(REFUSES) == set(M.WRONG)
    for mode, w, h, q in REFUSES[wrong]:
        data = IC.pillow_file(IC.noise(w, h, 7), mode, q)
        a, W, H, hv = M.arena_of_file(data)
        want = IC.pillow_pixels(data)
        assert np.array_equal(M.render(a, W, H, hv)[0], want)
        assert not np.array_equal(M.render(a, W, H, hv, wrong)[0], want), (wrong, mode, w, h, q)


def test_not_renderable_layouts_are_named():
    assert M.renderable([(1, 1)]) and M.renderable(IC.HV["420"]) and M.renderable(IC.HV["422"]) and M.renderable(IC.HV["444"])
    for hv in ([(1, 2), (1, 1), (1, 1)], [(4, 1), (1, 1), (1, 1)], [(2, 2), (2, 1), (1, 1)], [(1, 1), (1, 1)], [(1, 1)] * 4, [(2, 2)]):
        assert not M.renderable(hv), hv


def test_the_largest_levels_at_quantiser_255_wrap_as_the_contract_says():
    """Not compared with Pillow.  The arena wraps in int16 ((int16)(1023 * 255) = -1279); the IDCT's results pass 511; rendering twice gives the same bytes;
    and the wrap is the contract's: a transform carried out in exact (unbounded) integers and reduced modulo 2^32 only in front of each shift agrees."""
    data = IC.wild_file()
    a, w, h, hv = M.arena_of_file(data)
    assert int(a.max()) == 1279 and int(a.min()) == -1279 and hv == IC.HV["420"]
    px, peak = M.render(a, w, h, hv)
    px2, peak2 = M.render(a.copy(), w, h, hv)
    assert peak > 511 and peak == peak2 and np.array_equal(px, px2) and px.shape == (h, w, 3)
    # one block in Python integers, every product and sum exact
    def step(v, n):
        z1 = (v[2] + v[6]) * 4433; t2 = z1 - v[6] * 15137; t3 = z1 + v[2] * 6270; t0 = (v[0] + v[4]) << 13; t1 = (v[0] - v[4]) << 13
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        p, q, r, s = v[7], v[5], v[3], v[1]
        z1, z2, z3, z4 = p + s, q + r, p + r, q + s; z5 = (z3 + z4) * 9633
        p, q, r, s = p * 2446, q * 16819, r * 25172, s * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        p, q, r, s = p + z1 + z3, q + z2 + z4, r + z2 + z3, s + z1 + z4
        wrap = lambda x: ((x + (1 << (n - 1)) + (1 << 31)) % (1 << 32) - (1 << 31)) >> n
        return [wrap(x) for x in (t10 + s, t11 + r, t12 + q, t13 + p, t13 - p, t12 - q, t11 - r, t10 - s)]
    for blk in (a[0], a[5], np.full(64, -32768, np.int16), np.full(64, 32767, np.int16)):
        c = [[int(blk[8 * y + x]) for x in range(8)] for y in range(8)]
        cols = [step([c[k][x] for k in range(8)], 11) for x in range(8)]
        want = [step([cols[x][y] for x in range(8)], 18) for y in range(8)]
        assert M.idct(np.asarray(blk).reshape(8, 8)).tolist() == want
