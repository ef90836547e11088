"""CPU: tests/ijg_scaled_model.py -- the definition of jsnoop_batch_pack_ijg_scaled -- against Pillow's (libjpeg-turbo's) reduced-size decode of Pillow's own
files, exactly: the model reads what prog_codec.decode leaves of a file and must give the draft()ed decode byte for byte at 1/2, 1/4 and 1/8, over every
layout, the sizes around every block, MCU and clamp edge, four qualities, baseline and progressive, and pictures of extremes at quality 1, 3 and 100.  Every
comparison asserts the size Pillow reports and that the largest |transform result| is at most 511 (where libjpeg's masked table and a saturation agree).

Pictures smaller than s cannot be given their scale through draft(); there the decoder's scale is set by hand, a route that is first shown to give draft()'s
bytes wherever both apply.  Five wrong readings (ijg_scaled_model.WRONG) are each refused by a named case, and the wild file wraps as the contract says."""
import numpy as np
import pytest

import ijg_cases as IC
import ijg_model as M
import ijg_scaled_model as S

SIZES = IC.SIZES + [(9, 7), (15, 17), (25, 25), (31, 33)]


def check(data, mode, what):
    a, w, h, hv = M.arena_of_file(data)
    assert hv == IC.HV[mode], (what, hv)
    peak = 0
    for s in S.SCALES:
        got, pk = S.render(a, w, h, hv, s)
        assert pk <= 511, (what, s, pk)
        want = S.pillow_reduced(data, s)
        assert want.shape == (-(-h // s), -(-w // s), 3), (what, s, want.shape)
        assert got.shape == want.shape and np.array_equal(got, want), (what, s, int((got != want).sum()))
        peak = max(peak, pk)
    return peak


@pytest.mark.parametrize("progressive", [False, True], ids=["baseline", "progressive"])
@pytest.mark.parametrize("mode", IC.MODES)
def test_the_model_gives_pillows_reduced_pixels_over_the_matrix(mode, progressive):
    for k, (w, h) in enumerate(SIZES):
        for q in IC.QUALITIES:
            check(IC.pillow_file(IC.noise(w, h, 100 * k + q), mode, q, progressive), mode, (mode, w, h, q, progressive))


@pytest.mark.parametrize("mode", IC.MODES)
def test_pictures_of_extremes_at_the_ends_of_the_quality_range(mode):
    peak = 0
    for name, px in IC.extremes():
        for q in (1, 3, 100):
            peak = max(peak, check(IC.pillow_file(px, mode, q), mode, (mode, name, q)))
    assert peak > 128                                                # (these pictures do leave the sample range: the clamp is at work)


def test_the_scale_set_by_hand_gives_drafts_bytes_wherever_both_apply():
    for mode in IC.MODES:
        for k, (w, h) in enumerate(SIZES):
            data = IC.pillow_file(IC.noise(w, h, 3 * k + 1), mode, 85, progressive=bool(k & 1))
            for s in S.SCALES:
                if w >= s and h >= s:
                    assert np.array_equal(S.pillow_reduced(data, s), S.pillow_reduced(data, s, by_hand=True)), (mode, w, h, s)


# the case that refuses each wrong reading: (mode, width, height, quality, scale)
REFUSES = {"chroma_at_luma_size": [("420", 50, 70, 85, 2), ("420", 50, 70, 85, 4), ("420", 50, 70, 85, 8)], "triangle_at_8": [("422", 50, 70, 85, 8)],
           "floor_size": [("444", 17, 9, 85, 2), ("420", 33, 31, 85, 8)], "index4_fed": [("grey", 16, 16, 100, 2), ("420", 16, 16, 100, 4)],
           "dc_shift": [("grey", 64, 48, 100, 8), ("422", 64, 48, 100, 8)]}


@pytest.mark.parametrize("wrong", S.WRONG)
def test_every_wrong_reading_is_refused_by_a_named_case(wrong):
    assert set(REFUSES) == set(S.WRONG)
    for mode, w, h, q, s in REFUSES[wrong]:
        data = IC.pillow_file(IC.noise(w, h, 7), mode, q)
        a, W, H, hv = M.arena_of_file(data)
        want = S.pillow_reduced(data, s)
        assert np.array_equal(S.render(a, W, H, hv, s)[0], want)
        bad = S.render(a, W, H, hv, s, wrong)[0]
        assert bad.shape != want.shape or not np.array_equal(bad, want), (wrong, mode, w, h, q, s)


def test_transform_sizes_are_jdmasters():
    for s in S.SCALES:
        m = 8 // s
        for mode in ("grey", "444", "422"):
            assert [S.transform_size(IC.HV[mode], c, s) for c in range(len(IC.HV[mode]))] == [m] * len(IC.HV[mode])
        assert [S.transform_size(IC.HV["420"], c, s) for c in range(3)] == [m, 2 * m, 2 * m]


def test_the_wild_file_wraps_as_the_contract_says():
    """Not compared with Pillow.  The reduced steps carried out in exact (unbounded) Python integers and reduced modulo 2^32 only in front of each shift
    agree with the model on blocks of the wild file and on blocks of +-32768 / 32767."""
    data = IC.wild_file()
    a, w, h, hv = M.arena_of_file(data)
    assert int(a.max()) == 1279 and int(a.min()) == -1279
    for s in S.SCALES:
        px, peak = S.render(a, w, h, hv, s)
        px2, peak2 = S.render(a.copy(), w, h, hv, s)
        assert np.array_equal(px, px2) and peak == peak2 and px.shape == (-(-h // s), -(-w // s), 3)
    assert S.render(a, w, h, hv, 2)[1] > 511

    def wrap(x, n):
        return ((x + (1 << (n - 1)) + (1 << 31)) % (1 << 32) - (1 << 31)) >> n

    def step4(v, n):
        t0 = v[0] << 14; t2 = v[2] * 15137 - v[6] * 6270; t10, t12 = t0 + t2, t0 - t2
        p = -v[7] * 1730 + v[5] * 11893 - v[3] * 17799 + v[1] * 8697
        q = -v[7] * 4176 - v[5] * 4926 + v[3] * 7373 + v[1] * 20995
        return [wrap(x, n) for x in (t10 + q, t12 + p, t12 - p, t10 - q)]

    def step2(v, n):
        t10 = v[0] << 15; t0 = -v[7] * 5906 + v[5] * 6967 - v[3] * 10426 + v[1] * 29692
        return [wrap(t10 + t0, n), wrap(t10 - t0, n)]

    for blk in (a[0], a[5], np.full(64, -32768, np.int16), np.full(64, 32767, np.int16)):
        c = [[int(blk[8 * y + x]) for x in range(8)] for y in range(8)]
        for n, step, p1, p2 in ((4, step4, 12, 19), (2, step2, 13, 20)):
            cols = [step([c[k][x] for k in range(8)], p1) for x in range(8)]
            want = [step([cols[x][y] for x in range(8)], p2) for y in range(n)]
            assert S.idct(np.asarray(blk).reshape(8, 8), n).tolist() == want
        assert S.idct(np.asarray(blk).reshape(8, 8), 1).tolist() == [[(c[0][0] + 4) >> 3]]
