"""CPU: tests/resize_model.py, the numpy statement of what jsnoop_batch_pack_resized computes, against its own invariants and against torch's CPU
interpolation.  The GPU tests compare k_pack_resize with this model bit for bit; these tests pin the model to the convention the header promises."""
import numpy as np
import pytest

import resize_model as RM

SIZES = [(1, 1), (3, 1), (1, 7), (5, 9), (16, 16), (17, 7), (33, 17), (63, 9), (65, 67), (130, 17), (515, 9)]        # (rw, rh)
TARGETS = [(1, 1), (7, 3), (224, 224)]


def source(rw, rh, seed):
    return np.random.default_rng(seed).integers(0, 256, (rh, rw, 3), dtype=np.uint8)


def targets_of(rw, rh):
    """Fixed targets plus the scale factors 2, 1/2, 1.37 and 0.43 of this source."""
    out = list(TARGETS)
    for f in (2.0, 0.5, 1.37, 0.43):
        out.append((max(1, int(rw * f)), max(1, int(rh * f))))
    return out


@pytest.mark.parametrize("filt", [RM.NEAREST, RM.BILINEAR, RM.AREA])
def test_identity_gives_the_cropped_input(filt):
    for k, (rw, rh) in enumerate(SIZES):
        R = source(rw, rh, k)
        q = RM.resize_q(R, rw, rh, filt)
        assert np.array_equal(q, R.astype(np.float32)), (rw, rh)
        assert np.array_equal(RM.finish(q, "HWC", "uint8"), R)


def test_area_weights_sum_to_the_source_extent():
    for r in (1, 2, 3, 7, 16, 17, 224, 515, 1080, 65535):
        for out in (1, 2, 3, 7, 16, 224, 225, 1030, 32767):
            covered = np.zeros(r, np.int64)
            for o in sorted({0, 1, out // 2, out - 2, out - 1} & set(range(out))) if out > 64 else range(out):
                j0, w = RM.area_weights(o, r, out)
                assert int(w.sum()) == r and (w <= out).all() and j0 >= 0 and j0 + len(w) <= r, (r, out, o)
                covered[j0:j0 + len(w)] += w.astype(np.int64)
            if out <= 64:
                assert (covered == out).all(), (r, out)          # every source pixel is handed out exactly once


def test_bilinear_against_torch_cpu():
    """Catches a half-pixel shift, a flipped axis or a swapped ratio (they show as whole grey levels).

    Tolerance 255 * max(rw, rh) * 2^-22: torch forms the source coordinate (o + 0.5) * (r / out) - 0.5 in float32 -- the ratio is rounded once and the
    product once, each an error of at most half an ulp of a value below max(rw, rh), i.e. together at most max(rw, rh) * 2^-23 pixels per axis.  The
    interpolant moves by at most 255 grey levels per pixel of coordinate error along each axis, so both axes together stay below
    2 * 255 * max(rw, rh) * 2^-23 = 255 * max(rw, rh) * 2^-22.  (The lerp's own float32 roundings are a few ulps of 255, far below.)"""
    import torch
    import torch.nn.functional as F
    worst, worst_ratio = 0.0, 0.0
    for k, (rw, rh) in enumerate(SIZES):
        R = source(rw, rh, 100 + k)
        t = torch.from_numpy(R.astype(np.float32)).permute(2, 0, 1)[None]
        bound = 255.0 * max(rw, rh) * 2.0 ** -22
        for ow, oh in targets_of(rw, rh):
            q = RM.resize_q(R, ow, oh, RM.BILINEAR)
            ref = F.interpolate(t, size=(oh, ow), mode="bilinear", align_corners=False, antialias=False)[0].permute(1, 2, 0).numpy()
            err = float(np.abs(q.astype(np.float64) - ref.astype(np.float64)).max())
            worst, worst_ratio = max(worst, err), max(worst_ratio, err / bound)
            assert err <= bound, (rw, rh, ow, oh, err, bound)
    print("bilinear against torch: worst |q - ref| = %.6f, worst err / bound = %.3f" % (worst, worst_ratio))


def test_nearest_picks_the_pixel_under_the_output_centre():
    """((2 o + 1) r) div (2 out) is floor((o + 0.5) * r / out) in exact arithmetic."""
    from fractions import Fraction
    for r, out in [(1, 5), (5, 1), (17, 33), (33, 17), (515, 224), (224, 515), (65535, 32767)]:
        idx = RM.nearest_index(r, out)
        for o in sorted({0, 1, out // 3, out // 2, out - 1} & set(range(out))):
            assert idx[o] == (Fraction(2 * o + 1, 2) * r / out).__floor__()
        assert idx.min() >= 0 and idx.max() <= r - 1


def test_area_against_torch_cpu_at_integer_ratios():
    """At integer ratios torch's adaptive windows are whole pixels and equal this model's.  Tolerance: torch sums up to fx * fy floats of at most 255
    in float32 and divides; a few ulps of 255 (2^-16 each) -- 8 ulps = 1.2e-4."""
    import torch
    import torch.nn.functional as F
    worst = 0.0
    for k, (ow, oh, fx, fy) in enumerate([(1, 1, 1, 1), (7, 5, 2, 2), (16, 3, 4, 3), (33, 9, 3, 7), (64, 2, 8, 5), (3, 4, 1, 2)]):
        R = source(ow * fx, oh * fy, 200 + k)
        t = torch.from_numpy(R.astype(np.float32)).permute(2, 0, 1)[None]
        q = RM.resize_q(R, ow, oh, RM.AREA)
        ref = F.interpolate(t, size=(oh, ow), mode="area")[0].permute(1, 2, 0).numpy()
        err = float(np.abs(q.astype(np.float64) - ref.astype(np.float64)).max())
        worst = max(worst, err)
        assert err <= 8 * 2.0 ** -16, (ow, oh, fx, fy, err)
    print("area against torch at integer ratios: worst |q - ref| = %.3g" % worst)


def test_area_upscale_by_an_integer_repeats_pixels():
    R = source(5, 3, 7)
    assert np.array_equal(RM.resize_q(R, 15, 6, RM.AREA), np.repeat(np.repeat(R, 2, axis=0), 3, axis=1).astype(np.float32))


def test_uint8_ties_go_to_even_in_both_directions():
    R = source(64, 64, 9)
    q = RM.resize_q(R, 32, 32, RM.AREA)                           # 2:1: quarters, so exact .5 abound
    frac = q - np.floor(q)
    ties = frac == 0.5
    down = ties & (np.floor(q) % 2 == 0)
    up = ties & (np.floor(q) % 2 == 1)
    assert down.any() and up.any()
    u8 = RM.finish(q, "HWC", "uint8")
    assert np.array_equal(u8[down], np.floor(q[down]).astype(np.uint8)) and np.array_equal(u8[up], np.floor(q[up]).astype(np.uint8) + 1)


def test_the_64_bit_seams():
    R = source(16, 16, 11)
    R[3, 4] = 255
    s, d = RM.resize_sd(R, 2100, 2100, RM.BILINEAR)
    assert int(s.max()) > 2 ** 32 and d == 4200 * 4200
    q = RM.resize_q(R, 2100, 2100, RM.BILINEAR)
    assert q.min() >= 0 and 254.0 < q.max() <= 255.0
    flat = np.full((4097, 4096, 3), 255, np.uint8)                 # rw * rh > 2^24
    s, d = RM.resize_sd(flat, 1, 1, RM.AREA)
    assert d == 4097 * 4096 and d > 2 ** 24 and int(s[0, 0, 0]) == 255 * d
    assert np.array_equal(RM.resize_q(flat, 1, 1, RM.AREA), np.full((1, 1, 3), 255, np.float32))


def test_crop_and_finish_follow_the_plain_pack():
    from pack_model import pack_model
    dib = np.random.default_rng(5).integers(0, 256, (16, 24, 4), dtype=np.uint8)
    for bgr in (False, True):
        full = pack_model(dib, 21, 13, "HWC", "uint8", bgr)
        assert np.array_equal(RM.crop_of(dib, 21, 13, None, bgr), full)
        assert np.array_equal(RM.crop_of(dib, 21, 13, (0, 0, 0, 0), bgr), full)
        assert np.array_equal(RM.crop_of(dib, 21, 13, (3, 2, 7, 5), bgr), full[2:7, 3:10])
        for layout in ("HWC", "CHW"):
            for dtype, sc, bi in (("uint8", (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), ("float32", (0.1, 1 / 3, 0.7), (0.3, -1 / 7, 1e-3))):
                assert np.array_equal(RM.resize_model(dib, 21, 13, None, 21, 13, RM.AREA, layout, dtype, bgr, sc, bi), pack_model(dib, 21, 13, layout, dtype, bgr, sc, bi))
