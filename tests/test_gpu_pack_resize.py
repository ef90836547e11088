"""-m gpu: jsnoop_batch_pack_resized / k_pack_resize (jsnoop_pack_resize.hip) and JpegBatch.to_torch(size=...) -- a rectangle of every listed image of
a decoded batch, resampled to the size its destination asks for, in caller-owned device memory.

Every comparison is exact (np.array_equal / torch.equal) against tests/resize_model.py applied to the batch's own DIB (JpegBatch.dib), and once per
filter against the model applied to the ORACLE's DIB of the same files.  Raw calls write into the arena of tests/test_gpu_pack.py: 0xA5 bytes with a
guard band in front of, behind and between the destinations and in every pitch gap, and the whole arena is compared with what the model predicts.
Images are tiny; the larger cases are the ones that need their size (64-bit sums, the deal over many workgroups)."""
import ctypes as C

import numpy as np
import pytest

import prog_cases as PC
import resize_model as RM
from pack_model import pack_model, tells_fma_apart
from test_gpu_pack import Arena, decoded_batch, make_spec, SCALE, BIAS, SCALE2, BIAS2, SAMPLINGS

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 5, 16, 17, 33, 63, 65, 130, 515, 1030]
HEIGHTS = [1, 7, 9, 17, 67]
FILTERS = [RM.NEAREST, RM.BILINEAR, RM.AREA]
FORMS = [("HWC", "uint8"), ("CHW", "uint8"), ("HWC", "float32"), ("CHW", "float32")]
UNIT = 256                                                       # JS_RESIZE_SEG: output pixels of one unit


def seam_shapes():
    """Every width with two heights and two samplings (a sparse crossing), plus padding of 15 columns and 15 rows, the smallest and the largest."""
    out = []
    for k, w in enumerate(WIDTHS):
        out.append((w, HEIGHTS[k % 5], k % 4))
        out.append((w, HEIGHTS[(k + 2) % 5], (k + 1) % 4))
    out += [(17, 17, 2), (515, 9, 1), (1030, 67, 2), (130, 16, 0)]
    return out


def targets_of(k, w, h):
    """Three of the eight kinds of output size per source, rotating: 1x1, identity, x2, x1.37, exactly 1/2 (of the even part), x0.43, N x 1, 1 x N."""
    kinds = [(1, 1), (w, h), (2 * w, 2 * h), (max(1, int(w * 1.37)), max(1, int(h * 1.37))), (max(1, w // 2), max(1, h // 2)),
             (max(1, int(w * 0.43)), max(1, int(h * 0.43))), (w, 1), (1, h)]
    return [kinds[(k + j * 3) % 8] for j in range(3)]


def seam_dests(shapes):
    """(image, roi, out_w, out_h) of the one call every form makes over the seam batch."""
    dests = []
    for k, (w, h, _) in enumerate(shapes):
        for ow, oh in targets_of(k, w, h):
            dests.append((k, None, ow, oh))
    # output widths around the 4-pixel group, the wave and the unit, from sources of several widths
    for j, ow in enumerate([3, 4, 5, 63, 64, 65, UNIT - 1, UNIT, UNIT + 1, 2 * UNIT + 3]):
        src = [k for k, s in enumerate(shapes) if s[0] in (33, 130, 515)][j % 6]
        dests.append((src, None, ow, 1 + j % 3))
    return dests


def raw_resize(J, b, spec, filt, images, dsts):
    """jsnoop_batch_pack_resized as a C caller makes it: dsts = [(ptr, row_pitch, plane_pitch, out_w, out_h, (x, y, w, h) or None)].  Does not wait."""
    n = len(dsts)
    arr = (J.capi.ResizeDst * max(n, 1))()
    for k, (p, rp, pp, ow, oh, roi) in enumerate(dsts):
        x, y, w, h = roi or (0, 0, 0, 0)
        arr[k] = J.capi.ResizeDst(p, rp, pp, ow, oh, x, y, w, h)
    ind = (C.c_int * max(n, 1))(*images) if images is not None else None
    return J.load().jsnoop_batch_pack_resized(b._h, C.byref(spec), filt, ind, n, arr)


class LeadArena(Arena):
    """The arena of tests/test_gpu_pack.py with a lead of its own in front of every destination (up to 15 bytes off the 16-byte line)."""

    def __init__(self, torch, sizes, leads):
        super().__init__(torch, [nb + 16 for nb in sizes])
        self.offs = [o + l for o, l in zip(self.offs, leads)]
        self.sizes = list(sizes)


class Models:
    """resize_model over a list of DIBs: the interpolant of every (image, roi, size, filter) computed once (in R,G,B order), finished per form."""

    def __init__(self, dibs, dims):
        self.dibs, self.dims, self.memo = dibs, dims, {}

    def q(self, i, roi, ow, oh, filt):
        key = (i, roi, ow, oh, filt)
        if key not in self.memo:
            h, w = self.dims[i]
            q = RM.resize_q(RM.crop_of(self.dibs[i], w, h, roi), ow, oh, filt)
            q.setflags(write=False)
            self.memo[key] = q
        return self.memo[key]

    def __call__(self, i, roi, ow, oh, filt, layout, dtype, bgr=False, scale=None, bias=None):
        q = self.q(i, roi, ow, oh, filt)
        return RM.finish(np.ascontiguousarray(q[:, :, ::-1]) if bgr else q, layout, dtype, scale or (1.0, 1.0, 1.0), bias or (0.0, 0.0, 0.0))


def models_of(b):
    n = len(b)
    dims = [(b.info(i)["dim_y"], b.info(i)["dim_x"]) for i in range(n)]
    return Models([b.dib(i) for i in range(n)], dims), dims


def resize_and_check(J, torch, b, models, filt, layout, dtype, bgr, dests, scale=None, bias=None, vary=True, what=""):
    """One raw call for dests = [(image, roi, out_w, out_h)], then the whole arena against the model.  With vary, destinations take turns in being dense
    (pitch 0), dense with the pitch spelled out, and pitched with a gap; uint8 destinations start at every byte alignment."""
    elem = 4 if dtype == "float32" else 1
    geo = []
    for k, (i, roi, ow, oh) in enumerate(dests):
        gap = (0, 0, 5 * elem if elem == 1 else 8)[k % 3] if vary else 0
        rp = ow * elem * (3 if layout == "HWC" else 1) + gap
        pp = oh * rp + ((0, 0, 3 if elem == 1 else 12)[k % 3] if vary else 0)
        geo.append((rp, pp, oh * rp if layout == "HWC" else 3 * pp, k % 3 == 0 or not vary))
    leads = [(k % 4 if elem == 1 else 4 * (k % 4)) if vary else 0 for k in range(len(dests))]
    ar = LeadArena(torch, [g[2] for g in geo], leads)
    dsts = []
    for k, (i, roi, ow, oh) in enumerate(dests):
        rp, pp, _, dense = geo[k]
        ar.place(k, models(i, roi, ow, oh, filt, layout, dtype, bgr, scale, bias), layout, rp, pp)
        dsts.append((ar.ptr(k), 0 if dense else rp, 0 if dense or layout == "HWC" else pp, ow, oh, roi))
    torch.cuda.synchronize()                                      # (the fill ran on torch's stream, the call runs on the batch's)
    rc = raw_resize(J, b, make_spec(J, layout, dtype, bgr, scale, bias), filt, [d[0] for d in dests], dsts)
    assert rc == 0, J.last_error()
    torch.cuda.synchronize()
    ar.check("%s filter %d %s %s bgr=%d" % (what, filt, layout, dtype, bgr))


# ------------------------------------------------------------------------------------------------ the seam batch
@pytest.fixture(scope="module")
def seam(harness, oracle):
    import jpegsnoop_amd as J
    import torch
    shapes = seam_shapes()
    files = [harness.synth_jpeg(width=w, height=h, quality=90, seed=900 + k, **SAMPLINGS[s]) for k, (w, h, s) in enumerate(shapes)]
    b = decoded_batch(J, files)
    models, dims = models_of(b)
    assert dims == [(h, w) for w, h, _ in shapes]
    pads = [(b.info(i)["img_x"] - w, b.info(i)["img_y"] - h) for i, (w, h, _) in enumerate(shapes)]
    assert max(p[0] for p in pads) == 15 and max(p[1] for p in pads) == 15
    assert {s for _, _, s in shapes} == {0, 1, 2, 3}
    odibs = []
    for f in files:
        harness.drive(oracle, f)
        odibs.append(oracle.dib().copy())
    yield dict(J=J, torch=torch, b=b, files=files, shapes=shapes, models=models, dims=dims, oracle_models=Models(odibs, dims), n=len(files), dests=seam_dests(shapes))
    b.close()


def index_of(seam, w, h):
    return next(k for k, d in enumerate(seam["dims"]) if d == (h, w))


@pytest.mark.parametrize("layout,dtype", FORMS)
@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("filt", FILTERS)
def test_every_form_over_the_seams(seam, filt, layout, dtype, bgr):
    """All sources in ONE call per form: 1x1, identity, x2, x1.37, 1/2, x0.43, N x 1 and 1 x N outputs, output widths around the 4-pixel group, the wave and
    the unit, sources with up to 15 columns and rows of MCU padding that must never be read as pixels, dense and pitched destinations at every alignment."""
    sb = (None, None) if dtype == "uint8" else ((SCALE, BIAS) if not bgr else (SCALE2, BIAS2))
    resize_and_check(seam["J"], seam["torch"], seam["b"], seam["models"], filt, layout, dtype, bgr, seam["dests"], scale=sb[0], bias=sb[1], what="seams")


@pytest.mark.parametrize("filt", FILTERS)
def test_exact_against_the_model_on_the_oracles_dib(seam, filt):
    resize_and_check(seam["J"], seam["torch"], seam["b"], seam["oracle_models"], filt, "HWC", "uint8", False, seam["dests"], what="oracle DIB")
    resize_and_check(seam["J"], seam["torch"], seam["b"], seam["oracle_models"], filt, "CHW", "float32", True, seam["dests"], scale=SCALE, bias=BIAS, what="oracle DIB")


# ------------------------------------------------------------------------------------------------ identity
@pytest.mark.parametrize("filt", FILTERS)
def test_identity_is_the_plain_pack_cropped(seam, filt):
    """out = roi size: bit for bit what jsnoop_batch_pack writes for the same image, cropped -- uint8, and float32 with a scale and a bias."""
    J, torch, b = seam["J"], seam["torch"], seam["b"]
    name = {RM.NEAREST: "nearest", RM.BILINEAR: "bilinear", RM.AREA: "area"}[filt]
    cases = [(index_of(seam, 515, 9), (3, 2, 260, 5)), (index_of(seam, 17, 17), None), (index_of(seam, 1030, 67), (513, 1, 517, 66)), (index_of(seam, 1, 1), None),
             (index_of(seam, 65, 67), (1, 0, 64, 67)), (index_of(seam, 130, 17), (127, 16, 3, 1))]
    for i, roi in cases:
        h, w = seam["dims"][i]
        x, y, rw, rh = roi or (0, 0, w, h)
        for layout in ("HWC", "CHW"):
            for dtype, sc, bi in ((torch.uint8, None, None), (torch.float32, SCALE2, BIAS2)):
                plain = b.to_torch(images=[i], layout=layout, dtype=dtype, scale=sc, bias=bi)[0]
                want = plain[:, y:y + rh, x:x + rw] if layout == "CHW" else plain[y:y + rh, x:x + rw, :]
                got = b.to_torch(images=[i], layout=layout, dtype=dtype, scale=sc, bias=bi, size=(rh, rw), filter=name, roi=roi)
                assert tuple(got.shape) == (1,) + tuple(want.shape)
                assert torch.equal(got[0], want), (name, i, roi, layout, dtype)


# ------------------------------------------------------------------------------------------------ ROI
@pytest.mark.parametrize("filt", FILTERS)
def test_rois_at_borders_corners_and_every_left_alignment(seam, filt):
    J, torch, b = seam["J"], seam["torch"], seam["b"]
    i = index_of(seam, 130, 17)
    j = index_of(seam, 515, 9)
    dests = []
    for roi in [(0, 0, 40, 6), (90, 0, 40, 6), (0, 11, 40, 6), (90, 11, 40, 6),            # the four corners
                (0, 5, 9, 5), (121, 5, 9, 5), (50, 0, 30, 3), (50, 14, 30, 3),             # each border
                (0, 0, 1, 1), (129, 16, 1, 1), (64, 8, 1, 1), (7, 0, 1, 17), (129, 0, 1, 17), (0, 16, 130, 1), (3, 9, 100, 1)]:
        dests += [(i, roi, 12, 5), (i, roi, roi[2] * 2 + 1, roi[3] + 2)]
    for x in range(8):                                            # the ROI's left edge at every x mod 4, widths that end at every x mod 4 too
        dests += [(j, (x, 1, 300 + x % 3, 7), 37, 3), (j, (x + 4, 0, 16 + x, 9), 40 + x, 11), (j, (200 + x, 2, 515 - 200 - x, 5), 300, 4)]
    for layout, dtype in (("HWC", "uint8"), ("CHW", "float32")):
        resize_and_check(J, torch, b, seam["models"], filt, layout, dtype, False, dests, scale=SCALE if dtype == "float32" else None,
                         bias=BIAS if dtype == "float32" else None, what="ROIs")


@pytest.mark.parametrize("filt", FILTERS)
def test_nothing_outside_the_roi_is_mixed_in(harness, filt):
    """A black rectangle in a white frame and a white one in a black frame (flat 8x8 blocks, 4:4:4: every sample decodes to its block's value): whatever
    the size, the result is the model on the cropped array alone, i.e. flat -- one grey level from outside would show."""
    import jpegsnoop_amd as J
    import torch
    files, rois = [], []
    for inner, outer in ((0, 255), (255, 0)):
        a = np.full((40, 56, 3), outer, np.uint8)
        a[8:32, 16:40] = inner
        files.append(harness.encode_rgb(a, hs=1, vs=1, quality=95))
        rois.append((16, 8, 24, 24))
    b = decoded_batch(J, files)
    try:
        models, dims = models_of(b)
        for k in range(2):
            crop = RM.crop_of(b.dib(k), 56, 40, rois[k])
            assert crop.min() == crop.max() and abs(int(crop[0, 0, 0]) - (0, 255)[k]) <= 2, "the source is not the flat rectangle this test needs"
            assert abs(int(RM.crop_of(b.dib(k), 56, 40, None)[0, 0, 0]) - (255, 0)[k]) <= 2
        dests = [(k, rois[k], ow, oh) for k in range(2) for ow, oh in ((1, 1), (5, 7), (24, 24), (48, 48), (33, 19), (10, 100), (300, 2))]
        for layout, dtype in (("HWC", "uint8"), ("CHW", "float32")):
            resize_and_check(J, torch, b, models, filt, layout, dtype, False, dests, what="frame")
        flat = models(0, rois[0], 33, 19, filt, "HWC", "uint8")
        assert flat.min() == flat.max()
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ rounding
def test_uint8_ties_round_to_even_both_ways(seam):
    """AREA 2:1 (quarters) and BILINEAR x2 (sixteenths) on noisy sources: the model's q holds exact .5 below an even and below an odd integer; the device
    matches the model on all of them."""
    J, torch, b, models = seam["J"], seam["torch"], seam["b"], seam["models"]
    i, j = index_of(seam, 130, 16), index_of(seam, 65, 67)
    dests = [(i, None, 65, 8), (j, (1, 1, 64, 66), 32, 33), (i, None, 260, 32), (j, None, 130, 134)]
    filts = [RM.AREA, RM.AREA, RM.BILINEAR, RM.BILINEAR]
    for filt in (RM.AREA, RM.BILINEAR):
        down = up = 0
        mine = [d for d, f in zip(dests, filts) if f == filt]
        for (k, roi, ow, oh) in mine:
            q = models.q(k, roi, ow, oh, filt)
            ties = (q - np.floor(q)) == 0.5
            down += int((ties & (np.floor(q) % 2 == 0)).sum())
            up += int((ties & (np.floor(q) % 2 == 1)).sum())
        print("filter %d: %d ties round down to even, %d up to even" % (filt, down, up))
        assert down >= 1 and up >= 1
        for layout in ("HWC", "CHW"):
            resize_and_check(J, torch, b, models, filt, layout, "uint8", False, mine, what="ties")


@pytest.mark.parametrize("scale,bias", [(SCALE, BIAS), (SCALE2, BIAS2)])
def test_float_form_is_multiply_then_add_never_fused(seam, scale, bias):
    """Inputs on which a fused multiply-add gives another float than a multiply and an add (a condition checked here on the CPU, on the very q of this case):
    a contracted kernel fails the exact comparison."""
    J, torch, b, models = seam["J"], seam["torch"], seam["b"], seam["models"]
    assert all(len(a) > 0 for a in tells_fma_apart(scale, bias))
    i = index_of(seam, 515, 9)
    h, w = seam["dims"][i]
    for filt, ow, oh in ((RM.NEAREST, w, h), (RM.BILINEAR, w, h), (RM.AREA, w, h), (RM.AREA, w // 2, h // 2), (RM.BILINEAR, 2 * w, 2 * h)):
        q = models.q(i, None, ow, oh, filt).astype(np.float64)
        two = models(i, None, ow, oh, filt, "HWC", "float32", False, scale, bias)
        fused = (q * np.asarray(scale, np.float32).astype(np.float64) + np.asarray(bias, np.float32).astype(np.float64)).astype(np.float32)
        if ow == w:
            assert not np.array_equal(two, fused), "these pixels would not tell a fused kernel apart"
        resize_and_check(J, torch, b, models, filt, "HWC", "float32", False, [(i, None, ow, oh)], scale=scale, bias=bias, what="fma")
        resize_and_check(J, torch, b, models, filt, "CHW", "float32", True, [(i, None, ow, oh)], scale=scale, bias=bias, what="fma")


# ------------------------------------------------------------------------------------------------ 64-bit sums
def test_bilinear_sum_above_2_to_32(harness):
    import jpegsnoop_amd as J
    import torch
    bright = np.random.default_rng(3).integers(200, 256, (16, 16, 3), dtype=np.uint8)
    b = decoded_batch(J, [harness.encode_rgb(bright, hs=1, vs=1, quality=95)])
    try:
        models, _ = models_of(b)
        s, d = RM.resize_sd(RM.crop_of(b.dib(0), 16, 16), 2100, 2100, RM.BILINEAR)
        assert int(s.max()) > 2 ** 32 and d == 4200 * 4200
        resize_and_check(J, torch, b, models, RM.BILINEAR, "HWC", "uint8", False, [(0, None, 2100, 2100)], vary=False, what="S > 2^32")
    finally:
        b.close()


def test_area_sum_over_more_than_2_to_24_bright_pixels(harness):
    import jpegsnoop_amd as J
    import torch
    b = decoded_batch(J, [harness.encode_rgb(np.full((4112, 4096, 3), 255, np.uint8), hs=2, vs=2, quality=90)])
    try:
        models, dims = models_of(b)
        assert dims == [(4112, 4096)] and 4112 * 4096 > 2 ** 24
        crop = RM.crop_of(b.dib(0), 4096, 4112)
        assert crop.min() >= 250, "the source is not the bright field this test needs"
        dests = [(0, None, 1, 1), (0, None, 3, 2)]
        if crop.min() == 255:
            assert np.array_equal(models.q(0, None, 1, 1, RM.AREA), np.full((1, 1, 3), 255, np.float32))
        resize_and_check(J, torch, b, models, RM.AREA, "HWC", "uint8", False, dests, vary=False, what="> 2^24 pixels")
        resize_and_check(J, torch, b, models, RM.AREA, "CHW", "float32", False, dests, vary=False, what="> 2^24 pixels")
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ one allocation, many crops
def test_one_allocation_many_crops_in_shuffled_order(seam):
    J, torch, b, models = seam["J"], seam["torch"], seam["b"], seam["models"]
    big = index_of(seam, 1030, 67)
    others = [index_of(seam, 515, 9), index_of(seam, 17, 17), index_of(seam, 63, 7)]
    crops = [(big, (0, 0, 1030, 67)), (big, (1, 2, 200, 60)), (big, (515, 0, 515, 33)), (big, (1000, 50, 30, 17)), (big, (333, 13, 96, 48))] + [(i, None) for i in others]
    order = [5, 2, 7, 0, 4, 1, 6, 3]                              # entry e of the call fills slot order[e]
    for filt, layout, dtype in ((RM.BILINEAR, "CHW", "float32"), (RM.AREA, "CHW", "uint8"), (RM.NEAREST, "HWC", "uint8")):
        tdt = torch.float32 if dtype == "float32" else torch.uint8
        out = torch.full((8, 3, 32, 48) if layout == "CHW" else (8, 32, 48, 3), 7, dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        dsts = [(out[order[e]].data_ptr(), 0, 0, 48, 32, crops[e][1]) for e in range(8)]
        sb = (SCALE, BIAS) if dtype == "float32" else (None, None)
        assert raw_resize(J, b, make_spec(J, layout, dtype, False, *sb), filt, [c[0] for c in crops], dsts) == 0, J.last_error()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for e in range(8):
            assert np.array_equal(got[order[e]], models(crops[e][0], crops[e][1], 48, 32, filt, layout, dtype, False, *sb)), (filt, e)
    # the same through to_torch into a strided view: every second slot of a larger allocation, the slots between keep their content
    hold = torch.full((16, 3, 32, 48), 9, dtype=torch.uint8, device="cuda")
    view = hold[::2]
    r = b.to_torch(images=[c[0] for c in crops], size=(32, 48), filter="area", roi=[c[1] or (0, 0, seam["dims"][c[0]][1], seam["dims"][c[0]][0]) for c in crops], out=view)
    assert r is view
    got = hold.cpu().numpy()
    for e in range(8):
        assert np.array_equal(got[2 * e], models(crops[e][0], crops[e][1] or (0, 0, seam["dims"][crops[e][0]][1], seam["dims"][crops[e][0]][0]), 48, 32, RM.AREA, "CHW", "uint8")), e
        assert (got[2 * e + 1] == 9).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing_and_write_nothing(seam):
    J, torch, b, n = seam["J"], seam["torch"], seam["b"], seam["n"]
    i = index_of(seam, 515, 9)
    ar = Arena(torch, [64 * 64 * 12])
    p = ar.ptr(0)
    torch.cuda.synchronize()
    u8h, u8c = make_spec(J, "HWC", "uint8"), make_spec(J, "CHW", "uint8")
    f32h, f32c = make_spec(J, "HWC", "float32"), make_spec(J, "CHW", "float32")
    bad_layout, bad_dtype, too_long = make_spec(J, "HWC", "uint8"), make_spec(J, "HWC", "uint8"), make_spec(J, "HWC", "uint8")
    bad_layout.layout, bad_dtype.dtype, too_long.struct_size = 2, 7, C.sizeof(J.capi.PackSpec) + 8
    ok = (p, 0, 0, 64, 64, None)
    B = RM.BILINEAR
    cases = [("index past the end", u8h, B, [n], [ok], "out of range"), ("negative index", u8h, B, [-1], [ok], "out of range"),
             ("second index bad", u8h, B, [i, n + 3], [ok, ok], "entry 1"),
             ("NULL pointer", u8h, B, [i], [(0, 0, 0, 64, 64, None)], "NULL"), ("row_pitch below dense", u8h, B, [i], [(p, 191, 0, 64, 64, None)], "row_pitch"),
             ("CHW row_pitch below dense", u8c, B, [i], [(p, 63, 0, 64, 64, None)], "row_pitch"), ("plane_pitch below dense", u8c, B, [i], [(p, 64, 64 * 64 - 1, 64, 64, None)], "plane_pitch"),
             ("float pointer", f32h, B, [i], [(p + 2, 0, 0, 64, 64, None)], "multiples of 4"), ("float row_pitch", f32c, B, [i], [(p, 258, 0, 64, 64, None)], "multiples of 4"),
             ("float plane_pitch", f32c, B, [i], [(p, 256, 256 * 64 + 2, 64, 64, None)], "multiples of 4"),
             ("unknown layout", bad_layout, B, [i], [ok], "layout"), ("unknown dtype", bad_dtype, B, [i], [ok], "dtype"),
             ("struct_size of a later version", too_long, B, [i], [ok], "struct_size"),
             ("unknown filter", u8h, 3, [i], [ok], "filter"), ("negative filter", u8h, -1, [i], [ok], "filter"),
             ("out_w 0", u8h, B, [i], [(p, 0, 0, 0, 64, None)], "output size"), ("out_h 0", u8h, B, [i], [(p, 0, 0, 64, 0, None)], "output size"),
             ("out_w 32768", u8h, B, [i], [(p, 0, 0, 32768, 1, None)], "output size"), ("out_h 32768", u8h, B, [i], [(p, 0, 0, 1, 32768, None)], "output size"),
             ("roi_w 0 alone", u8h, B, [i], [(p, 0, 0, 64, 64, (0, 0, 0, 5))], "ROI"), ("roi_h 0 alone", u8h, B, [i], [(p, 0, 0, 64, 64, (0, 0, 5, 0))], "ROI"),
             ("empty ROI off the origin", u8h, B, [i], [(p, 0, 0, 64, 64, (1, 0, 0, 0))], "ROI"),
             ("ROI past the right edge", u8h, B, [i], [(p, 0, 0, 64, 64, (500, 0, 16, 9))], "leaves image %d" % i),
             ("ROI past the bottom", u8h, B, [i], [(p, 0, 0, 64, 64, (0, 1, 515, 9))], "leaves image %d" % i),
             ("ROI into the MCU padding", u8h, B, [i], [(p, 0, 0, 64, 64, (0, 0, 516, 9))], "leaves image %d" % i),
             ("ROI whose edge wraps", u8h, B, [i], [(p, 0, 0, 64, 64, (0xFFFFFFFF, 0, 2, 1))], "leaves image %d" % i),
             ("second ROI bad", u8h, RM.AREA, [i, i], [ok, (p, 0, 0, 8, 8, (0, 9, 1, 1))], "destination 1")]
    for what, spec, filt, images, dsts, word in cases:
        assert raw_resize(J, b, spec, filt, images, dsts) == -1, what
        err = J.last_error()
        assert word in err and "pack_resized" in err, (what, err)
    nb = J.JpegBatch()
    try:
        nb.add_jpeg(seam["files"][0])
        assert raw_resize(J, nb, u8h, B, [0], [ok]) == -1 and "not been decoded" in J.last_error()
        nb.upload()
        assert raw_resize(J, nb, u8h, B, [0], [ok]) == -1 and "not been decoded" in J.last_error()
    finally:
        nb.close()
    torch.cuda.synchronize()
    assert ar.untouched()
    # n == 0 is accepted; then one accepted call into the same arena
    assert raw_resize(J, b, u8h, B, None, []) == 0
    assert raw_resize(J, b, f32c, RM.AREA, [i], [(p, 0, 0, 64, 64, (3, 0, 512, 9))]) == 0, J.last_error()
    torch.cuda.synchronize()
    ar.place(0, seam["models"](i, (3, 0, 512, 9), 64, 64, RM.AREA, "CHW", "float32"), "CHW", 256, 256 * 64)
    ar.check("accepted after the refusals")


# ------------------------------------------------------------------------------------------------ ordering behind every decode form
def test_call_waits_for_both_halves_of_a_two_stream_decode(harness):
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=333, height=217, seed=40 + k) for k in range(5)]
    b = J.JpegBatch()
    try:
        for f in files:
            b.add_jpeg(f)
        b.set_split(2); b.upload()
        assert b.split_parts() == 2
        ar = Arena(torch, [100 * 60 * 3] * 5)
        torch.cuda.synchronize()
        b.decode()
        assert raw_resize(J, b, make_spec(J, "HWC", "uint8"), RM.AREA, None, [(ar.ptr(k), 0, 0, 100, 60, None) for k in range(5)]) == 0, J.last_error()
        b.sync()
        assert b.last_form() == 1
        models, _ = models_of(b)
        for k in range(5):
            ar.place(k, models(k, None, 100, 60, RM.AREA, "HWC", "uint8"), "HWC", 300, 0)
        ar.check("two-stream decode")
    finally:
        b.close()


def test_dc_only_fast_form_is_not_decoded_again(harness, oracle):
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=100, height=75, hs=2, vs=2, seed=500 + k) for k in range(3)]
    b = decoded_batch(J, files, decode_ac=False)
    try:
        assert b.last_form() == 2
        t = b.to_torch(layout="HWC", bgr=True, size=(30, 40), filter="area")
        assert b.last_form() == 2, "the call must not force a second decode"
        oracle.set_options(decode_ac=0)
        try:
            for k, f in enumerate(files):
                harness.drive(oracle, f)
                assert np.array_equal(t[k].cpu().numpy(), RM.resize_model(oracle.dib(), 100, 75, None, 40, 30, RM.AREA, "HWC", "uint8", True)), k
        finally:
            oracle.set_options()
    finally:
        b.close()


def test_progressive_batch(harness):
    import jpegsnoop_amd as J
    import torch
    c = PC.built(PC.NAMES[0])
    b = decoded_batch(J, [c.file, c.file])
    try:
        models, dims = models_of(b)
        h, w = dims[0]
        t = b.to_torch(layout="CHW", dtype=torch.float32, scale=SCALE, bias=BIAS, size=(h + 3, 2 * w + 1))
        for k in range(2):
            assert np.array_equal(t[k].cpu().numpy(), models(k, None, 2 * w + 1, h + 3, RM.BILINEAR, "CHW", "float32", False, SCALE, BIAS))
    finally:
        b.close()


def test_damaged_file_arrives_repaired_behind_sync(harness, oracle):
    """The damaged file of tests/test_gpu_pack.py: a call enqueued behind sync() resamples the reference's pixels of the damaged file."""
    import jpegsnoop_amd as J
    import torch
    base = harness.synth_jpeg(width=333, height=217, seed=61)
    harness.drive(oracle, base)
    clean = oracle.dib().copy()
    p = harness.parse_jpeg(base)
    at = p.scan_start + int((p.scan_end - p.scan_start) * 0.6)
    hurt, hurt_dib = None, None
    for bit in (0x10, 0x08, 0x20, 0x04, 0x40, 0x80, 0x01, 0x02):
        d = bytearray(base); d[at] ^= bit
        if d[at] == 0xFF or d[at - 1] == 0xFF:
            continue
        harness.drive(oracle, bytes(d))
        if oracle.status()["scan_bad"] and not np.array_equal(oracle.dib(), clean):
            hurt, hurt_dib = bytes(d), oracle.dib().copy()
            break
    assert hurt is not None
    b = decoded_batch(J, [base, hurt, base])
    try:
        assert b.info(1)["flags"] != 0 and b.info(1)["path"] == 1, "the flip must leave a flagged file on the parallel path"
        t = b.to_torch(layout="HWC", size=(217, 333), filter="nearest")
        assert np.array_equal(t[1].cpu().numpy(), pack_model(hurt_dib, 333, 217, "HWC"))
        t = b.to_torch(layout="HWC", size=(100, 150), filter="area")
        assert np.array_equal(t[1].cpu().numpy(), RM.resize_model(hurt_dib, 333, 217, None, 150, 100, RM.AREA, "HWC"))
        assert np.array_equal(t[0].cpu().numpy(), RM.resize_model(clean, 333, 217, None, 150, 100, RM.AREA, "HWC")) and torch.equal(t[0], t[2])
        assert not torch.equal(t[0], t[1])
    finally:
        b.close()


def test_same_handle_decoded_and_resized_again(harness):
    """decode, call, decode, call on one handle; then the handle cleared and refilled with more images (the record block grows), a plain pack and a resized
    one in turns through the one block."""
    import jpegsnoop_amd as J
    import torch
    first = [harness.synth_jpeg(width=65, height=17, seed=80), harness.synth_jpeg(width=33, height=9, hs=1, vs=1, seed=81)]
    b = decoded_batch(J, first)
    try:
        models, _ = models_of(b)
        for _ in range(2):
            t = b.to_torch(layout="HWC", size=(20, 30))
            for k in range(2):
                assert np.array_equal(t[k].cpu().numpy(), models(k, None, 30, 20, RM.BILINEAR, "HWC", "uint8"))
            b.decode()
        b.clear()
        more = [harness.synth_jpeg(width=16 + 3 * k, height=8 + k, seed=90 + k) for k in range(40)]
        for f in more:
            b.add_jpeg(f)
        b.upload(); b.decode(); b.sync()
        models, dims = models_of(b)
        a = b.to_torch(layout="CHW", size=(9, 11), filter="area")
        plain = b.to_torch(layout="HWC")
        h = b.to_torch(layout="HWC", bgr=True, size=(31, 7), filter="nearest")
        for k in range(40):
            assert np.array_equal(a[k].cpu().numpy(), models(k, None, 11, 9, RM.AREA, "CHW", "uint8")), k
            assert np.array_equal(plain[k].cpu().numpy(), pack_model(b.dib(k), dims[k][1], dims[k][0], "HWC")), k
            assert np.array_equal(h[k].cpu().numpy(), models(k, None, 7, 31, RM.NEAREST, "HWC", "uint8", True)), k
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ the Python surface
def test_to_torch_size_forms(seam):
    J, torch, b, models, dims = seam["J"], seam["torch"], seam["b"], seam["models"], seam["dims"]
    dev = torch.device("cuda", b.device())
    mixed = [index_of(seam, 515, 9), index_of(seam, 17, 17), index_of(seam, 1030, 67), index_of(seam, 130, 17)]
    names = {"nearest": RM.NEAREST, "bilinear": RM.BILINEAR, "area": RM.AREA}
    for name, filt in names.items():
        for layout in ("CHW", "HWC"):
            for dtype, tdt, sc, bi in (("uint8", torch.uint8, None, None), ("float32", torch.float32, SCALE, BIAS)):
                t = b.to_torch(images=mixed, layout=layout, dtype=tdt, scale=sc, bias=bi, size=(24, 32), filter=name)
                assert t.dtype == tdt and t.device == dev and tuple(t.shape) == ((4, 3, 24, 32) if layout == "CHW" else (4, 24, 32, 3)) and t.is_contiguous()
                for k, i in enumerate(mixed):
                    assert np.array_equal(t[k].cpu().numpy(), models(i, None, 32, 24, filt, layout, dtype, False, sc, bi)), (name, layout, dtype, k)
    # default filter is bilinear; roi as one tuple for all, and as a list
    one = (2, 1, 13, 7)
    t = b.to_torch(images=mixed, size=(5, 9), roi=one)
    for k, i in enumerate(mixed):
        assert np.array_equal(t[k].cpu().numpy(), models(i, one, 9, 5, RM.BILINEAR, "CHW", "uint8"))
    rois = [(0, 0, 515, 9), (16, 16, 1, 1), (1000, 60, 30, 7), (1, 0, 129, 17)]
    t = b.to_torch(images=mixed, size=(6, 10), roi=rois, filter="area", layout="HWC", bgr=True)
    for k, i in enumerate(mixed):
        assert np.array_equal(t[k].cpu().numpy(), models(i, rois[k], 10, 6, RM.AREA, "HWC", "uint8", True))
    # out= of exactly the shape is returned as it is
    out = torch.empty((4, 3, 6, 10), dtype=torch.float32, device=dev)
    assert b.to_torch(images=mixed, dtype=torch.float32, size=(6, 10), roi=rois, out=out) is out
    for k, i in enumerate(mixed):
        assert np.array_equal(out[k].cpu().numpy(), models(i, rois[k], 10, 6, RM.BILINEAR, "CHW", "float32"))
    assert tuple(b.to_torch(images=[], size=(4, 4)).shape) == (0, 3, 4, 4)
    # what Python refuses before the call
    with pytest.raises(ValueError, match="size="):
        b.to_torch(images=mixed, size=(4, 4), stack=True)
    with pytest.raises(ValueError, match="size="):
        b.to_torch(images=mixed, size=(4, 4), pad_to=(8, 8))
    with pytest.raises(ValueError, match="size="):
        b.to_torch(images=mixed, filter="area")
    with pytest.raises(ValueError, match="size="):
        b.to_torch(images=mixed, roi=one)
    with pytest.raises(ValueError, match="filter"):
        b.to_torch(images=mixed, size=(4, 4), filter="bicubic")
    with pytest.raises(ValueError, match="size"):
        b.to_torch(images=mixed, size=(0, 4))
    with pytest.raises(ValueError, match="size"):
        b.to_torch(images=mixed, size=(4, 32768))
    with pytest.raises(ValueError, match="size"):
        b.to_torch(images=mixed, size=7)
    with pytest.raises(ValueError, match="roi"):
        b.to_torch(images=mixed, size=(4, 4), roi=rois[:3])
    with pytest.raises(ValueError, match="leaves image"):
        b.to_torch(images=mixed, size=(4, 4), roi=(0, 0, 18, 5))
    with pytest.raises(ValueError, match="leaves image"):
        b.to_torch(images=mixed, size=(4, 4), roi=(0, 0, 0, 0))
    with pytest.raises(ValueError, match="shape"):
        b.to_torch(images=mixed, size=(6, 10), out=torch.empty((4, 3, 6, 11), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="shape"):
        b.to_torch(images=mixed, size=(6, 10), out=[torch.empty((3, 6, 10), dtype=torch.uint8, device=dev)] * 4)
    with pytest.raises(ValueError, match="cpu"):
        b.to_torch(images=mixed, size=(6, 10), out=torch.empty((4, 3, 6, 10), dtype=torch.uint8))
    with pytest.raises(ValueError, match="float32"):
        b.to_torch(images=mixed, size=(6, 10), out=torch.empty((4, 3, 6, 10), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="contiguous"):
        b.to_torch(images=mixed, size=(6, 10), out=torch.empty((4, 3, 6, 20), dtype=torch.uint8, device=dev)[:, :, :, ::2])
    # without size= nothing changed
    ts = b.to_torch(images=mixed[:2])
    assert isinstance(ts, list) and tuple(ts[1].shape) == (3, 17, 17)


def test_job_file_result_to_torch_size_inside_the_callback(harness):
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=65, height=33, seed=21), PC.built(PC.NAMES[0]).file, harness.synth_jpeg(width=17, height=9, gray=1, seed=22), b"not a jpeg"]
    job = J.JpegJob(devices=[0])
    try:
        for f in files:
            job.add(f)
        seen = {}

        def on_file(r):
            if r.status != "ok":
                with pytest.raises(RuntimeError):
                    r.to_torch(size=(8, 8))
                seen[r.index] = None
                return False
            dib = r.batch.dib(r.image)
            h, w = r.info["dim_y"], r.info["dim_x"]
            t = r.to_torch(layout="HWC", size=(12, 20), filter="area")
            f = r.to_torch(layout="CHW", dtype=torch.float32, scale=SCALE, bias=BIAS, size=(7, 5), roi=(1, 2, w - 2, h - 3))
            assert t.device == torch.device("cuda", r.device) and tuple(t.shape) == (1, 12, 20, 3) and tuple(f.shape) == (1, 3, 7, 5)
            seen[r.index] = (np.array_equal(t[0].cpu().numpy(), RM.resize_model(dib, w, h, None, 20, 12, RM.AREA, "HWC")),
                             np.array_equal(f[0].cpu().numpy(), RM.resize_model(dib, w, h, (1, 2, w - 2, h - 3), 5, 7, RM.BILINEAR, "CHW", "float32", False, SCALE, BIAS)))
            return False
        stats = job.run(on_file)
        assert stats["ok"] == 3 and stats["refused"] == 1
        assert seen[3] is None and all(seen[i] == (True, True) for i in range(3)), seen
    finally:
        job.close()


# ------------------------------------------------------------------------------------------------ the deal over many workgroups
def test_eight_1080p_and_one_2160p_in_one_call(harness):
    """More units than one round of workgroups takes, sources of two sizes: down to [9, 3, 224, 224] with AREA and BILINEAR, and to 640 x 360 NEAREST."""
    import jpegsnoop_amd as J
    import torch
    f1080 = [harness.synth_jpeg(width=1920, height=1080, seed=s) for s in (5, 6)]
    f2160 = harness.synth_jpeg(width=3840, height=2160, seed=7)
    files = [f1080[k % 2] for k in range(8)] + [f2160]
    b = decoded_batch(J, files)
    try:
        dibs = {i: b.dib(i) for i in (0, 1, 8)}
        dims = {0: (1920, 1080), 1: (1920, 1080), 8: (3840, 2160)}
        for name, filt, size in (("area", RM.AREA, (224, 224)), ("bilinear", RM.BILINEAR, (224, 224)), ("nearest", RM.NEAREST, (360, 640))):
            want = {i: RM.resize_model(dibs[i], dims[i][0], dims[i][1], None, size[1], size[0], filt, "CHW") for i in (0, 1, 8)}
            t = b.to_torch(layout="CHW", size=size, filter=name)
            assert tuple(t.shape) == (9, 3) + size
            got = t.cpu().numpy()
            for k in range(9):
                assert np.array_equal(got[k], want[8 if k == 8 else k % 2]), (name, k)
    finally:
        b.close()
