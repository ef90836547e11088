"""-m gpu: jsnoop_batch_pack_ijg_scaled / k_render_ijg_scaled (jsnoop_render_scaled.hip) and JpegBatch.to_torch(pixels="libjpeg", reduce=2 | 4 | 8) -- a decoded
batch rendered as libjpeg's reduced-size pixels into caller-owned device memory.

Every comparison is exact against tests/ijg_scaled_model.py fed the batch's OWN arena -- read through a jsnoop_batch_pack_coefs enqueued in front, the
cumulative DC in slot 0 -- and, for Pillow's files, against Pillow's draft()ed decode as well.  Raw calls write into an arena of 0xA5 bytes with guard bands
around and between the destinations and in every pitch gap, and the whole arena is compared with what the model predicts: a stray write anywhere shows.  A
failure names image, scale, component (channel) and the first differing pixel with its MCU.  Pictures are tiny; the helpers are test_gpu_pack_ijg's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deal_cases as D
import fuzz_util as F
import ijg_cases as IC
import ijg_model as M
import ijg_scaled_model as S
import test_gpu_pack_ijg as T

pytestmark = pytest.mark.gpu

ROOT = T.ROOT
SCALE, BIAS = T.SCALE, T.BIAS
SIZES = IC.SIZES + [(9, 7), (15, 17), (25, 25), (31, 33)]


@pytest.fixture(scope="module")
def J():
    import jpegsnoop_amd
    jpegsnoop_amd.load()
    return jpegsnoop_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def raw_scaled(J, b, spec, denom, images, dsts):
    """jsnoop_batch_pack_ijg_scaled as a C caller makes it: dsts = [(ptr, row_pitch, plane_pitch)].  Returns the call's value; does not wait."""
    n = len(dsts)
    arr = (J.capi.PackDst * max(n, 1))(*[J.capi.PackDst(p, rp, pp) for p, rp, pp in dsts])
    ind = (C.c_int * max(n, 1))(*images) if images is not None else None
    return J.load().jsnoop_batch_pack_ijg_scaled(b._h, C.byref(spec), denom, ind, n, arr)


def models_of(J, torch, b, scales=S.SCALES, images=None):
    """{(image, s): model pixels} from the batch's own arena as it is now; s = 1 is the full-size model."""
    images = list(range(len(b))) if images is None else images
    keep = T.arenas_now(J, torch, b, images)
    torch.cuda.synchronize()
    out = {}
    for i, a in T.arenas_of(b, keep).items():
        w, h, hv, _ = T.geometry(b, i)
        for s in scales:
            px = M.render(a, w, h, hv)[0] if s == 1 else S.render(a, w, h, hv, s)[0]
            px.setflags(write=False)
            out[i, s] = px
    return out


class Arena(T.Arena):
    """test_gpu_pack_ijg's arena; a mismatch is reported as image, scale, channel, pixel and MCU."""

    def explain(self, what, meta):
        got = self.buf.cpu().numpy()
        if np.array_equal(got, self.expect):
            return
        bad = int(np.flatnonzero(got != self.expect)[0])
        k = max([i for i, o in enumerate(self.offs) if o <= bad], default=-1)
        where = "outside every destination (arena offset %d)" % bad
        if k >= 0 and bad - self.offs[k] < self.sizes[k]:
            image, s, layout, elem, rp, pp, mcu = meta[k]
            o = bad - self.offs[k]
            if layout == "HWC":
                y, x, c = o // rp, (o % rp) // (3 * elem), ((o % rp) // elem) % 3
            else:
                c, y, x = o // pp, (o % pp) // rp, ((o % pp) % rp) // elem
            mw, mh = max(1, mcu[0] // s), max(1, mcu[1] // s)
            where = "image %d at 1/%d, component (channel) %d, pixel (x %d, y %d) of MCU (%d, %d), destination %d byte %d" % (image, s, c, x, y, x // mw, y // mh, k, o)
        raise AssertionError("%s: first wrong byte in %s: got 0x%02x, want 0x%02x; %d bytes differ" % (what, where, got[bad], self.expect[bad], int((got != self.expect).sum())))


def render_and_check(J, torch, b, models, s, layout, dtype, images, bgr=False, lead=0, row_extra=0, plane_extra=0, scale=None, bias=None, what="", denoms=None):
    """One raw call at denominator s for `images` with the given destination shape, then the whole arena against the model."""
    elem = 4 if dtype == "float32" else 1
    geo, meta = [], []
    for i in images:
        h, w = models[i, s].shape[:2]
        rp = w * elem * (3 if layout == "HWC" else 1) + row_extra
        pp = h * rp + plane_extra
        geo.append((rp, pp, h * rp if layout == "HWC" else 3 * pp))
        inf = b.info(i)
        meta.append((i, s, layout, elem, rp, pp, (inf["mcu_w"], inf["mcu_h"])))
    ar = Arena(torch, [g[2] for g in geo], lead)
    for k, i in enumerate(images):
        ar.place(k, T.form(models[i, s], layout, dtype, bgr, scale, bias), layout, geo[k][0], geo[k][1])
    dense = row_extra == 0 and plane_extra == 0
    dsts = [(ar.ptr(k), 0 if dense and k % 2 else geo[k][0], 0 if dense and k % 2 else (geo[k][1] if layout == "CHW" else 0)) for k in range(len(images))]
    torch.cuda.synchronize()                                      # (the fill above ran on torch's stream, the render runs on the batch's)
    assert raw_scaled(J, b, T.make_spec(J, layout, dtype, bgr, scale, bias), s, images, dsts) == 0, J.last_error()
    torch.cuda.synchronize()
    ar.explain("%s 1/%d %s %s bgr=%d lead=%d row+%d plane+%d" % (what, s, layout, dtype, bgr, lead, row_extra, plane_extra), meta)


# ------------------------------------------------------------------------------------------------ the four layouts against the model and Pillow
@pytest.fixture(scope="module")
def mixed(J, torch):
    """ONE mixed batch: the size list in all four layouts (baseline); the models of every image at 1, 1/2, 1/4, 1/8 from the batch's own arena, computed once."""
    files, modes = [], []
    for mode in IC.MODES:
        for k, (w, h) in enumerate(SIZES):
            files.append(IC.pillow_file(IC.noise(w, h, 17 * k + 3), mode, (10, 50, 85, 100)[k % 4])); modes.append(mode)
    b = T.decoded_batch(J, files)
    out = dict(b=b, files=files, modes=modes, models=models_of(J, torch, b, (1, 2, 4, 8)))
    yield out
    b.close()


def of_mode(m, mode):
    return [i for i, x in enumerate(m["modes"]) if x == mode]


@pytest.mark.parametrize("s", S.SCALES)
def test_every_size_of_every_layout_is_the_models_and_pillows(J, torch, mixed, s):
    b = mixed["b"]; n = len(b)
    for i, f in enumerate(mixed["files"]):                        # the model on the device's arena is Pillow's reduced decode of the file
        w, h = SIZES[i % len(SIZES)]
        assert b.ijg_scaled_size(i, s) == (-(-h // s), -(-w // s))
        assert np.array_equal(mixed["models"][i, s], S.pillow_reduced(f, s)), (mixed["modes"][i], w, h, s)
    render_and_check(J, torch, b, mixed["models"], s, "HWC", "uint8", list(range(n)), what="sizes")
    got = b.to_torch(layout="HWC", pixels="libjpeg", reduce=s)
    for i, f in enumerate(mixed["files"]):
        assert np.array_equal(got[i].cpu().numpy(), S.pillow_reduced(f, s)), (mixed["modes"][i], SIZES[i % len(SIZES)], s)


# ------------------------------------------------------------------------------------------------ unit, MCU and picture seams
def seam_sizes(mode, s):
    mw, mh = (8 if mode in ("grey", "444") else 16), (16 if mode == "420" else 8)
    run = 64 * s // mw                                            # MCUs of a unit: 64 reduced pixels
    ws = [(run + d) * mw + e for d in (-1, 0, 1) for e in (-1, 0, 1)]
    hs = [r * mh + d for r in (1, 2, 3) for d in (-1, 0, 1)]
    out = [(w, hs[(2 * k + 1) % len(hs)]) for k, w in enumerate(ws)] + [(ws[(5 * k) % len(ws)], h) for k, h in enumerate(hs)]
    # one MCU wide / high; X, Y no multiples of s; pictures smaller than s; 4:2:2 with reduced chroma widths of 2 and 3 at s = 2 (X = 8, 9)
    return out + [(mw, 3 * mh + 1), (mw - 1, 2 * mh), (2 * run * mw + 2, mh), (mw, mh), (1, 1), (s - 1, s - 1), (s - 1, 3 * s + 1), (2 * s + 1, 1), (s + 1, s + 1), (8, 5), (9, 4), (17, 3), (33, 2)]


@pytest.mark.parametrize("s", S.SCALES)
def test_unit_mcu_and_picture_seams(J, torch, s):
    files, sizes = [], []
    for mode in IC.MODES:
        for k, (w, h) in enumerate(seam_sizes(mode, s)):
            files.append(IC.pillow_file(IC.noise(w, h, 900 + k), mode, 92)); sizes.append((mode, w, h))
    b = T.decoded_batch(J, files)
    try:
        models = models_of(J, torch, b, (s,))
        for i in range(0, len(files), 7):
            assert np.array_equal(models[i, s], S.pillow_reduced(files[i], s)), sizes[i]
        render_and_check(J, torch, b, models, s, "HWC", "uint8", list(range(len(files))), what="seams")
        render_and_check(J, torch, b, models, s, "CHW", "uint8", list(range(len(files))), what="seams")
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ store forms
@pytest.mark.parametrize("layout,dtype", T.FORMS)
@pytest.mark.parametrize("bgr", [False, True])
def test_every_store_form(J, torch, mixed, layout, dtype, bgr):
    sb = (None, None) if dtype == "uint8" else (SCALE, BIAS)
    for s in S.SCALES:
        render_and_check(J, torch, mixed["b"], mixed["models"], s, layout, dtype, list(range(len(mixed["b"]))), bgr=bgr, scale=sb[0], bias=sb[1], what="forms")


@pytest.mark.parametrize("lead", [0, 1, 3, 15])
def test_uint8_destinations_at_any_byte_with_pitches_above_the_row(J, torch, mixed, lead):
    n = len(mixed["b"])
    for s in S.SCALES:
        render_and_check(J, torch, mixed["b"], mixed["models"], s, "HWC", "uint8", list(range(n)), lead=lead, row_extra=0, what="alignment")
        render_and_check(J, torch, mixed["b"], mixed["models"], s, "HWC", "uint8", list(range(n)), lead=lead, row_extra=13, what="alignment")
        render_and_check(J, torch, mixed["b"], mixed["models"], s, "CHW", "uint8", list(range(n)), lead=lead, row_extra=3, plane_extra=5, bgr=True, what="alignment")


def test_float_destinations_with_pitched_rows_and_planes(J, torch, mixed):
    n = len(mixed["b"])
    for s in S.SCALES:
        render_and_check(J, torch, mixed["b"], mixed["models"], s, "HWC", "float32", list(range(n)), lead=8, row_extra=20, scale=SCALE, bias=BIAS, what="pitched float")
        render_and_check(J, torch, mixed["b"], mixed["models"], s, "CHW", "float32", list(range(n)), lead=4, row_extra=8, plane_extra=12, scale=SCALE, bias=BIAS, what="pitched float")


# ------------------------------------------------------------------------------------------------ image lists
def test_a_shuffled_subset_an_image_listed_twice_and_per_image_reduce_lists(J, torch, mixed):
    b = mixed["b"]; n = len(b); models = mixed["models"]
    order = [int(i) for i in np.random.default_rng(4).permutation(n)[:23]] + [11, 2, 11]
    for s in S.SCALES:
        render_and_check(J, torch, b, models, s, "HWC", "uint8", order, what="shuffled")
    render_and_check(J, torch, b, models, 4, "CHW", "float32", order, scale=SCALE, bias=BIAS, what="shuffled")
    red = [(1, 2, 4, 8)[(3 * k + i) % 4] for k, i in enumerate(order)]
    got = b.to_torch(images=order, layout="HWC", pixels="libjpeg", reduce=red)
    for k, i in enumerate(order):
        assert np.array_equal(got[k].cpu().numpy(), models[i, red[k]]), (k, i, red[k])
    with pytest.raises(ValueError):
        b.to_torch(images=order, pixels="libjpeg", reduce=red[:-1])
    # reduce_for is Pillow's draft rule
    from PIL import Image
    import io
    for i in (9, 10, 11, 12, 30):
        inf = b.info(i)
        for size in ((1, 1), (3, 5), (8, 8), (inf["dim_y"], inf["dim_x"]), (inf["dim_y"] // 2, inf["dim_x"] // 2 + 1), (inf["dim_y"] // 4 or 1, inf["dim_x"] // 8 or 1), (1000, 1000)):
            im = Image.open(io.BytesIO(mixed["files"][i]))
            im.draft(None, (size[1], size[0]))
            s = b.reduce_for(i, size)
            assert s in (1, 2, 4, 8) and im.size == (-(-inf["dim_x"] // s), -(-inf["dim_y"] // s)), (i, size, s, im.size)


def test_reduce_1_is_the_full_size_render_and_the_other_paths_give_what_they_gave(J, torch, mixed):
    b = mixed["b"]; n = len(b); models = mixed["models"]
    before = [t.cpu().numpy().copy() for t in b.to_torch(layout="HWC")]
    full = b.to_torch(layout="HWC", pixels="libjpeg")
    one = b.to_torch(layout="HWC", pixels="libjpeg", reduce=1)
    for i in range(n):
        assert np.array_equal(full[i].cpu().numpy(), models[i, 1]) and np.array_equal(one[i].cpu().numpy(), models[i, 1]), i
    # the raw call at denom 1 writes what jsnoop_batch_pack_ijg writes, guard bands included
    sizes = [models[i, 1].size for i in range(n)]
    a1, a2 = Arena(torch, sizes, lead=3), Arena(torch, sizes, lead=3)
    torch.cuda.synchronize()
    spec = T.make_spec(J, "HWC", "uint8")
    assert raw_scaled(J, b, spec, 1, list(range(n)), [(a1.ptr(k), 0, 0) for k in range(n)]) == 0, J.last_error()
    assert T.raw_ijg(J, b, spec, list(range(n)), [(a2.ptr(k), 0, 0) for k in range(n)]) == 0, J.last_error()
    torch.cuda.synchronize()
    assert bool((a1.buf == a2.buf).all().item()) and not a1.untouched()
    b.to_torch(layout="CHW", pixels="libjpeg", reduce=8)
    after = b.to_torch(layout="HWC")
    assert all(np.array_equal(x, y.cpu().numpy()) for x, y in zip(before, after))


# ------------------------------------------------------------------------------------------------ the deal: a wave walks several units and records
@pytest.mark.parametrize("s", S.SCALES)
def test_calls_of_so_many_units_that_a_wave_walks_several_units_and_records(J, torch, harness, capsys, s):
    """Every test above stays far below RS_WAVES * 6 * compute units units, where a workgroup's share is four units and a wave takes one.  Here the call is
    sized from the device (tests/deal_cases.py; tests/test_deal_cases.py proves the lists on the CPU): a share of twelve units, every wave takes three
    one after the other through the same LDS -- three planes, the 4:2:2 halo columns, load tile and workspace --, reloads its record, passes over one-unit
    records, and sees H, V, ncomp, bpm, run, ny and nc change from one unit to the next: grey behind colour, 4:4:4 behind 4:2:0, 4:2:0 behind 4:2:2 and,
    where 4:2:2 is filtered (1/2, 1/4), chroma planes two and three samples wide behind a filtered unit (D.ADJACENT).  Fourteen distinct pictures, their
    widths stated in units, each once in the batch and listed once per record with a destination of its own shape; a baseline batch rendered HWC uint8
    and, at 1/2, a progressive one CHW uint8.  Everything against the model of the batch's own arena, and that against Pillow's reduced decode."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    K = D.KERNELS["render_scaled"]; m = 8 // s
    recs = D.render_scaled_records(cus, s)
    c = D.census_of("render_scaled", str(s), recs, cus)
    with capsys.disabled():
        print("\nk_render_ijg_scaled 1/%d, %d compute units: %s; %d records of %d pictures" % (s, cus, D.summary(c), len(recs), len({r.pic for r in recs})))
    assert D.missing(c, K["waves"], **D.conditions("render_scaled", str(s))) == [] and D.adjacency_missing(recs, cus, s) == [], D.summary(c)
    distinct = sorted({r.pic for r in recs}); image = {p: i for i, p in enumerate(distinct)}
    for progressive, layout in ((0, "HWC"), (1, "CHW"))[:2 if s == 2 else 1]:
        files = T.deal_files(harness, distinct, progressive)
        b = T.decoded_batch(J, [f for f, _own in files])
        try:
            models = models_of(J, torch, b, (s,))
            for i, (f, own) in enumerate(files):
                assert not own or np.array_equal(models[i, s], S.pillow_reduced(f, s)), (distinct[i], s)
            for r in recs:                                            # the units the census counted are the units of the call
                inf = b.info(image[r.pic]); H = inf["mcu_w"] // 8; run = K["unit"] // (H * m)
                assert r.units == inf["mcu_ymax"] * -(-inf["mcu_xmax"] // run) and sum(r.sizes) == inf["mcu_xmax"] * inf["mcu_ymax"] * H * m, (r.pic, s)
            T.deal_render_and_check(J, torch, recs, image, lambda i: models[i, s], lambda spec, images, dsts: raw_scaled(J, b, spec, s, images, dsts), layout, "uint8", cus, s,
                                    "deal at 1/%d, %s batch" % (s, "progressive" if progressive else "baseline"))
        finally:
            b.close()


# ------------------------------------------------------------------------------------------------ source kinds
def test_progressive_files_and_files_with_restart_intervals(J, torch, harness):
    sizes = [(50, 70), (130, 21), (33, 31), (17, 9)]
    prog = [IC.pillow_file(IC.noise(w, h, 40 + k), IC.MODES[k % 4], 85, progressive=True) for k, (w, h) in enumerate(sizes)]
    rst = [harness.synth_jpeg(width=141, height=93, hs=2, vs=1, restart_interval=3, seed=5), harness.synth_jpeg(width=200, height=120, quality=25, restart_interval=7, seed=6),
           harness.synth_jpeg(width=97, height=61, gray=1, restart_interval=1, seed=7)]
    for files, pillow in ((prog, True), (rst, False)):            # (the generator's files are not an encoder's: nothing bounds their IDCT results by 511)
        b = T.decoded_batch(J, files)
        try:
            models = models_of(J, torch, b)
            for s in S.SCALES:
                if pillow:
                    for i, f in enumerate(files):
                        assert np.array_equal(models[i, s], S.pillow_reduced(f, s)), (i, s)
                render_and_check(J, torch, b, models, s, "HWC", "uint8", list(range(len(files))), what="progressive" if files is prog else "restart")
        finally:
            b.close()


def test_dc_only_fast_form_is_decoded_once_more_and_rendered_from_a_dc_only_arena(J, torch, harness):
    files = [harness.synth_jpeg(width=100, height=75, hs=2, vs=2, restart_interval=3 * (k % 2), seed=500 + k) for k in range(3)]
    b = T.decoded_batch(J, files, decode_ac=False)
    try:
        assert b.last_form() == 2
        ar = Arena(torch, [25 * 19 * 3] * 3)
        torch.cuda.synchronize()
        assert raw_scaled(J, b, T.make_spec(J, "HWC", "uint8"), 4, [0, 1, 2], [(ar.ptr(k), 0, 0) for k in range(3)]) == 0, J.last_error()
        assert b.last_form() == 1, "behind a fast-form decode the call decodes again in the generic form"
        keep = T.arenas_now(J, torch, b, [0, 1, 2])
        torch.cuda.synchronize()
        for i, a in T.arenas_of(b, keep).items():
            assert not a[:, 1:].any()                                 # a DC-only arena
            ar.place(i, S.render(a, 100, 75, IC.HV["420"], 4)[0], "HWC", 75, 0)
        ar.explain("DC-only", [(i, 4, "HWC", 1, 75, 0, (16, 16)) for i in range(3)])
    finally:
        b.close()


def test_the_wild_file_wraps_as_the_model_does(J, torch):
    data = IC.wild_file()
    b = T.decoded_batch(J, [data, data])
    try:
        models = models_of(J, torch, b)
        a, w, h, hv = M.arena_of_file(data)
        for s in S.SCALES:
            assert np.array_equal(models[0, s], S.render(a, w, h, hv, s)[0])     # the device's arena is the codec's
            render_and_check(J, torch, b, models, s, "HWC", "uint8", [0, 1], what="wild")
    finally:
        b.close()


def test_a_damaged_file_before_and_after_sync(J, torch, harness):
    """Before jsnoop_batch_sync the render sees what the parallel path left, after it the repaired blocks: each time the model of the arena a
    jsnoop_batch_pack_coefs enqueued right in front of it read."""
    bases = F.bases(harness)
    hurt = [F.mutate(harness, np.random.default_rng(seed), bases[base])[0] for base, seed in T.DAMAGED]
    b = J.JpegBatch()
    try:
        for f in (bases[0], hurt[0], hurt[1], bases[1]):
            b.add_jpeg(f)
        b.upload(); b.decode()
        images = [0, 1, 2, 3]
        lib = J.load()
        for phase in ("before sync", "after sync"):
            for s in S.SCALES:
                dims = []
                for i in images:
                    w, h = C.c_uint(0), C.c_uint(0)
                    assert lib.jsnoop_batch_ijg_scaled_size(b._h, i, s, C.byref(w), C.byref(h)) == 0, J.last_error()
                    dims.append((h.value, w.value))
                ar = Arena(torch, [h * w * 3 for h, w in dims])
                keep = T.arenas_now(J, torch, b, images)
                assert raw_scaled(J, b, T.make_spec(J, "HWC", "uint8"), s, images, [(ar.ptr(k), 0, 0) for k in range(4)]) == 0, J.last_error()
                torch.cuda.synchronize()
                meta = []
                for i, a in T.arenas_of(b, keep).items():
                    w, h, hv, _ = T.geometry(b, i)
                    px = S.render(a, w, h, hv, s)[0]
                    assert px.shape[:2] == dims[i]
                    ar.place(i, px, "HWC", px.shape[1] * 3, 0)
                    meta.append((i, s, "HWC", 1, px.shape[1] * 3, 0, (8 * hv[0][0], 8 * hv[0][1])))
                ar.explain(phase, meta)
            b.sync()
        assert b.info(1)["flags"] != 0 and b.info(2)["flags"] != 0
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing_and_write_nothing(J, torch, harness, mixed):
    f440 = harness.synth_jpeg(width=64, height=48, hs=1, vs=2, seed=7)
    good = mixed["files"][of_mode(mixed, "420")[9]]               # 33 x 31
    b = T.decoded_batch(J, [good, f440])
    try:
        lib = J.load()
        w, h = C.c_uint(0), C.c_uint(0)
        assert b.ijg_scaled_size(0, 2) == (16, 17) and b.ijg_scaled_size(0, 8) == (4, 5) and b.ijg_scaled_size(0, 1) == (31, 33)
        assert lib.jsnoop_batch_ijg_scaled_size(b._h, 1, 2, C.byref(w), C.byref(h)) == -1 and "luma sampling 1 x 2" in J.last_error()
        assert lib.jsnoop_batch_ijg_scaled_size(b._h, 0, 3, C.byref(w), C.byref(h)) == -1 and "denom = 3" in J.last_error()
        assert lib.jsnoop_batch_ijg_scaled_size(b._h, 2, 2, C.byref(w), C.byref(h)) == -1 and "out of range" in J.last_error()
        u8h, u8c, f32h, f32c = T.make_spec(J, "HWC", "uint8"), T.make_spec(J, "CHW", "uint8"), T.make_spec(J, "HWC", "float32"), T.make_spec(J, "CHW", "float32")
        assert lib.jsnoop_batch_pack_ijg_scaled_bytes(b._h, C.byref(u8h), 2, 0) == 16 * 17 * 3 and lib.jsnoop_batch_pack_ijg_scaled_bytes(b._h, C.byref(f32c), 8, 0) == 4 * 5 * 12
        assert lib.jsnoop_batch_pack_ijg_scaled_bytes(b._h, C.byref(u8h), 1, 0) == 33 * 31 * 3
        assert lib.jsnoop_batch_pack_ijg_scaled_bytes(b._h, C.byref(u8h), 5, 0) == 0 and "denom = 5" in J.last_error()
        assert lib.jsnoop_batch_pack_ijg_scaled_bytes(b._h, C.byref(u8h), 2, 1) == 0 and lib.jsnoop_batch_pack_ijg_scaled_bytes(b._h, C.byref(u8h), 2, 2) == 0
        ar = Arena(torch, [64 * 48 * 12, 64 * 48 * 12])
        p = ar.ptr(0)
        torch.cuda.synchronize()
        bad_layout, bad_dtype, too_long = T.make_spec(J, "HWC", "uint8"), T.make_spec(J, "HWC", "uint8"), T.make_spec(J, "HWC", "uint8")
        bad_layout.layout, bad_dtype.dtype, too_long.struct_size = 2, 7, C.sizeof(J.capi.PackSpec) + 8
        w2, h2 = 17, 16                                             # the picture at 1/2
        cases = [("a 4:4:0 file in the list", u8h, 2, [0, 1], [(p, 0, 0), (ar.ptr(1), 0, 0)], "image 1: luma sampling 1 x 2"),
                 ("a 4:4:0 file in the list at 1/1", u8h, 1, [0, 1], [(p, 0, 0), (ar.ptr(1), 0, 0)], "image 1: luma sampling 1 x 2"),
                 ("denom 0", u8h, 0, [0], [(p, 0, 0)], "denom = 0"), ("denom 3", u8h, 3, [0], [(p, 0, 0)], "denom = 3"), ("denom 16", u8h, 16, [0], [(p, 0, 0)], "denom = 16"),
                 ("index past the end", u8h, 4, [2], [(p, 0, 0)], "out of range"), ("negative index", u8h, 8, [-1], [(p, 0, 0)], "out of range"),
                 ("NULL pointer", u8h, 2, [0], [(0, 0, 0)], "NULL"), ("row_pitch below dense", u8h, 2, [0], [(p, w2 * 3 - 1, 0)], "row_pitch"),
                 ("plane_pitch below dense", u8c, 2, [0], [(p, w2, w2 * h2 - 1)], "plane_pitch"), ("float pointer", f32h, 4, [0], [(p + 2, 0, 0)], "multiples of 4"),
                 ("float row_pitch", f32c, 2, [0], [(p, w2 * 4 + 2, 0)], "multiples of 4"), ("unknown layout", bad_layout, 2, [0], [(p, 0, 0)], "layout"),
                 ("unknown dtype", bad_dtype, 4, [0], [(p, 0, 0)], "dtype"), ("struct_size of a later version", too_long, 8, [0], [(p, 0, 0)], "struct_size")]
        for what, spec, denom, images, dsts, word in cases:
            assert raw_scaled(J, b, spec, denom, images, dsts) == -1, what
            assert word in J.last_error() and "pack_ijg" in J.last_error(), (what, J.last_error())
        with pytest.raises(RuntimeError):
            b.to_torch(pixels="libjpeg", reduce=2)
        for kw in (dict(reduce=2), dict(reduce=[2]), dict(reduce=[1]), dict(pixels="libjpeg", reduce=3), dict(pixels="libjpeg", reduce=[2, 2]), dict(pixels="libjpeg", reduce=2, size=(8, 8))):
            with pytest.raises(ValueError):
                b.to_torch(images=[0], **kw)
        with pytest.raises(ValueError):                             # stack=True needs equal REDUCED sizes
            b.to_torch(images=[0, 0], pixels="libjpeg", reduce=[2, 4], stack=True)
        nb = J.JpegBatch()
        try:
            nb.add_jpeg(good)
            assert raw_scaled(J, nb, u8h, 2, [0], [(p, 0, 0)]) == -1 and "not been decoded" in J.last_error()
            nb.upload()
            assert raw_scaled(J, nb, u8h, 2, [0], [(p, 0, 0)]) == -1 and "not been decoded" in J.last_error()
        finally:
            nb.close()
        torch.cuda.synchronize()
        assert ar.untouched()
        assert raw_scaled(J, b, u8h, 2, None, []) == 0              # n == 0 is accepted
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ paths
def test_torch_raw_pointer_and_cpp_paths(J, torch, mixed, tmp_path):
    b = mixed["b"]; models = mixed["models"]; i420 = of_mode(mixed, "420"); i422 = of_mode(mixed, "422")
    a, c, d = i420[9], i420[10], i422[11]                          # 33 x 31, 50 x 70, 130 x 21
    # torch: stacked, padded, into out=, float with scale and bias, CHW
    t = b.to_torch(images=[a, a], layout="CHW", stack=True, pixels="libjpeg", reduce=2)
    assert tuple(t.shape) == (2, 3, 16, 17) and np.array_equal(t[1].cpu().numpy(), T.form(models[a, 2], "CHW", "uint8"))
    t = b.to_torch(images=[c, d], layout="HWC", pad_to=(20, 40), dtype=torch.float32, scale=SCALE, bias=BIAS, bgr=True, pixels="libjpeg", reduce=4)
    assert np.array_equal(t[0, :18, :13].cpu().numpy(), T.form(models[c, 4], "HWC", "float32", True, SCALE, BIAS)) and not t[0, 18:].any() and not t[0, :, 13:].any() and not t[1, 6:].any()
    out = torch.full((1, 12, 20, 3), 7, dtype=torch.uint8, device="cuda")
    assert b.to_torch(images=[c], layout="HWC", out=out, pixels="libjpeg", reduce=8) is out
    assert np.array_equal(out[0, :9, :7].cpu().numpy(), models[c, 8]) and bool((out[0, 9:] == 7).all()) and bool((out[0, :, 7:] == 7).all())
    # the raw pointer: what render_and_check does everywhere above
    # C++: tests/cpp/render_scaled_demo.cpp through CJPEGsnoopCoreGpu::BatchPackIjgScaled
    exe = str(tmp_path / "render_scaled_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "render_scaled_demo.cpp"),
                           "-L" + os.path.join(ROOT, "jpegsnoop_amd"), "-ljsnoop_gpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "jpegsnoop_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    pick = [a, c, d, i420[3]]
    paths = []
    for k, i in enumerate(pick):
        paths.append(str(tmp_path / ("in%d.jpg" % k)))
        open(paths[-1], "wb").write(mixed["files"][i])
    lines = [ln.split() for ln in subprocess.check_output([exe, str(tmp_path), "4"] + paths, text=True).split("\n") if ln]
    assert [ln[0] for ln in lines] == ["3", "2", "1", "0"]
    for k, i in enumerate(pick):
        got = np.fromfile(str(tmp_path / ("out%d.rgb" % k)), np.uint8)
        assert [int(x) for x in lines[3 - k][1:3]] == [models[i, 4].shape[1], models[i, 4].shape[0]] and np.array_equal(got, models[i, 4].reshape(-1)), i
