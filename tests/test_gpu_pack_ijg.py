"""-m gpu: jsnoop_batch_pack_ijg / k_render_ijg (jsnoop_render.hip) and JpegBatch.to_torch(pixels="libjpeg") -- a decoded batch rendered as libjpeg's
pixels into caller-owned device memory.

Every comparison is exact (np.array_equal) against tests/ijg_model.py fed the batch's OWN arena -- read through jsnoop_batch_pack_coefs at that moment, the
cumulative DC in slot 0 -- and, for Pillow's files, against Pillow's decode as well.  Raw calls write into an arena of 0xA5 bytes with guard bands around
and between the destinations and in every pitch gap, and the whole arena is compared with what the model predicts: a stray write anywhere shows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import coef_model as CM
import deal_cases as D
import fuzz_util as F
import ijg_cases as IC
import ijg_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64
SCALE, BIAS = (1 / 255, 1 / 3, 0.7), (-0.485, 1 / 7, 1e-3)                                   # none of them a float32
FORMS = [("HWC", "uint8"), ("CHW", "uint8"), ("HWC", "float32"), ("CHW", "float32")]


# ------------------------------------------------------------------------------------------------ helpers
@pytest.fixture(scope="module")
def J():
    import jpegsnoop_amd
    jpegsnoop_amd.load()
    return jpegsnoop_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def decoded_batch(J, files, **kw):
    b = J.JpegBatch(**kw)
    for f in files:
        b.add_jpeg(f)
    b.upload(); b.decode(); b.sync()
    return b


def make_spec(J, layout, dtype, bgr=False, scale=None, bias=None):
    s = J.capi.PackSpec()
    J.load().jsnoop_pack_spec_defaults(C.byref(s))
    s.layout = J.capi.PACK_CHW if layout == "CHW" else J.capi.PACK_HWC
    s.dtype = J.capi.PACK_F32 if dtype == "float32" else J.capi.PACK_U8
    s.bgr = int(bgr)
    for c in range(3):
        if scale is not None:
            s.scale[c] = scale[c]
        if bias is not None:
            s.bias[c] = bias[c]
    return s


def raw_ijg(J, b, spec, images, dsts):
    """jsnoop_batch_pack_ijg as a C caller makes it: dsts = [(ptr, row_pitch, plane_pitch)].  Returns the call's value; does not wait."""
    n = len(dsts)
    arr = (J.capi.PackDst * max(n, 1))(*[J.capi.PackDst(p, rp, pp) for p, rp, pp in dsts])
    ind = (C.c_int * max(n, 1))(*images) if images is not None else None
    return J.load().jsnoop_batch_pack_ijg(b._h, C.byref(spec), ind, n, arr)


def geometry(b, i):
    inf = b.info(i)
    hv = [(1, 1)] if inf["ncomp"] == 1 else [(inf["mcu_w"] // 8, inf["mcu_h"] // 8), (1, 1), (1, 1)]
    return inf["dim_x"], inf["dim_y"], hv, CM.Geometry(hv, inf["mcu_xmax"], inf["mcu_ymax"])


def arenas_now(J, torch, b, images):
    """The arena rows of the listed images with the cumulative DC in slot 0, as the device holds them NOW: one raw jsnoop_batch_pack_coefs (blocks, int16,
    natural order) on the batch's stream -- nothing is waited for before it, the device is waited for after it."""
    spec = J.capi.CoefSpec(); J.load().jsnoop_coef_spec_defaults(C.byref(spec))
    dsts, idx, keep = [], [], []
    for i in images:
        _w, _h, hv, geo = geometry(b, i)
        for c in range(len(hv)):
            bw, bh = geo.grid(c)
            t = torch.zeros((bh, bw, 64), dtype=torch.int16, device="cuda")
            keep.append((i, c, t)); idx.append(i); dsts.append(J.capi.CoefDst(t.data_ptr(), 0, 0, c, 0))
    torch.cuda.synchronize()
    arr = (J.capi.CoefDst * len(dsts))(*dsts)
    assert J.load().jsnoop_batch_pack_coefs(b._h, C.byref(spec), (C.c_int * len(idx))(*idx), len(idx), arr) == 0, J.last_error()
    return keep


def arenas_of(b, keep):
    out = {}
    for i, c, t in keep:
        _w, _h, hv, geo = geometry(b, i)
        a = out.setdefault(i, np.zeros((geo.nblocks, 64), np.int16))
        a[geo.arena_index(c)] = t.cpu().numpy()
    return out


def models_of(J, torch, b, images=None):
    """{image: model pixels [H][W][3]} from the batch's own arena."""
    images = list(range(len(b))) if images is None else images
    keep = arenas_now(J, torch, b, images)
    torch.cuda.synchronize()
    out = {}
    for i, a in arenas_of(b, keep).items():
        w, h, hv, _ = geometry(b, i)
        px, _peak = M.render(a, w, h, hv)
        px.setflags(write=False)
        out[i] = px
    return out


def form(px, layout, dtype, bgr=False, scale=None, bias=None):
    """Model pixels [H][W][3] R G B -> the destination's elements."""
    out = px[..., ::-1] if bgr else px
    if dtype == "float32":
        prod = out.astype(np.float32) * np.asarray(scale or (1, 1, 1), np.float32).reshape(1, 1, 3)       # rounded once
        out = prod + np.asarray(bias or (0, 0, 0), np.float32).reshape(1, 1, 3)                          # rounded again
        assert out.dtype == np.float32
    out = np.ascontiguousarray(out)
    return np.ascontiguousarray(out.transpose(2, 0, 1)) if layout == "CHW" else out


class Arena:
    """One device allocation of 0xA5 bytes holding every destination of a call, and the bytes the model says it must hold afterwards."""

    def __init__(self, torch, sizes, lead=0):
        """lead: bytes past a 16-byte boundary every destination starts at, or one number per destination."""
        self.offs, pos = [], GUARD
        for k, nb in enumerate(sizes):
            pos = (pos + 15) // 16 * 16 + (lead[k] if isinstance(lead, (list, tuple)) else lead)
            self.offs.append(pos)
            pos += nb + GUARD
        self.buf = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.expect = np.full(pos, 0xA5, np.uint8)
        self.sizes = sizes

    def ptr(self, k):
        return self.buf.data_ptr() + self.offs[k]

    def place(self, k, model, layout, rp, pp):
        raw = np.ascontiguousarray(model).view(np.uint8)
        reg = self.expect[self.offs[k]:self.offs[k] + self.sizes[k]]
        if layout == "HWC":
            h = model.shape[0]; row = raw.reshape(h, -1)
            reg[:h * rp].reshape(h, rp)[:, :row.shape[1]] = row
        else:
            h = model.shape[1]
            for c in range(3):
                row = raw.reshape(3, h, -1)[c]
                reg[c * pp:c * pp + h * rp].reshape(h, rp)[:, :row.shape[1]] = row

    def check(self, what):
        got = self.buf.cpu().numpy()
        if not np.array_equal(got, self.expect):
            bad = int(np.flatnonzero(got != self.expect)[0])
            k = max([i for i, o in enumerate(self.offs) if o <= bad], default=-1)
            raise AssertionError("%s: first wrong byte at arena offset %d (destination %d + %d): got 0x%02x, want 0x%02x; %d bytes differ"
                                 % (what, bad, k, bad - self.offs[k] if k >= 0 else bad, got[bad], self.expect[bad], int((got != self.expect).sum())))

    def untouched(self):
        return bool((self.buf == 0xA5).all().item())


def render_and_check(J, torch, b, models, layout, dtype, images, bgr=False, lead=0, row_extra=0, plane_extra=0, scale=None, bias=None, what=""):
    """One raw call for `images` with the given destination shape, then the whole arena against the model."""
    elem = 4 if dtype == "float32" else 1
    geo = []
    for i in images:
        h, w = models[i].shape[:2]
        rp = w * elem * (3 if layout == "HWC" else 1) + row_extra
        pp = h * rp + plane_extra
        geo.append((rp, pp, h * rp if layout == "HWC" else 3 * pp))
    ar = Arena(torch, [g[2] for g in geo], lead)
    for k, i in enumerate(images):
        ar.place(k, form(models[i], layout, dtype, bgr, scale, bias), layout, geo[k][0], geo[k][1])
    dense = row_extra == 0 and plane_extra == 0
    dsts = [(ar.ptr(k), 0 if dense and k % 2 else geo[k][0], 0 if dense and k % 2 else (geo[k][1] if layout == "CHW" else 0)) for k in range(len(images))]
    torch.cuda.synchronize()                                      # (the fill above ran on torch's stream, the render runs on the batch's)
    assert raw_ijg(J, b, make_spec(J, layout, dtype, bgr, scale, bias), images, dsts) == 0, J.last_error()
    torch.cuda.synchronize()
    ar.check("%s %s %s bgr=%d lead=%d row+%d plane+%d" % (what, layout, dtype, bgr, lead, row_extra, plane_extra))


# ------------------------------------------------------------------------------------------------ the four layouts against the model and Pillow
@pytest.fixture(scope="module")
def mixed(J, torch):
    """One mixed batch per layout over the size list (baseline); the model of every image from the batch's own arena, computed once."""
    out = {}
    for mode in IC.MODES:
        files = [IC.pillow_file(IC.noise(w, h, 17 * k + 3), mode, (10, 50, 85, 100)[k % 4]) for k, (w, h) in enumerate(IC.SIZES)]
        b = decoded_batch(J, files)
        out[mode] = dict(b=b, files=files, models=models_of(J, torch, b))
    yield out
    for v in out.values():
        v["b"].close()


@pytest.mark.parametrize("mode", IC.MODES)
def test_every_size_of_every_layout_is_the_models_and_pillows(J, torch, mixed, mode):
    m = mixed[mode]; b = m["b"]; n = len(b)
    assert all(b.ijg_renderable(i) for i in range(n))
    for i, f in enumerate(m["files"]):                            # the model on the device's arena is Pillow's decode of the file
        assert np.array_equal(m["models"][i], IC.pillow_pixels(f)), (mode, IC.SIZES[i])
    render_and_check(J, torch, b, m["models"], "HWC", "uint8", list(range(n)), what=mode)
    got = b.to_torch(layout="HWC", pixels="libjpeg")
    for i, f in enumerate(m["files"]):
        assert np.array_equal(got[i].cpu().numpy(), IC.pillow_pixels(f)), (mode, IC.SIZES[i])


# ------------------------------------------------------------------------------------------------ unit and MCU seams
def seam_sizes(mode):
    mw, mh = 16, (16 if mode == "420" else 8)
    ws = [m * mw + d for m in (7, 8, 9, 28) for d in (-1, 0, 1)]
    hs = [r * mh + d for r in (1, 2, 3) for d in (-1, 0, 1)]
    out = [(w, hs[(2 * k + 1) % len(hs)]) for k, w in enumerate(ws)] + [(ws[(5 * k) % len(ws)], h) for k, h in enumerate(hs)]
    return out + [(mw, 3 * mh + 1), (mw - 1, 2 * mh), (9 * mw + 2, mh), (8 * mw, mh - 1), (3, 3 * mh), (4, mh + 1), (5, 2 * mh + 1), (6, mh)]   # one MCU wide / high; dw = 2, 2, 3, 3


@pytest.mark.parametrize("mode", ["420", "422"])
def test_the_filter_crosses_unit_and_mcu_row_seams(J, torch, mode):
    sizes = seam_sizes(mode)
    files = [IC.pillow_file(IC.noise(w, h, 900 + k), mode, 92) for k, (w, h) in enumerate(sizes)]
    b = decoded_batch(J, files)
    try:
        models = models_of(J, torch, b)
        for i in (0, 5, len(sizes) - 1, len(sizes) - 3):
            assert np.array_equal(models[i], IC.pillow_pixels(files[i])), sizes[i]
        render_and_check(J, torch, b, models, "HWC", "uint8", list(range(len(sizes))), what="seams " + mode)
        render_and_check(J, torch, b, models, "CHW", "uint8", list(range(len(sizes))), what="seams " + mode)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ store forms
@pytest.mark.parametrize("layout,dtype", FORMS)
@pytest.mark.parametrize("bgr", [False, True])
def test_every_store_form(J, torch, mixed, layout, dtype, bgr):
    sb = (None, None) if dtype == "uint8" else (SCALE, BIAS)
    for mode in ("420", "grey"):
        m = mixed[mode]
        render_and_check(J, torch, m["b"], m["models"], layout, dtype, list(range(len(m["b"]))), bgr=bgr, scale=sb[0], bias=sb[1], what="forms " + mode)


@pytest.mark.parametrize("lead", [0, 1, 3, 15])
def test_uint8_destinations_at_any_byte_with_pitches_above_the_row(J, torch, mixed, lead):
    m = mixed["422"]; n = len(m["b"])
    render_and_check(J, torch, m["b"], m["models"], "HWC", "uint8", list(range(n)), lead=lead, row_extra=0, what="alignment")
    render_and_check(J, torch, m["b"], m["models"], "HWC", "uint8", list(range(n)), lead=lead, row_extra=13, what="alignment")
    render_and_check(J, torch, m["b"], m["models"], "CHW", "uint8", list(range(n)), lead=lead, row_extra=3, plane_extra=5, bgr=True, what="alignment")


def test_float_destinations_with_pitched_rows_and_planes(J, torch, mixed):
    m = mixed["444"]; n = len(m["b"])
    render_and_check(J, torch, m["b"], m["models"], "HWC", "float32", list(range(n)), lead=8, row_extra=20, scale=SCALE, bias=BIAS, what="pitched float")
    render_and_check(J, torch, m["b"], m["models"], "CHW", "float32", list(range(n)), lead=4, row_extra=8, plane_extra=12, scale=SCALE, bias=BIAS, what="pitched float")


def test_a_shuffled_subset_and_an_image_listed_twice(J, torch, mixed):
    m = mixed["420"]; n = len(m["b"])
    order = [int(i) for i in np.random.default_rng(4).permutation(n)[:9]] + [11, 2, 11]
    render_and_check(J, torch, m["b"], m["models"], "HWC", "uint8", order, what="shuffled")
    render_and_check(J, torch, m["b"], m["models"], "CHW", "float32", order, scale=SCALE, bias=BIAS, what="shuffled")


# ------------------------------------------------------------------------------------------------ the deal: a wave walks several units and records
def deal_files(harness, distinct, progressive):
    """[(file, Pillow's own)] -- one file per distinct picture of a deal list, in its order (a batch holds one kind of file, so there are two lists).
    Baseline: Pillow's files of seeded noise at varying quality, and from the generator, with restart intervals, the long 4:2:2 picture and a grey one of
    three MCU rows.  Progressive: Pillow's, every one."""
    out = []
    for k, pic in enumerate(distinct):
        mode, w, h = pic
        if not progressive and pic == ("grey", 13, 24):
            out.append((harness.synth_jpeg(width=w, height=h, gray=1, restart_interval=1, seed=60 + k), False))
        elif not progressive and mode == "422" and h >= 8 * 30:
            out.append((harness.synth_jpeg(width=w, height=h, hs=2, vs=1, quality=60, restart_interval=5, seed=60 + k), False))
        else:
            # (Pillow gives libjpeg one buffer of width x height bytes for a progressive file: noise in colour passes it above quality 60)
            out.append((IC.pillow_file(IC.noise(w, h, 300 + k), mode, (10, 40, 25, 60)[k % 4] if progressive else IC.QUALITIES[k % 4], progressive=bool(progressive)), True))
    assert progressive or sum(not own for _f, own in out) == 2
    return out


def deal_where(ar, recs, image, meta, cus, denom):
    """None when the arena holds what the model says, or the first wrong byte as record, picture, pixel, MCU, unit -- and where the deal put that unit."""
    got = ar.buf.cpu().numpy()
    if np.array_equal(got, ar.expect):
        return None
    bad = int(np.flatnonzero(got != ar.expect)[0])
    k = max([i for i, o in enumerate(ar.offs) if o <= bad], default=-1)
    where = "outside every destination (arena offset %d, destination %d starts at %d)" % (bad, k, ar.offs[k] if k >= 0 else 0)
    if k >= 0 and bad - ar.offs[k] < ar.sizes[k]:
        layout, elem, rp, pp, w, h = meta[k]; o = bad - ar.offs[k]; pic = recs[k].pic
        if layout == "HWC":
            y, x, ch = o // rp, (o % rp) // (3 * elem), ((o % rp) // elem) % 3
        else:
            ch, y, x = o // pp, (o % pp) // rp, ((o % pp) % rp) // elem
        gap = " -- in a pitch gap, the unit is that of the nearest pixel" if (x >= w or y >= h) else ""
        x, y = min(x, w - 1), min(y, h - 1)
        H, V, _mx, _my, run, runs = D.render_grid(pic, denom); m = 8 // denom
        mcu_x, my = x // (H * m), y // (V * m); lu = my * runs + mcu_x // run
        where = "record %d, picture %s (image %d) at 1/%d, channel %d, pixel (x %d, y %d)%s of MCU (%d, %d): unit lu = %d (my %d, m0 %d), destination byte %d; %s" % (
            k, pic, image[pic], denom, ch, x, y, gap, mcu_x, my, lu, my, mcu_x // run * run, o,
            D.deal_place(recs, cus, "render" if denom == 1 else "render_scaled", "any", k, lu))
    return "first wrong byte in %s: got 0x%02x, want 0x%02x; %d bytes differ" % (where, got[bad], ar.expect[bad], int((got != ar.expect).sum()))


def deal_render_and_check(J, torch, recs, image, model_of, call, layout, dtype, cus, denom, what, scale=None, bias=None):
    """One raw call (call(spec, images, dsts)) with one destination per record of a deal list, then the whole arena against the models.  Records of the same
    picture are not interchangeable: every third destination is dense (pitches passed as 0), the others have row and plane pitches and all have leads that
    vary with the record index (float32: multiples of 4)."""
    elem = 4 if dtype == "float32" else 1
    formed = {p: form(model_of(i), layout, dtype, False, scale, bias) for p, i in image.items()}
    geo, lead, meta = [], [], []
    for k, r in enumerate(recs):
        h, w = model_of(image[r.pic]).shape[:2]
        dense = k % 3 == 0
        rp = w * elem * (3 if layout == "HWC" else 1) + (0 if dense else (1 + k % 5) * elem)
        pp = h * rp + (0 if dense else (k % 4) * elem)
        geo.append((rp, pp, h * rp if layout == "HWC" else 3 * pp, dense)); lead.append(k % 16 if elem == 1 else 4 * (k % 4))
        meta.append((layout, elem, rp, pp, w, h))
    ar = Arena(torch, [g[2] for g in geo], lead)
    for k, r in enumerate(recs):
        ar.place(k, formed[r.pic], layout, geo[k][0], geo[k][1])
    dsts = [(ar.ptr(k), 0 if dense else rp, 0 if dense or layout == "HWC" else pp) for k, (rp, pp, _nb, dense) in enumerate(geo)]
    torch.cuda.synchronize()                                      # (the fill above ran on torch's stream, the render runs on the batch's)
    assert call(make_spec(J, layout, dtype, False, scale, bias), [image[r.pic] for r in recs], dsts) == 0, J.last_error()
    torch.cuda.synchronize()
    wrong = deal_where(ar, recs, image, meta, cus, denom)
    assert wrong is None, "%s %s %s: %s" % (what, layout, dtype, wrong)


def test_calls_of_so_many_units_that_a_wave_walks_several_units_and_records(J, torch, harness, capsys):
    """Every test above stays far below RN_WAVES * 6 * compute units units, where a workgroup's share is four units and a wave takes one.  Here the call is
    sized from the device (tests/deal_cases.py; tests/test_deal_cases.py proves the lists on the CPU): a share of twelve units, every wave takes three
    one after the other through the same LDS -- luma rectangle, chroma planes, halo columns and rows, transpose tile --, reloads its record, passes over
    one-unit records, and takes a grey unit behind a colour one, 4:4:4 behind 4:2:0, 4:2:0 behind 4:2:2, a chroma plane two samples wide behind a
    filtered unit, a first and a last MCU row behind an interior unit of 4:2:0 (D.ADJACENT).  Fourteen distinct pictures, each once in the batch and
    listed once per record with a destination of its own shape; a baseline batch rendered HWC uint8, a progressive one CHW float32.  Everything
    against the model of the batch's own arena, and that against Pillow."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    recs = D.render_records(cus)
    c = D.census_of("render", "any", recs, cus)
    with capsys.disabled():
        print("\nk_render_ijg, %d compute units: %s; %d records of %d pictures" % (cus, D.summary(c), len(recs), len({r.pic for r in recs})))
    assert D.missing(c, D.KERNELS["render"]["waves"], **D.conditions("render", "any")) == [] and D.adjacency_missing(recs, cus) == [], D.summary(c)
    distinct = sorted({r.pic for r in recs}); image = {p: i for i, p in enumerate(distinct)}
    for progressive, (layout, dtype), sb in ((0, ("HWC", "uint8"), (None, None)), (1, ("CHW", "float32"), (SCALE, BIAS))):
        files = deal_files(harness, distinct, progressive)
        b = decoded_batch(J, [f for f, _own in files])
        try:
            models = models_of(J, torch, b)
            for i, (f, own) in enumerate(files):
                assert not own or np.array_equal(models[i], IC.pillow_pixels(f)), distinct[i]
            for r in recs:                                            # the units the census counted are the units of the call
                inf = b.info(image[r.pic])
                assert r.units == inf["mcu_ymax"] * -(-inf["mcu_xmax"] // D.KERNELS["render"]["unit"]) and sum(r.sizes) == inf["mcu_xmax"] * inf["mcu_ymax"], r.pic
            deal_render_and_check(J, torch, recs, image, lambda i: models[i], lambda spec, images, dsts: raw_ijg(J, b, spec, images, dsts), layout, dtype, cus, 1,
                                  "deal, %s batch" % ("progressive" if progressive else "baseline"), scale=sb[0], bias=sb[1])
        finally:
            b.close()


# ------------------------------------------------------------------------------------------------ source kinds
def test_progressive_files_and_files_with_restart_intervals(J, torch, harness):
    sizes = [(50, 70), (130, 21), (33, 31), (17, 9)]
    prog = [IC.pillow_file(IC.noise(w, h, 40 + k), IC.MODES[k % 4], 85, progressive=True) for k, (w, h) in enumerate(sizes)]
    rst = [harness.synth_jpeg(width=141, height=93, hs=2, vs=1, restart_interval=3, seed=5), harness.synth_jpeg(width=200, height=120, quality=25, restart_interval=7, seed=6),
           harness.synth_jpeg(width=97, height=61, gray=1, restart_interval=1, seed=7)]
    for files, pillow in ((prog, True), (rst, False)):            # (the generator's files are not an encoder's: nothing bounds their IDCT results by 511)
        b = decoded_batch(J, files)
        try:
            models = models_of(J, torch, b)
            if pillow:
                for i, f in enumerate(files):
                    assert np.array_equal(models[i], IC.pillow_pixels(f)), i
            render_and_check(J, torch, b, models, "HWC", "uint8", list(range(len(files))), what="progressive" if files is prog else "restart")
        finally:
            b.close()


def test_dc_only_fast_form_is_decoded_once_more_and_rendered_from_a_dc_only_arena(J, torch, harness):
    files = [harness.synth_jpeg(width=100, height=75, hs=2, vs=2, restart_interval=3 * (k % 2), seed=500 + k) for k in range(3)]
    b = decoded_batch(J, files, decode_ac=False)
    try:
        assert b.last_form() == 2
        sizes = [100 * 75 * 3] * 3
        ar = Arena(torch, sizes)
        torch.cuda.synchronize()
        assert raw_ijg(J, b, make_spec(J, "HWC", "uint8"), [0, 1, 2], [(ar.ptr(k), 0, 0) for k in range(3)]) == 0, J.last_error()
        assert b.last_form() == 1, "behind a fast-form decode the call decodes again in the generic form"
        keep = arenas_now(J, torch, b, [0, 1, 2])
        torch.cuda.synchronize()
        for i, a in arenas_of(b, keep).items():
            assert not a[:, 1:].any()                                 # a DC-only arena
            ar.place(i, M.render(a, 100, 75, IC.HV["420"])[0], "HWC", 300, 0)
        ar.check("DC-only")
    finally:
        b.close()


def test_the_wild_file_wraps_as_the_model_does(J, torch):
    data = IC.wild_file()
    b = decoded_batch(J, [data, data])
    try:
        models = models_of(J, torch, b)
        a, w, h, hv = M.arena_of_file(data)
        assert np.array_equal(models[0], M.render(a, w, h, hv)[0])           # the device's arena is the codec's
        render_and_check(J, torch, b, models, "HWC", "uint8", [0, 1], what="wild")
    finally:
        b.close()


DAMAGED = [(0, 81), (1, 77)]


def test_a_damaged_file_before_and_after_sync(J, torch, harness):
    """Before jsnoop_batch_sync the render sees what the parallel path left, after it the repaired blocks: each time the model of the arena a
    jsnoop_batch_pack_coefs enqueued right in front of it read."""
    bases = F.bases(harness)
    hurt = [F.mutate(harness, np.random.default_rng(seed), bases[base])[0] for base, seed in DAMAGED]
    b = J.JpegBatch()
    try:
        for f in (bases[0], hurt[0], hurt[1], bases[1]):
            b.add_jpeg(f)
        b.upload(); b.decode()
        images = [0, 1, 2, 3]
        dims = [(b.info(i)["dim_y"], b.info(i)["dim_x"]) for i in images]
        for phase in ("before sync", "after sync"):
            ar = Arena(torch, [h * w * 3 for h, w in dims])
            keep = arenas_now(J, torch, b, images)
            assert raw_ijg(J, b, make_spec(J, "HWC", "uint8"), images, [(ar.ptr(k), 0, 0) for k in range(4)]) == 0, J.last_error()
            torch.cuda.synchronize()
            for i, a in arenas_of(b, keep).items():
                w, h, hv, _ = geometry(b, i)
                ar.place(i, M.render(a, w, h, hv)[0], "HWC", w * 3, 0)
            ar.check(phase)
            b.sync()
        assert b.info(1)["flags"] != 0 and b.info(2)["flags"] != 0
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("sub,mode", [("4:4:4", "444"), ("4:2:2", "422"), ("4:2:0", "420")])
def test_round_trip_through_the_encoder_is_pillows_round_trip(J, torch, sub, mode):
    """Random pixels -> encode_jpeg -> add_jpeg -> to_torch(pixels="libjpeg") equals Pillow's decode of Pillow's file of the same pixels."""
    px = [IC.noise(w, h, 70 + k) for k, (w, h) in enumerate([(45, 29), (64, 48), (130, 21), (17, 33)])]
    enc = J.JpegEncoder()
    try:
        for quality in (35, 90):
            ours = enc.encode([torch.from_numpy(p).cuda() for p in px], quality=quality, subsampling=sub)
            b = decoded_batch(J, ours)
            try:
                got = b.to_torch(layout="HWC", pixels="libjpeg")
                for k, p in enumerate(px):
                    assert np.array_equal(got[k].cpu().numpy(), IC.pillow_pixels(IC.pillow_file(p, mode, quality))), (sub, quality, k)
            finally:
                b.close()
    finally:
        enc.close()


# ------------------------------------------------------------------------------------------------ refusals, the default path
def test_refusals_launch_nothing_and_write_nothing(J, torch, harness, mixed):
    f440 = harness.synth_jpeg(width=64, height=48, hs=1, vs=2, seed=7)
    good = mixed["420"]["files"][9]
    b = decoded_batch(J, [good, f440])
    try:
        assert b.ijg_renderable(0) and not b.ijg_renderable(1) and "luma sampling 1 x 2" in J.last_error()
        lib = J.load()
        assert lib.jsnoop_batch_ijg_renderable(b._h, 2) == 0 and b"out of range" in lib.jsnoop_last_error()
        before = [t.cpu().numpy().copy() for t in b.to_torch(layout="HWC")]
        ar = Arena(torch, [64 * 48 * 12, 64 * 48 * 12])
        p = ar.ptr(0)
        torch.cuda.synchronize()
        u8h, u8c, f32h, f32c = make_spec(J, "HWC", "uint8"), make_spec(J, "CHW", "uint8"), make_spec(J, "HWC", "float32"), make_spec(J, "CHW", "float32")
        bad_layout, bad_dtype, too_long = make_spec(J, "HWC", "uint8"), make_spec(J, "HWC", "uint8"), make_spec(J, "HWC", "uint8")
        bad_layout.layout, bad_dtype.dtype, too_long.struct_size = 2, 7, C.sizeof(J.capi.PackSpec) + 8
        w, h = 33, 31
        cases = [("a 4:4:0 file in the list", u8h, [0, 1], [(p, 0, 0), (ar.ptr(1), 0, 0)], "image 1: luma sampling 1 x 2"),
                 ("index past the end", u8h, [2], [(p, 0, 0)], "out of range"), ("negative index", u8h, [-1], [(p, 0, 0)], "out of range"),
                 ("NULL pointer", u8h, [0], [(0, 0, 0)], "NULL"), ("row_pitch below dense", u8h, [0], [(p, w * 3 - 1, 0)], "row_pitch"),
                 ("plane_pitch below dense", u8c, [0], [(p, w, w * h - 1)], "plane_pitch"), ("float pointer", f32h, [0], [(p + 2, 0, 0)], "multiples of 4"),
                 ("float row_pitch", f32c, [0], [(p, w * 4 + 2, 0)], "multiples of 4"), ("unknown layout", bad_layout, [0], [(p, 0, 0)], "layout"),
                 ("unknown dtype", bad_dtype, [0], [(p, 0, 0)], "dtype"), ("struct_size of a later version", too_long, [0], [(p, 0, 0)], "struct_size")]
        for what, spec, images, dsts, word in cases:
            assert raw_ijg(J, b, spec, images, dsts) == -1, what
            assert word in J.last_error() and "pack_ijg" in J.last_error(), (what, J.last_error())
        with pytest.raises(RuntimeError):
            b.to_torch(pixels="libjpeg")
        for kw in (dict(size=(8, 8)), dict(size=(8, 8), roi=(0, 0, 4, 4)), dict(pixels="pillow")):
            with pytest.raises(ValueError):
                b.to_torch(images=[0], **dict(dict(pixels="libjpeg"), **kw))
        nb = J.JpegBatch()
        try:
            nb.add_jpeg(good)
            assert raw_ijg(J, nb, u8h, [0], [(p, 0, 0)]) == -1 and "not been decoded" in J.last_error()
            nb.upload()
            assert raw_ijg(J, nb, u8h, [0], [(p, 0, 0)]) == -1 and "not been decoded" in J.last_error()
        finally:
            nb.close()
        torch.cuda.synchronize()
        assert ar.untouched()
        assert raw_ijg(J, b, u8h, None, []) == 0                    # n == 0 is accepted
        # the default path gives exactly the bytes it gave before, and a different answer from libjpeg's on a 4:2:0 photo
        after = b.to_torch(layout="HWC")
        assert all(np.array_equal(x, y.cpu().numpy()) for x, y in zip(before, after))
        assert np.array_equal(b.to_torch(layout="HWC", pixels="jpegsnoop")[0].cpu().numpy(), before[0])
        assert not np.array_equal(b.to_torch(images=[0], layout="HWC", pixels="libjpeg")[0].cpu().numpy(), before[0])
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ paths
def test_torch_raw_pointer_and_cpp_paths(J, torch, mixed, tmp_path):
    m = mixed["420"]; b = m["b"]; models = m["models"]
    # torch: stacked, padded, into out=, float with scale and bias, CHW
    t = b.to_torch(images=[9, 9], layout="CHW", stack=True, pixels="libjpeg")
    assert tuple(t.shape) == (2, 3, 31, 33) and np.array_equal(t[1].cpu().numpy(), form(models[9], "CHW", "uint8"))
    t = b.to_torch(images=[10, 3], layout="HWC", pad_to=(80, 64), dtype=torch.float32, scale=SCALE, bias=BIAS, bgr=True, pixels="libjpeg")
    assert np.array_equal(t[0, :70, :50].cpu().numpy(), form(models[10], "HWC", "float32", True, SCALE, BIAS)) and not t[0, 70:].any() and not t[1, 5:].any()
    out = torch.full((1, 48, 64, 3), 7, dtype=torch.uint8, device="cuda")
    assert b.to_torch(images=[7], layout="HWC", out=out, pixels="libjpeg") is out
    assert np.array_equal(out[0, :9, :17].cpu().numpy(), models[7]) and bool((out[0, 9:] == 7).all()) and bool((out[0, :, 17:] == 7).all())
    # the raw pointer: what render_and_check does everywhere above, here through the facade's own handle
    # C++: tests/cpp/render_demo.cpp through CJPEGsnoopCoreGpu::BatchPackIjg
    exe = str(tmp_path / "render_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "render_demo.cpp"),
                           "-L" + os.path.join(ROOT, "jpegsnoop_amd"), "-ljsnoop_gpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "jpegsnoop_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    pick = [9, 10, 11, 3]
    paths = []
    for k, i in enumerate(pick):
        paths.append(str(tmp_path / ("in%d.jpg" % k)))
        open(paths[-1], "wb").write(m["files"][i])
    lines = subprocess.check_output([exe, str(tmp_path)] + paths, text=True).split("\n")
    assert [ln.split()[0] for ln in lines if ln] == ["3", "2", "1", "0"]
    for k, i in enumerate(pick):
        got = np.fromfile(str(tmp_path / ("out%d.rgb" % k)), np.uint8)
        assert np.array_equal(got, models[i].reshape(-1)), i
