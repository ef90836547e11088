"""-m gpu: jsnoop_encode_run and k_encode (jsnoop_encode.hip), the export behind it and the Python, C++ and raw-pointer paths -- pixels in device memory
encoded as JPEG files on the device.

Value for value against tests/encode_model.py, which tests/test_encode_model.py pins on the CPU against Pillow (libjpeg-turbo): the arena and the
cumulative DC through jsnoop_encode_read_coefs for every layout, the sizes of the CPU grid, the seams of the unit (a run of JSNOOP_ENCODE_RUN MCUs), a
mixed call, every form a source can take, and the extreme pictures; the files of every export mode byte for byte against the export models fed the
model's arena; the round trip through the decoder; refusals; the wrappers."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import coef_model as CM
import deal_cases as D
import encode_cases as EC
import encode_model as M
import export_model as EM
import export_opt_model as OM
import export_prog_model as PM
import export_rst_model as RM
import prog_codec as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUB = {"grey": 0, "4:4:4": 0, "4:2:2": 1, "4:2:0": 2}
RUN = 8                                                              # JSNOOP_ENCODE_RUN (the ABI test holds it against the header)


@pytest.fixture(scope="module")
def J():
    import jpegsnoop_amd
    jpegsnoop_amd.load()
    return jpegsnoop_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def enc(J):
    e = J.JpegEncoder()
    yield e
    e.close()


def picture(layout, w, h, seed):
    return EC.picture(w, h, seed, grey=layout == "grey")


def assert_arena(enc, i, px, layout, tables, what, model=None):
    """model: M.encode(px, SUB[layout], tables) where the caller has it already."""
    arena, dccum, geo, _q = model or M.encode(px, SUB[layout], tables)
    a, d = enc.coefs(i)
    assert a.shape == arena.shape, (what, a.shape, arena.shape)
    bad = np.flatnonzero((a != arena).any(1) | (d != dccum))
    assert bad.size == 0, "%s: %d of %d blocks differ, first %d: arena %s / %s, dccum %d / %d" % (
        what, bad.size, geo.nblocks, bad[0], a[bad[0]].tolist(), arena[bad[0]].tolist(), d[bad[0]], dccum[bad[0]])
    inf = enc.info(i)
    assert (inf["dim_x"], inf["dim_y"], inf["mcu_xmax"], inf["mcu_ymax"], inf["total_blocks"], inf["ncomp"]) == (px.shape[1], px.shape[0], geo.mcu_x, geo.mcu_y, geo.nblocks, geo.ncomp)


def run_and_check(enc, torch, pics, layout, what, **opts):
    """One call over all pictures (a mixed call), every image against the model."""
    tables = opts["qtables"] if opts.get("qtables") else M.quality_tables(opts.get("quality", 75))
    assert enc.run([torch.from_numpy(p).cuda() for p in pics], subsampling=SUB[layout], **opts) == len(pics) == len(enc)
    for i, p in enumerate(pics):
        assert_arena(enc, i, p, layout, tables, "%s image %d (%d x %d)" % (what, i, p.shape[1], p.shape[0]))


# ---------------------------------------------------------------------------------------------------------------- 5: arena and dccum against the model
@pytest.mark.parametrize("layout", EC.LAYOUTS)
@pytest.mark.parametrize("quality", [1, 24, 50, 85, 100, "custom"])
def test_the_sizes_of_the_cpu_grid_in_every_layout(enc, torch, layout, quality):
    pics = [picture(layout, w, h, w + h) for w, h in EC.SIZES]
    opts = dict(qtables=EC.CUSTOM) if quality == "custom" else dict(quality=quality)
    run_and_check(enc, torch, pics, layout, "%s q%s" % (layout, quality), **opts)


@pytest.mark.parametrize("layout", EC.LAYOUTS)
def test_the_seams_of_the_unit(enc, torch, layout):
    """Widths of one unit of MCUs - 1 pixel, exactly one unit, one unit + 1 and three and a half units, on a one-MCU-high picture; the same in heights of
    MCUs on a one-MCU-wide picture; and both at once."""
    mw = 16 if SUB[layout] else 8; mh = 16 if SUB[layout] == 2 else 8; U = RUN * mw
    sizes = [(U - 1, mh), (U, mh), (U + 1, mh), (3 * U + U // 2, mh), (mw, mh - 1), (mw, mh), (mw, mh + 1), (mw, 3 * mh + mh // 2), (1, 3 * mh + 1), (U + 1, mh + 1), (2 * U, 2 * mh - 1)]
    run_and_check(enc, torch, [picture(layout, w, h, 3 * w + h) for w, h in sizes], layout, layout + " seams", quality=90)


def test_a_mixed_call_of_twelve_images_grey_and_colour(enc, torch):
    sizes = [(1, 1), (200, 3), (3, 200), (129, 17), (16, 16), (15, 33), (257, 31), (64, 64), (7, 7), (130, 130), (48, 9), (300, 20)]
    pics = [EC.picture(w, h, 5 * w + h, grey=k % 3 == 1) for k, (w, h) in enumerate(sizes)]
    assert enc.run([torch.from_numpy(p).cuda() for p in pics], quality=77, subsampling="4:2:0") == 12
    for i, p in enumerate(pics):
        assert_arena(enc, i, p, "grey" if p.ndim == 2 else "4:2:0", M.quality_tables(77), "mixed image %d" % i)
    # ... and once more at 4:2:2 into the same arena: nothing of the call before shows through
    assert enc.run([torch.from_numpy(p).cuda() for p in pics[::-1]], quality=30, subsampling="4:2:2") == 12
    for i, p in enumerate(pics[::-1]):
        assert_arena(enc, i, p, "grey" if p.ndim == 2 else "4:2:2", M.quality_tables(30), "mixed image %d, second call" % i)


@pytest.mark.parametrize("layout", ["4:4:4", "4:2:0"])
def test_every_form_of_a_source_gives_the_same_arena(J, enc, torch, layout):
    w, h = 50, 37
    px = EC.picture(w, h, 99); t = torch.from_numpy(px).cuda()
    srcs = []; keep = []

    def raw(buf, off, **desc):
        keep.append(buf); return dict(ptr=buf.data_ptr() + off, width=w, height=h, **desc)
    for off in (0, 1, 3, 15):                                       # a dense interleaved picture at every byte phase
        buf = torch.full((w * h * 3 + 32,), 0xEE, dtype=torch.uint8, device="cuda"); buf[off:off + w * h * 3] = t.reshape(-1)
        srcs.append(raw(buf, off, channels=3))
    pitched = torch.full((h, w * 3 + 7), 0xEE, dtype=torch.uint8, device="cuda"); pitched[:, :w * 3] = t.reshape(h, w * 3)
    srcs.append(raw(pitched, 0, channels=3, row_pitch=w * 3 + 7))    # a row pitch above the row
    rgba = torch.full((h, w, 4), 0xEE, dtype=torch.uint8, device="cuda"); rgba[..., :3] = t
    srcs.append(rgba[..., :3])                                       # interleaved, stride 4, as a tensor view
    srcs.append(t.permute(2, 0, 1).contiguous())                     # planar [3, H, W]
    planes = torch.full((3, h + 2, w + 9), 0xEE, dtype=torch.uint8, device="cuda"); planes[:, :h, :w] = t.permute(2, 0, 1)
    srcs.append(planes[:, :h, :w])                                   # planar with row and plane pitches above the dense ones
    bgr = t.flip(2).contiguous()
    srcs.append(raw(bgr, 0, channels=3, order="bgr"))                # B, G, R
    up = t.flip(0).contiguous()
    srcs.append(raw(up, 0, channels=3, bottom_up=True))              # bottom-up
    bgra_up = torch.full((h, w, 4), 0xEE, dtype=torch.uint8, device="cuda"); bgra_up[..., :3] = t.flip(0).flip(2)
    srcs.append(raw(bgra_up, 0, channels=3, order="bgr", pixel_stride=4, bottom_up=True))      # the form of a DIB
    srcs.append(raw(t.permute(2, 0, 1).flip(0).contiguous(), 0, channels=3, layout="planar", order="bgr"))
    torch.cuda.synchronize()
    assert enc.run(srcs, quality=85, subsampling=layout) == len(srcs)
    for i in range(len(srcs)):
        assert_arena(enc, i, px, layout, M.quality_tables(85), "%s source form %d" % (layout, i))
    # a batch's own DIB: BGRA, bottom-up, MCU-padded -- the picture's rows are its last dim_y rows
    Image = pytest.importorskip("PIL.Image")
    f = io.BytesIO(); Image.fromarray(px).save(f, "JPEG", quality=90, subsampling=2)
    b = J.JpegBatch()
    try:
        b.add_jpeg(f.getvalue()); b.upload(); b.decode(); b.sync()
        inf = b.info(0)
        dib = b._lib.jsnoop_batch_dib_dev(b._h, 0)
        host = b.dib(0)[::-1][:h, :w, 2::-1]                        # top-down, cropped, R, G, B
        src = dict(ptr=dib + (inf["img_y"] - h) * inf["img_x"] * 4, width=w, height=h, channels=3, order="bgr", pixel_stride=4, row_pitch=inf["img_x"] * 4, bottom_up=True)
        assert enc.run([src], quality=85, subsampling=layout) == 1
        assert_arena(enc, 0, np.ascontiguousarray(host), layout, M.quality_tables(85), layout + " DIB as source")
    finally:
        b.close()


@pytest.mark.parametrize("layout", EC.LAYOUTS)
def test_the_extreme_pictures(enc, torch, layout):
    pics = [np.ascontiguousarray(p[..., 0]) if layout == "grey" else p for p in EC.extremes().values()]
    run_and_check(enc, torch, pics, layout, layout + " extremes", quality=100)
    run_and_check(enc, torch, pics, layout, layout + " extremes q1", quality=1)


# ---------------------------------------------------------------------------------------------------------------- the deal: a wave walks several units and records
def test_calls_of_so_many_units_that_a_wave_walks_several_units_and_records(enc, torch, capsys):
    """Every test above stays below EN_WAVES * 4 * compute units units, where a workgroup's share is four units and a wave takes one.  Here the call is
    sized from the device (tests/deal_cases.py; tests/test_deal_cases.py proves the lists on the CPU): a share of twelve units or more, so every wave
    takes three and more one after the other through the same LDS, crosses records -- one-MCU pictures four in a row, which one step passes over --,
    leaves a long picture in the middle of a share and takes a one-MCU run directly behind a run of eight.  About a dozen distinct pictures, many source
    descriptors on the same tensors; grey and colour in one 4:2:0 call, then a 4:2:2 call with other tables.  Every image against the model."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for form, quality in (("420", 77), ("422", 40)):
        layout = "4:2:" + form[2]
        recs = D.encode_records(cus, form)
        c = D.census_of("encode", form, recs, cus)
        with capsys.disabled():
            print("\nk_encode %s, %d compute units: %s" % (layout, cus, D.summary(c)))
        assert D.missing(c, D.KERNELS["encode"]["waves"], **D.conditions("encode", form)) == [], D.summary(c)
        tables = M.quality_tables(quality)
        distinct = sorted({r.pic for r in recs})
        px = {p: EC.picture(p[1], p[2], 40 + k, grey=p[0] == "grey") for k, p in enumerate(distinct)}
        model = {p: M.encode(px[p], SUB[layout], tables) for p in distinct}
        for r in recs:                                                # the units the census counted are the units of the call
            geo = model[r.pic][2]
            assert r.units == -(-geo.mcu_x // RUN) * geo.mcu_y and sum(r.sizes) == geo.mcu_x * geo.mcu_y, r.pic
        dev = {p: torch.from_numpy(px[p]).cuda() for p in distinct}
        assert enc.run([dev[r.pic] for r in recs], quality=quality, subsampling=layout) == len(recs) == len(enc)
        for i, r in enumerate(recs):
            assert_arena(enc, i, px[r.pic], "grey" if r.pic[0] == "grey" else layout, tables, "deal %s image %d %s" % (layout, i, r.pic), model=model[r.pic])


# ---------------------------------------------------------------------------------------------------------------- 6: exports, round trip, wrappers
def first_difference(got, want):
    if got is None or want is None:
        return "got %s, want %s" % ("None" if got is None else "%d bytes" % len(got), "None" if want is None else "%d bytes" % len(want))
    n = min(len(got), len(want))
    k = next((i for i in range(n) if got[i] != want[i]), n)
    return "lengths %d / %d, first difference at byte %d: got %s, want %s" % (len(got), len(want), k, got[k:k + 8].hex(), want[k:k + 8].hex())


PICS = [("grey", 33, 31), ("4:4:4", 17, 9), ("4:2:2", 130, 21), ("4:2:0", 50, 70)]


@pytest.mark.parametrize("layout,w,h", PICS)
def test_every_export_mode_is_the_models_file(enc, torch, layout, w, h):
    px = picture(layout, w, h, 7); tables = M.quality_tables(85)
    arena, dccum, geo, qnat = M.encode(px, SUB[layout], tables)
    assert enc.run([torch.from_numpy(px).cuda()], quality=85, subsampling=SUB[layout]) == 1
    want = {"annex_k": EM.export_file(arena, dccum, geo, w, h, qnat), "optimal": OM.export_file(arena, dccum, geo, w, h, qnat),
            "rows1": RM.export_file(arena, dccum, geo, w, h, qnat, geo.mcu_x), "progressive": PM.export_file(arena, dccum, geo, w, h, qnat, PM.DEFAULT[geo.ncomp]),
            "nojfif": EM.export_file(arena, dccum, geo, w, h, qnat, jfif=False)}
    got = {"annex_k": enc.export(), "optimal": enc.export(huffman="optimal"), "rows1": enc.export(restart=("rows", 1)), "progressive": enc.export(progressive=True),
           "nojfif": enc.export(jfif=False)}
    for mode in want:
        assert want[mode][0] == EM.OK and got[mode][0] == want[mode][2], "%s %s: %s" % (layout, mode, first_difference(got[mode][0], want[mode][2]))
    assert len(enc.export_scans(0)) == 0 and enc.export_results()[0]["result"] == 0
    enc.export(progressive=True)
    assert len(enc.export_scans(0)) == len(PM.DEFAULT[geo.ncomp])
    Image = pytest.importorskip("PIL.Image")
    f = io.BytesIO(); Image.fromarray(px).save(f, "JPEG", quality=85, subsampling=SUB[layout]); f = f.getvalue()
    D, Dm = PC.decode(f), PC.decode(got["annex_k"][0])
    assert bytes(f[D.scans[0]["start"]:D.scans[0]["end"]]) == bytes(got["annex_k"][0][Dm.scans[0]["start"]:Dm.scans[0]["end"]])


@pytest.mark.parametrize("layout,w,h", PICS)
def test_round_trip_through_the_decoder(J, enc, torch, layout, w, h):
    Image = pytest.importorskip("PIL.Image")
    px = picture(layout, w, h, 21)
    files = enc.encode([torch.from_numpy(px).cuda()], quality=70, subsampling=SUB[layout], huffman="optimal")
    arena, dccum = enc.coefs(0)
    f = io.BytesIO(); Image.fromarray(px).save(f, "JPEG", quality=70, subsampling=SUB[layout])
    b = J.JpegBatch()
    try:
        b.add_jpeg(files[0]); b.add_jpeg(f.getvalue()); b.upload(); b.decode(); b.sync()
        back = b.coefs(0)
        geo = CM.Geometry(M.hv_of(1 if px.ndim == 2 else 3, SUB[layout]), b.info(0)["mcu_xmax"], b.info(0)["mcu_ymax"])
        assert np.array_equal(back[:, 1:], arena[:, 1:])
        assert np.array_equal(CM.running_dc(back, geo), dccum)
        assert np.array_equal(b.dib(0), b.dib(1)), "the DIB of the encoder's file is not the DIB of Pillow's file of the same pixels"
    finally:
        b.close()


def test_every_refusal_leaves_the_previous_result_alone(enc, torch):
    px = EC.picture(40, 24, 5); t = torch.from_numpy(px).cuda()
    files = enc.encode([t], quality=60, subsampling="4:2:2")
    before = (enc.coefs(0), enc.export_results())
    good = dict(ptr=t.data_ptr(), width=40, height=24, channels=3)
    for bad, word in [(dict(good, ptr=0), "ptr is NULL"), (dict(good, width=0), "1..65535"), (dict(good, height=65536), "1..65535"), (dict(good, channels=2), "channels"),
                      (dict(good, pixel_stride=2), "pixel_stride"), (dict(good, row_pitch=119), "row_pitch"), (dict(good, layout="planar", plane_pitch=5), "plane_pitch")]:
        with pytest.raises(RuntimeError, match=word):
            enc.run([good, bad], quality=60)
    for kw, word in [(dict(quality=0), "quality"), (dict(quality=101), "quality"), (dict(qtables=([0] * 64, [1] * 64)), "luma table is 0")]:
        with pytest.raises(RuntimeError, match=word):
            enc.run([good], **kw)
    with pytest.raises(RuntimeError, match="out of range"):
        enc.export(images=[0, 1])
    with pytest.raises(RuntimeError, match="out of range"):
        enc.export(images=[-1], restart=4)
    with pytest.raises(RuntimeError):
        enc.export(restart=70000)
    with pytest.raises(RuntimeError):
        enc.export(progressive=[((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 1)])              # AC successive approximation: refused as for a batch
    after = (enc.coefs(0), enc.export_results())
    assert len(enc) == 1 and np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1]) and before[1] == after[1]
    buf = (C.c_uint8 * len(files[0]))()
    assert enc._lib.jsnoop_encode_read_export(enc._h, 0, buf, len(files[0])) == len(files[0]) and bytes(buf) == files[0]
    assert enc.run([]) == 0 and len(enc) == 0 and enc.export_results() == []
    with pytest.raises(RuntimeError, match="nothing has been encoded"):
        enc.export()


def test_batch_encode_jpeg_writes_the_thumbnail_sheet(J, torch):
    Image = pytest.importorskip("PIL.Image")
    b = J.JpegBatch()
    try:
        for k, (w, h) in enumerate([(130, 70), (64, 48), (33, 31)]):
            f = io.BytesIO(); Image.fromarray(EC.picture(w, h, k)).save(f, "JPEG", quality=92, subsampling=k % 3)
            b.add_jpeg(f.getvalue())
        b.upload(); b.decode(); b.sync()
        thumbs = b.to_torch(layout="HWC", size=(24, 40), filter="area").cpu().numpy()
        files = b.encode_jpeg(size=(24, 40), filter="area", quality=80, subsampling="4:2:0")
        full = [t.cpu().numpy() for t in b.to_torch(layout="HWC")]
        files_full = b.encode_jpeg(images=[2, 0], quality=95, subsampling="4:4:4", huffman="optimal")
    finally:
        b.close()
    for k in range(3):
        arena, dccum, geo, qnat = M.encode(thumbs[k], 2, M.quality_tables(80))
        assert files[k] == EM.export_file(arena, dccum, geo, 40, 24, qnat)[2], "thumbnail %d" % k
    for k, i in enumerate([2, 0]):
        arena, dccum, geo, qnat = M.encode(full[i], 0, M.quality_tables(95))
        assert files_full[k] == OM.export_file(arena, dccum, geo, full[i].shape[1], full[i].shape[0], qnat)[2], "full-size image %d" % i


def test_torch_cpp_and_raw_pointer_paths(J, enc, torch, tmp_path):
    w, h = 45, 29
    yy, xx = np.mgrid[0:h, 0:w]
    px = np.stack([(7 * xx + 3 * yy) & 255, (xx * yy + 5) & 255, (xx + 2 * yy * yy) & 255], -1).astype(np.uint8)      # tests/cpp/encode_demo.cpp's picture
    arena, dccum, geo, qnat = M.encode(px, 1, M.quality_tables(65))
    want = EM.export_file(arena, dccum, geo, w, h, qnat)[2]
    t = torch.from_numpy(px).cuda()
    assert enc.encode([t], quality=65, subsampling="4:2:2") == [want]
    on_dev = enc.encode_to_torch([t, t.permute(2, 0, 1).contiguous()], quality=65, subsampling="4:2:2")
    assert [bytes(x.cpu().numpy()) for x in on_dev] == [want, want] and all(x.is_cuda for x in on_dev)
    assert enc.encode([dict(ptr=t.data_ptr(), width=w, height=h, channels=3)], quality=65, subsampling=1) == [want]
    grey = np.ascontiguousarray(px[..., 1]); tg = torch.from_numpy(grey).cuda()
    a1, d1, g1, q1 = M.encode(grey, 0, M.quality_tables(65))
    assert enc.encode([dict(ptr=tg.data_ptr(), width=w, height=h, channels=1)], quality=65) == [EM.export_file(a1, d1, g1, w, h, q1)[2]]
    exe = str(tmp_path / "encode_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "encode_demo.cpp"),
                           "-L" + os.path.join(ROOT, "jpegsnoop_amd"), "-ljsnoop_gpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "jpegsnoop_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe, str(tmp_path), str(w), str(h), "65", "1"], text=True).split()
    assert out == ["0", str(len(want)), "1", str(len(want))]
    for k in range(2):
        assert open(str(tmp_path / ("out%d.jpg" % k)), "rb").read() == want
