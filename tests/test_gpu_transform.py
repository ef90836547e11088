"""-m gpu: jsnoop_transform_run and k_transform (jsnoop_transform.hip), the export behind it and the Python, C++ and raw-pointer paths -- jpegtran's
lossless transforms of a decoded batch on the device.

Value for value against tests/transform_model.py, which tests/test_transform_model.py pins on the CPU by the float64 IDCT identity.  The model is fed what
the source batch holds -- the arena through read_coefs, the cumulative DC through slot 0 of coefs_to_torch, the multipliers through image_dqt -- and the
object's arena, cumulative DC, tables and descriptor must equal its output exactly: the layouts and sizes of the CPU sweep, pictures at the seams of the
wave's run of JSNOOP_TRANSFORM_RUN blocks, a mixed call, both stream arrangements, progressive, DC-only and damaged sources, the files of every export mode
byte for byte against the export models fed the model's output, round trips, refusals and the wrappers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import coef_model as CM
import deal_cases as D
import export_model as EM
import export_opt_model as OM
import export_prog_model as PM
import export_rst_model as RM
import fuzz_util as F
import transform_cases as TC
import transform_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_OPS = sorted(M.OPS.values())
RUN = 8                                                              # JSNOOP_TRANSFORM_RUN (the ABI test holds it against the header)


@pytest.fixture(scope="module")
def J():
    import jpegsnoop_amd
    jpegsnoop_amd.load()
    return jpegsnoop_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def decoded(J, files, **kw):
    b = J.JpegBatch(**kw)
    for f in files:
        b.add_jpeg(f)
    b.upload(); b.decode(); b.sync()
    return b


def held(b, i, geo):
    """What the batch holds for image i, in the model's form: (arena, dccum, geo, dim_x, dim_y, qnat)."""
    arena = b.coefs(i)
    dccum = np.zeros(geo.nblocks, np.int16)
    ts = b.coefs_to_torch(images=[i])[0]
    for c in range(geo.ncomp):
        dccum[geo.arena_index(c)] = ts[c].cpu().numpy()[..., 0]
    inf = b.info(i)
    assert (inf["mcu_xmax"], inf["mcu_ymax"], inf["total_blocks"]) == (geo.mcu_x, geo.mcu_y, geo.nblocks)
    return arena, dccum, geo, inf["dim_x"], inf["dim_y"], [[int(v) for v in b.dqt(i, c)] for c in range(geo.ncomp)]


class Sources:
    """A decoded batch and what it holds, read once."""

    def __init__(self, J, files, geos, **kw):
        self.b = decoded(J, files, **kw)
        self.src = [held(self.b, i, g) for i, g in enumerate(geos)]
        for s in self.src:
            for a in s[:2]:
                a.setflags(write=False)

    def close(self):
        self.b.close()


def made(J, shapes, shift=0, script=None, **kw):
    """Sources over generated files: shapes = [(layout, w, h)]."""
    files, geos = [], []
    for k, (layout, w, h) in enumerate(shapes):
        f, frame = TC.jpeg_file(layout, w, h, 17 * k + w + h, shift + k % 3, script)
        files.append(f); geos.append(TC.geometry(frame))
    return Sources(J, files, geos, **kw)


def check_run(t, S, images, what, **opts):
    """The object after run(images, **opts) against the model, entry by entry.  -> the model's results, one per entry."""
    op = M.OPS[opts["op"]] if isinstance(opts["op"], str) else opts["op"]
    edge = {"trim": M.TRIM, "perfect": M.PERFECT}[opts.get("edge", "trim")]
    once = {i: M.transform(*S.src[i], op, edge, opts.get("grayscale", False), opts.get("crop")) for i in set(images)}      # (a list may name an image many times)
    want = [once[i] for i in images]
    ent = t.entries()
    assert [e["result"] for e in ent] == [R.result for R in want], (what, opts, ent)
    k = 0
    for e, R, i in zip(ent, want, images):
        if R.result != M.OK:
            assert e["image"] == -1
            continue
        assert e["image"] == k, (what, ent)
        a, d = t.coefs(k)
        assert a.shape == R.arena.shape, (what, opts, i, a.shape, R.arena.shape)
        bad = np.flatnonzero((a != R.arena).any(1) | (d != R.dccum))
        assert bad.size == 0, "%s %s image %d: %d of %d blocks differ, first %d: arena %s / %s, dccum %d / %d" % (
            what, opts, i, bad.size, R.geo.nblocks, bad[0], a[bad[0]].tolist(), R.arena[bad[0]].tolist(), d[bad[0]], R.dccum[bad[0]])
        inf = t.info(k)
        assert (inf["dim_x"], inf["dim_y"], inf["mcu_xmax"], inf["mcu_ymax"], inf["total_blocks"], inf["ncomp"], inf["mcu_w"], inf["mcu_h"]) == (
            R.dim_x, R.dim_y, R.geo.mcu_x, R.geo.mcu_y, R.geo.nblocks, R.geo.ncomp, 8 * R.geo.hmax, 8 * R.geo.vmax), (what, opts, i, inf)
        assert [t.dqt(k, c) for c in range(R.geo.ncomp)] == R.qnat, (what, opts, i)
        k += 1
    assert len(t) == k
    return want


def run_and_check(S, images, what, **opts):
    t = S.b.transform(images=images, **opts)
    try:
        return check_run(t, S, images, what, **opts)
    finally:
        t.close()


# ---------------------------------------------------------------------------------------------------------------- arena, dccum, tables, descriptor
@pytest.mark.parametrize("layout", list(TC.LAYOUTS))
def test_the_layouts_and_sizes_of_the_cpu_sweep(J, layout):
    S = made(J, [(layout, w, h) for w, h in TC.SIZES])
    try:
        every = list(range(len(TC.SIZES))); n = 0
        for op in ALL_OPS:
            for opts in (dict(), dict(edge="perfect"), dict(grayscale=True), dict(crop=(5, 3, 20, 11)), dict(crop=(16, 16, 1000, 1000), edge="perfect")):
                n += sum(R.result == M.OK for R in run_and_check(S, every, layout, op=op, **opts))
        assert n >= 100
    finally:
        S.close()


def test_pictures_at_the_seams_of_the_waves_run(J):
    """Grey pictures of 7, 8, 9 and 28 blocks; one MCU wide and one MCU high; MCU grids of 3 x 2 -- under every op (a 4:2:0 MCU is 6 blocks: runs straddle MCUs)."""
    shapes = [("grey", 56, 8), ("grey", 64, 8), ("grey", 72, 8), ("grey", 56, 32), ("grey", 8, 8 * (RUN + 1)), ("4:2:0", 16, 80), ("4:2:0", 80, 16), ("4:2:0", 48, 32),
              ("4:2:2", 48, 16), ("4:1:1", 96, 16), ("4:4:4", 24, 16), ("4:4:0", 8, 48)]
    S = made(J, shapes)
    try:
        for op in ALL_OPS:
            want = run_and_check(S, list(range(len(shapes))), "seams", op=op, edge="perfect")
            assert all(R.result == M.OK for R in want)
            assert [R.geo.nblocks for R in want[:4]] == [7, 8, 9, 28]
    finally:
        S.close()


def test_a_mixed_call_of_twelve_entries_a_second_run_and_both_stream_arrangements(J):
    shapes = [("grey", 56, 20), ("4:2:0", 48, 40), ("4:4:4", 40, 9), ("4:2:0", 20, 33), ("grey", 29, 8), ("4:2:2", 80, 17), ("4:4:0", 40, 50), ("4:2:0", 30, 30),
              ("4:1:1", 128, 8), ("grey", 20, 20)]
    S = made(J, shapes)
    try:
        order = [3, 0, 1, 2, 4, 5, 9, 6, 7, 8, 1, 0]
        opts = dict(op="flip_h", edge="perfect", crop=(20, 0, 1000, 1000))
        t = S.b.transform(images=order, **opts)                       # the batch's stream
        try:
            want = check_run(t, S, order, "mixed", **opts)
            res = [R.result for R in want]
            assert len(res) == 12 and res.count(M.OK) >= 6 and M.IMPERFECT in res[1:-1] and M.EMPTY in res[1:-1] and res[0] == M.EMPTY and res[-1] == M.OK
            assert len({tuple(map(tuple, R.qnat)) for R in want if R.result == M.OK}) >= 3, "several table sets"
            t.run(S.b, "rot90", order[::-1], (20, 0, 1000, 1000), "trim")     # a second run into the same object: nothing of the call before shows through
            check_run(t, S, order[::-1], "second run", op="rot90", edge="trim", crop=(20, 0, 1000, 1000))
            t.run(S.b, "transverse", [1], None, "trim", True)
            check_run(t, S, [1], "third run", op="transverse", grayscale=True)
        finally:
            t.close()
        own = J.JpegTransform(device=S.b.device())                    # a stream of its own
        try:
            own.run(S.b, "rot270", order, None, "trim")
            check_run(own, S, order, "own stream", op="rot270")
        finally:
            own.close()
    finally:
        S.close()


def test_calls_of_so_many_units_that_a_wave_walks_several_units_and_records(J, torch, capsys):
    """The calls above stay below XF_WAVES * 8 * compute units units, where a workgroup's share is four units and a wave takes one.  Here the lists are
    sized from the device (tests/deal_cases.py, proven on the CPU by tests/test_deal_cases.py): a share of twelve units, so every wave takes three runs
    one after the other -- under a transposing op through the same LDS tile --, passes over three one-run entries in one step, leaves a long entry in
    the middle of a share and takes a run of fewer than eight blocks directly behind a full one.  flip_v as it comes, and rot90 with a crop and
    edge="perfect"; entries the call refuses (EMPTY, IMPERFECT) sit among those it writes and get no record.  About twenty distinct files under
    three table sets, listed many times; every entry against the model."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lists = {form: D.transform_records(cus, form) for form in D.TRANSFORM_FORMS}
    for form, recs in lists.items():
        c = D.census_of("transform", form, recs, cus)
        with capsys.disabled():
            print("\nk_transform %s, %d compute units: %s" % (D.TRANSFORM_FORMS[form], cus, D.summary(c)))
        assert D.missing(c, D.KERNELS["transform"]["waves"], **D.conditions("transform", form)) == [], D.summary(c)
    shapes = sorted({r.pic for recs in lists.values() for r in recs})
    S = made(J, shapes)
    try:
        for form, recs in lists.items():
            images = [shapes.index(r.pic) for r in recs]
            want = run_and_check(S, images, "deal " + form, **D.TRANSFORM_FORMS[form])
            for r, R in zip(recs, want):                              # the units the census counted are the units of the call
                assert (r.sizes is None) == (R.result != M.OK) and (r.sizes is None or (sum(r.sizes), r.units) == (R.geo.nblocks, -(-R.geo.nblocks // RUN))), r.pic
            assert {R.result for R in want} == ({M.OK, M.EMPTY, M.IMPERFECT} if form == "turned" else {M.OK, M.EMPTY})
    finally:
        S.close()


def test_a_run_on_a_stream_of_its_own_goes_behind_the_decode_enqueued_last(J, harness):
    """Clean files the parallel path decodes whole (no flags: nothing is left to sync): the decode is enqueued again and NOT waited for, and the run on the
    object's own stream must still read the finished arena -- it goes behind an event on the batch's stream."""
    files = [harness.synth_jpeg(width=640, height=480, hs=2, vs=2, quality=90, seed=900 + k) for k in range(4)]
    S = Sources(J, files, [CM.geometry_of(harness.parse_jpeg(f)) for f in files])
    own = J.JpegTransform(device=S.b.device())
    try:
        assert all(S.b.info(i)["flags"] == 0 and S.b.info(i)["path"] == 1 for i in range(4))
        for op in ("flip_v", "transpose"):
            S.b.decode()                                              # (enqueued, not waited for)
            own.run(S.b, op, [3, 2, 1, 0])
            check_run(own, S, [3, 2, 1, 0], "behind the decode", op=op)
        S.b.sync()
    finally:
        own.close(); S.close()


def test_a_progressive_source_batch(J):
    shapes = [("4:2:0", 50, 70), ("4:4:4", 17, 9), ("4:2:2", 33, 31)]
    S = made(J, shapes, script=PM.DEFAULT[3])
    try:
        assert all(S.b.info(i)["path"] == 3 for i in range(3))
        base = made(J, shapes)                                        # the same coefficients as baseline files hold the same arena
        try:
            for i in range(3):
                assert np.array_equal(S.src[i][1], base.src[i][1]) and S.src[i][5] == base.src[i][5]
        finally:
            base.close()
        for op in ("rot90", "flip_v", "transverse"):
            run_and_check(S, [2, 0, 1], "progressive", op=op)
    finally:
        S.close()


def test_a_batch_after_a_dc_only_fast_decode(J, harness):
    files = [harness.synth_jpeg(width=100, height=75, hs=2, vs=2, restart_interval=3 * (k % 2), seed=700 + k) for k in range(3)]
    geos = [CM.geometry_of(harness.parse_jpeg(f)) for f in files]
    b = decoded(J, files, decode_ac=False)
    try:
        assert b.last_form() == 2
        t = b.transform("rot90")
        try:
            assert b.last_form() == 1, "behind a fast-form decode the call decodes again in the generic form"
            src = [held(b, i, g) for i, g in enumerate(geos)]
            for i in range(3):
                assert not src[i][0][:, 1:].any()
                R = M.transform(*src[i], M.ROT_90)
                a, d = t.coefs(i)
                assert R.result == M.OK and np.array_equal(a, R.arena) and np.array_equal(d, R.dccum) and d.any()
        finally:
            t.close()
    finally:
        b.close()


def test_damaged_sources_after_sync_pass_through_as_repaired(J, harness):
    bases = F.bases(harness)
    files = [bases[0]]
    for base, seed in [(0, 81), (1, 77)]:                             # the two files of tests/test_gpu_coefs.py
        data, _q, mode = F.mutate(harness, np.random.default_rng(seed), bases[base])
        assert mode == 0 and data != bases[base]
        files.append(data)
    geos = [CM.geometry_of(harness.parse_jpeg(f)) for f in files]
    S = Sources(J, files, geos)
    try:
        assert S.b.info(1)["flags"] != 0 and S.b.info(2)["flags"] != 0
        for op in ("none", "rot180", "transpose"):
            want = run_and_check(S, [1, 2, 0], "damaged", op=op)
            assert all(R.result == M.OK for R in want)
    finally:
        S.close()


# ---------------------------------------------------------------------------------------------------------------- exports, round trips
def first_difference(got, want):
    if got is None or want is None:
        return "got %s, want %s" % ("None" if got is None else "%d bytes" % len(got), "None" if want is None else "%d bytes" % len(want))
    n = min(len(got), len(want))
    k = next((i for i in range(n) if got[i] != want[i]), n)
    return "lengths %d / %d, first difference at byte %d: got %s, want %s" % (len(got), len(want), k, got[k:k + 8].hex(), want[k:k + 8].hex())


@pytest.mark.parametrize("layout,w,h,op", [("grey", 33, 31, "rot90"), ("4:4:4", 17, 9, "flip_h"), ("4:2:2", 50, 21, "transpose"), ("4:2:0", 50, 70, "transverse"),
                                           ("4:1:1", 64, 16, "rot270"), ("4:4:0", 24, 32, "rot180")])
def test_every_export_mode_is_the_models_file(J, layout, w, h, op):
    S = made(J, [(layout, w, h)])
    try:
        R = M.transform(*S.src[0], M.OPS[op])
        assert R.result == M.OK
        a = (R.arena, R.dccum, R.geo, R.dim_x, R.dim_y, R.qnat)
        want = {"annex_k": EM.export_file(*a), "optimal": OM.export_file(*a), "rows1": RM.export_file(*a, R.geo.mcu_x),
                "progressive": PM.export_file(*a, PM.DEFAULT[R.geo.ncomp]), "nojfif": EM.export_file(*a, jfif=False)}
        t = S.b.transform(op)
        try:
            got = {"annex_k": t.export(), "optimal": t.export(huffman="optimal"), "rows1": t.export(restart=("rows", 1)), "progressive": t.export(progressive=True),
                   "nojfif": t.export(jfif=False)}
            for mode in want:
                assert want[mode][0] == EM.OK and got[mode][0] == want[mode][2], "%s %s %s: %s" % (layout, op, mode, first_difference(got[mode][0], want[mode][2]))
            assert len(t.export_scans(0)) == 0
            t.export(progressive=True)
            assert len(t.export_scans(0)) == len(PM.DEFAULT[R.geo.ncomp])
            assert t.export(restart="source") == [want["annex_k"][2]], "no restart interval is recorded"
        finally:
            t.close()
    finally:
        S.close()


@pytest.mark.parametrize("layout", ["grey", "4:2:0", "4:2:2", "4:1:1"])
def test_round_trips_through_export_and_decode_are_byte_identical(J, layout):
    hv = TC.LAYOUTS[layout]; m = 8 * max(max(a, b) for a, b in hv)
    S = made(J, [(layout, 3 * m, 2 * m)])
    try:
        plain = S.b.export_jpeg()[0]
        for chain in (["flip_h", "flip_h"], ["rot90"] * 4, ["transpose", "transpose"], ["rot90", "rot270"], ["rot180", "flip_v", "flip_h"]):
            b = S.b; mine = []
            try:
                for op in chain:
                    t = b.transform(op)
                    try:
                        f = t.export()[0]
                    finally:
                        t.close()
                    b = decoded(J, [f]); mine.append(b)
                assert f == plain, "%s %s: %s" % (layout, chain, first_difference(f, plain))
            finally:
                for x in mine:
                    x.close()
    finally:
        S.close()


# ---------------------------------------------------------------------------------------------------------------- refusals, wrappers
def test_every_refusal_leaves_the_previous_result_alone(J):
    from jpegsnoop_amd import capi
    S = made(J, [("4:2:0", 50, 70), ("grey", 33, 31)])
    fresh = J.JpegBatch()
    t = S.b.transform("rot90", images=[1, 0])
    try:
        files = t.export(huffman="optimal")
        before = (t.coefs(0), t.coefs(1), t.entries(), t.export_results())
        lib = t._lib
        good = capi.transform_spec(lib, "flip_h")
        ind = (C.c_int * 2)(0, 1)

        def refused(word, spec=good, batch=S.b._h, images=ind, n=2, obj=t._h):
            assert lib.jsnoop_transform_run(obj, batch, C.byref(spec) if spec is not None else None, images, n) == -1
            assert word.encode() in lib.jsnoop_last_error(), (word, lib.jsnoop_last_error())

        refused("transform object is NULL", obj=None); refused("batch is NULL", batch=None); refused("spec is NULL", spec=None)
        refused("n = -1", n=-1); refused("out of range", images=(C.c_int * 2)(0, 2)); refused("out of range", images=(C.c_int * 2)(-1, 0)); refused("without a list", images=None, n=3)
        for field, value, word in [("op", 8, "unknown op"), ("op", -1, "unknown op"), ("edge", 2, "unknown edge"), ("grayscale", 2, "grayscale"), ("crop", 2, "crop is 2"),
                                   ("crop_x", 4, "while crop is 0"), ("crop_w", 4, "while crop is 0"), ("reserved", 1, "reserved"), ("struct_size", 3, "struct_size"),
                                   ("struct_size", 44, "struct_size")]:
            s = capi.transform_spec(lib, "flip_h"); setattr(s, field, value)
            refused(word, spec=s)
        for crop in ((0, 0, 0, 5), (0, 0, 5, 0)):
            refused("crop size", spec=capi.transform_spec(lib, "none", crop=crop))
        fresh.add_jpeg(TC.jpeg_file("grey", 8, 8, 1)[0])
        refused("has not been decoded", batch=fresh._h, n=1)
        with pytest.raises(RuntimeError, match="out of range"):
            t.export(images=[0, 2])
        with pytest.raises(RuntimeError):
            t.export(progressive=[((0, 1, 2), 0, 0, 0, 0), ((0,), 1, 63, 0, 1)])              # AC successive approximation: refused as for a batch
        after = (t.coefs(0), t.coefs(1), t.entries(), t.export_results())
        assert len(t) == 2 and before[2:] == after[2:] and all(np.array_equal(x, y) for k in (0, 1) for x, y in zip(before[k], after[k]))
        buf = (C.c_uint8 * len(files[0]))()
        assert lib.jsnoop_transform_read_export(t._h, 0, buf, len(files[0])) == len(files[0]) and bytes(buf) == files[0]
        assert t.run(S.b, "none", []) == [] and len(t) == 0 and t.export_results() == []
        with pytest.raises(RuntimeError, match="nothing has been transformed"):
            t.export()
    finally:
        t.close(); fresh.close(); S.close()


def test_torch_cpp_and_raw_pointer_paths(J, torch, tmp_path):
    shapes = [("4:2:0", 50, 70), ("grey", 33, 31), ("4:2:2", 15, 9)]
    S = made(J, shapes)
    try:
        want = []
        for i in range(3):
            R = M.transform(*S.src[i], M.ROT_270)
            want.append(EM.export_file(R.arena, R.dccum, R.geo, R.dim_x, R.dim_y, R.qnat)[2] if R.result == M.OK else None)
        assert want[2] is None and want[0] and want[1]               # 15 wide at 4:2:2: nothing left of a reversed x axis
        t = S.b.transform("rot270")
        try:
            assert [e["result"] for e in t.entries()] == [M.OK, M.OK, M.EMPTY]
            assert t.export() == want[:2]
            on_dev = t.export_to_torch(device=S.b.device())
            assert [bytes(x.cpu().numpy()) for x in on_dev] == want[:2] and all(x.is_cuda for x in on_dev)
            res = t.export_results()                                  # the raw pointers: the files where they lie, copied by torch
            for k in range(2):
                n = res[k]["len"]; dst = torch.empty(n, dtype=torch.uint8, device="cuda")
                assert t._lib.jsnoop_transform_export_copy(t._h, k, dst.data_ptr(), n) == n
                host = (C.c_uint8 * n)()
                assert t._lib.jsnoop_transform_read_export(t._h, k, host, n) == n   # (waits for the stream: the copy above is done)
                assert bytes(dst.cpu().numpy()) == want[k] == bytes(host)
        finally:
            t.close()
        exe = str(tmp_path / "transform_demo")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "transform_demo.cpp"),
                               "-L" + os.path.join(ROOT, "jpegsnoop_amd"), "-ljsnoop_gpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "jpegsnoop_amd"), "-Wl,-rpath,/opt/rocm/lib"])
        paths = []
        for k, (layout, w, h) in enumerate(shapes):
            p = tmp_path / ("in%d.jpg" % k); p.write_bytes(TC.jpeg_file(layout, w, h, 17 * k + w + h, k % 3)[0]); paths.append(str(p))
        out = subprocess.check_output([exe, str(tmp_path), str(M.ROT_270), "0", "0"] + paths, text=True).split()
        assert out == ["0", "0", str(len(want[0])), "1", "0", str(len(want[1])), "2", str(M.EMPTY), "0"]
        for k in range(2):
            assert open(str(tmp_path / ("out%d.jpg" % k)), "rb").read() == want[k]
    finally:
        S.close()
