"""-m gpu: jsnoop_batch_pack / k_pack_rgb (jsnoop_pack.hip) and JpegBatch.to_torch -- a decoded batch as cropped, top-down, three-channel
pixels in caller-owned device memory.

Every comparison is exact (np.array_equal / torch.equal) against tests/pack_model.py applied to the batch's own DIB (JpegBatch.dib, the D2H
copy every parity test pins), and once per layout against the model applied to the ORACLE's DIB of the same files.  Raw calls write into an
arena of 0xA5 bytes: a guard band in front of, behind and between the destinations and in every pitch gap, and the whole arena is compared with
what the model predicts -- a stray write anywhere shows.  Images are tiny; the one larger case is there for the deal of work over many
workgroups."""
import ctypes as C

import numpy as np
import pytest

import prog_cases as PC
from pack_model import pack_model, tells_fma_apart

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 5, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 333]
HEIGHTS = [1, 7, 8, 9, 17, 217]
SAMPLINGS = [dict(hs=1, vs=1), dict(hs=2, vs=1), dict(hs=2, vs=2), dict(gray=1)]            # 4:4:4, 4:2:2, 4:2:0, grayscale
SCALE, BIAS = (1 / 255, 1 / 255, 1 / 255), (-0.485, -0.456, -0.406)
SCALE2, BIAS2 = (0.1, 1 / 3, 0.7), (0.3, -1 / 7, 1e-3)                                      # none of them a float32
FORMS = [("HWC", "uint8"), ("CHW", "uint8"), ("HWC", "float32"), ("CHW", "float32")]
GUARD = 64


def seam_shapes():
    """Every width with two heights and two samplings (a sparse crossing), plus the corners the issue names: padding of 15 columns and 15 rows."""
    out = []
    for k, w in enumerate(WIDTHS):
        out.append((w, HEIGHTS[k % 6], k % 4))
        out.append((w, HEIGHTS[(5 * k + 3) % 6], (k + 1) % 4))
    out += [(1, 1, 2), (17, 17, 2), (333, 217, 2), (129, 217, 0), (333, 1, 3)]
    return out


# ------------------------------------------------------------------------------------------------ helpers
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


def raw_pack(J, b, spec, images, dsts):
    """jsnoop_batch_pack as a C caller makes it: dsts = [(ptr, row_pitch, plane_pitch)].  Returns the call's value; does not wait."""
    n = len(dsts)
    arr = (J.capi.PackDst * max(n, 1))(*[J.capi.PackDst(p, rp, pp) for p, rp, pp in dsts])
    ind = (C.c_int * max(n, 1))(*images) if images is not None else None
    return J.load().jsnoop_batch_pack(b._h, C.byref(spec), ind, n, arr)


def dense_row(w, layout, elem):
    return w * elem * (3 if layout == "HWC" else 1)


class Arena:
    """One device allocation of 0xA5 bytes holding every destination of a call, and the bytes the model says it must hold afterwards."""

    def __init__(self, torch, sizes, lead=0):
        self.offs, pos = [], GUARD
        for nb in sizes:
            pos = (pos + 15) // 16 * 16 + lead
            self.offs.append(pos)
            pos += nb + GUARD
        self.buf = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.expect = np.full(pos, 0xA5, np.uint8)
        self.sizes = sizes

    def ptr(self, k):
        return self.buf.data_ptr() + self.offs[k]

    def place(self, k, model, layout, rp, pp):
        """The model's bytes at destination k under the given pitches; everything else of the region stays 0xA5."""
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


def pack_and_check(J, torch, b, models, dims, layout, dtype, bgr, images, lead=0, row_extra=0, plane_extra=0, scale=None, bias=None, what=""):
    """One raw call for `images` with the given destination shape, then the whole arena against the model."""
    elem = 4 if dtype == "float32" else 1
    geo = []
    for i in images:
        h, w = dims[i]
        rp = dense_row(w, layout, elem) + row_extra
        pp = h * rp + plane_extra
        geo.append((rp, pp, h * rp if layout == "HWC" else 3 * pp))
    ar = Arena(torch, [g[2] for g in geo], lead)
    for k, i in enumerate(images):
        ar.place(k, models(i, layout, dtype, bgr, scale, bias), layout, geo[k][0], geo[k][1])
    dense = row_extra == 0 and plane_extra == 0
    dsts = [(ar.ptr(k), 0 if dense and k % 2 else geo[k][0], 0 if dense and k % 2 else (geo[k][1] if layout == "CHW" else 0)) for k in range(len(images))]
    torch.cuda.synchronize()                                      # (the fill above ran on torch's stream, the pack runs on the batch's)
    rc = raw_pack(J, b, make_spec(J, layout, dtype, bgr, scale, bias), images, dsts)
    assert rc == 0, J.last_error()
    torch.cuda.synchronize()
    ar.check("%s %s %s bgr=%d lead=%d row+%d plane+%d" % (what, layout, dtype, bgr, lead, row_extra, plane_extra))


class Models:
    """pack_model over a list of DIBs, every (image, form) computed once."""

    def __init__(self, dibs, dims):
        self.dibs, self.dims, self.memo = dibs, dims, {}

    def __call__(self, i, layout, dtype, bgr=False, scale=None, bias=None):
        key = (i, layout, dtype, bool(bgr), scale, bias)
        if key not in self.memo:
            h, w = self.dims[i]
            m = pack_model(self.dibs[i], w, h, layout, dtype, bgr, scale or (1.0, 1.0, 1.0), bias or (0.0, 0.0, 0.0))
            m.setflags(write=False)
            self.memo[key] = m
        return self.memo[key]


def decoded_batch(J, files, **kw):
    b = J.JpegBatch(**kw)
    for f in files:
        b.add_jpeg(f)
    b.upload(); b.decode(); b.sync()
    return b


def models_of(b):
    n = len(b)
    dims = [(b.info(i)["dim_y"], b.info(i)["dim_x"]) for i in range(n)]
    return Models([b.dib(i) for i in range(n)], dims), dims


# ------------------------------------------------------------------------------------------------ the seam batch
@pytest.fixture(scope="module")
def seam(harness, oracle):
    import jpegsnoop_amd as J
    import torch
    shapes = seam_shapes()
    files = [harness.synth_jpeg(width=w, height=h, quality=90, seed=700 + k, **SAMPLINGS[s]) for k, (w, h, s) in enumerate(shapes)]
    b = decoded_batch(J, files)
    models, dims = models_of(b)
    assert dims == [(h, w) for w, h, _ in shapes]
    pads = [(b.info(i)["img_x"] - w, b.info(i)["img_y"] - h) for i, (w, h, _) in enumerate(shapes)]
    assert max(p[0] for p in pads) == 15 and max(p[1] for p in pads) == 15
    odibs = []
    for f in files:
        harness.drive(oracle, f)
        odibs.append(oracle.dib().copy())
    yield dict(J=J, torch=torch, b=b, files=files, models=models, dims=dims, oracle_models=Models(odibs, dims), n=len(files))
    b.close()


@pytest.mark.parametrize("layout,dtype", FORMS)
@pytest.mark.parametrize("bgr", [False, True])
def test_every_form_over_the_width_and_height_seams(seam, layout, dtype, bgr):
    """All images of the mixed batch in ONE call per form: widths around the 4-pixel group, the 64-lane wave and the 512-pixel unit, heights of one row
    to more rows than one workgroup's share, MCU padding of up to 15 columns and rows that must not be read as pixels."""
    J, torch, b = seam["J"], seam["torch"], seam["b"]
    sb = (None, None) if dtype == "uint8" else ((SCALE, BIAS) if not bgr else (SCALE2, BIAS2))
    pack_and_check(J, torch, b, seam["models"], seam["dims"], layout, dtype, bgr, list(range(seam["n"])), scale=sb[0], bias=sb[1], what="seams")


@pytest.mark.parametrize("layout", ["HWC", "CHW"])
def test_exact_against_the_model_on_the_oracles_dib(seam, layout):
    J, torch, b = seam["J"], seam["torch"], seam["b"]
    pack_and_check(J, torch, b, seam["oracle_models"], seam["dims"], layout, "uint8", False, list(range(seam["n"])), what="oracle DIB")
    pack_and_check(J, torch, b, seam["oracle_models"], seam["dims"], layout, "float32", True, list(range(seam["n"])), scale=SCALE, bias=BIAS, what="oracle DIB")


# ------------------------------------------------------------------------------------------------ destination alignment
@pytest.mark.parametrize("lead", [1, 2, 3])
@pytest.mark.parametrize("row_extra", [0, 1, 13])
def test_hwc_uint8_at_every_byte_alignment(seam, lead, row_extra):
    """Base pointer 1, 2, 3 bytes off a 16-byte line; row_pitch dense (rows of odd width then start at every alignment), + 1 (odd) and + 13."""
    pack_and_check(seam["J"], seam["torch"], seam["b"], seam["models"], seam["dims"], "HWC", "uint8", False, list(range(seam["n"])),
                   lead=lead, row_extra=row_extra, what="alignment")


@pytest.mark.parametrize("dtype,lead,row_extra,plane_extra", [("uint8", 0, 0, 5), ("uint8", 3, 3, 1), ("uint8", 1, 0, 0), ("float32", 0, 0, 16), ("float32", 4, 8, 12),
                                                             ("float32", 12, 4, 0)])
def test_chw_with_pitched_rows_and_planes(seam, dtype, lead, row_extra, plane_extra):
    """plane_pitch above the dense plane (odd for uint8), pitched rows, bases off the 16-byte line; float pitches are multiples of 4 only."""
    sb = (SCALE, BIAS) if dtype == "float32" else (None, None)
    pack_and_check(seam["J"], seam["torch"], seam["b"], seam["models"], seam["dims"], "CHW", dtype, True, list(range(seam["n"])),
                   lead=lead, row_extra=row_extra, plane_extra=plane_extra, scale=sb[0], bias=sb[1], what="pitched CHW")


def test_hwc_float_with_pitched_rows(seam):
    pack_and_check(seam["J"], seam["torch"], seam["b"], seam["models"], seam["dims"], "HWC", "float32", False, list(range(seam["n"])),
                   lead=8, row_extra=20, scale=SCALE2, bias=BIAS2, what="pitched HWC float")


def test_refusals_launch_nothing_and_write_nothing(seam):
    J, torch, b, n = seam["J"], seam["torch"], seam["b"], seam["n"]
    i = next(k for k, (h, w) in enumerate(seam["dims"]) if (h, w) == (217, 333))
    ar = Arena(torch, [333 * 217 * 12])
    p = ar.ptr(0)
    torch.cuda.synchronize()
    u8h, u8c = make_spec(J, "HWC", "uint8"), make_spec(J, "CHW", "uint8")
    f32h, f32c = make_spec(J, "HWC", "float32"), make_spec(J, "CHW", "float32")
    bad_layout, bad_dtype, too_long = make_spec(J, "HWC", "uint8"), make_spec(J, "HWC", "uint8"), make_spec(J, "HWC", "uint8")
    bad_layout.layout, bad_dtype.dtype, too_long.struct_size = 2, 7, C.sizeof(J.capi.PackSpec) + 8
    cases = [("index past the end", u8h, [n], [(p, 0, 0)], "out of range"), ("negative index", u8h, [-1], [(p, 0, 0)], "out of range"),
             ("second index bad", u8h, [i, n + 3], [(p, 0, 0), (p, 0, 0)], "out of range"),
             ("NULL pointer", u8h, [i], [(0, 0, 0)], "NULL"), ("row_pitch below dense", u8h, [i], [(p, 998, 0)], "row_pitch"),
             ("CHW row_pitch below dense", u8c, [i], [(p, 332, 0)], "row_pitch"), ("plane_pitch below dense", u8c, [i], [(p, 333, 333 * 217 - 1)], "plane_pitch"),
             ("float pointer", f32h, [i], [(p + 2, 0, 0)], "multiples of 4"), ("float row_pitch", f32c, [i], [(p, 1334, 0)], "multiples of 4"),
             ("float plane_pitch", f32c, [i], [(p, 1332, 1332 * 217 + 2)], "multiples of 4"),
             ("unknown layout", bad_layout, [i], [(p, 0, 0)], "layout"), ("unknown dtype", bad_dtype, [i], [(p, 0, 0)], "dtype"),
             ("struct_size of a later version", too_long, [i], [(p, 0, 0)], "struct_size")]
    for what, spec, images, dsts, word in cases:
        assert raw_pack(J, b, spec, images, dsts) == -1, what
        assert word in J.last_error(), (what, J.last_error())
    # a batch that has not been decoded
    nb = J.JpegBatch()
    try:
        nb.add_jpeg(seam["files"][0])
        assert raw_pack(J, nb, u8h, [0], [(p, 0, 0)]) == -1 and "not been decoded" in J.last_error()
        nb.upload()
        assert raw_pack(J, nb, u8h, [0], [(p, 0, 0)]) == -1 and "not been decoded" in J.last_error()
    finally:
        nb.close()
    torch.cuda.synchronize()
    assert ar.untouched()
    # n == 0 is accepted; a shorter struct (an older caller's) takes the defaults for what it lacks
    assert raw_pack(J, b, u8h, None, []) == 0
    short = make_spec(J, "CHW", "float32", scale=(9.0, 9.0, 9.0)); short.struct_size = 16
    assert raw_pack(J, b, short, [i], [(p, 0, 0)]) == 0, J.last_error()
    torch.cuda.synchronize()
    ar.place(0, seam["models"](i, "CHW", "float32"), "CHW", 1332, 1332 * 217)
    ar.check("short struct")
    assert J.load().jsnoop_batch_pack_bytes(b._h, C.byref(f32c), i) == 333 * 217 * 12 and b.pack_bytes(i, "HWC") == 333 * 217 * 3


# ------------------------------------------------------------------------------------------------ subsets and order
def test_subset_in_any_order_into_one_allocation(seam):
    J, torch, b, n, models = seam["J"], seam["torch"], seam["b"], seam["n"], seam["models"]
    order = [n - 1, 4, 17, 0, 9]
    pack_and_check(J, torch, b, models, seam["dims"], "HWC", "uint8", False, order, what="subset")
    pack_and_check(J, torch, b, models, seam["dims"], "CHW", "float32", False, [5, 5, 2], scale=SCALE, bias=BIAS, what="an image listed twice")
    ts = b.to_torch(images=order, layout="CHW")
    assert len(ts) == len(order) and len({t.untyped_storage().data_ptr() for t in ts}) == 1
    for t, i in zip(ts, order):
        assert t.dtype == torch.uint8 and t.is_cuda and tuple(t.shape) == (3,) + seam["dims"][i]
        assert np.array_equal(t.cpu().numpy(), models(i, "CHW", "uint8"))
    assert b.to_torch(images=[]) == []
    with pytest.raises(IndexError):
        b.to_torch(images=[0, n])


# ------------------------------------------------------------------------------------------------ float exactness
@pytest.mark.parametrize("scale,bias", [(SCALE, BIAS), (SCALE2, BIAS2)])
def test_float_form_is_multiply_then_add_never_fused(seam, scale, bias):
    """The constants tell a fused multiply-add apart (a condition on the inputs, checked here on the CPU: on the very DIB bytes of this batch a model
    with ONE rounding differs from the model the kernel must match), so a contracted kernel fails the exact comparison."""
    J, torch, b, models, dims = seam["J"], seam["torch"], seam["b"], seam["models"], seam["dims"]
    assert all(len(a) > 0 for a in tells_fma_apart(scale, bias))
    i = next(k for k, d in enumerate(dims) if d == (217, 333))
    two = models(i, "HWC", "float32", False, scale, bias)
    u8 = models(i, "HWC", "uint8").astype(np.float64)
    fused = (u8 * np.asarray(scale, np.float32).astype(np.float64) + np.asarray(bias, np.float32).astype(np.float64)).astype(np.float32)
    assert not np.array_equal(two, fused), "these pixels would not tell a fused kernel apart"
    for layout in ("HWC", "CHW"):
        t = b.to_torch(images=[i], layout=layout, dtype=torch.float32, scale=scale, bias=bias)[0]
        assert t.dtype == torch.float32
        assert np.array_equal(t.cpu().numpy(), models(i, layout, "float32", False, scale, bias))


# ------------------------------------------------------------------------------------------------ ordering behind every decode form
def test_pack_waits_for_both_halves_of_a_two_stream_decode(harness):
    """Full-IDCT batch on two streams: the pack is enqueued right behind decode(), before anything has waited."""
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=333, height=217, seed=40 + k) for k in range(5)]
    b = J.JpegBatch()
    try:
        for f in files:
            b.add_jpeg(f)
        b.set_split(2); b.upload()
        assert b.split_parts() == 2
        sizes = [333 * 217 * 3] * 5
        ar = Arena(torch, sizes)
        torch.cuda.synchronize()
        b.decode()
        assert raw_pack(J, b, make_spec(J, "HWC", "uint8"), None, [(ar.ptr(k), 0, 0) for k in range(5)]) == 0, J.last_error()
        b.sync()
        assert b.last_form() == 1
        models, _ = models_of(b)
        for k in range(5):
            ar.place(k, models(k, "HWC", "uint8"), "HWC", 999, 0)
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
        ts = b.to_torch(layout="HWC", bgr=True)
        assert b.last_form() == 2, "the pack must not force a second decode"
        oracle.set_options(decode_ac=0)
        try:
            for k, f in enumerate(files):
                harness.drive(oracle, f)
                assert np.array_equal(ts[k].cpu().numpy(), pack_model(oracle.dib(), 100, 75, "HWC", "uint8", True)), k
        finally:
            oracle.set_options()
        assert b.last_form() == 2
    finally:
        b.close()


def test_progressive_batch(harness):
    import jpegsnoop_amd as J
    import torch
    c = PC.built(PC.NAMES[0])
    b = decoded_batch(J, [c.file, c.file])
    try:
        models, dims = models_of(b)
        ts = b.to_torch(layout="CHW", dtype=torch.float32, scale=SCALE, bias=BIAS)
        for k in range(2):
            assert tuple(ts[k].shape) == (3,) + dims[k]
            assert np.array_equal(ts[k].cpu().numpy(), models(k, "CHW", "float32", False, SCALE, BIAS))
    finally:
        b.close()


def test_damaged_file_arrives_repaired_behind_sync(harness, oracle):
    """One flipped bit in the middle of the scan of one file of a batch, one that the reference's decode reports as bad scan data: the file is flagged, stays
    on the parallel path and is repaired at sync(); a pack enqueued behind sync() holds the reference's pixels of the damaged file."""
    import jpegsnoop_amd as J
    import torch
    base = harness.synth_jpeg(width=333, height=217, seed=61)
    harness.drive(oracle, base)
    clean = oracle.dib().copy()
    p = harness.parse_jpeg(base)
    at = p.scan_start + int((p.scan_end - p.scan_start) * 0.6)
    hurt, hurt_dib = None, None
    for bit in (0x10, 0x08, 0x20, 0x04, 0x40, 0x80, 0x01, 0x02):  # (most flips in noise re-synchronise silently: the first one the reference's own decode reports)
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
        print("damaged image: flags 0x%04x path %d" % (b.info(1)["flags"], b.info(1)["path"]))
        assert b.info(1)["flags"] != 0 and b.info(1)["path"] == 1, "the flip must leave a flagged file on the parallel path"
        ts = b.to_torch(layout="HWC")
        assert np.array_equal(ts[1].cpu().numpy(), pack_model(hurt_dib, 333, 217, "HWC"))
        assert np.array_equal(ts[0].cpu().numpy(), pack_model(clean, 333, 217, "HWC")) and torch.equal(ts[0], ts[2])
        assert not torch.equal(ts[0], ts[1])
    finally:
        b.close()


def test_same_handle_decoded_and_packed_again(harness):
    """decode, pack, decode, pack on one handle; then the handle cleared and refilled with more images (the record block grows) and packed twice in a row."""
    import jpegsnoop_amd as J
    import torch
    first = [harness.synth_jpeg(width=65, height=17, seed=80), harness.synth_jpeg(width=33, height=9, hs=1, vs=1, seed=81)]
    b = decoded_batch(J, first)
    try:
        models, _ = models_of(b)
        for _ in range(2):
            ts = b.to_torch(layout="HWC")
            for k in range(2):
                assert np.array_equal(ts[k].cpu().numpy(), models(k, "HWC", "uint8"))
            b.decode()
        b.clear()
        more = [harness.synth_jpeg(width=16 + 3 * k, height=8 + k, seed=90 + k) for k in range(40)]
        for f in more:
            b.add_jpeg(f)
        b.upload(); b.decode(); b.sync()
        models, dims = models_of(b)
        a = b.to_torch(layout="CHW")
        h = b.to_torch(layout="HWC", bgr=True)
        for k in range(40):
            assert np.array_equal(a[k].cpu().numpy(), models(k, "CHW", "uint8")), k
            assert np.array_equal(h[k].cpu().numpy(), models(k, "HWC", "uint8", True)), k
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ the Python surface
def test_to_torch_forms(seam):
    J, torch, b, models, dims = seam["J"], seam["torch"], seam["b"], seam["models"], seam["dims"]
    dev = torch.device("cuda", b.device())
    same = [next(k for k, d in enumerate(dims) if d == (217, 333))] * 3
    mixed = [0, 5, same[0], 12]
    # list
    ts = b.to_torch(images=mixed, layout="HWC", dtype=torch.float32, scale=2.0, bias=(0.5, 0.25, 0.125))
    for t, i in zip(ts, mixed):
        assert t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == dims[i] + (3,) and t.is_contiguous()
        assert np.array_equal(t.cpu().numpy(), models(i, "HWC", "float32", False, (2.0, 2.0, 2.0), (0.5, 0.25, 0.125)))
    # stack
    st = b.to_torch(images=same, layout="CHW", stack=True)
    assert st.dtype == torch.uint8 and st.device == dev and tuple(st.shape) == (3, 3, 217, 333)
    for k in range(3):
        assert np.array_equal(st[k].cpu().numpy(), models(same[0], "CHW", "uint8"))
    with pytest.raises(ValueError, match="image %d " % mixed[1]):
        b.to_torch(images=mixed, stack=True)
    # pad_to: every image in the top-left corner of its slot, zeros elsewhere
    for layout in ("CHW", "HWC"):
        pt = b.to_torch(images=mixed, layout=layout, pad_to=(224, 340))
        assert pt.dtype == torch.uint8 and pt.device == dev and tuple(pt.shape) == ((4, 3, 224, 340) if layout == "CHW" else (4, 224, 340, 3))
        got = pt.cpu().numpy()
        want = np.zeros_like(got)
        for k, i in enumerate(mixed):
            h, w = dims[i]
            if layout == "CHW":
                want[k, :, :h, :w] = models(i, "CHW", "uint8")
            else:
                want[k, :h, :w, :] = models(i, "HWC", "uint8")
        assert np.array_equal(got, want), layout
    with pytest.raises(ValueError, match="larger than pad_to"):
        b.to_torch(images=mixed, pad_to=(216, 340))
    # out=: a tensor with room around every image keeps what it held there; a list of exact tensors
    out = torch.full((4, 3, 220, 336), 7, dtype=torch.uint8, device=dev)
    assert b.to_torch(images=mixed, out=out) is out
    got = out.cpu().numpy(); want = np.full_like(got, 7)
    for k, i in enumerate(mixed):
        h, w = dims[i]; want[k, :, :h, :w] = models(i, "CHW", "uint8")
    assert np.array_equal(got, want)
    outs = [torch.empty(dims[i] + (3,), dtype=torch.float32, device=dev) for i in mixed]
    assert b.to_torch(images=mixed, layout="HWC", dtype=torch.float32, out=outs) is outs
    for t, i in zip(outs, mixed):
        assert np.array_equal(t.cpu().numpy(), models(i, "HWC", "float32"))
    # what out= refuses in Python, before the call
    with pytest.raises(ValueError, match="cpu"):
        b.to_torch(images=mixed, out=torch.empty((4, 3, 220, 336), dtype=torch.uint8))
    with pytest.raises(ValueError, match="float32"):
        b.to_torch(images=mixed, out=torch.empty((4, 3, 220, 336), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="larger than out"):
        b.to_torch(images=mixed, out=torch.empty((4, 3, 200, 336), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="shape"):
        b.to_torch(images=mixed, layout="HWC", out=[torch.empty((5, 5, 3), dtype=torch.uint8, device=dev)] * 4)
    with pytest.raises(ValueError, match="contiguous"):
        b.to_torch(images=mixed, out=torch.empty((4, 3, 220, 672), dtype=torch.uint8, device=dev)[:, :, :, ::2])
    with pytest.raises(ValueError):
        b.to_torch(layout="NCHW")
    with pytest.raises(ValueError):
        b.to_torch(dtype=torch.float16)
    with pytest.raises(ValueError):
        b.to_torch(scale=2.0)                                     # (scale belongs to the float form)


def test_job_file_result_to_torch_inside_the_callback(harness):
    """A JpegJob over baseline and progressive files on one device: every file's tensor taken inside the callback equals the model on the DIB the same
    callback reads from the same (batch, image)."""
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=65, height=33, seed=21), PC.built(PC.NAMES[0]).file, harness.synth_jpeg(width=17, height=9, gray=1, seed=22),
             PC.built(PC.NAMES[1]).file, b"not a jpeg"]
    job = J.JpegJob(devices=[0])
    try:
        for f in files:
            job.add(f)
        seen = {}

        def on_file(r):
            if r.status != "ok":
                with pytest.raises(RuntimeError):
                    r.to_torch()
                seen[r.index] = None
                return False
            dib = r.batch.dib(r.image)
            h, w = r.info["dim_y"], r.info["dim_x"]
            t = r.to_torch(layout="HWC")
            f = r.to_torch(layout="CHW", dtype=torch.float32, scale=SCALE, bias=BIAS, stack=True)
            assert t.device == torch.device("cuda", r.device) and tuple(t.shape) == (h, w, 3) and tuple(f.shape) == (1, 3, h, w)
            seen[r.index] = (r.kind, np.array_equal(t.cpu().numpy(), pack_model(dib, w, h, "HWC")),
                             np.array_equal(f[0].cpu().numpy(), pack_model(dib, w, h, "CHW", "float32", False, SCALE, BIAS)))
            return False
        stats = job.run(on_file)
        assert stats["ok"] == 4 and stats["refused"] == 1
        assert [seen[i] and seen[i][0] for i in range(5)] == ["baseline", "progressive", "baseline", "progressive", None]
        assert all(seen[i][1] and seen[i][2] for i in range(4)), seen
    finally:
        job.close()


# ------------------------------------------------------------------------------------------------ the deal over many workgroups
def test_eight_1080p_and_one_2160p_in_one_call(harness):
    """More units than one round of workgroups takes, images of two sizes in one list: every tensor against the model, compared on the device."""
    import jpegsnoop_amd as J
    import torch
    f1080 = [harness.synth_jpeg(width=1920, height=1080, seed=s) for s in (5, 6)]
    f2160 = harness.synth_jpeg(width=3840, height=2160, seed=7)
    files = [f1080[k % 2] for k in range(8)] + [f2160]
    b = decoded_batch(J, files)
    try:
        want = {}
        for i in (0, 1, 8):
            inf = b.info(i)
            want[i] = torch.from_numpy(pack_model(b.dib(i), inf["dim_x"], inf["dim_y"], "CHW")).cuda()
        ts = b.to_torch(layout="CHW")
        assert [tuple(t.shape) for t in ts] == [(3, 1080, 1920)] * 8 + [(3, 2160, 3840)]
        for k, t in enumerate(ts):
            assert torch.equal(t, want[8 if k == 8 else k % 2]), k
    finally:
        b.close()
