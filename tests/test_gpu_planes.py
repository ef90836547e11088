"""-m gpu: jsnoop_batch_pack_planes / k_pack_planes (jsnoop_planes.hip), JpegBatch.planes_to_torch and JobFileResult.planes_to_torch -- the retained
int16 planes of a decoded batch as one tensor per (image, component) in caller-owned device memory.

Every comparison is exact (np.array_equal / torch.equal) against tests/plane_model.py applied to the batch's own planes (JpegBatch.planes, the D2H copy),
and once per form against the model applied to the ORACLE's planes of the same files.  Raw calls write into an arena of 0xA5 bytes: a guard band in front
of, behind and between the destinations and in every pitch gap, and the whole arena is compared with what the model predicts -- a stray write anywhere
shows.  Images are tiny; the one larger case is there for the deal of work over many workgroups."""
import ctypes as C

import numpy as np
import pytest

import prog_cases as PC
from plane_model import expand_factors, fma_telling_values, plane_dims, plane_model

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 5, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 333, 511, 512, 513, 1023, 1025]
HEIGHTS = [1, 7, 8, 9, 17]
# 4:4:4, 4:2:2, 4:2:0, grayscale, 4:4:0, 4:1:1 (luma factors; chroma is 1 x 1)
SAMPLINGS = [dict(hs=1, vs=1), dict(hs=2, vs=1), dict(hs=2, vs=2), dict(gray=1), dict(hs=1, vs=2), dict(hs=4, vs=1)]
FORMS = [(res, dtype) for res in ("full", "native") for dtype in ("int16", "uint8", "float32")]
ELEM = {"int16": 2, "uint8": 1, "float32": 4}
SCALE, BIAS = (1 / 255, 1 / 219, 1 / 224), (-0.485, -0.456, -0.406)
SCALE2, BIAS2 = (0.1, 1 / 3, 0.7), (0.3, -1 / 7, 1e-3)                                      # none of them a float32
GUARD = 64


def seam_shapes():
    """Every width with two heights and two samplings (a sparse crossing), plus the corners: the 512-element unit seam under eh = 2 and eh = 4, the
    smallest dimensions (1, eh, eh + 1), padding of whole MCUs less one."""
    out = []
    for k, w in enumerate(WIDTHS):
        out.append((w, HEIGHTS[k % 5], k % 6))
        out.append((w, HEIGHTS[(3 * k + 2) % 5], (k + 3) % 6))
    out += [(1023, 9, 2), (1025, 8, 1), (1025, 17, 2), (1023, 7, 1), (513, 7, 5), (1025, 1, 5), (333, 17, 4), (17, 17, 2), (1, 1, 2), (2, 2, 2), (3, 3, 2), (4, 1, 5), (5, 2, 5),
            (1, 2, 4), (16, 3, 4), (512, 9, 0), (511, 17, 3)]
    return out


CLIP_SHAPE = (77, 24, 2)


def clip_picture(harness):
    """A 77 x 24 4:2:0 picture of black and white tiles at quality 30: the ringing takes the decoded samples out of the 8-bit range on both sides, so the U8
    form's clamp has something to clamp (the seam fixture checks that it does)."""
    w, h, _ = CLIP_SHAPE
    rgb = np.zeros((h, w, 3), np.uint8)
    rgb[(np.add.outer(np.arange(h) // 3, np.arange(w) // 5) % 2) == 1] = 255
    rgb[:, 40:, 0] = 255
    rgb[:, 60:, 2] = 0
    return harness.encode_rgb(rgb, hs=2, vs=2, quality=30)


def factors_of(s):
    kw = SAMPLINGS[s]
    return expand_factors(kw.get("hs", 1), kw.get("vs", 1), bool(kw.get("gray")))


# ------------------------------------------------------------------------------------------------ helpers
def make_spec(J, res, dtype, scale=None, bias=None):
    s = J.capi.PlaneSpec()
    J.load().jsnoop_plane_spec_defaults(C.byref(s))
    s.res = J.capi.PLANE_NATIVE if res == "native" else J.capi.PLANE_FULL
    s.dtype = {"int16": J.capi.PLANE_I16, "uint8": J.capi.PLANE_U8, "float32": J.capi.PLANE_F32}[dtype]
    for c in range(3):
        if scale is not None:
            s.scale[c] = scale[c]
        if bias is not None:
            s.bias[c] = bias[c]
    return s


def raw_pack(J, b, spec, images, dsts):
    """jsnoop_batch_pack_planes as a C caller makes it: dsts = [(ptr, row_pitch, comp[, reserved])].  Returns the call's value; does not wait."""
    n = len(dsts)
    arr = (J.capi.PlaneDst * max(n, 1))(*[J.capi.PlaneDst(d[0], d[1], d[2], d[3] if len(d) > 3 else 0) for d in dsts])
    ind = (C.c_int * max(n, 1))(*images) if images is not None else None
    return J.load().jsnoop_batch_pack_planes(b._h, C.byref(spec), ind, n, arr)


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

    def place(self, k, model, rp):
        """The model's bytes at destination k under row pitch rp; everything else of the region stays 0xA5."""
        h = model.shape[0]
        row = np.ascontiguousarray(model).view(np.uint8).reshape(h, -1)
        reg = self.expect[self.offs[k]:self.offs[k] + self.sizes[k]]
        assert reg.size == h * rp
        reg.reshape(h, rp)[:, :row.shape[1]] = row

    def check(self, what):
        got = self.buf.cpu().numpy()
        if not np.array_equal(got, self.expect):
            bad = int(np.flatnonzero(got != self.expect)[0])
            k = max([i for i, o in enumerate(self.offs) if o <= bad], default=-1)
            raise AssertionError("%s: first wrong byte at arena offset %d (destination %d + %d): got 0x%02x, want 0x%02x; %d bytes differ"
                                 % (what, bad, k, bad - self.offs[k] if k >= 0 else bad, got[bad], self.expect[bad], int((got != self.expect).sum())))

    def untouched(self):
        return bool((self.buf == 0xA5).all().item())


class Models:
    """plane_model over the planes of a list of images, every (image, component, form) computed once."""

    def __init__(self, planes, dims, factors):
        self.planes, self.dims, self.factors, self.memo = planes, dims, factors, {}

    def ncomp(self, i):
        return len(self.factors[i])

    def pairs(self, images=None):
        return [(i, c) for i in (range(len(self.dims)) if images is None else images) for c in range(self.ncomp(i))]

    def __call__(self, i, c, res, dtype, scale=None, bias=None):
        key = (i, c, res, dtype, scale, bias)
        if key not in self.memo:
            h, w = self.dims[i]
            eh, ev = self.factors[i][c]
            m = plane_model(self.planes[i][c], w, h, eh, ev, res, dtype, (scale or (1.0,) * 3)[c], (bias or (0.0,) * 3)[c])
            m.setflags(write=False)
            self.memo[key] = m
        return self.memo[key]


def pack_and_check(J, torch, b, models, res, dtype, pairs, lead=0, row_extra=0, scale=None, bias=None, what=""):
    """One raw call for the (image, component) pairs with the given destination shape, then the whole arena against the model."""
    ms = [models(i, c, res, dtype, scale, bias) for i, c in pairs]
    rps = [m.shape[1] * ELEM[dtype] + row_extra for m in ms]
    ar = Arena(torch, [m.shape[0] * rp for m, rp in zip(ms, rps)], lead)
    for k, m in enumerate(ms):
        ar.place(k, m, rps[k])
    dsts = [(ar.ptr(k), 0 if row_extra == 0 and k % 2 else rps[k], pairs[k][1]) for k in range(len(pairs))]
    torch.cuda.synchronize()                                      # (the fill above ran on torch's stream, the pack runs on the batch's)
    rc = raw_pack(J, b, make_spec(J, res, dtype, scale, bias), [i for i, _ in pairs], dsts)
    assert rc == 0, J.last_error()
    torch.cuda.synchronize()
    ar.check("%s %s %s lead=%d row+%d" % (what, res, dtype, lead, row_extra))


def decoded_batch(J, files, **kw):
    b = J.JpegBatch(want_planes=True, **kw)
    for f in files:
        b.add_jpeg(f)
    b.upload(); b.decode(); b.sync()
    return b


def models_of(b, factors):
    n = len(b)
    dims = [(b.info(i)["dim_y"], b.info(i)["dim_x"]) for i in range(n)]
    planes = [b.planes(i) for i in range(n)]
    assert [len(p) for p in planes] == [len(f) for f in factors]
    return Models(planes, dims, factors)


# ------------------------------------------------------------------------------------------------ the seam batch
@pytest.fixture(scope="module")
def seam(harness, oracle):
    import jpegsnoop_amd as J
    import torch
    shapes = seam_shapes()
    files = [harness.synth_jpeg(width=w, height=h, quality=90, seed=1700 + k, **SAMPLINGS[s]) for k, (w, h, s) in enumerate(shapes)] + [clip_picture(harness)]
    shapes = shapes + [CLIP_SHAPE]
    factors = [factors_of(s) for _, _, s in shapes]
    b = decoded_batch(J, files)
    models = models_of(b, factors)
    assert models.dims == [(h, w) for w, h, _ in shapes]
    for i, fs in enumerate(factors):                              # the sizes the library reports are the model's, for every component and both resolutions
        for c, (eh, ev) in enumerate(fs):
            for native in (False, True):
                assert b.plane_size(i, c, native) == plane_dims(shapes[i][0], shapes[i][1], eh, ev, "native" if native else "full"), (i, c, native)
    clip = models(len(files) - 1, 0, "full", "int16")
    assert (clip > 1023).sum() > 100 and (clip < -1024).sum() > 100, "the clip picture must leave the 8-bit range on both sides"
    assert models(len(files) - 1, 1, "full", "int16").min() < -1024 and models(len(files) - 1, 2, "full", "int16").max() > 1023
    oplanes = []
    for f in files:
        harness.drive(oracle, f)
        oplanes.append([p.copy() for p in oracle.planes() if p is not None][:len(factors[len(oplanes)])])
    yield dict(J=J, torch=torch, b=b, files=files, shapes=shapes, models=models, oracle_models=Models(oplanes, models.dims, factors), n=len(files))
    b.close()


@pytest.mark.parametrize("res,dtype", FORMS)
def test_every_form_over_the_width_and_height_seams(seam, res, dtype):
    """Every component of every image of the mixed batch in ONE call per form: widths around the 8-element lane, the 64-lane wave and the 512-element
    unit (and their halves and quarters under eh = 2 and 4), heights of one row to several MCU rows, MCU padding that must not be read as samples."""
    J, torch, b, models = seam["J"], seam["torch"], seam["b"], seam["models"]
    sb = (SCALE, BIAS) if dtype == "float32" else (None, None)
    pack_and_check(J, torch, b, models, res, dtype, models.pairs(), scale=sb[0], bias=sb[1], what="seams")


@pytest.mark.parametrize("res,dtype", FORMS)
def test_exact_against_the_model_on_the_oracles_planes(seam, res, dtype):
    J, torch, b, om = seam["J"], seam["torch"], seam["b"], seam["oracle_models"]
    sb = (SCALE2, BIAS2) if dtype == "float32" else (None, None)
    pack_and_check(J, torch, b, om, res, dtype, om.pairs(), scale=sb[0], bias=sb[1], what="oracle planes")


# ------------------------------------------------------------------------------------------------ destination alignment
@pytest.mark.parametrize("lead", list(range(16)))
def test_uint8_at_every_byte_alignment(seam, lead):
    """Base pointer 0 .. 15 bytes off a 16-byte line; row_pitch dense + 1, + 2 and + 64 in turn, FULL and NATIVE in turn."""
    models = seam["models"]
    pack_and_check(seam["J"], seam["torch"], seam["b"], models, ("full", "native")[lead % 2], "uint8", models.pairs(), lead=lead, row_extra=(1, 2, 64)[lead % 3], what="alignment")


@pytest.mark.parametrize("lead", list(range(0, 16, 2)))
def test_int16_at_every_even_alignment(seam, lead):
    models = seam["models"]
    pack_and_check(seam["J"], seam["torch"], seam["b"], models, ("full", "native")[(lead // 2) % 2], "int16", models.pairs(), lead=lead, row_extra=(2, 64, 6)[(lead // 2) % 3],
                   what="alignment")


@pytest.mark.parametrize("res,lead,row_extra", [("full", 4, 4), ("native", 12, 64), ("full", 8, 0)])
def test_float_with_pitched_rows(seam, res, lead, row_extra):
    models = seam["models"]
    pack_and_check(seam["J"], seam["torch"], seam["b"], models, res, "float32", models.pairs(), lead=lead, row_extra=row_extra, scale=SCALE2, bias=BIAS2, what="pitched float")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing_and_write_nothing(seam, harness):
    J, torch, b, n, models = seam["J"], seam["torch"], seam["b"], seam["n"], seam["models"]
    i = next(k for k, s in enumerate(seam["shapes"]) if s == (333, 17, 4))
    g = next(k for k, s in enumerate(seam["shapes"]) if s[2] == 3)
    j = next(k for k, s in enumerate(seam["shapes"]) if s == (17, 17, 2))      # 4:2:0: nine columns on the chroma grid
    ar = Arena(torch, [333 * 17 * 4])
    p = ar.ptr(0)
    torch.cuda.synchronize()
    form0 = b.last_form()
    i16, u8, f32, nu8 = make_spec(J, "full", "int16"), make_spec(J, "full", "uint8"), make_spec(J, "full", "float32"), make_spec(J, "native", "uint8")
    bad_res, bad_dtype, too_long = make_spec(J, "full", "uint8"), make_spec(J, "full", "uint8"), make_spec(J, "full", "uint8")
    bad_res.res, bad_dtype.dtype, too_long.struct_size = 2, 3, C.sizeof(J.capi.PlaneSpec) + 4
    cases = [("index past the end", u8, [n], [(p, 0, 0)], "out of range"), ("negative index", u8, [-1], [(p, 0, 0)], "out of range"),
             ("second index bad", u8, [i, n + 3], [(p, 0, 0), (p, 0, 0)], "out of range"),
             ("component past the count", u8, [i], [(p, 0, 3)], "component"), ("component of a gray image", u8, [g], [(p, 0, 1)], "component"),
             ("component above 2", u8, [i], [(p, 0, 7)], "component"),
             ("NULL pointer", u8, [i], [(0, 0, 0)], "NULL"), ("reserved", u8, [i], [(p, 0, 0, 1)], "reserved"),
             ("row_pitch below dense", u8, [i], [(p, 332, 0)], "row_pitch"), ("int16 row_pitch below dense", i16, [i], [(p, 664, 0)], "row_pitch"),
             ("float row_pitch below dense", f32, [i], [(p, 1328, 0)], "row_pitch"), ("native row_pitch below its own dense row", nu8, [j], [(p, 8, 1)], "row_pitch"),
             ("int16 pointer", i16, [i], [(p + 1, 0, 0)], "multiples of 2"), ("int16 row_pitch", i16, [i], [(p, 667, 0)], "multiples of 2"),
             ("float pointer", f32, [i], [(p + 2, 0, 0)], "multiples of 4"), ("float row_pitch", f32, [i], [(p, 1334, 0)], "multiples of 4"),
             ("unknown res", bad_res, [i], [(p, 0, 0)], "res"), ("unknown dtype", bad_dtype, [i], [(p, 0, 0)], "dtype"),
             ("struct_size of a later version", too_long, [i], [(p, 0, 0)], "struct_size")]
    for what, spec, images, dsts, word in cases:
        assert raw_pack(J, b, spec, images, dsts) == -1, what
        assert word in J.last_error(), (what, J.last_error())
    lib = J.load()
    assert lib.jsnoop_batch_pack_planes(b._h, C.byref(u8), None, 1, None) == -1 and "NULL" in J.last_error()
    assert lib.jsnoop_batch_pack_planes(b._h, None, None, 1, (J.capi.PlaneDst * 1)(J.capi.PlaneDst(p, 0, 0, 0))) == -1 and "NULL" in J.last_error()
    assert lib.jsnoop_batch_pack_planes(None, C.byref(u8), None, 1, (J.capi.PlaneDst * 1)(J.capi.PlaneDst(p, 0, 0, 0))) == -1 and "NULL" in J.last_error()
    # a batch that has not been decoded; a batch that keeps no planes
    nb = J.JpegBatch(want_planes=True)
    try:
        nb.add_jpeg(seam["files"][0])
        assert raw_pack(J, nb, u8, [0], [(p, 0, 0)]) == -1 and "not been decoded" in J.last_error()
        nb.upload()
        assert raw_pack(J, nb, u8, [0], [(p, 0, 0)]) == -1 and "not been decoded" in J.last_error()
    finally:
        nb.close()
    np_ = J.JpegBatch()
    try:
        np_.add_jpeg(seam["files"][i])
        np_.upload(); np_.decode(); np_.sync()
        assert raw_pack(J, np_, u8, [0], [(p, 0, 0)]) == -1 and "want_planes" in J.last_error()
        with pytest.raises(RuntimeError, match="want_planes"):
            np_.planes_to_torch()
    finally:
        np_.close()
    torch.cuda.synchronize()
    assert ar.untouched() and b.last_form() == form0
    # n == 0 is accepted; a shorter struct (an older caller's) takes the defaults for what it lacks
    assert raw_pack(J, b, u8, None, []) == 0
    short = make_spec(J, "full", "float32", scale=(9.0, 9.0, 9.0)); short.struct_size = 12
    assert raw_pack(J, b, short, [i], [(p, 0, 0)]) == 0, J.last_error()
    torch.cuda.synchronize()
    ar.place(0, models(i, 0, "full", "float32"), 1332)
    ar.check("short struct")
    assert lib.jsnoop_batch_plane_bytes(b._h, C.byref(f32), i, 2) == 333 * 17 * 4 and lib.jsnoop_batch_plane_bytes(b._h, C.byref(nu8), i, 2) == 333 * 9
    assert lib.jsnoop_batch_plane_bytes(b._h, C.byref(f32), i, 3) == 0 and lib.jsnoop_batch_plane_bytes(b._h, C.byref(f32), n, 0) == 0
    assert b.last_form() == form0


# ------------------------------------------------------------------------------------------------ subsets and order
def test_subsets_repeats_and_null_lists(seam):
    J, torch, b, n, models = seam["J"], seam["torch"], seam["b"], seam["n"], seam["models"]
    order = [n - 1, 4, 17, 0, 9]
    pack_and_check(J, torch, b, models, "full", "uint8", models.pairs(order), what="subset")
    pack_and_check(J, torch, b, models, "native", "int16", [(i, c) for i in order for c in reversed(range(models.ncomp(i)))], what="components backwards")
    tri = next(k for k in range(n) if models.ncomp(k) == 3)
    pack_and_check(J, torch, b, models, "native", "float32", [(tri, 1), (tri, 1), (5, 0), (tri, 1)], scale=SCALE, bias=BIAS, what="a pair listed three times")
    # images == NULL: images 0 .. n - 1, here component 0 of each
    ms = [models(i, 0, "full", "uint8") for i in range(n)]
    ar = Arena(torch, [m.size for m in ms])
    for k, m in enumerate(ms):
        ar.place(k, m, m.shape[1])
    torch.cuda.synchronize()
    assert raw_pack(J, b, make_spec(J, "full", "uint8"), None, [(ar.ptr(k), 0, 0) for k in range(n)]) == 0, J.last_error()
    assert raw_pack(J, b, make_spec(J, "full", "uint8"), None, []) == 0
    torch.cuda.synchronize()
    ar.check("images == NULL")
    ts = b.planes_to_torch(images=order, native=True)
    assert [len(r) for r in ts] == [models.ncomp(i) for i in order] and len({t.untyped_storage().data_ptr() for r in ts for t in r}) == 1
    for r, i in zip(ts, order):
        for c, t in enumerate(r):
            assert t.dtype == torch.int16 and t.is_cuda and t.is_contiguous() and np.array_equal(t.cpu().numpy(), models(i, c, "native", "int16"))
    assert b.planes_to_torch(images=[]) == []
    with pytest.raises(IndexError):
        b.planes_to_torch(images=[0, n])
    with pytest.raises(IndexError):
        b.planes_to_torch(images=[tri], comps=[3])


# ------------------------------------------------------------------------------------------------ float exactness
@pytest.mark.parametrize("scale,bias", [(SCALE, BIAS), (SCALE2, BIAS2)])
def test_float_form_is_multiply_then_add_never_fused(seam, scale, bias):
    """The constants tell a fused multiply-add apart on sample values these very planes hold (checked here on the CPU: a model with ONE rounding differs
    from the model the kernel must match), so a contracted kernel fails the exact comparison."""
    J, torch, b, models = seam["J"], seam["torch"], seam["b"], seam["models"]
    tell = fma_telling_values(scale, bias)
    assert all(len(a) > 0 for a in tell)
    i = next(k for k, s in enumerate(seam["shapes"]) if s == (333, 17, 4))
    for c in range(3):
        v = models(i, c, "full", "int16")
        assert np.isin(v, tell[c]).any(), "component %d holds none of the telling values" % c
        two = models(i, c, "full", "float32", scale, bias)
        fused = (v.astype(np.float64) * float(np.float32(scale[c])) + float(np.float32(bias[c]))).astype(np.float32)
        assert not np.array_equal(two, fused), "these samples would not tell a fused kernel apart"
    for native in (False, True):
        ts = b.planes_to_torch(images=[i], native=native, dtype=torch.float32, scale=scale, bias=bias)[0]
        for c in range(3):
            assert ts[c].dtype == torch.float32 and np.array_equal(ts[c].cpu().numpy(), models(i, c, "native" if native else "full", "float32", scale, bias))


# ------------------------------------------------------------------------------------------------ ordering behind every decode form
def test_pack_waits_for_both_halves_of_a_two_stream_decode(harness):
    """Full-IDCT batch on two streams: the call is enqueued right behind decode(), before anything has waited."""
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=333, height=217, seed=40 + k) for k in range(5)]
    b = J.JpegBatch(want_planes=True)
    try:
        for f in files:
            b.add_jpeg(f)
        b.set_split(2); b.upload()
        assert b.split_parts() == 2
        pairs = [(k, c) for k in range(5) for c in range(3)]
        ar = Arena(torch, [333 * 217] * 15)
        torch.cuda.synchronize()
        b.decode()
        assert raw_pack(J, b, make_spec(J, "full", "uint8"), [k for k, _ in pairs], [(ar.ptr(j), 0, c) for j, (_, c) in enumerate(pairs)]) == 0, J.last_error()
        b.sync()
        assert b.last_form() == 1
        models = models_of(b, [expand_factors(2, 2)] * 5)
        for j, (k, c) in enumerate(pairs):
            ar.place(j, models(k, c, "full", "uint8"), 333)
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
        full = b.planes_to_torch()
        nat = b.planes_to_torch(native=True, dtype=torch.uint8)
        assert b.last_form() == 2, "the call must not force a second decode"
        oracle.set_options(decode_ac=0)
        try:
            for k, f in enumerate(files):
                harness.drive(oracle, f)
                op = oracle.planes()
                for c, (eh, ev) in enumerate(expand_factors(2, 2)):
                    assert np.array_equal(full[k][c].cpu().numpy(), plane_model(op[c], 100, 75, eh, ev, "full", "int16")), (k, c)
                    assert np.array_equal(nat[k][c].cpu().numpy(), plane_model(op[c], 100, 75, eh, ev, "native", "uint8")), (k, c)
        finally:
            oracle.set_options()
        assert b.last_form() == 2
    finally:
        b.close()


def test_progressive_batch(harness):
    import jpegsnoop_amd as J
    import torch
    f = harness.synth_jpeg(width=77, height=41, hs=2, vs=2, progressive=1, seed=31)
    b = decoded_batch(J, [f, PC.built(PC.NAMES[0]).file, f])
    try:
        ncomp = b.info(1)["ncomp"]
        for native in (False, True):
            ts = b.planes_to_torch(images=[0, 2], native=native, dtype=torch.float32, scale=SCALE, bias=BIAS)
            for k, i in enumerate((0, 2)):
                ps = b.planes(i)
                for c, (eh, ev) in enumerate(expand_factors(2, 2)):
                    assert np.array_equal(ts[k][c].cpu().numpy(), plane_model(ps[c], 77, 41, eh, ev, "native" if native else "full", "float32", SCALE[c], BIAS[c])), (native, i, c)
        # a file of the progressive catalogue, whatever its layout: FULL is the crop of what read_planes gives
        ts = b.planes_to_torch(images=[1])[0]
        inf, ps = b.info(1), b.planes(1)
        assert len(ts) == ncomp
        for c in range(ncomp):
            assert np.array_equal(ts[c].cpu().numpy(), ps[c][:inf["dim_y"], :inf["dim_x"]]), c
    finally:
        b.close()


def test_damaged_file_arrives_repaired_behind_sync(harness, oracle):
    """One flipped bit in the middle of the scan of one file of a batch, one that the reference's decode reports as bad scan data (built as
    test_gpu_pack.py builds it): the file is flagged, stays on the parallel path and is repaired at sync().  A call enqueued before sync() is accepted and
    sees what the parallel path left; a call behind sync() holds the reference's samples of the damaged file."""
    import jpegsnoop_amd as J
    import torch
    base = harness.synth_jpeg(width=333, height=217, seed=61)
    harness.drive(oracle, base)
    clean, clean_planes = oracle.dib().copy(), [p.copy() for p in oracle.planes()]
    p = harness.parse_jpeg(base)
    at = p.scan_start + int((p.scan_end - p.scan_start) * 0.6)
    hurt, hurt_planes = None, None
    for bit in (0x10, 0x08, 0x20, 0x04, 0x40, 0x80, 0x01, 0x02):  # (most flips in noise re-synchronise silently: the first one the reference's own decode reports)
        d = bytearray(base); d[at] ^= bit
        if d[at] == 0xFF or d[at - 1] == 0xFF:
            continue
        harness.drive(oracle, bytes(d))
        if oracle.status()["scan_bad"] and not np.array_equal(oracle.dib(), clean):
            hurt, hurt_planes = bytes(d), [q.copy() for q in oracle.planes()]
            break
    assert hurt is not None
    b = J.JpegBatch(want_planes=True)
    try:
        for f in (base, hurt, base):
            b.add_jpeg(f)
        b.upload(); b.decode()
        fs = expand_factors(2, 2)
        before = torch.full((3, 217, 333), -7, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        assert raw_pack(J, b, make_spec(J, "full", "int16"), [1, 1, 1], [(before[c].data_ptr(), 0, c) for c in range(3)]) == 0, J.last_error()
        b.sync()
        assert b.info(1)["flags"] != 0 and b.info(1)["path"] == 1, "the flip must leave a flagged file on the parallel path"
        assert not bool((before == -7).all().item())                  # written by the call enqueued before sync(); what it holds is the parallel path's business
        ts = b.planes_to_torch()
        for c, (eh, ev) in enumerate(fs):
            assert np.array_equal(ts[1][c].cpu().numpy(), plane_model(hurt_planes[c], 333, 217, eh, ev)), c
            assert np.array_equal(ts[0][c].cpu().numpy(), plane_model(clean_planes[c], 333, 217, eh, ev)) and torch.equal(ts[0][c], ts[2][c]), c
        assert not torch.equal(ts[0][0], ts[1][0])
    finally:
        b.close()


def test_same_handle_decoded_and_packed_again(harness):
    """decode, pack, decode, pack on one handle; then the handle cleared and refilled with more images (the record block and the table grow) and packed
    twice in a row."""
    import jpegsnoop_amd as J
    import torch
    first = [harness.synth_jpeg(width=65, height=17, seed=80), harness.synth_jpeg(width=33, height=9, hs=1, vs=1, seed=81)]
    b = decoded_batch(J, first)
    try:
        models = models_of(b, [expand_factors(2, 2), expand_factors(1, 1)])
        for _ in range(2):
            ts = b.planes_to_torch(dtype=torch.uint8)
            for k in range(2):
                for c in range(3):
                    assert np.array_equal(ts[k][c].cpu().numpy(), models(k, c, "full", "uint8"))
            b.decode()
        b.clear()
        more = [harness.synth_jpeg(width=16 + 3 * k, height=8 + k, seed=90 + k) for k in range(40)]
        for f in more:
            b.add_jpeg(f)
        b.upload(); b.decode(); b.sync()
        models = models_of(b, [expand_factors(2, 2)] * 40)
        a = b.planes_to_torch(native=True)
        h = b.planes_to_torch(dtype=torch.uint8)
        for k in range(40):
            for c in range(3):
                assert np.array_equal(a[k][c].cpu().numpy(), models(k, c, "native", "int16")), (k, c)
                assert np.array_equal(h[k][c].cpu().numpy(), models(k, c, "full", "uint8")), (k, c)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ the Python surface
def test_planes_to_torch_forms(seam):
    J, torch, b, models, shapes = seam["J"], seam["torch"], seam["b"], seam["models"], seam["shapes"]
    dev = torch.device("cuda", b.device())
    i = next(k for k, s in enumerate(shapes) if s == (333, 17, 4))             # 4:4:0
    j = next(k for k, s in enumerate(shapes) if s == (17, 17, 2))              # 4:2:0
    g = next(k for k, s in enumerate(shapes) if s[2] == 3)                     # grayscale
    # list, comps=
    ts = b.planes_to_torch(images=[j, i], comps=[2, 0], dtype=torch.float32, scale=2.0, bias=(0.5, 0.25, 0.125))
    for r, k in zip(ts, (j, i)):
        assert len(r) == 2
        for t, c in zip(r, (2, 0)):
            assert t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == models.dims[k]
            assert np.array_equal(t.cpu().numpy(), models(k, c, "full", "float32", (2.0, 2.0, 2.0), (0.5, 0.25, 0.125)))
    assert len(b.planes_to_torch(images=[g])[0]) == 1
    # stack: FULL planes of one image stack; its NATIVE planes do not (4:4:0: luma 17 rows, chroma 9)
    st = b.planes_to_torch(images=[i, i], stack=True, dtype=torch.uint8)
    assert st.dtype == torch.uint8 and st.device == dev and tuple(st.shape) == (2, 3, 17, 333)
    for k in range(2):
        for c in range(3):
            assert np.array_equal(st[k, c].cpu().numpy(), models(i, c, "full", "uint8"))
    with pytest.raises(ValueError, match="component 1 of image %d is 9 x 333" % i):
        b.planes_to_torch(images=[i], native=True, stack=True)
    sn = b.planes_to_torch(images=[i, i], comps=[1, 2], native=True, stack=True)
    assert tuple(sn.shape) == (2, 2, 9, 333) and np.array_equal(sn[1, 0].cpu().numpy(), models(i, 1, "native", "int16"))
    with pytest.raises(ValueError, match="image %d " % j):
        b.planes_to_torch(images=[i, j], stack=True)
    # out=: a strided destination keeps what it held beside the rows; a stacked out
    big = torch.full((3, 17, 340), 7, dtype=torch.int16, device=dev)
    outs = [[big[c][:, :333] for c in range(3)]]
    assert b.planes_to_torch(images=[i], out=outs) is outs
    got = big.cpu().numpy(); want = np.full_like(got, 7)
    for c in range(3):
        want[c, :, :333] = models(i, c, "full", "int16")
    assert np.array_equal(got, want)
    so = torch.empty((1, 3, 17, 333), dtype=torch.uint8, device=dev)
    assert b.planes_to_torch(images=[i], stack=True, dtype=torch.uint8, out=so) is so and np.array_equal(so[0, 2].cpu().numpy(), models(i, 2, "full", "uint8"))
    # what out= refuses in Python, before the call
    ok = lambda **kw: [[torch.empty((17, 333), **{**dict(dtype=torch.int16, device=dev), **kw}) for _ in range(3)]]
    with pytest.raises(ValueError, match="cpu"):
        b.planes_to_torch(images=[i], out=ok(device="cpu"))
    with pytest.raises(ValueError, match="float32"):
        b.planes_to_torch(images=[i], out=ok(dtype=torch.float32))
    with pytest.raises(ValueError, match="shape"):
        b.planes_to_torch(images=[i], out=[[torch.empty((17, 332), dtype=torch.int16, device=dev)] * 3])
    with pytest.raises(ValueError, match="lists"):
        b.planes_to_torch(images=[i], out=[[torch.empty((17, 333), dtype=torch.int16, device=dev)] * 2])
    with pytest.raises(ValueError, match="contiguous"):
        b.planes_to_torch(images=[i], out=[[torch.empty((17, 666), dtype=torch.int16, device=dev)[:, ::2]] * 3])
    with pytest.raises(ValueError, match="shape"):
        b.planes_to_torch(images=[i], stack=True, out=torch.empty((1, 3, 17, 334), dtype=torch.int16, device=dev))
    with pytest.raises(ValueError):
        b.planes_to_torch(dtype=torch.float16)
    with pytest.raises(ValueError):
        b.planes_to_torch(scale=2.0)                              # (scale belongs to the float form)
    with pytest.raises(ValueError):
        b.planes_to_torch(dtype=torch.float32, scale=(1.0, 2.0))


def test_job_file_result_planes_to_torch_inside_the_callback(harness):
    """A JpegJob over a baseline, a progressive and a gray file on one device: every file's planes taken inside the callback equal the model on the planes
    the same callback reads from the same (batch, image)."""
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=65, height=33, seed=21), harness.synth_jpeg(width=45, height=19, hs=2, vs=1, progressive=1, seed=23),
             harness.synth_jpeg(width=17, height=9, gray=1, seed=22), b"not a jpeg"]
    factors = [expand_factors(2, 2), expand_factors(2, 1), expand_factors(1, 1, True)]
    job = J.JpegJob(devices=[0], want_planes=True)
    try:
        for f in files:
            job.add(f)
        seen = {}

        def on_file(r):
            if r.status != "ok":
                with pytest.raises(RuntimeError):
                    r.planes_to_torch()
                seen[r.index] = None
                return False
            ps = r.batch.planes(r.image)
            h, w = r.info["dim_y"], r.info["dim_x"]
            fs = factors[r.index]
            t = r.planes_to_torch(native=True, dtype=torch.uint8)
            f = r.planes_to_torch(dtype=torch.float32, scale=SCALE, bias=BIAS, stack=True)
            assert len(t) == len(fs) and tuple(f.shape) == (1, len(fs), h, w) and f.device == torch.device("cuda", r.device)
            seen[r.index] = (r.kind, all(np.array_equal(t[c].cpu().numpy(), plane_model(ps[c], w, h, eh, ev, "native", "uint8")) for c, (eh, ev) in enumerate(fs)),
                             all(np.array_equal(f[0, c].cpu().numpy(), plane_model(ps[c], w, h, eh, ev, "full", "float32", SCALE[c], BIAS[c])) for c, (eh, ev) in enumerate(fs)))
            return False
        stats = job.run(on_file)
        assert stats["ok"] == 3 and stats["refused"] == 1
        assert [seen[i] and seen[i][0] for i in range(4)] == ["baseline", "progressive", "baseline", None]
        assert all(seen[i][1] and seen[i][2] for i in range(3)), seen
    finally:
        job.close()


# ------------------------------------------------------------------------------------------------ the deal over many workgroups
def test_two_1080p_and_one_2160p_in_one_call(harness):
    """More units than one round of workgroups takes, images of two sizes in one list, all three components, NATIVE U8 and FULL I16: every tensor against
    the model, compared on the device."""
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=1920, height=1080, seed=5), harness.synth_jpeg(width=1920, height=1080, seed=6), harness.synth_jpeg(width=3840, height=2160, seed=7)]
    b = decoded_batch(J, files)
    try:
        planes = [b.planes(i) for i in range(3)]
        nat = b.planes_to_torch(native=True, dtype=torch.uint8)
        full = b.planes_to_torch()
        assert [tuple(t.shape) for r in nat for t in r] == [(1080, 1920), (540, 960), (540, 960)] * 2 + [(2160, 3840), (1080, 1920), (1080, 1920)]
        for i in range(3):
            inf = b.info(i)
            for c, (eh, ev) in enumerate(expand_factors(2, 2)):
                assert torch.equal(nat[i][c], torch.from_numpy(plane_model(planes[i][c], inf["dim_x"], inf["dim_y"], eh, ev, "native", "uint8")).cuda()), (i, c)
                assert torch.equal(full[i][c], torch.from_numpy(plane_model(planes[i][c], inf["dim_x"], inf["dim_y"], eh, ev, "full", "int16")).cuda()), (i, c)
    finally:
        b.close()
