"""-m gpu: jsnoop_batch_pack_coefs / k_pack_coefs (jsnoop_coef.hip), jsnoop_batch_image_dqt and JpegBatch.coefs_to_torch -- the coefficient arena
of a decoded batch as one tensor per component in caller-owned device memory.

Every comparison is exact against tests/coef_model.py fed with the ORACLE's numbers (tests/test_coef_model.py pins them on the CPU): the blocks
are oracle_coefs() of a Full-IDCT decode, the cumulative DC of a block is the top-left sample of its area in the int16 plane of the oracle's
decode_ac = 0 decode.  Raw calls write into an arena of 0xA5 bytes -- a guard band in front of, behind and between the destinations and in every
pitch gap -- and the whole arena is compared with what the model predicts: a stray write anywhere shows.  Images are tiny; the one larger batch
spreads the work over many workgroups, and the call behind it is sized so that a wave walks several units and destinations (tests/deal_cases.py).

The damaged files are tests/fuzz_util.py's flipped-bit variants (mode 0) of bases 0 and 1 with seeds 81 and 77: on the CPU the oracle's
decode_ac = 0 pass was checked to take the same path through them as its Full-IDCT pass (same status words, same slot 0 in every block)."""
import ctypes as C

import numpy as np
import pytest

import coef_model as M
import dc_scan_cases as DC
import deal_cases as D
import fuzz_util as F
import prog_cases as PC

pytestmark = pytest.mark.gpu

LAYOUTS = [dict(hs=1, vs=1), dict(hs=2, vs=1), dict(hs=2, vs=2), dict(hs=1, vs=2), dict(gray=1)]     # 4:4:4, 4:2:2, 4:2:0, 4:4:0, grey
WIDTHS = [1, 8, 9, 16, 17, 24, 72, 504, 512, 520, 1032]
HEIGHTS = [1, 8, 9, 17, 40]
FORMS = [(layout, dtype, zz) for layout in ("blocks", "freq") for dtype in ("int16", "float32") for zz in (False, True)]
GUARD = 64
DAMAGED = [(0, 81), (1, 77)]                                     # (base of fuzz_util.bases, seed)


def seam_shapes(tile):
    """(width, height, layout, restart interval): every width with two heights, two layouts and both restart settings (a sparse crossing), then the
    widths that put the luma grid (4:4:4, grey, 4:4:0) and the chroma grid (4:2:2, 4:2:0: one block per MCU of 16 pixels) at tile - 1, tile,
    tile + 1 and 2 * tile + 1 blocks."""
    out = []
    for k, w in enumerate(WIDTHS):
        out.append((w, HEIGHTS[k % 5], k % 5, 3 * (k % 2)))
        out.append((w, HEIGHTS[(3 * k + 2) % 5], (k + 2) % 5, 3 * ((k + 1) % 2)))
    for k, bw in enumerate((tile - 1, tile, tile + 1, 2 * tile + 1)):
        out.append((8 * bw, HEIGHTS[(k + 1) % 5], (0, 4, 3, 0)[k], 3 * (k % 2)))
        out.append((16 * bw, HEIGHTS[(k + 2) % 5], 1 + k % 2, 3 * ((k + 1) % 2)))
    return out


# ------------------------------------------------------------------------------------------------ the oracle's answer and the model over it
@pytest.fixture(scope="module")
def oracles(harness):
    full, dc = harness.oracle_backend(), harness.oracle_backend()
    full.set_options(decode_ac=1); dc.set_options(decode_ac=0)
    yield full, dc
    full.close(); dc.close()


class Truth:
    """One file: geometry, the oracle's blocks (Full IDCT; or given) and the cumulative DC of the oracle's DC-only planes; tensors computed once."""

    def __init__(self, harness, oracles, data, parsed=None, decode_ac=True):
        full, dc = oracles
        p = harness.drive(dc, data, parsed)
        self.geo = M.geometry_of(p)
        self.cum = M.cum_from_planes(dc.planes(), self.geo)
        if decode_ac:
            harness.drive(full, data, parsed); self.blocks = harness.oracle_coefs(full)
        else:
            self.blocks = harness.oracle_coefs(dc)
        assert self.blocks.shape == (self.geo.nblocks, 64)
        self.memo = {}

    def tensor(self, c, form):
        if (c, form) not in self.memo:
            layout, dtype, zz = form
            t = M.coef_tensor(self.blocks, self.cum, self.geo, c, layout, np.dtype(dtype), zz)
            t.setflags(write=False)
            self.memo[(c, form)] = t
        return self.memo[(c, form)]


# ------------------------------------------------------------------------------------------------ raw calls into a guarded arena
def make_spec(J, form):
    layout, dtype, zz = form
    s = J.capi.CoefSpec()
    J.load().jsnoop_coef_spec_defaults(C.byref(s))
    s.layout = J.capi.COEF_FREQ if layout == "freq" else J.capi.COEF_BLOCKS
    s.dtype = J.capi.COEF_F32 if dtype == "float32" else J.capi.COEF_I16
    s.order = J.capi.COEF_ZIGZAG if zz else J.capi.COEF_NATURAL
    return s


def raw_pack(J, b, spec, images, dsts):
    """jsnoop_batch_pack_coefs as a C caller makes it: dsts = [(ptr, row_pitch, plane_pitch, comp)] or CoefDst.  Returns the call's value; does not wait."""
    n = len(dsts)
    arr = (J.capi.CoefDst * max(n, 1))(*[d if isinstance(d, J.capi.CoefDst) else J.capi.CoefDst(d[0], d[1], d[2], d[3], 0) for d in dsts])
    ind = (C.c_int * max(n, 1))(*images) if images is not None else None
    return J.load().jsnoop_batch_pack_coefs(b._h, C.byref(spec) if spec is not None else None, ind, n, arr)


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
        if layout == "blocks":
            bh = model.shape[0]; row = raw.reshape(bh, -1)
            reg[:bh * rp].reshape(bh, rp)[:, :row.shape[1]] = row
        else:
            bh = model.shape[1]
            for f in range(64):
                row = raw.reshape(64, bh, -1)[f]
                reg[f * pp:f * pp + bh * rp].reshape(bh, rp)[:, :row.shape[1]] = row

    def check(self, what):
        got = self.buf.cpu().numpy()
        if not np.array_equal(got, self.expect):
            bad = int(np.flatnonzero(got != self.expect)[0])
            k = max([i for i, o in enumerate(self.offs) if o <= bad], default=-1)
            raise AssertionError("%s: first wrong byte at arena offset %d (destination %d + %d): got 0x%02x, want 0x%02x; %d bytes differ"
                                 % (what, bad, k, bad - self.offs[k] if k >= 0 else bad, got[bad], self.expect[bad], int((got != self.expect).sum())))

    def untouched(self):
        return bool((self.buf == 0xA5).all().item())


def geometry_of_dst(truth, c, form, row_extra=0, plane_extra=0):
    """(row_pitch, plane_pitch, bytes of the region) of component c in this form."""
    layout, dtype, _ = form; elem = 4 if dtype == "float32" else 2
    bw, bh = truth.geo.grid(c)
    rp = bw * elem * (64 if layout == "blocks" else 1) + row_extra
    pp = bh * rp + plane_extra
    return rp, pp, bh * rp if layout == "blocks" else 64 * pp


def pack_and_check(J, torch, b, truths, dests, form, lead=0, row_extra=0, plane_extra=0, what="", before_sync=False):
    """One raw call for dests = [(image, component)], then the whole arena against the model.  Dense destinations pass pitch 0 for every second one."""
    geo = [geometry_of_dst(truths[i], c, form, row_extra, plane_extra) for i, c in dests]
    ar = Arena(torch, [g[2] for g in geo], lead)
    for k, (i, c) in enumerate(dests):
        ar.place(k, truths[i].tensor(c, form), form[0], geo[k][0], geo[k][1])
    dense = row_extra == 0 and plane_extra == 0
    dsts = [(ar.ptr(k), 0 if dense and k % 2 else geo[k][0], 0 if dense and k % 2 else (geo[k][1] if form[0] == "freq" else 0), c) for k, (i, c) in enumerate(dests)]
    torch.cuda.synchronize()                                      # (the fill above ran on torch's stream, the pack runs on the batch's)
    rc = raw_pack(J, b, make_spec(J, form), [i for i, _ in dests], dsts)
    assert rc == 0, J.last_error()
    if before_sync:
        b.sync()
    torch.cuda.synchronize()
    ar.check("%s %s lead=%d row+%d plane+%d" % (what, form, lead, row_extra, plane_extra))


def decoded_batch(J, files, **kw):
    b = J.JpegBatch(**kw)
    for f in files:
        b.add_jpeg(f)
    b.upload(); b.decode(); b.sync()
    return b


def all_components(truths, images=None):
    return [(i, c) for i in (range(len(truths)) if images is None else images) for c in range(truths[i].geo.ncomp)]


# ------------------------------------------------------------------------------------------------ the seam batch
@pytest.fixture(scope="module")
def seam(harness, oracles):
    import jpegsnoop_amd as J
    import torch
    T = J.capi.COEF_TILE
    shapes = seam_shapes(T)
    files = [harness.synth_jpeg(width=w, height=h, quality=90, restart_interval=dri, seed=900 + k, **LAYOUTS[s]) for k, (w, h, s, dri) in enumerate(shapes)]
    truths = [Truth(harness, oracles, f) for f in files]
    b = decoded_batch(J, files)
    luma = {t.geo.grid(0)[0] for t in truths}; chroma = {t.geo.grid(1)[0] for t in truths if t.geo.ncomp == 3 and t.geo.hv[0][0] == 2}
    assert {T - 1, T, T + 1, 2 * T + 1} <= luma and {T - 1, T, T + 1, 2 * T + 1} <= chroma, (sorted(luma), sorted(chroma))
    for i, t in enumerate(truths):
        for c in range(t.geo.ncomp):
            assert b.coef_grid(i, c) == t.geo.grid(c), (i, c)
    yield J, torch, b, truths, shapes, files
    b.close()


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "%s-%s-%s" % (f[0], f[1], "zigzag" if f[2] else "natural"))
def test_every_form_over_the_tile_seams_every_component_dense_and_pitched(seam, form):
    """All components of all seam images in ONE call, dense; then once more with padded rows and planes from destinations that are no multiple of 16."""
    J, torch, b, truths, _, _files = seam
    elem = 4 if form[1] == "float32" else 2
    dests = all_components(truths)
    pack_and_check(J, torch, b, truths, dests, form, what="dense")
    pack_and_check(J, torch, b, truths, dests, form, lead=elem * 3, row_extra=elem * 5, plane_extra=elem * 7, what="pitched")


@pytest.mark.parametrize("form", [f for f in FORMS if f[1] == "int16" and (f[0] == "freq" or f[2] or f == ("blocks", "int16", False))] + [("blocks", "float32", False), ("freq", "float32", True)],
                         ids=lambda f: "%s-%s-%s" % (f[0], f[1], "zigzag" if f[2] else "natural"))
def test_destinations_at_every_legal_misalignment(seam, form):
    """Every offset from a 16-byte line the element size allows (2-byte steps for int16, 4-byte steps for float32), on the images around the tile seams."""
    J, torch, b, truths, shapes, files = seam
    T = J.capi.COEF_TILE; elem = 4 if form[1] == "float32" else 2
    pick = [i for i, t in enumerate(truths) if t.geo.grid(0)[0] in (1, 3, T + 1, 2 * T + 1) or (t.geo.ncomp == 3 and t.geo.grid(1)[0] == T + 1)][:6]
    assert len(pick) >= 4
    for lead in range(elem, 16, elem):
        pack_and_check(J, torch, b, truths, all_components(truths, pick), form, lead=lead, row_extra=elem * (lead % 3), what="misaligned")


def test_one_call_many_destinations_one_image_twice_in_any_order(seam):
    """40 images with every component of each, in descending order, one image listed a second time at the end: one call."""
    J, torch, b, truths, _, _files = seam
    assert len(truths) >= 30
    order = list(range(len(truths)))[::-1] + list(range(10))        # 40 entries over the batch, ten images twice
    order = order[:40]
    dests = all_components(truths, order)
    assert len(order) == 40 and len(set(order)) < 40
    pack_and_check(J, torch, b, truths, dests, ("freq", "int16", False), what="mixed list")
    pack_and_check(J, torch, b, truths, dests, ("blocks", "float32", True), what="mixed list")


def test_dqt_is_the_table_each_component_selects_and_levels_times_dqt_wrap_to_the_arena(seam, harness):
    J, torch, b, truths, shapes, files = seam
    for i in (0, 3, 7, len(truths) - 1):
        p = harness.parse_jpeg(files[i])
        for c in range(truths[i].geo.ncomp):
            q = b.dqt(i, c)
            assert q.dtype == np.uint16 and q.tolist() == list(p.dqt[p.comps[c][3]]), (i, c)
            idx = truths[i].geo.arena_index(c); blk = truths[i].blocks[idx].astype(np.int64)
            assert not (blk[..., 1:] % q[1:].astype(np.int64)).any(), "every AC value is a multiple of its multiplier (nothing wraps at quality 90)"
            levels = blk // np.maximum(q.astype(np.int64), 1)
            assert np.array_equal((levels[..., 1:] * q[1:]).astype(np.int16), truths[i].blocks[idx][..., 1:])
    lib = J.load(); out = (C.c_uint16 * 64)()
    assert lib.jsnoop_batch_image_dqt(b._h, len(truths), 0, out) == -1 and "out of range" in J.last_error()
    assert lib.jsnoop_batch_image_dqt(b._h, 0, 3, out) == -1 and "component" in J.last_error()
    grey = [i for i, t in enumerate(truths) if t.geo.ncomp == 1][0]
    assert lib.jsnoop_batch_image_dqt(b._h, grey, 1, out) == -1 and lib.jsnoop_batch_image_dqt(b._h, 0, 0, None) == -1


def test_refusals_launch_nothing_write_nothing_and_name_their_reason(seam, harness):
    J, torch, b, truths, _, _files = seam
    lib = J.load(); cap = J.capi
    i = [k for k, t in enumerate(truths) if t.geo.ncomp == 3 and t.geo.grid(0)[0] >= 3][0]
    bw, bh = truths[i].geo.grid(0)
    ar = Arena(torch, [bw * bh * 64 * 4 + 64])
    p = ar.ptr(0)
    torch.cuda.synchronize()
    bi, bf, fi, ff = ("blocks", "int16", False), ("blocks", "float32", False), ("freq", "int16", False), ("freq", "float32", False)

    def refused(form, images, dsts, word, spec=None):
        rc = raw_pack(J, b, make_spec(J, form) if spec is None else spec, images, dsts)
        assert rc == -1 and word in J.last_error(), (rc, word, J.last_error())

    refused(bi, [len(truths)], [(p, 0, 0, 0)], "out of range")
    refused(bi, [-1], [(p, 0, 0, 0)], "out of range")
    refused(bi, [i], [(p, 0, 0, 3)], "component")
    grey = [k for k, t in enumerate(truths) if t.geo.ncomp == 1][0]
    refused(bi, [grey], [(p, 0, 0, 1)], "component")
    refused(bi, [i], [(0, 0, 0, 0)], "NULL")
    refused(bi, [i], [cap.CoefDst(p, 0, 0, 0, 1)], "reserved")
    refused(bi, [i], [(p, bw * 128 - 2, 0, 0)], "row_pitch")
    refused(fi, [i], [(p, bw * 2 - 2, 0, 0)], "row_pitch")
    refused(fi, [i], [(p, bw * 2, bw * 2 * bh - 2, 0)], "plane_pitch")
    refused(bi, [i], [(p + 1, 0, 0, 0)], "multiples of 2")
    refused(bi, [i], [(p, bw * 128 + 1, 0, 0)], "multiples of 2")
    refused(fi, [i], [(p, bw * 2, bw * 2 * bh + 1, 0)], "multiples of 2")
    refused(bf, [i], [(p + 2, 0, 0, 0)], "multiples of 4")
    refused(ff, [i], [(p, bw * 4 + 2, 0, 0)], "multiples of 4")
    refused(ff, [i], [(p, bw * 4, bw * 4 * bh + 2, 0)], "multiples of 4")
    refused(bi, [i, len(truths)], [(p, 0, 0, 0), (p, 0, 0, 0)], "out of range")       # the second entry bad: nothing of the first is written
    for field, val, word in (("layout", 2, "layout"), ("dtype", -1, "dtype"), ("order", 2, "order"), ("struct_size", 20, "struct_size"), ("struct_size", 0, "struct_size")):
        s = make_spec(J, bi); setattr(s, field, val)
        refused(bi, [i], [(p, 0, 0, 0)], word, spec=s)
    assert lib.jsnoop_batch_pack_coefs(b._h, None, None, 1, (cap.CoefDst * 1)(cap.CoefDst(p, 0, 0, 0, 0))) == -1 and "spec is NULL" in J.last_error()
    assert lib.jsnoop_batch_pack_coefs(b._h, C.byref(make_spec(J, bi)), None, 1, None) == -1 and "dst is NULL" in J.last_error()
    assert lib.jsnoop_batch_pack_coefs(b._h, C.byref(make_spec(J, bi)), None, -1, None) == -1
    assert lib.jsnoop_batch_pack_coefs(None, C.byref(make_spec(J, bi)), None, 1, None) == -1 and "batch is NULL" in J.last_error()
    assert lib.jsnoop_batch_pack_coefs(b._h, C.byref(make_spec(J, bi)), None, 0, None) == 0                                     # n == 0
    fresh = J.JpegBatch()
    try:
        fresh.add_jpeg(harness.synth_jpeg(width=16, height=16, seed=5))
        assert raw_pack(J, fresh, make_spec(J, bi), [0], [(p, 0, 0, 0)]) == -1 and "not been decoded" in J.last_error()
        fresh.upload()
        assert raw_pack(J, fresh, make_spec(J, bi), [0], [(p, 0, 0, 0)]) == -1 and "not been decoded" in J.last_error()
    finally:
        fresh.close()
    b.sync(); torch.cuda.synchronize()
    assert ar.untouched(), "a refused call wrote to the destination"
    # shorter struct_size: the lacking fields at their defaults (order stays NATURAL although the caller's bytes say ZIGZAG)
    s = make_spec(J, ("blocks", "int16", True)); s.struct_size = 12
    ar2 = Arena(torch, [bw * bh * 128])
    ar2.place(0, truths[i].tensor(0, bi), "blocks", bw * 128, 0)
    torch.cuda.synchronize()
    assert raw_pack(J, b, s, [i], [(ar2.ptr(0), 0, 0, 0)]) == 0, J.last_error()
    b.sync(); torch.cuda.synchronize()
    ar2.check("struct_size 12")
    sz = lib.jsnoop_batch_coef_bytes
    assert sz(b._h, C.byref(make_spec(J, bi)), i, 0) == bw * bh * 128 and sz(b._h, C.byref(make_spec(J, ff)), i, 0) == bw * bh * 256
    assert sz(b._h, C.byref(make_spec(J, bi)), i, 3) == 0 and sz(b._h, C.byref(make_spec(J, bi)), len(truths), 0) == 0


# ------------------------------------------------------------------------------------------------ the deal, two streams, DC-only
def test_64_images_of_333x217_dealt_over_many_workgroups(harness, oracles):
    """About 4500 units over more than a thousand workgroups.  On a device of 256 compute units that is still below CF_WAVES * 5 * 256 units: a
    workgroup's share is four units and a wave takes ONE -- the shares fall on every phase of the destinations, but no wave walks from one unit to the
    next.  That is test_calls_of_so_many_units_that_a_wave_walks_several_units_and_records below."""
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=333, height=217, quality=80, restart_interval=(0, 3)[k % 2], seed=1200 + k, **LAYOUTS[(2, 1, 0, 3)[k % 4]]) for k in range(4)]
    truths = [Truth(harness, oracles, f) for f in files]
    b = J.JpegBatch()
    try:
        for f in files:
            b.add_jpeg(f)
        b.tile(64); b.upload(); b.decode(); b.sync()
        tr = [truths[i % 4] for i in range(64)]
        dests = all_components(tr)
        for form in (("blocks", "int16", False), ("freq", "int16", False), ("freq", "float32", True), ("blocks", "int16", True)):
            pack_and_check(J, torch, b, tr, dests, form, what="64 images")
    finally:
        b.close()


def test_calls_of_so_many_units_that_a_wave_walks_several_units_and_records(harness, oracles, capsys):
    """Sized from the device (tests/deal_cases.py, proven on the CPU by tests/test_deal_cases.py): a share of twelve units, so every wave takes three units
    one after the other -- in the forms that go through LDS, through the same tile --, passes over three one-row destinations in one step, leaves a long
    destination in the middle of a share and takes a one-block run directly behind a full tile.  The direct form (blocks, natural, int16: eight
    workgroups a compute unit) and a tiled one (freq, zig-zag, float32: five) get a list of their own.  A dozen distinct components of a few files, listed
    many times, each entry with a destination of its own; the whole arena of every call against the model."""
    import jpegsnoop_amd as J
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lists = {"direct": D.coefs_records(cus, "direct"), "tiled": D.coefs_records(cus, "tiled")}
    for form, recs in lists.items():
        c = D.census_of("coefs", form, recs, cus)
        with capsys.disabled():
            print("\nk_pack_coefs %s, %d compute units: %s" % (form, cus, D.summary(c)))
        assert D.missing(c, D.KERNELS["coefs"]["waves"], **D.conditions("coefs", form)) == [], D.summary(c)
    images = sorted({r.pic[:3] for recs in lists.values() for r in recs})
    files = [harness.synth_jpeg(width=w, height=h, quality=(80, 92)[k % 2], restart_interval=(0, 3)[k % 2], seed=1500 + k, **LAYOUTS[l]) for k, (l, w, h) in enumerate(images)]
    truths = [Truth(harness, oracles, f) for f in files]
    T = J.capi.COEF_TILE
    b = decoded_batch(J, files)
    try:
        for form, recs in lists.items():
            dests = [(images.index(r.pic[:3]), r.pic[3]) for r in recs]
            for r, (i, comp) in zip(recs, dests):                     # the units the census counted are the units of the call
                bw, bh = truths[i].geo.grid(comp)
                assert b.coef_grid(i, comp) == (bw, bh) and r.sizes == ([T] * (-(-bw // T) - 1) + [bw - T * (-(-bw // T) - 1)]) * bh, r.pic
            pack_and_check(J, torch, b, truths, dests, ("blocks", "int16", False) if form == "direct" else ("freq", "float32", True), what="deal " + form)
    finally:
        b.close()


def test_pack_waits_for_both_halves_of_a_two_stream_decode(harness, oracles):
    """Full-IDCT batch on two streams: the call is enqueued right behind decode(), before anything has waited."""
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=333, height=217, seed=40 + k) for k in range(5)]
    truths = [Truth(harness, oracles, f) for f in files]
    b = J.JpegBatch()
    try:
        for f in files:
            b.add_jpeg(f)
        b.set_split(2); b.upload()
        assert b.split_parts() == 2
        b.decode()
        pack_and_check(J, torch, b, truths, all_components(truths), ("freq", "int16", False), what="two-stream decode", before_sync=True)
        assert b.last_form() == 1
    finally:
        b.close()


def test_dc_only_fast_form_is_decoded_once_more_and_says_so(harness, oracles):
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=100, height=75, hs=2, vs=2, restart_interval=3 * (k % 2), seed=500 + k) for k in range(3)]
    truths = [Truth(harness, oracles, f, decode_ac=False) for f in files]
    for t in truths:
        assert not t.blocks[:, 1:].any()
    b = decoded_batch(J, files, decode_ac=False)
    try:
        assert b.last_form() == 2
        pack_and_check(J, torch, b, truths, all_components(truths), ("blocks", "int16", False), what="DC-only", before_sync=True)
        assert b.last_form() == 1, "behind a fast-form decode the call decodes again in the generic form"
        pack_and_check(J, torch, b, truths, all_components(truths), ("freq", "float32", True), what="DC-only, second call")
        assert b.last_form() == 1
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ unusual layouts, wrapping predictors, markers inside MCUs
def small_dc_cases():
    """The catalogue's files with at most 5000 MCUs (the name carries the count): the built catalogue where a test before this one built it, else these alone."""
    if DC._BUILT is not None:
        return [c for c in DC._BUILT if c.nmcu <= 5000]
    if "small" not in _DC_MEMO:
        _DC_MEMO["small"] = [fn() for fn in DC.CASES if int(fn.__name__.split("_")[2]) <= 5000]
    assert all(c.nmcu <= 5000 for c in _DC_MEMO["small"]) and len(_DC_MEMO["small"]) == 39
    return _DC_MEMO["small"]


_DC_MEMO = {}


def test_layouts_up_to_48_blocks_per_mcu_and_predictors_that_wrap(harness, oracles):
    """The all-DC files of tests/dc_scan_cases.py with at most 5000 MCUs: slot 0 is the oracle's cumulative DC, slots 1..63 are zero."""
    import jpegsnoop_amd as J
    import torch
    cases = small_dc_cases()
    assert {c.layout for c in cases} >= {"gray", "444", "422", "420", "luma4x2", "all4x4"} and any(c.group == "E" for c in cases)
    truths = [Truth(harness, oracles, c.file) for c in cases]
    for c, t in zip(cases, truths):
        assert t.geo.bpm == DC.BLOCKS[c.layout] and not t.blocks[:, 1:].any()
    b = decoded_batch(J, [c.file for c in cases])
    try:
        dests = all_components(truths)
        pack_and_check(J, torch, b, truths, dests, ("blocks", "int16", False), what="dc_scan_cases")
        pack_and_check(J, torch, b, truths, dests, ("freq", "int16", True), what="dc_scan_cases")
        ts = b.coefs_to_torch(layout="freq")
        for i, t in enumerate(truths):
            for c in range(t.geo.ncomp):
                assert not ts[i][c][1:].any().item(), (cases[i].name, c)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ progressive
PROG = ["dc_al3_three_refinements_between_ac", "successive_approximation_three_and_two_levels", "first_split_refined_whole",
        "dri_interval_of_one_eobrun_and_dc_refinement_byte", "refinement_stretches_and_zrl", "values_every_category_al0"]


def test_progressive_files_give_the_tensors_of_their_baseline_encoding(harness, oracles):
    """Six catalogue files (DC and AC refinement, restart intervals among them): the progressive batch gives what the baseline batch of the same coefficients
    gives, and that is the model over the oracle's decode of the baseline file.  The multipliers are the frame's tables."""
    import jpegsnoop_amd as J
    import torch
    assert set(PROG) <= set(PC.NAMES)
    cases = [PC.built(n) for n in PROG]
    scans = [s for c in cases for s in c.dec.scans]
    assert any(s["ss"] == 0 and s["ah"] > 0 for s in scans) and any(s["ss"] > 0 and s["ah"] > 0 for s in scans) and any(s["dri"] > 0 for s in scans), "both refinement kinds and restart intervals"
    truths = [Truth(harness, oracles, c.base) for c in cases]
    bp, bb = decoded_batch(J, [c.file for c in cases]), decoded_batch(J, [c.base for c in cases])
    try:
        for i in range(len(cases)):
            assert bp.info(i)["path"] == 3 and bb.info(i)["path"] != 3
        for form in (("blocks", "int16", False), ("freq", "float32", False), ("freq", "int16", True)):
            pack_and_check(J, torch, bb, truths, all_components(truths), form, what="baseline of progressive")
            pack_and_check(J, torch, bp, truths, all_components(truths), form, what="progressive")
        for i, c in enumerate(cases):
            for k in range(c.frame.ncomp):
                want = c.frame.qtabs[c.frame.comps[k][2]]                       # zig-zag order, as the DQT segment carries it
                nat = [0] * 64
                for z, n in enumerate(M.ZIGZAG):
                    nat[n] = want[z]
                assert bp.dqt(i, k).tolist() == nat == bb.dqt(i, k).tolist(), (c.name, k)
    finally:
        bp.close(); bb.close()


# ------------------------------------------------------------------------------------------------ damaged files
def test_damaged_files_behind_sync_hold_the_repaired_arena_and_the_oracles_dc(harness, oracles):
    import jpegsnoop_amd as J
    import torch
    bases = F.bases(harness)
    hurt = []
    for base, seed in DAMAGED:
        data, q, mode = F.mutate(harness, np.random.default_rng(seed), bases[base])
        assert mode == 0 and data != bases[base]
        hurt.append(data)
    full, dc = oracles
    truths = [Truth(harness, oracles, f) for f in hurt]
    for f in hurt:                                                # what the CPU search established for these seeds
        harness.drive(full, f); sf, cf = full.status(), harness.oracle_coefs(full)
        harness.drive(dc, f); sd, cd = dc.status(), harness.oracle_coefs(dc)
        assert sf == sd and sf["scan_bad"] and np.array_equal(cf[:, 0], cd[:, 0])
    b = decoded_batch(J, [bases[0], hurt[0], hurt[1], bases[1]])
    try:
        print("damaged images: flags 0x%04x path %d, flags 0x%04x path %d" % (b.info(1)["flags"], b.info(1)["path"], b.info(2)["flags"], b.info(2)["path"]))
        assert b.info(1)["flags"] != 0 and b.info(2)["flags"] != 0
        ts = b.coefs_to_torch(images=[1, 2])
        for k, i in enumerate((1, 2)):
            arena = b.coefs(i); t = truths[k]
            for c in range(t.geo.ncomp):
                idx = t.geo.arena_index(c); got = ts[k][c].cpu().numpy()
                assert np.array_equal(got[..., 1:], arena[idx][..., 1:]), "slots 1..63 are read_coefs' (image %d component %d)" % (i, c)
                assert np.array_equal(got[..., 0], t.cum[idx]), "slot 0 is the oracle's cumulative DC of the damaged bytes (image %d component %d)" % (i, c)
                assert np.array_equal(got, t.tensor(c, ("blocks", "int16", False)))
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ torch and the job
def test_coefs_to_torch_shapes_dtypes_out_and_component_subsets(seam):
    J, torch, b, truths, _, _files = seam
    pick = [2, 11, len(truths) - 1, 4]
    ts = b.coefs_to_torch(images=pick)
    assert len(ts) == 4
    for k, i in enumerate(pick):
        t = truths[i]
        assert len(ts[k]) == t.geo.ncomp
        for c in range(t.geo.ncomp):
            bw, bh = t.geo.grid(c)
            assert ts[k][c].dtype == torch.int16 and tuple(ts[k][c].shape) == (bh, bw, 64) and ts[k][c].is_cuda
            assert np.array_equal(ts[k][c].cpu().numpy(), t.tensor(c, ("blocks", "int16", False)))
    colour = [i for i, t in enumerate(truths) if t.geo.ncomp == 3][:5]
    fs = b.coefs_to_torch(images=colour, comps=[2, 0], layout="freq", dtype=torch.float32, zigzag=True)
    for k, i in enumerate(colour):
        assert len(fs[k]) == 2
        for j, c in enumerate((2, 0)):
            bw, bh = truths[i].geo.grid(c)
            assert fs[k][j].dtype == torch.float32 and tuple(fs[k][j].shape) == (64, bh, bw)
            assert np.array_equal(fs[k][j].cpu().numpy(), truths[i].tensor(c, ("freq", "float32", True)))
    # out=: strided outer dimensions, returned as it is, nothing outside the views touched
    i = [k for k, t in enumerate(truths) if t.geo.ncomp == 3 and t.geo.grid(0) != t.geo.grid(1) and min(t.geo.grid(1)) > 1][0]
    bw, bh = truths[i].geo.grid(0); cw, ch = truths[i].geo.grid(1)
    big = torch.full((64, bh + 1, bw + 3), -7, dtype=torch.int16, device="cuda"); small = torch.full((64, ch, cw), -7, dtype=torch.int16, device="cuda")
    out = [[big[:, :bh, :bw], small]]
    r = b.coefs_to_torch(images=[i], comps=[0, 1], layout="freq", out=out)
    assert r is out
    assert np.array_equal(big[:, :bh, :bw].cpu().numpy(), truths[i].tensor(0, ("freq", "int16", False))) and np.array_equal(small.cpu().numpy(), truths[i].tensor(1, ("freq", "int16", False)))
    assert bool((big[:, bh:, :] == -7).all().item()) and bool((big[:, :, bw:] == -7).all().item())
    for bad, word in (([[small, small]], "shape"), ([[big[:, :bh, :bw].float(), small]], "asked for"), ([[big[:, :bh, :bw].cpu(), small]], "is on"), ([[big[:, :bh, :bw]]], "must hold"),
                      ([[big[:, :bh, :bw], small.transpose(1, 2).contiguous().transpose(1, 2)]], "contiguous")):
        with pytest.raises(ValueError, match=word):
            b.coefs_to_torch(images=[i], comps=[0, 1], layout="freq", out=bad)
    with pytest.raises(IndexError):
        b.coefs_to_torch(images=[len(truths)])
    with pytest.raises(IndexError):
        b.coefs_to_torch(images=[i], comps=[3])
    with pytest.raises(ValueError):
        b.coefs_to_torch(layout="planes")
    with pytest.raises(ValueError):
        b.coefs_to_torch(dtype=torch.int32)
    assert b.coefs_to_torch(images=[]) == []


def test_job_file_result_coefs_to_torch_inside_the_callback(harness, oracles):
    """A JpegJob over baseline and progressive files on one device: every file's tensors taken inside the callback equal the model over the oracle."""
    import jpegsnoop_amd as J
    import torch
    c = PC.built(PROG[2])
    files = [harness.synth_jpeg(width=65, height=33, seed=70), c.file, harness.synth_jpeg(width=40, height=24, gray=1, seed=71), b"not a jpeg"]
    truths = [Truth(harness, oracles, files[0]), Truth(harness, oracles, c.base), Truth(harness, oracles, files[2]), None]
    job = J.JpegJob(devices=[0])
    seen = {}
    try:
        for f in files:
            job.add(f)

        def on_file(r):
            if r.status == "ok":
                seen[r.index] = [t.cpu().numpy() for t in r.coefs_to_torch(layout="freq", zigzag=True)]
            else:
                with pytest.raises(RuntimeError):
                    r.coefs_to_torch()
            return False

        job.run(on_file)
    finally:
        job.close()
    assert sorted(seen) == [0, 1, 2]
    for i in (0, 1, 2):
        assert len(seen[i]) == truths[i].geo.ncomp
        for k, got in enumerate(seen[i]):
            assert np.array_equal(got, truths[i].tensor(k, ("freq", "int16", True))), (i, k)
