"""-m gpu: jsnoop_batch_pack_coef_hist / jsnoop_batch_read_coef_hist / k_coef_hist (jsnoop_coef_hist.hip) and JpegBatch.coef_hist_to_torch -- the histogram
of every DCT frequency of any list of (image, component) pairs of a decoded batch, one row per pair in caller-owned device memory.

Every comparison is exact, word for word, against tests/coef_hist_model.py fed with the ORACLE's numbers the way tests/test_gpu_coefs.py builds its Truth
(coef_hist_cases.OracleView; tests/test_coef_hist_cases.py pins the catalogue's claims on the CPU).  Raw calls write into a device arena of 0xA5 bytes with
a guard band in front of, behind and between the rows and in every pitch gap; the whole arena is compared, so a stray write anywhere shows, and a failure
names pair, position, bin, got and want.  Every raw call is made twice into the same memory: the rows are initialised inside the call.  Images are tiny."""
import ctypes as C

import numpy as np
import pytest

import coef_hist_cases as HC
import coef_hist_model as HM
import coef_model as M
import deal_cases as D
import fuzz_util as F

pytestmark = pytest.mark.gpu

RANGES = HC.RANGES
LAYOUTS = [dict(hs=1, vs=1), dict(hs=2, vs=1), dict(hs=2, vs=2), dict(hs=1, vs=2), dict(gray=1), dict(hs=4, vs=1)]     # 4:4:4, 4:2:2, 4:2:0, 4:4:0, grey, 4:1:1
GUARD = 24                                                       # words
DAMAGED = [(0, 81), (1, 77)]                                     # tests/test_gpu_coefs.py's two damaged files: (base of fuzz_util.bases, seed)
FORMS = [(R, quantised, zz) for R in RANGES for quantised in (True, False) for zz in (False, True)]


def form_id(f):
    return "r%d-%s-%s" % (f[0], "levels" if f[1] else "values", "zigzag" if f[2] else "natural")


@pytest.fixture(scope="module")
def oracles(harness):
    full, dc = harness.oracle_backend(), harness.oracle_backend()
    full.set_options(decode_ac=1); dc.set_options(decode_ac=0)
    yield full, dc
    full.close(); dc.close()


# ------------------------------------------------------------------------------------------------ raw calls into a guarded arena
def make_spec(J, form):
    R, quantised, zz = form
    s = J.capi.CoefHistSpec()
    J.load().jsnoop_coef_hist_spec_defaults(C.byref(s))
    s.order = J.capi.COEF_ZIGZAG if zz else J.capi.COEF_NATURAL
    s.quantised, s.range = int(quantised), R
    return s


def raw_pack(J, b, spec, pairs, ptr, pitch):
    n = len(pairs)
    im = (C.c_int * max(n, 1))(*[i for i, _ in pairs]); cs = (C.c_int * max(n, 1))(*[c for _, c in pairs])
    return J.load().jsnoop_batch_pack_coef_hist(b._h, C.byref(spec) if spec is not None else None, im, cs, n, ptr, pitch)


class Arena:
    """GUARD words of 0xA5A5A5A5, then n rows `pitch` words apart, then GUARD words; `expect` is what the model says the whole of it must hold."""

    def __init__(self, torch, n, words, pitch):
        self.n, self.words, self.pitch = n, words, pitch
        total = GUARD + (n - 1) * pitch + words + GUARD if n else 2 * GUARD
        self.buf = torch.full((total,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda")
        self.expect = np.full(total, 0xA5A5A5A5, np.uint32)

    def ptr(self):
        return self.buf.data_ptr() + GUARD * 4

    def place(self, k, row):
        self.expect[GUARD + k * self.pitch:GUARD + k * self.pitch + self.words] = row

    def check(self, what, pairs, R):
        got = self.buf.cpu().numpy().view(np.uint32)
        if np.array_equal(got, self.expect):
            return
        bad = int(np.flatnonzero(got != self.expect)[0]); nb = 2 * R + 1
        k, w = divmod(bad - GUARD, self.pitch) if bad >= GUARD else (-1, bad)
        if 0 <= k < self.n and w < self.words:
            where = ("position %d bin %d (x = %d)" % (w // nb, w % nb, w % nb - R)) if w < 64 * nb else ("%s of position %d" % (("min", "max")[(w - 64 * nb) // 64], (w - 64 * nb) % 64))
            where = "pair %s (row %d), %s" % (pairs[k], k, where)
        else:
            where = "OUTSIDE the rows: arena word %d (behind row %d + %d words)" % (bad, k, w)
        signed = 0 <= k < self.n and 64 * nb <= w < self.words                   # minima and maxima are int32
        show = (lambda v: int(np.int32(v))) if signed else int
        raise AssertionError("%s: %s: got %d (0x%08x), want %d (0x%08x); %d words differ" % (what, where, show(got[bad]), got[bad], show(self.expect[bad]), self.expect[bad],
                                                                                        int((got != self.expect).sum())))

    def untouched(self):
        return bool((self.buf == 0xA5A5A5A5 - (1 << 32)).all().item())


def pack_and_check(J, torch, b, views, pairs, form, extra=0, what="", before_sync=False, calls=2):
    """Raw calls for pairs = [(image, component)] (two into the same memory), then the whole arena against the model."""
    R, quantised, zz = form
    words = HM.words(R); pitch = words + extra
    ar = Arena(torch, len(pairs), words, pitch)
    for k, (i, c) in enumerate(pairs):
        ar.place(k, views[i].row(c, R, quantised, zz))
    torch.cuda.synchronize()                                      # (the fill above ran on torch's stream, the pack runs on the batch's)
    for _ in range(calls):
        rc = raw_pack(J, b, make_spec(J, form), pairs, ar.ptr(), pitch if extra else 0)
        assert rc == 0, J.last_error()
    if before_sync:
        b.sync()
    torch.cuda.synchronize()
    ar.check("%s %s pitch+%d" % (what, form_id(form), extra), pairs, R)
    return ar


def decoded_batch(J, files, **kw):
    b = J.JpegBatch(**kw)
    for f in files:
        b.add_jpeg(f)
    b.upload(); b.decode(); b.sync()
    return b


def all_pairs(views, images=None):
    return [(i, c) for i in (range(len(views)) if images is None else images) for c in range(views[i].geo.ncomp)]


# ------------------------------------------------------------------------------------------------ the catalogue
@pytest.fixture(scope="module")
def catalogue(harness, oracles):
    """[(batch, views, cases)]: the baseline files of the catalogue in one batch, the progressive ones in another (a batch holds one kind)."""
    import jpegsnoop_amd as J
    import torch
    groups = []
    for prog in (False, True):
        cases = [c for c in HC.built() if c.decode_ac and (c.truth_data is not c.data) == prog]
        views = [HC.OracleView(harness, oracles, c.truth_data) for c in cases]
        groups.append((decoded_batch(J, [c.data for c in cases]), views, cases))
    assert len(groups[0][2]) >= 12 and len(groups[1][2]) == 2
    yield J, torch, groups
    for b, _, _ in groups:
        b.close()


def test_grids_and_tables_of_the_catalogue_are_the_files(catalogue):
    J, torch, groups = catalogue
    for b, views, cases in groups:
        for i, v in enumerate(views):
            assert b.info(i)["path"] == (3 if cases[i].truth_data is not cases[i].data else b.info(i)["path"])
            for c in range(v.geo.ncomp):
                assert b.coef_grid(i, c) == v.geo.grid(c) and b.dqt(i, c).tolist() == v.q(c).tolist(), (cases[i].name, c)


@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_the_catalogue_in_one_call_per_form(catalogue, form):
    J, torch, groups = catalogue
    for b, views, cases in groups:
        pack_and_check(J, torch, b, views, all_pairs(views), form, what="catalogue (%s ...)" % cases[0].name)


def test_the_claims_of_the_catalogue_hold_for_the_rows_the_kernel_writes(catalogue):
    """The claims of tests/coef_hist_cases.py -- counts in plain Python integers -- asked of coef_hist_all's rows instead of the model's."""
    J, torch, groups = catalogue

    class Kernel:
        def __init__(self, b, view, i):
            self.b, self.i, self.tensor, self.q, self.memo = b, i, view.tensor, view.q, {}

        def row(self, c, R, quantised=True, zigzag=False):
            key = (c, R, quantised, zigzag)
            if key not in self.memo:
                pairs, rows = self.b.coef_hist_all(images=[self.i], comps=[c], range=R, quantised=quantised, zigzag=zigzag)
                assert pairs == [(self.i, c)] and rows.shape == (1, HM.words(R)) and rows.dtype == np.uint32
                self.memo[key] = rows[0]
            return self.memo[key]

    for b, views, cases in groups:
        for i, case in enumerate(cases):
            if case.name != "one_value_everywhere_64x64_blocks" and not case.name.startswith("clamp_edges"):      # (those two kinds: the forms above compare every word)
                case.claim(Kernel(b, views[i], i))


def test_a_decode_ac_0_image_has_positions_1_to_63_in_the_zero_bin(harness, oracles):
    import jpegsnoop_amd as J
    import torch
    case = next(c for c in HC.built() if not c.decode_ac)
    view = HC.OracleView(harness, oracles, case.truth_data, decode_ac=False)
    assert not view.blocks[:, 1:].any()
    b = decoded_batch(J, [case.data], decode_ac=False)
    try:
        for form in ((2, True, False), (127, False, True)):
            pack_and_check(J, torch, b, [view], all_pairs([view]), form, what=case.name)
        pairs, rows = b.coef_hist_all(range=2)
        case.claim(type("K", (), {"tensor": view.tensor, "q": view.q, "row": staticmethod(lambda c, R, quantised=True, zigzag=False: rows[c])})())
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ geometry
def geometry_shapes(unit):
    """(width, height, layout, restart interval): widths and heights of 1, 8, 9 and 17 pixels over the six layouts, with and without restart intervals; then
    grids of unit - 1, unit, unit + 1 and 2 unit + 1 blocks of luma (grey: one block per MCU) and of chroma (4:2:0 and 4:1:1)."""
    out, k = [], 0
    for w in (1, 8, 9, 17):
        for h in (1, 8, 9, 17):
            out.append((w, h, k % 6, 2 * (k % 2))); k += 1
    for j, nblk in enumerate((unit - 1, unit, unit + 1, 2 * unit + 1)):
        out.append((8 * nblk, 8, 4, 3 * (j % 2)))                                  # grey: nblk blocks
        out.append((16 * nblk, 16, 2, 3 * ((j + 1) % 2)))                          # 4:2:0: nblk chroma blocks, 4 nblk luma blocks
        out.append((32 * nblk, 8, 5, 0))                                           # 4:1:1: nblk chroma blocks
    return out


@pytest.fixture(scope="module")
def geometry(harness, oracles):
    import jpegsnoop_amd as J
    import torch
    U = J.capi.COEF_HIST_UNIT
    shapes = geometry_shapes(U)
    files = [harness.synth_jpeg(width=w, height=h, quality=92, restart_interval=dri, seed=2100 + k, **LAYOUTS[s]) for k, (w, h, s, dri) in enumerate(shapes)]
    views = [HC.OracleView(harness, oracles, f) for f in files]
    sizes = {int(np.prod(v.geo.grid(c))) for v in views for c in range(v.geo.ncomp)}
    assert {U - 1, U, U + 1, 2 * U + 1} <= sizes and {v.geo.hv[0] for v in views} >= {(1, 1), (2, 1), (2, 2), (1, 2), (4, 1)}, sorted(sizes)
    b = decoded_batch(J, files)
    yield J, torch, b, views, shapes
    b.close()


@pytest.mark.parametrize("form", [(16, True, False), (127, False, True), (1, True, True), (2, False, False)], ids=form_id)
def test_layouts_sizes_and_unit_seams_dense_and_pitched(geometry, form):
    J, torch, b, views, _ = geometry
    pack_and_check(J, torch, b, views, all_pairs(views), form, what="geometry")
    pack_and_check(J, torch, b, views, all_pairs(views), form, extra=5, what="geometry", calls=1)


def test_lists_repeats_reversed_one_component_and_a_refused_grey_component(geometry):
    J, torch, b, views, shapes = geometry
    form = (16, True, False)
    grey = [i for i, v in enumerate(views) if v.geo.ncomp == 1]; colour = [i for i, v in enumerate(views) if v.geo.ncomp == 3]
    every = all_pairs(views)
    pack_and_check(J, torch, b, views, every[::-1], form, what="reversed")
    pack_and_check(J, torch, b, views, [every[3], every[3], every[0], every[3]], form, what="repeats")
    pack_and_check(J, torch, b, views, [(i, 1) for i in colour], form, what="one component only")
    pack_and_check(J, torch, b, views, all_pairs(views, [colour[-1]]), form, what="one image, dense")
    pack_and_check(J, torch, b, views, all_pairs(views, [colour[-1]]), form, extra=7, what="one image, pitched")
    pack_and_check(J, torch, b, views, [(grey[0], 0), (colour[0], 2), (grey[1], 0), (colour[1], 0), (grey[0], 0)], form, what="grey mixed with colour")
    # refusals: nothing launched, nothing written
    words = HM.words(16)
    ar = Arena(torch, 2, words, words)
    torch.cuda.synchronize()
    lib = J.load(); spec = make_spec(J, form)

    def refused(pairs, word, ptr=None, pitch=0, s=None):
        rc = raw_pack(J, b, spec if s is None else s, pairs, ar.ptr() if ptr is None else ptr, pitch)
        assert rc == -1 and word in J.last_error(), (rc, word, J.last_error())

    refused([(colour[0], 0), (grey[0], 1)], "component")                          # comp 1 of a grey image, behind a good entry
    refused([(colour[0], 3)], "component")
    refused([(colour[0], -1)], "component")
    refused([(len(views), 0)], "out of range")
    refused([(-1, 0)], "out of range")
    refused([(colour[0], 0)], "multiple of 4", ptr=ar.ptr() + 2)
    refused([(colour[0], 0)], "row_pitch_words", pitch=words - 1)
    refused([(colour[0], 0)], "NULL", ptr=0)
    for field, val, word in (("range", 0, "range"), ("range", 128, "range"), ("order", 2, "order"), ("struct_size", 20, "struct_size"), ("struct_size", 0, "struct_size")):
        s = make_spec(J, form); setattr(s, field, val)
        refused([(colour[0], 0)], word, s=s)
    one = (C.c_int * 1)(colour[0]); zero = (C.c_int * 1)(0)
    assert lib.jsnoop_batch_pack_coef_hist(b._h, None, one, zero, 1, ar.ptr(), 0) == -1 and "spec is NULL" in J.last_error()
    assert lib.jsnoop_batch_pack_coef_hist(b._h, C.byref(spec), None, zero, 1, ar.ptr(), 0) == -1 and "images is NULL" in J.last_error()
    assert lib.jsnoop_batch_pack_coef_hist(b._h, C.byref(spec), one, None, 1, ar.ptr(), 0) == -1 and "comps is NULL" in J.last_error()
    assert lib.jsnoop_batch_pack_coef_hist(b._h, C.byref(spec), one, zero, -1, ar.ptr(), 0) == -1
    assert lib.jsnoop_batch_pack_coef_hist(b._h, C.byref(spec), None, None, 0, None, 0) == 0                                   # n == 0
    fresh = J.JpegBatch()
    try:
        fresh.add_jpeg(b"" + bytes(HC.built()[0].data))
        assert raw_pack(J, fresh, spec, [(0, 0)], ar.ptr(), 0) == -1 and "not been decoded" in J.last_error()
    finally:
        fresh.close()
    b.sync(); torch.cuda.synchronize()
    assert ar.untouched(), "a refused call wrote to the destination"
    # a shorter struct_size: the lacking fields at their defaults (range stays 127 although the caller's bytes say 16)
    s = make_spec(J, (16, True, True)); s.struct_size = 8
    ar2 = Arena(torch, 1, HM.words(127), HM.words(127)); ar2.place(0, views[colour[0]].row(0, 127, True, True))
    torch.cuda.synchronize()
    assert raw_pack(J, b, s, [(colour[0], 0)], ar2.ptr(), 0) == 0, J.last_error()
    b.sync(); torch.cuda.synchronize()
    ar2.check("struct_size 8", [(colour[0], 0)], 127)


# ------------------------------------------------------------------------------------------------ the deal
def test_a_destination_over_three_shares_and_a_share_over_three_destinations(harness, oracles):
    """Sized from the kernel's own constants: the single-value file (64 units) lies behind six one-unit rows, so with shares of WAVES units (the grid rule gives
    no more while the units are few) it spans eight workgroups, whose sums meet in its row, and the first shares hold three destinations and more."""
    import jpegsnoop_amd as J
    import torch
    cap = J.capi
    one = next(c for c in HC.built() if c.name == "one_value_everywhere_64x64_blocks")
    small = [harness.synth_jpeg(width=24 + 8 * k, height=16, quality=95, seed=3100 + k, **LAYOUTS[(0, 4)[k % 2]]) for k in range(4)]
    files = small[:2] + [one.data] + small[2:]
    views = [HC.OracleView(harness, oracles, f) for f in files]
    pairs = all_pairs(views, [0, 1]) + [(2, 0)] + all_pairs(views, [3, 4]) + [(2, 0), (0, 0)]
    units = [-(-int(np.prod(views[i].geo.grid(c))) // cap.COEF_HIST_UNIT) for i, c in pairs]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for R in (127, 16):
        share = cap.coef_hist_share(sum(units), cus, R)
        start = np.cumsum([0] + units)
        spans = [int((start[k + 1] - 1) // share - start[k] // share + 1) for k in range(len(pairs))]          # shares a destination touches
        held = [len({k for k in range(len(pairs)) if start[k] < (s + 1) * share and start[k + 1] > s * share}) for s in range(-(-sum(units) // share))]
        assert max(spans) >= 3 and max(held) >= 3, (share, spans, held)
    b = decoded_batch(J, files)
    try:
        for form in ((127, True, False), (16, False, True), (1, True, False)):
            pack_and_check(J, torch, b, views, pairs, form, what="deal")
    finally:
        b.close()


def test_calls_of_so_many_units_that_a_wave_walks_several_units_and_destinations(harness, oracles, capsys):
    """The test above has shares of CH_WAVES units: a wave takes one unit of a destination, if any.  Here the list is sized from the device
    (tests/deal_cases.py, proven on the CPU by tests/test_deal_cases.py): a share of 24 units and more.  Destinations of 3 shares and more lie in the
    middle of the list -- whole shares inside one destination, every wave with three units and its minima and maxima carried from unit to unit --, a
    wave takes two and more units of a destination before the share flushes and moves on to the next, one share holds up to a share's length of
    one-unit destinations, flushed one after the other through the same histogram, and shares start inside destinations and on their first unit.
    k_coef_hist walks a share destination by destination: `k++` once a destination, no step passes over one.  A dozen distinct (file, component) pairs
    listed a few hundred times; R = 16 and R = 1, and R = 127 (65 KB a row) over the same list; the whole arena of every call against the model."""
    import jpegsnoop_amd as J
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    recs = D.coef_hist_records(cus)
    c = D.census_of("coef_hist", "any", recs, cus)
    with capsys.disabled():
        print("\nk_coef_hist, %d compute units: %s; some workgroup's waves take %d units each" % (cus, D.summary(c), c.best_full))
    assert D.missing(c, D.KERNELS["coef_hist"]["waves"], **D.conditions("coef_hist", "any")) == [], D.summary(c)
    assert len(recs) < 500
    images = sorted({r.pic[:3] for r in recs})
    files = [harness.synth_jpeg(width=w, height=h, quality=(95, 85)[k % 2], restart_interval=(0, 5)[k % 2], seed=3300 + k, **LAYOUTS[l]) for k, (l, w, h) in enumerate(images)]
    views = [HC.OracleView(harness, oracles, f) for f in files]
    pairs = [(images.index(r.pic[:3]), r.pic[3]) for r in recs]
    U = J.capi.COEF_HIST_UNIT
    for r, (i, comp) in zip(recs, pairs):                             # the units the census counted are the units of the call
        n = int(np.prod(views[i].geo.grid(comp)))
        assert r.sizes == [U] * (n // U) + ([n % U] if n % U else []), r.pic
    k_long = [k for k, r in enumerate(recs) if r.units >= 3 * c.S]
    assert any(len(recs) // 4 < k < 3 * len(recs) // 4 for k in k_long), "a destination of three shares in the middle of the list"
    for R in (16, 1, 127):
        assert c.S == J.capi.coef_hist_share(c.total, cus, R)
    b = decoded_batch(J, files)
    try:
        for form in ((16, True, False), (1, True, True), (127, False, True)):
            pack_and_check(J, torch, b, views, pairs, form, what="deal", calls=1 if form[0] == 127 else 2)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ read, torch, streams
def test_read_equals_pack_and_coef_hist_to_torch_with_out_and_on_another_stream(geometry):
    J, torch, b, views, _ = geometry
    colour = [i for i, v in enumerate(views) if v.geo.ncomp == 3]
    pairs, rows = b.coef_hist_to_torch(range=16)
    assert pairs == all_pairs(views) and rows.dtype == torch.int32 and tuple(rows.shape) == (len(pairs), HM.words(16)) and rows.is_cuda
    want = np.stack([views[i].row(c, 16) for i, c in pairs])
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), want)
    hp, host = b.coef_hist_all(range=16)
    assert hp == pairs and np.array_equal(host, want), "read equals pack"
    hist, mn, mx = J.coef_hist_fields(rows[0], 16)
    assert tuple(hist.shape) == (64, 33) and int(hist.sum()) == 64 * int(np.prod(views[0].geo.grid(0))) and int(mn[0]) <= int(mx[0])
    # subsets: images alone, comps alone, pairs
    p2, r2 = b.coef_hist_to_torch(images=[colour[1], 0], range=2, quantised=False, zigzag=True)
    assert p2 == all_pairs(views, [colour[1], 0]) and np.array_equal(r2.cpu().numpy().view(np.uint32), np.stack([views[i].row(c, 2, False, True) for i, c in p2]))
    p3, r3 = b.coef_hist_to_torch(images=[colour[0], colour[0], colour[2]], comps=[2, 2, 0], range=1)
    assert p3 == [(colour[0], 2), (colour[0], 2), (colour[2], 0)] and np.array_equal(r3.cpu().numpy().view(np.uint32), np.stack([views[i].row(c, 1) for i, c in p3]))
    # out=: a strided outer dimension, returned as it is, the columns behind the row untouched
    n, words = len(p3), HM.words(1)
    big = torch.full((n, words + 9), -7, dtype=torch.int32, device="cuda")
    p4, r4 = b.coef_hist_to_torch(images=[i for i, _ in p3], comps=[c for _, c in p3], range=1, out=big)
    assert r4 is big and np.array_equal(big[:, :words].cpu().numpy().view(np.uint32), r3.cpu().numpy().view(np.uint32)) and bool((big[:, words:] == -7).all().item())
    for bad, word in ((big[:2], "shape"), (big.float(), "wanted"), (big.cpu(), "wanted"), (big[:, :words - 1], "shape"), (big.t().contiguous().t(), "contiguous")):
        with pytest.raises(ValueError, match=word):
            b.coef_hist_to_torch(images=[i for i, _ in p3], comps=[c for _, c in p3], range=1, out=bad)
    with pytest.raises(IndexError):
        b.coef_hist_to_torch(images=[len(views)])
    with pytest.raises(IndexError):
        b.coef_hist_to_torch(images=[0], comps=[3])
    with pytest.raises(ValueError):
        b.coef_hist_to_torch(range=128)
    with pytest.raises(ValueError):
        b.coef_hist_to_torch(images=[0, 1], comps=[0])
    assert b.coef_hist_to_torch(images=[])[0] == []
    # a non-default torch stream: the fill on it is finished before the batch's stream writes, the rows are ready on return
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        out = torch.full((len(pairs), HM.words(16)), -1, dtype=torch.int32, device="cuda")
        _, r5 = b.coef_hist_to_torch(range=16, out=out)
        got = r5.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ ordering: two streams, DC-only, damaged files
def test_the_call_waits_for_both_halves_of_a_two_stream_decode(harness, oracles):
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=333, height=217, seed=40 + k) for k in range(5)]
    views = [HC.OracleView(harness, oracles, f) for f in files]
    b = J.JpegBatch()
    try:
        for f in files:
            b.add_jpeg(f)
        b.set_split(2); b.upload()
        assert b.split_parts() == 2
        b.decode()
        pack_and_check(J, torch, b, views, all_pairs(views), (127, True, False), what="two-stream decode", before_sync=True)
        assert b.last_form() == 1
    finally:
        b.close()


def test_behind_a_dc_only_fast_form_decode_the_form_goes_2_to_1(harness, oracles):
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=100, height=75, hs=2, vs=2, restart_interval=3 * (k % 2), seed=500 + k) for k in range(3)]
    views = [HC.OracleView(harness, oracles, f, decode_ac=False) for f in files]
    b = decoded_batch(J, files, decode_ac=False)
    try:
        assert b.last_form() == 2
        pack_and_check(J, torch, b, views, all_pairs(views), (16, True, False), what="DC-only", before_sync=True)
        assert b.last_form() == 1, "behind a fast-form decode the call decodes again in the generic form"
        pack_and_check(J, torch, b, views, all_pairs(views), (127, False, True), what="DC-only, second call")
        assert b.last_form() == 1
    finally:
        b.close()


def test_damaged_files_before_and_after_sync(harness, oracles):
    """After sync: the repaired arena, which is the oracle's decode of the damaged bytes.  Before sync: what the parallel path left -- the model is fed with the
    BLOCKS / I16 / NATURAL tensor jsnoop_batch_pack_coefs gives at that moment, whose slots 1..63 are read_coefs' of that moment."""
    import jpegsnoop_amd as J
    import torch
    bases = F.bases(harness)
    hurt = []
    for base, seed in DAMAGED:
        data, _q, mode = F.mutate(harness, np.random.default_rng(seed), bases[base])
        assert mode == 0 and data != bases[base]
        hurt.append(data)
    files = [bases[0], hurt[0], hurt[1], bases[1]]
    views = [HC.OracleView(harness, oracles, f) for f in files]
    form = (127, True, False); words = HM.words(127)
    b = J.JpegBatch()
    try:
        for f in files:
            b.add_jpeg(f)
        b.upload(); b.decode()                                      # no sync: what the parallel path left
        pairs = all_pairs(views)
        grids = [b.coef_grid(i, c) for i, c in pairs]
        tens = [torch.empty((bh, bw, 64), dtype=torch.int16, device="cuda") for bw, bh in grids]
        ar = Arena(torch, len(pairs), words, words)
        torch.cuda.synchronize()
        cs = J.capi.CoefSpec(); J.load().jsnoop_coef_spec_defaults(C.byref(cs))
        dst = (J.capi.CoefDst * len(pairs))(*[J.capi.CoefDst(t.data_ptr(), 0, 0, c, 0) for t, (_, c) in zip(tens, pairs)])
        ind = (C.c_int * len(pairs))(*[i for i, _ in pairs])
        assert J.load().jsnoop_batch_pack_coefs(b._h, C.byref(cs), ind, len(pairs), dst) == 0, J.last_error()
        assert raw_pack(J, b, make_spec(J, form), pairs, ar.ptr(), 0) == 0, J.last_error()
        arenas = {i: b.coefs(i) for i in range(len(files))}         # read_coefs of that moment (the copy runs on the batch's stream behind both calls)
        torch.cuda.synchronize()
        for k, (i, c) in enumerate(pairs):
            t = tens[k].cpu().numpy()
            assert np.array_equal(t[..., 1:], arenas[i][views[i].geo.arena_index(c)][..., 1:]), (i, c)
            ar.place(k, HM.row_of_tensor(t, b.dqt(i, c), 127, True, False))
        ar.check("before sync", pairs, 127)
        b.sync()
        assert b.info(1)["flags"] != 0 and b.info(2)["flags"] != 0
        pack_and_check(J, torch, b, views, pairs, form, what="after sync")
        pack_and_check(J, torch, b, views, pairs, (16, False, True), what="after sync")
    finally:
        b.close()


def test_baseline_and_progressive_files_in_one_job(harness, oracles):
    """A JpegJob over baseline and progressive catalogue files on one device: every file's rows taken inside the callback equal the model over the oracle's
    decode of the baseline encoding."""
    import jpegsnoop_amd as J
    import torch
    cases = [c for c in HC.built() if c.name.startswith("dc_constant_difference_1")] + [next(c for c in HC.built() if c.name == "extrema_through_the_int16_wrap")]
    assert sum(c.truth_data is not c.data for c in cases) == 2
    files = [c.data for c in cases] + [harness.synth_jpeg(width=65, height=33, seed=70), b"not a jpeg"]
    views = [HC.OracleView(harness, oracles, c.truth_data) for c in cases] + [HC.OracleView(harness, oracles, files[-2]), None]
    job = J.JpegJob(devices=[0])
    seen = {}
    try:
        for f in files:
            job.add(f)

        def on_file(r):
            if r.status == "ok":
                pairs, rows = r.coef_hist_to_torch(range=16, zigzag=True)
                p1, one = r.coef_hist_to_torch(range=16, zigzag=True, comps=[0])
                assert p1 == [pairs[0]] and torch.equal(one[0], rows[0])
                seen[r.index] = (r.kind, [c for _, c in pairs], rows.cpu().numpy().view(np.uint32))
            else:
                with pytest.raises(RuntimeError):
                    r.coef_hist_to_torch()
            return False

        job.run(on_file)
    finally:
        job.close()
    assert sorted(seen) == list(range(len(files) - 1)) and {k for k, _, _ in seen.values()} == {"baseline", "progressive"}
    for i, (kind, comps, rows) in seen.items():
        assert comps == list(range(views[i].geo.ncomp))
        for c in comps:
            assert np.array_equal(rows[c], views[i].row(c, 16, True, True)), (i, kind, c)
