"""-m gpu: the DC predictor scan (k_dc_scan; k_dc_scan_parts, the two-level form of jobs of up to JS_DC_PARTS_IMAGES = 8 images) on the
catalogue of tests/dc_scan_cases.py: all-DC files whose MCU counts, restart intervals and markers inside an MCU put resets and carries on
the seams of the scan -- lane 0 / 63 of a wave, the wave totals of a 1024-MCU step, the carry between steps, the part summaries and
their fold -- with predictors that wrap int16 thousands of times and, in group D, `int` sums that pass 2**31.
tests/test_dc_scan_cases.py proves on the CPU that every file holds its event, that a plain numpy model of the predictors reproduces the
oracle on every file, and that the oracle's answers are the compiled reference's.

Every file is decoded by BOTH forms of the scan: in a batch of at most 8 images (two-level) and as one of at least 9 (one-level); in every
form of the entropy path that changes how the scan is reached (split halves: no part summaries whatever the size; the write pass's lane
forms and its first version; decode_ac = 0 through the DC-only fast form and through the generic kernels), and alone through the
single-image call.  All comparisons are exact: the DIB, the int16 planes, the DIB checksum; through the single-image call also the
block-DC maps, the status words and the MCU file map.  Groups A..D must come from the parallel path without a flag; group E (markers
inside an MCU) from the parallel path with flag 0x8 and without 0x100 -- had the sequential mirror taken a file, the scan was not tested.
A failure names the first differing block, its MCU, MCU % 64, MCU % 1024 and MCU // per: the seam is readable from the message.
"""
import numpy as np
import pytest

import dc_scan_cases as DC

pytestmark = pytest.mark.gpu

XC_WRITE_V1 = 2          # jpegsnoop_amd.capi.XC_WRITE_V1
XC_DC_GENERIC = 0x40     # jpegsnoop_amd.capi.XC_DC_GENERIC
# (name, decode_ac, tuning)
FORMS = [("default", True, {}), ("split_1", True, {"split": 1}), ("split_2", True, {"split": 2}), ("write_lanes_1", True, {"write_lanes": 1}),
         ("write_lanes_2", True, {"write_lanes": 2}), ("write_v1", True, {"cross_checks": XC_WRITE_V1}),
         ("dc_only_fast", False, {}), ("dc_only_generic", False, {"cross_checks": XC_DC_GENERIC})]
BIG_FORMS = [f for f in FORMS if f[0] in ("default", "split_2", "dc_only_fast")]


class Answer:
    """The oracle's decode of one file: full (decode_ac = 1) and DC-only; one copy where the two are the same."""

    def __init__(self, harness, oracle, c):
        import jpegsnoop_amd as J
        self.full = self._take(harness, oracle, c, J)
        oracle.set_options(decode_ac=0)
        try:
            dc = self._take(harness, oracle, c, J)
        finally:
            oracle.set_options()
        same = dc["cks"] == self.full["cks"] and all(np.array_equal(a, b) for a, b in zip(dc["planes"], self.full["planes"]))
        self.dc_only = self.full if same else dc

    @staticmethod
    def _take(harness, oracle, c, J):
        harness.drive(oracle, c.file)
        dib = oracle.dib()
        return dict(size=oracle.image_size(), dib=dib, cks=J.dib_checksum_numpy(dib), planes=[p for p in oracle.planes() if p is not None],
                    blk_dc=oracle.blk_dc(), status=oracle.status(), mcu_map=oracle.mcu_map())


@pytest.fixture(scope="module")
def world(harness, oracle):
    import jpegsnoop_amd as J
    assert XC_WRITE_V1 == J.capi.XC_WRITE_V1 and XC_DC_GENERIC == J.capi.XC_DC_GENERIC
    cases = DC.build_all()
    return {c.name: (c, Answer(harness, oracle, c)) for c in cases}


def small(world):
    return [ca for ca in world.values() if ca[0].group in "ABE"]


def big(world):
    return [ca for ca in world.values() if ca[0].group in "CD"]


def plane_difference(c, got, want):
    """The first block whose top-left plane sample differs, per component, in decode order."""
    for comp in range(c.frame.ncomp):
        if got[comp].shape != want[comp].shape:
            return "%s: plane %d of %s, expected %s" % (c.name, comp, got[comp].shape, want[comp].shape)
        if np.array_equal(got[comp], want[comp]):
            continue
        rows, cols, _ = DC.planes_corner(c, [np.zeros(c.nmcu * h * v, np.int16) for h, v in c.frame.hv])[comp]
        e = DC.first_block_difference(c, comp, got[comp][rows, cols], want[comp][rows, cols])
        return e or "%s: plane %d differs behind the top-left samples of its blocks" % (c.name, comp)
    return None


def check_image(b, i, c, want, errs, what):
    inf = b.info(i)
    if c.group == "E":
        ok = inf["path"] == 1 and (inf["flags"] & 0x8) and not (inf["flags"] & 0x100)
    else:
        ok = inf["path"] == 1 and inf["flags"] == 0
    if not ok:
        errs.append("%s (image %d, %s): path %d flags %#x" % (c.name, i, what, inf["path"], inf["flags"]))
    e = plane_difference(c, b.planes(i), want["planes"])
    if e:
        errs.append("%s, image %d: %s" % (what, i, e))
    g = b.dib(i)
    if g.shape != want["dib"].shape or not np.array_equal(g, want["dib"]):
        errs.append("%s (image %d, %s): DIB differs in %d bytes" % (c.name, i, what, int((g != want["dib"]).sum()) if g.shape == want["dib"].shape else -1))


def run_batch(items, decode_ac, tuning, what, tile=0, full_compare=None):
    """items: [(case, answer)].  Decodes them as one batch (tiled to `tile` images), compares every image, decodes the resident batch once
    more.  Returns (last_form, per-image checksums)."""
    import jpegsnoop_amd as J
    b = J.JpegBatch(decode_ac=decode_ac, want_planes=True)
    try:
        b.set_tuning(**tuning)
        for c, _ in items:
            b.add_jpeg(c.file)
        if tile:
            b.tile(tile)
        b.upload(); b.decode(); b.sync()
        form = b.last_form()
        sums = [int(s) for s in b.dib_checksums()]
        errs = []
        for i in range(len(b)):
            c, a = items[i % len(items)]; want = a.full if decode_ac else a.dc_only
            if sums[i] != want["cks"]:
                errs.append("%s (image %d, %s): DIB checksum differs from the oracle's" % (c.name, i, what))
            if full_compare is None or i in full_compare:
                check_image(b, i, c, want, errs, what)
        assert not errs, "%s: %d findings\n%s" % (what, len(errs), "\n".join(errs[:25]))
        b.decode(); b.sync()                       # a second decode of the resident batch
        assert [int(s) for s in b.dib_checksums()] == sums, what
        return form, sums
    finally:
        b.close()


def by_form(items, decode_ac, tuning):
    """The batches a form decodes: the DC-only fast form takes a batch only if every image has one of its four layouts (here 4:4:4,
    4:2:2, 4:2:0), so those files go together and the others apart; group E's files go apart too (a marker inside an MCU raises flag
    0x8, and what sync() then does for a flagged image may decode the batch again in the generic form: their form is printed, not
    asserted).  Every other form takes the list as it is."""
    if decode_ac or tuning:
        return [(items, None)]
    fast = [ca for ca in items if ca[0].layout in DC.FAST_LAYOUTS and ca[0].group != "E"]
    fast_e = [ca for ca in items if ca[0].layout in DC.FAST_LAYOUTS and ca[0].group == "E"]
    rest = [ca for ca in items if ca[0].layout not in DC.FAST_LAYOUTS]
    return [(x, w) for x, w in ((fast, 2), (fast_e, None), (rest, 1)) if x]


def expect_form(name, form, want_fast, what):
    print("%s [%s]: last_form %d" % (what, name, form))
    if name == "dc_only_fast" and want_fast == 2:
        assert form == 2, what
    elif name != "dc_only_fast":
        assert form == 1, what


@pytest.mark.parametrize("name,decode_ac,tuning", FORMS, ids=[f[0] for f in FORMS])
def test_one_level_scan_groups_a_b_e(world, name, decode_ac, tuning):
    """One batch of the catalogue's groups A, B and E (more than 8 images: k_dc_scan, one workgroup per image)."""
    for items, want_fast in by_form(small(world), decode_ac, tuning):
        n = len(items)
        tile = 0 if n > DC.DC_PARTS_IMAGES else n * -(-(DC.DC_PARTS_IMAGES + 1) // n)
        form, _ = run_batch(items, decode_ac, tuning, "%s, one-level, %d files" % (name, n), tile=tile)
        expect_form(name, form, want_fast, "%d files" % n)


@pytest.mark.parametrize("name,decode_ac,tuning", FORMS, ids=[f[0] for f in FORMS])
def test_two_level_scan_groups_a_b_e(world, name, decode_ac, tuning):
    """The same files in batches of at most 8 images: k_dc_scan_parts, 64 parts per image, two launches (the split forms hand their
    halves no summaries: the one-level kernel on small batches)."""
    for items, want_fast in by_form(small(world), decode_ac, tuning):
        for k in range(0, len(items), DC.DC_PARTS_IMAGES):
            chunk = items[k:k + DC.DC_PARTS_IMAGES]
            form, _ = run_batch(chunk, decode_ac, tuning, "%s, two-level, files %d..%d" % (name, k, k + len(chunk) - 1))
            expect_form(name, form, want_fast, "files %d.." % k)


@pytest.mark.parametrize("name,decode_ac,tuning", BIG_FORMS, ids=[f[0] for f in BIG_FORMS])
def test_two_level_scan_parts_of_two_steps_groups_c_d(world, name, decode_ac, tuning):
    """More than 65536 MCUs: `per` = 2048, so a part runs two steps and the carry between them, any_reset and a fold over more than 32
    summaries carry values.  Batches of two files."""
    items = big(world)
    for k in range(0, len(items), 2):
        pair = items[k:k + 2]
        form, _ = run_batch(pair, decode_ac, tuning, "%s, two-level, %s" % (name, " + ".join(c.name for c, _ in pair)))
        print("%s [%s]: last_form %d" % (" + ".join(c.name for c, _ in pair), name, form))
        if name != "dc_only_fast":
            assert form == 1


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("name,decode_ac,tuning", BIG_FORMS, ids=[f[0] for f in BIG_FORMS])
def test_one_level_scan_groups_c_d(world, name, decode_ac, tuning, which):
    """Each file above 65536 MCUs tiled to 9 images: k_dc_scan runs 65 or 66 steps with one carry.  Every image's checksum; the first and
    the last image whole."""
    items = big(world); assert len(items) == 6
    c, a = items[which]
    form, _ = run_batch([(c, a)], decode_ac, tuning, "%s, one-level, 9 x %s" % (name, c.name), tile=DC.DC_PARTS_IMAGES + 1, full_compare=(0, DC.DC_PARTS_IMAGES))
    expect_form(name, form, 2 if c.layout in DC.FAST_LAYOUTS else 1, c.name)


def test_mixed_batch_of_8_and_of_9(world):
    """Eight images with eight different MCU counts (the summaries are indexed img * 64: a stride error shows only with unequal
    neighbours), and the same eight plus one more, which takes them to the one-level kernel: the same results per image."""
    names = ["a_420_63_dri_62", "a_gray_65_no_restart", "a_444_1023_dri_1022", "a_422_1024_dri_1023", "b_420_1025_no_restart", "b_420_2048_dri_1024",
             "a_luma4x2_2049_dri_2048", "b_gray_65536_dri_1023", "a_420_3073_no_restart"]
    items = [world[n] for n in names]
    assert len({c.nmcu for c, _ in items[:8]}) == 8 and len(items) == 9
    assert len({(c.parts, c.last_part) for c, _ in items[:8]}) >= 6, "unequal numbers of parts in use"
    _, s8 = run_batch(items[:8], True, {}, "mixed batch of 8")
    _, s9 = run_batch(items, True, {}, "mixed batch of 9")
    assert s9[:8] == s8


def single_image(harness, gpu, items):
    errs = []
    for c, a in items:
        want = a.full
        harness.drive(gpu, c.file)
        path, flags = gpu.lib.jsnoop_last_path(gpu.h), gpu.lib.jsnoop_last_flags(gpu.h)
        ok = (path == 1 and (flags & 0x8) and not (flags & 0x100)) if c.group == "E" else (path == 1 and flags == 0)
        if not ok:
            errs.append("%s: path %d flags %#x" % (c.name, path, flags))
        e = plane_difference(c, [p for p in gpu.planes() if p is not None], want["planes"])
        if e:
            errs.append("planes: " + e)
        if gpu.image_size() != want["size"] or not np.array_equal(gpu.dib(), want["dib"]):
            errs.append("%s: DIB differs" % c.name)
        for i, (pa, pb) in enumerate(zip(want["blk_dc"], gpu.blk_dc())):
            if pa is not None and not np.array_equal(pa, pb):
                errs.append("%s: block-DC map %d differs" % (c.name, i))
        if gpu.status() != want["status"]:
            errs.append("%s: status %s, oracle %s" % (c.name, gpu.status(), want["status"]))
        if not np.array_equal(gpu.mcu_map(), want["mcu_map"]):
            errs.append("%s: MCU file map differs" % c.name)
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:25]))


@pytest.mark.parametrize("group", ["A", "B", "E", "C"])
def test_alone_through_the_single_image_call(harness, gpu, world, group):
    """Every file of groups A, B and E, and one of group C (the one whose only reset lies in the first step of a part)."""
    items = [ca for ca in world.values() if ca[0].group == group]
    if group == "C":
        items = [ca for ca in items if ca[0].dri == 64000]
    assert items
    single_image(harness, gpu, items)
