"""-m gpu: the DC-only fast form (k_write_dc + k_dc_color, jsnoop_kernels.hip) against the oracle with decode_ac = 0.

DC-only is the reference's default mode: AC symbols are parsed and dropped, the IDCT never runs, every sample of a block is its
cumulative DC.  A batch whose every image is DC-only with one of the four common layouts decodes through a write pass without the
coefficient arena and a back end that goes straight from cumulative DC to DIB; jsnoop_batch_last_form() says which form produced the
results a batch holds (0 nothing, 1 Full-IDCT kernels, 2 fast form).  Everything here is compared bit for bit: the whole DIB (padding
included), the planes, the block-DC maps, the status words, the brightest pixel / average Y -- with the oracle, and the DIB hashes with
the same files through JSNOOP_XC_DC_GENERIC (the Full-IDCT kernels with the AC words masked off: the code DC-only ran through before)."""
import ctypes as C

import numpy as np
import pytest

import backend_images as BI
import base_cases as BC
import base_stream as BS
from golden_util import load_case, manifest

pytestmark = pytest.mark.gpu

LAYOUTS = ("444", "422", "440", "420")
SIZES = [(1, 1), (8, 8), (17, 9), (100, 75), (264, 40), (1032, 24)]      # 264: 1056 bytes per row; 1032: 129 luma blocks, more than a wave's 32
TIE_SIZES = [(100, 75), (264, 40), (1032, 24)]                             # room for two MCU rows of whole blocks in every layout


# ------------------------------------------------------------------------------------------------ inputs
def tie_picture(w, h, seed):
    """Noise no brighter than 200, and -- where the picture has three block rows and three block columns of whole blocks -- three flat white
    luma blocks: A = (1, 0), B = (last whole column, 0) in the same block row, C = (0, 2) in a later MCU row of every layout.  Flat blocks
    keep only their DC, so the three tie exactly; the first in raster order, A, is the brightest pixel."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 201, size=(h, w, 3), dtype=np.uint8)
    if (w, h) in TIE_SIZES:
        last = w // 8 - 1
        rgb[0:8, 8:16] = 255
        rgb[0:8, 8 * last:8 * last + 8] = 255
        rgb[16:24, 0:8] = 255
    return rgb


def parity_files(H):
    """(what, jpeg) for every layout x size x {no DRI, DRI = 1, DRI = one MCU row}, plus one 12-bit-precision file."""
    out = []
    for li, layout in enumerate(LAYOUTS):
        hs, vs, _ = BI.LAYOUTS[layout]
        for si, (w, h) in enumerate(SIZES):
            row = -(-w // (8 * hs))
            for dri in (0, 1, row):
                data = H.encode_rgb(tie_picture(w, h, 1000 + 10 * li + si), hs=hs, vs=vs, quality=90, restart_interval=dri)
                out.append(((layout, w, h, dri), data))
    data = bytearray(H.synth_jpeg(width=100, height=75, hs=2, vs=2, quality=85, restart_interval=3, seed=12))
    sof = data.find(b"\xFF\xC0")
    assert sof > 0 and data[sof + 4] == 8
    data[sof + 4] = 12                                            # SOF precision: values are divided by 1 << 4 (:1234-1238), DC included
    out.append((("420", 100, 75, "12-bit"), bytes(data)))
    return out


_ORACLE = {}


def oracle_dc(H, oracle, data):
    """The oracle's DC-only decode of one file, computed once and shared."""
    key = H.hash_bytes(data)
    if key not in _ORACLE:
        oracle.set_options(decode_ac=0)
        try:
            H.drive(oracle, data)
            _ORACLE[key] = {"dib": oracle.dib(), "planes": oracle.planes(), "bright_avg": oracle.bright_avg(), "blk_dc": oracle.blk_dc(),
                            "status": oracle.status(), "mcu_map": oracle.mcu_map()}
        finally:
            oracle.set_options()
    return _ORACLE[key]


def make_batch(files, decode_ac=False, want_planes=False, log=False, **tuning):
    import jpegsnoop_amd as J
    b = J.JpegBatch(decode_ac=decode_ac, want_planes=want_planes)
    if tuning:
        b.set_tuning(**tuning)
    if log:
        b.enable_log()
    for f in files:
        b.add_jpeg(f)
    b.upload(); b.decode(); b.sync()
    return b


def hashes(b):
    return [int(x) for x in b.dib_checksums()]


@pytest.fixture(scope="module")
def clean420(harness):
    return [harness.synth_jpeg(width=100, height=75, hs=2, vs=2, seed=500 + i) for i in range(3)]


# ------------------------------------------------------------------------------------------------ 1: the form is reported
def test_form_is_reported(harness, oracle, gpu, clean420):
    import jpegsnoop_amd as J
    assert J.capi.XC_DC_GENERIC == 0x40
    b = J.JpegBatch(decode_ac=False)
    try:
        assert b.last_form() == 0                                 # nothing decoded
        for f in clean420:
            b.add_jpeg(f)
        b.upload()
        assert b.last_form() == 0
        b.decode(); b.sync()
        assert b.last_form() == 2
        want = [J.dib_checksum_numpy(oracle_dc(harness, oracle, f)["dib"]) for f in clean420]
        assert hashes(b) == want
        b.clear()
        assert b.last_form() == 0
    finally:
        b.close()
    for kw, form in ((dict(cross_checks=J.capi.XC_DC_GENERIC), 1), (dict(decode_ac=True), 1), (dict(log=True), 1)):
        b = make_batch(clean420, **kw)
        try:
            assert b.last_form() == form, kw
            if not kw.get("decode_ac"):
                assert hashes(b) == want, kw
        finally:
            b.close()
    others = {"gray": harness.synth_jpeg(width=100, height=75, gray=1, seed=510), "h4v1": harness.synth_jpeg(width=100, height=75, hs=4, vs=1, seed=511)}
    for name, other in others.items():
        files = clean420 + [other]
        b = make_batch(files)
        try:
            assert b.last_form() == 1, name
            assert hashes(b) == [J.dib_checksum_numpy(oracle_dc(harness, oracle, f)["dib"]) for f in files], name
        finally:
            b.close()
    # jsnoop_batch_add, one image with decode_ac = 1: its decoder has the option set, and the batch's option -- which is what an image added
    # under a foreign decoder's tables takes its mode from -- is 1 while it is added
    for mixed in (False, True):
        b = J.JpegBatch(decode_ac=False)
        try:
            for i, f in enumerate(clean420):
                p = harness.parse_jpeg(f)
                harness.push_tables(gpu, p)
                ac = 1 if (mixed and i == 1) else 0
                gpu.set_options(decode_ac=ac)
                b._lib.jsnoop_batch_set_options(b._h, ac, 0, 0)
                b.add(gpu, f, p.scan_start)
            b.upload(); b.decode(); b.sync()
            assert b.last_form() == (1 if mixed else 2), mixed
            got = hashes(b)
            assert got[0] == want[0] and got[2] == want[2]
            if mixed:
                harness.drive(oracle, clean420[1])
                assert got[1] == J.dib_checksum_numpy(oracle.dib()) != want[1]      # that image really went through the IDCT
            else:
                assert got[1] == want[1]
        finally:
            gpu.set_options()
            b.close()


# ------------------------------------------------------------------------------------------------ 2: parity on small shapes
def test_tie_break_pictures_tie_where_they_should(harness, oracle):
    """CPU side of the generator: in the oracle's DC-only Y plane blocks A, B and C hold the maximum, and the brightest pixel is A's first."""
    seen = 0
    for (layout, w, h, dri), data in parity_files(harness):
        if (w, h) not in TIE_SIZES or dri == "12-bit":
            continue
        hs, vs, _ = BI.LAYOUTS[layout]
        want = oracle_dc(harness, oracle, data)
        y = want["planes"][0]
        last = w // 8 - 1
        top = int(y.max())
        blocks = {(bx, by) for by in range(y.shape[0] // 8) for bx in range(y.shape[1] // 8) if int(y[8 * by, 8 * bx]) == top}
        assert {(1, 0), (last, 0), (0, 2)} <= blocks, (layout, w, h, dri, sorted(blocks)[:8])      # two in one block row, one in a later MCU row
        assert (0, 0) not in blocks and 16 // (8 * vs) >= 1
        assert want["bright_avg"][7:9] == [8 // (8 * hs), 0], (layout, w, h, dri, want["bright_avg"])      # the earlier one: A
        seen += 1
    assert seen == len(LAYOUTS) * len(TIE_SIZES) * 3


def test_parity_smallest_shapes_mixed_layouts(harness, oracle):
    import jpegsnoop_amd as J
    cases = parity_files(harness)
    files = [d for _, d in cases]
    b = make_batch(files, want_planes=True)
    g = make_batch(files, want_planes=True, cross_checks=J.capi.XC_DC_GENERIC)
    try:
        assert b.last_form() == 2 and g.last_form() == 1
        assert hashes(b) == hashes(g)
        sums = hashes(b)
        for i, (what, data) in enumerate(cases):
            want = oracle_dc(harness, oracle, data)
            inf = b.info(i)
            assert inf["flags"] == 0 and inf["path"] == 1, (what, inf)
            dib = b.dib(i)
            assert dib.shape == want["dib"].shape and np.array_equal(dib, want["dib"]), (what, "DIB differs in %d bytes" % int((dib != want["dib"]).sum()))
            assert sums[i] == J.dib_checksum_numpy(want["dib"]), what
            for c, (pa, pb) in enumerate(zip(want["planes"], b.planes(i))):
                assert np.array_equal(pa, pb), (what, "plane %d" % c)
            so = b.side_outputs(i)
            for c in range(3):
                assert np.array_equal(so["blk_dc"][c], want["blk_dc"][c]), (what, "block-DC map %d" % c)
            assert np.array_equal(so["mcu_map"], want["mcu_map"]), what
            assert [int(v) for v in so["status"].values()] == [int(v) for v in want["status"].values()], (what, so["status"], want["status"])
            assert so["bright_avg"] == want["bright_avg"], (what, so["bright_avg"], want["bright_avg"])
        assert b.last_form() == 2                                 # nothing above fell back
    finally:
        b.close(); g.close()


# ------------------------------------------------------------------------------------------------ 3: every entropy form
def colour_pair_edge_cases():
    """Three of the pair-entry edge files of tests/base_cases.py (a visible pair whose second symbol starts -1 / 0 / +1 bits behind the ends and
    the middles of the sub-sequences of every sub_wl), re-framed: the same blocks, the same tables for all three components, written as one
    row of 4:4:4 MCUs -- the bit stream, and so every symbol's place against the sub-sequence boundaries, is the gray file's."""
    keep = BC.one_row
    def colour_row(tabs, blocks, name, check, comp_ids=((0, 0),), q=BC.QV, dri=0, **kw):
        assert dri == 0 and len(comp_ids) == 1
        blocks = list(blocks)
        while len(blocks) % 3:
            blocks.append([(0, 0), (0, 0)])                      # DC difference 0, end of block
        return BC.Case(name, BS.write(BC.color(len(blocks) // 3, 1, 1, 1, q, q), tabs, [comp_ids[0]] * 3, blocks, 0), check, **kw)
    BC.one_row = colour_row
    try:
        cases = [BC._sweep("colour_sweep_02_01_%+d" % d, 0x02, 0x01, d, 210 + d)() for d in (-1, 0, 1)]
    finally:
        BC.one_row = keep
    for c in cases:
        c.check(c)                                                # the census still proves the placement
        assert c.stream.frame.ncomp == 3
    return cases


ENTROPY_FORMS = [("sub_wl_%d" % w, {"sub_wl": w}) for w in (4, 5, 6, 7, 8)] + [
    ("cand_off", {"cand_rounds": -1}), ("cand_16", {"cand_rounds": 16}), ("sync_launches_2", {"sync_launches": 2}),
    ("split_1", {"split": 1}), ("split_2", {"split": 2}), ("write_lanes_1", {"write_lanes": 1}), ("write_lanes_2", {"write_lanes": 2}),
    ("unstuff_3pass", {"cross_checks": 0x20}), ("default", {})]


@pytest.fixture(scope="module")
def entropy_world(harness, oracle):
    import jpegsnoop_amd as J
    assert J.capi.XC_UNSTUFF_3PASS == 0x20
    a = [harness.synth_jpeg(width=100, height=75, hs=(2, 2, 1, 1)[i % 4], vs=(2, 1, 2, 1)[i % 4], restart_interval=(0, 0, 0, 0, 1, 7)[i % 6], seed=600 + i) for i in range(8)]
    a.append(harness.synth_jpeg(width=640, height=480, seed=609))
    e = [c.file for c in colour_pair_edge_cases()]
    return [(files, [J.dib_checksum_numpy(oracle_dc(harness, oracle, f)["dib"]) for f in files]) for files in (a, e)]


@pytest.mark.parametrize("form,tuning", ENTROPY_FORMS, ids=[f for f, _ in ENTROPY_FORMS])
def test_every_entropy_form_feeds_the_dc_write_pass(harness, oracle, entropy_world, form, tuning):
    for files, want in entropy_world:
        b = make_batch(files, **tuning)
        try:
            assert b.last_form() == 2, form
            assert all(b.info(i)["flags"] == 0 for i in range(len(files))), form
            assert hashes(b) == want, form
            for i in (0, len(files) - 1):
                assert np.array_equal(b.dib(i), oracle_dc(harness, oracle, files[i])["dib"]), (form, i)
            b.decode(); b.sync()                                  # a second decode of the resident batch
            assert b.last_form() == 2 and hashes(b) == want, form
        finally:
            b.close()


# ------------------------------------------------------------------------------------------------ 4: damaged files fall back
def test_damaged_files_fall_back_and_stay_right(harness, oracle, clean420):
    import jpegsnoop_amd as J
    names = [n for n in sorted(manifest()["cases"]) if n.startswith("bad_") and "gray" not in n]
    assert len(names) >= 12
    files = []
    for i, n in enumerate(names):
        files += [clean420[i % len(clean420)], load_case(n)]
    files.append(clean420[0])
    b = make_batch(files)
    g = make_batch(files, cross_checks=J.capi.XC_DC_GENERIC)
    try:
        assert b.last_form() == 1 and g.last_form() == 1
        assert any(g.info(i)["flags"] for i in range(len(files))), "the goldens must raise flags"
        hb, hg = hashes(b), hashes(g)
        for i, f in enumerate(files):
            want = oracle_dc(harness, oracle, f)["dib"]
            assert hb[i] == hg[i] == J.dib_checksum_numpy(want), i
            assert np.array_equal(b.dib(i), want), i
            assert (b.info(i)["flags"], b.info(i)["path"]) == (g.info(i)["flags"], g.info(i)["path"]), i
    finally:
        b.close(); g.close()


# ------------------------------------------------------------------------------------------------ 5: readers of the coefficient arena
def test_coefs_after_a_fast_decode(harness, oracle, clean420):
    import jpegsnoop_amd as J
    b = make_batch(clean420)
    g = make_batch(clean420, cross_checks=J.capi.XC_DC_GENERIC)
    try:
        assert b.last_form() == 2
        want = hashes(b)
        for i in range(len(clean420)):
            got = b.coefs(i)
            assert b.last_form() == 1                             # the arena was filled by a second, generic decode
            assert np.array_equal(got, g.coefs(i)), i
            assert not got[:, 1:].any() and got[:, 0].any()       # DC-only: AC positions stay empty
        assert hashes(b) == want
        b.decode(); b.sync()
        assert b.last_form() == 2 and hashes(b) == want           # the next decode takes the fast form again
    finally:
        b.close(); g.close()


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and np.array_equal(a, b)


def compare_single(oracle, gpu, what):
    if oracle.dib() is not None:
        assert same(gpu.dib(), oracle.dib()), what
    for c, (pa, pb) in enumerate(zip(oracle.planes(), gpu.planes())):
        assert same(pa, pb), (what, "plane %d" % c)
    assert gpu.bright_avg() == oracle.bright_avg(), what
    assert gpu.status() == oracle.status(), what


@pytest.mark.parametrize("display", [0, 1], ids=["bDisplay_false", "decode_ac_0"])
def test_single_image_decoder(harness, oracle, gpu, display):
    """bDisplay = FALSE forces DC-only (the scan is decoded, nothing is shown); with bDisplay = TRUE the option bDecodeScanImgAc = false does.  Neither has
    a log callback here: form 2.  A preview re-render reads the coefficient arena: the decode is repeated in the generic form first."""
    data = harness.synth_jpeg(width=176, height=112, seed=41)
    form = lambda: gpu.lib.jsnoop_last_form(C.c_void_p(gpu.h))
    want = oracle_dc(harness, oracle, data)                      # (bDisplay = FALSE leaves the oracle without DIB and planes: the samples are those of a DC-only decode)
    want_dc = want["dib"]
    try:
        for be in (oracle, gpu):
            be.set_options(decode_ac=0 if display else 1)
        harness.drive(gpu, data, display=display)
        assert form() == 1                                        # the harness backend logs through a callback: today's path
        gpu.set_log_callback(type(gpu._log_cb)(), None)            # (a null callback)
        for be in (oracle, gpu):
            harness.drive(be, data, display=display)
        assert form() == 2
        assert gpu.lib.jsnoop_last_path(gpu.h) == 1 and gpu.lib.jsnoop_last_flags(gpu.h) == 0
        if display:
            assert oracle.dib() is not None
        if display:
            compare_single(oracle, gpu, "decode")
            assert same(gpu.mcu_map(), oracle.mcu_map())
            for pa, pb in zip(oracle.blk_dc(), gpu.blk_dc()):
                assert same(pa, pb)
        assert np.array_equal(gpu.dib(), want_dc)
        for pa, pb in zip(want["planes"], gpu.planes()):
            assert same(pa, pb)
        for pa, pb in zip(want["blk_dc"], gpu.blk_dc()):
            assert same(pa, pb)
        assert form() == 2                                        # the side outputs need no coefficients
        for mode in (2, 1):
            for be in (oracle, gpu):
                be.set_preview_mode(mode)                         # re-render: the colour kernel reads the arena
            assert form() == 1
            if display:
                compare_single(oracle, gpu, ("preview", mode))
            elif oracle.dib() is not None:
                assert same(gpu.dib(), oracle.dib()), mode
            if mode == 1:
                assert np.array_equal(gpu.dib(), want_dc)
    finally:
        gpu.set_log_callback(gpu._log_cb, None)
        for be in (oracle, gpu):
            be.set_preview_mode(1)
            be.set_options()
