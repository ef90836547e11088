"""-m gpu: jsnoop_batch_export_jpeg_rst -- restart intervals in the exported files, coded on the device: the restart forms of
k_export_measure / k_export_symbols / k_export_bits, k_export_rst_scan, k_export_stuff_rst, and the Python, job, single-image and C++ wrappers.

Byte for byte against tests/export_rst_model.py (pinned on the CPU by tests/test_export_rst_model.py, against libjpeg among others), in both Huffman modes.
Where a file comes from the synthetic encoder the model is fed the ORACLE's numbers; where it is built block by block, the coefficients it was written from."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import export_cases as X
import export_model as EM
import export_rst_model as RM
import fuzz_util as F
import prog_cases as PCS
import prog_codec as PC
from test_gpu_export import DAMAGED, LAYOUTS, assert_files, decoded_batch, first_difference, oracle_inputs, same_decode, same_dib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["annex_k", "optimal"]


@pytest.fixture(scope="module")
def oracles(harness):
    full, dc = harness.oracle_backend(), harness.oracle_backend()
    full.set_options(decode_ac=1); dc.set_options(decode_ac=0)
    yield full, dc
    full.close(); dc.close()


class Source:
    """A file and what the model is fed for it, computed once."""

    def __init__(self, data, inputs):
        self.data = data; self.arena, self.dccum, self.geo, self.x, self.y, self.qnat = inputs
        self.nmcu = self.geo.nblocks // self.geo.bpm
        self._memo = {}

    def model(self, ri, mode="annex_k", jfif=True):
        key = (ri, mode, jfif)
        if key not in self._memo:
            self._memo[key] = RM.export_parts(self.arena, self.dccum, self.geo, self.x, self.y, self.qnat, ri, optimal=mode == "optimal", jfif=jfif)
        return self._memo[key]

    def want(self, ri, mode="annex_k"):
        return self.model(ri, mode)[2]


def synth_source(harness, oracles, **kw):
    data = harness.synth_jpeg(**kw)
    return Source(data, oracle_inputs(harness, oracles, data))


def frame_source(frame, coefs, dri=0):
    arena, dccum, geo, qnat = EM.frame_inputs(frame, coefs)
    return Source(PC.encode_baseline(frame, coefs, dri=dri), (arena, dccum, geo, frame.width, frame.height, qnat))


def grey_blocks(blocks, row=None):
    """A grey picture given block by block ({zig-zag position: level}, position 0 the DC level), multipliers 1, `row` blocks to a block row (default: one row)."""
    n = len(blocks); w = row or n
    assert n % w == 0
    f = PC.Frame(8 * w, 8 * (n // w), [(1, 1, 0)], {0: [1] * 64}); coefs = f.zeros()
    for i, b in enumerate(blocks):
        for z, v in b.items():
            coefs[0][i // w, i % w, z] = v
    return frame_source(f, coefs)


def check(b, sources, restart, ris, names=None, modes=MODES, images=None):
    """One call per Huffman mode: every entry the model's file for its Ri, the result words and what export_restart reports."""
    images = list(range(len(sources))) if images is None else images
    for mode in modes:
        got = b.export_jpeg(images=images, huffman=mode, restart=restart)
        want = [sources[i].model(ri, mode) for i, ri in zip(images, ris)]
        assert_files(got, [w[2] for w in want], ["%s %s Ri %d" % (names[k] if names else "entry %d" % k, mode, ris[k]) for k in range(len(images))])
        res = b.export_results()
        assert [(e["result"], e["detail"]) for e in res] == [(w[0], w[1]) for w in want]
        assert [b.export_restart(k) for k in range(len(images))] == [(ri, RM.intervals(sources[i].geo, ri) if w[2] is not None else 0) for (i, ri), w in zip(zip(images, ris), want)]


# ------------------------------------------------------------------------------------------------ layouts, sizes, intervals
SIZES = [(1, 1), (17, 9), (72, 40)]


@pytest.fixture(scope="module")
def grid(harness, oracles):
    import jpegsnoop_amd as J
    shapes = [(w, h, s) for s in range(6) for (w, h) in SIZES]
    src = [synth_source(harness, oracles, width=w, height=h, quality=92, restart_interval=(0, 3)[k % 2], seed=1300 + k, **LAYOUTS[s]) for k, (w, h, s) in enumerate(shapes)]
    b = decoded_batch(J, [s.data for s in src])
    yield J, b, shapes, src
    b.close()


def test_every_layout_and_size_with_intervals_of_1_2_and_a_row_in_one_call_each(grid):
    """ROWS 1 over eighteen pictures of three widths and six layouts is a list that mixes effective intervals."""
    J, b, shapes, src = grid
    names = ["%dx%d layout %d" % s for s in shapes]
    check(b, src, 1, [1] * len(src), names)
    check(b, src, 2, [2] * len(src), names)
    rows = [s.geo.mcu_x for s in src]
    assert len(set(rows)) >= 4
    check(b, src, ("rows", 1), rows, names)


@pytest.mark.parametrize("which", ["nmcu-1", "nmcu", "nmcu+1"])
def test_every_layout_and_size_with_the_last_interval_one_mcu_none_and_all(grid, which):
    J, b, shapes, src = grid
    for i, s in enumerate(src):
        ri = s.nmcu + {"nmcu-1": -1, "nmcu": 0, "nmcu+1": 1}[which]
        if ri:
            check(b, src, ri, [ri], ["%dx%d layout %d" % shapes[i]], images=[i])


def test_none_through_the_new_call_is_the_coded_call_and_source_is_the_sources_interval(grid):
    J, b, shapes, src = grid
    lib = J.load()
    spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
    for mode in MODES:
        old = b.export_jpeg(huffman=mode)
        rst = J.capi.export_restart(lib, 0)
        assert lib.jsnoop_batch_export_jpeg_rst(b._h, C.byref(spec), C.byref(J.capi.export_coding(lib, mode)), C.byref(rst), None, len(src)) == 0, J.last_error()
        got = []
        for k in range(len(src)):
            n = b.export_results()[k]["len"]; buf = (C.c_uint8 * n)()
            assert lib.jsnoop_batch_read_export(b._h, k, buf, n) == n
            got.append(bytes(buf))
        assert got == old and all(b.export_restart(k) == (0, 1) for k in range(len(src)))
        assert got == [s.want(0, mode) for s in src]
    # NULL coding and NULL restart: the defaults
    assert lib.jsnoop_batch_export_jpeg_rst(b._h, C.byref(spec), None, None, None, 2) == 0 and b.export_results()[1]["len"] == len(src[1].want(0))
    # SOURCE: every second picture was written with DRI 3, the others with none
    check(b, src, "source", [(0, 3)[k % 2] for k in range(len(src))])
    none = [k for k in range(len(src)) if k % 2 == 0]
    assert b.export_jpeg(images=none, restart="source") == [src[k].want(0) for k in none]          # a call in which no entry has an interval
    assert b.export_jpeg(images=[3], restart="source", jfif=False)[0] == src[3].model(3, "annex_k", jfif=False)[2]


def test_a_pillow_file_exported_with_source_has_the_sources_scan_bytes():
    pytest.importorskip("PIL")
    import jpegsnoop_amd as J
    from test_export_rst_model import pillow_file
    files = [pillow_file(layout, 129, 65, "rows", 1, seed=77 + k) for k, layout in enumerate(("420", "422", "444"))]
    b = decoded_batch(J, files)
    try:
        out = b.export_jpeg(restart="source")
        for k, (f, g) in enumerate(zip(files, out)):
            sc = PC.decode(f).scans[0]; sg = PC.decode(g).scans[0]
            assert sc["dri"] == sg["dri"] == b.export_restart(k)[0] and b.export_restart(k)[1] == len(sc["intervals"]) >= 5
            assert g[sg["start"]:] == f[sc["start"]:], first_difference(g[sg["start"]:], f[sc["start"]:])
        assert b.export_restart(2)[1] == 9                                           # (4:4:4: more than eight intervals)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ tile seams, tiles without a boundary, a scan step
def test_intervals_at_the_tile_seams(harness, oracles):
    import jpegsnoop_amd as J
    T = X.TILE
    counts = (T - 1, T, T + 1, 2 * T + 1)
    src = [synth_source(harness, oracles, width=8 * n, height=8, quality=90, gray=1, seed=1700 + n) for n in counts]
    src.append(synth_source(harness, oracles, width=16 * 86, height=16, quality=85, hs=2, vs=2, seed=1720))       # MCU 42 lies across the tile seam, Ri x 6 = 258
    src.append(synth_source(harness, oracles, width=8 * 4 * T, height=8, quality=90, gray=1, seed=1730))          # one interval over three tiles and a half
    b = decoded_batch(J, [s.data for s in src])
    try:
        for ri in (1, T - 1, T, T + 1):
            check(b, src, ri, [ri] * 4, ["%d blocks" % n for n in counts], images=[0, 1, 2, 3])
        check(b, src, 43, [43], ["4:2:0, 86 MCUs"], images=[4])
        check(b, src, 3 * T + T // 2, [3 * T + T // 2], ["1024 blocks"], images=[5])
    finally:
        b.close()


STEP_SHAPES = [(255, 256), (256, 256), (258, 255)]         # blocks: 255, 256 and 257 tiles (tests/test_gpu_export.py's scan-step pictures)
# (picture, Ri): an interval that ends on the entry's end or on the step seam (block 65536), and one that does neither
STEP_CASES = [(0, 32640), (0, 40000), (1, 32768), (1, 40000), (2, 32768), (2, 40000)]


@pytest.fixture(scope="module")
def step():
    """255, 256 and 257 tiles of blocks that hold a DC level and nothing else (cheap for the sequential model): one tile short of a scan step of
    k_export_rst_scan, exactly one step, and a step with one tile behind it."""
    import jpegsnoop_amd as J
    S, T = X.SCAN, X.TILE
    assert [-(-(w * h) // T) for w, h in STEP_SHAPES] == [S - 1, S, S + 1]
    src = []
    for k, (w, h) in enumerate(STEP_SHAPES):
        f = PC.Frame(8 * w, 8 * h, [(1, 1, 0)], {0: [1] * 64}); coefs = f.zeros()
        coefs[0][..., 0] = np.random.default_rng(5 + k).integers(-300, 301, (h, w))
        src.append(frame_source(f, coefs))
    b = decoded_batch(J, [s.data for s in src])
    yield b, src
    b.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "%d_tiles_ri_%d" % (X.SCAN - 1 + c[0], c[1]))
def test_intervals_one_tile_short_of_on_and_across_a_scan_step_of_tiles(step, case, mode):
    b, src = step
    i, ri = case
    nblk = STEP_SHAPES[i][0] * STEP_SHAPES[i][1]; seam = X.SCAN * X.TILE
    ends = ri in (32640, 32768)
    assert (nblk % ri == 0 or (nblk > seam and seam % ri == 0)) == ends and (ends or (seam % ri and nblk % ri))
    check(b, src, ri, [ri], ["%d blocks" % nblk], modes=[mode], images=[i])


# ------------------------------------------------------------------------------------------------ content
E, N9, N10 = X.EMPTY, {1: 1}, {1: 2}                 # 6, 9 and 10 bits under the Annex K tables (DC level 0 everywhere: a restart changes no length)
PADS = [[E, E, E, E], [E, N9, N9, N9], [E, N9, N9, N10], [E, E, E, N9], [E, E, E, N10], [N9, N9, N9, N10], [E, E, N9, N9], [E, E, N9, N10]]


def content_cases():
    """(name, source, Ri, census) -- the census asserts on the MODEL's Annex K file that the event is where it was meant to be."""
    out = []
    blocks = [blk for iv in PADS + PADS + PADS[:4] for blk in iv]

    def pads(f):
        lens = [sum({0: 6, 1: 9, 2: 10}[b.get(1, 0)] for b in iv) for iv in PADS]
        assert sorted(n % 8 for n in lens) == list(range(8))
        assert all(bytes([0xFF, 0xD0 + (r & 7)]) in f for r in range(19)) and f.count(b"\xFF\xD0") == 3 and f.count(b"\xFF\xD7") == 2      # 20 intervals: D7 -> D0 twice
    out.append(("every_padding_length_and_the_marker_index_wraps_twice", grey_blocks(blocks), 4, pads))
    out.append(("padded_last_byte_of_an_interval_is_ff", grey_blocks([N9, X.ONLY63] * 3), 2, lambda f: f.count(b"\xFF\x00\xFF\xD0") == 1 or pytest.fail("no FF 00 FF D0")))
    out.append(("interval_ends_byte_exact_on_ff", grey_blocks([E, E, E, N9, X.ONLY63] * 3), 5, lambda f: f.count(b"\xFF\x00\xFF\xD1") == 1 or pytest.fail("no FF 00 FF D1")))
    out.append(("longest_block_last_of_an_interval_past_the_window", grey_blocks(X.dc_swing(64)), 2, None))
    out.append(("64_worst_case_blocks_each_an_interval", grey_blocks(X.dc_swing(64)), 1, None))
    return out


CONTENT = content_cases()


@pytest.mark.parametrize("k", range(len(CONTENT)), ids=[c[0] for c in CONTENT])
def test_content_case_byte_for_byte(k):
    import jpegsnoop_amd as J
    name, src, ri, census = CONTENT[k]
    if census:
        census(src.want(ri))
    if name.startswith("longest"):
        T = RM.tokens(RM.levels(src.arena, src.dccum, src.geo, src.qnat, ri)[0], src.geo, ri)
        ends = EM.block_ends([t for t in T if t[0] != 2], EM.ANNEX_K)
        assert ends[1] - ends[0] == 1658 and (ends[1] % 8) and 32 * 3314 > 8 * X.WINDOW
    b = decoded_batch(J, [src.data])
    try:
        check(b, [src], ri, [ri], [name])
    finally:
        b.close()


def test_interval_ends_around_a_stuffing_chunk_one_byte_intervals_filling_chunks_and_a_last_interval_of_one_byte():
    """10927 empty blocks, 6 bits each.  Ri 5460 / 5461 / 5462: the first interval is 4095 / 4096 / 4097 bytes long, so its marker lies at the end of a chunk's
    output, wholly past the chunk's 4096 bytes, and behind the next chunk's first byte.  Ri 1: 10927 one-byte intervals, two chunks full of them (three bytes
    out for every byte in).  Ri 10926: the last interval is one byte long."""
    import jpegsnoop_amd as J
    C_ = X.CHUNK
    src = grey_blocks([E] * 10927, row=1561)                                     # (seven block rows: decode order is raster order)
    assert [-(-(6 * n) // 8) for n in (5460, 5461, 5462)] == [C_ - 1, C_, C_ + 1]
    one = src.want(1)
    assert one.count(b"\x2b\xff") == 10927 and one.endswith(b"\x2b\xff\xd9")          # '00' + '1010' + '11'
    b = decoded_batch(J, [src.data])
    try:
        for ri in (5460, 5461, 5462, 1, 10926):
            check(b, [src], ri, [ri], ["10927 empty blocks"])
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ result words
def test_result_words_a_restart_changes_beside_clean_entries(harness, oracles):
    import jpegsnoop_amd as J
    clean = synth_source(harness, oracles, width=40, height=24, seed=1811)
    # UNCODABLE with a restart only: steps of 2000 under a multiplier of 1 -- block 10 starts an interval with a level of 22000
    f1 = PC.Frame(96, 8, [(1, 1, 0)], {0: [1] * 64}); c1 = f1.zeros(); c1[0][0, :, 0] = [2000 * (i + 1) for i in range(12)]
    # INEXACT with a restart only: a cumulative DC that wrapped int16 under a multiplier of 3 (65538 = 3 x 21846 is held as 2), at the interval start behind the wrap
    f2 = PC.Frame(96, 8, [(1, 1, 0)], {0: [3] + [1] * 63}); c2 = f2.zeros(); c2[0][0, :, 0] = [2000 * (i + 1) for i in range(10)] + [21846, 21847]
    # UNSUPPORTED: the SOF says 12 bits
    at = clean.data.index(b"\xFF\xC0") + 4
    s12 = Source(clean.data[:at] + b"\x0c" + clean.data[at + 1:], (clean.arena, clean.dccum, clean.geo, clean.x, clean.y, clean.qnat))
    s12.model = lambda ri, mode="annex_k", jfif=True: (RM.UNSUPPORTED, 0, None, None, None)
    src = [clean, frame_source(f1, c1), clean, frame_source(f2, c2), s12, clean]
    assert src[1].model(10)[:2] == (RM.UNCODABLE, 10) and src[3].model(10)[:2] == (RM.INEXACT, 10) and src[1].model(0)[0] == src[3].model(0)[0] == src[1].model(12)[0] == RM.OK
    b = decoded_batch(J, [s.data for s in src])
    try:
        check(b, src, 10, [10] * 6)
        res = b.export_results()
        assert [e["result"] for e in res] == [0, 2, 0, 1, 3, 0] and [e["ptr"] for e in res if not e["len"]] == [0, 0, 0]
        check(b, src, 12, [12] * 6)                                                  # one interval: the two are written
        check(b, src, 0, [0] * 6)
        b.export_jpeg(huffman="optimal", restart=10)
        with pytest.raises(RuntimeError):
            b.export_tables(1)                                                       # not OK: no tables
    finally:
        b.close()


def test_an_interval_above_65535_is_unsupported_for_that_entry_alone(harness, oracles):
    import jpegsnoop_amd as J
    src = [synth_source(harness, oracles, width=8, height=24, gray=1, seed=1821), synth_source(harness, oracles, width=16, height=8, gray=1, seed=1822),
           synth_source(harness, oracles, width=8, height=8, gray=1, seed=1823)]
    b = decoded_batch(J, [s.data for s in src])
    try:
        check(b, src, ("rows", 65535), [65535, 131070, 65535])
        assert [e["result"] for e in b.export_results()] == [0, 3, 0] and b.export_restart(1) == (131070, 0)
        assert b.export_jpeg(images=[1], restart=("rows", 65535)) == [None]
    finally:
        b.close()


def test_refusals_name_their_reason_and_launch_nothing(grid):
    J, b, shapes, src = grid
    lib = J.load()
    spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
    before = b.export_jpeg(images=[4, 5], restart=2)

    def refused(word, mode, interval, reserved=0, size=16):
        r = J.capi.ExportRestart(); lib.jsnoop_export_restart_defaults(C.byref(r))
        r.mode, r.interval, r.reserved, r.struct_size = mode, interval, reserved, size
        assert lib.jsnoop_batch_export_jpeg_rst(b._h, C.byref(spec), None, C.byref(r), None, 3) == -1 and word in J.last_error(), (word, J.last_error())

    refused("mode = 4", 4, 0); refused("mode = -1", -1, 0)
    refused("interval = 0", 1, 0); refused("interval = 0", 2, 0); refused("interval = 65536", 1, 65536); refused("interval = 65536", 2, 65536)
    refused("takes none", 0, 1); refused("takes none", 3, 1)
    refused("reserved", 1, 5, reserved=1); refused("reserved", 0, 0, reserved=7)
    refused("struct_size", 1, 5, size=20); refused("struct_size", 1, 5, size=0)
    # nothing was launched, nothing was cleared: the entries of the call before are still there
    assert [e["len"] for e in b.export_results()] == [len(f) for f in before] and b.export_restart(1) == (2, RM.intervals(src[5].geo, 2))
    bad = J.capi.ExportCoding(); lib.jsnoop_export_coding_defaults(C.byref(bad)); bad.huffman = 2
    assert lib.jsnoop_batch_export_jpeg_rst(b._h, C.byref(spec), C.byref(bad), None, None, 3) == -1 and "huffman = 2" in J.last_error()
    assert lib.jsnoop_batch_export_jpeg_rst(b._h, None, None, None, None, 3) == -1 and "spec is NULL" in J.last_error()
    assert lib.jsnoop_batch_export_restart(b._h, 2, None, None) == -1 and "out of range" in J.last_error()
    assert lib.jsnoop_batch_export_restart(b._h, 1, None, None) == 0
    with pytest.raises(RuntimeError):
        b.export_jpeg(restart=70000)
    for bad in ("rows", False, 0.0, None):                                       # no restart value: refused in Python, whichever path it would have taken
        with pytest.raises(ValueError):
            b.export_jpeg(restart=bad)


# ------------------------------------------------------------------------------------------------ round trips, damaged and progressive sources
def test_round_trip_and_a_second_generation_with_the_same_spec(grid):
    import torch
    J, b, shapes, src = grid
    pick = [k for k in range(len(src)) if k % 3 != 0]                            # (not the 1 x 1 pictures)
    for mode in MODES:
        out = b.export_jpeg(images=pick, huffman=mode, restart=("rows", 1))
        assert all(f is not None and b"\xFF\xDD\x00\x04" in f[:900] for f in out)
        b2 = same_decode(J, torch, b, out, pick)
        try:
            same_dib(b, b2, pick)
            assert b2.export_jpeg(huffman=mode, restart=("rows", 1)) == out and b2.export_jpeg(huffman=mode, restart="source") == out
        finally:
            b2.close()


def test_a_damaged_file_behind_sync_with_a_marker_per_mcu_row(harness, oracles):
    """The export is the model's file on the ORACLE's reading of the damaged bytes, and decodes to the coefficient tensors the first batch holds."""
    import jpegsnoop_amd as J
    import torch
    bases = F.bases(harness)
    base, seed = DAMAGED[0]
    hurt = F.mutate(harness, np.random.default_rng(seed), bases[base])[0]
    src = [Source(bases[base], oracle_inputs(harness, oracles, bases[base])), Source(hurt, oracle_inputs(harness, oracles, hurt))]
    b = decoded_batch(J, [s.data for s in src])
    try:
        assert b.info(1)["flags"] != 0
        check(b, src, ("rows", 1), [s.geo.mcu_x for s in src], ["clean", "damaged"])
        out = b.export_jpeg(restart=("rows", 1))
        same_decode(J, torch, b, out).close()
    finally:
        b.close()


def test_a_progressive_file_with_dri_rows_and_source():
    """The model on the coefficients the file was written from (the merged scans); SOURCE is the DRI in force when the header walk ended."""
    import jpegsnoop_amd as J
    import torch
    case = PCS.built("dri_interval_of_one_eobrun_and_dc_refinement_byte")
    arena, dccum, geo, qnat = EM.frame_inputs(case.frame, case.dec.coefs)
    src = [Source(case.file, (arena, dccum, geo, case.frame.width, case.frame.height, qnat))]
    dris = [s["dri"] for s in case.dec.scans]
    assert len(set(dris)) > 1 and dris[-1] != 0
    b = decoded_batch(J, [case.file])
    try:
        assert b.info(0)["path"] == 3
        check(b, src, 3, [3], ["progressive"])
        check(b, src, "source", [dris[-1]], ["progressive, SOURCE"])
        out = b.export_jpeg(restart="source")
        b2 = same_decode(J, torch, b, out)
        try:
            same_dib(b, b2, [0])
        finally:
            b2.close()
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ call forms and wrappers
def test_behind_a_two_stream_decode_a_dc_only_fast_form_decode_and_into_a_guarded_arena(harness, oracles):
    import coef_model as CM
    import jpegsnoop_amd as J
    import torch
    lib = J.load()
    src = [synth_source(harness, oracles, width=333, height=217, seed=1840 + k) for k in range(3)]
    b = J.JpegBatch()
    try:
        for s in src:
            b.add_jpeg(s.data)
        b.set_split(2); b.upload()
        assert b.split_parts() == 2
        b.decode()
        spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
        rst = J.capi.export_restart(lib, ("rows", 2))
        assert lib.jsnoop_batch_export_jpeg_rst(b._h, C.byref(spec), None, C.byref(rst), None, 3) == 0, J.last_error()      # before anything has waited
        res = b.export_results()
        want = [s.want(2 * s.geo.mcu_x) for s in src]
        # export_copy into an arena of 0xA5 with guard bands: exactly len bytes change
        GUARD = 64
        offs, pos = [], GUARD
        for e in res:
            offs.append(pos + 3); pos += e["len"] + 3 + GUARD
        arena = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
        expect = np.full(pos, 0xA5, np.uint8)
        torch.cuda.synchronize()
        for k, e in enumerate(res):
            assert e["len"] == len(want[k])
            assert lib.jsnoop_batch_export_copy(b._h, k, arena.data_ptr() + offs[k], e["len"]) == e["len"]
            expect[offs[k]:offs[k] + e["len"]] = np.frombuffer(want[k], np.uint8)
        b.sync()
        assert np.array_equal(arena.cpu().numpy(), expect)
        ts = b.export_jpeg_to_torch(images=[2, 0], huffman="optimal", restart=7)
        assert [bytes(t.cpu().numpy()) for t in ts] == [src[2].want(7, "optimal"), src[0].want(7, "optimal")]
    finally:
        b.close()
    # a DC-only batch: decoded once more in the generic form, DC-only blocks
    full, dc = oracles
    files = [harness.synth_jpeg(width=100, height=75, hs=2, vs=2, restart_interval=3 * (k % 2), seed=1850 + k) for k in range(2)]
    srcs = []
    for f in files:
        p = harness.drive(dc, f); geo = CM.geometry_of(p)
        srcs.append(Source(f, (harness.oracle_coefs(dc), CM.cum_from_planes(dc.planes(), geo), geo, p.x, p.y, [list(p.dqt[p.comps[c][3]]) for c in range(3)])))
    b = decoded_batch(J, files, decode_ac=False)
    try:
        assert b.last_form() == 2
        check(b, srcs, 5, [5, 5], modes=["annex_k"])
        assert b.last_form() == 1
        check(b, srcs, 5, [5, 5])
    finally:
        b.close()


def test_tables_job_single_image_and_cpp_wrappers(harness, oracles, gpu, tmp_path):
    import jpegsnoop_amd as J
    src = [synth_source(harness, oracles, width=65, height=33, seed=1861), synth_source(harness, oracles, width=17, height=9, gray=1, seed=1862)]
    # export_tables: the counts of the tokens WITH the predictor resets
    b = decoded_batch(J, [s.data for s in src])
    try:
        b.export_jpeg(huffman="optimal", restart=1)
        for k, s in enumerate(src):
            _, _, _, freq, tabs = s.model(1, "optimal")
            plain = s.model(0, "optimal")[3]
            assert freq[0] != plain[0], "the DC counts differ from the export without restart"
            for slot, t in enumerate(b.export_tables(k)):
                assert t["freq"] == [freq[slot].get(sy, 0) for sy in range(256)] and (t["counts"], t["symbols"]) == (list(tabs[slot][0]), list(tabs[slot][1])), (k, slot)
    finally:
        b.close()
    job = J.JpegJob(devices=[0])
    try:
        for s in src:
            job.add(s.data)
        seen = {}

        def on_file(r):
            seen[r.index] = (r.export_jpeg(restart=("rows", 1)), r.export_jpeg(huffman="optimal", restart=3), r.export_jpeg())
            return False
        assert job.run(on_file)["ok"] == 2
        for i, s in enumerate(src):
            assert seen[i] == (s.want(s.geo.mcu_x), s.want(3, "optimal"), s.want(0))
    finally:
        job.close()
    # the single-image calls
    lib = J.load()
    path = str(tmp_path / "one.jpg")
    harness.drive(gpu, src[0].data)
    rst = J.capi.export_restart(lib, ("rows", 1))
    assert lib.jsnoop_export_jpeg_rst(gpu.h, path.encode(), None, C.byref(rst)) == 0, J.last_error()
    assert open(path, "rb").read() == src[0].want(src[0].geo.mcu_x)
    assert lib.jsnoop_export_jpeg_rst(gpu.h, path.encode(), C.byref(J.capi.export_coding(lib, "optimal")), None) == 0 and open(path, "rb").read() == src[0].want(0, "optimal")
    rst.reserved = 1
    assert lib.jsnoop_export_jpeg_rst(gpu.h, path.encode(), None, C.byref(rst)) == -1 and "reserved" in J.last_error()
    d = J.CimgDecode()
    try:
        assert d.export_jpeg(path, restart=4) is False                               # nothing decoded
    finally:
        d.close()
    # C++: CJPEGsnoopCoreGpu::BatchExportJpegRestart and BatchExportRestart
    exe = str(tmp_path / "export_rst_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "export_rst_demo.cpp"),
                           "-L" + os.path.join(ROOT, "jpegsnoop_amd"), "-ljsnoop_gpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "jpegsnoop_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    paths = []
    for i, s in enumerate(src):
        p = tmp_path / ("in%d.jpg" % i); p.write_bytes(s.data); paths.append(str(p))
    out = subprocess.check_output([exe, str(tmp_path), "1", "2", "1"] + paths, text=True).strip().splitlines()
    for i, s in enumerate(src):
        assert open(str(tmp_path / ("out%d.jpg" % i)), "rb").read() == s.want(s.geo.mcu_x, "optimal")
        assert [int(x) for x in out[i].split()] == [i, s.geo.mcu_x, s.geo.mcu_y], out[i]
    assert open(str(tmp_path / "single.jpg"), "rb").read() == src[0].want(src[0].geo.mcu_x, "optimal")     # CimgDecodeGpu::ExportJpegRestart


# ------------------------------------------------------------------------------------------------ the deal over many workgroups
def test_one_1080p_and_one_2160p_with_a_marker_per_mcu_row(harness):
    """More tiles and chunks than one round of workgroups takes, two sizes in one list: every file decodes (here, and by libjpeg) to what the batch holds."""
    import io
    import jpegsnoop_amd as J
    import torch
    from PIL import Image
    files = [harness.synth_jpeg(width=1920, height=1080, seed=1905), harness.synth_jpeg(width=3840, height=2160, restart_interval=7, seed=1907)]
    b = decoded_batch(J, files)
    try:
        for mode in MODES:
            out = b.export_jpeg(huffman=mode, restart=("rows", 1))
            assert [b.export_restart(k) for k in range(2)] == [(120, 68), (240, 135)]
            assert all(f[:2] == b"\xFF\xD8" and f[-2:] == b"\xFF\xD9" for f in out)
            b2 = same_decode(J, torch, b, out)
            try:
                for i in range(2):
                    assert torch.equal(torch.from_numpy(b.dib(i)), torch.from_numpy(b2.dib(i))), i
            finally:
                b2.close()
            im = Image.open(io.BytesIO(out[1])); im.load()
            assert im.size == (3840, 2160)
    finally:
        b.close()
