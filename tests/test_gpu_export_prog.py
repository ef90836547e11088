"""-m gpu: jsnoop_batch_export_jpeg_prog -- progressive (SOF2) files along a scan script, coded on the device: k_prog_classify,
k_prog_runs (end-of-band runs resolved by two segmented scans across tiles), the one walk with its three sinks, k_prog_huff, k_prog_bits, k_prog_place,
k_prog_stuff, and the Python wrappers.

Byte for byte against tests/export_prog_model.py (pinned on the CPU by tests/test_export_prog_model.py, against prog_codec and libjpeg).  Where a file
comes from the synthetic encoder the model is fed the ORACLE's numbers; where it is built block by block, the coefficients it was written from."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import export_prog_model as PM
import prog_codec as PC
from test_export_model import random_frame
from test_export_prog_model import BIG, BIG2, RESTARTS, eob_census, every_index, scripts_for
from test_gpu_export import LAYOUTS, assert_files, decoded_batch
from test_gpu_export_rst import frame_source, grey_blocks, synth_source

pytestmark = pytest.mark.gpu
TILE = 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = {"ri0": 0, "ri1": 1, "ri3": 3, "row": ("rows", 1)}               # RESTARTS of the model test as the wrappers take them


@pytest.fixture(scope="module")
def oracles(harness):
    full, dc = harness.oracle_backend(), harness.oracle_backend()
    full.set_options(decode_ac=1); dc.set_options(decode_ac=0)
    yield full, dc
    full.close(); dc.close()


def model(src, script, restart=(PM.NONE, 0), source_ri=0, memo={}):
    key = (id(src), repr(script), restart, source_ri)
    if key not in memo:
        memo[key] = (src, PM.export_parts(src.arena, src.dccum, src.geo, src.x, src.y, src.qnat, script, restart, source_ri))
    return memo[key][1]


def script_of(src, script):
    """The script an entry is judged by: True is the built-in one for its component count."""
    return PM.DEFAULT[src.geo.ncomp] if script is True else script


def check(b, sources, script, restart="ri0", names=None, images=None, source_ri=None):
    """One call: every entry the model's file, its result words, and what export_scans / export_restart report of it."""
    images = list(range(len(sources))) if images is None else images
    got = b.export_jpeg(images=images, progressive=script, restart=API.get(restart, restart))
    rs = (PM.ROWS, restart[1]) if isinstance(restart, tuple) else RESTARTS.get(restart, (PM.SOURCE, 0))
    want = [model(sources[i], script_of(sources[i], script), rs, source_ri[k] if source_ri else 0) for k, i in enumerate(images)]
    assert_files(got, [w[2] for w in want], ["%s, restart %s" % (names[k] if names else "entry %d" % k, restart) for k in range(len(images))])
    assert [(e["result"], e["detail"]) for e in b.export_results()] == [(w[0], w[1]) for w in want]
    for k, w in enumerate(want):
        scans = b.export_scans(k)
        if w[2] is None:
            assert scans == [] and b.export_restart(k) == (0, 0)
            continue
        keys = ("comps", "ss", "se", "ah", "al", "ri", "intervals", "sos_offset")
        assert [{x: s[x] for x in keys} for s in scans] == [{x: s[x] for x in keys} for s in w[3]]
        assert [s["data_bytes"] for s in scans] == [len(s["ecs"]) for s in w[3]]
        assert b.export_restart(k) == (w[3][0]["ri"], w[3][0]["intervals"])
    return got, want


# ------------------------------------------------------------------------------------------------ layouts, sizes, scripts, intervals
SIZES = [(1, 1), (17, 9), (72, 40)]
NAMES = ["grey", "444", "422", "420", "440", "411"]                   # LAYOUTS of test_gpu_export, in test_export_model's names


@pytest.fixture(scope="module")
def grid(harness, oracles):
    """Eighteen pictures from the synthetic encoder (the oracle's numbers) and eighteen written block by block (sparse blocks of every category, values
    outside the coded part of the padded grid)."""
    import jpegsnoop_amd as J
    shapes = [(w, h, s) for s in range(6) for (w, h) in SIZES]
    src = [synth_source(harness, oracles, width=w, height=h, quality=92, restart_interval=(0, 3)[k % 2], seed=1700 + k, **LAYOUTS[s]) for k, (w, h, s) in enumerate(shapes)]
    src += [frame_source(*random_frame(NAMES[s], w, h, seed=40 + k)) for k, (w, h, s) in enumerate(shapes)]
    b = decoded_batch(J, [s.data for s in src])
    yield J, b, ["%dx%d layout %d" % s for s in shapes] * 2, src
    b.close()


@pytest.mark.parametrize("restart", list(API))
def test_the_built_in_script_on_every_layout_and_size(grid, restart):
    """ROWS 1 gives the scans of a subsampled picture two different Ri (its MCU row and its luma row; chroma rows are MCU rows), so the built-in script
    changes the interval in force five times; and the list mixes widths."""
    J, b, names, src = grid
    _got, want = check(b, src, True, restart, names)
    assert all(w[0] == PM.OK for w in want)
    if restart == "row":
        assert max(len({s["ri"] for s in w[3]}) for w in want) == 2 and max(w[2].count(b"\xFF\xDD\x00\x04") for w in want) == 5


@pytest.mark.parametrize("restart", list(API))
@pytest.mark.parametrize("name", ["al0", "al2", "percomp"])
def test_scripts_for_three_components_and_for_one_refuse_the_other_kind_of_entry(grid, name, restart):
    J, b, names, src = grid
    for ncomp in (3, 1):
        _got, want = check(b, src, scripts_for(ncomp)[name], restart, names)
        assert [w[0] for w in want] == [PM.OK if s.geo.ncomp == ncomp else PM.UNSUPPORTED for s in src]


def test_a_call_in_which_no_entry_fits_the_script_writes_nothing_and_says_so(grid):
    J, b, names, src = grid
    _got, want = check(b, src, scripts_for(3)["al0"], "ri3", images=[0, 1, 2, 18])
    assert [w[0] for w in want] == [PM.UNSUPPORTED] * 4 and b.export_scans(0) == []
    with pytest.raises(IndexError):
        b.export_scan_tables(0, 0)
    lib = J.load()
    assert lib.jsnoop_batch_export_scan_tables(b._h, 0, 0, 0, None, None, None, None) == -1 and "was not exported" in J.last_error()


def test_every_ac_index_a_scan_of_its_own_190_scans(grid):
    J, b, names, src = grid
    mine = [i for i, s in enumerate(src) if (s.x, s.y) == (17, 9) and s.geo.ncomp == 3]
    _got, want = check(b, src, every_index(3), "ri3", images=mine)
    assert len(mine) == 10 and all(len(w[3]) == 190 for w in want)


def test_the_mode_off_is_the_restart_call_byte_for_byte(grid):
    J, b, names, src = grid
    lib = J.load()
    spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
    for mode in ("annex_k", "optimal"):
        for restart in (0, 3):
            old = b.export_jpeg(huffman=mode, restart=restart)
            prog = J.capi.export_progressive(lib, False)
            assert lib.jsnoop_batch_export_jpeg_prog(b._h, C.byref(spec), C.byref(J.capi.export_coding(lib, mode)), C.byref(J.capi.export_restart(lib, restart)), C.byref(prog), None, len(src)) == 0, J.last_error()
            got = []
            for k in range(len(src)):
                n = b.export_results()[k]["len"]; buf = (C.c_uint8 * n)()
                assert lib.jsnoop_batch_read_export(b._h, k, buf, n) == n
                got.append(bytes(buf))
                assert b.export_scans(k) == []
            assert got == old


# ------------------------------------------------------------------------------------------------ tile seams
def busy(z=63, v=1):
    return {0: 3, z: v}


def test_scans_of_255_256_257_and_513_units_and_runs_at_the_tile_seams():
    import jpegsnoop_amd as J
    rng = np.random.default_rng(3)
    src = []
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        blocks = [({0: int(rng.integers(-50, 50))} if rng.random() < 0.5 else {0: 1, int(rng.integers(1, 64)): int(rng.integers(1, 900))}) for _ in range(n)]
        src.append(grey_blocks(blocks))
    # a run across a tile seam (250 .. 260), ended by a tail block; a run over three and a half tiles; a tile of nothing but empty blocks between two busy ones
    blocks = [busy() for _ in range(5 * TILE)]
    for i in range(250, 261):
        blocks[i] = {0: 2}
    blocks[261] = {0: 1, 9: -4}
    for i in range(300, 300 + 3 * TILE + TILE // 2):
        blocks[i] = {0: -1}
    src.append(grey_blocks(blocks))
    blocks = [busy(5, -2) for _ in range(3 * TILE)]
    for i in range(TILE, 2 * TILE):
        blocks[i] = {0: 7}
    src.append(grey_blocks(blocks))
    b = decoded_batch(J, [s.data for s in src])
    try:
        for restart in ("ri0", "ri3"):
            _got, want = check(b, src, True, restart)
            assert all(w[0] == PM.OK for w in want)
        census = eob_census(model(src[4], PM.DEFAULT[1])[3][2]["tokens"])
        assert (3, 11) in census and (0, 1) in census and (9, 3 * TILE + TILE // 2) in census
        last = model(src[5], PM.DEFAULT[1])[3]                        # the band 1 .. 5 ends in its level: one run, the empty tile; the band 6 .. 63 is one run over all three
        assert eob_census(last[1]["tokens"]) == [(8, TILE)] and eob_census(last[2]["tokens"]) == [(9, 3 * TILE)]
    finally:
        b.close()


def test_one_component_scans_of_420_pictures_whose_odd_luma_width_cuts_mcus():
    """Luma's coded part is 17 x 15 = 255, 257 x 1, 27 x 19 = 513 and 17 x 16 = 272 blocks: its rows of units end inside an MCU, its tiles inside a row."""
    import jpegsnoop_amd as J
    src = [frame_source(*random_frame("420", w, h, seed=60 + k)) for k, (w, h) in enumerate([(136, 120), (2056, 8), (216, 152), (136, 128)])]
    assert [PM.coded(s.geo, s.x, s.y, 0) for s in src] == [(15, 17), (1, 257), (19, 27), (16, 17)]
    b = decoded_batch(J, [s.data for s in src])
    try:
        for restart in ("ri0", "row", "ri1"):
            check(b, src, True, restart)
        check(b, src, scripts_for(3)["percomp"], "ri3")
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ long runs, scan-step seams
def big_source(dims, edit):
    f = PC.Frame(dims[0] * 8, dims[1] * 8, [(1, 1, 0)], {0: [1] * 64}); coefs = f.zeros()
    flat = coefs[0].reshape(-1, 64)
    flat[:, 63] = 1
    edit(flat)
    return frame_source(f, coefs)


def test_runs_of_32766_32767_32768_and_65535_empty_blocks():
    import jpegsnoop_amd as J
    def hole(n, tail=False):
        def edit(flat):
            flat[1:1 + n] = 0
            if tail:
                flat[0, 63] = 0; flat[0, 7] = 1
        return edit
    src = [big_source(BIG, hole(32766)), big_source(BIG, hole(32767)), big_source(BIG, hole(32768)), big_source(BIG, hole(32766, True)), big_source(BIG2, hole(65535))]
    b = decoded_batch(J, [s.data for s in src])
    try:
        _got, want = check(b, src, True)
        assert [eob_census(w[3][2]["tokens"]) for w in want] == [[(14, 32766)], [(14, 32767)], [(14, 32767), (0, 1)], [(14, 32767)], [(14, 32767), (14, 32767), (0, 1)]]
        _got, want = check(b, src, True, "row", images=[1])          # an interval end inside the run, 128 times
        assert want[0][0] == PM.OK and eob_census(want[0][3][2]["tokens"])[:3] == [(7, 255), (8, 256), (8, 256)]
    finally:
        b.close()


def test_scans_of_255_256_and_257_tiles_with_a_run_across_the_scan_step():
    import jpegsnoop_amd as J
    def edit(flat):
        flat[TILE * TILE - 900:TILE * TILE + 200] = 0                  # across unit 65 536, where the 257th tile of a scan starts (the scan's end in the second picture)
        flat[TILE * 255 - 3:TILE * 255 + 3, 63] = 0; flat[TILE * 255 - 3:TILE * 255 + 3, 2] = -5
    src = [big_source((TILE, n), edit) for n in (255, 256, 257)]
    b = decoded_batch(J, [s.data for s in src])
    try:
        _got, want = check(b, src, True)
        assert [w[0] for w in want] == [PM.OK] * 3 and (10, 1100) in eob_census(want[2][3][2]["tokens"]) and (9, 900) in eob_census(want[1][3][2]["tokens"])
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ content
def test_padding_lengths_scans_of_one_byte_and_ff_in_front_of_the_next_dht():
    """Forty small grey pictures of different content: the census says every padding length occurs at a scan end and at an interval end, that some
    scan is one byte long, and that some scan ends in a stuffed FF directly in front of the next scan's FF C4."""
    import jpegsnoop_amd as J
    rng = np.random.default_rng(12)
    src = []
    for k in range(40):
        n = int(rng.integers(1, 9))
        src.append(grey_blocks([{0: int(rng.integers(-9, 9)), **({int(rng.integers(1, 64)): int(rng.integers(-300, 300)) or 1} if rng.random() < 0.7 else {})} for _ in range(n)]))
    # (the last byte of a scan of DC refinement bits that are all ones is FF whatever the tables)
    src.append(grey_blocks([{0: 3}] * 8)); src.append(grey_blocks([{0: 1}] * 16))
    b = decoded_batch(J, [s.data for s in src])
    try:
        pads = {"ri0": set(), "ri1": set()}; one_byte = ff_c4 = 0
        for restart in pads:
            _got, want = check(b, src, True, restart)
            for w in want:
                for s in w[3]:
                    codes = [PC._codes(t) if t else None for t in s["tables"]]; bits = 0
                    for kind, a, bb in s["tokens"]:
                        if kind == 2:
                            pads[restart].add(-bits % 8); bits = 0
                        else:
                            bits += codes[a][bb][1] if kind == 0 else bb
                    pads[restart].add(-bits % 8)
                    one_byte += len(s["ecs"]) == 1
                ff_c4 += b"\xFF\x00\xFF\xC4" in w[2]
        assert pads["ri0"] == set(range(8)) == pads["ri1"] and one_byte and ff_c4
    finally:
        b.close()


def token_positions(scan):
    """[(token index, bit position inside its interval)] of every EOB14 of a scan of the model."""
    codes = [PC._codes(t) if t else None for t in scan["tables"]]; bits = 0; out = []
    for i, (kind, a, bb) in enumerate(scan["tokens"]):
        if kind == 2:
            bits = 0; continue
        if kind == 0 and bb == 14 << 4:
            out.append((i, bits, codes[a][bb][1] + 14))
        bits += codes[a][bb][1] if kind == 0 else bb
    return out


def test_an_eob14_across_a_word_edge_inside_one_and_behind_the_lds_window():
    """A run of 16 384 blocks and more is an EOB14: a code and 14 extra bits in one group.  Six pictures shift it bit by bit (the census finds it across a
    word edge and inside a word); in the seventh its tile holds 255 blocks of 63 levels in front of it, more bits than the window of JSNOOP_EXPORT_WINDOW
    bytes takes, so the group goes to memory by itself."""
    import jpegsnoop_amd as J
    rng = np.random.default_rng(21)
    def picture(lead, heavy=False):
        def edit(flat):
            flat[:] = 0
            for i in range(lead):
                if heavy:
                    flat[i, 1:] = rng.integers(512, 1024, 63) * rng.choice([-1, 1], 63)
                else:
                    flat[i, 63] = int(rng.integers(1, 1024))
            flat[lead, 7] = 3                                        # the tail block that starts the run
            flat[lead + 1 + 16500:, 63] = 1
        return big_source((TILE, 70), edit)
    def at_the_window_end():
        """102 blocks with every level of the band 6 .. 63 and one with forty put the group's first word into the window's last and its second behind it."""
        def edit(flat):
            r = np.random.default_rng(33)
            flat[:] = 0
            for i in range(102):
                flat[i, 6:] = r.integers(512, 1024, 58) * r.choice([-1, 1], 58)
            flat[102, 6:46] = np.arange(700, 740)
            flat[103, 7] = 3
            flat[104 + 16500:, 63] = 1
        return big_source((TILE, 70), edit)
    src = [picture(m) for m in range(1, 7)] + [picture(TILE - 1, heavy=True), at_the_window_end()]
    b = decoded_batch(J, [s.data for s in src])
    try:
        _got, want = check(b, src, True)
        found = [token_positions(w[3][2])[0] for w in want]
        assert any(pos % 32 + n > 32 for _i, pos, n in found[:6]) and any(pos % 32 + n <= 32 for _i, pos, n in found[:6])
        assert found[6][1] > 8 * J.capi.EXPORT_WINDOW + 32 and [eob_census(w[3][2]["tokens"])[0] for w in want[:7]] == [(14, 16501)] * 7
        assert eob_census(want[7][3][2]["tokens"])[:2] == [(0, 1), (14, 16501)]        # (the block of forty levels ends in zeros: a run of its own in front of the tail block)
        _i, pos, n = found[7]                                        # (the picture's first tile starts at bit 0 of its scan: the window is words 0 .. WINDOW / 4 - 1)
        assert pos // 32 == J.capi.EXPORT_WINDOW // 4 - 1 and pos % 32 + n > 32, (pos, n)
    finally:
        b.close()


def test_the_longest_band_block_63_levels_of_26_bits_in_a_scan_whose_code_tree_needs_length_limiting():
    """One block of 63 levels of category 10 in a band 1 .. 63 whose other symbols have Fibonacci counts above and below its 63: Annex K.2's tree is 24
    deep, Adjust_BITS (Figure K.3) limits it to 16, and the symbol 0x0A gets a 16-bit code -- 63 x (16 + 10) = 1638 bits in one unit, 52 words of the
    window and the top of what a unit's uint16 length holds.  Blocks are filled with one symbol each (runs 0, 2, 6 and 8 divide the band exactly)."""
    import jpegsnoop_amd as J
    import export_opt_model as OM
    counts = [1, 1, 2, 3, 5, 8, 13, 21, 34, 63, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946, 17711, 28657, 46368, 75025, 121393]
    symbols = [(r, s) for r in (0, 2, 6, 8) for s in range(1, 11) if (r, s) != (0, 10)]
    assign = {}
    for i in sorted(range(len(counts)), key=lambda i: -counts[i]):       # the most frequent symbols are the densest ones
        assign[i] = (0, 10) if counts[i] == 63 else symbols[len([v for v in assign.values() if v != (0, 10)])]
    rng = np.random.default_rng(5); blocks = []
    for i, n in enumerate(counts):
        r, size = assign[i]
        while n > 0:
            k = min(63 // (r + 1), n); n -= k
            blk = np.zeros(64, np.int16)
            for j in range(k):
                blk[1 + j * (r + 1) + r] = int(rng.integers(1 << (size - 1), 1 << size)) * int(rng.choice([-1, 1]))
            blocks.append(blk)
    assert len(blocks) == 64 * 81
    f = PC.Frame(8 * 64, 8 * 81, [(1, 1, 0)], {0: [1] * 64}); coefs = f.zeros()
    coefs[0].reshape(-1, 64)[:] = np.array(blocks)
    src = [frame_source(f, coefs)]
    b = decoded_batch(J, [s.data for s in src])
    try:
        for restart in ("ri0", "ri1"):
            _got, want = check(b, src, scripts_for(1)["al0"], restart)
            scan = want[0][3][1]
            codes = PC._codes(scan["tables"][0])
            assert want[0][0] == PM.OK and codes[0x0A][1] == 16 and max(OM.group_codesizes(scan["freq"][0]).values()) > 16
            T = scan["tokens"]                                       # the census: 63 symbols 0x0A in a row, each with its ten value bits
            run = best = 0
            for k in range(0, len(T) - 1):
                if T[k] == (0, 0, 0x0A) and T[k + 1][0] == 1 and T[k + 1][2] == 10:
                    run += 1; best = max(best, run)
                elif T[k][0] != 1:
                    run = 0
            assert best == 63 and best * (codes[0x0A][1] + 10) == 1638
            tabs = b.export_scan_tables(0, 1)
            assert (tabs[0]["counts"], tabs[0]["symbols"]) == (list(scan["tables"][0][0]), list(scan["tables"][0][1]))
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ restart
def test_source_takes_the_recorded_interval_and_an_interval_above_65535_refuses_that_entry_alone(harness, oracles):
    import jpegsnoop_amd as J
    src = [synth_source(harness, oracles, width=72, height=40, quality=90, restart_interval=ri, seed=1800 + ri, hs=2, vs=2) for ri in (0, 2, 5)]
    wide = frame_source(*random_frame("grey", 8 * 300, 16, seed=9))
    b = decoded_batch(J, [s.data for s in src] + [wide.data])
    try:
        check(b, src + [wide], True, "source", source_ri=[0, 2, 5, 0])
        lib = J.load()
        # ROWS 219: 219 x 300 = 65 700 in every scan of the wide picture, 219 x 5 in the others
        got = b.export_jpeg(progressive=True, restart=("rows", 219))
        want = [model(s, PM.DEFAULT[s.geo.ncomp], (PM.ROWS, 219)) for s in src + [wide]]
        assert [w[0] for w in want] == [PM.OK] * 3 + [PM.UNSUPPORTED]
        assert_files(got, [w[2] for w in want], ["entry %d" % k for k in range(4)])
        assert [e["result"] for e in b.export_results()] == [w[0] for w in want] and lib.jsnoop_batch_export_scan_count(b._h, 3) == 0
        # ... and in ONE kind of scan of an entry: 2048 x 16 in 4:2:0 has 128 MCUs and 256 luma blocks a row; ROWS 256 is 32 768 in its interleaved and chroma
        # scans and 65 536 in its luma scans, ROWS 255 is 65 280 there
        long = frame_source(*random_frame("420", 2048, 16, seed=10))
        b2 = decoded_batch(J, [long.data, src[1].data])
        try:
            _got, want = check(b2, [long, src[1]], True, ("rows", 255))
            assert [w[0] for w in want] == [PM.OK, PM.OK] and [s["ri"] for s in want[0][3]] == [32640, 65280, 32640, 32640, 65280, 32640]
            _got, want = check(b2, [long, src[1]], True, ("rows", 256))
            assert [w[0] for w in want] == [PM.UNSUPPORTED, PM.OK]
        finally:
            b2.close()
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ result words, refusals
def test_result_words_beside_clean_entries():
    """What a clean baseline source can hold and a progressive file cannot: a DC level beyond 2047 that stands for itself behind a restart (fine at Al 1),
    and an AC product that wrapped int16 in the decode."""
    import jpegsnoop_amd as J
    f = PC.Frame(32, 24, [(1, 1, 0)], {0: [3] + [2] * 39 + [40] + [2] * 23})
    def pic(edit):
        coefs = f.zeros(); coefs[0][..., 0] = 5; coefs[0][1, 2, 40] = 7
        edit(coefs[0])
        return frame_source(f, coefs)
    def steep_dc(a):
        a[2, 1, 0] = 1500; a[2, 2, 0] = 3000; a[2, 3, 0] = 1500
    def wrapped_ac(a):
        a[1, 3, 40] = 1000                                           # 40 000 is -25 536 as an int16: no multiple of 40
    src = [pic(lambda a: None), pic(steep_dc), pic(wrapped_ac), pic(lambda a: None)]
    b = decoded_batch(J, [s.data for s in src])
    try:
        _got, want = check(b, src, True)
        assert [(w[0], w[1]) for w in want] == [(PM.OK, 0), (PM.OK, 0), (PM.INEXACT, 7), (PM.OK, 0)]
        _got, want = check(b, src, scripts_for(1)["al0"], "ri1")
        assert [(w[0], w[1]) for w in want] == [(PM.OK, 0), (PM.UNCODABLE, 10), (PM.INEXACT, 7), (PM.OK, 0)]
        _got, want = check(b, src, True, "ri1")
        assert [(w[0], w[1]) for w in want] == [(PM.OK, 0), (PM.OK, 0), (PM.INEXACT, 7), (PM.OK, 0)]
    finally:
        b.close()


def test_refusals_name_their_reason_launch_nothing_and_keep_the_previous_export(grid):
    J, b, names, src = grid
    lib = J.load()
    before = b.export_jpeg(images=[2, 4], progressive=True)
    from test_export_prog_model import BROKEN
    for name, script in BROKEN.items():
        if not script:
            continue
        with pytest.raises(RuntimeError):
            b.export_jpeg(progressive=script)
        assert J.last_error().startswith("export_jpeg:"), name
    spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
    def call(p):
        return lib.jsnoop_batch_export_jpeg_prog(b._h, C.byref(spec), None, None, C.byref(p), None, 2)
    p = J.capi.export_progressive(lib, True); p.mode = 3
    assert call(p) == -1 and "mode" in J.last_error()
    p = J.capi.export_progressive(lib, True); p.reserved = 1
    assert call(p) == -1 and "reserved" in J.last_error()
    p = J.capi.export_progressive(lib, PM.DEFAULT[3]); p.mode = J.capi.PROGRESSIVE_DEFAULT
    assert call(p) == -1 and "no script" in J.last_error()
    p = J.capi.export_progressive(lib, PM.DEFAULT[3]); p.nscans = 0
    assert call(p) == -1
    p = J.capi.export_progressive(lib, PM.DEFAULT[3]); p.nscans = 257
    assert call(p) == -1
    p = J.capi.export_progressive(lib, PM.DEFAULT[3]); p.scans = None
    assert call(p) == -1 and "NULL" in J.last_error()
    p = J.capi.export_progressive(lib, PM.DEFAULT[3]); p._scans[1].comps |= 8
    assert call(p) == -1 and "comps" in J.last_error()
    p = J.capi.export_progressive(lib, PM.DEFAULT[3]); p._scans[2].reserved[1] = 1
    assert call(p) == -1 and "reserved" in J.last_error()
    p = J.capi.export_progressive(lib, True); p.struct_size += 8
    assert call(p) == -1 and "struct_size" in J.last_error()
    # the other three specs are judged as in the calls that introduced them: coding.huffman too, though both of its values write the scans' own tables
    coding = J.capi.export_coding(lib, "optimal"); coding.huffman = 2
    p = J.capi.export_progressive(lib, True)
    assert lib.jsnoop_batch_export_jpeg_prog(b._h, C.byref(spec), C.byref(coding), None, C.byref(p), None, 2) == -1 and "huffman = 2" in J.last_error()
    rst = J.capi.export_restart(lib, 3); rst.reserved = 1
    assert lib.jsnoop_batch_export_jpeg_prog(b._h, C.byref(spec), None, C.byref(rst), C.byref(p), None, 2) == -1 and "reserved" in J.last_error()
    assert lib.jsnoop_batch_export_jpeg_prog(b._h, C.byref(spec), None, None, C.byref(p), (C.c_int * 2)(0, 99), 2) == -1 and "out of range" in J.last_error()
    # nothing was cleared: the previous export is still there, scan records included
    res = b.export_results()
    assert [e["image"] for e in res] == [2, 4] and len(b.export_scans(0)) == 4 and len(b.export_scans(1)) == 6
    buf = (C.c_uint8 * res[1]["len"])()
    assert lib.jsnoop_batch_read_export(b._h, 1, buf, res[1]["len"]) == res[1]["len"] and bytes(buf) == before[1]
    # the baseline tables call refuses a progressive entry and names the call to use
    assert lib.jsnoop_batch_export_tables(b._h, 0, 0, None, None, None, None) == -1 and "jsnoop_batch_export_scan_tables" in J.last_error()
    assert b.export_jpeg(images=[2], progressive=True, huffman="optimal") == b.export_jpeg(images=[2], progressive=True, huffman="annex_k")
    assert b.export_jpeg(images=[2, 4], progressive=True) == before


# ------------------------------------------------------------------------------------------------ tables, round trips, wrappers
def test_scan_tables_are_the_models(grid):
    J, b, names, src = grid
    images = [5, 11, 23]
    _got, want = check(b, src, True, "ri3", images=images)
    for k, w in enumerate(want):
        for i, s in enumerate(w[3]):
            tabs = b.export_scan_tables(k, i)
            assert len(tabs) == len([t for t in s["tables"] if t])
            for t, (counts, syms), freq in zip(tabs, s["tables"], s["freq"]):
                assert (t["counts"], t["symbols"]) == (list(counts), list(syms))
                assert {sy: n for sy, n in enumerate(t["freq"]) if n} == freq


def test_round_trip_second_generation_and_the_pixels_of_a_clean_source(grid):
    """The exported files decoded again by this library's progressive path: a second export with the same script is the first byte for byte; where the
    picture fills its MCUs the coefficient tensors and the DIB are the first decode's, elsewhere the pixels inside the SOF dimensions are."""
    import torch
    J, b, names, src = grid
    images = list(range(18))
    for restart in (0, ("rows", 1)):
        first = b.export_jpeg(images=images, progressive=True, restart=restart)
        b2 = decoded_batch(J, first)
        try:
            assert b2.export_jpeg(progressive=True, restart=restart) == first
            whole = [k for k, i in enumerate(images) if src[i].geo.hv[0] == (1, 1)]      # grey and 4:4:4: the coded part is the whole grid
            assert len(whole) == 6
            t1, t2 = b.coefs_to_torch(images=[images[k] for k in whole]), b2.coefs_to_torch(images=whole)
            for a, c in zip(t1, t2):
                assert all(torch.equal(x, y) for x, y in zip(a, c))
            for k in whole:
                assert np.array_equal(b.dib(images[k]), b2.dib(k))
            p1, p2 = b.to_torch(images=images), b2.to_torch()
            for k in range(len(images)):
                assert torch.equal(p1[k], p2[k]), names[k]
        finally:
            b2.close()


def test_to_torch_job_single_image_and_cpp_wrappers(grid, harness, gpu, tmp_path):
    J, b, names, src = grid
    images = [3, 9, 20]
    files = b.export_jpeg(images=images, progressive=True, restart=3)
    tens = b.export_jpeg_to_torch(images=images, progressive=True, restart=3)
    assert [bytes(t.cpu().numpy()) for t in tens] == files
    pair = [src[9], src[1]]
    want = [model(s, PM.DEFAULT[s.geo.ncomp], (PM.ROWS, 1)) for s in pair]
    job = J.JpegJob(devices=[0])
    try:
        for s in pair:
            job.add(s.data)
        seen = {}

        def on_file(r):
            seen[r.index] = r.export_jpeg(progressive=True, restart=("rows", 1))
            return False
        assert job.run(on_file)["ok"] == 2 and [seen[0], seen[1]] == [w[2] for w in want]
    finally:
        job.close()
    lib = J.load()
    path = str(tmp_path / "one.jpg")
    harness.drive(gpu, pair[0].data)
    prog = J.capi.export_progressive(lib, True)
    assert lib.jsnoop_export_jpeg_prog(gpu.h, path.encode(), None, C.byref(J.capi.export_restart(lib, ("rows", 1))), C.byref(prog)) == 0, J.last_error()
    assert open(path, "rb").read() == want[0][2]
    assert lib.jsnoop_export_jpeg_prog(gpu.h, path.encode(), None, None, None) == 0 and open(path, "rb").read() == pair[0].want(0)      # mode off: the baseline file
    d = J.CimgDecode()
    try:
        assert d.export_jpeg(path, progressive=True) is False                         # nothing decoded
    finally:
        d.close()
    exe = str(tmp_path / "export_prog_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "export_prog_demo.cpp"),
                           "-L" + os.path.join(ROOT, "jpegsnoop_amd"), "-ljsnoop_gpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "jpegsnoop_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    paths = []
    for i, s in enumerate(pair):
        p = tmp_path / ("in%d.jpg" % i); p.write_bytes(s.data); paths.append(str(p))
    out = subprocess.check_output([exe, str(tmp_path), "2", "1"] + paths, text=True).strip().splitlines()
    for i, w in enumerate(want):
        assert open(str(tmp_path / ("out%d.jpg" % i)), "rb").read() == w[2]
        assert out[i].split() == [str(i)] + ["%d:%d:%d:%d" % (sum(1 << c for c in s["comps"]), s["ri"], s["ss"], s["sos_offset"]) for s in w[3]], out[i]
    assert open(str(tmp_path / "single.jpg"), "rb").read() == want[0][2]
