"""-m gpu: jsnoop_batch_export_jpeg_coded with JSNOOP_HUFFMAN_OPTIMAL -- k_export_symbols, k_export_huff and the per-entry tables in k_export_measure /
k_export_bits (jsnoop_export.hip) --, jsnoop_batch_export_tables and the Python, job, single-image and C++ wrappers.

Files are compared byte for byte with tests/export_opt_model.py (which tests/test_export_opt_model.py pins on the CPU), fed the ORACLE's numbers where a
file comes from the synthetic encoder and the coefficients it was written from where it comes from tests/export_opt_cases.py or the progressive
catalogue.  jsnoop_batch_export_tables is compared count for count and table for table, so that a failure names the slot and the symbol where the file
bytes only say "differs".  Pictures too large for the sequential model are checked by the round trip."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import export_model as EM
import export_opt_cases as XO
import export_opt_model as OM
import prog_cases as PCS
import prog_codec as PC
from test_gpu_export import LAYOUTS, assert_files, decoded_batch, first_difference, oracle_inputs, same_decode, same_dib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 8, 9, 17, 72]


@pytest.fixture(scope="module")
def oracles(harness):
    full, dc = harness.oracle_backend(), harness.oracle_backend()
    full.set_options(decode_ac=1); dc.set_options(decode_ac=0)
    yield full, dc
    full.close(); dc.close()


def model_of(harness, oracles, data, jfif=True):
    """(result, detail, file, freq, tables) of the model on the oracle's reading of a baseline file."""
    blocks, cum, geo, x, y, qnat = oracle_inputs(harness, oracles, data)
    return OM.export_parts(blocks, cum, geo, x, y, qnat, jfif=jfif)


def assert_tables(b, k, freq, tabs, name):
    """Entry k of the last export against the model: symbol counts first (a wrong count explains a wrong table), then the table."""
    got = b.export_tables(k)
    assert len(got) == len(tabs), (name, len(got), len(tabs))
    for slot, g in enumerate(got):
        want = [freq[slot].get(s, 0) for s in range(256)]
        bad = [s for s in range(256) if g["freq"][s] != want[s]]
        assert not bad, "%s: slot %d, symbol 0x%02X counted %d times, the model has %d (%d symbols differ)" % (name, slot, bad[0], g["freq"][bad[0]], want[bad[0]], len(bad))
        assert g["counts"] == list(tabs[slot][0]), "%s: slot %d, codes per length %s, the model has %s" % (name, slot, g["counts"], tabs[slot][0])
        assert g["symbols"] == list(tabs[slot][1]), "%s: slot %d, symbols in code order %s, the model has %s" % (name, slot, g["symbols"], tabs[slot][1])


def assert_opt(b, got, want, names):
    """Files, result words and tables of a whole export against model results (result, detail, file, freq, tables)."""
    res = b.export_results()
    assert len(got) == len(want) == len(res)
    for k, (g, w, nm) in enumerate(zip(got, want, names)):
        assert (res[k]["result"], res[k]["detail"]) == (w[0], w[1]), nm
        if w[0] == OM.OK:
            assert_tables(b, k, w[3], w[4], nm)
        assert g == w[2], "%s: %s" % (nm, first_difference(g, w[2]))
        assert res[k]["len"] == (len(w[2]) if w[2] else 0), nm


# ------------------------------------------------------------------------------------------------ byte for byte: layouts and sizes
@pytest.fixture(scope="module")
def small(harness, oracles):
    """The six layouts x widths 1, 8, 9, 17, 72 (heights the same sizes, dealt round), restart markers in every second source."""
    import jpegsnoop_amd as J
    shapes = [(w, SIZES[(i + s) % 5], s, 2 * ((i + s) % 2)) for s in range(6) for i, w in enumerate(SIZES)]
    files = [harness.synth_jpeg(width=w, height=h, quality=92, restart_interval=dri, seed=1300 + k, **LAYOUTS[s]) for k, (w, h, s, dri) in enumerate(shapes)]
    want = [model_of(harness, oracles, f) for f in files]
    assert all(w[0] == OM.OK for w in want)
    b = decoded_batch(J, files)
    yield J, b, shapes, files, want
    b.close()


def test_every_layout_and_size_byte_for_byte_and_table_for_table(small, harness, oracles):
    J, b, shapes, files, want = small
    got = b.export_jpeg(huffman="optimal")
    assert_opt(b, got, want, ["%dx%d layout %d dri %d" % s for s in shapes])
    annex = b.export_jpeg()
    assert all(len(g) < len(a) for g, a in zip(got, annex)), "on these pictures the built tables save bytes"
    bare = b.export_jpeg(images=[5, 17], jfif=False, huffman="optimal")
    assert bare == [model_of(harness, oracles, files[i], jfif=False)[2] for i in (5, 17)] and bare[0] == got[5][:2] + got[5][20:]


def test_lists_with_repeats_subsets_a_null_list_and_grey_beside_colour(small):
    """Counts are per ENTRY: an image listed twice has two histograms, neither the sum."""
    J, b, shapes, files, want = small
    lib = J.load()
    order = [22, 2, 2, 0, 29, 22, 11, 2]                             # 0 .. 4 are grey, the others colour
    assert {shapes[i][2] for i in order} >= {0, 2, 4, 5}
    got = b.export_jpeg(images=order, huffman="optimal")
    assert_opt(b, got, [want[i] for i in order], ["entry %d (image %d)" % (k, i) for k, i in enumerate(order)])
    assert [e["image"] for e in b.export_results()] == order and len({e["ptr"] for e in b.export_results()}) == len(order)
    spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
    coding = J.capi.export_coding(lib, "optimal")
    assert lib.jsnoop_batch_export_jpeg_coded(b._h, C.byref(spec), C.byref(coding), None, 3) == 0, J.last_error()
    assert [e["image"] for e in b.export_results()] == [0, 1, 2]
    buf = (C.c_uint8 * 65536)()
    n = lib.jsnoop_batch_read_export(b._h, 2, buf, 65536)
    assert bytes(buf[:n]) == want[2][2]
    assert_tables(b, 1, want[1][3], want[1][4], "image 1 of a NULL list")
    assert lib.jsnoop_batch_export_jpeg_coded(b._h, C.byref(spec), C.byref(coding), None, 0) == 0 and lib.jsnoop_batch_export_count(b._h) == 0


def test_mode_0_through_the_new_call_is_the_old_call_and_the_modes_alternate_on_one_batch(small):
    """huffman = 0 equals jsnoop_batch_export_jpeg byte for byte; an Annex K export right after an optimal one and the reverse (regrown scratch, stale tables)."""
    J, b, shapes, files, want = small
    lib = J.load()
    pick = [3, 14, 27, 9]
    old = b.export_jpeg(images=pick)
    spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
    ind = (C.c_int * len(pick))(*pick)

    def coded(mode, coding=None):
        coding = coding or J.capi.export_coding(lib, mode)
        assert lib.jsnoop_batch_export_jpeg_coded(b._h, C.byref(spec), C.byref(coding), ind, len(pick)) == 0, J.last_error()
        out = []
        for k in range(len(pick)):
            n = b.export_results()[k]["len"]; buf = (C.c_uint8 * n)()
            assert lib.jsnoop_batch_read_export(b._h, k, buf, n) == n
            out.append(bytes(buf))
        return out

    opt = [want[i][2] for i in pick]
    assert coded("annex_k") == old
    assert coded("optimal") == opt
    assert coded("annex_k") == old
    assert b.export_jpeg(images=[9, 3, 3, 3, 14, 27, 9, 9], huffman="optimal") == [want[i][2] for i in (9, 3, 3, 3, 14, 27, 9, 9)]      # more entries: the scratch grows
    assert b.export_jpeg(images=pick) == old and coded("optimal") == opt
    short = J.capi.ExportCoding(); short.struct_size = 4; short.huffman = 1                # a shorter struct takes the defaults
    assert coded(None, short) == old
    for size, mode, word in ((12, 1, "struct_size"), (8, 2, "huffman = 2"), (8, -1, "huffman = -1")):
        bad = J.capi.ExportCoding(); bad.struct_size = size; bad.huffman = mode
        assert lib.jsnoop_batch_export_jpeg_coded(b._h, C.byref(spec), C.byref(bad), ind, len(pick)) == -1 and word in J.last_error(), J.last_error()
    assert lib.jsnoop_batch_export_jpeg_coded(b._h, C.byref(spec), None, ind, len(pick)) == -1 and "coding is NULL" in J.last_error()


def test_the_table_accessor_refuses_with_a_text(small):
    J, b, shapes, files, want = small
    lib = J.load()
    cnt = (C.c_uint8 * 16)()
    b.export_jpeg(images=[0, 7], huffman="optimal")                  # image 0 is grey
    assert lib.jsnoop_batch_export_tables(b._h, 0, 1, cnt, None, None, None) == 0 and list(cnt) == list(want[0][4][1][0])      # any output pointer may be NULL
    assert lib.jsnoop_batch_export_tables(b._h, 0, 2, cnt, None, None, None) == -1 and "slot 2" in J.last_error()
    assert lib.jsnoop_batch_export_tables(b._h, 1, 3, None, None, None, None) == 0
    assert lib.jsnoop_batch_export_tables(b._h, 1, 4, None, None, None, None) == -1 and "slot 4" in J.last_error()
    assert lib.jsnoop_batch_export_tables(b._h, 1, -1, None, None, None, None) == -1 and "slot -1" in J.last_error()
    assert lib.jsnoop_batch_export_tables(b._h, 2, 0, None, None, None, None) == -1 and "out of range" in J.last_error()
    b.export_jpeg(images=[0, 7])
    assert lib.jsnoop_batch_export_tables(b._h, 0, 0, None, None, None, None) == -1 and "Annex K" in J.last_error()
    with pytest.raises(ValueError):
        b.export_jpeg(huffman="best")


# ------------------------------------------------------------------------------------------------ the catalogue
CASES = XO.cases()


@pytest.fixture(scope="module")
def content():
    import jpegsnoop_amd as J
    b = decoded_batch(J, [c.file for c in CASES])
    got = b.export_jpeg(huffman="optimal")
    yield J, b, got, b.export_results()
    b.close()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c.name for c in CASES])
def test_catalogue_case_byte_for_byte_and_table_for_table(content, k):
    """tests/export_opt_cases.py: tables of one symbol, ties, every symbol there is, code trees 16, 17, 20 and 22 deep, counts above 2^16, a symbol in the
    last partial tile alone, ZRL (tests/test_export_opt_model.py has each case's census)."""
    J, b, got, res = content
    case = CASES[k]
    _T, freq, tabs, want = case.model()
    assert (res[k]["result"], res[k]["detail"]) == (0, 0)
    assert_tables(b, k, freq, tabs, case.name)
    assert got[k] == want, "%s: %s" % (case.name, first_difference(got[k], want))
    assert res[k]["len"] == len(want)


def test_block_counts_at_the_tile_seams_and_an_mcu_across_the_seam(harness, oracles):
    import jpegsnoop_amd as J
    T = XO.TILE
    counts = (T - 1, T, T + 1, 2 * T + 1)
    noise = [harness.synth_jpeg(width=8 * n, height=8, quality=90, gray=1, seed=1700 + n) for n in counts]
    colour = [harness.synth_jpeg(width=16 * n, height=16, quality=85, hs=2, vs=2, seed=1720 + n) for n in (42, 43)]          # 252 and 258 blocks: an MCU across the tile seam
    want = [model_of(harness, oracles, f) for f in noise + colour]
    b = decoded_batch(J, noise + colour)
    try:
        assert_opt(b, b.export_jpeg(huffman="optimal"), want, ["noise %d" % n for n in counts] + ["4:2:0 42 MCUs", "4:2:0 43 MCUs"])
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ result words
def test_entries_that_are_not_ok_beside_ok_ones(harness, oracles):
    """INEXACT / UNCODABLE / UNSUPPORTED: result and detail as in the Annex K mode, no file, no tables; the OK entries of the call untouched."""
    import jpegsnoop_amd as J
    clean = harness.synth_jpeg(width=40, height=24, seed=11)
    f1 = PC.Frame(64, 8, [(1, 1, 0)], {0: [1] + [30000] * 63}); c1 = f1.zeros(); c1[0][0, 5, 7] = 3; c1[0][0, 2, 7] = 1
    f2 = PC.Frame(48, 8, [(1, 1, 0)], {0: [2] * 64}); c2 = f2.zeros(); c2[0][0, :, 0] = [0, 5, -1500, 1500, 1500, 0]
    at = clean.index(b"\xFF\xC0") + 4
    f3 = clean[:at] + b"\x0c" + clean[at + 1:]
    files = [clean, PC.encode_baseline(f1, c1), clean, PC.encode_baseline(f2, c2, dri=1), f3, clean]
    m1 = OM.export_file(*EM.frame_inputs(f1, c1)[:3], 64, 8, EM.frame_inputs(f1, c1)[3])
    m2 = OM.export_file(*EM.frame_inputs(f2, c2)[:3], 48, 8, EM.frame_inputs(f2, c2)[3])
    assert m1[:2] == (OM.INEXACT, 5) and m2[:2] == (OM.UNCODABLE, 3)
    ok = model_of(harness, oracles, clean)
    b = decoded_batch(J, files)
    try:
        b.export_jpeg()
        annex = [(e["result"], e["detail"]) for e in b.export_results()]
        out = b.export_jpeg(huffman="optimal")
        res = b.export_results()
        assert [(e["result"], e["detail"]) for e in res] == annex == [(0, 0), (1, 5), (0, 0), (2, 3), (3, 0), (0, 0)]
        assert [e["len"] for e in res] == [len(ok[2]), 0, len(ok[2]), 0, 0, len(ok[2])] and [e["ptr"] for e in res if not e["len"]] == [0, 0, 0]
        assert out[1] is None and out[3] is None and out[4] is None
        assert_files([out[0], out[2], out[5]], [ok[2]] * 3, ["clean 0", "clean 2", "clean 5"])
        assert_tables(b, 5, ok[3], ok[4], "clean 5")
        lib = J.load()
        for k in (1, 3, 4):
            assert lib.jsnoop_batch_export_tables(b._h, k, 0, None, None, None, None) == -1 and "not exported" in J.last_error(), k
        assert b.export_jpeg(images=[4, 1], huffman="optimal") == [None, None] and [e["result"] for e in b.export_results()] == [3, 1]
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ round trips
def test_round_trip_of_clean_baseline_and_grey_files(small):
    import torch
    J, b, shapes, files, want = small
    pick = [2, 4, 8, 13, 19, 24, 29]
    assert {shapes[k][3] for k in pick} == {0, 2} and any(shapes[k][2] == 0 for k in pick)
    out = b.export_jpeg(images=pick, huffman="optimal")
    b2 = same_decode(J, torch, b, out, pick)
    try:
        same_dib(b, b2, pick)
        assert b2.export_jpeg(huffman="optimal") == out, "a second generation is the first, byte for byte"
    finally:
        b2.close()


PROG = ["dc_al3_three_refinements_between_ac", "values_every_category_al0"]


def test_round_trip_of_progressive_files_and_the_model_on_their_coefficients():
    import jpegsnoop_amd as J
    import torch
    cases = [PCS.built(n) for n in PROG]
    b = decoded_batch(J, [c.file for c in cases])
    try:
        assert all(b.info(i)["path"] == 3 for i in range(len(cases)))
        out = b.export_jpeg(huffman="optimal")
        want = []
        for c in cases:
            arena, dccum, geo, qnat = EM.frame_inputs(c.frame, c.dec.coefs)
            want.append(OM.export_parts(arena, dccum, geo, c.frame.width, c.frame.height, qnat))
        assert_opt(b, out, want, PROG)
        ok = [i for i in range(len(cases)) if out[i] is not None]
        assert ok
        b2 = same_decode(J, torch, b, [out[i] for i in ok], ok)
        try:
            same_dib(b, b2, ok)
            assert b2.export_jpeg(huffman="optimal") == [out[i] for i in ok]
        finally:
            b2.close()
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ call forms
def test_behind_a_two_stream_decode_before_anything_has_waited(harness, oracles):
    import jpegsnoop_amd as J
    files = [harness.synth_jpeg(width=333, height=217, seed=1040 + k) for k in range(4)]
    want = [model_of(harness, oracles, f)[2] for f in files]
    b = J.JpegBatch()
    try:
        for f in files:
            b.add_jpeg(f)
        b.set_split(2); b.upload()
        assert b.split_parts() == 2
        b.decode()
        lib = J.load(); spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec)); coding = J.capi.export_coding(lib, "optimal")
        assert lib.jsnoop_batch_export_jpeg_coded(b._h, C.byref(spec), C.byref(coding), None, 4) == 0, J.last_error()
        got = []
        for k in range(4):
            n = b.export_results()[k]["len"]; buf = (C.c_uint8 * n)()
            assert lib.jsnoop_batch_read_export(b._h, k, buf, n) == n
            got.append(bytes(buf))
        b.sync()
        assert_files(got, want, ["image %d" % k for k in range(4)])
    finally:
        b.close()


def test_behind_a_dc_only_fast_form_decode(harness, oracles):
    import coef_model as CM
    import jpegsnoop_amd as J
    files = [harness.synth_jpeg(width=100, height=75, hs=2, vs=2, restart_interval=3 * (k % 2), seed=1500 + k) for k in range(3)]
    full, dc = oracles
    want = []
    for f in files:
        p = harness.drive(dc, f); geo = CM.geometry_of(p)
        blocks = harness.oracle_coefs(dc)
        want.append(OM.export_parts(blocks, CM.cum_from_planes(dc.planes(), geo), geo, p.x, p.y, [list(p.dqt[p.comps[c][3]]) for c in range(3)]))
        assert set(want[-1][3][1]) == {0} and set(want[-1][3][3]) == {0}, "DC-only blocks: EOB is the only AC symbol"
    b = decoded_batch(J, files, decode_ac=False)
    try:
        assert b.last_form() == 2
        got = b.export_jpeg(huffman="optimal")
        assert b.last_form() == 1, "behind a fast-form decode the call decodes again in the generic form"
        assert_opt(b, got, want, ["image %d" % k for k in range(3)])
    finally:
        b.close()


def test_export_copy_writes_exactly_len_bytes_into_a_guarded_arena(small):
    import torch
    J, b, shapes, files, want = small
    lib = J.load()
    pick = [28, 1, 16]
    both = b.export_jpeg(images=pick, huffman="optimal")
    res = b.export_results()
    GUARD = 64
    offs, pos = [], GUARD
    for e in res:
        offs.append(pos + 3); pos += e["len"] + 3 + GUARD                          # (odd starts)
    arena = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    expect = np.full(pos, 0xA5, np.uint8)
    torch.cuda.synchronize()
    for k, e in enumerate(res):
        assert lib.jsnoop_batch_export_copy(b._h, k, arena.data_ptr() + offs[k], e["len"] - 1) == -1 and "cap" in J.last_error()
        assert lib.jsnoop_batch_export_copy(b._h, k, arena.data_ptr() + offs[k], e["len"] + 5) == e["len"]
        expect[offs[k]:offs[k] + e["len"]] = np.frombuffer(both[k], np.uint8)
    b.sync()
    assert np.array_equal(arena.cpu().numpy(), expect)
    ts = b.export_jpeg_to_torch(images=pick, huffman="optimal")
    b.export_jpeg(images=[0])
    assert [bytes(t.cpu().numpy()) for t in ts] == both == [want[i][2] for i in pick]


def test_job_single_image_and_cpp_wrappers(harness, oracles, gpu, tmp_path):
    import jpegsnoop_amd as J
    files = [harness.synth_jpeg(width=65, height=33, seed=1021), harness.synth_jpeg(width=17, height=9, gray=1, seed=1022)]
    want = [model_of(harness, oracles, f)[2] for f in files]
    job = J.JpegJob(devices=[0])
    try:
        for f in files:
            job.add(f)
        seen = {}

        def on_file(r):
            seen[r.index] = (r.export_jpeg(huffman="optimal"), r.export_jpeg())
            return False
        assert job.run(on_file)["ok"] == 2
        assert [seen[i][0] for i in range(2)] == want and all(seen[i][1] != seen[i][0] for i in range(2))
    finally:
        job.close()
    # the single-image call
    lib = J.load()
    path = str(tmp_path / "one.jpg")
    harness.drive(gpu, files[0])
    coding = J.capi.export_coding(lib, "optimal")
    assert lib.jsnoop_export_jpeg_coded(gpu.h, path.encode(), C.byref(coding)) == 0, J.last_error()
    assert open(path, "rb").read() == want[0]
    assert lib.jsnoop_export_jpeg_coded(gpu.h, path.encode(), None) == 0 and open(path, "rb").read() == seen[0][1]      # NULL: the defaults
    d = J.CimgDecode()
    try:
        assert d.export_jpeg(path, huffman="optimal") is False           # nothing decoded
    finally:
        d.close()
    # C++: CJPEGsnoopCoreGpu::BatchExportJpeg(files, bJfif, bOptimal) and BatchExportTables
    exe = str(tmp_path / "export_opt_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "export_opt_demo.cpp"),
                           "-L" + os.path.join(ROOT, "jpegsnoop_amd"), "-ljsnoop_gpu", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + os.path.join(ROOT, "jpegsnoop_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    paths = []
    for i, f in enumerate(files):
        p = tmp_path / ("in%d.jpg" % i); p.write_bytes(f); paths.append(str(p))
    out = subprocess.check_output([exe, str(tmp_path)] + paths, text=True).strip().splitlines()
    models = [model_of(harness, oracles, f) for f in files]
    for i in range(2):
        assert open(str(tmp_path / ("out%d.jpg" % i)), "rb").read() == want[i]
        assert [int(x) for x in out[i].split()] == [i] + [len(t[1]) for t in models[i][4]], out[i]


# ------------------------------------------------------------------------------------------------ the deal over many workgroups
def test_one_1080p_and_one_2160p_in_one_call(harness):
    """More tiles than one round of workgroups takes, two sizes in one list: every file decodes (here, and by libjpeg) to what the batch holds, and is
    shorter than its Annex K export."""
    import jpegsnoop_amd as J
    import torch
    from PIL import Image
    files = [harness.synth_jpeg(width=1920, height=1080, hs=2, vs=2, restart_interval=7, seed=1005), harness.synth_jpeg(width=3840, height=2160, hs=2, vs=2, seed=1007)]
    b = decoded_batch(J, files)
    try:
        annex = b.export_jpeg()
        out = b.export_jpeg(huffman="optimal")
        assert all(f[:2] == b"\xFF\xD8" and f[-2:] == b"\xFF\xD9" and len(f) < len(a) for f, a in zip(out, annex))
        tabs = b.export_tables(1)
        assert [sum(t["freq"]) for t in tabs[0::2]] == [240 * 135 * 4, 240 * 135 * 2], "a DC symbol per block"
        assert all(sum(t["counts"]) == len(t["symbols"]) == sum(1 for n in t["freq"] if n) for t in tabs)
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
