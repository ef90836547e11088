"""-m gpu: jsnoop_batch_export_jpeg and the k_export_* kernels (jsnoop_export.hip), the read / copy calls and the Python, job and single-image wrappers --
a decoded batch written back as baseline JPEG files.

Byte for byte against tests/export_model.py, which tests/test_export_model.py pins on the CPU against three decoders.  Where a file comes from the
synthetic encoder the model is fed the ORACLE's numbers (blocks of its Full-IDCT decode, cumulative DC off the planes of its DC-only decode, the
file's own tables); where it comes from tests/export_cases.py or the progressive catalogue, the coefficients it was written from.  The pictures
too large for the sequential model (a 2160p) are checked by the round trip: decoded again, they give the same tensors and the same DIB, on the device."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import coef_model as CM
import export_cases as X
import export_model as EM
import fuzz_util as F
import prog_cases as PCS
import prog_codec as PC

pytestmark = pytest.mark.gpu

# grey, 4:4:4, 4:2:2, 4:2:0, 4:4:0, 4:1:1
LAYOUTS = [dict(gray=1), dict(hs=1, vs=1), dict(hs=2, vs=1), dict(hs=2, vs=2), dict(hs=1, vs=2), dict(hs=4, vs=1)]
DIMS = [1, 8, 9, 16, 17, 24, 72]
DAMAGED = [(0, 81), (1, 77)]                                     # tests/test_gpu_coefs.py's: (base of fuzz_util.bases, seed)


@pytest.fixture(scope="module")
def oracles(harness):
    full, dc = harness.oracle_backend(), harness.oracle_backend()
    full.set_options(decode_ac=1); dc.set_options(decode_ac=0)
    yield full, dc
    full.close(); dc.close()


def oracle_inputs(harness, oracles, data):
    """(arena, dccum, geometry, dim_x, dim_y, multipliers) of a baseline file as the oracle decodes it."""
    full, dc = oracles
    p = harness.drive(dc, data)
    geo = CM.geometry_of(p)
    cum = CM.cum_from_planes(dc.planes(), geo)
    harness.drive(full, data)
    blocks = harness.oracle_coefs(full)
    qnat = [list(p.dqt[p.comps[c][3]]) for c in range(geo.ncomp)]
    return blocks, cum, geo, p.x, p.y, qnat


def model_of(harness, oracles, data, jfif=True):
    blocks, cum, geo, x, y, qnat = oracle_inputs(harness, oracles, data)
    return EM.export_file(blocks, cum, geo, x, y, qnat, jfif=jfif)


def decoded_batch(J, files, **kw):
    b = J.JpegBatch(**kw)
    for f in files:
        b.add_jpeg(f)
    b.upload(); b.decode(); b.sync()
    return b


def first_difference(got, want):
    if got is None or want is None:
        return "got %s, want %s" % ("None" if got is None else "%d bytes" % len(got), "None" if want is None else "%d bytes" % len(want))
    n = min(len(got), len(want))
    k = next((i for i in range(n) if got[i] != want[i]), n)
    return "lengths %d / %d, first difference at byte %d: got %s, want %s" % (len(got), len(want), k, got[k:k + 8].hex(), want[k:k + 8].hex())


def assert_files(got, want, names):
    assert len(got) == len(want)
    for g, w, nm in zip(got, want, names):
        assert g == w, "%s: %s" % (nm, first_difference(g, w))


def same_decode(J, torch, b1, files, images=None):
    """The files decode, in a second batch, to the coefficient tensors (cumulative DC in slot 0) and the DIB that images `images` of b1 hold."""
    images = list(range(len(files))) if images is None else images
    b2 = decoded_batch(J, files)
    try:
        t1, t2 = b1.coefs_to_torch(images=images), b2.coefs_to_torch()
        for k, i in enumerate(images):
            i1, i2 = b1.info(i), b2.info(k)
            assert (i1["dim_x"], i1["dim_y"], i1["ncomp"]) == (i2["dim_x"], i2["dim_y"], i2["ncomp"]), (k, i)
            for c in range(i1["ncomp"]):
                assert torch.equal(t1[k][c], t2[k][c]), "coefficients of entry %d (image %d), component %d" % (k, i, c)
                assert b1.dqt(i, c).tolist() == b2.dqt(k, c).tolist()
        return b2
    except BaseException:
        b2.close()
        raise


def same_dib(b1, b2, images):
    for k, i in enumerate(images):
        assert np.array_equal(b1.dib(i), b2.dib(k)), "DIB of entry %d (image %d)" % (k, i)


# ------------------------------------------------------------------------------------------------ byte for byte: layouts and sizes
def test_the_seam_constants_are_the_ones_the_cases_were_built_for():
    import jpegsnoop_amd as J
    cap = J.capi
    assert (cap.EXPORT_TILE, cap.EXPORT_SCAN, cap.EXPORT_CHUNK, cap.EXPORT_WINDOW) == (X.TILE, X.SCAN, X.CHUNK, X.WINDOW)


@pytest.fixture(scope="module")
def small(harness, oracles):
    """Every layout with every width and every height of DIMS (a sparse crossing: 7 x 7 shapes dealt over the six layouts, every layout with every width),
    restart markers in every second source."""
    import jpegsnoop_amd as J
    shapes = [(w, DIMS[(i + 2 * j) % 7], (i + j) % 6, 2 * ((i + j) % 2)) for i, w in enumerate(DIMS) for j in range(7)]
    assert {(w, s) for w, _, s, _ in shapes} == {(w, s) for w in DIMS for s in range(6)} and {h for _, h, _, _ in shapes} == set(DIMS)
    files = [harness.synth_jpeg(width=w, height=h, quality=92, restart_interval=dri, seed=300 + k, **LAYOUTS[s]) for k, (w, h, s, dri) in enumerate(shapes)]
    b = decoded_batch(J, files)
    yield J, b, shapes, files
    b.close()


def test_every_layout_and_size_byte_for_byte_against_the_model_on_the_oracles_numbers(small, harness, oracles):
    J, b, shapes, files = small
    want = [model_of(harness, oracles, f) for f in files]
    assert all(r == EM.OK for r, _, _ in want)
    got = b.export_jpeg()
    assert_files(got, [f for _, _, f in want], ["%dx%d layout %d dri %d" % s for s in shapes])
    assert [(e["image"], e["result"], e["detail"], e["len"]) for e in b.export_results()] == [(i, 0, 0, len(f)) for i, (_, _, f) in enumerate(want)]
    # without the APP0 segment: the same bytes, 18 fewer
    bare = b.export_jpeg(images=[5, 17], jfif=False)
    assert bare == [model_of(harness, oracles, files[i], jfif=False)[2] for i in (5, 17)] and bare[0] == got[5][:2] + got[5][20:]


def test_lists_with_repeats_subsets_any_order_and_a_null_list(small, harness, oracles):
    J, b, shapes, files = small
    lib = J.load()
    order = [30, 2, 2, 48, 0, 30, 11]
    want = {i: model_of(harness, oracles, files[i])[2] for i in set(order)}
    got = b.export_jpeg(images=order)
    assert_files(got, [want[i] for i in order], ["entry %d" % k for k in range(len(order))])
    assert [e["image"] for e in b.export_results()] == order
    ptrs = [e["ptr"] for e in b.export_results()]
    assert len(set(ptrs)) == len(order), "a repeated image is a file of its own"
    # images == NULL: 0 .. n - 1
    spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
    assert lib.jsnoop_batch_export_jpeg(b._h, C.byref(spec), None, 3) == 0, J.last_error()
    assert lib.jsnoop_batch_export_count(b._h) == 3 and [e["image"] for e in b.export_results()] == [0, 1, 2]
    buf = (C.c_uint8 * 65536)()
    n = lib.jsnoop_batch_read_export(b._h, 2, buf, 65536)
    assert bytes(buf[:n]) == model_of(harness, oracles, files[2])[2]
    # n == 0: nothing, and the entries of the call before are gone
    assert lib.jsnoop_batch_export_jpeg(b._h, C.byref(spec), None, 0) == 0 and lib.jsnoop_batch_export_count(b._h) == 0


def test_refusals_name_their_reason(small):
    J, b, shapes, files = small
    lib = J.load()
    spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
    one = (C.c_int * 1)(3)

    def refused(word, *a):
        assert lib.jsnoop_batch_export_jpeg(*a) == -1 and word in J.last_error(), (word, J.last_error())

    refused("out of range", b._h, C.byref(spec), (C.c_int * 2)(0, len(files)), 2)
    refused("out of range", b._h, C.byref(spec), (C.c_int * 1)(-1), 1)
    refused("without a list", b._h, C.byref(spec), None, len(files) + 1)
    refused("spec is NULL", b._h, None, one, 1)
    refused("n = -1", b._h, C.byref(spec), one, -1)
    bad = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(bad)); bad.struct_size = 12
    refused("struct_size", b._h, C.byref(bad), one, 1)
    fresh = J.JpegBatch()
    try:
        fresh.add_jpeg(files[3])
        refused("not been decoded", fresh._h, C.byref(spec), None, 1)
        fresh.upload()
        refused("not been decoded", fresh._h, C.byref(spec), None, 1)
    finally:
        fresh.close()
    # read / copy: entries out of range, a short cap, NULL destinations
    assert b.export_jpeg(images=[3])[0] is not None
    ln = b.export_results()[0]["len"]
    buf = (C.c_uint8 * ln)()
    assert lib.jsnoop_batch_read_export(b._h, 1, buf, ln) == -1 and "out of range" in J.last_error()
    assert lib.jsnoop_batch_read_export(b._h, 0, buf, ln - 1) == -1 and "cap" in J.last_error()
    assert lib.jsnoop_batch_read_export(b._h, 0, None, ln) == -1 and "NULL" in J.last_error()
    assert lib.jsnoop_batch_export_copy(b._h, 0, None, ln) == -1 and "NULL" in J.last_error()
    assert lib.jsnoop_batch_export_copy(b._h, -1, None, ln) == -1 and "out of range" in J.last_error()
    assert lib.jsnoop_batch_read_export(b._h, 0, buf, ln) == ln
    # clear() and upload() end the validity of the files
    b2 = decoded_batch(J, files[:2])
    try:
        b2.export_jpeg()
        assert lib.jsnoop_batch_export_count(b2._h) == 2
        b2.upload()
        assert lib.jsnoop_batch_export_count(b2._h) == 0
        b2.decode(); b2.export_jpeg(); b2.clear()
        assert lib.jsnoop_batch_export_count(b2._h) == 0 and b2.export_results() == []
    finally:
        b2.close()


# ------------------------------------------------------------------------------------------------ byte for byte: block counts at the kernels' seams
def grey_zero_case(nblocks):
    """A grey picture of exactly nblocks empty blocks (one block row): 6 bits a block."""
    f = PC.Frame(8 * nblocks, 8, [(1, 1, 0)], {0: [1] * 64})
    return f, f.zeros()


def test_block_counts_one_below_on_and_one_above_the_tile_and_the_stuffing_chunk(harness, oracles):
    """Tile (= the run of a k_export_bits workgroup): 255, 256, 257 blocks of noise, and 511, 512, 513.  Stuffing chunk: empty blocks whose stream is 4095, 4096 and
    4097 bytes long (5460, 5461, 5462 blocks of 6 bits).  And a 4:2:0 picture whose MCU lies across the tile seam."""
    import jpegsnoop_amd as J
    T = X.TILE
    noise = [harness.synth_jpeg(width=8 * n, height=8, quality=90, gray=1, seed=700 + n) for n in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1)]
    colour = [harness.synth_jpeg(width=16 * n, height=16, quality=85, hs=2, vs=2, seed=720 + n) for n in (42, 43)]          # 252 and 258 blocks: an MCU across the tile seam
    empties = [grey_zero_case(n) for n in (5460, 5461, 5462)]
    assert [-(-(6 * f.mcu_x) // 8) for f, _ in empties] == [X.CHUNK - 1, X.CHUNK, X.CHUNK + 1]
    files = noise + colour + [PC.encode_baseline(f, c) for f, c in empties]
    want = [model_of(harness, oracles, f)[2] for f in noise + colour]
    for f, c in empties:
        arena, dccum, geo, qnat = EM.frame_inputs(f, c)
        want.append(EM.export_file(arena, dccum, geo, f.width, f.height, qnat)[2])
    b = decoded_batch(J, files)
    try:
        assert_files(b.export_jpeg(), want, ["noise %d" % n for n in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1)] + ["4:2:0 42 MCUs", "4:2:0 43 MCUs", "5460 empty", "5461 empty", "5462 empty"])
    finally:
        b.close()


def test_block_counts_around_a_scan_step_of_tiles(harness, oracles):
    """255, 256 and 257 tiles (grey pictures of 255 x 256, 256 x 256 and 258 x 255 blocks, smooth and coarse so that the sequential model stays quick): the
    64-bit carry of the prefix sum moves on.  (A scan step of stuffing chunks: the content case worst_past_a_scan_step_of_chunks.)"""
    import jpegsnoop_amd as J
    S, T = X.SCAN, X.TILE
    shapes = [(255, 256), (256, 256), (258, 255)]
    assert [-(-(w * h) // T) for w, h in shapes] == [S - 1, S, S + 1]
    files = [harness.synth_jpeg(width=8 * w, height=8 * h, quality=30, gray=1, noise_sigma=4, seed=800 + k) for k, (w, h) in enumerate(shapes)]
    want = [model_of(harness, oracles, f)[2] for f in files]
    b = decoded_batch(J, files)
    try:
        assert_files(b.export_jpeg(), want, ["%d x %d blocks" % s for s in shapes])
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ content seams
CASES = X.cases()


@pytest.fixture(scope="module")
def content():
    import jpegsnoop_amd as J
    b = decoded_batch(J, [c.file for c in CASES])
    got = b.export_jpeg()
    res = b.export_results()
    yield J, b, got, res
    b.close()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c.name for c in CASES])
def test_content_case_byte_for_byte(content, k):
    """tests/export_cases.py: empty blocks sharing words, the longest block alone and past the LDS window, runs of 62, no EOB, blocks ending on byte / word /
    range boundaries, every padding length, FF bytes at the edges of stuffing chunks and as the padded last byte (test_export_model.py has each case's census)."""
    J, b, got, res = content
    case = CASES[k]
    X.check_census(case)
    want = case.model()[4]
    assert got[k] == want, "%s: %s" % (case.name, first_difference(got[k], want))
    assert (res[k]["result"], res[k]["detail"], res[k]["len"]) == (0, 0, len(want))


# ------------------------------------------------------------------------------------------------ round trips
def test_round_trip_of_clean_baseline_files_with_and_without_restart_markers_and_grey(small):
    import torch
    J, b, shapes, files = small
    pick = [k for k in range(len(files)) if k % 3 == 0]
    assert {shapes[k][3] for k in pick} == {0, 2} and any(shapes[k][2] == 0 for k in pick)
    out = b.export_jpeg(images=pick)
    for f in out:
        assert f is not None and b"\xFF\xDD" not in f[:900], "no restart interval is written"
    b2 = same_decode(J, torch, b, out, pick)
    try:
        same_dib(b, b2, pick)
        # a second generation is the first, byte for byte
        assert b2.export_jpeg() == out
    finally:
        b2.close()


PROG = ["dc_al3_three_refinements_between_ac", "successive_approximation_three_and_two_levels", "dri_interval_of_one_eobrun_and_dc_refinement_byte", "values_every_category_al0"]


def test_round_trip_of_progressive_files_and_the_model_on_their_coefficients():
    """Four files of the progressive catalogue: the export is the model's file for the coefficients they were written from (the merged scans), and decodes
    to the same tensors and DIB."""
    import jpegsnoop_amd as J
    import torch
    assert set(PROG) <= set(PCS.NAMES)
    cases = [PCS.built(n) for n in PROG]
    b = decoded_batch(J, [c.file for c in cases])
    try:
        assert all(b.info(i)["path"] == 3 for i in range(len(cases)))
        out = b.export_jpeg()
        res = b.export_results()
        for i, c in enumerate(cases):
            arena, dccum, geo, qnat = EM.frame_inputs(c.frame, c.dec.coefs)
            r, d, want = EM.export_file(arena, dccum, geo, c.frame.width, c.frame.height, qnat)
            assert (res[i]["result"], res[i]["detail"]) == (r, d), c.name
            assert out[i] == want, "%s: %s" % (c.name, first_difference(out[i], want))
        ok = [i for i in range(len(cases)) if out[i] is not None]
        assert len(ok) >= 3
        b2 = same_decode(J, torch, b, [out[i] for i in ok], ok)
        try:
            same_dib(b, b2, ok)
            assert all(b2.info(k)["path"] != 3 for k in range(len(ok)))
        finally:
            b2.close()
    finally:
        b.close()


def test_damaged_files_are_exported_as_repaired(harness, oracles):
    """The two damaged files of test_gpu_coefs.py behind sync(): the export is the model's file on the ORACLE's reading of the damaged bytes (the model calls
    both OK: checked on the CPU), and decodes to the coefficient tensors the first batch holds.  The DIB is not compared."""
    import jpegsnoop_amd as J
    import torch
    bases = F.bases(harness)
    hurt = [F.mutate(harness, np.random.default_rng(seed), bases[base])[0] for base, seed in DAMAGED]
    want = [model_of(harness, oracles, f) for f in hurt]
    assert all(r == EM.OK for r, _, _ in want)
    b = decoded_batch(J, [bases[0], hurt[0], hurt[1], bases[1]])
    try:
        assert b.info(1)["flags"] != 0 and b.info(2)["flags"] != 0
        out = b.export_jpeg(images=[1, 2])
        assert_files(out, [f for _, _, f in want], ["damaged 0", "damaged 1"])
        same_decode(J, torch, b, out, [1, 2]).close()
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ result words
def test_result_words_and_the_other_images_of_the_call_untouched(harness, oracles):
    import jpegsnoop_amd as J
    clean = harness.synth_jpeg(width=40, height=24, seed=11)
    # INEXACT: a 16-bit multiplier whose product wrapped in the decode -- level 3 x 30000 = 90000 -> (int16) 24464, in block 5
    f1 = PC.Frame(64, 8, [(1, 1, 0)], {0: [1] + [30000] * 63}); c1 = f1.zeros(); c1[0][0, 5, 7] = 3; c1[0][0, 2, 7] = 1
    # UNCODABLE: restart intervals of one MCU let the cumulative DC jump by more than 2047 quantiser steps between neighbours (block 3)
    f2 = PC.Frame(48, 8, [(1, 1, 0)], {0: [2] * 64}); c2 = f2.zeros(); c2[0][0, :, 0] = [0, 5, -1500, 1500, 1500, 0]
    # UNSUPPORTED: the SOF says 12 bits
    at = clean.index(b"\xFF\xC0") + 4
    assert clean[at] == 8
    f3 = clean[:at] + b"\x0c" + clean[at + 1:]
    files = [clean, PC.encode_baseline(f1, c1), clean, PC.encode_baseline(f2, c2, dri=1), f3, clean]
    m1 = EM.export_file(*EM.frame_inputs(f1, c1)[:3], 64, 8, EM.frame_inputs(f1, c1)[3])
    m2 = EM.export_file(*EM.frame_inputs(f2, c2)[:3], 48, 8, EM.frame_inputs(f2, c2)[3])
    assert m1[:2] == (EM.INEXACT, 5) and m2[:2] == (EM.UNCODABLE, 3)
    want_clean = model_of(harness, oracles, clean)[2]
    b = decoded_batch(J, files)
    try:
        out = b.export_jpeg()
        res = b.export_results()
        assert [(e["result"], e["detail"], e["len"]) for e in res] == [(0, 0, len(want_clean)), (1, 5, 0), (0, 0, len(want_clean)), (2, 3, 0), (3, 0, 0), (0, 0, len(want_clean))]
        assert [e["ptr"] for e in res if not e["len"]] == [0, 0, 0]
        assert out[1] is None and out[3] is None and out[4] is None
        assert_files([out[0], out[2], out[5]], [want_clean] * 3, ["clean 0", "clean 2", "clean 5"])
        lib = J.load()
        assert lib.jsnoop_batch_read_export(b._h, 1, None, 0) == 0 and lib.jsnoop_batch_export_copy(b._h, 3, None, 0) == 0      # nothing to copy
        # only bad entries in a call
        assert b.export_jpeg(images=[4, 1]) == [None, None] and [e["result"] for e in b.export_results()] == [3, 1]
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ call forms
def test_export_behind_a_two_stream_decode_before_anything_has_waited(harness, oracles):
    import jpegsnoop_amd as J
    files = [harness.synth_jpeg(width=333, height=217, seed=40 + k) for k in range(5)]
    want = [model_of(harness, oracles, f)[2] for f in files]
    b = J.JpegBatch()
    try:
        for f in files:
            b.add_jpeg(f)
        b.set_split(2); b.upload()
        assert b.split_parts() == 2
        b.decode()
        lib = J.load(); spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
        assert lib.jsnoop_batch_export_jpeg(b._h, C.byref(spec), None, 5) == 0, J.last_error()
        got = []
        for k in range(5):
            n = b.export_results()[k]["len"]; buf = (C.c_uint8 * n)()
            assert lib.jsnoop_batch_read_export(b._h, k, buf, n) == n
            got.append(bytes(buf))
        b.sync()
        assert_files(got, want, ["image %d" % k for k in range(5)])
    finally:
        b.close()


def test_dc_only_fast_form_is_decoded_once_more_and_a_dc_only_batch_exports_dc_only_blocks(harness, oracles):
    import jpegsnoop_amd as J
    import torch
    files = [harness.synth_jpeg(width=100, height=75, hs=2, vs=2, restart_interval=3 * (k % 2), seed=500 + k) for k in range(3)]
    full, dc = oracles
    want = []
    for f in files:
        p = harness.drive(dc, f); geo = CM.geometry_of(p)
        blocks = harness.oracle_coefs(dc)
        assert not blocks[:, 1:].any()
        want.append(EM.export_file(blocks, CM.cum_from_planes(dc.planes(), geo), geo, p.x, p.y, [list(p.dqt[p.comps[c][3]]) for c in range(3)])[2])
    b = decoded_batch(J, files, decode_ac=False)
    try:
        assert b.last_form() == 2
        got = b.export_jpeg()
        assert b.last_form() == 1, "behind a fast-form decode the call decodes again in the generic form"
        assert_files(got, want, ["image %d" % k for k in range(3)])
        assert b.export_jpeg() == got and b.last_form() == 1
        same_decode(J, torch, b, got).close()
    finally:
        b.close()


def test_second_export_regrows_the_memory_and_export_copy_writes_exactly_len_bytes(small, harness, oracles):
    import torch
    J, b, shapes, files = small
    lib = J.load()
    b1 = decoded_batch(J, [files[0], harness.synth_jpeg(width=640, height=480, seed=77)])
    try:
        first = b1.export_jpeg(images=[0])
        both = b1.export_jpeg(images=[1, 0, 1])                                     # far larger than the first call's memory
        assert both[1] == first[0] and both[0] == both[2] == model_of(harness, oracles, harness.synth_jpeg(width=640, height=480, seed=77))[2]
        res = b1.export_results()
        # export_copy into an arena of 0xA5 with guard bands: exactly len bytes change
        GUARD = 64
        offs, pos = [], GUARD
        for e in res:
            offs.append(pos + 3); pos += e["len"] + 3 + GUARD                      # (odd starts)
        arena = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
        expect = np.full(pos, 0xA5, np.uint8)
        torch.cuda.synchronize()
        for k, e in enumerate(res):
            assert lib.jsnoop_batch_export_copy(b1._h, k, arena.data_ptr() + offs[k], e["len"] - 1) == -1 and "cap" in J.last_error()
            assert lib.jsnoop_batch_export_copy(b1._h, k, arena.data_ptr() + offs[k], e["len"] + 5) == e["len"]
            expect[offs[k]:offs[k] + e["len"]] = np.frombuffer(both[k], np.uint8)
        b1.sync()
        assert np.array_equal(arena.cpu().numpy(), expect)
        # the torch wrapper: tensors that outlive the next export
        ts = b1.export_jpeg_to_torch(images=[0, 1])
        b1.export_jpeg(images=[0])
        assert [bytes(t.cpu().numpy()) for t in ts] == [both[1], both[0]] and all(t.dtype == torch.uint8 and t.is_cuda for t in ts)
    finally:
        b1.close()


def test_job_and_single_image_wrappers(harness, oracles, gpu, tmp_path):
    import jpegsnoop_amd as J
    files = [harness.synth_jpeg(width=65, height=33, seed=21), harness.synth_jpeg(width=45, height=19, hs=2, vs=1, progressive=1, seed=23),
             harness.synth_jpeg(width=17, height=9, gray=1, seed=22), b"not a jpeg"]
    job = J.JpegJob(devices=[0])
    try:
        for f in files:
            job.add(f)
        seen = {}

        def on_file(r):
            if r.status != "ok":
                with pytest.raises(RuntimeError):
                    r.export_jpeg()
                seen[r.index] = None
                return False
            seen[r.index] = r.export_jpeg()
            return False
        stats = job.run(on_file)
        assert stats["ok"] == 3 and stats["refused"] == 1
        assert seen[0] == model_of(harness, oracles, files[0])[2] and seen[2] == model_of(harness, oracles, files[2])[2] and seen[3] is None
        D = PC.decode(seen[1])
        assert D.sof == 0xC0 and (D.frame.width, D.frame.height) == (45, 19) and np.array_equal(np.concatenate([c.ravel() for c in D.coefs]), np.concatenate([c.ravel() for c in PC.decode(files[1]).coefs]))
    finally:
        job.close()
    # the single-image call, beside jsnoop_export_tiff
    lib = J.load()
    path = str(tmp_path / "one.jpg")
    harness.drive(gpu, files[0])
    assert lib.jsnoop_export_jpeg(gpu.h, path.encode()) == 0, J.last_error()
    assert open(path, "rb").read() == seen[0]
    f2 = PC.Frame(48, 8, [(1, 1, 0)], {0: [2] * 64}); c2 = f2.zeros(); c2[0][0, :, 0] = [0, 0, -1500, 1500, 1500, 0]
    harness.drive(gpu, PC.encode_baseline(f2, c2, dri=1))
    bad = str(tmp_path / "bad.jpg")
    assert lib.jsnoop_export_jpeg(gpu.h, bad.encode()) == -1 and "UNCODABLE" in J.last_error() and "block 3" in J.last_error() and not os.path.exists(bad)
    assert lib.jsnoop_export_jpeg(gpu.h, str(tmp_path / "no" / "dir.jpg").encode()) == -1
    d = J.CimgDecode()
    try:
        assert d.export_jpeg(path) is False                                          # nothing decoded
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ the deal over many workgroups
def test_two_1080p_and_one_2160p_in_one_call(harness):
    """More tiles and chunks than one round of workgroups takes, pictures of two sizes in one list: every file decodes (here, and by libjpeg) to what the batch
    holds -- the coefficient tensors and the DIB, compared on the device."""
    import jpegsnoop_amd as J
    import torch
    from PIL import Image
    files = [harness.synth_jpeg(width=1920, height=1080, seed=5), harness.synth_jpeg(width=1920, height=1080, restart_interval=7, seed=6), harness.synth_jpeg(width=3840, height=2160, seed=7)]
    b = decoded_batch(J, files)
    try:
        out = b.export_jpeg()
        assert all(f is not None and f[:2] == b"\xFF\xD8" and f[-2:] == b"\xFF\xD9" for f in out)
        b2 = same_decode(J, torch, b, out)
        try:
            for i in range(3):
                assert torch.equal(torch.from_numpy(b.dib(i)), torch.from_numpy(b2.dib(i))), i
        finally:
            b2.close()
        im = Image.open(io.BytesIO(out[2])); im.load()
        assert im.size == (3840, 2160)
    finally:
        b.close()
