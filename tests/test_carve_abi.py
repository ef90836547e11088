"""CPU: the ABI of jsnoop_carve_* without a device -- header, exports, binding and C++ wrapper carry the new entry points, the structs have the sizes the C
compiler gives them, the defaults are the documented ones, every refusal that needs no device comes with its text, and neither the ABI version nor
JsnoopTuning moved.  The host side -- spec import, refusals, list sizing for the all-FF blob, the budget check, the walk's record, the parent pass on
hand-made tables -- runs as a stand-alone host program (tests/cpp/carve_check.cpp) under the address and undefined-behaviour sanitizers, and the table it
prints for a blob is tests/carve_model.py's."""
import ctypes as C
import os
import re
import subprocess

import pytest

import carve_cases as CC
import carve_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_carve_create", "jsnoop_carve_destroy", "jsnoop_carve_spec_defaults", "jsnoop_carve_run", "jsnoop_carve_host", "jsnoop_carve_count", "jsnoop_carve_frame",
       "jsnoop_carve_frames", "jsnoop_carve_frames_dev", "jsnoop_carve_lists_dev", "jsnoop_carve_totals", "jsnoop_carve_copy", "jsnoop_job_add_carved")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/cpp/carve_check.cpp compiled for the host alone, with the sanitizers."""
    exe = tmp_path_factory.mktemp("carve_check") / "carve_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "carve_check.cpp")])
    return str(exe)


def test_header_exports_binding_and_wrappers_carry_the_carve_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    for k, word in enumerate(("OK", "NO_SOS", "NO_EOI", "STOPPED", "LIMIT")):
        assert re.search(r"#define JSNOOP_CARVE_%s\s+%d\b" % (word, k), hdr) and getattr(capi, "CARVE_" + word) == k == getattr(M, word)
    for k, word in enumerate(("NOT_A_MARKER", "RST_OUTSIDE_SCAN", "BAD_LENGTH", "UNKNOWN_MARKER"), 1):
        assert re.search(r"#define JSNOOP_CARVE_%s\s+%d\b" % (word, k), hdr) and getattr(capi, "CARVE_" + word) == k == getattr(M, word)
    for k, word in enumerate(("SOI_AGAIN", "DQT", "DHT", "DRI", "AVI1")):
        assert re.search(r"#define JSNOOP_CARVE_SEEN_%s\s+%du" % (word, 1 << k), hdr) and getattr(capi, "CARVE_SEEN_" + word) == 1 << k == getattr(M, word)
    for name, val in (("LANE", capi.CARVE_LANE), ("WAVE", capi.CARVE_WAVE), ("TILE", capi.CARVE_TILE), ("WALK", capi.CARVE_WALK), ("REC_WORDS", capi.CARVE_REC_WORDS)):
        assert int(re.search(r"#define JSNOOP_CARVE_%s\s+(\d+)u" % name, hdr).group(1)) == val, name
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"static bool CarveBlob\(const uint8_t\*", wrapper) and "bool bExtractAll = false" in wrapper and "jsnoop_job_add_carved(j," in wrapper
    import jpegsnoop_amd as J
    for fn in (J.Carve.run, J.Carve.frames, J.Carve.frames_to_torch, J.carve_host, J.JpegJob.add_carved):
        assert callable(fn)
    mk = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "Makefile")).read()
    assert "jsnoop_carve.hip" in mk and "jsnoop_carve.cpp" in mk


def test_struct_sizes_are_the_c_compilers_and_nothing_else_moved(lib, tmp_path):
    from jpegsnoop_amd import capi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jsnoop_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %d %zu %zu\\n", sizeof(JsnoopCarveSpec), offsetof(JsnoopCarveSpec, max_scratch_bytes), sizeof(JsnoopCarveFrame),\n'
                   '    offsetof(JsnoopCarveFrame, seen), offsetof(JsnoopCarveFrame, parent), sizeof(JsnoopTuning), JSNOOP_ABI_VERSION, sizeof(JsnoopExportSpec), sizeof(JsnoopJobFile)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(capi.CarveSpec), capi.CarveSpec.max_scratch_bytes.offset, C.sizeof(capi.CarveFrame), capi.CarveFrame.seen.offset, capi.CarveFrame.parent.offset,
                   C.sizeof(capi.Tuning), 1, C.sizeof(capi.ExportSpec), C.sizeof(capi.JobFile)]
    assert got[:7] == [16, 8, 72, 28, 68, 56, 1]
    assert lib.jsnoop_abi_version() == 1


def test_defaults_and_the_refusals_that_need_no_device(lib):
    from jpegsnoop_amd import capi
    s = capi.CarveSpec()
    C.memset(C.byref(s), 0xEE, C.sizeof(s))
    lib.jsnoop_carve_spec_defaults(C.byref(s))
    assert (s.struct_size, s.max_markers, s.max_scratch_bytes) == (16, 4096, 0)
    lib.jsnoop_carve_spec_defaults(None)                             # (tolerated)
    blob = (C.c_uint8 * 8)(0xFF, 0xD8, 0xFF, 0xD9, 0, 0, 0, 0)
    fr = (capi.CarveFrame * 2)()
    err = lambda: lib.jsnoop_last_error()
    assert lib.jsnoop_carve_run(None, C.byref(s), blob, 8, 0) == -1 and b"carve is NULL" in err()
    assert lib.jsnoop_carve_host(None, blob, 8, fr, 2) == -1 and b"spec is NULL" in err()
    assert lib.jsnoop_carve_host(C.byref(s), None, 8, fr, 2) == -1 and b"blob is NULL" in err()
    assert lib.jsnoop_carve_host(C.byref(s), blob, 1 << 32, fr, 2) == -1 and b"positions are 32 bits" in err()
    assert lib.jsnoop_carve_host(C.byref(s), blob, 8, None, 2) == -1 and b"frames is NULL" in err()
    s.struct_size = 24
    assert lib.jsnoop_carve_host(C.byref(s), blob, 8, fr, 2) == -1 and b"struct_size 24" in err()
    s.struct_size = 8                                                # an older, shorter struct: max_markers only
    assert lib.jsnoop_carve_host(C.byref(s), blob, 8, fr, 2) == 1 and (fr[0].start, fr[0].end, fr[0].status, fr[0].markers, fr[0].parent, fr[0].struct_size) == (0, 4, M.NO_SOS, 2, -1, 72)
    assert lib.jsnoop_carve_host(C.byref(s), None, 0, None, 0) == 0
    assert lib.jsnoop_carve_count(None) == 0 and lib.jsnoop_carve_frames_dev(None) is None
    assert lib.jsnoop_carve_frame(None, 0, fr) == -1 and lib.jsnoop_carve_frames(None, fr, 2) == -1 and lib.jsnoop_carve_totals(None, None, None) == -1
    assert lib.jsnoop_carve_lists_dev(None, None, None) == -1 and lib.jsnoop_carve_copy(None, 0, None, 0) == -1 and b"carve is NULL" in err()
    assert lib.jsnoop_job_add_carved(None, blob, 8, fr, 1, 0, None) == -1 and b"null argument" in err()
    lib.jsnoop_carve_destroy(None)                                   # (tolerated)


def test_without_a_device_a_carve_cannot_be_created(lib):
    import torch
    if torch.cuda.is_available():
        h = lib.jsnoop_carve_create(0)
        assert h
        assert lib.jsnoop_carve_create(4096) is None and b"not available" in lib.jsnoop_last_error()
        lib.jsnoop_carve_destroy(h)
    else:
        assert lib.jsnoop_carve_create(0) is None and b"no CPU fallback" in lib.jsnoop_last_error()


def test_host_side_as_a_host_program_under_sanitizers(checker):
    p = subprocess.run([checker], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_the_checkers_table_is_the_models(checker, harness):
    cases = CC.build_all(harness)
    picks = [c for c in cases if len(c.blob) < 3000] + [None]
    for c in picks:
        blob, mm = (c.blob, c.max_markers or M.MAX_MARKERS) if c else (CC.random_blobs()[7], CC.RANDOM_MAX_MARKERS)
        if not blob:
            continue
        out = subprocess.check_output([checker, "table", blob.hex(), str(mm)]).decode().splitlines()
        want = M.table(blob, mm)
        assert [[int(x) for x in l.split()] for l in out[:-1]] == [[f[k] for k in M.FIELDS] for f in want], c.name if c else "random"
        assert [int(x) for x in out[-1].split()[1:]] == M.lists(blob)[0]
