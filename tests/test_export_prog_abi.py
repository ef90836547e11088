"""CPU: the ABI of jsnoop_batch_export_jpeg_prog without a device -- header, exports, binding and wrappers carry the new entry points, the two new structs have
the sizes the C compiler gives them, the defaults are the documented ones, what needs no device is refused with a text, and the older specs, JsnoopTuning
and the ABI version did not move.  The host arithmetic of the progressive mode -- spec import and every refusal, every rule of a script, the default
scripts, scan records and the unit-to-block map, the run operators, plans, the layout and the worst-case size of a file -- runs as a stand-alone host
program (tests/cpp/export_prog_check.cpp) under the address and undefined-behaviour sanitizers; the header pieces it plans are the model's."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_export_progressive_defaults", "jsnoop_batch_export_jpeg_prog", "jsnoop_batch_export_scan_count", "jsnoop_batch_export_scan_info",
       "jsnoop_batch_export_scan_tables", "jsnoop_export_jpeg_prog")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/cpp/export_prog_check.cpp compiled for the host alone, with the sanitizers."""
    exe = tmp_path_factory.mktemp("export_prog_check") / "export_prog_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "export_prog_check.cpp")])
    return str(exe)


def test_header_exports_binding_and_wrappers_carry_the_progressive_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    for word in ("#define JSNOOP_PROGRESSIVE_OFF     0", "#define JSNOOP_PROGRESSIVE_DEFAULT 1", "#define JSNOOP_PROGRESSIVE_SCRIPT  2", "#define JSNOOP_EXPORT_MAX_SCANS    256u",
                 "typedef struct JsnoopExportScan { uint8_t comps , ss, se, ah, al, reserved[3]; } JsnoopExportScan;",
                 "typedef struct JsnoopExportProgressive { uint32_t struct_size; int32_t mode; uint32_t nscans; uint32_t reserved; const JsnoopExportScan* scans; } JsnoopExportProgressive;",
                 "typedef struct JsnoopExportRestart { uint32_t struct_size; int32_t mode; uint32_t interval; uint32_t reserved; } JsnoopExportRestart;",
                 "typedef struct JsnoopExportCoding { uint32_t struct_size; int32_t huffman; } JsnoopExportCoding;"):
        assert word in hdr, word
    full = open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read()
    assert "BOTH values write own tables in a progressive mode, because Annex K has no codes for the end-of-band runs" in full
    assert (capi.PROGRESSIVE_OFF, capi.PROGRESSIVE_DEFAULT, capi.PROGRESSIVE_SCRIPT, capi.EXPORT_MAX_SCANS) == (0, 1, 2, 256)
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+BatchExportJpegProgressive\(const std::vector<int>& files, bool bJfif, int nMode, unsigned nInterval, const std::vector<JsnoopExportScan>& scans = \{\}\)", wrapper)
    assert re.search(r"bool\s+ExportJpegProgressive\(const std::string& strFnameOut, int nMode, unsigned nInterval, const std::vector<JsnoopExportScan>& scans = \{\}\)", wrapper)
    assert "jsnoop_batch_export_jpeg_prog(m_b," in wrapper and "jsnoop_export_jpeg_prog(m_h," in wrapper and "jsnoop_batch_export_scan_info(m_b," in wrapper
    import jpegsnoop_amd as J
    for fn in (J.JpegBatch.export_jpeg, J.JpegBatch.export_jpeg_to_torch, J.CimgDecode.export_jpeg):
        p = inspect.signature(fn).parameters
        assert p["progressive"].default is False and p["restart"].default == 0 and p["huffman"].default == "annex_k", fn
    assert callable(J.JpegBatch.export_scans) and callable(J.JpegBatch.export_scan_tables) and callable(J.JobFileResult.export_jpeg)
    src = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_export_prog.hip")).read()
    assert "k_prog_runs" in src and "js_run_fwd_combine" in src and "js_run_bwd_combine" in src and "asm" not in src
    assert "jsnoop_export_prog.hip" in open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "Makefile")).read()


def test_struct_sizes_are_the_c_compilers_and_nothing_else_moved(lib, tmp_path):
    from jpegsnoop_amd import capi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jsnoop_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(JsnoopExportScan), offsetof(JsnoopExportScan, al), offsetof(JsnoopExportScan, reserved),\n'
                   '    sizeof(JsnoopExportProgressive), offsetof(JsnoopExportProgressive, mode), offsetof(JsnoopExportProgressive, nscans), offsetof(JsnoopExportProgressive, reserved),\n'
                   '    offsetof(JsnoopExportProgressive, scans), sizeof(JsnoopExportRestart), sizeof(JsnoopExportCoding), sizeof(JsnoopExportSpec), sizeof(JsnoopTuning), JSNOOP_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    S, P = capi.ExportScan, capi.ExportProgressive
    assert got == [C.sizeof(S), S.al.offset, S.reserved.offset, C.sizeof(P), P.mode.offset, P.nscans.offset, P.reserved.offset, P.scans.offset,
                   C.sizeof(capi.ExportRestart), C.sizeof(capi.ExportCoding), C.sizeof(capi.ExportSpec), C.sizeof(capi.Tuning), 1]
    assert got == [8, 4, 5, 24, 4, 8, 12, 16, 16, 8, 8, 56, 1]
    assert lib.jsnoop_abi_version() == 1


def test_defaults_the_helper_and_the_refusals_that_need_no_device(lib):
    from jpegsnoop_amd import capi
    p = capi.ExportProgressive()
    C.memset(C.byref(p), 0xEE, C.sizeof(p))
    lib.jsnoop_export_progressive_defaults(C.byref(p))
    assert (p.struct_size, p.mode, p.nscans, p.reserved, bool(p.scans)) == (24, 0, 0, 0, False)
    lib.jsnoop_export_progressive_defaults(None)                     # (tolerated)
    s = capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(s))
    assert lib.jsnoop_batch_export_jpeg_prog(None, C.byref(s), None, None, C.byref(p), None, 1) == -1 and b"batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_batch_export_scan_count(None, 0) == 0
    assert lib.jsnoop_batch_export_scan_info(None, 0, 0, None, None, None, None, None) == -1 and b"batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_batch_export_scan_tables(None, 0, 0, 0, None, None, None, None) == -1 and b"batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_export_jpeg_prog(None, b"x", None, None, C.byref(p)) == -1 and b"bad argument" in lib.jsnoop_last_error()
    assert capi.export_progressive(lib, False).mode == 0 and capi.export_progressive(lib, True).mode == 1
    q = capi.export_progressive(lib, [((0, 1, 2), 0, 0, 0, 1), (0, 1, 5, 0, 0), ([2], 1, 63, 0, 0)])
    assert (q.mode, q.nscans) == (2, 3) and [(x.comps, x.ss, x.se, x.ah, x.al) for x in q._scans] == [(7, 0, 0, 0, 1), (1, 1, 5, 0, 0), (4, 1, 63, 0, 0)]
    assert capi.export_progressive(lib, []).nscans == 0                                 # (the library refuses it, with its text)
    for bad in (1, "default", [(0, 1, 5)], [((9,), 0, 0, 0, 0)], [(None, 0, 0, 0, 0)], [((0,), 1, 319, 0, 0)], [((0,), 0, 0, 0, 256)], [((0,), -1, 0, 0, 0)], [((0,), 0, 0, 1.0, 0)]):
        with pytest.raises(ValueError):
            capi.export_progressive(lib, bad)


def test_host_arithmetic_and_the_run_operators_as_a_host_program_under_sanitizers(checker):
    p = subprocess.run([checker], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_the_header_pieces_the_host_plans_are_the_models(checker):
    """A 333 x 217 4:2:0 picture, multipliers 3 + 2 c, the built-in script with ROWS 1: the bytes up to SOF2 and every scan's DRI / SOS."""
    import coef_model as CM
    import export_prog_model as PM
    lines = subprocess.check_output([checker, "headers"], text=True).strip().splitlines()
    geo = CM.Geometry([(2, 2), (1, 1), (1, 1)], 21, 14)
    qnat = [[3 + 2 * c] * 64 for c in range(3)]
    res, _, data, scans = PM.export_parts(np.zeros((geo.nblocks, 64), np.int16), np.zeros(geo.nblocks, np.int16), geo, 333, 217, qnat, PM.DEFAULT[3], (PM.ROWS, 1))
    assert res == PM.OK and bytes.fromhex(lines[0]) == PM.head(geo, 333, 217, qnat) == data[:len(bytes.fromhex(lines[0]))]
    in_force = 0
    for line, s in zip(lines[1:], scans):
        post, nunits, ri, ni = line.split()
        dri = 6 if s["ri"] != in_force else 0; in_force = s["ri"]
        sos = s["sos_offset"]; n = 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
        assert bytes.fromhex(post) == data[sos - dri:sos + n] and (dri == 0 or data[sos - 6:sos - 2] == b"\xFF\xDD\x00\x04")
        units, row = PM.scan_units(geo, 333, 217, s["comps"])
        assert (int(nunits), int(ni)) == (sum(len(u) for u in units), s["intervals"]) and int(ri) == s["ri"] * len(units[0])
    assert len(lines) == 7
