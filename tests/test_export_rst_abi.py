"""CPU: the ABI of jsnoop_batch_export_jpeg_rst without a device -- header, exports, binding and wrappers carry the new entry points, the restart spec has
the size the C compiler gives it, the defaults are the documented ones, what needs no device is refused with a text, and JsnoopExportSpec,
JsnoopExportCoding, JsnoopTuning and the ABI version did not move.  The host arithmetic of the restart mode -- spec import and every refusal, the effective
interval of the four modes, side records, interval tables, the worst-case size of a file, the layout, and the scan operator the kernels place blocks with --
runs as a stand-alone host program (tests/cpp/export_rst_check.cpp) under the address and undefined-behaviour sanitizers."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_export_restart_defaults", "jsnoop_batch_export_jpeg_rst", "jsnoop_batch_export_restart", "jsnoop_export_jpeg_rst")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/cpp/export_rst_check.cpp compiled for the host alone, with the sanitizers."""
    exe = tmp_path_factory.mktemp("export_rst_check") / "export_rst_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "export_rst_check.cpp")])
    return str(exe)


def test_header_exports_binding_and_wrappers_carry_the_restart_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    for word in ("#define JSNOOP_RESTART_NONE   0", "#define JSNOOP_RESTART_MCUS   1", "#define JSNOOP_RESTART_ROWS   2", "#define JSNOOP_RESTART_SOURCE 3",
                 "typedef struct JsnoopExportRestart { uint32_t struct_size; int32_t mode; uint32_t interval; uint32_t reserved; } JsnoopExportRestart;",
                 "typedef struct JsnoopExportSpec { uint32_t struct_size; int32_t jfif; } JsnoopExportSpec;",
                 "typedef struct JsnoopExportCoding { uint32_t struct_size; int32_t huffman; } JsnoopExportCoding;"):
        assert word in hdr, word
    full = open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read()
    assert "the DRI in force when the walk ended" in full                # what SOURCE means on a progressive image is stated in the header
    assert (capi.RESTART_NONE, capi.RESTART_MCUS, capi.RESTART_ROWS, capi.RESTART_SOURCE) == (0, 1, 2, 3)
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+BatchExportJpeg\(const std::vector<int>& files = \{\}, bool bJfif = true, bool bOptimal = false\)", wrapper)
    assert re.search(r"bool\s+BatchExportJpegRestart\(const std::vector<int>& files, bool bJfif, bool bOptimal, int nMode, unsigned nInterval\)", wrapper)
    assert re.search(r"bool\s+ExportJpegRestart\(const std::string& strFnameOut, bool bOptimal, int nMode, unsigned nInterval\)", wrapper)
    assert "jsnoop_batch_export_jpeg_rst(m_b," in wrapper and "jsnoop_export_jpeg_rst(m_h," in wrapper and "jsnoop_batch_export_restart(m_b," in wrapper
    import jpegsnoop_amd as J
    for fn in (J.JpegBatch.export_jpeg, J.JpegBatch.export_jpeg_to_torch, J.CimgDecode.export_jpeg):
        p = inspect.signature(fn).parameters
        assert p["restart"].default == 0 and p["huffman"].default == "annex_k", fn
    assert callable(J.JpegBatch.export_restart) and callable(J.JobFileResult.export_jpeg)
    src = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_export.hip")).read()
    assert "k_export_rst_scan" in src and "k_export_stuff_rst" in src and "asm" not in src


def test_struct_size_is_the_c_compilers_and_nothing_else_moved(lib, tmp_path):
    from jpegsnoop_amd import capi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jsnoop_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(JsnoopExportRestart), offsetof(JsnoopExportRestart, mode), offsetof(JsnoopExportRestart, interval),\n'
                   '    offsetof(JsnoopExportRestart, reserved), sizeof(JsnoopExportCoding), sizeof(JsnoopExportSpec), sizeof(JsnoopTuning), JSNOOP_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    R = capi.ExportRestart
    assert got == [C.sizeof(R), R.mode.offset, R.interval.offset, R.reserved.offset, C.sizeof(capi.ExportCoding), C.sizeof(capi.ExportSpec), C.sizeof(capi.Tuning), 1]
    assert got == [16, 4, 8, 12, 8, 8, 56, 1]
    assert lib.jsnoop_abi_version() == 1


def test_defaults_the_helper_and_the_refusals_that_need_no_device(lib):
    from jpegsnoop_amd import capi
    r = capi.ExportRestart()
    C.memset(C.byref(r), 0xEE, C.sizeof(r))
    lib.jsnoop_export_restart_defaults(C.byref(r))
    assert (r.struct_size, r.mode, r.interval, r.reserved) == (16, 0, 0, 0)
    lib.jsnoop_export_restart_defaults(None)                         # (tolerated)
    s = capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(s))
    assert lib.jsnoop_batch_export_jpeg_rst(None, C.byref(s), None, C.byref(r), None, 1) == -1 and b"batch is NULL" in lib.jsnoop_last_error()
    ri, n = C.c_uint32(7), C.c_uint64(9)
    assert lib.jsnoop_batch_export_restart(None, 0, C.byref(ri), C.byref(n)) == -1 and (ri.value, n.value) == (7, 9) and b"batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_export_jpeg_rst(None, b"x", None, C.byref(r)) == -1 and b"bad argument" in lib.jsnoop_last_error()

    def fields(x):
        return x.mode, x.interval, x.reserved

    assert fields(capi.export_restart(lib, 0)) == (0, 0, 0) and fields(capi.export_restart(lib, 120)) == (1, 120, 0)
    assert fields(capi.export_restart(lib, ("rows", 3))) == (2, 3, 0) and fields(capi.export_restart(lib, "source")) == (3, 0, 0)
    assert fields(capi.export_restart(lib, 65536)) == (1, 65536, 0)   # (the library refuses it, with its text)
    for bad in ("rows", ("rows",), ("cols", 1), -1, 1.5, None, True, ("rows", -1)):
        with pytest.raises(ValueError):
            capi.export_restart(lib, bad)


def test_host_arithmetic_and_the_scan_operator_as_a_host_program_under_sanitizers(checker):
    p = subprocess.run([checker], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
