"""CPU: the ABI of jsnoop_batch_export_jpeg_coded without a device -- header, exports, binding and wrappers carry the new entry points, the coding spec
has the size the C compiler gives it, the defaults are the documented ones, a NULL batch is refused with a text, and JsnoopExportSpec, JsnoopTuning and the
ABI version did not move.  The host arithmetic of the optimal mode -- coding-spec import and refusals, the 2^26-block refusal, the side records, the layout
with returned header lengths, the split of the header -- runs as a stand-alone host program (tests/cpp/export_opt_check.cpp) under the address and
undefined-behaviour sanitizers.  (What jsnoop_batch_export_tables refuses needs a decoded batch: tests/test_gpu_export_opt.py.)"""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_export_coding_defaults", "jsnoop_batch_export_jpeg_coded", "jsnoop_batch_export_tables", "jsnoop_export_jpeg_coded")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/cpp/export_opt_check.cpp compiled for the host alone, with the sanitizers."""
    exe = tmp_path_factory.mktemp("export_opt_check") / "export_opt_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "export_opt_check.cpp")])
    return str(exe)


def test_header_exports_binding_and_wrappers_carry_the_coded_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    for word in ("#define JSNOOP_HUFFMAN_ANNEX_K 0", "#define JSNOOP_HUFFMAN_OPTIMAL 1", "typedef struct JsnoopExportCoding { uint32_t struct_size; int32_t huffman; } JsnoopExportCoding;"):
        assert word in hdr, word
    assert (capi.HUFFMAN_ANNEX_K, capi.HUFFMAN_OPTIMAL) == (0, 1) and capi.HUFFMAN_MODES == {"annex_k": 0, "optimal": 1}
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+BatchExportJpeg\(const std::vector<int>& files = \{\}, bool bJfif = true, bool bOptimal = false\)", wrapper)
    assert "jsnoop_batch_export_jpeg_coded(m_b," in wrapper and "jsnoop_batch_export_tables(m_b," in wrapper
    import jpegsnoop_amd as J
    for fn in (J.JpegBatch.export_jpeg, J.JpegBatch.export_jpeg_to_torch, J.CimgDecode.export_jpeg):
        assert inspect.signature(fn).parameters["huffman"].default == "annex_k", fn
    assert callable(J.JpegBatch.export_tables) and callable(J.JobFileResult.export_jpeg)
    src = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_export.hip")).read()
    assert "k_export_symbols" in src and "k_export_huff" in src and "asm" not in src


def test_struct_size_is_the_c_compilers_and_nothing_else_moved(lib, tmp_path):
    from jpegsnoop_amd import capi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jsnoop_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(JsnoopExportCoding), offsetof(JsnoopExportCoding, huffman), sizeof(JsnoopExportSpec), sizeof(JsnoopTuning),\n'
                   '    JSNOOP_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(capi.ExportCoding), capi.ExportCoding.huffman.offset, C.sizeof(capi.ExportSpec), C.sizeof(capi.Tuning), 1]
    assert got == [8, 4, 8, 56, 1]
    assert lib.jsnoop_abi_version() == 1


def test_defaults_and_the_refusals_that_need_no_device(lib):
    from jpegsnoop_amd import capi
    c = capi.ExportCoding()
    C.memset(C.byref(c), 0xEE, C.sizeof(c))
    lib.jsnoop_export_coding_defaults(C.byref(c))
    assert (c.struct_size, c.huffman) == (8, 0)
    lib.jsnoop_export_coding_defaults(None)                          # (tolerated)
    s = capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(s))
    assert lib.jsnoop_batch_export_jpeg_coded(None, C.byref(s), C.byref(c), None, 1) == -1 and b"batch is NULL" in lib.jsnoop_last_error()
    n = C.c_uint32(7)
    assert lib.jsnoop_batch_export_tables(None, 0, 0, None, None, C.byref(n), None) == -1 and n.value == 7 and b"batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_export_jpeg_coded(None, b"x", C.byref(c)) == -1 and b"bad argument" in lib.jsnoop_last_error()
    assert capi.export_coding(lib, "optimal").huffman == 1 and capi.export_coding(lib, "annex_k").huffman == 0
    with pytest.raises(ValueError):
        capi.export_coding(lib, "best")


def test_host_arithmetic_as_a_host_program_under_sanitizers(checker):
    p = subprocess.run([checker], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
