"""CPU: the ABI of jsnoop_batch_export_jpeg without a device -- header, exports, binding and C++ wrapper carry the new entry points, the spec has
the size the C compiler gives it, the defaults are the documented ones, a NULL batch is refused with a text, and neither the ABI version nor
JsnoopTuning moved.  The host arithmetic -- every refusal, the header bytes for Pq 0 / 1 and one / three components, records, prefix tables, sizes
past 2^32 bits -- runs as a stand-alone host program (tests/cpp/export_check.cpp) under the address and undefined-behaviour sanitizers, and the
headers it writes are tests/export_model.py's, byte for byte."""
import ctypes as C
import os
import re
import subprocess

import pytest

import coef_model as CM
import export_model as EM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_export_spec_defaults", "jsnoop_batch_export_jpeg", "jsnoop_batch_export_count", "jsnoop_batch_export_file", "jsnoop_batch_read_export",
       "jsnoop_batch_export_copy", "jsnoop_export_jpeg")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/cpp/export_check.cpp compiled for the host alone, with the sanitizers."""
    exe = tmp_path_factory.mktemp("export_check") / "export_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "export_check.cpp")])
    return str(exe)


def test_header_exports_binding_and_wrappers_carry_the_export_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    for word in ("JSNOOP_EXPORT_OK          0", "JSNOOP_EXPORT_INEXACT     1", "JSNOOP_EXPORT_UNCODABLE   2", "JSNOOP_EXPORT_UNSUPPORTED 3", "JsnoopExportSpec"):
        assert word in hdr, word
    for name, val in (("TILE", capi.EXPORT_TILE), ("SCAN", capi.EXPORT_SCAN), ("CHUNK", capi.EXPORT_CHUNK), ("WINDOW", capi.EXPORT_WINDOW)):
        assert int(re.search(r"#define JSNOOP_EXPORT_%s\s+(\d+)u" % name, hdr).group(1)) == val, name
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+BatchExportJpeg\(const std::vector<int>&", wrapper) and "jsnoop_batch_export_jpeg(m_b," in wrapper and "jsnoop_export_jpeg(m_h," in wrapper
    import jpegsnoop_amd as J
    for fn in (J.JpegBatch.export_jpeg, J.JpegBatch.export_jpeg_to_torch, J.JpegBatch.export_results, J.JobFileResult.export_jpeg, J.CimgDecode.export_jpeg):
        assert callable(fn)
    assert (capi.EXPORT_OK, capi.EXPORT_INEXACT, capi.EXPORT_UNCODABLE, capi.EXPORT_UNSUPPORTED) == (0, 1, 2, 3)
    assert "jsnoop_export.hip" in open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "Makefile")).read()


def test_struct_size_is_the_c_compilers_and_nothing_else_moved(lib, tmp_path):
    from jpegsnoop_amd import capi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jsnoop_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %zu %zu\\n", sizeof(JsnoopExportSpec), offsetof(JsnoopExportSpec, jfif), sizeof(JsnoopTuning), JSNOOP_ABI_VERSION,\n'
                   '    sizeof(JsnoopPlaneSpec), sizeof(JsnoopCoefSpec)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(capi.ExportSpec), capi.ExportSpec.jfif.offset, C.sizeof(capi.Tuning), 1, C.sizeof(capi.PlaneSpec), C.sizeof(capi.CoefSpec)]
    assert got == [8, 4, 56, 1, 36, 16]
    assert lib.jsnoop_abi_version() == 1


def test_defaults_and_the_refusals_that_need_no_device(lib):
    from jpegsnoop_amd import capi
    s = capi.ExportSpec()
    C.memset(C.byref(s), 0xEE, C.sizeof(s))
    lib.jsnoop_export_spec_defaults(C.byref(s))
    assert (s.struct_size, s.jfif) == (8, 1)
    lib.jsnoop_export_spec_defaults(None)                            # (tolerated)
    assert lib.jsnoop_batch_export_jpeg(None, C.byref(s), None, 1) == -1 and b"batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_batch_export_count(None) == 0
    ln = C.c_uint64(7)
    assert lib.jsnoop_batch_export_file(None, 0, None, C.byref(ln), None, None, None) == -1 and ln.value == 7 and b"batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_batch_read_export(None, 0, None, 0) == -1 and lib.jsnoop_batch_export_copy(None, 0, None, 0) == -1
    assert lib.jsnoop_export_jpeg(None, b"x") == -1 and b"bad argument" in lib.jsnoop_last_error()


def test_host_arithmetic_as_a_host_program_under_sanitizers(checker):
    p = subprocess.run([checker], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


@pytest.mark.parametrize("image,jfif,q63", [(0, 1, 0), (0, 0, 0), (1, 1, 0), (2, 1, 0), (3, 0, 0), (0, 1, 300), (3, 1, 65535)])
def test_the_headers_of_the_host_code_are_the_models(checker, image, jfif, q63):
    """The checker's descriptors: 0 = 4:2:0 333 x 217, 1 = grey 1 x 1, 2 = 4:1:1 1025 x 9, 3 = (1x2, 2x1, 1x1) 100 x 50; multipliers 3, 5 + k, 7 by
    component, q63 (non-zero) replacing natural index 63 of component 1: above 255 it makes that table, and the frame, 16-bit."""
    hv, dims = [([(2, 2), (1, 1), (1, 1)], (333, 217)), ([(1, 1)], (1, 1)), ([(4, 1), (1, 1), (1, 1)], (1025, 9)), ([(1, 2), (2, 1), (1, 1)], (100, 50))][image]
    hmax = max(h for h, _ in hv); vmax = max(v for _, v in hv)
    geo = CM.Geometry(hv, -(-dims[0] // (8 * hmax)), -(-dims[1] // (8 * vmax)))
    qnat = [[3] * 64, [5 + k for k in range(64)], [7] * 64][:len(hv)]
    args = [checker, "header", str(image), str(jfif)]
    if q63:
        args.append(str(q63))
        if len(hv) > 1:
            qnat[1][63] = q63
    got = bytes.fromhex(subprocess.check_output(args).decode().strip())
    want = EM.header(geo, dims[0], dims[1], qnat, jfif=bool(jfif))
    assert got == want
    assert (b"\xFF\xC1" in got[:600]) == (q63 > 255 and len(hv) > 1)
