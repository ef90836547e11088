"""CPU: the ABI of jsnoop_batch_pack_coefs without a device -- header, exports, binding and C++ wrapper carry the new entry points, the two
structs have the sizes the C compiler gives them, the defaults are the documented ones, a NULL batch is refused with a text, and neither the
ABI version nor JsnoopTuning moved.  The argument checks, the grid arithmetic and the prefix table run as a stand-alone host program
(tests/cpp/coef_check.cpp) under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_coef_spec_defaults", "jsnoop_batch_coef_grid", "jsnoop_batch_coef_bytes", "jsnoop_batch_pack_coefs", "jsnoop_batch_image_dqt")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


def test_header_exports_binding_and_wrapper_carry_the_coefficient_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    for word in ("JSNOOP_COEF_BLOCKS  0", "JSNOOP_COEF_FREQ    1", "JSNOOP_COEF_I16     0", "JSNOOP_COEF_F32     1", "JSNOOP_COEF_NATURAL 0", "JSNOOP_COEF_ZIGZAG  1",
                 "JsnoopCoefSpec", "JsnoopCoefDst"):
        assert word in hdr, word
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+BatchPackCoefs\(const JsnoopCoefSpec&\s*\w*, const std::vector<int>&\s*\w*, const std::vector<JsnoopCoefDst>&\s*\w*\)", wrapper)
    assert "jsnoop_batch_pack_coefs(m_b," in wrapper
    import jpegsnoop_amd as J
    assert callable(J.JpegBatch.coefs_to_torch) and callable(J.JobFileResult.coefs_to_torch) and callable(J.JpegBatch.coef_grid) and callable(J.JpegBatch.dqt)
    assert (capi.COEF_BLOCKS, capi.COEF_FREQ, capi.COEF_I16, capi.COEF_F32, capi.COEF_NATURAL, capi.COEF_ZIGZAG) == (0, 1, 0, 1, 0, 1)
    types = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_types.h")).read()
    assert int(re.search(r"#define JS_COEF_TILE (\d+)u", types).group(1)) == capi.COEF_TILE


def test_struct_sizes_are_the_c_compilers_and_nothing_else_moved(lib, tmp_path):
    from jpegsnoop_amd import capi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jsnoop_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(JsnoopCoefSpec), sizeof(JsnoopCoefDst), sizeof(JsnoopTuning), JSNOOP_ABI_VERSION,\n'
                   '    offsetof(JsnoopCoefSpec, layout), offsetof(JsnoopCoefSpec, dtype), offsetof(JsnoopCoefSpec, order), offsetof(JsnoopCoefDst, row_pitch),\n'
                   '    offsetof(JsnoopCoefDst, plane_pitch), offsetof(JsnoopCoefDst, comp), offsetof(JsnoopCoefDst, reserved), sizeof(JsnoopPackSpec), sizeof(JsnoopPackDst)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(capi.CoefSpec), C.sizeof(capi.CoefDst), C.sizeof(capi.Tuning), 1, capi.CoefSpec.layout.offset, capi.CoefSpec.dtype.offset, capi.CoefSpec.order.offset,
                   capi.CoefDst.row_pitch.offset, capi.CoefDst.plane_pitch.offset, capi.CoefDst.comp.offset, capi.CoefDst.reserved.offset, C.sizeof(capi.PackSpec), C.sizeof(capi.PackDst)]
    assert got[:3] == [16, 32, 56] and got[-2:] == [40, 24]
    assert lib.jsnoop_abi_version() == 1
    t = capi.Tuning(); lib.jsnoop_tuning_defaults(C.byref(t))
    assert t.struct_size == 56


def test_defaults_and_the_refusal_of_a_null_batch(lib):
    from jpegsnoop_amd import capi
    s = capi.CoefSpec()
    C.memset(C.byref(s), 0xEE, C.sizeof(s))
    lib.jsnoop_coef_spec_defaults(C.byref(s))
    assert (s.struct_size, s.layout, s.dtype, s.order) == (16, capi.COEF_BLOCKS, capi.COEF_I16, capi.COEF_NATURAL)
    lib.jsnoop_coef_spec_defaults(None)                              # (tolerated)
    d = capi.CoefDst(ptr=0x1000, row_pitch=0, plane_pitch=0, comp=0, reserved=0)
    assert lib.jsnoop_batch_pack_coefs(None, C.byref(s), None, 1, C.byref(d)) == -1
    assert b"batch is NULL" in lib.jsnoop_last_error()
    bw, bh = C.c_uint(7), C.c_uint(7)
    assert lib.jsnoop_batch_coef_grid(None, 0, 0, C.byref(bw), C.byref(bh)) == -1 and (bw.value, bh.value) == (7, 7)
    assert lib.jsnoop_batch_coef_bytes(None, C.byref(s), 0, 0) == 0
    q = (C.c_uint16 * 64)()
    assert lib.jsnoop_batch_image_dqt(None, 0, 0, q) == -1 and b"batch is NULL" in lib.jsnoop_last_error()


def test_argument_checks_as_a_host_program_under_sanitizers(tmp_path):
    """tests/cpp/coef_check.cpp: the checks jsnoop_batch_pack_coefs makes before it touches the device (jsnoop_coef_check.h), compiled for the host alone."""
    exe = tmp_path / "coef_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "coef_check.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
