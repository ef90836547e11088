"""CPU: the ABI of jsnoop_batch_pack without a device -- header, exports, binding and C++ wrapper carry the new entry points, the two structs
have the sizes the C compiler gives them, the defaults are the documented ones, a NULL batch is refused with a text, and neither the ABI
version nor JsnoopTuning moved.  The argument checks themselves run as a stand-alone host program (tests/cpp/pack_check.cpp) under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_pack_spec_defaults", "jsnoop_batch_pack_bytes", "jsnoop_batch_pack")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


def test_header_exports_binding_and_wrapper_carry_the_pack_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW + ("jsnoop_batch_device",):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    for word in ("JSNOOP_PACK_HWC 0", "JSNOOP_PACK_CHW 1", "JSNOOP_PACK_U8  0", "JSNOOP_PACK_F32 1", "JsnoopPackSpec", "JsnoopPackDst"):
        assert word in hdr, word
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+BatchPack\(const JsnoopPackSpec&\s*\w*, const std::vector<int>&\s*\w*, const std::vector<JsnoopPackDst>&\s*\w*\)", wrapper)
    assert "jsnoop_batch_pack(m_b," in wrapper
    import jpegsnoop_amd as J
    assert callable(J.JpegBatch.to_torch) and callable(J.JobFileResult.to_torch)
    assert (capi.PACK_HWC, capi.PACK_CHW, capi.PACK_U8, capi.PACK_F32) == (0, 1, 0, 1)


def test_struct_sizes_are_the_c_compilers_and_nothing_else_moved(lib, tmp_path):
    from jpegsnoop_amd import capi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jsnoop_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %zu %zu %zu %zu %zu\\n", sizeof(JsnoopPackSpec), sizeof(JsnoopPackDst), sizeof(JsnoopTuning), JSNOOP_ABI_VERSION,\n'
                   '    offsetof(JsnoopPackSpec, scale), offsetof(JsnoopPackSpec, bias), offsetof(JsnoopPackDst, row_pitch), offsetof(JsnoopPackDst, plane_pitch), offsetof(JsnoopPackSpec, bgr)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(capi.PackSpec), C.sizeof(capi.PackDst), C.sizeof(capi.Tuning), 1, capi.PackSpec.scale.offset, capi.PackSpec.bias.offset,
                   capi.PackDst.row_pitch.offset, capi.PackDst.plane_pitch.offset, capi.PackSpec.bgr.offset]
    assert got[:3] == [40, 24, 56]
    assert lib.jsnoop_abi_version() == 1
    t = capi.Tuning(); lib.jsnoop_tuning_defaults(C.byref(t))
    assert t.struct_size == 56


def test_defaults_and_the_refusal_of_a_null_batch(lib):
    from jpegsnoop_amd import capi
    s = capi.PackSpec()
    C.memset(C.byref(s), 0xEE, C.sizeof(s))
    lib.jsnoop_pack_spec_defaults(C.byref(s))
    assert (s.struct_size, s.layout, s.dtype, s.bgr) == (C.sizeof(capi.PackSpec), 0, 0, 0)
    assert list(s.scale) == [1.0, 1.0, 1.0] and list(s.bias) == [0.0, 0.0, 0.0]
    lib.jsnoop_pack_spec_defaults(None)                              # (tolerated)
    d = capi.PackDst(ptr=0x1000, row_pitch=0, plane_pitch=0)
    assert lib.jsnoop_batch_pack(None, C.byref(s), None, 1, C.byref(d)) == -1
    assert b"batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_batch_pack_bytes(None, C.byref(s), 0) == 0
    assert lib.jsnoop_batch_device(None) == -1


def test_argument_checks_as_a_host_program_under_sanitizers(tmp_path):
    """tests/cpp/pack_check.cpp: the checks jsnoop_batch_pack makes before it touches the device (jsnoop_pack_check.h), compiled for the host alone."""
    exe = tmp_path / "pack_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "pack_check.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
