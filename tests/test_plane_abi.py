"""CPU: the ABI of jsnoop_batch_pack_planes without a device -- header, exports, binding and C++ wrapper carry the new entry points, the two
structs have the sizes the C compiler gives them, the defaults are the documented ones, a NULL batch is refused with a text, and neither the
ABI version nor JsnoopTuning moved.  The argument checks, the size arithmetic and the prefix table run as a stand-alone host program
(tests/cpp/plane_check.cpp) under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_plane_spec_defaults", "jsnoop_batch_plane_size", "jsnoop_batch_plane_bytes", "jsnoop_batch_pack_planes")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


def test_header_exports_binding_and_wrapper_carry_the_plane_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    for word in ("JSNOOP_PLANE_FULL   0", "JSNOOP_PLANE_NATIVE 1", "JSNOOP_PLANE_I16    0", "JSNOOP_PLANE_U8     1", "JSNOOP_PLANE_F32    2", "JsnoopPlaneSpec", "JsnoopPlaneDst"):
        assert word in hdr, word
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+BatchPackPlanes\(const JsnoopPlaneSpec&\s*\w*, const std::vector<int>&\s*\w*, const std::vector<JsnoopPlaneDst>&\s*\w*\)", wrapper)
    assert "jsnoop_batch_pack_planes(m_b," in wrapper
    import jpegsnoop_amd as J
    assert callable(J.JpegBatch.planes_to_torch) and callable(J.JobFileResult.planes_to_torch) and callable(J.JpegBatch.plane_size)
    assert (capi.PLANE_FULL, capi.PLANE_NATIVE, capi.PLANE_I16, capi.PLANE_U8, capi.PLANE_F32) == (0, 1, 0, 1, 2)
    types = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_types.h")).read()
    assert int(re.search(r"#define JS_PLANE_SEG (\d+)u", types).group(1)) == capi.PLANE_SEG
    full = open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read()
    assert "clamp_s8(v >> 3) + 128" in full and "CapYccRange" in full             # the header says what U8 is, in both spellings


def test_struct_sizes_are_the_c_compilers_and_nothing_else_moved(lib, tmp_path):
    from jpegsnoop_amd import capi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jsnoop_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(JsnoopPlaneSpec), sizeof(JsnoopPlaneDst), sizeof(JsnoopTuning), JSNOOP_ABI_VERSION,\n'
                   '    offsetof(JsnoopPlaneSpec, res), offsetof(JsnoopPlaneSpec, dtype), offsetof(JsnoopPlaneSpec, scale), offsetof(JsnoopPlaneSpec, bias), offsetof(JsnoopPlaneDst, row_pitch),\n'
                   '    offsetof(JsnoopPlaneDst, comp), offsetof(JsnoopPlaneDst, reserved), sizeof(JsnoopPackSpec), sizeof(JsnoopPackDst), sizeof(JsnoopCoefSpec), sizeof(JsnoopCoefDst)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(capi.PlaneSpec), C.sizeof(capi.PlaneDst), C.sizeof(capi.Tuning), 1, capi.PlaneSpec.res.offset, capi.PlaneSpec.dtype.offset, capi.PlaneSpec.scale.offset,
                   capi.PlaneSpec.bias.offset, capi.PlaneDst.row_pitch.offset, capi.PlaneDst.comp.offset, capi.PlaneDst.reserved.offset, C.sizeof(capi.PackSpec), C.sizeof(capi.PackDst),
                   C.sizeof(capi.CoefSpec), C.sizeof(capi.CoefDst)]
    assert got[:3] == [36, 24, 56] and got[-4:] == [40, 24, 16, 32]
    assert lib.jsnoop_abi_version() == 1
    t = capi.Tuning(); lib.jsnoop_tuning_defaults(C.byref(t))
    assert t.struct_size == 56


def test_defaults_and_the_refusal_of_a_null_batch(lib):
    from jpegsnoop_amd import capi
    s = capi.PlaneSpec()
    C.memset(C.byref(s), 0xEE, C.sizeof(s))
    lib.jsnoop_plane_spec_defaults(C.byref(s))
    assert (s.struct_size, s.res, s.dtype, list(s.scale), list(s.bias)) == (36, capi.PLANE_FULL, capi.PLANE_I16, [1.0] * 3, [0.0] * 3)
    lib.jsnoop_plane_spec_defaults(None)                             # (tolerated)
    d = capi.PlaneDst(ptr=0x1000, row_pitch=0, comp=0, reserved=0)
    assert lib.jsnoop_batch_pack_planes(None, C.byref(s), None, 1, C.byref(d)) == -1
    assert b"batch is NULL" in lib.jsnoop_last_error()
    w, h = C.c_uint(7), C.c_uint(7)
    assert lib.jsnoop_batch_plane_size(None, C.byref(s), 0, 0, C.byref(w), C.byref(h)) == -1 and (w.value, h.value) == (7, 7)
    assert b"batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_batch_plane_bytes(None, C.byref(s), 0, 0) == 0


def test_argument_checks_as_a_host_program_under_sanitizers(tmp_path):
    """tests/cpp/plane_check.cpp: the checks jsnoop_batch_pack_planes makes before it touches the device (jsnoop_plane_check.h), compiled for the host alone."""
    exe = tmp_path / "plane_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "plane_check.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
