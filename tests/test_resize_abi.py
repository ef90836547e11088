"""CPU: the ABI of jsnoop_batch_pack_resized without a device -- header, exports, binding and C++ wrapper carry the entry point, JsnoopResizeDst
has the layout the C compiler gives it, a NULL batch is refused with a text, and none of the pinned structs nor the ABI version moved.  The
argument checks and the record arithmetic run as a stand-alone host program (tests/cpp/resize_check.cpp) under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "jsnoop_batch_pack_resized"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


def test_header_exports_binding_and_wrapper_carry_the_entry_point(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    assert re.search(r"\bint\s+%s\s*\(JsnoopBatch\*, const JsnoopPackSpec\* spec, int filter,\s*const int\* images, int n, const JsnoopResizeDst\* dst\);" % NAME, hdr)
    assert re.search(r"\bT %s\b" % NAME, out)
    assert NAME in capi.SIGNATURES and hasattr(lib, NAME)
    res, args = capi.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 6 and args[1] == C.POINTER(capi.PackSpec) and args[2] is C.c_int and args[5] == C.POINTER(capi.ResizeDst)
    for word in ("#define JSNOOP_RESIZE_NEAREST  0", "#define JSNOOP_RESIZE_BILINEAR 1", "#define JSNOOP_RESIZE_AREA     2", "JsnoopResizeDst"):
        assert word in hdr, word
    assert (capi.RESIZE_NEAREST, capi.RESIZE_BILINEAR, capi.RESIZE_AREA) == (0, 1, 2)
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+BatchPackResized\(const JsnoopPackSpec&\s*\w*, int\s+\w*, const std::vector<int>&\s*\w*, const std::vector<JsnoopResizeDst>&\s*\w*\)", wrapper)
    assert "jsnoop_batch_pack_resized(m_b," in wrapper
    import inspect
    import jpegsnoop_amd as J
    params = inspect.signature(J.JpegBatch.to_torch).parameters
    assert params["size"].default is None and params["filter"].default == "bilinear" and params["roi"].default is None


def test_struct_layout_is_the_c_compilers_and_nothing_else_moved(lib, tmp_path):
    from jpegsnoop_amd import capi
    fields = ["ptr", "row_pitch", "plane_pitch", "out_w", "out_h", "roi_x", "roi_y", "roi_w", "roi_h"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jsnoop_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d", sizeof(JsnoopResizeDst), sizeof(JsnoopPackSpec), sizeof(JsnoopPackDst), sizeof(JsnoopTuning), JSNOOP_ABI_VERSION);\n'
                   + "".join('    printf(" %%zu", offsetof(JsnoopResizeDst, %s));\n' % f for f in fields) + '    printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got[0] == C.sizeof(capi.ResizeDst) == 48
    assert got[1:5] == [40, 24, 56, 1] and [C.sizeof(capi.PackSpec), C.sizeof(capi.PackDst), C.sizeof(capi.Tuning)] == [40, 24, 56]
    assert got[5:] == [getattr(capi.ResizeDst, f).offset for f in fields]
    assert lib.jsnoop_abi_version() == 1


def test_a_null_batch_is_refused_with_a_text(lib):
    from jpegsnoop_amd import capi
    s = capi.PackSpec(); lib.jsnoop_pack_spec_defaults(C.byref(s))
    d = capi.ResizeDst(ptr=0x1000, out_w=4, out_h=4)
    assert lib.jsnoop_batch_pack_resized(None, C.byref(s), capi.RESIZE_BILINEAR, None, 1, C.byref(d)) == -1
    err = lib.jsnoop_last_error()
    assert b"pack_resized" in err and b"batch is NULL" in err


def test_plan_and_checks_as_a_host_program_under_sanitizers(tmp_path):
    """tests/cpp/resize_check.cpp: what jsnoop_batch_pack_resized checks and computes before it touches the device, compiled for the host alone."""
    exe = tmp_path / "resize_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "resize_check.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
