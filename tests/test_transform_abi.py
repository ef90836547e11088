"""CPU: the ABI of jsnoop_transform_* without a device -- header, exports, binding and wrappers carry the entry points, the struct has the size the C
compiler gives it, the defaults are the documented ones, a NULL object is refused with a text, and neither the ABI version nor the older structs moved.
The host arithmetic and the block map the kernel runs -- every refusal of the spec, the divisions, entry geometry and the map against a brute-force walk,
the bijection, result words, the plan and 2^31 blocks -- run as a stand-alone host program (tests/cpp/transform_check.cpp) under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_transform_create", "jsnoop_transform_destroy", "jsnoop_transform_spec_defaults", "jsnoop_transform_run", "jsnoop_transform_entry",
       "jsnoop_transform_entry_count", "jsnoop_transform_count", "jsnoop_transform_image_info", "jsnoop_transform_image_dqt", "jsnoop_transform_read_coefs",
       "jsnoop_transform_export", "jsnoop_transform_export_count", "jsnoop_transform_export_file", "jsnoop_transform_read_export", "jsnoop_transform_export_copy",
       "jsnoop_transform_export_scan_count", "jsnoop_transform_export_scan_info", "jsnoop_batch_stream")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/cpp/transform_check.cpp compiled for the host alone, with the sanitizers."""
    exe = tmp_path_factory.mktemp("transform_check") / "transform_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "transform_check.cpp")])
    return str(exe)


def test_header_exports_binding_and_wrappers_carry_the_transform_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    names = "NONE FLIP_H FLIP_V TRANSPOSE TRANSVERSE ROT_90 ROT_180 ROT_270".split()
    for k, n in enumerate(names):                                    # libjpeg's JXFORM codes
        assert int(re.search(r"#define JSNOOP_XFORM_%s\s+(\d+)" % n, hdr).group(1)) == k == getattr(capi, "XFORM_" + n)
    for n, v in (("EDGE_TRIM", 0), ("EDGE_PERFECT", 1), ("OK", 0), ("IMPERFECT", 1), ("EMPTY", 2), ("UNSUPPORTED", 3)):
        assert int(re.search(r"#define JSNOOP_XFORM_%s\s+(\d+)" % n, hdr).group(1)) == v == getattr(capi, "XFORM_" + n)
    assert int(re.search(r"#define JSNOOP_TRANSFORM_RUN\s+(\d+)u", hdr).group(1)) == capi.TRANSFORM_RUN
    assert [capi.XFORM_EXIF[k] for k in range(2, 9)] == [capi.XFORM_FLIP_H, capi.XFORM_ROT_180, capi.XFORM_FLIP_V, capi.XFORM_TRANSPOSE, capi.XFORM_ROT_90,
                                                         capi.XFORM_TRANSVERSE, capi.XFORM_ROT_270]
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+TransformJpeg\(", wrapper) and "jsnoop_transform_run(" in wrapper and "jsnoop_transform_export(" in wrapper
    import jpegsnoop_amd as J
    for fn in (J.JpegTransform.run, J.JpegTransform.entries, J.JpegTransform.coefs, J.JpegTransform.export, J.JpegTransform.export_to_torch, J.JpegBatch.transform):
        assert callable(fn)
    mk = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "Makefile")).read()
    assert "jsnoop_transform.hip" in mk and "jsnoop_transform.cpp" in mk
    src = "".join(open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", f)).read() for f in ("jsnoop_transform.hip", "jsnoop_transform.cpp", "jsnoop_transform_check.h"))
    assert "getenv" not in src and "asm(" not in src and "asm volatile" not in src


def test_struct_size_is_the_c_compilers_and_nothing_else_moved(lib, tmp_path):
    from jpegsnoop_amd import capi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jsnoop_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %zu %zu\\n", sizeof(JsnoopTransformSpec), offsetof(JsnoopTransformSpec, edge),\n'
                   '    offsetof(JsnoopTransformSpec, crop_x), offsetof(JsnoopTransformSpec, reserved), sizeof(JsnoopEncodeSpec), sizeof(JsnoopTuning), sizeof(JsnoopExportSpec),\n'
                   '    JSNOOP_ABI_VERSION, sizeof(JsnoopExportProgressive), sizeof(JsnoopPackSpec)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(capi.TransformSpec), capi.TransformSpec.edge.offset, capi.TransformSpec.crop_x.offset, capi.TransformSpec.reserved.offset, C.sizeof(capi.EncodeSpec),
                   C.sizeof(capi.Tuning), C.sizeof(capi.ExportSpec), 1, C.sizeof(capi.ExportProgressive), C.sizeof(capi.PackSpec)]
    assert got[:8] == [40, 8, 20, 36, 24, 56, 8, 1]
    assert lib.jsnoop_abi_version() == 1


def test_defaults_and_the_refusals_that_need_no_device(lib):
    from jpegsnoop_amd import capi
    s = capi.TransformSpec()
    C.memset(C.byref(s), 0xEE, C.sizeof(s))
    lib.jsnoop_transform_spec_defaults(C.byref(s))
    assert (s.struct_size, s.op, s.edge, s.grayscale, s.crop, s.crop_x, s.crop_y, s.crop_w, s.crop_h, s.reserved) == (40, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    lib.jsnoop_transform_spec_defaults(None)                         # (tolerated)
    t = capi.transform_spec(lib, "rot90", "perfect", True, (1, 2, 3, 4))
    assert (t.op, t.edge, t.grayscale, t.crop, t.crop_x, t.crop_y, t.crop_w, t.crop_h) == (5, 1, 1, 1, 1, 2, 3, 4)
    with pytest.raises(ValueError):
        capi.transform_spec(lib, "rot45")
    with pytest.raises(ValueError):
        capi.transform_spec(lib, "none", "keep")
    with pytest.raises(ValueError):
        capi.transform_spec(lib, "none", crop=(1, 2, 3))
    assert lib.jsnoop_transform_run(None, None, C.byref(s), None, 0) == -1 and b"transform object is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_transform_count(None) == 0 and lib.jsnoop_transform_entry_count(None) == 0 and lib.jsnoop_transform_export_count(None) == 0
    assert lib.jsnoop_transform_export_scan_count(None, 0) == 0 and lib.jsnoop_batch_stream(None) is None
    info = (C.c_uint * 16)(); q = (C.c_uint16 * 64)(); r = C.c_int(7)
    assert lib.jsnoop_transform_entry(None, 0, C.byref(r), None) == -1 and r.value == 7
    assert lib.jsnoop_transform_image_info(None, 0, info) == -1 and lib.jsnoop_transform_image_dqt(None, 0, 0, q) == -1 and lib.jsnoop_transform_read_coefs(None, 0, None, None, 0) == -1
    assert lib.jsnoop_transform_export(None, None, None, None, None, None, 0) == -1 and b"transform object is NULL" in lib.jsnoop_last_error()
    ln = C.c_uint64(7)
    assert lib.jsnoop_transform_export_file(None, 0, None, C.byref(ln), None, None, None) == -1 and ln.value == 7
    assert lib.jsnoop_transform_read_export(None, 0, None, 0) == -1 and lib.jsnoop_transform_export_copy(None, 0, None, 0) == -1
    assert lib.jsnoop_transform_export_scan_info(None, 0, 0, None, None, None, None, None) == -1
    lib.jsnoop_transform_destroy(None)                               # (tolerated)
    import torch
    if not torch.cuda.is_available():
        assert not lib.jsnoop_transform_create(None) and b"no CPU fallback" in lib.jsnoop_last_error()


def test_host_arithmetic_and_the_block_map_as_a_host_program_under_sanitizers(checker):
    p = subprocess.run([checker], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
