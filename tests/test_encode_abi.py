"""CPU: the ABI of jsnoop_encode_* without a device -- header, exports and binding carry the entry points, the structs have the sizes the C compiler
gives them, the defaults are the documented ones, the tables of every quality are the model's, a NULL object is refused with a text, and neither the ABI
version nor the older structs moved.  The host arithmetic and the integer transform the kernel runs -- every refusal of spec and source, tables,
geometry and the unit plan against a brute-force walk, the exhaustive proof of the quantiser's reciprocal, the int16 bounds -- run as a stand-alone
host program (tests/cpp/encode_check.cpp) under the address and undefined-behaviour sanitizers; its transform of a block is the model's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import encode_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_encode_create", "jsnoop_encode_destroy", "jsnoop_encode_spec_defaults", "jsnoop_encode_qtables", "jsnoop_encode_run", "jsnoop_encode_count",
       "jsnoop_encode_image_info", "jsnoop_encode_read_coefs", "jsnoop_encode_export", "jsnoop_encode_export_count", "jsnoop_encode_export_file",
       "jsnoop_encode_read_export", "jsnoop_encode_export_copy", "jsnoop_encode_export_scan_count", "jsnoop_encode_export_scan_info")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/cpp/encode_check.cpp compiled for the host alone, with the sanitizers."""
    exe = tmp_path_factory.mktemp("encode_check") / "encode_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "encode_check.cpp")])
    return str(exe)


def test_header_exports_binding_and_wrappers_carry_the_encode_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    for word in ("JSNOOP_ENCODE_444         0", "JSNOOP_ENCODE_422         1", "JSNOOP_ENCODE_420         2", "JSNOOP_ENCODE_PLANAR      1", "JSNOOP_ENCODE_BGR         1",
                 "JsnoopEncodeSpec", "JsnoopEncodeSrc"):
        assert word in hdr, word
    assert int(re.search(r"#define JSNOOP_ENCODE_RUN\s+(\d+)u", hdr).group(1)) == capi.ENCODE_RUN
    assert (capi.ENCODE_444, capi.ENCODE_422, capi.ENCODE_420, capi.ENCODE_INTERLEAVED, capi.ENCODE_PLANAR, capi.ENCODE_RGB, capi.ENCODE_BGR) == (0, 1, 2, 0, 1, 0, 1)
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+EncodeJpeg\(", wrapper) and "jsnoop_encode_run(" in wrapper and "jsnoop_encode_export(" in wrapper
    import jpegsnoop_amd as J
    for fn in (J.JpegEncoder.encode, J.JpegEncoder.encode_to_torch, J.JpegEncoder.coefs, J.JpegBatch.encode_jpeg):
        assert callable(fn)
    mk = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "Makefile")).read()
    assert "jsnoop_encode.hip" in mk and "jsnoop_encode.cpp" in mk
    src = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_encode.hip")).read() + open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_encode.cpp")).read()
    assert "getenv" not in src and "asm(" not in src and "asm volatile" not in src


def test_struct_sizes_are_the_c_compilers_and_nothing_else_moved(lib, tmp_path):
    from jpegsnoop_amd import capi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jsnoop_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %zu %zu\\n", sizeof(JsnoopEncodeSpec), offsetof(JsnoopEncodeSpec, qtables), sizeof(JsnoopEncodeSrc),\n'
                   '    offsetof(JsnoopEncodeSrc, pixel_stride), offsetof(JsnoopEncodeSrc, row_pitch), offsetof(JsnoopEncodeSrc, bottom_up), sizeof(JsnoopTuning), sizeof(JsnoopExportSpec),\n'
                   '    JSNOOP_ABI_VERSION, sizeof(JsnoopExportProgressive), sizeof(JsnoopPackSpec)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(capi.EncodeSpec), capi.EncodeSpec.qtables.offset, C.sizeof(capi.EncodeSrc), capi.EncodeSrc.pixel_stride.offset, capi.EncodeSrc.row_pitch.offset,
                   capi.EncodeSrc.bottom_up.offset, C.sizeof(capi.Tuning), C.sizeof(capi.ExportSpec), 1, C.sizeof(capi.ExportProgressive), C.sizeof(capi.PackSpec)]
    assert got[:9] == [24, 16, 56, 28, 32, 48, 56, 8, 1]
    assert lib.jsnoop_abi_version() == 1


def test_defaults_tables_and_the_refusals_that_need_no_device(lib):
    from jpegsnoop_amd import capi
    s = capi.EncodeSpec()
    C.memset(C.byref(s), 0xEE, C.sizeof(s))
    lib.jsnoop_encode_spec_defaults(C.byref(s))
    assert (s.struct_size, s.quality, s.subsampling, s.reserved, bool(s.qtables)) == (24, 75, capi.ENCODE_420, 0, False)
    lib.jsnoop_encode_spec_defaults(None)                            # (tolerated)
    luma, chroma = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
    for q in range(1, 101):
        s.quality = q
        assert lib.jsnoop_encode_qtables(C.byref(s), luma, chroma) == 0
        assert (list(luma), list(chroma)) == M.quality_tables(q), q
    for bad in (0, 101, -5):
        s.quality = bad
        assert lib.jsnoop_encode_qtables(C.byref(s), luma, chroma) == -1 and b"quality" in lib.jsnoop_last_error()
    custom = ([1 + k for k in range(64)], [255 - k for k in range(64)])
    t = capi.encode_spec(lib, quality=0, qtables=custom)
    assert lib.jsnoop_encode_qtables(C.byref(t), luma, chroma) == 0 and (list(luma), list(chroma)) == custom
    t = capi.encode_spec(lib, qtables=([0] + [1] * 63, [1] * 64))
    assert lib.jsnoop_encode_qtables(C.byref(t), luma, chroma) == -1 and b"luma table is 0" in lib.jsnoop_last_error()
    with pytest.raises(ValueError):
        capi.encode_spec(lib, subsampling="4:1:1")
    with pytest.raises(ValueError):
        capi.encode_spec(lib, qtables=([1] * 63, [1] * 64))
    s.quality = 75
    assert lib.jsnoop_encode_run(None, C.byref(s), None, 0) == -1 and b"encoder is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_encode_count(None) == 0 and lib.jsnoop_encode_export_count(None) == 0 and lib.jsnoop_encode_export_scan_count(None, 0) == 0
    info = (C.c_uint * 16)()
    assert lib.jsnoop_encode_image_info(None, 0, info) == -1 and lib.jsnoop_encode_read_coefs(None, 0, None, None, 0) == -1
    assert lib.jsnoop_encode_export(None, None, None, None, None, None, 0) == -1 and b"encoder is NULL" in lib.jsnoop_last_error()
    ln = C.c_uint64(7)
    assert lib.jsnoop_encode_export_file(None, 0, None, C.byref(ln), None, None, None) == -1 and ln.value == 7
    assert lib.jsnoop_encode_read_export(None, 0, None, 0) == -1 and lib.jsnoop_encode_export_copy(None, 0, None, 0) == -1
    assert lib.jsnoop_encode_export_scan_info(None, 0, 0, None, None, None, None, None) == -1
    lib.jsnoop_encode_destroy(None)                                  # (tolerated)
    import torch
    if not torch.cuda.is_available():
        assert not lib.jsnoop_encode_create(None) and b"no CPU fallback" in lib.jsnoop_last_error()


def test_host_arithmetic_as_a_host_program_under_sanitizers(checker):
    p = subprocess.run([checker], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


@pytest.mark.parametrize("seed,q", [(1, 1), (2, 2), (3, 16), (4, 99), (5, 255)])
def test_the_transform_of_the_shared_code_is_the_models(checker, seed, q):
    """The functions k_encode calls (one jfdctint pass, the reciprocal quantiser), run on the host: random blocks and blocks of extremes."""
    rng = np.random.default_rng(seed)
    for blk in (rng.integers(0, 256, (8, 8)), rng.integers(0, 2, (8, 8)) * 255, np.full((8, 8), 255 * (seed & 1))):
        got = [int(x) for x in subprocess.check_output([checker, "block", str(q)] + [str(int(v)) for v in blk.reshape(-1)]).decode().split()]
        co = M.fdct(blk.astype(np.int64) - 128).reshape(64)
        want = np.sign(co) * ((np.abs(co) + 4 * q) // (8 * q)) * q
        assert got == [int(v) for v in want]
