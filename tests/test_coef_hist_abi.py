"""CPU: the ABI of jsnoop_batch_pack_coef_hist / jsnoop_batch_read_coef_hist without a device -- header, exports, binding, C++ wrapper and Python layer
carry the new entry points, a NULL batch is refused with a text, the ABI version did not move, and the constants the Python layer and the tests restate
are the kernel's.  The argument checks, the records and the 64-bit prefix table run as a stand-alone host program (tests/cpp/coef_hist_check.cpp) under
the address and undefined-behaviour sanitizers; the binning header the kernel compiles is swept over every value and every divisor by a second one
(tests/cpp/coef_hist_sweep.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_coef_hist_spec_defaults", "jsnoop_coef_hist_words", "jsnoop_batch_pack_coef_hist", "jsnoop_batch_read_coef_hist")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


def test_header_exports_binding_and_wrapper_carry_the_histogram_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"typedef struct JsnoopCoefHistSpec \{ uint32_t struct_size; int32_t order, quantised; uint32_t range; \} JsnoopCoefHistSpec;", hdr)
    assert re.search(r"jsnoop_batch_pack_coef_hist\(JsnoopBatch\*, const JsnoopCoefHistSpec\*, const int\* images, const int\* comps, int n, void\* dst, uint64_t row_pitch_words\)", hdr)
    assert re.search(r"jsnoop_batch_read_coef_hist\(JsnoopBatch\*, const JsnoopCoefHistSpec\*, const int\* images, const int\* comps, int n, uint32_t\* host_dst\)", hdr)
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+BatchPackCoefHist\(const JsnoopCoefHistSpec&\s*\w*, const std::vector<int>&\s*\w*, const std::vector<int>&\s*\w*, void\*\s*\w*,", wrapper)
    assert "jsnoop_batch_pack_coef_hist(m_b," in wrapper
    import jpegsnoop_amd as J
    assert callable(J.JpegBatch.coef_hist_to_torch) and callable(J.JpegBatch.coef_hist_all) and callable(J.JobFileResult.coef_hist_to_torch) and callable(J.coef_hist_fields)
    assert lib.jsnoop_abi_version() == 1
    types = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_types.h")).read()
    assert int(re.search(r"#define JS_COEF_HIST_UNIT (\d+)u", types).group(1)) == capi.COEF_HIST_UNIT
    assert int(re.search(r"#define JS_COEF_HIST_WAVES (\d+)u", types).group(1)) == capi.COEF_HIST_WAVES
    assert int(re.search(r"#define JS_COEF_HIST_WG_PER_CU (\d+)u", types).group(1)) == capi.COEF_HIST_WG_PER_CU
    kernel = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_coef_hist.hip")).read()
    assert "#define CH_LDS_PER_CU 163840u" in kernel and "jsnoop_coef_bin.h" in kernel, "capi.coef_hist_share restates the launch's grid rule"
    assert capi.coef_hist_share(10, 256, 127) == 5 and capi.coef_hist_share(100, 256, 127) == 8 and capi.coef_hist_share(100000, 256, 127) == 196 and capi.coef_hist_share(100000, 256, 16) == 196


def test_spec_defaults_and_row_length(lib):
    from jpegsnoop_amd import capi
    s = capi.CoefHistSpec()
    lib.jsnoop_coef_hist_spec_defaults(C.byref(s))
    assert (s.struct_size, s.order, s.quantised, s.range) == (C.sizeof(capi.CoefHistSpec), capi.COEF_NATURAL, 1, 127) and C.sizeof(capi.CoefHistSpec) == 16
    lib.jsnoop_coef_hist_spec_defaults(None)                        # NULL tolerated
    for R in range(0, 130):
        s.range = R
        want = capi.coef_hist_words(R) if 1 <= R <= 127 else 0
        assert lib.jsnoop_coef_hist_words(C.byref(s)) == want, R
    assert capi.coef_hist_words(127) == 16448 and lib.jsnoop_coef_hist_words(None) == 0
    s.range = 16; s.order = 2
    assert lib.jsnoop_coef_hist_words(C.byref(s)) == 0 and b"order" in lib.jsnoop_last_error()
    s.order = 0; s.struct_size = 20
    assert lib.jsnoop_coef_hist_words(C.byref(s)) == 0 and b"struct_size" in lib.jsnoop_last_error()
    s.struct_size = 4                                               # a shorter struct: the defaults, whatever the bytes behind it say
    assert lib.jsnoop_coef_hist_words(C.byref(s)) == capi.coef_hist_words(127)


def test_the_refusal_of_a_null_batch(lib):
    from jpegsnoop_amd import capi
    s = capi.CoefHistSpec()
    lib.jsnoop_coef_hist_spec_defaults(C.byref(s))
    buf = (C.c_uint32 * 8)(*([0xABCD] * 8))
    one = (C.c_int * 1)(0)
    assert lib.jsnoop_batch_pack_coef_hist(None, C.byref(s), one, one, 1, C.cast(buf, C.c_void_p), 0) == -1
    assert b"batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_batch_read_coef_hist(None, C.byref(s), one, one, 1, C.cast(buf, C.c_void_p)) == -1 and b"batch is NULL" in lib.jsnoop_last_error()
    assert list(buf) == [0xABCD] * 8


def test_coef_hist_fields_gives_views():
    import jpegsnoop_amd as J
    from jpegsnoop_amd import capi
    for R in (1, 16, 127):
        nb = 2 * R + 1
        row = np.arange(capi.coef_hist_words(R), dtype=np.uint32)
        hist, mn, mx = J.coef_hist_fields(row, R)
        assert hist.shape == (64, nb) and mn.shape == (64,) == mx.shape and mn.dtype == np.int32 == mx.dtype
        assert hist[3, 2] == 3 * nb + 2 and mn[0] == 64 * nb and mx[63] == 64 * nb + 127
        hist[5, 1] = 77; mn[2] = -9; mx[3] = -1
        assert row[5 * nb + 1] == 77 and row[64 * nb + 2] == 0xFFFFFFF7 and row[64 * nb + 64 + 3] == 0xFFFFFFFF, "views, not copies"
    with pytest.raises(ValueError):
        J.coef_hist_fields(np.zeros(capi.coef_hist_words(16), np.uint32), 17)
    with pytest.raises(ValueError):
        J.coef_hist_fields(np.zeros((2, capi.coef_hist_words(16)), np.uint32), 16)
    import torch
    t = torch.zeros(capi.coef_hist_words(2), dtype=torch.int32)
    hist, mn, mx = J.coef_hist_fields(t, 2)
    hist[1, 1] = 5; mx[63] = 9
    assert tuple(hist.shape) == (64, 5) and int(t[6]) == 5 and int(t[-1]) == 9


def test_argument_checks_as_a_host_program_under_sanitizers(tmp_path):
    """tests/cpp/coef_hist_check.cpp: the checks jsnoop_batch_pack_coef_hist makes before it touches the device (jsnoop_coef_hist_check.h), compiled for the host alone."""
    exe = tmp_path / "coef_hist_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "coef_hist_check.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


def test_the_binning_header_swept_over_every_value_and_divisor(tmp_path):
    """tests/cpp/coef_hist_sweep.cpp: jsnoop_coef_bin.h -- the text the kernel compiles -- against C's `/` for all 65536 values and every divisor 1 .. 65535, and
    against the clamp for every range.  No sanitizer: 4.3e9 divisions."""
    exe = tmp_path / "coef_hist_sweep"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "coef_hist_sweep.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
