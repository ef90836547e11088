"""CPU: the ABI of jsnoop_batch_pack_stats / jsnoop_batch_read_stats without a device -- header, exports, binding, C++ wrapper and Python layer carry
the new entry points, a NULL batch is refused with a text, the ABI version did not move, and the constants the Python layer and the test catalogue
restate are the kernels'.  The argument checks, the records and the 64-bit prefix table run as a stand-alone host program
(tests/cpp/stats_check.cpp) under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_batch_pack_stats", "jsnoop_batch_read_stats")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


def test_header_exports_binding_and_wrapper_carry_the_statistics_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"jsnoop_batch_pack_stats\(JsnoopBatch\*, int histo_en, const int\* images, int n, void\* dst, uint64_t row_pitch_words, uint32_t\* totals\)", hdr)
    assert re.search(r"jsnoop_batch_read_stats\(JsnoopBatch\*, int histo_en, const int\* images, int n, uint32_t\* host_dst\)", hdr)
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+BatchPackStats\(bool\s*\w*, const std::vector<int>&\s*\w*, void\*\s*\w*,", wrapper) and "jsnoop_batch_pack_stats(m_b," in wrapper
    import jpegsnoop_amd as J
    assert callable(J.JpegBatch.stats_to_torch) and callable(J.JpegBatch.stats_all) and callable(J.JobFileResult.stats_to_torch) and callable(J.stats_fields)
    assert lib.jsnoop_abi_version() == 1
    types = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "jsnoop_types.h")).read()
    assert int(re.search(r"#define JS_STATS_UNIT (\d+)u", types).group(1)) == capi.STATS_UNIT
    assert int(re.search(r"#define JSNOOP_STATS_WORDS (\d+)", hdr).group(1)) == capi.STATS_WORDS == 2482


def test_the_refusal_of_a_null_batch(lib):
    buf = (C.c_uint32 * 8)(*([0xABCD] * 8))
    assert lib.jsnoop_batch_pack_stats(None, 1, None, 1, C.cast(buf, C.c_void_p), 0, None) == -1
    assert b"batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_batch_read_stats(None, 1, None, 1, C.cast(buf, C.c_void_p)) == -1 and b"batch is NULL" in lib.jsnoop_last_error()
    assert list(buf) == [0xABCD] * 8


def test_stats_fields_names_the_words():
    import jpegsnoop_amd as J
    row = np.arange(2482, dtype=np.uint32)
    f = J.stats_fields(row)
    assert f["records"].shape == (12, 3) and f["records"][3].tolist() == [9, 10, 11] and int(f["count"]) == 36
    assert f["clip"].tolist() == list(range(37, 50)) and f["r"][0] == 50 and f["g"][0] == 178 and f["b"][127] == 433 and f["y"].shape == (2048,) and f["y"][2047] == 2481
    assert sum(int(np.asarray(v).size) for v in f.values()) == 2482
    f["y"][5] = 7
    assert row[439] == 7, "views, not copies"
    with pytest.raises(ValueError):
        J.stats_fields(row[:100])


def test_argument_checks_as_a_host_program_under_sanitizers(tmp_path):
    """tests/cpp/stats_check.cpp: the checks jsnoop_batch_pack_stats makes before it touches the device (jsnoop_stats_check.h), compiled for the host alone."""
    exe = tmp_path / "stats_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "stats_check.cpp")])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
