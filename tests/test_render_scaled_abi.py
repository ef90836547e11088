"""CPU: the ABI of jsnoop_batch_pack_ijg_scaled without a device -- header, exports, binding and wrappers carry the three entry points, a NULL batch and a bad
denominator are refused with a text, the ABI version did not move.  The host arithmetic and the reduced render the kernel runs -- every refusal, the sizes, the
unit plan and the job list of every unit against a brute-force walk for four layouts x three scales -- run as a stand-alone host program
(tests/cpp/render_scaled_check.cpp) under the address and undefined-behaviour sanitizers; its reduced transforms of a block are the model's, and its rendering
of whole images -- with the very stage functions k_render_ijg_scaled calls, lanes in turn, through a poisoned copy of a wave's LDS, from an arena in which
every value the contract says is not read is poisoned -- is the model's, byte for byte."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ijg_cases as IC
import ijg_model as M
import ijg_scaled_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_batch_ijg_scaled_size", "jsnoop_batch_pack_ijg_scaled_bytes", "jsnoop_batch_pack_ijg_scaled")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/cpp/render_scaled_check.cpp compiled for the host alone, with the sanitizers."""
    exe = tmp_path_factory.mktemp("render_scaled_check") / "render_scaled_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "render_scaled_check.cpp")])
    return str(exe)


def test_header_exports_binding_and_wrappers_carry_the_scaled_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    ijg, scaled = capi.SIGNATURES["jsnoop_batch_pack_ijg"], capi.SIGNATURES["jsnoop_batch_pack_ijg_scaled"]
    assert scaled[0] == ijg[0] and scaled[1][:2] + scaled[1][3:] == ijg[1] and scaled[1][2] is C.c_uint     # jsnoop_batch_pack_ijg with a denominator
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+BatchPackIjgScaled\(", wrapper) and "jsnoop_batch_pack_ijg_scaled(" in wrapper and "jsnoop_batch_ijg_scaled_size(" in wrapper
    import jpegsnoop_amd as J
    sig = inspect.signature(J.JpegBatch.to_torch)
    assert sig.parameters["reduce"].default == 1 and sig.parameters["pixels"].default == "jpegsnoop"
    assert callable(J.JpegBatch.ijg_scaled_size) and callable(J.JpegBatch.reduce_for)
    mk = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "Makefile")).read()
    assert "jsnoop_render_scaled.hip" in mk and "jsnoop_render_scaled.cpp" in mk
    src = "".join(open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", f)).read() for f in ("jsnoop_render_scaled.hip", "jsnoop_render_scaled.cpp", "jsnoop_render_scaled_check.h"))
    assert "getenv" not in src and "asm(" not in src and "asm volatile" not in src and not re.search(r"\batomic\w+\s*\(", src)


def test_the_refusals_that_need_no_device_and_the_version(lib):
    from jpegsnoop_amd import capi
    spec = capi.PackSpec()
    lib.jsnoop_pack_spec_defaults(C.byref(spec))
    w, h = C.c_uint(7), C.c_uint(7)
    assert lib.jsnoop_batch_pack_ijg_scaled(None, C.byref(spec), 2, None, 0, None) == -1 and b"pack_ijg_scaled: batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_batch_ijg_scaled_size(None, 0, 2, C.byref(w), C.byref(h)) == -1 and b"pack_ijg_scaled: batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_batch_pack_ijg_scaled_bytes(None, C.byref(spec), 2, 0) == 0 and b"pack_ijg_scaled: batch is NULL" in lib.jsnoop_last_error()
    assert (w.value, h.value) == (7, 7)
    assert lib.jsnoop_abi_version() == 1
    assert C.sizeof(capi.PackSpec) == 40 and C.sizeof(capi.PackDst) == 24


def test_host_arithmetic_as_a_host_program_under_sanitizers(checker):
    p = subprocess.run([checker], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_reduced_transforms_of_the_shared_code_are_the_models(checker, seed):
    """The functions k_render_ijg_scaled calls (the 4 x 4 and 2 x 2 steps, the 1 x 1), run on the host over columns, then rows: random, extreme and wild
    (+-32767) blocks."""
    rng = np.random.default_rng(seed)
    for blk in (rng.integers(-1024, 1025, 64), rng.integers(0, 2, 64) * 2046 - 1023, rng.integers(0, 2, 64) * 65534 - 32767, rng.integers(-32768, 32768, 64),
                np.array([8 * 127] + [0] * 63), np.array([-32768] * 64), np.array([32767] * 64)):
        for n in (4, 2, 1):
            got = [int(x) for x in subprocess.check_output([checker, "block", str(n)] + [str(int(v)) for v in blk]).decode().split()]
            assert got == [int(v) for v in S.idct(blk.reshape(8, 8), n).reshape(-1)], (n, blk.tolist())


@pytest.mark.parametrize("s", S.SCALES)
@pytest.mark.parametrize("mode", IC.MODES)
def test_the_kernels_walk_run_on_the_host_renders_the_models_bytes(checker, mode, s, tmp_path):
    """Units, groups, sub-rounds, halo columns, clamped look-ups and four-pixel lanes as the kernel has them: the size list, sizes around the unit's run
    (8, 16, 32 MCUs of 16 pixels; 16, 32, 64 of 8), one MCU, reduced chroma widths of 2 and 3; the wild file."""
    mw = 8 if mode in ("grey", "444") else 16
    run = 64 * s // mw
    sizes = IC.SIZES + [(9, 7), (15, 17), (25, 25), (31, 33)] + [((run + d) * mw + e, 17 + 8 * k) for k, (d, e) in enumerate([(-1, 0), (0, -1), (0, 0), (0, 1), (1, 0), (1, 1)])]
    sizes += [(2 * run * mw + 3, 9), (8, 1), (9, 8), (s, s), (s + 1, s - 1), (17, 5)]
    files = [IC.pillow_file(IC.noise(w, h, 31 * k + 5), mode, 90) for k, (w, h) in enumerate(sizes) if w >= 1 and h >= 1]
    if mode == "420":
        files.append(IC.wild_file())
    for data in files:
        a, w, h, hv = M.arena_of_file(data)
        want, _ = S.render(a, w, h, hv, s)
        a.tofile(str(tmp_path / "a.bin"))
        p = subprocess.run([checker, "render", str(w), str(h), str(len(hv)), str(hv[0][0]), str(hv[0][1]), str(s), str(tmp_path / "a.bin"), str(tmp_path / "o.bin")],
                           capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout.split() == ["ok", str(want.shape[1]), str(want.shape[0])], (w, h, p.stdout + p.stderr)
        got = np.fromfile(str(tmp_path / "o.bin"), np.uint8).reshape(want.shape)
        assert np.array_equal(got, want), (mode, s, w, h, np.argwhere(got != want)[:4].tolist())
