"""CPU: the ABI of jsnoop_batch_pack_ijg without a device -- header, exports, binding and wrappers carry the entry points, the structs it shares with
jsnoop_batch_pack kept their sizes, a NULL batch is refused with a text, and the ABI version did not move.  The host arithmetic and the integer render the
kernel runs -- every refusal, the unit plan and the job list of every unit against a brute-force walk, the colour lines over all 2^24 inputs -- run as a
stand-alone host program (tests/cpp/render_check.cpp) under the address and undefined-behaviour sanitizers; its transform of a block is the model's, and
its rendering of a whole image -- unit by unit, job by job, through a poisoned copy of a wave's LDS, with the functions k_render_ijg calls -- is the model's."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ijg_cases as IC
import ijg_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("jsnoop_batch_pack_ijg", "jsnoop_batch_ijg_renderable")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tests/cpp/render_check.cpp compiled for the host alone, with the sanitizers."""
    exe = tmp_path_factory.mktemp("render_check") / "render_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "render_check.cpp")])
    return str(exe)


def test_header_exports_binding_and_wrappers_carry_the_render_entry_points(lib):
    from jpegsnoop_amd import capi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "jpegsnoop_amd", "libjsnoop_gpu.so")]).decode()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in capi.SIGNATURES and hasattr(lib, name), name
    assert capi.SIGNATURES["jsnoop_batch_pack_ijg"] == capi.SIGNATURES["jsnoop_batch_pack"]           # the seventh sibling: the pack's own spec and destinations
    wrapper = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "ImgDecodeGpu.h")).read()
    assert re.search(r"bool\s+BatchPackIjg\(", wrapper) and "jsnoop_batch_pack_ijg(" in wrapper and "jsnoop_batch_ijg_renderable(" in wrapper
    import inspect
    import jpegsnoop_amd as J
    sig = inspect.signature(J.JpegBatch.to_torch)
    assert sig.parameters["pixels"].default == "jpegsnoop" and callable(J.JpegBatch.ijg_renderable)
    mk = open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", "Makefile")).read()
    assert "jsnoop_render.hip" in mk and "jsnoop_render.cpp" in mk
    src = "".join(open(os.path.join(ROOT, "jpegsnoop_amd", "csrc", f)).read() for f in ("jsnoop_render.hip", "jsnoop_render.cpp", "jsnoop_render_check.h"))
    assert "getenv" not in src and "asm(" not in src and "asm volatile" not in src and not re.search(r"\batomic\w+\s*\(", src)


def test_struct_sizes_are_the_c_compilers_and_nothing_else_moved(lib, tmp_path):
    from jpegsnoop_amd import capi
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "jsnoop_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d\\n", sizeof(JsnoopPackSpec), offsetof(JsnoopPackSpec, scale), sizeof(JsnoopPackDst),\n'
                   '    offsetof(JsnoopPackDst, plane_pitch), sizeof(JsnoopTuning), JSNOOP_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(capi.PackSpec), capi.PackSpec.scale.offset, C.sizeof(capi.PackDst), capi.PackDst.plane_pitch.offset, C.sizeof(capi.Tuning), 1]
    assert got[:4] == [40, 16, 24, 16]
    assert lib.jsnoop_abi_version() == 1


def test_the_refusals_that_need_no_device(lib):
    from jpegsnoop_amd import capi
    spec = capi.PackSpec()
    lib.jsnoop_pack_spec_defaults(C.byref(spec))
    assert lib.jsnoop_batch_pack_ijg(None, C.byref(spec), None, 0, None) == -1 and b"pack_ijg: batch is NULL" in lib.jsnoop_last_error()
    assert lib.jsnoop_batch_ijg_renderable(None, 0) == 0 and b"pack_ijg: batch is NULL" in lib.jsnoop_last_error()


def test_host_arithmetic_as_a_host_program_under_sanitizers(checker):
    p = subprocess.run([checker], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_transform_of_the_shared_code_is_the_models(checker, seed):
    """The function k_render_ijg calls (one jidctint step), run on the host over columns, then rows: random, extreme and wild (+-32767) blocks."""
    rng = np.random.default_rng(seed)
    for blk in (rng.integers(-1024, 1025, 64), rng.integers(0, 2, 64) * 2046 - 1023, rng.integers(0, 2, 64) * 65534 - 32767, rng.integers(-32768, 32768, 64),
                np.array([8 * 127] + [0] * 63)):
        got = [int(x) for x in subprocess.check_output([checker, "block"] + [str(int(v)) for v in blk]).decode().split()]
        assert got == [int(v) for v in M.idct(blk.reshape(8, 8)).reshape(-1)]


@pytest.mark.parametrize("mode", IC.MODES)
def test_the_kernels_walk_run_on_the_host_renders_the_models_bytes(checker, mode, tmp_path):
    """Units, jobs, halo cells, clamped look-ups and four-pixel lanes as the kernel has them: sizes around the 8-MCU unit, one MCU, dw = 2 and 3; the wild file."""
    sizes = IC.SIZES + [(111, 17), (112, 16), (113, 15), (127, 33), (128, 32), (129, 31), (143, 47), (144, 48), (145, 49), (449, 33), (16, 1), (300, 8)]
    files = [IC.pillow_file(IC.noise(w, h, 31 * k + 5), mode, 90) for k, (w, h) in enumerate(sizes)]
    if mode == "420":
        files.append(IC.wild_file())
    for data in files:
        a, w, h, hv = M.arena_of_file(data)
        want, _ = M.render(a, w, h, hv)
        a.tofile(str(tmp_path / "a.bin"))
        p = subprocess.run([checker, "render", str(w), str(h), str(len(hv)), str(hv[0][0]), str(hv[0][1]), str(tmp_path / "a.bin"), str(tmp_path / "o.bin")], capture_output=True, text=True)
        assert p.returncode == 0 and p.stdout.strip() == "ok", (w, h, p.stdout + p.stderr)
        got = np.fromfile(str(tmp_path / "o.bin"), np.uint8).reshape(h, w, 3)
        assert np.array_equal(got, want), (mode, w, h, np.argwhere(got != want)[:4].tolist())
