"""CPU: the host-only parts of the job layer (jsnoop_job_* of include/jsnoop_gpu.h).  jsnoop_partition_lpt is the greedy
longest-processing-time rule of jpegsnoop_amd.shard.partition_lpt behind the C ABI and needs no device; the C++ side of the job
(jpegsnoop_amd/csrc/ImgDecodeGpu.h: GenBatchFileList, DoBatchFileProcessAll, JobRun) builds -Wall -Werror with plain g++; and without
a device a job cannot be created: no CPU fallback."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "job_demo")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G
    G.build()
    import jpegsnoop_amd
    return jpegsnoop_amd.load(require_device=False)


def build_job_demo():
    import __graft_entry__ as G
    G.build()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "job_demo.cpp"),
                           "-L" + os.path.join(ROOT, "jpegsnoop_amd"), "-ljsnoop_gpu", "-Wl,-rpath," + os.path.join(ROOT, "jpegsnoop_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])


def c_partition(lib, costs, parts):
    n = len(costs)
    arr = (C.c_uint64 * max(1, n))(*costs)
    out = (C.c_int * max(1, n))(*([-7] * max(1, n)))
    assert lib.jsnoop_partition_lpt(arr, n, parts, out) == 0
    bins = [[] for _ in range(parts)]
    for i in range(n):
        assert 0 <= out[i] < parts
        bins[out[i]].append(i)                                    # (ascending within a bin by construction)
    return bins


def cost_sets():
    rng = np.random.default_rng(20261017)
    yield "empty", []
    yield "one", [5]
    yield "all equal", [7] * 23
    yield "zeros", [0] * 11
    for k in range(6):                                            # few distinct values: ties everywhere
        yield "ties %d" % k, [int(x) for x in rng.integers(0, 4 + k, 40 + 13 * k)]
    for k in range(4):
        yield "spread %d" % k, [int(x) for x in rng.integers(0, 1 << 40, 64 + k)]
    yield "fewer than parts", [9, 3, 9]
    big = (1 << 63)
    yield "near 2^63", [big - 1, big - 1, big - 2, big, big + 5, 3, big - 1, 1, big, (1 << 64) - 1, (1 << 64) - 1, 17]
    yield "near 2^63, ties", [big] * 9 + [big - 1] * 5


@pytest.mark.parametrize("parts", range(1, 10))
def test_partition_lpt_equals_the_python_rule(lib, parts):
    from jpegsnoop_amd.shard import partition_lpt
    for name, costs in cost_sets():
        assert c_partition(lib, costs, parts) == partition_lpt(costs, parts), (name, parts)
        assert c_partition(lib, costs, parts) == c_partition(lib, costs, parts), (name, "deterministic")


def test_partition_lpt_refuses_bad_arguments(lib):
    out = (C.c_int * 4)()
    arr = (C.c_uint64 * 4)(1, 2, 3, 4)
    assert lib.jsnoop_partition_lpt(arr, 4, 0, out) == -1
    assert lib.jsnoop_partition_lpt(arr, -1, 2, out) == -1
    assert lib.jsnoop_partition_lpt(None, 4, 2, out) == -1
    assert lib.jsnoop_partition_lpt(None, 0, 3, None) == 0        # nothing to place


def test_job_structs_match_the_header(lib):
    """The ctypes structs are the header's: the library writes its own sizes into a defaults struct / accepts ours."""
    from jpegsnoop_amd import capi
    o = capi.JobOptions()
    lib.jsnoop_job_options_defaults(C.byref(o))
    assert o.struct_size == C.sizeof(capi.JobOptions) and o.decode_ac == 1
    assert (o.want_planes, o.enable_log, o.max_images_per_round, o.max_round_bytes, o.partition, o.keep_resident) == (0, 0, 0, 0, 0, 0)
    src = open(os.path.join(ROOT, "include", "jsnoop_gpu.h")).read()
    assert "#define JSNOOP_JOB_MAX_SHARDS %d" % capi.JOB_MAX_SHARDS in src
    exe = os.path.join(ROOT, "tests", "cpp", "job_sizes")
    code = ('#include <cstdio>\n#include "%s"\nint main() { printf("%%zu %%zu %%zu\\n", sizeof(JsnoopJobOptions), sizeof(JsnoopJobFile), sizeof(JsnoopJobStats)); }\n'
            % os.path.join(ROOT, "include", "jsnoop_gpu.h"))
    subprocess.run(["g++", "-x", "c++", "-", "-o", exe], input=code, text=True, check=True)
    try:
        sizes = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    finally:
        os.remove(exe)
    assert sizes == [C.sizeof(capi.JobOptions), C.sizeof(capi.JobFile), C.sizeof(capi.JobStats)]


def test_no_job_without_a_device(lib):
    import jpegsnoop_amd
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    assert not lib.jsnoop_job_create(None, 0)
    assert b"no CPU fallback" in lib.jsnoop_last_error()
    devs = (C.c_int * 2)(0, 0)
    assert not lib.jsnoop_job_create(devs, 2)
    assert b"no CPU fallback" in lib.jsnoop_last_error()
    with pytest.raises(RuntimeError):
        jpegsnoop_amd.JpegJob()


def test_job_demo_builds_and_refuses_without_gpu(tmp_path):
    """tests/cpp/job_demo.cpp against ImgDecodeGpu.h + the C ABI: -Wall -Werror, plain g++."""
    import torch
    build_job_demo()
    if torch.cuda.is_available():
        pytest.skip("GPU visible: the run is covered by tests/test_gpu_job.py")
    (tmp_path / "src").mkdir()
    r = subprocess.run([EXE, str(tmp_path / "src"), str(tmp_path / "dst")], capture_output=True, text=True)
    assert r.returncode == 3 and "no CPU fallback" in r.stdout
