"""jsnoop_batch_export_jpeg_coded with the image's own Huffman tables (JSNOOP_HUFFMAN_OPTIMAL) against the Annex K export of the same batch.

Input: tools/export_bench.py's -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box).  The batch is
decoded once; then --warmup rounds and --reps timed rounds of (Annex K export of all images, optimal export of all images), alternating in one process, each
between its own two events on the batch's stream; median and minimum are reported, the wall clock of the call beside them (an export waits for the device
twice inside the call, so its event span holds the host's work between the two phases too).

Reported: the time of each mode, their ratio, the bytes each wrote and the saving.  The optimal mode adds one walk over the blocks (the symbol counts) to the
two there are, and one workgroup per image for the tables.

Kernel split: `rocprofv3 --kernel-trace --stats` over this tool with --images 256, in a run of its own (profiles/export_opt_kernels.txt).

Prints one JSON line; --out FILE also saves it (profiles/export_opt_bench.json is a run of this tool).
usage: python tools/export_opt_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jpegsnoop_amd as J                                            # noqa: E402
from oracle import harness as H                                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.warmup >= 5 and a.reps >= 20, "at least 5 warm-ups and 20 repetitions"
    H.build(["synth"])
    lib = J.load()
    dev = torch.device("cuda", 0)
    assert lib.jsnoop_set_device(0) == 0, J.last_error()
    stream = torch.cuda.Stream(dev)
    b = J.JpegBatch(stream=stream.cuda_stream)
    for i in range(min(a.distinct, a.images)):
        b.add_jpeg(H.synth_jpeg(width=a.width, height=a.height, hs=2, vs=2, quality=85, seed=i + 1))
    b.tile(a.images)
    b.upload(); b.decode(); b.sync()
    n = a.images
    spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
    coding = J.capi.export_coding(lib, "optimal")

    def annex():
        assert lib.jsnoop_batch_export_jpeg(b._h, C.byref(spec), None, n) == 0, J.last_error()

    def optimal():
        assert lib.jsnoop_batch_export_jpeg_coded(b._h, C.byref(spec), C.byref(coding), None, n) == 0, J.last_error()

    size = {}
    for name, fn in (("annex_k", annex), ("optimal", optimal)):
        fn()
        res = b.export_results()
        assert all(e["result"] == 0 for e in res), "every picture of the bench is exported"
        size[name] = sum(e["len"] for e in res)
    for _ in range(a.warmup):
        annex(); optimal()
    stream.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(a.reps)]
    wall = {"annex_k": [], "optimal": []}
    for e in ev:
        e[0].record(stream); t0 = time.perf_counter(); annex(); wall["annex_k"].append((time.perf_counter() - t0) * 1e3); e[1].record(stream)
        e[2].record(stream); t0 = time.perf_counter(); optimal(); wall["optimal"].append((time.perf_counter() - t0) * 1e3); e[3].record(stream)
    stream.synchronize()
    ta = [e[0].elapsed_time(e[1]) for e in ev]; to = [e[2].elapsed_time(e[3]) for e in ev]
    ma, mo = statistics.median(ta), statistics.median(to)
    out = {"tool": "tools/export_opt_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": min(a.distinct, n), "width": a.width, "height": a.height,
           "warmup": a.warmup, "reps": a.reps, "timing": "events on the batch stream around each call, Annex K and optimal export alternating; a span includes the call's two host waits",
           "annex_k_ms_median": round(ma, 4), "annex_k_ms_min": round(min(ta), 4), "annex_k_wall_ms_median": round(statistics.median(wall["annex_k"]), 4),
           "optimal_ms_median": round(mo, 4), "optimal_ms_min": round(min(to), 4), "optimal_wall_ms_median": round(statistics.median(wall["optimal"]), 4),
           "optimal_over_annex_k": round(mo / ma, 3), "annex_k_file_bytes": size["annex_k"], "optimal_file_bytes": size["optimal"],
           "bytes_saved": size["annex_k"] - size["optimal"], "saving_percent": round(100.0 * (size["annex_k"] - size["optimal"]) / size["annex_k"], 3)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
