"""jsnoop_batch_export_jpeg against a plain device-to-device copy of the same traffic and against the decode of the same batch.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box).  The batch is
decoded once; then --warmup rounds and --reps timed rounds of (export of all images, copy, decode), alternating in one process, each between its own two
events on the batch's stream; median and minimum are reported.  The export waits for the device twice inside the call, so its event span holds the host's
work between the two phases too (the stream idles meanwhile); the wall clock of the call is given beside it.

Yardstick: hipMemcpyAsync device to device (a contiguous torch copy_ on the same stream) moving (arena + dccum read once + file bytes written) / 2 bytes each
way -- the least traffic a one-read encoder would have.  The call as built reads the arena and dccum twice (the measuring pass, the writing pass), writes and
reads the per-block lengths, and writes, reads twice and rewrites the stream (bits, FF count, stuffing): "traffic_as_built" adds those up.

Stage split: not taken here (the kernels run between two host waits; events cannot be put between them from outside).  `rocprofv3 --kernel-trace --stats`
over this tool with --images 256 --reps 20, in a run of its own, gives the kernels' times (profiles/export_kernels.txt).

Beside them, on --host-images images, the way there was before: jsnoop_batch_read_coefs per image, wall clock -- before any encoding.

Prints one JSON line; --out FILE also saves it (profiles/export_bench.json is a run of this tool).
usage: python tools/export_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--host-images 64] [--out FILE]"""
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
    ap.add_argument("--host-images", type=int, default=64)
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

    def export():
        assert lib.jsnoop_batch_export_jpeg(b._h, C.byref(spec), None, n) == 0, J.last_error()

    export()
    res = b.export_results()
    assert all(e["result"] == 0 for e in res), "every picture of the bench is exported"
    file_bytes = sum(e["len"] for e in res)
    blocks = n * sum(w * h for w, h in (b.coef_grid(0, c) for c in range(3)))                  # (the pictures have one size)
    arena, dccum = blocks * 128, blocks * 2
    half = (arena + dccum + file_bytes) // 2
    as_built = 2 * (arena + dccum) + 2 * blocks * 2 + 4 * file_bytes
    src_c = torch.empty(half, dtype=torch.uint8, device=dev); dst_c = torch.empty(half, dtype=torch.uint8, device=dev)

    def copy():
        with torch.cuda.stream(stream):
            dst_c.copy_(src_c, non_blocking=True)

    for _ in range(a.warmup):
        export(); copy(); b.decode()
    stream.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(a.reps)]
    wall = []
    for e in ev:
        e[0].record(stream); t0 = time.perf_counter(); export(); wall.append((time.perf_counter() - t0) * 1e3); e[1].record(stream)
        e[2].record(stream); copy(); e[3].record(stream)
        e[4].record(stream); b.decode(); e[5].record(stream)
    stream.synchronize()
    b.sync()
    te = [e[0].elapsed_time(e[1]) for e in ev]; tc = [e[2].elapsed_time(e[3]) for e in ev]; td = [e[4].elapsed_time(e[5]) for e in ev]
    me, mc, md, mw = statistics.median(te), statistics.median(tc), statistics.median(td), statistics.median(wall)
    # the way there was before: read_coefs per image
    hn = min(a.host_images, n)
    b.coefs(0)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for i in range(hn):
        b.coefs(i)
    host_ms = (time.perf_counter() - t0) * 1e3
    out = {"tool": "tools/export_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": min(a.distinct, n), "width": a.width, "height": a.height,
           "warmup": a.warmup, "reps": a.reps, "timing": "events on the batch stream around each call, alternating export / copy / decode; the export's span includes its two host waits",
           "blocks": blocks, "arena_bytes": arena, "dccum_bytes": dccum, "file_bytes": file_bytes, "copy_bytes_each_way": half, "traffic_as_built": as_built,
           "export_ms_median": round(me, 4), "export_ms_min": round(min(te), 4), "export_wall_ms_median": round(mw, 4), "export_wall_ms_min": round(min(wall), 4),
           "copy_ms_median": round(mc, 4), "copy_ms_min": round(min(tc), 4), "decode_ms_median": round(md, 4), "decode_ms_min": round(min(td), 4),
           "export_over_copy": round(me / mc, 3), "export_over_decode": round(me / md, 3),
           "export_gb_per_s_least_traffic": round(2 * half / me / 1e6, 1), "export_gb_per_s_as_built": round(as_built / me / 1e6, 1), "copy_gb_per_s": round(2 * half / mc / 1e6, 1),
           "host_path": {"images": hn, "what": "JpegBatch.coefs(i) (jsnoop_batch_read_coefs) per image, wall clock, before any encoding", "ms": round(host_ms, 2),
                         "ms_per_image": round(host_ms / max(hn, 1), 3)}}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
