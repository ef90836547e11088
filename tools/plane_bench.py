"""jsnoop_batch_pack_planes against a plain device-to-device copy of the same traffic.

Input: the bench's config 3 with retained planes -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller
box).  The batch is decoded once with want_planes; then every form packs its planes of all images into one dense allocation, timed by events on the
batch's stream: --warmup calls, then --reps pairs of (call, copy), each between its own two events; median and minimum are reported.

Forms: Y alone FULL U8; all three FULL I16; all three NATIVE U8 (three-plane 4:2:0); all three FULL F32.

Yardstick: hipMemcpyAsync device to device (a contiguous torch copy_ on the same stream), in the same process, moving the same total traffic.  The call
reads whole source rows -- every row of a FULL plane, every ev-th row of a NATIVE one, dim_x int16 each -- and writes w * h * elem bytes per plane; the
copy moves (read + written) / 2 bytes, so its read plus its write equals the call's.  Rates are (bytes read + bytes written) / time.

Beside them, on --host-images images, the only way there was before: jsnoop_batch_read_planes per image (three staged D2H copies and a wait) and an
upload of the three planes, wall clock.

Prints one JSON line; --out FILE also saves it (profiles/plane_bench.json is a run of this tool).
usage: python tools/plane_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--host-images 64] [--out FILE]"""
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

FORMS = [("Y_FULL_U8", "full", "uint8", (0,)), ("YCbCr_FULL_I16", "full", "int16", (0, 1, 2)), ("YCbCr_NATIVE_U8", "native", "uint8", (0, 1, 2)),
         ("YCbCr_FULL_F32", "full", "float32", (0, 1, 2))]
ELEM = {"uint8": 1, "int16": 2, "float32": 4}


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
    b = J.JpegBatch(stream=stream.cuda_stream, want_planes=True)
    for i in range(min(a.distinct, a.images)):
        b.add_jpeg(H.synth_jpeg(width=a.width, height=a.height, hs=2, vs=2, quality=85, seed=i + 1))
    b.tile(a.images)
    b.upload(); b.decode(); b.sync()
    n, px = a.images, a.width * a.height
    big = torch.empty(n * px * 12, dtype=torch.uint8, device=dev)            # the largest form's output; the copy's source
    other = torch.empty(n * px * 9, dtype=torch.uint8, device=dev)           # (the largest form reads 6 and writes 12 bytes a pixel: 9 each way)
    torch.cuda.synchronize(dev)
    forms = {}
    for name, res, dtype, comps in FORMS:
        spec = J.capi.PlaneSpec(); lib.jsnoop_plane_spec_defaults(C.byref(spec))
        spec.res = J.capi.PLANE_NATIVE if res == "native" else J.capi.PLANE_FULL
        spec.dtype = {"uint8": J.capi.PLANE_U8, "int16": J.capi.PLANE_I16, "float32": J.capi.PLANE_F32}[dtype]
        for c in range(3):
            spec.scale[c], spec.bias[c] = 1 / 255, -0.5
        sizes = [b.plane_size(0, c, res == "native") for c in comps]           # (h, w) per component, the same for every image
        per = [h * w * ELEM[dtype] for h, w in sizes]
        for c, nb in zip(comps, per):
            assert lib.jsnoop_batch_plane_bytes(b._h, C.byref(spec), 0, c) == nb
        m = n * len(comps)
        ind = (C.c_int * m)(*[i for i in range(n) for _ in comps])
        dst = (J.capi.PlaneDst * m)()
        off = 0
        for i in range(n):
            for k, c in enumerate(comps):
                dst[i * len(comps) + k] = J.capi.PlaneDst(big.data_ptr() + off, 0, c, 0)
                off += (per[k] + 15) // 16 * 16
        assert off <= big.numel()
        read = n * sum(h * a.width * 2 for h, _ in sizes)                      # whole source rows of the rows read
        written = n * sum(per)
        half = (read + written) // 2
        src_c, dst_c = big[:half], other[:half]

        def pack():
            assert lib.jsnoop_batch_pack_planes(b._h, C.byref(spec), ind, m, dst) == 0, J.last_error()

        def copy():
            with torch.cuda.stream(stream):
                dst_c.copy_(src_c, non_blocking=True)
        for _ in range(a.warmup):
            pack(); copy()
        stream.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(a.reps)]
        for e in ev:
            e[0].record(stream); pack(); e[1].record(stream)
            e[2].record(stream); copy(); e[3].record(stream)
        stream.synchronize()
        tp = [e[0].elapsed_time(e[1]) for e in ev]
        tc = [e[2].elapsed_time(e[3]) for e in ev]
        mp, mc = statistics.median(tp), statistics.median(tc)
        forms[name] = {
            "destinations": m, "bytes_read": read, "bytes_written": written, "copy_bytes_each_way": half,
            "call_ms_median": round(mp, 4), "call_ms_min": round(min(tp), 4), "copy_ms_median": round(mc, 4), "copy_ms_min": round(min(tc), 4),
            "call_tb_per_s": round((read + written) / mp / 1e9, 3), "copy_tb_per_s": round(2 * half / mc / 1e9, 3),
            "call_over_copy": round(mp / mc, 3)}
    # the way there was before: read_planes per image, then an upload
    hn = min(a.host_images, n)
    b.planes(0)                                                               # (the landing buffer and torch's allocator warm)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    keep = []
    for i in range(hn):
        keep.append([torch.from_numpy(p).to(dev) for p in b.planes(i)])
    torch.cuda.synchronize(dev)
    host_ms = (time.perf_counter() - t0) * 1e3
    out = {"tool": "tools/plane_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": min(a.distinct, n), "width": a.width, "height": a.height,
           "warmup": a.warmup, "reps": a.reps, "timing": "events on the batch stream, one launch per call; rates = (read + written) / median", "forms": forms,
           "host_path": {"images": hn, "what": "JpegBatch.planes(i) + upload of the three padded int16 planes, wall clock", "ms": round(host_ms, 2),
                         "ms_per_image": round(host_ms / max(hn, 1), 3)}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
