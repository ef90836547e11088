"""jsnoop_batch_pack against a plain device-to-device copy of the same traffic.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box).  The batch
is decoded once; then every form (HWC / CHW x uint8 / float32) packs all images into one dense allocation, timed by events on the batch's stream:
--warmup packs, then --reps pairs of (pack, copy), each between its own two events; median and minimum are reported.

Yardstick: hipMemcpyAsync device to device (a contiguous torch copy_ on the same stream), in the same process, moving the same total traffic: the pack
reads dim_x * dim_y * 4 bytes and writes dim_x * dim_y * 3 * elem bytes per image, the copy moves (read + written) / 2 bytes, so its read plus its
write equals the pack's.  Rates are (bytes read + bytes written) / time.

Prints one JSON line; --out FILE also saves it (profiles/pack_bench.json is a run of this tool).
usage: python tools/pack_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

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
    n, px = a.images, a.width * a.height
    read = n * px * 4
    big = torch.empty(n * px * 12, dtype=torch.uint8, device=dev)           # the largest form's output; the copy's source
    other = torch.empty((read + n * px * 12) // 2, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ind = (C.c_int * n)(*range(n))
    forms = {}
    for layout in ("HWC", "CHW"):
        for dtype, elem in (("uint8", 1), ("float32", 4)):
            spec = J.capi.PackSpec(); lib.jsnoop_pack_spec_defaults(C.byref(spec))
            spec.layout = J.capi.PACK_CHW if layout == "CHW" else J.capi.PACK_HWC
            spec.dtype = J.capi.PACK_F32 if elem == 4 else J.capi.PACK_U8
            for c in range(3):
                spec.scale[c], spec.bias[c] = 1 / 255, -0.5
            per = px * 3 * elem
            assert lib.jsnoop_batch_pack_bytes(b._h, C.byref(spec), 0) == per
            dst = (J.capi.PackDst * n)(*[J.capi.PackDst(big.data_ptr() + i * per, 0, 0) for i in range(n)])
            written = n * per
            half = (read + written) // 2
            src_c, dst_c = big[:half], other[:half]

            def pack():
                assert lib.jsnoop_batch_pack(b._h, C.byref(spec), ind, n, dst) == 0, J.last_error()

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
            forms["%s_%s" % (layout, dtype)] = {
                "bytes_read": read, "bytes_written": written, "copy_bytes_each_way": half,
                "pack_ms_median": round(mp, 4), "pack_ms_min": round(min(tp), 4), "copy_ms_median": round(mc, 4), "copy_ms_min": round(min(tc), 4),
                "pack_tb_per_s": round((read + written) / mp / 1e9, 3), "copy_tb_per_s": round(2 * half / mc / 1e9, 3),
                "pack_over_copy": round(mp / mc, 3)}
    out = {"tool": "tools/pack_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": min(a.distinct, n), "width": a.width, "height": a.height,
           "warmup": a.warmup, "reps": a.reps, "timing": "events on the batch stream, one launch per pack; rates = (read + written) / median", "forms": forms}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
