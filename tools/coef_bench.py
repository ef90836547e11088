"""jsnoop_batch_pack_coefs against a plain device-to-device copy of the same traffic, and against what the same tensors cost on the host.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box).  The batch
is decoded once; then every form (BLOCKS / FREQ x int16 / float32 x natural / zig-zag) packs all three components of all images into one dense
allocation in ONE call, timed by events on the batch's stream: --warmup calls, then --reps pairs of (call, copy), each between its own two events;
median and minimum are reported.

Yardstick: hipMemcpyAsync device to device (a contiguous torch copy_ on the same stream), in the same process, moving the same total traffic: the call
reads 130 bytes per block (128 of the arena, 2 of the cumulative DC) and writes 64 * elem, the copy moves (read + written) / 2 bytes, so its read plus
its write equals the call's.  Rates are (bytes read + bytes written) / time.

Host path: what a consumer does today -- jsnoop_batch_read_coefs per image (the D2H copy of the raw arena) and the block shuffle, the predictor sum and
the transposition in numpy (tests/coef_model.py) -- timed with the wall clock over --host-images images and scaled to the batch.

Prints one JSON line; --out FILE also saves it (profiles/coef_bench.json is a run of this tool).
usage: python tools/coef_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--host-images 64] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpegsnoop_amd as J                                            # noqa: E402
from oracle import harness as H                                      # noqa: E402
import coef_model as M                                               # noqa: E402


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
    grids = [b.coef_grid(0, c) for c in range(3)]
    blocks = sum(bw * bh for bw, bh in grids)
    assert blocks == b.info(0)["total_blocks"]
    read = n * blocks * 130
    big = torch.empty(n * blocks * 256, dtype=torch.uint8, device=dev)           # the largest form's output; the copy's source
    other = torch.empty((read + n * blocks * 256) // 2, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ind = (C.c_int * (3 * n))(*[i for i in range(n) for _ in range(3)])
    forms = {}
    for layout in ("BLOCKS", "FREQ"):
        for dtype, elem in (("I16", 2), ("F32", 4)):
            for order in ("NATURAL", "ZIGZAG"):
                spec = J.capi.CoefSpec(); lib.jsnoop_coef_spec_defaults(C.byref(spec))
                spec.layout = getattr(J.capi, "COEF_" + layout); spec.dtype = getattr(J.capi, "COEF_" + dtype); spec.order = getattr(J.capi, "COEF_" + order)
                dst = (J.capi.CoefDst * (3 * n))()
                pos = big.data_ptr()
                for i in range(n):
                    for c in range(3):
                        per = grids[c][0] * grids[c][1] * 64 * elem
                        if i == 0:
                            assert lib.jsnoop_batch_coef_bytes(b._h, C.byref(spec), 0, c) == per
                        d = dst[3 * i + c]; d.ptr, d.row_pitch, d.plane_pitch, d.comp, d.reserved = pos, 0, 0, c, 0
                        pos += per
                written = n * blocks * 64 * elem
                half = (read + written) // 2
                src_c, dst_c = big[:half], other[:half]

                def pack():
                    assert lib.jsnoop_batch_pack_coefs(b._h, C.byref(spec), ind, 3 * n, dst) == 0, J.last_error()

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
                forms["%s_%s_%s" % (layout, dtype, order)] = {
                    "bytes_read": read, "bytes_written": written, "copy_bytes_each_way": half,
                    "pack_ms_median": round(mp, 4), "pack_ms_min": round(min(tp), 4), "copy_ms_median": round(mc, 4), "copy_ms_min": round(min(tc), 4),
                    "pack_tb_per_s": round((read + written) / mp / 1e9, 3), "copy_tb_per_s": round(2 * half / mc / 1e9, 3),
                    "pack_over_copy": round(mp / mc, 3)}
    del big, other
    # the host path: D2H of the raw arena, then shuffle + predictor sum + transposition in numpy
    hn = max(1, min(a.host_images, n))
    geo = M.Geometry([(2, 2), (1, 1), (1, 1)], grids[1][0], grids[1][1])
    t0 = time.perf_counter()
    arenas = [b.coefs(i) for i in range(hn)]
    t1 = time.perf_counter()
    for arena in arenas:
        cum = M.running_dc(arena, geo, 0)
        for c in range(3):
            M.coef_tensor(arena, cum, geo, c, "freq", "int16", False)
    t2 = time.perf_counter()
    host = {"images_timed": hn, "read_coefs_ms_per_image": round((t1 - t0) * 1e3 / hn, 3), "numpy_model_ms_per_image": round((t2 - t1) * 1e3 / hn, 3),
            "scaled_to_batch_ms": round((t2 - t0) * 1e3 / hn * n, 1), "form": "FREQ_I16_NATURAL"}
    out = {"tool": "tools/coef_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": min(a.distinct, n), "width": a.width, "height": a.height,
           "blocks_per_image": blocks, "tile": J.capi.COEF_TILE, "warmup": a.warmup, "reps": a.reps,
           "timing": "events on the batch stream, one launch per call (all three components of all images); rates = (read + written) / median",
           "aim": "BLOCKS_I16_NATURAL at most 1.3 x the copy", "forms": forms, "host_path": host}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
