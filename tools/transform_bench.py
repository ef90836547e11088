"""jsnoop_transform_run against a plain device-to-device copy of the same traffic and the decode of the same batch.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box) -- decoded once.
1080 is not a multiple of 16: the ops that reverse y (ROT_180, ROT_90 here) run under EDGE_TRIM at 1072 rows, the others move all 68 MCU rows.  Then, on
one stream, --warmup rounds and --reps timed rounds in which one process alternates, each between its own two events:
  none, flip_h, rot180, transpose, rot90   jsnoop_transform_run alone, all images, into one transform object on the batch's stream (the span holds the
                  call's host arithmetic, one H2D copy of the records and k_transform)
  copy            hipMemcpyAsync device to device (a contiguous torch copy_) of the bytes the NONE form reads plus writes, halved, so its read plus its
                  write equals that form's (130 bytes a block each way: the arena row and the cumulative DC)
  decode          jsnoop_batch_decode of the same batch
Reported per form: median and minimum ms; for the transforms their rate over (bytes read + bytes written) of their own block count and their ratio to the
copy scaled to that count.

Prints one JSON line; --out FILE also saves it (profiles/transform_bench.json is a run of this tool).
usage: python tools/transform_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--out FILE]"""
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

OPS = ["none", "flip_h", "rot180", "transpose", "rot90"]


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
    n, distinct = a.images, min(a.distinct, a.images)
    b = J.JpegBatch(stream=stream.cuda_stream)
    for i in range(distinct):
        b.add_jpeg(H.synth_jpeg(width=a.width, height=a.height, hs=2, vs=2, quality=85, seed=i + 1))
    b.tile(n)
    b.upload(); b.decode(); b.sync()
    t = J.JpegTransform(device=0, stream=stream.cuda_stream)
    specs = {op: J.capi.transform_spec(lib, op) for op in OPS}
    ind = (C.c_int * n)(*range(n))

    def run(op):
        def go():
            assert lib.jsnoop_transform_run(t._h, b._h, C.byref(specs[op]), ind, n) == 0, J.last_error()
        return go

    blocks = {}
    for op in OPS:                                                   # (also grows the object's arena to its largest size before anything is timed)
        run(op)()
        assert all(e["result"] == 0 for e in t.entries()), "every picture of the bench is written"
        blocks[op] = sum(t.info(k)["total_blocks"] for k in range(n))
    half = blocks["none"] * 130
    src_c = torch.empty(half, dtype=torch.uint8, device=dev); dst_c = torch.empty(half, dtype=torch.uint8, device=dev)

    def copy():
        with torch.cuda.stream(stream):
            dst_c.copy_(src_c, non_blocking=True)

    forms = [(op, run(op)) for op in OPS] + [("copy", copy), ("decode", b.decode)]
    for _ in range(a.warmup):
        for _name, fn in forms:
            fn()
    stream.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in forms] for _ in range(a.reps)]
    for row in ev:
        for (e0, e1), (_name, fn) in zip(row, forms):
            e0.record(stream); fn(); e1.record(stream)
    stream.synchronize(); b.sync()
    out_forms = {}
    for k, (name, _fn) in enumerate(forms):
        ts = [row[k][0].elapsed_time(row[k][1]) for row in ev]
        out_forms[name] = {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4)}
    mc = out_forms["copy"]["ms_median"]
    out_forms["copy"].update(tb_per_s=round(2 * half / mc / 1e9, 3), bytes_each_way=half)
    for op in OPS:
        m = out_forms[op]["ms_median"]; traffic = blocks[op] * 260
        out_forms[op].update(blocks=blocks[op], tb_per_s=round(traffic / m / 1e9, 3), over_copy=round(m / (mc * blocks[op] / blocks["none"]), 3),
                             us_per_image=round(m * 1000 / n, 3), over_decode=round(m / out_forms["decode"]["ms_median"], 3))
    out = {"tool": "tools/transform_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": distinct, "width": a.width, "height": a.height,
           "subsampling": "4:2:0", "edge": "trim", "warmup": a.warmup, "reps": a.reps,
           "timing": "events on one stream around each call, the seven forms alternating in one process; over_copy: against the copy scaled to the form's own block count",
           "forms": out_forms}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    t.close(); b.close()


if __name__ == "__main__":
    main()
