"""jsnoop_batch_pack_ijg_scaled at 1/2, 1/4, 1/8 against the full-size jsnoop_batch_pack_ijg, against today's way to a small picture (jsnoop_batch_pack_resized
with the area filter from the DIB), against a plain device-to-device copy of each scaled form's traffic, and against the decode of the same batch.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box) -- decoded once.
Then, on one stream, --warmup rounds and --reps timed rounds in which one process alternates, each form between its own two events:
  scaled_2 / _4 / _8   jsnoop_batch_pack_ijg_scaled of the whole batch into one HWC uint8 tensor of the reduced size (the span holds the call's host
                       arithmetic, one H2D copy of the records and k_render_ijg_scaled)
  full                 jsnoop_batch_pack_ijg of the whole batch at full size
  resized_2 / _4 / _8  jsnoop_batch_pack_resized, area filter, of the DIB to the same sizes
  copy_2 / _4 / _8     hipMemcpyAsync device to device (a contiguous torch copy_) of (bytes read + bytes written) / 2 of the scaled form
  decode               jsnoop_batch_decode of the same batch
Bytes read of a scaled form are the 16-byte arena segments its transforms fetch (8 of a block at 8 x 8, 7 at 4 x 4, 5 at 2 x 2, none at 1 x 1) plus two bytes
of dccum a block; bytes written are its pixels.  Reported per form: median and minimum ms; for every scaled form its ratio to the full-size render (the
expectation: below 1), to its copy and to the resize.  No time is fixed in advance.

Prints one JSON line; --out FILE also saves it (profiles/render_scaled_bench.json is a run of this tool).
usage: python tools/render_scaled_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--out FILE]"""
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

SEGMENTS = {8: 8, 4: 7, 2: 5, 1: 0}                                  # 16-byte arena segments a transform of that size fetches of a block


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
    assert all(b.ijg_renderable(i) for i in range(n))
    spec = J.capi.PackSpec(); lib.jsnoop_pack_spec_defaults(C.byref(spec)); spec.layout = J.capi.PACK_HWC; spec.dtype = J.capi.PACK_U8
    mcus = sum(b.info(k)["mcu_xmax"] * b.info(k)["mcu_ymax"] for k in range(n))
    forms, traffic, keep = [], {}, []
    with torch.cuda.stream(stream):
        full = torch.empty((n, a.height, a.width, 3), dtype=torch.uint8, device=dev)
    d_full = (J.capi.PackDst * n)(*[J.capi.PackDst(full[k].data_ptr(), 0, 0) for k in range(n)])
    for s in (2, 4, 8):
        h, w = b.ijg_scaled_size(0, s)
        with torch.cuda.stream(stream):
            t = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev); r = torch.empty_like(t)
        d_s = (J.capi.PackDst * n)(*[J.capi.PackDst(t[k].data_ptr(), 0, 0) for k in range(n)])
        d_r = (J.capi.ResizeDst * n)(*[J.capi.ResizeDst(r[k].data_ptr(), 0, 0, w, h, 0, 0, 0, 0) for k in range(n)])
        m = 8 // s
        read = mcus * (4 * (16 * SEGMENTS[m] + 2) + 2 * (16 * SEGMENTS[2 * m] + 2)); written = n * h * w * 3
        half = (read + written) // 2
        src_c = torch.empty(half, dtype=torch.uint8, device=dev); dst_c = torch.empty(half, dtype=torch.uint8, device=dev)
        keep += [t, r, d_s, d_r, src_c, dst_c]
        traffic[s] = dict(read=read, written=written, half=half, h=h, w=w, resized_read=n * a.width * a.height * 3)

        def scaled(s=s, d_s=d_s):
            assert lib.jsnoop_batch_pack_ijg_scaled(b._h, C.byref(spec), s, None, n, d_s) == 0, J.last_error()

        def resized(d_r=d_r):
            assert lib.jsnoop_batch_pack_resized(b._h, C.byref(spec), J.capi.RESIZE_AREA, None, n, d_r) == 0, J.last_error()

        def copy(src_c=src_c, dst_c=dst_c):
            with torch.cuda.stream(stream):
                dst_c.copy_(src_c, non_blocking=True)

        forms += [("scaled_%d" % s, scaled), ("resized_%d" % s, resized), ("copy_%d" % s, copy)]

    def render_full():
        assert lib.jsnoop_batch_pack_ijg(b._h, C.byref(spec), None, n, d_full) == 0, J.last_error()

    forms += [("full", render_full), ("decode", b.decode)]
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
        t = [row[k][0].elapsed_time(row[k][1]) for row in ev]
        out_forms[name] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4)}
    blocks = sum(b.info(k)["total_blocks"] for k in range(n))
    mf = out_forms["full"]["ms_median"]
    out_forms["full"].update(bytes_read=blocks * 130, bytes_written=n * a.width * a.height * 3)
    for s in (2, 4, 8):
        tr = traffic[s]; ms = out_forms["scaled_%d" % s]["ms_median"]; mc = out_forms["copy_%d" % s]["ms_median"]; mr = out_forms["resized_%d" % s]["ms_median"]
        out_forms["scaled_%d" % s].update(bytes_read=tr["read"], bytes_written=tr["written"], out_h=tr["h"], out_w=tr["w"], tb_per_s=round((tr["read"] + tr["written"]) / ms / 1e9, 3),
                                          over_full=round(ms / mf, 3), over_copy=round(ms / mc, 3), over_resized=round(ms / mr, 3), us_per_image=round(ms * 1000 / n, 3))
        out_forms["resized_%d" % s].update(bytes_read=tr["resized_read"], bytes_written=tr["written"])
        out_forms["copy_%d" % s].update(bytes_each_way=tr["half"], tb_per_s=round(2 * tr["half"] / mc / 1e9, 3))
    out = {"tool": "tools/render_scaled_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": distinct, "width": a.width, "height": a.height,
           "warmup": a.warmup, "reps": a.reps, "blocks": blocks,
           "timing": "events on one stream around each call, the eleven forms alternating in one process",
           "expectation": "every scaled form takes less than the full-size render of the same process",
           "expectation_met": {str(s): bool(out_forms["scaled_%d" % s]["ms_median"] < mf) for s in (2, 4, 8)}, "forms": out_forms}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    b.close()


if __name__ == "__main__":
    main()
