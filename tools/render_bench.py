"""jsnoop_batch_pack_ijg against jsnoop_batch_pack, jsnoop_encode_run, a plain device-to-device copy of the same traffic and the decode of the same batch.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box) -- decoded once.
Then, on one stream, --warmup rounds and --reps timed rounds in which one process alternates, each between its own two events:
  render          jsnoop_batch_pack_ijg of the whole batch into one HWC uint8 tensor (the span holds the call's host arithmetic, one H2D copy of the records
                  and k_render_ijg)
  pack            jsnoop_batch_pack of the whole batch into a tensor of the same shape
  encode          jsnoop_encode_run on the packed tensor at 4:2:0 q85: the inverse of the render's first half (the same block count, a transform of the same size)
  copy            hipMemcpyAsync device to device (a contiguous torch copy_) of (bytes read + bytes written) / 2 of the render
  decode          jsnoop_batch_decode of the same batch
Reported per form: median and minimum ms; for the render its rate over (bytes read + bytes written), its ratio to the copy and to encode + pack -- the aim is
that the render takes no longer than those two together.

Prints one JSON line; --out FILE also saves it (profiles/render_bench.json is a run of this tool).
usage: python tools/render_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--out FILE]"""
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
    n, distinct = a.images, min(a.distinct, a.images)
    b = J.JpegBatch(stream=stream.cuda_stream)
    for i in range(distinct):
        b.add_jpeg(H.synth_jpeg(width=a.width, height=a.height, hs=2, vs=2, quality=85, seed=i + 1))
    b.tile(n)
    b.upload(); b.decode(); b.sync()
    assert all(b.ijg_renderable(i) for i in range(n))
    with torch.cuda.stream(stream):
        pics = b.to_torch(layout="HWC", stack=True)                  # [n, H, W, 3] uint8: the pack's destination and the encode's source
        ijg = torch.empty_like(pics)                                 # the render's destination
    stream.synchronize()
    spec = J.capi.PackSpec(); lib.jsnoop_pack_spec_defaults(C.byref(spec)); spec.layout = J.capi.PACK_HWC; spec.dtype = J.capi.PACK_U8
    d_pack = (J.capi.PackDst * n)(*[J.capi.PackDst(pics[k].data_ptr(), 0, 0) for k in range(n)])
    d_ijg = (J.capi.PackDst * n)(*[J.capi.PackDst(ijg[k].data_ptr(), 0, 0) for k in range(n)])
    enc = J.JpegEncoder(device=0, stream=stream.cuda_stream)
    espec = J.capi.encode_spec(lib, quality=85, subsampling="4:2:0")
    src = (J.capi.EncodeSrc * n)()
    for k in range(n):
        src[k].ptr = pics[k].data_ptr(); src[k].width = a.width; src[k].height = a.height; src[k].channels = 3

    def render():
        assert lib.jsnoop_batch_pack_ijg(b._h, C.byref(spec), None, n, d_ijg) == 0, J.last_error()

    def pack():
        assert lib.jsnoop_batch_pack(b._h, C.byref(spec), None, n, d_pack) == 0, J.last_error()

    def encode():
        assert lib.jsnoop_encode_run(enc._h, C.byref(espec), src, n) == 0, J.last_error()

    blocks = sum(b.info(k)["total_blocks"] for k in range(n))
    read = blocks * 130; written = n * a.width * a.height * 3
    half = (read + written) // 2
    src_c = torch.empty(half, dtype=torch.uint8, device=dev); dst_c = torch.empty(half, dtype=torch.uint8, device=dev)

    def copy():
        with torch.cuda.stream(stream):
            dst_c.copy_(src_c, non_blocking=True)

    forms = [("render", render), ("pack", pack), ("encode", encode), ("copy", copy), ("decode", b.decode)]
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
    mr, mc = out_forms["render"]["ms_median"], out_forms["copy"]["ms_median"]
    budget = out_forms["encode"]["ms_median"] + out_forms["pack"]["ms_median"]
    out_forms["render"].update(tb_per_s=round((read + written) / mr / 1e9, 3), over_copy=round(mr / mc, 3), us_per_image=round(mr * 1000 / n, 3),
                               over_encode_plus_pack=round(mr / budget, 3), over_decode=round(mr / out_forms["decode"]["ms_median"], 3))
    out_forms["copy"].update(tb_per_s=round(2 * half / mc / 1e9, 3), bytes_each_way=half)
    differ = float((ijg[0] != pics[0]).float().mean().item())        # how far the two answers are apart on one picture of the bench
    out = {"tool": "tools/render_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": distinct, "width": a.width, "height": a.height,
           "warmup": a.warmup, "reps": a.reps, "blocks": blocks, "bytes_read": read, "bytes_written": written,
           "timing": "events on one stream around each call, the five forms alternating in one process",
           "aim": "render <= encode + pack", "aim_met": bool(mr <= budget), "encode_plus_pack_ms_median": round(budget, 4),
           "bytes_that_differ_between_the_two_pixel_kinds_image_0": round(differ, 4), "forms": out_forms}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    enc.close(); b.close()


if __name__ == "__main__":
    main()
