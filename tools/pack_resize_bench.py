"""jsnoop_batch_pack_resized against today's route to the same tensor, and against the plain pack of the same images.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box).  The batch is
decoded once.  Target: [N, 3, 224, 224] (--size).  Two ROI settings: the whole image, and a seeded list of random-resized-crop rectangles (area 8 % .. 100 %
of the picture, aspect 3/4 .. 4/3).  Per setting, per filter and for CHW float32 and HWC uint8:
  (a) the fused call: one jsnoop_batch_pack_resized into the stacked tensor;
  (b) today's route: to_torch(dtype=float32) of every image, then per image F.interpolate (bilinear / nearest-exact / area) on the slice, written into the
      stacked tensor (rounded to uint8 and permuted for the HWC uint8 form);
  (c) the plain jsnoop_batch_pack HWC uint8 of the same list: the figure for "read every DIB byte once".
Everything runs on the batch's stream and is timed by events on it: --warmup rounds, then --reps rounds of (a), (b), (c) in turn, each between its own two
events; median and minimum are reported.  Bytes: read = ROI pixels * 4, written = output elements * element size; rates are (read + written) / median.

Gate: (a) is faster than (b) in every row by more than the largest spread (max - min over the repetitions) of either form in that row; the tool fails otherwise.

Prints one JSON line; --out FILE also saves it (profiles/pack_resize_bench.json is a run of this tool).
usage: python tools/pack_resize_bench.py [--images 1024] [--distinct 64] [--size 224] [--warmup 5] [--reps 20] [--out FILE]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jpegsnoop_amd as J                                            # noqa: E402
from oracle import harness as H                                      # noqa: E402

FILTERS = [("bilinear", J.capi.RESIZE_BILINEAR, dict(mode="bilinear", align_corners=False, antialias=False)),
           ("nearest", J.capi.RESIZE_NEAREST, dict(mode="nearest-exact")), ("area", J.capi.RESIZE_AREA, dict(mode="area"))]


def random_resized_crops(n, w, h, seed):
    """(x, y, w, h) per image: area 8 % .. 100 % of the picture, log-uniform aspect 3/4 .. 4/3, ten tries, else the centre crop."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        for _ in range(10):
            area = w * h * rng.uniform(0.08, 1.0)
            ar = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
            cw, ch = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
            if 0 < cw <= w and 0 < ch <= h:
                out.append((int(rng.randint(0, w - cw + 1)), int(rng.randint(0, h - ch + 1)), cw, ch))
                break
        else:
            s = min(w, h)
            out.append(((w - s) // 2, (h - s) // 2, s, s))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=20261018)
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
    n, S, W, Hh = a.images, a.size, a.width, a.height
    ind = (C.c_int * n)(*range(n))
    plain = torch.empty((n, Hh, W, 3), dtype=torch.uint8, device=dev)
    plain_spec = J.capi.PackSpec(); lib.jsnoop_pack_spec_defaults(C.byref(plain_spec))
    plain_dst = (J.capi.PackDst * n)(*[J.capi.PackDst(plain[k].data_ptr(), 0, 0) for k in range(n)])
    rows = {}
    with torch.cuda.stream(stream):
        for roi_name, rois in (("whole", [(0, 0, W, Hh)] * n), ("random_resized_crop", random_resized_crops(n, W, Hh, a.seed))):
            read = 4 * sum(r[2] * r[3] for r in rois)
            for fname, fid, fkw in FILTERS:
                for layout, dtype, elem in (("CHW", torch.float32, 4), ("HWC", torch.uint8, 1)):
                    chw = layout == "CHW"
                    spec = J.capi.PackSpec(); lib.jsnoop_pack_spec_defaults(C.byref(spec))
                    spec.layout = J.capi.PACK_CHW if chw else J.capi.PACK_HWC
                    spec.dtype = J.capi.PACK_F32 if elem == 4 else J.capi.PACK_U8
                    fused = torch.empty((n, 3, S, S) if chw else (n, S, S, 3), dtype=dtype, device=dev)
                    today = torch.empty_like(fused)
                    dst = (J.capi.ResizeDst * n)(*[J.capi.ResizeDst(fused[k].data_ptr(), 0, 0, S, S, *rois[k]) for k in range(n)])
                    written = fused.numel() * elem

                    def run_a():
                        assert lib.jsnoop_batch_pack_resized(b._h, C.byref(spec), fid, ind, n, dst) == 0, J.last_error()

                    def run_b():
                        ts = b.to_torch(dtype=torch.float32)
                        for k, t in enumerate(ts):
                            x, y, w, h = rois[k]
                            r = F.interpolate(t[None, :, y:y + h, x:x + w], size=(S, S), **fkw)[0]
                            if chw:
                                today[k] = r
                            else:
                                today[k] = r.round().to(torch.uint8).permute(1, 2, 0)

                    def run_c():
                        assert lib.jsnoop_batch_pack(b._h, C.byref(plain_spec), ind, n, plain_dst) == 0, J.last_error()
                    for _ in range(a.warmup):
                        run_a(); run_b(); run_c()
                    stream.synchronize()
                    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(a.reps)]
                    for e in ev:
                        e[0].record(stream); run_a(); e[1].record(stream)
                        e[2].record(stream); run_b(); e[3].record(stream)
                        e[4].record(stream); run_c(); e[5].record(stream)
                    stream.synchronize()
                    ta, tb, tc = ([e[2 * j].elapsed_time(e[2 * j + 1]) for e in ev] for j in range(3))
                    ma, mb, mc = statistics.median(ta), statistics.median(tb), statistics.median(tc)
                    spread = max(max(ta) - min(ta), max(tb) - min(tb))
                    worst = float((fused.float() - today.float()).abs().max().item())
                    rows["%s_%s_%s_%s" % (roi_name, fname, layout, "float32" if elem == 4 else "uint8")] = {
                        "bytes_read": read, "bytes_written": written,
                        "fused_ms_median": round(ma, 4), "fused_ms_min": round(min(ta), 4), "today_ms_median": round(mb, 4), "today_ms_min": round(min(tb), 4),
                        "plain_pack_ms_median": round(mc, 4), "plain_pack_ms_min": round(min(tc), 4),
                        "fused_tb_per_s": round((read + written) / ma / 1e9, 3), "largest_spread_ms": round(spread, 4),
                        "today_over_fused": round(mb / ma, 2), "fused_over_plain_pack": round(ma / mc, 3),
                        "max_abs_difference_to_today": round(worst, 5), "gate_fused_faster_than_today_by_more_than_the_spread": bool(mb - ma > spread)}
                    del fused, today
    out = {"tool": "tools/pack_resize_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": min(a.distinct, n), "width": W, "height": Hh, "size": S,
           "warmup": a.warmup, "reps": a.reps, "seed": a.seed,
           "timing": "events on the batch stream; fused = one launch; today = to_torch(float32) + per-image F.interpolate; rates = (read + written) / median",
           "plain_pack_bytes": {"read": n * W * Hh * 4, "written": n * W * Hh * 3}, "rows": rows}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    b.close()
    failed = [k for k, v in rows.items() if not v["gate_fused_faster_than_today_by_more_than_the_spread"]]
    assert not failed, "the fused call is not faster than today's route by more than the spread in: %s" % ", ".join(failed)


if __name__ == "__main__":
    main()
