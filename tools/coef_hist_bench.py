"""jsnoop_batch_pack_coef_hist against a plain device-to-device copy of the same traffic, against the cheapest way to the same rows with the other doors
(jsnoop_batch_pack_coefs FREQ / I16 and torch histogramming of its tensors), against the host path, and on two adversarial inputs.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box).  The batch is
decoded once; then every form (R = 127 and 16, quantised levels and arena values) turns all three components of all images into rows in ONE call, timed by
events on the batch's stream: --warmup rounds, then --reps rounds of (call, yardstick, pack_coefs), each between its own two events, alternating in one
process; median and minimum are reported.

Yardsticks.  (1) hipMemcpyAsync device to device (a contiguous torch copy_ on the same stream) moving (read + written) / 2 bytes: the call reads 130 bytes
per block (128 of the arena, 2 of the cumulative DC) and writes its rows.  (2) jsnoop_batch_pack_coefs FREQ / I16 / NATURAL of the same destinations into
one dense allocation, then torch histogramming of those tensors (divide, clamp, one bincount per destination; min / max per frequency) over --torch-images
images, scaled to the batch.  The door exists only if the call beats the pack_coefs step ALONE: `margin_over_pack_coefs` must be above 1.
(3) The host path: jsnoop_batch_read_coefs per image and tests/coef_hist_model.py in numpy over --host-images images, scaled.

Adversarial inputs, --adv-images pictures each, next to natural pictures of the same count: flat (every AC zero: the skip path) and quality-100 noise of small
amplitude (most coefficients +-1 and +-2: many lanes add to the same few LDS words).

Prints one JSON line; --out FILE also saves it (profiles/coef_hist_bench.json is a run of this tool).
--counters is the workload of a profiler pass (profiles/coef_hist_counters.txt: rocprofv3 --pmc alone, one group, 256 images): three calls per range, no timing.
usage: python tools/coef_hist_bench.py [--images 1024] [--distinct 64] [--adv-images 256] [--warmup 5] [--reps 20] [--torch-images 64] [--host-images 64] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpegsnoop_amd as J                                            # noqa: E402
from oracle import harness as H                                      # noqa: E402
import coef_model as M                                               # noqa: E402
import coef_hist_model as HM                                         # noqa: E402

FORMS = [(127, True), (16, True), (127, False), (16, False)]


def hist_spec(lib, R, quantised):
    s = J.capi.CoefHistSpec(); lib.jsnoop_coef_hist_spec_defaults(C.byref(s))
    s.range, s.quantised = R, int(quantised)
    return s


def timed(stream, fns, warmup, reps):
    """fns in turn, `reps` rounds behind `warmup` untimed ones, each call between its own two events on `stream`; [[ms] per fn]."""
    for _ in range(warmup):
        for f in fns:
            f()
    stream.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(reps)]
    for row in ev:
        for f, (e0, e1) in zip(fns, row):
            e0.record(stream); f(); e1.record(stream)
    stream.synchronize()
    return [[row[k][0].elapsed_time(row[k][1]) for row in ev] for k in range(len(fns))]


def batch_of(files, n, stream):
    b = J.JpegBatch(stream=stream.cuda_stream)
    for f in files:
        b.add_jpeg(f)
    b.tile(n)
    b.upload(); b.decode(); b.sync()
    return b


def hist_call(lib, b, n, R, quantised, rows):
    spec = hist_spec(lib, R, quantised)
    ind = (C.c_int * (3 * n))(*[i for i in range(n) for _ in range(3)]); cs = (C.c_int * (3 * n))(*[c for _ in range(n) for c in range(3)])

    def call():
        assert lib.jsnoop_batch_pack_coef_hist(b._h, C.byref(spec), ind, cs, 3 * n, rows.data_ptr(), 0) == 0, J.last_error()
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--adv-images", type=int, default=256)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-images", type=int, default=64)
    ap.add_argument("--host-images", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--counters", action="store_true", help="profiler runs: decode --images pictures, three calls with R = 127, then three with R = 16 (quantised), nothing else")
    a = ap.parse_args()
    assert a.counters or (a.warmup >= 5 and a.reps >= 20), "at least 5 warm-ups and 20 repetitions"
    H.build(["synth"])
    lib = J.load()
    dev = torch.device("cuda", 0)
    assert lib.jsnoop_set_device(0) == 0, J.last_error()
    stream = torch.cuda.Stream(dev)
    n = a.images
    natural = [H.synth_jpeg(width=a.width, height=a.height, hs=2, vs=2, quality=85, seed=i + 1) for i in range(min(a.distinct, n))]
    b = batch_of(natural, n, stream)
    grids = [b.coef_grid(0, c) for c in range(3)]
    blocks = sum(bw * bh for bw, bh in grids)
    assert blocks == b.info(0)["total_blocks"]
    if a.counters:
        for R in (127, 16):
            rows = torch.empty((3 * n, J.capi.coef_hist_words(R)), dtype=torch.int32, device=dev)
            call = hist_call(lib, b, n, R, True, rows)
            for _ in range(3):
                call()
            stream.synchronize()
        b.close()
        return
    read = n * blocks * 130
    tensors = torch.empty(n * blocks * 64, dtype=torch.int16, device=dev)          # pack_coefs FREQ / I16 of every destination, dense; also the copy's source
    other = torch.empty(n * blocks * 128, dtype=torch.uint8, device=dev)
    cspec = J.capi.CoefSpec(); lib.jsnoop_coef_spec_defaults(C.byref(cspec)); cspec.layout = J.capi.COEF_FREQ
    cdst = (J.capi.CoefDst * (3 * n))(); cind = (C.c_int * (3 * n))(*[i for i in range(n) for _ in range(3)])
    offs, pos = [], 0
    for i in range(n):
        for c in range(3):
            d = cdst[3 * i + c]; d.ptr, d.row_pitch, d.plane_pitch, d.comp, d.reserved = tensors.data_ptr() + pos * 2, 0, 0, c, 0
            offs.append(pos); pos += grids[c][0] * grids[c][1] * 64

    def pack_coefs():
        assert lib.jsnoop_batch_pack_coefs(b._h, C.byref(cspec), cind, 3 * n, cdst) == 0, J.last_error()

    forms = {}
    for R, quantised in FORMS:
        words = J.capi.coef_hist_words(R)
        rows = torch.empty((3 * n, words), dtype=torch.int32, device=dev)
        written = 3 * n * words * 4
        half = (read + written) // 2
        src_c, dst_c = tensors.view(torch.uint8)[:half], other[:half]

        def copy():
            with torch.cuda.stream(stream):
                dst_c.copy_(src_c, non_blocking=True)
        th, tc, tp = timed(stream, [hist_call(lib, b, n, R, quantised, rows), copy, pack_coefs], a.warmup, a.reps)
        mh, mc, mp = statistics.median(th), statistics.median(tc), statistics.median(tp)
        forms["R%d_%s" % (R, "levels" if quantised else "values")] = {
            "bytes_read": read, "bytes_written": written, "copy_bytes_each_way": half,
            "hist_ms_median": round(mh, 4), "hist_ms_min": round(min(th), 4), "copy_ms_median": round(mc, 4), "copy_ms_min": round(min(tc), 4),
            "pack_coefs_freq_i16_ms_median": round(mp, 4), "pack_coefs_freq_i16_ms_min": round(min(tp), 4),
            "hist_tb_per_s": round((read + written) / mh / 1e9, 3), "copy_tb_per_s": round(2 * half / mc / 1e9, 3),
            "hist_over_copy": round(mh / mc, 3), "margin_over_pack_coefs": round(mp / mh, 3)}
        del rows
    # torch histogramming of pack_coefs' tensors (R = 127, quantised), over the first images, scaled
    tn = max(1, min(a.torch_images, n)); R = 127; nb = 2 * R + 1
    q = [torch.from_numpy(np.maximum(b.dqt(0, c).astype(np.int32), 1)).to(dev) for c in range(3)]
    trow = torch.empty((3 * tn, J.capi.coef_hist_words(R)), dtype=torch.int32, device=dev)
    fidx = [torch.arange(64, device=dev, dtype=torch.int64).repeat_interleave(grids[c][0] * grids[c][1]) * nb + R for c in range(3)]

    def torch_hist():
        with torch.cuda.stream(stream):
            for k in range(3 * tn):
                c = k % 3; per = grids[c][0] * grids[c][1]
                t = tensors[offs[k]:offs[k] + per * 64].view(64, per).to(torch.int32)
                x = torch.div(t, q[c][:, None], rounding_mode="trunc")
                trow[k, :64 * nb] = torch.bincount((x.clamp(-R, R).view(-1).to(torch.int64) + fidx[c]), minlength=64 * nb)
                trow[k, 64 * nb:64 * nb + 64] = x.amin(1); trow[k, 64 * nb + 64:] = x.amax(1)
    pack_coefs()
    (tt,) = timed(stream, [torch_hist], a.warmup, a.reps)
    check = torch.empty((3 * tn, J.capi.coef_hist_words(R)), dtype=torch.int32, device=dev)
    hist_call(lib, b, tn, R, True, check)(); stream.synchronize()
    same = bool(torch.equal(check, trow))
    mt = statistics.median(tt)
    torch_path = {"images_timed": tn, "torch_hist_ms_median": round(mt, 3), "scaled_to_batch_ms": round(mt / tn * n, 1), "rows_equal_the_calls": same, "form": "R127_levels"}
    del tensors, other
    # the host path: D2H of the raw arena, then the numpy model
    hn = max(1, min(a.host_images, n))
    geo = M.Geometry([(2, 2), (1, 1), (1, 1)], grids[1][0], grids[1][1])
    dq = [b.dqt(0, c) for c in range(3)]
    t0 = time.perf_counter()
    arenas = [b.coefs(i) for i in range(hn)]
    t1 = time.perf_counter()
    for arena in arenas:
        cum = M.running_dc(arena, geo, 0)
        for c in range(3):
            HM.row(arena, cum, geo, c, dq[c], 127)
    t2 = time.perf_counter()
    host = {"images_timed": hn, "read_coefs_ms_per_image": round((t1 - t0) * 1e3 / hn, 3), "numpy_model_ms_per_image": round((t2 - t1) * 1e3 / hn, 3),
            "scaled_to_batch_ms": round((t2 - t0) * 1e3 / hn * n, 1), "form": "R127_levels"}
    del arenas
    b.close()
    # adversarial inputs next to natural pictures of the same count
    an = max(1, min(a.adv_images, n)); rng = np.random.default_rng(7)
    flat = [H.encode_rgb(np.broadcast_to(rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), (a.height, a.width, 3)).copy(), hs=2, vs=2, quality=85) for _ in range(4)]
    noise = [H.encode_rgb(np.clip(128 + rng.normal(0, 1.6, (a.height, a.width, 3)), 0, 255).astype(np.uint8), hs=2, vs=2, quality=100) for _ in range(4)]
    adv = {"images": an}
    for name, files in (("natural", natural[:16]), ("flat", flat), ("noise_q100", noise)):
        bb = batch_of(files, an, stream)
        arena = bb.coefs(0)
        adv[name] = {"nonzero_ac_fraction": round(float((arena[:, 1:] != 0).mean()), 4), "abs_1_or_2_fraction": round(float(((np.abs(arena[:, 1:]) >= 1) & (np.abs(arena[:, 1:]) <= 2)).mean()), 4)}
        for R in (127, 16):
            rows = torch.empty((3 * an, J.capi.coef_hist_words(R)), dtype=torch.int32, device=dev)
            (t,) = timed(stream, [hist_call(lib, bb, an, R, True, rows)], a.warmup, a.reps)
            adv[name]["R%d_levels_ms_median" % R] = round(statistics.median(t), 4); adv[name]["R%d_levels_ms_min" % R] = round(min(t), 4)
            del rows
        bb.close()
    for name in ("flat", "noise_q100"):
        for R in (127, 16):
            adv[name]["R%d_ratio_to_natural" % R] = round(adv[name]["R%d_levels_ms_median" % R] / adv["natural"]["R%d_levels_ms_median" % R], 3)
    out = {"tool": "tools/coef_hist_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": min(a.distinct, n), "width": a.width, "height": a.height,
           "blocks_per_image": blocks, "unit": J.capi.COEF_HIST_UNIT, "warmup": a.warmup, "reps": a.reps,
           "timing": "events on the batch stream, one launch per call (all three components of all images) behind the rows' initialisation; call, copy and pack_coefs alternate in one process",
           "hard_condition": "margin_over_pack_coefs > 1 in every form", "aim": "at most 1.3 x the copy", "forms": forms, "torch_path": torch_path, "host_path": host, "adversarial": adv}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
