"""jsnoop_batch_pack_stats against today's route -- a loop of jsnoop_batch_color_stats over the same images -- and against a plain device-to-device copy.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box), decoded once with
want_planes.  Per histo_en (1: records and histograms, 0: only the clip counters) three forms alternate in one process, each between its own two events on
the batch's stream: the ONE call for all images; the loop of per-image calls (its host round trips are what it costs, so they are inside the events); the
yardstick of DESIGN.md 4.7, a device-to-device copy that moves half the bytes the call reads (its read plus its write equal the call's read).  --warmup
rounds, then --reps rounds; median, minimum and spread (max - min) are reported.  A loop pass that takes longer than --loop-budget-s makes the tool cut the
loop's repetitions (never the call's) so that the run ends; the JSON says how many were made.

The same for a FLAT set -- every pixel of a picture one colour, the worst case for histogram-bin conflicts (--flat-distinct pictures tiled) -- and for two
single pictures whose 11 range events all lie in the first and in the last picture row (the second launch, k_stats_order, against k_clip_order).

Also: what the planes cost the decode -- one batch with want_planes and one without, decoded in turn, events on each batch's stream.

Gate: the one call is faster than the loop in every row by more than the largest spread of either form.  Prints one JSON line; --out FILE also saves it
(profiles/stats_bench.json is a run of this tool).  --counters: only the one call, three times per histo_en on --images images, for a counter pass of a
profiler in a run of its own.
usage: python tools/stats_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--out FILE] [--counters]"""
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
import stats_cases as SC                                             # noqa: E402

WORDS = J.capi.STATS_WORDS


def flat_picture(width, height, k):
    """4:2:0, every block of a component at one level (all DC, quantiser 1): every pixel of the picture is one colour."""
    fr = SC.frame_of("420", width, height)
    lv = [(-700 + 173 * k) % 1800 - 900, (311 * k) % 1400 - 700, (-197 * k) % 1400 - 700]
    return SC.Case("flat_%d" % k, "bench", "420", width, height, [np.full(fr.grid(c), lv[c], np.int64) for c in range(3)]).file


def events_picture(width, height, row):
    """4:2:0, grey, 11 single samples of picture row `row` (of the MCU-padded picture) out of range."""
    fr = SC.frame_of("420", width, height)
    peaks = [(0, row // 8, (97 * k + 5) % (width // 8), row % 8, (3 * k) % 8, SC.HIGH) for k in range(11)]
    return SC.Case("events_row_%d" % row, "bench", "420", width, height, [np.zeros(fr.grid(c), np.int64) for c in range(3)], peaks=peaks).file


def decoded(files, total, stream, want_planes=True):
    b = J.JpegBatch(stream=stream.cuda_stream, want_planes=want_planes)
    for f in files:
        b.add_jpeg(f)
    if total > len(files):
        b.tile(total)
    b.upload(); b.decode(); b.sync()
    return b


def timed(stream, forms, warmup, reps, budget_s):
    """forms: {name: callable}, alternating; returns {name: [ms]}.  A form whose single pass exceeds budget_s / reps gets fewer repetitions (at least 3)."""
    each = {}
    for name, fn in forms.items():                                   # one pass each, timed with the wall clock: the first warm-up, and the size of the job
        stream.synchronize(); t0 = time.perf_counter(); fn(); stream.synchronize(); each[name] = time.perf_counter() - t0
    nrep = {name: reps if each[name] * (reps + warmup) <= budget_s else max(3, int(budget_s / each[name]) - 1) for name in forms}
    for w in range(warmup - 1):
        for name, fn in forms.items():
            if w < nrep[name]:
                fn()
    stream.synchronize()
    out = {name: [] for name in forms}
    for r in range(reps):
        evs = {}
        for name, fn in forms.items():
            if r >= nrep[name]:
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream); evs[name] = (e0, e1)
        stream.synchronize()
        for name, (e0, e1) in evs.items():
            out[name].append(e0.elapsed_time(e1))
    return out


def summary(ms):
    return {"reps": len(ms), "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_spread": round(max(ms) - min(ms), 4)}


def stats_rows(lib, b, n, stream, dev, warmup, reps, budget_s, copy=True):
    """One row of the result per histo_en for batch b."""
    rows = torch.empty((n, WORDS), dtype=torch.int32, device=dev)
    host = np.zeros(WORDS, np.uint32)
    read = sum(b.info(i)["blk_xmax"] * 8 * b.info(i)["blk_ymax"] * 8 * (3 if b.info(i)["ncomp"] == 3 else 1) * 2 for i in range(min(n, 1))) * n   # (tiled: every image has image 0's geometry)
    half = read // 2
    src = torch.empty(half, dtype=torch.uint8, device=dev) if copy else None
    dst = torch.empty(half, dtype=torch.uint8, device=dev) if copy else None
    out = {}
    for histo_en in (1, 0):
        def call():
            assert lib.jsnoop_batch_pack_stats(b._h, histo_en, None, n, rows.data_ptr(), 0, None) == 0, J.last_error()

        def loop():
            for i in range(n):
                assert lib.jsnoop_batch_color_stats(b._h, i, histo_en, host.ctypes.data) == 0, J.last_error()

        def cp():
            with torch.cuda.stream(stream):
                dst.copy_(src, non_blocking=True)
        forms = {"call": call, "loop": loop}
        if copy:
            forms["copy"] = cp
        t = timed(stream, forms, warmup, reps, budget_s)
        r = {k: summary(v) for k, v in t.items()}
        r["bytes_read"] = read
        r["call_tb_per_s_read"] = round(read / r["call"]["ms_median"] / 1e9, 3)
        r["loop_over_call"] = round(r["loop"]["ms_median"] / r["call"]["ms_median"], 2)
        if copy:
            r["copy_bytes_each_way"] = half
            r["call_over_copy"] = round(r["call"]["ms_median"] / r["copy"]["ms_median"], 3)
        margin = max(r["call"]["ms_spread"], r["loop"]["ms_spread"])
        r["gate_call_faster_by_more_than_spread"] = bool(r["loop"]["ms_median"] - r["call"]["ms_median"] > margin)
        # the two doors agree (the last image, after the timing)
        stream.synchronize()
        assert lib.jsnoop_batch_color_stats(b._h, n - 1, histo_en, host.ctypes.data) == 0
        assert np.array_equal(rows[n - 1].cpu().numpy().view(np.uint32), host), "the one call and the loop differ"
        out["histo_en_%d" % histo_en] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--flat-distinct", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-budget-s", type=float, default=40.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--counters", action="store_true")
    a = ap.parse_args()
    H.build(["synth"])
    lib = J.load()
    dev = torch.device("cuda", 0)
    assert lib.jsnoop_set_device(0) == 0, J.last_error()
    stream = torch.cuda.Stream(dev)
    n = a.images
    natural = [H.synth_jpeg(width=a.width, height=a.height, hs=2, vs=2, quality=85, seed=i + 1) for i in range(min(a.distinct, n))]
    if a.counters:
        b = decoded(natural, n, stream)
        rows = torch.empty((n, WORDS), dtype=torch.int32, device=dev)
        for histo_en in (1, 0):
            for _ in range(3):
                assert lib.jsnoop_batch_pack_stats(b._h, histo_en, None, n, rows.data_ptr(), 0, None) == 0, J.last_error()
        b.sync(); b.close()
        print(json.dumps({"tool": "tools/stats_bench.py --counters", "images": n, "calls_per_histo_en": 3}))
        return
    assert a.warmup >= 5 and a.reps >= 20, "at least 5 warm-ups and 20 repetitions"
    res = {"tool": "tools/stats_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": min(a.distinct, n), "width": a.width, "height": a.height,
           "unit": J.capi.STATS_UNIT, "warmup": a.warmup, "reps": a.reps,
           "timing": "events on the batch stream around each form, forms alternating in one process; the loop's host round trips are inside its events"}
    b = decoded(natural, n, stream)
    res["natural"] = stats_rows(lib, b, n, stream, dev, a.warmup, a.reps, a.loop_budget_s)
    # what the planes cost the decode: the same images without them, decoded in turn
    s2 = torch.cuda.Stream(dev)
    b0 = decoded(natural, n, s2, want_planes=False)
    td = {"with_planes": [], "without_planes": []}
    for r in range(a.warmup + a.reps):
        for name, bb, st in (("with_planes", b, stream), ("without_planes", b0, s2)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st); bb.decode(); e1.record(st); bb.sync()
            if r >= a.warmup:
                td[name].append(e0.elapsed_time(e1))
    res["decode"] = {k: summary(v) for k, v in td.items()}
    res["decode"]["planes_cost_ms_median"] = round(res["decode"]["with_planes"]["ms_median"] - res["decode"]["without_planes"]["ms_median"], 4)
    b0.close(); b.close()
    torch.cuda.empty_cache()
    flat = [flat_picture(a.width, a.height, k) for k in range(min(a.flat_distinct, n))]
    b = decoded(flat, n, stream)
    res["flat"] = stats_rows(lib, b, n, stream, dev, a.warmup, a.reps, a.loop_budget_s, copy=False)
    b.close()
    padded = -(-a.height // 16) * 16
    for name, row in (("events_first_row", 0), ("events_last_row", padded - 1)):
        b = decoded([events_picture(a.width, a.height, row)], 1, stream)
        res[name] = stats_rows(lib, b, 1, stream, dev, a.warmup, a.reps, a.loop_budget_s, copy=False)
        tot = torch.zeros((1, 6), dtype=torch.int32, device=dev); rows = torch.empty((1, WORDS), dtype=torch.int32, device=dev)
        assert lib.jsnoop_batch_pack_stats(b._h, 1, None, 1, rows.data_ptr(), 0, tot.data_ptr()) == 0
        b.sync()
        res[name]["events_in_all"] = int(tot.sum().item()); res[name]["events_counted"] = int(rows[0, 37:43].sum().item())
        b.close()
    res["gate"] = all(v["gate_call_faster_by_more_than_spread"] for k in ("natural", "flat", "events_first_row", "events_last_row") for v in res[k].values() if isinstance(v, dict))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
