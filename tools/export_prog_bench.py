"""jsnoop_batch_export_jpeg_prog: what progressive output costs the export, and what this library's own decode makes of the exported files.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box).  The batch is
decoded once; then --warmup rounds and --reps timed rounds in which one process alternates four exports, each between its own two events on the batch's
stream: baseline files with own Huffman tables (JSNOOP_PROGRESSIVE_OFF, JSNOOP_HUFFMAN_OPTIMAL) and progressive files along the built-in script, each
without restart markers and with ROWS 1.  Reported per form: median (minimum) ms, the bytes written, and the ratios to the baseline form with the same
restart spec.  The export waits for the device twice inside the call, so a span holds the host's work between the two phases too.

Then the decode of the re-imported files: --decode-files exported files of each of three forms (baseline, progressive, progressive with ROWS 1) are read
back, the source batch is closed, and ONE batch is loaded with the file sets in turn (clear, add, upload) -- every timed decode, between two events on the
stream, follows a fresh upload of its set; the sets alternate, --decode-warmup untimed and --decode-reps timed rounds (a progressive file without restart
markers decodes slowly: that is what the comparison is about).

Prints one JSON line; --out FILE also saves it (profiles/export_prog_bench.json is a run of this tool).
usage: python tools/export_prog_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--decode-files 8] [--out FILE]"""
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

FORMS = [("baseline/none", False, 0), ("progressive/none", True, 0), ("baseline/rows_1", False, ("rows", 1)), ("progressive/rows_1", True, ("rows", 1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--decode-files", type=int, default=8)
    ap.add_argument("--decode-warmup", type=int, default=3)
    ap.add_argument("--decode-reps", type=int, default=10)
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
    spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
    coding = J.capi.export_coding(lib, "optimal")
    calls = [(name, J.capi.export_progressive(lib, prog), J.capi.export_restart(lib, restart)) for name, prog, restart in FORMS]

    def export(prog, rst):
        assert lib.jsnoop_batch_export_jpeg_prog(b._h, C.byref(spec), C.byref(coding), C.byref(rst), C.byref(prog), None, n) == 0, J.last_error()

    written = {}; scans = {}
    for name, prog, rst in calls:
        export(prog, rst)
        res = b.export_results()
        assert all(e["result"] == 0 for e in res), "every picture of the bench is exported"
        written[name] = sum(e["len"] for e in res); scans[name] = [(s["ri"], s["intervals"]) for s in b.export_scans(0)]
    for _ in range(a.warmup):
        for _name, prog, rst in calls:
            export(prog, rst)
    stream.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls] for _ in range(a.reps)]
    for row in ev:
        for (e0, e1), (_name, prog, rst) in zip(row, calls):
            e0.record(stream); export(prog, rst); e1.record(stream)
    stream.synchronize()
    forms = {}
    for k, (name, _p, _r) in enumerate(calls):
        t = [row[k][0].elapsed_time(row[k][1]) for row in ev]
        forms[name] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "bytes": written[name], "scans_ri_intervals": scans[name]}
    for rst in ("none", "rows_1"):
        base, f = forms["baseline/" + rst], forms["progressive/" + rst]
        f["ms_over_baseline"] = round(f["ms_median"] / base["ms_median"], 3); f["bytes_over_baseline"] = round(f["bytes"] / base["bytes"], 4)
    # the decode of the re-imported files
    m = min(a.decode_files, distinct)
    files = {name: b.export_jpeg(images=list(range(m)), huffman="optimal", progressive=prog, restart=restart) for name, prog, restart in (FORMS[0], FORMS[1], FORMS[3])}
    b.close()
    r = J.JpegBatch(stream=stream.cuda_stream)

    def load(name):
        r.clear()
        for f in files[name]:
            r.add_jpeg(f)
        r.upload()

    for _ in range(a.decode_warmup):
        for name in files:
            load(name); r.decode(); r.sync()
    dv = {name: [] for name in files}; path = {}
    for _ in range(a.decode_reps):
        for name in files:
            load(name)
            stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); r.decode(); e1.record(stream)
            stream.synchronize(); r.sync()
            dv[name].append(e0.elapsed_time(e1)); path[name] = r.info(0)["path"]
    decode = {name: {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "path": path[name], "files": m} for name, t in dv.items()}
    decode["progressive_rows_1_over_progressive_none"] = round(decode["progressive/rows_1"]["ms_median"] / decode["progressive/none"]["ms_median"], 4)
    out = {"tool": "tools/export_prog_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": distinct, "width": a.width, "height": a.height,
           "warmup": a.warmup, "reps": a.reps, "timing": "events on the batch stream around each call, the four exports alternating in one process; a span includes the call's two host waits",
           "export": forms, "decode_of_the_reimported_export": decode,
           "decode_timing": "one batch of %d files reloaded with each file set in turn; events around the decode alone; %d warm-ups, %d repetitions" % (m, a.decode_warmup, a.decode_reps)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    r.close()


if __name__ == "__main__":
    main()
