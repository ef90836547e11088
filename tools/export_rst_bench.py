"""jsnoop_batch_export_jpeg_rst: what restart intervals cost the export, and what they do to this library's own baseline decode of the exported files.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box).  The batch is
decoded once; then --warmup rounds and --reps timed rounds in which one process alternates, for both Huffman modes, the export with JSNOOP_RESTART_NONE, with
ROWS 1 (Ri = 120: a marker per MCU row) and with MCUS 1 (every MCU an interval), each call between its own two events on the batch's stream.  Reported per
form: median (minimum) ms, the bytes written, and the ratios to NONE of the same Huffman mode.  The export waits for the device twice inside the call, so a
span holds the host's work between the two phases too.

Then the decode of the re-imported files, on the same batch slots: the --distinct exported files of NONE and of ROWS 1 (Annex K tables) are read back, the
source batch is closed, and ONE batch is loaded with the two file sets in turn (clear, add, tile to --images, upload) -- every timed decode, between two events
on the stream, follows a fresh upload of its set; the two alternate with the same warm-up and repetitions.

Prints one JSON line; --out FILE also saves it (profiles/export_rst_bench.json is a run of this tool).
usage: python tools/export_rst_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--out FILE]"""
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

FORMS = [("none", 0), ("rows_1", ("rows", 1)), ("mcus_1", 1)]
MODES = ["annex_k", "optimal"]


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
    spec = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(spec))
    calls = [(mode, name, J.capi.export_coding(lib, mode), J.capi.export_restart(lib, restart)) for mode in MODES for name, restart in FORMS]

    def export(coding, rst):
        assert lib.jsnoop_batch_export_jpeg_rst(b._h, C.byref(spec), C.byref(coding), C.byref(rst), None, n) == 0, J.last_error()

    written = {}; ri = {}
    for mode, name, coding, rst in calls:
        export(coding, rst)
        res = b.export_results()
        assert all(e["result"] == 0 for e in res), "every picture of the bench is exported"
        written[(mode, name)] = sum(e["len"] for e in res); ri[name] = b.export_restart(0)
    for _ in range(a.warmup):
        for _mode, _name, coding, rst in calls:
            export(coding, rst)
    stream.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls] for _ in range(a.reps)]
    for row in ev:
        for (e0, e1), (_mode, _name, coding, rst) in zip(row, calls):
            e0.record(stream); export(coding, rst); e1.record(stream)
    stream.synchronize()
    forms = {}
    for k, (mode, name, _c, _r) in enumerate(calls):
        t = [row[k][0].elapsed_time(row[k][1]) for row in ev]
        forms[mode + "/" + name] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "bytes": written[(mode, name)], "ri": ri[name][0], "intervals": ri[name][1]}
    for mode in MODES:
        base = forms[mode + "/none"]
        for name, _ in FORMS[1:]:
            f = forms[mode + "/" + name]
            f["ms_over_none"] = round(f["ms_median"] / base["ms_median"], 3); f["bytes_over_none"] = round(f["bytes"] / base["bytes"], 4)
    # the decode of the re-imported files, with and without a marker per MCU row
    files = {}
    for name, restart in FORMS[:2]:
        files[name] = b.export_jpeg(images=list(range(distinct)), restart=restart)
    b.close()
    # one batch, its slots loaded with the two file sets in turn: clear, add, tile, upload, then the timed decode
    r = J.JpegBatch(stream=stream.cuda_stream)

    def load(name):
        r.clear()
        for f in files[name]:
            r.add_jpeg(f)
        r.tile(n)
        r.upload()

    for _ in range(a.warmup):
        for name in files:
            load(name); r.decode(); r.sync()
    dv = {name: [] for name in files}; path = {}
    for _ in range(a.reps):
        for name in files:
            load(name)
            stream.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); r.decode(); e1.record(stream)
            stream.synchronize(); r.sync()
            dv[name].append(e0.elapsed_time(e1)); path[name] = r.info(0)["path"]
    decode = {name: {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "path": path[name]} for name, t in dv.items()}
    decode["rows_1_over_none"] = round(decode["rows_1"]["ms_median"] / decode["none"]["ms_median"], 3)
    out = {"tool": "tools/export_rst_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": distinct, "width": a.width, "height": a.height,
           "warmup": a.warmup, "reps": a.reps, "timing": "events on the batch stream around each call, the six exports alternating in one process; a span includes the call's two host waits",
           "export": forms, "decode_of_the_reimported_export": decode, "decode_timing": "one batch reloaded with each file set in turn; events around the decode alone"}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    r.close()


if __name__ == "__main__":
    main()
