"""jsnoop_carve_run against a plain device-to-device copy of the blob, the page-locked upload of the blob, the host-only carve, a numpy search for
FF D8 FF alone, and carve + job against the job on the files handed over one by one.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85 files, 64 distinct synthetic pictures repeated (--images / --distinct for a smaller box) -- inside
RIFF-style chunks ("00dc", little-endian length, the file, an odd padding that differs from chunk to chunk), one blob.

Timing: jsnoop_carve_run waits for the device twice inside the call (totals, then records), so it is timed by the host clock around the call, which ends in a
device synchronise; the copy and the upload by events on a torch stream; the host-only legs by the host clock.  --warmup rounds and --reps timed rounds of
(carve, copy, upload) alternate in one process; median and minimum are reported.  The slow host legs and the two job legs run --host-reps times.
The count and emit passes each read the blob once, the copy reads it once and writes it once: "carve_over_copy" is the ratio to write down.

Kernel split: not taken here.  `rocprofv3 --kernel-trace --stats -- python tools/carve_bench.py --only-carve`, in a run of its own, gives the four kernels' times.

Prints one JSON line; --out FILE also saves it (profiles/carve_bench.json is a run of this tool).
usage: python tools/carve_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--host-reps 3] [--only-carve] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jpegsnoop_amd as J                                            # noqa: E402
from oracle import harness as H                                      # noqa: E402


def container(files):
    out = bytearray(b"RIFF\0\0\0\0AVI LIST" + bytes(24) + b"movi"); at = []
    for k, f in enumerate(files):
        out += b"00dc" + len(f).to_bytes(4, "little")
        at.append((len(out), len(out) + len(f)))
        out += f + bytes(1 + 2 * (k % 7))
    return bytes(out), at


def wall_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--only-carve", action="store_true", help="the device carve alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.warmup >= 5 and a.reps >= 20, "at least 5 warm-ups and 20 repetitions"
    H.build(["synth"])
    lib = J.load()
    dev = torch.device("cuda", 0)
    assert lib.jsnoop_set_device(0) == 0, J.last_error()
    distinct = [H.synth_jpeg(width=a.width, height=a.height, hs=2, vs=2, quality=85, seed=i + 1) for i in range(min(a.distinct, a.images))]
    files = [distinct[i % len(distinct)] for i in range(a.images)]
    blob, at = container(files)
    n = len(blob)
    host = np.frombuffer(blob, np.uint8)
    pinned = torch.from_numpy(host.copy()).pin_memory()
    d_blob = pinned.to(dev); d_copy = torch.empty_like(d_blob)
    stream = torch.cuda.Stream(dev)
    carve = J.Carve(0)

    def run_carve():
        carve.run(d_blob)

    def copy():
        with torch.cuda.stream(stream):
            d_copy.copy_(d_blob, non_blocking=True)

    def upload():
        with torch.cuda.stream(stream):
            d_copy.copy_(pinned, non_blocking=True)

    run_carve()
    frames = carve.frames()
    nterm, ncand = carve.totals()
    ok = [f for f in frames if f["status"] == 0]
    assert [(f["start"], f["end"]) for f in ok if f["parent"] < 0] == at, "every file of the container is carved where it was put"
    if a.only_carve:
        for _ in range(a.warmup + a.reps):
            run_carve()
        print(json.dumps({"tool": "tools/carve_bench.py", "only_carve": True, "blob_bytes": n, "runs": 1 + a.warmup + a.reps}))
        return
    for _ in range(a.warmup):
        run_carve(); copy(); upload()
    stream.synchronize()
    tc, tk, tu = [], [], []
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(a.reps)]
    for e in ev:
        tc += wall_ms(run_carve, 1)
        e[0].record(stream); copy(); e[1].record(stream)
        e[2].record(stream); upload(); e[3].record(stream)
        stream.synchronize()
    tk = [e[0].elapsed_time(e[1]) for e in ev]; tu = [e[2].elapsed_time(e[3]) for e in ev]
    th = wall_ms(lambda: J.carve_host(host), a.host_reps)
    tn = wall_ms(lambda: np.flatnonzero((host[:-2] == 0xFF) & (host[1:-1] == 0xD8) & (host[2:] == 0xFF)), a.host_reps)

    def job_carved():
        c = J.Carve(0); c.run(host); fr = c.frames(); c.close()
        job = J.JpegJob(devices=[0])
        assert len(job.add_carved(host, fr)) == len(ok)
        st = job.run(); job.close()
        return st

    def job_files():
        job = J.JpegJob(devices=[0])
        for f in files:
            job.add(f)
        st = job.run(); job.close()
        return st

    sa = job_carved(); sb = job_files()                              # (one warm-up each)
    assert sa["ok"] == len(ok) and sb["ok"] == len(files) and (len(ok) != len(files) or sa["dib_hash_sum"] == sb["dib_hash_sum"])
    tja, tjb = [], []
    for _ in range(a.host_reps):
        tja += wall_ms(job_carved, 1); tjb += wall_ms(job_files, 1)
    med = statistics.median
    out = {"tool": "tools/carve_bench.py", "device": torch.cuda.get_device_name(dev), "images": a.images, "distinct": len(distinct), "width": a.width, "height": a.height,
           "warmup": a.warmup, "reps": a.reps, "host_reps": a.host_reps, "blob_bytes": n, "terminators": nterm, "candidates": ncand, "frames_ok": len(ok),
           "timing": "carve: host clock around the call (two device waits inside); copy, upload: events on a torch stream; alternating; host legs and jobs: host clock",
           "carve_ms_median": round(med(tc), 4), "carve_ms_min": round(min(tc), 4), "copy_ms_median": round(med(tk), 4), "copy_ms_min": round(min(tk), 4),
           "upload_ms_median": round(med(tu), 4), "upload_ms_min": round(min(tu), 4), "carve_over_copy": round(med(tc) / med(tk), 3), "upload_over_carve": round(med(tu) / med(tc), 3),
           "carve_gb_per_s_two_reads": round(2 * n / med(tc) / 1e6, 1), "copy_gb_per_s_read_plus_write": round(2 * n / med(tk) / 1e6, 1), "upload_gb_per_s": round(n / med(tu) / 1e6, 1),
           "carve_host_ms_median": round(med(th), 2), "numpy_soi_search_ms_median": round(med(tn), 2),
           "job_on_carved_blob_ms_median": round(med(tja), 2), "job_on_files_ms_median": round(med(tjb), 2), "job_carved_over_files": round(med(tja) / med(tjb), 3)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    carve.close()


if __name__ == "__main__":
    main()
