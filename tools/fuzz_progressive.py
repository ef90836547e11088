"""Randomised transitive parity of the progressive path: random size / sampling / quality / restart interval / scan script;
the progressive file must decode to the pixels of the baseline file carrying the same coefficients (oracle).
usage: python tools/fuzz_progressive.py [n_cases] [seed] [--pg-lanes N]
--pg-lanes N aims the run at one form of the scan kernels (JsnoopTuning.pg_lanes: 1, 2, 4, 8, 16 or 64; 0 = by batch size) through jsnoop_set_tuning."""
import argparse, ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from oracle import harness as H
import jpegsnoop_amd
H.build(["oracle", "synth"])
ap = argparse.ArgumentParser()
ap.add_argument("n_cases", nargs="?", type=int, default=60); ap.add_argument("seed", nargs="?", type=int, default=1)
ap.add_argument("--pg-lanes", type=int, default=0, choices=(0, 1, 2, 4, 8, 16, 64))
args = ap.parse_args()
n_cases = args.n_cases
rng = np.random.default_rng(args.seed)
orc = H.oracle_backend(); gpu = H.Backend(jpegsnoop_amd.load(), "jsnoop_", "hip")
tune = jpegsnoop_amd.capi.Tuning(); gpu.lib.jsnoop_tuning_defaults(ctypes.byref(tune)); tune.pg_lanes = args.pg_lanes
if gpu.lib.jsnoop_set_tuning(ctypes.c_void_p(gpu.h), ctypes.byref(tune)) != 0:
    sys.exit("jsnoop_set_tuning: " + jpegsnoop_amd.last_error())
bad = 0
for k in range(n_cases):
    gray = int(rng.integers(6) == 0)
    hs, vs = (1, 1) if gray else [(1, 1), (2, 1), (1, 2), (2, 2)][int(rng.integers(4))]
    kw = dict(width=int(rng.integers(8, 700)), height=int(rng.integers(8, 500)), hs=hs, vs=vs, gray=gray,
              quality=int(rng.choice([10, 30, 50, 75, 85, 95, 100])), restart_interval=int(rng.choice([0, 0, 1, 2, 7, 33, 200])),
              seed=int(rng.integers(1 << 30)), optimize_huffman=int(rng.integers(2)))
    mode = int(rng.integers(1, 3))
    base = H.synth_jpeg(progressive=0, **kw); prog = H.synth_jpeg(progressive=mode, **kw)
    H.drive(orc, base)
    ns = gpu.decode_progressive(prog)
    if ns <= 0 or gpu.lib.jsnoop_last_flags(gpu.h):
        bad += 1; print("case", k, kw, "mode", mode, "decode failed", ns, gpu.lib.jsnoop_last_error()); continue
    a, b = orc.dib(), gpu.dib()
    Hh, W = kw["height"], kw["width"]
    ok = a.shape == b.shape and np.array_equal(a[a.shape[0] - Hh:, :W], b[b.shape[0] - Hh:, :W])
    if ok:
        for pa, pb in zip(orc.planes(), gpu.planes()):
            if pa is not None and not np.array_equal(pa[:Hh, :W], pb[:Hh, :W]): ok = False
    if not ok: bad += 1; print("case", k, kw, "mode", mode, "MISMATCH")
print("progressive cases", n_cases, "pg_lanes", args.pg_lanes, "mismatches", bad)
