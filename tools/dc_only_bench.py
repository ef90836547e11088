#!/usr/bin/env python3
"""DC-only decode of a batch of 1920x1080 4:2:0 JPEGs (the workload of bench.py's config 3, decoded in the reference's default mode):
the DC-only fast form (k_write_dc + k_dc_color) against the same decode through the Full-IDCT kernels (JSNOOP_XC_DC_GENERIC), in ONE
process, steps of the two forms alternating.

    python tools/dc_only_bench.py [--images 1024] [--distinct 64] [--pairs 6] [--warmup 2] [--out FILE]

The parent process never touches the GPU: it starts the measuring step as a child of its own under `timeout` and relays its result --
one JSON line: ms per step of both forms for every alternating pair, stage times of both forms, k_dc_color's fraction of 8 TB/s on the
DIB bytes it writes, and the verdicts (fast below generic in every pair; the smallest margin against the largest spread between two
steps of one form).  Gate before any timing: every DIB hash equal between the forms, equal to the oracle's DC-only decode on every
distinct picture, no flags, forms 2 and 1.  Exit status 0 only when the gate holds."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8e12          # MI355X HBM3E


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--pairs", type=int, default=6, help="alternating (fast, generic) pairs that are timed; at least four")
    ap.add_argument("--warmup", type=int, default=2, help="pairs before them")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds the GPU step may take")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    return ap.parse_args(argv)


def _synth(spec):
    from oracle import harness as H
    w, h, seed = spec
    return H.synth_jpeg(width=w, height=h, hs=2, vs=2, quality=85, seed=seed)


_ORC = None


def _oracle_dc(data):
    """The oracle's DIB checksum of one file decoded DC-only."""
    global _ORC
    from oracle import harness as H
    import jpegsnoop_amd as J
    if _ORC is None:
        _ORC = H.oracle_backend()
        _ORC.set_options(decode_ac=0)
    H.drive(_ORC, data)
    return J.dib_checksum_numpy(_ORC.dib())


def worker(args):
    import concurrent.futures as cf
    import multiprocessing as mp
    from oracle import harness as H
    import jpegsnoop_amd as J
    H.build(["oracle", "synth"])
    nproc = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4))
    with cf.ProcessPoolExecutor(max_workers=nproc, mp_context=mp.get_context("spawn")) as pool:
        files = list(pool.map(_synth, [(args.width, args.height, i + 1) for i in range(args.distinct)]))     # bench.py's pictures of rank 0
        want_jobs = [pool.submit(_oracle_dc, f) for f in files]
        lib = J.load()
        assert lib.jsnoop_set_device(0) == 0, J.last_error()
        batches = {}
        for name, xc in (("fast", 0), ("generic", J.capi.XC_DC_GENERIC)):
            b = J.JpegBatch(decode_ac=False, want_planes=False)
            b.set_tuning(cross_checks=xc)
            for f in files:
                b.add_jpeg(f)
            b.tile(args.images)
            b.upload()
            b.set_split(0)
            b.decode(); b.sync()
            batches[name] = b
        want = [fut.result() for fut in want_jobs]
    bf, bg = batches["fast"], batches["generic"]
    hf, hg = [int(x) for x in bf.dib_checksums()], [int(x) for x in bg.dib_checksums()]
    gate = {"forms": [bf.last_form(), bg.last_form()], "hashes_equal_between_forms": hf == hg,
            "hashes_equal_oracle": all(hf[i] == want[i % args.distinct] for i in range(args.images)),
            "flags_zero": all(bf.info(i)["flags"] == 0 and bg.info(i)["flags"] == 0 for i in range(args.images))}
    gate["ok"] = gate["forms"] == [2, 1] and gate["hashes_equal_between_forms"] and gate["hashes_equal_oracle"] and gate["flags_zero"]
    out = {"tool": "dc_only_bench", "images": args.images, "distinct": args.distinct, "size": [args.width, args.height], "gate": gate}
    if not gate["ok"]:
        return out, 1

    def step(b):
        t0 = time.perf_counter()
        ms, stages = b.decode_timed(1)
        b.sync()
        return (time.perf_counter() - t0) * 1e3, ms, stages

    def pairs(n):
        rows = []
        for _ in range(n):
            wf, ef, sf = step(bf)
            wg, eg, sg = step(bg)
            rows.append({"fast": {"wall_ms": wf, "ms": ef, "stages": sf}, "generic": {"wall_ms": wg, "ms": eg, "stages": sg}})
        return rows

    pairs(args.warmup)
    rows = pairs(max(4, args.pairs))
    # the same with one stream per decode: per-stage times are then those of whole-batch launches (two halves side by side share the chip)
    for b in (bf, bg):
        b.set_split(1)
    pairs(1)
    rows1 = pairs(4)
    for b in (bf, bg):
        b.set_split(0)
    after = [int(x) for x in bf.dib_checksums()] == hf and [int(x) for x in bg.dib_checksums()] == hg and bf.last_form() == 2 and bg.last_form() == 1

    def summary(rows, key):
        f = [r["fast"][key] for r in rows]; g = [r["generic"][key] for r in rows]
        spread = max(max(f) - min(f), max(g) - min(g))
        margin = min(gi - fi for fi, gi in zip(f, g))
        return {"fast": [round(x, 4) for x in f], "generic": [round(x, 4) for x in g], "fast_mean": round(sum(f) / len(f), 4), "generic_mean": round(sum(g) / len(g), 4),
                "fast_below_generic_in_every_pair": all(fi < gi for fi, gi in zip(f, g)), "smallest_margin": round(margin, 4),
                "largest_spread_within_a_form": round(spread, 4), "margin_exceeds_spread": margin > spread}

    def stage_means(rows, form):
        names = list(rows[0][form]["stages"])
        return {n: round(sum(r[form]["stages"][n] for r in rows) / len(rows), 4) for n in names}

    dib_bytes = sum(bf.info(i)["img_x"] * bf.info(i)["img_y"] * 4 for i in range(args.distinct)) * (args.images // args.distinct) if args.images % args.distinct == 0 \
        else sum(bf.info(i)["img_x"] * bf.info(i)["img_y"] * 4 for i in range(args.images))
    st1f, st1g = stage_means(rows1, "fast"), stage_means(rows1, "generic")
    out.update({
        "ms_per_step": summary(rows, "ms"), "wall_ms_per_step": summary(rows, "wall_ms"),
        "stage_ms": {"fast": stage_means(rows, "fast"), "generic": stage_means(rows, "generic")},
        "one_stream": {"ms_per_step": summary(rows1, "ms"), "stage_ms": {"fast": st1f, "generic": st1g}},
        "dib_bytes": dib_bytes,
        "k_dc_color": {"ms": st1f["idct_color"], "fraction_of_8TBps": round(dib_bytes / (st1f["idct_color"] * 1e-3) / PEAK_BYTES_PER_S, 4)},
        "k_idct_color_dc_only": {"ms": st1g["idct_color"], "fraction_of_8TBps": round(dib_bytes / (st1g["idct_color"] * 1e-3) / PEAK_BYTES_PER_S, 4)},
        "results_unchanged_after_timing": after,
    })
    for b in (bf, bg):
        b.close()
    return out, 0 if after else 1


def main():
    args = parse_args()
    if args.worker:
        out, rc = worker(args)
        print("DC_ONLY_BENCH " + json.dumps(out))
        sys.exit(rc)
    cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker"]
    for k in ("images", "distinct", "width", "height", "pairs", "warmup"):
        cmd += ["--" + k, str(getattr(args, k))]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)       # a fresh child owns the GPU; its exit status decides
    line = next((l[len("DC_ONLY_BENCH "):] for l in p.stdout.splitlines() if l.startswith("DC_ONLY_BENCH ")), None)
    if line is None:
        print(json.dumps({"tool": "dc_only_bench", "error": "the GPU step ended with status %d and no result" % p.returncode}))
        sys.exit(p.returncode or 1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(p.returncode)


if __name__ == "__main__":
    main()
