"""jsnoop_encode_run against a plain device-to-device copy of the same traffic, the export behind it, the decode of the same batch, and a host encoder.

Input: the bench's config 3 -- 1024 x 1920x1080 4:2:0 q85, 64 distinct synthetic pictures tiled (--images / --distinct for a smaller box) -- decoded once and
taken as uint8 R, G, B tensors [H, W, 3] from JpegBatch.to_torch.  Then, on one stream, --warmup rounds and --reps timed rounds in which one process
alternates, each between its own two events:
  encode          jsnoop_encode_run alone at 4:2:0 q85 (the source descriptions are built once; the span holds the call's host arithmetic, one H2D copy of the
                  records and k_encode)
  encode+export   the same run followed by jsnoop_encode_export with the Annex K tables (the export waits for the device twice inside the call)
  copy            hipMemcpyAsync device to device (a contiguous torch copy_) of (bytes read + bytes written) / 2, so its read plus its write equals the encode's
  decode          jsnoop_batch_decode of the same batch
Reported per form: median and minimum ms; for the encode its rate over (bytes read + bytes written) and its ratio to the copy -- the figure the packs report.
Last, Pillow (libjpeg-turbo) encodes --host-files of the pictures on one host core, quality 85, 4:2:0, not optimised: median ms per image.

Prints one JSON line; --out FILE also saves it (profiles/encode_bench.json is a run of this tool).
usage: python tools/encode_bench.py [--images 1024] [--distinct 64] [--warmup 5] [--reps 20] [--host-files 8] [--out FILE]"""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--host-files", type=int, default=8)
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
    with torch.cuda.stream(stream):
        pics = b.to_torch(layout="HWC", stack=True)                  # [n, H, W, 3] uint8
    stream.synchronize()
    enc = J.JpegEncoder(device=0, stream=stream.cuda_stream)
    spec = J.capi.encode_spec(lib, quality=85, subsampling="4:2:0")
    src = (J.capi.EncodeSrc * n)()
    for k in range(n):
        src[k].ptr = pics[k].data_ptr(); src[k].width = a.width; src[k].height = a.height; src[k].channels = 3
    ex = J.capi.ExportSpec(); lib.jsnoop_export_spec_defaults(C.byref(ex))

    def encode():
        assert lib.jsnoop_encode_run(enc._h, C.byref(spec), src, n) == 0, J.last_error()

    def export():
        assert lib.jsnoop_encode_export(enc._h, C.byref(ex), None, None, None, None, n) == 0, J.last_error()

    encode(); export()
    res = enc.export_results()
    assert all(e["result"] == 0 for e in res), "every picture of the bench is written"
    blocks = sum(enc.info(k)["total_blocks"] for k in range(n))
    read = n * a.width * a.height * 3; written = blocks * 130
    half = (read + written) // 2
    src_c = torch.empty(half, dtype=torch.uint8, device=dev); dst_c = torch.empty(half, dtype=torch.uint8, device=dev)

    def copy():
        with torch.cuda.stream(stream):
            dst_c.copy_(src_c, non_blocking=True)

    def both():
        encode(); export()

    forms = [("encode", encode), ("encode+export", both), ("copy", copy), ("decode", b.decode)]
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
    me, mc = out_forms["encode"]["ms_median"], out_forms["copy"]["ms_median"]
    out_forms["encode"].update(tb_per_s=round((read + written) / me / 1e9, 3), over_copy=round(me / mc, 3), us_per_image=round(me * 1000 / n, 3),
                               over_decode=round(me / out_forms["decode"]["ms_median"], 3))
    out_forms["copy"].update(tb_per_s=round(2 * half / mc / 1e9, 3), bytes_each_way=half)
    out_forms["encode+export"].update(file_bytes=sum(e["len"] for e in res))
    # the host encoder: one core, the same pixels
    host = {}
    try:
        from PIL import Image
        torch.set_num_threads(1)
        imgs = [Image.fromarray(pics[k].cpu().numpy()) for k in range(min(a.host_files, n))]
        ts = []
        for im in imgs * 3:
            f = io.BytesIO(); t0 = time.perf_counter(); im.save(f, "JPEG", quality=85, subsampling=2); ts.append((time.perf_counter() - t0) * 1000)
        host = {"encoder": "Pillow %s (libjpeg-turbo), one core" % __import__("PIL").__version__, "files": len(imgs), "ms_per_image_median": round(statistics.median(ts), 3),
                "ms_per_image_min": round(min(ts), 3)}
    except ImportError:
        host = {"encoder": "Pillow is not installed"}
    out = {"tool": "tools/encode_bench.py", "device": torch.cuda.get_device_name(dev), "images": n, "distinct": distinct, "width": a.width, "height": a.height,
           "quality": 85, "subsampling": "4:2:0", "warmup": a.warmup, "reps": a.reps, "blocks": blocks, "bytes_read": read, "bytes_written": written,
           "timing": "events on one stream around each call, the four forms alternating in one process; the export's span includes its two host waits",
           "forms": out_forms, "host": host}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    enc.close(); b.close()


if __name__ == "__main__":
    main()
