#!/usr/bin/env python3
"""Brightest pixel, average Y and colour statistics of the pictures of tests/backend_images.py (flat fields in every layout, the raster
tie-break, the wrapping luminance sum, saturated colour fields) as the COMPILED REFERENCE (oracle/_ref) computes them
-> tests/golden/backend_reductions.json.  Data only: the pictures are regenerated from code where the file is read."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import harness as H          # noqa: E402
import backend_images as BI              # noqa: E402


def main():
    H.build(["synth", "ref"])
    ref = H.ref_backend()
    out = {name: BI.record(H, ref, data) for name, data in sorted(BI.golden_cases(H).items())}
    ref.close()
    with open(os.path.join(HERE, "backend_reductions.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d records" % len(out))


if __name__ == "__main__":
    main()
