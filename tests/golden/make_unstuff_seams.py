#!/usr/bin/env python3
"""DIB, planes, MCU file map, block-DC maps and status words of the inputs of tests/unstuff_inputs.py (restart markers and stuffed bytes on the
4 KiB / 16 KiB seams of the un-stuffing stage under all 16 scan-start phases, scans that end on a grid line, tiny scans, interval tables filled
to the last entry, damaged seams) as the COMPILED REFERENCE (oracle/_ref) computes them -> tests/golden/unstuff_seams.json, with the census of
every file beside its digest.  Data only: digests and small numbers; the files are regenerated from code where the JSON is read.

To regenerate (after a deliberate change of the generator or of an input set): build the reference (`make -C oracle ref`, needs the reference
sources), run `python tests/golden/make_unstuff_seams.py`, and check with `python -m pytest tests/test_unstuff_seams_golden.py` that the
oracle still reproduces every record."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import harness as H          # noqa: E402
import unstuff_inputs as U               # noqa: E402


def main():
    H.build(["synth", "ref"])
    ref = H.ref_backend()
    out = {}
    for name, data in sorted(U.all_inputs(H).items()):
        out[name] = U.record(H, ref, data)
        out[name]["census"] = U.census(data)
    ref.close()
    with open(os.path.join(HERE, "unstuff_seams.json"), "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(v, sort_keys=True) for k, v in sorted(out.items())) + "\n}\n")     # one record per line
    print("wrote %d records" % len(out))


if __name__ == "__main__":
    main()
