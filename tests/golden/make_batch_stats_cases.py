"""Writes tests/golden/batch_stats_cases.json: what the COMPILED REFERENCE (oracle/_ref, built by __graft_entry__.build() where the reference's
sources are present) makes of every file of the batch statistics catalogue (tests/batch_stats_cases.py).  The files themselves are not
committed: they are rebuilt from their description and pinned by their sha256.

Per case: the sha256 of the file and, per option set (tests/stats_cases_util.OPTION_SETS), one digest of the 2482-word statistics record
after the decode.  The oracle has to reproduce every record, and every DIB, before anything is written.

    python tests/golden/make_batch_stats_cases.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import batch_stats_cases as BC                # noqa: E402
from stats_cases_util import OPTION_SETS, run_passes    # noqa: E402
from oracle import harness as H              # noqa: E402


def main():
    assert H.have_ref(), "the compiled reference is not built"
    ref, orc = H.ref_backend(), H.oracle_backend()
    out = {}
    for c in BC.build_all():
        rec = {"sha256": H.hash_bytes(c.file), "stats": {}}
        for key in OPTION_SETS:
            r = run_passes(H, ref, c, key); o = run_passes(H, orc, c, key)
            assert r["dib"] == o["dib"], "%s [%s]: the oracle's DIB differs from the reference's" % (c.name, key)
            assert (r["words"][0] == o["words"][0]).all(), "%s [%s]: the oracle's record differs from the reference's" % (c.name, key)
            rec["stats"][key] = r["digest"][0]
        out[c.name] = rec
    with open(os.path.join(HERE, "batch_stats_cases.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("%d cases" % len(out))


if __name__ == "__main__":
    main()
