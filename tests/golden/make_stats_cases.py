"""Writes tests/golden/stats_cases.json: what the COMPILED REFERENCE (oracle/_ref, built by __graft_entry__.build() where the
reference's sources are present) makes of every file of the colour statistics catalogue (tests/stats_cases.py).  The files themselves are
not committed: they are rebuilt from their description and pinned by their sha256.

Per case: the sha256 of the file; under "stats" per option set (tests/stats_cases_util.OPTION_SETS) one digest of the 2482-word statistics
record after the decode and after each re-render of the case; under "log" the reference's `YCC Clipped` / `Only reported first 10` lines,
verbatim, per pass -- under "all" where Full IDCT and DC only wrote the same lines, under "full" and "dc" otherwise (bHistoEn or bStatClipEn alone
makes no difference to them; the script checks that).

The oracle has to reproduce every record before it is written.  One exception is allowed for: a group D file on which the two differ is left
out and named under "_left_out" with both values (the sums of those files pass 2**31, which is undefined in the reference's C++).

    python tests/golden/make_stats_cases.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import stats_cases as SC                      # noqa: E402
from stats_cases_util import OPTION_SETS, run_passes    # noqa: E402
from oracle import harness as H              # noqa: E402


def main():
    assert H.have_ref(), "the compiled reference is not built"
    ref, orc = H.ref_backend(), H.oracle_backend()
    out = {}; left_out = {}
    for c in SC.build_all():
        rec = {"sha256": H.hash_bytes(c.file), "stats": {}, "log": {}}
        differs = None
        for key in OPTION_SETS:
            r = run_passes(H, ref, c, key); o = run_passes(H, orc, c, key)
            assert r["dib"] == o["dib"], "%s [%s]: the oracle's DIB differs from the reference's" % (c.name, key)
            for p, (a, b) in enumerate(zip(r["words"], o["words"])):
                if not (a == b).all() and differs is None:
                    k = int((a != b).argmax()); differs = {"option_set": key, "pass": p, "word": k, "reference": int(a[k]), "oracle": int(b[k])}
            rec["stats"][key] = r["digest"]; rec["log"][key] = r["log"]
        if differs:
            assert c.group == "D", "%s: the oracle differs from the reference: %s" % (c.name, differs)
            left_out[c.name] = differs
            continue
        lg = rec["log"]
        assert lg["histo"] == lg["clip"] and lg["histo_dc"] == lg["clip_dc"], "%s: the warnings do not depend on bHistoEn" % c.name
        rec["log"] = {"all": lg["histo"]} if lg["histo"] == lg["histo_dc"] else {"full": lg["histo"], "dc": lg["histo_dc"]}
        out[c.name] = rec
    if left_out:
        out["_left_out"] = left_out
    with open(os.path.join(HERE, "stats_cases.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d left out" % (len(out) - bool(left_out), len(left_out)))


if __name__ == "__main__":
    main()
