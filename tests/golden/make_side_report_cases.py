"""Writes tests/golden/side_report_cases.json: what the COMPILED REFERENCE (oracle/_ref, built by __graft_entry__.build() where the
reference's sources are present) makes of every file of the damaged-file catalogue (tests/side_report_cases.py), per err_max the case
is driven with.

Per case: the sha256 of the file, the status words of the undamaged file where the case has one ("clean_status"), and per err_max
("runs") the record of tests/golden_util.record -- image size, digests of the DIB, the int16 planes, the MCU file map, the block-DC
maps and the code-length histogram, the status words, the brightest-pixel / average record -- plus the log at quiet = 0: the lines
from "*** Decoding SCAN Data ***" up to "Compression stats" verbatim ("section") and the sha256 of the whole log ("log_sha256").
The script stops where the oracle does not reproduce the reference's record (the oracle keeps no log).

    python tests/golden/make_side_report_cases.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import side_report_cases as SC               # noqa: E402
from oracle import harness as H              # noqa: E402


def main():
    assert H.have_ref(), "the compiled reference is not built"
    ref, orc = H.ref_backend(), H.oracle_backend()
    out = {}
    for c in SC.build_all():
        c.check(c)
        e = {"sha256": H.hash_bytes(c.file), "runs": {}}
        if c.clean is not None:
            e["clean_status"] = SC.run(H, ref, c.clean, 20)["status"]
        for em in c.err_max:
            r = SC.run(H, ref, c.file, em); o = SC.run(H, orc, c.file, em, log=False)
            bad = [k for k in o if r[k] != o[k]]
            assert not bad, "%s, err_max %d: the oracle differs from the reference in %s" % (c.name, em, bad)
            e["runs"][str(em)] = r
        out[c.name] = e
    ref.set_options(); orc.set_options()
    with open(os.path.join(HERE, "side_report_cases.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases, %d records" % (len(out), sum(len(e["runs"]) for e in out.values())))


if __name__ == "__main__":
    main()
