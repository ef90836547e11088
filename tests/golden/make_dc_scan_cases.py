"""Writes tests/golden/dc_scan_cases.json: what the COMPILED REFERENCE (oracle/_ref, built by __graft_entry__.build() where the
reference's sources are present) makes of every file of the DC scan catalogue (tests/dc_scan_cases.py).  The files themselves are
not committed: they are rebuilt from their seeds and pinned by their sha256.

Per case: the sha256 of the file and the record of tests/golden_util.record -- image size, digests of the DIB, the int16 planes, the
MCU file map, the block-DC maps and the code-length histogram (dht_histo), the status words and the brightest-pixel / average record.
The reference keeps no coefficient arena (one block's m_anDctBlock at a time, gone after its IDCT); its planes are the IDCT of every
block's coefficients plus the DC sums.  The arena digest ("coefs") is therefore the oracle's, and it is only written after the oracle
has reproduced every reference output of the case -- the script stops otherwise.

    python tests/golden/make_dc_scan_cases.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import dc_scan_cases as BC                    # noqa: E402
from golden_util import record               # noqa: E402
from oracle import harness as H              # noqa: E402


def main():
    assert H.have_ref(), "the compiled reference is not built"
    ref, orc = H.ref_backend(), H.oracle_backend()
    out = {}
    for c in BC.build_all():
        c.check(c)
        H.drive(ref, c.file); r = record(H, ref)
        H.drive(orc, c.file); o = record(H, orc)
        assert r == o, "%s: the oracle differs from the reference in %s" % (c.name, [k for k in r if r[k] != o.get(k)])
        r["coefs"] = H.hash_bytes(H.oracle_coefs(orc))
        r["sha256"] = H.hash_bytes(c.file)
        out[c.name] = r
    with open(os.path.join(HERE, "dc_scan_cases.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases" % len(out))


if __name__ == "__main__":
    main()
