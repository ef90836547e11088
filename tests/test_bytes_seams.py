"""CPU: the marker searches of the staging code (jpegsnoop_amd/csrc/jsnoop_bytes.h: js_next_ff, js_scan_end) walk sixteen bytes per step with a
byte-loop tail, and every byte of every file passes through them when it is added to a batch -- but the library does not load without a device,
so nothing on the CPU reached them.  tests/cpp/bytes_seams.cpp compares both with a byte-at-a-time restatement of the rule (the pass the
reference's SOS handler makes over the entropy-coded segment: FF 00 and FF D0..D7 are skipped, any other FF xx ends the data, and a byte
without a successor is never a marker) at every alignment of an FF run against the sixteen-byte steps and the end of the buffer.  It is built
twice with the host compiler: as is (the SSE2 steps), and with -U__SSE2__ (the byte loops that hosts without SSE2 keep)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "bytes_seams.cpp")
INC = os.path.join(ROOT, "jpegsnoop_amd", "csrc")


@pytest.mark.parametrize("form,flags,sse2", [("sse2", [], 1), ("byte_loops", ["-U__SSE2__"], 0)])
def test_marker_searches_agree_with_the_byte_walk(tmp_path, form, flags, sse2):
    exe = str(tmp_path / ("bytes_seams_" + form))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", *flags, "-I" + INC, "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    last = r.stdout.strip().splitlines()[-1]
    m = re.fullmatch(r"sse2=(\d) cases=(\d+) mismatches=(\d+)", last)
    assert m, r.stdout[-2000:]
    if sse2 and int(m.group(1)) == 0:
        pytest.skip("the host compiler has no SSE2: both builds are the byte loops")
    assert int(m.group(1)) == sse2, "the build is not the form it was meant to be"
    assert r.returncode == 0 and int(m.group(3)) == 0, r.stdout[-2000:]
    assert int(m.group(2)) > 5_000_000, last                     # 81 lengths x 18 offsets x positions x runs x followers, two searches each
