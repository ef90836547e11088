"""-m gpu: the report of a damaged file -- message lines with their offsets, status words, MCU file map, block-DC maps, code-length
histogram -- on the catalogue of tests/side_report_cases.py: one named event per file at a seam of the three producers of
js_side_only (1: the parallel side pass with its overflow records, 3: one exact reader per chunk of MCUs, stitched on the host,
2: the sequential mirror).  tests/test_side_report_cases.py proves on the CPU where every event lies and that the compiled reference
flags every case; its answers are data (tests/golden/side_report_cases.json), so nothing here depends on the reference being present.

Every case, under every err_max it names, goes through the single-image call with a log callback at quiet = 0 and twice through a
batch of the whole catalogue with clean files in between (results asked for in ascending order, then in a shuffled order: the second
request of a batch runs the clean images' side passes all at once while flagged images keep their own paths).  The comparison is
exact: differs(oracle, gpu) is None, the record equals the recorded one, the message section equals the recorded lines, the digest
of the whole log equals the recorded digest.  No case is skipped.  Which producer answered is printed per case (run with -s) and
asserted where the code determines it."""
import random

import numpy as np
import pytest

import side_report_cases as SC
from golden_util import record

pytestmark = pytest.mark.gpu

PREFIX = ("", "W:", "E:")


def first_difference(got, want):
    k = next((j for j, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    return "line %d: got %r, recorded %r (%d lines against %d)" % (k, got[k] if k < len(got) else None, want[k] if k < len(want) else None, len(got), len(want))


class World:
    def __init__(self, harness, oracle, gpu):
        import json
        import os
        self.H, self.oracle, self.gpu = harness, oracle, gpu
        self.cases = SC.build_all()
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "side_report_cases.json")) as f:
            self.want = json.load(f)
        self.done = {}                                        # group -> (findings, {(case, err_max): mode})

    def single(self, group):
        """Every case of the group through the single-image call, once per module."""
        if group in self.done:
            return self.done[group]
        from fuzz_util import differs
        H, oracle, gpu = self.H, self.oracle, self.gpu
        errs = []; modes = {}
        try:
            for c in self.cases:
                if c.group != group:
                    continue
                for em in c.err_max:
                    w = self.want[c.name]["runs"][str(em)]; tag = "%s [err_max %d]" % (c.name, em)
                    oracle.set_options(decode_ac=1, err_max=em); gpu.set_options(decode_ac=1, err_max=em)
                    p = H.drive(oracle, c.file)
                    H.drive(gpu, c.file, p, quiet=0)
                    lines = gpu.log_lines()
                    modes[(c.name, em)] = (gpu.lib.jsnoop_last_side_mode(gpu.h), gpu.lib.jsnoop_last_path(gpu.h), gpu.lib.jsnoop_last_flags(gpu.h))
                    d = differs(oracle, gpu)
                    if d is not None:
                        errs.append("%s: differs from the oracle in %s" % (tag, d))
                    r = record(H, gpu)
                    for k, v in r.items():
                        if v != w[k]:
                            errs.append("%s: %s is %s, recorded %s" % (tag, k, v, w[k]))
                    try:
                        sec = SC.section(lines)
                    except StopIteration:
                        sec = lines
                    if sec != w["section"]:
                        errs.append("%s: message section, %s" % (tag, first_difference(sec, w["section"])))
                    elif SC.log_digest(lines) != w["log_sha256"]:
                        errs.append("%s: the log outside the message section differs from the recorded one (digest)" % tag)
        finally:
            oracle.set_options(); gpu.set_options()
        self.done[group] = (errs, modes)
        return self.done[group]


@pytest.fixture(scope="module")
def world(harness, oracle, gpu):
    return World(harness, oracle, gpu)


def print_modes(modes):
    for (name, em), (sm, path, flags) in sorted(modes.items()):
        print("%-72s err_max %-3d side mode %d path %d flags %#06x" % (name, em, sm, path, flags))


@pytest.mark.parametrize("group", SC.GROUPS)
def test_single_image_report_equals_the_recorded_one(world, group):
    errs, modes = world.single(group)
    print_modes(modes)
    assert modes, group
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:30]))


def test_the_producer_is_the_one_the_code_determines(world):
    """An overflow 48 bits in front of an interval or scan end is the parallel side pass's (mode 1), one 39 bits in front of it is not;
    96 events in a chunk fit its record (mode 3), 99 do not (mode 2); and modes 1, 2 and 3 all occur in the run."""
    modes = {}
    for g in SC.GROUPS:
        modes.update(world.single(g)[1])
    print_modes(modes)
    bad = []; stated = 0
    for c in world.cases:
        if c.mode is None:
            continue
        for em in c.err_max:
            sm = modes[(c.name, em)][0]; stated += 1
            if (sm == 1) if c.mode == "not1" else (sm != c.mode):
                bad.append("%s [err_max %d]: side mode %d, the catalogue states %s" % (c.name, em, sm, c.mode))
    assert not bad, "\n".join(bad)
    assert stated >= 19
    assert {sm for sm, _p, _f in modes.values()} >= {1, 2, 3}, sorted({sm for sm, _p, _f in modes.values()})


def _batch_record(H, b, i):
    so = b.side_outputs(i)
    keys = ("scan_bad", "scan_end", "restart_read", "num_pixels", "pos0", "align", "warn_bad", "first")
    return {"mcu_map": H.hash_bytes(np.ascontiguousarray(so["mcu_map"])),
            "blk_dc": [H.hash_bytes(np.ascontiguousarray(p)) if p is not None else None for p in so["blk_dc"]],
            "histo": H.hash_bytes(np.ascontiguousarray(so["dht_histo"])),
            "status": dict(zip(keys, (int(v) for v in so["status"].values()))),
            "bright_avg": [int(v) for v in so["bright_avg"]]}


@pytest.mark.parametrize("order", ["ascending", "shuffled"])
def test_batch_of_the_whole_catalogue(world, order):
    import jpegsnoop_amd as J
    H, gpu = world.H, world.gpu
    clean = SC.clean_files()
    items = []                                                # (name, err_max, data, recorded answer or None)
    for n, c in enumerate(world.cases):
        for em in c.err_max:
            items.append((c.name, em, c.file, world.want[c.name]["runs"][str(em)]))
        if n % 4 == 0:
            items.append(("clean_%d" % (n % len(clean)), 20, clean[n % len(clean)], None))
    b = J.JpegBatch(want_planes=True)
    errs = []
    try:
        b.enable_log(True)
        for name, em, data, _w in items:
            gpu.set_options(decode_ac=1, err_max=em)
            p = H.parse_jpeg(data)
            H.push_tables(gpu, p)
            assert b.add(gpu.h, data, p.scan_start) == len(b) - 1, name
        b.upload(); b.decode(); b.sync()
        idx = list(range(len(items)))
        if order == "shuffled":
            random.Random(20240607).shuffle(idx)
        for i in idx:
            name, em, data, w = items[i]; tag = "%s [err_max %d, image %d]" % (name, em, i)
            got = _batch_record(H, b, i)
            lines = [PREFIX[min(max(l, 0), 2)] + t for l, t in b.log_lines(i)]
            if _batch_record(H, b, i) != got or [PREFIX[min(max(l, 0), 2)] + t for l, t in b.log_lines(i)] != lines:
                errs.append("%s: the second request answers differently" % tag)
            sec = SC.section(lines)
            if w is None:
                if b.info(i)["flags"] or b.info(i)["path"] != 1 or SC.messages(sec) or got["status"]["scan_bad"]:
                    errs.append("%s: a clean file with path %d flags %#x and %d messages" % (tag, b.info(i)["path"], b.info(i)["flags"], len(SC.messages(sec))))
                continue
            if H.hash_bytes(b.dib(i)) != w["dib"]:
                errs.append("%s: DIB differs from the recorded one" % tag)
            for k, v in got.items():
                if v != w[k]:
                    errs.append("%s: %s is %s, recorded %s" % (tag, k, v, w[k]))
            if sec != w["section"]:
                errs.append("%s: message section, %s" % (tag, first_difference(sec, w["section"])))
            elif SC.log_digest(lines) != w["log_sha256"]:
                errs.append("%s: the log outside the message section differs from the recorded one (digest)" % tag)
    finally:
        b.close(); gpu.set_options()
    assert not errs, "%d findings\n%s" % (len(errs), "\n".join(errs[:30]))
