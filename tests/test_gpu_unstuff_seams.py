"""GPU: the un-stuffing stage at its seams -- restart markers and stuffed bytes split over the 16-byte, 1 KiB, 4 KiB and 16 KiB lines of its grid in
every position, under all 16 phases of the scan start; scans that end on, one byte before and one byte behind a 4 KiB line; scans inside one
or two threads' bytes; interval tables with one entry to spare, exactly full and one short; damaged bytes on a seam.  The inputs and the census
conditions that say they really do this are in tests/unstuff_inputs.py (asserted here on the CPU before any GPU result is trusted); the oracle
is pinned to the compiled reference on the same files by tests/test_unstuff_seams_golden.py.  Everything is bit-exact; for well-formed files the
parallel path must have decoded the image unaided (path == 1 and flags == 0: where it is wrong it usually flags the image and the exact mirror
repairs it), and the coefficients are compared as well as the DIB (a DIB clamps).

Which tuning reaches which kernel (js_launch_unstuff, jsnoop_kernels.hip):
  sub_wl = 4                              k_unstuff_write<true>   (4 KiB chunks, look-back over chunks, linear stream)
  sub_wl = 5 / 6 / 7 / 8                  k_unstuff_fused<5 / 6 / 7 / 8>   (16 KiB super-chunks, look-back over super-chunks, interleaved stream)
  cross_checks = XC_UNSTUFF_3PASS         k_unstuff_count + k_unstuff_scan + k_unstuff_write<false>, and for sub_wl 5..8 k_interleave<5..8>
  split = 2                               the same kernels launched over each half of the images (us_base[0] != 0 in the second half)
  side_outputs(i)                         k_unstuff_write<false> in index mode, reading the per-chunk prefixes the decode left behind
                                          (written by k_unstuff_write<true> at sub_wl 4, by k_unstuff_fused<7> per 4 KiB chunk at sub_wl 7)
  the single-image call                   the private batch of a decoder: sub_wl 4 for a file this small, k_unstuff_write<true>
  sub_wl = 4, cand_rounds = 0 / -1        the candidate form / the rounds of k_sync behind the same un-stuffed stream"""
import numpy as np
import pytest

import unstuff_inputs as U

pytestmark = pytest.mark.gpu

STATUS_KEYS = ("scan_bad", "scan_end", "restart_read", "num_pixels", "pos0", "align", "warn_bad", "first")


def _picture(name):
    """The picture a file shows: pads move the scan, not the pixels."""
    return name[:name.rindex("_p")] if "_p" in name else name


class _Snapshot:
    """What the oracle left behind for one file, with the accessors fuzz_util.differs reads from a backend."""

    def __init__(self, b, harness, shared=None):
        self._size, self._status, self._bright = b.image_size(), b.status(), b.bright_avg()
        self._mcu, self._dc, self._histo = b.mcu_map(), b.blk_dc(), b.dht_histo()
        if shared is None:
            shared = {"dib": b.dib(), "planes": b.planes(), "coefs": harness.oracle_coefs(b)}
        else:                                                     # a padded variant: pixels and coefficients are the picture's (checked, not assumed)
            assert np.array_equal(b.dib(), shared["dib"]) and np.array_equal(harness.oracle_coefs(b), shared["coefs"])
        self.shared = shared

    def image_size(self): return self._size
    def dib(self): return self.shared["dib"]
    def planes(self): return self.shared["planes"]
    def coefs(self): return self.shared["coefs"]
    def mcu_map(self): return self._mcu
    def blk_dc(self): return self._dc
    def dht_histo(self): return self._histo
    def status(self): return self._status
    def bright_avg(self): return self._bright


class _Truth:
    """Oracle answers, decoded lazily and kept for the module: per picture (DIB, planes, coefficients) and per file (everything that moves with it)."""

    def __init__(self, harness, oracle):
        self.H, self.o, self.pictures, self.files = harness, oracle, {}, {}

    def picture(self, name, data):
        pic = _picture(name)
        if pic not in self.pictures:
            self.H.drive(self.o, data)
            self.pictures[pic] = {"dib": self.o.dib(), "planes": self.o.planes(), "coefs": self.H.oracle_coefs(self.o)}
        return self.pictures[pic]

    def file(self, name, data):
        if name not in self.files:
            had = _picture(name) in self.pictures
            self.H.drive(self.o, data)
            snap = _Snapshot(self.o, self.H, self.pictures[_picture(name)] if had else None)
            self.pictures.setdefault(_picture(name), snap.shared)
            self.files[name] = snap
        return self.files[name]


@pytest.fixture(scope="module")
def sets(harness):
    """Every input set, with its condition asserted on the CPU first."""
    s = {"seam": U.seam_set(harness), "plain": U.plain_set(harness), "end": U.end_set(harness), "end16": U.end_all_pads(harness), "tiny": U.tiny_set(harness),
         "count": U.count_set(harness), "edge": U.edge_set(harness), "bad": U.damaged_set(harness)}
    U.check_seam_set(s["seam"]); U.check_plain_set(s["plain"]); U.check_end_set(s["end"]); U.check_tiny_set(s["tiny"])
    U.check_count_set(s["count"]); U.check_edge_set(s["edge"]); U.check_damaged_set(harness, s["bad"])
    return s


@pytest.fixture(scope="module")
def truth(harness, oracle):
    return _Truth(harness, oracle)


def _interleaved(large, small):
    """The large files with the small ones dealt between them: chunk and super-chunk bases that differ from image to image."""
    large, small = list(large.items()), list(small.items())
    out, per = [], -(-len(small) // len(large))
    for i, item in enumerate(large):
        out.append(item)
        out += small[i * per:(i + 1) * per]
    assert len(out) == len(large) + len(small)
    return out


def _decode(J, files, **tuning):
    b = J.JpegBatch()
    b.set_tuning(**tuning)
    for _, data in files:
        b.add_jpeg(data)
    b.upload()
    b.decode(); b.decode()                                       # twice: the second decode meets the state words of the first (epoch tag)
    b.sync()
    return b


def _assert_clean_and_exact(b, i, want, what):
    inf = b.info(i)
    assert inf["path"] == 1 and inf["flags"] == 0, (what, inf["path"], hex(inf["flags"]))
    assert np.array_equal(b.dib(i), want["dib"]), (what, "dib")
    assert np.array_equal(b.coefs(i), want["coefs"]), (what, "coefs")


def _xc():
    from jpegsnoop_amd import capi
    return capi.XC_UNSTUFF_3PASS


FORMS = ([("wl%d" % wl, dict(sub_wl=wl, split=1)) for wl in (4, 5, 6, 7, 8)] +
         [("wl%d_3pass" % wl, dict(sub_wl=wl, split=1, xc=True)) for wl in (4, 5, 6, 7, 8)] +
         [("wl%d_split2" % wl, dict(sub_wl=wl, split=2)) for wl in (5, 7)] +
         [("wl4_rounds", dict(sub_wl=4, cand_rounds=-1)), ("wl4_default", dict(sub_wl=4))])


@pytest.mark.parametrize("form", [f for _, f in FORMS], ids=[n for n, _ in FORMS])
def test_every_form_of_the_stage_over_the_seam_batch(harness, truth, sets, form):
    """One batch: the 16 seam variants (every pattern on a 4 KiB and a 16 KiB seam, every start phase) with the tiny, end and chunk-count images
    between them."""
    import jpegsnoop_amd as J
    tuning = dict(form)
    if tuning.pop("xc", False):
        tuning["cross_checks"] = _xc()
    small = dict(sets["tiny"]); small.update(sets["end"]); small.update(sets["count"])
    files = _interleaved(sets["seam"], small)
    b = _decode(J, files, **tuning)
    try:
        t = b.tuning()
        assert t.sub_wl == form["sub_wl"] and b.split_parts() == (form.get("split") or 2)      # (automatic: two streams from 8 MB of scan data)
        if form.get("split") == 2:
            half = len(files) // 2
            assert any(n.startswith("seam") for n, _ in files[:half]) and any(n.startswith("seam") for n, _ in files[half:])
        for i, (name, data) in enumerate(files):
            _assert_clean_and_exact(b, i, truth.picture(name, data), (form, name))
    finally:
        b.close()


@pytest.mark.parametrize("form", [dict(sub_wl=4, split=1), dict(sub_wl=5, split=1), dict(sub_wl=7, split=1), dict(sub_wl=7, split=1, xc=True), dict(sub_wl=7, split=2)],
                         ids=["wl4", "wl5", "wl7", "wl7_3pass", "wl7_split2"])
def test_stuffed_bytes_on_the_seams_without_restart_markers(harness, truth, sets, form):
    """The same picture without restart markers under all 16 pads (FF|00 on 4 KiB and 16 KiB seams): one interval, so a byte lost or kept at a seam
    shifts everything behind it."""
    import jpegsnoop_amd as J
    tuning = dict(form)
    if tuning.pop("xc", False):
        tuning["cross_checks"] = _xc()
    files = _interleaved(sets["plain"], sets["count"])
    b = _decode(J, files, **tuning)
    try:
        for i, (name, data) in enumerate(files):
            _assert_clean_and_exact(b, i, truth.picture(name, data), (form, name))
    finally:
        b.close()


def _assert_side_outputs(so, want, what, full=True):
    assert np.array_equal(so["mcu_map"], want.mcu_map()), (what, "mcu_map")
    assert {k: int(v) for k, v in so["status"].items()} == {("rst_count" if k == "restart_read" else k): int(v) for k, v in want.status().items()}, (what, "status")
    if full:
        for got, ref in zip(so["blk_dc"], want.blk_dc()):
            if ref is not None:
                assert np.array_equal(got, ref), (what, "blk_dc")
        assert np.array_equal(so["dht_histo"], want.dht_histo()), (what, "dht_histo")


@pytest.mark.parametrize("wl", [4, 7])
def test_side_passes_on_the_seams(harness, truth, sets, wl):
    """MCU file map, block-DC maps, code-length histogram and status words of the seam, end and tiny images, against the oracle driven on the PADDED
    file (file positions move with the pad): the only reader of the per-chunk prefixes the decode leaves behind and of the index mode of
    k_unstuff_write<false>."""
    import jpegsnoop_amd as J
    small = dict(sets["tiny"]); small.update(sets["end"])
    files = _interleaved(sets["seam"], small)
    b = _decode(J, files, sub_wl=wl, split=1)
    try:
        for i, (name, data) in enumerate(files):
            want = truth.file(name, data)
            inf = b.info(i)
            assert inf["path"] == 1 and inf["flags"] == 0, (wl, name)
            _assert_side_outputs(b.side_outputs(i, bright=False), want, (wl, name))
    finally:
        b.close()


@pytest.mark.parametrize("which", ["tiny", "end16", "seam"])
def test_single_image_call_under_every_pad(harness, truth, gpu, sets, which):
    from fuzz_util import differs
    files = sets[which]
    assert len(files) == (32 if which == "tiny" else 16)
    for name, data in files.items():
        want = truth.file(name, data)
        harness.drive(gpu, data)
        assert gpu.lib.jsnoop_last_path(gpu.h) == 1 and gpu.lib.jsnoop_last_flags(gpu.h) == 0, name
        assert differs(want, gpu) is None, (name, differs(want, gpu))


@pytest.mark.parametrize("wl", [4, 5])
def test_interval_table_filled_to_its_last_entry(harness, truth, sets, wl):
    """Streams with more markers than their header announces: nmcu - 1 markers against a table sized for nmcu / 3 intervals -- one entry to spare,
    exactly full, one too many (the library may hand that image to the mirror: no assertion on its path).  Alone, and back to back with a
    well-formed neighbour in both orders: an entry written one past a table lands in the neighbour's."""
    import jpegsnoop_amd as J
    edge = list(sets["edge"].items())
    nb = ("edge_neighbour", U.edge_neighbour(harness))
    assert U.census(nb[1])["markers"] + 2 <= U.edge_seg_cap(72, 1)
    orders = [[e] for e in edge] + [edge + [nb], list(reversed(edge + [nb])), [nb] + edge + [nb] + list(reversed(edge)) + [nb]]
    for files in orders:
        b = _decode(J, files, sub_wl=wl)
        try:
            for i, (name, data) in enumerate(files):
                want = truth.file(name, data)
                what = (wl, [n for n, _ in files], i)
                assert np.array_equal(b.dib(i), want.dib()), what
                _assert_side_outputs(b.side_outputs(i, bright=False), want, what)
                if name == "edge_neighbour":
                    assert b.info(i)["path"] == 1 and b.info(i)["flags"] == 0, what
                    assert np.array_equal(b.coefs(i), want.coefs()), what
        finally:
            b.close()


def test_interval_table_edges_through_the_single_image_call(harness, truth, gpu, sets):
    from fuzz_util import differs
    for name, data in sets["edge"].items():
        harness.drive(gpu, data)
        assert differs(truth.file(name, data), gpu) is None, (name, differs(truth.file(name, data), gpu))


def test_damaged_seams_through_the_single_image_call(harness, truth, gpu, sets):
    """FF|FF, FF FF|00, FF|FF D3, FF D3|FF D4, FF|D9 and FF|E0 written over a 4 KiB and over a 16 KiB seam."""
    for name, data in sets["bad"].items():
        want = truth.file(name, data)
        harness.drive(gpu, data)
        assert np.array_equal(gpu.dib(), want.dib()), name
        assert gpu.status() == want.status(), (name, gpu.status(), want.status())
        assert np.array_equal(gpu.mcu_map(), want.mcu_map()), name


@pytest.mark.parametrize("wl", [4, 7])
def test_damaged_seams_inside_a_batch_of_clean_variants(harness, truth, sets, wl):
    import jpegsnoop_amd as J
    clean = {k: v for k, v in sets["seam"].items() if k in ("seam_p03", "seam_p06", "seam_p07", "seam_p13")}     # (16 KiB seams: FF|00 and FF|Dn, FF|Dn and FF Dn|, FF|Dn and |FF Dn, FF Dn|)
    files = _interleaved(clean, sets["bad"])
    b = _decode(J, files, sub_wl=wl, split=1)
    try:
        for i, (name, data) in enumerate(files):
            if name.startswith("seam"):
                _assert_clean_and_exact(b, i, truth.picture(name, data), (wl, name))
            else:
                want = truth.file(name, data)
                assert np.array_equal(b.dib(i), want.dib()), (wl, name)
                _assert_side_outputs(b.side_outputs(i, bright=False), want, (wl, name), full=False)
    finally:
        b.close()
