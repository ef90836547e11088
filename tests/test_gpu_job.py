"""-m gpu: the job layer (jsnoop_job_* of include/jsnoop_gpu.h, jpegsnoop_amd.JpegJob) on one MI355X.

One call takes a folder's worth of files -- baseline files of several geometries and samplings, progressive files from the catalogue of
tests/prog_cases.py, and planted bad entries -- spreads them over logical shards on device 0 and decodes them in memory-bounded rounds.
Every file's pixels are pinned to the oracle (of the file itself for baseline files, of the baseline form of the codec's truth for
progressive ones), its kind, path and flags to a plain JpegBatch holding that file alone; the refused and unreadable entries are exactly
the planted ones.  Logical shards stay at four or fewer: a process has four hardware queues and every batch brings its own streams.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import prog_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG_NAMES = ["dc_interleaved_ac_whole_cr_y_cb", "successive_approximation_three_and_two_levels", "first_split_refined_whole",
              "values_every_category_al0", "huffman_four_dc_tables_and_ac_table_redefined"]
BASELINE = [("gray", dict(width=97, height=61, gray=1)),
            ("444", dict(width=128, height=64, hs=1, vs=1)),
            ("422_rst", dict(width=141, height=93, hs=2, vs=1, restart_interval=3)),
            ("420_small", dict(width=320, height=240)),
            ("420_odd_rst", dict(width=333, height=217, restart_interval=5)),
            ("440", dict(width=64, height=48, hs=1, vs=2)),
            ("vga", dict(width=640, height=480, quality=92)),
            ("svga_422", dict(width=800, height=600, hs=2, vs=1)),
            ("720p", dict(width=1280, height=720)),
            ("1080p", dict(width=1920, height=1080)),
            ("1080p_422_rst", dict(width=1920, height=1080, hs=2, vs=1, restart_interval=120)),
            ("uxga", dict(width=1600, height=1200, quality=70)),
            ("1080p_q60", dict(width=1920, height=1080, quality=60)),
            ("1080p_q95", dict(width=1920, height=1080, quality=95)),
            ("1080p_rst", dict(width=1920, height=1080, restart_interval=40))]


class Entry:
    def __init__(self, name, data=None, path=None, planted=None, kind=None, answer=None):
        self.name, self.data, self.path, self.planted, self.kind, self.answer = name, data, path, planted, kind, answer
        self.want_hash = self.want_dib = self.alone = None


class FileSet:
    """The job's input in a fixed order, with what every entry must come to."""

    def __init__(self, harness, oracle, tmp):
        import jpegsnoop_amd as J
        rng = np.random.default_rng(77)
        es = []
        for k, (name, kw) in enumerate(BASELINE):
            es.append(Entry(name, data=harness.synth_jpeg(seed=100 + k, **kw), kind="baseline"))
        vga = harness.synth_jpeg(width=640, height=480, seed=29)
        p = harness.parse_jpeg(vga)
        cut = vga[: p.scan_start + int((p.scan_end - p.scan_start) * 0.6)]
        es.insert(5, Entry("damaged_cut", data=cut, kind="baseline"))
        vga2 = bytearray(harness.synth_jpeg(width=640, height=480, seed=31))
        p2 = harness.parse_jpeg(bytes(vga2))
        at = p2.scan_start + int((p2.scan_end - p2.scan_start) * 0.8)
        vga2[at:at + 2] = b"\xff\xe3"                             # a marker that is no RSTn inside the scan
        es.insert(9, Entry("damaged_marker", data=bytes(vga2), kind="baseline"))
        for k, name in enumerate(PROG_NAMES):
            c = PC.built(name)
            es.insert(2 + 3 * k, Entry("prog_" + name, data=c.file, kind="progressive", answer=c.base))
        junk = bytes(rng.integers(0, 256, 4096, dtype=np.uint8))
        if junk[:2] == b"\xff\xd8":
            junk = b"\x00" + junk[1:]
        es.insert(1, Entry("random_bytes", data=junk, planted="refused"))
        es.insert(7, Entry("empty", data=b"", planted="refused"))
        es.insert(12, Entry("cut_in_header", data=es[0].data[:60], planted="refused"))
        es.insert(16, Entry("missing_path", path=str(tmp / "does_not_exist.jpg"), planted="unreadable"))
        # every third good entry goes in by path: read by the shard that owns it
        for i, e in enumerate(es):
            if e.planted is None and i % 3 == 0:
                e.path = str(tmp / ("%02d_%s.jpg" % (i, e.name)))
                with open(e.path, "wb") as f:
                    f.write(e.data)
        self.entries = es
        # the oracle decodes every non-planted file of the set: the cap on refusals below is a condition of the set, checked here
        for e in es:
            if e.planted:
                continue
            harness.drive(oracle, e.answer if e.answer is not None else e.data)
            d = oracle.dib()
            assert d is not None, e.name + ": the oracle does not decode this file"
            e.want_dib = np.array(d, copy=True)
            e.want_hash = J.dib_checksum_numpy(e.want_dib)
            if e.kind == "baseline":
                e.want_mcu_map = np.array(oracle.mcu_map(), copy=True)
            b = J.JpegBatch()
            b.add_jpeg(e.data); b.upload(); b.decode(); b.sync()
            inf = b.info(0)
            e.alone = (inf["path"], inf["flags"])
            e.alone_bytes = b.device_bytes()
            assert int(b.dib_checksums()[0]) == e.want_hash, e.name + ": a plain batch of the file alone differs from the oracle"
            b.close()
        self.planted_refused = sorted(i for i, e in enumerate(es) if e.planted == "refused")
        self.planted_unreadable = sorted(i for i, e in enumerate(es) if e.planted == "unreadable")
        self.good = [i for i, e in enumerate(es) if not e.planted]
        self.hash_sum = sum(es[i].want_hash for i in self.good) & 0xFFFFFFFFFFFFFFFF
        self.largest = max(self.good, key=lambda i: es[i].alone_bytes)

    def index_of(self, name):
        return [e.name for e in self.entries].index(name)


@pytest.fixture(scope="module")
def fs(harness, oracle, tmp_path_factory):
    s = FileSet(harness, oracle, tmp_path_factory.mktemp("jobfiles"))
    assert len(s.planted_refused) == 3 and len(s.planted_unreadable) == 1
    assert s.entries[s.index_of("damaged_cut")].alone[1] != 0, "the damaged file must decode with flags"
    assert s.entries[s.index_of("damaged_marker")].alone[1] != 0
    assert sum(1 for e in s.entries if e.kind == "progressive") == len(PROG_NAMES)
    return s


def run_job(fs, on_file=None, **kw):
    """Runs the whole set through a fresh JpegJob.  Returns (job, stats, records of the callback in arrival order)."""
    import jpegsnoop_amd as J
    job = J.JpegJob(**kw)
    for i, e in enumerate(fs.entries):
        assert (job.add_path(e.path) if e.path is not None else job.add(e.data)) == i
    seen = []

    def cb(r):
        seen.append(r)
        return on_file(r) if on_file else False
    stats = job.run(cb)
    return job, stats, seen


def check_results(fs, job, stats, seen, what):
    """The parity assertion: every file, whatever the partition."""
    res = job.results()
    errs = []
    assert len(res) == len(fs.entries) and sorted(r.index for r in seen) == list(range(len(fs.entries))), what
    by_cb = {r.index: r for r in seen}
    for i, (e, r) in enumerate(zip(fs.entries, res)):
        c = by_cb[i]
        if (c.status, c.kind, c.dib_hash, c.info, c.shard, c.round, c.message) != (r.status, r.kind, r.dib_hash, r.info, r.shard, r.round, r.message):
            errs.append("%s: callback and jsnoop_job_file_result disagree" % e.name)
        if e.planted:
            if r.status != e.planted:
                errs.append("%s: status %s, planted as %s" % (e.name, r.status, e.planted))
            if not r.message:
                errs.append("%s: no message" % e.name)
            continue
        if r.status != "ok":
            errs.append("%s: status %s (%s)" % (e.name, r.status, r.message))
            continue
        if r.kind != e.kind:
            errs.append("%s: kind %s, expected %s" % (e.name, r.kind, e.kind))
        if r.dib_hash != e.want_hash:
            errs.append("%s: DIB checksum differs from the oracle's" % e.name)
        if (r.info["path"], r.info["flags"]) != e.alone:
            errs.append("%s: path / flags %s, alone in a plain batch %s" % (e.name, (r.info["path"], r.info["flags"]), e.alone))
        if (r.info["img_y"], r.info["img_x"]) != e.want_dib.shape[:2]:
            errs.append("%s: size %dx%d" % (e.name, r.info["img_x"], r.info["img_y"]))
    assert not errs, "%s: %d findings\n%s" % (what, len(errs), "\n".join(errs[:25]))
    # no hiding behind refusals: exactly the planted ones, counted
    assert sorted(r.index for r in res if r.status == "refused") == fs.planted_refused, what
    assert sorted(r.index for r in res if r.status == "unreadable") == fs.planted_unreadable, what
    assert stats["refused"] == 3 and stats["unreadable"] == 1 and stats["ok"] == len(fs.good), (what, stats)
    assert stats["ok"] + stats["refused"] + stats["unreadable"] == stats["files"] == len(fs.entries), (what, stats)
    assert stats["dib_hash_sum"] == fs.hash_sum, what
    assert stats["flagged"] == sum(1 for i in fs.good if fs.entries[i].alone[1] != 0), what
    assert stats["pixels"] == sum(res[i].info["dim_x"] * res[i].info["dim_y"] for i in fs.good), what


SAMPLE = ("gray", "422_rst", "damaged_cut", "damaged_marker", "1080p", "prog_dc_interleaved_ac_whole_cr_y_cb", "prog_values_every_category_al0")


@pytest.mark.parametrize("partition", ["lpt", "contiguous"])
@pytest.mark.parametrize("shards", [1, 2, 3, 4])
def test_every_file_decodes_like_the_oracle_whatever_the_partition(fs, shards, partition):
    dibs = {}

    def grab(r):                                                  # full DIB bytes of a sample of files, read from inside the callback
        if fs.entries[r.index].name in SAMPLE:
            assert r.batch is not None
            dibs[r.index] = r.batch.dib(r.image)
        return False
    job, stats, seen = run_job(fs, on_file=grab, devices=[0] * shards, partition=partition)
    what = "%d shards, %s" % (shards, partition)
    check_results(fs, job, stats, seen, what)
    assert stats["nshards"] == shards and len(stats["shard_ms"]) == shards
    assert {r.shard for r in seen} <= set(range(shards)) and all(r.device == 0 for r in seen)
    if partition == "contiguous":
        assert [r.shard for r in job.results()] == sorted(r.shard for r in job.results())
    assert sorted(dibs) == sorted(fs.index_of(n) for n in SAMPLE)
    for i, d in dibs.items():
        assert d.shape == fs.entries[i].want_dib.shape and np.array_equal(d, fs.entries[i].want_dib), (what, fs.entries[i].name)
    assert all(r.batch is None for r in job.results())            # the handles were the callback's
    job.close()


def test_rounds_are_bounded_by_the_memory_budget(fs):
    budget = int(2.5 * fs.entries[fs.largest].alone_bytes)
    job, stats, seen = run_job(fs, devices=[0], max_round_bytes=budget)
    print("budget %d bytes, rounds %d, largest round %d bytes" % (budget, stats["rounds"], stats["max_round_device_bytes"]))
    check_results(fs, job, stats, seen, "one shard, budget of 2.5 largest images")
    assert stats["rounds"] >= 3, stats
    assert 0 < stats["max_round_device_bytes"] <= budget, stats
    rounds = [r.round for r in job.results()]
    assert rounds == sorted(rounds) and rounds[-1] == stats["rounds"] - 1       # one shard: files in order, round by round
    job.close()
    # two shards under the same budget
    job, stats, seen = run_job(fs, devices=[0, 0], max_round_bytes=budget)
    check_results(fs, job, stats, seen, "two shards, budget of 2.5 largest images")
    assert stats["rounds"] >= 3 and stats["max_round_device_bytes"] <= budget, stats
    job.close()


def test_an_image_larger_than_the_budget_decodes_alone(fs):
    job, stats, seen = run_job(fs, devices=[0], max_round_bytes=1000)
    check_results(fs, job, stats, seen, "budget below every image")
    res = job.results()
    good_rounds = [res[i].round for i in fs.good]
    assert len(set(good_rounds)) == len(fs.good), "every decodable file in a round of its own"
    assert stats["max_round_device_bytes"] == fs.entries[fs.largest].alone_bytes
    job.close()
    job, stats, seen = run_job(fs, devices=[0, 0], max_images_per_round=2)
    check_results(fs, job, stats, seen, "two images per round")
    assert stats["rounds"] >= len(fs.good) // 2
    job.close()


def test_batch_device_bytes_covers_the_arenas_and_never_falls(fs):
    import jpegsnoop_amd as J
    for kind in ("baseline", "progressive"):
        b = J.JpegBatch()
        assert b.device_bytes() == 0
        last, blocks, dib = 0, 0, 0
        for e in fs.entries:
            if e.kind != kind:
                continue
            i = b.add_jpeg(e.data)
            inf = b.info(i)
            blocks += inf["total_blocks"]; dib += inf["img_x"] * inf["img_y"] * 4
            now = b.device_bytes()
            assert now >= last, (e.name, now, last)
            assert now >= 128 * blocks + dib, (e.name, now, blocks, dib)
            last = now
        b.upload(); b.decode(); b.sync()
        assert b.device_bytes() == last                            # host arithmetic: decoding does not change it
        b.close()


def test_keep_resident(fs, oracle, harness):
    import jpegsnoop_amd as J
    # a plan of several rounds is refused before anything decodes
    job = J.JpegJob(devices=[0, 0], keep_resident=True, max_round_bytes=int(1.5 * fs.entries[fs.largest].alone_bytes))
    for e in fs.entries:
        job.add_path(e.path) if e.path is not None else job.add(e.data)
    calls = []
    with pytest.raises(RuntimeError, match="keep_resident"):
        job.run(lambda r: calls.append(r.index))
    assert not calls and all(r.status == "pending" and r.batch is None for r in job.results())
    job.close()
    # one round per shard: every handle stays valid behind run()
    job, stats, seen = run_job(fs, devices=[0, 0, 0], keep_resident=True, want_planes=True)
    check_results(fs, job, stats, seen, "keep_resident, three shards")
    assert stats["rounds"] <= 3
    res = job.results()
    for i in fs.good:
        e, r = fs.entries[i], res[i]
        assert r.batch is not None and r.image >= 0
        assert np.array_equal(r.batch.dib(r.image), e.want_dib), e.name
        if e.kind == "baseline":
            so = r.batch.side_outputs(r.image)
            assert np.array_equal(so["mcu_map"], e.want_mcu_map), e.name
    assert all(res[i].batch is None for i in fs.planted_refused + fs.planted_unreadable)
    job.clear()
    assert len(job) == 0
    job.close()


def test_logs_from_inside_the_callback_equal_the_single_file_batch(fs):
    import jpegsnoop_amd as J
    names = ("420_odd_rst", "damaged_cut", "damaged_marker", "vga")
    got = {}

    def grab(r):
        e = fs.entries[r.index]
        if e.name in names:
            got[e.name] = r.batch.log_lines(r.image)
        elif e.kind == "progressive":
            with pytest.raises(RuntimeError, match="progressive image has no DecodeScanImg log"):
                r.batch.log_lines(r.image)
        return False
    job, stats, seen = run_job(fs, on_file=grab, devices=[0, 0], enable_log=True, want_planes=True)
    check_results(fs, job, stats, seen, "enable_log, two shards")
    job.close()
    assert sorted(got) == sorted(names)
    for n in names:
        b = J.JpegBatch(want_planes=True)
        b.enable_log(); b.add_jpeg(fs.entries[fs.index_of(n)].data); b.upload(); b.decode(); b.sync()
        want = b.log_lines(0)
        b.close()
        assert len(want) > 5 and got[n] == want, n
    for n in names:
        print("%s: %d lines, %d of them warnings or errors" % (n, len(got[n]), sum(1 for lvl, _ in got[n] if lvl > 0)))
    assert got["damaged_marker"] != got["vga"] and got["damaged_cut"] != got["vga"]


def test_a_callback_can_cancel(fs):
    stop_after = 5
    count = [0]

    def cb(r):
        count[0] += 1
        return count[0] >= stop_after
    job, stats, seen = run_job(fs, on_file=cb, devices=[0, 0], max_images_per_round=3)
    assert stats["cancelled"] and len(seen) == stop_after and stats["files"] == stop_after
    res = job.results()
    reported = {r.index for r in seen}
    assert all((r.status == "pending") == (r.index not in reported) for r in res)
    assert sum(1 for r in res if r.status == "pending") == len(fs.entries) - stop_after
    job.close()                                                   # destroy behind a cancelled run
    # ... and an exception in the callback cancels the same way and comes out of run()
    import jpegsnoop_amd as J
    job = J.JpegJob(devices=[0])
    job.add(fs.entries[0].data)

    def boom(r):
        raise KeyError("from the callback")
    with pytest.raises(KeyError):
        job.run(boom)
    assert job.run()["ok"] == 1                                   # the job runs again
    job.close()


def test_bad_arguments_are_refused(fs):
    import jpegsnoop_amd as J
    from jpegsnoop_amd import capi
    with pytest.raises(RuntimeError, match="at most 16"):
        J.JpegJob(devices=[0] * 17)
    with pytest.raises(RuntimeError, match="not available"):
        J.JpegJob(devices=[0, 4096])
    lib = capi.load()
    h = lib.jsnoop_job_create(None, 0)
    assert h
    o = capi.JobOptions(); lib.jsnoop_job_options_defaults(C.byref(o))
    o.struct_size = C.sizeof(capi.JobOptions) + 8
    assert lib.jsnoop_job_set_options(h, C.byref(o)) == -1
    o.struct_size = 12                                            # an older, shorter struct: decode_ac and want_planes only
    assert lib.jsnoop_job_set_options(h, C.byref(o)) == 0
    st = capi.JobStats(); st.struct_size = C.sizeof(capi.JobStats)
    assert lib.jsnoop_job_run(h, C.cast(None, capi.JOB_FILE_FN), None, C.byref(st)) == 0 and st.files == 0      # an empty job is no error
    lib.jsnoop_job_destroy(h)


def test_job_demo_processes_a_folder(fs, tmp_path):
    """C++: GenBatchFileList + DoBatchFileProcessAll + JobRun of ImgDecodeGpu.h over a folder with sub-folders, both kinds and a text file."""
    from test_job_partition import EXE, build_job_demo
    build_job_demo()
    src, dst = tmp_path / "src", tmp_path / "dst"
    (src / "sub" / "deeper").mkdir(parents=True)
    put = {"a_gray.jpg": "gray", "b_prog.jpeg": "prog_first_split_refined_whole", "sub/c_422.JPG": "422_rst", "sub/d_cut.jpg": "damaged_cut",
           "sub/deeper/e_prog.jpg": "prog_values_every_category_al0", "sub/deeper/f_vga.Jpeg": "vga"}
    for rel, name in put.items():
        (src / rel).write_bytes(fs.entries[fs.index_of(name)].data)
    (src / "notes.txt").write_text("not a picture\n")
    (src / "sub" / "g_junk.jpg").write_bytes(b"this is no JPEG stream")
    out = subprocess.check_output([EXE, str(src), str(dst), "2"], text=True).strip().splitlines()
    assert out[0] == "listed 7 first=a_gray.jpg", out
    assert out[1] == "processed ok=6 files=7 refused=1 unreadable=0 shards=2", out
    assert out[-1] == "jobrun rc=0", out
    lines = {}
    for l in out[2:-1]:
        tag, rel, rest = l.split(" ", 2)
        assert tag == "file"
        lines[rel] = dict(kv.split("=") for kv in rest.split())
    assert sorted(lines) == sorted(list(put) + ["sub/g_junk.jpg"])
    for rel, name in put.items():
        e = fs.entries[fs.index_of(name)]
        assert lines[rel]["status"] == "0" and lines[rel]["kind"] == ("1" if e.kind == "baseline" else "2"), rel
        assert lines[rel]["hash"] == "%016x" % e.want_hash, rel
        assert lines[rel]["size"] == "%dx%d" % (e.want_dib.shape[1], e.want_dib.shape[0]), rel
    assert lines["sub/g_junk.jpg"]["status"] == "1"
    # one report per listed file, where BatchLogSave would put it; a DecodeScanImg report for every decodable baseline file
    reports = sorted(os.path.relpath(os.path.join(d, f), dst) for d, _s, files in os.walk(dst) for f in files)
    assert reports == sorted(rel + ".txt" for rel in lines), reports
    for rel, name in put.items():
        text = (dst / (rel + ".txt")).read_text()
        if fs.entries[fs.index_of(name)].kind == "baseline":
            assert text.startswith("*** Decoding SCAN Data ***\n") and "Finished Decoding SCAN Data" in text, rel
        else:
            assert "progressive image has no DecodeScanImg log" in text, rel
    assert "not a JPEG stream" in (dst / "sub" / "g_junk.jpg.txt").read_text()


def test_two_devices(fs):
    """The parity assertion over two PHYSICAL devices.  Skipped with fewer than two visible; it has not run on such a box yet."""
    from jpegsnoop_amd import capi
    if capi.load().jsnoop_device_count() < 2:
        pytest.skip("fewer than two devices visible")
    for partition in ("lpt", "contiguous"):
        job, stats, seen = run_job(fs, devices=[0, 1], partition=partition)
        check_results(fs, job, stats, seen, "devices 0 and 1, " + partition)
        assert {r.device for r in seen} == {0, 1}
        job.close()
