"""Overhead of the job layer (JpegJob, keep_resident, one and two logical shards on device 0) against a plain JpegBatch over the same
256 x 1080p 4:2:0 files: same process, alternating, fresh objects every repetition, wall milliseconds.
usage: python tools/job_overhead.py [output file]   (profiles/job_overhead.txt keeps the run this tree was measured with)"""
import os, sys, time, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jpegsnoop_amd as J
from oracle import harness as H

N, DISTINCT, REPS = 256, 32, 7
seeds = [H.synth_jpeg(width=1920, height=1080, seed=500 + k) for k in range(DISTINCT)]
files = [seeds[i % DISTINCT] for i in range(N)]
lib = J.load()
rows = {"readd": [], "plain_udS": [], "plain_all": [], "plain_all_hash": [], "job1": [], "job2": [], "job1_shard": [], "job2_shard": []}
sums = set()

def plain():
    b = J.JpegBatch()
    t0 = time.perf_counter()
    for f in files: b.add_jpeg(f)
    t1 = time.perf_counter()
    b.upload(); b.decode(); b.sync()
    t2 = time.perf_counter()
    cs = b.dib_checksums()
    t3 = time.perf_counter()
    b.clear()
    t4 = time.perf_counter()
    for f in files: b.add_jpeg(f)                     # the staging area already holds this many bytes: header walks and copies only
    rows["readd"].append((time.perf_counter() - t4) * 1e3)
    sums.add(int(sum(int(c) for c in cs) & 0xFFFFFFFFFFFFFFFF))
    rows["plain_udS"].append((t2 - t1) * 1e3); rows["plain_all"].append((t2 - t0) * 1e3); rows["plain_all_hash"].append((t3 - t0) * 1e3)
    b.close()

def job(shards, key):
    j = J.JpegJob(devices=[0] * shards, keep_resident=True)
    for f in files: j.add(f)
    st = j.run()
    assert st["ok"] == N and st["rounds"] == shards, st
    sums.add(st["dib_hash_sum"])
    rows[key].append(st["wall_ms"]); rows[key + "_shard"].append(max(st["shard_ms"]))
    j.close()

plain(); job(1, "job1"); job(2, "job2")             # warm-up: code objects, first allocations
for k in rows: rows[k].clear()
for r in range(REPS):
    plain(); job(1, "job1"); job(2, "job2")
assert len(sums) == 1, sums
med = {k: statistics.median(v) for k, v in rows.items()}
out = []
out.append("tools/job_overhead.py -- job layer against a plain JpegBatch: %d x 1080p 4:2:0 (%d distinct files), one MI355X, same process, alternating," % (N, DISTINCT))
out.append("fresh objects every repetition, median of %d repetitions after one warm-up of each, wall milliseconds." % REPS)
out.append("")
out.append("plain JpegBatch   upload + decode + sync                      %8.2f" % med["plain_udS"])
out.append("plain JpegBatch   add_jpeg x %d + upload + decode + sync      %8.2f" % (N, med["plain_all"]))
out.append("plain JpegBatch   add_jpeg x %d again after clear() (staging area already grown)  %8.2f" % (N, med["readd"]))
out.append("plain JpegBatch   ... + dib_checksums                          %8.2f" % med["plain_all_hash"])
out.append("JpegJob 1 shard   run() (keep_resident, one round)             %8.2f   busiest shard thread %8.2f" % (med["job1"], med["job1_shard"]))
out.append("JpegJob 2 shards  run() (keep_resident, one round each)        %8.2f   busiest shard thread %8.2f" % (med["job2"], med["job2_shard"]))
out.append("")
out.append("ratio  job 1 shard  / plain upload + decode + sync             %8.3f" % (med["job1"] / med["plain_udS"]))
out.append("ratio  job 1 shard  / plain add + upload + decode + sync + checksums  %6.3f   (what run() does: staging, decode, per-file checksums)" % (med["job1"] / med["plain_all_hash"]))
out.append("ratio  job 2 shards / job 1 shard                              %8.3f" % (med["job2"] / med["job1"]))
out.append("")
out.append("all repetitions (ms):")
for k, v in rows.items():
    out.append("  %-16s %s" % (k, " ".join("%.2f" % x for x in v)))
out.append("checksum sum identical over every run: %016x" % sums.pop())
txt = "\n".join(out) + "\n"
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt)
print(txt)
