// jsnoop_job.cpp -- the job layer of include/jsnoop_gpu.h: "these N files" -> a result for each of them, from every device.
//
// The reference's batch loop (CJPEGsnoopCore::DoBatchFileProcess, source/JPEGsnoopCore.cpp:765-845, over the list GenBatchFileList :454
// builds) hosted on the whole node.  Scheduling only: every pixel comes out of the decode kernels behind JsnoopBatch, which this file
// drives through the C ABI; a job is built ON batches, not into them.
//
//   shard   = one host thread + two round slots, bound to one device (jsnoop_set_device on that thread)
//   slot    = a baseline batch and a progressive batch (a batch holds one kind), each with its own stream
//   round   = what a slot holds at a time, bounded by images and by jsnoop_batch_device_bytes
//
// A shard's thread:  stage(0);  for r = 0, 1, ...: { enqueue decode(r);  stage(r + 1) into the other slot once the callbacks of round r - 1
// have returned;  wait + fix-up + checksums of round r;  hand round r to the calling thread }.  The calling thread runs the callbacks.
//
// Shards of one device create batches concurrently.  What batch creation shares between threads was read for that case: the per-device
// unaligned-store probe of JsnoopBatch::init keeps its verdict in atomics (two threads may both probe, each on its own stream and buffer,
// and store the same verdict), the LDS opt-in of the back end's launch wrapper raises a per-device atomic monotonically, and the process
// defaults of the tuning struct are a function-local static (initialised once under the language's guarantee).  None of it needs a lock;
// batch creation is serialised here all the same, it costs nothing against a round.
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <filesystem>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "jsnoop_host.h"
#include "jsnoop_carve_check.h"

namespace {

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct JobEntry {
    std::vector<uint8_t> bytes; std::string path; bool is_path = false;
    JsnoopJobFile res; std::string msg; bool reported = false;
};
struct Slot {
    JsnoopBatch* bat[2] = { nullptr, nullptr };                   // [0] baseline, [1] progressive
    std::vector<int> files;                                       // the round's files in index order (refused and unreadable ones too)
    int round = 0; uint64_t dev_bytes = 0; bool handed = false;   // handed: with the calling thread (guarded by JsnoopJob::mu)
};
struct Shard {
    int id = 0, device = 0; std::vector<int> list; size_t pos = 0; Slot slot[2]; std::thread th; double ms = 0; int rounds = 0; uint64_t budget = 0;
    std::vector<uint8_t> carry; int carry_for = -1;               // bytes of the file that closed the last round (read once)
};

}  // namespace

struct JsnoopJob {
    std::vector<Shard> shards; std::deque<JobEntry> files;
    JsnoopJobOptions opt; JsnoopTuning tune; bool have_tune = false;
    std::mutex mu, create_mu; std::condition_variable cv;
    std::deque<std::pair<int, int>> done;                         // (shard, slot) rounds ready for their callbacks
    std::atomic<bool> cancel{ false }; bool failed = false; std::string fail_text;
    int planned = 0, running = 0; bool go = false, multi_round = false;      // keep_resident: every shard stages first, then all decode or none
    bool resident = false;                                        // the slots still hold the last run's batches for the caller

    void fail(const std::string& text)
    {
        std::lock_guard<std::mutex> l(mu);
        if (!failed) { failed = true; fail_text = text; }
        cancel.store(true); cv.notify_all();
    }
    void drop_batches()
    {
        for (Shard& s : shards) for (Slot& sl : s.slot) { for (JsnoopBatch*& b : sl.bat) if (b) { jsnoop_batch_destroy(b); b = nullptr; } sl.files.clear(); sl.handed = false; }
        for (JobEntry& e : files) { e.res.batch = nullptr; }
        resident = false;
    }
    JsnoopBatch* batch_of(Shard& s, Slot& sl, int kind);
    int  stage(Shard& s, Slot& sl);
    int  finish(Shard& s, Slot& sl);
    void work(Shard& s);
};

static void reset_result(JobEntry& e, int index)
{
    memset(&e.res, 0, sizeof e.res); e.res.struct_size = (uint32_t)sizeof e.res; e.res.index = index; e.res.status = JSNOOP_JOB_PENDING;
    e.res.shard = e.res.device = e.res.round = e.res.image = -1; e.msg.clear(); e.res.message = e.msg.c_str(); e.reported = false;
}

JsnoopBatch* JsnoopJob::batch_of(Shard& s, Slot& sl, int kind)
{
    JsnoopBatch*& b = sl.bat[kind];
    if (b) return b;
    std::lock_guard<std::mutex> l(create_mu);
    b = jsnoop_batch_create(nullptr);                              // on this thread's device (jsnoop_set_device in work())
    if (!b) return nullptr;
    jsnoop_batch_set_options(b, opt.decode_ac, opt.want_planes, 0);
    if ((have_tune && jsnoop_batch_set_tuning(b, &tune)) || (opt.enable_log && jsnoop_batch_enable_log(b, 1))) { jsnoop_batch_destroy(b); b = nullptr; }
    (void)s;
    return b;
}

// Fills the slot with the shard's next files.  0, or -1 on a device error (text in jsnoop_last_error() of this thread).
int JsnoopJob::stage(Shard& s, Slot& sl)
{
    for (JsnoopBatch* b : sl.bat) if (b) jsnoop_batch_clear(b);
    sl.files.clear(); sl.dev_bytes = 0; sl.round = s.rounds;
    const int max_images = opt.max_images_per_round > 0 ? opt.max_images_per_round : 1024;
    int nimg = 0;
    while (s.pos < s.list.size() && nimg < max_images && !cancel.load()) {
        const int idx = s.list[s.pos]; JobEntry& e = files[idx];
        e.res.shard = s.id; e.res.device = s.device; e.res.round = sl.round;
        const uint8_t* p = e.bytes.data(); size_t len = e.bytes.size();
        if (e.is_path) {
            if (s.carry_for != idx) {
                s.carry.clear(); s.carry_for = -1;
                FILE* f = fopen(e.path.c_str(), "rb");
                bool ok = f != nullptr;
                if (f) {
                    uint8_t tmp[65536]; size_t n;
                    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) s.carry.insert(s.carry.end(), tmp, tmp + n);
                    ok = !ferror(f); fclose(f);
                }
                if (!ok) {
                    e.res.status = JSNOOP_JOB_UNREADABLE; e.msg = "cannot read " + e.path; e.res.message = e.msg.c_str();
                    sl.files.push_back(idx); s.pos++; continue;
                }
                s.carry_for = idx;
            }
            p = s.carry.data(); len = s.carry.size();
        }
        const int kind = js_is_progressive(p, len) ? 1 : 0;
        JsnoopBatch* b = batch_of(s, sl, kind);
        if (!b) return -1;
        const JsBatchMark mark = js_batch_mark(b);
        const int img = jsnoop_batch_add_jpeg(b, p, len);
        if (img < 0) {
            e.res.status = JSNOOP_JOB_REFUSED; e.msg = jsnoop_last_error(); if (e.msg.empty()) e.msg = "refused by the front end";
            e.res.message = e.msg.c_str(); s.carry_for = -1;
            sl.files.push_back(idx); s.pos++; continue;
        }
        const uint64_t bytes = jsnoop_batch_device_bytes(sl.bat[0]) + jsnoop_batch_device_bytes(sl.bat[1]);
        if (bytes > s.budget && nimg > 0) { js_batch_rewind(b, mark); break; }      // closes the round; the file opens the next one (its bytes stay in carry)
        sl.dev_bytes = bytes;
        e.res.status = JSNOOP_JOB_OK; e.res.kind = kind + 1; e.res.batch = b; e.res.image = img; s.carry_for = -1;
        sl.files.push_back(idx); s.pos++; nimg++;
    }
    if (cancel.load()) return 0;                                  // (a cancelled job issues nothing more)
    for (JsnoopBatch* b : sl.bat) if (b && jsnoop_batch_count(b) > 0 && jsnoop_batch_upload(b)) return -1;
    return 0;
}

// Waits for the round, then collects what every result carries.
int JsnoopJob::finish(Shard& s, Slot& sl)
{
    std::vector<uint64_t> hash[2];
    for (int k = 0; k < 2; k++) {
        JsnoopBatch* b = sl.bat[k]; const int n = b ? jsnoop_batch_count(b) : 0;
        if (!n) continue;
        if (cancel.load()) return 1;
        if (jsnoop_batch_sync(b)) return -1;
        hash[k].resize((size_t)n);
        if (jsnoop_batch_dib_hashes(b, hash[k].data())) return -1;
    }
    for (int idx : sl.files) {
        JobEntry& e = files[idx];
        if (e.res.status != JSNOOP_JOB_OK) continue;
        if (jsnoop_batch_image_info(e.res.batch, e.res.image, e.res.info16)) return -1;
        e.res.dib_hash = hash[e.res.kind - 1][(size_t)e.res.image];
    }
    (void)s;
    return 0;
}

void JsnoopJob::work(Shard& s)
{
    const double t0 = now_ms();
    auto bail = [&](bool error) {
        if (error) fail("shard " + std::to_string(s.id) + " (device " + std::to_string(s.device) + "): " + jsnoop_last_error());
        s.ms = now_ms() - t0;
        std::lock_guard<std::mutex> l(mu); running--; cv.notify_all();
    };
    if (jsnoop_set_device(s.device)) return bail(true);
    int cur = 0;
    if (stage(s, s.slot[0])) return bail(true);
    if (opt.keep_resident) {                                       // all shards stage, then all decode or none does
        std::unique_lock<std::mutex> l(mu);
        planned++; if (s.pos < s.list.size()) multi_round = true;
        cv.notify_all();
        cv.wait(l, [&] { return go || cancel.load(); });
    }
    while (!cancel.load()) {
        Slot& sl = s.slot[cur];
        if (sl.files.empty()) break;                               // nothing left
        for (JsnoopBatch* b : sl.bat) if (b && jsnoop_batch_count(b) > 0 && jsnoop_batch_decode(b)) return bail(true);
        s.rounds++;
        Slot& nx = s.slot[cur ^ 1];
        {   // the other slot is the previous round's: its callbacks must have returned before it is refilled
            std::unique_lock<std::mutex> l(mu);
            cv.wait(l, [&] { return !nx.handed || cancel.load(); });
        }
        if (cancel.load()) break;
        if (stage(s, nx)) return bail(true);
        const int rc = finish(s, sl);
        if (rc < 0) return bail(true);
        if (rc > 0) break;
        { std::lock_guard<std::mutex> l(mu); sl.handed = true; done.emplace_back(s.id, cur); cv.notify_all(); }
        cur ^= 1;
    }
    bail(false);
}

static uint64_t file_cost(const JobEntry& e)
{
    if (!e.is_path) return e.bytes.size();
    std::error_code ec; const auto n = std::filesystem::file_size(e.path, ec);
    return ec ? 0 : (uint64_t)n;
}

extern "C" {

int jsnoop_partition_lpt(const uint64_t* costs, int n, int parts, int* part_of)
{
    if (n < 0 || parts < 1 || (n > 0 && (!costs || !part_of))) { js_set_error("jsnoop_partition_lpt: bad argument"); return -1; }
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return costs[a] > costs[b]; });      // (-cost, index)
    // loads may pass 2^64 where costs are near 2^63: two words, compared as the unbounded integers the rule is stated in
    std::vector<uint64_t> lo((size_t)parts, 0), hi((size_t)parts, 0);
    for (int i : order) {
        int r = 0;
        for (int k = 1; k < parts; k++) if (hi[(size_t)k] < hi[(size_t)r] || (hi[(size_t)k] == hi[(size_t)r] && lo[(size_t)k] < lo[(size_t)r])) r = k;
        const uint64_t before = lo[(size_t)r]; lo[(size_t)r] += costs[i]; if (lo[(size_t)r] < before) hi[(size_t)r]++;
        part_of[i] = r;
    }
    return 0;
}

JsnoopJob* jsnoop_job_create(const int* devices, int nshards)
{
    const int ndev = jsnoop_device_count();
    if (ndev <= 0) { js_set_error("no HIP device visible: libjsnoop_gpu has no CPU fallback"); return nullptr; }
    std::vector<int> devs;
    if (!devices || nshards <= 0) { for (int d = 0; d < ndev; d++) devs.push_back(d); }
    else devs.assign(devices, devices + nshards);
    if (devs.size() > JSNOOP_JOB_MAX_SHARDS) { js_set_error("jsnoop_job_create: %zu shards, at most %d", devs.size(), JSNOOP_JOB_MAX_SHARDS); return nullptr; }
    for (int d : devs) if (d < 0 || d >= ndev) { js_set_error("jsnoop_job_create: device %d not available (%d visible)", d, ndev); return nullptr; }
    JsnoopJob* j = new JsnoopJob;
    j->shards.resize(devs.size());
    for (size_t i = 0; i < devs.size(); i++) { j->shards[i].id = (int)i; j->shards[i].device = devs[i]; }
    jsnoop_job_options_defaults(&j->opt);
    return j;
}
void jsnoop_job_clear(JsnoopJob* j) { if (!j) return; j->drop_batches(); j->files.clear(); }
void jsnoop_job_destroy(JsnoopJob* j) { if (!j) return; j->drop_batches(); delete j; }
void jsnoop_job_options_defaults(JsnoopJobOptions* out)
{
    if (!out) return;
    memset(out, 0, sizeof *out); out->struct_size = (uint32_t)sizeof *out; out->decode_ac = 1;
}
int jsnoop_job_set_options(JsnoopJob* j, const JsnoopJobOptions* o)
{
    if (!j || !o) { js_set_error("jsnoop_job_set_options: null argument"); return -1; }
    if (o->struct_size < 8 || o->struct_size > sizeof(JsnoopJobOptions)) { js_set_error("job options: struct_size %u, this library has %zu", o->struct_size, sizeof(JsnoopJobOptions)); return -1; }
    JsnoopJobOptions in; jsnoop_job_options_defaults(&in);
    memcpy(&in, o, o->struct_size); in.struct_size = (uint32_t)sizeof in;
    if (in.max_images_per_round < 0 || in.partition < 0 || in.partition > 1) { js_set_error("job options: max_images_per_round >= 0, partition 0 or 1"); return -1; }
    if (j->resident) j->drop_batches();                            // (batches carry the options they were created with)
    j->opt = in;
    return 0;
}
int jsnoop_job_set_tuning(JsnoopJob* j, const JsnoopTuning* t)
{
    if (!j || !t) { js_set_error("jsnoop_job_set_tuning: null argument"); return -1; }
    JsnoopTuning in;
    if (js_import_tuning(t, &in)) return -1;
    if (j->resident) j->drop_batches();
    j->tune = in; j->have_tune = true;
    return 0;
}
int jsnoop_job_add_file(JsnoopJob* j, const uint8_t* file, size_t len)
{
    if (!j || (!file && len)) { js_set_error("jsnoop_job_add_file: null argument"); return -1; }
    j->files.emplace_back();
    JobEntry& e = j->files.back(); if (len) e.bytes.assign(file, file + len);
    reset_result(e, (int)j->files.size() - 1);
    return (int)j->files.size() - 1;
}
int jsnoop_job_add_carved(JsnoopJob* j, const uint8_t* blob, uint64_t len, const JsnoopCarveFrame* frames, int64_t nframes, int include_no_eoi, int* first_index)
{
    if (!j || (!blob && len)) { js_set_error("jsnoop_job_add_carved: null argument"); return -1; }
    std::vector<int64_t> pick;
    if (js_carve_pick(frames, nframes, len, include_no_eoi, &pick)) return -1;
    if (first_index) *first_index = pick.empty() ? -1 : (int)j->files.size();
    for (int64_t k : pick) if (jsnoop_job_add_file(j, blob + frames[k].start, (size_t)(frames[k].end - frames[k].start)) < 0) return -1;
    return (int)pick.size();
}
int jsnoop_job_add_path(JsnoopJob* j, const char* path)
{
    if (!j || !path) { js_set_error("jsnoop_job_add_path: null argument"); return -1; }
    j->files.emplace_back();
    JobEntry& e = j->files.back(); e.path = path; e.is_path = true;
    reset_result(e, (int)j->files.size() - 1);
    return (int)j->files.size() - 1;
}
int jsnoop_job_count(const JsnoopJob* j) { return j ? (int)j->files.size() : 0; }

int jsnoop_job_run(JsnoopJob* j, jsnoop_job_file_fn on_file, void* user, JsnoopJobStats* stats)
{
    if (!j) { js_set_error("jsnoop_job_run: no job"); return -1; }
    const double t0 = now_ms();
    const int n = (int)j->files.size(), ns = (int)j->shards.size();
    j->drop_batches();
    for (int i = 0; i < n; i++) reset_result(j->files[(size_t)i], i);
    j->cancel.store(false); j->failed = false; j->fail_text.clear(); j->done.clear();
    j->planned = 0; j->go = false; j->multi_round = false;

    // partition
    for (Shard& s : j->shards) { s.list.clear(); s.pos = 0; s.rounds = 0; s.ms = 0; s.carry.clear(); s.carry_for = -1; }
    if (j->opt.partition == 1) {
        const int base = n / ns, rem = n % ns; int start = 0;
        for (int r = 0; r < ns; r++) { const int cnt = base + (r < rem ? 1 : 0); for (int i = start; i < start + cnt; i++) j->shards[(size_t)r].list.push_back(i); start += cnt; }
    } else {
        std::vector<uint64_t> costs((size_t)n); std::vector<int> part((size_t)n);
        for (int i = 0; i < n; i++) costs[(size_t)i] = file_cost(j->files[(size_t)i]);
        if (jsnoop_partition_lpt(costs.data(), n, ns, part.data())) return -1;
        for (int i = 0; i < n; i++) j->shards[(size_t)part[(size_t)i]].list.push_back(i);     // (ascending within a shard)
    }
    // budget of a round: the caller's, or half of the device's free memory over the shards on it and the two slots
    int dev_before = 0; const bool have_before = hipGetDevice(&dev_before) == hipSuccess;
    for (Shard& s : j->shards) {
        s.budget = j->opt.max_round_bytes;
        if (!s.budget) {
            size_t free_b = 0, total_b = 0; int on_dev = 0;
            for (const Shard& o : j->shards) on_dev += o.device == s.device;
            hipError_t e = hipSetDevice(s.device);
            if (e == hipSuccess) e = hipMemGetInfo(&free_b, &total_b);
            if (e != hipSuccess) { js_set_error("jsnoop_job_run: hipMemGetInfo on device %d: %s", s.device, hipGetErrorString(e)); return -1; }
            s.budget = std::max<uint64_t>(1, (uint64_t)free_b / 2 / (uint64_t)on_dev / 2);
        }
    }
    if (have_before) (void)hipSetDevice(dev_before);

    j->running = ns;
    for (Shard& s : j->shards) s.th = std::thread([j, &s] { j->work(s); });

    JsnoopJobStats st; memset(&st, 0, sizeof st); st.nshards = ns;
    bool cancelled_by_cb = false, refuse_multi = false;
    {
        std::unique_lock<std::mutex> l(j->mu);
        if (j->opt.keep_resident) {
            j->cv.wait(l, [&] { return j->planned == ns || j->running < ns || j->cancel.load(); });
            if (j->planned == ns && !j->multi_round && !j->cancel.load()) j->go = true;
            else { refuse_multi = j->planned == ns && j->multi_round; j->cancel.store(true); }
            j->cv.notify_all();
        }
        for (;;) {
            j->cv.wait(l, [&] { return !j->done.empty() || j->running == 0; });
            if (j->done.empty()) break;                            // every worker has returned and nothing is queued
            const std::pair<int, int> it = j->done.front(); j->done.pop_front();
            Slot& sl = j->shards[(size_t)it.first].slot[it.second];
            l.unlock();
            if (!cancelled_by_cb && !j->cancel.load()) {
                st.rounds++; st.max_round_device_bytes = std::max(st.max_round_device_bytes, sl.dev_bytes);
                for (int idx : sl.files) {
                    JobEntry& e = j->files[(size_t)idx];
                    st.files++;
                    if (e.res.status == JSNOOP_JOB_OK) { st.ok++; st.flagged += e.res.info16[11] != 0; st.pixels += (uint64_t)e.res.info16[0] * e.res.info16[1]; st.dib_hash_sum += e.res.dib_hash; }
                    else if (e.res.status == JSNOOP_JOB_REFUSED) st.refused++; else st.unreadable++;
                    e.reported = true;
                    if (on_file && on_file(user, &e.res)) { cancelled_by_cb = true; j->cancel.store(true); break; }
                }
            }
            l.lock();
            sl.handed = false; j->cv.notify_all();
        }
    }
    for (Shard& s : j->shards) if (s.th.joinable()) s.th.join();
    for (int i = 0; i < n; i++) if (!j->files[(size_t)i].reported) reset_result(j->files[(size_t)i], i);     // staged, never handed over: no result
    for (int i = 0; i < ns; i++) st.shard_ms[i] = j->shards[(size_t)i].ms;
    const int rc = (j->failed || refuse_multi) ? -1 : (cancelled_by_cb ? 1 : 0);
    if (rc == 0 && j->opt.keep_resident) j->resident = true;
    else j->drop_batches();                                        // a result keeps everything but its handles
    st.wall_ms = now_ms() - t0;
    if (stats) {
        const uint32_t want = stats->struct_size; const size_t sz = (want >= 8 && want <= sizeof st) ? want : sizeof st;
        st.struct_size = (uint32_t)sz; memcpy(stats, &st, sz);
    }
    if (j->failed) js_set_error("jsnoop_job_run: %s", j->fail_text.c_str());
    else if (refuse_multi) js_set_error("jsnoop_job_run: keep_resident needs every shard's files in one round (raise max_round_bytes / max_images_per_round, or add shards)");
    return rc;
}

int jsnoop_job_file_result(const JsnoopJob* j, int index, JsnoopJobFile* out)
{
    if (!j || !out || index < 0 || (size_t)index >= j->files.size()) { js_set_error("jsnoop_job_file_result: file index out of range"); return -1; }
    const uint32_t want = out->struct_size; const size_t sz = (want >= 8 && want <= sizeof(JsnoopJobFile)) ? want : sizeof(JsnoopJobFile);
    JsnoopJobFile r = j->files[(size_t)index].res; r.struct_size = (uint32_t)sz;
    memcpy(out, &r, sz);
    return 0;
}

}  // extern "C"
