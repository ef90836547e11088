// jsnoop_stats.cpp -- jsnoop_batch_pack_stats / _read_stats: the colour statistics of a decoded batch, one row of JSNOOP_STATS_WORDS words per listed image, from the
// retained planes (kernels: jsnoop_stats.hip; checks and records: jsnoop_stats_check.h).
#include "jsnoop_host.h"
#include "jsnoop_launch.h"
#include "jsnoop_stats_check.h"

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    js_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

// The pack's block, event and place on the batch stream: one H2D copy of the call's records, two fills (the rows; the scratch), two launches, nothing waited for.
// Never decodes: the planes are what the decode enqueued last left, whichever form it took.
int JsnoopBatch::pack_stats(int histo_en, const int* images, int n, void* dst, uint64_t row_pitch_words, uint32_t* totals)
{
    if (!uploaded || last_form == 0 || !dev.imgs) { js_set_error("pack_stats: the batch has not been decoded"); return -1; }
    if (!opt_want_planes || !dev.planes) { js_set_error("pack_stats: the batch keeps no planes (want_planes)"); return -1; }
    if (n < 0) { js_set_error("pack_stats: n = %d", n); return -1; }
    if (n == 0) return 0;
    if (totals && ((uint64_t)(uintptr_t)totals & 3u)) { js_set_error("pack_stats: totals must be a multiple of 4"); return -1; }
    HIP_TRY(hipSetDevice(device));
    const size_t rec_bytes = ((size_t)n * sizeof(JsStatRec) + 15) & ~(size_t)15, total = rec_bytes + ((size_t)n + 1) * 8;
    if (pack_block(total)) return -1;
    JsStatRec* recs = reinterpret_cast<JsStatRec*>(h_pack); uint64_t* base = reinterpret_cast<uint64_t*>(h_pack + rec_bytes);
    uint64_t row_words = 0;
    if (js_stats_plan(imgs.data(), imgs.size(), images, n, dst, row_pitch_words, recs, base, &row_words)) return -1;
    const uint64_t units = base[n];
    const size_t scratch = (size_t)js_stats_scratch_bytes(n, row_words);
    if (scratch > d_stats_cap) {                                 // (hipFree waits for the device: no earlier call still uses the old block)
        if (d_stats) hipFree(d_stats);
        d_stats = nullptr; d_stats_cap = 0;
        HIP_TRY(hipMalloc((void**)&d_stats, scratch + scratch / 4 + 4096));
        d_stats_cap = scratch + scratch / 4 + 4096;
    }
    if (pack_send(total)) return -1;
    const uint64_t pitch = js_stats_pitch(row_pitch_words);
    HIP_TRY(hipMemset2DAsync(dst, (size_t)pitch * 4, 0, (size_t)JSNOOP_STATS_WORDS * 4, (size_t)n, stream));       // the rows, not what lies between them
    HIP_TRY(hipMemsetAsync(d_stats, 0, scratch, stream));
    uint32_t* tot = reinterpret_cast<uint32_t*>(d_stats);
    if (js_launch_stats_batch(stream, dev.planes, reinterpret_cast<const JsStatRec*>(d_pack), reinterpret_cast<const uint64_t*>(d_pack + rec_bytes), (uint32_t)n, units,
                              histo_en != 0, tot, tot + (size_t)n * JS_STATS_TOT_WORDS, totals)) {
        js_set_error("pack_stats: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    return 0;
}

int JsnoopBatch::read_stats(int histo_en, const int* images, int n, uint32_t* host_dst)
{
    if (n > 0 && !host_dst) { js_set_error("read_stats: host_dst is NULL"); return -1; }
    if (n <= 0) return pack_stats(histo_en, images, n, nullptr, 0, nullptr);
    if (!uploaded || last_form == 0 || !dev.imgs) { js_set_error("pack_stats: the batch has not been decoded"); return -1; }
    HIP_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)n * JSNOOP_STATS_WORDS * 4;
    if (bytes > d_stats_rows_cap) {
        if (d_stats_rows) hipFree(d_stats_rows);
        d_stats_rows = nullptr; d_stats_rows_cap = 0;
        HIP_TRY(hipMalloc((void**)&d_stats_rows, bytes));
        d_stats_rows_cap = bytes;
    }
    if (pack_stats(histo_en, images, n, d_stats_rows, 0, nullptr)) return -1;
    HIP_TRY(hipMemcpyAsync(host_dst, d_stats_rows, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

extern "C" {

int jsnoop_batch_pack_stats(JsnoopBatch* b, int histo_en, const int* images, int n, void* dst, uint64_t row_pitch_words, uint32_t* totals)
{
    if (!b) { js_set_error("pack_stats: batch is NULL"); return -1; }
    return b->pack_stats(histo_en, images, n, dst, row_pitch_words, totals);
}
int jsnoop_batch_read_stats(JsnoopBatch* b, int histo_en, const int* images, int n, uint32_t* host_dst)
{
    if (!b) { js_set_error("pack_stats: batch is NULL"); return -1; }
    return b->read_stats(histo_en, images, n, host_dst);
}

} // extern "C"
