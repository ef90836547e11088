// jsnoop_coef_hist.cpp -- jsnoop_batch_pack_coef_hist / _read_coef_hist: the histogram of every DCT frequency of any list of (image, component) pairs of a
// decoded batch, one row per pair (kernel: jsnoop_coef_hist.hip; checks and records: jsnoop_coef_hist_check.h; the binning: jsnoop_coef_bin.h).
#include "jsnoop_host.h"
#include "jsnoop_launch.h"
#include "jsnoop_coef_hist_check.h"

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    js_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); return -1; } } while (0)

static int chist_dqt(void* ctx, int image, int comp, uint16_t* out64) { return jsnoop_batch_image_dqt(static_cast<const JsnoopBatch*>(ctx), image, comp, out64); }

// The pack's block, event and place on the batch stream: one H2D copy of the call's records, the rows' initialisation and one launch, nothing waited for --
// except behind a DC-only fast-form decode, whose arena does not hold the blocks: the batch is then decoded once more in the generic form (ensure_generic,
// as jsnoop_batch_read_coefs does), after every argument has passed its checks.
int JsnoopBatch::pack_coef_hist(const JsnoopCoefHistSpec* spec_in, const int* images, const int* comps, int n, void* dst, uint64_t row_pitch_words)
{
    if (!uploaded || last_form == 0 || !dev.coef || !dev.dccum) { js_set_error("pack_coef_hist: the batch has not been decoded"); return -1; }
    JsnoopCoefHistSpec spec;
    if (js_coef_hist_import_spec(spec_in, &spec)) return -1;
    if (n < 0) { js_set_error("pack_coef_hist: n = %d", n); return -1; }
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(device));
    const size_t rec_bytes = (size_t)n * sizeof(JsCoefHistRec), total = rec_bytes + ((size_t)n + 1) * 8;
    if (pack_block(total)) return -1;
    JsCoefHistRec* recs = reinterpret_cast<JsCoefHistRec*>(h_pack); uint64_t* base = reinterpret_cast<uint64_t*>(h_pack + rec_bytes);
    if (js_coef_hist_plan(imgs.data(), imgs.size(), spec, images, comps, n, dst, row_pitch_words, chist_dqt, this, recs, base)) return -1;
    if (ensure_generic()) return -1;
    if (pack_send(total)) return -1;
    if (js_launch_coef_hist(stream, dev.coef, dev.dccum, reinterpret_cast<const JsCoefHistRec*>(d_pack), reinterpret_cast<const uint64_t*>(d_pack + rec_bytes), (uint32_t)n, base[n],
                            spec.order, spec.range, dst, js_coef_hist_pitch(row_pitch_words, js_chist_words(spec.range)))) {
        js_set_error("pack_coef_hist: launch failed: %s", hipGetErrorString(hipGetLastError())); return -1; }
    return 0;
}

int JsnoopBatch::read_coef_hist(const JsnoopCoefHistSpec* spec_in, const int* images, const int* comps, int n, uint32_t* host_dst)
{
    if (n > 0 && !host_dst) { js_set_error("read_coef_hist: host_dst is NULL"); return -1; }
    if (n <= 0) return pack_coef_hist(spec_in, images, comps, n, nullptr, 0);
    if (!uploaded || last_form == 0 || !dev.coef || !dev.dccum) { js_set_error("pack_coef_hist: the batch has not been decoded"); return -1; }
    JsnoopCoefHistSpec spec;
    if (js_coef_hist_import_spec(spec_in, &spec)) return -1;
    HIP_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)n * js_chist_words(spec.range) * 4;
    if (bytes > d_chist_rows_cap) {                              // (hipFree waits for the device: no earlier call still uses the old block)
        if (d_chist_rows) hipFree(d_chist_rows);
        d_chist_rows = nullptr; d_chist_rows_cap = 0;
        HIP_TRY(hipMalloc((void**)&d_chist_rows, bytes));
        d_chist_rows_cap = bytes;
    }
    if (pack_coef_hist(&spec, images, comps, n, d_chist_rows, 0)) return -1;
    HIP_TRY(hipMemcpyAsync(host_dst, d_chist_rows, bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return 0;
}

extern "C" {

void jsnoop_coef_hist_spec_defaults(JsnoopCoefHistSpec* out) { if (out) js_coef_hist_spec_defaults(out); }
uint32_t jsnoop_coef_hist_words(const JsnoopCoefHistSpec* spec_in)
{
    JsnoopCoefHistSpec spec;
    return js_coef_hist_import_spec(spec_in, &spec) ? 0u : js_chist_words(spec.range);
}
int jsnoop_batch_pack_coef_hist(JsnoopBatch* b, const JsnoopCoefHistSpec* spec, const int* images, const int* comps, int n, void* dst, uint64_t row_pitch_words)
{
    if (!b) { js_set_error("pack_coef_hist: batch is NULL"); return -1; }
    return b->pack_coef_hist(spec, images, comps, n, dst, row_pitch_words);
}
int jsnoop_batch_read_coef_hist(JsnoopBatch* b, const JsnoopCoefHistSpec* spec, const int* images, const int* comps, int n, uint32_t* host_dst)
{
    if (!b) { js_set_error("pack_coef_hist: batch is NULL"); return -1; }
    return b->read_coef_hist(spec, images, comps, n, host_dst);
}

} // extern "C"
