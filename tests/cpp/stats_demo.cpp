// The colour statistics of a batch through the C++ facade (jpegsnoop_amd/csrc/ImgDecodeGpu.h): CJPEGsnoopCoreGpu::BatchPackStats into device memory the
// program owns, copied back and printed as one line per file -- "<file index> <FNV-1a 64 of the row's 2482 words> <six totals>" -- for
// tests/test_gpu_batch_stats.py to compare with JpegBatch.stats_to_torch.  usage: stats_demo histo_en file...; exit 3 without a device.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../jpegsnoop_amd/csrc/ImgDecodeGpu.h"

int main(int argc, char** argv)
{
    if (argc < 3) { printf("usage: stats_demo histo_en file...\n"); return 2; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { printf("no device: no CPU fallback\n"); return 3; }
    CJPEGsnoopCoreGpu core;
    core.BatchSetOptions(true, true);
    for (int a = 2; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb"); if (!f) { printf("cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> buf; uint8_t tmp[65536]; size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
        fclose(f);
        if (core.BatchAddFile(buf.data(), buf.size()) < 0) { printf("refused %s: %s\n", argv[a], jsnoop_last_error()); return 2; }
    }
    const int n = (int)core.GetBatchFileCount();
    if (!core.DoBatchProcess()) { printf("decode failed: %s\n", jsnoop_last_error()); return 2; }
    std::vector<int> files; for (int i = n - 1; i >= 0; i--) files.push_back(i);            // listed backwards: row k is file n - 1 - k
    const uint64_t pitch = JSNOOP_STATS_WORDS + 6;
    uint32_t* d_rows = nullptr; uint32_t* d_tot = nullptr;
    if (hipMalloc((void**)&d_rows, (size_t)n * pitch * 4) != hipSuccess || hipMalloc((void**)&d_tot, (size_t)n * 24) != hipSuccess) { printf("hipMalloc failed\n"); return 2; }
    if (!core.BatchPackStats(atoi(argv[1]) != 0, files, d_rows, pitch, d_tot)) { printf("BatchPackStats failed: %s\n", jsnoop_last_error()); return 2; }
    if (hipDeviceSynchronize() != hipSuccess) { printf("the device reports an error\n"); return 4; }
    std::vector<uint32_t> rows((size_t)n * pitch), tot((size_t)n * 6);
    if (hipMemcpy(rows.data(), d_rows, rows.size() * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(tot.data(), d_tot, tot.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 4;
    for (int k = 0; k < n; k++) {
        uint64_t h = 0xcbf29ce484222325ull;
        const uint8_t* p = reinterpret_cast<const uint8_t*>(rows.data() + (size_t)k * pitch);
        for (size_t i = 0; i < (size_t)JSNOOP_STATS_WORDS * 4; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
        printf("%d %016llx %u %u %u %u %u %u\n", files[k], (unsigned long long)h, tot[k * 6], tot[k * 6 + 1], tot[k * 6 + 2], tot[k * 6 + 3], tot[k * 6 + 4], tot[k * 6 + 5]);
    }
    (void)hipFree(d_rows); (void)hipFree(d_tot);
    return 0;
}
