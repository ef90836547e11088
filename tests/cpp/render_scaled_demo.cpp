// libjpeg's reduced-size pixels of a batch through the C++ facade (jpegsnoop_amd/csrc/ImgDecodeGpu.h): CJPEGsnoopCoreGpu::BatchPackIjgScaled into device memory
// the program owns -- dense HWC uint8, R G B, the files listed backwards -- copied back and written as <out dir>/out<file index>.rgb, one line
// "<file index> <width> <height> <bytes>" per file -- for tests/test_gpu_pack_ijg_scaled.py, which holds them against the model.
// usage: render_scaled_demo outdir denom file...; exit 3 without a device.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../jpegsnoop_amd/csrc/ImgDecodeGpu.h"

int main(int argc, char** argv)
{
    if (argc < 4) { printf("usage: render_scaled_demo outdir denom file...\n"); return 2; }
    const unsigned denom = (unsigned)atoi(argv[2]);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { printf("no device: no CPU fallback\n"); return 3; }
    CJPEGsnoopCoreGpu core;
    core.BatchSetOptions(true, false);
    for (int a = 3; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb"); if (!f) { printf("cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> buf; uint8_t tmp[65536]; size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
        fclose(f);
        if (core.BatchAddFile(buf.data(), buf.size()) < 0) { printf("refused %s: %s\n", argv[a], jsnoop_last_error()); return 2; }
    }
    const int n = (int)core.GetBatchFileCount();
    if (!core.DoBatchProcess()) { printf("decode failed: %s\n", jsnoop_last_error()); return 2; }
    JsnoopPackSpec spec; jsnoop_pack_spec_defaults(&spec); spec.layout = JSNOOP_PACK_HWC; spec.dtype = JSNOOP_PACK_U8;
    std::vector<int> files; std::vector<uint64_t> off; std::vector<unsigned> ws, hs; uint64_t total = 0;
    for (int i = n - 1; i >= 0; i--) {
        unsigned w = 0, h = 0;
        if (!core.BatchIjgScaledSize(i, denom, w, h)) { printf("file %d is not rendered: %s\n", i, jsnoop_last_error()); return 2; }
        const uint64_t bytes = jsnoop_batch_pack_ijg_scaled_bytes(core.Handle(), &spec, denom, i);
        if (bytes != (uint64_t)w * h * 3) { printf("file %d: %llu bytes for %u x %u\n", i, (unsigned long long)bytes, w, h); return 2; }
        files.push_back(i); off.push_back(total); ws.push_back(w); hs.push_back(h); total += bytes;
    }
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, total) != hipSuccess) { printf("hipMalloc failed\n"); return 2; }
    std::vector<JsnoopPackDst> dst(files.size(), JsnoopPackDst{});
    for (size_t k = 0; k < files.size(); k++) dst[k].ptr = d + off[k];
    if (!core.BatchPackIjgScaled(spec, denom, files, dst)) { printf("BatchPackIjgScaled failed: %s\n", jsnoop_last_error()); return 2; }
    if (hipDeviceSynchronize() != hipSuccess) { printf("the device reports an error\n"); return 4; }
    std::vector<uint8_t> host(total);
    if (hipMemcpy(host.data(), d, total, hipMemcpyDeviceToHost) != hipSuccess) return 4;
    (void)hipFree(d);
    for (size_t k = 0; k < files.size(); k++) {
        const uint64_t len = (k + 1 < files.size() ? off[k + 1] : total) - off[k];
        const std::string path = std::string(argv[1]) + "/out" + std::to_string(files[k]) + ".rgb";
        FILE* f = fopen(path.c_str(), "wb"); if (!f) { printf("cannot write %s\n", path.c_str()); return 2; }
        const bool ok = fwrite(host.data() + off[k], 1, len, f) == len; fclose(f);
        if (!ok) return 2;
        printf("%d %u %u %llu\n", files[k], ws[k], hs[k], (unsigned long long)len);
    }
    return 0;
}
