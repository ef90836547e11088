// libjpeg's pixels of a batch through the C++ facade (jpegsnoop_amd/csrc/ImgDecodeGpu.h): CJPEGsnoopCoreGpu::BatchPackIjg into device memory the program
// owns -- dense HWC uint8, R G B, the files listed backwards -- copied back and written as <out dir>/out<file index>.rgb, one line "<file index> <bytes>" per
// file -- for tests/test_gpu_pack_ijg.py, which holds them against the model.  usage: render_demo outdir file...; exit 3 without a device.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../jpegsnoop_amd/csrc/ImgDecodeGpu.h"

int main(int argc, char** argv)
{
    if (argc < 3) { printf("usage: render_demo outdir file...\n"); return 2; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { printf("no device: no CPU fallback\n"); return 3; }
    CJPEGsnoopCoreGpu core;
    core.BatchSetOptions(true, false);
    for (int a = 2; a < argc; a++) {
        FILE* f = fopen(argv[a], "rb"); if (!f) { printf("cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> buf; uint8_t tmp[65536]; size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
        fclose(f);
        if (core.BatchAddFile(buf.data(), buf.size()) < 0) { printf("refused %s: %s\n", argv[a], jsnoop_last_error()); return 2; }
    }
    const int n = (int)core.GetBatchFileCount();
    if (!core.DoBatchProcess()) { printf("decode failed: %s\n", jsnoop_last_error()); return 2; }
    JsnoopPackSpec spec; jsnoop_pack_spec_defaults(&spec); spec.layout = JSNOOP_PACK_HWC; spec.dtype = JSNOOP_PACK_U8;
    std::vector<int> files; std::vector<uint64_t> off; uint64_t total = 0;
    for (int i = n - 1; i >= 0; i--) {
        if (!core.BatchIjgRenderable(i)) { printf("file %d is not rendered: %s\n", i, jsnoop_last_error()); return 2; }
        files.push_back(i); off.push_back(total); total += jsnoop_batch_pack_bytes(core.Handle(), &spec, i);
    }
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, total) != hipSuccess) { printf("hipMalloc failed\n"); return 2; }
    std::vector<JsnoopPackDst> dst(files.size(), JsnoopPackDst{});
    for (size_t k = 0; k < files.size(); k++) dst[k].ptr = d + off[k];
    if (!core.BatchPackIjg(spec, files, dst)) { printf("BatchPackIjg failed: %s\n", jsnoop_last_error()); return 2; }
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
        printf("%d %llu\n", files[k], (unsigned long long)len);
    }
    return 0;
}
