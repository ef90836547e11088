// The lossless transform through the C++ facade (jpegsnoop_amd/csrc/ImgDecodeGpu.h): the files named on the command line are decoded as one batch and
// CJPEGsnoopCoreGpu::TransformJpeg writes every one of them transformed to <out dir>/out<k>.jpg -- for tests/test_gpu_transform.py, which holds them against
// the model's files.  usage: transform_demo outdir op edge grayscale file...; prints "<k> <result> <bytes>" per file; exit 3 without a device.
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../jpegsnoop_amd/csrc/ImgDecodeGpu.h"

int main(int argc, char** argv)
{
    if (argc < 6) { printf("usage: transform_demo outdir op edge grayscale file...\n"); return 2; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { printf("no device: no CPU fallback\n"); return 3; }
    CJPEGsnoopCoreGpu core;
    for (int k = 5; k < argc; k++) {
        FILE* f = fopen(argv[k], "rb"); if (!f) { printf("cannot read %s\n", argv[k]); return 2; }
        std::vector<uint8_t> data; uint8_t buf[4096]; size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
        fclose(f);
        if (core.BatchAddFile(data.data(), data.size()) < 0) { printf("BatchAddFile failed: %s\n", jsnoop_last_error()); return 2; }
    }
    if (!core.DoBatchProcess()) { printf("DoBatchProcess failed: %s\n", jsnoop_last_error()); return 2; }
    JsnoopTransformSpec spec; jsnoop_transform_spec_defaults(&spec);
    spec.op = atoi(argv[2]); spec.edge = atoi(argv[3]); spec.grayscale = (uint32_t)atoi(argv[4]);
    std::vector<int> results; std::vector<std::vector<uint8_t>> files;
    if (!core.TransformJpeg(spec, {}, results, files) || files.size() != (size_t)(argc - 5)) { printf("TransformJpeg failed: %s\n", jsnoop_last_error()); return 2; }
    for (size_t k = 0; k < files.size(); k++) {
        if (!files[k].empty()) {
            const std::string path = std::string(argv[1]) + "/out" + std::to_string(k) + ".jpg";
            FILE* f = fopen(path.c_str(), "wb"); if (!f) { printf("cannot write %s\n", path.c_str()); return 2; }
            const bool ok = fwrite(files[k].data(), 1, files[k].size(), f) == files[k].size(); fclose(f);
            if (!ok) return 2;
        }
        printf("%zu %d %zu\n", k, results[k], files[k].size());
    }
    return 0;
}
