"""jpegsnoop_amd -- MI355X-native JPEGsnoop scan-decode stage.

The product is `libjsnoop_gpu.so` (hand-written HIP kernels behind the C ABI of
include/jsnoop_gpu.h).  This package is its binding layer: `CimgDecode` mirrors the
reference's decoder object, `JpegBatch` is the batched submit, `JpegJob` decodes a mixed
file list over all devices.
"""
from .capi import load, last_error, LIB_PATH  # noqa: F401
from .imgdecode import CimgDecode, JpegBatch, JpegJob, JobFileResult, JpegPipeline, dib_checksum_numpy, stats_fields, coef_hist_fields  # noqa: F401
from .imgdecode import Carve, carve_host, JpegEncoder, JpegTransform  # noqa: F401
from .shard import partition_lpt, partition_contiguous, reduce_job_stats  # noqa: F401
