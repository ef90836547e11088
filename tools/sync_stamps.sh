cp jpegsnoop_amd/libjsnoop_gpu.so /tmp/orig.so; cp gpurun_variants/lib_r06_syncstamp.so jpegsnoop_amd/libjsnoop_gpu.so
LOG=${SYNCSTAMP_LOG:-syncstamp.log}
python bench.py --full --images 128 --distinct 16 --steps 1 --warmup 0 --cpu-seconds 0 --no-extras --no-split > $LOG 2>&1
cp /tmp/orig.so jpegsnoop_amd/libjsnoop_gpu.so
grep -c STAMP $LOG
python - $LOG <<'PY'
import re, sys
T=V=L=N=0; n=0
for l in open(sys.argv[1]):
    if l.startswith('STAMP'):
        a=l.split(); T+=int(a[2]); V+=int(a[3]); L+=int(a[4]); N+=int(a[5]); n+=1
print("walks", n, "cycles/walk", T/max(n,1), "vm wait frac", V/max(T,1), "lds wait frac", L/max(T,1), "refill events per walk", N/max(n,1), "vm wait per event", V/max(N,1))
PY
