"""The anchor kernels (csrc/k_anchor.hip) alone on one batch of sorted reads with N read groups: bqc_anchor_enqueue + complete, over
and over on a fresh context (the handles are completed and held, never submitted).  Run it under `rocprofv3 --kernel-trace --stats`
for the kernels' device time, one read-group count per run; prints the host-side time of an enqueue + sync + complete.
usage: python tools/anchor_kernels_time.py [n_reads] [n_read_groups] [iterations]"""
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bamqc_amd import Aggregator, _lib, synth  # noqa: E402
from tests.hipmem import Hip  # noqa: E402
from tests.test_gpu_anchor import device_batch  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
n_lanes = int(sys.argv[2]) if len(sys.argv) > 2 else 1
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
lens = [1_000_000] * 4  # (a 4 Mb span: even with 32 groups a group's reads are ~130 positions apart, as in a 30x genome split over lanes)
lib = _lib.load()
cols = synth.batch(1003, n, lens, None, n_lanes=n_lanes)
agg = Aggregator(n_refs=4, n_lanes=n_lanes, max_read_len=1024)
hip = Hip()
try:
    b, d_cov = device_batch(hip, cols)
    ts = []
    for it in range(iters):
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = lib.bqc_anchor_enqueue(agg.h, C.byref(b), d_cov, None, C.byref(h))
        assert rc == 0, rc
        assert hip.rt.hipDeviceSynchronize() == 0
        rc = lib.bqc_anchor_complete(agg.h, h, None)
        assert rc == 0, rc
        ts.append(time.perf_counter() - t0)
    print("%d reads, %d read groups: enqueue + sync + complete %.3f ms (median of %d; first %.3f ms)" %
          (n, n_lanes, 1e3 * statistics.median(ts[1:] or ts), iters, 1e3 * ts[0]))
    agg.close()
finally:
    hip.free()
