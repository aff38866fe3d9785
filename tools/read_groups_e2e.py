"""Whole-program wall time on a synthetic BAM file with several read groups, the reader on the card, with the coverage anchors made on
the card (BQC_DEVICE_ANCHORS=1) and by the host's pass (=0), run alternately; the median of the runs of each, and the [timing] lines of
the last run of each.  Run it once with 1 read group and once with several to compare the two files of the same size.
usage: python tools/read_groups_e2e.py [n_reads] [n_read_groups] [runs] [dir]"""
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bamqc_amd import hostio  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
n_lanes = int(sys.argv[2]) if len(sys.argv) > 2 else 8
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
d = sys.argv[4] if len(sys.argv) > 4 else "/tmp"
names = ["chr%d" % i for i in range(1, 23)]
lens = [int(100_000_000 * n / 10_000_000 // 22) + 1_000_000] * 22
bam, fa = os.path.join(d, "rg%d_%d.bam" % (n_lanes, n)), os.path.join(d, "rg%d_%d.fa" % (n_lanes, n))
if not os.path.exists(bam):
    t0 = time.time()
    hostio.synth_stream(bam, fa, 2024, n, names, lens, n_lanes=n_lanes)
    print("wrote %s (%.1f MB) in %.1f s" % (bam, os.path.getsize(bam) / 1e6, time.time() - t0), flush=True)
walls = {"1": [], "0": []}
last = {}
for k in range(runs):
    for anchors in ("1", "0"):
        out = os.path.join(d, "rg_out_%s.bamqc" % anchors)
        env = dict(os.environ, BQC_GPU_DECODE="1", BQC_TIMING="1", BQC_DEVICE_ANCHORS=anchors)
        t0 = time.time()
        r = subprocess.run([EXE, "-r", fa, "-o", out, bam], env=env, capture_output=True, text=True)
        walls[anchors].append(time.time() - t0)
        if r.returncode:
            sys.exit("bamqualcheck failed: %s" % r.stderr[-2000:])
        last[anchors] = [ln for ln in r.stderr.splitlines() if ln.startswith("[timing]")]
same = open(os.path.join(d, "rg_out_1.bamqc"), "rb").read() == open(os.path.join(d, "rg_out_0.bamqc"), "rb").read()
print("%d reads, %d read groups: anchors on the card %.3f s, host pass %.3f s (medians of %d, alternating); outputs %s" %
      (n, n_lanes, statistics.median(walls["1"]), statistics.median(walls["0"]), runs, "identical" if same else "DIFFER"))
print("  card: %s" % " ".join("%.3f" % x for x in walls["1"]))
print("  host: %s" % " ".join("%.3f" % x for x in walls["0"]))
for anchors in ("1", "0"):
    print("--- BQC_DEVICE_ANCHORS=%s, last run" % anchors)
    for ln in last[anchors]:
        print("  " + ln)
