#!/bin/bash
# The host's SAM text reader (header lines, the line parser, lines from a FILE* and from memory) under ASan + UBSan on the wild file
# of tests/sam_sweeps.py, the odd and bad lines, and 100 randomly damaged copies.  A stand-alone program on the CPU.
# Usage: tools/asan_sam_text.sh
set -e
cd "$(dirname "$0")/.."
T=$(mktemp -d)
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -o $T/check tools/sam_text_check.cpp \
    bamqc_amd/host/bam_io.cpp bamqc_amd/host/bgzf.cpp bamqc_amd/host/inflate_fast.cpp bamqc_amd/host/crc32_fast.cpp tools/gpu_inflate_stub.cpp -lz -lpthread
python - "$T" <<'PY'
import sys, random
sys.path.insert(0, ".")
import numpy as np
from tests import sam_sweeps
T = sys.argv[1]
sam_sweeps.wild(T + "/wild.sam")
rng = np.random.default_rng(2)
lines = [l for _, l in sam_sweeps.odd_lines(rng)]
open(T + "/odd.sam", "w").write(sam_sweeps.header() + "\n".join(lines) + "\n")
for k, (_, line, _, _) in enumerate(sam_sweeps.bad_lines(rng)):
    open(T + "/bad%d.sam" % k, "w").write(sam_sweeps.header() + sam_sweeps.plain_line(rng, "g") + "\n" + line + "\n")
data = open(T + "/wild.sam", "rb").read()
r = random.Random(1)
for k in range(100):
    d = bytearray(data)
    for _ in range(r.choice((1, 3, 10, 100))):
        i = r.randrange(len(d))
        d[i] = r.choice((9, 10, 13, 0, 42, 58, 64, r.randrange(256)))
    if k % 5 == 0:
        d = d[:r.randrange(len(d))]
    open(T + "/d%03d.sam" % k, "wb").write(d)
PY
$T/check $T/wild.sam $T/odd.sam $T/bad*.sam $T/d*.sam > $T/out.txt 2>&1 || { tail -40 $T/out.txt; echo "FAILED (sanitizer report, crash, or FILE* and memory disagree)"; exit 1; }
grep -q "wild.sam: 3000 records rc 0" $T/out.txt && grep -q "odd.sam: 6 records rc 0" $T/out.txt || { grep -E "wild|odd" $T/out.txt; echo "FAILED"; exit 1; }
[ "$(grep -c '/bad[0-9].sam: 0 records rc [167] ' $T/out.txt)" = 8 ] || { grep bad $T/out.txt; echo "FAILED (bad lines)"; exit 1; }
if grep -q "runtime error\|AddressSanitizer" $T/out.txt; then grep -n "runtime error\|AddressSanitizer" $T/out.txt | head; echo FAILED; exit 1; fi
echo "ok: $(grep -c 'records rc 0' $T/out.txt) files read completely, $(grep -c 'records rc [1-9]' $T/out.txt) ended at an error, no sanitizer report"
rm -rf $T
