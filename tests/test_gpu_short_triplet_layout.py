"""GPU parity of k_short's triplet bins at the edges of their LDS layout and of the branch-free bin atomics: every table
(fwd1st fwd2nd rev1st rev2nd) inside one wave, reads where all lanes hit one bin, flank mismatches and Ns, the quality
thresholds 20 and 94, last lanes with 1 to 15 valid cycles, segment tiles, and the BQC_SHORT_PARTS ablations."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import synth
from tests.parity import assert_parity

pytestmark = pytest.mark.gpu

P, PR, REV, FIRST, LAST = 0x1, 0x2, 0x10, 0x40, 0x80
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS4 = [P | PR | FIRST, P | PR | LAST, P | PR | FIRST | REV, P | PR | LAST | REV]  # one read of each table, in turn


def _read(ref, pos, L, flag, rng, ops=None, p_mm=0.0, p_n=0.0, quals=None):
    codes = np.pad(ref, (0, 300))[pos:pos + L].astype(np.int64)
    if p_mm:
        m = rng.random(L) < p_mm
        codes[m] = (codes[m] + rng.integers(1, 4, int(m.sum()))) % 4
    if p_n:
        codes[rng.random(L) < p_n] = 4
    seq = "".join("ACGTN"[int(c)] for c in codes)
    q = list(quals) if quals is not None else rng.integers(25, 41, size=L).tolist()
    ops = ops or [(L, "M")]
    nm = sum(n for n, c in ops if c in "ID")
    return synth.single_read(seq, q, ops, flag, pos=pos, mapq=60, as_=90, nm=nm)


def _ref(rng, n):
    return rng.integers(0, 4, size=n).astype(np.uint8)


def test_four_tables_in_one_wave():
    # 150 bp: 10 lanes per read, 6 reads per wave; consecutive reads cycle through the four tables, so every group of a wave
    # mixes them (both mates, both strands)
    rng = np.random.default_rng(501)
    ref = _ref(rng, 20_000)
    recs = [_read(ref, int(rng.integers(0, 19_000)), 150, FLAGS4[i % 4], rng, p_mm=0.01) for i in range(1200)]
    assert_parity(synth.concat(recs), [ref])


def test_homopolymer_and_low_complexity():
    # every lane of a read on one bin (homopolymers), or on two / three (di- and trinucleotide repeats), with and without
    # mismatches against a reference of the same runs
    rng = np.random.default_rng(502)
    parts = []
    for unit in ("A", "C", "G", "T", "AC", "GT", "CAG", "AT"):
        parts.append(np.array(["ACGT".index(c) for c in unit * (1500 // len(unit))], np.uint8))
    ref = np.concatenate(parts)
    recs = []
    for i in range(900):
        seg = i % len(parts)
        pos = seg * 1500 + int(rng.integers(0, 1500 - 160))
        recs.append(_read(ref, pos, int(rng.choice([150, 151, 100, 36])), FLAGS4[i % 4], rng, p_mm=0.02 if i % 3 == 0 else 0.0))
    assert_parity(synth.concat(recs), [ref])


def test_flank_mismatches_and_ns_at_lane_edges():
    # mismatches and Ns next to counted positions, in particular at the cycles where a lane's 16 end (15/16, 31/32, ...) and the
    # flank comes from the neighbouring lane
    rng = np.random.default_rng(503)
    ref = _ref(rng, 30_000)
    recs = []
    for i in range(1500):
        L = int(rng.choice([150, 151, 140, 64, 33]))
        pos = int(rng.integers(0, 29_000))
        codes = ref[pos:pos + L].astype(np.int64).copy()
        edge = [c for c in range(15, L, 16)] + [c for c in range(16, L, 16)]
        for c in rng.choice(edge, size=min(len(edge), int(rng.integers(1, 4))), replace=False):
            codes[c] = 4 if rng.random() < 0.4 else (codes[c] + int(rng.integers(1, 4))) % 4
        codes[rng.random(L) < 0.01] = 4
        seq = "".join("ACGTN"[int(c)] for c in codes)
        recs.append(synth.single_read(seq, rng.integers(20, 41, size=L).tolist(), [(L, "M")], FLAGS4[i % 4], pos=pos, mapq=60, as_=90))
    assert_parity(synth.concat(recs), [ref])


def test_quality_thresholds_20_and_94():
    # a position counts for 20 <= q <= 94: qualities on both sides of both limits, per cycle
    rng = np.random.default_rng(504)
    ref = _ref(rng, 20_000)
    qs = np.array([18, 19, 20, 21, 92, 93, 94, 95, 96, 127, 0, 40])
    recs = [_read(ref, int(rng.integers(0, 19_000)), 150, FLAGS4[i % 4], rng, p_mm=0.005, quals=rng.choice(qs, size=150))
            for i in range(1000)]
    assert_parity(synth.concat(recs), [ref])


@pytest.mark.parametrize("base", [16, 128, 240])
def test_last_lane_with_1_to_15_cycles(base):
    # read lengths base + r, r = 1..15: the last lane holds r valid cycles (past-the-end cycles read as code 0), mixed in one batch
    rng = np.random.default_rng(505 + base)
    ref = _ref(rng, 20_000)
    recs = []
    for i in range(600):
        L = base + 1 + i % 15
        recs.append(_read(ref, int(rng.integers(0, 19_500)), L, FLAGS4[(i // 15) % 4], rng, p_mm=0.01))
    assert_parity(synth.concat(recs), [ref], max_read_len=512)


def test_segment_tiles():
    # many multi-operation CIGARs: enough triplet-segment entries for whole segment tiles of every wave, next to read tiles
    rng = np.random.default_rng(506)
    ref = _ref(rng, 40_000)
    recs = []
    for i in range(3000):
        L = int(rng.choice([150, 151, 100]))
        a = int(rng.integers(5, L - 20))
        kind = i % 3
        if kind == 0: ops = [(a, "M"), (2, "D"), (L - a, "M")]
        elif kind == 1: ops = [(a, "M"), (1, "I"), (L - a - 1, "M")]
        else: ops = [(a // 2, "M"), (3, "N"), (a - a // 2, "M"), (2, "I"), (L - a - 2, "M")]
        recs.append(_read(ref, int(rng.integers(0, 39_000)), L, FLAGS4[i % 4], rng, ops=ops, p_mm=0.01, p_n=0.005))
    assert_parity(synth.concat(recs), [ref])


_ABLATION = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests import synth
from tests.parity import run_gpu, run_oracle
rng = np.random.default_rng(507)
ref = rng.integers(0, 4, size=20_000).astype(np.uint8)
recs = []
for i in range(800):
    L = 150 if i % 5 else 143
    pos = int(rng.integers(0, 19_000))
    ops = [(L, "M")] if i % 4 else [(60, "M"), (2, "D"), (L - 60, "M")]
    seq = "".join("ACGT"[int(c)] for c in ref[pos:pos + L])
    flag = [0x43, 0x83, 0x53, 0x93][i % 4]
    recs.append(synth.single_read(seq, [30] * L, ops, flag, pos=pos, mapq=60, as_=90, nm=2 if i % 4 == 0 else 0))
cols = synth.concat(recs)
rc_o, co, _ = run_oracle([cols], [ref], n_refs=1)
rc_g, cg, _ = run_gpu([cols], [ref], n_refs=1)
print(json.dumps({"rc": [rc_o, rc_g], "triplet_equal": bool(np.array_equal(co[0]["triplet"], cg[0]["triplet"])),
                  "triplets": int(cg[0]["triplet"].sum())}))
"""


@pytest.mark.parametrize("parts", [4, 12, 11, 7])
def test_short_parts_ablations_run(parts):
    # BQC_SHORT_PARTS is read once per process: a child per setting.  Every setting runs; with the triplet bit the triplet
    # counts still match the oracle
    env = dict(os.environ, BQC_SHORT_PARTS=str(parts))
    out = subprocess.run([sys.executable, "-c", _ABLATION, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["rc"] == [0, 0]
    if parts & 4:
        assert r["triplet_equal"] and r["triplets"] > 0
