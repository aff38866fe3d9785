"""CPU half of the per-read statistics tests (tests/test_gpu_read_stats.py): for every directed batch of tests/rs_steps.py the
restatement (tests/rs_ref.py) and the oracle agree on every key the restatement models and on the error code, so that a failure on
the card cannot hide behind an input the reference refuses or behind a wrong restatement; every batch holds the values it was built
for; the constants and the launch rules restated in the two files are the sources'.

Where the oracle's DEFINED: choices decide an outcome (oracle/bamqc_oracle.c; the reference itself has undefined behaviour there):
  clips          a 5' clip longer than the read marks the read's own cycles only (cigar_count); a 3' clip longer than the read marks
                 nothing (the reference's unsigned loop start lies behind the read's end)
  lengths        a mapped read of no bases without a CIGAR counts as "no operations": deletions 0, insertions 0
  caps_wrap      NM < D + I wraps to about 2^32 in the reference's unsigned arithmetic: any count >= hist_cap ends the run"""
import os
import re

import numpy as np
import pytest

from bamqc_amd import _abi
from tests import rs_ref, rs_steps
from tests.parity import run_oracle, split
from tests.rs_ref import BQC_CT, RS_HB, RS_INS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bamqc_amd", "csrc")
NOMINAL_CU = 256  # the card's; the rule is checked for other counts as well


def both(cols_list, refs, opts):
    """(code, the restatement's counts, the oracle's counts), after the two have been compared."""
    rc_r, want = rs_ref.counts(cols_list, **opts)
    rc_o, got, _ = run_oracle(cols_list, refs, **opts)
    assert rc_r == rc_o, "error code: restatement %d, oracle %d" % (rc_r, rc_o)
    if rc_r == 0:
        d = rs_ref.diff(want, got)
        assert not d, "\n".join(d[:20])
    return rc_r, want, got


@pytest.mark.parametrize("name", list(rs_steps.BATCHES))
def test_restatement_and_oracle_agree(name):
    cols, refs, opts = rs_steps.made(name)
    rc, want, _ = both([cols], refs, opts)
    assert rc == rs_steps.BATCHES[name][1]
    L = cols["l_seq"]
    assert name in ("lengths", "lengths_over", "clips") or L.max() <= rs_ref.BQC_FAST_MAXLEN  # (k_short takes every read of the other batches)
    if rc == 0:
        REACHES[name.split("_")[0] if name.startswith("insert") else name](want[0], opts)


@pytest.mark.parametrize("name", rs_steps.SPLIT)
def test_split_batches_agree(name):
    cols, refs, opts = rs_steps.made(name)
    cut = (len(cols["flag"]) // 2) | 1
    rc, want, _ = both(split(cols, [cut]), refs, opts)
    assert rc == 0 and not _abi.diff_counts(want, rs_ref.counts(cols, **opts)[1])


def nonzero(c, key, bins):
    return all(len(c[key]) > b and c[key][b] > 0 for b in bins)


def reaches_bins(c, opts):
    edge = [RS_HB - 2, RS_HB - 1, RS_HB, RS_HB + 1, 200]
    for m in ("r1.", "r2."):
        for key in ("mismatch", "delhist", "inshist"):
            assert nonzero(c, m + key, [0, 1] + edge), m + key
            assert all(c[m + key][b] >= 6 for b in edge)  # three reads a value on either strand


def reaches_insert(c, opts):
    isize = opts["isize"]
    h = c["r1.insertSize"]
    assert len(h) == isize + 1 and not c["r2.insertSize"].any()
    for v in rs_steps.insert_values(isize):
        assert h[min(v, isize)] >= (2 if v == 0 else 4), v
    assert h[isize] >= 4 * sum(v >= isize for v in rs_steps.insert_values(isize)) + 3  # everything at and behind the cap, |INT32_MIN| included
    assert int(h.sum()) == 4 * len(rs_steps.insert_values(isize)) + 3                 # and none of the reads behind the gates
    assert (isize < RS_INS) == (isize in (500, 1023)) and (isize == RS_INS - 1) == (isize == 1023)


def reaches_lengths(c, opts):
    for m in ("r1.", "r2."):
        assert nonzero(c, m + "readLength", rs_steps.LENGTHS), m
    assert c["r1.readLength"][rs_steps.LENGTHS_MAX] == 1 and len(c["r1.readLength"]) == opts["max_read_len"] + 1
    assert int(c["scalars"][rs_ref.S_TOTALBPS]) == 2 * sum(rs_steps.LENGTHS) + rs_steps.LENGTHS_MAX > 1 << 18
    assert c["r1.delhist"][0] == len(rs_steps.LENGTHS) + 1  # (the read without a CIGAR among them)


def reaches_clips(c, opts):
    for m in ("r1.", "r2."):
        sc5, sc3 = c[m + "sc5"], c[m + "sc3"]
        assert len(sc5) == 400 and sc5[BQC_CT - 2] == 6 and sc5[BQC_CT - 1] == 4 and sc5[BQC_CT] == 2 and sc5[BQC_CT + 1] == 0  # 400-base reads, both strands
        assert sc5[28] == 14 and sc5[29] == 12 and sc5[30] == 6  # 30-base reads: clips of 29; of 30 (twice) and 35; then the 400-base reads alone
        assert sc3[BQC_CT - 2] > sc3[BQC_CT - 1] > sc3[BQC_CT] > sc3[BQC_CT + 1] == 0  # reads of 303, 304 and 305 bases clipped at 3'
        assert sc3[0] == 2 * 4  # whole reads clipped at 3': 30, 303, 304 and 305 bases
        assert sc3[28] < sc3[29]  # clips of 1


def reaches_clip_cancel(c, opts):
    k = rs_steps.CANCEL_K
    assert c["r1.sc3"][99] == k and c["r1.sc3"][100] == k and c["r1.sc3"][109] == k and c["r1.sc3"][89] == 0 and len(c["r1.sc3"]) == 110
    assert c["r2.sc3"][70] == 2 * k and c["r2.sc3"][99] == 2 * k and c["r2.sc3"][69] == 0 and len(c["r2.sc3"]) == 100


def reaches_caps(c, opts):
    cap = opts["hist_cap"]
    for m in ("r1.", "r2."):
        for key in ("mismatch", "delhist", "inshist"):
            assert len(c[m + key]) == cap and c[m + key][cap - 1] >= 2, m + key
    assert c["r1.mismatch"][cap - 1] == 3 and c["r2.mismatch"][RS_HB] == 1  # the further NM tags


def reaches_flags(c, opts):
    assert all(int(v) > 0 for v in c["scalars"])
    for m in ("r1.", "r2."):
        assert nonzero(c, m + "mapQ", rs_steps.MAPQS) and len(c[m + "mapQ"]) == 256


REACHES = {"bins": reaches_bins, "insert": reaches_insert, "lengths": reaches_lengths, "clips": reaches_clips, "clip_cancel": reaches_clip_cancel,
           "caps": reaches_caps, "flags": reaches_flags}


def test_flag_combinations_are_complete():
    ok, bad = rs_steps.flag_values(False), rs_steps.flag_values(True)
    assert len(ok) + len(bad) == 2048 == len(set(ok) | set(bad)) and len(bad) == 128  # (the seven other bits)
    cols = rs_steps.made("flags")[0]
    assert sorted(set((cols["flag"] & 0xFFF).tolist())) == sorted(rs_steps.P | f for f in ok)
    assert all(((cols["rid"] == r) & (cols["flag"] == cols["flag"][k])).sum() == 1 for r in (0, 1) for k in (0, 77, 3000))


# ---------------------------------------------------------------------------------------------------------------------------
# flush_reuse
# ---------------------------------------------------------------------------------------------------------------------------
def test_flush_reuse_small_card():
    """The batch for a card of 16 CUs (the card's own count makes the same batch, longer): the restatement against the oracle, the
    parity of every bin, and the workgroups that cross."""
    n_cu = 16
    cols, refs, opts = rs_steps.made_flush(n_cu)
    rc, want, _ = both([cols], refs, opts)
    assert rc == 0
    for g, c in enumerate(want):
        odd = g & 1
        for m in ("r1.", "r2."):
            for key in ("readLength", "mapQ", "mismatch", "delhist", "inshist") + (("insertSize",) if m == "r1." else ()):
                h = c[m + key]
                assert h[odd::2].sum() > 0 and not h[1 - odd::2].any(), (g, m + key)
    short, reads = rs_steps.flush_crossings(cols, n_cu)
    assert short and reads
    shuffled = rs_steps.made_flush(n_cu, True)[0]
    rc, again, _ = both([shuffled], refs, opts)
    assert rc == 0 and not _abi.diff_counts(want, again)
    assert rs_steps.flush_crossings(shuffled, n_cu) == (short, reads)
    rc, twice, _ = both([cols, shuffled], refs, opts)  # the second part on top of the first
    assert rc == 0 and all(np.array_equal(t["r1.mapQ"], 2 * w["r1.mapQ"]) for t, w in zip(twice, want))


@pytest.mark.parametrize("n_cu", [1, 8, 64, 104, NOMINAL_CU, 304])
def test_flush_reuse_crosses_on_every_card(n_cu):
    """The launch rules alone, on the lane, flag and length columns the batch would have (no read is built)."""
    sizes = rs_steps.flush_sizes(n_cu)
    n = sum(sizes)
    cols = dict(lane=np.repeat(np.arange(3), sizes).astype(np.uint8), l_seq=np.full(n, 21, np.uint32),
                flag=np.where(np.arange(n) % 2 == 0, rs_steps.FIRST, rs_steps.LAST).astype(np.uint16))
    short, reads = rs_steps.flush_crossings(cols, n_cu)
    assert 0 in short and 0 in reads
    assert rs_steps.grid_reads(cols, True, n_cu) == rs_steps.READS_GRID_PER_CU * n_cu
    assert len(rs_steps.chunk_lanes_short(cols)) == n // 1024 and len(rs_steps.chunk_lanes_reads(cols, True)) == n // rs_steps.CHUNK_READS
    assert not rs_steps.chunk_lanes_reads(cols, False) and rs_steps.grid_reads(cols, False, n_cu) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the constants and the rules against the sources
# ---------------------------------------------------------------------------------------------------------------------------
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


def test_constants_are_the_sources():
    rs, dt, ks, kp, pl, kr = (_src(f) for f in ("read_stats.h", "device_types.h", "k_short.hip", "k_prep.hip", "bqc_pipeline.cpp", "k_reads.hip"))
    assert _one(r"#define RS_HB\s+(\d+)", rs) == RS_HB
    assert _one(r"#define RS_INS\s+(\d+)", rs) == RS_INS
    assert re.search(r"#define RS_CT\s+BQC_CT\b", rs)
    assert _one(r"#define BQC_CT\s+(\d+)", dt) == BQC_CT
    assert _one(r"#define BQC_FAST_MAXLEN\s+(\d+)", dt) == rs_ref.BQC_FAST_MAXLEN
    assert _one(r"#define BQC_CHUNK_READS\s+(\d+)", dt) == rs_steps.CHUNK_READS
    assert _one(r"#define BQC_SW_READS\s+(\d+)", dt) == rs_steps.SW_READS
    assert _one(r"#define BQC_FAST_WAVES\s+(\d+)", dt) == rs_steps.FAST_WAVES
    assert 8 * _one(r"#define BQC_FAST_NH\s+(\d+)", dt) == rs_steps.LANE_CYCLES
    # the error bits' meaning
    assert _one(r"BQC_ERR_NO_MATE_FLAG = (\d+)", open(os.path.join(ROOT, "include", "bamqc.h")).read()) == rs_ref.ERR_NO_MATE_FLAG
    assert _one(r"BQC_ERR_RANGE = (\d+)", open(os.path.join(ROOT, "include", "bamqc.h")).read()) == rs_ref.ERR_RANGE
    # the launch rules restated in rs_steps.py
    assert re.search(r"for \(uint32_t ci = blockIdx\.x; ci < n_chunks; ci \+= gridDim\.x\)", kr)
    assert re.search(r"uint32_t ci = blockIdx\.x, ci_step = gridDim\.x, ci_end = n_chunks;", ks)
    assert re.search(r"std::min\(m\.n_chunks_slow_ub, c->n_cu \* %d\), 0, c->stream\)" % rs_steps.READS_GRID_PER_CU, pl)
    assert re.search(r"const uint64_t cs_cap = H\.n_slow / BQC_CHUNK_READS \+ n_st \+ 4;", pl)
    assert re.search(r"const uint32_t grid = c->n_cu; // one workgroup per CU", pl)
    assert re.search(r"s_fast_w = max\(1u, \(m \+ 8 \* BQC_FAST_NH - 1\) / \(8 \* BQC_FAST_NH\)\);", kp)
    assert re.search(r"const uint32_t fast_w = s_fast_w, rpw = 64u / fast_w, h0 = \(rpw \+ 1\) / 2, h1 = rpw / 2;", kp)
    assert re.search(r"const uint32_t groups_cap = BQC_FAST_WAVES \* \(64u / rpw\);", kp)
    assert re.search(r"g = max\(\(c\.n0 \+ h0 - 1\) / h0, \(c\.n1 \+ h1 - 1\) / h1\);", kp)
    assert re.search(r"return !a\.no_fast && L <= BQC_FAST_MAXLEN \? \(\(flag & 0x40u\) \? 0u : 1u\) : 2u;", kp)


def _defines(text, prefix):
    """The #define lines NAME value of `text` whose name starts with prefix and whose value is an integer expression over earlier ones."""
    env = {}
    for name, expr in re.findall(r"^#define (%s\w*)[ \t]+(.+?)\s*(?://.*)?$" % prefix, text, re.M):
        expr = re.sub(r"(\d+)u\b", r"\1", expr).replace("/", "//")
        try:
            env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
        except Exception:
            pass
    return env


def test_lds_map_fits():
    """read_stats.h's map: the tables follow each other without a gap in the order the flush assumes, and the kernels' LDS fits: k_reads
    declares RS_WORDS statically (64 KiB at the most), k_short asks for KS_WORDS dynamically, which must fit the 160 KiB of a CU of
    gfx950 (the other tables of k_short take more than 64 KiB on their own: 65 536 packed 8-mer counters)."""
    dt = _defines(_src("device_types.h"), "BQC_")
    env = dict(dt)
    text = _src("read_stats.h")
    for name, expr in re.findall(r"^#define (RS_\w+)[ \t]+(.+?)\s*(?://.*)?$", text, re.M):
        env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
    ct, hb = BQC_CT, RS_HB
    assert env["RS_M_READLEN"] == 1 and env["RS_M_MAPQ"] == 1 + ct + 1 and env["RS_M_MM"] == env["RS_M_MAPQ"] + 256
    assert (env["RS_M_DEL"], env["RS_M_INS"], env["RS_M_SC5"]) == (env["RS_M_MM"] + hb, env["RS_M_MM"] + 2 * hb, env["RS_M_MM"] + 3 * hb)
    assert env["RS_M_SC3"] == env["RS_M_SC5"] + ct + 1 and env["RS_M_WORDS"] == env["RS_M_SC3"] + ct + 1
    assert env["RS_MATE"] == 16 and env["RS_INSERT"] == 16 + 2 * env["RS_M_WORDS"] and env["RS_WORDS"] == env["RS_INSERT"] + RS_INS
    assert env["RS_WORDS"] * 4 <= 64 * 1024
    ks = _src("k_short.hip")
    kenv = dict(env, KS_NH=dt["BQC_FAST_NH"], KS_WAVES=dt["BQC_FAST_WAVES"])
    for name, expr in re.findall(r"^#define (KS_\w+)[ \t]+(.+?)\s*(?://.*)?$", ks, re.M):
        if name in kenv:
            continue
        expr = re.sub(r"(\d+)u\b", r"\1", expr).replace("/", "//")
        if name == "KS_META":  # KS_LUT + the mask table, padded to a multiple of four words
            assert expr.startswith("(KS_LUT + (KS_NB + 1) * KS_LUTW + (((KS_NB + 1) * KS_LUTW) % 4 ? 4 - "), expr
            table = (kenv["KS_NB"] + 1) * kenv["KS_LUTW"]
            kenv[name] = kenv["KS_LUT"] + table + (-table) % 4
            continue
        m = re.fullmatch(r"\((.+?) \? (.+?) : (.+)\)", expr)
        if m:
            expr = "(%s if %s else %s)" % (m.group(2), m.group(1), m.group(3))
        kenv[name] = int(eval(expr, {"__builtins__": {}}, dict(kenv)))
    assert kenv["KS_WORDS"] == kenv["KS_RS"] + env["RS_WORDS"] and kenv["KS_T8"] == 0 and kenv["KS_TRIP"] == 16384
    assert 64 * 1024 < kenv["KS_WORDS"] * 4 <= 160 * 1024
    assert re.search(r"hipFuncAttributeMaxDynamicSharedMemorySize, KS_WORDS \* 4\)", ks)
