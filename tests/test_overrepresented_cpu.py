"""No GPU: the restatement of the overrepresented sequences (tests/ovr_ref.py) held against itself — the loops against numpy — on every
batch of tests/ovr_steps.py, and every batch against the edge it is named for."""
import os
import re

import numpy as np
import pytest

from tests import ovr_ref, ovr_steps
from tests.adp_steps import FIRST, LAST, P, cols_of

KS = [20, 28, 29, 50, 56]
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bamqc_amd", "csrc")


def both(cols, n_lanes, K=50, ppm=1000, capacity=1 << 26):
    v, w = ovr_ref.view(cols, n_lanes, K, ppm, capacity), ovr_ref.view_fast(cols, n_lanes, K, ppm, capacity)
    assert ovr_ref.same_view(v, w) is None, ovr_ref.same_view(v, w)
    for m in range(2):
        assert len(v["listed"][m]) <= 1_000_000 // ppm  # the derived bound the list's buffer is sized by
        assert sum(c for s, c, src in v["listed"][m]) <= int(v["lanes"][:, m].sum()) - int(v["lanes"][:, 2 + m].sum())
        assert int(v["hist"][m].sum()) == int(v["distinct"][m])
    return v


@pytest.mark.parametrize("K", [50, 56])
def test_rule_batch(K):
    cols, reads, marks = ovr_steps.rule_batch(K)
    v = both(cols, ovr_steps.RULE_LANES, K)
    assert 200 <= len(reads) <= 1000 and set(int(g) for g in cols["lane"]) == {0, 1, 2}
    sets, lanes, per_read = ovr_ref.count_sets(cols, ovr_steps.RULE_LANES, K)
    key = per_read[0]
    for name, m in marks.items():
        if isinstance(m, list):
            assert all(key[i] is None for i in m), name
        elif m[0] == "skipped":
            assert key[m[1]] == "skipped", name
        elif m[0] == "entered":
            assert isinstance(key[m[1]], tuple), name
        else:
            assert isinstance(key[m[0]], tuple) and isinstance(key[m[1]], tuple), name
            assert (1 if key[m[0]] == key[m[1]] else 2) == m[2], name
    assert sum(1 for m in marks.values() if m[0] == "skipped") == 12 * 2 * 2 and sum(1 for m in marks.values() if m[0] == "entered") == 12 * 2
    assert v["lanes"][:, 2:].sum() == 4 * 48 and (K != 56 or (1, "T" * 56) not in sets and (0, "T" * 56) in sets)


def test_restatement_of_the_rule_itself():
    """What cannot reach the card through the library: a primary read without a mate flag, a read group at or behind n_lanes."""
    S = "ACGTTGCATT" * 3
    cols, _ = cols_of([(S, P | FIRST), (S, P), (S, P | LAST), (S, P | FIRST), ("ACGN" + S, P | FIRST | 0x10), (S + "N", P | FIRST)], [0, 0, 0, 5, 1, 1])
    v = both(cols, 2, 20)
    assert v["lanes"].tolist() == [[1, 1, 0, 0], [2, 0, 0, 0]] and v["distinct"].tolist() == [2, 1]  # (the reverse read's N lies behind its 20 bases)
    assert ovr_ref.threshold(3000, 1000) == 3 and ovr_ref.threshold(3001, 1000) == 4 and ovr_ref.threshold(0, 10) == 2
    assert ovr_ref.threshold(1 << 40, 1_000_000) == 1 << 40
    assert ovr_ref.source("TT" + ovr_steps.UNI) == "Illumina_Universal" and ovr_ref.source("A" * 12 + "G" * 12) == "PolyA" and ovr_ref.source("ACGT" * 9) == "-"
    with pytest.raises(ovr_ref.Overflow):
        ovr_ref.view(ovr_steps.probe_batch(1, 17), 1, 50, 1000, 16)


@pytest.mark.parametrize("K", KS)
def test_layout_batch(K):
    cols, reads, starts = ovr_steps.layout_batch(K)
    v = both(cols, 1, K, 10)
    L = cols["l_seq"].astype(np.int64)
    assert all(starts[(n, rev)] == {0, 1, 2, 3} for n in ovr_steps.LAYOUT_LENGTHS for rev in (False, True))
    assert all((n, rev) in starts for n in ovr_steps.LONG_LENGTHS for rev in (False, True))
    assert L[-1] & 1 and cols["flag"][-1] & 0x10 and cols["seq"][-1] & 15 == 8  # the last read: reverse, odd, its pad nibble a T
    assert v["lanes"][:, 2:].sum() == 0 and int(v["threshold"].max()) == 2
    sets, _, _ = ovr_ref.count_sets(cols, 1, K)
    assert all(c == 2 for (m, s), c in sets.items() if len(s) >= 16)
    listed = {s for m in range(2) for s, c, src in v["listed"][m]}
    assert all(s in listed for (m, s), c in sets.items() if len(s) >= 16)  # ppm 10: every pair is listed, so the keys' letters are compared
    # a key that took the pad nibble or the next read's first base would differ: the twin of an odd read holds other bases there
    odd = [i for i in range(len(reads)) if len(reads[i][0]) & 1 and len(reads[i][0]) < K]
    assert len(odd) > 100


@pytest.mark.parametrize("shared", ["first", "second"])
def test_race_batch(shared):
    cols = ovr_steps.race_batch(shared)
    v = both(cols, 1, 56)
    assert v["distinct"].tolist() == [64, 0] and v["hist"][0, 63] == 64
    sets, _, _ = ovr_ref.count_sets(cols, 1, 56)
    assert len({s[:28] for m, s in sets}) == (1 if shared == "first" else 64) and len({s[28:] for m, s in sets}) == (64 if shared == "first" else 1)


def test_hot_and_probe_batches():
    v = both(ovr_steps.hot_batch(2000), 2)
    assert v["distinct"].tolist() == [1, 0] and v["largest"].tolist() == [2000, 0] and v["lanes"].tolist() == [[1000, 0, 0, 0]] * 2
    for seed in range(4):
        assert int(both(ovr_steps.probe_batch(seed), 1, capacity=16)["distinct"].sum()) == 16
    assert int(both(ovr_steps.probe_batch(1, 17), 1)["distinct"].sum()) == 17


def test_steps_batch():
    cols = ovr_steps.steps_batch(2)  # (a card of two CUs: the batch's size follows the CU count, its make-up does not)
    n = len(cols["flag"])
    assert n > 2 * ovr_steps.OV_STEP * 2 and -(-n // 2) > 2 * ovr_steps.OV_STEP  # either workgroup's share: three steps
    assert re.search(r"^#define OV_THREADS\s+1024\b", open(os.path.join(CSRC, "k_ovr.hip")).read(), re.M)
    v = both(cols, 3, 20)
    assert int(v["distinct"].sum()) > 1000 and (np.diff(cols["lane"].astype(int)) >= 0).all() and set(cols["lane"].tolist()) == {0, 1, 2}


def test_threshold_batches():
    for name, (reads, ppm, want) in ovr_steps.threshold_batches().items():
        v = both(ovr_steps.cols(reads), 1, 50, ppm)
        for m in range(2):
            assert [s for s, c, src in v["listed"][m]] == want[m], name
    t = ovr_steps.threshold_batches()
    v = both(ovr_steps.cols(t["T = 3 at 3000 reads"][0]), 1)
    assert v["threshold"][0] == 3 and v["hist"][0, 1] == 1 and v["hist"][0, 2] == 1   # a set of T - 1 exists and is not listed
    v = both(ovr_steps.cols(t["T = 4 at 3001 reads"][0]), 1)
    assert v["threshold"][0] == 4 and v["hist"][0, 2] == 1 and v["hist"][0, 3] == 1
    v = both(ovr_steps.cols(t["ten sets at ppm 10^5"][0]), 1, 50, 100_000)
    assert len(v["listed"][1]) == 10 == 1_000_000 // 100_000
    v = both(ovr_steps.cols(t["sources"][0]), 1)
    assert [src for s, c, src in v["listed"][0]] == ["Illumina_Universal", "PolyG", "-"]


def test_order_batch():
    cols = ovr_steps.order_batch()
    v = both(cols, ovr_steps.ORDER_LANES)
    assert v["lanes"][:, 2:].sum() > 50 and v["largest"].min() >= 100 and v["distinct"].min() > 50 and all(len(l) > 3 for l in v["listed"])
    assert len(cols["flag"]) - int(v["lanes"][:, :2].sum()) > 100  # reads that are not examined
