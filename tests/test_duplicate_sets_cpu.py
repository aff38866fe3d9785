"""CPU: the restatement of the duplicate sets (tests/dup_ref.py) — the loops against numpy — and the batches of the GPU tests
(tests/dup_steps.py): each crosses the edge it is named for.  Also the library-size estimate on cases worked out by hand."""
import math

import numpy as np
import pytest

from tests import dup_ref, dup_steps, synth


def both(cols, n_lanes, n_refs, capacity=1 << 26):
    a, b = dup_ref.view(cols, n_lanes, n_refs, capacity), dup_ref.view_fast(cols, n_lanes, n_refs, capacity)
    assert dup_ref.same_view(a, b) is None, dup_ref.same_view(a, b)
    return a


def test_rule_batch_holds_every_case():
    cols, reads, marks = dup_steps.rule_batch()
    assert 150 <= len(reads) <= 600
    sets, lanes, sig = dup_ref.count_sets(cols, dup_steps.RULE_LANES, dup_steps.RULE_REFS)
    for name, m in marks.items():
        if isinstance(m, list):
            assert all(sig[i] is None for i in m), name
        else:
            a, b, n = m
            assert sig[a] is not None and sig[b] is not None and (sig[a] == sig[b]) == (n == 1), (name, sig[a], sig[b])
    for name, field in (("strand", 1), ("mate strand", 2), ("class", 0), ("rid", 3), ("u5", 4), ("tlen", 5)):  # differing ONLY in the one field
        a, b, _ = marks[name]
        diff = [k for k in range(6) if sig[a][k] != sig[b][k]]
        assert diff == ([0, 5] if name == "class" else [field]), (name, sig[a], sig[b])  # (a single's tlen is 0 by the rule)
    a, b, _ = marks["lane only"]
    assert cols["lane"][a] != cols["lane"][b]
    for bit, i in zip((0x4, 0x100, 0x200, 0x800), marks["not examined"]):
        assert cols["flag"][i] & 0xB04 == bit
    assert all(cols["tlen"][i] < 0 for i in marks["second end"])
    assert sig[marks["negative u5"][0]][4] == -10 and sig[marks["far end"][0]][4] == dup_steps.POS_MAX + 3 + 3 * dup_steps.OPMAX > 1 << 31
    assert sig[marks["all clips forward"][1]][4] == 9995 and sig[marks["all clips reverse"][1]][4] == 9999
    v = both(cols, dup_steps.RULE_LANES, dup_steps.RULE_REFS)
    assert v["lanes"][:, 2:4].sum() > 0 and v["lanes"][:, 4].sum() == 12 and (v["lanes"][:, :2] > 0).all()
    assert v["sets"][0] > 3 and v["sets"][1] > 10


def test_clips_by_hand():
    S, H, M, D, I = dup_steps.S, dup_steps.H, dup_steps.M, dup_steps.D, dup_steps.I
    assert dup_ref.clips([(3, H), (2, S), (10, M), (1, I), (4, D), (5, M), (6, S)]) == (5, 6, 19)
    assert dup_ref.clips([(3, S), (4, H)]) == (7, 0, 0)
    assert dup_ref.clips([(10, M), (2, S), (5, M)]) == (0, 0, 15)
    assert dup_ref.clips([(2, S), (1, 6), (2, S)]) == (2, 2, 0)  # a pad is no clip
    assert dup_ref.u5_of([(2, S), (10, M), (3, S)], 100, False) == 98 and dup_ref.u5_of([(2, S), (10, M), (3, S)], 100, True) == 112


@pytest.mark.parametrize("shared", ["k0", "k1"])
def test_race_batches_share_one_word(shared):
    cols = dup_steps.race_batch(shared)
    cls, k0, k1 = dup_ref.keys_fast(cols, 1, dup_steps.RACE_REFS)
    assert len(k0) == 4096 and (cls == dup_ref.PAIR).all()
    same, other = (k0, k1) if shared == "k0" else (k1, k0)
    assert len(np.unique(same)) == 1 and len(np.unique(other)) == 64
    assert all(len(np.unique(other[i:i + 64])) == 64 for i in range(0, 4096, 64))  # interleaved: every wave holds all 64
    v = both(cols, 1, dup_steps.RACE_REFS)
    assert v["sets"].tolist() == [0, 64] and v["hist"][1, 63] == 64 and v["largest"][1] == 64


def test_hot_batch():
    v = both(dup_steps.hot_batch(), 2, 1)
    assert v["sets"].tolist() == [0, 1] and v["largest"].tolist() == [0, 20_000] and v["hist"][1, 255] == 1 and v["hist"].sum() == 1
    assert v["lanes"][:, 1].tolist() == [10_000, 10_000]


def test_probe_batches_fill_the_capacity_exactly():
    assert dup_ref.slots(16) == 32 and dup_ref.slots(17) == 64 and dup_ref.slots(1 << 26) == 1 << 27 and dup_ref.slots(1 << 31) == 1 << 32
    for seed in range(dup_steps.PROBE_ROUNDS):
        v = both(dup_steps.probe_batch(seed), 1, 2, 16)
        assert v["sets"].sum() == 16 and v["sets"].min() > 0
    with pytest.raises(dup_ref.Overflow):
        dup_ref.view(dup_steps.probe_batch(1, 17), 1, 2, 16)
    with pytest.raises(dup_ref.Overflow):
        dup_ref.view_fast(dup_steps.probe_batch(1, 17), 1, 2, 16)


def test_path_batch_crosses_the_paths():
    reads, twins = dup_steps.path_batch()
    assert sorted({len(r["cigar"]) for r in reads}) == sorted(set(dup_steps.PATH_NCIGARS + [dup_steps.DP_T + 4]))
    assert dup_steps.DP_T in dup_steps.PATH_NCIGARS and dup_steps.DP_T + 1 in dup_steps.PATH_NCIGARS and dup_steps.PASS + 1 in dup_steps.PATH_NCIGARS
    for r in reads:
        if len(r["cigar"]) > 1 and len(r["cigar"]) in dup_steps.PATH_NCIGARS:
            lead, trail, reflen = dup_ref.clips(r["cigar"])
            assert lead > 0 and trail > 0 and reflen > 0
            inner = r["cigar"][2:-3]
            assert len(r["cigar"]) < 12 or any(op == dup_steps.S for _, op in inner)  # clips inside that belong to neither end
    cols = dup_steps.cols_with_tlen(reads + twins, 1)
    v = both(cols, 1, 2)
    assert v["sets"].tolist() == [len(reads), 0] and v["hist"][0, 1] == len(reads)
    assert all(len(t["cigar"]) == 1 for t in twins)


def test_order_batch_and_pieces():
    cols = dup_steps.order_batch()
    v = both(cols, dup_steps.ORDER_LANES, dup_steps.ORDER_REFS)
    assert v["sets"].min() >= 30 and v["largest"].min() > 8 and v["lanes"][:, 4].min() > 0 and v["lanes"][:, 2:4].min() > 0
    assert 0 < v["estimated_library_size"]
    n = len(cols["flag"])
    perm = np.random.default_rng(9).permutation(n)
    shuffled = synth.concat([synth.slice_batch(cols, int(i), int(i) + 1) for i in perm])
    assert dup_ref.same_view(dup_ref.view_fast(shuffled, dup_steps.ORDER_LANES, dup_steps.ORDER_REFS), v) is None
    t = dup_ref.text(v, "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    lines = t.split("\n")
    assert lines[0] == "sample_id S" and lines[1] == "duplicate_sets_capacity 67108864" and lines[2] == "lane g2" and lines.count("all_lanes") == 1
    assert lines[3] == "duplicate_reads_examined_single %d" % v["lanes"][2, 0] and len(lines[-4].split()) == 257 and t.endswith("\n")


def test_estimate_by_hand():
    assert dup_ref.estimate(1000, 1000) == 0 and dup_ref.estimate(1000, 1001) == 0  # c >= n
    assert dup_ref.estimate(1000, 0) == 0 and dup_ref.estimate(0, 0) == 0
    # n = 1000 read pairs, c = 800 unique: the closed form c / x - 1 + exp(-n / x) changes sign at the estimate
    n, c = 1000, 800
    L = dup_ref.estimate(n, c)
    f = lambda x: c / x - 1 + math.exp(-n / x)
    assert f(L - 1) > 0 > f(L + 2) and 2000 < L < 2300  # (x = 2 n: 0.4 - 1 + e^-0.5 = 0.0065 > 0; x = 2.3 n: 0.348 - 1 + 0.647 < 0)
    # one duplicate among a million pairs: x (1 - e^(-n / x)) = n - 1 gives x close to n^2 / 2
    L = dup_ref.estimate(10**6, 10**6 - 1)
    assert abs(L / (10**12 / 2) - 1) < 1e-3
