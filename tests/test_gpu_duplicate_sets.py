"""GPU: duplicate sets by alignment signature (bqc_enable_duplicate_sets, --duplicate-sets; bamqc_amd/csrc/k_dup.hip) against the
restatement of the rule (tests/dup_ref.py), through the C ABI: the whole view — the sets by class and size, the largest sets, the
estimate and every read group's sums — and the `.dup` text.

k_dup computes every examined read's signature (a thread for a CIGAR of at most 8 operations, a wave beyond) and counts it in a hash
table in device memory whose insert is two compare-and-swaps and an add; k_dup_final scans the table.  The batches (tests/dup_steps.py;
tests/test_duplicate_sets_cpu.py asserts that they cross the edges they are named for) put no read on a main chromosome and load no
contig: the genome is not read."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, _abi, hostio
from tests import dup_ref, dup_steps, pybam, synth
from tests.dup_steps import cols_with_tlen
from tests.parity import split

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
ERR_ARG, ERR_RANGE, ERR_STATE = 1, 6, 8
CAP = 1 << 12


def context(n_lanes, n_refs, capacity=CAP, **more):
    """No contig is main and none is given: the genome is not read."""
    return Aggregator(n_lanes=n_lanes, duplicate_sets=capacity, **dict(dict(n_refs=n_refs, main_chrom=[0] * n_refs, max_read_len=16_384, isize=2000), **more))


def check_view(a, want):
    got = a.duplicate_sets()
    bad = dup_ref.same_view(got, want)
    assert bad is None, (bad, got[bad], want[bad])


def run_and_check(batches, n_lanes, n_refs, want, capacity=CAP):
    a = context(n_lanes, n_refs, capacity)
    for b in batches:
        a.submit(b)
    a.finalize()
    check_view(a, want)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule
# ---------------------------------------------------------------------------------------------------------------------------
def test_rule():
    cols, reads, marks = dup_steps.rule_batch()
    want = dup_ref.view(cols, dup_steps.RULE_LANES, dup_steps.RULE_REFS, CAP)  # (the loops: this batch is small)
    run_and_check([cols], dup_steps.RULE_LANES, dup_steps.RULE_REFS, want)
    # every marked pair alone (one context, emptied in between): one set of two reads, or two sets
    a = context(dup_steps.RULE_LANES, dup_steps.RULE_REFS)
    for name, m in marks.items():
        if isinstance(m, list):
            continue
        two = cols_with_tlen([reads[m[0]], reads[m[1]]])
        w = dup_ref.view(two, dup_steps.RULE_LANES, dup_steps.RULE_REFS, CAP)
        assert int(w["sets"].sum()) == m[2], name
        a.reset()
        a.submit(two)
        a.finalize()
        bad = dup_ref.same_view(a.duplicate_sets(), w)
        assert bad is None, (name, bad)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the two-word race
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", ["k0", "k1"])
def test_two_word_race(shared):
    cols = dup_steps.race_batch(shared)
    want = dup_ref.view_fast(cols, 1, dup_steps.RACE_REFS, CAP)
    assert want["sets"].tolist() == [0, 64] and want["hist"][1, 63] == 64
    run_and_check([cols], 1, dup_steps.RACE_REFS, want)
    n = len(cols["flag"])
    run_and_check(split(cols, list(range(1, n))), 1, dup_steps.RACE_REFS, want)  # 4096 batches of one read


# ---------------------------------------------------------------------------------------------------------------------------
# 3. contention
# ---------------------------------------------------------------------------------------------------------------------------
def test_20000_reads_of_one_signature():
    cols = dup_steps.hot_batch(20_000)
    a = context(2, 1)
    a.submit(cols)
    a.finalize()
    v = a.duplicate_sets()
    assert v["sets"].tolist() == [0, 1] and v["largest"].tolist() == [0, 20_000]
    assert v["hist"][1, 255] == 1 and v["hist"].sum() == 1
    assert v["lanes"].tolist() == [[0, 10_000, 0, 0, 0]] * 2
    check_view(a, dup_ref.view_fast(cols, 2, 1, CAP))
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. probing and the limits
# ---------------------------------------------------------------------------------------------------------------------------
def test_full_capacity_of_the_smallest_table():
    """Capacity 16, 32 slots, exactly 16 signatures, dup_steps.PROBE_ROUNDS times over (reset in between): every signature is found with
    its count whatever run of taken slots its probe sequence has to cross, the table's end included."""
    a = context(1, 2, 16)
    for seed in range(dup_steps.PROBE_ROUNDS):
        cols = dup_steps.probe_batch(seed)
        a.submit(cols)
        a.finalize()
        check_view(a, dup_ref.view(cols, 1, 2, 16))
        a.reset()
    a.close()


def test_one_signature_too_many():
    cols = dup_steps.probe_batch(1, 17)
    a = context(1, 2, 16)
    with pytest.raises(BamQCError) as e:
        a.submit(cols)
        a.finalize()
    assert e.value.code == ERR_RANGE and "16" in str(e.value) and "capacity" in str(e.value), str(e.value)
    with pytest.raises(BamQCError) as e:  # the context is poisoned like after other stream errors
        a.submit(cols)
    assert e.value.code == ERR_STATE
    a.reset()  # ... and a reset empties the table: 16 signatures fit again
    cols = dup_steps.probe_batch(2)
    a.submit(cols)
    a.finalize()
    check_view(a, dup_ref.view(cols, 1, 2, 16))
    a.close()


def test_far_too_many_signatures():
    """Thousands of different signatures into 32 slots: every probe sequence gives up, nothing hangs."""
    reads = [dict(flag=dup_steps.P | dup_steps.FIRST, pos=10 * i, tlen=200, cigar=[(20, dup_steps.M)]) for i in range(5000)]
    a = context(1, 1, 16)
    with pytest.raises(BamQCError) as e:
        a.submit(cols_with_tlen(reads))
        a.finalize()
    assert e.value.code == ERR_RANGE
    a.close()


@pytest.mark.parametrize("capacity", [0, 15, (1 << 31) + 1])
def test_capacity_out_of_range(capacity):
    with pytest.raises(BamQCError) as e:
        context(1, 1, capacity)
    assert e.value.code == ERR_ARG and str(capacity) in str(e.value), str(e.value)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. CIGAR lengths: thread path against wave path
# ---------------------------------------------------------------------------------------------------------------------------
def test_paths_mixed_in_one_step():
    reads, twins = dup_steps.path_batch()
    mixed = [r for pair in zip(reads, twins) for r in pair]
    cols = cols_with_tlen(mixed, 1)
    want = dup_ref.view_fast(cols, 1, 2, CAP)
    assert want["sets"].tolist() == [len(reads), 0] and want["hist"][0, 1] == len(reads)  # every read shares a set with its twin
    run_and_check([cols], 1, 2, want)


def test_paths_each_read_alone():
    reads, twins = dup_steps.path_batch()
    a = context(1, 2)
    for k in range(len(reads)):  # a read, then its twin, each in a batch of its own
        a.submit(cols_with_tlen([reads[k]], 100 + k))
        a.submit(cols_with_tlen([twins[k]], 200 + k))
    a.finalize()
    check_view(a, dup_ref.view_fast(cols_with_tlen(reads + twins, 1), 1, 2, CAP))
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. order independence
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def order():
    cols = dup_steps.order_batch()
    return cols, dup_ref.view_fast(cols, dup_steps.ORDER_LANES, dup_steps.ORDER_REFS, CAP)


def test_one_batch_against_seven_shuffled(order, tmp_path):
    cols, want = order
    run_and_check([cols], dup_steps.ORDER_LANES, dup_steps.ORDER_REFS, want)
    n = len(cols["flag"])
    perm = np.random.default_rng(9).permutation(n)
    shuffled = synth.concat([synth.slice_batch(cols, int(i), int(i) + 1) for i in perm])
    a = context(dup_steps.ORDER_LANES, dup_steps.ORDER_REFS)
    for part in split(shuffled, [1, 3, 6, 906, 1807, 1808]):  # seven pieces
        a.submit(part)
    a.finalize()
    check_view(a, want)
    out = str(tmp_path / "order.dup")  # the text through the library's writer, lanes in an order of the caller's
    a.write_duplicate_sets(out, "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    assert open(out).read() == dup_ref.text(want, "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. life cycle
# ---------------------------------------------------------------------------------------------------------------------------
def test_finalize_twice_and_reset(order):
    cols, want = order
    a = context(dup_steps.ORDER_LANES, dup_steps.ORDER_REFS)
    a.submit(cols)
    a.finalize()
    check_view(a, want)
    a.finalize()  # twice: the table is left as it is
    check_view(a, want)
    a.reset()
    with pytest.raises(BamQCError) as e:  # (nothing finalised since the reset)
        a._chk(a.lib.bqc_duplicate_sets(a.h, C.byref(_abi.DupView())))
    assert e.value.code == ERR_STATE
    a.submit(cols)
    a.finalize()
    check_view(a, want)  # the same, not doubled
    a.close()


def test_state_vector_is_untouched(order):
    cols, want = order
    base = dict(n_lanes=dup_steps.ORDER_LANES, n_refs=dup_steps.ORDER_REFS, main_chrom=[0] * dup_steps.ORDER_REFS, max_read_len=16_384, isize=2000)
    off, on = Aggregator(**base), Aggregator(duplicate_sets=CAP, **base)
    assert on.state_words == off.state_words
    off.submit(cols)
    on.submit(cols)
    assert np.array_equal(off.state_export_host(), on.state_export_host())
    both = Aggregator(duplicate_sets=CAP, indel_by_cycle=16, qual_by_cycle=8, **base)
    only = Aggregator(indel_by_cycle=16, qual_by_cycle=8, **base)
    assert both.state_words == only.state_words
    for x in (off, on, both, only):
        x.close()


def test_enable_errors(order):
    cols, want = order
    base = dict(n_lanes=dup_steps.ORDER_LANES, n_refs=dup_steps.ORDER_REFS, main_chrom=[0] * dup_steps.ORDER_REFS, max_read_len=16_384, isize=2000)
    a = Aggregator(duplicate_sets=16, **base)  # (the lower limit is a value)
    with pytest.raises(BamQCError) as e:
        a.enable_duplicate_sets(64)
    assert e.value.code == ERR_STATE
    a.close()
    for spoil in ("submit", "export", "finalize"):
        a = Aggregator(**base)
        a.submit(cols) if spoil == "submit" else a.state_export_host() if spoil == "export" else a.finalize()
        with pytest.raises(BamQCError) as e:
            a.enable_duplicate_sets(64)
        assert e.value.code == ERR_STATE, spoil
        if spoil == "finalize":
            with pytest.raises(BamQCError) as e:  # (the module is off)
                a.duplicate_sets()
            assert e.value.code == ERR_STATE
        a.close()
    a = Aggregator(duplicate_sets=CAP, **base)
    a.submit(cols)
    with pytest.raises(BamQCError) as e:  # (before finalize: the call itself, Aggregator.duplicate_sets would finalise first)
        a._chk(a.lib.bqc_duplicate_sets(a.h, C.byref(_abi.DupView())))
    assert e.value.code == ERR_STATE
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the program
# ---------------------------------------------------------------------------------------------------------------------------
CHROMS = ["-c", "chr1,chr2"]
NAMES, LENS = ["chr1", "chr2"], [400_000, 150_000]


def run(args, env=None, **kw):
    return subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, **(env or {})), timeout=120, **kw)


def same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """4000 synthetic paired reads in two read groups (the file of the `.rcv` tests), the same file with 300 of its records written a
    second and 40 of those a third time, the `.bamqc` of runs without the option, and the text the restatement makes of each file."""
    d = tmp_path_factory.mktemp("dup")
    plain, fa, dupd = str(d / "plain.bam"), str(d / "in.fa"), str(d / "dupd.bam")
    hostio.synth_write(plain, fa, seed=31, n_reads=4000, ref_names=NAMES, ref_lens=LENS, n_lanes=2)
    cols, refs, lanes, sample = pybam.columns(plain)
    assert len(lanes) == 2 and [nm for nm, _ in refs] == NAMES
    pick = np.random.default_rng(35).choice(len(cols["flag"]), 300, replace=False)
    order = np.sort(np.concatenate([np.arange(len(cols["flag"])), pick, pick[:40]]))  # (a copy directly behind its original: the file stays sorted)
    cuts = [0] + [int(k) for k in np.nonzero(np.diff(order) != 1)[0] + 1] + [len(order)]
    more = synth.concat([synth.slice_batch(cols, int(order[lo]), int(order[hi - 1]) + 1) for lo, hi in zip(cuts[:-1], cuts[1:])])
    assert len(more["flag"]) == len(cols["flag"]) + 340
    hostio.write_bam(dupd, more, NAMES, LENS, n_lanes=2)
    names = sorted(lanes)  # the `.bamqc` lists the lanes by name
    idx = [lanes[nm] for nm in names]
    out = dict(dir=d, fa=fa, plain=plain, dupd=dupd)
    for name, path in (("plain", plain), ("dupd", dupd)):
        out["base_" + name] = str(d / ("base_%s.bamqc" % name))
        r = run(["-r", fa, "-o", out["base_" + name]] + CHROMS + [path])
        assert r.returncode == 0, r.stderr
        assert not os.path.exists(out["base_" + name] + ".dup")
        c = pybam.columns(path)[0]
        v = dup_ref.view_fast(c, 2, 2, 1 << 26)
        out["view_" + name] = v
        out["want_" + name] = lambda capacity=1 << 26, v=v: dup_ref.text(dict(v, capacity=capacity), sample, names, idx)
    vp, vd = out["view_plain"], out["view_dupd"]
    assert int(vd["lanes"][:, :2].sum()) - int(vd["sets"].sum()) >= int(vp["lanes"][:, :2].sum()) - int(vp["sets"].sum()) + 100  # the written duplicates are seen (about half of the copies are second ends)
    return out


@pytest.mark.parametrize("decode", ["0", "1"])
def test_program_bam(files, decode):
    out = str(files["dir"] / ("bam%s.bamqc" % decode))
    r = run(["-r", files["fa"], "-o", out, "--duplicate-sets", "--duplicate-sets-capacity", "100000"] + CHROMS + [files["dupd"]], env=dict(BQC_GPU_DECODE=decode))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base_dupd"])
    assert open(out + ".dup").read() == files["want_dupd"](100000)
    assert not os.path.exists(out + ".rcv") and not os.path.exists(out + ".ibc")


def test_program_sam_on_stdin_default_capacity(files):
    out = str(files["dir"] / "sam.bamqc")
    sam = pybam.bam_to_sam_text(files["dupd"]).encode()
    r = run(["-r", files["fa"], "-o", out, "--duplicate-sets"] + CHROMS + ["-"], input=sam)
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base_dupd"])
    assert open(out + ".dup").read() == files["want_dupd"]()


def test_program_manifest_resets_per_job(files):
    d = files["dir"]
    jobs = [(files["dupd"], str(d / "m1.bamqc"), "dupd"), (files["plain"], str(d / "m2.bamqc"), "plain"), (files["dupd"], str(d / "m3.bamqc"), "dupd")]
    lst = str(d / "jobs.tsv")
    with open(lst, "w") as f:
        for i, o, _ in jobs:
            f.write("%s\t%s\n" % (i, o))
    r = run(["-r", files["fa"], "--duplicate-sets", "--duplicate-sets-capacity", "65536", "--manifest", lst] + CHROMS)
    assert r.returncode == 0, r.stderr
    for i, o, which in jobs:
        assert same_bytes(o, files["base_" + which])
        assert open(o + ".dup").read() == files["want_" + which](65536)
    assert files["want_dupd"]() != files["want_plain"]()


def test_program_all_nine_modules(files):
    d = files["dir"]
    eight, nine = str(d / "eight.bamqc"), str(d / "nine.bamqc")
    sites, bed = str(d / "sites.tsv"), str(d / "panel.bed")
    with open(sites, "w") as f:
        f.write("".join("chr1\t%d\n" % p for p in range(1000, 3000, 7)))
    with open(bed, "w") as f:
        f.write("".join("chr1\t%d\t%d\n" % (p, p + 300) for p in range(2000, 390_000, 5000)))
    mods = ["--qual-by-cycle", "--mismatch-by-cycle", "--adapter-by-cycle", "--gc-bias", "--indel-by-cycle", "--substitutions", "--site-alleles", sites, "--regions", bed]
    r = run(["-r", files["fa"], "-o", eight] + mods + CHROMS + [files["dupd"]])
    assert r.returncode == 0, r.stderr
    r = run(["-r", files["fa"], "-o", nine] + mods + ["--duplicate-sets", "--duplicate-sets-capacity", "4096"] + CHROMS + [files["dupd"]])
    assert r.returncode == 0, r.stderr
    for ext in ("", ".qbc", ".mbc", ".adp", ".gcb", ".ibc", ".sbc", ".sac", ".rcv"):
        assert same_bytes(nine + ext, eight + ext), ext
    assert same_bytes(nine, files["base_dupd"])
    assert open(nine + ".dup").read() == files["want_dupd"](4096)


def test_program_messages(files):
    d = files["dir"]
    never = str(d / "never.bamqc")
    r = run(["--gpus", "2", "-r", files["fa"], "-o", never, "--duplicate-sets"] + CHROMS + [files["dupd"]], env=dict(BQC_GPUS_SHARE_DEVICE="1"))
    assert r.returncode != 0 and b"--duplicate-sets with --gpus is not supported" in r.stderr, r.stderr
    r = run(["-r", files["fa"], "-o", never, "--duplicate-sets-capacity", "4096"] + CHROMS + [files["dupd"]])
    assert r.returncode != 0 and b"needs --duplicate-sets" in r.stderr and b"--duplicate-sets-capacity" in r.stderr, r.stderr
    for bad in ("15", "2147483649", "x"):
        r = run(["-r", files["fa"], "-o", never, "--duplicate-sets", "--duplicate-sets-capacity", bad] + CHROMS + [files["dupd"]])
        assert r.returncode != 0 and b"16 to 2147483648" in r.stderr, r.stderr
    assert not os.path.exists(never) and not os.path.exists(never + ".dup")
    small = str(d / "small.bamqc")
    r = run(["-r", files["fa"], "-o", small, "--duplicate-sets", "--duplicate-sets-capacity", "16"] + CHROMS + [files["dupd"]])
    assert r.returncode == 1, r.stderr
    assert b"16" in r.stderr and b"--duplicate-sets-capacity" in r.stderr and not os.path.exists(small + ".dup"), r.stderr
    blocked = str(d / "blocked.bamqc")
    os.mkdir(blocked + ".dup")  # (a directory where the table's file would go)
    r = run(["-r", files["fa"], "-o", blocked, "--duplicate-sets", "--duplicate-sets-capacity", "100000"] + CHROMS + [files["dupd"]])
    assert r.returncode == 1
    assert b"Could not write output file" in r.stderr and b".dup" in r.stderr
