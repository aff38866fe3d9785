"""GPU: overrepresented sequences (bqc_enable_overrepresented, --overrepresented; bamqc_amd/csrc/k_ovr.hip) against the restatement of
the rule (tests/ovr_ref.py), through the C ABI: the whole view — every read group's sums, per mate the sets by size, the largest set,
the threshold and the list with its letters and sources — and the `.ovr` text.

k_ovr takes a read's first n bases as sequenced from the 4-bit payload (a thread a read: the aligned dwords that hold them, shifted,
packed to 2 bits a base, a reverse read's turned and complemented) and counts the key in a hash table in device memory whose insert
is two compare-and-swaps and an add; k_ovr_final scans the table.  The batches (tests/ovr_steps.py; tests/test_overrepresented_cpu.py
asserts that they cross the edges they are named for) put no read on a main chromosome and load no contig: the genome is not read.

Not here: a primary read without a mate flag and a read group at or behind n_lanes.  The core statistics refuse such a batch as a
whole, so these rules cannot be reached through the library; the restatement's side of them is in the CPU test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bamqc_amd import Aggregator, BamQCError, _abi, hostio
from tests import ovr_ref, ovr_steps, pybam, synth
from tests.parity import split

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
ERR_ARG, ERR_RANGE, ERR_STATE = 1, 6, 8
CAP = 1 << 13
BASE = dict(n_refs=1, main_chrom=[0], max_read_len=1 << 17, isize=2000)


def context(n_lanes, K=50, ppm=1000, capacity=CAP, **more):
    """No contig is main and none is given: the genome is not read."""
    return Aggregator(n_lanes=n_lanes, overrepresented=(K, capacity), overrepresented_ppm=ppm, **dict(BASE, **more))


def check_view(a, want, what=""):
    got = a.overrepresented()
    bad = ovr_ref.same_view(got, want)
    assert bad is None, (what, bad, got[bad], want[bad])


def run_and_check(batches, n_lanes, want, **kw):
    a = context(n_lanes, want["K"], want["ppm"], want["capacity"], **kw)
    for b in batches:
        a.submit(b)
    a.finalize()
    check_view(a, want)
    a.close()


def singles(cols):
    n = len(cols["flag"])
    return split(cols, list(range(1, n)))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the rule
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [50, 56])
def test_rule(K):
    cols, reads, marks = ovr_steps.rule_batch(K)
    want = ovr_ref.view(cols, ovr_steps.RULE_LANES, K, 1000, CAP)  # (the loops: this batch is small)
    run_and_check([cols], ovr_steps.RULE_LANES, want)
    # every marked pair alone (one context, emptied in between): one set of two reads, or two sets; a marked read alone: skipped or entered
    a = context(ovr_steps.RULE_LANES, K)
    for name, m in marks.items():
        if isinstance(m, list):
            continue
        some = ovr_steps.cols([reads[i] for i in m if not isinstance(i, str)][:2])
        w = ovr_ref.view(some, ovr_steps.RULE_LANES, K, 1000, CAP)
        if isinstance(m[0], str):
            assert int(w["lanes"][:, 2:].sum()) == (1 if m[0] == "skipped" else 0) and int(w["distinct"].sum()) == (0 if m[0] == "skipped" else 1), name
        else:
            assert int(w["distinct"].sum()) == m[2], name
        a.reset()
        a.submit(some)
        a.finalize()
        check_view(a, w, name)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the layout
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [20, 28, 29, 50, 56])
def test_layout(K):
    """Every length on both strands at every alignment of its first byte, pad nibbles that hold a base, long reads, the batch's last
    read reverse and odd — in one batch, and every read alone in a batch (there its bytes start the payload and nothing follows them).
    ppm 10: every set of two is listed, so the keys' letters are compared, not only their number."""
    cols, reads, starts = ovr_steps.layout_batch(K)
    want = ovr_ref.view_fast(cols, 1, K, 10, CAP)
    assert sum(len(l) for l in want["listed"]) > 1000
    run_and_check([cols], 1, want)
    run_and_check(singles(cols), 1, want)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the two-word race
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", ["first", "second"])
def test_two_word_race(shared):
    cols = ovr_steps.race_batch(shared)
    want = ovr_ref.view_fast(cols, 1, 56, 1000, CAP)
    assert want["distinct"].tolist() == [64, 0] and want["hist"][0, 63] == 64 and len(want["listed"][0]) == 64
    run_and_check([cols], 1, want)
    run_and_check(singles(cols), 1, want)  # 4096 batches of one read


# ---------------------------------------------------------------------------------------------------------------------------
# 4. contention
# ---------------------------------------------------------------------------------------------------------------------------
def test_20000_reads_of_one_sequence():
    cols = ovr_steps.hot_batch(20_000)
    a = context(2)
    a.submit(cols)
    a.finalize()
    v = a.overrepresented()
    assert v["distinct"].tolist() == [1, 0] and v["largest"].tolist() == [20_000, 0]
    assert v["hist"][0, 255] == 1 and v["hist"].sum() == 1
    assert v["lanes"].tolist() == [[10_000, 0, 0, 0]] * 2
    assert [c for s, c, src in v["listed"][0]] == [20_000] and v["listed"][1] == []
    check_view(a, ovr_ref.view_fast(cols, 2, 50, 1000, CAP))
    a.close()


def test_three_steps_per_workgroup():
    """More than 2 x 1024 reads for every workgroup the card can have: columns loaded ahead of the step, and the new-set counters' turn."""
    from tests.test_gpu_value_limits import n_cu
    cols = ovr_steps.steps_batch(n_cu())
    want = ovr_ref.view_fast(cols, 3, 20, 1000, 1 << 18)
    assert int(want["distinct"].sum()) > 30_000 and want["largest"].min() > 10
    run_and_check([cols], 3, want)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. capacity and the limits
# ---------------------------------------------------------------------------------------------------------------------------
def test_full_capacity_of_the_smallest_table():
    """Capacity 16, 32 slots, exactly 16 keys, ovr_steps.PROBE_ROUNDS times over (reset in between): every key is found with its count
    whatever run of taken slots its probe sequence has to cross, the table's end included."""
    a = context(1, capacity=16)
    for seed in range(ovr_steps.PROBE_ROUNDS):
        cols = ovr_steps.probe_batch(seed)
        a.submit(cols)
        a.finalize()
        check_view(a, ovr_ref.view(cols, 1, 50, 1000, 16), seed)
        a.reset()
    a.close()


def test_one_key_too_many():
    cols = ovr_steps.probe_batch(1, 17)
    a = context(1, capacity=16)
    with pytest.raises(BamQCError) as e:
        a.submit(cols)
        a.finalize()
    assert e.value.code == ERR_RANGE and "16" in str(e.value) and "capacity" in str(e.value) and "--overrepresented-capacity" in str(e.value), str(e.value)
    with pytest.raises(BamQCError) as e:  # the context is poisoned like after other stream errors
        a.submit(cols)
    assert e.value.code == ERR_STATE
    a.reset()  # ... and a reset empties the table: 16 keys fit again
    cols = ovr_steps.probe_batch(2)
    a.submit(cols)
    a.finalize()
    check_view(a, ovr_ref.view(cols, 1, 50, 1000, 16))
    a.close()


def test_far_too_many_keys():
    """5000 different keys into 32 slots: every probe sequence gives up, nothing hangs."""
    a = context(1, capacity=16)
    with pytest.raises(BamQCError) as e:
        a.submit(ovr_steps.many_keys(5000))
        a.finalize()
    assert e.value.code == ERR_RANGE
    a.close()


@pytest.mark.parametrize("K,ppm,capacity,named", [(50, 1000, 0, "0"), (50, 1000, 15, "15"), (50, 1000, (1 << 31) + 1, str((1 << 31) + 1)), (19, 1000, CAP, "19"),
                                                 (57, 1000, CAP, "57"), (50, 9, CAP, "9"), (50, 1_000_001, CAP, "1000001")])
def test_values_out_of_range(K, ppm, capacity, named):
    with pytest.raises(BamQCError) as e:
        context(1, K, ppm, capacity)
    assert e.value.code == ERR_ARG and named in str(e.value), str(e.value)


def test_limits_are_values():
    for K, ppm, capacity in ((20, 10, 16), (56, 1_000_000, 16)):
        a = context(1, K, ppm, capacity)
        a.submit(ovr_steps.probe_batch(3))
        a.finalize()
        check_view(a, ovr_ref.view(ovr_steps.probe_batch(3), 1, K, ppm, capacity))
        a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. threshold and list
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ovr_steps.threshold_batches()))
def test_threshold_and_list(name):
    reads, ppm, listed = ovr_steps.threshold_batches()[name]
    cols = ovr_steps.cols(reads)
    want = ovr_ref.view(cols, 1, 50, ppm, CAP)
    assert [[s for s, c, src in want["listed"][m]] for m in range(2)] == [listed[0], listed[1]]
    run_and_check([cols], 1, want)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. order and life cycle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def order():
    cols = ovr_steps.order_batch()
    return cols, ovr_ref.view_fast(cols, ovr_steps.ORDER_LANES, 50, 1000, CAP)


def test_one_batch_against_seven_shuffled(order, tmp_path):
    cols, want = order
    run_and_check([cols], ovr_steps.ORDER_LANES, want)
    n = len(cols["flag"])
    perm = np.random.default_rng(9).permutation(n)
    shuffled = synth.concat([synth.slice_batch(cols, int(i), int(i) + 1) for i in perm])
    a = context(ovr_steps.ORDER_LANES)
    for part in split(shuffled, [1, 3, 6, 906, 1807, 1808]):  # seven pieces
        a.submit(part)
    a.finalize()
    check_view(a, want)
    out = str(tmp_path / "order.ovr")  # the text through the library's writer, lanes in an order of the caller's
    a.write_overrepresented(out, "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    assert open(out).read() == ovr_ref.text(want, "S", ["g2", "g0", "g3", "g1"], [2, 0, 3, 1])
    a.close()


def test_finalize_twice_and_reset(order):
    cols, want = order
    a = context(ovr_steps.ORDER_LANES)
    a.submit(cols)
    a.finalize()
    check_view(a, want)
    a.finalize()  # twice: the table is left as it is
    check_view(a, want)
    a.reset()
    with pytest.raises(BamQCError) as e:  # (nothing finalised since the reset)
        a._chk(a.lib.bqc_overrepresented(a.h, C.byref(_abi.OvrView())))
    assert e.value.code == ERR_STATE
    a.submit(cols)
    a.finalize()
    check_view(a, want)  # the same, not doubled
    a.close()


def test_state_vector_is_untouched(order):
    cols, want = order
    base = dict(BASE, n_lanes=ovr_steps.ORDER_LANES)
    off, on = Aggregator(**base), Aggregator(overrepresented=(50, CAP), **base)
    assert on.state_words == off.state_words
    off.submit(cols)
    on.submit(cols)
    assert np.array_equal(off.state_export_host(), on.state_export_host())
    both = Aggregator(overrepresented=(50, CAP), indel_by_cycle=16, qual_by_cycle=8, duplicate_sets=64, **base)
    only = Aggregator(indel_by_cycle=16, qual_by_cycle=8, **base)
    assert both.state_words == only.state_words
    for x in (off, on, both, only):
        x.close()


def test_enable_errors(order):
    cols, want = order
    base = dict(BASE, n_lanes=ovr_steps.ORDER_LANES)
    a = Aggregator(overrepresented=(20, 16), **base)
    with pytest.raises(BamQCError) as e:  # a second call
        a.enable_overrepresented(50, 1000, 64)
    assert e.value.code == ERR_STATE
    a.close()
    for spoil in ("submit", "export", "finalize"):
        a = Aggregator(**base)
        a.submit(cols) if spoil == "submit" else a.state_export_host() if spoil == "export" else a.finalize()
        with pytest.raises(BamQCError) as e:
            a.enable_overrepresented(50, 1000, 64)
        assert e.value.code == ERR_STATE, spoil
        if spoil == "finalize":
            with pytest.raises(BamQCError) as e:  # (the module is off)
                a.overrepresented()
            assert e.value.code == ERR_STATE
        a.close()
    a = context(ovr_steps.ORDER_LANES)
    a.submit(cols)
    with pytest.raises(BamQCError) as e:  # (before finalize: the call itself, Aggregator.overrepresented would finalise first)
        a._chk(a.lib.bqc_overrepresented(a.h, C.byref(_abi.OvrView())))
    assert e.value.code == ERR_STATE
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. 256 read groups
# ---------------------------------------------------------------------------------------------------------------------------
def test_256_read_groups(tmp_path):
    cols = ovr_steps.order_batch(seed=12, n=4000, n_lanes=256)
    want = ovr_ref.view_fast(cols, 256, 50, 1000, CAP)
    assert (want["lanes"][:, :2].sum(axis=1) > 0).all() and want["lanes"][:, 2:].sum() > 50
    a = context(256)
    for part in split(cols, [1500]):
        a.submit(part)
    a.finalize()
    check_view(a, want)
    idx = [int(i) for i in np.random.default_rng(3).permutation(256)]
    names = ["rg%03d" % i for i in idx]
    out = str(tmp_path / "groups.ovr")
    a.write_overrepresented(out, "S", names, idx)
    assert open(out).read() == ovr_ref.text(want, "S", names, idx)
    a.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 10. the module off: no memory, no launch
# ---------------------------------------------------------------------------------------------------------------------------
def _free_bytes():
    from tests.hipmem import Hip
    free_b, total_b = C.c_size_t(), C.c_size_t()
    assert Hip().rt.hipMemGetInfo(C.byref(free_b), C.byref(total_b)) == 0
    return free_b.value


def test_module_off_allocates_and_launches_nothing(order):
    cols, want = order
    base = dict(BASE, n_lanes=ovr_steps.ORDER_LANES)
    warm = Aggregator(**base)  # (the runtime's own first allocations are not the context's)
    warm.close()
    table = 24 << 23           # capacity 2^22: 2^23 slots of 24 bytes
    used = {}
    for which, more in (("off", {}), ("off again", {}), ("on", dict(overrepresented=(50, 1 << 22)))):
        before = _free_bytes()
        a = Aggregator(**dict(base, **more))
        used[which] = before - _free_bytes()
        a.set_timing(True)
        b = a.upload(cols)
        a.process(b)
        a.sync()
        names = a.last_timing()
        assert ("k_ovr" in names) == (which == "on"), names
        b.free()
        a.close()
    assert abs(used["off"] - used["off again"]) < table // 4 and used["on"] - used["off"] >= table - table // 4, used


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the program
# ---------------------------------------------------------------------------------------------------------------------------
CHROMS = ["-c", "chr1,chr2"]
NAMES, LENS = ["chr1", "chr2"], [400_000, 150_000]


def run(args, env=None, **kw):
    return subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, **(env or {})), timeout=120, **kw)


def same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """4000 synthetic paired reads in two read groups, the same file with 300 of its records written a second and 40 of those a third
    time (the triples reach the threshold of either mate), the `.bamqc` of runs without the option, and the text the restatement makes
    of each file."""
    d = tmp_path_factory.mktemp("ovr")
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
        assert not os.path.exists(out["base_" + name] + ".ovr")
        c = pybam.columns(path)[0]
        out["want_" + name] = lambda K=50, ppm=1000, capacity=1 << 26, c=c: ovr_ref.text(ovr_ref.view_fast(c, 2, K, ppm, capacity), sample, names, idx)
        out["view_" + name] = ovr_ref.view_fast(c, 2, 50, 1000, 1 << 26)
    vp, vd = out["view_plain"], out["view_dupd"]
    assert sum(len(l) for l in vd["listed"]) >= 30 and int(vd["distinct"].sum()) == int(vp["distinct"].sum()) and vd["hist"][:, 2].sum() >= 30
    return out


@pytest.mark.parametrize("decode", ["0", "1"])
def test_program_bam(files, decode):
    out = str(files["dir"] / ("bam%s.bamqc" % decode))
    r = run(["-r", files["fa"], "-o", out, "--overrepresented", "--overrepresented-capacity", "100000"] + CHROMS + [files["dupd"]], env=dict(BQC_GPU_DECODE=decode))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base_dupd"])
    assert open(out + ".ovr").read() == files["want_dupd"](capacity=100000)
    assert not os.path.exists(out + ".dup") and not os.path.exists(out + ".wdp")


def test_program_sam_on_stdin_other_length_and_threshold(files):
    out = str(files["dir"] / "sam.bamqc")
    sam = pybam.bam_to_sam_text(files["dupd"]).encode()
    r = run(["-r", files["fa"], "-o", out, "--overrepresented-len", "29", "--overrepresented-ppm", "500"] + CHROMS + ["-"], input=sam)
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["base_dupd"])
    assert open(out + ".ovr").read() == files["want_dupd"](29, 500)


def test_program_manifest_resets_per_job(files):
    d = files["dir"]
    jobs = [(files["dupd"], str(d / "m1.bamqc"), "dupd"), (files["plain"], str(d / "m2.bamqc"), "plain"), (files["dupd"], str(d / "m3.bamqc"), "dupd")]
    lst = str(d / "jobs.tsv")
    with open(lst, "w") as f:
        for i, o, _ in jobs:
            f.write("%s\t%s\n" % (i, o))
    r = run(["-r", files["fa"], "--overrepresented", "--overrepresented-capacity", "65536", "--manifest", lst] + CHROMS)
    assert r.returncode == 0, r.stderr
    for i, o, which in jobs:
        assert same_bytes(o, files["base_" + which])
        assert open(o + ".ovr").read() == files["want_" + which](capacity=65536)
    assert files["want_dupd"]() != files["want_plain"]()


def test_program_all_other_modules(files):
    d = files["dir"]
    ten, eleven = str(d / "ten.bamqc"), str(d / "eleven.bamqc")
    sites, bed = str(d / "sites.tsv"), str(d / "panel.bed")
    with open(sites, "w") as f:
        f.write("".join("chr1\t%d\n" % p for p in range(1000, 3000, 7)))
    with open(bed, "w") as f:
        f.write("".join("chr1\t%d\t%d\n" % (p, p + 300) for p in range(2000, 390_000, 5000)))
    mods = ["--qual-by-cycle", "--mismatch-by-cycle", "--adapter-by-cycle", "--gc-bias", "--indel-by-cycle", "--substitutions", "--site-alleles", sites, "--regions", bed,
            "--duplicate-sets", "--duplicate-sets-capacity", "4096", "--window-depth"]
    r = run(["-r", files["fa"], "-o", ten] + mods + CHROMS + [files["dupd"]])
    assert r.returncode == 0, r.stderr
    r = run(["-r", files["fa"], "-o", eleven] + mods + ["--overrepresented", "--overrepresented-capacity", "4096"] + CHROMS + [files["dupd"]])
    assert r.returncode == 0, r.stderr
    for ext in ("", ".qbc", ".mbc", ".adp", ".gcb", ".ibc", ".sbc", ".sac", ".rcv", ".dup", ".wdp"):
        assert same_bytes(eleven + ext, ten + ext), ext
    assert same_bytes(eleven, files["base_dupd"])
    assert open(eleven + ".ovr").read() == files["want_dupd"](capacity=4096)


def test_program_messages(files):
    d = files["dir"]
    never = str(d / "never.bamqc")
    r = run(["--gpus", "2", "-r", files["fa"], "-o", never, "--overrepresented"] + CHROMS + [files["dupd"]], env=dict(BQC_GPUS_SHARE_DEVICE="1"))
    assert r.returncode != 0 and b"--overrepresented with --gpus is not supported" in r.stderr, r.stderr
    for opt, bad, words in (("--overrepresented-len", ("10", "19", "57", "x"), b"20 to 56"), ("--overrepresented-ppm", ("9", "1000001", ""), b"10 to 1000000"),
                            ("--overrepresented-capacity", ("15", "2147483649", "-1"), b"16 to 2147483648")):
        for v in bad:
            r = run(["-r", files["fa"], "-o", never, opt, v] + CHROMS + [files["dupd"]])
            assert r.returncode != 0 and words in r.stderr, (opt, v, r.stderr)
    assert not os.path.exists(never) and not os.path.exists(never + ".ovr")
    small = str(d / "small.bamqc")
    r = run(["-r", files["fa"], "-o", small, "--overrepresented-capacity", "16"] + CHROMS + [files["dupd"]])
    assert r.returncode == 1, r.stderr
    assert b"16" in r.stderr and b"--overrepresented-capacity" in r.stderr and not os.path.exists(small + ".ovr"), r.stderr
    blocked = str(d / "blocked.bamqc")
    os.mkdir(blocked + ".ovr")  # (a directory where the table's file would go)
    r = run(["-r", files["fa"], "-o", blocked, "--overrepresented", "--overrepresented-capacity", "100000"] + CHROMS + [files["dupd"]])
    assert r.returncode == 1
    assert b"Could not write output file" in r.stderr and b".ovr" in r.stderr
