"""Device time of the overrepresented sequences (k_ovr, k_ovr_final, the table's clear; --overrepresented) beside k_dup on the same
batch in the same process, on reads resident in HBM (tools/ibc_time.py's short batch: 10 M x 150 bp paired reads over 4 x 25 M bases),
both tables at the program's default capacity (2^26 keys: 2^27 slots, 3 GiB each), prefix length 50:
  sorted     the batch as the generator gives it, by coordinate;
  shuffled   the same reads in a random order;
  hot        the sorted reads with the bases AND the alignment of the first of every 5000 consecutive reads: a few thousand sequences
             (and signatures) of thousands of reads, side by side (adapter dimers at a file's end, an amplicon panel).
Each order is timed FRESH (the context is reset before every pass: every key is new to the table) and REPEATED (the passes that
follow: every key is there already), in three modes of the kernel's measuring switch: as built (equal keys of a wave are combined
where two of them lie side by side), BQC_OVR_COMBINE=0 (never combined), =2 (combined in every wave).  k_ovr makes one insert a read
as k_dup does, and reads up to 29 payload bytes a read in addition: k_dup is the yardstick.
The as-built child also times bqc_finalize's scan (k_ovr_final) and the clear of the table (the wall time of bqc_reset with the module
on minus off) against the bytes they move at the card's measured copy rate.  --program N times the program itself on a file of N
reads with and without --overrepresented, alternating.

usage: python tools/ovr_time.py [--reads N] [--passes P] [--only MODE] [--program N] [--out FILE]
Every mode runs in a process of its own (the switch is read once per process).  Kernel times come from bqc_set_timing /
bqc_last_timing (HIP events around each launch), after two warm-up passes, as the median and the range of P passes.  The parent checks
that every mode and order counted the same sets."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.dup_time import shuffled  # noqa: E402
from tools.ibc_time import COPY_CEILING, SHAPES, short_cigars  # noqa: E402
from tools.rcv_time import stats  # noqa: E402

MODES = {"built": {}, "no_combine": {"BQC_OVR_COMBINE": "0"}, "always_combine": {"BQC_OVR_COMBINE": "2"}}
CAPACITY = 1 << 26
SLOT_BYTES = 24
K = 50


def child(mode, reads, passes):
    import numpy as np
    from bamqc_amd import Aggregator, synth
    S = SHAPES["short"]
    n_refs = len(S["lens"])
    cols = synth.batch(S["seed"], reads, S["lens"], None, read_len=S["read_len"], isize=S["isize"])
    cols["mapq"][:] = 0  # (no read is eligible for the triplets: no contig is needed, and the reads may come in any order)
    L = cols["l_seq"].astype(np.int64)
    ncig, w, _ = short_cigars(np, L, 0.01, np.random.default_rng(7))
    cols["n_cigar"], cols["cigar"] = np.where(L > 0, ncig, 0).astype(np.uint16), w.astype(np.uint32)
    cols["nm"] = np.full(len(L), -1, np.int32)
    f = cols["flag"].astype(np.int64)
    ex = ((f & 0x900) == 0) & ((f & 0xC0) != 0) & (L > 0)
    out = {"mode": mode, "env": MODES[mode], "reads": reads, "prefix_len": K, "capacity": CAPACITY, "slots": 2 * CAPACITY, "table_bytes": 2 * CAPACITY * SLOT_BYTES,
           "examined_reads": int(ex.sum()), "payload_bytes": int(len(cols["seq"])), "orders": {}}
    base = dict(n_refs=n_refs, isize=S["isize"], max_read_len=S["max_read_len"], hist_cap=S["hist_cap"])
    for order in ("sorted", "shuffled", "hot"):
        c = cols if order == "sorted" else shuffled(np, cols, np.random.default_rng(5).permutation(len(L))) if order == "shuffled" else dict(cols)
        if order == "hot":
            n, rl = len(L), int(L[0])
            first = np.arange(n) // 5000 * 5000
            c["seq"] = cols["seq"].reshape(n, rl // 2)[first].ravel()
            c["flag"] = ((cols["flag"] & ~np.uint16(0x10)) | (cols["flag"][first] & np.uint16(0x10))).astype(np.uint16)
            c["rid"] = np.where(cols["rid"] >= 0, 0, cols["rid"]).astype(np.int32)
            c["pos"] = (first // 5000 * 100).astype(np.int32)
            c["tlen"] = (np.sign(cols["tlen"]) * 300).astype(np.int32)
        a = Aggregator(duplicate_sets=CAPACITY, overrepresented=(K, CAPACITY), **base)
        db = a.upload(c)
        for _ in range(2):  # warm-up: code objects, clocks
            a.reset()
            a.process(db)
        a.sync()
        a.set_timing(True)
        fresh, again = {}, {}
        for _ in range(passes):
            a.reset()
            a.process(db)
            for k, v in a.last_timing().items():
                fresh.setdefault(k, []).append(v)
        for _ in range(passes):
            a.process(db)
            for k, v in a.last_timing().items():
                again.setdefault(k, []).append(v)
        v = a.overrepresented()
        entered = int(v["lanes"][:, :2].sum()) - int(v["lanes"][:, 2:].sum())
        o = {"distinct": [int(x) for x in v["distinct"]], "largest": [int(x) for x in v["largest"]], "listed": [len(l) for l in v["listed"]],
             "entered_reads": entered // (passes + 1),
             "fresh_ms": {k: stats(np, fresh[k]) for k in ("k_ovr", "k_dup")}, "repeated_ms": {k: stats(np, again[k]) for k in ("k_ovr", "k_dup")}}
        assert int(v["lanes"][:, :2].sum()) == out["examined_reads"] * (passes + 1), (v["lanes"], out["examined_reads"])
        o["fresh_ratio_to_k_dup"] = o["fresh_ms"]["k_ovr"]["median"] / o["fresh_ms"]["k_dup"]["median"]
        o["repeated_ratio_to_k_dup"] = o["repeated_ms"]["k_ovr"]["median"] / o["repeated_ms"]["k_dup"]["median"]
        o["payload_floor_ms"] = out["payload_bytes"] / COPY_CEILING * 1e3  # (every line of the payload is touched: a read's 75 bytes hold its 25 to 29)
        out["orders"][order] = o
        db.free()
        a.close()
    if mode == "built":  # the scan and the clear
        a = Aggregator(overrepresented=(K, CAPACITY), **base)
        b = Aggregator(**base)
        db = a.upload(cols)
        a.process(db)
        a.sync()
        a.set_timing(True)
        fin = []
        for _ in range(passes):
            a.finalize_raw()
            fin.append(a.last_timing()["k_ovr_final"])
        out["k_ovr_final_ms"] = stats(np, fin)
        out["final_floor_ms"] = {"bytes_read": 2 * CAPACITY * 16 / COPY_CEILING * 1e3, "lines_touched": out["table_bytes"] / COPY_CEILING * 1e3}
        on, off = [], []
        for _ in range(passes):
            t0 = time.perf_counter()
            a.reset()
            on.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            b.reset()
            off.append((time.perf_counter() - t0) * 1e3)
        out["reset_wall_ms"] = {"module_on": stats(np, on), "module_off": stats(np, off)}
        out["clear_ms"] = float(np.median(on) - np.median(off))
        out["clear_floor_ms"] = out["table_bytes"] / COPY_CEILING * 1e3
        db.free()
        a.close()
        b.close()
    print("OVR_CHILD " + json.dumps({"key": mode, "result": out}), flush=True)


def run_child(mode, reads, passes):
    env = dict(os.environ)
    env.pop("BQC_OVR_COMBINE", None)
    env.update(MODES[mode])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--reads", str(reads), "--passes", str(passes)], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [json.loads(l[10:]) for l in r.stdout.splitlines() if l.startswith("OVR_CHILD ")]


def program(n_reads, runs=5):
    """Wall time of the program on a file of n_reads reads, with and without --overrepresented, alternating."""
    import numpy as np
    from bamqc_amd import hostio
    exe = os.path.join(ROOT, "bin", "bamqualcheck")
    out = {"reads": n_reads, "with_ms": [], "without_ms": []}
    with tempfile.TemporaryDirectory() as d:
        bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "in.fa")
        hostio.synth_write(bam, fa, seed=77, n_reads=n_reads, ref_names=["chr1", "chr2"], ref_lens=[40_000_000, 20_000_000], n_lanes=2)
        for k in range(runs + 1):  # (the first pair warms the file cache and is left out)
            for key, opt in (("without_ms", []), ("with_ms", ["--overrepresented"])):
                t0 = time.perf_counter()
                r = subprocess.run([exe, "-r", fa, "-o", os.path.join(d, "out.bamqc"), "-c", "chr1,chr2"] + opt + [bam], capture_output=True, timeout=600)
                assert r.returncode == 0, r.stderr
                if k:
                    out[key].append((time.perf_counter() - t0) * 1e3)
    out["with"], out["without"] = stats(np, out.pop("with_ms")), stats(np, out.pop("without_ms"))
    out["added_ms"] = out["with"]["median"] - out["without"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--only", default=None)
    ap.add_argument("--program", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reads, args.passes)
    res = {"what": "tools/ovr_time.py: k_ovr beside k_dup on the same batch, k_ovr_final, the table's clear; HIP-event times, median and range of the passes", "modes": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    for mode in MODES:
        if args.only and args.only != mode:
            continue
        for item in run_child(mode, args.reads, args.passes):
            res["modes"][item["key"]] = item["result"]
            print(item["key"], json.dumps({o: {"fresh": v["fresh_ms"]["k_ovr"]["median"], "repeated": v["repeated_ms"]["k_ovr"]["median"], "k_dup_fresh": v["fresh_ms"]["k_dup"]["median"],
                                               "k_dup_repeated": v["repeated_ms"]["k_dup"]["median"]} for o, v in item["result"]["orders"].items()}), flush=True)
        save()
    for shape in (("sorted", "shuffled"), ("hot",)):  # (the same sets by every mode, and by both orders of the same reads)
        sets = {(m, o): v["distinct"] for m, r in res["modes"].items() for o, v in r["orders"].items() if o in shape}
        assert len({tuple(s) for s in sets.values()}) <= 1, sets
    if args.program:
        res["program"] = program(args.program)
        print("program", json.dumps(res["program"]), flush=True)
    save()


if __name__ == "__main__":
    main()
