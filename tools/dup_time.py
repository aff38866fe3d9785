"""Device time of the duplicate sets (k_dup, k_dup_final, the table's clear; --duplicate-sets) beside k_ibc and k_rcv (200 K regions) on
the same batch, on reads resident in HBM (tools/ibc_time.py's short batch: 10 M x 150 bp paired reads over 4 x 25 M bases), at the
program's default capacity (2^26 signatures: 2^27 slots, 3 GiB):
  sorted     the batch as the generator gives it, by coordinate;
  shuffled   the same reads in a random order;
  hot        the sorted reads moved onto 2000 positions of one contig, 5000 consecutive reads each, with one template length: a few
             thousand signatures of thousands of reads, side by side (an amplicon panel, the contention case).
Each order is timed FRESH (the context is reset before every pass: every signature is new to the table) and REPEATED (the passes that
follow: every signature is there already), in five modes of the kernel's two measuring switches: as built (equal signatures of a wave
are combined where two of them lie side by side; the whole signature is mixed), BQC_DUP_COMBINE=0 (never combined), =2 (combined in
every wave), BQC_DUP_HASH=1 (u5's low 6 bits stay in the slot: locality), and the last two together.
The as-built child also times bqc_finalize's scan (k_dup_final) and the clear of the table (the wall time of bqc_reset with the module
on minus off) against the bytes they move at the card's measured copy rate, and the wall time of creating a context with the module
on and off.  --program N times the program itself on a file of N reads with and without --duplicate-sets, alternating.

usage: python tools/dup_time.py [--reads N] [--passes P] [--only MODE] [--program N] [--out FILE]
Every mode runs in a process of its own (the switches are read once per process).  Kernel times come from bqc_set_timing /
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
from tools.ibc_time import COPY_CEILING, SHAPES, short_cigars  # noqa: E402
from tools.rcv_time import N_REGIONS, REGION_LEN, even_regions, stats  # noqa: E402

MODES = {"built": {}, "no_combine": {"BQC_DUP_COMBINE": "0"}, "always_combine": {"BQC_DUP_COMBINE": "2"}, "local_hash": {"BQC_DUP_HASH": "1"},
         "always_combine_local_hash": {"BQC_DUP_COMBINE": "2", "BQC_DUP_HASH": "1"}}
CAPACITY = 1 << 26
SLOT_BYTES = 24


def shuffled(np, cols, perm):
    """The reads of `cols` (all of one length) in the order `perm`."""
    n = len(perm)
    L = int(cols["l_seq"][0])
    assert (cols["l_seq"] == L).all() and L % 2 == 0
    out = {k: v[perm] for k, v in cols.items() if k not in ("seq", "qual", "cigar")}
    out["seq"] = cols["seq"].reshape(n, L // 2)[perm].ravel()
    out["qual"] = cols["qual"].reshape(n, L)[perm].ravel()
    nc = cols["n_cigar"].astype(np.int64)
    off = np.cumsum(nc) - nc
    ncp = nc[perm]
    k = np.arange(int(ncp.sum())) - np.repeat(np.cumsum(ncp) - ncp, ncp)
    out["cigar"] = cols["cigar"][np.repeat(off[perm], ncp) + k]
    return out


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
    ex = ((f & 0xB04) == 0) & (L > 0) & (cols["n_cigar"] > 0) & (cols["rid"] >= 0)
    second = ex & ((f & 1) != 0) & ((f & 8) == 0) & (cols["tlen"] < 0)
    key = cols["rid"].astype(np.int64) << 32 | cols["pos"].astype(np.int64)
    out = {"mode": mode, "env": MODES[mode], "reads": reads, "capacity": CAPACITY, "slots": 2 * CAPACITY, "table_bytes": 2 * CAPACITY * SLOT_BYTES,
           "examined_reads": int(ex.sum()), "inserted_reads": int((ex & ~second).sum()), "sorted_input": bool((np.diff(key[cols["rid"] >= 0]) >= 0).all()), "orders": {}}
    regions = even_regions(np, S["lens"], N_REGIONS, REGION_LEN)
    base = dict(n_refs=n_refs, isize=S["isize"], max_read_len=S["max_read_len"], hist_cap=S["hist_cap"])
    for order in ("sorted", "shuffled", "hot"):
        c = cols if order == "sorted" else shuffled(np, cols, np.random.default_rng(5).permutation(len(L))) if order == "shuffled" else dict(cols)
        if order == "hot":
            c["rid"] = np.where(cols["rid"] >= 0, 0, cols["rid"]).astype(np.int32)
            c["pos"] = (np.arange(len(L)) // 5000 * 100).astype(np.int32)
            c["tlen"] = (np.sign(cols["tlen"]) * 300).astype(np.int32)
        a = Aggregator(indel_by_cycle=1024, regions=regions, region_min_mapq=0, duplicate_sets=CAPACITY, **base)
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
        v = a.duplicate_sets()
        o = {"sets": [int(x) for x in v["sets"]], "largest": [int(x) for x in v["largest"]], "estimated_library_size": v["estimated_library_size"],
             "fresh_ms": {k: stats(np, fresh[k]) for k in ("k_dup", "k_ibc", "k_rcv")}, "repeated_ms": {k: stats(np, again[k]) for k in ("k_dup", "k_ibc", "k_rcv")}}
        assert int(v["lanes"][:, :2].sum()) == out["inserted_reads"] * (passes + 1), (v["lanes"], out["inserted_reads"])
        o["fresh_inserts_per_us"] = out["inserted_reads"] / (o["fresh_ms"]["k_dup"]["median"] * 1e3)
        o["repeated_inserts_per_us"] = out["inserted_reads"] / (o["repeated_ms"]["k_dup"]["median"] * 1e3)
        out["orders"][order] = o
        db.free()
        a.close()
    if mode == "built":  # the scan, the clear and the context's creation
        t0 = time.perf_counter()
        a = Aggregator(duplicate_sets=CAPACITY, **base)
        a.sync()  # (the clear is left on the stream: this waits for it)
        t_on = time.perf_counter() - t0
        t0 = time.perf_counter()
        b = Aggregator(**base)
        b.sync()
        t_off = time.perf_counter() - t0
        out["create_wall_ms"] = {"module_on": t_on * 1e3, "module_off": t_off * 1e3}
        db = a.upload(cols)
        a.process(db)
        a.sync()
        a.set_timing(True)
        fin = []
        for _ in range(passes):
            a.finalize_raw()
            fin.append(a.last_timing()["k_dup_final"])
        out["k_dup_final_ms"] = stats(np, fin)
        scan_bytes = 2 * CAPACITY * 16  # (k0 and the count of every slot; every line of the table is touched: 24 B a slot)
        out["final_floor_ms"] = {"bytes_read": scan_bytes / COPY_CEILING * 1e3, "lines_touched": out["table_bytes"] / COPY_CEILING * 1e3}
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
    print("DUP_CHILD " + json.dumps({"key": mode, "result": out}), flush=True)


def run_child(mode, reads, passes):
    env = dict(os.environ)
    for k in ("BQC_DUP_COMBINE", "BQC_DUP_HASH"):
        env.pop(k, None)
    env.update(MODES[mode])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--reads", str(reads), "--passes", str(passes)], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [json.loads(l[10:]) for l in r.stdout.splitlines() if l.startswith("DUP_CHILD ")]


def program(n_reads, runs=5):
    """Wall time of the program on a file of n_reads reads, with and without --duplicate-sets, alternating."""
    import numpy as np
    from bamqc_amd import hostio
    exe = os.path.join(ROOT, "bin", "bamqualcheck")
    out = {"reads": n_reads, "with_ms": [], "without_ms": []}
    with tempfile.TemporaryDirectory() as d:
        bam, fa = os.path.join(d, "in.bam"), os.path.join(d, "in.fa")
        hostio.synth_write(bam, fa, seed=77, n_reads=n_reads, ref_names=["chr1", "chr2"], ref_lens=[40_000_000, 20_000_000], n_lanes=2)
        for k in range(runs + 1):  # (the first pair warms the file cache and is left out)
            for key, opt in (("without_ms", []), ("with_ms", ["--duplicate-sets"])):
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
    res = {"what": "tools/dup_time.py: k_dup beside k_ibc and k_rcv on the same batch, k_dup_final, the table's clear; HIP-event times, median and range of the passes", "modes": {}}
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
            print(item["key"], json.dumps({o: {"fresh": v["fresh_ms"]["k_dup"]["median"], "repeated": v["repeated_ms"]["k_dup"]["median"], "k_ibc": v["fresh_ms"]["k_ibc"]["median"],
                                               "k_rcv": v["fresh_ms"]["k_rcv"]["median"]} for o, v in item["result"]["orders"].items()}), flush=True)
        save()
    for shape in (("sorted", "shuffled"), ("hot",)):  # (the same sets by every mode, and by both orders of the same reads)
        sets = {(m, o): v["sets"] for m, r in res["modes"].items() for o, v in r["orders"].items() if o in shape}
        assert len({tuple(s) for s in sets.values()}) <= 1, sets
    if args.program:
        res["program"] = program(args.program)
        print("program", json.dumps(res["program"]), flush=True)
    save()


if __name__ == "__main__":
    main()
