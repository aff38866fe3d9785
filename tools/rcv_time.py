"""Device time of the depth over given regions (k_rcv, k_rcv_final; --regions) beside k_ibc and k_sac (1 M sites) on the same batch, on
reads resident in HBM (tools/ibc_time.py's batches):
  exome   10 M x 150 bp over 4 x 25 M bases against 200 K regions of 200 bases, one every 500 bases: about 70 % of the reads on target;
  panel   the same reads moved onto 50 amplicons of 200 bases: every read on a region, the contention case;
  long    50 K x 10 kb over 250 M bases (an ONT-like CIGAR of about one operation per five bases) against 200 K regions of 200 bases.
Each is timed as the kernel is, with BQC_RCV_INDEX=0 (a binary search over the contig's whole run of regions instead of the bucket
index) and, for the long reads, with BQC_RCV_T=65535 (every read by its own thread).  After the exome passes bqc_finalize is timed
(k_rcv_final: B = 40 M, R = 200 K) with 1 and with 4 read groups, against the bytes it must read (8 B a slot, twice) at the card's
measured copy rate.

usage: python tools/rcv_time.py [--reads N] [--long-reads N] [--passes P] [--only SHAPE_MODE] [--out FILE]
Every (shape, mode) runs in a process of its own (the switches are read once per process).  Times come from bqc_set_timing /
bqc_last_timing (HIP events around each launch), after three warm-up passes, as the median and the range of P passes.  The parent
checks that the modes of a shape counted the same."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.ibc_time import COPY_CEILING, SHAPES, long_cigars, short_cigars  # noqa: E402
from tools.sac_time import even_sites  # noqa: E402

MODES = {"index": {}, "plain_search": {"BQC_RCV_INDEX": "0"}, "thread_path": {"BQC_RCV_T": "65535"}}
RUNS = [("exome", "index"), ("exome", "plain_search"), ("panel", "index"), ("long", "index"), ("long", "plain_search"), ("long", "thread_path")]
BATCH_OF = {"exome": "short", "panel": "short", "long": "long"}
N_REGIONS, REGION_LEN, N_SITES = 200_000, 200, 1_000_000


def even_regions(np, lens, total, length):
    """`total` regions of `length` bases spread evenly over the contigs, in proportion to their lengths."""
    rid, start = even_sites(np, lens, total)
    assert (np.diff(start.astype(np.int64))[np.diff(rid) == 0] > length).all()
    start = np.minimum(start.astype(np.int64), np.asarray(lens, np.int64)[rid] - length).astype(np.int32)
    return rid, start, (start + length).astype(np.int32)


def stats(np, v):
    v = np.array(v)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "passes": [float(x) for x in v]}


def child(shape, mode, reads, passes):
    import numpy as np
    from bamqc_amd import Aggregator, synth
    S = SHAPES[BATCH_OF[shape]]
    refs = [synth.reference(S["seed"], i, n) for i, n in enumerate(S["lens"])]
    cols = synth.batch(S["seed"], reads, S["lens"], refs, read_len=S["read_len"], isize=S["isize"], long_reads=S["long_reads"])
    L = cols["l_seq"].astype(np.int64)
    rng = np.random.default_rng(7)
    ncig, w, _ = short_cigars(np, L, 0.01, rng) if BATCH_OF[shape] == "short" else long_cigars(np, L)
    ncig = np.where(L > 0, ncig, 0)
    cols["n_cigar"], cols["cigar"] = ncig.astype(np.uint16), w.astype(np.uint32)
    cols["nm"] = np.full(len(L), -1, np.int32)
    if shape == "panel":
        regions = even_regions(np, S["lens"][:1], 50, REGION_LEN)
        i = np.arange(len(L))
        cols["rid"] = np.where(cols["rid"] >= 0, 0, cols["rid"]).astype(np.int32)
        cols["pos"] = (regions[1][i % 50].astype(np.int64) + i % 40).astype(np.int32)
    else:
        regions = even_regions(np, S["lens"], N_REGIONS, REGION_LEN)
    f = cols["flag"].astype(np.int64)
    examined = ((f & 0xF04) == 0) & (cols["mapq"] >= 20) & (L > 0) & (ncig > 0) & (cols["rid"] >= 0)
    B, R = int((regions[2].astype(np.int64) - regions[1]).sum()), len(regions[0])
    out = {"shape": shape, "mode": mode, "env": MODES[mode], "reads": reads, "bases": int(L.sum()), "cigar_words": int(len(w)), "regions": R, "target_bases": B,
           "examined_reads_per_pass": int(examined.sum()), "passes_counted": passes + 3, "kernels_ms": {}}
    sac = dict(site_alleles=even_sites(np, S["lens"], N_SITES)) if mode == "index" and shape != "panel" else {}
    a = Aggregator(n_refs=len(refs), isize=S["isize"], max_read_len=S["max_read_len"], hist_cap=S["hist_cap"], indel_by_cycle=1024, regions=regions, **sac)
    for i, r in enumerate(refs):
        a.set_reference(i, r)
    db = a.upload(cols)
    for _ in range(3):  # warm-up: code objects, clocks
        a.process(db)
    a.sync()
    a.set_timing(True)
    kt = {}
    for _ in range(passes):
        a.process(db)
        for k, v in a.last_timing().items():
            kt.setdefault(k, []).append(v)
    fin = []
    for _ in range(passes if shape == "exome" and mode == "index" else 1):
        a.finalize_raw()
        fin.append(a.last_timing()["k_rcv_final"])
    v = a.region_coverage(0)
    out.update(reads_on_target=v["reads_on_target"], reads_examined=v["reads_examined"], bases_on_target=v["bases_on_target"], aligned_bases=v["aligned_bases"],
               max_depth=int(v["regions"][:, 2].max()))
    assert v["reads_examined"] == out["examined_reads_per_pass"] * (passes + 3), (v["reads_examined"], out["examined_reads_per_pass"])
    for k in ("k_rcv", "k_ibc") + (("k_sac",) if sac else ()):
        out["kernels_ms"][k] = stats(np, kt[k])
    out["kernels_ms"]["k_rcv_final"] = stats(np, fin)
    floor_bytes = 2 * 8 * (B + R)
    out["final_floor_bytes"], out["final_floor_ms"] = floor_bytes, floor_bytes / COPY_CEILING * 1e3
    out["final_floor_fraction"] = out["final_floor_ms"] / out["kernels_ms"]["k_rcv_final"]["median"]
    db.free()
    a.close()
    if shape == "exome" and mode == "index":  # the finalize pass with four read groups (the reads are all of the first)
        a = Aggregator(n_lanes=4, n_refs=len(refs), isize=S["isize"], max_read_len=S["max_read_len"], hist_cap=S["hist_cap"], regions=regions)
        for i, r in enumerate(refs):
            a.set_reference(i, r)
        db = a.upload(cols)
        a.process(db)
        a.sync()
        a.set_timing(True)
        fin = []
        for _ in range(passes):
            a.finalize_raw()
            fin.append(a.last_timing()["k_rcv_final"])
        out["kernels_ms"]["k_rcv_final_4_lanes"] = stats(np, fin)
        out["final_4_lanes_floor_ms"] = 4 * out["final_floor_ms"]
        out["final_4_lanes_floor_fraction"] = 4 * out["final_floor_ms"] / out["kernels_ms"]["k_rcv_final_4_lanes"]["median"]
        db.free()
        a.close()
    print("RCV_CHILD " + json.dumps({"key": "%s_%s" % (shape, mode), "result": out}), flush=True)


def run_child(shape, mode, reads, passes):
    env = dict(os.environ)
    for k in ("BQC_RCV_T", "BQC_RCV_INDEX"):
        env.pop(k, None)
    env.update(MODES[mode])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%s_%s" % (shape, mode), "--reads", str(reads), "--passes", str(passes)], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [json.loads(l[10:]) for l in r.stdout.splitlines() if l.startswith("RCV_CHILD ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--long-reads", type=int, default=50_000)
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        shape, mode = args.child.split("_", 1)
        return child(shape, mode, args.reads, args.passes)
    res = {"what": "tools/rcv_time.py: k_rcv beside k_ibc and k_sac on the same batch, and k_rcv_final; HIP-event times, median and range of the passes", "variants": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    for shape, mode in RUNS:
        if args.only and args.only != "%s_%s" % (shape, mode):
            continue
        for item in run_child(shape, mode, args.long_reads if shape == "long" else args.reads, args.passes):
            res["variants"][item["key"]] = item["result"]
            print(item["key"], json.dumps({k: v["median"] for k, v in item["result"]["kernels_ms"].items()}), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    v = res["variants"]
    res["ratios"] = {}
    for shape in ("exome", "long"):
        base = v.get("%s_index" % shape)
        for mode in ("plain_search", "thread_path"):
            other = v.get("%s_%s" % (shape, mode))
            if base and other:
                assert all(base[k] == other[k] for k in ("reads_on_target", "bases_on_target", "aligned_bases")), (shape, mode)  # (the same sums by every path)
                key = "%s_%s_over_index" % (shape, mode)
                res["ratios"][key] = other["kernels_ms"]["k_rcv"]["median"] / base["kernels_ms"]["k_rcv"]["median"]
                print("%s: %.2f" % (key, res["ratios"][key]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
