"""Device time of the depth in fixed genome windows (k_wdp; --window-depth) beside k_ibc on the same batch (the same walk without hot
adds) and beside k_rcv on its exome list, on reads resident in HBM (tools/ibc_time.py's batches):
  sorted     10 M x 150 bp over 4 x 25 M bases as the generator gives them, by coordinate: the 64 reads of a wave lie in one or two
             windows;
  shuffled   the same reads in a random order;
  long       50 K x 10 kb over 250 M bases (an ONT-like CIGAR of about one operation per five bases): the wave path.
Each with windows of 1000 and of 100 bases, and each of those as the kernel is (adds of neighbouring lanes to one word combined in the
waves that have such lanes), with BQC_WDP_COMBINE=0 (never combined) and =2 (combined in every wave).  The switch is read at every
launch, so the modes of a (batch, window) run in one context on one resident batch, between resets; the tool asserts that they leave
the same words.

usage: python tools/wdp_time.py [--reads N] [--long-reads N] [--passes P] [--only SHAPE] [--bench FILE] [--out FILE]
Every shape runs in a process of its own.  Times come from bqc_set_timing / bqc_last_timing (HIP events around each launch), after
three warm-up passes, as the median and the range of P passes.  --bench FILE merges the six numbers of the alternating plain bench.py
runs of this tree and its parent (a JSON object with the lists "parent" and "this_tree", ms a step) under bench_module_off."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.dup_time import shuffled  # noqa: E402
from tools.ibc_time import SHAPES, long_cigars, short_cigars  # noqa: E402
from tools.rcv_time import N_REGIONS, REGION_LEN, even_regions, stats  # noqa: E402

MODES = {"default": None, "never": "0", "always": "2"}
WINDOWS = (1000, 100)
RUNS = ("sorted", "shuffled", "long")


def child(shape, reads, passes):
    import numpy as np
    from bamqc_amd import Aggregator, synth
    S = SHAPES["long" if shape == "long" else "short"]
    n_refs = len(S["lens"])
    cols = synth.batch(S["seed"], reads, S["lens"], None, read_len=S["read_len"], isize=S["isize"], long_reads=S["long_reads"])
    cols["mapq"][:] = 0  # (no read is eligible for the triplets: no contig is needed, and the reads may come in any order; MQ is 0 below)
    L = cols["l_seq"].astype(np.int64)
    ncig, w, _ = short_cigars(np, L, 0.01, np.random.default_rng(7)) if shape != "long" else long_cigars(np, L)
    cols["n_cigar"], cols["cigar"] = np.where(L > 0, ncig, 0).astype(np.uint16), w.astype(np.uint32)
    cols["nm"] = np.full(len(L), -1, np.int32)
    key = cols["rid"].astype(np.int64) << 32 | cols["pos"].astype(np.int64)
    by_coordinate = bool((np.diff(key[cols["rid"] >= 0]) >= 0).all())
    if shape == "shuffled":
        cols = shuffled(np, cols, np.random.default_rng(5).permutation(len(L)))
    f = cols["flag"].astype(np.int64)
    ex = ((f & 0xF04) == 0) & (cols["l_seq"] > 0) & (cols["n_cigar"] > 0) & (cols["rid"] >= 0)
    out = {"shape": shape, "reads": reads, "bases": int(L.sum()), "cigar_words": int(len(w)), "examined_reads_per_pass": int(ex.sum()),
           "generated_by_coordinate": by_coordinate, "windows": {}}
    regions = even_regions(np, S["lens"], N_REGIONS, REGION_LEN)
    for W in WINDOWS:
        rcv = dict(regions=regions, region_min_mapq=0) if shape == "sorted" and W == WINDOWS[0] else {}  # k_rcv on its exome list, in the same call
        a = Aggregator(n_refs=n_refs, isize=S["isize"], max_read_len=S["max_read_len"], hist_cap=S["hist_cap"], indel_by_cycle=1024,
                       window_depth=(W, S["lens"]), window_min_mapq=0, **rcv)
        db = a.upload(cols)
        res = {"n_windows": int(sum((n + W - 1) // W for n in S["lens"])), "modes": {}}
        digest = {}
        for mode, value in MODES.items():
            if value is None:
                os.environ.pop("BQC_WDP_COMBINE", None)
            else:
                os.environ["BQC_WDP_COMBINE"] = value
            a.reset()
            a.set_timing(False)
            for _ in range(3):  # warm-up: code objects, clocks
                a.process(db)
            a.sync()
            a.set_timing(True)
            kt = {}
            for _ in range(passes):
                a.process(db)
                for k, v in a.last_timing().items():
                    kt.setdefault(k, []).append(v)
            a.finalize_raw()
            v = a.window_depth(0)
            assert v["reads_examined"] == out["examined_reads_per_pass"] * (passes + 3), (v["reads_examined"], out["examined_reads_per_pass"])
            digest[mode] = hashlib.sha256(b"".join(v[k].tobytes() for k in ("reads", "bases", "bases_low")) + str((v["reads_examined"], v["bases_outside"])).encode()).hexdigest()
            res["modes"][mode] = {"env": {} if value is None else {"BQC_WDP_COMBINE": value},
                                  "kernels_ms": {k: stats(np, kt[k]) for k in ("k_wdp", "k_ibc") + (("k_rcv",) if rcv else ())},
                                  "bases": int(v["bases"].sum()), "bases_outside": v["bases_outside"], "max_window_bases": int(v["bases"].max())}
        assert len(set(digest.values())) == 1, digest  # (the same words by every mode)
        res["words_sha256"] = digest["default"]
        out["windows"][str(W)] = res
        db.free()
        a.close()
    os.environ.pop("BQC_WDP_COMBINE", None)
    print("WDP_CHILD " + json.dumps({"key": shape, "result": out}), flush=True)


def run_child(shape, reads, passes):
    env = dict(os.environ)
    env.pop("BQC_WDP_COMBINE", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--reads", str(reads), "--passes", str(passes)], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [json.loads(l[10:]) for l in r.stdout.splitlines() if l.startswith("WDP_CHILD ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--long-reads", type=int, default=50_000)
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--only", default=None)
    ap.add_argument("--bench", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reads, args.passes)
    res = {"what": "tools/wdp_time.py: k_wdp with its combining as built, never and always, beside k_ibc on the same batch and k_rcv on its exome list; "
                   "HIP-event times, median and range of the passes", "shapes": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    for shape in RUNS:
        if args.only and args.only != shape:
            continue
        for item in run_child(shape, args.long_reads if shape == "long" else args.reads, args.passes):
            res["shapes"][item["key"]] = item["result"]
            for W, r in item["result"]["windows"].items():
                print(item["key"], "W", W, json.dumps({m: {k: v["median"] for k, v in x["kernels_ms"].items()} for m, x in r["modes"].items()}), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    # the default rule against the better forced mode, by that mode's own range
    res["default_rule"] = {}
    for shape, r in res["shapes"].items():
        for W, x in r["windows"].items():
            t = {m: x["modes"][m]["kernels_ms"]["k_wdp"] for m in MODES}
            best = min(("never", "always"), key=lambda m: t[m]["median"])
            res["default_rule"]["%s_W%s" % (shape, W)] = {"default_ms": t["default"]["median"], "better_forced": best, "better_forced_ms": t[best]["median"],
                                                           "better_forced_range_ms": t[best]["max"] - t[best]["min"],
                                                           "default_within_range": t["default"]["median"] <= t[best]["median"] + (t[best]["max"] - t[best]["min"]),
                                                           "k_wdp_over_k_ibc": t["default"]["median"] / x["modes"]["default"]["kernels_ms"]["k_ibc"]["median"]}
    if "sorted" in res["shapes"] and "shuffled" in res["shapes"]:  # (the same reads in two orders: the same words)
        for W in res["shapes"]["sorted"]["windows"]:
            assert res["shapes"]["sorted"]["windows"][W]["words_sha256"] == res["shapes"]["shuffled"]["windows"][W]["words_sha256"], W
    if args.bench:
        with open(args.bench) as f:
            res["bench_module_off"] = json.load(f)
    print(json.dumps(res["default_rule"], indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
