"""Device time of the allele counts at given sites (k_sac; --site-alleles) beside k_ibc on the same batch, on reads resident in HBM:
the config-2 shape (10 M x 150 bp over 4 x 25 M bases, an indel in about 1 % of the reads) and the long-read shape (50 K x 10 kb over
250 M bases, an ONT-like CIGAR of about one operation per five bases: tools/ibc_time.py's batches), each with 10 K, 1 M and 16 M sites
spread evenly over the contigs.  Each (shape, sites) is timed as the kernel is, with BQC_SAC_INDEX=0 (a binary search over the
contig's whole run of sites instead of the bucket index) and, for the long reads, with BQC_SAC_T=65535 (every read by its own thread).

usage: python tools/sac_time.py [--reads N] [--long-reads N] [--passes P] [--only SHAPE_MODE] [--out FILE]
Every (shape, mode) runs in a process of its own (the switches are read once per process) and builds its batch once for the three
site counts.  Times come from bqc_set_timing / bqc_last_timing (HIP events around each launch), after three warm-up passes, as the
median and the range of P passes.  The floor is the bytes of the fixed columns that every read costs k_sac — flag, mapq, lane, rid, pos,
l_seq, n_cigar, cigar_off — at the card's measured copy rate.  The parent checks that the modes of a (shape, sites) counted the same."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.ibc_time import COPY_CEILING, SHAPES, long_cigars, short_cigars  # noqa: E402

SITE_COUNTS = {"10k": 10_000, "1m": 1_000_000, "16m": 1 << 24}
MODES = {"index": {}, "plain_search": {"BQC_SAC_INDEX": "0"}, "thread_path": {"BQC_SAC_T": "65535"}}
RUNS = [("short", "index"), ("short", "plain_search"), ("long", "index"), ("long", "plain_search"), ("long", "thread_path")]
COLUMN_BYTES = 2 + 1 + 1 + 4 + 4 + 4 + 2 + 4  # flag, mapq, lane, rid, pos, l_seq, n_cigar, cigar_off


def even_sites(np, lens, total):
    """`total` sites spread evenly over the contigs, in proportion to their lengths."""
    rid, pos = [], []
    whole = sum(lens)
    left = total
    for r, n in enumerate(lens):
        k = left if r == len(lens) - 1 else total * n // whole
        left -= k
        p = (np.arange(k, dtype=np.int64) * n) // max(k, 1)
        assert k <= n
        rid.append(np.full(k, r, np.int32))
        pos.append(p.astype(np.int32))
    return np.concatenate(rid), np.concatenate(pos)


def child(shape, mode, reads, passes):
    import numpy as np
    from bamqc_amd import Aggregator, synth
    S = SHAPES[shape]
    refs = [synth.reference(S["seed"], i, n) for i, n in enumerate(S["lens"])]
    cols = synth.batch(S["seed"], reads, S["lens"], refs, read_len=S["read_len"], isize=S["isize"], long_reads=S["long_reads"])
    L = cols["l_seq"].astype(np.int64)
    rng = np.random.default_rng(7)
    ncig, w, _ = short_cigars(np, L, 0.01, rng) if shape == "short" else long_cigars(np, L)
    ncig = np.where(L > 0, ncig, 0)
    cols["n_cigar"], cols["cigar"] = ncig.astype(np.uint16), w.astype(np.uint32)
    cols["nm"] = np.full(len(L), -1, np.int32)
    f = cols["flag"].astype(np.int64)
    examined = ((f & 0xF04) == 0) & ((f & 0x8000) == 0) & (cols["mapq"] >= 20) & (L > 0) & (ncig > 0) & (cols["rid"] >= 0)
    for name, total in SITE_COUNTS.items():
        sites = even_sites(np, S["lens"], total)
        a = Aggregator(n_refs=len(refs), isize=S["isize"], max_read_len=S["max_read_len"], hist_cap=S["hist_cap"], indel_by_cycle=1024, site_alleles=sites)
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
        a.finalize()
        count_sum = int(a.site_alleles(0).sum())
        db.free()
        a.close()
        floor_bytes = reads * COLUMN_BYTES
        out = {"shape": shape, "mode": mode, "sites": total, "reads": reads, "bases": int(L.sum()), "cigar_words": int(len(w)), "env": MODES[mode],
               "examined_reads_per_pass": int(examined.sum()), "count_sum": count_sum, "passes_counted": passes + 3,
               "floor_bytes": floor_bytes, "floor_ms": floor_bytes / COPY_CEILING * 1e3, "kernels_ms": {}}
        assert count_sum % (passes + 3) == 0 and count_sum > 0, count_sum
        for k in ("k_sac", "k_ibc"):
            v = np.array(kt[k])
            out["kernels_ms"][k] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "passes": [float(x) for x in v]}
        out["k_sac_over_floor"] = out["kernels_ms"]["k_sac"]["median"] / out["floor_ms"]
        print("SAC_CHILD " + json.dumps({"key": "%s_%s_%s" % (shape, name, mode), "result": out}), flush=True)


def run_child(shape, mode, reads, passes):
    env = dict(os.environ)
    for k in ("BQC_SAC_T", "BQC_SAC_INDEX"):
        env.pop(k, None)
    env.update(MODES[mode])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%s_%s" % (shape, mode), "--reads", str(reads), "--passes", str(passes)], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [json.loads(l[10:]) for l in r.stdout.splitlines() if l.startswith("SAC_CHILD ")]


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
    res = {"what": "tools/sac_time.py: k_sac beside k_ibc on the same batch, HIP-event times, median and range of the passes", "variants": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    for shape, mode in RUNS:
        if args.only and args.only != "%s_%s" % (shape, mode):
            continue
        for item in run_child(shape, mode, args.reads if shape == "short" else args.long_reads, args.passes):
            res["variants"][item["key"]] = item["result"]
            print(item["key"], json.dumps(item["result"]["kernels_ms"]["k_sac"]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    v = res["variants"]
    res["ratios"] = {}
    for shape in ("short", "long"):
        for name in SITE_COUNTS:
            base = v.get("%s_%s_index" % (shape, name))
            for mode in ("plain_search", "thread_path"):
                other = v.get("%s_%s_%s" % (shape, name, mode))
                if base and other:
                    assert base["count_sum"] == other["count_sum"], (shape, name, mode)  # (the same table by every path)
                    key = "%s_%s_%s_over_index" % (shape, name, mode)
                    res["ratios"][key] = other["kernels_ms"]["k_sac"]["median"] / base["kernels_ms"]["k_sac"]["median"]
                    print("%s: %.2f" % (key, res["ratios"][key]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
