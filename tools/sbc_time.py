"""Device time of the substitution tables (k_sbc; --substitutions) beside k_mbc on the same batch, on reads resident in HBM: the
config-2 shape (10 M x 150 bp over 4 x 25 M bases) and the long-read shape (50 K x 10 kb over 250 M bases), both at N = 1024, at the
thresholds Q / MQ = 0 / 0 and 20 / 30 — as the kernel is (one table X for the workgroup, a Y tile of 1024 cycles), with BQC_SBC_X=1
(one table X, a Y tile of 512 cycles) and with BQC_SBC_X=2 (a table X per wave, which leaves room for 512 cycles).  k_mbc is the yardstick: the same walk and loads, one table fewer on the hot bins.

usage: python tools/sbc_time.py [--reads N] [--long-reads N] [--passes P] [--only VARIANT] [--parent DIR] [--rounds R] [--out FILE]
Every variant runs in a process of its own (BQC_SBC_X is read once per process) under a time limit of its own, and nothing more is
started after one has failed.  Times come from bqc_set_timing / bqc_last_timing (HIP events around each launch), after three warm-up
passes, as the median and the range of P passes.  The floor is the bytes k_sbc must read — qualities, packed bases, one genome byte a
base, the CIGAR words and eleven fixed columns (k_mbc's ten and mapq) — at the card's measured copy rate, as DESIGN.md 4.2e computes
k_mbc's.
  --parent DIR: a checkout of the parent commit with its library built (DIR/bench.py, DIR/bamqc_amd/libbamqc_gpu.so).  The default
  path — every module off — is then measured as `bench.py --gpus 1 --steps 20 --warmup 3` in DIR and in this tree alternately,
  R rounds (left out: no comparison)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING = 6.29e12  # bytes/s, the card's measured copy rate
SHAPES = {"short": dict(seed=1002, lens=[25_000_000] * 4, read_len=150, long_reads=False, isize=1000, max_read_len=1024, hist_cap=4096),
          "long": dict(seed=1005, lens=[250_000_000], read_len=10_000, long_reads=True, isize=30_000, max_read_len=16_384, hist_cap=16_384)}
N = 1024
# variant: (shape, Q, MQ, BQC_SBC_X)
X_NAMES = ("one_x_c1024", "one_x_c512", "x_per_wave_c512")
VARIANTS = {"%s_q%d_mq%d_%s" % (shape, q, mq, X_NAMES[x]): (shape, q, mq, x)
            for shape in ("short", "long") for q, mq in ((0, 0), (20, 30)) for x in (0, 1, 2)}
COLUMN_BYTES = 2 + 1 + 4 + 2 + 4 + 4 + 4 + 4 + 4 + 1  # flag, lane, l_seq, n_cigar, rid, pos, the three payload offsets, mapq
CHILD_LIMIT = 600  # seconds a variant may take, its batch's making included


def child(variant, reads, passes):
    import numpy as np
    from bamqc_amd import Aggregator, synth
    shape, q, mq, x = VARIANTS[variant]
    S = SHAPES[shape]
    refs = [synth.reference(S["seed"], i, n) for i, n in enumerate(S["lens"])]
    cols = synth.batch(S["seed"], reads, S["lens"], refs, read_len=S["read_len"], isize=S["isize"], long_reads=S["long_reads"])
    a = Aggregator(n_refs=len(refs), isize=S["isize"], max_read_len=S["max_read_len"], hist_cap=S["hist_cap"], mismatch_by_cycle=N, substitutions=N,
                   subst_min_qual=q, subst_min_mapq=mq)
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
    L = cols["l_seq"].astype(np.int64)
    bases = int(L.sum())
    words = int(cols["n_cigar"].astype(np.int64).sum())
    y = sum(int(a.substitutions(0, m)[1].sum()) for m in range(2))
    xs = sum(int(a.substitutions(0, m)[0].sum()) for m in range(2))
    diag = sum(int(np.einsum("cii->", a.substitutions(0, m)[1])) for m in range(2))
    aligned = sum(int(a.mismatch_by_cycle(0, m)[0].sum()) for m in range(2))
    if q == 0 and mq == 0:
        assert y == aligned, (y, aligned)  # the identity with the `.mbc`: the same pairs
    floor_bytes = bases + (bases + 1) // 2 + bases + 4 * words + reads * COLUMN_BYTES
    out = {"variant": variant, "shape": shape, "reads": reads, "bases": bases, "cigar_words": words, "N": N, "Q": q, "MQ": mq, "BQC_SBC_X": x,
           "passes_counted": passes + 3, "Y_sum": y, "X_sum": xs, "matches_share_of_Y": diag / y if y else None, "mbc_aligned_sum": aligned,
           "floor_bytes": floor_bytes, "floor_ms": floor_bytes / COPY_CEILING * 1e3, "kernels_ms": {}}
    for k in ("k_sbc", "k_mbc"):
        v = np.array(kt[k])
        out["kernels_ms"][k] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "passes": [float(t) for t in v]}
    out["k_sbc_over_k_mbc"] = out["kernels_ms"]["k_sbc"]["median"] / out["kernels_ms"]["k_mbc"]["median"]
    out["k_sbc_over_floor"] = out["kernels_ms"]["k_sbc"]["median"] / out["floor_ms"]
    print("SBC_CHILD " + json.dumps(out), flush=True)


def run_child(variant, reads, passes):
    env = dict(os.environ)
    if VARIANTS[variant][3]:
        env["BQC_SBC_X"] = str(VARIANTS[variant][3])
    else:
        env.pop("BQC_SBC_X", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant, "--reads", str(reads), "--passes", str(passes)], env=env,
                       capture_output=True, text=True, timeout=CHILD_LIMIT)
    assert r.returncode == 0, "%s: exit status %d\n%s%s" % (variant, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("SBC_CHILD "))[10:])


def bench_once(tree):
    """One plain `bench.py --gpus 1 --steps 20 --warmup 3` in `tree` -> its JSON result line."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=tree, capture_output=True, text=True, timeout=CHILD_LIMIT)
    assert r.returncode == 0, "bench.py in %s: exit status %d\n%s%s" % (tree, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--long-reads", type=int, default=50_000)
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--only", default=None, help="variants whose name contains this")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reads, args.passes)
    res = {"what": "tools/sbc_time.py: k_sbc beside k_mbc on the same batch, HIP-event times, median and range of the passes", "variants": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    for variant, (shape, q, mq, x) in VARIANTS.items():
        if args.only and args.only not in variant:
            continue
        res["variants"][variant] = run_child(variant, args.reads if shape == "short" else args.long_reads, args.passes)  # (a failure ends the run here)
        print(variant, json.dumps(res["variants"][variant]["kernels_ms"]), flush=True)
        save()
    v = res["variants"]
    for name in list(v):  # the alternatives over the kernel as it is
        if not name.endswith(X_NAMES[0]):
            continue
        for alt in X_NAMES[1:]:
            twin = name[:-len(X_NAMES[0])] + alt
            if twin in v:
                key = "%s_over_%s_%s" % (alt, X_NAMES[0], name[:-len(X_NAMES[0]) - 1])
                res[key] = v[twin]["kernels_ms"]["k_sbc"]["median"] / v[name]["kernels_ms"]["k_sbc"]["median"]
                print("%s: %.3f" % (key, res[key]))
    if args.parent:
        ab = res.setdefault("bench_module_off", {"what": "bench.py --gpus 1 --steps 20 --warmup 3, the parent's tree and this one alternately", "parent": [], "this_tree": []})
        for _ in range(args.rounds):
            for key, tree in (("parent", os.path.abspath(args.parent)), ("this_tree", ROOT)):
                ab[key].append(bench_once(tree))
                print("bench", key, json.dumps(ab[key][-1]), flush=True)
                save()
    save()


if __name__ == "__main__":
    main()
