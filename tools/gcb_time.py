"""Device time of the GC bias (k_gcb_reads, k_gcb_genome; --gc-bias) beside k_qcyc on the same batch, and of the whole step with the
module on and off, on reads resident in HBM: the config-2 shape (10 M x 150 bp over 4 x 25 M bases) and the long-read shape
(50 K x 10 kb over 250 M bases), both at W = 100.  The module off is also measured with ANOTHER build of the library (the parent
commit's), in alternating rounds on one box, and so is bench.py --gpus 1 --steps 20 --warmup 3 (parent, this tree, parent, this tree).

usage: python tools/gcb_time.py [--reads N] [--rounds R] [--steps K] [--parent DIR] [--no-bench] [--no-shapes] [--bench-rounds B]
                                [--bench-key KEY] [--out FILE]
  --parent DIR: a checkout and build of the parent commit: DIR/bamqc_amd/libbamqc_gpu.so, DIR/bench.py (left out: no comparison)
  --no-shapes / --no-bench with an --out FILE that exists: the part left out is kept as an earlier call wrote it
Every variant runs in a process of its own — the parent's library with the module off, this tree's with it off (no
bqc_enable_gc_bias), this tree's with it on (qual_by_cycle with it: k_qcyc is the yardstick) — one after the other, in R rounds of
`blocks` blocks of K steps: what is compared has been measured the same way.  Kernel times come from bqc_last_timing: k_gcb_reads
behind a batch, k_gcb_genome behind a bqc_finalize (its genome: the shape's contigs)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING = 6.29e12  # bytes/s, the card's measured copy rate
W = 100
SHAPES = {"short": dict(seed=1002, lens=[25_000_000] * 4, read_len=150, long_reads=False, isize=1000, max_read_len=1024, hist_cap=4096),
          "long": dict(seed=1005, lens=[250_000_000], read_len=10_000, long_reads=True, isize=30_000, max_read_len=16_384, hist_cap=16_384)}
NEW_CALLS = ("bqc_enable_gc_bias", "bqc_gc_bias", "bqc_write_gc_bias")
COLUMN_BYTES = 2 + 1 + 4 + 4 + 4 + 2 + 4 + 4  # flag, lane, rid, pos, l_seq, n_cigar, qual_off, cigar_off


def child(shape, reads, steps, blocks, with_module):
    """One process, one library (BQC_LIB_PATH), the module on or off: `blocks` blocks of `steps` steps, each block timed with the host
    clock around steps that end in a synchronise; then the kernels' own times from the library's events."""
    import numpy as np
    from bamqc_amd import Aggregator, _lib, synth
    if not with_module:  # (the parent's library does not export the module's calls)
        for name in NEW_CALLS:
            _lib._SIGNATURES.pop(name, None)
    S = SHAPES[shape]
    refs = [synth.reference(S["seed"], i, n) for i, n in enumerate(S["lens"])]
    cols = synth.batch(S["seed"], reads, S["lens"], refs, read_len=S["read_len"], isize=S["isize"], long_reads=S["long_reads"])
    name = "on" if with_module else "off"
    a = Aggregator(n_refs=len(refs), isize=S["isize"], max_read_len=S["max_read_len"], hist_cap=S["hist_cap"], **({"qual_by_cycle": 1024, "gc_bias": W} if with_module else {}))
    for i, r in enumerate(refs):
        a.set_reference(i, r)
    db = a.upload(cols)
    for _ in range(3):  # warm-up: code objects, scratch tables
        a.process(db)
    a.sync()
    L = cols["l_seq"].astype(np.int64)
    rev = (cols["flag"].astype(np.int64) & 0x10) != 0
    out = {"reads": reads, "bases": int(L.sum()), "cigar_words_of_reverse_reads": int(cols["n_cigar"].astype(np.int64)[rev].sum()),
           "genome_bases": int(sum(S["lens"])), "step_ms": {name: []}, "kernels_ms": {}}
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(steps):
            a.process(db)
        a.sync()
        out["step_ms"][name].append((time.perf_counter() - t0) * 1e3 / steps)
    a.set_timing(True)  # per kernel, from the library's own events (a run of their own)
    kt = {}
    for _ in range(5):
        a.process(db)
        for k, v in a.last_timing().items():
            kt.setdefault(k, []).append(v)
    out["kernels_ms"][name] = {k: float(np.median(v)) for k, v in kt.items()}
    if with_module:  # the genome table: one launch per finalize; and what the module found, so that the time is that of tables with content
        gt = []
        for _ in range(5):
            a.finalize()
            gt.append(a.last_timing()["k_gcb_genome"])
        out["k_gcb_genome_ms"] = gt
        g, r, b, q = a.gc_bias(0)
        nz = np.flatnonzero(g)
        out["tables"] = {"genome_windows": int(g.sum()), "genome_bins_used": int(len(nz)), "bins_holding_90_percent": int(np.searchsorted(np.cumsum(np.sort(g)[::-1]), 0.9 * g.sum()) + 1),
                         "read_starts": int(r.sum()), "bases": int(b.sum()), "qual_sum": int(q.sum())}
    print("GCB_CHILD " + json.dumps(out), flush=True)


def run_child(lib, shape, reads, steps, blocks, with_module):
    env = dict(os.environ)
    if lib:
        env["BQC_LIB_PATH"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--reads", str(reads), "--steps", str(steps), "--blocks", str(blocks)] +
                       (["--with-module"] if with_module else []), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("GCB_CHILD "))[10:])


def run_bench(root):
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["value"]


def overlap(a, b):
    return min(a) <= max(b) and min(b) <= max(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--long-reads", type=int, default=50_000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--no-shapes", action="store_true")
    ap.add_argument("--bench-rounds", type=int, default=2)
    ap.add_argument("--bench-key", default="bench")  # (a second call of the comparison keeps the first one's numbers beside its own)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--with-module", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reads, args.steps, args.blocks, args.with_module)
    parent_lib = os.path.join(args.parent, "bamqc_amd", "libbamqc_gpu.so") if args.parent else None
    res = {"what": "tools/gcb_time.py: module on (with qual_by_cycle) / off, this tree against the parent commit's build, alternating rounds on one box", "shapes": {}}
    if args.out and os.path.exists(args.out) and (args.no_shapes or args.no_bench):  # (the part left out now is kept as an earlier call wrote it)
        with open(args.out) as f:
            res = json.load(f)
    if args.parent:
        args.parent = os.path.abspath(args.parent)

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
    for shape, reads in (() if args.no_shapes else (("short", args.reads), ("long", args.long_reads))):
        rows = {"on": [], "off": [], "parent": []}
        for rnd in range(args.rounds):  # parent, this off, this on, parent ...: `blocks` blocks of `steps` steps each
            if parent_lib:
                rows["parent"].append(run_child(parent_lib, shape, reads, args.steps, args.blocks, False))
            rows["off"].append(run_child(None, shape, reads, args.steps, args.blocks, False))
            rows["on"].append(run_child(None, shape, reads, args.steps, args.blocks, True))
        t = rows["on"]
        # k_gcb_reads' own traffic: the quality bytes, W genome bytes a read, eight fixed columns, the CIGARs of the reverse reads
        floor_bytes = t[0]["bases"] + reads * W + reads * COLUMN_BYTES + 4 * t[0]["cigar_words_of_reverse_reads"]
        s = {"reads": reads, "bases": t[0]["bases"], "window": W, "tables": t[0]["tables"],
             "k_gcb_reads_ms_by_round": [r["kernels_ms"]["on"]["k_gcb_reads"] for r in t], "k_gcb_reads_floor_bytes": floor_bytes,
             "k_gcb_reads_floor_ms": floor_bytes / COPY_CEILING * 1e3, "k_qcyc_ms_by_round": [r["kernels_ms"]["on"]["k_qcyc"] for r in t],
             "genome_bases": t[0]["genome_bases"], "k_gcb_genome_ms_by_round": [r["k_gcb_genome_ms"] for r in t],
             "k_gcb_genome_floor_ms": t[0]["genome_bases"] / COPY_CEILING * 1e3,
             "kernels_ms_on": t[-1]["kernels_ms"]["on"], "kernels_ms_off": rows["off"][-1]["kernels_ms"]["off"],
             "step_ms_on_by_round": [r["step_ms"]["on"] for r in t], "step_ms_off_by_round": [r["step_ms"]["off"] for r in rows["off"]]}
        if parent_lib:
            s["step_ms_parent_by_round"] = [r["step_ms"]["off"] for r in rows["parent"]]
            s["kernels_ms_parent"] = rows["parent"][-1]["kernels_ms"]["off"]
            off = [x for r in s["step_ms_off_by_round"] for x in r]
            par = [x for r in s["step_ms_parent_by_round"] for x in r]
            s["gate_off_inside_parent_spread"] = {"off_range_ms": [min(off), max(off)], "parent_range_ms": [min(par), max(par)],
                                                  "inside": min(par) <= min(off) and max(off) <= max(par), "overlaps": overlap(off, par),
                                                  "off_beyond_parent_ms": max(0.0, max(off) - max(par))}
        res["shapes"][shape] = s
        print(shape, json.dumps(s), flush=True)
        save()
    if not args.no_bench:
        b = {"command": "bench.py --gpus 1 --steps 20 --warmup 3", "unit": "reads/s", "order": "parent, this, parent, this, ..."}
        b["this"], b["parent"] = [], []
        for rnd in range(args.bench_rounds):
            if args.parent:
                b["parent"].append(run_bench(args.parent))
            b["this"].append(run_bench(ROOT))
        if args.parent:
            b["parent_from_parent"] = max(b["parent"]) - min(b["parent"])
            b["this_below_lowest_parent"] = max(0.0, min(b["parent"]) - min(b["this"]))
            b["holds"] = min(b["this"]) >= min(b["parent"]) or b["this_below_lowest_parent"] <= b["parent_from_parent"]
        else:
            del b["parent"]
        res[args.bench_key] = b
        print("bench", json.dumps(b), flush=True)
    save()


if __name__ == "__main__":
    main()
