"""Device time of the mismatches by cycle and base quality (k_mbc, --mismatch-by-cycle) beside k_qcyc on the same batch, and of the
whole step with the module on and off, on reads resident in HBM: the config-2 shape (10 M x 150 bp) and the long-read shape (50 K x 10 kb).  The module off is also
measured with ANOTHER build of the library (the parent commit's), in alternating rounds on one box, and so is the program's wall
time on the 10 M-read file without the option.

usage: python tools/mbc_time.py [--reads N] [--rounds R] [--steps K] [--parent DIR] [--no-program] [--no-shapes] [--out FILE]
  --parent DIR: a build of the parent commit, DIR/bamqc_amd/libbamqc_gpu.so and DIR/bin/bamqualcheck (left out: no comparison)
Every measurement runs in a process of its own — the parent's library with the module off, this tree's with it off, this tree's with
it on (and qual_by_cycle with it: k_qcyc is the yardstick) — one after the other, round after round: what is compared has been measured the same way."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING = 6.29e12  # bytes/s, the card's measured copy rate
SHAPES = {"short": dict(seed=1002, lens=[25_000_000] * 4, read_len=150, long_reads=False, isize=1000, max_read_len=1024, hist_cap=4096),
          "long": dict(seed=1005, lens=[250_000_000], read_len=10_000, long_reads=True, isize=30_000, max_read_len=16_384, hist_cap=16_384)}


def child(shape, reads, steps, blocks, with_module):
    """One process, one library (BQC_LIB_PATH), the module on or off: `blocks` blocks of `steps` steps, each block timed with the host
    clock around steps that end in a synchronise; then the kernels' own times from the library's events."""
    import numpy as np
    from bamqc_amd import Aggregator, _abi, _lib, synth
    if not with_module:  # (the parent's library does not export the module's two calls, and takes the structure without its field)
        for name in ("bqc_mismatch_by_cycle", "bqc_write_mismatch_by_cycle"):
            _lib._SIGNATURES.pop(name, None)
    S = SHAPES[shape]
    refs = [synth.reference(S["seed"], i, n) for i, n in enumerate(S["lens"])]
    cols = synth.batch(S["seed"], reads, S["lens"], refs, read_len=S["read_len"], isize=S["isize"], long_reads=S["long_reads"])
    variants = {"on": 1024} if with_module else {"off": 0}
    ctx = {}
    for name, N in variants.items():
        a = Aggregator(n_refs=len(refs), isize=S["isize"], max_read_len=S["max_read_len"], hist_cap=S["hist_cap"], **({"qual_by_cycle": N, "mismatch_by_cycle": N} if N else {"struct_size": _abi.Options.mismatch_by_cycle.offset}))
        for i, r in enumerate(refs):
            a.set_reference(i, r)
        db = a.upload(cols)
        for _ in range(3):  # warm-up: code objects, scratch tables
            a.process(db)
        a.sync()
        ctx[name] = (a, db)
    out = {"reads": reads, "qual_bytes": int(cols["l_seq"].astype(np.int64).sum()), "cigar_words": int(cols["n_cigar"].astype(np.int64).sum()), "step_ms": {k: [] for k in ctx}, "kernels_ms": {}}
    for _ in range(blocks):
        for name, (a, db) in ctx.items():
            t0 = time.perf_counter()
            for _ in range(steps):
                a.process(db)
            a.sync()
            out["step_ms"][name].append((time.perf_counter() - t0) * 1e3 / steps)
    for name, (a, db) in ctx.items():  # per kernel, from the library's own events (a run of their own: the events serialise nothing, but keep the two apart)
        a.set_timing(True)
        kt = {}
        for _ in range(5):
            a.process(db)
            for k, v in a.last_timing().items():
                kt.setdefault(k, []).append(v)
        out["kernels_ms"][name] = {k: float(np.median(v)) for k, v in kt.items()}
    print("MBC_CHILD " + json.dumps(out), flush=True)


def run_child(lib, shape, reads, steps, blocks, with_module):
    env = dict(os.environ)
    if lib:
        env["BQC_LIB_PATH"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--reads", str(reads), "--steps", str(steps), "--rounds", str(blocks)] +
                       (["--with-module"] if with_module else []), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith("MBC_CHILD "))[10:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--long-reads", type=int, default=50_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--no-program", action="store_true")
    ap.add_argument("--no-shapes", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--with-module", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reads, args.steps, args.rounds, args.with_module)
    parent_lib = os.path.join(args.parent, "bamqc_amd", "libbamqc_gpu.so") if args.parent else None
    res = {"what": "tools/mbc_time.py: module on (with qual_by_cycle) / off, this tree against the parent commit's build, alternating rounds on one box", "shapes": {}}
    for shape, reads in (() if args.no_shapes else (("short", args.reads), ("long", args.long_reads))):
        rows = {"on": [], "off": [], "parent": []}
        for rnd in range(args.rounds):  # parent, this off, this on, parent ...: 4 blocks of `steps` steps each
            if parent_lib:
                rows["parent"].append(run_child(parent_lib, shape, reads, args.steps, 4, False))
            rows["off"].append(run_child(None, shape, reads, args.steps, 4, False))
            rows["on"].append(run_child(None, shape, reads, args.steps, 4, True))
        t = rows["on"]
        qual_bytes = t[0]["qual_bytes"]
        # k_mbc's own traffic: qualities, packed bases (a nibble each), genome bytes (one per compared base, taken as one per base),
        # CIGAR words, and ten fixed columns: flag 2, lane 1, l_seq 4, n_cigar 2, rid 4, pos 4, qual_off 4, seq_off 4, cigar_off 4
        floor_bytes = qual_bytes + qual_bytes // 2 + qual_bytes + 4 * t[0]["cigar_words"] + reads * (2 + 1 + 4 + 2 + 4 + 4 + 4 + 4 + 4)
        s = {"reads": reads, "qual_bytes": qual_bytes, "cigar_words": t[0]["cigar_words"],
             "k_mbc_ms_by_round": [r["kernels_ms"]["on"]["k_mbc"] for r in t], "k_mbc_floor_ms": floor_bytes / COPY_CEILING * 1e3,
             "k_qcyc_ms_by_round": [r["kernels_ms"]["on"]["k_qcyc"] for r in t],
             "kernels_ms_on": t[-1]["kernels_ms"]["on"], "kernels_ms_off": rows["off"][-1]["kernels_ms"]["off"],
             "step_ms_on_by_round": [r["step_ms"]["on"] for r in t], "step_ms_off_by_round": [r["step_ms"]["off"] for r in rows["off"]]}
        if parent_lib:
            s["step_ms_parent_by_round"] = [r["step_ms"]["off"] for r in rows["parent"]]
            s["kernels_ms_parent"] = rows["parent"][-1]["kernels_ms"]["off"]
        res["shapes"][shape] = s
        print(shape, json.dumps(s), flush=True)
    if not args.no_program:
        from bamqc_amd import hostio
        tmp = tempfile.mkdtemp(prefix="bqc_mbc_")
        names, lens = ["chr1", "chr2", "chr3", "chr4"], [25_000_000] * 4
        bam, fa = os.path.join(tmp, "c2.bam"), os.path.join(tmp, "c2.fa")
        hostio.synth_stream(bam, fa, 1002, args.reads, names, lens, read_len=150, level=1)
        exes = {"this": (os.path.join(ROOT, "bin", "bamqualcheck"), []), "this --mismatch-by-cycle": (os.path.join(ROOT, "bin", "bamqualcheck"), ["--mismatch-by-cycle"])}
        if args.parent:
            exes["parent"] = (os.path.join(args.parent, "bin", "bamqualcheck"), [])
        wall = {k: [] for k in exes}
        for rnd in range(args.rounds + 1):  # (round 0: the file into the page cache, every program once; not recorded)
            for name, (exe, extra) in exes.items():
                t0 = time.perf_counter()
                r = subprocess.run([exe, "-r", fa, "-o", os.path.join(tmp, "o.bamqc"), "-c", ",".join(names)] + extra + [bam], capture_output=True, text=True, timeout=600)
                assert r.returncode == 0, r.stderr[-2000:]
                if rnd:
                    wall[name].append(round(time.perf_counter() - t0, 3))
        res["program_wall_s"] = {"reads": args.reads, "by_round": wall}
        print("program", json.dumps(res["program_wall_s"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
