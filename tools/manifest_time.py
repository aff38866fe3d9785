"""Many files through one resident worker (`bamqualcheck --manifest`), timed against the same files as single runs back to back.
Writes (and extends) profiles/manifest_ab.json.

usage: python tools/manifest_time.py --round K [--files 10] [--reads 10000000] [--with-c] [--parent DIR] [--bench-pairs N] [--out FILE]
  One call is ONE round: (a) N single runs of the program back to back, as bench.py's e2e.back_to_back runs them, then (b) one
  `--manifest` run over the same N files; wall time per file, every job's `[timing]` lines.  Call it three times (--round 1, 2, 3): the
  rounds alternate (a) and (b) on one box.
  --with-c: once, (c) the list of (b) with a file over a second FASTA / contig set in the middle: what changing the genome costs.
  --parent DIR: a built checkout of the parent commit (DIR/bin/bamqualcheck, DIR/bench.py): its program on the same inputs, once — the
      single runs' outputs must be its bytes — and, with --bench-pairs N, N alternating pairs of plain `bench.py` and of
      `bench.py --full`'s e2e leg, parent against this tree.
The file is the 10 M-read file bench.py writes for its e2e leg (the same plan and seed).  Every program run has a time limit of its
own; the first run that does not end with status 0 ends the script."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bamqc_amd import hostio  # noqa: E402

NAMES, LENS = ["chr1", "chr2", "chr3", "chr4"], [25_000_000] * 4
NAMES2, LENS2 = ["chr5", "chr6"], [30_000_000, 20_000_000]
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
CHROMS = ",".join(NAMES + NAMES2)


def checked(cmd, limit, env=None, cwd=None):
    """A run under its own time limit: (wall seconds, stdout, stderr); anything but status 0 ends the script."""
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})), cwd=cwd)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        print(r.stderr[-3000:])
        sys.exit("a run ended with status %d: nothing more is started" % r.returncode)
    return dt, r.stdout, r.stderr


def timing_lines(err):
    return [ln for ln in err.splitlines() if ln.startswith("[timing]")]


def phases(err):
    """Every `[timing] phases:` line of a run as {phase: seconds}."""
    out = []
    for ln in err.splitlines():
        if ln.startswith("[timing] phases:"):
            out.append({k.strip(): float(v) for k, v in re.findall(r"(FASTA|context|references|record loop|finalize|write|destroy) ([\d.]+) s", ln)})
    return out


def single_runs(exe, bam, fa, tmp, n, tag):
    """(a): every front end starts the moment the one before has left."""
    walls, errs = [], []
    time.sleep(1.0)
    t0 = time.perf_counter()
    for k in range(n):
        dt, _, err = checked([exe, "-r", fa, "-o", os.path.join(tmp, "%s%d.bamqc" % (tag, k)), "-c", CHROMS, bam], 120, {"BQC_TIMING": "1"})
        walls.append(dt)
        errs.append(err)
    total = time.perf_counter() - t0
    return dict(files=n, wall_s=total, s_per_file=total / n, each_s=walls, phases=[p for e in errs for p in phases(e)], timing_lines_last=timing_lines(errs[-1]))


def manifest_run(jobs, tmp, tag):
    """(b) / (c): one process, the list of jobs [(bam, out)]; the genome is per directory."""
    lst = os.path.join(tmp, tag + ".tsv")
    with open(lst, "w") as f:
        f.write("".join("%s\t%s\n" % j for j in jobs))
    time.sleep(1.0)
    dt, _, err = checked([EXE, "-r", "{dir}/genome.fa", "-c", CHROMS, "--manifest", lst], 300, {"BQC_TIMING": "1"})
    return dict(files=len(jobs), wall_s=dt, s_per_file=dt / len(jobs), phases=phases(err), job_lines=[ln for ln in timing_lines(err) if " job " in ln],
                session_line=[ln for ln in timing_lines(err) if "session after" in ln], timing_lines=timing_lines(err))


def bench_once(tree, full):
    extra = ["--full", "--no-cpu", "--no-extra", "--no-large"] if full else []
    _, out, _ = checked([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"] + extra, 500, cwd=tree)
    line = json.loads(out.strip().splitlines()[-1])
    return dict(value=line.get("value"), e2e_wall_s=(line.get("e2e") or {}).get("wall_s"), e2e_back_to_back_s_per_file=((line.get("e2e") or {}).get("back_to_back") or {}).get("s_per_file"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--round", type=int, required=True)
    ap.add_argument("--files", type=int, default=10)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--with-c", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--bench-pairs", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "manifest_ab.json"))
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else dict(reads_per_file=a.reads, read_length=150, files=a.files, rounds=[])
    with tempfile.TemporaryDirectory(prefix="bqc_manifest_") as tmp:
        g1, g2 = os.path.join(tmp, "g1"), os.path.join(tmp, "g2")
        os.makedirs(g1), os.makedirs(g2)
        bam, fa = os.path.join(g1, "c2.bam"), os.path.join(g1, "genome.fa")
        t0 = time.perf_counter()
        hostio.synth_stream(bam, fa, 1002, a.reads, NAMES, LENS, level=1)
        res["file_bytes"] = os.path.getsize(bam)
        print("file: %d reads, %.0f MB, written in %.1f s" % (a.reads, res["file_bytes"] / 1e6, time.perf_counter() - t0), flush=True)
        rnd = dict(round=a.round)
        rnd["a_single_runs"] = single_runs(EXE, bam, fa, tmp, a.files, "a")
        print("(a) %d single runs back to back: %.3f s per file" % (a.files, rnd["a_single_runs"]["s_per_file"]), flush=True)
        rnd["b_manifest"] = manifest_run([(bam, os.path.join(tmp, "b%d.bamqc" % k)) for k in range(a.files)], tmp, "b")
        print("(b) one --manifest run of %d jobs: %.3f s per file" % (a.files, rnd["b_manifest"]["s_per_file"]), flush=True)
        print("\n".join(rnd["b_manifest"]["job_lines"] + rnd["b_manifest"]["session_line"]), flush=True)
        want = open(os.path.join(tmp, "a0.bamqc"), "rb").read()
        same = all(open(os.path.join(tmp, "%s%d.bamqc" % (t, k)), "rb").read() == want for t in "ab" for k in range(a.files))
        assert same, "outputs differ"
        rnd["outputs_identical"] = True
        if a.with_c:
            bam2, fa2 = os.path.join(g2, "other.bam"), os.path.join(g2, "genome.fa")
            hostio.synth_stream(bam2, fa2, 1004, a.reads, NAMES2, LENS2, level=1)
            _ = checked([EXE, "-r", fa2, "-o", os.path.join(tmp, "c_single.bamqc"), "-c", CHROMS, bam2], 120)
            half = a.files // 2
            jobs = [(bam, os.path.join(tmp, "c%d.bamqc" % k)) for k in range(half)] + [(bam2, os.path.join(tmp, "c_other.bamqc"))] + \
                   [(bam, os.path.join(tmp, "c%d.bamqc" % k)) for k in range(half, a.files)]
            c = manifest_run(jobs, tmp, "c")
            assert open(os.path.join(tmp, "c_other.bamqc"), "rb").read() == open(os.path.join(tmp, "c_single.bamqc"), "rb").read(), "outputs differ"
            assert all(open(os.path.join(tmp, "c%d.bamqc" % k), "rb").read() == want for k in range(a.files)), "outputs differ"
            c["what"] = "the list of (b) with one file over a second FASTA and contig set in the middle (%d jobs); s_per_file_beyond_b: its wall time less (b)'s, " \
                        "i.e. the file itself, the two changes of genome and the contexts that go with them" % len(jobs)
            c["s_beyond_b"] = c["wall_s"] - rnd["b_manifest"]["wall_s"]
            res["c_second_genome_in_the_middle"] = c
            print("(c) %d jobs, a second genome in the middle: %.3f s (%.3f s more than (b))" % (len(jobs), c["wall_s"], c["s_beyond_b"]), flush=True)
            print("\n".join(c["job_lines"]), flush=True)
        if a.parent:
            old = os.path.join(a.parent, "bin", "bamqualcheck")
            checked([old, "-r", fa, "-o", os.path.join(tmp, "parent.bamqc"), "-c", CHROMS, bam], 120)
            assert open(os.path.join(tmp, "parent.bamqc"), "rb").read() == want, "this tree's single run differs from the parent's"
            res["single_run_output_equals_parent"] = True
        res["rounds"] = [r for r in res["rounds"] if r["round"] != a.round] + [rnd]
    if a.parent and a.bench_pairs:
        res["bench"] = dict(plain=[], full_e2e=[])
        for full in (False, True):
            for _ in range(a.bench_pairs):
                for who, tree in (("parent", a.parent), ("new", ROOT)):
                    row = dict(build=who, **bench_once(tree, full))
                    res["bench"]["full_e2e" if full else "plain"].append(row)
                    print("bench %s %s: %s" % ("--full" if full else "plain", who, row), flush=True)
                    json.dump(res, open(a.out, "w"), indent=1)
    rs = sorted(res["rounds"], key=lambda r: r["round"])
    res["rounds"] = rs
    av, bv = [r["a_single_runs"]["s_per_file"] for r in rs], [r["b_manifest"]["s_per_file"] for r in rs]
    res["summary"] = dict(a_s_per_file=av, b_s_per_file=bv, slowest_b_beats_fastest_a=max(bv) < min(av), rounds=len(rs))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out, res["summary"])


main()
