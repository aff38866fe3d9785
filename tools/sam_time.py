"""`bamqualcheck -` on a SAM stream: this tree's program against another build of it (the parent commit's), alternating; where the record
loop's time goes; and the stream size from which the reader on the card is not slower than the host's.  Writes profiles/sam_reader_ab.json.

usage: python tools/sam_time.py --parent DIR [--reads 4000000] [--out profiles/sam_reader_ab.json] [--no-kernel-stats] [--no-bench] [--only-kernel-stats]
  DIR: a built checkout of the program to compare with (DIR/bin/bamqualcheck, DIR/bench.py).
Also: the reader's kernels per million reads from one `rocprofv3 --kernel-trace --stats` run of its own (the first million reads of the
stream, the card forced), and one alternating pair of plain bench.py runs of the two builds.
The stream is written here with bqc_sam_write from a seeded synthetic batch and fed from the page cache through a pipe (cat).  Every run
has a time limit of its own; the first run that does not end with status 0 ends the script."""
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


def generate(tmp, reads):
    import numpy as np
    bam, fa, sam = (os.path.join(tmp, x) for x in ("s.bam", "s.fa", "s.sam"))
    hostio.synth_stream(bam, fa, 1002, reads, NAMES, LENS, level=1)
    f = hostio.BamFile(bam)
    got = list(f.batches(1 << 20, 1 << 40))
    f.close()
    cols = {k: np.concatenate([b[k] for b in got]) for k in got[0]}
    hostio.write_sam(sam, cols, NAMES, LENS)
    os.remove(bam)
    return sam, fa


def run(exe, sam, fa, out, env, limit=300):
    """One run of `cat sam | exe ... -`: (wall seconds, stderr)."""
    t0 = time.perf_counter()
    cat = subprocess.Popen(["cat", sam], stdout=subprocess.PIPE)
    r = subprocess.run(["timeout", "-k", "10", str(limit), exe, "-r", fa, "-o", out, "-c", ",".join(NAMES), "-"], stdin=cat.stdout, capture_output=True, text=True,
                       env=dict(os.environ, BQC_TIMING="1", **env))
    cat.stdout.close()
    cat.wait()
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        print(r.stderr[-3000:])
        sys.exit("a run ended with status %d: nothing more is started" % r.returncode)
    return dt, r.stderr


def kernel_stats(exe, sam, fa, tmp, reads):
    """One run under rocprofv3 (kernel trace only): {kernel: microseconds per million reads} of the reader's kernels, and of all kernels."""
    import csv
    import glob
    d = os.path.join(tmp, "kt")
    cat = subprocess.Popen(["cat", sam], stdout=subprocess.PIPE)
    r = subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", exe, "-r", fa, "-o", os.path.join(tmp, "kt.bamqc"),
                        "-c", ",".join(NAMES), "-"], stdin=cat.stdout, capture_output=True, text=True, env=dict(os.environ, BQC_GPU_DECODE="1", BQC_NO_FORK="1", BQC_FAST_EXIT="0"))  # (one process that ends the usual way: the profiler writes when it does)
    cat.stdout.close()
    cat.wait()
    if r.returncode != 0:
        print(r.stderr[-3000:])
        sys.exit("the run under rocprofv3 ended with status %d: nothing more is started" % r.returncode)
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            out[row["Name"].split("(")[0]] = dict(calls=int(row["Calls"]), us_per_million_reads=float(row["TotalDurationNs"]) / 1e3 / (reads / 1e6))
    return out


def bench_once(tree):
    r = subprocess.run(["timeout", "-k", "10", "200", sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree, capture_output=True, text=True)
    if r.returncode != 0:
        print(r.stderr[-3000:])
        sys.exit("bench.py ended with status %d: nothing more is started" % r.returncode)
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_reader_ab.json"))
    ap.add_argument("--no-kernel-stats", action="store_true")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--only-kernel-stats", action="store_true", help="add the kernel trace to an existing result file")
    a = ap.parse_args()
    new_exe, old_exe = os.path.join(ROOT, "bin", "bamqualcheck"), os.path.join(a.parent, "bin", "bamqualcheck")
    res = dict(reads=a.reads, read_length=150)
    if a.only_kernel_stats:
        res = json.load(open(a.out))
        a.reads, a.no_bench = 1_100_000, True
    with tempfile.TemporaryDirectory(prefix="bqc_sam_") as tmp:
        t0 = time.perf_counter()
        sam, fa = generate(tmp, a.reads)
        if not a.only_kernel_stats:
            res["text_bytes"] = os.path.getsize(sam)
        print("stream: %d reads, %.0f MB of text, generated in %.1f s" % (a.reads, res["text_bytes"] / 1e6, time.perf_counter() - t0), flush=True)
        subprocess.run(["cat", sam], stdout=subprocess.DEVNULL)  # (into the page cache)
        text = open(sam, "rb")
        part = os.path.join(tmp, "head.sam")
        # program time: three alternating pairs
        walls = dict(parent=[], new=[])
        last_err = ""
        for rep in range(0 if a.only_kernel_stats else 3):
            for who, exe in (("parent", old_exe), ("new", new_exe)):
                dt, err = run(exe, sam, fa, os.path.join(tmp, who + ".bamqc"), {})
                walls[who].append(dt)
                print("%s run %d: %.3f s = %.2f M reads/s" % (who, rep, dt, a.reads / dt / 1e6), flush=True)
                if who == "new":
                    last_err = err
        if not a.only_kernel_stats:
            assert open(os.path.join(tmp, "parent.bamqc"), "rb").read() == open(os.path.join(tmp, "new.bamqc"), "rb").read(), "outputs differ"
            res["program_seconds"] = walls
            res["outputs_identical"] = True
            res["parent_spread_seconds"] = max(walls["parent"]) - min(walls["parent"])
            res["factor_best_of_three"] = min(walls["parent"]) / min(walls["new"])
            res["new_beats_parent_by_more_than_its_spread"] = min(walls["parent"]) - max(walls["new"]) > res["parent_spread_seconds"]
            # where the time goes (the last run of this tree's program)
            lines = [ln for ln in last_err.splitlines() if ln.startswith(("[sam reader]", "[timing]"))]
            res["timing_lines"] = lines
            m = re.search(r"(\d+) records: decode thread busy ([\d.]+) s, .* loop ([\d.]+) s", last_err)
            if m:
                res["record_loop"] = dict(records=int(m.group(1)), decode_thread_busy_s=float(m.group(2)), loop_s=float(m.group(3)), reads_per_s=int(m.group(1)) / max(float(m.group(3)), 1e-9))
            m = re.search(r"read\(\) ([\d.]+) s in the reader thread; the decode thread waited ([\d.]+) s for input, copied text for ([\d.]+) s, ran kernels for ([\d.]+) s", last_err)
            if m:
                res["reader_seconds"] = dict(read=float(m.group(1)), waiting_for_input=float(m.group(2)), copying_text=float(m.group(3)), kernels_and_batch_tail=float(m.group(4)))
            print("\n".join(lines), flush=True)
            # the crossing point: parent against the card, forced, on the head of the stream
            cross = []
            for mb in (1, 4, 16, 64):
                text.seek(0)
                head = text.read(mb << 20)
                head = head[:head.rfind(b"\n") + 1]
                open(part, "wb").write(head)
                row = dict(text_mb=mb, parent=[], card=[])
                for rep in range(3):
                    row["parent"].append(run(old_exe, part, fa, os.path.join(tmp, "hp.bamqc"), {}, 120)[0])
                    row["card"].append(run(new_exe, part, fa, os.path.join(tmp, "hc.bamqc"), {"BQC_GPU_DECODE": "1"}, 120)[0])
                assert open(os.path.join(tmp, "hp.bamqc"), "rb").read() == open(os.path.join(tmp, "hc.bamqc"), "rb").read(), "outputs differ at %d MB" % mb
                print("%3d MB: parent %s, card %s" % (mb, ["%.3f" % x for x in row["parent"]], ["%.3f" % x for x in row["card"]]), flush=True)
                cross.append(row)
            res["crossing"] = cross
            t_mb = None  # the smallest size from which (and above which) the card is not slower
            for r in reversed(cross):
                if min(r["card"]) > min(r["parent"]):
                    break
                t_mb = r["text_mb"]
            res["card_not_slower_from_mb"] = t_mb
        if not a.no_kernel_stats:  # the first million reads, a run of its own
            text.seek(0)
            head = text.read(370 << 20)
            head = head[:head.rfind(b"\n") + 1]
            open(part, "wb").write(head)
            n_head = head.count(b"\n") - head.count(b"\n@")
            ks = kernel_stats(new_exe, part, fa, tmp, n_head)
            res["kernel_trace"] = dict(reads=n_head, text_bytes=len(head), kernels=ks,
                                       sam_reader_us_per_million_reads=sum(v["us_per_million_reads"] for k, v in ks.items() if k.startswith("k_gs_")))
            print("kernels of the SAM reader: %s" % {k: round(v["us_per_million_reads"], 1) for k, v in ks.items() if k.startswith("k_gs_")}, flush=True)
    if not a.no_bench:  # parent, new, parent, new
        runs = [(who, bench_once(tree)) for who, tree in (("parent", a.parent), ("new", ROOT)) * 2]
        res["bench"] = [dict(build=who, line=line) for who, line in runs]
        for who, line in runs:
            print("bench %s: %s" % (who, json.dumps(line)[:300]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


main()
