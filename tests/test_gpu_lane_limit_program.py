"""GPU: the program on files whose header has 256 `@RG` lines — the readers' table of read-group ids on the host and on the card (BAM and
SAM text), the `--gpus N` wire with a LaneWire per read group, and the writers with 256 lane blocks — and on a header with 257.

Every run has --no-sketch: the program's k-mer sketch has a table of 4 227 073 words per read group at the default error rate, 8.7 GB
for 256 read groups on the card and again in the oracle; the sketch at the limit is tests/test_gpu_lane_limit.py's, at a smaller table.
--batch-reads 4000 keeps a batch's window changes (a read group's reads lie thousands of bases apart: nearly every read is one) below
what the card's anchor chain takes per batch."""
import os
import re
import subprocess

import numpy as np
import pytest

from bamqc_amd import hostio
from tests import bamqc_text, dup_ref, ibc_ref, pybam, qbc_ref, rcv_ref, synth
from tests.cli_oracle import oracle_bamqualcheck

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")
NAMES, LENS = ["chr1", "chr2"], [300_000, 100_000]
N_LANES = 256
COMMON = ["-c", "chr1,chr2", "--no-sketch", "--batch-reads", "4000"]
QBC_LEN = 160       # (the default of 1024 cycles is 117 M words for 256 read groups, in the restatement as well)
DUP_CAPACITY = 100_000


def run(args, env=None, **kw):
    return subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, **(env or {})), timeout=300, **kw)


def same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """About 20 000 synthetic paired reads of 256 read groups on two contigs, the file as SAM text, the oracle's `.bamqc`, a BED file and
    the texts the restatements make of the file's columns."""
    d = tmp_path_factory.mktemp("rg256")
    bam, fa = str(d / "in.bam"), str(d / "in.fa")
    hostio.synth_write(bam, fa, seed=61, n_reads=20_000, ref_names=NAMES, ref_lens=LENS, n_lanes=N_LANES)
    cols, refs, lanes, sample = pybam.columns(bam)
    assert len(lanes) == N_LANES and [nm for nm, _ in refs] == NAMES
    count = np.bincount(cols["lane"], minlength=N_LANES)
    assert count.min() > 0 and 19_000 <= len(cols["flag"]) <= 21_000
    want = str(d / "oracle.bamqc")
    assert oracle_bamqualcheck(bam, fa, want, chroms="chr1,chr2", klist=(), qlist=(), batch_reads=4000) == 0
    assert len(re.findall(r"^lane ", open(want).read(), re.M)) == N_LANES
    bed = str(d / "panel.bed")
    rng = np.random.default_rng(62)
    with open(bed, "w") as f:
        for k, name in enumerate(NAMES):
            for p in np.sort(rng.choice(LENS[k] // 500, 60, replace=False)) * 500:
                f.write("%s\t%d\t%d\n" % (name, p, p + int(rng.integers(1, 400))))
    names = sorted(lanes)  # the program lists the lanes by name
    idx = [lanes[nm] for nm in names]
    return dict(dir=d, bam=bam, fa=fa, want=want, bed=bed, cols=cols, sample=sample, names=names, idx=idx, sam=pybam.bam_to_sam_text(bam).encode())


@pytest.fixture(scope="module")
def module_texts(files):
    """The `.qbc`, `.ibc`, `.rcv` and `.dup` of the file by the restatements, from pybam's columns."""
    cols, sample, names, idx = files["cols"], files["sample"], files["names"], files["idx"]
    parsed = bamqc_text.parse(files["want"])
    cycles = np.zeros((N_LANES, 2), np.int64)
    for nm, l in zip(names, idx):
        cycles[l] = [len(parsed[nm]["As_by_position_first"]), len(parsed[nm]["As_by_position_second"])]
    rid, start, end, given, unnamed, merged = hostio.load_regions(files["bed"], NAMES, LENS)
    assert given == 120 and unnamed == 0
    prod = rcv_ref.products_fast(rcv_ref.state_fast(cols, (rid, start, end), N_LANES, 2, 20), (rid, start, end), 2)
    assert sum(p["reads_on_target"] for p in prod) > 1000 and prod[63]["reads_examined"] > 0 and prod[64]["reads_examined"] > 0
    return {"qbc": qbc_ref.text(qbc_ref.table_fast(cols, N_LANES, QBC_LEN), cycles, sample, names, idx),
            "ibc": ibc_ref.text(ibc_ref.table_fast(cols, N_LANES, 1024), sample, names, idx),
            "rcv": rcv_ref.text(prod, (rid, start, end), NAMES, 20, rcv_ref.DEFAULT_THRESHOLDS, sample, names, idx),
            "dup": dup_ref.text(dup_ref.view_fast(cols, N_LANES, 2, DUP_CAPACITY), sample, names, idx)}


def anchored_batches(stderr):
    m = re.findall(r"\[timing\] (\d+) batches anchored on the card \(fixed columns never on the host\) of (\d+) batches", stderr)
    assert m, stderr
    return [(int(a), int(b)) for a, b in m]


@pytest.mark.parametrize("decode", ["0", "1"])
def test_bam_with_256_read_groups_is_the_oracles_bytes(files, decode):
    out = str(files["dir"] / ("plain%s.bamqc" % decode))
    r = run(["-r", files["fa"], "-o", out] + COMMON + [files["bam"]], env=dict(BQC_GPU_DECODE=decode, BQC_TIMING="1"))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["want"])
    if decode == "1":  # the reader on the card: every batch anchored there, none through the host decoder
        [(k, total)] = anchored_batches(r.stderr.decode())
        assert total >= 5 and k == total, r.stderr
        assert b"went through the host decoder" not in r.stderr


def test_sam_text_on_stdin_with_256_read_groups(files):
    out = str(files["dir"] / "sam.bamqc")
    r = run(["-r", files["fa"], "-o", out] + COMMON + ["-"], input=files["sam"])
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["want"])


def test_modules_with_256_read_groups_both_decoders(files, module_texts):
    mods = ["--qual-by-cycle-len", str(QBC_LEN), "--indel-by-cycle", "--regions", files["bed"], "--duplicate-sets", "--duplicate-sets-capacity", str(DUP_CAPACITY)]
    outs = {}
    for decode in ("0", "1"):
        outs[decode] = str(files["dir"] / ("mods%s.bamqc" % decode))
        r = run(["-r", files["fa"], "-o", outs[decode]] + mods + COMMON + [files["bam"]], env=dict(BQC_GPU_DECODE=decode))
        assert r.returncode == 0, r.stderr
        assert same_bytes(outs[decode], files["want"])
    for ext, text in module_texts.items():
        assert same_bytes(outs["0"] + "." + ext, outs["1"] + "." + ext), ext
        got = open(outs["1"] + "." + ext).read()
        if got != text:
            gl, wl = got.split("\n"), text.split("\n")
            k = next((i for i, (a, b) in enumerate(zip(gl, wl)) if a != b), min(len(gl), len(wl)))
            raise AssertionError(".%s: line %d of %d / %d differs: %r != %r" % (ext, k + 1, len(gl), len(wl), gl[k][:200] if k < len(gl) else None, wl[k][:200] if k < len(wl) else None))


def test_two_workers_on_one_card_with_256_read_groups(files):
    out = str(files["dir"] / "gpus2.bamqc")
    r = run(["--gpus", "2", "-r", files["fa"], "-o", out] + COMMON + [files["bam"]], env=dict(BQC_GPUS_SHARE_DEVICE="1"))
    assert r.returncode == 0, r.stderr
    assert same_bytes(out, files["want"])


@pytest.fixture(scope="module")
def files257(files):
    """The first 300 reads under a header with 257 `@RG` lines, as BAM and as SAM text."""
    d = files["dir"]
    bam, sam = str(d / "rg257.bam"), str(d / "rg257.sam")
    cols = synth.slice_batch(files["cols"], 0, 300)
    hostio.write_bam(bam, cols, NAMES, LENS, n_lanes=257)
    hostio.write_sam(sam, cols, NAMES, LENS, n_lanes=257)
    text = open(sam).read()
    assert len(re.findall(r"^@RG\t", text, re.M)) == 257 and len(re.findall(r"^@RG\t", pybam.read_bam(bam)[0], re.M)) == 257
    return dict(bam=bam, sam=sam, text=text.encode())


@pytest.mark.parametrize("how", ["bam, decode 0", "bam, decode 1", "sam file, decode 0", "sam file, decode 1", "sam text on stdin"])
def test_257_read_groups_are_refused_by_name(files, files257, how):
    """a non-zero status, a message that names the limit, and no output file — not even an empty one"""
    out = str(files["dir"] / ("never_%s.bamqc" % re.sub(r"\W+", "_", how)))
    env = dict(BQC_GPU_DECODE=how[-1]) if "decode" in how else {}
    src = files257["bam"] if how.startswith("bam") else files257["sam"] if how.startswith("sam file") else "-"
    r = run(["-r", files["fa"], "-o", out] + COMMON + [src], env=env, input=files257["text"] if src == "-" else None)
    assert r.returncode != 0, r.stderr
    assert b"257 @RG lines" in r.stderr and b"at most 256 read groups" in r.stderr, r.stderr
    assert not os.path.exists(out)
