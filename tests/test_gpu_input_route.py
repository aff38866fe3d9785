"""GPU: every input form through the one opener ("which reader takes it"), by the program and by `hostio.BamFile(gpu=0)`,
with BQC_GPU_DECODE=1 and =0: the reader the program names and the library's `on_card` are what bqc_input_route answers for facts this test
writes down itself; every `.bamqc` file and every set of columns equals the one of the BAM file read by the host readers.  Every read
happens in a child under a time limit (tests/bam_stream_util.py).  The thresholds of the unset variable would need inputs of tens of
megabytes: tests/test_input_route_cpu.py covers them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bamqc_amd import hostio, synth
from tests.bam_stream_util import READER, ROOT, TIMEOUT, program, same, through_fifo
from tests.sam_bgzf_util import members
from tests.test_input_route_cpu import (BAM, C_BAM, C_TEXT, LIB_CARD, OFF, ON, PROGRAM, RD_GPU_BAM, RD_GPU_SAM, RD_GPU_SAM_BGZF, SAM, SAM_BGZF, STDIN,
                                        STREAM, _facts, route)

pytestmark = pytest.mark.gpu
NAMES, LENS = ["chr1", "chr2"], [50_000, 30_000]
# form -> (which bytes, how they arrive: a file / FIFO of that name or stdin, what input_kind and the look at the stream find)
FORMS = {
    "x.bam file": ("bam", "x.bam", dict(kind=BAM, regular=1)),
    "FIFO x.bam": ("bam", "fifo x.bam", dict(kind=STREAM, carries=C_BAM)),
    "- carrying BAM": ("bam", "-", dict(kind=STDIN, dash_bgzf=1, carries=C_BAM)),
    "x.sam file": ("sam", "x.sam", dict(kind=SAM, regular=1)),
    "- carrying SAM text": ("sam", "-", dict(kind=STDIN)),
    "x.sam.gz file": ("sam.gz", "x.sam.gz", dict(kind=SAM_BGZF, regular=1)),
    "FIFO x.sam.gz": ("sam.gz", "fifo x.sam.gz", dict(kind=SAM_BGZF, regular=0)),
    "- carrying BGZF SAM text": ("sam.gz", "-", dict(kind=STDIN, dash_bgzf=1, carries=C_TEXT)),
}
DECODED = {RD_GPU_BAM: "on the GPU (csrc/gpu_bam.hip)", RD_GPU_SAM: "on the GPU (csrc/gpu_sam.hip)", RD_GPU_SAM_BGZF: "on the GPU (csrc/gpu_inflate.hip + csrc/gpu_sam.hip)"}


def _arrive(tmp, data, how, run):
    """run(path, stdin bytes or None) with `data` in a file or a FIFO of the name `how` gives, or on stdin"""
    if how == "-":
        return run("-", data)
    if how.startswith("fifo "):
        fifo = os.path.join(tmp, how[5:])
        return through_fifo(fifo, data, lambda: run(fifo, None))
    path = os.path.join(tmp, how)
    with open(path, "wb") as f:
        f.write(data)
    try:
        return run(path, None)
    finally:
        os.unlink(path)


def _program(tmp, data, how, env):
    out = os.path.join(tmp, "out.bamqc")

    def run(path, stdin):
        r = program(["-r", os.path.join(tmp, "ref.fa"), "-o", out, path], data=stdin, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return r.stderr.decode()

    err = _arrive(tmp, data, how, run)
    with open(out, "rb") as f:
        got = f.read()
    os.unlink(out)
    return err, got


def _library(tmp, data, how, gpu, env):
    out = os.path.join(tmp, "cols.npz")

    def run(path, stdin):
        kw = dict(input=stdin) if stdin is not None else dict(stdin=subprocess.DEVNULL)
        r = subprocess.run([sys.executable, "-c", READER, path, "777", gpu, out, ROOT], capture_output=True, env=dict(os.environ, **env), timeout=TIMEOUT, **kw)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        return r.stdout.decode()

    report = _arrive(tmp, data, how, run)
    with np.load(out) as z:
        cols = {k: z[k] for k in z.files}
    os.unlink(out)
    return cols, report


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """(directory with ref.fa, the bytes of each kind, the host readers' `.bamqc` and columns of the BAM file): made once, left unchanged"""
    tmp = str(tmp_path_factory.mktemp("input_route"))
    hostio.write_fasta(os.path.join(tmp, "ref.fa"), NAMES, [synth.reference(5, i, n) for i, n in enumerate(LENS)])
    cols = hostio.synth_slice(5, 2000, 0, 2000, LENS)
    hostio.write_bam(os.path.join(tmp, "src.bam"), cols, NAMES, LENS, n_lanes=2)
    hostio.write_sam(os.path.join(tmp, "src.sam"), cols, NAMES, LENS, n_lanes=2)
    data = {"bam": open(os.path.join(tmp, "src.bam"), "rb").read(), "sam": open(os.path.join(tmp, "src.sam"), "rb").read()}
    data["sam.gz"] = members(data["sam"], [0xff00])[0]
    err, bamqc = _program(tmp, data["bam"], "x.bam", {"BQC_GPU_DECODE": "0"})
    assert "records decoded on the host" in err
    want_cols, _ = _library(tmp, data["bam"], "x.bam", "host", {})
    assert len(want_cols["flag"]) == 2000
    return tmp, data, bamqc, want_cols


@pytest.mark.parametrize("form", list(FORMS))
def test_the_reader_is_the_routes_and_the_results_are_the_same(inputs, form):
    tmp, data, want_bamqc, want_cols = inputs
    which, how, found = FORMS[form]
    for value, gd in (("1", ON), ("0", OFF)):
        # (has_rg: two @RG lines; size and `ended` have no say while the variable is set)
        facts = dict(found, gpu_decode=gd, has_rg=1, size=len(data[which]) if found.get("regular") else 0)
        env = {"BQC_GPU_DECODE": value}
        err, bamqc = _program(tmp, data[which], how, env)
        reader = route(**_facts(caller=PROGRAM, **facts))["reader"]
        assert "[timing] records decoded %s\n" % DECODED.get(reader, "on the host") in err, (form, value, err[-2000:])
        assert err.count("records decoded on") == 1
        assert bamqc == want_bamqc, (form, value)
        cols, report = _library(tmp, data[which], how, "0", env)
        reader = route(**_facts(caller=LIB_CARD, **facts))["reader"]
        assert "on_card=%r " % (reader >= RD_GPU_BAM) in report, (form, value, report)
        same(want_cols, cols)
