"""CPU: the program's command line answers as recorded.  tests/golden/program_options/cases.json holds a matrix of command lines with what
the parser answered to each BEFORE its option rules were gathered into one table (host/program_options.cpp) — the return code, the input
path and the exact bytes on stderr of bqc_program_args (no GPU call), or of bqc_session_open for a session's form of the options — and
help.txt the help text.  The matrix: for every bounded number its bounds, one beyond each, "", x, 12x, -1, 1e2, numbers of 25 digits, valid
values padded with zeros to 10 and 11 characters, the --opt=value form and the option as the last argument; every option that implies or
needs a module alone, with the module, in front of and behind the module's own option; two options that need one module (the last one
given is named); each module that cannot run with --gpus, by its flag and by a parameter option; the faults of --adapter and
--regions-thresholds; the positional, -o and --manifest rules; what a session refuses."""
import ctypes
import json
import os

from bamqc_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "program_options")
RECORDED = json.load(open(os.path.join(GOLDEN, "cases.json")))


def c_argv(args):
    return len(args) + 1, (ctypes.c_char_p * (len(args) + 1))(b"bamqualcheck", *[a.encode() for a in args])


def program(args):
    buf = ctypes.create_string_buffer(b"untouched", 4096)
    rc = _lib.load().bqc_program_args(*c_argv(args), buf, 4096)
    return rc, buf.value.decode()


def session(args):
    lib, h = _lib.load(), ctypes.c_void_p()
    rc = lib.bqc_session_open(*c_argv(args), ctypes.byref(h))
    if rc == 0:
        lib.bqc_session_close(h)  # (nothing has touched a card: a session only starts the runtime with its first job)
    return rc, ""


def test_matrix_covers_what_it_says():
    cases = RECORDED["cases"]
    assert len(cases) > 600 and len({(c["entry"], tuple(c["args"])) for c in cases}) == len(cases)
    assert sum(c["rc"] == 0 for c in cases) > 200 and sum(c["rc"] == 1 for c in cases) > 400 and any(c["rc"] == 2 for c in cases)
    text = " ".join(c["stderr"] for c in cases)
    for piece in ("is not a number of cycles", "is not a base quality", "is not a mapping quality", "is not a histogram cap", "is not a prefix length", "is not a number of reads per million",
                  "is not a number of sequences", "is not a window size", "is not a number of signatures", "is not a window length", "is not a list of depths", "is not an adapter",
                  "is given twice", "at most 8 adapters", "needs --site-alleles FILE", "needs --regions FILE", "needs --duplicate-sets (", "--gc-bias with --gpus", "--duplicate-sets with --gpus",
                  "--overrepresented with --gpus", "illegal option -- gpus", "a session takes the program's options", "-o cannot be given with it", "no BAMFILE can be given with it",
                  "Not enough arguments", "Too many arguments", "required option -r/--reference missing", "required option -o/--output-file missing", "valid file extensions"):
        assert piece in text, piece
    # the digit limit is a fact of the newer options only: both answers to a valid value of 11 characters are in the matrix
    by_args = {tuple(c["args"][4:]): c["rc"] for c in cases if c["entry"] == "program"}
    assert by_args[("--qual-by-cycle-len", "00000000001", "in.bam")] == 0 and by_args[("--duplicate-sets", "--duplicate-sets-capacity", "00000000016", "in.bam")] == 1
    assert by_args[("--substitutions-len", str(0x7FFFFFF), "in.bam")] == 0 and by_args[("--substitutions-len", str(0x7FFFFFF + 1), "in.bam")] == 1


def test_every_command_line_answers_as_recorded(capfd, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # (the lists of the --manifest cases, by relative name: the name is part of the messages)
    for name, text in RECORDED["files"].items():
        (tmp_path / name).write_text(text)
    flush = ctypes.CDLL(None).fflush
    capfd.readouterr()
    wrong = []
    for c in RECORDED["cases"]:
        rc, path = (program if c["entry"] == "program" else session)(c["args"])
        flush(None)  # (the library prints help and version through C's stdout)
        cap = capfd.readouterr()
        if (rc, path, cap.err) != (c["rc"], c["path"], c["stderr"]) or ("stdout" in c and cap.out != c["stdout"]):
            wrong.append((c["entry"], c["args"], (rc, path, cap.err), (c["rc"], c["path"], c["stderr"])))
    assert not wrong, "%d of %d differ; the first: %r" % (len(wrong), len(RECORDED["cases"]), wrong[:3])


def test_help_text_is_byte_identical(capfd):
    capfd.readouterr()
    assert program(["--help"]) == (2, "untouched")
    ctypes.CDLL(None).fflush(None)
    assert capfd.readouterr().out.encode() == open(os.path.join(GOLDEN, "help.txt"), "rb").read()


def test_two_modules_that_cannot_run_with_gpus(capfd):
    """The front end's order decides which one is named, here as there: gc-bias, then duplicate-sets, then overrepresented (the one
    answer of this parser that differs from the recorded parser's, which looked for duplicate-sets first)."""
    base = ["-r", "g.fa", "-o", "x.bamqc", "--gpus", "2"]
    capfd.readouterr()
    for mods, named in ((["--overrepresented", "--duplicate-sets", "--gc-bias"], "--gc-bias"), (["--overrepresented-len=30", "--duplicate-sets"], "--duplicate-sets"),
                        (["--duplicate-sets", "--gc-bias-window", "50"], "--gc-bias")):
        assert program(base + mods + ["in.bam"]) == (1, "untouched")
        assert capfd.readouterr().err.startswith("bamqualcheck: %s with --gpus is not supported: " % named)
