"""`bamqualcheck --manifest LIST` on the command line: the list is read and checked by the program's own parser (bqc_program_args, no GPU
call) before any job runs or any output file is touched — a valid list answers (0, ""), every usage error 1 with nothing created on disk —
and today's forms answer as before.  The front end refuses `--gpus N` with a list before it forks."""
import ctypes
import os
import subprocess

import pytest

from bamqc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "bamqualcheck")


def ask(*args):
    lib = _lib.load()
    argv = (ctypes.c_char_p * (len(args) + 1))(b"bamqualcheck", *[a.encode() for a in args])
    buf = ctypes.create_string_buffer(b"untouched", 4096)
    rc = lib.bqc_program_args(len(args) + 1, argv, buf, 4096)
    return rc, buf.value.decode()


def write_list(tmp_path, text, name="jobs.tsv"):
    p = tmp_path / name
    p.write_bytes(text.encode() if isinstance(text, str) else text)
    return str(p)


def test_valid_list(tmp_path):
    before = sorted(os.listdir(tmp_path))
    lst = write_list(tmp_path, "# cohort 7\n\na.bam\ta.bamqc\r\nsub/b.sam\tsub/b.bamqc\n\n#c.bam\tc.bamqc\nd.bam\td out.bamqc")  # (no newline at the end)
    assert ask("-r", "g.fa", "--manifest", lst) == (0, "")
    assert ask("-r", "g.fa", "--manifest=" + lst, "-k", "21,32", "--batch-reads", "7001", "--no-sketch") == (0, "")
    assert sorted(os.listdir(tmp_path)) == before + ["jobs.tsv"]  # no output file, no directory: nothing is touched by the check


# what is wrong: (the list, a piece of the message the parser must give — the line it means and why)
BAD_LISTS = {
    "no tab": ("a.bam a.bamqc\n", "line 1: expected INPUT<TAB>OUTPUT"),
    "two tabs": ("a.bam\ta.bamqc\textra\n", "line 1: expected INPUT<TAB>OUTPUT"),
    "empty input": ("\ta.bamqc\n", "line 1: expected INPUT<TAB>OUTPUT"),
    "empty output": ("# c\na.bam\t\n", "line 2: expected INPUT<TAB>OUTPUT"),
    "bad line behind a good one": ("a.bam\ta.bamqc\n\nb.bam\n", "line 3: expected INPUT<TAB>OUTPUT"),
    "not bam or sam": ("a.txt\ta.bamqc\n", "line 1: the given path 'a.txt' does not have one of the valid file extensions"),
    "no extension": ("a\ta.bamqc\n", "line 1: the given path 'a' does not have one of the valid file extensions"),
    "stdin is not a job": ("-\ta.bamqc\n", "line 1: a stream on stdin is not a job"),
    "same output twice": ("a.bam\tx.bamqc\nb.bam\ty.bamqc\nc.bam\tx.bamqc\n", "line 3: the output 'x.bamqc' is named twice"),
    "empty list": ("", "names no job"),
    "only comments": ("# nothing\n\n\r\n# here\n", "names no job"),
}


@pytest.mark.parametrize("what", sorted(BAD_LISTS))
def test_bad_list_is_a_usage_error_and_touches_nothing(tmp_path, capfd, what):
    text, message = BAD_LISTS[what]
    lst = write_list(tmp_path, text)
    capfd.readouterr()
    assert ask("-r", "g.fa", "--manifest", lst) == (1, "untouched")
    err = capfd.readouterr().err
    assert message in err and lst in err, err  # (its own message: not the answer to an option the parser does not know)
    assert os.listdir(tmp_path) == ["jobs.tsv"]


def test_list_with_other_arguments(tmp_path, capfd):
    lst = write_list(tmp_path, "a.bam\ta.bamqc\n")
    capfd.readouterr()
    assert ask("-r", "g.fa", "--manifest", lst, "in.bam")[0] == 1             # a positional input beside the list
    assert "no BAMFILE can be given with it" in capfd.readouterr().err
    assert ask("-r", "g.fa", "--manifest", lst, "-o", "x.bamqc")[0] == 1
    assert "-o cannot be given with it" in capfd.readouterr().err
    assert ask("-r", "g.fa", "--manifest", str(tmp_path / "no_such_list"))[0] == 1
    assert "cannot be read" in capfd.readouterr().err
    assert ask("-r", "g.fa", "--manifest", lst, "-")[0] == 1
    assert ask("-r", "g.fa", "--manifest", lst, "-o", "x.bamqc")[0] == 1      # -o beside the list
    assert ask("-r", "g.fa", "--manifest=" + lst, "--output-file=x.bamqc")[0] == 1
    assert ask("--manifest", lst)[0] == 1                                      # -r is required as ever
    assert ask("-r", "g.fa", "--manifest")[0] == 1                             # the option wants its argument
    assert ask("-r", "g.fa", "--manifest", str(tmp_path / "no_such_list"))[0] == 1   # unreadable
    assert ask("-r", "g.fa", "--manifest", str(tmp_path))[0] == 1              # a directory: nothing to read
    assert os.listdir(tmp_path) == ["jobs.tsv"]


def test_todays_forms_answer_as_before():
    assert ask("-r", "g.fa", "-o", "x.bamqc", "in.bam") == (0, "in.bam")
    assert ask("-r", "g.fa", "in.bam", "-o", "looks_like_input.bam") == (0, "in.bam")
    assert ask("-r", "g.fa", "-o", "x.bamqc", "-") == (0, "-")
    assert ask("-r", "g.fa", "-o", "x.bamqc", "--no-such-option", "in.bam")[0] == 1
    assert ask("-r", "g.fa", "-o", "x.bamqc")[0] == 1
    assert ask("-r", "g.fa", "in.bam")[0] == 1
    assert ask("-o", "x.bamqc", "in.bam")[0] == 1
    assert ask("-r", "g.fa", "-o", "x.bamqc", "in.txt")[0] == 1
    assert ask("-r", "g.fa", "-o", "x.bamqc", "a.bam", "b.bam")[0] == 1
    assert ask("--help")[0] == 2


def test_session_options_are_the_programs_without_input_and_output():
    lib = _lib.load()

    def open_close(*args):
        argv = (ctypes.c_char_p * (len(args) + 1))(b"bamqualcheck", *[a.encode() for a in args])
        h = ctypes.c_void_p()
        rc = lib.bqc_session_open(len(args) + 1, argv, ctypes.byref(h))
        if rc == 0:
            assert h.value
            lib.bqc_session_close(h)  # (nothing has touched a card: a session only starts the runtime with its first job)
        else:
            assert not h.value
        return rc

    assert open_close("-r", "g.fa") == 0
    assert open_close("-r", "{dir}/genome.fa", "-c", "chr1", "-k", "21,32", "-q", "10", "--batch-reads", "3000") == 0
    assert open_close() == 1                                    # -r is required
    assert open_close("-r", "g.fa", "in.bam") == 1              # an input
    assert open_close("-r", "g.fa", "-o", "x.bamqc") == 1       # an output
    assert open_close("-r", "g.fa", "--manifest", "l.tsv") == 1
    assert open_close("-r", "g.fa", "--no-such-option") == 1
    assert open_close("-r", "g.fa", "--help") == 1


def test_front_end_refuses_gpus_with_a_list_before_it_forks(tmp_path):
    lst = write_list(tmp_path, "a.bam\ta.bamqc\n")
    for gpus in (["--gpus", "2"], ["--gpus=1"]):
        r = subprocess.run([EXE, "-r", "g.fa", "--manifest", lst] + gpus, capture_output=True, text=True)
        assert r.returncode == 1 and "not supported" in r.stderr and "--manifest" in r.stderr, r.stderr
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--manifest LIST" in r.stdout
    assert os.listdir(tmp_path) == ["jobs.tsv"]
