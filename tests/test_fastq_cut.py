"""km_fastq_cut (km_amd.lib.fastq_cut): where the last complete record of a block of 4-line FASTQ text ends, and the
`count -Q` flag's parsing.  CPU only: the cut is host code and the flag is argparse.

The model is written from the definition: a record is complete when its four lines are there with their newlines,
so the cut of a well-formed prefix is the end of the last line whose number (from 1) is a multiple of four."""
import ctypes as C

import numpy as np
import pytest

from km_amd import cli
from km_amd import lib as kmlib


def model_cut(text):
    ends = [i + 1 for i, ch in enumerate(text) if ch == 0x0A]
    whole = len(ends) // 4
    return ends[4 * whole - 1] if whole else 0


R1 = b"@r1 first\nACGTACGT\n+\nIIIIIIII\n"
R2 = b"@r2\nGGCC\n+r2\n!!!!\n"


def test_text_that_ends_at_a_record_end():
    assert kmlib.fastq_cut(R1) == len(R1)
    assert kmlib.fastq_cut(R1 + R2) == len(R1 + R2)


@pytest.mark.parametrize("tail, name", [(b"@r2", "header"), (b"@r2\nGG", "sequence"), (b"@r2\nGGCC\n+r", "plus"),
                                        (b"@r2\nGGCC\n+r2\n!!", "quality"), (b"@r2\n", "header done"),
                                        (b"@r2\nGGCC\n", "sequence done"), (b"@r2\nGGCC\n+r2\n", "plus done"),
                                        (b"@r2\nGGCC\n+r2\n!!!!", "quality without its newline")])
def test_a_cut_in_each_of_the_four_lines_and_in_mid_line(tail, name):
    assert kmlib.fastq_cut(R1 + tail) == len(R1), name
    assert kmlib.fastq_cut(R1 + R2 + tail) == len(R1 + R2), name


def test_a_quality_line_that_starts_with_at():
    a = b"@r1\nACGT\n+\n@III\n"
    for tail in (b"", b"@r2", b"@r2\n", b"@r2\nAC", b"@r2\nACGT\n", b"@r2\nACGT\n+", b"@r2\nACGT\n+\n", b"@r2\nACGT\n+\nII"):
        assert kmlib.fastq_cut(R1 + a + tail) == len(R1 + a), tail
    b = b"@r2\nACGT\n+\n@@II\n"
    assert kmlib.fastq_cut(a + b + b"@r3\nAC") == len(a + b)


def test_quality_lines_that_start_with_at_and_with_plus():
    """The quality of one record starts with '@', that of the next with '+' (and its sequence line is followed by
    a '+' line like any other): only the line two below decides."""
    a = b"@r1\nACGT\n+\n@+II\n"
    b = b"@r2\nTTGA\n+\n+@II\n"
    c = b"@r3\nCCCC\n+\n++++\n"
    text = a + b + c
    for at in range(len(text) + 1):
        assert kmlib.fastq_cut(text[:at]) == model_cut(text[:at]), at
    assert kmlib.fastq_cut(text) == len(text)


def test_crlf_text():
    text = (R1 + R2 + R1).replace(b"\n", b"\r\n")
    for at in range(len(text) + 1):
        assert kmlib.fastq_cut(text[:at]) == model_cut(text[:at]), at


def test_no_complete_record_and_one_record_without_a_final_newline():
    for text in (b"", b"@", b"@r1\nACGT\n+\nIII", b"@r1\nACGT\n+\nIIII", b"\n", b"ACGT\nACGT\n"):
        assert kmlib.fastq_cut(text) == 0, text
    assert kmlib.fastq_cut(b"@r1\nACGT\n+\nIIII\n") == 16
    assert kmlib.fastq_cut(b"@r\n\n+\n\n") == 7                   # an empty sequence and an empty quality line


def test_random_record_sets_cut_at_every_offset_of_the_last_two_records():
    rng = np.random.default_rng(7)
    first = np.frombuffer(b"@+ACGTI!5", np.uint8)                  # quality lines start with these, '@' and '+' often
    for _ in range(200):
        recs = []
        for i in range(int(rng.integers(2, 7))):
            ln = int(rng.integers(0, 40))
            seq = np.frombuffer(b"ACGTNacgt", np.uint8)[rng.integers(0, 9, ln)].tobytes()
            qual = rng.integers(33, 75, ln).astype(np.uint8)
            if ln:
                qual[0] = first[rng.integers(0, first.size)]
            nl = b"\r\n" if rng.integers(4) == 0 else b"\n"
            plus = b"+" + (b"r%d" % i if rng.integers(2) else b"")
            recs.append(b"@r%d x" % i + nl + seq + nl + plus + nl + qual.tobytes() + nl)
        text = b"".join(recs)
        lo = len(text) - len(recs[-1]) - len(recs[-2])
        for at in range(lo, len(text) + 1):
            assert kmlib.fastq_cut(text[:at]) == model_cut(text[:at]), (text, at)


def test_argument_errors():
    lib = kmlib.load()
    n = C.c_uint64()
    buf = np.frombuffer(R1, np.uint8)
    assert lib.km_fastq_cut(kmlib.ptr(buf), buf.size, None) == 4
    assert lib.km_fastq_cut(None, 4, C.byref(n)) == 4
    assert lib.km_fastq_cut(None, 0, C.byref(n)) == 0 and n.value == 0
    assert lib.km_counter_add_fastq(None, kmlib.ptr(buf), buf.size, 1, 0, C.byref(n)) == 4
    with pytest.raises(ValueError):
        kmlib._qual_byte("ab")


def test_cli_min_qual_char_takes_exactly_one_character(capsys):
    parser = cli.build_parser()
    with pytest.raises(SystemExit) as e:
        parser.parse_args(["count", "-Q", "ab", "reads.fq"])
    assert e.value.code == 2 and "exactly one character" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["count", "--min-qual-char", "", "reads.fq"])
    args = parser.parse_args(["count", "-m", "31", "-C", "-Q", "+", "-L", "2", "reads.fq"])
    assert args.min_qual_char == "+" and args.lower_count == 2
    assert parser.parse_args(["count", "--min-qual-char", "5", "reads.fq"]).min_qual_char == "5"
    assert parser.parse_args(["count", "reads.fq"]).min_qual_char is None
