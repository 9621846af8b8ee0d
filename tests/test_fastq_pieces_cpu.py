"""The piece cutter every consumer of raw FASTQ text shares (csrc/fastq_cut.h: kmcut::call_end, kmcut::next_piece),
driven on the CPU under AddressSanitizer + UBSan (tests/host/fastq_pieces.cpp).  No GPU, and no Python in the
sanitised process.

The model is written from the definition, as in tests/test_fastq_cut.py: a record is complete when its four lines are
there with their newlines, so the cut of a well-formed text is the end of the last line whose number (from 1) is a
multiple of four.  A piece is the longest run of whole records within a staging buffer, or all that is left if that
fits; a non-final call takes the whole records of its text, a final one all of it."""
import bisect
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
N_SETS = 100


def line_ends(text):
    return [i + 1 for i, ch in enumerate(text) if ch == 0x0A]


def model_cut(ends, lo, hi):
    """The cut of text[lo:hi], from the definition; ends = line_ends(text).  (A line of the slice ends at e - lo for
    every e in ends with lo < e <= hi: looked up, so that the slice is not walked again for every piece.)"""
    a, b = bisect.bisect_right(ends, lo), bisect.bisect_right(ends, hi)
    whole = (b - a) // 4
    return ends[a + 4 * whole - 1] - lo if whole else 0


def record_sets():
    """The seeded random record sets of tests/test_fastq_cut.py: 2-6 records, sequences of 0-39 bases, CRLF mixed in,
    quality lines that start with '@' and '+' often; each with and without the newline of its last record."""
    rng = np.random.default_rng(11)
    first = np.frombuffer(b"@+ACGTI!5", np.uint8)
    texts = []
    for _ in range(N_SETS):
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
        texts.append(text)
        texts.append(text[:-len(nl)])
    return texts


def test_the_model_cut_on_slices():
    text = b"@a\nAC\n+\nII\n@b\nG\n+\nI\n@c\nT\n+\nI"
    ends = line_ends(text)
    assert ends == [3, 6, 8, 11, 14, 16, 18, 20, 23, 25, 27]        # records end at 11 and 20; the third is open
    assert model_cut(ends, 0, len(text)) == 20 and model_cut(ends, 0, 19) == 11 and model_cut(ends, 0, 10) == 0
    assert model_cut(ends, 11, len(text)) == 9 and model_cut(ends, 11, 19) == 0 and model_cut(ends, 20, len(text)) == 0


def test_pieces_program_under_sanitizers(tmp_path):
    """Every record set, as a non-final and as a final call, at every staging size from 6 bytes (the smallest record)
    to the text's length + 1: the pieces are contiguous from 0, none is longer than a staging buffer, each ends where
    the model's cut of the next `stage` bytes ends (so it is maximal) except the last one of a final call, which ends
    with the text; a non-final call stops at the model's cut of the text; and "no record fits" is reported exactly
    when the model's cut of the next `stage` bytes is 0 and more than `stage` bytes remain, at that offset."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "fastq_pieces")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "host", "fastq_pieces.cpp")])
    texts = record_sets()
    path = str(tmp_path / "in.bin")
    with open(path, "wb") as fh:
        fh.write(b"%d\n" % len(texts))
        for text in texts:
            fh.write(b"%d\n" % len(text) + text)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    proc = subprocess.run([exe, path], capture_output=True, env=env, timeout=600)
    assert proc.returncode == 0 and proc.stdout.endswith(b"FASTQ PIECES OK\n"), (proc.stdout[-500:], proc.stderr[-3000:])
    assert b"ERROR: AddressSanitizer" not in proc.stderr and b"runtime error" not in proc.stderr, proc.stderr[-3000:]
    lines = iter(proc.stdout.split(b"\n"))
    n_cases = n_nofit = n_open_last = 0
    for t, text in enumerate(texts):
        assert next(lines) == b"TEXT %d" % t
        n, ends = len(text), line_ends(text)
        for stage in range(6, n + 2):
            for final in (0, 1):
                word = next(lines).split()
                assert word[:5] == [b"S", b"%d" % stage, b"F", b"%d" % final, b"END"] and word[6] == b"P", (t, word)
                end = int(word[5])
                assert end == (n if final else model_cut(ends, 0, n)), (t, stage, final)
                pos, nofit = 0, None
                for w in word[7:]:
                    if w == b"X":                                           # (nothing comes behind a failure)
                        nofit = int(word[-1])
                        assert word[-2] == b"X"
                        break
                    take = int(w)
                    assert 0 < take <= stage and pos + take <= end, (t, stage, final, pos)
                    want = model_cut(ends, pos, min(pos + stage, end))
                    if final and end - pos <= stage:                        # the last piece of a final call
                        want = end - pos
                        n_open_last += text[-1:] != b"\n"
                    assert take == want, (t, stage, final, pos)
                    pos += take
                rest = end - pos
                starved = rest > stage and model_cut(ends, pos, pos + stage) == 0
                assert (nofit is not None) == starved, (t, stage, final, pos)
                if starved:
                    assert nofit == pos, (t, stage, final)
                    n_nofit += 1
                else:
                    assert pos == end, (t, stage, final)
                n_cases += 1
    assert next(lines) == b"FASTQ PIECES OK"
    assert n_cases == sum(2 * (len(text) - 4) for text in texts) and n_nofit and n_open_last
