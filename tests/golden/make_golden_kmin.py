#!/usr/bin/env python3
"""Generate tests/golden/linear_kmin.json from the UNMODIFIED reference's `km linear_kmin`.

Runs only where the reference tree is available (REF below); the GPU tests read the JSON alone.
`linear_kmin` never opens a k-mer database, but km/utils/common.py imports the Jellyfish binding at
module load, so an empty module named ``jellyfish`` is put on sys.path first.

Every case is one call of the reference's main_linear_kmin (km/tools/linear_kmin.py:49-61) on real
files, so file reading (km/utils/common.py:25-45: records joined and upper-cased, lines before the
first header ignored, consecutive headers merged) is part of what is pinned.  Stored per case: the
file texts, the -s value, the reference's whole stdout and, where it raised, the exception's type
and message.

usage:  python tests/golden/make_golden_kmin.py [--out tests/golden] [--jobs 8]
"""

import argparse
import contextlib
import io
import json
import multiprocessing
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = "/root/reference"
CATALOG = sorted(os.listdir(os.path.join(TESTS, "data", "catalog", "GRCh38")))
SEED = 20261016


def _init(standin_dir):
    sys.path.insert(0, REF)
    sys.path.insert(0, standin_dir)


def run_reference(job):
    """job = {"files": {relname: text} | None, "paths": [...], "start": int|None} -> stdout, error."""
    from km.tools import linear_kmin as lk
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for p in job["paths"]:
            if job.get("files") is not None:
                full = os.path.join(tmp, p)
                with open(full, "w") as fh:
                    fh.write(job["files"][p])
                paths.append(full)
            else:
                paths.append(os.path.join(TESTS, p))
        ns = argparse.Namespace(target_fn=paths, start=10 if job["start"] is None else job["start"])
        out = io.StringIO()
        err = None
        with contextlib.redirect_stdout(out):
            try:
                lk.main_linear_kmin(ns, None)
            except Exception as e:      # noqa: BLE001 - the reference's own exception is the datum
                err = {"type": type(e).__name__, "message": str(e)}
    return {"stdout": out.getvalue(), "error": err}


# ------------------------------------------------------------------ synthetic targets
def _rand(rng, n, alphabet):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _length(rng):
    r = rng.random()
    if r < 0.15:
        return rng.randint(0, 12)
    if r < 0.75:
        return rng.randint(13, 300)
    if r < 0.93:
        return rng.randint(301, 900)
    return rng.randint(901, 2000)


def _target(rng, kind):
    alphabet = "ACGTN"[:rng.randint(1, 5)] if kind != "acgt" else "ACGT"
    n = _length(rng)
    if kind == "acgt" or kind == "alphabet":
        return _rand(rng, n, alphabet)
    base = _rand(rng, n, "ACGT" if rng.random() < 0.7 else "ACGTN")
    if kind == "homopolymer":
        h = rng.randint(1, 40)
        head, tail = rng.choice("ACGTN") * h, rng.choice("ACGTN") * rng.randint(0, 40)
        return head + base + tail if rng.random() < 0.5 else base + tail + head
    if kind == "prefix_suffix":             # the exempt {0, L} pair: the first bases equal the last
        p = _rand(rng, rng.randint(1, 30), "ACGT")
        return p + base + p
    if kind == "tandem":
        if not base:
            base = _rand(rng, 40, "ACGT")
        i = rng.randint(0, len(base))
        dup = _rand(rng, rng.randint(1, 60), "ACGT")
        return base[:i] + dup * rng.randint(2, 3) + base[i:]
    raise ValueError(kind)


def _fasta(rng, name, seq):
    """seq as FASTA text: mixed case, wrapped lines, now and then several records, text before the first
    header, or a run of consecutive headers (the reference keeps the first of them)."""
    if rng.random() < 0.4:
        seq = "".join(c.lower() if rng.random() < 0.5 else c for c in seq)
    parts = [seq]
    if len(seq) > 20 and rng.random() < 0.25:
        cut = sorted(rng.sample(range(1, len(seq)), 2))
        parts = [seq[:cut[0]], seq[cut[0]:cut[1]], seq[cut[1]:]]
    text = ""
    if rng.random() < 0.1:
        text += "free text before the first header\n"
    width = rng.choice([60, 70, 80, 1000000])
    for i, part in enumerate(parts):
        text += ">%s_%d chr1:%d-%d\n" % (name, i, 1, len(part) + 1)
        if rng.random() < 0.1:
            text += ">second header line of the same record\n"
        text += "".join(part[j:j + width] + "\n" for j in range(0, len(part), width)) or "\n"
    return text


def synthetic_cases(n_cases=200):
    rng = random.Random(SEED)
    kinds = ["acgt", "alphabet", "homopolymer", "prefix_suffix", "tandem"]
    cases = []
    for c in range(n_cases):
        seq = _target(rng, kinds[c % len(kinds)])
        name = "syn%03d" % c
        n = len(seq)
        start = rng.choice([-2, 0, 1, 2, 3, 5, 10, 10, 10, 31, n - 1, n, n + 1])
        cases.append({"kind": kinds[c % len(kinds)], "start": start, "paths": [name + ".fa"],
                      "files": {name + ".fa": _fasta(rng, name, seq)}})
    return cases


ERROR_FILES = {
    # a '|' field without exactly one '=': ValueError of `k, v = x.split("=")` (km/utils/common.py:38-40)
    "bad_field.fa": ">chr13:28033000-28034000|strand\nACGTACGTTTGACCA\n",
    "two_equals.fa": ">name=x|a=b\nACGTACGTTTGACCA\n",
    # a header with nothing after it: next(groups) inside the generator -> RuntimeError
    "no_sequence.fa": ">t1\nACGTTGCAAC\n>t2\n",
    "only_header.fa": ">t1\n",
    # well-formed quirks: text before the first header, consecutive headers, an empty line
    "quirks.fa": "junk line\n>first|a=b\n>second\nacgtTGCA\n\nGGCCAATT\n>third\nttttAAAA\n",
    "fine.fa": ">ok\nACGTACGGTTACCAGT\n",
}


def error_cases():
    c = []
    for bad in ("bad_field.fa", "two_equals.fa", "no_sequence.fa", "only_header.fa"):
        c.append({"kind": "error", "start": None, "paths": ["fine.fa", "quirks.fa", bad, "fine.fa"],
                  "files": dict(ERROR_FILES)})
    c.append({"kind": "error", "start": 5, "paths": ["quirks.fa", "fine.fa"], "files": dict(ERROR_FILES)})
    return c


def fixture_cases():
    cases = []
    for f in CATALOG:
        path = "data/catalog/GRCh38/" + f
        with open(os.path.join(TESTS, path)) as fh:
            n = len("".join(l.strip() for l in fh if not l.startswith(">")))
        for s in (-2, 0, 1, 2, 5, 10, 31, n - 1, n, n + 1, n + 5):
            cases.append({"kind": "fixture", "start": s, "paths": [path], "files": None})
    paths = ["data/catalog/GRCh38/" + f for f in CATALOG]
    cases.append({"kind": "fixture_list", "start": 5, "paths": paths, "files": None})
    cases.append({"kind": "fixture_list", "start": None, "paths": paths, "files": None})
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    cases = fixture_cases() + synthetic_cases() + error_cases()
    with tempfile.TemporaryDirectory() as standin:
        with open(os.path.join(standin, "jellyfish.py"), "w") as fh:
            fh.write('"""Empty stand-in: linear_kmin never opens a database."""\n')
        with multiprocessing.Pool(args.jobs, initializer=_init, initargs=(standin,)) as pool:
            results = pool.map(run_reference, cases, chunksize=1)
    for case, res in zip(cases, results):
        case.update(res)
    with open(os.path.join(args.out, "linear_kmin.json"), "w") as fh:
        json.dump({"generator": "tests/golden/make_golden_kmin.py", "seed": SEED, "cases": cases}, fh,
                  separators=(",", ":"))
    print("%d cases, %d with an error" % (len(cases), sum(c["error"] is not None for c in cases)))


if __name__ == "__main__":
    main()
