"""CPU tests of `km find_mutation` over several GPU batches (km_amd/cli.py main_find_mut): which rows are out when a
batch stops the run.  The reference (km/tools/find_mutation.py:37-58) builds every RefSeq before the first walk, so an
input error prints no row at all; a node-limit exit or a naming exception comes after the rows of the earlier targets.
The GPU finder is replaced by a stub that writes the oracle's rows, batch by batch, and stops where it is told to."""
import argparse
import io

import pytest

from km_amd import cli, synth
from km_amd import kmer as km
from km_amd.finder import NodeLimitExceeded
from oracle import km_oracle as ko

N_TARGETS = 25          # with CHUNK = 7: batches of targets 0-6, 7-13, 14-20, 21-24
STOP_AT = 16            # a target of the third batch


@pytest.fixture(scope="module")
def catalog(tmp_path_factory):
    root = tmp_path_factory.mktemp("cli_chunks")
    case = synth.make_case(n_targets=N_TARGETS, length=160, n_keys=12_000, seed=4711, variant_frac=0.6,
                           variants_per_target=(1, 2))
    jf_path = str(root / "cat.jf")
    synth.write_jf(jf_path, case["keys"], case["counts"], 31)
    files, rows = [], {}
    db = ko.KmerDB(None, cutoff=0.05, n_cutoff=5,
                   records={"k": 31, "canonical": True, "keys": case["keys"], "counts": case["counts"]})
    for t, codes in enumerate(case["targets"]):
        name = "t%03d" % t
        seq = km.decode(codes)
        path = str(root / (name + ".fa"))
        with open(path, "w") as fh:
            fh.write(">%s\n%s\n" % (name, seq))
        files.append(path)
        rows[name] = ko.target_rows(ko.analyse_target(seq, name, db), jf_path)
    want, err = ko.run_find_mutation(files, jf_path)
    assert err is None and sum(len(r) > 1 for r in rows.values()) >= 5
    n_head = want.index(ko.HEADER) + 1
    assert want[n_head:] == [r for name in sorted(rows) for r in rows[name]]
    return {"files": files, "jf": jf_path, "rows": rows, "head": want[:n_head]}


class _Jf:
    k = 31

    def __init__(self, *a, **kw):
        pass


class _StubFinder:
    """BatchFinder.write_rows as km_amd/finder.py behaves: an input error is raised before any row of its batch; a
    node limit or a naming exception after the rows of the batch's earlier targets."""
    rows = {}
    stop = None                  # (target index, "input" | "limit" | "naming")
    batches = []

    def __init__(self, jf, max_stack=500, max_break=10, max_node=10000):
        self.max_node = max_node

    def write_rows(self, targets, out, db_name=None):
        _StubFinder.batches.append(len(targets))
        idx = [int(name[1:]) for name, _seq in targets]
        where, kind = _StubFinder.stop or (-1, None)
        if kind == "input" and where in idx:
            exc = ValueError("target t%03d: repeated k-mer" % where)
            exc.km_input_error = True
            raise exc
        for t, (name, _seq) in zip(idx, targets):
            if t == where and kind == "limit":
                out.flush()
                raise NodeLimitExceeded(self.max_node)
            if t == where and kind == "naming":
                out.flush()
                raise IndexError("list index out of range")
            for row in _StubFinder.rows[name]:
                out.write(row + "\n")


def _run(catalog, monkeypatch, stop, stream):
    monkeypatch.setattr(cli, "BatchFinder", _StubFinder)
    monkeypatch.setattr(cli, "Jellyfish", _Jf)
    monkeypatch.setattr(cli, "CHUNK", 7)
    if stream:
        monkeypatch.setattr(cli, "STREAM_ABOVE", N_TARGETS - 1)
    assert (cli.CHUNK < N_TARGETS <= cli.STREAM_ABOVE) == (not stream)
    _StubFinder.rows, _StubFinder.stop, _StubFinder.batches = catalog["rows"], stop, []
    p = argparse.ArgumentParser()
    cli.add_find_mutation_args(p)
    args = p.parse_args(catalog["files"] + [catalog["jf"]])
    out, err = io.StringIO(), io.StringIO()
    exc = None
    try:
        cli.main_find_mut(args, out=out, err=err)
    except (SystemExit, Exception) as e:          # noqa: B902 — what the run ends with is part of the check
        exc = e
    return out.getvalue().splitlines(), exc


def _rows_before(catalog, n):
    return [r for t in range(n) for r in catalog["rows"]["t%03d" % t]]


@pytest.mark.parametrize("stream", [False, True])
def test_clean_catalog_prints_every_batch(catalog, monkeypatch, stream):
    lines, exc = _run(catalog, monkeypatch, None, stream)
    assert exc is None
    assert _StubFinder.batches == [7, 7, 7, 4]
    assert lines[-1].startswith("#Elapsed time:")
    assert lines[:-1] == catalog["head"] + _rows_before(catalog, N_TARGETS)


@pytest.mark.parametrize("stream", [False, True])
def test_input_error_in_the_third_batch(catalog, monkeypatch, stream):
    """Held (the catalog fits STREAM_ABOVE): not one row, as the reference.  Streamed: the first two batches are out."""
    lines, exc = _run(catalog, monkeypatch, (STOP_AT, "input"), stream)
    assert isinstance(exc, ValueError) and getattr(exc, "km_input_error", False)
    assert _StubFinder.batches == [7, 7, 7]
    assert lines == catalog["head"] + (_rows_before(catalog, 14) if stream else [])


@pytest.mark.parametrize("stream", [False, True])
def test_node_limit_in_the_third_batch(catalog, monkeypatch, stream):
    """Every row before the target, then the reference's sys.exit message."""
    lines, exc = _run(catalog, monkeypatch, (STOP_AT, "limit"), stream)
    assert isinstance(exc, SystemExit) and str(exc.code) == "ERROR: Node query count limit exceeded: max=10000"
    assert _StubFinder.batches == [7, 7, 7]
    assert lines == catalog["head"] + _rows_before(catalog, STOP_AT)


@pytest.mark.parametrize("stream", [False, True])
def test_naming_exception_releases_the_earlier_rows(catalog, monkeypatch, stream):
    lines, exc = _run(catalog, monkeypatch, (STOP_AT, "naming"), stream)
    assert isinstance(exc, IndexError) and not getattr(exc, "km_input_error", False)
    assert _StubFinder.batches == [7, 7, 7]
    assert lines == catalog["head"] + _rows_before(catalog, STOP_AT)

