"""Filtered counting (km_counter_set_filter, Counter.set_filter, count_files(only=), `count --if`): what is decided
without a GPU, and the model the GPU tests (test_count_filter.py) compare with.

The model is written from the definition (DESIGN.md §10 "Filtered counting"): every byte of ACGTacgt is a base, any
other byte a break; every window of k bases is a k-mer, replaced by min(key, reverse complement) for a canonical
counter; a window adds 1 to its key only if that key is in the filter, and every key of the filter is in the result,
with 0 if it never occurred.  It walks the text byte by byte in plain Python and shares no code with the kernels."""
import ctypes as C
import os

import numpy as np
import pytest

from km_amd import cli
from km_amd import count as kc
from km_amd import lib as kmlib

E_ARG = 4
_CODE = {ch: c for ch, c in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3))}


def revcomp_key(key, k):
    out = 0
    for _ in range(k):
        out = (out << 2) | (3 - (key & 3))
        key >>= 2
    return out


def canonical_key(key, k, canonical):
    key = int(key)
    return min(key, revcomp_key(key, k)) if canonical else key


def filtered_model(data, k, canonical, keys):
    """{key: count} over the filter `keys` (any iterable of ints; canonicalised here for a canonical counter) for the
    text `data` (bytes of bases and breaks)."""
    want = {canonical_key(key, k, canonical): 0 for key in keys}
    mask = (1 << (2 * k)) - 1
    top = 2 * (k - 1)
    fwd = rev = run = 0                                  # rev: the reverse complement of fwd, rolled beside it
    for ch in bytes(data):
        c = _CODE.get(ch)
        if c is None:
            run = 0
            continue
        fwd = ((fwd << 2) | c) & mask
        rev = (rev >> 2) | ((3 - c) << top)
        run += 1
        if run >= k:
            key = min(fwd, rev) if canonical else fwd
            if key in want:
                want[key] += 1
    return want


def brute_counts(data, k, canonical):
    """{key: count} of every window of `data`, from the letters of each substring."""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    text = bytes(data).upper()
    out = {}
    for i in range(len(text) - k + 1):
        mer = text[i:i + k]
        if any(ch not in b"ACGT" for ch in mer):
            continue
        if canonical:
            mer = min(mer, mer.translate(comp)[::-1])
        key = 0
        for ch in mer:
            key = key * 4 + b"ACGT".index(ch)
        out[key] = out.get(key, 0) + 1
    return out


def test_model_equals_brute_force_on_a_short_text():
    rng = np.random.default_rng(7)
    text = bytearray(np.frombuffer(b"ACGTacgt", np.uint8)[rng.integers(0, 8, 200)].tobytes())
    for at in (17, 60, 61, 140):
        text[at] = ord("N")
    text[99] = ord("\n")
    for k, canonical in ((2, False), (3, True), (5, True), (5, False), (31, True), (32, False)):
        brute = brute_counts(text, k, canonical)
        present = sorted(brute)
        assert present
        absent = [key for key in range(min(40, 4 ** k)) if canonical_key(key, k, canonical) not in brute]
        chosen = present[::2] + absent + present[:3]                  # half of what occurs, absent keys, repeats
        want = {canonical_key(key, k, canonical): brute.get(canonical_key(key, k, canonical), 0) for key in chosen}
        assert filtered_model(text, k, canonical, chosen) == want
        if canonical:                                                 # the other strand names the same key
            flipped = [revcomp_key(key, k) for key in chosen]
            assert filtered_model(text, k, canonical, flipped) == want
        assert filtered_model(text, k, canonical, []) == {}
        assert sum(filtered_model(text, k, canonical, present).values()) == sum(brute.values())


def test_argument_errors_before_any_hip_call():
    lib = kmlib.load()
    keys = np.zeros(4, np.uint64)
    assert lib.km_counter_set_filter(None, kmlib.ptr(keys), 4) == E_ARG
    assert lib.km_counter_set_filter(None, None, 0) == E_ARG
    # null keys with n > 0: refused on the arguments alone, whatever the counter (never looked at)
    not_a_counter = C.create_string_buffer(4096)
    assert lib.km_counter_set_filter(C.cast(not_a_counter, C.c_void_p), None, 4) == E_ARG
    assert lib.km_counter_filter_stats(None, None, None, None, None, None) == E_ARG


def test_parse_args_if_may_repeat():
    args = cli.parse_args(["count", "--if", "a", "--if", "b", "-m", "21", "reads.fq"], cli.build_parser())
    assert args.only == ["a", "b"] and args.mer_len == 21 and args.reads == ["reads.fq"]
    args = cli.parse_args(["count", "reads.fq"], cli.build_parser())
    assert args.only is None
    assert "--if" in cli.build_parser()._subparsers._group_actions[0].choices["count"].format_help()


def _no_counter(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError("a counter was created")
    monkeypatch.setattr(kmlib, "Counter", refuse)


def test_count_files_refuses_a_filter_file_before_a_counter_exists(tmp_path, monkeypatch):
    _no_counter(monkeypatch)
    jf = str(tmp_path / "k21.jf")
    kc.write_records(jf, np.array([1, 2, 3], np.uint64), np.array([1, 1, 1], np.uint32), 21, True)
    with pytest.raises(ValueError, match="k=21"):
        kc.count_files(["reads.fq"], k=31, canonical=True, only=[jf])
    with pytest.raises(ValueError, match="canonical"):
        kc.count_files(["reads.fq"], k=21, canonical=False, only=[jf])
    with pytest.raises(OSError):
        kc.count_files(["reads.fq"], k=21, canonical=True, only=[str(tmp_path / "missing.fa")])
    foreign = tmp_path / "foreign.bin"
    foreign.write_bytes(b"\x00\x01 neither FASTA nor a table\n" * 8)
    with pytest.raises(ValueError, match="neither FASTA nor"):
        kc.count_files(["reads.fq"], k=21, canonical=True, only=[str(foreign)])


def test_filter_keys_reads_fasta_tables_and_arrays(tmp_path):
    fa = tmp_path / "t.fa"
    fa.write_text("\n>one\nACGTA\nCGNAC\n>two\nTTTTT\n")
    jf = str(tmp_path / "k3.jf")
    kc.write_records(jf, np.array([5, 9], np.uint64), np.array([2, 0], np.uint32), 3, False)
    got = kc.filter_keys([str(fa), jf], 3, False)
    want = sorted(brute_counts(b"ACGTACGNAC\nTTTTT", 3, False))
    assert sorted(set(got[:-1].tolist())) == want and got[-1:].tolist() == [5]     # (a record with count 0 is absent)
    assert got.dtype == np.uint64
    same = np.array([7, 7, 1], np.uint64)
    assert kc.filter_keys(same, 3, False).tolist() == [7, 7, 1]
    assert kc.filter_keys(str(fa), 3, True).tolist() == kc.query_keys(3, True, seq_files=[str(fa)]).tolist()
    assert os.path.exists(jf)
