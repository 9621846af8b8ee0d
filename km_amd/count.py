"""Counting k-mers from read files on the GPU: what `jellyfish count -m k -C -L n -s size reads.fq` does in
front of every km tool (``python -m km_amd count``).

``merge_files`` sums (or takes the maximum of) the records of existing .jf files into one table on the GPU, or
intersects / subtracts them (``python -m km_amd merge``).

``count_files`` streams FASTA / FASTQ files (plain or gzip) through :class:`km_amd.lib.Counter` and returns the
database built on the device from the counted records; ``write_records`` writes such records in the file
framing the readers of this project load, sorted by key; ``write_jellyfish`` writes them in Jellyfish's own
record order (sorted on the GPU), as ``Counter.write_jf`` does for records still on the device.
``histo_file``, ``format_histo`` and ``format_stats`` are behind ``python -m km_amd histo`` / ``stats``: the histogram
of a file's counts and its four statistics in one pass on the GPU.  ``dump_file`` and ``query_file`` are behind
``dump`` / ``query``: a file's records, or the counts of given k-mers, as text built on the GPU; the k-mers of
``query -s`` files are cut there too.  ``select_files`` is behind ``bait``: the reads of FASTQ files that hit (or
miss) a table, found and gathered on the GPU.  Only the standard library and numpy.
"""

import contextlib
import gzip
import json
import os
import sys

import numpy as np

from . import lib as _lib

BLOCK = 8 << 20          # text bytes read per add_text call


def _open(path):
    if path == "-":
        return sys.stdin.buffer, False
    fh = open(path, "rb")
    magic = fh.read(2)
    fh.seek(0)
    if magic == b"\x1f\x8b":
        return gzip.open(fh, "rb"), True
    return fh, True


def feed_file(counter, path, block=BLOCK, min_qual_char=None):
    """One file through counter.add_text in blocks, the unconsumed tail carried in front of the next block.
    With min_qual_char (not None) a file whose first non-blank byte is '@' goes through counter.add_fastq with
    that quality threshold instead, from that byte on; a FASTA file has no qualities and takes add_text."""
    blocks = _Blocks(path, block, sniff=None if min_qual_char is None else "report")
    try:
        def add(text, final):
            if blocks.fastq:
                return counter.add_fastq(text, final=final, min_qual_char=min_qual_char)
            return counter.add_text(text, final=final)
        for buf in blocks:
            blocks.used(add(buf, final=False))
        add(blocks.tail, final=True)
    finally:
        blocks.close()


def filter_keys(only, k, canonical):
    """The key array of count_files' `only`, on the host and without a GPU: a uint64 array goes through as it is; a
    path, or a list of paths, gives the keys of its files in the order given.  A file whose first non-blank byte is
    '>' (plain or gzip) is FASTA and gives the k-mers of each of its records (query_keys); any other file must be a
    `binary/sorted` file and gives the keys of its records (one with count 0 is absent, as for every reader here), and
    its k and canonical setting must equal (k, canonical).  OSError for a missing file, ValueError for a foreign one or
    one of another k / canonical."""
    if isinstance(only, np.ndarray):
        return np.ascontiguousarray(only, np.uint64).reshape(-1)
    if isinstance(only, (str, bytes, os.PathLike)):
        only = [only]
    only = list(only)
    if only and all(isinstance(v, (int, np.integer)) for v in only):
        return np.array(only, np.uint64)
    parts = []
    for path in only:
        fh, close = _open(path)
        try:
            head = fh.read(1 << 12).lstrip(b"\r\n \t")
        finally:
            if close:
                fh.close()
        if head[:1] == b">":
            parts.append(query_keys(k, canonical, seq_files=[path]))
            continue
        try:
            info = _lib.jf_file_info(path)
        except _lib.KmError as e:
            raise ValueError("%s is neither FASTA nor a binary/sorted file (%s)" % (path, e.detail)) from e
        if (info["k"], info["canonical"]) != (int(k), bool(canonical)):
            raise ValueError("%s holds k=%d canonical=%s, but the k-mers are counted with k=%d canonical=%s" % (
                path, info["k"], info["canonical"], k, bool(canonical)))
        db = _lib.Database.open(path)
        try:
            parts.append(np.array(db.records()[0], np.uint64))
        finally:
            db.close()
    return np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, np.uint64), np.uint64)


def count_files(paths, k=31, canonical=True, lower_count=1, device=0, expected_distinct=0, keep_counter=False,
                min_qual_char=None, only=None, solid=None):
    """Count the k-mers of every read of `paths` (FASTA or 4-line FASTQ, gzip recognised by its magic, '-' =
    stdin) -> (Database, stats).  stats is the dict of Counter.stats() before the cut at lower_count.
    keep_counter=True returns (Database, stats, Counter) so that the caller can fetch the records.
    min_qual_char (an int or one character; Jellyfish's -Q): FASTQ files are parsed on the GPU (Counter.add_fastq)
    and a base whose quality byte is below it is read as N; None: the host stripper, qualities never looked at.
    only (Jellyfish's --if; a uint64 array of keys, or paths as filter_keys reads them): count only these k-mers
    (Counter.set_filter).  Each of them is a record, with count 0 if it never occurred, so lower_count=0 lists the whole
    set; expected_distinct is ignored, the table is sized by the set.  stats gains filter_kmers, kmers_hit and
    filter_tier.  Everything about `only` that can fail fails before a counter exists.
    solid (an int N, the expected number of distinct k-mers in the reads; this project's own): the k-mers seen once stay
    out of the table.  Every path is fed twice: a first pass notes the k-mers in a sketch of lib.sketch_words(N) words
    (Counter.set_sketch), the second counts those the sketch saw again.  The records are exactly those of a plain count
    cut at max(2, lower_count), which is the cut that is applied; expected_distinct then speaks of the k-mers seen at
    least twice.  stats gains sketch_words, sketch_bits_1, sketch_bits_2, kmers_admitted and lower_count (the
    effective one).  A path '-' (stdin cannot be read twice) and `solid` beside `only` raise ValueError before a counter
    exists."""
    if isinstance(paths, (str, bytes)):
        paths = [paths]
    if solid is not None:
        paths = list(paths)
        if only is not None:
            raise ValueError("solid and only exclude each other: a counter takes a sketch or a filter, not both")
        if "-" in paths:
            raise ValueError("solid reads every input twice: '-' (standard input) can be read once")
        if not 0 <= int(solid) <= 1 << 41:
            raise ValueError("solid=%d: the expected number of distinct k-mers is 0 .. 2^41" % solid)
        words = _lib.sketch_words(solid)
        lower_count = max(2, int(lower_count))
    keys = None if only is None else filter_keys(only, k, canonical)
    counter = _lib.Counter(k=k, canonical=canonical, device=device,
                           expected_distinct=expected_distinct if keys is None else 1)
    try:
        if keys is not None:
            counter.set_filter(keys)
        if solid is not None:
            counter.set_sketch(words)
            for p in paths:
                feed_file(counter, p, min_qual_char=min_qual_char)
            counter.sketch_done()
        for p in paths:
            feed_file(counter, p, min_qual_char=min_qual_char)
        stats = counter.stats()
        if keys is not None:
            fs = counter.filter_stats()
            stats.update(filter_kmers=fs["n_keys"], kmers_hit=fs["kmers_hit"], filter_tier=fs["tier"])
        if solid is not None:
            ss = counter.sketch_stats()
            stats.update(sketch_words=ss["words"], sketch_bits_1=ss["bits_1"], sketch_bits_2=ss["bits_2"],
                         kmers_admitted=ss["kmers_admitted"], lower_count=lower_count)
        db = counter.finish(lower_count)
    except BaseException:
        counter.close()
        raise
    if keep_counter:
        return db, stats, counter
    counter.close()
    return db, stats


def _not_fastq(path):
    return ValueError("%s does not start with '@': bait takes 4-line FASTQ reads only" % path)


def _preflight(paths):
    """Every file but stdin is opened once and its beginning looked at: OSError for a missing one, ValueError for one
    whose first non-blank byte is not '@'."""
    for path in paths:
        if path == "-":
            continue
        fh, _ = _open(path)
        try:
            head = b""
            while not head:
                data = fh.read(1 << 16)
                if not data:
                    break
                head = data.lstrip(b"\r\n")
            if head and head[:1] != b"@":
                raise _not_fastq(path)
        finally:
            fh.close()


class _Blocks:
    """The only reader of a file in blocks: next() -> the unconsumed tail with the next block of the file behind it,
    used(n) says how much of it was taken; done: the file has been read to its end, so what next() returns is all there
    will be.  Iterating yields next() until then.  `sniff` looks at the first non-blank byte, once the leading blank
    lines are dropped: "raise" takes 4-line FASTQ only (ValueError unless it is '@'), "report" says in `fastq` whether
    it is '@'; None passes the file on as it is."""

    def __init__(self, path, block, sniff="raise"):
        self.path, self.block, self.sniff = path, block, sniff
        self.fh, self.close_it = _open(path)
        self.tail, self.started, self.done, self.fastq = b"", sniff is None, False, False

    def next(self):
        while not self.done:
            data = self.fh.read(self.block)
            if not data:
                self.done = True
                break
            buf = self.tail + data if self.tail else data
            if not self.started:
                buf = buf.lstrip(b"\r\n")
                if not buf:
                    continue
                self.fastq = buf[:1] == b"@"
                if not self.fastq and self.sniff == "raise":
                    raise _not_fastq(self.path)
                self.started = True
            self.tail = buf
            break
        return self.tail

    def __iter__(self):
        while True:
            buf = self.next()
            if self.done:
                return
            yield buf

    def used(self, n):
        self.tail = self.tail[n:]

    def close(self):
        if self.close_it:
            self.fh.close()


def select_pair_files(db, paths1, paths2, out1, out2, min_hits=1, invert=False, min_qual_char=None, rule="any",
                      check_names=True, block=BLOCK):
    """select_files for the two mate files of paired-end runs: file i of `paths1` pairs with file i of `paths2`, record
    r of one with record r of the other, and a pair is kept or dropped whole (lib.PairSelector: rule "any", "both" or
    "sum"; check_names compares the mates' names).  Mate 1's kept records go to `out1` and mate 2's to `out2` (paths or
    file objects with fileno()), byte for byte and in input order, so the outputs line up record for record -> the dict
    of km_select_pair_stats_t.  Files are plain or gzip; at most one may be '-' (stdin).  Each file pair is a pair of
    streams of its own, fed in blocks with either unconsumed tail carried in front of that file's next block, and ended
    by a final call.

    The lists must have equal length (ValueError).  Before either output is opened, the pre-flight checks of
    select_files run for all files of both lists.  A KmError names both files of the pair.  An output given as a path
    that this call created is removed again when the call fails; that holds for both outputs."""
    if isinstance(paths1, (str, bytes)):
        paths1 = [paths1]
    if isinstance(paths2, (str, bytes)):
        paths2 = [paths2]
    paths1, paths2 = list(paths1), list(paths2)
    if len(paths1) != len(paths2):
        raise ValueError("%d mate-1 files but %d mate-2 files: every file needs its mate file" % (len(paths1), len(paths2)))
    if not paths1:
        raise ValueError("no input files")
    if (paths1 + paths2).count("-") > 1:
        raise ValueError("at most one input may be '-': standard input can be read once")
    if out1 is None or out2 is None:
        raise ValueError("paired output needs two outputs: standard output cannot carry two files")
    same = out1 is out2
    if not same and all(isinstance(o, (str, bytes, os.PathLike)) for o in (out1, out2)):
        same = os.path.abspath(os.fspath(out1)) == os.path.abspath(os.fspath(out2))
    if same:
        raise ValueError("the two outputs are one: mate 1 and mate 2 need a file each")
    _preflight(paths1 + paths2)
    with _text_out(out1) as fd1, _text_out(out2) as fd2:
        with _lib.PairSelector(db, fd1, fd2, min_hits=min_hits, invert=invert, min_qual_char=min_qual_char, rule=rule,
                               check_names=check_names) as sel:
            for path1, path2 in zip(paths1, paths2):
                mates = []
                try:
                    mates.append(_Blocks(path1, block))
                    mates.append(_Blocks(path2, block))
                    a, b = mates
                    while True:
                        # read where the selector ran dry; a side that is far ahead waits with what it holds
                        need_a = not a.done and (len(a.tail) <= len(b.tail) or b.done)
                        need_b = not b.done and (len(b.tail) <= len(a.tail) or a.done)
                        buf1 = a.next() if need_a else a.tail
                        buf2 = b.next() if need_b else b.tail
                        if a.done and b.done:
                            break
                        used1, used2 = sel.add_fastq(buf1, buf2, final=False)
                        del buf1, buf2                            # (freed before the next two blocks are read)
                        a.used(used1)
                        b.used(used2)
                    sel.add_fastq(a.tail, b.tail, final=True)     # (always: an empty one still ends the pair of streams)
                except _lib.KmError as e:
                    raise _lib.KmError(e.code, "%s, %s: %s" % (path1, path2, e.detail)) from e
                finally:
                    for m in mates:
                        m.close()
            return sel.stats()


def select_files(db, paths, out=None, min_hits=1, invert=False, min_qual_char=None, block=BLOCK):
    """The reads of the 4-line FASTQ files `paths` (plain or gzip, '-' = stdin) that hit the uploaded table `db`: a read
    is kept iff (its windows of k bases whose k-mer `db` holds number at least min_hits) != invert, with a base whose
    quality byte is below min_qual_char read as N first.  The kept records go to `out` (a path, a file object with
    fileno(), or None for standard output) byte for byte and in input order, file after file; they are found and
    gathered on the GPU (lib.Selector) and the host only writes them -> the dict of km_select_stats_t.  Every file is
    a stream of its own, fed in blocks with the unconsumed tail carried in front of the next block and ended by a final
    call, as feed_file does it; a last record without newline gets one.

    Before `out` is opened, every file but stdin is opened once and its beginning looked at: a missing file raises
    OSError, one whose first non-blank byte is not '@' (FASTA, for one) ValueError: reads without qualities are not
    covered.  A malformed record raises KmError whose text names the file and the byte offset within it (of the
    decompressed text); the pieces before it are on `out` by then, but an `out` given as a path that this call
    created is removed again when the call fails, as for the other commands."""
    if isinstance(paths, (str, bytes)):
        paths = [paths]
    paths = list(paths)
    _preflight(paths)
    with _text_out(out) as fd:
        with _lib.Selector(db, fd, min_hits=min_hits, invert=invert, min_qual_char=min_qual_char) as sel:
            for path in paths:
                blocks = _Blocks(path, block)
                try:
                    for buf in blocks:
                        blocks.used(sel.add_fastq(buf, final=False))
                    sel.add_fastq(blocks.tail, final=True)   # (always: an empty one still ends the file's stream)
                except _lib.KmError as e:
                    raise _lib.KmError(e.code, "%s: %s" % (path, e.detail)) from e
                finally:
                    blocks.close()
            return sel.stats()


MAX_LABELS = 32                           # km_select_labels_*: one bit of a 32-bit mask per label


def label_table(label_keys, k, canonical, device=0):
    """The label table of lib.LabelSelector, uploaded: `label_keys` is a list of uint64 key arrays, one per label (at
    most 32; a label may have none); the table holds the union of the keys, and a key's "count" is the mask of the
    labels that have it (bit l = label l) -> Database.  The union and the masks are made on the host with numpy."""
    label_keys = [np.ascontiguousarray(keys, np.uint64).reshape(-1) for keys in label_keys]
    if not 1 <= len(label_keys) <= MAX_LABELS:
        raise ValueError("%d labels: a label table holds 1 to %d" % (len(label_keys), MAX_LABELS))
    every = np.concatenate(label_keys)
    bits = np.concatenate([np.full(keys.size, 1 << l, np.uint32) for l, keys in enumerate(label_keys)])
    keys, inverse = np.unique(every, return_inverse=True)
    masks = np.zeros(keys.size, np.uint32)
    np.bitwise_or.at(masks, inverse.reshape(-1), bits)
    db = _lib.Database.from_records(keys, masks, k, canonical)
    try:
        db.upload(device)
    except BaseException:
        db.close()
        raise
    return db


_TSV_COLUMNS = ("Query", "Type", "Variant_name", "Sequence", "Reference_sequence", "Info")


def _label_kmers(seq, without, k):
    """The canonical k-mers of `seq` upper-cased that are no k-mers of `without`, distinct and ascending."""
    from . import kmer as km
    sets = []
    for text in (seq, without):
        keys = _windows(np.frombuffer(text.upper().encode("latin-1"), np.uint8), k)
        sets.append(np.unique(np.minimum(keys, km.revcomp(keys, k))) if keys.size else keys)
    return np.ascontiguousarray(np.setdiff1d(sets[0], sets[1]), np.uint64)


def rows_labels(tsv, k, with_ref=False, info="vs_ref"):
    """The labels of the variant rows of a `find_mutation` TSV (a path or a file object of text lines): '#' lines and
    the header line are skipped, and a row is taken when its Info column matches `info` (re.search, as `find_report -i`
    reads it), its Type is not Reference and its Sequence is not empty.  Taken row i (from 1) gives the label
    "%02d_<Query>_<Type>.alt" (characters outside [A-Za-z0-9._-] become '_') whose keys are the canonical k-mers of
    Sequence, upper-cased, that Reference_sequence does not have; with_ref adds "....ref" with the two sequences
    exchanged.  A label may have no keys (the .ref label of an ITD: every reference k-mer lies on its path too).
    -> a list of dicts with name, query, type, variant_name, allele ("alt" / "ref") and keys, in label order.
    More than 32 labels raise ValueError; nothing here touches the GPU.  The TSV does not record its k: `k` must be
    the k of the run that wrote it."""
    import re
    if isinstance(tsv, (str, bytes, os.PathLike)):
        with open(tsv, "r") as fh:
            lines = fh.read().splitlines()
    else:
        lines = [ln.decode("latin-1") if isinstance(ln, bytes) else ln for ln in tsv.read().splitlines()]
    want = re.compile(info)
    col, rows = None, []
    for line in lines:
        if not line.strip() or line.startswith("#"):
            continue
        cells = line.split("\t")
        if cells[:2] == ["Database", "Query"]:
            col = {name: cells.index(name) for name in _TSV_COLUMNS}
            continue
        if col is None:
            raise ValueError("a row comes before the header line (Database, Query, ...)")
        if len(cells) <= max(col.values()):
            raise ValueError("a row has %d columns, fewer than the header names" % len(cells))
        row = {name: cells[at] for name, at in col.items()}
        if want.search(row["Info"]) and row["Type"] != "Reference" and row["Sequence"]:
            rows.append(row)
    per = 2 if with_ref else 1
    if len(rows) * per > MAX_LABELS:
        raise ValueError("%d variant rows give %d labels, more than the %d of one run: split the run (fewer rows per "
                         "TSV, a narrower -i, or without --with-ref)" % (len(rows), len(rows) * per, MAX_LABELS))
    labels = []
    for i, row in enumerate(rows, 1):
        stem = re.sub(r"[^A-Za-z0-9._-]", "_", "%02d_%s_%s" % (i, row["Query"], row["Type"]))
        for allele, seq, other in (("alt", row["Sequence"], row["Reference_sequence"]),
                                   ("ref", row["Reference_sequence"], row["Sequence"]))[:per]:
            labels.append({"name": "%s.%s" % (stem, allele), "query": row["Query"], "type": row["Type"],
                           "variant_name": row["Variant_name"], "allele": allele, "keys": _label_kmers(seq, other, k)})
    return labels


def select_label_files(db, names, paths, out_dir, min_hits=1, min_qual_char=None, block=BLOCK):
    """select_files with one output per label: `db` is a label table (label_table) of len(names) labels, and the reads
    of the 4-line FASTQ files `paths` whose windows of k bases with label l's bit number at least min_hits go to
    out_dir/<names[l]>.fq, byte for byte and in input order, file after file (lib.LabelSelector: one pass over the
    reads, split on the GPU) -> the dict of km_select_labels_stats_t with records_out and bytes_out as lists and
    `files`, the paths written.  The pre-flight checks of select_files run before anything is created; out_dir is
    created if absent; a label file this call created is removed again when the call fails."""
    if isinstance(paths, (str, bytes)):
        paths = [paths]
    paths, names = list(paths), list(names)
    if not 1 <= len(names) <= MAX_LABELS:
        raise ValueError("%d labels: one run takes 1 to %d" % (len(names), MAX_LABELS))
    if len(set(names)) != len(names):
        raise ValueError("two labels have one name: every label needs a file of its own")
    _preflight(paths)
    os.makedirs(out_dir, exist_ok=True)
    files = [os.path.join(out_dir, name + ".fq") for name in names]
    with contextlib.ExitStack() as stack:
        fds = [stack.enter_context(_text_out(path)) for path in files]
        with _lib.LabelSelector(db, fds, min_hits=min_hits, min_qual_char=min_qual_char) as sel:
            for path in paths:
                blocks = _Blocks(path, block)
                try:
                    for buf in blocks:
                        blocks.used(sel.add_fastq(buf, final=False))
                    sel.add_fastq(blocks.tail, final=True)   # (always: an empty one still ends the file's stream)
                except _lib.KmError as e:
                    raise _lib.KmError(e.code, "%s: %s" % (path, e.detail)) from e
                finally:
                    blocks.close()
            stats = sel.stats()
    stats["files"] = files
    return stats


def merge_files(paths, mode="sum", lower_count=1, device=0, expected_distinct=0, keep_counter=False,
                upper_count=0xFFFFFFFF):
    """Merge `binary/sorted` files of one k and one canonical setting into one table on the GPU.  Per key the counts
    are summed (saturating at 2^32 - 1) or, with mode="max", their maximum is kept.  mode="intersect" keeps the keys
    that every file holds (count > 0), with the minimum of their counts; mode="subtract" keeps the records of the
    FIRST file whose key no later file holds (Counter.set_jf).  lower_count and upper_count cut the RESULT
    -> (Database, stats), with keep_counter=True (Database, stats, Counter) as count_files.  stats is
    Counter.stats() before the cut plus k, canonical, mode, records_in (records taken with count > 0) and records_out
    (records after the cuts).

    Every header is read first (lib.jf_file_info, no GPU): a file whose k or canonical differs from the first
    file's raises ValueError before a counter exists.  The table is sized from expected_distinct, or else from the
    largest input's record count (sum, max), where it doubles when the union needs it to, or from the first file's
    (intersect, subtract), whose keys are all the table ever holds.  These are this project's own semantics of
    "merge", not checked against a run of `jellyfish merge`."""
    if isinstance(paths, (str, bytes)):
        paths = [paths]
    paths = list(paths)
    if not paths:
        raise ValueError("no input files")
    if mode not in _lib.MERGE_MODES and mode not in _lib.SET_OPS:
        raise ValueError("mode %r is none of 'sum', 'max', 'intersect', 'subtract'" % (mode,))
    infos = [_lib.jf_file_info(p) for p in paths]
    first = infos[0]
    for p, info in zip(paths, infos):
        if (info["k"], info["canonical"]) != (first["k"], first["canonical"]):
            raise ValueError("%s holds k=%d canonical=%s, but %s (the first file) holds k=%d canonical=%s" % (
                p, info["k"], info["canonical"], paths[0], first["k"], first["canonical"]))
    set_op = mode in _lib.SET_OPS
    size = int(expected_distinct) or (first["n_records"] if set_op else max(info["n_records"] for info in infos))
    counter = _lib.Counter(k=first["k"], canonical=first["canonical"], device=device, expected_distinct=size)
    try:
        for p in paths:
            if set_op:
                counter.set_jf(p, op=mode)
            else:
                counter.add_jf(p, mode=mode)
        stats = counter.stats()
        stats.update(k=first["k"], canonical=first["canonical"], mode=mode,
                     records_in=counter.merge_stats()["records_in"])
        db = counter.finish(lower_count, upper_count)
        stats["records_out"] = counter.n_records()
    except BaseException:
        counter.close()
        raise
    if keep_counter:
        return db, stats, counter
    counter.close()
    return db, stats


MAX_COMPARE_INPUTS = 32
COMPARE_FORMS = ("pairs", "shared", "jaccard", "summary", "spectrum")


def compare_files(paths, lower_count=1, upper_count=0xFFFFFFFF, device=0):
    """How up to 32 `binary/sorted` files of one k and one canonical setting relate, counted on the GPU in one table
    whose count cells are membership masks (Counter.mark_jf, Counter.cooccurrence): file i is the set of the keys of its
    records with lower_count <= count <= upper_count, and the result holds, for every pair, how many keys both sets
    have -> (result, stats).  result is Counter.cooccurrence()'s dict (n_inputs, union, shared[n, n], in_exactly[n + 1],
    private[n]) plus records = the record count of every file; stats: k, canonical, records_in (records that passed the
    cut), distinct, slots, n_grow, mark_ms and cooc_ms (the two kernels' times, 0 without KM_COUNT_TIME_MERGE=1).

    Every header is read first (lib.jf_file_info, no GPU): no file, more than 32, a file that cannot be read, or one
    whose k or canonical differs from the first file's raises ValueError, naming the number of inputs, before a counter
    exists.  Every file crosses to the device once, whatever the number of pairs.  This project's own definitions
    (include/kmgpu.h)."""
    if isinstance(paths, (str, bytes)):
        paths = [paths]
    paths = list(paths)
    if not paths:
        raise ValueError("0 inputs: nothing to compare")
    if len(paths) > MAX_COMPARE_INPUTS:
        raise ValueError("%d inputs: one run compares at most %d" % (len(paths), MAX_COMPARE_INPUTS))
    infos = []
    for p in paths:
        try:
            infos.append(_lib.jf_file_info(p))
        except _lib.KmError as e:
            raise ValueError("input %d of %d: %s" % (len(infos) + 1, len(paths), e)) from None
    first = infos[0]
    for p, info in zip(paths, infos):
        if (info["k"], info["canonical"]) != (first["k"], first["canonical"]):
            raise ValueError("%s holds k=%d canonical=%s, but %s (the first of %d inputs) holds k=%d canonical=%s" % (
                p, info["k"], info["canonical"], paths[0], len(paths), first["k"], first["canonical"]))
    size = max(info["n_records"] for info in infos)
    counter = _lib.Counter(k=first["k"], canonical=first["canonical"], device=device, expected_distinct=size)
    try:
        for p in paths:
            counter.mark_jf(p, lower_count, upper_count)
        result = counter.cooccurrence()
        merged = counter.merge_stats()
        stats = counter.stats()
    finally:
        counter.close()
    result["records"] = [int(info["n_records"]) for info in infos]
    return result, {"k": first["k"], "canonical": first["canonical"], "records_in": merged["records_in"],
                    "distinct": stats["distinct"], "slots": stats["slots"], "n_grow": stats["n_grow"],
                    "mark_ms": merged["kernel_ms"], "cooc_ms": result.pop("kernel_ms")}


def _ratio(num, den):
    return "%.6f" % (num / den) if den else "NA"


def format_compare(names, result, what="pairs"):
    """The text of `compare` from a result of compare_files (n^2 numbers: built on the host), tab-separated:
      "pairs"     a header, then one row per pair i < j in the order (0,1), (0,2), .., (1,2), ..: a, b, distinct_a,
                  distinct_b, shared, jaccard = shared / (distinct_a + distinct_b - shared), contain_x = shared / distinct_x;
      "shared" / "jaccard"   the square matrix, the names as header row (behind an empty cell) and first column;
      "summary"   a header, then one row per input: input, records, distinct, private;
      "spectrum"  one row "m<TAB>kmers" for m = 1 .. n, without a header.
    Ratios are printed %.6f, or NA where the denominator is 0."""
    if what not in COMPARE_FORMS:
        raise ValueError("what %r is none of %s" % (what, ", ".join(repr(w) for w in COMPARE_FORMS)))
    names = [os.fsdecode(x) for x in names]
    n = int(result["n_inputs"])
    if len(names) != n:
        raise ValueError("%d names for %d inputs" % (len(names), n))
    shared = [[int(v) for v in row] for row in result["shared"]]
    jaccard = lambda i, j: _ratio(shared[i][j], shared[i][i] + shared[j][j] - shared[i][j])
    lines = []
    if what == "pairs":
        lines.append("a\tb\tdistinct_a\tdistinct_b\tshared\tjaccard\tcontain_a\tcontain_b")
        for i in range(n):
            for j in range(i + 1, n):
                s, da, db = shared[i][j], shared[i][i], shared[j][j]
                lines.append("%s\t%s\t%d\t%d\t%d\t%s\t%s\t%s" % (names[i], names[j], da, db, s, jaccard(i, j), _ratio(s, da),
                                                                 _ratio(s, db)))
    elif what in ("shared", "jaccard"):
        lines.append("\t".join([""] + names))
        for i in range(n):
            cells = [str(shared[i][j]) if what == "shared" else jaccard(i, j) for j in range(n)]
            lines.append("\t".join([names[i]] + cells))
    elif what == "summary":
        lines.append("input\trecords\tdistinct\tprivate")
        for i in range(n):
            lines.append("%s\t%d\t%d\t%d" % (names[i], int(result["records"][i]), shared[i][i], int(result["private"][i])))
    else:
        for m in range(1, n + 1):
            lines.append("%d\t%d" % (m, int(result["in_exactly"][m])))
    return "".join(line + "\n" for line in lines)


def histo_file(path, low=1, high=10000, increment=1, lower_count=1, upper_count=0xFFFFFFFF, device=0):
    """The histogram of the counts of a `binary/sorted` file and its four statistics, what `jellyfish histo -l low
    -h high -i increment` and `jellyfish stats` print -> (base, bins ndarray uint64, stats dict), as Counter.histo.
    The records stream through the GPU piece by piece (lib.jf_histo); a record takes part iff
    max(lower_count, 1) <= count <= upper_count.  This project's reading of the two commands, not checked against a
    run of Jellyfish."""
    return _lib.jf_histo(path, low=low, high=high, increment=increment, lower_count=lower_count,
                         upper_count=upper_count, device=device)


def format_histo(base, increment, bins, full=False):
    """The text of `histo`: one line "<label> <n>" per bin with n > 0, or per bin with full (the native writer)."""
    return _lib.histo_text(base, increment, bins, full=full)


def format_stats(stats):
    """The text of `stats`: Unique / Distinct / Total / Max_count, labels padded to one column (the native writer)."""
    return _lib.histo_stats_text(stats)


def write_histo(counter, path):
    """The default-layout histogram of a finished counter's records to `path`: what `histo` prints for the file
    written from them (count --histo, merge --histo)."""
    base, bins, _ = counter.histo()
    with open(path, "w") as fh:
        fh.write(format_histo(base, 1, bins))


@contextlib.contextmanager
def _text_out(out):
    """The descriptor of `out`: a path (opened here; a file this call created is removed again if the block fails,
    one that was there before is not), a file object with fileno() (flushed before its descriptor is handed over), or
    None for standard output."""
    if out is None:
        out = sys.stdout
    if isinstance(out, (str, bytes, os.PathLike)):
        created = not os.path.exists(out)
        fh = open(out, "wb")
        try:
            yield fh.fileno()
        except BaseException:
            fh.close()
            if created:
                with contextlib.suppress(OSError):
                    os.remove(out)
            raise
        fh.close()
    else:
        yield _lib.out_descriptor(out)


def dump_file(path, out=None, fmt="fasta", lower_count=0, upper_count=0xFFFFFFFF, device=0):
    """What `jellyfish dump [-c [-t]] [-L lower_count] [-U upper_count] db.jf` prints: the records of a
    `binary/sorted` file with lower_count <= count <= upper_count, in file order, as ">COUNT\nMER\n" ("fasta"),
    "MER COUNT\n" ("column") or "MER\tCOUNT\n" ("tab").  The records stream through the GPU piece by piece and the
    text is built there (lib.jf_dump); the host only writes it.  `out`: a path, a file object with fileno(), or None
    for standard output -> the dict of km_dump_stats_t.  This project's reading of the command, not checked against a
    run of Jellyfish."""
    _lib.jf_file_info(path)                               # a missing or foreign input fails before `out` is opened
    with _text_out(out) as fd:
        return _lib.jf_dump(path, fd, fmt=fmt, lower_count=lower_count, upper_count=upper_count, device=device)


_BASE_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _BASE_CODE[_c] = _BASE_CODE[_c + 32] = _i


def check_mers(mers, k):
    """Every MER argument of `query` has exactly k letters of ACGTacgt, else SystemExit naming it and its position."""
    for pos, mer in enumerate(mers, 1):
        text = mer if isinstance(mer, str) else bytes(mer).decode("latin-1")
        if len(text) != k or any(ch not in "ACGTacgt" for ch in text):
            raise SystemExit("ERROR: query: MER argument %d (%r) is not %d letters of ACGT" % (pos, text, k))


def _fasta_records(path):
    """The sequences of a FASTA file (plain or gzip), the lines of a record joined, as uint8 arrays."""
    fh, close = _open(path)
    try:
        lines = None
        for line in fh:
            if line.startswith(b">"):
                if lines is not None:
                    yield np.frombuffer(b"".join(lines), np.uint8)
                lines = []
            elif lines is not None:
                lines.append(line.strip())
        if lines is not None:
            yield np.frombuffer(b"".join(lines), np.uint8)
    finally:
        if close:
            fh.close()


def _windows(seq, k):
    """The packed k-mers of all windows of `seq` (uint8 text) in order; a window with a non-ACGT byte is skipped."""
    if seq.size < k:
        return np.zeros(0, np.uint64)
    codes = _BASE_CODE[seq]
    n = seq.size - k + 1
    keys = np.zeros(n, np.uint64)
    for j in range(k):                                   # k vectorised steps: the stated limit of `query -s`
        keys = (keys << np.uint64(2)) | (codes[j:j + n] & 3).astype(np.uint64)
    bad = np.concatenate(([0], np.cumsum(codes == 4)))
    return keys[bad[k:] == bad[:-k]]


def query_keys(k, canonical, mers=(), seq_files=()):
    """The key array `query` looks up, on the host: every k window of every record of the `seq_files` (FASTA), in the
    order given, then the `mers`; for a canonical database every key is min(key, reverse complement)."""
    from . import kmer as km
    check_mers(mers, k)
    parts = [_windows(seq, k) for path in seq_files for seq in _fasta_records(path)]
    if mers:
        text = "".join(m if isinstance(m, str) else bytes(m).decode("latin-1") for m in mers)
        # (the mers end to end, each checked above: every k-th window of that text is one of them)
        parts.append(_windows(np.frombuffer(text.encode("latin-1"), np.uint8), k)[::k])
    keys = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    if canonical and keys.size:
        keys = np.minimum(keys, km.revcomp(keys, k))
    return np.ascontiguousarray(keys, np.uint64)


def query_file(db_path, mers=(), seq_files=(), out=None, device=0):
    """What `jellyfish query db.jf [-s FILE]... [MER ...]` prints: "MER COUNT" per k-mer, 0 for one that is not in
    the table; the windows of the -s files first, in the order given, then the MER arguments.  For a canonical database
    the canonical k-mer is looked up and printed.  The records of the -s files go to the device as text, where their
    k-mers are cut, looked up and printed (Database.scan_text, one call per file); the MER arguments are packed here
    and go through Database.query_text -> the dict of km_dump_stats_t, summed over those calls.  This project's
    reading of the command, not checked against a run of Jellyfish."""
    info = _lib.jf_file_info(db_path)
    check_mers(mers, info["k"])                           # before the table is loaded
    keys = query_keys(info["k"], info["canonical"], mers=mers)
    files = [list(_fasta_records(path)) for path in seq_files]     # (a missing file fails before `out` is opened)
    db = _lib.Database.open(db_path)
    try:
        db.upload(device)
        with _text_out(out) as fd:
            stats = [db.scan_text(records, fd) for records in files]       # files first, then the mers
            if keys.size:
                stats.append(db.query_text(keys, fd))
        return {name: sum(st[name] for st in stats) for name in ("records_in", "records_out", "bytes_out", "pieces")}
    finally:
        db.close()


def write_records(path, keys, counts, k, canonical, cmdline=None):
    """Write (keys, counts) as a `binary/sorted`-framed file that kmjf_open / kmjf_load and the test oracle's
    reader load: 9 ASCII digits (the header length), a JSON header (format, key_len = 2k, counter_len = 4,
    canonical, ...) padded to 8 bytes, then one little-endian record per k-mer: ceil(2k / 8) key bytes and 4
    count bytes (12 bytes for k = 29..32).  Records are sorted by key, so the same records give the same bytes
    whatever order they arrive in.

    Real Jellyfish orders the records of such a file by its matrix hash and binary-searches that order; it
    could not query this file (write_jellyfish writes that order).  Readers that load all records (every reader
    here) do not care."""
    keys, counts = _lib._records(keys, counts)
    if not 2 <= int(k) <= 32:
        raise ValueError("k=%d unsupported" % k)
    order = np.argsort(keys, kind="stable")
    keys, counts = keys[order], counts[order]
    size = 16
    while size < 2 * keys.size:
        size <<= 1
    header = {
        "alignment": 8,
        "canonical": bool(canonical),
        "cmdline": list(cmdline) if cmdline is not None else ["km_amd", "count"],
        "counter_len": 4,
        "format": "binary/sorted",
        "key_len": 2 * int(k),
        "size": size,
        "val_len": 32,
    }
    text = json.dumps(header, separators=(",", ":"), sort_keys=True).encode("ascii")
    text += b"\0" * ((-(9 + len(text))) % 8)
    kb = (2 * int(k) + 7) // 8
    rec = np.zeros((keys.size, kb + 4), dtype=np.uint8)
    rec[:, :kb] = keys.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :kb]
    rec[:, kb:] = counts.astype("<u4").view(np.uint8).reshape(-1, 4)
    with open(path, "wb") as fh:
        fh.write(b"%09d" % len(text))
        fh.write(text)
        fh.write(rec.tobytes())


def write_jellyfish(path, keys, counts, k, canonical, cmdline=None, seed=0, device=0):
    """Write host-resident (keys, counts) as a `binary/sorted` file in Jellyfish's own record order: ascending
    pos = matrix1 . key over GF(2), ties by key ("File, Jellyfish order").  The header (size,
    matrix1 from `seed`, the keys of a real Jellyfish header minus the informational ones) comes from the
    library's own writer and the records are sorted on the GPU, so the file equals, byte for byte, what
    Counter.write_jf writes for the same records, cmdline and seed."""
    keys, counts = _lib._records(keys, counts)
    if not 2 <= int(k) <= 32:
        raise ValueError("k=%d unsupported" % k)
    header, columns, size_log2 = _lib.jf_header(k, canonical, keys.size, cmdline=cmdline, seed=seed)
    rec = _lib.jf_sort_records(columns, k, size_log2, keys, counts, device=device)
    with open(path, "wb") as fh:
        fh.write(header)
        fh.write(rec.tobytes())
