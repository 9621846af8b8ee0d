"""``km find_mutation`` / ``km min_cov`` / ``km linear_kmin`` drop-in command line, ``count``, ``merge``, ``compare``, ``histo``,
``stats``, ``dump``, ``query``, ``cov`` and ``bait``.

Same flags, same ``#key:value`` echo, same TSV and ``#Elapsed time`` trailer as
km/tools/find_mutation.py:17-60 and km/argparser/find_mutation.py:4-58, so the
output pipes into ``km find_report`` unchanged.  The GPU is selected with the
environment variable KM_DEVICE (no extra flags: the reference's tests index
output lines); KM_DEVICES=0,1,.. (or a torchrun launch) runs one
rank per GPU: targets sharded for ``find_mutation``, samples sharded for ``samples``.
"""

import argparse
import io
import os
import sys
import time

from . import report
from .finder import BatchFinder, NodeLimitExceeded
from .jellyfish import Jellyfish, default_device


def add_find_mutation_args(p):
    p.add_argument("-c", "--count", action="store", nargs="?", default=5, type=int,
                   help="Minimum occurence needed for exploration of alternative (default: -c 5)")
    p.add_argument("-p", "--ratio", action="store", nargs="?", default=0.05, type=float,
                   help="Minimum occurence ratio needed for exploration of alternative (default: -p 0.05)")
    p.add_argument("-s", "--steps", action="store", nargs="?", default=500, type=int,
                   help="Maximum steps to discover a new branch on a target sequence (default: -s 500)")
    p.add_argument("-b", "--branchs", action="store", nargs="?", default=10, type=int,
                   help="Maximum branchs until getback to target sequence (default: -b 10)")
    p.add_argument("-n", "--nodes", action="store", nargs="?", default=10000, type=int,
                   help="Maximum nodes queried from jellyfish database (default: -n 5000)")
    p.add_argument("-g", "--graphical", action="store_true", help="Display coverage graph.")
    p.add_argument("-v", "--verbose", action="store_true", help="Get more information.")
    p.add_argument("-vv", "--debug", action="store_true", help="Get much more information.")
    p.add_argument("target_fn", nargs="*", help="Filename of the target sequence file or directory.")
    p.add_argument("jellyfish_fn", help="Filename of the jellyfish database.")


def list_target_files(args):
    """km/utils/common.py:7-17 (a single directory argument expands in listdir order)."""
    if len(args) == 1 and os.path.isdir(args[0]):
        return [os.path.join(args[0], f) for f in os.listdir(args[0])]
    return list(args)


def read_target(path):
    """All FASTA records of a file, concatenated and upper-cased
    (km/utils/common.py:25-45, km/tools/find_mutation.py:39-43)."""
    chunks, seen_header = [], False
    with open(path) as fh:
        for line in fh:
            if line.startswith(">"):
                seen_header = True
            elif seen_header:
                chunks.append(line.strip())
    return "".join(chunks).upper()


def read_target_records(path):
    """The target as ``km linear_kmin`` reads it: km/utils/common.py:25-45 (file_2_seq) joined
    (km/tools/linear_kmin.py:55-56).  Records are joined and upper-cased, lines before the first header are
    ignored, consecutive headers count as one (the first is parsed).  The reference's errors are raised
    with its exception type and text: a header field (``>`` read as ``location=``, fields split at ``|``)
    without exactly one ``=`` fails its ``k, v = x.split("=")``; a header with no line after it ends its
    FASTA generator with ``RuntimeError: generator raised StopIteration``."""
    seqs = []
    header, lines = None, None

    def finish():
        for field in header.replace(">", "location=", 1).split("|"):
            k, v = field.split("=")                  # noqa: F841 - the unpack is the reference's check
        seqs.append("".join(lines).upper())

    with open(path) as fh:
        for line in fh:
            if line.startswith(">"):
                if lines is not None:
                    finish()
                    header, lines = None, None
                if header is None:
                    header = line.strip()
            elif header is not None:
                if lines is None:
                    lines = []
                lines.append(line.strip())
    if lines is not None:
        finish()
    elif header is not None:
        raise RuntimeError("generator raised StopIteration")
    return "".join(seqs)


def main_linear_kmin(args, out=None):
    """km/tools/linear_kmin.py:49-61: every target file read first, then ONE km_linear_kmin call for all of
    them.  Where a file fails to read, the rows of the files before it are printed, then the reference's
    exception is raised, as the reference (which prints while it goes) leaves it."""
    out = sys.stdout if out is None else out
    out.write("target_name\tlinear_kmin\n")
    if not args.target_fn:
        raise IndexError("list index out of range")    # km/utils/common.py:13 reads args[0]
    names, seqs, error = [], [], None
    for f in list_target_files(args.target_fn):
        try:
            seq = read_target_records(f)
        except Exception as e:                          # noqa: BLE001 - re-raised after the earlier rows
            error = e
            break
        if not seq.isascii():
            error = SystemExit("ERROR: %s: linear_kmin takes ASCII sequences only (km_amd compares bytes)" % f)
            break
        names.append(os.path.splitext(os.path.basename(f))[0])
        seqs.append(seq)
    if seqs:
        if args.start is None:                          # `-s` without a value: what `k_len = start - 1` raises
            raise TypeError("unsupported operand type(s) for -: 'NoneType' and 'int'")
        from . import lib
        kmin = lib.linear_kmin(seqs, start=args.start, device=default_device())
        out.write("".join("%s\t%d\n" % (name, k) for name, k in zip(names, kmin.tolist())))
    out.flush()
    if error is not None:
        raise error


CHUNK = 8192          # targets per GPU batch; rows are flushed after every batch
STREAM_ABOVE = 2_000_000   # catalogs larger than this are printed batch by batch (see main_find_mut)


def _verbose_lines(name_seq, raw, t, k, err, glog=None):
    """The INFO lines of km/utils/MutationFinder.py:101,126,160-161,183-187 and km/utils/Graph.py:198,231, in the
    reference's order (format "VERBOSE: %(message)s", km/tools/find_mutation.py:20-24).  Node indices and the two
    edge counts follow our canonical node order (target k-mers first); the reference's depend on its hash seed
    (its `if last_cur` skips whichever node has index 0: its 'Removed' count is ours or ours - 1).
    `glog`: Batch.graph_log() of the run."""
    from . import kmer as km
    seq = name_seq[1]
    n_ref = int(raw["n_ref"][t])
    x0 = int(raw["extra_off"][t])
    n_nodes = n_ref + int(raw["extra_off"][t + 1]) - x0
    err.write("VERBOSE: Ref. set contains %d kmers.\n" % n_ref)
    if glog is not None:
        for node in glog[2].get(t, ()):                     # where the walk met a k-mer of its own stack
            mer = seq[node:node + k] if node < n_ref else km.unpack(int(raw["extra_kmer"][x0 + node - n_ref]), k)
            err.write("VERBOSE: Broke loop at kmer: %s\n" % mer)
    err.write("VERBOSE: k-mer graph contains %d nodes.\n" % (n_nodes + 2))
    err.write("VERBOSE: BigBang=%d, BigCrunch=%d\n" % (n_nodes, n_nodes + 1))
    err.write("VERBOSE: Start kmer %s %d\n" % (seq[:k], 0))
    err.write("VERBOSE: End   kmer %s %d\n" % (seq[n_ref - 1:n_ref - 1 + k], n_ref - 1))
    if glog is not None:
        err.write("VERBOSE: Removed %d ref edges.\n" % int(glog[0][t]))
        err.write("VERBOSE: %d edges in non-ref edge set.\n" % int(glog[1][t]))
    err.write("VERBOSE: %d path(s) from BigBang to BigCrunch.\n"
              % (int(raw["path_off"][t + 1]) - int(raw["path_off"][t])))


def _print_rows(blocks, out):
    for rows in blocks:
        if isinstance(rows, NodeLimitExceeded):
            out.flush()
            sys.exit(str(rows))
        if isinstance(rows, BaseException):        # what the reference raises while naming a variant
            raise rows
        for row in rows:
            out.write(row + "\n")
    out.flush()


def main_find_mut(args, out=None, err=None):
    out = sys.stdout if out is None else out
    err = sys.stderr if err is None else err
    t0 = time.time()
    if args.graphical:
        sys.exit("ERROR: -g/--graphical (matplotlib coverage plots, km/utils/MutationFinder.py:591-611) "
                 "is not supported by km_amd")
    from . import dist as kd
    rank, _local_rank, world = kd.env_world()
    if world > 1:
        import torch
        dev = kd.local_device()
        torch.cuda.set_device(dev)
        kd.init(os.environ.get("KM_DIST_BACKEND", "nccl"), torch.device("cuda", dev))
    if rank == 0:
        for key, val in vars(args).items():
            out.write("#" + str(key) + ":" + str(val) + "\n")
    targets = []
    for f in list_target_files(args.target_fn):
        name = os.path.splitext(os.path.basename(f))[0]
        targets.append((name, read_target(f)))
    params = {"ratio": args.ratio, "count": args.count, "steps": args.steps, "branchs": args.branchs,
              "nodes": args.nodes}
    if world > 1:
        # one process per GPU (torchrun, or KM_DEVICES=0,1,.. which starts the ranks): targets are
        # sharded, the database records cross the links once, rank 0 prints in target order
        if (args.verbose or args.debug) and rank == 0:
            err.write("km_amd: -v / -d lines are printed by single-process runs only (the ranks return rows, not node lists)\n")
        blocks = kd.find_mutation_sharded(targets, args.jellyfish_fn, params=params)
        if rank == 0:
            out.write(report.HEADER + "\n")
            _print_rows(blocks, out)
            out.write("#Elapsed time:" + str(time.time() - t0) + "\n")
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
        return
    jf = Jellyfish(args.jellyfish_fn, cutoff=args.ratio, n_cutoff=args.count)
    out.write(report.HEADER + "\n")
    finder = BatchFinder(jf, args.steps, args.branchs, args.nodes)
    # The reference builds every RefSeq before the first MutationFinder (km/tools/find_mutation.py:37-45):
    # a target that is too short, has a non-ACGT base or repeats a k-mer stops the run BEFORE any row is
    # printed.  Those errors come out of the GPU batch here, so with more than one batch the rows are
    # held back until every batch has passed that check (up to STREAM_ABOVE targets; beyond that — some
    # GB of text — batches are printed as they finish and such an error may follow rows already out).
    hold = CHUNK < len(targets) <= STREAM_ABOVE
    held = []
    sink = out

    def release():
        for text in held:
            out.write(text)
        del held[:]

    for lo in range(0, len(targets), CHUNK):
        part = targets[lo:lo + CHUNK]
        if hold:
            sink = io.StringIO()
        try:
            finder.write_rows(part, sink)          # native reporting (km_report_rows), one write per batch
        except NodeLimitExceeded as e:
            if hold:
                held.append(sink.getvalue())
                release()                          # the rows of the earlier targets, then the reference's exit
            out.flush()
            sys.exit(str(e))
        except BaseException as e:
            if hold and not getattr(e, "km_input_error", False):
                held.append(sink.getvalue())
                release()                          # an exception while naming a variant: the earlier rows are out
                out.flush()
            raise
        if hold:
            held.append(sink.getvalue())
        if args.verbose or args.debug:
            glog = finder.graph_log(len(part))
            for t in range(len(part)):
                _verbose_lines(part[t], finder.last_raw, t, jf.k, err, glog)
        if not hold:
            out.flush()
    release()
    out.flush()
    out.write("#Elapsed time:" + str(time.time() - t0) + "\n")


def main_samples(args, out=None):
    """catalog x N samples, sample-sharded over the ranks (km_amd.dist.sample_matrix): one TSV
    stream per target for `km find_report -t <target.fa> -f table`, replacing the loop of
    example/run_leucegene.sh:29-35."""
    out = sys.stdout if out is None else out
    from . import dist as kd
    rank, _local_rank, world = kd.env_world()
    if world > 1:
        import torch
        dev = kd.local_device()
        torch.cuda.set_device(dev)
        kd.init(os.environ.get("KM_DIST_BACKEND", "nccl"), torch.device("cuda", dev))
    params = {"ratio": args.ratio, "count": args.count, "steps": args.steps, "branchs": args.branchs,
              "nodes": args.nodes}
    files = kd.sample_matrix(list(args.jellyfish_fn), list_target_files(args.targets), args.out_dir, params)
    if rank == 0:
        for f in files:
            out.write(f + "\n")
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def main_min_cov(args, out=None):
    """km/tools/min_cov.py:10-25 over the batched probe kernel."""
    out = sys.stdout if out is None else out
    dbs = list_target_files(args.jellyfish_fn)
    seq = args.target_fn
    if os.path.isfile(seq):
        seq = read_target(seq)
    from . import common
    out.write("DB\tcount\tlength\tmin\tmax\tmean\tkmer_nb\tkmer_nb_0\n")
    for db in dbs:
        res = common.get_cov(db, seq)
        common.close(db)                 # one database in HBM at a time, as the reference holds one (min_cov.py:18-25)
        out.write("%s\t%d\t%d\t%d\t%d\t%.2f\t%d\t%d\n" % ((db,) + tuple(res)))


COV_HEADER = "DB\ttarget\trecord\tcount\tlength\tmin\tmax\tmean\tkmer_nb\tkmer_nb_0\tkmer_nb_skipped\n"


def cov_row(db, target, record, length, c):
    """One line of `cov`: the numbers of min_cov in its formats and the skipped windows behind them; a record without
    a valid window has NA for min, max and mean."""
    n, total = int(c["n_kmers"]), int(c["total"])
    head = "%s\t%s\t%d\t%d\t%d\t" % (db, target, record, total, length)
    mid = "%d\t%d\t%.2f" % (int(c["min"]), int(c["max"]), float(total) / n) if n else "NA\tNA\tNA"
    return head + mid + "\t%d\t%d\t%d\n" % (n, int(c["n_zero"]), int(c["n_skipped"]))


def main_cov(args, out=None):
    """`cov [-o out.tsv] -t <targets.fa ...|dir> <db.jf> [<db.jf> ...]`: the coverage of EVERY record of the target
    files in every database, one row per database and record, database-major.  Where `min_cov` joins the records of
    one file into one sequence and stops at a non-ACGT letter, here a record is a sequence of its own and a window
    with such a letter is skipped and counted.  All records of all files go to the device in one call per database
    (common.cov_many); one database is in HBM at a time."""
    from . import common
    from . import count as kc
    files = list_target_files(args.targets)
    names, seqs = [], []
    for path in files:                   # everything is read before anything touches the GPU
        stem = os.path.splitext(os.path.basename(path))[0]
        for i, seq in enumerate(kc._fasta_records(path), 1):
            names.append((stem, i))
            seqs.append(seq)
    fh = open(args.output, "w") if args.output else None
    out = fh if fh is not None else (sys.stdout if out is None else out)
    try:
        out.write(COV_HEADER)
        for db in args.jellyfish_fn:
            cov = common.cov_many(db, seqs)
            common.close(db)
            for (stem, i), seq, c in zip(names, seqs, cov):
                out.write(cov_row(db, stem, i, len(seq), c))
    finally:
        if fh is not None:
            fh.close()


def main_count(args, err=None):
    """`jellyfish count -m K [-C] -L N -s SIZE -o OUT reads..` on the GPU (km_amd.count): the k-mers of the read
    files counted on the device, the records with count >= -L written to OUT (read by every tool here).  The file
    is sorted by key, which real Jellyfish could not query (km_amd.count.write_records); with --jellyfish-order
    it is sorted on the device into Jellyfish's own record order and written from there (Counter.write_jf).
    -Q CHAR (Jellyfish's --min-qual-char, as in example/run_leucegene.sh:22): FASTQ files are parsed on the GPU and
    a base whose quality character is below CHAR is read as N (Counter.add_fastq).
    --if FILE (Jellyfish's "count only k-mers in this file", may repeat): only the k-mers of the FILEs are counted
    (FASTA records, or the keys of a .jf of the same -m and -C; Counter.set_filter), each of them is a record and -L 0
    writes the whole set with its zeros; -s is ignored.  This project's reading of --if, not checked against a run of
    Jellyfish.
    --solid N (this project's own flag; the job of `jellyfish bc` + `count --bc`): the reads are read twice, a first
    pass notes their k-mers in a Bloom sketch sized for N distinct k-mers, the second counts only those seen again
    (Counter.set_sketch).  The records are those of the same command without --solid at -L max(2, -L), which is the
    -L that is applied and written into the header; the table never holds the k-mers seen once."""
    err = sys.stderr if err is None else err
    from . import count as kc
    only = None
    if args.only:
        try:                                            # (before the GPU is touched and before the output exists)
            only = kc.filter_keys(args.only, args.mer_len, args.canonical)
        except (OSError, ValueError) as e:
            sys.exit("ERROR: count: %s" % e)
    solid = args.solid
    lower_count = args.lower_count if solid is None else max(2, args.lower_count)
    try:
        db, stats, counter = kc.count_files(args.reads, k=args.mer_len, canonical=args.canonical,
                                            lower_count=lower_count, device=default_device(),
                                            expected_distinct=args.size, keep_counter=True,
                                            min_qual_char=args.min_qual_char, only=only, solid=solid)
    except ValueError as e:
        if solid is None:
            raise
        sys.exit("ERROR: count: %s" % e)
    cmdline = ["km_amd", "count", "-m", str(args.mer_len)] + (["-C"] if args.canonical else []) + [
        "-L", str(lower_count), "-s", str(args.size)] + (
        ["-Q", args.min_qual_char] if args.min_qual_char is not None else []) + (
        [a for f in args.only or () for a in ("--if", f)]) + (
        ["--solid", str(solid)] if solid is not None else []) + (
        ["--jellyfish-order"] if args.jellyfish_order else []) + ["-o", args.output] + list(args.reads)
    try:
        if args.jellyfish_order:
            counter.write_jf(args.output, cmdline=cmdline)
        else:
            keys, counts = counter.records()
        if args.histo:
            kc.write_histo(counter, args.histo)
    finally:
        counter.close()
        db.close()
    for key in ("bases", "kmers", "distinct", "slots", "n_grow"):
        err.write("#%s:%d\n" % (key, stats[key]))
    if args.min_qual_char is not None:
        err.write("#min_qual_char:%s\n" % args.min_qual_char)
    if only is not None:
        err.write("#filter_kmers:%d\n#kmers_hit:%d\n#filter_tier:%s\n" % (
            stats["filter_kmers"], stats["kmers_hit"], stats["filter_tier"]))
    if solid is not None:
        for key in ("lower_count", "sketch_words", "sketch_bits_1", "sketch_bits_2", "kmers_admitted"):
            err.write("#%s:%d\n" % (key, stats[key]))
    if not args.jellyfish_order:
        kc.write_records(args.output, keys, counts, args.mer_len, args.canonical, cmdline=cmdline)
    if args.dump:                                       # of the file just written: its records in its order
        kc.dump_file(args.output, out=args.dump, fmt="column", device=default_device())


def main_merge(args, err=None):
    """Several .jf files of one k into one on the GPU (km_amd.count.merge_files): per k-mer the counts are summed
    (saturating at 2^32 - 1) or, with --max, their maximum is kept; --min keeps the k-mers that every input holds, with
    their minimum count, --subtract the records of the first input whose k-mer no later input holds.  The records of
    the result with -L <= count <= -U are written to OUT as `count` writes them (sorted by key, or Jellyfish's own
    order with --jellyfish-order).  With one input it is a filter and re-writer.  This project's own semantics, not
    checked against `jellyfish merge`."""
    err = sys.stderr if err is None else err
    from . import count as kc
    mode = "max" if args.max else "intersect" if args.min else "subtract" if args.subtract else "sum"
    upper = 0xFFFFFFFF if args.upper_count is None else args.upper_count
    db, stats, counter = kc.merge_files(args.inputs, mode=mode, lower_count=args.lower_count, upper_count=upper,
                                        device=default_device(), keep_counter=True)
    # (-U is named only when given: a file written by an invocation without it keeps its bytes)
    cmdline = ["km_amd", "merge", "-L", str(args.lower_count)] + (
        ["-U", str(args.upper_count)] if args.upper_count is not None else []) + (["--max"] if args.max else []) + (
        ["--min"] if args.min else []) + (["--subtract"] if args.subtract else []) + (
        ["--jellyfish-order"] if args.jellyfish_order else []) + ["-o", args.output] + list(args.inputs)
    try:
        if args.jellyfish_order:
            counter.write_jf(args.output, cmdline=cmdline)
        else:
            keys, counts = counter.records()
        if args.histo:
            kc.write_histo(counter, args.histo)
    finally:
        counter.close()
        db.close()
    for key in ("distinct", "slots", "n_grow", "records_in"):
        err.write("#%s:%d\n" % (key, stats[key]))
    err.write("#mode:%s\n" % mode)
    if mode in ("intersect", "subtract"):
        err.write("#records_out:%d\n" % stats["records_out"])
    if not args.jellyfish_order:
        kc.write_records(args.output, keys, counts, stats["k"], stats["canonical"], cmdline=cmdline)
    if args.dump:                                       # of the file just written: its records in its order
        kc.dump_file(args.output, out=args.dump, fmt="column", device=default_device())


def main_compare(args, out=None, err=None):
    """How up to 32 .jf files of one k relate, counted on the GPU (km_amd.count.compare_files): file i is the set of its
    k-mers with -L <= count <= -U, and every file crosses to the device once, whatever the number of pairs.  By default
    a header and one row per pair i < j: a, b, distinct_a, distinct_b, shared, jaccard, contain_a, contain_b; --matrix
    prints the square matrix of shared counts or of Jaccard indices instead.  --summary FILE gets one row per input
    (input, records, distinct, private), --spectrum FILE "m<TAB>kmers" for the k-mers held by exactly m inputs.  One input
    is legal and gives no pair rows.  This project's own semantics."""
    err = sys.stderr if err is None else err
    from . import count as kc
    from .lib import KmError
    try:
        result, stats = kc.compare_files(args.inputs, lower_count=args.lower_count, upper_count=args.upper_count,
                                         device=default_device())
    except (ValueError, KmError) as e:
        sys.exit("ERROR: compare: %s" % e)
    n = result["n_inputs"]
    for key, value in (("inputs", n), ("records_in", stats["records_in"]), ("union", result["union"]),
                       ("core", int(result["in_exactly"][n])), ("slots", stats["slots"]), ("n_grow", stats["n_grow"])):
        err.write("#%s:%d\n" % (key, value))
    _write_text(kc.format_compare(args.inputs, result, args.matrix or "pairs"), args.output, out)
    if args.summary:
        _write_text(kc.format_compare(args.inputs, result, "summary"), args.summary)
    if args.spectrum:
        _write_text(kc.format_compare(args.inputs, result, "spectrum"), args.spectrum)


def _write_text(text, path, out=None):
    if path:
        with open(path, "w") as fh:
            fh.write(text)
    else:
        out = sys.stdout if out is None else out
        out.write(text)
        out.flush()


def main_histo(args, out=None):
    """`jellyfish histo -l LOW -h HIGH -i INC [-f] db.jf` on the GPU (km_amd.count.histo_file): one line
    "<count> <k-mers>" per bin; counts above HIGH + INC collect in the last bin.  -L / -U look only at the records
    with -L <= count <= -U.  This project's reading of the command, not checked against a run of Jellyfish."""
    from . import count as kc
    base, bins, _ = kc.histo_file(args.db, low=args.low, high=args.high, increment=args.increment,
                                  lower_count=args.lower_count, upper_count=args.upper_count, device=default_device())
    _write_text(kc.format_histo(base, args.increment, bins, full=args.full), args.output, out)


def main_stats(args, out=None):
    """`jellyfish stats [-L N] [-U N] db.jf` on the GPU: Unique (count 1), Distinct, Total (sum of counts) and
    Max_count of the records with -L <= count <= -U.  This project's reading, not checked against Jellyfish."""
    from . import count as kc
    _, _, stats = kc.histo_file(args.db, lower_count=args.lower_count, upper_count=args.upper_count,
                                device=default_device())
    _write_text(kc.format_stats(stats), args.output, out)


def main_dump(args):
    """`jellyfish dump [-c] [-t] [-L N] [-U N] [-o FILE] db.jf` on the GPU (km_amd.count.dump_file): the records of
    the file in file order, ">COUNT" and MER on two lines, or "MER COUNT" with -c ("MER<tab>COUNT" with -c -t); -L / -U
    print only the records with -L <= count <= -U.  The library writes straight to the output's descriptor.  This
    project's reading of the command, not checked against a run of Jellyfish."""
    from . import count as kc
    from .lib import KmError
    fmt = "fasta" if not args.column else "tab" if args.tab else "column"
    try:
        kc.dump_file(args.db, out=args.output, fmt=fmt, lower_count=args.lower_count, upper_count=args.upper_count,
                     device=default_device())
    except KmError as e:
        sys.exit("ERROR: dump: %s" % e)


def main_query(args):
    """`jellyfish query [-s FILE]... [-o FILE] db.jf [MER ...]` on the GPU (km_amd.count.query_file): "MER COUNT" per
    k-mer, the k-mers of the -s FASTA files first, then the MER arguments; the canonical k-mer for a canonical
    database.  This project's reading of the command, not checked against a run of Jellyfish."""
    from . import count as kc
    from .lib import KmError
    try:
        kc.query_file(args.db, mers=args.mers, seq_files=args.sequence, out=args.output, device=default_device())
    except KmError as e:
        sys.exit("ERROR: query: %s" % e)


def main_bait(args, err=None):
    """`bait [-n N] [-v] [-Q CHAR] [-o out.fq] (-t targets.fa [-t ...] [-m K] | -d db.jf) reads.fq[.gz] ...`: the reads
    with at least N k-mers of the bait table (with -v: the others), byte for byte and in input order, found and gathered
    on the GPU (km_amd.count.select_files).  The table: the canonical k-mers of the FASTA records of the -t files (a
    directory expands to its files), counted here with count_files, or an existing -d file with its own k and
    canonical setting.  Standard output carries the records only; the figures go to standard error.

    Paired-end: `bait ... -1 R1.fq[.gz] [-1 ...] -2 R2.fq[.gz] [-2 ...] -o out_1.fq -O out_2.fq [--pair-rule any|both|sum]
    [--no-name-check]` keeps or drops the mates of a pair together (km_amd.count.select_pair_files), so the two outputs
    line up record for record; the figures are then #pairs_in, #pairs_out, #bytes_in_1/2, #bytes_out_1/2, #pieces and
    #pair_rule.

    One file per label: `bait --split-dir DIR ...` is main_bait_split."""
    err = sys.stderr if err is None else err
    from . import count as kc
    from . import lib
    if args.split_dir is not None:
        return main_bait_split(args, err)
    db = None
    try:
        if args.db is not None:
            lib.jf_file_info(args.db)                     # a missing or foreign file fails before anything is opened
            db = lib.Database.open(args.db)
            db.upload(default_device())
        else:
            files = [f for t in args.targets for f in list_target_files([t])]
            db, _ = kc.count_files(files, k=31 if args.mer_len is None else args.mer_len, canonical=True,
                                   device=default_device())
        n_kmers = int(db.info.n_records)
        if args.mate1:
            stats = kc.select_pair_files(db, args.mate1, args.mate2, args.output, args.output2, min_hits=args.min_hits,
                                         invert=args.invert, min_qual_char=args.min_qual_char,
                                         rule=args.pair_rule or "any", check_names=not args.no_name_check)
        else:
            stats = kc.select_files(db, args.reads, out=args.output, min_hits=args.min_hits, invert=args.invert,
                                    min_qual_char=args.min_qual_char)
    except (lib.KmError, ValueError, OSError) as e:
        sys.exit("ERROR: bait: %s" % e)
    finally:
        if db is not None:
            db.close()
    err.write("#bait_kmers:%d\n" % n_kmers)
    if args.mate1:
        err.write("#pairs_in:%d\n#pairs_out:%d\n" % (stats["pairs_in"], stats["pairs_out"]))
        for key in ("bytes_in", "bytes_out"):
            for mate in (0, 1):
                err.write("#%s_%d:%d\n" % (key, mate + 1, stats[key][mate]))
        err.write("#pieces:%d\n#pair_rule:%s\n" % (stats["pieces"], args.pair_rule or "any"))
        return
    for key, name in (("records_in", "reads_in"), ("records_out", "reads_out"), ("bytes_in", "bytes_in"),
                      ("bytes_out", "bytes_out"), ("pieces", "pieces")):
        err.write("#%s:%d\n" % (name, stats[key]))


def split_labels(args):
    """The labels of `bait --split-dir`, on the host and without a GPU -> (k, [dict as count.rows_labels gives them]).
    With -t: one label per target file after directory expansion, named by the file's stem (find_mutation's Query),
    its keys the canonical k-mers of the file's records; two files with one stem are a ValueError."""
    import numpy as np
    from . import count as kc
    k = 31 if args.mer_len is None else args.mer_len
    if args.rows is not None:
        return k, kc.rows_labels(sys.stdin if args.rows == "-" else args.rows, k, with_ref=args.with_ref,
                                 info="vs_ref" if args.info is None else args.info)
    files = [f for t in args.targets for f in list_target_files([t])]
    labels, seen = [], {}
    for f in files:
        stem = os.path.splitext(os.path.basename(f))[0]
        if stem in seen:
            raise ValueError("%s and %s have one stem, %s: every label needs a name of its own" % (seen[stem], f, stem))
        seen[stem] = f
        labels.append({"name": stem, "query": "", "type": "", "variant_name": "", "allele": "target",
                       "keys": np.unique(kc.query_keys(k, True, seq_files=[f]))})
    if len(labels) > kc.MAX_LABELS:
        raise ValueError("%d target files give %d labels, more than the %d of one run: split the run" % (
            len(files), len(labels), kc.MAX_LABELS))
    return k, labels


def main_bait_split(args, err):
    """`bait --split-dir DIR (-t targets [-t ...] | --rows TSV [--with-ref] [-i INFO]) [-m K] [-n N] [-Q C] reads ...`:
    one FASTQ per label in DIR, DIR/<label>.fq, from one pass over the reads (km_amd.count.select_label_files), and
    DIR/labels.tsv with label, query, type, variant_name, allele, kmers, reads, bytes per label.  A read that carries
    k-mers of several labels is in each of their files.  The figures go to standard error."""
    from . import count as kc
    from . import lib
    db = None
    try:
        k, labels = split_labels(args)
        if not labels:
            raise ValueError("no labels: %s" % ("no row of the TSV was taken" if args.rows is not None else "no target files"))
        db = kc.label_table([lab["keys"] for lab in labels], k, True, device=default_device())
        n_kmers = int(db.info.n_records)
        stats = kc.select_label_files(db, [lab["name"] for lab in labels], args.reads, args.split_dir,
                                      min_hits=args.min_hits, min_qual_char=args.min_qual_char)
        with open(os.path.join(args.split_dir, "labels.tsv"), "w") as fh:
            fh.write("label\tquery\ttype\tvariant_name\tallele\tkmers\treads\tbytes\n")
            for lab, reads, nbytes in zip(labels, stats["records_out"], stats["bytes_out"]):
                fh.write("%s\t%s\t%s\t%s\t%s\t%d\t%d\t%d\n" % (lab["name"], lab["query"], lab["type"], lab["variant_name"],
                                                             lab["allele"], lab["keys"].size, reads, nbytes))
    except (lib.KmError, ValueError, OSError) as e:
        sys.exit("ERROR: bait: %s" % e)
    finally:
        if db is not None:
            db.close()
    err.write("#labels:%d\n#bait_kmers:%d\n" % (len(labels), n_kmers))
    for key, name in (("records_in", "reads_in"), ("records_any", "reads_any"), ("records_multi", "reads_multi"),
                      ("bytes_in", "bytes_in"), ("pieces", "pieces"), ("gather_passes", "gather_passes")):
        err.write("#%s:%d\n" % (name, stats[key]))


def _min_hits(text):
    """argparse type of bait's -n: a 32-bit count of at least 1."""
    value = _count32(text)
    if value < 1:
        raise argparse.ArgumentTypeError("expected at least 1, got %r" % text)
    return value


def _count_value(text):
    """argparse type of the count-valued options of histo / stats: a non-negative integer."""
    value = int(text)
    if value < 0:
        raise argparse.ArgumentTypeError("expected a non-negative integer, got %r" % text)
    return value


def _count32(text):
    """argparse type of -L / -U of histo / stats: a count, 0 .. 2^32 - 1."""
    value = _count_value(text)
    if value > 0xFFFFFFFF:
        raise argparse.ArgumentTypeError("counts are 32-bit: at most 4294967295, got %r" % text)
    return value


def _one_char(text):
    """argparse type of -Q: exactly one character that is one byte."""
    if len(text) != 1 or ord(text) > 255:
        raise argparse.ArgumentTypeError("expected exactly one character, got %r" % text)
    return text


def build_parser():
    parser = argparse.ArgumentParser(prog="km")
    sub = parser.add_subparsers(dest="_cmd")
    fm = sub.add_parser("find_mutation")
    add_find_mutation_args(fm)
    mc = sub.add_parser("min_cov")
    mc.add_argument("target_fn")
    mc.add_argument("jellyfish_fn", nargs="*")
    sm = sub.add_parser("samples", help="catalog x N samples -> one TSV stream per target (find_report -f table)")
    for flag, dest, default, typ in (("-c", "--count", 5, int), ("-p", "--ratio", 0.05, float),
                                     ("-s", "--steps", 500, int), ("-b", "--branchs", 10, int),
                                     ("-n", "--nodes", 10000, int)):
        sm.add_argument(flag, dest, default=default, type=typ)
    sm.add_argument("-t", "--targets", nargs="+", required=True, help="target FASTA files or one directory")
    sm.add_argument("-o", "--out-dir", required=True)
    sm.add_argument("jellyfish_fn", nargs="+", help="one .jf per sample")
    lk = sub.add_parser("linear_kmin")
    lk.add_argument("-s", "--start", help="starting length (default: -s 10)", action="store", nargs="?",
                    default=10, type=int)
    lk.add_argument("target_fn", help="Filename of the reference sequence file or directory.", nargs="*")
    ct = sub.add_parser("count", help="count the k-mers of FASTA / FASTQ reads on the GPU -> a .jf the other tools read")
    ct.add_argument("-m", "--mer-len", type=int, default=31, help="length of mer (default: -m 31)")
    ct.add_argument("-C", "--canonical", action="store_true", help="count both strands, canonical representation")
    ct.add_argument("-L", "--lower-count", type=int, default=1, help="don't output k-mers with count < lower-count")
    ct.add_argument("-s", "--size", type=int, default=0,
                    help="expected number of distinct k-mers (0: grow as needed); ignored with --if, whose set sizes the table")
    ct.add_argument("-o", "--output", default="mer_counts.jf", help="output file (default: mer_counts.jf)")
    ct.add_argument("--jellyfish-order", action="store_true",
                    help="write the records in Jellyfish's own order (matrix position, then key), sorted on the GPU")
    ct.add_argument("-Q", "--min-qual-char", type=_one_char, default=None, metavar="CHAR",
                    help="a base of a FASTQ read whose quality character is below CHAR is read as N (FASTQ is then "
                         "parsed on the GPU; no effect on FASTA)")
    ct.add_argument("--if", dest="only", action="append", default=None, metavar="FILE",
                    help="count only the k-mers of FILE (FASTA, or a .jf of the same -m / -C); may be repeated; every "
                         "k-mer of the set is a record, so -L 0 writes those that never occurred with count 0")
    ct.add_argument("--solid", type=_count_value, default=None, metavar="N",
                    help="keep the k-mers seen once out of the table: read the reads twice, note their k-mers in a Bloom "
                         "sketch sized for N expected distinct k-mers, count those seen again; -L is at least 2 then, and "
                         "-s speaks of the k-mers seen twice; not with --if or standard input")
    ct.add_argument("--histo", metavar="FILE", default=None,
                    help="also write the histogram of the counts written (after -L), as `histo OUT` prints it")
    ct.add_argument("--dump", metavar="FILE", default=None,
                    help="also write the records written (after -L) as text: byte for byte what `dump -c OUT` prints")
    ct.add_argument("reads", nargs="+", help="FASTA or FASTQ files, plain or gzip; - is stdin")
    mg = sub.add_parser("merge", help="sum (or --max), intersect (--min) or --subtract several .jf files of one k on the GPU -> one .jf")
    mg.add_argument("-L", "--lower-count", type=int, default=1, help="don't output k-mers with a merged count < lower-count")
    mg.add_argument("-U", "--upper-count", type=_count32, default=None,
                    help="don't output k-mers with a merged count > upper-count (default: no upper cut)")
    mg.add_argument("--max", action="store_true", help="keep the maximum count per k-mer instead of the sum")
    mg.add_argument("--min", action="store_true",
                    help="intersect: keep the k-mers that every input holds, with their minimum count")
    mg.add_argument("--subtract", action="store_true",
                    help="keep the records of the first input whose k-mer no later input holds")
    mg.add_argument("-o", "--output", default="mer_counts_merged.jf", help="output file (default: mer_counts_merged.jf)")
    mg.add_argument("--jellyfish-order", action="store_true",
                    help="write the records in Jellyfish's own order (matrix position, then key), sorted on the GPU")
    mg.add_argument("--histo", metavar="FILE", default=None,
                    help="also write the histogram of the counts written (after -L), as `histo OUT` prints it")
    mg.add_argument("--dump", metavar="FILE", default=None,
                    help="also write the records written (after -L) as text: byte for byte what `dump -c OUT` prints")
    mg.add_argument("inputs", nargs="+", metavar="db.jf", help="binary/sorted files of one k and one canonical setting")
    cp = sub.add_parser("compare", help="the k-mers that up to 32 .jf files of one k share, pair by pair, counted on the GPU")
    cp.add_argument("-L", "--lower-count", type=_count32, default=1, help="a file holds a k-mer only with count >= lower-count")
    cp.add_argument("-U", "--upper-count", type=_count32, default=0xFFFFFFFF, help="a file holds a k-mer only with count <= upper-count")
    cp.add_argument("--matrix", choices=("shared", "jaccard"), default=None,
                    help="print the square matrix of shared k-mers or of Jaccard indices instead of the rows per pair")
    cp.add_argument("--summary", metavar="FILE", default=None, help="also write one row per input: input, records, distinct, private")
    cp.add_argument("--spectrum", metavar="FILE", default=None,
                    help="also write m<TAB>kmers for m = 1 .. n: the k-mers that exactly m inputs hold")
    cp.add_argument("-o", "--output", default=None, help="output file (default: standard output)")
    cp.add_argument("inputs", nargs="+", metavar="db.jf", help="binary/sorted files of one k and one canonical setting, at most 32")
    hs = sub.add_parser("histo", add_help=False,
                        help="histogram of the counts of a .jf file, on the GPU (-h is --high as in Jellyfish: help is "
                             "--help only)")
    hs.add_argument("--help", action="help", help="show this help message and exit (-h is --high, as in Jellyfish)")
    hs.add_argument("-l", "--low", type=_count_value, default=1, help="low count value of the histogram (default: -l 1)")
    hs.add_argument("-h", "--high", type=_count_value, default=10000, help="high count value of the histogram (default: -h 10000)")
    hs.add_argument("-i", "--increment", type=_count_value, default=1, help="width of a bin (default: -i 1)")
    hs.add_argument("-f", "--full", action="store_true", help="print every bin, the empty ones too")
    hs.add_argument("-L", "--lower-count", type=_count32, default=1, help="ignore k-mers with count < lower-count")
    hs.add_argument("-U", "--upper-count", type=_count32, default=0xFFFFFFFF, help="ignore k-mers with count > upper-count")
    hs.add_argument("-o", "--output", default=None, help="output file (default: standard output)")
    hs.add_argument("db", metavar="db.jf", help="a binary/sorted file")
    ss = sub.add_parser("stats", help="Unique / Distinct / Total / Max_count of a .jf file, on the GPU")
    ss.add_argument("-L", "--lower-count", type=_count32, default=1, help="ignore k-mers with count < lower-count")
    ss.add_argument("-U", "--upper-count", type=_count32, default=0xFFFFFFFF, help="ignore k-mers with count > upper-count")
    ss.add_argument("-o", "--output", default=None, help="output file (default: standard output)")
    ss.add_argument("db", metavar="db.jf", help="a binary/sorted file")
    dp = sub.add_parser("dump", help="the k-mers and counts of a .jf file as text, built on the GPU")
    dp.add_argument("-c", "--column", action="store_true", help="column format: MER COUNT on one line")
    dp.add_argument("-t", "--tab", action="store_true", help="with -c: a tab between MER and COUNT")
    dp.add_argument("-L", "--lower-count", type=_count32, default=0, help="don't print k-mers with count < lower-count")
    dp.add_argument("-U", "--upper-count", type=_count32, default=0xFFFFFFFF, help="don't print k-mers with count > upper-count")
    dp.add_argument("-o", "--output", default=None, help="output file (default: standard output)")
    dp.add_argument("db", metavar="db.jf", help="a binary/sorted file")
    qr = sub.add_parser("query", help="the counts of given k-mers in a .jf file, looked up and printed on the GPU")
    qr.add_argument("-s", "--sequence", action="append", default=[], metavar="FILE",
                    help="query every k-mer of this FASTA file (plain or gzip); may be given several times")
    qr.add_argument("-o", "--output", default=None, help="output file (default: standard output)")
    qr.add_argument("db", metavar="db.jf", help="a binary/sorted file")
    qr.add_argument("mers", nargs="*", metavar="MER", help="k-mers of the file's k, letters of ACGT")
    cv = sub.add_parser("cov", help="coverage of every record of the target files in every database, k-mers cut on the GPU")
    cv.add_argument("-t", "--targets", nargs="+", required=True,
                    help="target FASTA files or one directory; when the databases follow directly, the targets end at "
                         "the first argument that is neither a directory nor a file that starts like FASTA")
    cv.add_argument("-o", "--output", default=None, help="output file (default: standard output)")
    cv.add_argument("jellyfish_fn", nargs="*", metavar="db.jf", help="one or more databases")
    bt = sub.add_parser("bait", help="the FASTQ reads that hit (or, with -v, miss) a k-mer table, extracted on the GPU")
    bt.add_argument("-n", "--min-hits", type=_min_hits, default=1, metavar="N",
                    help="keep a read with at least N k-mers of the table (default: -n 1)")
    bt.add_argument("-v", "--invert", action="store_true", help="keep the reads that do NOT have N k-mers of the table")
    bt.add_argument("-Q", "--min-qual-char", type=_one_char, default=None, metavar="CHAR",
                    help="a base whose quality character is below CHAR is read as N before the k-mers are looked up")
    bt.add_argument("-o", "--output", default=None, help="output file (default: standard output)")
    bt.add_argument("-t", "--targets", action="append", default=[], metavar="FASTA",
                    help="bait k-mers from the records of this FASTA file or directory; may be given several times")
    bt.add_argument("-m", "--mer-len", type=int, default=None, help="with -t: length of the bait k-mers (default: -m 31)")
    bt.add_argument("-d", "--db", default=None, metavar="db.jf", help="bait k-mers from an existing binary/sorted file")
    bt.add_argument("-1", "--mate1", action="append", default=[], metavar="R1.fq",
                    help="paired-end: a mate-1 file; the i-th -1 pairs with the i-th -2, and a pair is kept or dropped whole")
    bt.add_argument("-2", "--mate2", action="append", default=[], metavar="R2.fq", help="paired-end: the mate-2 file of a -1")
    bt.add_argument("-O", "--output2", default=None, metavar="out_2.fq",
                    help="with -1/-2: the kept mate-2 records (-o takes the mate-1 records)")
    bt.add_argument("--pair-rule", choices=("any", "both", "sum"), default=None,
                    help="with -1/-2: N k-mers in either mate (any, the default), in each mate (both) or in the two together (sum)")
    bt.add_argument("--no-name-check", action="store_true",
                    help="with -1/-2: do not compare the mates' names (a /1 or /2 at the end is ignored by the check)")
    bt.add_argument("--split-dir", default=None, metavar="DIR",
                    help="one FASTQ per label in DIR, split on the GPU in one pass over the reads: with -t one label per "
                         "target file, with --rows one per variant row; DIR/labels.tsv lists them")
    bt.add_argument("--rows", default=None, metavar="TSV",
                    help="with --split-dir: the labels are the variant rows of this find_mutation TSV (- is stdin), the "
                         "k-mers of a row's Sequence that its Reference_sequence lacks; the TSV does not record its k: "
                         "give the k of the run that wrote it with -m (default: -m 31)")
    bt.add_argument("--with-ref", action="store_true",
                    help="with --rows: also a .ref label per row, the reference k-mers that the variant lacks")
    bt.add_argument("-i", "--info", default=None, metavar="INFO",
                    help="with --rows: take the rows whose Info column matches INFO (default: vs_ref)")
    bt.add_argument("reads", nargs="*", help="4-line FASTQ files, plain or gzip; - is stdin")
    return parser


def _looks_like_target(path):
    """A directory, or a file whose first byte is '>' (FASTA) or the gzip magic: what `cov -t` takes as a target when
    the databases follow it without another option in between.  Anything else, a missing file too, is a database."""
    if os.path.isdir(path):
        return True
    try:
        with open(path, "rb") as fh:
            head = fh.read(2)
    except OSError:
        return False
    return head[:1] == b">" or head == b"\x1f\x8b"


def parse_args(argv=None, parser=None):
    """build_parser().parse_args plus what argparse cannot say on its own, refused the same way (exit status 2):
    `dump -t` without `-c`, `query` with neither -s nor a MER, `count` with --solid beside --if, `merge` with more than one of --max / --min /
    --subtract, `bait --split-dir` beside any of -v, -o, -O, -d, -1, -2 or without exactly one of -t / --rows, --rows
    without --split-dir, --with-ref or -i without --rows, `bait` without exactly one of -t / -d or with -m beside -d, without reads, with unequal numbers of -1 and
    -2, with plain reads beside them, with -1/-2 but not both of -o and -O or with one path for both, and with -O,
    --pair-rule or --no-name-check but no -1/-2."""
    parser = build_parser() if parser is None else parser
    args = parser.parse_args(argv)
    if args._cmd == "dump" and args.tab and not args.column:
        parser.error("dump: -t needs -c")
    if args._cmd == "count" and args.solid is not None and args.only:
        parser.error("count: --solid and --if exclude each other")
    if args._cmd == "merge" and args.max + args.min + args.subtract > 1:
        parser.error("merge: --max, --min and --subtract exclude each other")
    if args._cmd == "query" and not args.sequence and not args.mers:
        parser.error("query: nothing to query: give -s FILE or MER arguments")
    if args._cmd == "bait":
        if args.split_dir is not None:
            if args.invert or args.output is not None or args.output2 is not None or args.db is not None \
                    or args.mate1 or args.mate2:
                parser.error("bait: --split-dir goes with none of -v, -o, -O, -d, -1 and -2")
            if bool(args.targets) == (args.rows is not None):
                parser.error("bait: --split-dir takes its labels from exactly one of -t targets.fa and --rows TSV")
            if args.rows == "-" and "-" in args.reads:
                parser.error("bait: --rows - reads the TSV from standard input, so the reads cannot be - as well")
        elif args.rows is not None:
            parser.error("bait: --rows goes with --split-dir only")
        if args.rows is None and (args.with_ref or args.info is not None):
            parser.error("bait: --with-ref and -i go with --rows only")
        if args.rows is None and bool(args.targets) == (args.db is not None):
            parser.error("bait: give exactly one of -t targets.fa and -d db.jf")
        if args.db is not None and args.mer_len is not None:
            parser.error("bait: -m goes with -t only: a -d file has its own k")
        if args.mate1 or args.mate2:
            if len(args.mate1) != len(args.mate2):
                parser.error("bait: every -1 file needs its -2 file: %d of -1, %d of -2" % (len(args.mate1), len(args.mate2)))
            if args.reads:
                parser.error("bait: give the reads either as -1/-2 pairs or as plain arguments, not both")
            if args.output is None or args.output2 is None:
                parser.error("bait: -1/-2 need both -o and -O: standard output cannot carry two files")
            if os.path.abspath(args.output) == os.path.abspath(args.output2):
                parser.error("bait: -o and -O name one file")
        else:
            if not args.reads:
                parser.error("bait: no reads: give FASTQ files, or -1/-2 pairs")
            if args.output2 is not None or args.pair_rule is not None or args.no_name_check:
                parser.error("bait: -O, --pair-rule and --no-name-check go with -1/-2 only")
    if args._cmd == "cov" and not args.jellyfish_fn:     # `-t a.fa b.fa db.jf ..`: -t took the databases too
        n = 0
        while n < len(args.targets) and _looks_like_target(args.targets[n]):
            n += 1
        args.targets, args.jellyfish_fn = args.targets[:n], args.targets[n:]
        if not args.targets or not args.jellyfish_fn:
            parser.error("cov: give -t <targets.fa ...|dir> and at least one db.jf")
    return args


def main(argv=None):
    parser = build_parser()
    args = parse_args(argv, parser)
    cmd = args._cmd
    del args._cmd
    # KM_DEVICES=0,1,..: one rank per listed GPU, started here (before anything touches a GPU)
    if cmd in ("find_mutation", "samples") and "RANK" not in os.environ:
        from . import dist as kd
        devs = kd.devices_from_env()
        if devs and len(devs) > 1:
            sys.exit(kd.launch_ranks(len(devs), sys.argv[1:] if argv is None else list(argv)))
    if cmd == "find_mutation":
        main_find_mut(args)
    elif cmd == "samples":
        main_samples(args)
    elif cmd == "min_cov":
        main_min_cov(args)
    elif cmd == "linear_kmin":
        main_linear_kmin(args)
    elif cmd == "count":
        main_count(args)
    elif cmd == "merge":
        main_merge(args)
    elif cmd == "compare":
        main_compare(args)
    elif cmd == "histo":
        main_histo(args)
    elif cmd == "stats":
        main_stats(args)
    elif cmd == "dump":
        main_dump(args)
    elif cmd == "query":
        main_query(args)
    elif cmd == "cov":
        main_cov(args)
    elif cmd == "bait":
        main_bait(args)
    else:
        parser.print_help(sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
