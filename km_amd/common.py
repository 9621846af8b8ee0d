"""Drop-ins for the two helpers of km/utils/common.py that touch the k-mer database.

``get_cov(db, ref_seq)`` is what ``km min_cov`` (km/tools/min_cov.py:10-25) and
``km find_report -e <exclusion.jf>`` (km/tools/find_report.py:137-139) call: the coverage
statistics of every k-mer of a sequence.  The reference opens the database and issues one
``Jellyfish.query`` per k-mer on every call (km/utils/common.py:73-92); here a database is
loaded into HBM once per path and the sequences of a call — one, or MANY with ``get_cov_many`` —
go to the device as text: their k-mers are cut, looked up and reduced to the statistics there
(``Database.cov_seqs``), and only one cell per sequence comes back.  ``cov_many`` returns those cells
as they are, for callers that want a row for every sequence instead of the reference's exceptions.
"""

from .jellyfish import Jellyfish

_OPEN = {}


def _handle(db):
    if isinstance(db, Jellyfish):
        return db
    jf = _OPEN.get(db)
    if jf is None:
        jf = _OPEN[db] = Jellyfish(db)
    return jf


def close(db):
    """Free the HBM table of one database opened through get_cov (a path), if it is open."""
    jf = _OPEN.pop(db, None)
    if jf is not None:
        jf.db.close()


def close_all():
    for jf in _OPEN.values():
        jf.db.close()
    _OPEN.clear()


def cov_many(db, seqs):
    """The raw statistics of every sequence of `seqs`: the structured array of Database.cov_seqs (total, n_kmers,
    n_zero, n_skipped, n_nonbase, min, max).  Nothing is raised for a sequence without windows or with bytes outside
    ACGTacgt: such windows are skipped and counted."""
    return _handle(db).db.cov_seqs(seqs)


def _stats(seq, c):
    n = int(c["n_kmers"])
    if n == 0:
        # the reference takes min() of an empty list here
        raise ValueError("min() arg is an empty sequence")
    total = int(c["total"])
    return (total, len(seq), int(c["min"]), int(c["max"]), float(total) / n, n, int(c["n_zero"]))


def get_cov(db, ref_seq):
    """(count, len(ref_seq), min, max, mean, kmer_nb, kmer_nb_0) — km/utils/common.py:73-92."""
    return get_cov_many(db, [ref_seq])[0]


def get_cov_many(db, seqs):
    """get_cov of every sequence of `seqs` with ONE scan of the device.  As before: a byte outside ACGTacgt anywhere
    in the call is a ValueError, and so is, after that, the first sequence shorter than k."""
    seqs = list(seqs)
    cov = cov_many(db, seqs)
    if cov["n_nonbase"].any():
        raise ValueError("non-ACGT character in sequence")
    return [_stats(s, c) for s, c in zip(seqs, cov)]
