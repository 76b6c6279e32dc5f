"""What the encoder's two per-position tracks share on the host: the depth classes (pepper_amd/variant/Coverage.py) and the
reference blocks (pepper_amd/variant/RefConfidence.py).

Both classify every position of a candidate window by ascending lower bounds b[0] = 0 < b[1] < ... (at most 8): class k holds
the values in [b[k], b[k + 1]), the last class is open above; a position outside every target has the class OFF_TARGET.  Both
report the maximal runs of equal class (the reference blocks with the minima of two columns over each run), collect the
workers' runs per interval of the planner and finish them once.  This module holds the parser of the bounds, the run rule in
numpy (what depth_runs_kernel and ref_blocks_kernel, pepper_amd/csrc/encoder.hip, do per tile) and the collecting track.
"""
import threading

import numpy as np

MAX_CLASSES = 8
OFF_TARGET = -1                      # the class of a position outside every target (pa_encoder_set_targets): never written


def parse_bounds(bounds, prefix, noun, limit):
    """A sequence of integers or their text "0,1,5,20" -> int32 lower bounds.  prefix / noun: how the messages begin and what
    they call a class ("coverage bins", "bin"); limit(value) -> None, or what is wrong with a value that is too large.
    ValueError, naming the entry: more than 8 classes, none at all, a first bound that is not 0, a bound that is not above the
    one before it, not an integer or too large."""
    fields = [f.strip() for f in bounds.split(",")] if isinstance(bounds, str) else list(bounds)
    if len(fields) == 0:
        raise ValueError("%s: no %s" % (prefix, noun))
    if len(fields) > MAX_CLASSES:
        raise ValueError("%s: entry %d is one more than the %d %ss a table may have" % (prefix, MAX_CLASSES, MAX_CLASSES, noun))
    out = []
    for k, field in enumerate(fields):
        try:
            if isinstance(field, (float, np.floating)) and float(field) != int(field):
                raise ValueError
            value = int(field)
        except (TypeError, ValueError):
            raise ValueError("%s: entry %d (%r) is not an integer" % (prefix, k, field)) from None
        if k == 0 and value != 0:
            raise ValueError("%s: entry 0 must be 0, not %d" % (prefix, value))
        if k > 0 and value <= out[-1]:
            raise ValueError("%s: entry %d (%d) is not above the one before it (%d)" % (prefix, k, value, out[-1]))
        if limit(value) is not None:
            raise ValueError("%s: entry %d (%d) %s" % (prefix, k, value, limit(value)))
        out.append(value)
    return np.array(out, np.int32)


def classes_of(values, bounds):
    """The class of every value: the last bound at or below it."""
    return np.searchsorted(np.asarray(bounds, np.int64), np.asarray(values, np.int64), side="right") - 1


def class_runs(values, first_position, bounds, on_target=None, minimise=()):
    """values[i] speaks of position first_position + i -> (starts, ends, class, *minima) of the maximal runs of equal class,
    int64 / int64 / int32, ends half-open, with the smallest entry of every column of `minimise` over each run (int32).
    on_target (bool per position; None: all): a position outside has the class OFF_TARGET, and its runs are reported like any
    other."""
    which = classes_of(values, bounds).astype(np.int32)
    if on_target is not None:
        which = np.where(np.asarray(on_target, bool), which, np.int32(OFF_TARGET)).astype(np.int32)
    n = len(which)
    if n == 0:
        return (np.zeros(0, np.int64), np.zeros(0, np.int64)) + tuple(np.zeros(0, np.int32) for _ in range(1 + len(minimise)))
    heads = np.flatnonzero(np.concatenate([[True], which[1:] != which[:-1]]))
    starts = heads.astype(np.int64) + int(first_position)
    ends = np.concatenate([heads[1:], [n]]).astype(np.int64) + int(first_position)
    return (starts, ends, which[heads]) + tuple(np.minimum.reduceat(np.asarray(c, np.int64), heads).astype(np.int32) for c in minimise)


def merge_touching(key, starts, ends, which, *minima):
    """Records in key and position order: touching records of one key and equal class joined, with the smaller of their
    minima -> the same columns, shorter."""
    if len(key) == 0:
        return (key, starts, ends, which) + minima
    joins = (key[1:] == key[:-1]) & (starts[1:] == ends[:-1]) & (which[1:] == which[:-1])
    heads = np.flatnonzero(np.concatenate([[True], ~joins]))
    last = np.concatenate([heads[1:], [len(key)]]) - 1
    return (key[heads], starts[heads], ends[last], which[heads]) + tuple(np.minimum.reduceat(m, heads) for m in minima)


class RunTrack(object):
    """The runs of a whole job, collected from its workers in any order (add) and finished once (finish_arrays).

    contigs: the FASTA's contig names in its order.  A subclass names itself (`what`, `noun`: its messages) and the types of
    a record's columns behind starts and ends (`columns`: the class, then the minima)."""
    what, noun, columns = "run track", "runs", (np.int32,)

    def __init__(self, contigs):
        self.contigs = list(contigs)
        self.order = {name: k for k, name in enumerate(self.contigs)}
        self._lock = threading.Lock()
        self._pieces = []

    def add(self, contig, interval, runs):
        """One interval of the planner: interval = (pos_start, pos_end), both inclusive; runs = (starts, ends, class, *minima)
        of its window in contig coordinates, ascending."""
        if contig not in self.order:
            raise ValueError("%s: contig %r is not in the FASTA" % (self.what, contig))
        cols = [np.array(v, t) for v, t in zip(runs, (np.int64, np.int64) + self.columns)]
        if len(set(len(c) for c in cols)) != 1:
            raise ValueError("%s: %s of unequal lengths" % (self.what, self.noun))
        with self._lock:
            self._pieces.append((self.order[contig], int(interval[0]), int(interval[1])) + tuple(cols))

    def finish_arrays(self):
        """-> (contig index int64, start, end, class, *minima) of the finished runs, in FASTA order, ends half-open: the pieces
        ordered by contig and start; the position two consecutive intervals of split_intervals share (pos_end of one ==
        pos_start of the next) belongs to the one that starts there -- the earlier interval's runs are cut at the next
        interval's start (a cut run keeps its minima: they are then lower bounds) and dropped when nothing is left; off-target
        runs dropped; touching runs of equal class merged with their minima.  Whole-array work: a job has a run every few
        positions where the reads are noisy."""
        with self._lock:
            pieces = sorted(self._pieces, key=lambda p: p[:3])
        if not pieces:
            return tuple(np.zeros(0, t) for t in (np.int64, np.int64, np.int64) + self.columns)
        cols = [[] for _ in range(3 + len(self.columns))]
        for k, (rank, _s, _e, starts, ends, *rest) in enumerate(pieces):
            if k + 1 < len(pieces) and pieces[k + 1][0] == rank:
                ends = np.minimum(ends, pieces[k + 1][1])          # the next interval of the contig owns everything from its start
            for col, v in zip(cols, [np.full(len(starts), rank, np.int64), starts, ends] + rest):
                col.append(v)
        cols = [np.concatenate(c) for c in cols]
        keep = (cols[1] < cols[2]) & (cols[3] != OFF_TARGET)
        return merge_touching(*(c[keep] for c in cols))

    def finish(self):
        """finish_arrays as [(contig, start, end, class, *minima)] with Python integers."""
        rank, *rest = self.finish_arrays()
        return list(zip([self.contigs[k] for k in rank.tolist()], *(c.tolist() for c in rest)))
