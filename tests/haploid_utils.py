"""Shared by the haploid tests: the host library with a ploidy per row as the oracle (pa_candidates_reference_flags +
pa_candidates_select_format_ploidy, pepper_amd/csrc/candidates.cpp) over a select_utils.Case, and the cases the device test runs."""
import ctypes

import numpy as np

from pepper_amd import h5
from pepper_amd.variant import Targets
from select_utils import BASES, Case, contig_text

HET = (0.125, 0.5, 0.375)                       # primed: (0.25, 0, 0.75) -- genotype 1 becomes 2
TIE = (0.25, 0.5, 0.25)                         # primed: (0.5, 0, 0.5) -- genotype 1 becomes 0 (the first maximum)
ALL_HET = (0.0, 1.0, 0.0)                       # s == 0: (0.5, 0, 0.5)
DELETE_AFTER = (0.5625, 0.234375, 0.1875)       # non_alt 0.234375 < 0.25 raw, 0.1875 / 0.75 = 0.25 primed: swapped only when haploid
DELETE_BEFORE = (0.75, 0.25, 0.0)               # non_alt 0.25 raw, 0 primed: swapped only when diploid


def host_select_ploidy(case, rule, haploid):
    """select_utils.host_select through pa_candidates_select_format_ploidy.  haploid: uint8 / bool per row, or None (NULL).
    -> None for -2, else the kept rows' arrays (flags with bit 1 cleared, bit 3 kept)."""
    io = h5.load()
    n = case.n
    letters, repeat = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    bounds = [r[0] for r in case.regions] + [n]
    for k, (first, start, text) in enumerate(case.regions):
        lo, hi = bounds[k], bounds[k + 1]
        if hi > lo:
            pos = np.ascontiguousarray(case.position[lo:hi])
            le, re = np.empty(hi - lo, np.uint8), np.empty(hi - lo, np.uint8)
            assert io.pa_candidates_reference_flags(text, len(text), start, hi - lo, pos.ctypes.data, le.ctypes.data, re.ctypes.data) == 0
            letters[lo:hi], repeat[lo:hi] = le, re
    blob = case.blob
    starts = np.zeros(n + 1, np.int64)
    starts[1:] = np.cumsum([len(name) + 1 for name in case.names])
    depth, support = case.depth.astype(np.int64), case.support.astype(np.int64)
    row, ref_len, flags = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint8)
    offsets = np.empty(n + 1, np.int64)
    cap = len(blob) + n * 210 + 64
    lines = np.empty(cap, np.uint8)
    mask = None if haploid is None else np.ascontiguousarray(haploid, np.uint8)
    m = io.pa_candidates_select_format_ploidy(
        ctypes.byref(rule), b"c", n, case.position.ctypes.data, depth.ctypes.data, support.ctypes.data, case.prediction.ctypes.data,
        letters.ctypes.data, repeat.ctypes.data, blob + b"\0", starts.ctypes.data, 1, row.ctypes.data, ref_len.ctypes.data,
        flags.ctypes.data, ctypes.c_void_p(lines.ctypes.data), cap, offsets.ctypes.data, None if mask is None else mask.ctypes.data)
    if m == -2:
        return None
    assert m >= 0, io.pa_h5_last_error()
    row = row[:m].copy()
    kept_names = [case.names[i] for i in row.tolist()]
    return {"row": row, "flags": flags[:m] & 0x3d, "full_flags": flags[:m].copy(), "letter": letters[row], "in_repeat": repeat[row],
            "position": case.position[row], "depth": depth[row], "support": support[row], "prediction": case.prediction[row],
            "names": b"".join(name + b"\0" for name in kept_names),
            "name_offsets": np.concatenate([[0], np.cumsum([len(name) + 1 for name in kept_names])]).astype(np.int64),
            "ref_len": ref_len[:m].copy(), "lines": [lines[offsets[k]:offsets[k + 1]].tobytes() for k in range(m)]}


def par_table(size, length=3000):
    """A PAR table of `size` intervals inside [40, length): (starts, ends) int64, ascending, disjoint and not touching."""
    if size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    step = (length - 80) // size
    starts = 40 + step * np.arange(size, dtype=np.int64)
    return starts, starts + max(1, step // 4)


def mask_of(table, positions):
    """The rule in numpy for a haploid contig: haploid unless a PAR interval holds the position."""
    return ~Targets.contains(table[0], table[1], positions)


def haploid_case(n, seed, table):
    """n rows of ONE region that is the whole contig (select_utils.contig_text), every name a valid allele.  The first rows are
    hand-built: position 0 and the hand-derived triples at haploid positions, then rows at start - 1, start, end - 1 and end of the
    table's first and last interval; the rest have random positions and float32 softmax triples that lean to HET, some replaced by
    p0 == p2 ties."""
    text = contig_text()
    r = np.random.default_rng(seed)
    position = np.sort(r.integers(0, len(text), n)).astype(np.int64)
    logits = r.normal(0.0, 2.0, (n, 3)).astype(np.float32)
    logits[:, 1] += np.float32(1.5)
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    prediction = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    tie = r.random(n) < 0.08
    prediction[tie, 2] = prediction[tie, 0]
    kinds = r.choice(np.frombuffer(b"1112233", np.uint8), n)
    lens = np.where(kinds == ord("1"), 1, r.integers(1, 6, n))
    letters = BASES[r.integers(0, 4, (n, 6))]
    names = [bytes([kinds[i]]) + letters[i, :lens[i]].tobytes() for i in range(n)]
    depth = r.integers(4, 61, n).astype(np.int32)
    support = np.minimum(depth, r.integers(0, 30, n)).astype(np.int32)
    fixed = [(0, HET, b"1C"), (1, DELETE_AFTER, b"3ACG"), (2, DELETE_BEFORE, b"3ACG"), (3, TIE, b"1A"), (4, ALL_HET, b"2AC")]
    if len(table[0]):
        for k in (0, len(table[0]) - 1):
            s, e_ = int(table[0][k]), int(table[1][k])
            fixed += [(p, HET, b"1G") for p in (s - 1, s, e_ - 1, e_)]
    for i, (p, triple, name) in enumerate(fixed[:n]):
        position[i], prediction[i], names[i], depth[i], support[i] = p, triple, name, 40, 10
    return Case(position, depth, support, prediction, names, [(0, 0, text)])
