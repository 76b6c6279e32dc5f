"""Shared by the device-selection tests: the host library as the oracle (pa_candidates_reference_flags +
pa_candidates_select_format, pepper_amd/csrc/candidates.cpp) and the inputs the tests give to both sides."""
import ctypes

import numpy as np

from pepper_amd import h5
from pepper_amd.variant.FastCandidates import _Rules

BASES = np.frombuffer(b"ACGT", np.uint8)


def rules(p=(0.5, 0.4, 0.6), p_lc=(0.7, 0.3, 0.8), above=(0.3, 0.25, 0.25), cutoffs=(15.0, 12.0, 10.0, 8.0)):
    return _Rules((ctypes.c_double * 3)(*p), (ctypes.c_double * 3)(*p_lc), (ctypes.c_double * 3)(*above), *cutoffs)


class Case(object):
    """One call's rows: position int64 [n], depth / support int32 [n], prediction float32 [n, 3], names (list of bytes),
    regions [(first_row, reference_start, reference bytes)]."""

    def __init__(self, position, depth, support, prediction, names, regions):
        self.position = np.ascontiguousarray(position, np.int64)
        self.depth = np.ascontiguousarray(depth, np.int32)
        self.support = np.ascontiguousarray(support, np.int32)
        self.prediction = np.ascontiguousarray(prediction, np.float32).reshape(len(self.position), 3)
        self.names = list(names)
        self.regions = list(regions)

    @property
    def n(self):
        return len(self.position)

    @property
    def blob(self):
        return b"".join(name + b"\0" for name in self.names)


def host_select(case, rule):
    """What the host library keeps of a case -> None when it returns -2, else a dict of the kept rows' arrays (flags with bit 1
    cleared: QUAL and its cutoff are not the device's business), plus `letters` / `repeat` of every row."""
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
    starts[1:] = np.cumsum([len(name) + 1 for name in case.names]) if n else []
    depth, support = case.depth.astype(np.int64), case.support.astype(np.int64)
    row, ref_len, flags = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.uint8)
    offsets = np.empty(n + 1, np.int64)
    cap = len(blob) + n * 210 + 64
    lines = np.empty(cap, np.uint8)
    pad = np.zeros(1, np.int64)            # (n == 0: the library is not given NULL for arrays it never reads)
    m = io.pa_candidates_select_format(
        ctypes.byref(rule), b"c", n, case.position.ctypes.data if n else pad.ctypes.data, depth.ctypes.data if n else pad.ctypes.data,
        support.ctypes.data if n else pad.ctypes.data, case.prediction.ctypes.data if n else pad.ctypes.data,
        letters.ctypes.data if n else pad.ctypes.data, repeat.ctypes.data if n else pad.ctypes.data, blob + b"\0", starts.ctypes.data, 1,
        row.ctypes.data if n else pad.ctypes.data, ref_len.ctypes.data if n else pad.ctypes.data,
        flags.ctypes.data if n else pad.ctypes.data, ctypes.c_void_p(lines.ctypes.data), cap, offsets.ctypes.data)
    if m == -2:
        return None
    assert m >= 0, io.pa_h5_last_error()
    row = row[:m].copy()
    kept_names = [case.names[i] for i in row.tolist()]
    return {"row": row, "flags": flags[:m] & 0x35, "full_flags": flags[:m].copy(), "letter": letters[row], "in_repeat": repeat[row],
            "position": case.position[row], "depth": depth[row], "support": support[row], "prediction": case.prediction[row],
            "names": b"".join(name + b"\0" for name in kept_names),
            "name_offsets": np.concatenate([[0], np.cumsum([len(name) + 1 for name in kept_names])]).astype(np.int64),
            "letters": letters, "repeat": repeat, "ref_len": ref_len[:m].copy(),
            "lines": [lines[offsets[k]:offsets[k + 1]].tobytes() for k in range(m)]}


def contig_text(seed=5, length=3000):
    """3 kb of ACGT with homopolymers of 4, 5 and 6 planted every 40 bases or so, two lower-case stretches and two stretches of N."""
    r = np.random.default_rng(seed)
    text = BASES[r.integers(0, 4, length)].copy()
    at = 30
    while at + 8 < length:
        text[at:at + int(r.integers(4, 7))] = BASES[int(r.integers(0, 4))]
        at += int(r.integers(25, 60))
    for lo, hi in ((400, 520), (2100, 2160)):
        text[lo:hi] |= 0x20
    for lo, hi in ((900, 960), (2500, 2530)):
        text[lo:hi] = ord("N")
    return text.tobytes()


def random_case(n, seed, text=None, name_bytes=None):
    """n rows over three regions of the contig (the first starts at 0, the others keep 100 bases in front of their rows), positions
    ascending with repeats inside each region, a few past the end of the last region's reference.  name_bytes: the names are
    lengthened (letters of ACGT appended, at most 63 per allele) until their bytes, NULs included, are exactly that many."""
    text = contig_text() if text is None else text
    r = np.random.default_rng(seed)
    L = len(text)
    spans = [(0, 0, 1100), (900, 1000, 2000), (1900, 2000, L + 15)]        # (reference start, first position, end of positions)
    cut = [0, n // 3, (2 * n) // 3, n]
    position = np.empty(n, np.int64)
    regions = []
    for k, (ref0, lo, hi) in enumerate(spans):
        m = cut[k + 1] - cut[k]
        position[cut[k]:cut[k + 1]] = np.sort(r.integers(lo, hi, m))
        regions.append((cut[k], ref0, text[ref0:min(L, hi + 100)]))
    depth = r.integers(1, 61, n).astype(np.int32)
    support = np.minimum(depth, r.integers(0, 40, n)).astype(np.int32)
    prediction = r.random((n, 3)).astype(np.float32)
    prediction[r.random(n) < 0.3, 0] += 1.0                                 # (rows the probability does not admit)
    tie = r.random(n) < 0.05
    prediction[tie, 2] = prediction[tie, 1]
    kinds = r.choice(np.frombuffer(b"1231230412", np.uint8), n)
    lens = np.where(kinds == ord("1"), 1, r.integers(1, 7, n))
    letters = BASES[r.integers(0, 4, (n, 6))]
    odd = r.random(n) < 0.04
    names = []
    for i in range(n):
        allele = letters[i, :lens[i]].tobytes()
        if odd[i]:
            allele = allele[:-1] + (b"N" if i % 2 else b"a")
        names.append(bytes([kinds[i]]) + allele)
    if name_bytes is not None:
        need = name_bytes - sum(len(name) + 1 for name in names)
        assert need >= 0, "fewer name bytes asked for than the rows have"
        i = 0
        while need > 0:
            assert i < n, "the rows cannot hold that many name bytes"
            add = min(need, 64 - len(names[i]))
            names[i] += BASES[r.integers(0, 4, add)].tobytes()
            need -= add
            i += 1
    return Case(position, depth, support, prediction, names, regions)


def branches(case, rule, kept):
    """Which branches of the rules a case's host result takes -> a dict of counts."""
    n = case.n
    name_ok = np.array([all(c in b"ACGT" for c in name[1:]) for name in case.names], bool)
    kind = np.array([name[0] - ord("1") for name in case.names])
    letter_ok = np.isin(kept["letters"], BASES)
    row, flags = kept["row"], kept["full_flags"]
    non_alt = np.maximum(case.prediction[:, 1], case.prediction[:, 2]).astype(np.float64)[row]
    rep = kept["repeat"][row].astype(bool)
    k = kind[row]
    thr = np.where(rep, np.array(rule.p_value_in_lc)[k], np.array(rule.p_value)[k])
    by_p = non_alt >= thr
    out = {"rows": n, "kept": len(row), "refused_letter": int((~letter_ok).sum()), "refused_allele": int((letter_ok & ~name_ok).sum()),
           "type_outside": int((letter_ok & name_ok & ((kind < 0) | (kind > 2))).sum()),
           "by_probability": int((by_p & ~rep).sum()), "by_probability_lc": int((by_p & rep).sum()), "by_frequency": int((~by_p).sum()),
           "swap": int(((flags & 4) != 0).sum()), "unswapped_delete": int(((k == 2) & ((flags & 4) == 0)).sum())}
    for t in range(3):
        out["kind%d" % t] = int((k == t).sum())
    for g in range(3):
        out["genotype%d" % g] = int(((flags >> 4) == g).sum())
    return out
