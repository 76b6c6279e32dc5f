"""Golden results of the read re-aligner on the hand-built reads of tests/realign_cases.py, produced by the REFERENCE's own SSW
build compiled into oracle/_ref (`make -C oracle ref`, where the reference's sources are), driven the way
ReadAligner::align_reads_to_reference drives it:   python tests/golden/make_golden_realign_cases.py
Stores results only -- per family the case names, status, score, new position, new end position and the CIGAR texts -- and a
SHA-256 of the catalogue's inputs; the inputs themselves are rebuilt by the catalogue."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import realign_cases as rc                   # noqa: E402
from oracle import ssw                       # noqa: E402

OUT = os.path.join(HERE, "realign_edge_cases.npz")
OP_TEXT = {7: "=", 8: "X", 1: "I", 2: "D", 4: "S"}


def results(cases, aligner):
    """[(status, score, pos, pos_end, ops)] of a family's cases, in the order of the dict."""
    return [ssw.realign_reads(window, start, [pos], [seq], aligner=aligner)[0] for start, window, pos, seq, _ in cases.values()]


def cigar_text(ops):
    return "".join("%d%s" % (n, OP_TEXT[o]) for o, n in ops)


def golden_arrays(aligner=None, families=None):
    aligner = aligner or (lambda r, q: ssw.align_reference(r, q) + (0,))
    families = families or {name: fn() for name, fn in rc.FAMILIES.items()}
    out = {"input_sha256": np.array(rc.input_digest(families))}
    for fam, cases in sorted(families.items()):
        res = results(cases, aligner)
        out[fam + "__names"] = np.array("|".join(cases))
        out[fam + "__status"] = np.array([r[0] for r in res], np.int32)
        out[fam + "__score"] = np.array([r[1] for r in res], np.int32)
        out[fam + "__pos"] = np.array([r[2] for r in res], np.int64)
        out[fam + "__pos_end"] = np.array([r[3] for r in res], np.int64)
        out[fam + "__cigars"] = np.array("|".join(cigar_text(r[4]) for r in res))
    return out


if __name__ == "__main__":
    assert ssw.have_reference(), "needs oracle/_ref/libref_ssw.so (make -C oracle ref)"
    arrays = golden_arrays()
    np.savez_compressed(OUT, **arrays)
    print(sum(len(str(v).split("|")) for k, v in arrays.items() if k.endswith("__names")), "reads,", os.path.getsize(OUT), "bytes")
