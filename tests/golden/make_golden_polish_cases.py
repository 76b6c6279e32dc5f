"""Golden vectors of the polish summary encoder on the hand-built pileups of tests/polish_encoder_cases.py (the families
tile_edges, many_operations, spans and scan_edges), produced by the REFERENCE's SummaryGenerator compiled into oracle/_ref
(`make -C oracle ref`, where the reference's sources are):   python tests/golden/make_golden_polish_cases.py
Stores only outputs, one pair of arrays per case and span: <family>__<case>__<span index>__image / __positions; the inputs are
rebuilt by the catalogue."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pileup_utils as pu                    # noqa: E402
import polish_encoder_cases as pc            # noqa: E402

OUT = os.path.join(HERE, "encoder_polish_cases.npz")


def golden_arrays(lib):
    out = {}
    for family in pc.GOLDEN_FAMILIES:
        for name, case in pc.FAMILIES[family]().items():
            pile = pc.pileup(case)
            for k, (start, end) in enumerate(case[4]):
                img, pos = pu.run_polish_reference(lib, pile, start, end)
                out["%s__%s__%d__image" % (family, name, k)] = img
                out["%s__%s__%d__positions" % (family, name, k)] = pos
    return out


if __name__ == "__main__":
    pref = pu.load_reference_polish_encoder()
    assert pref is not None, "needs oracle/_ref/libref_polish_encoder.so (make -C oracle ref)"
    arrays = golden_arrays(pref)
    np.savez_compressed(OUT, **arrays)
    print(len(arrays) // 2, "summaries,", sum(len(v) for k, v in arrays.items() if k.endswith("image")), "rows,",
          os.path.getsize(OUT), "bytes")
