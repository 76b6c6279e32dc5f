"""Golden vectors of the variant summary encoder on the hand-built pileups of tests/variant_encoder_cases.py (its
GOLDEN_FAMILIES), produced by the REFERENCE's encoder compiled into oracle/_ref (`make -C oracle ref`, where the reference's
sources are):   python tests/golden/make_golden_variant_cases.py
Stores only outputs, five arrays per case: <family>__<case>__candidates (the keys joined by newlines) / __positions / __depths /
__candidate_frequency / __images (int16, as the other variant goldens); the inputs are rebuilt by the catalogue."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pileup_utils as pu                    # noqa: E402
import variant_encoder_cases as vc           # noqa: E402

OUT = os.path.join(HERE, "encoder_variant_cases.npz")
KEYS = ("candidates", "positions", "depths", "candidate_frequency", "images")


def as_golden(result):
    """A result of pileup_utils.run_variant in the form the file holds."""
    assert np.abs(result["images"]).max(initial=0) < 2 ** 15
    return dict(candidates=np.array("\n".join(result["candidates"])), positions=result["positions"].astype(np.int64),
                depths=result["depths"].astype(np.int32), candidate_frequency=result["candidate_frequency"].astype(np.int32),
                images=result["images"].astype(np.int16))


def golden_arrays(lib):
    out = {}
    for family in vc.GOLDEN_FAMILIES:
        for name, case in vc.FAMILIES[family]().items():
            got = as_golden(pu.run_variant(lib, vc.pileup(case), vc.params(case), reference_impl=True))
            for key in KEYS:
                out["%s__%s__%s" % (family, name, key)] = got[key]
    return out


if __name__ == "__main__":
    ref = pu.load_reference_encoder()
    assert ref is not None, "needs oracle/_ref/libref_variant_encoder.so (make -C oracle ref)"
    arrays = golden_arrays(ref)
    np.savez_compressed(OUT, **arrays)
    print(len(arrays) // len(KEYS), "cases,", sum(len(v) for k, v in arrays.items() if k.endswith("positions")), "candidates,",
          os.path.getsize(OUT), "bytes")
