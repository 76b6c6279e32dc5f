"""pa_encoder_select_candidates -- the device selection over an encoder's last run, its lists read where the run left them --
against pa_selector_run over the lists pa_encoder_get_results returns and the FASTA text, and against the host library."""
import numpy as np
import pytest
import torch

from pepper_amd.variant.DeviceSelect import DeviceSelector
from select_utils import Case, host_select, rules
from test_gpu_device_candidates_pipeline import job  # noqa: F401 -- the 40 kb job (a module-scoped fixture)
from test_gpu_long_cigars import PARAMS
from test_gpu_select import _same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("device_candidates", [True, False])
def test_encoder_selection_equals_the_lists_and_the_host(job, device_candidates):  # noqa: F811
    from pepper_amd.variant.bam import BAM_handler
    from pepper_amd.variant.fasta import FASTA_handler
    from pepper_amd.variant.PEPPER_VARIANT import PackedEncoder
    edges = list(range(4000, 24001, 4000))                     # five intervals of 4 kb; the pile of short reads is in the last
    starts, stops = [a - 100 for a in edges[:-1]], [b + 100 for b in edges[1:]]
    regions = list(zip(starts, stops))
    fasta = FASTA_handler(job.fasta)
    refs = [bytes(fasta.get_reference_bytes("ctg", a, b + 1)) for a, b in regions]
    enc = PackedEncoder(0, arena_bytes=64 << 20)
    selector, plain = DeviceSelector(0), DeviceSelector(0)
    try:
        enc.set_device_candidates(device_candidates)
        n_done, region_pairs, counts = enc.pack(BAM_handler(job.bam), "ctg", starts, stops, False, 1)
        assert n_done == len(starts)
        per_region, live = enc.encode(regions, refs, region_pairs, counts, PARAMS, list(zip(edges[:-1], edges[1:])), fetch=False)
        assert enc.candidate_calls() == ((1, 0) if device_candidates else (0, 0))
        n = int(per_region.sum())
        assert n > 60 and (per_region > 0).sum() >= 4
        probs = np.random.default_rng(77).random((n, 3)).astype(np.float32)
        probs[::7, 0] += 1.0
        rule = rules(p=(0.75, 0.65, 0.85), p_lc=(0.9, 0.5, 0.95), above=(0.3, 0.3, 0.3))
        on_device = torch.from_numpy(probs).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        # nothing of the run has been downloaded yet
        status, m, name_bytes = selector.run_encoder(enc.enc, rule, on_device)
        assert status == 0
        taken = selector.take()
        # the same rows from the lists the encoder returns and the FASTA text
        outs = enc.last.results()
        assert [len(o["positions"]) for o in outs] == per_region.tolist()
        names = [c.encode("latin-1") for o in outs for c in o["candidates"]]
        first = np.concatenate([[0], np.cumsum(per_region)[:-1]]).tolist()
        case = Case(np.concatenate([o["positions"] for o in outs]), np.concatenate([o["depths"] for o in outs]),
                    np.concatenate([o["candidate_frequency"] for o in outs]), probs, names,
                    [(first[r], starts[r], refs[r]) for r in range(len(regions))])
        assert plain.run(rule, case.position, case.depth, case.support, case.prediction, case.blob, case.regions)[0] == 0
        want = host_select(case, rule)
        assert 0 < len(want["row"]) < n and (m, name_bytes) == (len(want["row"]), len(want["names"]))
        _same(plain.take(), want)
        _same(taken, want)
        # and once more after the download, on the same handles: the same bytes
        assert selector.run_encoder(enc.enc, rule, on_device)[0] == 0
        _same(selector.take(), want)
    finally:
        selector.close()
        plain.close()
        enc.close()
