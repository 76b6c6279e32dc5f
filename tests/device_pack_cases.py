"""Header tables built by hand for the device pack's tests (tests/test_gpu_device_pack.py on the GPU, tests/test_device_pack_cpu.py
without one): no test lives here."""
import numpy as np

TID = 1             # the contig of the walk: one contig in front of it, one behind
STATUS_OF_RC = {-6: (2, 5), -8: (3,), -9: (4,)}         # pa_bam_pack_headers' failures -> the statuses the device may report for them


def headers(rows):
    """rows: dicts with any of the header's fields; defaults describe a kept read of contig TID."""
    from pepper_amd.variant.bam import RECORD_HEADER
    out = np.zeros(len(rows), RECORD_HEADER)
    for k, row in enumerate(rows):
        h = dict(data_off=(k * 97) % 4000, ref_id=TID, pos=0, l_seq=50, n_cigar=3, flag=0, mapq=60, ref_len=100, state=0, block_size=300)
        h.update(row)
        for key in ("data_off", "ref_id", "pos", "l_seq", "n_cigar", "ref_len", "state", "block_size"):
            out[k][key] = h[key]
        out[k]["flags"] = h["flag"] | (h["mapq"] << 16)
    return out


def random_headers(rng, n, max_pos):
    rows = []
    for pos in np.sort(rng.integers(0, max_pos, n)):
        rows.append(dict(pos=int(pos), ref_len=int(rng.choice([0, 1, 80, 700, 2500])), l_seq=int(rng.integers(1, 3000)),
                         n_cigar=int(rng.integers(1, 40)), flag=int(rng.choice([0, 16, 0, 16, 0x4, 0x100, 0x200, 0x400, 0x800])),
                         mapq=int(rng.choice([0, 4, 5, 60])), data_off=int(rng.integers(0, 20000))))
    return headers(rows)


def layouts(n_regions, kind):
    edges = np.arange(n_regions + 1) * 3000 + 2000
    if kind == "abutting":
        return edges[:-1], edges[1:]
    if kind == "flank":
        return np.maximum(0, edges[:-1] - 100), edges[1:] + 100
    return edges[:-1], edges[:-1] + 900          # a gap of 2 100 positions behind every region
