"""tests/record_walk_cases.py without a GPU: every case builds and its restatement terminates, the catalogue reaches every
verdict the device test (tests/test_gpu_record_walk.py) is meant to see -- so that test cannot pass by never reaching a
branch -- and the restatement is tied to the host code: the headers it derives, given to pa_bam_pack_headers, build the
tables pa_bam_pack_inflated builds from the bytes of the same span."""
import pytest

import record_walk_cases as rw
from pepper_amd.variant.bam import BamError

# what the catalogue must reach, over both settings of `split` (the counts the device test's docstring quotes)
MIN_PER_STATE = 20
REASONS = ("core", "a fixed-size value cut by the record end", "a string without its NUL", "an array cut inside its subtype and count",
           "an array of an unknown subtype", "an array longer than the record", "an unknown type letter")


def _walks():
    for case in rw.CASES:
        span, data_bytes, entries, cap = case.build()
        for split in (0, 1):
            reasons = []
            headers, flags = rw.restated_walk(span, data_bytes, entries, cap, split, reasons)
            yield case, split, headers, flags, reasons


@pytest.fixture(scope="module")
def walks():
    return list(_walks())


@pytest.fixture(scope="module")
def handle(tmp_path_factory):
    """A tiny BAM written only for a handle that names the contig."""
    bam = rw.contig_handle(tmp_path_factory.mktemp("record_walk"))
    yield bam
    bam.close()


def test_every_case_builds_and_the_restatement_terminates(walks):
    assert len(walks) == 2 * len(rw.CASES) and len({c.name for c in rw.CASES}) == len(rw.CASES)
    for case, _split, headers, flags, _reasons in walks:
        span, data_bytes, entries, cap = case.build()
        assert len(span) < 2 << 20 and data_bytes <= len(span), case.name
        assert flags[0] in range(16) and flags[1] in (0, 1) and (len(headers) == 0 or flags[0] == 0), case.name
        assert len(headers) <= len(entries) * cap, case.name


def test_the_catalogue_reaches_every_verdict(walks):
    states = {0: 0, 1: 0, 2: 0, 3: 0}
    bits = {1: 0, 2: 0, 8: 0}
    cuts, reasons = 0, {}
    for _case, _split, headers, flags, why in walks:
        for s in states:
            states[s] += int((headers["state"] == s).sum())
        for b in bits:
            bits[b] += 1 if flags[0] & b else 0
        cuts += flags[1]
        if flags[0] == 0:                       # (reasons of walks whose headers are delivered)
            for r in why:
                reasons[r] = reasons.get(r, 0) + 1
    print(states, bits, cuts, reasons)
    assert all(n >= MIN_PER_STATE for n in states.values()), states
    assert all(n >= 1 for n in bits.values()) and cuts >= 1, (bits, cuts)
    assert sorted(reasons) == sorted(REASONS) and all(reasons[r] >= 1 for r in REASONS), reasons
    # state 2 from the core and from the tag walk separately, and each in a hand-written case too (not only the random family)
    by_hand = [(c, s, h, f, w) for c, s, h, f, w in walks if not c.name.startswith("random")]
    assert any("core" in w for _c, _s, _h, f, w in by_hand if f[0] == 0)
    assert any(any(r != "core" for r in w) for _c, s, _h, f, w in by_hand if f[0] == 0 and s == 1)
    # a saturated ref_len and one just below it
    nine = next(h for c, s, h, _f, _w in walks if c.name.startswith("nine N") and s == 1)
    assert nine["ref_len"].tolist()[:7] == [rw.INT32_MAX] * 3 + [rw.INT32_MAX - 1] + [rw.INT32_MAX] * 3 and nine["state"].tolist()[:2] == [0, 3]
    # both flags[0] == 1 (a lane out of slots) and a clean walk whose largest lane fills its slots exactly
    full = next(h for c, s, h, _f, _w in walks if c.name == "150 entries, the largest count met exactly" and s == 0)
    assert len(full) == sum(rw.ENTRY_COUNTS[:149])


host_tables = rw.host_tables


def test_restated_headers_pack_as_the_host_walk_packs_the_span(walks, handle):
    compared = refused = reads = split_reads = 0
    for case, split, headers, flags, _reasons in walks:
        if split != 1 or flags[0] != 0:
            continue
        span, data_bytes, entries, _cap = case.build()
        if (headers["state"] == 2).any():
            with pytest.raises(BamError) as e:
                host_tables(handle, span, data_bytes, entries[0], headers)
            assert e.value.code == -6, case.name
            refused += 1
            continue
        got, want = host_tables(handle, span, data_bytes, entries[0], headers), host_tables(handle, span, data_bytes, entries[0])
        for key in want:
            assert got[key] == want[key], (case.name, key)
        assert want["n_done"] == len(rw.REGION_STARTS)
        compared += 1
        reads += want["counts"][0]
        split_reads += want["n_split"]
    print(compared, refused, reads, split_reads)
    assert compared >= 20 and refused >= 10 and reads > 5000 and split_reads > 300


def test_the_nine_n_records_reach_every_region(walks, handle):
    """2 415 919 105 reference bases from position 100: a read of all three regions, in the core form and in the CG form, by the
    headers (ref_len saturated at INT32_MAX) as by the host walk's 64-bit sum."""
    case = rw.by_name("nine N operations of 2^28 - 1 bases")
    span, data_bytes, entries, _cap = case.build()
    headers = next(h for c, s, h, _f, _w in walks if c is case and s == 1)
    for tables in (host_tables(handle, span, data_bytes, entries[0], headers), host_tables(handle, span, data_bytes, entries[0])):
        assert tables["counts"][0] == 10 and tables["n_split"] == 1
        rp, pr = tables["region_pairs"], tables["pair_read"]
        assert pr[rp[0]:rp[1]] == list(range(9)) and pr[rp[1]:rp[2]] == list(range(7)) + [8, 9] and pr[rp[2]:rp[3]] == list(range(7))
