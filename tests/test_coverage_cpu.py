"""pepper_amd.variant.Coverage without a GPU: the bins, the run rule in numpy, the track's bookkeeping, and the tie of
tests/coverage_cases.py depth_numpy -- the yardstick of the GPU tests -- to the restatement of the reference's encoder."""
import threading

import numpy as np
import pytest

import pileup_utils as pu
from coverage_cases import depth_numpy
from pepper_amd.variant import Coverage


# ---- parse_bins ------------------------------------------------------------------------------------------------------
def test_default_bins_and_labels():
    bins, labels = Coverage.parse_bins(None, 3)
    assert bins.dtype == np.int32 and bins.tolist() == [0, 1, 3] and labels == ["NO_COVERAGE", "LOW_COVERAGE", "CALLABLE"]
    bins, labels = Coverage.parse_bins(None, 2.5)                       # cov >= 2.5 iff cov >= 3
    assert bins.tolist() == [0, 1, 3] and labels == ["NO_COVERAGE", "LOW_COVERAGE", "CALLABLE"]
    bins, labels = Coverage.parse_bins("", 2)
    assert bins.tolist() == [0, 1, 2] and labels == ["NO_COVERAGE", "LOW_COVERAGE", "CALLABLE"]
    # duplicates removed: with a threshold of 1 no depth is LOW_COVERAGE, with 0 every depth is CALLABLE
    assert Coverage.parse_bins(None, 1)[0].tolist() == [0, 1] and Coverage.parse_bins(None, 1)[1] == ["NO_COVERAGE", "CALLABLE"]
    assert Coverage.parse_bins(None, 0)[0].tolist() == [0] and Coverage.parse_bins(None, 0)[1] == ["CALLABLE"]


def test_custom_bins_get_mosdepth_labels():
    bins, labels = Coverage.parse_bins([0, 1, 5, 20])
    assert bins.tolist() == [0, 1, 5, 20] and labels == ["0:1", "1:5", "5:20", "20:inf"]
    assert Coverage.parse_bins("0, 1,5 ,20")[1] == labels
    assert Coverage.parse_bins((0,))[1] == ["0:inf"]
    assert Coverage.parse_bins(np.array([0, 3], np.int64))[0].tolist() == [0, 3]
    assert len(Coverage.parse_bins(range(8))[0]) == 8


@pytest.mark.parametrize("bins,entry", [
    (list(range(9)), "entry 8"), ([1, 2], "entry 0"), ([0, 5, 5], "entry 2"), ([0, 5, 4], "entry 2"), ([0, -1], "entry 1"),
    ("0,x", "entry 1"), ([0, 1.5], "entry 1"), ([0, 1 << 31], "entry 1"), ([], "no bin"),
])
def test_refused_bins_name_the_entry(bins, entry):
    with pytest.raises(ValueError) as err:
        Coverage.parse_bins(bins)
    assert entry in str(err.value)


def test_neither_bins_nor_threshold():
    with pytest.raises(ValueError):
        Coverage.parse_bins(None, None)


# ---- runs_numpy ------------------------------------------------------------------------------------------------------
def _runs(depths, first, bins, on_target=None):
    s, e, b = Coverage.runs_numpy(depths, first, bins, on_target)
    assert s.dtype == np.int64 and e.dtype == np.int64 and b.dtype == np.int32
    return list(zip(s.tolist(), e.tolist(), b.tolist()))


def test_runs_with_an_edge_on_the_first_and_the_last_row():
    #          100 101 102 103 104 105 106 107
    depths = [0, 3, 3, 7, 2, 2, 2, 0]
    assert _runs(depths, 100, [0, 1, 3]) == [(100, 101, 0), (101, 104, 2), (104, 107, 1), (107, 108, 0)]


def test_a_one_base_run_and_bounds_are_inclusive_below():
    assert _runs([5, 5, 4, 5, 5], 0, [0, 5]) == [(0, 2, 1), (2, 3, 0), (3, 5, 1)]
    assert _runs([0, 1, 2, 3, 4], 10, [0, 1, 3]) == [(10, 11, 0), (11, 13, 1), (13, 15, 2)]
    assert _runs([1000000], 7, [0, 1, 3]) == [(7, 8, 2)]               # the last bin is open above


def test_all_rows_in_one_bin_and_no_rows():
    assert _runs([9] * 600, 50, [0, 1, 3]) == [(50, 650, 2)]
    assert _runs([0] * 3, 0, [0]) == [(0, 3, 0)]
    assert _runs([], 5, [0, 1]) == []


def test_sentinel_rows():
    depths = [4, 4, 4, 4, 0, 0, 4]
    on = [False, True, True, False, False, True, True]
    assert _runs(depths, 20, [0, 1, 3], on) == [(20, 21, -1), (21, 23, 2), (23, 25, -1), (25, 26, 0), (26, 27, 2)]
    assert _runs(depths, 20, [0, 1, 3], [False] * 7) == [(20, 27, -1)]
    bases, total = Coverage.totals_numpy(depths, [0, 1, 3], on)
    assert bases.tolist() == [1, 0, 3, 0, 0, 0, 0, 0] and total == 12
    bases, total = Coverage.totals_numpy(depths, [0, 1, 3])
    assert bases.tolist() == [2, 0, 5, 0, 0, 0, 0, 0] and total == 20


# ---- CoverageTrack ---------------------------------------------------------------------------------------------------
BINS, LABELS = [0, 1, 3], ["NO_COVERAGE", "LOW_COVERAGE", "CALLABLE"]


def _piece(contig, start, end, depths, on_target=None):
    """An interval (start, end inclusive) as a worker delivers it."""
    assert len(depths) == end - start + 1
    return (contig, (start, end), Coverage.runs_numpy(depths, start, BINS, on_target), Coverage.totals_numpy(depths, BINS, on_target))


def _track(pieces, contigs=("chrA", "chrB")):
    track = Coverage.CoverageTrack(contigs, BINS, LABELS)
    for piece in pieces:
        track.add(*piece)
    return track


def test_the_shared_boundary_belongs_to_the_interval_that_starts_there():
    # intervals [0, 10] and [10, 20]: position 10 is CALLABLE for the first and LOW for the second -- the second one's word counts
    first = _piece("chrA", 0, 10, [0] * 5 + [5] * 6)
    second = _piece("chrA", 10, 20, [2] * 4 + [5] * 7)
    assert _track([first, second]).finish() == [("chrA", 0, 5, 0), ("chrA", 5, 10, 2), ("chrA", 10, 14, 1), ("chrA", 14, 21, 2)]


def test_a_trimmed_run_that_becomes_empty_is_dropped():
    # the first interval's last run is the shared position alone
    first = _piece("chrA", 0, 10, [5] * 10 + [0])
    second = _piece("chrA", 10, 20, [5] * 11)
    assert _track([first, second]).finish() == [("chrA", 0, 21, 2)]


def test_runs_merge_across_intervals_and_gaps_do_not():
    a = _piece("chrA", 0, 10, [5] * 11)
    b = _piece("chrA", 10, 20, [5] * 6 + [0] * 5)
    c = _piece("chrA", 20, 30, [0] * 11)
    d = _piece("chrA", 40, 50, [0] * 11)                               # (the interval 30 - 40 was dropped at planning)
    assert _track([a, b, c, d]).finish() == [("chrA", 0, 16, 2), ("chrA", 16, 31, 0), ("chrA", 40, 51, 0)]


def test_contig_order_is_the_fastas_and_sentinels_are_dropped(tmp_path):
    on = [True] * 3 + [False] * 5 + [True] * 3
    pieces = [_piece("chrA", 0, 10, [5] * 11, on), _piece("chrB", 0, 10, [1] * 11), _piece("chrA", 10, 20, [5] * 11)]
    track = _track(pieces, contigs=("chrB", "chrA"))
    want = [("chrB", 0, 11, 1), ("chrA", 0, 3, 2), ("chrA", 8, 21, 2)]
    assert track.finish() == want
    path = tmp_path / "out.bed"
    assert track.write(str(path)) == want
    assert path.read_text() == "chrB\t0\t11\tLOW_COVERAGE\nchrA\t0\t3\tCALLABLE\nchrA\t8\t21\tCALLABLE\n"
    bases, mean = track.summary()
    assert bases == [0, 11, 16]
    # the totals as the intervals reported them: 6 + 11 + 11 on-target positions, depths 30 + 11 + 55
    assert mean == pytest.approx(96 / 28)
    assert "LOW_COVERAGE 11" in track.log_line() and "CALLABLE 16" in track.log_line()
    with pytest.raises(ValueError):
        track.add("chrC", (0, 1), ([0], [2], [0]))


def test_the_track_does_not_depend_on_the_order_of_delivery():
    rng = np.random.default_rng(11)
    pieces = []
    for contig in ("chrA", "chrB"):
        for start in range(0, 400, 40):
            pieces.append(_piece(contig, start, start + 40, rng.integers(0, 5, 41).tolist()))
    want = _track(pieces).finish()
    assert len(want) > 40
    for seed in range(3):
        order = np.random.default_rng(seed).permutation(len(pieces))
        assert _track([pieces[k] for k in order]).finish() == want
    # ... nor on the threads that deliver
    track = Coverage.CoverageTrack(("chrA", "chrB"), BINS, LABELS)
    workers = [threading.Thread(target=lambda k=k: [track.add(*p) for p in pieces[k::4]]) for k in range(4)]
    for w in workers:
        w.start()
    for w in workers:
        w.join()
    assert track.finish() == want


# ---- depth_numpy against the restatement of the reference's encoder ------------------------------------------------------
@pytest.mark.parametrize("over", [dict(), dict(min_snp_baseq=10, min_indel_baseq=10)])
def test_depth_numpy_is_the_depth_of_every_candidate(over):
    """At every candidate of the restated encoder, depth_numpy equals the candidate's depth (CandidateImageSummary.depth is
    coverage_vector at its position, unclamped below MAXC).  ~30x, so that the clamp is not reached -- asserted."""
    rng = np.random.default_rng(2024)
    start, length = 50_000, 3000
    ref = pu.random_reference(rng, length)
    sites = {start + int(p): ("ACGT"[(("ACGT".index(ref[p])) + 1) % 4], 0.5) for p in rng.choice(np.arange(50, length - 50), 60, replace=False)}
    indels = {start + 700: ("I", "GATT", 0.5), start + 1500: ("D", 5, 0.5), start + 2200: ("I", "C", 0.6)}
    reads = pu.simulate_reads(rng, ref, start, n_reads=30 * length // 500, read_len=(300, 700), snp_sites=sites, indel_sites=indels,
                              low_q_rate=0.2, skip_rate=0.002)
    assert any(r["mapq"] == 0 for r in reads)
    params = dict(pu.ONT_PARAMS)
    params.update(over)
    lo, hi = start + 100, start + length - 101                          # the candidate window is narrower than the region
    out = pu.run_variant(pu.load_restatement(), pu.FlatPileup(start, start + length - 1, ref, reads), pu.make_params(lo, hi, **over))
    depth = depth_numpy(reads, start, start + length - 1, params["min_snp_baseq"], params["min_indel_baseq"], 0)
    assert len(out["positions"]) > 80
    # raw coverage ~30x (fewer bases pass a min_snp_baseq of 10): the depths stay below the int8 clamp MAXC = 125 of candidates.h
    assert depth[200:-200].mean() > 10 and depth.max() < 125 and out["depths"].max() < 125
    kinds = {c[0] for c in out["candidates"]}
    assert kinds == {"1", "2", "3"}
    assert np.array_equal(depth[out["positions"] - start], out["depths"].astype(np.int64))
    # the rescue rule of insert anchors is exercised: some position's depth exceeds its count of good aligned bases
    plain = depth_numpy(reads, start, start + length - 1, params["min_snp_baseq"], 1e18, 0)      # (no insert passes the indel rule)
    assert (depth - plain).min() >= 0 and (depth - plain).sum() > 0
