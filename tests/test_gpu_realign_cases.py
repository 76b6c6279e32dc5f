"""The read re-aligner's kernels (pepper_amd/csrc/realign.hip) on the hand-built reads of tests/realign_cases.py: both sides of
the 8-bit to 16-bit switch, a read on either side of every step of the strip ladder, gaps around the 129- and 257-slot first rows
and the 64-cell chunk ends, the half width doubling from 1 past 64 (the kernel's own ST_WIDER), both branches of
stride = min(2 bw + 1, n), window ends, the longest read and the largest score, the band stage's stated limit; host-fed (a
family per call, all families in one call, each kernel form forced in a child process) and device-fed (the reads as BAM
records through the polish chain).  The expectation is the restatement, which tests/test_realign_cases_cpu.py pins to the
reference's SSW build on exactly these reads, and the committed golden (for the device-fed form the reference builds
themselves).  Integer work: every field and every operation identical, no tolerances.

Found: before this catalogue, a 4 000-base read with a deletion of 64 or more (longest/del64, del200) made the whole call fail
with "alignment too long for the band stage": the full band rows of three wavefronts need more LDS than a workgroup gets.  Such
a round now runs with one wavefront per read; what one wavefront cannot hold either (band_limit/over) is refused by the limit
include/pepper_amd_realign.h states.

Deliberate breaks, each tried once on a scratch copy of realign.hip against this module (not committed):
    - the chunk carry dropped (`carry_a = max(carry_a, bcast63(pm))` removed from band_kernel): 9 of 13 failed --
      test_a_family_in_a_call_of_its_own[band_single], [band_doubling] and [longest], test_all_families_in_one_call,
      test_the_band_stage_refuses_only_what_its_header_says, the three children of test_every_case_in_the_forced_kernel_forms,
      test_device_fed_chain_on_the_planted_reads.
    - first_band_width returning 128 and 256: nothing failed, and nothing can: a band whose 2 bw + 1 slots do not fit the row gets
      full rows at layout time or the kernel's ST_WIDER verdict, and the next round gives the same alignment one launch later.  The
      edit costs time, not results; no output of the re-aligner tells in which round a read finished.
    - the switch threshold `run_max + BIAS >= 255` moved to 257 in all four passes: nothing failed.  Only a read whose score is
      exactly 250 changes its pass, and the kernels do not saturate, so it must differ between the 16- and the 8-segment layout to
      show: switch/sub65 does not, and neither did any of 2 900 further reads of score 250 (one or two edits at every row of 64 ..
      99 bases) tried in the restatement with the same edit.  The edge is covered (248 narrow, 250 wide, with and without gaps);
      the edit is not observable in what the re-aligner returns.
    - REG_ROWS raised by 64: not run.  With it the host passes no LDS for ladder's 1 537-base reads (1 552 padded rows) while the
      kernel still takes the LDS form for them (25 rows per lane, no register strip that long): every access of the column lies
      outside the workgroup's allocation.  That is an out-of-bounds kernel by construction; it was not put on a shared GPU."""
import os

import numpy as np
import pytest

import bam_utils as bu
import pileup_utils as pu
import realign_cases as rc
from conftest import need_reference_build
from oracle import ssw
from test_gpu_realign import _assert_same, _gpu_align

pytestmark = pytest.mark.gpu

CHILD = "PEPPER_AMD_REALIGN_CASES_CHILD"
CALL_FAMILIES = tuple(sorted(set(rc.FAMILIES) - {"band_limit"}))
_families, _want, _golden = {}, {}, {}


def family(name):
    if name not in _families:
        _families[name] = rc.FAMILIES[name]()
    return _families[name]


def want(name):
    """The restatement's results of a family, in the order of its cases: computed once, never changed."""
    if name not in _want:
        _want[name] = tuple(ssw.realign_reads(window, start, [pos], [seq])[0] for start, window, pos, seq, _ in family(name).values())
    return _want[name]


def golden(name, golden_dir):
    """What the reference's SSW build gave (tests/golden/realign_edge_cases.npz)."""
    if not _golden:
        g = np.load(os.path.join(golden_dir, "realign_edge_cases.npz"), allow_pickle=False)
        assert str(g["input_sha256"]) == rc.input_digest()
        for fam in rc.FAMILIES:
            cigars = str(g[fam + "__cigars"]).split("|")
            assert str(g[fam + "__names"]).split("|") == list(family(fam))
            _golden[fam] = tuple((int(g[fam + "__status"][k]), int(g[fam + "__score"][k]), int(g[fam + "__pos"][k]), int(g[fam + "__pos_end"][k]),
                                  ssw.parse_cigar(cigars[k])) for k in range(len(cigars)))
    return _golden[name]


def _check(out, names, golden_dir):
    expect, gold = [], []
    for name in names:
        expect += want(name)
        gold += golden(name, golden_dir)
    assert len(out["status"]) == len(expect)
    _assert_same(out, expect)
    _assert_same(out, gold)
    assert (out["status"] == 1).all()


# ---- host-fed ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CALL_FAMILIES)
def test_a_family_in_a_call_of_its_own(name, golden_dir):
    """A small call: sw_ends_kernel and band_kernel<3> unless the forms are forced (below)."""
    cases = family(name)
    start, window = rc.window_of(cases)
    out = _gpu_align(window, start, [c[2] for c in cases.values()], [c[3] for c in cases.values()])
    _check(out, [name], golden_dir)


def test_all_families_in_one_call(golden_dir):
    """One window per family through align_windows: strips of every size, narrow and wide reads, first rows and full rows in one
    job table."""
    from pepper_amd.polish.PEPPER import align_windows
    windows, which, pos, seqs = [], [], [], []
    for w, name in enumerate(CALL_FAMILIES):
        windows.append(rc.window_of(family(name)))
        for c in family(name).values():
            which.append(w)
            pos.append(c[2])
            seqs.append(c[3])
    blob = [s.encode() for s in seqs]
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(b) for b in blob], out=off[1:])
    out = align_windows(windows, which, pos, off, np.frombuffer(b"".join(blob), np.uint8), collapse_eqx=False)
    _check(out, CALL_FAMILIES, golden_dir)


def test_the_band_stage_refuses_only_what_its_header_says(golden_dir):
    """include/pepper_amd_realign.h: 13 n2 + m2 + 128 <= 153 600.  band_limit/under (n2 = 11 410) is aligned, band_limit/over
    (n2 = 11 566) is an error of the call, and the handle goes on."""
    from pepper_amd import _lib
    cases = family("band_limit")
    names = list(cases)
    assert names == ["under", "over"] and cases["under"][4]["fits"] and not cases["over"][4]["fits"]
    start, window, pos, seq, _ = cases["under"]
    out = _gpu_align(window, start, [pos], [seq])
    _assert_same(out, [want("band_limit")[0]])
    _assert_same(out, [golden("band_limit", golden_dir)[0]])
    assert int(out["pos_end"][0]) - int(out["pos"][0]) + 1 == cases["under"][4]["n2"]
    start, window, pos, seq, _ = cases["over"]
    with pytest.raises(_lib.PepperAmdError, match="too long for the band stage") as err:
        _gpu_align(window, start, [pos], [seq])
    assert err.value.code == _lib.PA_ERR_INVALID
    sw = family("switch")
    start, window = rc.window_of(sw)
    _check(_gpu_align(window, start, [c[2] for c in sw.values()], [c[3] for c in sw.values()]), ["switch"], golden_dir)


@pytest.mark.parametrize("single,band_waves", [("0", "1"), ("0", "3"), ("1", "1")])
def test_every_case_in_the_forced_kernel_forms(single, band_waves):
    """PA_REALIGN_SINGLE / PA_BAND_WAVES pin the kernel forms for a whole process: this module again through
    sw_ends_pair_kernel and band_kernel<1> (and the other mixes), each in a fresh child process."""
    import subprocess
    import sys
    if os.environ.get(CHILD) == "1":
        pytest.skip("the child run itself")
    env = dict(os.environ, PA_REALIGN_SINGLE=single, PA_BAND_WAVES=band_waves)
    env[CHILD] = "1"
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                         env=env, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-2000:]


# ---- device-fed: the reads as BAM records through the polish chain -----------------------------------------------------------------
HOMES = 9                                      # intervals 0 .. 8 of a 10 000-base draft: [1000 k - 100, 1000 k + 1100]; the tenth is [8900, 9999]


def _planted_reads(draft):
    """band_single, band_doubling and switch planted into the draft with their CIGARs, each wholly inside its home interval
    (the longest spans 979 draft bases from 1000 k + 120 on)."""
    shapes = [(n, s, g) for n, s, g, _ in rc.band_single_shapes()] + [(n, s, g) for n, s, g, _ in rc.band_doubling_shapes()] + \
             [(n, s, g) for n, s, _, _, g in rc.SWITCH_SHAPES]
    out = []
    for k, (name, shape, gaps) in enumerate(shapes):
        home = k % HOMES
        pos = 1000 * home + 120 + (k // HOMES) % 2
        seq, cigar, span = rc.plant(draft, pos, shape, salt=k)
        assert pos + span <= 1000 * home + 1100
        out.append(dict(pos=pos, reverse=bool(k % 2), mapq=60, seq=seq, qual=np.full(len(seq), 25, np.uint8), cigar=cigar,
                        case=name, gaps=gaps, home=home))
    return out


def test_device_fed_chain_on_the_planted_reads(tmp_path, monkeypatch):
    """jobs_of_reads_kernel, pair_jobs_kernel (forced forms), band_layout_kernel and -- for the reads whose half width passes
    64 -- the host-laid-out later rounds: the chain's chunks against the reference's SSW and SummaryGenerator builds and against
    the host form."""
    import test_gpu_polish_chain as pc
    from pepper_amd.polish.ImageGenerationUI import UserInterfaceSupport
    ref_enc = pu.load_reference_polish_encoder()
    if ref_enc is None or not ssw.have_reference():
        need_reference_build("oracle/_ref (polish encoder, SSW)")
    planted = []

    def extra(draft):
        planted.extend(_planted_reads(draft))
        return planted
    draft, reads, bam_path, fa_path = pc._dataset(tmp_path, 23, 10_000, 24, (300, 900), extra=extra)
    _, intervals = UserInterfaceSupport.make_intervals([("ctg1", None)], fa_path)
    assert len(intervals) == 10 and len(planted) == 2 * len(rc.BAND_GAPS) + len(rc.DOUBLING_GAPS) + len(rc.SWITCH_SHAPES)
    clipped = {k: bu.restated_get_reads(reads, start, end, False, 0) for k, (_, start, end) in enumerate(intervals)}
    assert all(clipped.values())                     # (every interval has reads: each writes its chunks)
    later_rounds = 0
    for r in planted:
        _, start, end = intervals[r["home"]]
        mine = [c for c in clipped[r["home"]] if c["name"] == r["name"]]
        assert len(mine) == 1 and mine[0]["seq"] == r["seq"] and mine[0]["pos"] == r["pos"] and mine[0]["cigar"] == r["cigar"], r["case"]
        # ... and against its interval's window the read keeps the gaps it was planted with
        score, rb, re_, qb, qe, cigar, wide = ssw.align(draft[r["pos"]:end + 20], r["seq"])
        assert [(o, n) for o, n in ssw.parse_cigar(cigar) if o in (rc.I, rc.D)] == r["gaps"], (r["case"], cigar)
        later_rounds += bool(r["gaps"]) and (abs((re_ - rb) - (qe - qb)) + 1 > 64 or (len(r["gaps"]) == 2 and r["gaps"][0][1] > 64))
    assert later_rounds >= 2 * sum(g >= 64 for g in rc.BAND_GAPS) + sum(g > 64 for g in rc.DOUBLING_GAPS)
    got = pc._make(bam_path, fa_path, str(tmp_path / "chain"), 1, True, monkeypatch)
    checked = 0
    for k, (_, start, end) in enumerate(intervals):
        checked += pc._check_interval(got, ref_enc, "ctg1", draft, start, end, clipped[k])
    assert checked == len(got) and checked >= 10
    host = pc._make(bam_path, fa_path, str(tmp_path / "host"), 1, False, monkeypatch)
    pc._assert_same(got, host)
