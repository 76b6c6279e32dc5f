"""The expectation of tests/test_gpu_realign_cases.py pinned on the CPU: on every hand-built read of tests/realign_cases.py the
restatement (oracle/ssw_oracle.cpp) equals the reference's own SSW build (oracle/_ref/libref_ssw.so), a committed golden holds
what that build gave (the check that still runs where the build is absent), and every case's `expect` -- the edge it exists
for -- holds on the restatement's own result: a condition, not a measurement.  An edit of the catalogue that moves a case off
its edge fails here, so the GPU module cannot pass by missing one.  CPU only; exact integer parity."""
import importlib.util
import os

import numpy as np
import pytest

import realign_cases as rc
from conftest import need_reference_build
from oracle import ssw

GOLDEN_NAME = "realign_edge_cases.npz"


@pytest.fixture(scope="module")
def families():
    return {name: fn() for name, fn in rc.FAMILIES.items()}


@pytest.fixture(scope="module")
def restated(families):
    """{family: {case: ssw.align's tuple}}: computed once."""
    return {fam: {name: ssw.align(c[1][c[2] - c[0]:], c[3]) for name, c in cases.items()} for fam, cases in families.items()}


@pytest.fixture(scope="module")
def maker(golden_dir):
    spec = importlib.util.spec_from_file_location("make_golden_realign_cases", os.path.join(golden_dir, "make_golden_realign_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("family", sorted(rc.FAMILIES))
def test_restatement_equals_reference_build_on_the_catalogue(families, restated, family):
    if not ssw.have_reference():
        need_reference_build("oracle/_ref/libref_ssw.so")
    for name, (start, window, pos, seq, _) in families[family].items():
        want = ssw.align_reference(window[pos - start:], seq)
        got = restated[family][name]
        assert want[0] > 1 and got[:6] == want, (family, name, got[:5], want[:5])


def test_restatement_against_the_committed_golden(families, restated, golden_dir):
    g = np.load(os.path.join(golden_dir, GOLDEN_NAME), allow_pickle=False)
    assert str(g["input_sha256"]) == rc.input_digest(families), "the catalogue's inputs changed: re-make the golden"
    seen = 0
    for fam, cases in families.items():
        assert str(g[fam + "__names"]).split("|") == list(cases)
        cigars = str(g[fam + "__cigars"]).split("|")
        for k, (name, (start, window, pos, seq, _)) in enumerate(cases.items()):
            score, rb, re_, qb, qe, cigar, _wide = restated[fam][name]
            assert int(g[fam + "__status"][k]) == 1 and score == int(g[fam + "__score"][k]), (fam, name)
            assert (pos + rb, pos + re_) == (int(g[fam + "__pos"][k]), int(g[fam + "__pos_end"][k])), (fam, name)
            assert cigar == cigars[k], (fam, name)
            seen += 1
    assert seen == sum(len(c) for c in families.values()) and len(g.files) == 1 + 6 * len(families)


def test_golden_reproduces_from_its_script_and_stays_small(golden_dir, maker):
    """What tests/golden/make_golden_realign_cases.py would write today is what is committed; results only, a few kilobytes."""
    if not ssw.have_reference():
        need_reference_build("oracle/_ref/libref_ssw.so")
    want = maker.golden_arrays()
    g = np.load(os.path.join(golden_dir, GOLDEN_NAME), allow_pickle=False)
    assert sorted(g.files) == sorted(want)
    for key, value in want.items():
        assert g[key].dtype == value.dtype and np.array_equal(g[key], value), key
    assert os.path.getsize(os.path.join(golden_dir, GOLDEN_NAME)) < 32 * 1024


# ---- what the catalogue promises -----------------------------------------------------------------------------------------------
def _properties(result, m):
    score, rb, re_, qb, qe, cigar, wide = result
    ops = ssw.parse_cigar(cigar)
    rows = -(-m // 16) * 16
    return dict(score=score, wide=wide, gaps=[(o, n) for o, n in ops if o in (rc.I, rc.D)], bw=abs((re_ - rb + 1) - (qe - qb + 1)) + 1,
                strip=-(-rows // 64), lds_form=rows > 1536, cigar=cigar, n2=re_ - rb + 1,
                fits=rc.band_lds_bytes(re_ - rb + 1, qe - qb + 1, 1) <= rc.BAND_LDS_LIMIT)


@pytest.mark.parametrize("family", sorted(rc.FAMILIES))
def test_every_case_hits_the_edge_it_exists_for(families, restated, family):
    for name, case in families[family].items():
        expect = case[4]
        have = _properties(restated[family][name], len(case[3]))
        assert expect and set(expect) <= set(have), (family, name)
        for key, value in expect.items():
            assert have[key] == value, (family, name, key, have[key], value)


def test_catalogue_shapes(families, restated):
    """The edges, counted: both sides of the 8-bit switch; every ladder step with a read on either side; gaps either side of the
    129- and 257-slot rows and of the 64- and 128-cell chunk ends; the doubling past 64; both branches of the stride; the
    three-wavefront LDS need of the longest reads on either side of the limit."""
    sw = {name: restated["switch"][name] for name in families["switch"]}
    assert sorted({r[0] for r in sw.values()}) == [240, 244, 246, 248, 250, 252, 256]
    assert {r[0] for r in sw.values() if not r[6]} == {240, 244, 246, 248} and {r[0] for r in sw.values() if r[6]} == {250, 252, 256}
    assert sw["sub65"][5] == "32=1X32=" and sw["del65"][5] == "40=1D25="

    lad = families["ladder"]
    lengths = sorted({len(c[3]) for c in lad.values()})
    assert lengths == sorted(rc.LADDER_LENGTHS) and len(lengths) == 51
    for m in lengths:
        mine = [n for n, c in lad.items() if len(c[3]) == m]
        assert "copy%d" % m in mine and (len(mine) == 3 or m < 33), (m, mine)
    strips = {c[4]["strip"] for c in lad.values()}
    assert strips == set(range(1, 26))                                             # 1 .. 24 in registers, 25 = 1 552 rows in LDS
    for k in range(1, 13):
        assert [lad["copy%d" % (128 * k + d)][4]["strip"] for d in (-1, 0, 1)] == [2 * k, 2 * k, 2 * k + 1]
    assert [lad["copy%d" % m][4]["lds_form"] for m in (1535, 1536, 1537)] == [False, False, True]
    assert all(rc.strip_of(len(c[3])) == c[4]["strip"] for c in lad.values())
    # the replaced bases make gaps and mismatches next to the segment start
    with_gap = sum(1 for n in lad if not n.startswith("copy") and any(ch in restated["ladder"][n][5] for ch in "ID"))
    assert with_gap >= 40, with_gap

    bs = families["band_single"]
    assert len(bs) == 2 * len(rc.BAND_GAPS) and {c[4]["bw"] for c in bs.values()} == {g + 1 for g in rc.BAND_GAPS}
    for edge in (64, 128, 256):                        # bw - 1 = g: 2 g + 1 slots against 129 and 257; chunk ends
        assert {edge - 1, edge, edge + 1} <= set(rc.BAND_GAPS)
    bd = families["band_doubling"]
    assert [c[4]["gaps"][0][1] for c in bd.values()] == list(rc.DOUBLING_GAPS) and all(c[4]["bw"] == 1 for c in bd.values())
    assert sum(1 for L in rc.DOUBLING_GAPS if L > 64) == 4 and sum(1 for L in rc.DOUBLING_GAPS if L > 128) == 1

    bm = families["band_wider_than_matrix"]
    strides = [(2 * c[4]["bw"] + 1, restated["band_wider_than_matrix"][n][2] - restated["band_wider_than_matrix"][n][1] + 1) for n, c in bm.items()]
    assert [s for s, _ in strides] == list(range(115, 128, 2)) and {n for _, n in strides} == {120}

    lg = families["longest"]
    assert max(len(c[3]) for c in lg.values()) == 4000 and max(r[0] for r in restated["longest"].values()) == 16_000
    need = {}
    for name in lg:
        _, rb, re_, qb, qe = restated["longest"][name][:5]
        need[name] = rc.band_lds_bytes(re_ - rb + 1, qe - qb + 1, 3)
    assert need["del64"] == 154_592 and need["del200"] > rc.BAND_LDS_LIMIT           # three wavefronts do not fit: one does
    assert need["copy4000"] <= rc.BAND_LDS_LIMIT and 64 * 1024 < need["del200_of_3000"] <= rc.BAND_LDS_LIMIT
    assert rc.band_lds_bytes(4064, 4000, 1) < 64 * 1024
    bl = families["band_limit"]
    assert bl["under"][4]["fits"] and not bl["over"][4]["fits"] and len(bl["over"][3]) == 4000
