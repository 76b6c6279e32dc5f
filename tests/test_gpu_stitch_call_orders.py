"""The order of calls on one pa_stitcher handle after a single finish: edits, gate, fill, withheld and variants in the orders the
writers never take, every step against the numpy twins' bytes (Edits.records_numpy, Stitch.gate_numpy, Variants.records_numpy) and
against what pa_stitcher_stats promises for table_bytes -- 16 bytes per live edit or withheld record, 4 per position and 1 or 2
per letter of a live fill, the variants' tables counted once and gone with the fill they describe.

One table of about 1 100 positions: its slots cross the 1 024-slot scan block, a run of uncovered positions is closed by the first
slot of the second block, an insert column stands in the first, the draft has lower-case letters and Ns, and edits of every kind
lie on both sides of the border with phreds on both sides of the gate.  One piece (threads = 1) for the orders that fill, two
pieces for those that do not."""
import ctypes

import numpy as np
import pytest

import polish_edits_cases as cases
import test_polish_gate_cpu as gcases
from pepper_amd import _lib
from pepper_amd.polish import Edits, Stitch, Variants
from pepper_amd.polish.DeviceStitch import DeviceStitcher

pytestmark = pytest.mark.gpu

B = 1024                                                             # slots per workgroup of the scans (asserted below)
Q = 20
FIRST, SIZE, RUN = 7, 1110, 10
KEYS = [("memory", "c-0-%d" % k, 0, k) for k in (1, 2, 3)]           # three regions: one piece with threads = 1, two with 3
OK, INVALID = _lib.PA_OK, _lib.PA_ERR_INVALID


def _build():
    rng = np.random.default_rng(1024)
    draft = gcases._marked_draft(rng, FIRST + SIZE + 9)
    table = {(p, 0): (cases.CODE.get(draft[p].upper(), 1), int(rng.integers(0, 256))) for p in range(FIRST, FIRST + SIZE)}
    for k, p in enumerate(range(FIRST + 8, FIRST + SIZE - 3, 5)):    # every kind, at phreds on both sides of the gate
        phred = (0, 1, 19, 20, 21, 254, 255)[k % 7]
        if k % 3 == 0:
            table[(p, 0)] = (cases.other(draft[p], 1 + k % 3), phred)
        elif k % 3 == 1:
            table[(p, 0)] = (0, phred)
        else:
            table[(p, 1)] = (1 + k % 4, phred)
    for i in range(1, 11):                                           # an insert column, two slots of it without a base
        table[(FIRST + 40, i)] = (i % 5, (5, 19, 20, 200)[i % 4])
    # the run of uncovered positions: behind slot B - 1, so that the first slot of the second workgroup closes it
    width = {}
    for p, i in table:
        width[p] = max(width.get(p, 0), i + 1)
    slots, at = 0, FIRST
    while slots < B:
        slots += width[at]
        at += 1
    assert slots == B and all(width[p] == 1 for p in range(at - 2, at + RUN + 2))
    for p in range(at, at + RUN):
        del table[(p, 0)]
    keys = sorted(table)
    assert keys[B - 1] == (at - 1, 0) and keys[B] == (at + RUN, 0) and len(keys) > B + 60
    return draft, table, at


@pytest.fixture(scope="module")
def case():
    """(draft, table, first position of the uncovered run); shared, and left as it is."""
    assert DeviceStitcher.limits()["scan_block"] == B
    return _build()


def _pieces(table, n_pieces):
    """The table as the pieces the plan makes of the three regions: all of it, or regions 1 and 2 | region 3."""
    cut = FIRST + 400
    if n_pieces == 1:
        return [table]
    return [{k: v for k, v in table.items() if k[0] < cut}, {k: v for k, v in table.items() if k[0] >= cut}]


def _feed(st, table):
    """Region k holds the positions of its third of the range (every region starts at 0: nothing is dropped)."""
    bounds = [FIRST, FIRST + 200, FIRST + 400, FIRST + SIZE]
    for k, key in enumerate(KEYS):
        part = sorted(e for e in table if bounds[k] <= e[0] < bounds[k + 1])
        n = (len(part) + 60) // 61
        pos, idx = -np.ones((n, 61), np.int64), -np.ones((n, 61), np.int64)
        lab, phr = np.zeros((n, 61), np.uint8), np.zeros((n, 61), np.uint8)
        for j, (p, i) in enumerate(part):
            pos[j // 61, j % 61], idx[j // 61, j % 61] = p, i
            lab[j // 61, j % 61], phr[j // 61, j % 61] = table[(p, i)]
        st.add("c", [key] * n, list(range(n)), pos, idx, lab, phr)


def _twin(tables, draft, q=None, fill=False):
    """The twins piece by piece -> (sequence, edit records, withheld records or None), placed as the contig's."""
    stored = np.frombuffer(draft.encode(), np.uint8)
    text, records, withheld, at = [], [np.zeros(0, Edits.EDIT_DTYPE)], [np.zeros(0, Edits.EDIT_DTYPE)], 0
    for k, table in enumerate(tables):
        if q:
            positions, indices, labels, phred, held = gcases._gate(table, draft, q, filled=fill)
            withheld.append(Edits.place(held, k, at))
        else:
            positions, indices, labels, phred = gcases._arrays(table)
        letters = Stitch._DECODE[labels]
        piece = letters[letters != 0]
        if fill:
            piece, _ = Stitch.filled_piece(stored, int(positions[0]), positions, letters, None)
        records.append(Edits.place(Edits.records_numpy(positions, indices, labels, phred, draft, filled=fill), k, at))
        text.append(piece.tobytes().decode())
        at += len(text[-1])
    return ''.join(text), np.concatenate(records), np.concatenate(withheld) if q else None


class _Calls(object):
    """The C entry points on a DeviceStitcher's handle."""

    def __init__(self, st, n_pieces):
        self.lib, self.st = _lib.load(), st
        self.n, self.kinds = ctypes.c_int64(), (ctypes.c_int64 * 6)()
        self.total, self.gate_counts, self.length = ctypes.c_int64(), (ctypes.c_int64 * 4)(), (ctypes.c_int64 * n_pieces)()
        self.filled, self.fill_counts = ctypes.c_int64(), (ctypes.c_int64 * 2)()
        self.n_variants, self.variant_counts = ctypes.c_int64(), (ctypes.c_int64 * 5)()

    def edits(self, draft, length):
        rc = self.lib.pa_stitcher_edits(self.st.handle, draft, length, ctypes.byref(self.n), self.kinds)
        assert rc == OK, self.error()
        records = np.zeros(self.n.value, Edits.EDIT_DTYPE)
        assert self.lib.pa_stitcher_take_edits(self.st.handle, records.ctypes.data, len(records)) == OK
        return records

    def gate(self, draft, q):
        return self.lib.pa_stitcher_gate(self.st.handle, draft, len(draft), q, self.length, ctypes.byref(self.total), self.gate_counts)

    def fill(self, draft, length):
        return self.lib.pa_stitcher_fill(self.st.handle, draft, length, ctypes.byref(self.filled), self.fill_counts)

    def withheld(self):
        records = np.zeros(self.gate_counts[0], Edits.EDIT_DTYPE)
        assert self.lib.pa_stitcher_take_withheld(self.st.handle, records.ctypes.data, len(records)) == OK, self.error()
        return records

    def variants(self, draft, length):
        return self.lib.pa_stitcher_variants(self.st.handle, draft, length, ctypes.byref(self.n_variants), self.variant_counts)

    def take_variants(self):
        records = np.zeros(self.n_variants.value, Variants.VARIANT_DTYPE)
        assert self.lib.pa_stitcher_take_variants(self.st.handle, records.ctypes.data, len(records)) == OK, self.error()
        return records

    def take(self, n):
        buf = ctypes.create_string_buffer(max(1, n))
        assert self.lib.pa_stitcher_take(self.st.handle, buf, n) == OK, self.error()
        return buf.raw[:n].decode()

    def no_edits(self):
        return self.lib.pa_stitcher_take_edits(self.st.handle, None, 0) == INVALID and b"has not run" in self.error()

    def no_variants(self):
        return self.lib.pa_stitcher_take_variants(self.st.handle, None, 0) == INVALID and b"has not run" in self.error()

    def error(self):
        return self.lib.pa_last_error()

    def bytes(self):
        return self.st.stats()["table_bytes"]


def _same(records, want):
    assert records.dtype == want.dtype and len(records) == len(want) and records.tobytes() == want.tobytes()


def _kinds(records):
    return [0] + [int((records["kind"] == k).sum()) for k in range(1, 6)]


@pytest.mark.parametrize("n_pieces", [1, 2])
def test_the_orders_that_do_not_fill(case, n_pieces):
    text, table, run_at = case
    draft, tables = text.encode(), _pieces(table, n_pieces)
    sequence, records, _ = _twin(tables, text)
    gated, gated_records, withheld = _twin(tables, text, Q)
    assert len(records) > 300 and len(withheld) > 60 and len(gated_records) > 100 and gated != sequence
    for want in (records, gated_records):                            # the run's GAP pair, and every kind on both sides of it
        pair = np.flatnonzero(want["kind"] == Edits.GAP_OPEN)
        assert len(pair) == 1 and int(want["position"][pair[0]]) == run_at
        assert all(k in want["kind"][:pair[0]] and k in want["kind"][pair[0] + 2:] for k in (Edits.SUB, Edits.DEL, Edits.INS))
    with DeviceStitcher(0) as st:
        c = _Calls(st, n_pieces)
        _feed(st, table)
        # edits with a draft of the caller's, twice: the same records, counted once
        assert st.finish("c", 3 if n_pieces == 2 else 1, KEYS, qualities=True)[0] == sequence
        assert len(st.pieces()) == n_pieces and st.stats()["slots"] == len(table) > B
        bare = c.bytes()
        for _ in range(2):
            _same(c.edits(draft, len(draft)), records)
            assert list(c.kinds) == _kinds(records) and c.bytes() == bare + 16 * len(records)
        # gate, edits from the gate's draft, the withheld records twice, edits again; a second gate is refused
        assert c.gate(draft, Q) == OK and c.total.value == len(gated) and c.take(len(gated)) == gated
        assert list(c.gate_counts) == [len(withheld)] + Edits.kind_counts(withheld) and c.no_edits()
        gate_bytes = bare + 16 * len(withheld) + len(gated) - len(sequence)
        assert c.bytes() == gate_bytes
        _same(c.edits(None, len(draft)), gated_records)
        assert c.bytes() == gate_bytes + 16 * len(gated_records)
        _same(c.withheld(), withheld)
        _same(c.withheld(), withheld)
        _same(c.edits(None, len(draft)), gated_records)
        assert c.bytes() == gate_bytes + 16 * len(gated_records)
        assert c.gate(draft, 30) == INVALID and b"a gate already ran" in c.error()
        assert c.take(len(gated)) == gated and c.bytes() == gate_bytes + 16 * len(gated_records)
        _same(c.withheld(), withheld)
        _same(c.edits(draft, len(draft)), gated_records)
        # a finish drops all of it
        assert st.finish("c", 3 if n_pieces == 2 else 1, KEYS, qualities=True)[0] == sequence and c.bytes() == bare
        assert c.no_edits() and c.edits(draft, len(draft)).tobytes() == records.tobytes()


def test_the_orders_that_fill(case):
    text, table, run_at = case
    draft, tables, n = text.encode(), [table], len(text)
    sequence, _, _ = _twin(tables, text)
    filled, filled_records, _ = _twin(tables, text, fill=True)
    gated, gated_records, withheld = _twin(tables, text, Q)
    gated_filled, gated_filled_records, withheld_filled = _twin(tables, text, Q, fill=True)
    assert len(filled) == len(sequence) + FIRST + RUN + 9 and withheld_filled.tobytes() != withheld.tobytes()
    want_variants, want_counts = Variants.records_numpy(filled_records, text, filled, True)
    want_gated_variants, want_gated_counts = Variants.records_numpy(gated_filled_records, text, gated_filled, True)
    assert len(want_variants) > len(want_gated_variants) > 50
    with DeviceStitcher(0) as st:
        c = _Calls(st, 1)
        _feed(st, table)
        positions = SIZE

        def fill_bytes(letters):
            return 4 * positions + 2 * len(letters)

        # gate -> edits -> withheld -> fill -> withheld (shifted once) -> withheld -> edits -> variants x 2 -> fill -> edits
        assert st.finish("c", 1, KEYS, qualities=True)[0] == sequence and st.stats()["positions"] == positions
        bare = c.bytes()
        assert c.gate(draft, Q) == OK and c.take(c.total.value) == gated
        gate_bytes = bare + 16 * len(withheld) + len(gated) - len(sequence)
        assert c.bytes() == gate_bytes
        _same(c.edits(None, n), gated_records)
        assert c.bytes() == gate_bytes + 16 * len(gated_records)
        _same(c.withheld(), withheld)
        assert c.fill(None, n) == OK and c.filled.value == len(gated_filled) and c.take(len(gated_filled)) == gated_filled
        assert c.no_edits() and c.bytes() == gate_bytes + fill_bytes(gated_filled)
        _same(c.withheld(), withheld_filled)
        _same(c.withheld(), withheld_filled)
        _same(c.edits(None, n), gated_filled_records)
        live = gate_bytes + fill_bytes(gated_filled) + 16 * len(gated_filled_records)
        assert c.bytes() == live
        assert c.variants(None, n) == OK and list(c.variant_counts) == want_gated_counts
        _same(c.take_variants(), want_gated_variants)
        with_variants = c.bytes()
        assert with_variants > live
        assert c.variants(None, n) == OK and c.bytes() == with_variants
        _same(c.take_variants(), want_gated_variants)
        assert c.fill(None, n) == OK and c.take(len(gated_filled)) == gated_filled
        assert c.no_edits() and c.no_variants() and c.bytes() == gate_bytes + fill_bytes(gated_filled)
        _same(c.edits(None, n), gated_filled_records)
        assert c.bytes() == live
        _same(c.withheld(), withheld_filled)
        # a gate behind a fill is refused, and the handle is as it was
        assert c.gate(draft, Q) == INVALID and b"a gate already ran" in c.error()
        assert c.take(len(gated_filled)) == gated_filled and c.bytes() == live

        # fill -> edits -> variants -> edits with a draft of its own -> variants without one (refused) -> variants with it
        assert st.finish("c", 1, KEYS, qualities=True)[0] == sequence and c.bytes() == bare
        assert c.fill(draft, n) == OK and c.take(c.filled.value) == filled and c.bytes() == bare + fill_bytes(filled)
        _same(c.edits(None, n), filled_records)
        live = bare + fill_bytes(filled) + 16 * len(filled_records)
        assert c.bytes() == live
        assert c.variants(None, n) == OK and list(c.variant_counts) == want_counts
        _same(c.take_variants(), want_variants)
        with_variants = c.bytes()
        assert with_variants > live
        _same(c.edits(draft, n), filled_records)
        assert c.bytes() == with_variants
        assert c.variants(None, n) == INVALID and b"null draft, and the copy the fill uploaded is gone" in c.error()
        assert c.bytes() == with_variants
        assert c.variants(draft, n) == OK and list(c.variant_counts) == want_counts and c.bytes() == with_variants
        _same(c.take_variants(), want_variants)
        assert c.gate(draft, Q) == INVALID and b"a fill already ran" in c.error()
        assert c.take(len(filled)) == filled and c.bytes() == with_variants
        _same(c.edits(None, n), filled_records)
        assert c.fill(draft, n) == OK and c.no_variants() and c.bytes() == bare + fill_bytes(filled)
