"""What the stitch changed: draft-to-consensus edits (opt-in: polish(..., edits=True) / PEPPER_AMD_POLISH_EDITS=1; not in the
reference).

The stitch holds, for every key (position, insert index) of a piece, the winning label, the winner's phred and the letter's place
in the consensus; the position is a coordinate of the draft.  A RECORD (EDIT_DTYPE, 16 bytes, `pa_stitch_edit` of
include/pepper_amd_encoder.h) is one key that differs from the draft, or one end of a run of positions no row covered:

    kind          where                          condition
    1 SUB         slot (p, 0)                    the winner is a base and differs from upper(draft[p]) (a draft letter outside
                                                 ACGT always differs)
    2 DEL         slot (p, 0)                    the winner is a gap, or the slot has no writer
    3 INS         slot (p, i > 0)                the winner is a base
    4 GAP_OPEN    position p inside the piece    p has no slot and p - 1 has one
    5 GAP_CLOSE   the same                       p has no slot and p + 1 has one (a run of one position: both, GAP_OPEN first)

Pieces in the order the consensus concatenates them, inside a piece the keys in order.  `offset` counts letters of the contig's
consensus: the record's own letter for SUB and INS, the letters in front of the record for the others.

records_numpy() makes them from the numpy merge's sorted last-write arrays (Stitch.small_chunk_stitch_numpy); the device makes
the same bytes from its tables (pa_stitcher_edits).  hunks() and write_edits() turn either into the text both forms write, and
apply() replays the records over the draft: it gives back the consensus, which is the check that needs no twin.

FILL (opt-in: polish(..., fill=True) / PEPPER_AMD_POLISH_FILL=1): the contig is merged as ONE piece and every position of the draft
that has no slot gives the draft's own letter, so the consensus is complete.  The records keep their layout and kinds; `offset`
counts letters of the FILLED consensus (the draft letters in front of the piece and the filled positions count), and a GAP pair's
offset is the first filled letter of its run.  The one piece is (first, last, filled length).  filled_hunks(), write_contig(...,
filled=True) and apply_filled() read such records: a run is a `filled` hunk with equal draft and polished intervals, and so are
[0, first) and (last, draft_length); `uncovered` and `duplicated` cannot occur.

GATE (opt-in: polish(..., min_quality=Q) / PEPPER_AMD_POLISH_MIN_QUALITY=Q): the SUB / DEL / INS edits whose winner has a phred
below Q are withheld before anything here reads the merge (Stitch.gate_numpy, pa_stitcher_gate), so the records are exactly the
applied edits.  The withheld ones come as records of the same layout -- letter the model's, offset the place of the kept draft
letter (SUB, DEL) or the letters in front of the slot (INS) -- which write_withheld() prints, one line each, into
<prefix>_pepper_polished.withheld.tsv; the summary line of the .edits.tsv then ends with withheld=<n>.
"""
import numpy as np

SUB, DEL, INS, GAP_OPEN, GAP_CLOSE = 1, 2, 3, 4, 5
EDIT_DTYPE = np.dtype([("position", "<u4"), ("offset", "<u4"), ("index", "<u2"), ("piece", "<u2"), ("kind", "u1"), ("draft", "u1"),
                       ("letter", "u1"), ("phred", "u1")])
assert EDIT_DTYPE.itemsize == 16
MAX_PIECES = 0xFFFF
HEADER = "#contig\tdraft_start\tdraft_end\tpolished_start\tpolished_end\tkind\tdraft\tpolished\tmin_phred\n"
HUNK_KINDS = ("sub", "ins", "del", "complex", "uncovered", "duplicated", "filled")
SUMMARY_KEYS = ("sub", "ins", "del", "complex_draft", "complex_polished", "uncovered", "duplicated")
_DECODE = np.frombuffer(b"\0ACGT", dtype=np.uint8)
_UPPER = bytes(c - 32 if 97 <= c <= 122 else c for c in range(256))


def edits_path(output_prefix):
    return output_prefix + '_pepper_polished.edits.tsv'


WITHHELD_HEADER = "#contig\tdraft_position\tinsert_index\tkind\tdraft\tmodel\tphred\tpolished_offset\n"
_WITHHELD_KINDS = {SUB: "sub", DEL: "del", INS: "ins"}


def withheld_path(output_prefix):
    return output_prefix + '_pepper_polished.withheld.tsv'


def write_withheld(file, contig, records):
    """One line per edit the min_quality gate kept back (Stitch.gate_numpy / pa_stitcher_gate), in the records' order: contig,
    draft position (0-based), insert index, kind, the draft's letter ('-' for ins), the model's letter ('-' for del), the winner's
    phred, and the offset in the polished contig -- of the kept draft letter for sub and del, of the letter behind the slot for ins."""
    records = np.asarray(records, dtype=EDIT_DTYPE)
    file.writelines("%s\t%d\t%d\t%s\t%s\t%s\t%d\t%d\n" % (contig, p, i, _WITHHELD_KINDS[k], chr(d) if d else "-", chr(c) if c else "-", q, o)
                    for p, o, i, _, k, d, c, q in records.tolist())


def kind_counts(records):
    """[SUB, DEL, INS] records."""
    kind = np.asarray(records, dtype=EDIT_DTYPE)["kind"]
    return [int((kind == k).sum()) for k in (SUB, DEL, INS)]


def upper_bytes(draft):
    """A draft span (str or bytes) as upper-case uint8."""
    if isinstance(draft, str):
        draft = draft.encode()
    return np.frombuffer(bytes(draft).translate(_UPPER), dtype=np.uint8)


def records_numpy(positions, indices, labels, phred, draft, draft_start=0, piece=0, offset=0, filled=False):
    """The records of ONE piece.  positions / indices / labels: its keys after the merge -- sorted by (position, index), one
    entry per key, labels 0..4 -- and phred the winners' (None: the contig has no qualities, every record gets 0).  draft: the
    draft letters from draft_start on, covering [positions[0], positions[-1]].  piece / offset: the piece's place among the
    contig's pieces and the letters in front of it.  filled: the records of the filled consensus -- the contig's one piece; every
    offset also counts the positions in front of the piece and the positions without a key in front of the record's own."""
    positions = np.asarray(positions, dtype=np.int64)
    if positions.size == 0:
        return np.zeros(0, EDIT_DTYPE)
    indices = np.asarray(indices, dtype=np.int64)
    letters = _DECODE[np.asarray(labels, dtype=np.int64)]
    phred = np.zeros(positions.size, np.int64) if phred is None else np.asarray(phred, dtype=np.int64)
    draft = upper_bytes(draft)
    if int(positions[-1]) - draft_start >= draft.size or int(positions[0]) < draft_start:
        raise ValueError("the draft span [%d, %d) does not cover the piece [%d, %d]" %
                         (draft_start, draft_start + draft.size, positions[0], positions[-1]))
    is_letter = letters != 0
    before = offset + np.cumsum(is_letter) - is_letter               # letters in front of every key
    first = np.ones(positions.size, dtype=bool)                      # the first key of every position
    first[1:] = positions[1:] != positions[:-1]
    if filled:                                                       # and the draft's letters: every position in front of the
        before = before + positions - (np.cumsum(first) - 1)         # key's own that has no key (from position 0 on)
    at0, deeper = indices == 0, indices > 0
    d = draft[positions - draft_start]
    sub = at0 & is_letter & (letters != d)
    dele = at0 & ~is_letter
    ins = deeper & is_letter
    keep = sub | dele | ins
    kind = np.where(sub, SUB, np.where(dele, DEL, INS))
    parts = [(positions[keep], before[keep], indices[keep], kind[keep], np.where(ins, 0, d)[keep], np.where(dele, 0, letters)[keep],
              phred[keep])]
    # a position whose keys start above index 0 has an empty slot (p, 0)
    hole = first & deeper
    zeros = np.zeros(int(hole.sum()), np.int64)
    parts.append((positions[hole], before[hole], zeros, zeros + DEL, d[hole], zeros, zeros))
    # runs of positions without a key, between two positions that have one
    heads = np.flatnonzero(first)
    run = np.flatnonzero(positions[heads][1:] - positions[heads][:-1] > 1)
    zeros = np.zeros(run.size, np.int64)
    open_at, close_at, lead = positions[heads][run] + 1, positions[heads][run + 1] - 1, before[heads][run + 1]
    if filled:                                                        # the run's own letters lie behind its offset
        lead = lead - (close_at - open_at + 1)
    parts.append((open_at, lead, zeros, zeros + GAP_OPEN, draft[open_at - draft_start], zeros, zeros))
    parts.append((close_at, lead, zeros, zeros + GAP_CLOSE, draft[close_at - draft_start], zeros, zeros))
    columns = [np.concatenate([p[k] for p in parts]) for k in range(7)]
    order = np.lexsort((columns[3], columns[2], columns[0]))       # position, index, then GAP_OPEN before GAP_CLOSE
    if int(columns[2].max(initial=0)) > 0xFFFF or int(columns[0].max(initial=0)) > 0xFFFFFFFF:
        raise ValueError("a record's position or insert index does not fit its field")
    out = np.zeros(order.size, EDIT_DTYPE)
    for name, column in zip(("position", "offset", "index", "kind", "draft", "letter", "phred"), columns):
        out[name] = column[order]
    out["piece"] = piece
    return out


def place(records, piece, offset):
    """Records made with piece 0 / offset 0 (a worker does not know its piece's place) moved to where the piece lies."""
    if piece > MAX_PIECES:
        raise ValueError("a record names %d pieces at most" % MAX_PIECES)
    records = records.copy()
    records["piece"] = piece
    records["offset"] += np.uint32(offset)
    return records


def _record_hunks(records, has_qualities, filled=False):
    """The hunks the records of ONE piece give, as columns: (draft_start, draft_end, polished_start, polished_end, kind, draft
    text, polished text, min_phred), lists of equal length in record order.  filled: a GAP pair is a `filled` hunk whose polished
    interval is as long as its draft interval."""
    if records.size == 0:
        return tuple([] for _ in range(8))
    kind = records["kind"]
    opens, closes = np.flatnonzero(kind == GAP_OPEN), np.flatnonzero(kind == GAP_CLOSE)
    if opens.size != closes.size or np.any(closes != opens + 1):
        raise ValueError("a GAP_OPEN record without its GAP_CLOSE behind it")
    close_at = np.zeros(records.size, np.int64)
    close_at[opens] = records["position"][closes]
    unit = kind != GAP_CLOSE                                         # one unit per edit record and per GAP pair
    kind, close_at = kind[unit].astype(np.int64), close_at[unit]
    p, o = records["position"][unit].astype(np.int64), records["offset"][unit].astype(np.int64)
    gap = kind == GAP_OPEN
    d0 = p + (kind == INS)
    d1 = np.where(gap, close_at + 1, p + 1)
    o1 = o + ((kind == SUB) | (kind == INS))
    if filled:
        o1 = np.where(gap, o + d1 - d0, o1)
    join = np.zeros(p.size, dtype=bool)
    join[1:] = ~gap[1:] & ~gap[:-1] & (d0[1:] == d1[:-1]) & (o[1:] == o1[:-1])
    starts = np.flatnonzero(~join)
    ends = np.append(starts[1:], p.size) - 1
    h_d0, h_d1, h_o0, h_o1, h_gap = d0[starts], d1[ends], o[starts], o1[ends], gap[starts]
    dn, on = h_d1 - h_d0, h_o1 - h_o0
    names = np.array(HUNK_KINDS)[np.where(h_gap, 6 if filled else 4, np.where(dn == on, 0, np.where(dn == 0, 1, np.where(on == 0, 2, 3))))]
    # the letters: every SUB and DEL brings one draft letter, every SUB and INS one polished letter, so a hunk's texts are dn and
    # on letters of the two streams
    units = records[unit]
    draft_text = units["draft"][(kind == SUB) | (kind == DEL)].tobytes().decode()
    polished_text = units["letter"][(kind == SUB) | (kind == INS)].tobytes().decode()
    dn, on = np.where(h_gap, 0, dn), np.where(h_gap, 0, on)          # a run brings no letters of either stream
    da = np.cumsum(dn) - dn
    oa = np.cumsum(on) - on
    low = np.minimum.reduceat(units["phred"], starts)
    texts_d = [draft_text[a:a + n] or "." for a, n in zip(da.tolist(), dn.tolist())]
    texts_o = [polished_text[a:a + n] or "." for a, n in zip(oa.tolist(), on.tolist())]
    phreds = [str(q) if has_qualities and not g else "." for q, g in zip(low.tolist(), h_gap.tolist())]
    return (h_d0.tolist(), h_d1.tolist(), h_o0.tolist(), h_o1.tolist(), names.tolist(), texts_d, texts_o, phreds)


def _hunk_blocks(records, pieces, draft_length, has_qualities):
    """hunks(), one list per piece (a contig's hunks are never all in memory as tuples when they are only written)."""
    records = np.asarray(records, dtype=EDIT_DTYPE)
    piece_of = records["piece"].astype(np.int64)
    if records.size and (np.any(np.diff(piece_of) < 0) or int(piece_of[-1]) >= len(pieces)):
        raise ValueError("the records are not in the order of their pieces")
    by_piece = np.searchsorted(piece_of, np.arange(len(pieces) + 1))
    start = 0                                                        # letters in front of the piece
    for k, (first, last, length) in enumerate(pieces):
        out = []
        if k == 0:
            if first > 0:
                out.append((0, first, 0, 0, "uncovered", ".", ".", "."))
        else:
            before = pieces[k - 1][1]
            if first > before + 1:
                out.append((before + 1, first, start, start, "uncovered", ".", ".", "."))
            elif first < before + 1:
                out.append((first, before + 1, start, start, "duplicated", ".", ".", "."))
        out.extend(zip(*_record_hunks(records[by_piece[k]:by_piece[k + 1]], has_qualities)))
        start += length
        yield out
    if pieces:
        if pieces[-1][1] + 1 < draft_length:
            yield [(pieces[-1][1] + 1, draft_length, start, start, "uncovered", ".", ".", ".")]
    elif draft_length > 0:
        yield [(0, draft_length, 0, 0, "uncovered", ".", ".", ".")]


def _filled_blocks(records, pieces, draft_length, has_qualities):
    """filled_hunks(), as _hunk_blocks gives hunks(): the leading run, the piece's hunks, the trailing run."""
    records = np.asarray(records, dtype=EDIT_DTYPE)
    if len(pieces) > 1 or (not pieces and records.size) or (records.size and records["piece"].any()):
        raise ValueError("a filled consensus has one piece")
    if not pieces:
        if draft_length > 0:
            yield [(0, draft_length, 0, draft_length, "filled", ".", ".", ".")]
        return
    first, last, length = pieces[0]
    if last >= draft_length:
        raise ValueError("the piece ends at position %d, the draft has %d letters" % (last, draft_length))
    if first > 0:
        yield [(0, first, 0, first, "filled", ".", ".", ".")]
    yield list(zip(*_record_hunks(records, has_qualities, filled=True)))
    if last + 1 < draft_length:
        yield [(last + 1, draft_length, length - (draft_length - last - 1), length, "filled", ".", ".", ".")]


def filled_hunks(records, pieces, draft_length, has_qualities):
    """hunks() for the records of a FILLED consensus (pieces: its one piece, or none for a contig without a prediction): a
    GAP_OPEN / GAP_CLOSE pair is one `filled` hunk whose polished interval holds the draft's letters, and from the piece bounds
    come `filled` hunks for [0, first) and (last, draft_length)."""
    return [hunk for block in _filled_blocks(records, pieces, draft_length, has_qualities) for hunk in block]


def hunks(records, pieces, draft_length, has_qualities):
    """-> [(draft_start, draft_end, polished_start, polished_end, kind, draft, polished, min_phred)] in the consensus' order;
    0-based half-open coordinates, '.' for an empty column.  pieces: [(first, last, length)] in the order of the consensus.

    A record of kinds 1-3 occupies a draft and a polished interval -- SUB [p, p+1) [o, o+1); DEL [p, p+1) [o, o); INS
    [p+1, p+1) [o, o+1) -- and joins its predecessor in the piece when both intervals start where the predecessor's end.  The
    run's kind follows from its lengths: equal and positive `sub`, draft empty `ins`, polished empty `del`, else `complex`.
    A GAP_OPEN / GAP_CLOSE pair is one `uncovered` hunk.  From the piece bounds come `uncovered` hunks for [0, first_0), between
    two pieces and (last_n, draft_length), and a `duplicated` hunk for [first_k+1, last_k + 1) where consecutive pieces overlap
    (its polished interval is empty, at the first letter of piece k + 1)."""
    return [hunk for block in _hunk_blocks(records, pieces, draft_length, has_qualities) for hunk in block]


def summary(hunk_list, total=None, filled=False):
    """Bases per hunk kind: draft bases for sub / del / uncovered / duplicated / filled, polished bases for ins, both for complex
    (total: a summary to add to; filled: a new summary has a `filled` count, behind the others)."""
    if total is None:
        total = dict.fromkeys(SUMMARY_KEYS + (("filled",) if filled else ()), 0)
    for d0, d1, o0, o1, kind, _, _, _ in hunk_list:
        if kind == "complex":
            total["complex_draft"] += d1 - d0
            total["complex_polished"] += o1 - o0
        elif kind == "ins":
            total["ins"] += o1 - o0
        else:
            total[kind] += d1 - d0
    return total


def write_edits(file, contig, hunk_list, draft_length, polished_length, blocks=False, filled=False, withheld=None):
    """One line per hunk, then the contig's summary line (blocks: hunk_list is an iterable of lists of hunks; filled: the
    summary line ends with filled=<bases>; withheld: the run has a min_quality gate, and the line ends with withheld=<edits the
    gate kept back>)."""
    total = None
    for block in (hunk_list if blocks else [hunk_list]):
        file.writelines(contig + "\t%d\t%d\t%d\t%d\t%s\t%s\t%s\t%s\n" % hunk for hunk in block)
        total = summary(block, total, filled)
    file.write("##contig=" + contig + "\tdraft_length=" + str(draft_length) + "\tpolished_length=" + str(polished_length) +
               "".join("\t%s=%d" % kv for kv in (total or summary([], None, filled)).items()) +
               ("" if withheld is None else "\twithheld=%d" % withheld) + "\n")


def write_contig(file, contig, records, pieces, draft_length, has_qualities, filled=False, withheld=None):
    """hunks() + write_edits(), piece by piece: what both stitch forms call per contig (pieces: [(first, last, length)]).
    filled: filled_hunks() instead; a contig without a piece is the whole draft.  withheld: write_edits'."""
    if filled:
        write_edits(file, contig, _filled_blocks(records, pieces, draft_length, has_qualities), draft_length,
                    pieces[0][2] if pieces else draft_length, blocks=True, filled=True, withheld=withheld)
        return
    write_edits(file, contig, _hunk_blocks(records, pieces, draft_length, has_qualities), draft_length, sum(p[2] for p in pieces),
                blocks=True, withheld=withheld)


def apply(draft_sequence, records, pieces):
    """The consensus again: the records replayed over the draft, piece by piece.  A position of a piece gives its draft letter
    (upper-cased) unless a DEL or a GAP run takes it or a SUB replaces it; INS letters follow their position by index."""
    records = np.asarray(records, dtype=EDIT_DTYPE)
    draft = upper_bytes(draft_sequence)
    out = []
    for k, (first, last, _length) in enumerate(pieces):
        mine = records[records["piece"] == k]
        position = mine["position"].astype(np.int64)
        letters = draft[first:last + 1].copy()
        keep = np.ones(letters.size, dtype=bool)
        kind = mine["kind"]
        keep[position[kind == DEL] - first] = False
        for a, b in zip(position[kind == GAP_OPEN], position[kind == GAP_CLOSE]):
            keep[a - first:b - first + 1] = False
        letters[position[kind == SUB] - first] = mine["letter"][kind == SUB]
        ins = kind == INS
        key = np.concatenate([(np.arange(first, last + 1, dtype=np.int64) << 16)[keep],
                              (position[ins] << 16) | mine["index"][ins].astype(np.int64)])
        text = np.concatenate([letters[keep], mine["letter"][ins]])
        out.append(text[np.argsort(key, kind="stable")].tobytes().decode())
    return "".join(out)


def apply_filled(draft_sequence, records, pieces):
    """apply() for the records of a FILLED consensus: the whole contig again.  Inside the one piece a position gives its draft
    letter upper-cased unless a DEL takes it or a SUB replaces it; a position of a GAP run, and every position in front of the
    piece and behind it, gives its draft letter as the draft has it."""
    records = np.asarray(records, dtype=EDIT_DTYPE)
    raw = np.frombuffer(draft_sequence.encode() if isinstance(draft_sequence, str) else bytes(draft_sequence), dtype=np.uint8)
    if not pieces:
        return raw.tobytes().decode()
    if len(pieces) > 1 or records["piece"].any():
        raise ValueError("a filled consensus has one piece")
    first, last, _length = pieces[0]
    position = records["position"].astype(np.int64)
    kind = records["kind"]
    letters = upper_bytes(draft_sequence)[first:last + 1].copy()
    keep = np.ones(letters.size, dtype=bool)
    keep[position[kind == DEL] - first] = False
    for a, b in zip(position[kind == GAP_OPEN], position[kind == GAP_CLOSE]):
        letters[a - first:b - first + 1] = raw[a:b + 1]
    letters[position[kind == SUB] - first] = records["letter"][kind == SUB]
    ins = kind == INS
    key = np.concatenate([(np.arange(first, last + 1, dtype=np.int64) << 16)[keep],
                          (position[ins] << 16) | records["index"][ins].astype(np.int64)])
    text = np.concatenate([letters[keep], records["letter"][ins]])
    return (raw[:first].tobytes() + text[np.argsort(key, kind="stable")].tobytes() + raw[last + 1:].tobytes()).decode()
