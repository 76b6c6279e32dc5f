"""Position-keyed merge of the predicted labels into one sequence per contig.

replaces: /root/reference/pepper/modules/python/Stitch.py
    small_chunk_stitch        :36-94    {(position, insert index): label}, later chunks overwrite
    create_consensus_sequence :97-128   pieces ordered by their first position and concatenated
Vectorised with numpy: per piece the (position, index, label) triples of all its 1000-row chunks
are concatenated in the reference's iteration order (chunk ids sorted as strings), filtered
(position/index >= 0; for regions not starting at 0 positions <= start + 2 * MIN_IMAGE_OVERLAP are
overlap and dropped), then the last write of every key wins and keys come out sorted.
qualities=True (opt-in, not in the reference): the phred_score of the row that supplied a letter's label travels with it and
comes out as Sanger text, chr(33 + min(phred, 93)); a winning gap gives neither a letter nor a quality.
edits=<draft FASTA> (opt-in, not in the reference): every piece also gives the records of what it changed against the draft
(pepper_amd/polish/Edits.py); a worker reads the span of the draft its piece covers from the file itself.
fill=<draft FASTA> (opt-in, not in the reference): the contig is merged as ONE piece whatever `threads` is, and every position of
the draft that has no key gives the draft's own letter (in the case the file stores it, quality '!'): the consensus is complete
and does not depend on the thread count.  Edits taken with it are those of the filled consensus (Edits.py, FILL).
Pinned: tests/golden/polish_stitch_ref.fa is the reference's own output on the same prediction arrays.
"""
import concurrent.futures
import os

import numpy as np

from pepper_amd import h5
from pepper_amd.polish.Options import ImageSizeOptions

label_decoder = {1: 'A', 2: 'C', 3: 'G', 4: 'T', 0: ''}
_DECODE = np.frombuffer(b"\0ACGT", dtype=np.uint8)
MIN_SEQUENCE_REQUIRED_FOR_MULTITHREADING = 2
MAX_QUALITY = 93                          # Sanger: '!' + 93 = '~' (the model writes 100 for "certain", a file may hold 255)


def chunks(file_names, threads):
    return [file_names[i:i + threads] for i in range(0, len(file_names), threads)]


def small_chunk_stitch(contig, small_chunk_keys, qualities=False, edits=None, fill=None, min_quality=None, draft=None):
    """One piece of the consensus.  The merge runs inside the I/O library (pa_h5_stitch_polish_regions: chunk rows straight
    from the mapped prediction files, each chunk merged into the tail of the piece; 3 k -> see DESIGN.md chunks/s);
    PEPPER_AMD_STITCH_NUMPY=1 keeps the numpy form below, which tests hold it to.  qualities: (first, last, sequence, quality),
    always through the numpy form (the library's merge carries no phred).  edits: the draft FASTA's path; the piece's edit
    records (piece 0, offsets from the piece's first letter) follow as one more element, through the numpy form as well.
    fill: the draft FASTA's path; the keys are the whole contig's and the piece comes out filled (numpy form).
    min_quality / draft: the gate (gate_numpy) over the piece's winners, against the draft FASTA `draft`; the withheld records
    follow as the last element (numpy form)."""
    if qualities or edits is not None or fill is not None or min_quality:
        return small_chunk_stitch_numpy(contig, small_chunk_keys, qualities=qualities, edits=edits, fill=fill, min_quality=min_quality,
                                        draft=draft)
    if os.environ.get("PEPPER_AMD_STITCH_NUMPY") == "1":
        return small_chunk_stitch_numpy(contig, small_chunk_keys)
    buffer_positions = ImageSizeOptions.MIN_IMAGE_OVERLAP * 2
    open_files, order = {}, []
    try:
        which, paths, starts = [], [], []
        for file_name, contig_name, _st, _end in small_chunk_keys:
            if file_name not in open_files:
                open_files[file_name] = len(order)
                order.append(h5.File(file_name, 'r'))
            which.append(open_files[file_name])
            paths.append('predictions/' + contig + '/' + contig_name + '-' + str(_st) + '-' + str(_end))
            starts.append(_st)
        return h5.stitch_polish_regions(order, which, paths, starts, buffer_positions)
    finally:
        for f in order:
            f.close()


def filled_piece(draft, first, positions, letters, quality):
    """The filled consensus of a contig: draft (uint8, the whole contig as stored), the merged keys' positions and letters (0: no
    letter), quality (the letters' Sanger bytes, or None) -> (sequence, quality or None) as uint8 arrays.  Every position of the
    draft without a key gives draft[p] and '!'."""
    last = int(positions[-1])
    is_letter = letters != 0
    slot = positions - first
    covered = np.zeros(last - first + 1, dtype=bool)
    covered[slot] = True
    holes = np.cumsum(~covered) - ~covered                           # uncovered positions of the piece in front of every position
    per_position = np.bincount(slot, weights=is_letter, minlength=covered.size).astype(np.int64)
    letters_before = np.cumsum(per_position) - per_position
    n_letters, n_holes, tail = int(is_letter.sum()), int((~covered).sum()), draft.size - last - 1
    out = np.empty(first + n_letters + n_holes + tail, dtype=np.uint8)
    out[:first] = draft[:first]
    out[out.size - tail:] = draft[last + 1:]
    at_letter = first + np.flatnonzero(is_letter) - np.cumsum(~is_letter)[is_letter] + holes[slot[is_letter]]
    out[at_letter] = letters[is_letter]
    empty = np.flatnonzero(~covered)
    at_hole = first + letters_before[empty] + holes[empty]
    out[at_hole] = draft[first + empty]
    if quality is None:
        return out, None
    text = np.full(out.size, 33, dtype=np.uint8)
    text[at_letter] = quality
    return out, text


def whole_draft(fill, contig):
    """A contig of the draft as the filled consensus of no prediction: (sequence, quality) -- its letters as stored, all '!'."""
    from pepper_amd.variant.fasta import FASTA_handler
    draft = FASTA_handler(fill)
    try:
        length = draft.get_chromosome_sequence_length(contig)
        if length < 0:
            raise KeyError("CONTIG NOT PRESENT IN THE DRAFT FASTA: " + contig)
        sequence = draft.get_reference_bytes(contig, 0, length, stored_case=True).decode()
    finally:
        draft.close()
    return sequence, "!" * len(sequence)


_CODE = np.zeros(256, dtype=np.int64)
_CODE[np.frombuffer(b"ACGT", dtype=np.uint8)] = (1, 2, 3, 4)


def with_empty_slots(positions, indices, labels, phred):
    """The merge's winners -- sorted by (position, index), one entry per key -- with the slots (p, 0) that have no writer beside
    insert slots put in as label 0, phred 0: the tables the gate works on.  (Such a slot is a DEL; the consensus and the edit
    records are the same with it or without.)"""
    positions, indices = np.asarray(positions, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    labels, phred = np.asarray(labels, dtype=np.int64), np.asarray(phred, dtype=np.int64)
    first = np.ones(positions.size, dtype=bool)
    first[1:] = positions[1:] != positions[:-1]
    hole = np.flatnonzero(first & (indices > 0))
    if hole.size == 0:
        return positions, indices, labels, phred
    return (np.insert(positions, hole, positions[hole]), np.insert(indices, hole, 0), np.insert(labels, hole, 0),
            np.insert(phred, hole, 0))


def gate_numpy(positions, indices, labels, phred, draft, min_quality, draft_start=0, filled=False):
    """min_quality polish, the host twin of pa_stitcher_gate: apply only the edits the model is sure of.  positions / indices /
    labels / phred: the winners of ONE piece's merge with its empty slots (with_empty_slots); draft: the draft's letters from
    draft_start on (any case); min_quality 1..255.  -> (labels, phred, withheld records).

        slot (p, 0), d = upper(draft[p]) in ACGT, the winner is a base other than d (SUB) or a gap / no writer (DEL), and its
        phred < min_quality: WITHHELD -- the slot gets d's label and phred 0
        slot (p, i > 0), the winner is a base (INS), phred < min_quality: WITHHELD -- the slot gets the gap's label and phred 0
        every other slot is untouched: phred >= min_quality, a winner equal to d, a gap in an insert slot, and every slot (p, 0)
        whose draft letter is outside ACGT (there is no letter to keep: the model's decision stands)

    The records (Edits.EDIT_DTYPE, piece 0) are ordered as the keys are: kind SUB / DEL / INS, letter the model's (0 for DEL),
    draft d (0 for INS), phred the winner's, offset the place of the kept draft letter (SUB, DEL) or the letters in front of the
    slot (INS) in the gated piece; filled: in the filled consensus, as Edits.records_numpy(..., filled=True) counts."""
    from pepper_amd.polish import Edits
    positions, indices = np.asarray(positions, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    labels, phred = np.asarray(labels, dtype=np.int64), np.asarray(phred, dtype=np.int64)
    if positions.size == 0:
        return labels, phred, np.zeros(0, Edits.EDIT_DTYPE)
    d = Edits.upper_bytes(draft)[positions - draft_start]
    code = _CODE[d]
    letters = _DECODE[labels]
    is_letter, at0, low = letters != 0, indices == 0, phred < min_quality
    sub = at0 & is_letter & (letters != d) & (code != 0) & low
    dele = at0 & ~is_letter & (code != 0) & low
    ins = ~at0 & is_letter & low
    held = sub | dele | ins
    gated = np.where(sub | dele, code, np.where(ins, 0, labels))
    emits = gated != 0
    before = np.cumsum(emits) - emits                                # gated letters in front of every key
    if filled:
        first = np.ones(positions.size, dtype=bool)
        first[1:] = positions[1:] != positions[:-1]
        before = before + positions - (np.cumsum(first) - 1)
    out = np.zeros(int(held.sum()), Edits.EDIT_DTYPE)
    out["position"], out["offset"], out["index"] = positions[held], before[held], indices[held]
    out["kind"] = np.where(sub, Edits.SUB, np.where(dele, Edits.DEL, Edits.INS))[held]
    out["draft"], out["letter"], out["phred"] = np.where(ins, 0, d)[held], letters[held], phred[held]
    return gated, np.where(held, 0, phred), out


def _contig_of(draft_fasta, contig, last):
    """The whole contig of the draft as the file stores it (uint8); it must reach position `last`."""
    from pepper_amd.variant.fasta import FASTA_handler
    draft = FASTA_handler(draft_fasta)
    try:
        length = draft.get_chromosome_sequence_length(contig)
        if length < 0:
            raise KeyError("CONTIG NOT PRESENT IN THE DRAFT FASTA: " + contig)
        if length <= last:
            raise ValueError("the draft FASTA %s has no letter at position %d of %s" % (draft_fasta, last, contig))
        return np.frombuffer(draft.get_reference_bytes(contig, 0, length, stored_case=True), dtype=np.uint8)
    finally:
        draft.close()


def _gated_piece(contig, positions, indices, labels, phred, want_qualities, edits, fill, min_quality, draft):
    """small_chunk_stitch_numpy's result for a piece whose winners (sorted keys, labels 0..4, raw phred) go through the gate:
    (first, last, sequence[, quality][, edit records], withheld records).  The whole contig of the draft is read once and serves
    the gate, the fill and the edits."""
    from pepper_amd.polish import Edits
    stored = _contig_of(draft, contig, int(positions[-1]))
    filled = fill is not None
    positions, indices, labels, phred = with_empty_slots(positions, indices, labels, np.minimum(phred, 255))
    labels, phred, withheld = gate_numpy(positions, indices, labels, phred, stored, min_quality, filled=filled)
    letters = _DECODE[labels]
    quality = (33 + np.minimum(phred[letters != 0], MAX_QUALITY)).astype(np.uint8)
    if filled:
        text, quality = filled_piece(stored, int(positions[0]), positions, letters, quality)
    else:
        text = letters[letters != 0]
    result = (int(positions[0]), int(positions[-1]), text.tobytes().decode())
    if want_qualities:
        result += (quality.tobytes().decode(),)
    if edits is not None:
        result += (Edits.records_numpy(positions, indices, labels, phred, stored, filled=filled),)
    return result + (withheld,)


def small_chunk_stitch_numpy(contig, small_chunk_keys, qualities=False, edits=None, fill=None, min_quality=None, draft=None):
    if fill is not None and edits is not None and str(edits) != str(fill):
        raise ValueError("with fill the edits are taken against the draft that fills: %s is not %s" % (edits, fill))
    if min_quality:
        if draft is None or any(other is not None and str(other) != str(draft) for other in (edits, fill)):
            raise ValueError("min_quality needs the draft FASTA, the one that fills and the edits are taken against")
    want_qualities = qualities
    qualities = qualities or edits is not None or bool(min_quality)      # the edit records and the gate read the winners' phred
    buffer_positions = ImageSizeOptions.MIN_IMAGE_OVERLAP * 2
    nothing = (-1, -1, '', '') if want_qualities else (-1, -1, '')
    if edits is not None or min_quality:
        from pepper_amd.polish import Edits
    if edits is not None:
        nothing += (np.zeros(0, Edits.EDIT_DTYPE),)
    if min_quality:                       # (the withheld records: one more element, the last)
        nothing += (np.zeros(0, Edits.EDIT_DTYPE),)
    names = ('position', 'index', 'bases', 'phred_score') if qualities else ('position', 'index', 'bases')
    pos_parts, idx_parts, base_parts, phred_parts = [], [], [], []
    open_files = {}                       # each prediction file is opened once per call, not once per region
    try:
        for file_name, contig_name, _st, _end in small_chunk_keys:
            chunk_name = contig_name + '-' + str(_st) + '-' + str(_end)
            prefix = 'predictions/' + contig + '/' + chunk_name
            hdf5_file = open_files.get(file_name)
            if hdf5_file is None:
                hdf5_file = open_files[file_name] = h5.File(file_name, 'r')
            # every chunk of the region in one library call (chunk ids in string order, as sorted() gives them)
            phred = None
            try:
                if qualities:
                    positions, indices, bases, phred = hdf5_file.read_polish_prediction_region(prefix, ImageSizeOptions.SEQ_LENGTH,
                                                                                               qualities=True)
                    phred = phred.reshape(-1).astype(np.int64)
                else:
                    positions, indices, bases = hdf5_file.read_polish_prediction_region(prefix, ImageSizeOptions.SEQ_LENGTH)
                positions, indices, bases = positions.reshape(-1), indices.reshape(-1), bases.reshape(-1).astype(np.int64)
            except h5.H5Error:                  # chunks of another length (not written by this pipeline): one by one
                parts = [[] for _ in names]
                for chunk in sorted(set(hdf5_file.keys(prefix)) - {'contig_start', 'contig_end'}):
                    for k, name in enumerate(names):
                        parts[k].append(np.asarray(hdf5_file[prefix + '/' + chunk + '/' + name], dtype=np.int64).reshape(-1))
                positions, indices, bases = (np.concatenate(p) if p else np.zeros(0, np.int64) for p in parts[:3])
                if qualities:
                    phred = np.concatenate(parts[3]) if parts[3] else np.zeros(0, np.int64)
            keep = (indices >= 0) & (positions >= 0)
            if _st > 0:
                keep &= positions > _st + buffer_positions
            pos_parts.append(positions[keep])
            idx_parts.append(indices[keep])
            base_parts.append(bases[keep])
            if qualities:
                phred_parts.append(phred[keep])
    finally:
        for f in open_files.values():
            f.close()
    if not pos_parts:
        return nothing
    positions = np.concatenate(pos_parts)
    if positions.size == 0:
        return nothing
    indices = np.concatenate(idx_parts)
    bases = np.concatenate(base_parts)
    # stable sort on (position, index): the last element of every run is the last write
    order = np.lexsort((indices, positions))
    positions, indices, bases = positions[order], indices[order], bases[order]
    last = np.ones(positions.size, dtype=bool)
    last[:-1] = (positions[1:] != positions[:-1]) | (indices[1:] != indices[:-1])
    labels = bases[last]
    if labels.size and (labels.min() < 0 or labels.max() > 4):
        raise KeyError(int(labels[(labels < 0) | (labels > 4)][0]))      # label_decoder[...] in the reference
    if min_quality:                       # the gate works on the winners; everything below reads what it leaves
        return _gated_piece(contig, positions[last], indices[last], labels, np.concatenate(phred_parts)[order][last], want_qualities,
                            edits, fill, min_quality, draft)
    letters = _DECODE[labels]
    sequence = letters[letters != 0].tobytes().decode()
    result = (int(positions[0]), int(positions[-1]), sequence)
    if qualities:                         # the phred the winning write carried, for the winners that are bases
        phred = np.concatenate(phred_parts)[order][last]
        if want_qualities:
            result += ((33 + np.minimum(phred[letters != 0], MAX_QUALITY)).astype(np.uint8).tobytes().decode(),)
    if fill is not None:                  # the whole contig of the draft is read, and the records are those of the filled piece
        from pepper_amd.variant.fasta import FASTA_handler
        draft = FASTA_handler(fill)
        try:
            length = draft.get_chromosome_sequence_length(contig)
            if length < 0:
                raise KeyError("CONTIG NOT PRESENT IN THE DRAFT FASTA: " + contig)
            if length <= result[1]:
                raise ValueError("the draft FASTA %s has no letter at position %d of %s" % (fill, result[1], contig))
            stored = np.frombuffer(draft.get_reference_bytes(contig, 0, length, stored_case=True), dtype=np.uint8)
        finally:
            draft.close()
        text, quality = filled_piece(stored, result[0], positions[last], letters,
                                     (33 + np.minimum(phred[letters != 0], MAX_QUALITY)).astype(np.uint8) if want_qualities else None)
        result = result[:2] + (text.tobytes().decode(),) + ((quality.tobytes().decode(),) if want_qualities else ())
        if edits is not None:
            from pepper_amd.polish import Edits
            result += (Edits.records_numpy(positions[last], indices[last], labels, np.minimum(phred, 255), stored, filled=True),)
        return result
    if edits is not None:                 # only the span the piece covers is read from the draft
        from pepper_amd.variant.fasta import FASTA_handler
        draft = FASTA_handler(edits)
        try:
            if draft.get_chromosome_sequence_length(contig) <= result[1]:
                raise ValueError("the draft FASTA %s has no letter at position %d of %s" % (edits, result[1], contig))
            span = draft.get_reference_bytes(contig, result[0], result[1] + 1)
        finally:
            draft.close()
        result += (Edits.records_numpy(positions[last], indices[last], labels, np.minimum(phred, 255), span, result[0]),)
    return result


def _gated_consensus(contig, sequence_chunk_keys, threads, qualities, edits, fill, min_quality, draft):
    """create_consensus_sequence(..., min_quality=, draft=): the same plan -- one piece with fill, else pieces of consecutive regions
    -- every piece through the numpy merge and the gate."""
    from pepper_amd.polish import Edits
    key_list = sorted(((file_name, contig, int(contig_start), int(contig_end))
                       for file_name, _, contig_start, contig_end in sorted(sequence_chunk_keys, key=lambda e: e[1])),
                      key=lambda e: (e[2], e[3]))
    extra = (bool(qualities), edits, fill, min_quality, draft)
    if fill is not None:
        file_chunks = [key_list]
    else:
        file_chunks = chunks(key_list, max(MIN_SEQUENCE_REQUIRED_FOR_MULTITHREADING, int(len(key_list) / max(1, threads)) + 1))
    if threads <= 1 or len(file_chunks) <= 1:
        results = [small_chunk_stitch(contig, chunk, *extra) for chunk in file_chunks]
    else:
        with concurrent.futures.ProcessPoolExecutor(max_workers=threads) as executor:
            results = [f.result() for f in [executor.submit(small_chunk_stitch, contig, chunk, *extra) for chunk in file_chunks]]
    pieces = sorted((r for r in results if r[0] != -1 and r[1] != -1), key=lambda e: (e[0], e[1]))
    empty = np.zeros(0, Edits.EDIT_DTYPE)
    if fill is not None and not pieces:                               # no kept row: the draft as it is
        sequence, quality = whole_draft(fill, contig)
        records, withheld, bounds = empty, empty, []
    else:
        sequence = ''.join(piece[2] for piece in pieces)
        quality = ''.join(piece[3] for piece in pieces) if qualities else None
        records, withheld, at = [empty], [empty], 0
        for k, piece in enumerate(pieces):
            withheld.append(Edits.place(piece[-1], k, at))
            if edits is not None:
                records.append(Edits.place(piece[-2], k, at))
            at += len(piece[2])
        records, withheld = np.concatenate(records), np.concatenate(withheld)
        bounds = [(piece[0], piece[1], len(piece[2])) for piece in pieces]
    if edits is not None:
        return sequence, quality if qualities else None, records, bounds, withheld
    if qualities:
        return sequence, quality, withheld
    return sequence, withheld


def create_consensus_sequence(contig, sequence_chunk_keys, threads, qualities=False, edits=None, fill=None, min_quality=None,
                              draft=None):
    """The consensus of one contig; qualities: (sequence, quality), the pieces' qualities concatenated as their letters are.
    edits (the draft FASTA's path): (sequence, quality or None, records, pieces) -- the contig's edit records and its pieces
    [(first, last, length)], both in the order of the consensus (pepper_amd/polish/Edits.py).
    fill (the draft FASTA's path): the same forms for the FILLED consensus -- every region of the contig in one piece, in the
    order they are iterated here, and the draft's letters where no key is; `threads` does not shape it.
    min_quality (1..255; None or 0: off) with draft (the draft FASTA's path): every piece's winners go through gate_numpy first, and
    the contig's withheld records (piece and offset as the edit records have them) follow the form asked for as one more element
    -- a bare sequence becomes (sequence, withheld)."""
    from pepper_amd import _lib
    min_quality = _lib.min_quality_value(min_quality)
    if min_quality:
        return _gated_consensus(contig, sequence_chunk_keys, threads, qualities, edits, fill, min_quality, draft)
    extra = (bool(qualities), edits) if edits is not None else (True,) if qualities else ()
    key_list = sorted(((file_name, contig, int(contig_start), int(contig_end))
                       for file_name, _, contig_start, contig_end in sorted(sequence_chunk_keys, key=lambda e: e[1])),
                      key=lambda e: (e[2], e[3]))
    if fill is not None:
        piece = small_chunk_stitch(contig, key_list, bool(qualities), edits, fill)
        if piece[0] == -1 or piece[1] == -1:                      # no kept row: the draft as it is
            sequence, quality = whole_draft(fill, contig)
            piece, pieces = (-1, -1, sequence) + ((quality,) if qualities else ()), []
            records = None
        else:
            pieces, records = [(piece[0], piece[1], len(piece[2]))], piece[-1]
        if edits is not None:
            from pepper_amd.polish import Edits
            return (piece[2], piece[3] if qualities else None, records if records is not None else np.zeros(0, Edits.EDIT_DTYPE),
                    pieces)
        return (piece[2], piece[3]) if qualities else piece[2]
    file_chunks = chunks(key_list, max(MIN_SEQUENCE_REQUIRED_FOR_MULTITHREADING, int(len(key_list) / max(1, threads)) + 1))
    if threads <= 1 or len(file_chunks) <= 1:
        results = [small_chunk_stitch(contig, chunk, *extra) for chunk in file_chunks]
    else:
        with concurrent.futures.ProcessPoolExecutor(max_workers=threads) as executor:
            results = [f.result() for f in [executor.submit(small_chunk_stitch, contig, chunk, *extra) for chunk in file_chunks]]
    pieces = sorted((r for r in results if r[0] != -1 and r[1] != -1), key=lambda e: (e[0], e[1]))
    if edits is not None:
        from pepper_amd.polish import Edits
        records, at = [np.zeros(0, Edits.EDIT_DTYPE)], 0
        for k, piece in enumerate(pieces):
            records.append(Edits.place(piece[-1], k, at))
            at += len(piece[2])
        return (''.join(piece[2] for piece in pieces), ''.join(piece[3] for piece in pieces) if qualities else None,
                np.concatenate(records), [(piece[0], piece[1], len(piece[2])) for piece in pieces])
    if qualities:
        return ''.join(piece[2] for piece in pieces), ''.join(piece[3] for piece in pieces)
    return ''.join(sequence for _, _, sequence in pieces)
