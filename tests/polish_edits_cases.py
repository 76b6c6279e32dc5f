"""Inputs and the literal restatement for the polish edits tests (tests/test_polish_edits_cpu.py, tests/test_gpu_polish_edits.py):
small prediction directories and drafts built here, chunks of a few dozen rows, and `dict_records`, the dictionary loop the
numpy twin (pepper_amd/polish/Edits.records_numpy) is held to.  No test lives in this module."""
import os

import numpy as np

from pepper_amd import h5
from pepper_amd.polish import Edits
from pepper_amd.polish.DataStorePredict import DataStore
from pepper_amd.polish.Stitch import create_consensus_sequence
from pepper_amd.polish.perform_stitch import get_file_paths_from_directory, perform_stitch

CODE = {'A': 1, 'C': 2, 'G': 3, 'T': 4}
LETTER = {0: 0, 1: ord('A'), 2: ord('C'), 3: ord('G'), 4: ord('T')}


# ---- the literal restatement ----
def dict_tables(pred_files, contig, threads):
    """Per piece the dictionary {(position, index): (label, phred)} of the reference's merge, pieces sorted by (first, last)."""
    keys = []
    for fn in pred_files:
        with h5.File(fn) as f:
            if contig not in f.keys('predictions'):
                continue
            for ck in sorted(f.keys('predictions/' + contig)):
                keys.append((fn, ck, int(f[f'predictions/{contig}/{ck}/contig_start']), int(f[f'predictions/{contig}/{ck}/contig_end'])))
    keys = sorted(sorted(keys, key=lambda e: e[1]), key=lambda e: (e[2], e[3]))
    size = max(2, int(len(keys) / threads) + 1)
    tables = []
    for i in range(0, len(keys), size):
        table = {}
        for fn, ck, st, en in keys[i:i + size]:
            with h5.File(fn) as f:
                for cid in sorted(set(f.keys(f'predictions/{contig}/{ck}')) - {'contig_start', 'contig_end'}):
                    base = f'predictions/{contig}/{ck}/{cid}/'
                    for pos, idx, b, q in zip(f[base + 'position'].tolist(), f[base + 'index'].tolist(), f[base + 'bases'].tolist(),
                                              f[base + 'phred_score'].tolist()):
                        if (st > 0 and pos <= st + 200) or idx < 0 or pos < 0:
                            continue
                        table[(pos, idx)] = (b, q)
        if table:
            tables.append(table)
    return sorted(tables, key=lambda t: (min(t)[0], max(t)[0]))


def dict_records(tables, draft):
    """-> (consensus, [record tuples in EDIT_DTYPE's field order], [(first, last, length)])."""
    out, pieces, text = [], [], []
    for piece, table in enumerate(tables):
        first, last, width = min(table)[0], max(table)[0], {}
        for p, i in table:
            width[p] = max(width.get(p, 0), i + 1)
        begin = len(text)
        for p in range(first, last + 1):
            d = ord(draft[p].upper())
            if p not in width:
                out += [(p, len(text), 0, piece, kind, d, 0, 0) for kind, q in ((4, p - 1), (5, p + 1)) if q in width]
                continue
            for i in range(width[p]):
                label, q = table.get((p, i), (0, 0))
                letter = LETTER[label]
                if i == 0 and letter == 0:
                    out.append((p, len(text), 0, piece, 2, d, 0, q))
                elif i == 0 and letter != d:
                    out.append((p, len(text), 0, piece, 1, d, letter, q))
                elif i > 0 and letter:
                    out.append((p, len(text), i, piece, 3, 0, letter, q))
                if letter:
                    text.append(chr(letter))
        pieces.append((first, last, len(text) - begin))
    return ''.join(text), out, pieces


def expected(pred, draft, contig, threads):
    return dict_records(dict_tables(get_file_paths_from_directory(str(pred)), contig, threads), draft)


# ---- running the host form ----
def write_draft(path, drafts):
    """{contig: sequence} as a FASTA with 60-letter lines."""
    with open(path, "w") as fh:
        for name, seq in drafts.items():
            fh.write(">" + name + "\n")
            for a in range(0, len(seq), 60):
                fh.write(seq[a:a + 60] + "\n")
    return str(path)


def contig_keys(pred, contig):
    keys = []
    for fn in get_file_paths_from_directory(str(pred)):
        with h5.File(fn, 'r') as f:
            if 'predictions' in f.keys() and contig in f.keys('predictions'):
                keys.extend((fn, name, start, end) for name, start, end in f.list_polish_regions(contig))
    return keys


def host_records(pred, draft_fa, contig, threads):
    """(sequence, records, pieces) of the numpy twin, through create_consensus_sequence."""
    sequence, _, records, pieces = create_consensus_sequence(contig, contig_keys(pred, contig), threads, edits=str(draft_fa))
    return sequence, records, pieces


def host_texts(pred, draft_fa, where, threads):
    """(FASTA, .edits.tsv) perform_stitch writes."""
    out = perform_stitch(str(pred), str(where), threads, edits=str(draft_fa))
    assert out == str(where) + "_pepper_polished.fa"
    return open(out).read(), open(str(where) + "_pepper_polished.edits.tsv").read()


def fasta_sequences(text):
    lines = text.splitlines()
    return dict(zip((name[1:] for name in lines[0::2]), lines[1::2]))


def as_tuples(records):
    return [tuple(int(v) for v in r) for r in np.asarray(records, Edits.EDIT_DTYPE).tolist()]


def check_contig(pred, draft_fa, draft, contig, threads, sequence=None):
    """The twin against the restatement, and the round trip; -> (sequence, records, pieces)."""
    got_sequence, records, pieces = host_records(pred, draft_fa, contig, threads)
    want_sequence, want_records, want_pieces = expected(pred, draft, contig, threads)
    assert got_sequence == want_sequence and pieces == want_pieces
    assert as_tuples(records) == want_records
    assert Edits.apply(draft, records, pieces) == got_sequence
    if sequence is not None:
        assert got_sequence == sequence
    return got_sequence, records, pieces


# ---- building prediction files ----
def random_draft(rng, n):
    return ''.join("ACGT"[k] for k in rng.integers(0, 4, n))


def other(letter, step=1):
    """A base that is not `letter`, as a label."""
    return ("ACGT".index(letter.upper()) + step) % 4 + 1 if letter.upper() in "ACGT" else 1 + step % 4


def rows(draft, a, b, changes=None, phred=40):
    """Rows (position, index, label, phred) that repeat draft[a:b] (a letter outside ACGT: label A), then `changes`:
    {(position, index): (label, phred)} sets or adds a row, {(position, index): None} takes it away."""
    table = {(p, 0): (CODE.get(draft[p].upper(), 1), phred) for p in range(a, b)}
    for key, value in (changes or {}).items():
        if value is None:
            table.pop(key, None)
        else:
            table[key] = value
    keys = sorted(table)
    return (np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64),
            np.array([table[k][0] for k in keys], np.int64), np.array([table[k][1] for k in keys], np.int64))


def write_region(store, contig, start, end, region_rows, chunk=37):
    """The rows as chunks of `chunk` rows (shorter than the pipeline's: read dataset by dataset)."""
    pos, idx, lab, phr = region_rows
    for cid, at in enumerate(range(0, len(pos), chunk)):
        store.write_prediction(contig, start, end, cid, pos[at:at + chunk], idx[at:at + chunk], lab[at:at + chunk], phr[at:at + chunk])


def planted_draft():
    rng = np.random.default_rng(404)
    draft = list(random_draft(rng, 400))
    for p in range(70, 76):
        draft[p] = draft[p].lower()
    draft[80] = draft[81] = draft[82] = 'N'
    draft[83] = 'n'
    return ''.join(draft)


def write_planted(pred, second_from=170):
    """Contig `ctg`, four regions named (0, 100) .. (0, 400): rows 10..99, 100..180, second_from..260 and 280..350 of a 400-base
    draft.  threads = 1: one piece with a 19-position gap at 261..279; threads = 3: two pieces, overlapping in
    [second_from, 181) with second_from = 170, apart with second_from = 190.  The first two regions hold one of everything."""
    draft = planted_draft()
    d = draft
    first = {
        (20, 0): (other(d[20]), 0),                                  # SUB, phred 0
        (30, 0): (0, 100),                                           # DEL, phred 100
        (40, 1): (3, 255),                                           # INS, phred 255
        (50, 0): (other(d[50]), 11), (50, 1): (1, 12), (50, 2): (2, 13), (51, 0): (other(d[51]), 9),   # SUB INS INS SUB: one complex
        (60, 0): (0, 21), (62, 0): (0, 22),                          # two DELs, a match between them
        (72, 0): (other(d[72]), 30),                                 # lower-case draft letters: 70..75 match, 72 does not
        (81, 0): (0, 31), (82, 0): (2, 32),                          # N: always a SUB (80, 82), or a DEL (81); n as well (83)
        (90, 0): None, (90, 1): (4, 33),                             # an empty index-0 slot under a filled index-1 slot
        (95, 1): (0, 34), (96, 2): (1, 35),                          # a gap at index 1: nothing; index 1 empty under index 2
    }
    second = {
        (120, 0): None,                                              # a one-position gap
        (130, 0): (other(d[130]), 50), (131, 0): (other(d[131], 2), 40), (132, 0): (other(d[132]), 60),   # a 3-base sub hunk
        (140, 1): (1, 70), (140, 2): (2, 71), (140, 3): (3, 72),     # a 3-base ins hunk
        (150, 0): (0, 80), (151, 0): (0, 81),                        # a 2-base del hunk
    }
    third = {(175, 0): (other(d[175]), 44), (200, 1): (4, 45)} if second_from <= 175 else {(200, 1): (4, 45)}
    pred.mkdir()
    with DataStore(str(pred / "p.hdf"), "w") as s:
        write_region(s, "ctg", 0, 100, rows(d, 10, 100, first))
        write_region(s, "ctg", 0, 200, rows(d, 100, 181, second))
        write_region(s, "ctg", 0, 300, rows(d, second_from, 261, third))
        write_region(s, "ctg", 0, 400, rows(d, 280, 351, {(300, 0): (0, 5)}))
    return {"ctg": draft}


def golden_draft(golden_dir):
    """{contig: draft} derived from the golden consensus by planted changes: every 97th base replaced, every 211th dropped,
    an extra base after every 389th; then long enough to cover every position the golden rows name."""
    g = np.load(os.path.join(golden_dir, "polish_stitch_inputs.npz"), allow_pickle=False)
    top = {}
    for ri in range(int(g["n_regions"])):
        contig, n_chunks = str(g["r%d_contig" % ri]), int(g["r%d_meta" % ri][3])
        for cid in range(n_chunks):
            top[contig] = max(top.get(contig, 0), int(g["r%d_c%d_position" % (ri, cid)].max()))
    drafts = {}
    for name, seq in fasta_sequences(open(os.path.join(golden_dir, "polish_stitch_ref.fa")).read()).items():
        out = []
        for k, c in enumerate(seq):
            if k % 211 == 5:
                continue
            out.append("ACGT"[("ACGT".index(c) + 1) % 4] if k % 97 == 3 else c)
            if k % 389 == 7:
                out.append("T")
        draft = ''.join(out)
        drafts[name] = draft + "A" * max(0, top.get(name, 0) + 1 - len(draft))
    for name in top:
        drafts.setdefault(name, "A" * (top[name] + 1))
    return drafts
