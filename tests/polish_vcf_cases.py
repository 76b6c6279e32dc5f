"""Inputs and the literal restatement for the polish VCF tests (tests/test_polish_vcf_cpu.py, tests/test_gpu_polish_vcf.py):
random small contigs as prediction rows, and `restated`, the rule of pepper_amd/polish/Variants.py hunk by hunk on Python
strings, which the numpy twin (Variants.records_numpy) and through it the device are held to.  No test lives in this module."""
import numpy as np

from pepper_amd.polish import Edits

CODE = {'A': 1, 'C': 2, 'G': 3, 'T': 4}


def keys_of(draft, changes=None, first=0, last=None, holes=()):
    """The merge's winners for rows that repeat draft[first .. last] (a letter outside ACGT: label A) with `changes`
    {(position, index): label or None (no key)} and without any key at the positions of `holes` -> (positions, indices, labels)
    sorted, as Edits.records_numpy takes them."""
    last = len(draft) - 1 if last is None else last
    table = {(p, 0): CODE.get(draft[p].upper(), 1) for p in range(first, last + 1) if p not in holes}
    for key, label in (changes or {}).items():
        if label is None:
            table.pop(key, None)
        else:
            table[key] = label
    keys = sorted(table)
    return (np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64),
            np.array([table[k] for k in keys], np.int64))


def filled(draft, keys, phred=None):
    """(edit records of the filled consensus, pieces, the filled consensus) of the winners `keys`."""
    positions, indices, labels = keys
    if positions.size == 0:
        return np.zeros(0, Edits.EDIT_DTYPE), [], draft
    phred = np.full(positions.size, 40, np.int64) if phred is None else np.asarray(phred, np.int64)
    records = Edits.records_numpy(positions, indices, labels, phred, draft, filled=True)
    pieces = [(int(positions[0]), int(positions[-1]), 0)]
    return records, pieces, Edits.apply_filled(draft, records, pieces)


def random_case(rng):
    """A draft of 1..24 letters over A, AC or ACGT, and winners with substitutions, deletions and 1-to-3-letter insertions at
    about 10 % each (phred 1..60 per key); now and then a piece that does not span the contig, or a position without a key."""
    alphabet = ("A", "AC", "ACGT")[int(rng.integers(0, 3))]
    n = int(rng.integers(1, 25))
    draft = ''.join(alphabet[int(k)] for k in rng.integers(0, len(alphabet), n))
    first, last, holes = 0, n - 1, ()
    if n > 3 and rng.random() < 0.15:
        first = int(rng.integers(0, 2))
        last = n - 1 - int(rng.integers(0, 2))
        holes = tuple(int(p) for p in rng.integers(first + 1, last, 1)) if last - first > 2 else ()
    changes = {}
    for p in range(first, last + 1):
        if p in holes:
            continue
        r = rng.random()
        if r < 0.1:
            changes[(p, 0)] = CODE[alphabet[int(rng.integers(0, len(alphabet)))]] if len(alphabet) > 1 else 2
        elif r < 0.2:
            changes[(p, 0)] = 0
        if rng.random() < 0.1:
            for i in range(1, int(rng.integers(1, 4)) + 1):
                changes[(p, i)] = CODE[alphabet[int(rng.integers(0, len(alphabet)))]]
    keys = keys_of(draft, changes, first, last, holes)
    return draft, keys, rng.integers(1, 61, keys[0].size)


def restated(records, pieces, draft, consensus, has_qualities=True):
    """The rule on strings, hunk by hunk -> ([(POS, REF, ALT, QUAL or None, shift, bound or None)], counts)."""
    D = draft.upper()
    hunks = [h for h in Edits.filled_hunks(records, pieces, len(draft), True) if h[4] in ("sub", "ins", "del", "complex")]
    trimmed = []
    for d0, d1, o0, o1, _kind, _dt, _pt, _q in hunks:
        a, b, alt = d0, d1, consensus[o0:o1]
        while b > a and alt and D[b - 1] == alt[-1]:
            b, alt = b - 1, alt[:-1]
        while b > a and alt and D[a] == alt[0]:
            a, alt = a + 1, alt[1:]
        trimmed.append((a, b, alt))
    pure = [(b > a) != bool(alt) for a, b, alt in trimmed]
    F = 0
    while F < len(hunks) and pure[F] and trimmed[F][0] == (0 if F == 0 else trimmed[F - 1][1] + 1):
        F += 1
    out, noops, unanchored, shifted, letters = [], 0, 0, 0, 0
    for i, (a, b, alt) in enumerate(trimmed):
        qual = int(hunks[i][7]) if has_qualities else None
        if b == a and not alt:
            noops += 1
        elif b > a and alt:
            out.append((a + 1, D[a:b], alt, qual, 0, None))
        elif i < F:
            if b == len(D):
                unanchored += 1
            else:
                out.append((a + 1, D[a:b + 1], alt + D[b], qual, 0, None))
        else:
            bound = 0 if i == 0 else trimmed[F - 1][1] + 1 if i == F else hunks[i - 1][1]
            assert a - 1 >= bound, "a pure indel behind the contig's start has room for its anchor"
            k = 0
            while a - 2 >= bound and D[a - 1] == (D[b - 1] if b > a else alt[-1]):
                if b == a:
                    alt = D[a - 1] + alt[:-1]
                a, b, k = a - 1, b - 1, k + 1
            out.append((a, D[a - 1:b], D[a - 1] + alt, qual, k, bound))
            shifted += k > 0
            letters += k
    return out, [len(out), noops, unanchored, shifted, letters]
