"""What polish changed, as a normalised VCF (opt-in: polish(..., vcf=True, fill=True) / PEPPER_AMD_POLISH_VCF=1; not in the
reference).  <prefix>_pepper_polished.vcf.gz and its .tbi: one record per hunk of the FILLED
consensus, trimmed and left-aligned against the draft, so that two edit sets of one draft can be compared line by line and a
subset can be applied with any tool that reads VCF.

THE RULE.  Input: the edit records of a filled contig (Edits.EDIT_DTYPE), the draft upper-cased, the filled consensus.  The
units are the hunks of Edits._record_hunks of kinds sub / ins / del / complex, with its joining rule (a record joins its
predecessor when its draft and polished intervals start where the predecessor's end); GAP pairs (`filled` runs) give nothing.
Hunk i has a draft interval [a0, b0), the polished letters ALT0 = consensus[o0, o1) and q = the minimum phred of its records.
Two hunks always have an unchanged draft letter between them.

  1. Trim.  While both alleles are non-empty and end in the same letter, drop it from both; then the same for the first letter:
     (a, b, alt).  Both empty: a no-op, no record, counted.  Both non-empty: POS = a + 1, REF = draft[a:b], ALT = alt.
  2. A pure indel (exactly one allele empty) is left-aligned: while a - 2 >= bound, and draft[a-1] == draft[b-1] (deletion) or
     draft[a-1] == alt[-1] (insertion): an insertion rotates, alt = draft[a-1] + alt[:-1]; a and b move one to the left.  Then
     POS = a (the anchor, 1-based), REF = draft[a-1:b], ALT = draft[a-1] + alt.  bound = the UNTRIMMED b0 of the hunk in front
     (0 for the first): the anchor never lies inside the record in front, and no hunk depends on another one's result.
  3. The contig's start.  link_0: hunk 0 is a pure indel with trimmed a == 0; link_j: hunk j is a pure indel with trimmed
     a_j == b_(j-1) + 1 (trimmed b).  F = the first j whose link is false.  The hunks i < F have no letter to their left that
     is theirs, and are anchored on the right, unshifted: POS = a + 1, REF = draft[a:b+1], ALT = alt + draft[b].  Hunk F > 0
     takes bound = b_(F-1) + 1.  A right-anchored hunk with b == the draft's length has no letter on either side: no record,
     counted as `unanchored` (a deletion of the whole contig; or the last of a chain of indels one letter apart that runs
     from the first letter to the last -- replaying the records then leaves that one hunk out).
  4. QUAL = q, or '.' for a contig added without qualities.

A RECORD (VARIANT_DTYPE, 32 bytes, `pa_stitch_variant` of include/pepper_amd_encoder.h) carries no letters:
    REF = draft[position : position + ref_len)
    ALT = draft[position : position + lead) + consensus[offset : offset + alt_len - lead - tail) + (tail: draft[position + ref_len - 1])
For an insertion of n letters moved k places lead = 1 + min(k, n); a deletion has lead 1, a right-anchored record lead 0 and tail 1,
everything else lead 0 and tail 0.  `shift` = k.  records_numpy() is the host form; the device makes the same bytes
(pa_stitcher_variants).  lines() makes the text of either, replay() applies such text to the draft again.
"""
import numpy as np

from pepper_amd.polish import Edits

KIND_SUB, KIND_INS, KIND_DEL, KIND_COMPLEX = 1, 2, 3, 4
VARIANT_DTYPE = np.dtype([("position", "<u4"), ("ref_len", "<u4"), ("alt_len", "<u4"), ("lead", "<u4"), ("offset", "<u4"),
                          ("shift", "<u4"), ("phred", "u1"), ("kind", "u1"), ("tail", "u1"), ("pad", "u1"), ("reserved", "<u4")])
assert VARIANT_DTYPE.itemsize == 32
COUNT_KEYS = ("records", "noops", "unanchored", "shifted", "letters_shifted")
SAMPLE_NAME = "SAMPLE"
_SHORT = 48                      # alleles up to this many letters are composed as fixed-width columns


def vcf_path(output_prefix):
    return output_prefix + '_pepper_polished.vcf.gz'


def check_vcf(vcf, fill):
    """What every stitch form asks of its vcf argument: the records describe the FILLED consensus of the draft that fills."""
    if vcf is None:
        return
    if fill is None:
        raise ValueError("vcf needs fill: the records describe one complete consensus per contig")
    if str(vcf) != str(fill):
        raise ValueError("with vcf the draft is the one that fills: %s is not %s" % (vcf, fill))


def _bytes(text):
    return np.frombuffer(text.encode() if isinstance(text, str) else bytes(text), dtype=np.uint8)


def hunk_table(records):
    """The hunks of kinds sub / ins / del / complex the records of ONE filled piece give, as int64 columns (a0, b0, o0, o1, q):
    Edits._record_hunks' units and joining rule, without the texts."""
    records = np.asarray(records, dtype=Edits.EDIT_DTYPE)
    kind = records["kind"]
    edit = (kind >= Edits.SUB) & (kind <= Edits.INS)
    if not edit.any():
        return tuple(np.zeros(0, np.int64) for _ in range(5))
    p, o = records["position"].astype(np.int64), records["offset"].astype(np.int64)
    d0, d1 = p + (kind == Edits.INS), p + 1
    o1 = o + ((kind == Edits.SUB) | (kind == Edits.INS))
    head = edit.copy()
    head[1:] &= ~(edit[:-1] & (d0[1:] == d1[:-1]) & (o[1:] == o1[:-1]))
    last = edit.copy()
    last[:-1] &= ~(edit[1:] & ~head[1:])
    first_at, last_at = np.flatnonzero(head), np.flatnonzero(last)
    at = np.flatnonzero(edit)
    q = np.minimum.reduceat(records["phred"][at], np.flatnonzero(head[at])).astype(np.int64)
    return d0[first_at], d1[last_at], o[first_at], o1[last_at], q


def records_numpy(edit_records, draft, consensus, has_qualities=True):
    """The twin of pa_stitcher_variants: (records as VARIANT_DTYPE, counts as [records, no-ops, unanchored, shifted, letters
    shifted]).  edit_records: the records of the filled consensus; draft: the whole contig (any case); consensus: the filled one."""
    D, C = Edits.upper_bytes(draft), _bytes(consensus)
    a0, b0, o0, o1, q = hunk_table(edit_records)
    n = a0.size
    if n == 0:
        return np.zeros(0, VARIANT_DTYPE), [0, 0, 0, 0, 0]
    a, b, s, t = a0.copy(), b0.copy(), o0.copy(), o1.copy()
    act = np.arange(n)
    while act.size:                                                  # 1. trim: the last letters, then the first
        act = act[(b[act] > a[act]) & (t[act] > s[act])]
        act = act[D[b[act] - 1] == C[t[act] - 1]]
        b[act] -= 1
        t[act] -= 1
    act = np.arange(n)
    while act.size:
        act = act[(b[act] > a[act]) & (t[act] > s[act])]
        act = act[D[a[act]] == C[s[act]]]
        a[act] += 1
        s[act] += 1
    rn, an = b - a, t - s
    noop = (rn == 0) & (an == 0)
    pure = (rn == 0) != (an == 0)
    link = pure & (a == np.concatenate([[-1], b[:-1]]) + 1)          # 3. the contig's start
    F = int(np.argmin(link)) if not link.all() else n
    right = np.arange(n) < F
    bound = np.concatenate([[0], b0[:-1]])
    if 0 < F < n:
        bound[F] = b[F - 1] + 1
    k = np.zeros(n, np.int64)                                        # 2. left-align the pure indels
    length, is_del = np.where(rn > 0, rn, an), rn > 0
    act = np.flatnonzero(pure & ~right)
    while act.size:
        x = a[act] - k[act] - 1
        act, x = act[x >= bound[act] + 1], x[x >= bound[act] + 1]
        y = x + length[act]
        from_alt = ~is_del[act] & (y >= a[act])
        vy = np.where(from_alt, C[np.clip(s[act] + y - a[act], 0, max(C.size - 1, 0))] if C.size else 0,
                      D[np.clip(y, 0, D.size - 1)])
        act = act[D[x] == vy]
        k[act] += 1
    left = pure & ~right
    unanchored = right & (b == D.size)
    out = np.zeros(n, VARIANT_DTYPE)
    out["position"] = np.where(left, a - k - 1, a)
    out["ref_len"] = rn + pure
    out["alt_len"] = an + pure
    out["lead"] = np.where(left, np.where(is_del, 1, 1 + np.minimum(k, an)), 0)
    out["offset"] = s
    out["shift"] = k
    out["phred"] = q if has_qualities else 0
    out["kind"] = np.where(pure, np.where(is_del, KIND_DEL, KIND_INS), np.where(rn == an, KIND_SUB, KIND_COMPLEX))
    out["tail"] = right
    keep = ~noop & ~unanchored
    out = out[keep]
    return out, [int(keep.sum()), int(noop.sum()), int(unanchored.sum()), int((k > 0).sum()), int(k.sum())]


def alleles(records, draft, consensus):
    """[(POS 1-based, REF, ALT)] of the records, letters upper-cased: the definition, record by record (the tests and replay use it;
    lines() composes the same text in columns)."""
    D, C = Edits.upper_bytes(draft).tobytes().decode(), bytes(_bytes(consensus)).translate(Edits._UPPER).decode()
    out = []
    for p, rl, al, lead, o, _k, _q, _kind, tail, _, _ in np.asarray(records, dtype=VARIANT_DTYPE).tolist():
        out.append((p + 1, D[p:p + rl], D[p:p + lead] + C[o:o + al - lead - tail] + (D[p + rl - 1] if tail else "")))
    return out


def header(contigs):
    """The VCF header: contigs = [(name, length)] of the draft FASTA, in its order."""
    text = "##fileformat=VCFv4.2\n##source=pepper_amd polish\n##FILTER=<ID=PASS,Description=\"All filters passed\">\n"
    text += "".join("##contig=<ID=%s,length=%d>\n" % (name, length) for name, length in contigs)
    text += "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
    text += "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype Quality\">\n"
    return text + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + SAMPLE_NAME + "\n"


def _columns(D, C, position, ref_len, alt_len, lead, offset, tail):
    """REF and ALT of records whose alleles have at most _SHORT letters, as two 'S' arrays."""
    j = np.arange(_SHORT, dtype=np.int64)[None, :]
    p, rl, al, ld, o, tl = (v[:, None] for v in (position, ref_len, alt_len, lead, offset, tail))
    ref = np.where(j < rl, D[np.minimum(p + j, D.size - 1)], 0).astype(np.uint8)
    if C.size:
        middle = C[np.clip(o + j - ld, 0, C.size - 1)]
    else:
        middle = np.zeros((position.size, _SHORT), np.uint8)
    alt = np.where(j < ld, D[np.minimum(p + j, D.size - 1)],
                   np.where(j < al - tl, middle, np.where(j < al, D[np.minimum(p + rl - 1, D.size - 1)], 0))).astype(np.uint8)
    kind = 'S%d' % _SHORT
    return np.ascontiguousarray(ref).view(kind).ravel(), np.ascontiguousarray(alt).view(kind).ravel()


def lines(contig, records, draft, consensus, has_qualities=True):
    """The records' text: (start 0-based, len(REF), [line as bytes]) in record order, every line
    `contig POS . REF ALT QUAL PASS . GT:GQ 1:QUAL` (without qualities: `... . PASS . GT 1`).  Composed in columns; only records
    with an allele above 48 letters are written one by one."""
    records = np.asarray(records, dtype=VARIANT_DTYPE)
    position, ref_len = records["position"].astype(np.int64), records["ref_len"].astype(np.int64)
    if records.size == 0:
        return position, ref_len, []
    D = Edits.upper_bytes(draft)
    C = np.frombuffer(bytes(_bytes(consensus)).translate(Edits._UPPER), dtype=np.uint8)
    alt_len = records["alt_len"].astype(np.int64)
    ref, alt = _columns(D, C, position, ref_len, alt_len, records["lead"].astype(np.int64), records["offset"].astype(np.int64),
                        records["tail"].astype(np.int64))
    add = np.char.add
    text = add(add((contig + "\t").encode(), (position + 1).astype('S')), b"\t.\t")
    text = add(add(add(text, ref), b"\t"), alt)
    if has_qualities:
        q = records["phred"].astype(np.int64).astype('S')
        text = add(add(add(add(text, b"\t"), q), b"\tPASS\t.\tGT:GQ\t1:"), add(q, b"\n"))
    else:
        text = add(text, b"\t.\tPASS\t.\tGT\t1\n")
    out = text.tolist()
    long_ones = np.flatnonzero((ref_len > _SHORT) | (alt_len > _SHORT))
    if long_ones.size:
        for i, (pos, r, a) in zip(long_ones.tolist(), alleles(records[long_ones], draft, consensus)):
            q = str(int(records["phred"][i]))
            tail = "\t%s\tPASS\t.\tGT:GQ\t1:%s\n" % (q, q) if has_qualities else "\t.\tPASS\t.\tGT\t1\n"
            out[i] = ("%s\t%d\t.\t%s\t%s" % (contig, pos, r, a) + tail).encode()
    return position, ref_len, out


class VcfOutput(object):
    """<prefix>_pepper_polished.vcf.gz and .tbi of a stitch: VcfWriter._VcfFile (BGZF plus tabix) with this module's header;
    contigs come in the order the FASTA is written in."""

    def __init__(self, files, output_prefix, lengths):
        from pepper_amd.variant.VcfWriter import _VcfFile
        self.path = vcf_path(output_prefix)
        self._file = _VcfFile(self.path, header(list(lengths.items())))
        files.callback(self._file.close)
        self.totals = dict.fromkeys(COUNT_KEYS, 0)

    def contig(self, contig, records, counts, draft, consensus, has_qualities):
        for key, v in zip(COUNT_KEYS, counts):
            self.totals[key] += int(v)
        if counts[2]:
            import sys
            sys.stderr.write("WARNING: " + contig + ": %d HUNK WITHOUT A LETTER TO ANCHOR IT ON IS NOT IN THE VCF.\n" % counts[2])
        start, ref_len, text = lines(contig, records, draft, consensus, has_qualities)
        if text:
            self._file.write_columns([contig], np.zeros(len(text), np.int64), start, ref_len,
                                     np.fromiter((len(line) for line in text), np.int64, len(text)), text)


def parse(text):
    """{contig: [(POS, REF, ALT)]} of a VCF's text, in file order (for replay)."""
    out = {}
    for line in (text.decode() if isinstance(text, bytes) else text).splitlines():
        if line and not line.startswith("#"):
            fields = line.split("\t")
            out.setdefault(fields[0], []).append((int(fields[1]), fields[3], fields[4]))
    return out


def replay(draft_sequence, calls):
    """The inverse, for tests: the calls [(POS 1-based, REF, ALT)] applied to the draft upper-cased.  ValueError where a REF is
    not what the draft holds there, or where two calls overlap or are out of order."""
    draft = Edits.upper_bytes(draft_sequence).tobytes().decode()
    out, at = [], 0
    for pos, ref, alt in calls:
        start = pos - 1
        if start < at:
            raise ValueError("the call at %d begins inside the one in front of it" % pos)
        if draft[start:start + len(ref)] != ref.upper():
            raise ValueError("REF %s at %d is not the draft's %s" % (ref, pos, draft[start:start + len(ref)]))
        out.append(draft[at:start])
        out.append(alt.upper())
        at = start + len(ref)
    out.append(draft[at:])
    return "".join(out)
