"""The worlds and the known answers of K23 (the transcript-anchored HGVS bridge), shared by tests/test_hgvs_tx_cpu.py and
tests/test_gpu_hgvs_tx.py: one small assembly, restatement transcripts (reftx_ref.make_tx) over it, and the values the
reference's own tests state (bridge.rs:1046-1304) or that follow from vrs_ref.normalize over the mRNA alone."""
import hgvs_ref as HR
import reftx_ref as R

SEQS = {
    "chrF": b"TTTTACGTACGTGGGGGGGGTTAACCGGAAAA",   # the reference's forward fixture: exons [4,12) [20,28)
    "chrR": b"ACGTTTAAGGCCAACCGGTT",               # its reverse fixture: exons [0,4) [4,8), reverse strand
    "chrJ": b"GGGGACAGCAGCAGCAGGTCAGCAGTACCCC",    # a CAG repeat cut by an intron: exons [4,11) [19,27)
    "chrM": b"GGGGTACTGCTGACCTGCTGCTGCTGTCCCC",    # chrJ reverse-complemented: exons [4,12) [20,27), reverse strand
    "chrE": b"AAAAAAAAAAACGTGTCAAAAAAAAA",         # a homopolymer that runs on past both ends of the transcript
}
MRNA_JUNCTION = b"ACAGCAGCAGCAGTA"
MRNA_ENDS = b"AAACCAAA"
NEIGHBOURS = ["NR_NBR%d.1" % k for k in range(8)]  # mRNA AAAAAAAA each; the store orders them around NR_END.1 by hash


def transcripts():
    d = {name: R.digest_bytes(R.sha512t24u(s)) for name, s in SEQS.items()}
    missing = R.digest_bytes(R.sha512t24u(b"no such chromosome"))
    txs = [
        R.make_tx("NM_FWD.1", d["chrF"], 1, [(4, 12), (20, 28)], (4, 28), gene="GENEA", mane=1),
        R.make_tx("NR_FWD.1", d["chrF"], 1, [(4, 12), (20, 28)]),
        R.make_tx("NM_REV.1", d["chrR"], -1, [(0, 4), (4, 8)], (0, 8)),
        R.make_tx("NR_JUN.1", d["chrJ"], 1, [(4, 11), (19, 27)]),
        R.make_tx("NR_MIR.1", d["chrM"], -1, [(4, 12), (20, 27)]),
        R.make_tx("NR_END.1", d["chrE"], 1, [(8, 12), (16, 20)]),
        R.make_tx("NM_UTR.1", d["chrF"], 1, [(4, 12), (20, 28)], (6, 24)),        # 2 bases of 5' UTR, 4 of 3' UTR
        R.make_tx("NR_EMPTY.1", d["chrF"], 1, [(4, 8), (10, 10), (20, 24)]),      # an empty exon between two real ones
        R.make_tx("NR_PAST.1", d["chrR"], 1, [(10, 30)]),                         # an exon past the chromosome's end
        R.make_tx("NM_NOCHR.1", missing, 1, [(4, 12)], (4, 12)),                  # its chromosome is not in the assembly
        R.make_tx("NM_GENEB.1", d["chrF"], 1, [(4, 12)], (4, 12), gene="GENEB"),  # a gene without MANE Select
    ]
    return txs + [R.make_tx(acc, d["chrE"], 1, [(0, 8)]) for acc in NEIGHBOURS]


# bridge.rs:1046-1304: the non-normalized span and ALT
SPANS = [("NM_FWD.1:c.6C>A", (5, 6, b"A")), ("NM_REV.1:c.3A>G", (2, 3, b"G")), ("NR_FWD.1:n.6C>A", (5, 6, b"A")),
         ("NM_FWD.1:c.5_6del", (4, 6, b"")), ("NM_FWD.1:c.5_6insTT", (5, 5, b"TT")), ("NM_FWD.1:c.8_9insGG", (8, 8, b"GG"))]
# (status, detail)
FAILURES = [("NM_FWD.1:c.1_5insAT", HR.INCONSISTENT_EDIT, 0), ("NM_FWD.1:c.8+1A>G", HR.MAPPING_ERROR, R.NOT_EXONIC),
            ("NM_FWD.1:c.5+1A>G", HR.MAPPING_ERROR, R.INVALID_OFFSET), ("NM_FWD.1:c.6T>A", HR.REF_MISMATCH, 0)]
# the roll across the junction and its mirror: (expression on NR_JUN.1 / NR_MIR.1, normalized start, end, allele)
JUNCTION = [("n.5_7del", 1, 13, b"CAGCAGCAG"), ("n.8_10del", 1, 13, b"CAGCAGCAG"), ("n.11_13del", 1, 13, b"CAGCAGCAG"),
            ("n.5_7dup", 1, 13, b"CAGCAGCAGCAGCAG"), ("n.7_8insCAG", 1, 13, b"CAGCAGCAGCAGCAG")]
ENDS = [("NR_END.1:n.2del", 0, 3, b"AA"), ("NR_END.1:n.7del", 5, 8, b"AA")]
# the remaining statuses
OTHERS = [
    ("chrF:g.6C>A", HR.UNSUPPORTED_REFERENCE_TYPE, 0), ("NM_FWD.1:m.6C>A", HR.UNSUPPORTED_REFERENCE_TYPE, 0),
    ("NM_FWD.1:r.6c>a", HR.UNSUPPORTED_REFERENCE_TYPE, 0), ("NP_1.1:p.Val600Glu", HR.UNSUPPORTED_REFERENCE_TYPE, 0),
    ("NOGENE:g.6C>A", HR.UNSUPPORTED_REFERENCE_TYPE, 0),  # (the reference type is looked at before the MANE index)
    ("NM_NONE.1:c.6C>A", HR.TRANSCRIPT_NOT_FOUND, 0), ("NM_NONE.1:c.5_6inv", HR.UNSUPPORTED_EDIT, 0),  # (inv before the lookup)
    ("GENEA:c.6C>A", HR.OK, 0), ("genea:c.6C>A", HR.OK, 0), ("GENEB:c.6C>A", HR.NO_MANE_TRANSCRIPT, 0), ("NOGENE:c.5_6inv", HR.NO_MANE_TRANSCRIPT, 0),
    ("NM_NOCHR.1:c.3A>T", HR.UNKNOWN_CHROM, 0), ("NR_PAST.1:n.3A>T", HR.OUT_OF_BOUNDS, 0),
    ("NR_EMPTY.1:n.4_5insG", HR.OK, 0), ("NR_EMPTY.1:n.4T>A", HR.OK, 0), ("NR_EMPTY.1:n.5T>A", HR.OK, 0), ("NR_EMPTY.1:n.4+1T>A", HR.MAPPING_ERROR, R.NOT_EXONIC),
    ("NM_UTR.1:c.-2A>T", HR.OK, 0), ("NM_UTR.1:c.-3A>T", HR.MAPPING_ERROR, R.UTR5_OVERFLOW),
    ("NM_UTR.1:c.*4G>T", HR.OK, 0), ("NM_UTR.1:c.*5G>T", HR.MAPPING_ERROR, R.UTR3_OVERFLOW),
    ("NM_FWD.1:c.5_6inv", HR.UNSUPPORTED_EDIT, 0), ("NM_FWD.1:c.=", HR.UNSUPPORTED_EDIT, 0), ("NM_FWD.1:c.(4_6)_9del", HR.UNSUPPORTED_EDIT, 0),
    ("NM_FWD.1:c.(4_5)_6insA", HR.UNSUPPORTED_EDIT, 0),
    ("NM_FWD.1:c.(6C>A)", HR.OK, 0), ("not an expression", HR.PARSE_ERROR, 0), ("NM_FWD.1:c.6C>", HR.PARSE_ERROR, 0),
    ("NM_REV.1:c.3A>R", HR.OK, 0), ("NM_REV.1:c.3T>G", HR.REF_MISMATCH, 0), ("NM_REV.1:c.2_4delTAA", HR.OK, 0), ("NM_REV.1:c.3a>G", HR.REF_MISMATCH, 0),
    ("NM_FWD.1:c.5_6dup", HR.OK, 0), ("NM_FWD.1:c.5_6dupAC", HR.OK, 0), ("NM_FWD.1:c.7_10=", HR.OK, 0), ("NM_FWD.1:c.8_9delinsacgtnRYK", HR.OK, 0),
    ("NM_FWD.1:c.16G>T", HR.OK, 0), ("NM_FWD.1:c.17G>T", HR.MAPPING_ERROR, R.OUTSIDE_CDS), ("NM_FWD.1:c.16_17insA", HR.MAPPING_ERROR, R.OUTSIDE_CDS),
    ("NM_FWD.1:c.16insA", HR.OK, 0), ("NR_FWD.1:n.9-1G>A", HR.MAPPING_ERROR, R.NOT_EXONIC), ("NR_FWD.1:n.8+9T>G", HR.OK, 0),
]
NEIGHBOUR_ROWS = [acc + ":n.%d%s" % (p, e) for acc in NEIGHBOURS for p, e in ((1, "del"), (8, "del"), (4, "dup"))]


def everything():
    """every expression of this file, the junction cases on both strands"""
    out = [s for s, _ in SPANS] + [s for s, _, _ in FAILURES] + [s for s, _, _ in OTHERS] + [s for s, _, _, _ in ENDS] + NEIGHBOUR_ROWS
    for acc in ("NR_JUN.1", "NR_MIR.1"):
        out += [acc + ":" + e for e, _, _, _ in JUNCTION]
    return out
