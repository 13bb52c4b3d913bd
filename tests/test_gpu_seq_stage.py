"""The staged upload of the packed genome image (csrc/seqstats.hip: assembly_build) with small staging blocks.

The image leaves the host through two pinned blocks of GTARS_SEQ_STAGE_BYTES (default 32 MiB) that take turns; the suite's
largest assembly is 2.1 MB, so by default the fill loop runs once: no block is ever reused, no chromosome is cut by a block
seam, no seam falls into the 16 .. 31 padding bytes between two chromosomes.  Here the assembly of test_gpu_seqstats.py (lengths
1, 2, 15, 16, 17, 4095, 4096, 4097, 100,003 and 2,000,000; every chromosome starts and ends with a nucleotide) is built with
blocks of 16, 48, 4096 and 4112 bytes and with the smallest block above 48 bytes whose seams land in all four places that the
fill loop tells apart: inside a chromosome's data, exactly between its last data byte and its first padding byte, inside the
padding, and exactly on the next chromosome's offset (the test finds the size from the packed offsets and checks the places).
Every build takes thousands of blocks, so both staging blocks are refilled many times.

What every build is checked with, always against the plain-Python restatements:
  * sha512t24u, MD5 and alphabet class of every record, hashed from the image (GTARS_REFGET_HOST_LEN above every length):
    any wrong data byte changes a digest; the padding behind an ACGT-only record must be zero or its class changes;
  * every whole sequence as a substring of the image;
  * GC and dinucleotide counts of every whole chromosome, of short regions that between them straddle EVERY block seam under
    a chromosome's data or at its end (nine bytes on either side; with blocks of 16 bytes one region takes up to four seams in
    a row, so that the restatement has tens of thousands of rows to count and not 131,000) and of the last 33 bytes of every
    chromosome, whose last aligned load reads the padding.

Every build is held to its block count: gtars_debug_seq_stage_blocks() rises across it by ceil(image bytes / block), so a switch
that the library ignored -- one block of 32 MiB -- fails the test.

The limit of this test: with blocks this small a copy has long finished when its block's turn comes again, so the fill loop,
the carry of a cut chromosome and the turn-taking are covered -- a missing wait on a copy still in flight is not."""
import numpy as np
import pytest

import refget_ref as RG
import seqstats_ref as R
from test_gpu_seqstats import LENGTHS, _make_sequences, _rs
from test_refget_cpu import check_collection

pytestmark = pytest.mark.gpu


def packed_offsets():
    """(offsets, total) of the image: 16 .. 31 zero bytes behind every chromosome, the next one 16-byte aligned"""
    off, at = [], 0
    for _, n in LENGTHS:
        off.append(at)
        at = (at + n + 16 + 15) & ~15
    return off, at


def seam_places(block):
    """-> {place: [(chromosome index, position in the chromosome or None)]} of the seams k * block inside the image"""
    off, total = packed_offsets()
    places = {"data": [], "end": [], "padding": [], "next": []}
    for c, (_, n) in enumerate(LENGTHS):
        nxt = off[c + 1] if c + 1 < len(LENGTHS) else total
        for seam in range((off[c] // block + 1) * block, min(nxt, total - 1) + 1, block):
            if seam < off[c] + n:
                places["data"].append((c, seam - off[c]))
            elif seam == off[c] + n:
                places["end"].append((c, n))
            elif seam < nxt:
                places["padding"].append((c, None))
            elif c + 1 < len(LENGTHS):
                places["next"].append((c + 1, 0))
    return places


def every_place_block():
    return next(b for b in range(64, 4096, 16) if all(seam_places(b).values()))


def test_the_chosen_block_size_puts_a_seam_in_every_place():
    block = every_place_block()
    assert block % 16 == 0 and block > 48
    assert all(len(v) >= 1 for v in seam_places(block).values()), seam_places(block)
    assert set(k for k, v in seam_places(16).items() if v) == {"data", "end", "padding", "next"}
    assert not seam_places(4096)["padding"] and not seam_places(4112)["end"]  # (why a size is computed)


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """the FASTA file, its sequences and the restatement's records, made once"""
    seqs = _make_sequences()
    path = tmp_path_factory.mktemp("seq_stage") / "asm.fa"
    with open(path, "wb") as f:
        for name, s in seqs.items():
            f.write(b">" + name.encode() + b"\n")
            for k in range(0, len(s), 60):
                f.write(s[k:k + 60] + b"\n")
    want = RG.walk_fasta(path.read_bytes())
    assert [w["length"] for w in want] == [n for _, n in LENGTHS]
    assert RG.ALPHABET_NAMES[want[0]["alphabet"]] == "dna2bit" == RG.ALPHABET_NAMES[want[1]["alphabet"]]  # ACGT-only records
    return str(path), seqs, want


def straddling_rows(block):
    """(rows, seams): regions from 9 bytes before a block seam to 9 bytes behind it, or behind the last of the seams that follow
    within 48 bytes, for every seam that cuts a chromosome's data or falls on its end"""
    places = seam_places(block)
    rows, seams = [], 0
    for c, (name, n) in enumerate(LENGTHS):
        cuts = sorted(p for k, p in places["data"] + places["end"] if k == c)
        seams += len(cuts)
        i = 0
        while i < len(cuts):
            j = i
            while j + 1 < len(cuts) and cuts[j + 1] - cuts[i] <= 48:
                j += 1
            rows.append((name, max(cuts[i] - 9, 0), min(cuts[j] + 9, n)))
            i = j + 1
    return rows, seams


def test_the_straddling_rows_cover_every_seam():
    off, total = packed_offsets()
    for block in (16, 48, 4096, 4112, every_place_block()):
        rows, seams = straddling_rows(block)
        start = dict(zip([name for name, _ in LENGTHS], off))
        covered = set()
        for name, s, e in rows:
            assert e - s <= 66
            covered |= {k for k in range((start[name] + s) // block, (start[name] + e) // block + 1) if start[name] + s <= k * block <= start[name] + e}
        under_data = {k for k in range(1, total // block + 1)
                      if any(o < k * block <= o + n for o, (_, n) in zip(off, LENGTHS))}
        assert under_data <= covered and seams == len(under_data), block


@pytest.mark.parametrize("block", [16, 48, 4096, 4112, "every_place"])
def test_builds_with_small_staging_blocks(written, monkeypatch, block):
    import gtars_amd.refget as G
    from gtars_amd.seqstats import GenomeAssembly, calc_dinucl_freq, calc_gc_content

    path, seqs, want = written
    from gtars_amd._lib import lib

    block = every_place_block() if block == "every_place" else block
    blocks = -(-packed_offsets()[1] // block)
    assert blocks >= 3  # stage[0] is filled a second time (and many more)
    monkeypatch.setenv("GTARS_REFGET_HOST_LEN", str(1 << 30))  # no record goes to the host tail
    col = G.load_fasta(path)  # (the file is read here; the collection's device image is built at its first device call, below)
    check_collection(col, want, True)
    monkeypatch.setenv("GTARS_SEQ_STAGE_BYTES", str(block + 7))  # (rounded down to a multiple of 16)
    # digests of every record, hashed from the collection's image, which this call builds
    before = lib.gtars_debug_seq_stage_blocks()
    text, md5, cls = G.digest_records(col)
    assert lib.gtars_debug_seq_stage_blocks() - before == blocks
    assert (text, md5, cls.tolist()) == ([w["sha512t24u"] for w in want], [w["md5"] for w in want], [w["alphabet"] for w in want])
    # whole sequences out of the image
    n = len(want)
    status, off, blob = G._handle_of(col).substrings(np.arange(n), np.zeros(n), [w["length"] for w in want], on_host=False)
    assert status.tolist() == [0] * n and off.tolist() == np.concatenate([[0], np.cumsum([w["length"] for w in want])]).tolist()
    assert blob == b"".join(w["sequence"] for w in want)
    # counts: whole chromosomes, regions across the seams, the last 33 bytes of every chromosome
    genome = GenomeAssembly(path)
    rows = [(name, 0, size) for name, size in LENGTHS] + straddling_rows(block)[0]
    rows += [(name, max(size - 33, 0), size) for name, size in LENGTHS]
    rs = _rs(rows)
    before = lib.gtars_debug_seq_stage_blocks()
    assert calc_gc_content(rs, genome) == R.calc_gc_content(rows, seqs)  # (the assembly's image is built by its first device call)
    assert lib.gtars_debug_seq_stage_blocks() - before == blocks
    labels, counts = R.calc_dinucl_counts(rows, seqs)
    got = calc_dinucl_freq(rs, genome, raw_counts=True)
    assert got["region_labels"] == labels and got["frequencies"] == [[float(c) for c in row] for row in counts]
    assert genome.device >= 0
