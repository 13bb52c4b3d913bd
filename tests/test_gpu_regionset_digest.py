"""K25 on the device (csrc/bed_text.hip) against the hashlib restatement (tests/bed_text_ref.py): exact equality of the
identifiers, file digests and BED text, from the list calls of gtars.models and from gtars_bed_digests_device on resident
columns, at the smallest shapes that can break the kernels: MD5's padding edges as stream lengths, the digit-count edges,
sets of one to three rows (the commas), names of 1 to 40 bytes under different ids, partly filled waves and wave boundaries,
a 1-row set next to a 5000-row set, the host tail, several chunks, the fill past its grid cap, rest on some rows."""
import os
import random

import numpy as np
import pytest

import bed_text_ref as R
from test_regionset_digest_cpu import BEDSET, BEDSET_IDENTIFIER, FILE_DIGEST, IDENTIFIER, PEAKS, make_set, random_rows

pytestmark = pytest.mark.gpu

PAD_EDGES = [0, 1, 55, 56, 63, 64, 65, 119, 120, 128]
DIGIT_EDGES = [0, 9, 10, 99, 100, 999999999, 1000000000, 4294967295]
NEW_SWITCHES = ("GTARS_BED_DIGEST_HOST_LEN", "GTARS_BED_TEXT_BYTES", "GTARS_BED_TEXT_DEVICE_ROWS", "GTARS_GRID_CAP")


@pytest.fixture(scope="module")
def M():
    import gtars_amd
    import gtars_amd.models as M

    assert gtars_amd.device_count() > 0
    assert not [s for s in NEW_SWITCHES if s in os.environ]
    return M


def stream_lengths(rows):
    """the byte lengths of the four streams of a set"""
    return [len(",".join(r[0] for r in rows).encode()), len(",".join(str(r[1]) for r in rows)), len(",".join(str(r[2]) for r in rows)),
            len(R.bed_text(rows))]


def device_digests(sets, what):
    """gtars_bed_digests_device on resident columns.  The names table holds every set's names in the set's own order of first
    appearance, one set after the other: a name that two sets share stands in the table twice, under different ids."""
    import torch

    from gtars_amd._lib import check, lib

    set_off, chrom, start, end, has_rest, rest_off, names, rest = [0], [], [], [], [], [0], [], bytearray()
    for rows in sets:
        base, mine = len(names), {}
        for c, s, e, x in rows:
            if c not in mine:
                mine[c] = base + len(mine)
                names.append(c.encode())
            chrom.append(mine[c]), start.append(s), end.append(e), has_rest.append(1 if x else 0)
            rest += (x or "").encode()
            rest_off.append(len(rest))
        set_off.append(len(chrom))
    name_off = np.cumsum([0] + [len(n) for n in names]).astype(np.uint64)
    dev = torch.device("cuda:0")

    def up(values, dtype, as_dtype):
        a = np.ascontiguousarray(values, dtype=dtype)
        return torch.from_numpy(a.view(as_dtype).copy()).to(dev)

    cols = [up(chrom, np.uint32, np.int32), up(start, np.uint32, np.int32), up(end, np.uint32, np.int32), up(name_off, np.uint64, np.int64),
            up(np.frombuffer(b"".join(names), dtype=np.uint8), np.uint8, np.uint8), up(rest_off, np.uint64, np.int64),
            up(np.frombuffer(bytes(rest), dtype=np.uint8), np.uint8, np.uint8), up(has_rest, np.uint8, np.uint8)]
    c, s, e, no, nb, ro, rb, hr = (t.data_ptr() for t in cols)
    out = torch.zeros(16 * len(sets) + 8, dtype=torch.uint8, device=dev)
    h_set_off = np.array(set_off, dtype=np.uint64)
    check(lib.gtars_bed_digests_device(h_set_off.ctypes.data, len(sets), c, s, e, no, nb, len(names), ro, rb, hr, what, out.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream))
    raw = out.cpu().numpy().tobytes()
    return [raw[16 * i:16 * i + 16].hex() for i in range(len(sets))]


def check_both_ways(M, sets):
    """the list calls and the device entry against the restatement, identifiers and file digests"""
    want_id, want_fd = [R.identifier(rows) for rows in sets], [R.file_digest(rows) for rows in sets]
    lst = M.RegionSetList([make_set(M, rows) for rows in sets])
    assert lst.identifiers(on_host=False) == want_id
    assert lst.file_digests(on_host=False) == want_fd
    assert device_digests(sets, 0) == want_id
    assert device_digests(sets, 1) == want_fd
    return lst


def test_the_reference_literals_on_the_device(M):
    lst = M.RegionSetList([M.RegionSet(PEAKS), M.RegionSet(PEAKS + ".bed.gz")])
    assert lst.identifiers(on_host=False) == [IDENTIFIER] * 2 and lst.file_digests(on_host=False) == [FILE_DIGEST] * 2
    bedset = M.RegionSetList([M.RegionSet(p) for p in BEDSET])
    assert bedset.identifier(on_host=False) == BEDSET_IDENTIFIER == bedset.identifier(on_host=True)
    assert bedset.identifiers(on_host=False) == [R.identifier(R.load(p)) for p in BEDSET]


def test_md5_padding_edges_as_stream_lengths(M):
    """one-row sets whose name stream, and whose line, has exactly the edge length; the empty set is length 0"""
    sets = [[]]
    for n in PAD_EDGES[1:]:
        sets.append([("n" * n, 7, 8, None)])                 # CHR stream of n bytes
        fixed = len(R.line(("c", 5, 6, None)))               # c \t 5 \t 6 \n
        if n > fixed:
            sets.append([("c", 5, 6, "r" * (n - fixed - 1))])   # LINE stream of n bytes
    sets.append([("c", 1, 2, None)] * 28)                    # START / END streams of 55 bytes, CHR of 55
    sets.append([("c", 1, 2, None)] * 28 + [("c", 10, 20, None)])  # ... of 58; and below 56, 64, 120 by digits and commas
    sets.append([("c", 10, 10, None)] * 19)                  # 19 * 3 - 1 = 56
    sets.append([("c", 100, 1000, None)] * 16)               # 16 * 4 - 1 = 63, 16 * 5 - 1 = 79
    sets.append([("c", 1000, 10, None)] * 13)                # 13 * 5 - 1 = 64
    sets.append([("c", 10000, 100, None)] * 11 + [("c", 1, 10, None)])  # 65, 46
    sets.append([("c", 100, 10000, None)] * 30)              # 119
    sets.append([("c", 10, 100, None)] * 40 + [("c", 1, 1000000, None)])  # 121; 40 * 4 + 7 = 167
    sets.append([("c", 100, 10, None)] * 30 + [("c", 0, 1, None)])  # 30 * 4 + 1 = 121
    sets.append([("cc", 10, 100, None)] * 40)                # CHR 119, START 119
    sets.append([("cc", 10, 100, None)] * 40 + [("", 0, 0, None)])  # CHR 120 (an empty name behind the comma)
    sets.append([("c", 1000000, 1, None)] * 16 + [("c", 1, 1, None)])  # 16 * 8 + 1 = 129
    sets.append([("c", 1000000, 1, None)] * 16)              # 127
    sets.append([("ccc", 1, 1, None)] * 32 + [("", 0, 0, None)])   # CHR 32 * 4 = 128
    seen = {n for rows in sets for n in stream_lengths(rows)}
    assert set(PAD_EDGES) <= seen, sorted(set(PAD_EDGES) - seen)
    check_both_ways(M, sets)


def test_digit_edges_commas_and_names(M):
    edge_rows = [("chr1", a, b, None) for a in DIGIT_EDGES for b in DIGIT_EDGES]
    sets = [edge_rows, edge_rows[:1], edge_rows[5:7], edge_rows[61:64]]  # 64, 1, 2 and 3 rows
    sets += [[("c", v, v, None)] for v in DIGIT_EDGES]
    names = ["x", "chr_8_by", "chr_9_byt", "n" * 40]
    sets.append([(nm, 1, 2, None) for nm in names])
    sets.append([(nm, 3, 4, "rest") for nm in reversed(names)])  # the same names under other ids
    sets.append([(names[k % 4], k, k + 1, None) for k in range(9)])
    check_both_ways(M, sets)


@pytest.fixture(scope="module")
def big_batch():
    """70 sets: a 1-row set next to a 5000-row set, the rest small; 210 streams, rest on some rows"""
    rng = random.Random(2511)
    sets = [random_rows(rng, rng.randrange(0, 60)) for _ in range(68)]
    sets.insert(30, random_rows(rng, 5000))
    sets.insert(30, [("chr1", 1, 2, None)])
    assert len(sets) == 70 and len(sets[30]) == 1 and len(sets[31]) == 5000
    return sets, [R.identifier(rows) for rows in sets], [R.file_digest(rows) for rows in sets]


def test_wave_layout(M, big_batch):
    """1, 21, 22 and 70 sets are 3, 63, 66 and 210 streams: a partly filled wave, a wave boundary, several workgroups"""
    sets, want_id, want_fd = big_batch
    lst = [make_set(M, rows) for rows in sets]
    for n in (1, 21, 22, 70):
        part = M.RegionSetList(lst[:n] if n < 70 else lst)
        assert part.identifiers(on_host=False) == want_id[:n]
        assert part.file_digests(on_host=False) == want_fd[:n]
    assert device_digests(sets, 0) == want_id and device_digests(sets, 1) == want_fd
    assert M.RegionSetList(lst).identifier(on_host=False) == R.list_identifier(sets)


def test_routes_agree(M, big_batch, monkeypatch):
    """the host tail for most streams, for none, and several chunks with one set larger than the chunk: one batch, equal results"""
    sets, want_id, want_fd = big_batch
    lst = M.RegionSetList([make_set(M, rows) for rows in sets])
    lengths = [n for rows in sets for n in stream_lengths(rows)[:3]]
    assert sum(n > 256 for n in lengths) > len(lengths) // 2 and sum(n <= 256 for n in lengths) >= 10
    got = {}
    for name, value in (("GTARS_BED_DIGEST_HOST_LEN", "256"), ("GTARS_BED_DIGEST_HOST_LEN", str(1 << 39)), ("GTARS_BED_TEXT_BYTES", "4096")):
        monkeypatch.setenv(name, value)
        got[name, value] = (lst.identifiers(on_host=False), lst.file_digests(on_host=False), device_digests(sets, 0), device_digests(sets, 1))
        monkeypatch.delenv(name)
    for route in got.values():
        assert route == (want_id, want_fd, want_id, want_fd)


def test_fill_past_its_grid_cap(M, big_batch, monkeypatch):
    """GTARS_GRID_CAP=2: k_csr_fill over BedTextSrc walks its grid-stride loop many times (two workgroups write 4096 bytes a trip)"""
    from gtars_amd._lib import lib

    sets, want_id, want_fd = big_batch
    assert sum(stream_lengths(sets[31])[:3]) > 5 * 2048 * 2 and stream_lengths(sets[31])[3] > 5 * 2048 * 2
    lst = M.RegionSetList([make_set(M, rows) for rows in sets[28:34]])
    monkeypatch.setenv("GTARS_GRID_CAP", "2")
    clips = lib.gtars_debug_grid_clips()
    assert lst.identifiers(on_host=False) == want_id[28:34]
    assert lst.file_digests(on_host=False) == want_fd[28:34]
    assert lst[3]._bed_text(False) == R.bed_text(sets[31])
    assert lib.gtars_debug_grid_clips() > clips


def test_line_text_from_the_device(M, monkeypatch, tmp_path):
    rng = random.Random(2512)
    rows = random_rows(rng, 300)
    rows[0] = ("chr1", 0, 4294967295, "tabs\tinside\t\tthe rest")
    rows[299] = ("chr1", 1000000000, 999999999, None)
    assert any(r[3] for r in rows) and any(not r[3] for r in rows)
    rs = make_set(M, rows)
    assert rs._bed_text(False) == rs._bed_text(True) == R.bed_text(rows)
    assert M.RegionSet.from_regions([])._bed_text(False) == b""
    monkeypatch.setenv("GTARS_BED_TEXT_DEVICE_ROWS", "0")  # to_bed formats on the device
    rs.to_bed(tmp_path / "device.bed")
    rs.to_bed_gz(tmp_path / "device.bed.gz")
    monkeypatch.setenv("GTARS_BED_TEXT_DEVICE_ROWS", "1000000")  # ... and on the host
    rs.to_bed(tmp_path / "host.bed")
    import gzip

    assert (tmp_path / "device.bed").read_bytes() == (tmp_path / "host.bed").read_bytes() == R.bed_text(rows)
    assert gzip.decompress((tmp_path / "device.bed.gz").read_bytes()) == R.bed_text(rows)


def test_random_batches(M):
    """100 batches from fixed seeds, at most 40 sets of at most 300 rows, through the device entry"""
    for seed in range(100):
        rng = random.Random(2600 + seed)
        sets = [random_rows(rng, rng.randrange(0, 301) if rng.random() < 0.7 else rng.choice([0, 1, 2])) for _ in range(rng.randrange(1, 41))]
        assert device_digests(sets, 0) == [R.identifier(rows) for rows in sets], seed
        assert device_digests(sets, 1) == [R.file_digest(rows) for rows in sets], seed
