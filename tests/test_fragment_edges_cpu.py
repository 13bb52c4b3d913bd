"""The edge cases of tests/fragment_edge_cases.py sit where they claim (no GPU): every witness the builders report is asserted
here, the oracle's restatement of the two-step pipeline accepts every good case and finds tokenized fragments in every mapped
file, and zlib / gzip rejects every corrupt= file with a CRC error and reads its twin.  tests/test_gpu_fragment_edges.py runs the
same cases on the device; this module keeps them from drifting off their edges when a builder is edited."""
import gzip
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fragment_edge_cases as fe  # noqa: E402
from test_sharding_gloo import oracle_fragment_pipeline  # noqa: E402


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """name -> Case, each built once"""
    root = tmp_path_factory.mktemp("fragment_edges")
    builders = fe.all_cases(fe.write_dense_universe(root))
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = builders[name](root)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def oracles():
    import oracle

    cache = {}

    def get(case):
        if case.universe not in cache:
            cache[case.universe] = oracle.OracleTokenizer(case.universe)
        return oracle.OracleBarcodeMap(case.map), cache[case.universe]

    return get


def names(prefix):
    return [n for n in fe.CASE_NAMES if n.startswith(prefix)]


def test_every_section_has_its_cases():
    for prefix, n in (("a_", 19), ("b_", 9), ("c1_", 1), ("c2_", 9), ("d_", 7), ("e_", 17)):
        assert len(names(prefix)) == n, prefix
    assert len(fe.CASE_NAMES) == 62


def test_building_blocks():
    assert len(fe.line("chr1", 5, 9, "BC", 64)) == 64 and len(fe.line("chr1", 5, 9, "BC", 64, eol="\r\n")) == 64
    assert fe.line("chr1", 5, 9, "BC", 14) == "chr1\t5\t9\tBC\t1\n" and len(fe.line("chr1", 5, 9, "BC", 40000).split("\t")) == 6
    with pytest.raises(ValueError):
        fe.line("chr1", 5, 9, "BC", 15)  # (no room for a tab and a byte of filler)
    assert [fe.table_capacity(n) for n in (0, 1, 2, 3, 4, 63, 64, 127, 16383, 16384)] == [1, 4, 8, 8, 16, 128, 256, 256, 32768, 65536]
    # FNV-1a's published vectors, behind the final mix
    for key, fnv in ((b"", 0x811C9DC5), (b"a", 0xE40C292C), (b"foobar", 0xBF9CF968)):
        assert fe.frag_hash(key) == fnv ^ (fnv >> 15)
    text = b"".join(b"%05d....\n" % k for k in range(300))
    blob = fe.gz_members(text, [0, 7, 1500, 1500], levels=(0, 9))
    assert gzip.decompress(blob) == text
    bad = fe.gz_members(text, [7, 1500], corrupt=(1, 9))
    with pytest.raises(gzip.BadGzipFile, match="CRC check failed"):
        gzip.decompress(bad)
    with pytest.raises(AssertionError):
        fe.gz_members(text, [7], corrupt=(1, 4))  # (a digit: not filler)
    lay = fe.device_layout([b"a\nbb", b"", b"c\n"])
    assert lay["text"] == b"a\nbb\nc\n" and lay["file_off"].tolist() == [0, 5, 5, 7] and lay["file_line"].tolist() == [0, 2, 2, 3]
    assert [fe.dense_hits(s, e) for s, e in ((1003, 1083), (1000, 1080), (990, 1001), (0, 1000), (40990, 50000), (41000, 41010), (6000, 9000))] == \
        [9, 8, 1, 0, 1, 0, 300]


# ---------------------------------------------------------------------------------------------------------------- witnesses
def test_a_newlines_sit_on_the_lane_and_chunk_edges(built):
    seen = set()
    for name in names("a_newline_at_"):
        case = built(name)
        pos, lay = case.w["pos"], case.w["layout"]
        assert pos in lay["newlines"] and lay["text"][pos - 1:pos] != b"\r", name
        seen.add((pos % fe.FP_BYTES, pos % fe.FP_CHUNK if pos > 1000 else None))
    # lane bytes 63, 0 and 1 in the middle of a chunk, and the same around the first chunk border (chunk bytes 16383, 0, 1)
    assert seen == {(63, None), (0, None), (1, None), (63, fe.FP_CHUNK - 1), (0, 0), (1, 1)}
    for name, pos in (("a_crlf_split_at_448", 448), ("a_crlf_split_at_16384", fe.FP_CHUNK)):
        lay = built(name).w["layout"]
        assert pos in lay["newlines"] and lay["text"][pos - 1:pos + 1] == b"\r\n" and (pos - 1) % fe.FP_BYTES == 63 and pos % fe.FP_BYTES == 0, name
    for total in (fe.FP_CHUNK, 2 * fe.FP_CHUNK):
        lay = built(f"a_text_of_{total}").w["layout"]
        assert lay["n_bytes"] == total and lay["n_chunks"] * fe.FP_CHUNK == total and lay["newlines"][-1] == total - 1
    lay = built("a_long_lines").w["layout"]
    nl = lay["newlines"]
    lanes_with = set((nl // fe.FP_BYTES).tolist())
    assert any(l not in lanes_with and l + 1 not in lanes_with for l in range(lay["n_bytes"] // fe.FP_BYTES - 1))  # whole lanes inside a line
    assert not np.any((nl >= fe.FP_CHUNK) & (nl < 2 * fe.FP_CHUNK)) and lay["n_chunks"] >= 4  # the second chunk holds no line end
    case = built("a_one_line_no_newline")
    assert not case.texts[0].endswith(b"\n") and len(case.w["layout"]["newlines"]) == 1


def test_a_file_borders_sit_on_the_chunk_and_workgroup_edges(built):
    lay = built("a_file_ends_on_chunk").w["layout"]
    assert lay["file_off"].tolist()[1] == fe.FP_CHUNK and lay["n_bytes"] > fe.FP_CHUNK
    lay = built("a_empty_file_between").w["layout"]
    assert lay["file_off"][1] == lay["file_off"][2] and 0 < lay["file_line"][1] == lay["file_line"][2] < len(lay["newlines"])
    lay = built("a_empty_first_and_last").w["layout"]
    assert lay["file_off"].tolist()[:2] == [0, 0] and lay["file_off"][2] == lay["file_off"][3] == lay["n_bytes"]
    lay = built("a_48_files_of_3_lines").w["layout"]
    assert len(lay["groups"]) == 1 and lay["groups"][0]["files"] == 48 and not lay["groups"][0]["one_file"]
    for n in (255, 256, 257):
        case = built(f"a_first_file_of_{n}_lines")
        lay = case.w["layout"]
        assert lay["file_line"].tolist() == [0, n, n + 20] and len(lay["groups"]) == 2
        # 255: the first workgroup holds a line of the second file; 256: the border IS the workgroup border (both workgroups
        # single-file); 257: the second workgroup starts with the first file's last line
        assert [g["one_file"] for g in lay["groups"]] == {255: [False, True], 256: [True, True], 257: [True, False]}[n]
    for name in names("a_"):
        case = built(name)
        multi = len(case.files) > 1
        assert case.waves == (2 if multi else 1) and (case.env.get("GTARS_HOST_THREADS") == "16") == multi, name
        assert all(not f.endswith(".gz") for f in case.files), name  # plain text: no CRC work


def test_b_groups_sit_on_the_staging_threshold(built):
    def spans(name):
        return [g["span"] for g in built(name).w["layout"]["groups"]]

    assert spans("b_span_32768")[:2] == [fe.PARSE_LDS, 16000]
    assert spans("b_span_32769")[:2] == [fe.PARSE_LDS + 1, 16000 + 1]  # (the second group's base is rounded down to 16 bytes)
    assert spans("b_span_32780_barcode_last")[0] == fe.PARSE_LDS + 12
    lay = built("b_span_32780_barcode_last").w["layout"]
    end = int(lay["newlines"][255])
    assert lay["text"][fe.PARSE_LDS:end] == b"IJKLMNOPQ\t1"  # the last line's barcode ends behind the staging buffer
    s = spans("b_span_40000_then_under")
    assert s[0] == 40000 and s[1] <= fe.PARSE_LDS  # both readers in one launch
    lay = built("b_one_line_of_33k").w["layout"]
    lens = np.diff(np.concatenate([[-1], lay["newlines"][:256]]))
    assert lay["groups"][0]["span"] > fe.PARSE_LDS and lens.max() == 33 << 10 and lens.sum() - lens.max() < fe.PARSE_LDS
    for name, span in (("b_unaligned_span_32768", fe.PARSE_LDS), ("b_unaligned_span_32769", fe.PARSE_LDS + 1)):
        lay = built(name).w["layout"]
        g = lay["groups"]
        assert lay["file_line"].tolist()[:2] == [0, 3] and g[1]["span_lo"] & 15 == 9 and g[1]["span"] == span and g[0]["span"] <= fe.PARSE_LDS, name
        assert not g[0]["one_file"] and g[1]["one_file"]
    for name in names("b_error_"):
        case = built(name)
        g = case.w["layout"]["groups"][0]
        assert g["span"] == 40000 and g["first"] <= case.w["bad_line"] <= g["last"] and case.error, name
    # the parser's rules inside the first (threshold) group of every case: barcodes of 1, 3, 4, 5 and 17 bytes, their unmapped
    # twins, '#', an unknown chromosome, '+', 0, u32::MAX, leading zeros beyond ten digits
    assert sorted(len(b) for b in fe.B_MAPPED) == [1, 3, 4, 5, 17]
    assert all(len(a) == len(b) and a[:-1] == b[:-1] and a != b for a, b in zip(fe.B_MAPPED, fe.B_UNMAPPED))
    for name in names("b_"):
        lay = built(name).w["layout"]
        g = lay["groups"][1 if "unaligned" in name else 0]
        lo, hi = g["span_lo"], int(lay["newlines"][g["last"]]) + 1
        lines = lay["text"][lo:hi].decode().split("\n")
        cols = [l.split("\t") for l in lines if l]
        barcodes = {c[3] for c in cols}
        assert barcodes >= set(fe.B_MAPPED) | set(fe.B_UNMAPPED), name
        assert any(c[0].startswith("#") and c[3] in fe.B_MAPPED for c in cols) and any(c[0] == "chrNope" and c[3] in fe.B_MAPPED for c in cols), name
        starts, ends = {c[1] for c in cols if c[3] in fe.B_MAPPED}, {c[2] for c in cols if c[3] in fe.B_MAPPED}
        assert "0" in starts and "4294967295" in ends and "0000000000000000000012" in starts and any(s.startswith("+") for s in starts), name


def test_c_members_cover_every_fold_length_and_phase(built):
    case = built("c1_member_lengths")
    members = [m for f in case.w["members"] for m in f]
    assert {n for _, n in members} >= set(fe.C1_LENGTHS)
    assert {off % 4 for off, n in members if n} == {0, 1, 2, 3}
    assert {off % 4 for off, n in members if n > fe.CRC_CHUNK} == {0, 1, 2, 3}  # (the unaligned head loop needs a chunk of >= 4 bytes)
    for f, text in zip(case.w["members"], case.texts):
        assert len(text) % 4 == 0 and sum(n for _, n in f) == len(text)
    first, middle, last = (any(cond(f) for f in case.w["members"]) for cond in
                           (lambda f: f[0][1] == 0, lambda f: any(n == 0 for _, n in f[1:-1]), lambda f: f[-1][1] == 0))
    assert first and middle and last
    for name, text in zip(case.files, case.texts):
        assert gzip.decompress(open(case.path(name), "rb").read()) == text


@pytest.mark.parametrize("name", names("c2_"))
def test_c_corrupt_files_fail_their_crc_and_nothing_else(built, name):
    case = built(name)
    blob, twin = open(case.path("f1.bed.gz"), "rb").read(), open(case.twin.path("f1.bed.gz"), "rb").read()
    assert gzip.decompress(twin) == case.texts[0]
    with pytest.raises(gzip.BadGzipFile, match="CRC check failed"):
        gzip.decompress(blob)
    d = zlib.decompressobj(31)
    with pytest.raises(zlib.error, match="incorrect data check"):
        rest = blob
        while rest:  # (member by member)
            d.decompress(rest)
            rest, d = d.unused_data, zlib.decompressobj(31)
    off, n = case.w["members"][0][case.w["member"]]
    byte = case.w["byte"]
    assert case.texts[0][off + byte:off + byte + 1] == b"." and 0 <= byte < n
    where = {"c2_head_byte_unaligned": off % 4 != 0 and byte == 0,
             "c2_last_byte_of_513": n == 513 and byte == 512,
             "c2_last_byte_of_1024": n == 1024 and byte == n - 1,
             "c2_byte_511": n > 1024 and byte == 511,
             "c2_byte_512": n > 1024 and byte == 512,
             "c2_last_chunk_of_first_group": n == 65537 and fe.CRC_GROUP - fe.CRC_CHUNK <= byte < fe.CRC_GROUP,
             "c2_first_byte_of_second_group": n == 65537 and byte == fe.CRC_GROUP,
             "c2_only_byte_of_third_group": n == 65537 and byte == 2 * fe.CRC_GROUP,
             "c2_middle_member_of_three": len([m for m in case.w["members"][0] if m[1] == 4000]) == 3 and
             case.w["members"][0][case.w["member"] - 1][1] == 4000 and case.w["members"][0][case.w["member"] + 1][1] == 4000}
    assert where[name]


def test_d_tables_total_the_slot_counts(built):
    want = {"d_slots_1": ([1], 1), "d_slots_4": ([4], 3), "d_slots_8_two_files": ([4, 4], 4), "d_slots_128": ([128], 8),
            "d_slots_256_two_files": ([128, 128], 9), "d_slots_32768": ([32768], 16), "d_slots_65536": ([65536], 17)}
    assert sorted(want) == names("d_")
    for name, (caps, bits) in want.items():
        case = built(name)
        assert case.w["capacities"] == caps and case.w["total_slots"] == sum(caps) and case.w["key_bits"] == bits, name
        assert (case.env.get("GTARS_HOST_THREADS") == "16") == (len(caps) > 1) and case.waves == (2 if len(caps) > 1 else 1)
        if sum(caps) > 1:
            # the barcode in the highest occupied slot of every table is used, and lines that sort last lie between the mapped ones
            assert all(used == occupied for used, occupied in case.w["highest_used_slot"]), name
            if sum(caps) >= 128:
                assert all(used >= c // 2 for (used, _), c in zip(case.w["highest_used_slot"], caps)), name
            text = case.texts[-1].decode()
            assert "\tNOPE1\t" in text and "\n#" in text and len(text.splitlines()) >= 3000
    # no_key itself needs one bit more than every real key exactly at the powers of two
    assert [built(n).w["total_slots"].bit_length() - (built(n).w["total_slots"] - 1).bit_length() for n in ("d_slots_256_two_files", "d_slots_65536")] == [1, 1]


def test_e_fragments_sit_on_the_emit_chunk_edges(built):
    for n in (1023, 1024, 1025, 2048, 2049):
        w = built(f"e_dense_{n}").w
        assert w["n_tokenized"] == n and w["n_ids"] > 2 * n + 1024 and 7.5 < w["n_ids"] / n < 9.5  # the refill runs
        assert built(f"e_sparse_{n}").w["n_tokenized"] == n
    w = built("e_run_starts_at_1024").w
    assert fe.EM_TPB in w["run_starts"] and w["run_starts"][:2] == [0, fe.EM_TPB]  # ... and the first run ends at 1023
    assert built("e_run_starts_at_1023").w["run_starts"][:2] == [0, fe.EM_TPB - 1]
    w = built("e_unk_at_1023_and_1024").w
    assert w["tagged"]["special"] == [1023, 1024] and [w["hits"][j] for j in (1022, 1023, 1024, 1025)] == [w["hits"][1022], 0, 0, w["hits"][1025]]
    assert w["hits"][1022] and w["hits"][1025]
    w = built("e_unk_opens_run_at_1024").w
    assert w["tagged"]["special"] == [fe.EM_TPB] and fe.EM_TPB in w["run_starts"] and w["hits"][fe.EM_TPB] == 0
    w = built("e_300_hits_at_1023").w
    assert w["tagged"]["special"] == [1023] and w["hits"][1023] == 300
    w = built("e_all_unk").w
    assert w["n_tokenized"] == 1500 and w["n_ids"] == 0 and w["n_emitted"] == 1500
    assert built("e_one_fragment").w["n_tokenized"] == 1
    for name in names("e_"):
        assert built(name).waves == 1 and built(name).w["total_slots"] == 16


# ------------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", fe.CASE_NAMES)
def test_the_oracle_accepts_the_good_cases_and_finds_fragments_in_every_mapped_file(built, oracles, name):
    case = built(name)
    om, otok = oracles(case)
    paths = sorted((os.path.join(case.frags, n) for n in os.listdir(case.frags)), key=os.fsencode)
    if case.error and case.twin is None:
        if case.oracle_error:
            with pytest.raises(ValueError, match=case.oracle_error):
                oracle_fragment_pipeline(paths, om, otok)
        return
    good = case.twin or case
    if case.twin is not None:
        om, otok = oracles(good)
        paths = [good.path("f1.bed.gz")]
    want = oracle_fragment_pipeline(paths, om, otok)
    total = sum(int(v[1][-1]) for v in want.values())
    if name == "d_slots_1":
        assert total == 0 and not good.mapped_files  # no mapped barcode: empty clusters
        return
    assert good.mapped_files, name
    for n in good.mapped_files:
        one = oracle_fragment_pipeline([good.path(n)], om, otok)
        assert sum(int(v[1][-1]) for v in one.values()) > 0, (name, n)
    if "n_emitted" in good.w:  # the model's id count is the oracle's
        assert total == good.w["n_emitted"], name
    if name.startswith("e_sparse_"):
        assert total <= 2 * good.w["n_tokenized"] + 1024, name  # no refill on the sparse universe
