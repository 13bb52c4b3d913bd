"""The device stages of the fused fragment pipeline (gtars_amd/csrc/fragparse.hip) at their thresholds: the cases
of tests/fragment_edge_cases.py (tests/test_fragment_edges_cpu.py proves that each sits on its edge), every good one three ways --
the device route, the host parser (GTARS_FRAG_HOST_PARSE=1) and the oracle's restatement of the two-step pipeline -- which must
agree barcode by barcode and id by id; every failing one with the reference's message on every route.  A false alarm of the
device stage is not silent: the host then re-parses the file and the call ends with "the device parser rejected a line that the
host parser accepts", so a good case that raises is a failure of the device stage."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fragment_edge_cases as fe  # noqa: E402
from test_sharding_gloo import oracle_fragment_pipeline, same_cluster_results  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the case builders, and one tokenizer / oracle tokenizer per universe, each made once"""
    import gtars_amd
    import oracle
    from gtars_amd.tokenizers import Tokenizer

    assert gtars_amd.device_count() > 0
    root = tmp_path_factory.mktemp("fragment_edges")
    builders = fe.all_cases(fe.write_dense_universe(root))
    toks = {}

    def tokenizers(universe):
        if universe not in toks:
            toks[universe] = (Tokenizer.from_bed(universe), oracle.OracleTokenizer(universe))
        return toks[universe]

    return lambda name: builders[name](root), tokenizers


def names(*prefixes):
    return [n for n in fe.CASE_NAMES if n.startswith(prefixes)]


def run(case, tok):
    from gtars_amd.fragsplit import BarcodeToClusterMap, fragsplit_tokenize

    return fragsplit_tokenize(case.frags, BarcodeToClusterMap.from_file(case.map), tok, as_arrays=True)


def device_route(case, tok, monkeypatch, capfd):
    """The call on the device route.  Where the case says how many batches it is about (a lead file and the case's files: two;
    one file: one), the library's timing report must say the same -- batches size themselves by thread timing, so a call that
    was cut otherwise is made again (its result is checked all the same), a few times at the most."""
    monkeypatch.setenv("GTARS_HOST_TIMING", "1")
    results, waves = [], None
    for _ in range(6):
        capfd.readouterr()
        results.append(run(case, tok))
        m = re.search(r"(\d+) files in (\d+) wave\(s\)", capfd.readouterr().err)
        assert m and int(m.group(1)) == len(os.listdir(case.frags))
        waves = int(m.group(2))
        if case.waves is None or waves == case.waves:
            break
    monkeypatch.delenv("GTARS_HOST_TIMING")
    print(f"{case.name}: {waves} batch(es), {len(results)} call(s)")
    assert case.waves is None or waves == case.waves, f"{case.name}: the files of the case never shared one batch"
    return results


def three_ways(case, world, monkeypatch, capfd, also=()):
    import oracle

    tok, otok = world[1](case.universe)
    from gtars_amd.fragsplit import list_fragment_files

    want = oracle_fragment_pipeline(list_fragment_files(case.frags), oracle.OracleBarcodeMap(case.map), otok)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    for got in device_route(case, tok, monkeypatch, capfd):
        assert same_cluster_results(got, want), (case.name, "device route")
    for switch in ("GTARS_FRAG_HOST_PARSE",) + tuple(also):
        monkeypatch.setenv(switch, "1")
        assert same_cluster_results(run(case, tok), want), (case.name, switch)
        monkeypatch.delenv(switch)
    return want


def messages(case, world, monkeypatch):
    """the call's error message on the device route, with the CRC on the host, and on the host parser"""
    tok, _ = world[1](case.universe)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    out = []
    for switch in (None, "GTARS_FRAG_HOST_CRC", "GTARS_FRAG_HOST_PARSE"):
        if switch:
            monkeypatch.setenv(switch, "1")
        with pytest.raises(RuntimeError, match=case.error) as e:
            run(case, tok)
        out.append(str(e.value))
        if switch:
            monkeypatch.delenv(switch)
    return out


@pytest.mark.parametrize("name", names("a_"))
def test_line_split_geometry(world, monkeypatch, capfd, name):
    """k_frag_lines / k_frag_scan_chunks / k_frag_file_lines: line ends on bytes 63 / 0 / 1 of a lane and of a 16-KiB chunk, texts
    of whole chunks, CRLF across a lane and a chunk border, lanes and chunks without a line end, file borders on chunk borders
    and on the 256-line workgroup border of k_frag_parse, empty files, one workgroup over 48 files"""
    want = three_ways(world[0](name), world, monkeypatch, capfd)
    assert sum(int(v[1][-1]) for v in want.values()) > 0


@pytest.mark.parametrize("name", [n for n in names("b_") if "error" not in n])
def test_lds_staging_threshold(world, monkeypatch, capfd, name):
    """k_frag_parse: groups of 256 lines whose span is 32768 (staged), 32769 and beyond (read in global memory), aligned and
    not, with every line rule inside them"""
    want = three_ways(world[0](name), world, monkeypatch, capfd)
    assert sum(int(v[1][-1]) for v in want.values()) > 0


@pytest.mark.parametrize("name", names("b_error"))
def test_lds_staging_threshold_errors(world, monkeypatch, name):
    """the reference's message for a line it fails on, found by the global-memory reader"""
    case = world[0](name)
    msgs = messages(case, world, monkeypatch)
    assert msgs[0] == msgs[1] == msgs[2], msgs


def test_crc_fold_at_every_member_length(world, monkeypatch, capfd):
    """k_crc_chunks / k_crc_groups / k_crc_members: members of 0 .. 3 x 32768 bytes at every start offset mod 4; the same result
    with the CRC on the host"""
    want = three_ways(world[0]("c1_member_lengths"), world, monkeypatch, capfd, also=("GTARS_FRAG_HOST_CRC",))
    assert sum(int(v[1][-1]) for v in want.values()) > 0


@pytest.mark.parametrize("name", names("c2_"))
def test_crc_depends_on_every_fold_position(world, monkeypatch, capfd, name):
    """one data byte changed under an unchanged trailer, at every position of the fold: the reference's data error on every
    route, with one message; the uncorrupted twin passes"""
    case = world[0](name)
    msgs = messages(case, world, monkeypatch)
    assert msgs[0] == msgs[1] == msgs[2] and "gzip read error" in msgs[0], msgs
    three_ways(case.twin, world, monkeypatch, capfd, also=("GTARS_FRAG_HOST_CRC",))


@pytest.mark.parametrize("name", names("d_"))
def test_sort_key_width(world, monkeypatch, capfd, name):
    """the radix sort's key width: 1, 3, 4, 8 (one pass), 9 (two passes: the ninth bit is set in no_key alone), 16 and 17
    (three passes) bits; unrouted and '#' lines sort last, a barcode's fragments keep their line order"""
    want = three_ways(world[0](name), world, monkeypatch, capfd)
    assert (sum(int(v[1][-1]) for v in want.values()) > 0) == (name != "d_slots_1")


@pytest.mark.parametrize("name", names("e_"))
def test_regrouping_and_capacity_refill(world, monkeypatch, capfd, name):
    """k_frag_emit_counts / k_frag_emit and the refill behind a short capacity guess: 1023 .. 2049 fragments on a universe of
    ~9 ids per fragment (refill) and on the sparse golden one (none), run borders, zero-hit and 300-hit fragments on the border
    of the 1024-fragment chunks, a batch of unk ids only, a batch of one fragment"""
    case = world[0](name)
    want = three_ways(case, world, monkeypatch, capfd)
    if "n_emitted" in case.w:
        assert sum(int(v[1][-1]) for v in want.values()) == case.w["n_emitted"]
