"""A short run of the soak fuzzers inside the GPU suite (round-5 verdict: most of the randomised evidence lived outside the
driver-run suite).  The fuzzers proper -- tests/soak/fuzz_tokenize.py, fuzz_igd.py, fuzz_fragments.py, fuzz_bam.py, fuzz_vrs.py,
fuzz_transcripts.py: hundreds to thousands of cases each, minutes of run time -- stay outside; here 120 + 100 + 3 + 60 cases of
the first three and 60 + 60 + 40 cases of K17 - K20 from their own generators with seeds of this file, every case bit-exact
against the oracle or the restatement like there (their assertions are the test).

The case counts of the three K17 - K20 tests are chosen so that tests/test_soak_generators_cpu.py finds its required edges among
their tags, and so that each test stays within a few seconds.  Measured: the reference side alone (make_case plus expected over
the test's seeds, on a CPU without a device) and the whole test, reference side included, on an MI355X machine (whose CPU is
the faster one):

    test_short_soak_bam          60 cases   reference 0.9 s   on the device 2.9 s
    test_short_soak_vrs          60 cases   reference 0.6 s   on the device 0.4 s
    test_short_soak_transcripts  40 cases   reference 1.3 s   on the device 1.0 s"""
import importlib.util
import os
import shutil
import tempfile

import pytest

pytestmark = pytest.mark.gpu

SOAK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "soak")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(SOAK, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def clean_switches():
    """the fuzzers set GTARS_* switches per case: whatever they left is removed, and the library takes a new snapshot"""
    before = {k: v for k, v in os.environ.items() if k.startswith("GTARS_")}
    yield
    import gtars_amd

    for k in [k for k in os.environ if k.startswith("GTARS_")]:
        if k not in before:
            del os.environ[k]
    os.environ.update(before)
    gtars_amd.reload_env()


def test_short_soak_tokenize(clean_switches):
    fz = _load("fuzz_tokenize")
    ids = 0
    for seed in range(120):
        ids += fz.one(910_000 + seed)[2]
    assert ids > 0


def test_short_soak_igd(clean_switches):
    fz = _load("fuzz_igd")
    for seed in range(100):
        fz.one(920_000 + seed)
    for seed in range(3):
        fz.one_big(930_000 + seed)


def test_short_soak_fragments(clean_switches):
    import oracle
    from gtars_amd.tokenizers import Tokenizer

    fz = _load("fuzz_fragments")
    ub = os.path.join(os.path.dirname(SOAK), "golden", "tokenizers", "peaks.bed")
    chroms = sorted({l.split()[0] for l in open(ub) if l.strip()})
    tok, otok = Tokenizer.from_bed(ub), oracle.OracleTokenizer(ub)
    tmp = tempfile.mkdtemp(prefix="gtars_fuzzfrag_")
    try:
        for seed in range(60):
            fz.one(940_000 + seed, tmp, tok, otok, chroms, ub)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# the seeds of K17 - K20: tests/test_soak_generators_cpu.py runs the generators and the restatements over exactly these, without
# a device, and asserts the edges they reach
BAM_SEEDS = range(950_000, 950_060)
VRS_SEEDS = range(960_000, 960_060)
TRANSCRIPT_SEEDS = range(970_000, 970_040)


def _short_soak(name, seeds, tmp_path):
    fz = _load(name)
    tags = set()
    for seed in seeds:
        tags |= fz.one(seed, tmp_path)
    assert tags


def test_short_soak_bam(clean_switches, tmp_path):
    _short_soak("fuzz_bam", BAM_SEEDS, tmp_path)


def test_short_soak_vrs(clean_switches, tmp_path):
    _short_soak("fuzz_vrs", VRS_SEEDS, tmp_path)


def test_short_soak_transcripts(clean_switches, tmp_path):
    _short_soak("fuzz_transcripts", TRANSCRIPT_SEEDS, tmp_path)
