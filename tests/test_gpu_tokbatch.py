"""The batched tokenizer on the MI355X (csrc/tokbatch.hip, K15) against the CPU oracle's per-query CSR plus the plain-Python
restatement tests/tokbatch_ref.py -- never against the library's own single-set call, except for the one consistency check at
the end.  The universe is disjoint 100-bp regions at the multiples of 1000 on three chromosomes, region i of a chromosome
at [1000 i, 1000 i + 100): a query from region f over k consecutive regions yields exactly the ids f .. f + k - 1, so set
lengths are exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tokbatch_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOK = os.path.join(GOLD, "tokenizers")
PER_CHROM = 2000
N_CHROM = 3
UNKNOWN = 0xFFFFFFFF

HIT6 = ("chr1", 151399441, 151399547)
HIT78 = ("chr2", 203871346, 203871616)
MISS = ("chr1", 10, 20)


# ---- the universe, the tokenizer over it and the oracle -------------------------------------------------------------
class World:
    def __init__(self, tok, oracle_index, n_regions):
        self.tok, self.oracle, self.n = tok, oracle_index, n_regions
        self.unk, self.pad = n_regions, n_regions + 1
        self.names = tok.chrom_names

    def rows(self, batch, max_length=None):
        """the expected ragged result: the oracle's CSR of the concatenated batch through the restatement"""
        c, s, e, so = batch
        q_off, ids = self.oracle.tokenize(c, s, e)
        return T.encode_sets(q_off, ids, so, self.unk, max_length)


def _universe_columns():
    from gtars_amd import synth

    chrom = np.repeat(np.arange(N_CHROM, dtype=np.uint32), PER_CHROM)
    start = np.tile(np.arange(PER_CHROM, dtype=np.uint32) * 1000, N_CHROM)
    return [synth.CHROM_NAMES[c] for c in range(N_CHROM)], chrom, start, start + 100


def _write_universe(path):
    names, chrom, start, end = _universe_columns()
    path.write_text("".join(f"{names[c]}\t{s}\t{e}\n" for c, s, e in zip(chrom, start, end)))
    return str(path)


def _world(cfg_path, kind=0):
    import oracle
    from gtars.tokenizers import Tokenizer

    tok = Tokenizer(cfg_path)
    names, chrom, start, end = _universe_columns()
    assert tok.chrom_names == names
    ref = oracle.Index(chrom, start, end, np.arange(len(chrom), dtype=np.uint32), n_chrom=N_CHROM, kind=kind)
    return World(tok, ref, len(chrom))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = _world(_write_universe(tmp_path_factory.mktemp("tokbatch") / "universe.bed"))
    assert w.tok.unk_token_id == w.unk and w.tok.pad_token_id == w.pad
    return w


def q(chrom, first, k):
    """one query row: k >= 1 consecutive regions of `chrom` from region `first`; k == 0: between two regions (no hit)"""
    if k == 0:
        return chrom, first * 1000 + 300, first * 1000 + 400
    assert first + k <= PER_CHROM
    return chrom, first * 1000 + 50, (first + k - 1) * 1000 + 60


def batch_of(sets):
    """sets: lists of query rows (chrom id, start, end) -> the concatenated columns and set_offsets"""
    flat = [r for s in sets for r in s]
    col = lambda k, dt: np.asarray([r[k] for r in flat], dtype=dt) if flat else np.zeros(0, dtype=dt)  # noqa: E731
    so = np.zeros(len(sets) + 1, dtype=np.uint64)
    so[1:] = np.cumsum([len(s) for s in sets], dtype=np.uint64)
    return col(0, np.uint32), col(1, np.uint32), col(2, np.uint32), so


def sets_with_lengths(lengths, seed=1):
    """a batch whose set b yields exactly lengths[b] ids: one query per set (0: a query without a hit)"""
    rng = np.random.RandomState(seed)
    return [[q(int(rng.randint(N_CHROM)), int(rng.randint(0, PER_CHROM - max(k, 1) + 1)), k)] for k in lengths]


def check_ragged(w, batch, max_length=None):
    want = w.rows(batch, max_length)
    off, ids = w.tok.encode_many_arrays(*batch, max_length=max_length)
    w_off, w_ids = T.ragged(want)
    assert off.dtype == np.uint64 and ids.dtype == np.uint32
    assert np.array_equal(off, w_off)
    assert np.array_equal(ids, w_ids)
    return want


def check_padded(w, batch, want, padding="longest", side="right", max_length=None, tensors="np"):
    enc = w.tok.batch_arrays(*batch, padding=padding, max_length=max_length, padding_side=side, return_tensors=tensors)
    ids, mask = enc["input_ids"], enc["attention_mask"]
    if tensors == "pt":
        import torch

        assert ids.is_cuda and mask.is_cuda and ids.dtype == torch.int32 and mask.dtype == torch.uint8
        ids, mask = ids.cpu().numpy().view(np.uint32), mask.cpu().numpy()
    w_ids, w_mask = T.pad_sets(want, w.pad, None if padding == "longest" else padding, side)
    assert ids.shape == w_ids.shape and mask.shape == w_mask.shape
    assert np.array_equal(ids, w_ids)
    assert np.array_equal(mask, w_mask)


# ---- the known-answer batch on the reference's fixture ---------------------------------------------------------------
def _known_sets(tmp_path):
    from gtars.models import Region, RegionSet

    bed = tmp_path / "third.bed"
    bed.write_text("%s\t%d\t%d\n" % HIT78)
    return [[Region(*HIT6)], RegionSet.from_vectors([MISS[0]], [MISS[1]], [MISS[2]]), str(bed)]


def test_known_answer_batch(tmp_path):
    import torch
    from gtars.models import RegionSet
    from gtars.tokenizers import Tokenizer

    tok = Tokenizer(os.path.join(TOK, "tokenizer.toml"))
    sets = _known_sets(tmp_path)
    assert tok.encode_many(sets) == [[6], [25], [7, 8]]
    assert tok.tokenize_many(sets) == [["chr1:151399431-151399527"], ["<unk>"], ["chr2:203871200-203871375", "chr2:203871387-203871588"]]
    as_sets = [RegionSet.from_vectors([r[0]], [r[1]], [r[2]]) for r in (HIT6, MISS, HIT78)]
    assert tok.encode_many(as_sets) == [[6], [25], [7, 8]]  # (the all-RegionSet form: gtars_tokenizer_encode_sets)
    assert tok.encode_many(as_sets, max_length=1) == [[6], [25], [7]]
    right, left = [[6, 26], [25, 26], [7, 8]], [[26, 6], [26, 25], [7, 8]]
    mask_r, mask_l = [[1, 0], [1, 0], [1, 1]], [[0, 1], [0, 1], [1, 1]]
    enc = tok.batch(sets)
    assert enc["input_ids"] == right and enc["attention_mask"] == mask_r and isinstance(enc["input_ids"], list)
    enc = tok.batch(sets, padding_side="left")
    assert enc["input_ids"] == left and enc["attention_mask"] == mask_l
    for side, ids, mask in (("right", right, mask_r), ("left", left, mask_l)):
        enc = tok.batch(sets, padding_side=side, return_tensors="np")
        assert isinstance(enc["input_ids"], np.ndarray) and enc["input_ids"].dtype == np.uint32 and enc["attention_mask"].dtype == np.uint8
        assert enc["input_ids"].tolist() == ids and enc["attention_mask"].tolist() == mask
        enc = tok.batch(sets, padding_side=side, return_tensors="pt")
        assert isinstance(enc["input_ids"], torch.Tensor) and enc["input_ids"].is_cuda and enc["attention_mask"].is_cuda
        assert enc["input_ids"].cpu().tolist() == ids and enc["attention_mask"].cpu().tolist() == mask
    with pytest.raises(ValueError):
        tok.batch(sets, return_tensors="tf")
    with pytest.raises(ValueError):
        tok.batch(sets, padding_side="middle")
    with pytest.raises(ValueError):
        tok.batch(sets, padding="max_length")
    with pytest.raises(ValueError):
        tok.encode_many(sets, max_length=0)


# ---- degenerate batches --------------------------------------------------------------------------------------------------
def test_no_set_one_set_and_sets_without_regions(world):
    w = world
    assert w.tok.encode_many([]) == [] and w.tok.tokenize_many([]) == []
    off, ids = w.tok.encode_many_arrays([], [], [], [0])
    assert off.tolist() == [0] and len(ids) == 0
    for tensors in (None, "np", "pt"):
        enc = w.tok.batch([], return_tensors=tensors)
        assert len(enc["input_ids"]) == 0 and len(enc["attention_mask"]) == 0
    assert w.tok.batch([], padding=4, return_tensors="np")["input_ids"].shape == (0, 4)
    assert tuple(w.tok.batch([], padding=4, return_tensors="pt")["attention_mask"].shape) == (0, 4)
    one = batch_of([[q(1, 5, 3), q(0, 7, 0), q(2, 0, 1)]])
    want = check_ragged(w, one)
    assert want == [[PER_CHROM + 5, PER_CHROM + 6, PER_CHROM + 7, 2 * PER_CHROM]]
    for tensors in ("np", "pt"):
        check_padded(w, one, want, tensors=tensors)
    hollow = batch_of([[], [], [], [], []])
    want = check_ragged(w, hollow)
    assert want == [[w.unk]] * 5
    for tensors in ("np", "pt"):
        check_padded(w, hollow, want, tensors=tensors)
        check_padded(w, hollow, want, padding=3, side="left", tensors=tensors)


# ---- empty sets and the [unk] rule ---------------------------------------------------------------------------------------
UNK_CASES = {
    "empty_first": [[], [q(0, 1, 2)], [q(1, 2, 1)]],
    "empty_last": [[q(0, 1, 2)], [q(1, 2, 1)], []],
    "empty_middle": [[q(0, 1, 2)], [], [q(1, 2, 1)]],
    "empty_runs": [[], [], [q(0, 1, 3)], [], [], [], [q(2, 9, 1)], [], []],
    "regions_without_hit": [[q(0, 3, 0), q(1, 4, 0)], [q(0, 1, 2)], [q(2, 8, 0)]],
    "unknown_chromosome": [[(UNKNOWN, 1050, 1060)], [q(0, 1, 1), (UNKNOWN, 50, 5000)], [(7, 50, 60), (UNKNOWN, 0, 9)]],
    "all_unk": [[], [q(0, 3, 0)], [(UNKNOWN, 50, 60)], [], [q(2, 0, 0), q(1, 1, 0)]],
}


@pytest.mark.parametrize("case", sorted(UNK_CASES))
def test_empty_sets_become_unk(world, case):
    w = world
    batch = batch_of(UNK_CASES[case])
    want = check_ragged(w, batch)
    assert all(len(r) >= 1 for r in want)
    if case == "all_unk":
        assert want == [[w.unk]] * 5
    if case == "unknown_chromosome":
        assert want == [[w.unk], [1], [w.unk]]
    for side in ("right", "left"):
        check_padded(w, batch, want, side=side)
    check_padded(w, batch, want, tensors="pt")
    check_ragged(w, batch, max_length=1)
    check_ragged(w, batch, max_length=2)


# ---- set lengths at the wave, workgroup and pack-tile edges ------------------------------------------------------------------
def _edge_lengths():
    from gtars_amd._lib import lib

    tile = int(lib.gtars_debug_tokbatch_tile())
    return [1, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1]


@pytest.mark.parametrize("with_empty", [False, True], ids=["raw_ids_are_the_result", "packed"])
def test_set_lengths_at_the_edges(world, with_empty):
    w = world
    lengths = _edge_lengths()
    for k in lengths:  # every length on its own, next to an empty set or not
        one = batch_of(sets_with_lengths([k] + ([0] if with_empty else []), seed=k))
        want = check_ragged(w, one)
        assert len(want[0]) == k
    mixed = lengths + lengths[::-1]
    if with_empty:
        mixed = [0] + mixed[:7] + [0, 0] + mixed[7:] + [0]
    batch = batch_of(sets_with_lengths(mixed))
    want = check_ragged(w, batch)
    assert [len(r) for r in want] == [max(k, 1) for k in mixed]
    for side in ("right", "left"):
        check_padded(w, batch, want, side=side, tensors="pt")
    check_padded(w, batch, want, padding=max(mixed) + 3)


@pytest.mark.parametrize("n_sets", [63, 64, 65, 257, 4097])
@pytest.mark.parametrize("with_empty", [False, True], ids=["raw_ids_are_the_result", "packed"])
def test_many_short_sets_share_a_wave(world, n_sets, with_empty):
    w = world
    rng = np.random.RandomState(n_sets)
    lengths = rng.randint(1, 4, size=n_sets)
    if with_empty:
        lengths[rng.rand(n_sets) < 0.2] = 0
        lengths[[0, n_sets // 2, n_sets - 1]] = 0
    batch = batch_of(sets_with_lengths(lengths.tolist(), seed=n_sets + 1))
    want = check_ragged(w, batch)
    check_padded(w, batch, want, side="left" if with_empty else "right", tensors="pt")
    check_ragged(w, batch, max_length=2)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_large_set_among_many_small(world, where):
    """about 200k ids in one set next to 2000 sets of one to three: the pack is balanced over ids, not over sets"""
    w = world
    rng = np.random.RandomState(11)
    small = sets_with_lengths(rng.choice([0, 1, 2, 3], size=2000, p=[0.1, 0.3, 0.3, 0.3]).tolist(), seed=12)
    large = [q(int(rng.randint(N_CHROM)), int(rng.randint(0, PER_CHROM - 500)), 500) for _ in range(400)] + [q(0, 0, 37)]
    at = {"first": 0, "middle": 1000, "last": 2000}[where]
    sets = small[:at] + [large] + small[at:]
    batch = batch_of(sets)
    want = check_ragged(w, batch)
    assert len(want[at]) == 200_037
    check_ragged(w, batch, max_length=200_036)
    check_padded(w, batch, w.rows(batch, 5), max_length=5, tensors="pt")


# ---- padded widths ----------------------------------------------------------------------------------------------------------
def test_padded_widths(world):
    w = world
    ones = batch_of(sets_with_lengths([1, 0, 1, 1, 0, 1, 1]))
    want = check_ragged(w, ones)
    for tensors in ("np", "pt"):
        for side in ("right", "left"):
            check_padded(w, ones, want, side=side, tensors=tensors)  # W = 1
            check_padded(w, ones, want, padding=1, side=side, tensors=tensors)
    for longest in (5, 7):
        lengths = [longest, 1, 0, 3, longest - 1, 2, 0, longest, 4]
        batch = batch_of(sets_with_lengths(lengths, seed=longest))
        want = check_ragged(w, batch)
        for tensors in ("np", "pt"):
            for side in ("right", "left"):
                check_padded(w, batch, want, side=side, tensors=tensors)
                check_padded(w, batch, want, padding=longest, side=side, tensors=tensors)
                check_padded(w, batch, want, padding=longest + 6, side=side, tensors=tensors)
            with pytest.raises(ValueError, match="longest|longer"):
                w.tok.batch_arrays(*batch, padding=longest - 1, return_tensors=tensors)
        enc = w.tok.batch_arrays(*batch, padding=longest - 1, max_length=longest - 1, return_tensors="np")  # (max_length is what cuts)
        assert np.array_equal(enc["input_ids"], T.pad_sets(w.rows(batch, longest - 1), w.pad)[0])


def test_pad_entry_refuses_a_width_that_cannot_hold_a_set_or_be_counted(world):
    import torch
    from gtars_amd import OverlapIndex

    dev = torch.device("cuda", torch.cuda.current_device())
    off = torch.tensor([0, 2, 5], dtype=torch.int64, device=dev)
    ids = torch.arange(5, dtype=torch.int32, device=dev)
    out = torch.full((2, 4), -1, dtype=torch.int32, device=dev)
    mask = torch.full((2, 4), 9, dtype=torch.uint8, device=dev)
    OverlapIndex.pad_sets_device(off.data_ptr(), ids.data_ptr(), 2, 4, 77, out.data_ptr(), mask.data_ptr(), "left")
    assert out.cpu().tolist() == [[77, 77, 0, 1], [77, 2, 3, 4]] and mask.cpu().tolist() == [[0, 0, 1, 1], [0, 1, 1, 1]]
    with pytest.raises(ValueError, match="longer than the width"):
        OverlapIndex.pad_sets_device(off.data_ptr(), ids.data_ptr(), 2, 2, 77, out.data_ptr(), mask.data_ptr())
    with pytest.raises(ValueError, match="overflows"):
        OverlapIndex.pad_sets_device(off.data_ptr(), ids.data_ptr(), 1 << 31, 1 << 40, 77, out.data_ptr(), mask.data_ptr())
    with pytest.raises(ValueError, match="overflows"):
        OverlapIndex.pad_sets_device(off.data_ptr(), ids.data_ptr(), 1 << 31, (1 << 32) - 1, 77, out.data_ptr(), mask.data_ptr())
    with pytest.raises(ValueError):
        OverlapIndex.pad_sets_device(off.data_ptr(), ids.data_ptr(), 2, 4, 77, out.data_ptr(), mask.data_ptr(), "up")


# ---- max_length -------------------------------------------------------------------------------------------------------------
def test_max_length(world):
    w = world
    lengths = [9, 0, 1, 300, 0, 0, 2, 299, 64, 0]
    batch = batch_of(sets_with_lengths(lengths, seed=3))
    full = check_ragged(w, batch)
    assert max(len(r) for r in full) == 300
    for ml in (1, 299, 300, 301, 1 << 40):
        want = check_ragged(w, batch, max_length=ml)
        assert want == [r[:ml] for r in full] and all(len(r) >= 1 for r in want)
        check_padded(w, batch, want, max_length=ml, side="left", tensors="pt")
    dense = batch_of(sets_with_lengths([9, 4, 1, 300, 2, 299, 64], seed=4))  # no empty set: only the cut makes the pack run
    for ml in (1, 299, 300, 301):
        check_ragged(w, dense, max_length=ml)
    with pytest.raises(ValueError):
        w.tok.encode_many_arrays(*batch, max_length=0)


# ---- the device-pointer entry: capacity, sizing pass, malformed set offsets ------------------------------------------------
def _device_call(w, batch, cap, max_length=None, ids_null=False):
    import torch
    from gtars_amd import engine

    c, s, e, so = batch
    dev = torch.device("cuda", torch.cuda.current_device())
    d = [torch.from_numpy(a.view(np.int32)).to(dev) for a in (c, s, e)]
    d_so = torch.from_numpy(so.view(np.int64)).to(dev)
    off = torch.full((len(so),), -1, dtype=torch.int64, device=dev)
    ids = torch.full((cap + 8,), -1, dtype=torch.int32, device=dev)
    try:
        got = engine.tokenize_sets_device(w.tok.engine_index, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(c), d_so.data_ptr(),
                                          len(so) - 1, w.unk, off.data_ptr(), 0 if ids_null else ids.data_ptr(), cap, max_length,
                                          torch.cuda.current_stream().cuda_stream)
        err = None
    except Exception as ex:  # noqa: BLE001
        got, err = None, ex
    return got, err, off.cpu().numpy().view(np.uint64), ids.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("with_empty", [False, True], ids=["raw_ids_are_the_result", "packed"])
def test_capacity_and_sizing_pass(world, with_empty):
    import gtars_amd

    w = world
    lengths = [3, 70, 1, 1, 500, 2] + ([0, 0] if with_empty else []) + [5]
    batch = batch_of(sets_with_lengths(lengths, seed=5))
    want = w.rows(batch)
    w_off, w_ids = T.ragged(want)
    total = len(w_ids)
    got, err, off, ids = _device_call(w, batch, total)
    assert err is None and got == (total, 500)
    assert np.array_equal(off, w_off) and np.array_equal(ids[:total], w_ids)
    assert (ids[total:] == 0xFFFFFFFF).all()  # nothing behind the capacity is touched
    got, err, off, ids = _device_call(w, batch, total - 1)
    assert isinstance(err, gtars_amd.CapacityError) and err.needed == total
    assert np.array_equal(off, w_off)
    assert (ids[total - 1:] == 0xFFFFFFFF).all()
    got, err, off, ids = _device_call(w, batch, 0, ids_null=True)  # the sizing pass
    assert err is None and got == (total, 500) and np.array_equal(off, w_off)
    # a cut that makes the result fit a buffer the raw ids do not fit
    cut = w.rows(batch, 4)
    c_off, c_ids = T.ragged(cut)
    got, err, off, ids = _device_call(w, batch, len(c_ids), max_length=4)
    assert err is None and got == (len(c_ids), 4)
    assert np.array_equal(off, c_off) and np.array_equal(ids[:len(c_ids)], c_ids) and (ids[len(c_ids):] == 0xFFFFFFFF).all()


def test_malformed_set_offsets(world):
    w = world
    c, s, e, so = batch_of(sets_with_lengths([2, 1, 3, 1]))
    for bad in ([1, 2, 3, 4], [0, 2, 1, 4], [0, 1, 2, 3], [0, 1, 2, 5], [0, 1, 2, 1 << 40]):
        bad = np.asarray(bad, dtype=np.uint64)
        with pytest.raises(ValueError, match="set_offsets"):
            w.tok.encode_many_arrays(c, s, e, bad)
        with pytest.raises(ValueError, match="set_offsets"):
            w.tok.batch_arrays(c, s, e, bad, return_tensors="np")
        got, err, _, _ = _device_call(w, (c, s, e, bad), 64)  # (the device entry checks them in k_set_lengths)
        assert isinstance(err, ValueError) and "set_offsets" in str(err)
        with pytest.raises(ValueError, match="set_offsets"):
            w.tok.batch_arrays(c, s, e, bad, return_tensors="pt")
    with pytest.raises(ValueError):
        w.tok.encode_many_arrays(c, s, e, [])
    with pytest.raises(ValueError):
        w.tok.encode_many_arrays(c, s[:-1], e, so)


# ---- other tokenizers ----------------------------------------------------------------------------------------------------
def _fixture_sets():
    import oracle

    peaks = [tuple(r[:3]) for r in oracle.read_region_set(os.path.join(TOK, "peaks.bed"), sort=False)]
    wide = [(c, max(s, 100) - 100, e + 100) for c, s, e in peaks]
    return [peaks[:7], [], [MISS], [("chrZ", 5, 50)], wide, [MISS, ("chrZ", 1, 2)], peaks[::-1], [HIT78, HIT6, HIT78]]


def _as_regions(sets):
    from gtars.models import Region

    return [[Region(*r) for r in s] for s in sets]


def test_ailist_kind_tokenizer():
    import oracle
    from gtars.tokenizers import Tokenizer

    cfg = os.path.join(TOK, "tokenizer_ailist.toml")
    tok, ref = Tokenizer(cfg), oracle.OracleTokenizer(cfg)
    sets = _fixture_sets()
    want = [ref.encode_regions(s) for s in sets]
    assert tok.encode_many(_as_regions(sets)) == want
    enc = tok.batch(_as_regions(sets), padding_side="left", return_tensors="np")
    w_ids, w_mask = T.pad_sets(want, 26, side="left")
    assert np.array_equal(enc["input_ids"], w_ids) and np.array_equal(enc["attention_mask"], w_mask)


def test_custom_unk_and_pad_tokens(tmp_path):
    import oracle
    from gtars.tokenizers import Tokenizer

    _write_universe(tmp_path / "universe.bed")
    cfg = tmp_path / "custom.toml"
    cfg.write_text('universe = "universe.bed"\nspecial_tokens = [\n    {name="pad", token="<PADDING>"},\n    {name="unk", token="<UNKNOWN>"},\n]\n')
    w = _world(str(cfg))
    ref = oracle.OracleTokenizer(str(cfg))
    assert w.tok.unk_token == "<UNKNOWN>" and w.tok.pad_token == "<PADDING>"
    assert w.tok.unk_token_id == ref.universe.region_to_id["<UNKNOWN>"] and w.tok.pad_token_id == ref.universe.region_to_id["<PADDING>"]
    w.unk, w.pad = w.tok.unk_token_id, w.tok.pad_token_id
    sets = [[q(0, 4, 2)], [], [q(2, 1, 0)], [q(1, 0, 3)]]
    batch = batch_of(sets)
    want = check_ragged(w, batch)
    assert want == [[4, 5], [w.unk], [w.unk], [PER_CHROM, PER_CHROM + 1, PER_CHROM + 2]]
    check_padded(w, batch, want, tensors="pt")
    from gtars.models import Region

    names = w.names
    assert w.tok.tokenize_many([[Region(names[c], s, e) for c, s, e in st] for st in sets])[1:3] == [["<UNKNOWN>"], ["<UNKNOWN>"]]


# ---- random differential ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sets", [2, 17, 300])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_batches(world, seed, n_sets):
    from gtars_amd import synth

    w = world
    rng = np.random.RandomState(1000 * seed + n_sets)
    sizes = rng.randint(0, 401, size=n_sets)
    sizes[rng.rand(n_sets) < 0.2] = 0
    so = np.zeros(n_sets + 1, dtype=np.uint64)
    so[1:] = np.cumsum(sizes, dtype=np.uint64)
    _, chrom, start, end = _universe_columns()
    qs = synth.make_queries({"chrom": chrom, "start": start, "end": end}, int(so[-1]), seed=seed)
    c = np.where(qs["chrom"] < N_CHROM, qs["chrom"], UNKNOWN).astype(np.uint32)
    # (the background queries were drawn on hg38: bring them onto the universe's span, so that they hit and miss)
    s = (qs["start"] % np.uint32(PER_CHROM * 1000)).astype(np.uint32)
    e = s + (qs["end"] - qs["start"]) * np.uint32(1 + seed)
    batch = (c, s, e, so)
    want = check_ragged(w, batch)
    assert sum(r == [w.unk] for r in want) >= int((sizes == 0).sum())
    check_padded(w, batch, want, side="right", tensors="pt")
    check_padded(w, batch, want, side="left", tensors="np")
    ml = 1 + int(rng.randint(0, 50))
    check_padded(w, batch, check_ragged(w, batch, max_length=ml), max_length=ml, tensors="pt")


# ---- consistency with the single-set call ------------------------------------------------------------------------------------
def test_one_set_equals_the_single_set_call(world):
    from gtars.models import Region

    w = world
    names = w.names
    for rows in ([q(0, 3, 4), q(2, 9, 0), q(1, 7, 2)], [q(1, 5, 0)], []):
        regions = [Region(names[c], s, e) for c, s, e in rows]
        single = [int(i) for i in w.tok._encode_regions(regions)]
        assert w.tok.encode_many([regions]) == [single]
        assert w.tok.batch([regions])["input_ids"] == [single]
