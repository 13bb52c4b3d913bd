"""Plain numpy / Python restatement of the batched tokenizer (K15), written from its semantics alone: a batch of region sets
is B independent Tokenizer::tokenize calls (gtars-tokenizers/src/tokenizer.rs:140-163), padded the way the reference's Python
binding builds input_ids / attention_mask (gtars-python/src/tokenizers/py_tokenizers/mod.rs:275-299).  Imports nothing of
the package under test."""
import numpy as np


def check_set_offsets(set_offsets, n):
    """set_offsets[0 .. B]: starts at 0, never descends, ends at n"""
    so = [int(x) for x in set_offsets]
    if len(so) < 1 or so[0] != 0:
        raise ValueError("set_offsets must start at 0")
    if any(a > b for a, b in zip(so, so[1:])):
        raise ValueError("set_offsets must never descend")
    if so[-1] != int(n):
        raise ValueError("set_offsets must end at the number of regions")
    return so


def encode_sets(q_off, ids, set_offsets, unk, max_length=None):
    """q_off[nq + 1], ids: the per-query CSR of the concatenated batch (regions on unknown chromosomes have an empty range).
    -> the ragged result as a list of B lists: set b's ids in region order, [unk] if there is none, then the first max_length"""
    if max_length is not None and max_length < 1:
        raise ValueError("max_length must be at least 1")
    so = check_set_offsets(set_offsets, len(q_off) - 1)
    out = []
    for b in range(len(so) - 1):
        row = [int(x) for x in ids[int(q_off[so[b]]):int(q_off[so[b + 1]])]]
        if not row:
            row = [int(unk)]
        if max_length is not None:
            row = row[:max_length]
        out.append(row)
    return out


def ragged(rows):
    """list of lists -> (out_offsets u64[B + 1], out_ids u32)"""
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    for b, r in enumerate(rows):
        off[b + 1] = off[b] + np.uint64(len(r))
    flat = [x for r in rows for x in r]
    return off, np.asarray(flat, dtype=np.uint32)


def pad_sets(rows, pad, width=None, side="right"):
    """-> (input_ids u32[B, W], attention_mask u8[B, W]); W = the longest row, or `width`, which must hold it"""
    if side not in ("right", "left"):
        raise ValueError("side")
    longest = max((len(r) for r in rows), default=0)
    if width is None:
        width = longest
    elif width < longest:
        raise ValueError(f"width {width} is smaller than the longest set ({longest})")
    ids = np.full((len(rows), width), pad, dtype=np.uint32)
    mask = np.zeros((len(rows), width), dtype=np.uint8)
    for b, r in enumerate(rows):
        if not r:
            continue
        if side == "right":
            ids[b, :len(r)] = r
            mask[b, :len(r)] = 1
        else:
            ids[b, width - len(r):] = r
            mask[b, width - len(r):] = 1
    return ids, mask
