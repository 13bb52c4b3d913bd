#!/usr/bin/env python3
"""The fused fragment pipeline on BGZF input: GTARS_FRAG_INFLATE=host against =device (both rings), alternating in one process.

Three shapes of BASELINE config 5's fragment files, rewritten as bgzip would write them (zlib level 6, 0xFF00-byte blocks, EOF
block; the block writer of tests/bam_ref.py): 48 files x 1e5 fragments, 1000 files x 1e4, one file of 5e6.  Per shape and
setting: the median of 10 calls after 2 warm-ups (with min and max), the library's stage report of the last call, the member
kernel's time by HIP events and its inflated GB/s.  Every result is compared with the first host call's.  The rule for the
default: device wins a shape when its median lies below the host's by more than the larger of the two
settings' min-max spreads.

  python tools/frag_bgzf_bench.py [--shapes 48x100000,1000x10000,1x5000000] [--out profiles/frag_bgzf_bench.json]
  python tools/frag_bgzf_bench.py --plain   # the plain-gzip config-5 folder only (A/B against another build: GTARS_AMD_LIB)"""
import argparse
import ctypes as C
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import bam_ref  # noqa: E402
import gtars_amd  # noqa: E402
from gtars_amd import _lib, synth  # noqa: E402
from gtars_amd.fragsplit import BarcodeToClusterMap, fragsplit_tokenize  # noqa: E402
from gtars_amd.tokenizers import Tokenizer  # noqa: E402

SETTINGS = [("host", {"GTARS_FRAG_INFLATE": "host"}),
            ("device_ring32", {"GTARS_FRAG_INFLATE": "device", "GTARS_FRAG_INFLATE_RING": "32"}),
            ("device_ring8", {"GTARS_FRAG_INFLATE": "device", "GTARS_FRAG_INFLATE_RING": "8"})]
WARMUPS, CALLS = 2, 10


def rewrite_as_bgzf(src_dir, dst_dir):
    os.mkdir(dst_dir)
    names = sorted(os.listdir(src_dir))

    def one(name):
        with open(os.path.join(src_dir, name), "rb") as f:
            text = zlib.decompress(f.read(), 31)
        data = bam_ref.bgzf_bytes(text)
        with open(os.path.join(dst_dir, name), "wb") as f:
            f.write(data)
        return len(text), len(data), -(-len(text) // 0xFF00) + 1  # (the EOF block is a member as well)

    with ThreadPoolExecutor(max_workers=min(16, len(names))) as ex:
        res = list(ex.map(one, names))
    return sum(r[0] for r in res), sum(r[1] for r in res), sum(r[2] for r in res)


def same(a, b):
    return list(a) == list(b) and all(list(a[k][0]) == list(b[k][0]) and np.array_equal(a[k][1], b[k][1]) and np.array_equal(a[k][2], b[k][2]) for k in a)


def reports():
    st = (C.c_double * 12)()
    _lib.lib.gtars_fragsplit_last_stages(C.cast(st, C.c_void_p))
    keys = ["device_route", "waves", "read_inflate_s", "append_s", "device_waves_s", "behind_last_wave_s", "regroup_s", "h2d_s", "parse_s",
            "gather_s", "tokenize_s", "d2h_s"]
    out = {k: round(v, 6) for k, v in zip(keys, st)}
    if hasattr(_lib.lib, "gtars_fragsplit_last_inflate"):
        z = (C.c_double * 4)()
        _lib.lib.gtars_fragsplit_last_inflate(C.cast(z, C.c_void_p))
        out.update(members_on_device=int(z[0]), files_handed_back=int(z[1]), compressed_bytes_copied=int(z[2]), member_kernel_s=round(z[3], 6))
    return out


def measure(folder, mp, tok, settings, text_bytes):
    m = BarcodeToClusterMap.from_file(mp)
    times, last, want = {n: [] for n, _ in settings}, {}, None
    for rep in range(WARMUPS + CALLS):
        for name, env in settings:
            for k, v in env.items():
                os.environ[k] = v
            gtars_amd.reload_env()
            t = time.perf_counter()
            got = fragsplit_tokenize(folder, m, tok, as_arrays=True)
            dt = time.perf_counter() - t
            if want is None:
                want = got
            assert same(got, want), (name, rep, "differs from the host route's result")
            if rep >= WARMUPS:
                times[name].append(dt)
            last[name] = reports()
    out = {}
    for name, _ in settings:
        ts = times[name]
        r = {"median_s": round(statistics.median(ts), 5), "min_s": round(min(ts), 5), "max_s": round(max(ts), 5), "last_call": last[name]}
        k = last[name].get("member_kernel_s", 0)
        if k:
            r["member_kernel_inflated_GB_per_s"] = round(text_bytes / k / 1e9, 2)
        out[name] = r
    return out


def verdict(res):
    h = res["host"]
    out = {}
    for name in ("device_ring32", "device_ring8"):
        d = res[name]
        spread = max(h["max_s"] - h["min_s"], d["max_s"] - d["min_s"])
        out[name] = {"gain_s": round(h["median_s"] - d["median_s"], 5), "larger_spread_s": round(spread, 5),
                     "wins": h["median_s"] - d["median_s"] > spread}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="48x100000,1000x10000,1x5000000")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["GTARS_HOST_TIMING"] = "1"  # (the member kernel is timed only under it; its lines go to stderr)
    u = synth.make_universe(100_000)
    import torch

    result = {"device": torch.cuda.get_device_name(0), "warmups": WARMUPS, "calls": CALLS, "shapes": {}}
    for shape in a.shapes.split(","):
        files, frags = (int(x) for x in shape.split("x"))
        tmp = tempfile.mkdtemp(prefix="gtars_bgzf_")
        try:
            ub, fd, mp, gz_bytes = synth.write_config5_inputs(tmp, u, files, frags)
            tok = Tokenizer.from_bed(ub)
            if a.plain:
                res = measure(fd, mp, tok, SETTINGS[:1], 0)
                result["shapes"][shape] = {"plain_gzip_bytes": gz_bytes, "plain_gzip": res["host"]}
                continue
            text_bytes, bgzf_bytes, members = rewrite_as_bgzf(fd, os.path.join(tmp, "bgzf"))
            res = measure(os.path.join(tmp, "bgzf"), mp, tok, SETTINGS, text_bytes)
            result["shapes"][shape] = {"text_bytes": text_bytes, "bgzf_bytes": bgzf_bytes, "members": members, "settings": res,
                                       "rule": verdict(res)}
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        print(shape, json.dumps(result["shapes"][shape]), flush=True)
    line = json.dumps(result, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
