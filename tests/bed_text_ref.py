"""The definitions of RegionSet.identifier / file_digest / to_bed and RegionSetList.identifier, restated with hashlib over
plain Python columns (gtars-core/src/models/region_set.rs:240-330, 502-505, region.rs:30-40, region_set_list.rs:85-98).

Rows are (chr, start, end, rest) tuples, rest a str or None, in the order given: nothing here sorts but ``sort_rows`` and
``load``.  Names and rest are encoded as UTF-8."""
import gzip
import hashlib


def md5_hex(data: bytes) -> str:
    return hashlib.md5(data).hexdigest()


def identifier(rows) -> str:
    c = md5_hex(",".join(r[0] for r in rows).encode())
    s = md5_hex(",".join(str(r[1]) for r in rows).encode())
    e = md5_hex(",".join(str(r[2]) for r in rows).encode())
    return md5_hex(f"{c},{s},{e}".encode())


def line(row) -> bytes:
    chr_, start, end, rest = row
    return (f"{chr_}\t{start}\t{end}" + (f"\t{rest}" if rest else "") + "\n").encode()


def bed_text(rows) -> bytes:
    return b"".join(line(r) for r in rows)


def file_digest(rows) -> str:
    return md5_hex(bed_text(rows))


def list_identifier(sets) -> str:
    return md5_hex("".join(sorted(identifier(rows) for rows in sets)).encode())


def sort_rows(rows):
    """stable by (chr bytewise, start)"""
    return sorted(rows, key=lambda r: (r[0].encode(), r[1]))


def load(path):
    """a BED file as sorted rows: comment lines (#, browser, track) and a first line whose start is not a number are skipped"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    rows, first = [], True
    for raw in data.decode().split("\n"):
        raw = raw.rstrip("\r")
        if not raw:
            continue
        if raw.startswith(("#", "browser", "track")):
            first = False
            continue
        f = raw.split("\t", 3)
        if first and len(f) >= 3 and not f[1].isdigit():
            first = False
            continue
        first = False
        rows.append((f[0], int(f[1]), int(f[2]), f[3] if len(f) > 3 and f[3] else None))
    return sort_rows(rows)
