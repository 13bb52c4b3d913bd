"""A pure Python (struct + zlib) BGZF / BAM writer and reader, and bam_qc_ref: gtars-uniwig/src/bamqc.rs:68-245 restated
statement by statement.  Written from the SAM/BAM specification (sections 4.1 and 4.2); nothing here touches the library.

A record is a dict: ref_id, pos (0-based, -1 = none), mapq, flag, name (bytes, without the NUL; b"*" = missing), cigar (list of
(op letter, length)), l_seq, next_ref_id, next_pos, tlen.  Missing keys take the defaults of rec()."""
import struct
import zlib

CIGAR_OPS = "MIDNSHP=X"
REF_CONSUMING = set("MDN=X")
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def rec(ref_id=0, pos=0, mapq=60, flag=0, name=b"r", cigar=(("M", 10),), l_seq=10, next_ref_id=-1, next_pos=-1, tlen=0):
    return dict(ref_id=ref_id, pos=pos, mapq=mapq, flag=flag, name=bytes(name), cigar=list(cigar), l_seq=l_seq, next_ref_id=next_ref_id,
                next_pos=next_pos, tlen=tlen)


# ---- writer ---------------------------------------------------------------------------------------------------------
def encode_record(r):
    name = r["name"] + b"\0"
    cig = b"".join(struct.pack("<I", (n << 4) | CIGAR_OPS.index(op)) for op, n in r["cigar"])
    l_seq = r["l_seq"]
    body = struct.pack("<iiBBHHHiiii", r["ref_id"], r["pos"], len(name), r["mapq"], 4680, len(r["cigar"]), r["flag"], l_seq, r["next_ref_id"],
                       r["next_pos"], r["tlen"])
    body += name + cig + b"\x11" * ((l_seq + 1) // 2) + b"\x1e" * l_seq
    return struct.pack("<I", len(body)) + body


def encode_header(refs, text=""):
    t = text.encode()
    out = b"BAM\1" + struct.pack("<i", len(t)) + t + struct.pack("<i", len(refs))
    for name, length in refs:
        nm = name.encode() + b"\0"
        out += struct.pack("<i", len(nm)) + nm + struct.pack("<i", length)
    return out


def bgzf_block(data, level=6):
    assert len(data) <= 65536
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    if len(comp) + 26 > 65536:  # (incompressible: stored)
        co = zlib.compressobj(0, zlib.DEFLATED, -15)
        comp = co.compress(data) + co.flush()
    bsize = len(comp) + 25
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize) + comp +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def bgzf_bytes(stream, cuts=None, eof=True, block=0xFF00):
    """the BGZF file of `stream`: a block ends at every offset in `cuts` (a repeated offset gives an empty block) and after
    `block` bytes at the latest"""
    bounds = sorted(cuts or [])
    out, at = [], 0
    for c in bounds + [len(stream)]:
        c = min(max(c, at), len(stream))
        while c - at > block:
            out.append(bgzf_block(stream[at:at + block]))
            at += block
        if c > at or c in bounds:
            out.append(bgzf_block(stream[at:c]))
        at = c
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def bam_stream(refs, records, text=""):
    return encode_header(refs, text) + b"".join(encode_record(r) for r in records)


def write_bam(path, refs, records, cuts=None, eof=True, text="", block=0xFF00):
    data = bgzf_bytes(bam_stream(refs, records, text), cuts, eof, block)
    with open(path, "wb") as f:
        f.write(data)
    return data


# ---- reader ---------------------------------------------------------------------------------------------------------
def read_blocks(data):
    """[(coff, csize, isize, crc, uoff)], inflated stream"""
    blocks, out, at, uoff = [], [], 0, 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04", at
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        x, bsize = at + 12, None
        while x < at + 12 + xlen:
            si, slen = data[x:x + 2], struct.unpack_from("<H", data, x + 2)[0]
            if si == b"BC":
                bsize = struct.unpack_from("<H", data, x + 4)[0]
            x += 4 + slen
        csize = bsize + 1
        crc, isize = struct.unpack_from("<II", data, at + csize - 8)
        raw = zlib.decompress(data[at + 12 + xlen:at + csize - 8], -15)
        assert len(raw) == isize and (zlib.crc32(raw) & 0xFFFFFFFF) == crc
        blocks.append((at, csize, isize, crc, uoff))
        out.append(raw)
        uoff += isize
        at += csize
    return blocks, b"".join(out)


def parse_stream(s):
    """-> header text, [(name, length)], offset of the first record, record offsets, records"""
    assert s[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", s, 4)[0]
    text = s[8:8 + l_text].rstrip(b"\0").decode()
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", s, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", s, at)[0]
        refs.append((s[at + 4:at + 4 + l_name].rstrip(b"\0").decode(), struct.unpack_from("<i", s, at + 4 + l_name)[0]))
        at += 8 + l_name
    first, offs, recs = at, [], []
    while at < len(s):
        bs = struct.unpack_from("<I", s, at)[0]
        offs.append(at)
        ref_id, pos, l_name, mapq, _bin, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", s, at + 4)
        name = s[at + 36:at + 36 + l_name - 1]
        cig = [(CIGAR_OPS[v & 15], v >> 4) for v in struct.unpack_from("<%dI" % n_cig, s, at + 36 + l_name)]
        recs.append(dict(ref_id=ref_id, pos=pos, mapq=mapq, flag=flag, name=name, cigar=cig, l_seq=l_seq, next_ref_id=nref, next_pos=npos,
                         tlen=tlen))
        at += 4 + bs
    return text, refs, first, offs, recs


def read_bam(path):
    with open(path, "rb") as f:
        data = f.read()
    blocks, stream = read_blocks(data)
    text, refs, first, offs, recs = parse_stream(stream)
    return dict(blocks=blocks, stream=stream, text=text, refs=refs, first=first, offsets=offs, records=recs)


def ref_span(r):
    return sum(n for op, n in r["cigar"] if op in REF_CONSUMING)


def columns_ref(records):
    import numpy as np

    cols = {"ref_id": [r["ref_id"] for r in records], "start": [r["pos"] for r in records], "end": [r["pos"] + ref_span(r) for r in records],
            "flag": [r["flag"] for r in records], "mapq": [r["mapq"] for r in records], "l_seq": [r["l_seq"] for r in records],
            "tlen": [r["tlen"] for r in records]}
    return {k: np.asarray(v, dtype=np.int32).reshape(-1) for k, v in cols.items()}


# ---- bamqc.rs:68-245 ------------------------------------------------------------------------------------------------
MIN_MAPQ = 30


def is_mitochondrial(chrom):
    lower = chrom.lower()
    return lower == "chrm" or lower == "mt" or lower == "chrmt" or "rcrsd" in lower


def process_chromosome(records, c, chrom):
    """bamqc.rs:68-163 over the records whose refID is c"""
    res = dict(position_counts={}, total_reads=0, num_pairs=0, dup_count=0, mito_reads=0, is_paired=False)
    mine = [r for r in records if r["ref_id"] == c]
    if is_mitochondrial(chrom):
        for r in mine:
            if r["mapq"] != 255 and r["mapq"] < MIN_MAPQ:
                continue
            if not r["flag"] & 0x4:
                res["total_reads"] += 1
                res["mito_reads"] += 1
                if r["flag"] & 0x400:
                    res["dup_count"] += 1
        return res
    read1, read2 = {}, {}
    pc = res["position_counts"]
    for r in mine:
        if r["mapq"] != 255 and r["mapq"] < MIN_MAPQ:
            continue
        if r["flag"] & 0x4:
            continue
        res["total_reads"] += 1
        if r["flag"] & 0x400:
            res["dup_count"] += 1
        if r["pos"] == -1:
            continue
        pos = r["pos"] + 1
        if r["flag"] & 0x1:
            res["is_paired"] = True
            if r["name"] == b"*":
                continue
            if r["flag"] & 0x40:
                read1[r["name"]] = (pos, r["tlen"])
            elif r["flag"] & 0x80:
                read2[r["name"]] = (pos, r["tlen"])
        else:
            key = (pos, r["l_seq"], 0, 0)
            pc[key] = pc.get(key, 0) + 1
    if res["is_paired"]:
        joined = 0
        for qname, (pos1, tlen1) in read1.items():
            if qname in read2:
                pos2, tlen2 = read2[qname]
                key = (pos1, tlen1, pos2, tlen2)
                pc[key] = pc.get(key, 0) + 1
                joined += 1
        res["num_pairs"] = joined
    return res


def bam_qc_ref(refs, records):
    """bamqc.rs:247-319 -> dict of the nine fields"""
    total_reads = total_pairs = dup_count = mito_count = m_distinct = m1 = m2 = 0
    is_paired_data = False
    for c, (chrom, _) in enumerate(refs):
        cr = process_chromosome(records, c, chrom)
        total_reads += cr["total_reads"]
        total_pairs += cr["num_pairs"]
        dup_count += cr["dup_count"]
        mito_count += cr["mito_reads"]
        if cr["is_paired"]:
            is_paired_data = True
        m_distinct += len(cr["position_counts"])
        for count in cr["position_counts"].values():
            if count == 1:
                m1 += 1
            elif count == 2:
                m2 += 1
    effective_total = total_pairs if is_paired_data else total_reads - mito_count
    total_f = float(max(effective_total, 1))
    return dict(total_reads=effective_total, distinct=m_distinct, m1=m1, m2=m2, dups=dup_count, mito_reads=mito_count, nrf=m1 / total_f,
                pbc1=m1 / float(max(m_distinct, 1)), pbc2=m1 / float(max(m2, 1)))


def bam_qc_ref_file(path):
    b = read_bam(path)
    return bam_qc_ref(b["refs"], b["records"])
