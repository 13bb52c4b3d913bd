"""A bit-by-bit restatement of the reference's sequence encoding (gtars-refget/src/digest/alphabet.rs:114-383,
digest/encoder.rs:99-130 and 175-203) in plain Python: the tables written out, one bit at a time, no shifts over words.
The tests of K22 compare the library and the kernels against it."""

BITS = (2, 3, 4, 5, 8, 8)  # by alphabet class: dna2bit, dna3bit, dnaio, protein, ASCII, Unknown
IUPAC = {"A": 1, "C": 2, "G": 4, "T": 8, "U": 8, "R": 5, "Y": 10, "S": 6, "W": 9, "K": 7, "M": 3, "B": 12, "D": 13, "H": 14, "V": 15, "N": 0}
PROTEIN = "ACDEFGHIKLMNPQRSTVWY*X-."
DECODE = ("TCAG", "ACGTNRYX", "NACMGRSKTWYDBHVV", PROTEIN + "X" * 8)


def upper(b: int) -> int:
    return b - 32 if 97 <= b <= 122 else b


def encode_table(cls: int):
    """the code of every byte value; both letter cases alike"""
    tab = []
    for b in range(256):
        ch = chr(upper(b))
        if cls == 0:
            tab.append("TCAG".index(ch) if ch in "TCAG" else 0)
        elif cls == 1:
            tab.append("ACGTNRY".index(ch) if ch in "ACGTNRY" else 7)
        elif cls == 2:
            tab.append(IUPAC.get(ch, 0))
        elif cls == 3:
            tab.append(PROTEIN.index(ch) if ch in PROTEIN else 0)
        else:
            tab.append(upper(b))
    return tab


def decode_table(cls: int):
    """the character of every code of the class's width"""
    if cls >= 4:
        return list(range(256))
    return [ord(c) for c in DECODE[cls]][:1 << BITS[cls]]


def encode(seq: bytes, cls: int) -> bytes:
    """MSB first: symbol i has bits [i b, i b + b) counted from the top bit of byte 0; the unused low bits stay zero"""
    bits, tab = BITS[cls], encode_table(cls)
    out = bytearray((len(seq) * bits + 7) // 8)
    at = 0
    for b in seq:
        code = tab[b]
        for j in range(bits - 1, -1, -1):
            out[at // 8] |= ((code >> j) & 1) << (7 - at % 8)
            at += 1
    return bytes(out)


def decode(window: bytes, byte_offset: int, start: int, end: int, cls: int) -> bytes:
    """symbols [start, end) of an encoding of which `window` holds bytes [byte_offset, byte_offset + len(window)); every bit
    outside the window is zero; end <= start is empty"""
    bits, tab = BITS[cls], decode_table(cls)
    out = bytearray()
    for i in range(start, end):
        code = 0
        for j in range(bits):
            pos = i * bits + j
            at = pos // 8 - byte_offset
            bit = (window[at] >> (7 - pos % 8)) & 1 if 0 <= at < len(window) else 0
            code = (code << 1) | bit
        out.append(tab[code])
    return bytes(out)


def byte_range(start: int, end: int, bits: int):
    return (start * bits) // 8, (end * bits + 7) // 8


def round_trip(seq: bytes, cls: int) -> bytes:
    """what a record reads as after encode and decode: upper-cased, bytes outside the table as its default, and for IUPAC
    the reference's non-inverse (D -> H, H -> V, U -> T)"""
    return decode(encode(seq, cls), 0, 0, len(seq), cls)
