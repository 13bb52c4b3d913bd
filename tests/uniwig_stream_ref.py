"""Plain-Python restatement of the streaming uniwig (gtars-uniwig/src/stream.rs), statement by statement: the line parser,
the deque-based UniwigStreamProcessor (process_record, emit_up_to, ensure_buffer_covers, finalize), WigWriter, the bedGraph
writer, read_chrom_sizes and uniwig_streaming.  Slow on purpose; the tests hold the device against it.

Integers: positions are the reference's i32, counts its u32.  A count past 2^32 - 1 wraps (the reference's release build).
"""
from __future__ import annotations

import zlib
from collections import deque
from typing import Dict, Iterable, List, Optional, Tuple

START, END, CORE = "start", "end", "core"
Record = Tuple[str, int, int]  # chrom, 1-based position, count

_INT_ERR_EMPTY = "cannot parse integer from empty string"
_INT_ERR_DIGIT = "invalid digit found in string"
_INT_ERR_POS = "number too large to fit in target type"
_INT_ERR_NEG = "number too small to fit in target type"


def parse_i32(text: str) -> int:
    """i32::from_str; ValueError carries the ParseIntError's text"""
    if text == "":
        raise ValueError(_INT_ERR_EMPTY)
    digits = text[1:] if text[0] in "+-" else text
    if digits == "" or any(c not in "0123456789" for c in digits):
        raise ValueError(_INT_ERR_DIGIT)
    v = int(digits)
    if text[0] == "-":
        v = -v
        if v < -(1 << 31):
            raise ValueError(_INT_ERR_NEG)
    elif v > (1 << 31) - 1:
        raise ValueError(_INT_ERR_POS)
    return v


# char::is_whitespace (the Unicode White_Space property)
_WS = ("\t\n\x0b\x0c\r \x85\xa0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009\u200a\u2028\u2029\u202f"
       "\u205f\u3000")


def _split_whitespace(text: str) -> List[str]:
    out, cur = [], ""
    for c in text:
        if c in _WS:
            if cur:
                out.append(cur)
            cur = ""
        else:
            cur += c
    if cur:
        out.append(cur)
    return out


def parse_bed_line(line: bytes) -> Optional[Tuple[str, int, int, int]]:
    """stream.rs:57-112 -> (chrom, start, end, score) or None for a skipped line; ValueError with the reference's message"""
    if len(line) == 0:
        return None
    if line[0] == ord("#"):
        return None
    try:
        line_str = line.decode("utf-8")
    except UnicodeDecodeError as e:
        raise ValueError(f"Invalid UTF-8: {e}")
    trimmed = line_str.strip(_WS)
    if trimmed == "":
        return None
    if trimmed.startswith("track") or trimmed.startswith("browser"):
        return None
    fields = _split_whitespace(trimmed)
    if len(fields) < 3:
        raise ValueError(f"BED line has fewer than 3 fields: '{trimmed}'")
    chrom = fields[0]
    try:
        start = parse_i32(fields[1])
    except ValueError as e:
        raise ValueError(f"Cannot parse start '{fields[1]}': {e}")
    try:
        end = parse_i32(fields[2])
    except ValueError as e:
        raise ValueError(f"Cannot parse end '{fields[2]}': {e}")
    if len(fields) >= 5:
        try:
            score = parse_i32(fields[4])
        except ValueError:
            score = 1
        score = max(score, 0)
    else:
        score = 1
    return chrom, start, end, score


class UniwigStreamProcessor:
    """stream.rs:124-382"""

    def __init__(self, smooth_size: int, step_size: int, count_type: str, chrom_sizes: Dict[str, int]):
        self.state: Optional[str] = None  # None: AwaitingFirstRecord, else InChromosome { name }
        self.count_buffer: deque = deque()
        self.buffer_start_pos = 0
        self.smooth_size = smooth_size
        self.step_size = step_size
        self.count_type = count_type
        self.chrom_sizes = chrom_sizes
        self.output_records: List[Record] = []
        self.max_gap = 0

    def set_max_gap(self, max_gap: int) -> None:
        self.max_gap = max_gap

    def process_line_bytes(self, line: bytes) -> None:
        rec = parse_bed_line(line)
        if rec is not None:
            self.process_record(*rec)

    def process_record(self, chrom: str, start: int, end: int, score: int) -> None:
        if self.count_type == START:
            center = start + 1
            window_start = max(center - self.smooth_size, 1)
            window_end = center + self.smooth_size
        elif self.count_type == END:
            center = end
            window_start = max(center - self.smooth_size, 1)
            window_end = center + self.smooth_size
        else:
            window_start = start + 1
            window_end = end - 1
            if window_end < window_start:
                return
        if self.state is None:
            self.state = chrom
            if self.max_gap < 0:
                self.buffer_start_pos = 1
                self.emit_up_to(window_start)
            else:
                self.buffer_start_pos = window_start
        elif self.state != chrom:
            self.finalize_current_chromosome()
            self.reset_counting_state()
            self.state = chrom
            if self.max_gap < 0:
                self.buffer_start_pos = 1
                self.emit_up_to(window_start)
            else:
                self.buffer_start_pos = window_start
        self.emit_up_to(window_start)
        self.ensure_buffer_covers(window_start, window_end)
        if score > 0:
            for pos in range(window_start, window_end + 1):
                idx = pos - self.buffer_start_pos
                if idx < 0:
                    continue  # (`as usize` of a negative i32 is far past the buffer's length)
                if idx < len(self.count_buffer):
                    self.count_buffer[idx] = (self.count_buffer[idx] + score) & 0xFFFFFFFF

    def _on_step(self, pos: int) -> bool:
        # Rust's % truncates; positions are >= 1 wherever this is asked
        return self.step_size <= 1 or (pos - 1) % self.step_size == 0

    def emit_up_to(self, up_to_pos: int) -> None:
        if self.state is None:
            return
        chrom_name = self.state
        while self.buffer_start_pos < up_to_pos and self.count_buffer:
            pos = self.buffer_start_pos
            count = self.count_buffer.popleft()
            if self._on_step(pos):
                self.output_records.append((chrom_name, pos, count))
            self.buffer_start_pos += 1
        if not self.count_buffer and self.buffer_start_pos < up_to_pos:
            gap_width = up_to_pos - self.buffer_start_pos
            should_fill = self.max_gap < 0 or gap_width <= self.max_gap
            if should_fill:
                while self.buffer_start_pos < up_to_pos:
                    if self._on_step(self.buffer_start_pos):
                        self.output_records.append((chrom_name, self.buffer_start_pos, 0))
                    self.buffer_start_pos += 1
            else:
                self.buffer_start_pos = up_to_pos

    def ensure_buffer_covers(self, start: int, end: int) -> None:
        if not self.count_buffer:
            self.buffer_start_pos = start
        buffer_end_pos = self.buffer_start_pos + len(self.count_buffer) - 1
        if end > buffer_end_pos:
            self.count_buffer.extend([0] * (end - buffer_end_pos))

    def finalize_current_chromosome(self) -> None:
        if self.state is None:
            return
        chrom_name = self.state
        while self.count_buffer:
            pos = self.buffer_start_pos
            count = self.count_buffer.popleft()
            if self._on_step(pos):
                self.output_records.append((chrom_name, pos, count))
            self.buffer_start_pos += 1
        if self.max_gap < 0 and chrom_name in self.chrom_sizes:
            chrom_size = self.chrom_sizes[chrom_name]
            as_i32 = chrom_size - (1 << 32) if chrom_size >= (1 << 31) else chrom_size
            end_pos = as_i32 + 1
            if end_pos >= (1 << 31):  # the release build wraps
                end_pos -= 1 << 32
            while self.buffer_start_pos < end_pos:
                if self._on_step(self.buffer_start_pos):
                    self.output_records.append((chrom_name, self.buffer_start_pos, 0))
                self.buffer_start_pos += 1

    def reset_counting_state(self) -> None:
        self.count_buffer.clear()
        self.buffer_start_pos = 0

    def drain_output(self) -> List[Record]:
        out, self.output_records = self.output_records, []
        return out

    def finish(self) -> List[Record]:
        self.finalize_current_chromosome()
        return self.output_records


class WigWriter:
    """stream.rs:389-438"""

    def __init__(self):
        self.current_chrom: Optional[str] = None
        self.last_pos: Optional[int] = None

    def write_records(self, out: List[bytes], records: Iterable[Record]) -> None:
        for chrom, position, count in records:
            if self.current_chrom is None:
                need_header = True
            elif self.current_chrom != chrom:
                need_header = True
            else:
                need_header = self.last_pos is None or position != self.last_pos + 1
            if need_header:
                out.append(f"fixedStep chrom={chrom} start={position} step=1\n".encode())
                self.current_chrom = chrom
            out.append(f"{count}\n".encode())
            self.last_pos = position


def write_records_as_wig(records: Iterable[Record]) -> bytes:
    out: List[bytes] = []
    WigWriter().write_records(out, records)
    return b"".join(out)


def write_records_as_bedgraph(records: Iterable[Record]) -> bytes:
    return b"".join(f"{c}\t{p - 1}\t{p}\t{k}\n".encode() for c, p, k in records)


def read_chrom_sizes(text: str) -> Dict[str, int]:
    """stream.rs:473-495"""
    sizes: Dict[str, int] = {}
    for line in text.split("\n"):
        if line.endswith("\r"):
            line = line[:-1]  # (BufRead::lines cuts "\r\n")
        trimmed = line.strip(_WS)
        if trimmed == "" or trimmed.startswith("#"):
            continue
        fields = trimmed.split("\t")
        if len(fields) < 2:
            raise ValueError(f"chrom.sizes line has fewer than 2 fields: '{trimmed}'")
        text_size = fields[1]
        digits = text_size[1:] if text_size[:1] == "+" else text_size
        if text_size == "":
            raise ValueError(f"Cannot parse size '{text_size}': {_INT_ERR_EMPTY}")
        if digits == "" or any(c not in "0123456789" for c in digits):
            raise ValueError(f"Cannot parse size '{text_size}': {_INT_ERR_DIGIT}")
        if int(digits) > 0xFFFFFFFF:
            raise ValueError(f"Cannot parse size '{text_size}': {_INT_ERR_POS}")
        sizes[fields[0]] = int(digits)
    return sizes


def gunzip_first_member(data: bytes) -> bytes:
    """flate2::bufread::GzDecoder: one member, the rest of the input is left alone"""
    d = zlib.decompressobj(16 + zlib.MAX_WBITS)
    try:
        out = d.decompress(data)
    except zlib.error as e:
        raise ValueError(f"corrupt gzip input: {e}")
    if not d.eof:
        raise ValueError("gzip input ends inside its first member")
    return out


def split_lines(data: bytes) -> List[bytes]:
    """read_line + trim_end_matches('\\n' | '\\r') of process_lines (stream.rs:516-539)"""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [ln.rstrip(b"\r\n") for ln in lines]


def run_processor(data: bytes, smooth_size: int, step_size: int, count_type: str, chrom_sizes: Dict[str, int], max_gap: int = 0
                  ) -> List[Record]:
    p = UniwigStreamProcessor(smooth_size, step_size, count_type, dict(chrom_sizes))
    p.set_max_gap(max_gap)
    for line in split_lines(data):
        p.process_line_bytes(line)
    return p.drain_output() + p.finish()


def run_rows(rows: Iterable[Tuple[str, int, int, int]], smooth_size: int, step_size: int, count_type: str,
             chrom_sizes: Dict[str, int], max_gap: int = 0) -> List[Record]:
    p = UniwigStreamProcessor(smooth_size, step_size, count_type, dict(chrom_sizes))
    p.set_max_gap(max_gap)
    for chrom, start, end, score in rows:
        p.process_record(chrom, int(start), int(end), int(score))
    return p.finish()


def uniwig_streaming(data: bytes, chrom_sizes: Dict[str, int], smooth_size: int, step_size: int, count_type: str,
                     output_format: str, max_gap: int) -> bytes:
    """stream.rs:548-596 -> the bytes written.  (The reference has written the lines in front of a bad one when it fails.)"""
    if len(data) >= 2 and data[0] == 0x1F and data[1] == 0x8B:
        data = gunzip_first_member(data)
    data.decode("utf-8")  # read_line into a String
    records = run_processor(data, smooth_size, step_size, count_type, chrom_sizes, max_gap)
    return write_records_as_wig(records) if output_format == "wig" else write_records_as_bedgraph(records)
