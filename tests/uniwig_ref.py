"""Plain-Python restatement of gtars-uniwig for BED input, statement by statement: the BED reader (reading.rs:17-101), the
two count sweeps (counting.rs:32-290), the start-position helpers and compress_counts (utils.rs:31-81), the four writers
and write_combined_files (writing.rs:13-214) and the BED branch of uniwig_main (lib.rs:50-581).  Test infrastructure
only: the product path never imports it.  Variable names follow the reference so the two can be read side by side.

Vectors of (position, score) pairs are lists of tuples here as there; i32 arithmetic is Python integers (nothing in the
tests comes near the i32 range).
"""
from __future__ import annotations

import gzip
import json
import os
import struct


# ---- reading.rs:17-101 -------------------------------------------------------------------------------------------------
def parse_bedlike_file(line):
    """gtars-core/src/utils.rs:88-106: split on TAB, fields 2 and 3 as i32 or -1"""
    fields = line.split("\t")

    def num(s):
        try:
            if s.strip() != s or not s.lstrip("+-").isdigit():
                return -1
            return int(s)
        except ValueError:
            return -1

    st = num(fields[1]) if len(fields) > 1 else -1
    en = num(fields[2]) if len(fields) > 2 else -1
    return fields[0], st, en


def create_chrom_vec_default_score(path):
    """-> [(chrom, starts, ends)], starts / ends lists of (position, 1) sorted independently; a chromosome is a run of
    consecutive equal names in file order"""
    default_score = 1
    opener = gzip.open if str(path).endswith(".gz") else open
    chromosome_vec = []
    chrom = ""
    name, starts, ends = "", [], []
    with opener(path, "rt") as fh:
        for line_string in fh.read().splitlines():
            parsed_chr, parsed_start, parsed_end = parse_bedlike_file(line_string)
            if chrom == "":
                name = parsed_chr.strip()
                chrom = parsed_chr.strip()
                starts.append((parsed_start + 1, default_score))
                ends.append((parsed_end, default_score))
                continue
            if parsed_chr.strip() != chrom:
                starts.sort()
                ends.sort()
                chromosome_vec.append((name, starts, ends))
                name = parsed_chr.strip()
                chrom = parsed_chr.strip()
                starts, ends = [], []
            starts.append((parsed_start + 1, default_score))
            ends.append((parsed_end, default_score))
    starts.sort()
    ends.sort()
    chromosome_vec.append((name, starts, ends))
    return chromosome_vec


def read_chromosome_sizes(path):
    """reading.rs:226-275, the .sizes branch"""
    sizes = {}
    with open(path) as fh:
        for line in fh.read().splitlines():
            it = line.split()
            sizes[it[0]] = int(it[1])
    return sizes


# ---- counting.rs:32-158 ------------------------------------------------------------------------------------------------
def start_end_counts(starts_vector, chrom_size, smoothsize, stepsize):
    v_coordinate_positions = []
    v_coord_counts = []
    coordinate_position = 1
    count = 0
    prev_coordinate_value = 0
    collected_end_sites = []
    collected_counts = []

    adjusted_start_site = list(starts_vector[0])
    original_position = adjusted_start_site[0]
    adjusted_start_site[0] = max(original_position - smoothsize, 1)

    current_score = adjusted_start_site[1]
    collected_counts.insert(0, current_score)
    count += current_score

    current_end_site = list(adjusted_start_site)
    current_end_site[0] = original_position + smoothsize + 1

    while coordinate_position < adjusted_start_site[0]:
        coordinate_position += stepsize

    for coord in starts_vector[1:]:
        coordinate_value = coord
        original_position = coordinate_value[0]
        adjusted_start_site = list(coordinate_value)
        adjusted_start_site[0] = max(original_position - smoothsize, 1)

        new_end_site = list(adjusted_start_site)
        new_end_site[0] = original_position + smoothsize + 1
        collected_end_sites.append(new_end_site)

        if adjusted_start_site[0] == prev_coordinate_value:
            current_score = adjusted_start_site[1]
            collected_counts.insert(0, current_score)
            count += current_score
            continue

        while coordinate_position < adjusted_start_site[0]:
            while current_end_site[0] == coordinate_position:
                most_recent_score = collected_counts.pop(0)
                count -= most_recent_score
                if count < 0:
                    count = 0
                if not collected_end_sites:
                    current_end_site[0] = 0
                else:
                    current_end_site = collected_end_sites.pop(0)
            if coordinate_position % stepsize == 0:
                v_coord_counts.append(count)
                v_coordinate_positions.append(coordinate_position)
            coordinate_position += 1

        current_score = adjusted_start_site[1]
        collected_counts.insert(0, current_score)
        count += current_score
        prev_coordinate_value = adjusted_start_site[0]

    while coordinate_position <= chrom_size:
        while current_end_site[0] == coordinate_position:
            most_recent_score = collected_counts.pop(0)
            count -= most_recent_score
            if count < 0:
                count = 0
            if not collected_end_sites:
                current_end_site[0] = 0
            else:
                current_end_site = collected_end_sites.pop(0)
        if coordinate_position % stepsize == 0:
            v_coord_counts.append(count)
            v_coordinate_positions.append(coordinate_position)
        coordinate_position += 1

    return v_coord_counts, v_coordinate_positions


# ---- counting.rs:167-290 -----------------------------------------------------------------------------------------------
def core_counts(starts_vector, ends_vector, chrom_size, stepsize):
    v_coordinate_positions = []
    v_coord_counts = []
    coordinate_position = 1
    count = 0
    prev_coordinate_value = 0
    collected_end_sites = []
    collected_counts = []

    current_start_site = list(starts_vector[0])
    current_end_site = list(ends_vector[0])

    if current_start_site[0] < 1:
        current_start_site[0] = 1

    current_score = current_start_site[1]
    collected_counts.insert(0, current_score)
    count += current_score

    while coordinate_position < current_start_site[0]:
        coordinate_position += stepsize

    for index, coord in enumerate(starts_vector):
        if index == 0:
            continue
        coordinate_value = coord
        current_start_site = list(coordinate_value)

        if current_start_site[0] < 1:
            current_start_site[0] = 1

        current_index = index
        collected_end_sites.append(list(ends_vector[current_index]))

        if current_start_site[0] == prev_coordinate_value:
            current_score = current_start_site[1]
            collected_counts.insert(0, current_score)
            count += current_score
            continue

        while coordinate_position < current_start_site[0]:
            while current_end_site[0] == coordinate_position:
                most_recent_score = collected_counts.pop(0)
                count -= most_recent_score
                if count < 0:
                    count = 0
                if not collected_end_sites:
                    current_end_site[0] = 0
                else:
                    current_end_site = collected_end_sites.pop(0)
            if coordinate_position % stepsize == 0:
                v_coord_counts.append(count)
                v_coordinate_positions.append(coordinate_position)
            coordinate_position += 1

        current_score = current_start_site[1]
        count += current_score
        collected_counts.insert(0, current_score)
        prev_coordinate_value = current_start_site[0]

    while coordinate_position <= chrom_size:
        while current_end_site[0] == coordinate_position:
            most_recent_score = collected_counts.pop(0)
            count -= most_recent_score
            if count < 0:
                count = 0
            if not collected_end_sites:
                current_end_site[0] = 0
            else:
                current_end_site = collected_end_sites.pop(0)
        if coordinate_position % stepsize == 0:
            v_coord_counts.append(count)
            v_coordinate_positions.append(coordinate_position)
        coordinate_position += 1

    return v_coord_counts, v_coordinate_positions


# ---- utils.rs:31-81 ----------------------------------------------------------------------------------------------------
def clamped_start_position(start, smoothsize, wig_shift):
    return max(1, start - smoothsize + wig_shift)


def clamped_start_position_zero_pos(start, smoothsize):
    return max(0, start - smoothsize)


def compress_counts(count_results, start_position):
    final_starts, final_ends, final_counts = [], [], []
    previous_count = count_results[0][0]
    previous_start = start_position
    current_start = previous_start
    current_end = start_position
    for u, _i in zip(count_results[0], count_results[1]):
        current_count = u
        current_end += 1
        if current_count != previous_count:
            final_starts.append(current_start)
            final_ends.append(current_end)
            final_counts.append(previous_count)
            current_start = current_end
            previous_count = current_count
        else:
            previous_count = current_count
    final_starts.append(current_start)
    final_ends.append(current_end)
    final_counts.append(previous_count)
    return final_starts, final_ends, final_counts


# ---- writing.rs:13-214 -------------------------------------------------------------------------------------------------
def _mkparent(filename):
    parent = os.path.dirname(filename)
    if parent:
        os.makedirs(parent, exist_ok=True)


def npy_bytes(counts):
    """what ndarray_npy::write_npy writes for Array1<u32>: a version 1.0 file, header dict padded with spaces to a
    multiple of 64 bytes and closed by a newline"""
    header = "{'descr': '<u4', 'fortran_order': False, 'shape': (%d,), }" % len(counts)
    pad = (64 - (10 + len(header) + 1) % 64) % 64
    header = header + " " * pad + "\n"
    return b"\x93NUMPY\x01\x00" + struct.pack("<H", len(header)) + header.encode("latin1") + struct.pack(
        "<%dI" % len(counts), *counts)


def write_to_npy_file(counts, filename, chromname, start_position, stepsize, metafilename):
    _mkparent(metafilename)
    with open(filename, "wb") as fh:
        fh.write(npy_bytes(counts))
    with open(metafilename, "a") as fh:
        fh.write("fixedStep chrom=" + chromname + " start=" + str(start_position) + " step=" + str(stepsize) + "\n")


def write_to_wig_file(counts, filename, chromname, start_position, stepsize, chrom_size):
    _mkparent(filename)
    with open(filename, "a") as fh:
        fh.write("fixedStep chrom=" + chromname + " start=" + str(start_position) + " step=" + str(stepsize))
        fh.write("\n")
        for count in counts[:chrom_size]:
            fh.write("%d\n" % count)


def write_to_wig_file_variable(counts, filename, chromname, start_position, stepsize, chrom_size):
    _mkparent(filename)
    with open(filename, "a") as fh:
        fh.write("variableStep chrom=%s" % chromname)
        fh.write("\n")
        for i, count in enumerate(counts[:chrom_size]):
            if count > 0:
                position = start_position + i * stepsize
                fh.write("%d\t%d\n" % (position, count))


def write_to_bed_graph_file(count_info, filename, chromname, _stepsize):
    _mkparent(filename)
    assert len(count_info[0]) == len(count_info[1]) == len(count_info[2])
    with open(filename, "a") as fh:
        for i in range(len(count_info[0])):
            fh.write("%s\t%d\t%d\t%d\n" % (chromname, count_info[0][i], count_info[1][i], count_info[2][i]))


def write_combined_files(location, output_type, bwfileheader, chromosomes):
    combined = "%s_%s.%s" % (bwfileheader, location, output_type)
    _mkparent(combined)
    with open(combined, "ab") as out:
        inputs = []
        for chrom in chromosomes:
            file_name = "%s%s_%s.%s" % (bwfileheader, chrom[0], location, output_type)
            if os.path.exists(file_name):
                inputs.append(file_name)
        for input_file in inputs:
            with open(input_file, "rb") as fh:
                out.write(fh.read())
            os.remove(input_file)


# ---- lib.rs:50-581, BED input --------------------------------------------------------------------------------------------
def get_final_chromosomes(filepath, chrom_sizes):
    """utils.rs:85-282 for one BED file without scores: chromosomes the sizes file lacks are dropped"""
    final = []
    for chromosome in create_chrom_vec_default_score(filepath):
        if len(chromosome[1]) != len(chromosome[2]):
            break
        if chromosome[0] not in chrom_sizes:
            continue
        final.append(chromosome)
    return final


def uniwig_main(vec_count_type, smoothsize, filepath, chromsizerefpath, bwfileheader, output_type, stepsize=1,
                wigstep="fixed"):
    chrom_sizes = read_chromosome_sizes(chromsizerefpath)
    final_chromosomes = get_final_chromosomes(filepath, chrom_sizes)
    if output_type in ("bedgraph", "bw", "bigwig"):
        output_type = "bedGraph"
    meta = {k: "%s%s.meta" % (bwfileheader, k) for k in ("start", "end", "core")}
    for chrom_name, starts, ends in final_chromosomes:
        primary_start = starts[0]
        primary_end = ends[0]
        current_chrom_size = chrom_sizes[chrom_name]
        for count_type in vec_count_type:
            if smoothsize == 0:  # lib.rs:135: nothing is counted or written per chromosome
                continue
            if count_type not in ("start", "end", "core"):
                continue
            file_name = "%s%s_%s.%s" % (bwfileheader, chrom_name, count_type, output_type)
            if count_type == "start":
                count_result = start_end_counts(starts, current_chrom_size, smoothsize, stepsize)
                wig_start = clamped_start_position(primary_start[0], smoothsize, 0)
                bg_start = clamped_start_position_zero_pos(primary_start[0], smoothsize)
                npy_start = clamped_start_position_zero_pos(primary_start[0], smoothsize)
            elif count_type == "end":
                count_result = start_end_counts(ends, current_chrom_size, smoothsize, stepsize)
                wig_start = clamped_start_position(primary_end[0], smoothsize, 0)
                bg_start = clamped_start_position(primary_end[0], smoothsize, 0)
                npy_start = clamped_start_position(primary_end[0], smoothsize, 0)
            else:
                count_result = core_counts(starts, ends, current_chrom_size, stepsize)
                wig_start = clamped_start_position(primary_start[0], 0, 0)
                bg_start = clamped_start_position_zero_pos(primary_start[0], 0)
                npy_start = clamped_start_position_zero_pos(primary_start[0], 0)
            if output_type == "wig":
                if wigstep == "variable":
                    write_to_wig_file_variable(count_result[0], file_name, chrom_name, wig_start, stepsize, current_chrom_size)
                else:
                    write_to_wig_file(count_result[0], file_name, chrom_name, wig_start, stepsize, current_chrom_size)
            elif output_type == "bedGraph":
                write_to_bed_graph_file(compress_counts(count_result, bg_start), file_name, chrom_name, stepsize)
            else:
                write_to_npy_file(count_result[0], file_name, chrom_name, npy_start, stepsize, meta[count_type])
    if output_type in ("wig", "bedGraph"):
        for location in vec_count_type:
            write_combined_files(location, output_type, bwfileheader, final_chromosomes)
    elif output_type == "npy":
        npy_meta_data_map = {}
        for chrom_name, _, _ in final_chromosomes:
            npy_meta_data_map[chrom_name] = {"stepsize": stepsize, "reported_chrom_size": chrom_sizes[chrom_name]}
        for location in vec_count_type:
            temp = "%s%s.meta" % (bwfileheader, location)
            if os.path.exists(temp):
                with open(temp) as fh:
                    for line in fh.read().splitlines():
                        parts = line.split()
                        if len(parts) >= 3:
                            chrom = parts[1].split("=")[1]
                            starting_position = int(parts[2].split("=")[1])
                            if chrom in npy_meta_data_map:
                                npy_meta_data_map[chrom][location] = starting_position
                os.remove(temp)
        # (serde_json::to_string_pretty of a HashMap: the key order is not defined there; compare the parsed value)
        with open("%snpy_meta.json" % bwfileheader, "w") as fh:
            fh.write(json.dumps(npy_meta_data_map, indent=2))


# ---- the closed form the device computes ------------------------------------------------------
def closed_form(opens, closes, chrom_size):
    """opens / closes: the window opens a_i and closes e_i (any order) -> (counts, first position)"""
    import numpy as np

    a = np.sort(np.asarray(opens, dtype=np.int64))
    e = np.sort(np.asarray(closes, dtype=np.int64))
    first = int(a[0])
    last = max(int(chrom_size), int(a[-1]) - 1)
    if last < first:
        return np.zeros(0, dtype=np.uint32), first
    pos = np.arange(first, last + 1, dtype=np.int64)
    c = np.searchsorted(a, pos, side="right") - np.searchsorted(e, pos, side="right")
    return c.astype(np.uint32), first


def closed_form_start_end(positions, chrom_size, smoothsize):
    import numpy as np

    p = np.asarray(positions, dtype=np.int64)
    return closed_form(np.maximum(1, p - smoothsize), p + smoothsize + 1, chrom_size)


def closed_form_core(starts, ends, chrom_size):
    import numpy as np

    return closed_form(np.maximum(1, np.asarray(starts, dtype=np.int64)), np.asarray(ends, dtype=np.int64), chrom_size)
