/*
 * gtars_amd_host.h -- C ABI of the host ("string world") layer of
 * libgtars_amd.so: BED / BED.gz parsing, RegionSet, Universe + Tokenizer,
 * fragment files, .gtok, IGD databases from BED files.  It sits on top of the
 * integer engine in gtars_amd.h and mirrors the reference's Rust types
 * (cited per entry point, file:line relative to the reference checkout), so a
 * binding (pyo3-style, ctypes, cgo, extendr) can expose the same classes.
 *
 * Strings are UTF-8, NUL terminated.  `const char*` results are borrowed from
 * the handle they were asked of and stay valid until that handle is freed.
 * Same status / error conventions as gtars_amd.h.
 */
#ifndef GTARS_AMD_HOST_H
#define GTARS_AMD_HOST_H

#include "gtars_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------
 * RegionSet  (gtars-core/src/models/region_set.rs:40-45)
 * ---------------------------------------------------------------------- */
typedef struct gtars_regionset gtars_regionset_t;

/* RegionSet::try_from(&Path) (region_set.rs:52-186): BED or BED.gz (by
 * extension, utils.rs:115-126); header / comment handling (:112-135); rest =
 * columns 4+ joined by tabs; EmptyRegionSet -> GTARS_ERR_EMPTY; the result is
 * stably sorted by (chr, start) (:182, :502-505). */
gtars_status gtars_regionset_from_bed(const char *path, gtars_regionset_t **out);
/* From<Vec<Region>> (region_set.rs:212-220): in-memory, NOT sorted. rest may
 * be NULL (all None) and individual entries may be NULL. */
gtars_status gtars_regionset_from_arrays(const char *const *chrs, const uint32_t *starts,
                                         const uint32_t *ends, const char *const *rest,
                                         uint64_t n, gtars_regionset_t **out);
void gtars_regionset_free(gtars_regionset_t *rs);
uint64_t gtars_regionset_len(const gtars_regionset_t *rs);
const char *gtars_regionset_header(const gtars_regionset_t *rs); /* NULL if none */
/* dictionary-encoded columns (ids index gtars_regionset_chrom_name) */
uint32_t gtars_regionset_n_chrom(const gtars_regionset_t *rs);
const char *gtars_regionset_chrom_name(const gtars_regionset_t *rs, uint32_t id);
const uint32_t *gtars_regionset_chrom_ids(const gtars_regionset_t *rs);
const uint32_t *gtars_regionset_starts(const gtars_regionset_t *rs);
const uint32_t *gtars_regionset_ends(const gtars_regionset_t *rs);
const char *gtars_regionset_rest(const gtars_regionset_t *rs, uint64_t i); /* NULL if None */
/* generate_region_to_id_map (gtars-core/src/utils.rs:202-214): dense ids in first-seen order over the whole Region
 * (chr, start, end, rest): what gtars-scoring's ConsensusSet stores as interval payload (files.rs:60-83).
 * *out_ids: gtars_regionset_len ids (gtars_free); *out_n_ids (may be NULL): number of distinct regions */
gtars_status gtars_regionset_dense_ids(const gtars_regionset_t *rs, uint32_t **out_ids, uint32_t *out_n_ids);

/* IndexedRegionSet::new(other) then count / any / find_overlaps(self)
 * (gtars-overlaprs/src/indexed_region_set.rs:111-113, 234-263) -- the
 * semantics of python RegionSet.count_overlaps / any_overlaps / find_overlaps
 * (gtars-python/src/models/region_set.rs:445-478): `self` queries, `other` is
 * indexed on the GPU.  kind: GTARS_KIND_AILIST is the reference default. */
gtars_status gtars_regionset_count_overlaps(const gtars_regionset_t *self,
                                            const gtars_regionset_t *other, int kind,
                                            int has_min, int32_t min_overlap, uint32_t *counts);
gtars_status gtars_regionset_any_overlaps(const gtars_regionset_t *self,
                                          const gtars_regionset_t *other, int kind,
                                          int has_min, int32_t min_overlap, uint8_t *out);
gtars_status gtars_regionset_find_overlaps(const gtars_regionset_t *self,
                                           const gtars_regionset_t *other, int kind,
                                           int has_min, int32_t min_overlap, uint64_t *offsets,
                                           uint32_t **out_idx, uint64_t *out_n);

/* ------------------------------------------------------------------------
 * RegionSet set algebra (gtars-core/src/models/region_set.rs:675-1420, the
 * IntervalSetOps trait; gtars-python/src/models/region_set.rs:369-494), on
 * the current device.  Chromosome names order bytewise ("chr10" < "chr2").
 * Result sets have no rest and no header.  Widths and bp totals are the
 * reference's release-build u32 values: (u32)(end - start) summed modulo
 * 2^32, intersection = a_bp + b_bp - union_bp in wrapping u32.
 * ---------------------------------------------------------------------- */
/* reduce (:675-707): stable sort by (chr, start), merge while next.start <= current.end */
gtars_status gtars_regionset_reduce(const gtars_regionset_t *rs, gtars_regionset_t **out);
/* union (:731-733): reduce(concat(self, other)) */
gtars_status gtars_regionset_union(const gtars_regionset_t *self, const gtars_regionset_t *other,
                                   gtars_regionset_t **out);
/* IntervalSetOps::setdiff / intersect (:1229-1370): both sets reduced, one sweep per chromosome of self */
gtars_status gtars_regionset_setdiff(const gtars_regionset_t *self, const gtars_regionset_t *other,
                                     gtars_regionset_t **out);
gtars_status gtars_regionset_intersect(const gtars_regionset_t *self, const gtars_regionset_t *other,
                                       gtars_regionset_t **out);
/* jaccard / coverage / overlap_coefficient (:1383-1415), 0.0 on a zero denominator */
gtars_status gtars_regionset_jaccard(const gtars_regionset_t *self, const gtars_regionset_t *other, double *out);
gtars_status gtars_regionset_coverage(const gtars_regionset_t *self, const gtars_regionset_t *other, double *out);
gtars_status gtars_regionset_overlap_coefficient(const gtars_regionset_t *self, const gtars_regionset_t *other,
                                                 double *out);
/* closest (:1132-1225): (self_idx, other_idx, distance) in self order; regions of self on a chromosome
 * other lacks are skipped; nothing when other is empty.  Where several regions of other share the
 * query's start, the walk starts at the FIRST of them (the reference's binary_search_by_key leaves
 * that index unspecified).  The three arrays: gtars_free each (*out_n entries). */
gtars_status gtars_regionset_closest(const gtars_regionset_t *self, const gtars_regionset_t *other,
                                     uint64_t **out_self_idx, uint64_t **out_other_idx, int64_t **out_dist,
                                     uint64_t *out_n);
/* cluster (:1093-1129): ids[gtars_regionset_len(rs)] in input order, counted up from 0 in (chr, start, end)
 * order; a new cluster on a chromosome change or where start > cluster_end.saturating_add(max_gap) */
gtars_status gtars_regionset_cluster(const gtars_regionset_t *rs, uint32_t max_gap, uint32_t *ids);
/* RegionSetList::pairwise_jaccard (gtars-genomicdist/src/region_set_list_ops.rs:20-45): out[i * n + j] =
 * reduce(S_i).jaccard(reduce(S_j)), 1.0 on the diagonal; every pair in one device pass */
gtars_status gtars_regionset_pairwise_jaccard(const gtars_regionset_t *const *sets, uint64_t n, double *out);
/* RegionSetListOps (region_set_list_ops.rs:103-181): the folds over a list of n sets.  "None" is GTARS_OK with *out == NULL.
 * Results of a device fold are plain sets in bytewise chromosome order; where the reference returns a clone the result is
 * an unreduced copy of that set, rest included, made on the host.
 * union_all: NULL when n == 0; the copy of the set when n == 1; else reduce(concat of all sets).
 * intersect_all: NULL when n == 0; the copy when n == 1; else the left fold of intersect (each step reduces both
 * operands): the stretches of positive length that every set's own reduce covers.
 * union_except: NULL when n < 2 or skip >= n; the copy of the other set when n == 2; else reduce(concat of every set but
 * skip).
 * bulk_union_except: both NULL when n < 2; else *out_union = union_all and (*out_except)[i] = union_except(i), from one
 * upload, one sort and one scan.  *out_except: n handles, each released with gtars_regionset_free, then the array with
 * gtars_free. */
gtars_status gtars_regionset_list_union_all(const gtars_regionset_t *const *sets, uint64_t n, gtars_regionset_t **out);
gtars_status gtars_regionset_list_intersect_all(const gtars_regionset_t *const *sets, uint64_t n, gtars_regionset_t **out);
gtars_status gtars_regionset_list_union_except(const gtars_regionset_t *const *sets, uint64_t n, uint64_t skip,
                                               gtars_regionset_t **out);
gtars_status gtars_regionset_list_bulk_union_except(const gtars_regionset_t *const *sets, uint64_t n,
                                                    gtars_regionset_t **out_union, gtars_regionset_t ***out_except);

/* ------------------------------------------------------------------------
 * K25: what names a set and writes it back out (gtars-core/src/models/region_set.rs:240-330, 502-505,
 * region_set_list.rs:85-98; csrc/bed_text_core.h states the text once for the host paths and the kernels).  Rows are in
 * the handle's order; nothing but the sort entry sorts.
 * identifier: the bed digest -- md5 of "c,s,e", c / s / e = md5 of the chromosome names / decimal starts / decimal
 * ends joined by ','.  file_digest: md5 of the lines chr \t start \t end [\t rest] \n.  out33: 32 lower-case hex
 * characters and a NUL.  The single-set entries run on the host threads.
 * bed_text: those lines as one malloc'ed block (*out, gtars_free; *len bytes and a NUL), formatted on the host threads
 * (on_host) or on the device.  write_bed: the lines to `path` (parent directories are created, an existing file is
 * replaced), as they are or (gz) as one gzip member at the best compression level; formatted on the device from
 * GTARS_BED_TEXT_DEVICE_ROWS rows up (unset: on the host threads whatever the size).
 * sort: stable, in place, by (chr bytewise, start) -- the order the file loader produces; rest moves with its rows.
 * list_digests: out[32 * i ..] = the identifier (what = GTARS_BED_IDENTIFIER) or file digest (GTARS_BED_FILE_DIGEST) of
 * set i, not terminated; list_identifier: the member identifiers sorted as strings, concatenated, hashed.  Both run on the
 * device -- every stream of every set one lane of k_bed_md5 -- or (on_host) on `threads` host threads (0: all). */
gtars_status gtars_regionset_identifier(const gtars_regionset_t *rs, char *out33);
gtars_status gtars_regionset_file_digest(const gtars_regionset_t *rs, char *out33);
gtars_status gtars_regionset_bed_text(const gtars_regionset_t *rs, int on_host, char **out, uint64_t *len);
gtars_status gtars_regionset_write_bed(const gtars_regionset_t *rs, const char *path, int gz);
gtars_status gtars_regionset_sort(gtars_regionset_t *rs);
gtars_status gtars_regionset_list_digests(const gtars_regionset_t *const *sets, uint64_t n, int what, int on_host,
                                          uint32_t threads, char *out);
gtars_status gtars_regionset_list_identifier(const gtars_regionset_t *const *sets, uint64_t n, int on_host,
                                             uint32_t threads, char *out33);

/* ------------------------------------------------------------------------
 * Structural operations and region-set statistics (gtars-core region_set.rs,
 * gtars-genomicdist/src/{consensus,statistics}.rs; gtars-python/src/models/
 * region_set.rs:288-531, genomic_distributions/tools.rs:157-190), on the
 * current device.  chrom_sizes are parallel arrays names[n_sizes] /
 * sizes[n_sizes]; a later entry of a name replaces an earlier one.  Arrays
 * returned through pointers: gtars_free each.
 * ---------------------------------------------------------------------- */
/* disjoin (region_set.rs:1051-1090): the pieces between consecutive boundaries (every start and end) of a chromosome that
 * some region with start <= piece.start and piece.end <= end covers (inverted and zero-width regions add boundaries, never
 * coverage); sorted by (chr, start).  Up to 2n boundaries: more than the device set operations' limit is an error. */
gtars_status gtars_regionset_disjoin(const gtars_regionset_t *rs, gtars_regionset_t **out);
/* gaps (region_set.rs:786-878): leading, inter-run and trailing gaps of reduce(rs), clipped to the chromosome size, and
 * [0, size) for a sized chromosome without regions; nothing for size 0 or unsized chromosomes.  Ordered by
 * chrom_karyotype_key (gtars-core/src/utils.rs:359-370), start, then name bytewise (the reference leaves names that share
 * a key in hash-map order). */
gtars_status gtars_regionset_gaps(const gtars_regionset_t *rs, const char *const *names, const uint32_t *sizes,
                                  uint64_t n_sizes, gtars_regionset_t **out);
/* consensus (consensus.rs:29-68): *out_union = reduce(concat(sets)); (*out_count)[i] = the number of sets with a region
 * that AIList any_overlaps reports for union region i (start < u.end && u.start < end) */
gtars_status gtars_regionset_consensus(const gtars_regionset_t *const *sets, uint64_t n, gtars_regionset_t **out_union,
                                       uint32_t **out_count);
/* calc_neighbor_distances (statistics.rs:258-285): chromosomes in order of first appearance (region_set.rs:399-407),
 * regions sorted by (start, end), every next.start - prev.end > 0 as i64; chromosomes with < 2 regions skipped */
gtars_status gtars_regionset_neighbor_distances(const gtars_regionset_t *rs, int64_t **out, uint64_t *out_n);
/* calc_nearest_neighbors (statistics.rs:287-316): the same walk, one value per region: min of the gaps to its left and
 * right neighbours, each clamped at 0 */
gtars_status gtars_regionset_nearest_neighbors(const gtars_regionset_t *rs, uint32_t **out, uint64_t *out_n);
/* distribution (statistics.rs:143-256, region_set.rs:322-349): regions counted per bin of their midpoint
 * start + (u32)(end - start) / 2.  has_sizes == 0: bin_size = max(max_end / n_bins, 1) from get_max_end_per_chr
 * (region_set.rs:584-606: the last contiguous run of a chromosome), bins end at min(start + bin_size, that end).
 * has_sizes: regions on unsized chromosomes or with midpoint >= size skipped, rid clamped to n_bins - 1, the last bin
 * ends at the size, n_bins == 0 gives nothing.  *out_rows: *out_n rows of 5 u32 (chromosome id of rs, start, end, n,
 * rid), sorted by (chr, start). */
gtars_status gtars_regionset_distribution(const gtars_regionset_t *rs, uint32_t n_bins, int has_sizes,
                                          const char *const *names, const uint32_t *sizes, uint64_t n_sizes,
                                          uint32_t **out_rows, uint64_t *out_n);
/* chromosome_statistics (statistics.rs:88-141): one entry per chromosome of rs, names bytewise.  *out_rows: rows of 6
 * u32 (chromosome id of rs, number of regions, min start, max end, min width, max width); *out_f64: rows of 2 (mean
 * width = u64 sum / count, median width; an even count adds the two middle widths in wrapping u32 first). */
gtars_status gtars_regionset_chromosome_statistics(const gtars_regionset_t *rs, uint32_t **out_rows, double **out_f64,
                                                   uint64_t *out_n);

/* ------------------------------------------------------------------------
 * Gene models and TSS / feature distances (gtars-genomicdist/src/
 * {models.rs:516-690, partitions.rs:123-340, stranded_region_set.rs:84-135};
 * gtars-python/src/models/{tss_index,gene_model,gda}.rs).  Strands are
 * coded 0 = '+', 1 = '-', 2 = unstranded (the reference's strand_ord).
 * ---------------------------------------------------------------------- */
/* GeneModel::from_gtf's reader (partitions.rs:123-250): plain text, or gzip (several members) when the path ends in ".gz".
 * Every line must be UTF-8; lines starting with '#' and rows of fewer than 9 TAB-separated fields are skipped; only the
 * feature types gene, exon, three_prime_utr, five_prime_utr, UTR and CDS are kept, and with filter_protein_coding only rows
 * whose 9th field contains `gene_biotype "protein_coding"` or `gene_type "protein_coding"`; convert_ensembl_ucsc prefixes
 * "chr" to names without it; start = (u32 parse of field 4).saturating_sub(1), end = u32 parse of field 5 (GTARS_ERR_PARSE
 * "Parsing GTF start: ..." / "Parsing GTF end: ..."); strand from the first character of field 7.  Host only.
 * *out_rows: the kept rows in file order (no rest); *out_strand and *out_feature (gtars_free each): one code per row,
 * features 0 gene, 1 exon, 2 three_prime_utr, 3 five_prime_utr, 4 UTR, 5 CDS. */
gtars_status gtars_gtf_read(const char *path, int filter_protein_coding, int convert_ensembl_ucsc, gtars_regionset_t **out_rows,
                            uint8_t **out_strand, uint8_t **out_feature);
/* StrandedRegionSet::reduce (stranded_region_set.rs:84-135) of the rows i of rs with keep[i] != 0 (keep NULL: all), on the
 * current device: stable sort by (chr bytewise, strand, start), merge while same chr and strand and start <= current end.
 * *out (sorted that way, no rest) and *out_strand (gtars_free) */
gtars_status gtars_regionset_stranded_reduce(const gtars_regionset_t *rs, const uint8_t *strand, const uint8_t *keep,
                                             gtars_regionset_t **out, uint8_t **out_strand);

/* StrandedRegionSet::setdiff (stranded_region_set.rs:138-217), on the current device: both sides stranded-reduced, then per
 * (chr, strand) group of a the sweep of gtars_regionset_setdiff, so a row is only ever cut by rows of its own strand code.
 * *out: a's reduced order, no rest; *out_strand (gtars_free) */
gtars_status gtars_regionset_stranded_setdiff(const gtars_regionset_t *a, const uint8_t *a_strand, const gtars_regionset_t *b,
                                              const uint8_t *b_strand, gtars_regionset_t **out, uint8_t **out_strand);
/* The UTR rows of GeneModel::from_gtf before their reduce (partitions.rs:144-328), read and filtered as gtars_gtf_read does.
 * Host only.  *out_kind: 0 three-prime, 1 five-prime.
 *   - three_prime_utr / five_prime_utr rows as they are, strand from field 7 ('.' when empty), in file order; then
 *   - every UTR row whose 9th field names a transcript (the text between the first `transcript_id "` and the next '"')
 *     that has a CDS row: five-prime when mid(UTR) < mid(CDS bounds) on '+', when mid(UTR) > mid(CDS bounds) on any other
 *     strand character, else three-prime; mid = (start + end) / 2 in u64, the CDS bounds are the smallest start and the
 *     largest end of the transcript's CDS rows; the strand character is field 7's first, '+' when empty;
 *   - only when neither gave a row: per exon row of a transcript with a CDS, [start, min(end, cds start)) when start <
 *     cds start (three-prime on '-', else five-prime) and [max(start, cds end), end) when end > cds end (five-prime on '-',
 *     else three-prime), in file order.  The reference emits these in hash-map order; every consumer reduces them. */
gtars_status gtars_gtf_read_utrs(const char *path, int filter_protein_coding, int convert_ensembl_ucsc, gtars_regionset_t **out_rows,
                                 uint8_t **out_strand, uint8_t **out_kind);

typedef struct gtars_tss_index gtars_tss_index_t;
/* TssIndex::try_from(RegionSet) (models.rs:525-549): a snapshot of rs; host only -- the device index (midpoints
 * start + (u32)(end - start) / 2 sorted per chromosome, duplicates kept) is built at the first distance call, on the
 * device current then, which the handle keeps (scope-or-refuse: later calls run there) */
gtars_status gtars_tss_index_from_regionset(const gtars_regionset_t *rs, gtars_tss_index_t **out);
void gtars_tss_index_free(gtars_tss_index_t *ix);
uint64_t gtars_tss_index_len(const gtars_tss_index_t *ix); /* regions the index was built from */
int gtars_tss_index_device(const gtars_tss_index_t *ix);   /* -1 until the first distance call */
/* calc_tss_distances and calc_feature_distances (models.rs:588-690) of query, in one device pass.  Results come by
 * chromosome in order of first appearance in query (iter_chroms), set order within one.  out_abs[len(query)]: distance
 * to the nearest midpoint, 0 on an exact hit, UINT32_MAX on a chromosome the index lacks; out_signed[len(query)]:
 * nearest midpoint - query midpoint, the left neighbour on a tie, INT64_MAX on a chromosome the index lacks. */
gtars_status gtars_tss_index_distances(gtars_tss_index_t *ix, const gtars_regionset_t *query, uint32_t *out_abs,
                                       int64_t *out_signed);

/* ------------------------------------------------------------------------
 * Genomic partitions  (gtars-genomicdist/src/partitions.rs:363-784; csrc/partitions.cpp, csrc/partitions.hip: K14)
 *
 * A partition list is an ordered list of named region sets (at most 255); the order is the priority.  The handle keeps
 * a snapshot of the rows on one chromosome dictionary (names in order of first appearance over the sets).  Its device
 * index is built at the first counting call, on the device current then, which the handle keeps: the host call runs
 * there whatever the caller's current device is, the device-pointer call refuses another one.  Empty sets are legal.
 * ---------------------------------------------------------------------- */
typedef struct gtars_partition_list gtars_partition_list_t;
gtars_status gtars_partition_list_from_sets(const char *const *names, const gtars_regionset_t *const *sets, uint32_t n,
                                            gtars_partition_list_t **out);
void gtars_partition_list_free(gtars_partition_list_t *pl);
uint32_t gtars_partition_list_len(const gtars_partition_list_t *pl);
const char *gtars_partition_list_name(const gtars_partition_list_t *pl, uint32_t i); /* NULL: out of range */
uint32_t gtars_partition_list_n_chrom(const gtars_partition_list_t *pl);
const char *gtars_partition_list_chrom_name(const gtars_partition_list_t *pl, uint32_t id);
/* *out: a new region set with the rows of partition i in their order (no rest) */
gtars_status gtars_partition_list_set(const gtars_partition_list_t *pl, uint32_t i, gtars_regionset_t **out);
/* out[len]: per partition the u64 sum of (u32)(end - start), what calc_expected_partitions calls its size */
gtars_status gtars_partition_list_sizes(const gtars_partition_list_t *pl, uint64_t *out);
int gtars_partition_list_device(const gtars_partition_list_t *pl); /* -1 until the first counting call */
/* calc_partitions (partitions.rs:493-592).  A row hits a query when row.start < q.end && row.end > q.start on the same
 * chromosome name.  counts[len + 1], the last entry is "intergenic".
 *   bp_proportion == 0: counts[p] = queries whose first hit partition in list order is p, counts[len] = queries
 *       without a hit, *total = (u32)len(query); assignments (may be NULL): per query that bucket, in query order
 *   bp_proportion != 0: counts[p] = sum over queries and the rows of p they hit of min(q.end, row.end) - max(q.start,
 *       row.start) where positive, once per row hit; *total = sum of (u32)(q.end - q.start); both wrap in u32 as the
 *       reference's release build does, and so does the sum of the counts that counts[len] = total.saturating_sub(sum)
 *       takes.  assignments must be NULL.
 * An empty query gives zero counts and total 0.
 * gtars_partitions_count_device: the queries are n device rows, d_chrom ids of the list's dictionary (any other value:
 * no hit), queued on `stream` (a hipStream_t) of the current device, which is drained before the call returns;
 * d_assignments (may be NULL) is a device pointer to n bytes. */
gtars_status gtars_partitions_count(gtars_partition_list_t *pl, const gtars_regionset_t *query, int bp_proportion,
                                    uint32_t *counts, uint32_t *total, uint8_t *assignments);
gtars_status gtars_partitions_count_device(gtars_partition_list_t *pl, const uint32_t *d_chrom, const uint32_t *d_start,
                                           const uint32_t *d_end, uint64_t n, int bp_proportion, void *stream,
                                           uint32_t *counts, uint32_t *total, uint8_t *d_assignments);
/* The rows of calc_expected_partitions (partitions.rs:598-784) from observed[n_partitions + 1] (the last: intergenic),
 * the partitions' sizes and the genome size, host f64 arithmetic.  The intergenic size is genome_size.saturating_sub(sum
 * of sizes); expected = (size / genome_size) * total; log10_oe = -inf when observed == 0, else +inf when expected == 0,
 * else log10(observed / expected); pvalue = 1 - P(0.5, chi / 2) with chi = (O - E)^2 / E + ((T - O) - (T - E))^2 / (T - E),
 * 1.0 when T == 0, E == 0 or T - E == 0.  P is the reference's own regularized lower incomplete gamma: the series
 * below a + 1 and one minus Lentz's continued fraction (clamped to [0, 1]) from there, both at most 199 terms with
 * tolerance 1e-14 and floor 1e-30, over its Lanczos (g = 7, n = 9) ln_gamma.  Each output has n_partitions + 1 entries. */
gtars_status gtars_partition_expected(const uint32_t *observed, const uint64_t *partition_bp, uint32_t n_partitions,
                                      uint32_t total, uint64_t genome_size, double *expected, double *log10_oe,
                                      double *pvalue);

/* ------------------------------------------------------------------------
 * Coverage tracks  (gtars-uniwig, BED input: counting.rs:32-290, utils.rs:31-81, writing.rs:113-214)
 *
 * One chromosome per call.  A track is given by columns of n u32 (any order, each is sorted on the device):
 *   GTARS_UNIWIG_START / _END (start_end_counts): opens = start + 1 (resp. end) of every row, closes NULL; a position
 *       p opens a window at max(1, p - smoothsize) and closes it at p + smoothsize + 1
 *   GTARS_UNIWIG_CORE (core_counts): opens = start + 1, closes = end of every row; smoothsize is ignored
 * With a the sorted opens and e the sorted closes, entry k of the track is the count at position first + k:
 *   #{a <= pos} - #{e <= pos},  first = a_0,  last = max(chrom_size, a_{n-1} - 1)   (n == 0: an empty track)
 * which is what the reference's sweeps give for unit scores and step 1.  Outside that domain they give something
 * else, so a core-track row with closes[i] < opens[i] (a zero-length or inverted row) is GTARS_ERR_INVALID_ARG, as is
 * anything that does not fit the reference's i32.
 * ---------------------------------------------------------------------- */
#define GTARS_UNIWIG_START 0
#define GTARS_UNIWIG_END 1
#define GTARS_UNIWIG_CORE 2
/* the whole track: *first, *counts (gtars_free) and *n_counts.  The device holds at most max_device_bytes of counts at a
 * time (0: the library's default, 1 GiB); a longer track is produced in position windows. */
gtars_status gtars_uniwig_counts(const uint32_t *opens, const uint32_t *closes, uint64_t n, uint32_t chrom_size,
                                 uint32_t smoothsize, int kind, uint64_t max_device_bytes, uint64_t *first, uint32_t **counts,
                                 uint64_t *n_counts);
/* first and length of that track without computing it (host only; same argument checks) */
gtars_status gtars_uniwig_extent(const uint32_t *opens, const uint32_t *closes, uint64_t n, uint32_t chrom_size,
                                 uint32_t smoothsize, int kind, uint64_t *first, uint64_t *n_counts);
/* positions window_first .. window_first + window_len - 1 of the track into d_counts (device memory, 16-byte aligned),
 * queued on `stream` (a hipStream_t); nothing is synchronised.  d_opens / d_closes: device columns that ASCEND. */
gtars_status gtars_uniwig_counts_device(const uint32_t *d_opens, const uint32_t *d_closes, uint64_t n, uint32_t smoothsize,
                                        int kind, uint64_t window_first, uint64_t window_len, uint32_t *d_counts, void *stream);
/* compress_counts (utils.rs:40-81) of the track: runs (start, end, count) that begin at start_position and advance by
 * one per ENTRY, the closing run always emitted; three columns (gtars_free each) of *n_runs.  Only the runs leave the
 * device.  GTARS_ERR_EMPTY for a track without entries (the reference reads entry 0). */
gtars_status gtars_uniwig_runs(const uint32_t *opens, const uint32_t *closes, uint64_t n, uint32_t chrom_size,
                               uint32_t smoothsize, int kind, uint32_t start_position, uint32_t **run_start,
                               uint32_t **run_end, uint32_t **run_count, uint64_t *n_runs);
/* the non-zero entries among the first chrom_size ENTRIES of the track as (start_position + k, count)
 * (write_to_wig_file_variable, writing.rs:149-179): two columns (gtars_free each) of *n_out */
gtars_status gtars_uniwig_nonzero(const uint32_t *opens, const uint32_t *closes, uint64_t n, uint32_t chrom_size,
                                  uint32_t smoothsize, int kind, uint32_t start_position, uint32_t **position,
                                  uint32_t **count, uint64_t *n_out);
/* the writers' lines (writing.rs:141-144, 172-177, 205-212) as one malloc'ed text (gtars_free), *out_len bytes:
 * "count\n" per entry; "a\tb\n" per pair; "chrom\tstart\tend\tcount\n" per run */
gtars_status gtars_uniwig_format_counts(const uint32_t *counts, uint64_t n, char **out_text, uint64_t *out_len);
gtars_status gtars_uniwig_format_pairs(const uint32_t *a, const uint32_t *b, uint64_t n, char **out_text, uint64_t *out_len);
gtars_status gtars_uniwig_format_bedgraph(const char *chrom, const uint32_t *run_start, const uint32_t *run_end,
                                          const uint32_t *run_count, uint64_t n, char **out_text, uint64_t *out_len);

/* ------------------------------------------------------------------------
 * Streaming uniwig  (K24; gtars-uniwig/src/stream.rs: scored, sparse, gap-filled, any step)
 *
 * Rows are (chromosome id, start, end, score) in FILE ORDER; no order is required.  Per row a window [ws, we], 1-based
 * and inclusive: START c = start + 1, ws = max(1, c - m), we = c + m; END c = end, the same; CORE ws = start + 1,
 * we = end - 1, and a CORE row with we < ws is dropped before anything else.  A run is a maximal run of consecutive equal
 * chromosome ids.  Inside a run, with M the inclusive prefix maximum of ws and B the exclusive prefix maximum of we, row
 * i adds its score to [M_i, we_i]; it opens a segment when it is the run's first row, or when M_i > B_i + 1 and the gap
 * M_i - B_i - 1 is not filled (filled: max_gap < 0, or gap <= max_gap).  A segment spans its head's M to the largest we
 * of its rows; with max_gap < 0 a run's one segment starts at 1 and reaches at least sizes_by_cid[id] (0: no size).
 * The counts are the positions of the segments one after the other ("compacted" coordinates), each the sum of the
 * scores of the rows that cover it, modulo 2^32.  start, end, end + m + 1 and start + m + 1 must fit an i32 and a score
 * must be below 2^31: otherwise GTARS_ERR_INVALID_ARG names the first such row.
 * ---------------------------------------------------------------------- */
typedef struct gtars_uniwig_rows gtars_uniwig_rows;
typedef struct gtars_uniwig_plan gtars_uniwig_plan;
/* parse_bed_line and the line loop of stream.rs over a file (path) or, with path NULL, over data[0, n): plain text, or
 * gzip when it starts with 1f 8b (only the first member is decoded).  Lines are trimmed and split on any white space;
 * empty lines, lines whose first byte is '#' and lines that start with "track" or "browser" are skipped; the score is
 * column 5 as an i32, 1 when it is absent or no i32, 0 when negative.  A bad line is GTARS_ERR_PARSE with the
 * reference's message, and no row is returned. */
gtars_status gtars_uniwig_stream_parse(const char *path, const void *data, uint64_t n, gtars_uniwig_rows **out);
void gtars_uniwig_rows_free(gtars_uniwig_rows *rows);
uint64_t gtars_uniwig_rows_len(const gtars_uniwig_rows *rows);
uint32_t gtars_uniwig_rows_n_chrom(const gtars_uniwig_rows *rows);
const char *gtars_uniwig_rows_chrom_name(const gtars_uniwig_rows *rows, uint32_t i); /* first-seen order */
/* the columns, owned by the handle: chromosome id, start and end as parsed (i32, may be negative), score */
gtars_status gtars_uniwig_rows_columns(const gtars_uniwig_rows *rows, const uint32_t **cid, const int32_t **start,
                                       const int32_t **end, const uint32_t **score);
/* host columns in; out: the segments that hold positions (chromosome id, first position, length at step 1; gtars_free
 * each) and the counts of the positions with (pos - 1) % step == 0, segment after segment (gtars_free).  The device holds
 * at most max_device_bytes of counts at a time (0: the library's default, 1 GiB). */
gtars_status gtars_uniwig_stream(const uint32_t *cid, const uint32_t *start, const uint32_t *end, const uint32_t *score, uint64_t n,
                                 const uint32_t *sizes_by_cid, uint32_t n_chrom, uint32_t smoothsize, uint32_t step, int kind,
                                 int64_t max_gap, uint64_t max_device_bytes, uint32_t **seg_cid, uint32_t **seg_first,
                                 uint32_t **seg_len, uint64_t *n_seg, uint32_t **counts, uint64_t *n_counts);
/* the plan of device-resident columns (sizes_by_cid is host memory): the segment table and, on the device, the event
 * columns that gtars_uniwig_stream_device reads.  The table has n_seg entries (seg_off: n_seg + 1, the last one the
 * compacted length) and keeps segments of length 0; a NULL column is skipped. */
gtars_status gtars_uniwig_stream_plan_device(const uint32_t *d_cid, const uint32_t *d_start, const uint32_t *d_end,
                                             const uint32_t *d_score, uint64_t n, const uint32_t *sizes_by_cid, uint32_t n_chrom,
                                             uint32_t smoothsize, int kind, int64_t max_gap, gtars_uniwig_plan **plan);
void gtars_uniwig_plan_free(gtars_uniwig_plan *plan);
uint64_t gtars_uniwig_plan_segments(const gtars_uniwig_plan *plan);
uint64_t gtars_uniwig_plan_total(const gtars_uniwig_plan *plan);
gtars_status gtars_uniwig_plan_table(const gtars_uniwig_plan *plan, uint32_t *seg_cid, uint32_t *seg_first, uint32_t *seg_len,
                                     uint64_t *seg_off);
/* compacted positions window_first .. window_first + window_len - 1 (step 1) into d_counts (device memory, 16-byte
 * aligned), queued on `stream` (a hipStream_t); nothing is synchronised */
gtars_status gtars_uniwig_stream_device(const gtars_uniwig_plan *plan, uint64_t window_first, uint64_t window_len,
                                        uint32_t *d_counts, void *stream);
/* write_records_as_bedgraph (stream.rs:450-466): "chrom\tpos-1\tpos\tcount\n" for pos = first, first + step, ... */
gtars_status gtars_uniwig_format_bedgraph_bases(const char *chrom, uint32_t first, uint32_t step, const uint32_t *counts,
                                                uint64_t n, char **out_text, uint64_t *out_len);

/* ------------------------------------------------------------------------
 * Genome assemblies, GC content and dinucleotide frequencies  (gtars-genomicdist/src/models.rs:145-492,
 * statistics.rs:331-483; gtars-python/src/models/genome_assembly.rs, genomic_distributions/tools.rs:8-70)
 *
 * An assembly handle holds the sequences on the host as the file has them: no case folding, N stays.  Its device
 * image -- one packed byte buffer, every chromosome at a 16-byte-aligned offset and followed by at least 16 zero bytes,
 * with u64 offset and length columns -- is built at the first counting call, on the device current then, which the
 * handle keeps: host-column calls run there whatever the caller's current device is, the device-pointer call refuses
 * another one.
 *
 * FASTA (GenomeAssembly::try_from, models.rs:163-187; plain files only).  The reference reads through an external
 * FASTA crate; what its fixtures pin is kept, the rest is this library's choice:
 *   - a record starts at a line whose first byte is '>'; its name is the text behind '>' up to the first ASCII
 *     whitespace (an empty name is a name); the sequence is the following lines up to the next '>' line, joined,
 *     every line stripped of trailing ASCII whitespace ('\r' included), blank lines adding nothing
 *   - an empty file is an assembly without chromosomes; a non-empty file whose first byte is not '>' is
 *     GTARS_ERR_PARSE; a missing or unreadable file GTARS_ERR_IO
 *   - a repeated name keeps the LAST record (HashMap::insert); chromosome ids follow the first appearance of a name
 * .fab (BinaryGenomeAssembly::from_file, models.rs:249-318): "GFAB", version u8 = 1, n_chroms u32 LE, per chromosome
 *   { name_len u16 LE, name, file offset u64 LE, length u64 LE }, then the sequences.  GTARS_ERR_PARSE for a file that
 *   is too short, has bad magic bytes, another version, a truncated index or index entry, a name that is not UTF-8, or
 *   (checked per query by the reference, here on load) an entry with offset + length beyond the file.  A repeated
 *   name resolves to the last entry.
 * ---------------------------------------------------------------------- */
typedef struct gtars_assembly gtars_assembly_t;
gtars_status gtars_assembly_from_fasta(const char *path, gtars_assembly_t **out);
gtars_status gtars_assembly_from_fab(const char *path, gtars_assembly_t **out);
/* BinaryGenomeAssembly::write_from_fasta (models.rs:357-412): every record of the FASTA file in file order, repeated
 * names included, sequences back to back behind the index */
gtars_status gtars_fab_write_from_fasta(const char *fasta_path, const char *out_path);
void gtars_assembly_free(gtars_assembly_t *a);
uint32_t gtars_assembly_n_chrom(const gtars_assembly_t *a);
const char *gtars_assembly_chrom_name(const gtars_assembly_t *a, uint32_t id);
uint64_t gtars_assembly_chrom_len(const gtars_assembly_t *a, uint32_t id);
int gtars_assembly_contains(const gtars_assembly_t *a, const char *name);
/* seq_from_region (models.rs:190-210, 321-350): *out = the bytes [start, end) of chromosome `name`, borrowed from the
 * handle; GTARS_ERR_INVALID_ARG for an unknown chromosome or unless end <= length && start <= end */
gtars_status gtars_assembly_sequence(const gtars_assembly_t *a, const char *name, uint64_t start, uint64_t end,
                                     const uint8_t **out);
int gtars_assembly_device(const gtars_assembly_t *a); /* -1 until the first counting call */

#define GTARS_SEQ_GC 0
#define GTARS_SEQ_DINUCL 1
/* bytes of a region one work item of the counting kernels covers (a region of width w is ceil(w / piece) of them) */
uint32_t gtars_seqstats_piece_bytes(void);
/* Integer counts of n device rows (d_chrom: chromosome ids of the assembly; every row start <= end <= length, anything
 * else is GTARS_ERR_INVALID_ARG and is never read from the image), queued on `stream` (a hipStream_t) of the current
 * device.  GTARS_SEQ_GC: d_out[n] = bytes of [start, end) that are G, C, g or c.  GTARS_SEQ_DINUCL: d_out[n * 16]
 * (16-byte aligned) = windows (b[i], b[i + 1]) with start <= i and i + 1 < end whose bytes are both in ACGTacgt, in the
 * order AA AC AG AT CA .. TT (DINUCL_ORDER, statistics.rs:386-391).  The stream is drained before the call returns (the
 * number of work items comes to the host on the way).  n == 0 touches nothing. */
gtars_status gtars_seqstats_counts_device(gtars_assembly_t *a, const uint32_t *d_chrom, const uint32_t *d_start,
                                          const uint32_t *d_end, uint64_t n, int mode, uint32_t *d_out, void *stream);
/* calc_gc_content / calc_dinucl_freq (statistics.rs:331-483) of rs.  Output rows: chromosomes in order of first
 * appearance in rs (iter_chroms), set order within one.  ignore_unk != 0: chromosomes the assembly lacks and rows with
 * end > length or start > end are skipped; otherwise the first such row in output order fails the call
 * (GTARS_ERR_INVALID_ARG, the message names chr, start and end) before anything is launched.
 *   gc:      *gc[*n_out] = count / (end - start) as f64, 0.0 for an empty region (every byte counts, N included)
 *   dinucl:  *row_index[*n_out] = the row of rs behind each output row; *freq[*n_out * 16] = the counts as f64
 *            (raw_counts != 0), else (count / total) * 100.0 with total = the row's valid windows, a zero row for
 *            total == 0
 * The divisions are host f64 arithmetic on the device's integer counts.  gtars_free each array. */
gtars_status gtars_seqstats_gc(gtars_assembly_t *a, const gtars_regionset_t *rs, int ignore_unk, double **gc, uint64_t *n_out);
gtars_status gtars_seqstats_dinucl(gtars_assembly_t *a, const gtars_regionset_t *rs, int raw_counts, int ignore_unk,
                                   uint64_t **row_index, double **freq, uint64_t *n_out);

/* ------------------------------------------------------------------------
 * Signal matrices and calc_summary_signal  (gtars-genomicdist/src/signal.rs; csrc/signal.cpp, csrc/signal.hip: K13)
 *
 * A handle holds a region x condition matrix of f64 on the host -- the rows in file order, never sorted, duplicates
 * kept -- and reads its files without a device.  Its device image (the row-major values and an AIList-kind overlap
 * index of the rows with val = row) is built at the first summary call, on the device current then, which the handle
 * keeps: the host call runs there whatever the caller's current device is, the device-pointer call refuses another one.
 *
 * TSV (SignalMatrix::from_tsv, signal.rs:73-164), read through gtars_read_file (".gz" by extension).  A line ends at
 * '\n', a '\r' in front of it is dropped.  The first line is the header, split on tab: fewer than 2 fields is
 * GTARS_ERR_PARSE, fields 1.. are the condition names.  Every later line is split on tab; field 0 is split on '_' and
 * must give exactly three parts (a contig name that contains '_' drops the row, an empty name is a name); parts 1 and 2
 * parse as u32 by Rust's rule (an optional '+', digits only, overflow fails); fewer than 1 + n_conditions fields skip
 * the row, extra fields are ignored; every value parses by Rust's f64::from_str (optional sign; decimal digits with an
 * optional '.' and exponent, "5." and ".5" included, "." not; inf / infinity / nan in any case; no whitespace, no hex;
 * correctly rounded).  Any failure skips the row silently.  An empty file and a file without a valid row are
 * GTARS_ERR_PARSE.
 *
 * SIGM version 2 (save_bin / load_bin_from_bytes, signal.rs:170-354), little-endian: u32 magic 0x5349474D, u32 version,
 * u32 n_regions, u32 n_conditions; the string table, u32 n_strings then per string u32 length + bytes; u32 n_names
 * (== n_conditions) and a u16 string id per condition; a u16 chromosome string id per region, a u32 start per region,
 * a u32 end per region; n_regions x n_conditions f64, row-major.  Written: the table holds the chromosome names in
 * order of first appearance, then the condition names it lacks (more than 65536 strings: GTARS_ERR_INVALID_ARG).
 * Read: wrong magic, another version, truncation anywhere, a name-count mismatch and a string id outside the table are
 * GTARS_ERR_PARSE; bytes behind the values are ignored.
 * ---------------------------------------------------------------------- */
typedef struct gtars_signal gtars_signal_t;
gtars_status gtars_signal_from_tsv(const char *path, gtars_signal_t **out);
gtars_status gtars_signal_load_bin(const char *path, gtars_signal_t **out);
gtars_status gtars_signal_save_bin(const gtars_signal_t *sm, const char *path);
/* n rows (chrom[i] < n_chrom indexes chrom_names) with values[n * n_conditions], row-major; n and n_conditions >= 1.
 * The handle's chromosome ids follow the first appearance of a name among the rows. */
gtars_status gtars_signal_from_arrays(const char *const *chrom_names, uint32_t n_chrom, const uint32_t *chrom,
                                      const uint32_t *start, const uint32_t *end, uint64_t n, const double *values,
                                      const char *const *condition_names, uint32_t n_conditions, gtars_signal_t **out);
void gtars_signal_free(gtars_signal_t *sm);
uint64_t gtars_signal_n_regions(const gtars_signal_t *sm);
uint32_t gtars_signal_n_conditions(const gtars_signal_t *sm);
const char *gtars_signal_condition_name(const gtars_signal_t *sm, uint32_t i);
/* the rows as dictionary-encoded columns (ids index gtars_signal_chrom_name) and the values, borrowed from the handle */
uint32_t gtars_signal_n_chrom(const gtars_signal_t *sm);
const char *gtars_signal_chrom_name(const gtars_signal_t *sm, uint32_t id);
const uint32_t *gtars_signal_chrom_ids(const gtars_signal_t *sm);
const uint32_t *gtars_signal_starts(const gtars_signal_t *sm);
const uint32_t *gtars_signal_ends(const gtars_signal_t *sm);
const double *gtars_signal_values(const gtars_signal_t *sm);
int gtars_signal_device(const gtars_signal_t *sm); /* -1 until the first summary call */

/* calc_summary_signal (signal.rs:364-454), Bed labels.  A query overlaps a row when row.start < q.end && row.end >
 * q.start (zero-length and inverted queries as the overlap index treats them; nothing else is filtered).  Output rows:
 * the queries with at least one hit, in query order.
 *   *qidx[*n_rows]                   the query's row in rs (its label is "{chr}_{start}_{end}")
 *   *values[*n_rows * n_conditions]  per condition the fold of the hit rows' values in AIList result order: the first
 *                                    hit's value, replaced by every later value that is greater.  So a NaN in the first
 *                                    hit stays (bits kept), NaNs elsewhere are ignored, ties keep the earlier hit
 *                                    (0.0 against -0.0).  Bit-exact.
 *   *stats[n_conditions * 5]         boxplot_stats (signal.rs:461-513) of every result column: lower whisker, lower
 *                                    hinge, median, upper hinge, upper whisker.  A column that holds a NaN has no
 *                                    defined result in the reference (its comparator is inconsistent there); here NaNs
 *                                    sort last.
 * *n_rows == 0 leaves all three NULL (the reference returns no statistics then).  gtars_free each array.
 * gtars_signal_summary_device: the queries are n device rows, d_chrom the matrix's chromosome ids (any other value: no
 * hits), queued on `stream` (a hipStream_t) of the current device, which is drained on the way and before the call
 * returns.  qidx and values may both be NULL: the rows then stay on the device and only the statistics come back. */
gtars_status gtars_signal_summary(gtars_signal_t *sm, const gtars_regionset_t *rs, uint32_t **qidx, double **values,
                                  double **stats, uint64_t *n_rows);
gtars_status gtars_signal_summary_device(gtars_signal_t *sm, const uint32_t *d_chrom, const uint32_t *d_start,
                                         const uint32_t *d_end, uint64_t n, void *stream, uint32_t **qidx, double **values,
                                         double **stats, uint64_t *n_rows);

/* ------------------------------------------------------------------------
 * Tokenizer  (gtars-tokenizers/src/tokenizer.rs:36-279, universe/mod.rs,
 * config.rs, utils/mod.rs:34-99, utils/special_tokens.rs)
 * ---------------------------------------------------------------------- */
typedef struct gtars_tokenizer gtars_tokenizer_t;

/* Tokenizer::from_auto / from_config / from_bed (tokenizer.rs:61-138) */
gtars_status gtars_tokenizer_from_auto(const char *path, gtars_tokenizer_t **out);
gtars_status gtars_tokenizer_from_config(const char *path, gtars_tokenizer_t **out);
gtars_status gtars_tokenizer_from_bed(const char *path, gtars_tokenizer_t **out);
void gtars_tokenizer_free(gtars_tokenizer_t *t);

uint64_t gtars_tokenizer_vocab_size(const gtars_tokenizer_t *t);       /* get_vocab_size */
int gtars_tokenizer_kind(const gtars_tokenizer_t *t);                  /* GTARS_KIND_* */
/* convert_id_to_token / convert_token_to_id (universe/mod.rs:64-80) */
const char *gtars_tokenizer_id_to_token(const gtars_tokenizer_t *t, uint32_t id); /* NULL: none */
int64_t gtars_tokenizer_token_to_id(const gtars_tokenizer_t *t, const char *token); /* -1: none */
/* get_vocab(): the i-th (token, id) pair of region_to_id, i < vocab_size */
const char *gtars_tokenizer_vocab_token(const gtars_tokenizer_t *t, uint64_t i, uint32_t *id);
/* special tokens in the order unk,pad,mask,cls,eos,bos,sep (special_tokens.rs:59-71) */
const char *gtars_tokenizer_special_token(const gtars_tokenizer_t *t, int which);
/* universe metadata (BED5+ universes): name / score of a region string, NULL / NaN if absent */
const char *gtars_tokenizer_region_name(const gtars_tokenizer_t *t, const char *region);
double gtars_tokenizer_region_score(const gtars_tokenizer_t *t, const char *region);

/* chromosome dictionary of the core (for array fast paths): -1 = unknown */
int64_t gtars_tokenizer_chrom_id(const gtars_tokenizer_t *t, const char *chr);
uint32_t gtars_tokenizer_n_chrom(const gtars_tokenizer_t *t);
const char *gtars_tokenizer_chrom_name(const gtars_tokenizer_t *t, uint32_t id);
/* borrowed engine handle for gtars_tokenize_device & friends */
const gtars_index_t *gtars_tokenizer_index(const gtars_tokenizer_t *t);

/* Tokenizer::encode (tokenizer.rs:165-171) of a region set: ids in reference
 * order, [unk] when nothing overlapped (tokenizer.rs:158-160). */
gtars_status gtars_tokenizer_encode_regionset(const gtars_tokenizer_t *t,
                                              const gtars_regionset_t *rs, uint32_t **out_ids,
                                              uint64_t *out_n);
/* same on parallel arrays with chromosome NAMES */
gtars_status gtars_tokenizer_encode_arrays(const gtars_tokenizer_t *t, const char *const *chrs,
                                           const uint32_t *starts, const uint32_t *ends,
                                           uint64_t n, uint32_t **out_ids, uint64_t *out_n);
/* additive array fast path: chromosome IDS of this tokenizer's dictionary
 * (GTARS_UNKNOWN_CHROM for unknown); returns the CSR too (offsets n+1) and
 * does NOT apply the batch-level unk rule. */
gtars_status gtars_tokenizer_encode_ids(const gtars_tokenizer_t *t, const uint32_t *chrom_ids,
                                        const uint32_t *starts, const uint32_t *ends, uint64_t n,
                                        uint64_t *offsets, uint32_t **out_ids, uint64_t *out_n);

/* Tokenizer::encode of n_sets region sets in one device pass (gtars_tokenize_sets_device): per set what
 * gtars_tokenizer_encode_regionset gives for it alone -- [unk] for a set without any id -- cut to its first max_length
 * ids (0: all of them).  *out_offsets: n_sets + 1 entries, set b's ids are (*out_ids)[(*out_offsets)[b] ..
 * (*out_offsets)[b + 1]); *out_n = their number; both arrays are released with gtars_free.  n_sets == 0 is valid.
 * gtars_tokenizer_encode_sets_ids is the array form: chromosome IDS of this tokenizer's dictionary for the concatenated
 * sets, set b = rows [set_offsets[b], set_offsets[b + 1]); set_offsets that do not start at 0, descend or do not end at n
 * are GTARS_ERR_INVALID_ARG.
 * gtars_tokenizer_encode_sets_padded gives the [n_sets, *width] matrices over the same inputs: the sets' ids and the
 * tokenizer's pad id on `side` (GTARS_PAD_RIGHT / GTARS_PAD_LEFT), the mask 1 on ids and 0 on padding.  width_or_0 == 0: the
 * longest set; otherwise that width, and GTARS_ERR_INVALID_ARG when a set is longer -- nothing is cut silently.
 * Without a device every one of the three fails with GTARS_ERR_NO_DEVICE before it looks at its arguments. */
gtars_status gtars_tokenizer_encode_sets(const gtars_tokenizer_t *t, const gtars_regionset_t *const *sets,
                                         uint64_t n_sets, uint64_t max_length, uint64_t **out_offsets,
                                         uint32_t **out_ids, uint64_t *out_n);
gtars_status gtars_tokenizer_encode_sets_ids(const gtars_tokenizer_t *t, const uint32_t *chrom_ids,
                                             const uint32_t *starts, const uint32_t *ends, uint64_t n,
                                             const uint64_t *set_offsets, uint64_t n_sets, uint64_t max_length,
                                             uint64_t **out_offsets, uint32_t **out_ids, uint64_t *out_n);
gtars_status gtars_tokenizer_encode_sets_padded(const gtars_tokenizer_t *t, const uint32_t *chrom_ids,
                                                const uint32_t *starts, const uint32_t *ends, uint64_t n,
                                                const uint64_t *set_offsets, uint64_t n_sets, uint64_t max_length,
                                                uint64_t width_or_0, int side, uint32_t **input_ids,
                                                uint8_t **mask, uint64_t *width);

/* ------------------------------------------------------------------------
 * Fragment files as SoA columns (parse_fragment_line, utils/fragments.rs:12-40):
 * `chr start end barcode count` split on whitespace, lines starting with '#'
 * skipped, fewer than 5 fields / unparsable start or end -> GTARS_ERR_PARSE with
 * the reference's message and 0-based line number.  .gz by extension.  The text
 * is parsed in place by all host threads (GTARS_HOST_THREADS overrides);
 * chromosome and barcode ids are dictionary codes in first-seen order.
 * ---------------------------------------------------------------------- */
typedef struct gtars_fragments gtars_fragments_t;
gtars_status gtars_fragments_read(const char *path, gtars_fragments_t **out);
/* the same with the fifth field (read support) required to parse as u32, as Fragment::from_str does
 * (gtars-core/src/models/fragments.rs:16-41: the parser behind gtars-scoring) */
gtars_status gtars_fragments_read_strict(const char *path, gtars_fragments_t **out);
/* BED3 text mode of the `gtars overlaprs` front end (gtars-cli/src/overlaprs/handlers.rs:64-92, 123-139): EVERY line is a
 * record (no header / comment skipping), fields split on TAB only, start and end through str::parse::<u32>; errors name
 * the file and the 1-based line ("Missing start field", "Missing end field", "invalid digit found in string").  The
 * columns come back in a gtars_fragments_t without barcodes (file order, chromosome ids in first-seen order). */
gtars_status gtars_bed3_lines_read(const char *path, gtars_fragments_t **out);
/* the front end's output (handlers.rs:141-150): one line chr<TAB>start<TAB>end per hit, in the order given; *out_text is
 * malloc'ed (gtars_free), NUL-terminated, *out_len bytes long */
gtars_status gtars_format_hit_lines(const char *const *chrom_names, const uint32_t *hit_chrom, const uint32_t *hit_start,
                                    const uint32_t *hit_end, uint64_t n, char **out_text, uint64_t *out_len);
void gtars_fragments_free(gtars_fragments_t *f);
uint64_t gtars_fragments_len(const gtars_fragments_t *f);
uint32_t gtars_fragments_n_chrom(const gtars_fragments_t *f);
uint32_t gtars_fragments_n_barcodes(const gtars_fragments_t *f);
const char *gtars_fragments_chrom_name(const gtars_fragments_t *f, uint32_t id);
const char *gtars_fragments_barcode_name(const gtars_fragments_t *f, uint32_t id);
const uint32_t *gtars_fragments_chrom_ids(const gtars_fragments_t *f);
const uint32_t *gtars_fragments_starts(const gtars_fragments_t *f);
const uint32_t *gtars_fragments_ends(const gtars_fragments_t *f);
const uint32_t *gtars_fragments_barcode_ids(const gtars_fragments_t *f);

/* tokenize_fragment_file (utils/fragments.rs:61-82): one single-region
 * tokenize per fragment line (so every non-overlapping fragment yields one
 * unk id), grouped by barcode.  Result: n_barcodes names (first-seen order)
 * and a CSR of ids per barcode. */
typedef struct gtars_fragment_tokens {
    uint64_t n_barcodes;
    char **barcodes;      /* n_barcodes strings */
    uint64_t *offsets;    /* n_barcodes + 1 */
    uint32_t *ids;        /* offsets[n_barcodes] */
} gtars_fragment_tokens_t;
gtars_status gtars_tokenizer_tokenize_fragment_file(const gtars_tokenizer_t *t, const char *path,
                                                    gtars_fragment_tokens_t **out);
void gtars_fragment_tokens_free(gtars_fragment_tokens_t *ft);
/* the barcodes of `ft` in one buffer, '\n'-separated (no newline behind the last; barcodes are whitespace-free fields): one call
 * for a binding that would otherwise convert n_barcodes C strings one by one (19,200 of them were a fifth of the fused
 * pipeline's 48-file call from Python).  *out: gtars_free. */
gtars_status gtars_fragment_tokens_barcodes_joined(const gtars_fragment_tokens_t *ft, char **out, uint64_t *out_len);

/* ------------------------------------------------------------------------
 * gtars-fragsplit: pseudobulking of fragment files by a barcode -> cluster map.
 *   gtars_barcode_map_from_file   BarcodeToClusterMap::from_file (gtars-fragsplit/src/map.rs:34-81): one
 *                                 `<file stem>+<barcode> <cluster>` pair per line, split on whitespace, later lines win;
 *                                 a line with fewer than two fields -> GTARS_ERR_PARSE ("Invalid line format ...")
 *   gtars_fragsplit               pseudobulk_fragment_files (split.rs:36-151): every regular file of `files_dir`
 *                                 (.gz by extension), lines split on whitespace into chr start end barcode
 *                                 read_support (fewer than five fields -> GTARS_ERR_PARSE "Failed to parse fragments
 *                                 file at line {0-based index}: {line}"), looked up as "{stem}+{barcode}" with the stem
 *                                 stripped of ALL extensions (utils.rs remove_all_extensions), and written as
 *                                 "chr\tstart\tend\tbarcode\tread_support\n" to <out_dir>/cluster_<id>.bed.gz (one
 *                                 file per cluster label, also when empty; gzip level 6).  The reference visits the
 *                                 files in read_dir order (unspecified); here they are visited in byte order of their
 *                                 names, so the output is deterministic.  Files are parsed by all host threads.
 *   gtars_fragsplit_tokenize      the "gtars-fragsplit -> tokenizer" pipeline without the intermediate files: for every
 *                                 cluster (labels in byte order) exactly what tokenize_fragment_file returns for
 *                                 cluster_<id>.bed.gz -- the routed lines are parsed like fragment-file lines ('#'
 *                                 lines skipped, start / end must parse as u32), one batched GPU tokenization per cluster.
 * ---------------------------------------------------------------------- */
typedef struct gtars_barcode_map gtars_barcode_map_t;
gtars_status gtars_barcode_map_from_file(const char *path, gtars_barcode_map_t **out);
void gtars_barcode_map_free(gtars_barcode_map_t *m);
uint64_t gtars_barcode_map_len(const gtars_barcode_map_t *m);
uint32_t gtars_barcode_map_n_clusters(const gtars_barcode_map_t *m);
/* i-th cluster label in byte order */
const char *gtars_barcode_map_cluster_label(const gtars_barcode_map_t *m, uint32_t i);
/* cluster label of a "stem+barcode" key, NULL when it is not in the map */
const char *gtars_barcode_map_lookup(const gtars_barcode_map_t *m, const char *key);
gtars_status gtars_fragsplit(const char *files_dir, const gtars_barcode_map_t *m, const char *out_dir,
                             uint64_t *n_reads, uint64_t *n_written);
/* *out: array of n_clusters results (gtars_fragment_tokens_free each, gtars_free the array) */
gtars_status gtars_fragsplit_tokenize(const gtars_tokenizer_t *t, const char *files_dir, const gtars_barcode_map_t *m,
                                      gtars_fragment_tokens_t ***out, uint64_t *n_reads);
/* the same pipeline over an explicit list of fragment files, visited in the order given: what one rank of the multi-GPU
 * driver runs on its run of the directory's sorted file list (files are independent; the per-cluster results
 * of consecutive runs merge by concatenation per barcode, gtars_amd/sharding.py fragsplit_tokenize_sharded) */
gtars_status gtars_fragsplit_tokenize_files(const gtars_tokenizer_t *t, const char *const *paths, uint64_t n_paths,
                                            const gtars_barcode_map_t *m, gtars_fragment_tokens_t ***out, uint64_t *n_reads);

/* Diagnostic: seconds per stage of the calling thread's last gtars_fragsplit_tokenize(_files) call.  out12 = { 1 if the text was
 * parsed on the device (else on the host threads), waves, read + inflate on the host threads (host parser: + parse + route),
 * per-cluster append (host parser only), device waves / tokenizer calls in total, of which behind the last wave's files,
 * regroup by barcode, then for the device waves: text to the device, line split + parse + sort by cluster, gather, tokenize,
 * results to the host }. */
void gtars_fragsplit_last_stages(double *out12);
/* ... and what the device inflate of that call did (GTARS_FRAG_INFLATE=device; zeros otherwise): out4 = { BGZF members inflated
 * on the device, files handed back to the host's decoders, compressed bytes copied to the device, seconds in the member kernel by
 * the device's clock (measured only under GTARS_HOST_TIMING) }. */
void gtars_fragsplit_last_inflate(double *out4);

/* The member table of a BGZF file held in memory (data[0, n)), nothing inflated: what the fragment pipeline hands to the device
 * under GTARS_FRAG_INFLATE=device.  GTARS_ERR_PARSE (no message: it is an answer, not a failure) unless every member is a BGZF
 * block -- a gzip member with FEXTRA alone and a "BC" subfield of length 2 -- and BSIZE + 1 leads from member to member to
 * exactly the end of the data; such a file takes the ordinary gzip reader.  *n_members: the members; of the first `cap`, the
 * offset and length of the raw deflate stream in the data, ISIZE and CRC-32 of the trailer and the prefix sum of ISIZE (any of
 * the arrays may be NULL).  *last_byte (may be NULL): the last byte of the inflated data, found by inflating the last
 * non-empty member on the host; -1 when every member is empty, -2 when the host decoder refuses that member. */
gtars_status gtars_bgzf_members(const void *data, uint64_t n, uint64_t cap, uint64_t *n_members, uint64_t *stream_off,
                                uint32_t *stream_len, uint32_t *isize, uint32_t *crc, uint64_t *uoff, int32_t *last_byte);

/* Host threads one call of the file pipelines above starts at most: hardware threads, capped by the container's CPU quota
 * (cgroup v2 cpu.max) and by `cap`, divided by LOCAL_WORLD_SIZE when the process is one of several ranks of a launcher on this
 * node (torch.distributed.run sets it; each rank of the sharded fragment pipeline inflates and parses on its share of the cores);
 * GTARS_HOST_THREADS overrides.  Diagnostic: the reference has no threads on this path (gtars-fragsplit/src/split.rs:36-151). */
uint32_t gtars_host_threads(uint32_t cap);

/* get_dynamic_reader (gtars-core/src/utils.rs:115-126) as one call: the file's bytes, gunzipped iff its extension is "gz"
 * (concatenated members decoded one after the other, every member's CRC-32 and length checked; a ".gz" without the gzip magic is
 * returned as it is).  What every file front end above reads through.  *out: malloc'ed (gtars_free), *out_n bytes.
 * GTARS_ERR_IO with the reader's message otherwise. */
gtars_status gtars_read_file(const char *path, char **out, uint64_t *out_n);

/* ------------------------------------------------------------------------
 * .gtok  (gtars-io/src/gtok.rs:125-210, consts.rs:1-3)
 * ---------------------------------------------------------------------- */
gtars_status gtars_gtok_write(const char *path, const uint32_t *tokens, uint64_t n);
gtars_status gtars_gtok_read(const char *path, uint32_t **out_tokens, uint64_t *out_n);

/* ------------------------------------------------------------------------
 * IGD database built from BED files (gtars-igd/src/igd.rs:170-242, 850-867)
 * ---------------------------------------------------------------------- */
typedef struct gtars_igddb gtars_igddb_t;

/* Igd::from_bed_files: unreadable files and files without a parseable line
 * are skipped; lines with start < 0 are parsed but not added. */
gtars_status gtars_igddb_from_bed_files(const char *const *paths, uint64_t n_paths,
                                        gtars_igddb_t **out);
/* Igd::from_bed_dir: *.bed / *.gz regular files of the directory, sorted */
gtars_status gtars_igddb_from_bed_dir(const char *dir, gtars_igddb_t **out);
void gtars_igddb_free(gtars_igddb_t *db);
uint32_t gtars_igddb_n_files(const gtars_igddb_t *db);
uint32_t gtars_igddb_n_contigs(const gtars_igddb_t *db);
/* FileInfo (igd.rs:52-59) */
const char *gtars_igddb_file_name(const gtars_igddb_t *db, uint32_t i);
uint32_t gtars_igddb_file_num_regions(const gtars_igddb_t *db, uint32_t i);
double gtars_igddb_file_avg_width(const gtars_igddb_t *db, uint32_t i);
int64_t gtars_igddb_chrom_id(const gtars_igddb_t *db, const char *chr); /* -1 unknown */
const char *gtars_igddb_chrom_name(const gtars_igddb_t *db, uint32_t id); /* contigs in creation order */
const gtars_igd_t *gtars_igddb_engine(const gtars_igddb_t *db);        /* borrowed */
/* Igd::count_set_overlaps (binary=0) / count_region_hits (binary=1) of a region set */
gtars_status gtars_igddb_count_regionset(const gtars_igddb_t *db, const gtars_regionset_t *rs,
                                         int32_t min_overlap, int binary, uint64_t *hits);

/* Igd::save / Igd::from_igd_file (gtars-igd/src/igd.rs:320-486): the .igd v1 file -- LE i32 header {nbp, gType = 1,
 * nCtg}, tiles per contig, record counts per tile, 40-byte NUL-padded contig names, 16-byte records {file idx, start,
 * end, value} tile by tile (a record is written once for every nbp-tile it touches) -- and its companion
 * <stem>.tsv ("Index\tFile\tNumber of Regions\tAvg size").  On load a record is kept from the tile it starts in, so
 * the device holds every stored interval once; gType 0 files (12-byte records) load with value 0.
 * gtars_igddb_from_arrays builds a database handle from columns the caller has already parsed (chromosome ids index
 * chrom_names; file i is described by file_names[i], num_regions[i], avg_width[i]). */
gtars_status gtars_igddb_from_arrays(const char *const *chrom_names, uint32_t n_chrom, const uint32_t *chrom,
                                     const int32_t *start, const int32_t *end, const int32_t *value,
                                     const uint32_t *file_idx, uint64_t n, const char *const *file_names,
                                     const uint32_t *num_regions, const double *avg_width, uint32_t n_files,
                                     gtars_igddb_t **out);
gtars_status gtars_igddb_save(const gtars_igddb_t *db, const char *path, int32_t nbp);
gtars_status gtars_igddb_load(const char *path, gtars_igddb_t **out, int32_t *nbp);

/* ------------------------------------------------------------------------
 * LOLA statistics tail  (gtars-lola/src/enrichment.rs:19-169, 243-394; output.rs:35-113)
 * ---------------------------------------------------------------------- */
/* Everything run_lola computes from the contingency cells, for all tables of a run in one threaded call.
 * a, b, c, d: [n_user_sets x n_db] row-major i64 cells (what gtars_lola_contingency_device leaves; b, c, d may be
 * negative: such a table gets pValueLog 0 and oddsRatio NaN, enrichment.rs:226-247).  direction: 0 enrichment
 * (p = sf(a - 1)), 1 depletion (p = cdf(a)).  Outputs, same layout, row = user set * n_db + db set:
 *   p_value_log  -log10(p + 1e-322)                                  (enrichment.rs:166-169)
 *   odds_ratio   conditional MLE as R's fisher.test: NaN for a one-point support, 0 / inf at its ends (:62-160)
 *   rnk_pv / rnk_or / rnk_sup / max_rnk / mean_rnk: min-ranks inside a user set, descending, NaN odds ratios last,
 *                ties by bit pattern (NaN == NaN, 0.0 != -0.0)       (:296-394)  -- all five NULL: values only
 *   order        the rows in the reference's output order: pValueLog descending, then meanRnk ascending, stable (:285-294)
 *   q_value      Benjamini-Hochberg per user set over the rows in that order (output.rs:35-113)
 * order / q_value may be NULL.  Hypergeometric sums and the odds-ratio equation are evaluated over the window of terms that
 * matter (see csrc/lola_stats.cpp); parity with the reference's statrs 0.18 values is to floating-point tolerance. */
gtars_status gtars_lola_stats(const int64_t *a, const int64_t *b, const int64_t *c, const int64_t *d, uint64_t n_db,
                              uint64_t n_user_sets, int direction, double *p_value_log, double *odds_ratio,
                              uint32_t *rnk_pv, uint32_t *rnk_or, uint32_t *rnk_sup, uint32_t *max_rnk, double *mean_rnk,
                              uint64_t *order, double *q_value);
/* rank_results (enrichment.rs:353-394) on the n rows of ONE user set, values given: min-ranks by pValueLog, oddsRatio (NaN
 * last) and support, all descending; maxRnk and meanRnk. */
gtars_status gtars_lola_rank(const double *p_value_log, const double *odds_ratio, const uint64_t *support, uint64_t n,
                             uint32_t *rnk_pv, uint32_t *rnk_or, uint32_t *rnk_sup, uint32_t *max_rnk, double *mean_rnk);
/* apply_fdr_correction (output.rs:35-113) on n_rows result rows in the order they stand: Benjamini-Hochberg q-values per
 * user set (q_value[r] for row r). */
gtars_status gtars_lola_fdr(const double *p_value_log, const uint64_t *user_set, uint64_t n_rows, double *q_value);
/* ContingencyTable::fisher_pvalue / odds_ratio of one table (enrichment.rs:19-53, 62-160) */
double gtars_lola_fisher_pvalue(uint64_t a, uint64_t b, uint64_t c, uint64_t d, int direction);
double gtars_lola_odds_ratio(uint64_t a, uint64_t b, uint64_t c, uint64_t d);

/* ------------------------------------------------------------------------
 * BAM input and BAM QC  (K17; gtars-uniwig/src/reading.rs:279-319, bamqc.rs:68-245)
 * ---------------------------------------------------------------------- */
/* A BAM file: its BGZF block table (one pass over the file, nothing decoded), its header, and the entry points that read
 * its records.  Coordinate-sorted files only (refID never descends, unplaced records last); no .bai is needed or read.
 * Host threads only inflate; the records are decoded and the QC is computed on the device (GTARS_ERR_NO_DEVICE
 * without one).  A damaged container or record is GTARS_ERR_PARSE with the block's or the record's index. */
typedef struct gtars_bam gtars_bam_t;
typedef struct {
    uint64_t total_reads; /* joined pairs if any reference held a paired read, else reads - mitochondrial reads */
    uint64_t distinct, m1, m2, dups, mito_reads;
    double nrf, pbc1, pbc2;
} gtars_bam_qc_result;

gtars_status gtars_bam_open(const char *path, gtars_bam_t **out);
void gtars_bam_close(gtars_bam_t *b);
const char *gtars_bam_header_text(const gtars_bam_t *b);
uint32_t gtars_bam_n_ref(const gtars_bam_t *b);
const char *gtars_bam_ref_name(const gtars_bam_t *b, uint32_t i);
uint32_t gtars_bam_ref_len(const gtars_bam_t *b, uint32_t i);
uint64_t gtars_bam_n_blocks(const gtars_bam_t *b);
uint64_t gtars_bam_n_bytes(const gtars_bam_t *b);      /* inflated */
uint64_t gtars_bam_first_record(const gtars_bam_t *b); /* inflated offset behind the header */
/* per block (any array may be NULL): offset and size in the file, ISIZE, CRC-32 and offset in the inflated stream */
gtars_status gtars_bam_block_table(const gtars_bam_t *b, uint64_t *coff, uint32_t *csize, uint32_t *isize, uint32_t *crc,
                                   uint64_t *uoff);
/* blocks [block0, block1) inflated to dst (block k at uoff[k] - uoff[block0]); every block's length and CRC-32 are
 * checked.  threads: 0 = gtars_host_threads(0), never more than that. */
gtars_status gtars_bam_inflate(const gtars_bam_t *b, uint64_t block0, uint64_t block1, void *dst, uint64_t capacity,
                               uint32_t threads);
/* the offsets (of the block_size fields) of the records in data[begin, n), gtars_free; *consumed: where the first
 * incomplete record starts (an error when final != 0) */
gtars_status gtars_bam_record_offsets(const gtars_bam_t *b, const void *data, uint64_t n, uint64_t begin, int final,
                                      uint64_t **offsets, uint64_t *count, uint64_t *consumed);
/* records [first, first + count) of the file, decoded on the device: *cols = 7 arrays of *n int32 one behind the other
 * (refID, pos, end = pos + the CIGAR's reference span, flag, mapq, l_seq, tlen), gtars_free.
 * max_window_bytes: inflated bytes per device window, 0 = 256 MiB. */
gtars_status gtars_bam_decode(const gtars_bam_t *b, uint64_t first, uint64_t count, uint64_t max_window_bytes,
                              uint32_t threads, int32_t **cols, uint64_t *n);
gtars_status gtars_bam_qc(const gtars_bam_t *b, uint64_t max_window_bytes, uint32_t threads, gtars_bam_qc_result *out);
/* the calling thread's last gtars_bam_qc / gtars_bam_decode / gtars_bam_fragments: seconds of open (read + block table +
 * header), inflate, record walk; windows; records; seconds of the whole call */
void gtars_bam_last_stages(double *out6);

/* BAM to fragments (K26; DESIGN.md section 3 K26 states the rule -- it is this library's, no reference pins it).  A
 * coordinate-sorted paired-end BAM becomes the deduplicated fragments of a 10x-style fragment file: the leftmost mate of a
 * proper pair makes the fragment (pos + shift_left, pos + tlen + shift_right), clamped to the reference; equal (reference,
 * start, end, barcode) tuples collapse into one row whose count is their multiplicity.  The records are filtered, their aux
 * tags walked, and the rows sorted and collapsed on the device. */
typedef struct gtars_bam_frags gtars_bam_frags_t;
typedef struct {
    char barcode_tag[2];     /* the aux tag (type Z) that holds the cell barcode */
    int32_t use_barcode_tag; /* 0: no tag is read, every pair belongs to `sample` */
    const char *sample;      /* read when use_barcode_tag == 0: not empty, no white space */
    int32_t min_mapq;        /* >= 0 */
    int64_t max_fragment_length; /* >= 1 */
    int32_t shift_left, shift_right;
    uint32_t require_flags, exclude_flags;
} gtars_bam_frag_params;
/* barcode_tag "CB", min_mapq 30, max_fragment_length 2000, shift (4, -5), require 0x3, exclude 0xB0C, sample "bulk" */
void gtars_bam_frag_params_default(gtars_bam_frag_params *p);
/* records, then the reasons a record gives no fragment in the order they are tested (unplaced, flag, mapq, mate_ref,
 * not_leftmost, too_long, no_barcode, empty), kept_pairs, fragments (rows), barcodes: records = the reasons + kept_pairs,
 * the sum of the count column = kept_pairs */
#define GTARS_BAM_FRAG_N_STATS 12
/* Malformed aux data in a record that reaches the barcode step is GTARS_ERR_PARSE with the record range of its window.
 * More than 2^32 - 2 kept pairs are refused.  *out: gtars_bam_frags_free. */
gtars_status gtars_bam_fragments(const gtars_bam_t *b, const gtars_bam_frag_params *params, uint64_t max_window_bytes,
                                 uint32_t threads, gtars_bam_frags_t **out);
uint64_t gtars_bam_frags_len(const gtars_bam_frags_t *f);
/* the columns, borrowed: refID, start, end, barcode id and count of every row, in (refID, start, end, barcode) order */
const int32_t *gtars_bam_frags_ref(const gtars_bam_frags_t *f);
const uint32_t *gtars_bam_frags_start(const gtars_bam_frags_t *f);
const uint32_t *gtars_bam_frags_end(const gtars_bam_frags_t *f);
const uint32_t *gtars_bam_frags_barcode(const gtars_bam_frags_t *f);
const uint32_t *gtars_bam_frags_count(const gtars_bam_frags_t *f);
/* the distinct barcodes in id order (their byte order, a prefix before the longer string); *len: bytes without the NUL */
uint64_t gtars_bam_frags_n_barcodes(const gtars_bam_frags_t *f);
const char *gtars_bam_frags_barcode_name(const gtars_bam_frags_t *f, uint64_t i, uint64_t *len);
void gtars_bam_frags_stats(const gtars_bam_frags_t *f, uint64_t *out12);
/* `chrom \t start \t end \t barcode \t count \n` per row, chrom from the header of `b`; one gzip member when the path ends
 * in ".gz".  No row: an empty file. */
gtars_status gtars_bam_frags_write(const gtars_bam_frags_t *f, const gtars_bam_t *b, const char *path);
void gtars_bam_frags_free(gtars_bam_frags_t *f);
/* the same writer over the caller's host columns and name tables (host code, no device) */
gtars_status gtars_fragments_write_text(const char *path, const char *const *ref_names, uint32_t n_ref, const char *const *barcodes,
                                        uint64_t n_barcodes, const int32_t *ref, const uint32_t *start, const uint32_t *end,
                                        const uint32_t *barcode, const uint32_t *count, uint64_t n);

/* ------------------------------------------------------------------------
 * VRS allele identifiers  (K18; gtars-vrs/src/normalize.rs:362-441, digest.rs:52-86, vcf_core.rs:35-189, vcf.rs:56-73;
 * gtars-python/src/vrs/funcs.rs)
 * ---------------------------------------------------------------------- */
/* The scalar calls: host code, no device.  out33: 32 characters and a NUL.
 * sha512t24u: the first 24 bytes of SHA-512 in base64url without padding.  The two digests hash the canonical texts of
 * digest.rs:60-81 with `accession` written as given ("SQ." included) and the sequence as a literal state; neither is
 * JSON-escaped (accessions are base64url, sequences nucleotide letters).
 * gtars_vrs_normalize: normalize() over the caller's sequence bytes, which are read upper-cased; allele bytes are used as
 * given.  *allele: gtars_free.  A failure is GTARS_ERR_INVALID_ARG with NormalizeError's text. */
gtars_status gtars_sha512t24u(const void *data, uint64_t n, char *out33);
gtars_status gtars_vrs_location_digest(const char *accession, uint64_t start, uint64_t end, char *out33);
gtars_status gtars_vrs_allele_digest(const char *accession, uint64_t start, uint64_t end, const char *sequence,
                                     uint64_t sequence_len, char *out33);
gtars_status gtars_vrs_normalize(const uint8_t *sequence, uint64_t sequence_len, uint64_t start, const uint8_t *ref,
                                 uint64_t ref_len, const uint8_t *alt, uint64_t alt_len, uint64_t *new_start, uint64_t *new_end,
                                 uint8_t **allele, uint64_t *allele_len);
/* sha512t24u of every chromosome's upper-cased bytes, one chromosome per host task (threads: 0 = as many as
 * gtars_host_threads allows), computed once and kept on the handle.  *out: borrowed, 33 bytes per chromosome id (32
 * characters and a NUL). */
gtars_status gtars_assembly_refget_digests(gtars_assembly_t *a, uint32_t threads, const char **out);

/* A batch of alleles as columns.  Allele i: chromosome id chrom[i] of the assembly, 0-based interbase start[i], REF =
 * pool[ref_off[i], ref_off[i] + ref_len[i]), ALT likewise (rows may share pool bytes).  accessions: 32 digest characters per
 * chromosome id, a row of zero bytes = none (its alleles get status 4); NULL: the assembly's own refget digests.
 * Per allele (any output may be NULL): status -- 0, or 1 start + len(REF) overflows, 2 REF reaches past the chromosome's
 * end (a start beyond the chromosome too), 3 REF differs from the assembly (the three kinds of NormalizeError), 4 unknown
 * chromosome id / no accession, 5 allele bytes outside the pool --, the normalized interval, and the 32 characters of the
 * Allele digest (zero bytes for a failed allele; "ga4gh:VA." is the caller's).  A call never fails for data.
 * seq_offsets / seq_bytes (both or neither; gtars_free each): the normalized sequences as a byte CSR of n + 1 offsets.
 * on_host != 0: the library's host path on `threads` threads (0 = gtars_host_threads), no device; otherwise the kernels
 * of csrc/vrs.hip on the assembly's device (GTARS_ERR_NO_DEVICE without one). */
gtars_status gtars_vrs_alleles(gtars_assembly_t *a, const char *accessions, const uint32_t *chrom, const uint64_t *start,
                               const uint8_t *pool, uint64_t pool_bytes, const uint32_t *ref_off, const uint32_t *ref_len,
                               const uint32_t *alt_off, const uint32_t *alt_len, uint64_t n, int on_host, uint32_t threads,
                               uint8_t *status, uint64_t *new_start, uint64_t *new_end, char *digests, uint64_t **seq_offsets,
                               uint8_t **seq_bytes);
/* The same for columns, pool and outputs that are device memory (d_digests: n * 32 bytes, 8-byte aligned; any output may
 * be NULL), queued on `stream`, which is drained before the call returns.  The current device must be the assembly's:
 * anything else is refused, as by the other handle-taking device entries. */
gtars_status gtars_vrs_ids_device(gtars_assembly_t *a, const char *accessions, const uint32_t *d_chrom, const uint64_t *d_start,
                                  const uint8_t *d_pool, uint64_t pool_bytes, const uint32_t *d_ref_off, const uint32_t *d_ref_len,
                                  const uint32_t *d_alt_off, const uint32_t *d_alt_len, uint64_t n, uint8_t *d_status,
                                  uint64_t *d_new_start, uint64_t *d_new_end, char *d_digests, void *stream);

/* The alleles of a VCF file: plain text, gzip or BGZF by the magic bytes, not the extension.  Lines: trailing CR / LF
 * stripped; empty lines, lines starting with '#', lines with fewer than 5 tab-separated fields and lines whose POS is no
 * u64 or is 0 are skipped; ALT is split on ',' and a piece is kept unless it is empty, starts with '<', or is "*" or ".";
 * a row whose chromosome the assembly (or the accession table) lacks is skipped.  File order, ALTs in their order.
 * gtars_vcf_read_alleles parses only (host); gtars_vrs_from_vcf also computes the digests and fails with
 * "Failed to normalize variant at <chrom>:<POS>: <cause>" for the first allele in file order that does not normalize. */
typedef struct gtars_vrs_results gtars_vrs_results_t;
gtars_status gtars_vcf_read_alleles(gtars_assembly_t *a, const char *path, const char *accessions, uint32_t threads,
                                    gtars_vrs_results_t **out);
gtars_status gtars_vrs_from_vcf(gtars_assembly_t *a, const char *path, const char *accessions, int on_host, uint32_t threads,
                                gtars_vrs_results_t **out);
void gtars_vrs_results_free(gtars_vrs_results_t *r);
uint64_t gtars_vrs_results_len(const gtars_vrs_results_t *r);
/* borrowed columns of the results: chromosome ids, 0-based positions, the pool and the four allele columns, 32 digest
 * characters per allele (*digests NULL after gtars_vcf_read_alleles) */
gtars_status gtars_vrs_results_columns(const gtars_vrs_results_t *r, const uint32_t **chrom, const uint64_t **pos,
                                       const uint8_t **pool, uint64_t *pool_bytes, const uint32_t **ref_off, const uint32_t **ref_len,
                                       const uint32_t **alt_off, const uint32_t **alt_len, const char **digests);

/* ------------------------------------------------------------------------
 * Transcripts  (K19; gtars-refget/src/transcripts/{models,builder,store,mapper,sequence}.rs, gtars-python/src/reftx/mod.rs)
 * ---------------------------------------------------------------------- */
/* A builder stages transcripts.  Exons are (start, end) pairs of u32, 0-based half-open, in genomic order; a CDS end that
 * is 0xFFFFFFFF is "none"; strand is +1 or -1; mane_flags: bit 0 MANE Select, bit 1 MANE Plus Clinical.  A chromosome is
 * named by its refget accession, "SQ." + base64url of 24 bytes ("SQ." optional); anything else is GTARS_ERR_INVALID_ARG
 * with the text of reftx/mod.rs:282-300.
 * add_cdot applies the skip rules of builder.rs:146-208 to one cdot transcript: *added = 0 for a contig without a
 * mapping, a strand that is not +1 / -1 or an empty exon list; MANE flags by full accession, then by base accession.
 * add_mane records the flags of one accession under its full and its base form (builder.rs:114-125).
 * bytes: the .reftx v2 image (gtars_free); build: the image written to a temporary file in the destination's directory
 * and renamed onto `path`; GTARS_ERR_EMPTY "No transcripts to write" for an empty builder; an accession or gene longer
 * than 255 bytes, or more than 65535 exons, is GTARS_ERR_INVALID_ARG. */
typedef struct gtars_txbuilder gtars_txbuilder_t;
gtars_status gtars_txbuilder_new(gtars_txbuilder_t **out);
void gtars_txbuilder_free(gtars_txbuilder_t *b);
uint64_t gtars_txbuilder_len(const gtars_txbuilder_t *b);
gtars_status gtars_txbuilder_add(gtars_txbuilder_t *b, const char *accession, const char *gene, const char *chrom_accession, int strand,
                                 uint32_t cds_start, uint32_t cds_end, uint32_t mane_flags, const uint32_t *exons, uint64_t n_exons);
gtars_status gtars_txbuilder_add_chrom_mapping(gtars_txbuilder_t *b, const char *name, const char *chrom_accession);
gtars_status gtars_txbuilder_add_mane(gtars_txbuilder_t *b, const char *accession, uint32_t flags);
gtars_status gtars_txbuilder_add_cdot(gtars_txbuilder_t *b, const char *id, const char *gene, const char *contig, int64_t strand,
                                      uint32_t cds_start, uint32_t cds_end, const uint32_t *exons, uint64_t n_exons, int *added);
gtars_status gtars_txbuilder_bytes(const gtars_txbuilder_t *b, uint8_t **out, uint64_t *n);
gtars_status gtars_txbuilder_build(const gtars_txbuilder_t *b, const char *path);

/* A read-only store: the file is read whole and every record decoded when it is opened.  Bad magic, another version, an
 * index or a record that does not fit the bytes: GTARS_ERR_PARSE, never a read past the buffer.  Transcripts are numbered
 * in the file's index order.  lookup / lookup_mane (gene, ASCII case-insensitive): the transcript's index, -1: none.
 * lookup_many: accession i is pool[offsets[i], offsets[i + 1]); idx[i] = its index or 2^32 - 1.
 * record: borrowed strings and exon pairs, the chromosome digest as 32 characters and a NUL (without "SQ.").
 * map: the host path of the mapping columns, see gtars_txbind_map. */
typedef struct gtars_txstore gtars_txstore_t;
gtars_status gtars_txstore_open(const char *path, gtars_txstore_t **out);
gtars_status gtars_txstore_from_bytes(const uint8_t *data, uint64_t n, gtars_txstore_t **out);
void gtars_txstore_free(gtars_txstore_t *s);
uint64_t gtars_txstore_len(const gtars_txstore_t *s);
int gtars_txstore_has_mane(const gtars_txstore_t *s);
int64_t gtars_txstore_lookup(const gtars_txstore_t *s, const char *accession);
int64_t gtars_txstore_lookup_mane(const gtars_txstore_t *s, const char *gene);
gtars_status gtars_txstore_lookup_many(const gtars_txstore_t *s, const uint8_t *pool, const uint64_t *offsets, uint64_t n, uint32_t threads,
                                       uint32_t *idx);
gtars_status gtars_txstore_record(const gtars_txstore_t *s, uint64_t i, const char **accession, const char **gene, char *chrom33, int *strand,
                                  uint32_t *mane_flags, uint32_t *cds_start, uint32_t *cds_end, uint32_t *length, uint32_t *cds_length,
                                  const uint32_t **exons, uint64_t *n_exons);
gtars_status gtars_txstore_map(const gtars_txstore_t *s, const uint32_t *tx, const uint8_t *kind, const int64_t *pos, const int64_t *offset,
                               const uint8_t *star, uint64_t n, uint32_t threads, uint64_t *out, uint8_t *status);

/* A store bound to an assembly: every distinct chromosome digest of the store is matched against the assembly's refget
 * digests.  The store and the assembly must outlive the binding.  The mapping tables go to the assembly's device at the
 * first device call and stay there.
 * map: query i is (transcript index tx[i], kind[i] 0 = c. / 1 = n. / 2 = genomic -> mature-mRNA offset, pos[i],
 * intronic offset[i], star[i] != 0 for c.*N); offset and star may be NULL (all zero).  out[i]: the 0-based genomic
 * position (kinds 0, 1) or the 0-based transcript offset (kind 2), 0 unless status[i] is 0.  status: 1 transcript not
 * found, 2 non-coding, 3 outside CDS, 4 outside transcript, 5 / 6 5' / 3' UTR overflow, 7 invalid intronic offset
 * (mapper.rs:19-50), 8 the genomic position lies in no exon, 9 unknown kind, 10 the transcript's exons are not ascending
 * and disjoint.  A call never fails for data.
 * sequences: row i is transcript idx[i]; status 0, 1 not found, 2 the assembly has no chromosome with the transcript's
 * digest, 3 an exon reaches past the chromosome's end, 4 exons not ascending and disjoint (rows that fail are never read
 * from the assembly); digests: the 32 characters of sha512t24u of the mature mRNA per row (zero bytes for a failed row;
 * "SQ." is the caller's); seq_offsets / seq_bytes (both or neither, gtars_free each): the mature mRNAs as a byte CSR --
 * forward transcripts are the assembly's bytes upper-cased, reverse ones reversed and complemented, any byte outside
 * ACGTN becoming N (sequence.rs:36-53).
 * on_host != 0: the library's host path on `threads` threads, no device; otherwise the kernels of csrc/reftx.hip on the
 * assembly's device (GTARS_ERR_NO_DEVICE without one).
 * The _device forms take columns and outputs that are device memory (d_digests: n * 32 bytes, 8-byte aligned), queued on
 * `stream`, which is drained before the call returns.  The current device must be the assembly's: anything else is
 * refused, as by the other handle-taking device entries. */
typedef struct gtars_txbind gtars_txbind_t;
gtars_status gtars_txbind_new(const gtars_txstore_t *s, gtars_assembly_t *a, uint32_t threads, gtars_txbind_t **out);
void gtars_txbind_free(gtars_txbind_t *b);
gtars_status gtars_txbind_map(gtars_txbind_t *b, const uint32_t *tx, const uint8_t *kind, const int64_t *pos, const int64_t *offset,
                              const uint8_t *star, uint64_t n, int on_host, uint32_t threads, uint64_t *out, uint8_t *status);
gtars_status gtars_txbind_sequences(gtars_txbind_t *b, const uint32_t *idx, uint64_t n, int on_host, uint32_t threads, uint8_t *status,
                                    char *digests, uint64_t **seq_offsets, uint8_t **seq_bytes);
gtars_status gtars_tx_map_device(gtars_txbind_t *b, const uint32_t *d_tx, const uint8_t *d_kind, const int64_t *d_pos,
                                 const int64_t *d_offset, const uint8_t *d_star, uint64_t n, uint64_t *d_out, uint8_t *d_status,
                                 void *stream);
gtars_status gtars_tx_digests_device(gtars_txbind_t *b, const uint32_t *d_idx, uint64_t n, uint8_t *d_status, char *d_digests,
                                     void *stream);

/* ------------------------------------------------------------------------
 * HGVS expressions  (K20; gtars-vrs/src/hgvs/{ast,parser,bridge}.rs, gtars-python/src/vrs/hgvs.rs)
 * ---------------------------------------------------------------------- */
/* One parsed expression.  Accession, gene, ref and alt are (offset, length) spans into the text that was parsed; nothing is
 * copied.  ref_type: 0 g, 1 c, 2 n, 3 m, 4 r, 5 p.  loc: 0 single, 1 range, 2 whole sequence, 3 / 4 / 5 a range whose
 * start / end / both are uncertain.  pos[0]: the start or its low bound, pos[1]: the start's high bound, pos[2]: the end or
 * its low bound, pos[3]: the end's high bound; present = 0 for a position the kind does not have and for "?"; datum: 0
 * sequence start, 1 CDS start, 2 CDS end (c.*N).  edit: 0 substitution, 1 deletion, 2 duplication, 3 insertion, 4 delins,
 * 5 inversion, 6 identity, 7 unknown, 8 copy (count), 9 repeat (its unit in the ref span, count).  flags: bit 0 a gene in
 * parentheses, bit 1 a reference allele, bit 2 uncertain. */
typedef struct gtars_hgvs_position {
    int64_t base, offset;
    uint8_t datum, present;
    uint8_t reserved[6];
} gtars_hgvs_position;
typedef struct gtars_hgvs_row {
    uint32_t acc_off, acc_len, gene_off, gene_len, ref_off, ref_len, alt_off, alt_len;
    gtars_hgvs_position pos[4];
    uint32_t count;
    uint8_t ref_type, loc, edit, flags;
} gtars_hgvs_row;
/* Parsed rows as columns of n entries, host or device memory.  pre: 0, or the status parsing and the accession lookup
 * left; kind / loc / edit as in a row; flags: bit 1 a reference allele, bit 2 uncertain, bit 3 / bit 4 the first / second
 * position is c.*N; tx: the transcript's index in the store for c. and n., the chromosome id of the assembly for g.
 * (2^32 - 1: unknown); base1 / off1: the single position or the range's start, base2 / off2: the range's end; the alleles
 * of row i are text[text_off[i] + ref_off[i], + ref_len[i]) and text[text_off[i] + alt_off[i], + alt_len[i]). */
typedef struct gtars_hgvs_columns {
    uint8_t *pre, *kind, *loc, *edit, *flags;
    uint32_t *tx;
    int64_t *base1, *off1, *base2, *off2;
    uint64_t *text_off;
    uint32_t *ref_off, *ref_len, *alt_off, *alt_len;
    const uint8_t *text;
    uint64_t text_bytes;
    uint64_t n;
} gtars_hgvs_columns;

/* Row statuses: 0 ok, 1 parse error, 2 unsupported reference type (m. r. p.), 3 unsupported edit (inv, unknown, copy,
 * repeat, whole-sequence, uncertain position range), 4 transcript not found, 5 no MANE transcript, 6 unknown chromosome,
 * 7 mapping error (detail: the status of gtars_txbind_map), 8 out of bounds, 9 inconsistent edit, 10 ref mismatch,
 * 11 normalize error (detail: the status of gtars_vrs_alleles).  status_name: NULL past the last one.
 * parse: the nucleotide grammar of parser.rs over text[0, len); *status 0, 1 (then *err_pos is the byte position and
 * err_text, of err_cap bytes, the message of the error) or 2 for a protein expression, whose positions and edit are not
 * parsed.  looks_like_gene_symbol: bridge.rs:552-589. */
const char *gtars_hgvs_status_name(uint32_t status);
gtars_status gtars_hgvs_parse(const char *text, uint64_t len, gtars_hgvs_row *row, uint8_t *status, uint64_t *err_pos, char *err_text,
                              uint64_t err_cap);
int gtars_hgvs_looks_like_gene_symbol(const char *accession);
/* The batch calls on a bound store.  Expression i is text[offsets[i], offsets[i + 1]).  The strings are parsed and their
 * accessions looked up on `threads` host threads (0 = gtars_host_threads): a gene symbol through the store's MANE index,
 * the accession of a c. / n. expression through the store's index, the accession of a g. expression as a chromosome name
 * of the assembly or as alias i = alias_pool[alias_offsets[i], alias_offsets[i + 1]) for chromosome id alias_chrom[i]
 * (n_alias may be 0).  resolve stops there and fills the caller's columns (out->text, text_bytes and n are set by it).
 * to_vrs goes on: the span of every row, REF read from the assembly and ALT made from the text, then normalization and the
 * digests of K18.  accessions as for gtars_vrs_alleles.  Outputs of n entries, any may be NULL: status, detail, warnings
 * (bit 0: uncertain expression), the chromosome id (2^32 - 1 for a row that failed), the normalized interval and the 32
 * characters of the Allele digest (zero bytes for a row that failed).  A call never fails for data.
 * on_host != 0: the library's host path, no device; otherwise the kernels of csrc/hgvs.hip and csrc/vrs.hip on the
 * assembly's device (GTARS_ERR_NO_DEVICE without one).
 * ids_device: the same from resolved columns, text and outputs that are device memory (d_digests: n * 32 bytes, 8-byte
 * aligned), queued on `stream`, which is drained before the call returns.  The current device must be the assembly's. */
gtars_status gtars_hgvs_resolve(gtars_txbind_t *b, const uint8_t *text, const uint64_t *offsets, uint64_t n, const uint8_t *alias_pool,
                                const uint64_t *alias_offsets, const uint32_t *alias_chrom, uint64_t n_alias, uint32_t threads,
                                gtars_hgvs_columns *out);
gtars_status gtars_hgvs_to_vrs(gtars_txbind_t *b, const uint8_t *text, const uint64_t *offsets, uint64_t n, const uint8_t *alias_pool,
                               const uint64_t *alias_offsets, const uint32_t *alias_chrom, uint64_t n_alias, const char *accessions,
                               int on_host, uint32_t threads, uint8_t *status, uint8_t *detail, uint8_t *warnings, uint32_t *chrom,
                               uint64_t *start, uint64_t *end, char *digests);
gtars_status gtars_hgvs_ids_device(gtars_txbind_t *b, const gtars_hgvs_columns *d_cols, const char *accessions, uint8_t *d_status,
                                   uint8_t *d_detail, uint8_t *d_warnings, uint32_t *d_chrom, uint64_t *d_start, uint64_t *d_end,
                                   char *d_digests, void *stream);

/* ---- K23: the transcript-anchored bridge (bridge.rs:226-534; csrc/hgvs_tx.hip, csrc/hgvs_tx_core.h) -----------------------
 * The allele of a c. / n. expression on the transcript's own mature mRNA: its anchor is "SQ." + sha512t24u of the mRNA
 * derived from the assembly, coordinates, REF, ALT and the normalization are in mRNA space and in transcript orientation
 * (nothing is reverse-complemented; ALT is taken as written).  g. m. r. p. rows get status 2.  A position that is intronic
 * or outside the mature mRNA gets status 7 with detail 8 (the TX_NOT_EXONIC of gtars_txbind_map); a transcript whose
 * chromosome the assembly lacks 6, one with an exon past the chromosome's end 8, one with bad exons 7 with detail 10.
 * to_transcript_vrs takes the strings (as gtars_hgvs_to_vrs; gene symbols go through the MANE index);
 * transcript_ids_device takes resolved columns, text and outputs that are device memory, queued on `stream`, which is
 * drained before the call returns (the current device must be the assembly's; the digest columns 8-byte aligned).
 * vrs_transcript_ids is the layer under the bridge: allele i lies on the mRNA of transcript tx[i] (index in the store) at
 * 0-based interbase start[i], REF and ALT in the byte pool as for gtars_vrs_alleles; its statuses are gtars_vrs_alleles'
 * (4: no such transcript, or the assembly cannot give its sequence).
 * Outputs of n entries, any may be NULL: status, detail, warnings, the transcript's index (2^32 - 1 for a row the bridge
 * refused), the normalized interval on the mRNA, the 32 characters of the Allele digest and the 32 characters of the
 * anchor's digest (both zero bytes for a row that failed).  A call never fails for data.  on_host != 0: the library's host
 * path, no device. */
gtars_status gtars_hgvs_to_transcript_vrs(gtars_txbind_t *b, const uint8_t *text, const uint64_t *offsets, uint64_t n, int on_host,
                                          uint32_t threads, uint8_t *status, uint8_t *detail, uint8_t *warnings, uint32_t *tx, uint64_t *start,
                                          uint64_t *end, char *digests, char *anchors);
gtars_status gtars_hgvs_transcript_ids_device(gtars_txbind_t *b, const gtars_hgvs_columns *d_cols, uint8_t *d_status, uint8_t *d_detail,
                                              uint8_t *d_warnings, uint32_t *d_tx, uint64_t *d_start, uint64_t *d_end, char *d_digests,
                                              char *d_anchors, void *stream);
gtars_status gtars_vrs_transcript_ids(gtars_txbind_t *b, const uint32_t *tx, const uint64_t *start, const uint8_t *pool, uint64_t pool_bytes,
                                      const uint32_t *ref_off, const uint32_t *ref_len, const uint32_t *alt_off, const uint32_t *alt_len,
                                      uint64_t n, int on_host, uint32_t threads, uint8_t *status, uint64_t *new_start, uint64_t *new_end,
                                      char *digests, char *anchors);

/* ---- K21: refget (gtars-refget/src/digest, store/readonly.rs; csrc/refget.cpp, csrc/refget.hip) -------------------------
 * Scalar calls, host code: md5 gives 32 lower-case hex characters and a NUL; alphabet the class of n bytes read upper-cased
 * (0 dna2bit, 1 dna3bit, 2 dnaio, 3 protein, 4 ASCII; no bytes: dna2bit); class_table the class of every byte value;
 * host_len the GTARS_REFGET_HOST_LEN in force (records longer than this are hashed on the host threads, default 65536).
 *
 * A gtars_seqcol_t holds the records of one FASTA text in file order -- plain or gzip by the magic bytes; text before the
 * first '>' is ignored; the name is the first whitespace-delimited token of the trimmed header, the description the trimmed
 * rest; a sequence line is a line that is not blank, without its trailing ASCII whitespace; a repeated name stays a record
 * of its own.  flags: GTARS_SEQCOL_KEEP_BYTES keeps the sequence data (needed by every call below `digests`),
 * GTARS_SEQCOL_ON_HOST hashes on `threads` host threads (0 = gtars_host_threads) instead of the device,
 * GTARS_SEQCOL_NO_DIGESTS reads names, lengths and FAI data only (no device either).  Without ON_HOST and NO_DIGESTS the
 * records up to host_len bytes are hashed on the current device from an image of those records alone, the longer ones on
 * the host threads meanwhile (GTARS_ERR_NO_DEVICE without a device).
 * record: the strings live as long as the handle; *description NULL without one; FAI data as samtools faidx has them
 * (*has_fai 0 for a record without a sequence line and for gzip input); sha33 / md5_33 empty and *alphabet 5 without
 * digests; *bytes the record's bytes as the file has them (not upper-cased), NULL when they were not kept.
 * digests: seven times 32 characters and a NUL -- the collection digest, the level-1 digests names, sequences, lengths and
 * the ancillary name_length_pairs, sorted_name_length_pairs, sorted_sequences (types.rs:204-347).
 * assembly: an assembly over the kept bytes with one entry per record, owned by the collection (NULL without bytes).
 * substrings: as gtars_refget_substrings_device for host columns; *offsets (n + 1) and *bytes: gtars_free.  on_host != 0:
 * the library's host path, no device.  digest_records: the per-record digests again from the kept bytes, through the
 * collection's full device image (or on the host): n * 32 characters, n * 16 MD5 bytes, n classes, any may be NULL. */
#define GTARS_SEQCOL_KEEP_BYTES 1
#define GTARS_SEQCOL_ON_HOST 2
#define GTARS_SEQCOL_NO_DIGESTS 4
gtars_status gtars_md5(const void *data, uint64_t n, char *out33);
int gtars_refget_alphabet(const void *data, uint64_t n);
void gtars_refget_class_table(uint8_t *out256);
uint32_t gtars_refget_host_len(void);
gtars_status gtars_seqcol_from_fasta(const char *path, int flags, uint32_t threads, gtars_seqcol_t **out);
gtars_status gtars_seqcol_from_fasta_bytes(const void *text, uint64_t n, int flags, uint32_t threads, gtars_seqcol_t **out);
void gtars_seqcol_free(gtars_seqcol_t *c);
uint64_t gtars_seqcol_len(const gtars_seqcol_t *c);
int gtars_seqcol_is_gzip(const gtars_seqcol_t *c);
gtars_assembly_t *gtars_seqcol_assembly(gtars_seqcol_t *c);
gtars_status gtars_seqcol_record(const gtars_seqcol_t *c, uint64_t i, const char **name, const char **description, uint64_t *length,
                                 int *has_fai, uint64_t *fai_offset, uint32_t *line_bases, uint32_t *line_bytes, char *sha33, char *md5_33,
                                 int *alphabet, const uint8_t **bytes);
gtars_status gtars_seqcol_digests(const gtars_seqcol_t *c, char *out7x33);
gtars_status gtars_seqcol_substrings(gtars_seqcol_t *c, const uint32_t *seq, const uint64_t *start, const uint64_t *end, uint64_t n, int on_host,
                                     uint32_t threads, uint8_t *status, uint64_t **offsets, uint8_t **bytes);
gtars_status gtars_seqcol_digest_records(gtars_seqcol_t *c, int on_host, uint32_t threads, char *digests, uint8_t *md5, uint8_t *alphabet);

/* ---- K22: the encoded storage mode and the `.seq` files of a refget store (gtars-refget/src/digest/encoder.rs, alphabet.rs,
 * store/readonly.rs; csrc/refget_pack_core.h, csrc/refget_pack.cpp, csrc/refget_pack.hip) ------------------------------------
 * Scalar calls, host code, no device.  bits: 2 / 3 / 4 / 5 / 8 bits per symbol of alphabet class 0 .. 4, 8 for 5 (Unknown).
 * encode: n bytes -> ceil(n * bits / 8) packed bytes, MSB first, the unused low bits of the last byte zero; *n_bytes is set
 * and more than `cap` is GTARS_ERR_CAPACITY ("need N").  2-bit: T C A G = 0 .. 3, others 0; 3-bit: A C G T N R Y = 0 .. 6,
 * others 7; IUPAC: A 1, C 2, G 4, T and U 8, R 5, Y 10, S 6, W 9, K 7, M 3, B 12, D 13, H 14, V 15, N and others 0; protein:
 * the position in ACDEFGHIKLMNPQRSTVWY*X-., others 0; 8-bit: the byte upper-cased.  Both letter cases encode alike.
 * decode: symbols [start, end) of an encoding of which `packed` holds bytes [byte_offset, byte_offset + n_packed); bits
 * outside that window read as zero; end <= start writes nothing; out: end - start characters.  The tables: TCAG, ACGTNRYX,
 * NACMGRSKTWYDBHVV (no inverse of the encoding: D comes back as H, H as V, U as T), ACDEFGHIKLMNPQRSTVWY*X-. with X for
 * codes 24 .. 31, and the code itself.  byte_range: the bytes [*b0, *b1) of an encoding that hold symbols [start, end).
 *
 * A gtars_seqpack_t is the packed image of a collection: record r at a 16-byte-aligned offset, ceil(length * bits / 8) bytes
 * at the width of its own class, at least 16 zero bytes behind it; kept on the host and, from the first device call on, on
 * the device current then (every later device call must run there).
 * from_seqcol: from a collection read with its sequence data; alphabet: one class per record, NULL = the classes of the
 * collection's digests.  on_host == 0: k_refget_pack packs the collection's raw device image (built on the current device
 * if it is not yet) in one launch; on_host != 0: the same text on `threads` host threads, no device.
 * from_files: record i is the whole file paths[i], read on the host threads and uploaded as it is -- nothing is decoded on
 * the host; a file whose size is not ceil(length[i] * bits / 8) is GTARS_ERR_PARSE naming it.  from_buffers: the same from
 * host memory.  write_files: each record's exact packed bytes into paths[i] (NULL: skipped).  record: the host copy of one
 * record's packed bytes (valid while the handle lives), its length and class.
 * substrings / decode_records: as gtars_seqcol_substrings, the rows decoded from the packed image (k_refget_fill_packed);
 * decode_records is every record from 0 to its length.  *offsets and *bytes: gtars_free.  on_host != 0: the host threads.
 *
 * A Raw store's `.seq` files are upper-case text: gtars_seqcol_from_seq_files reads them (a file whose size is not length[i]
 * is GTARS_ERR_PARSE) and gtars_seqcol_from_buffers takes host memory into a collection with its bytes kept and no digests,
 * the records named by their numbers; gtars_seqcol_write_files writes every record's upper-cased bytes (NULL: skipped). */
typedef struct gtars_seqpack gtars_seqpack_t;
uint32_t gtars_refget_bits(int alphabet);
gtars_status gtars_refget_encode(const void *seq, uint64_t n, int alphabet, uint8_t *out, uint64_t cap, uint64_t *n_bytes);
gtars_status gtars_refget_decode(const uint8_t *packed, uint64_t n_packed, uint64_t byte_offset, uint64_t start, uint64_t end, int alphabet,
                                 uint8_t *out);
void gtars_refget_byte_range(uint64_t start, uint64_t end, uint32_t bits, uint64_t *b0, uint64_t *b1);
gtars_status gtars_seqpack_from_seqcol(gtars_seqcol_t *c, const uint8_t *alphabet, int on_host, uint32_t threads, gtars_seqpack_t **out);
gtars_status gtars_seqpack_from_files(const char *const *paths, const uint64_t *length, const uint8_t *alphabet, uint64_t n, uint32_t threads,
                                      gtars_seqpack_t **out);
gtars_status gtars_seqpack_from_buffers(const uint8_t *const *packed, const uint64_t *n_packed, const uint64_t *length, const uint8_t *alphabet,
                                        uint64_t n, gtars_seqpack_t **out);
void gtars_seqpack_free(gtars_seqpack_t *p);
uint64_t gtars_seqpack_len(const gtars_seqpack_t *p);
int gtars_seqpack_device(const gtars_seqpack_t *p);
uint64_t gtars_seqpack_image_bytes(const gtars_seqpack_t *p);
gtars_status gtars_seqpack_record(const gtars_seqpack_t *p, uint64_t i, const uint8_t **bytes, uint64_t *n_bytes, uint64_t *length, int *alphabet);
gtars_status gtars_seqpack_write_files(const gtars_seqpack_t *p, const char *const *paths, uint32_t threads);
gtars_status gtars_seqpack_substrings(gtars_seqpack_t *p, const uint32_t *seq, const uint64_t *start, const uint64_t *end, uint64_t n,
                                      int on_host, uint32_t threads, uint8_t *status, uint64_t **offsets, uint8_t **bytes);
gtars_status gtars_seqpack_decode_records(gtars_seqpack_t *p, int on_host, uint32_t threads, uint64_t **offsets, uint8_t **bytes);
gtars_status gtars_seqcol_from_seq_files(const char *const *paths, const uint64_t *length, uint64_t n, uint32_t threads, gtars_seqcol_t **out);
gtars_status gtars_seqcol_from_buffers(const uint8_t *const *seq, const uint64_t *length, uint64_t n, gtars_seqcol_t **out);
gtars_status gtars_seqcol_write_files(const gtars_seqcol_t *c, const char *const *paths, uint32_t threads);

#ifdef __cplusplus
}
#endif
#endif
