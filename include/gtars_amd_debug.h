/*
 * gtars_amd_debug.h -- test, A/B and diagnostics hooks of libgtars_amd.so.  NOT part of the drop-in boundary
 * (include/gtars_amd.h, include/gtars_amd_host.h): nothing a binding of the reference's API needs is declared here, and
 * these entry points may change with the kernels they look into.  Same status / error conventions as gtars_amd.h.
 */
#ifndef GTARS_AMD_DEBUG_H
#define GTARS_AMD_DEBUG_H

#include "gtars_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test / diagnostics hook: launches `workgroups` workgroups of 1024 threads that each hold `lds_bytes` of LDS and spin
 * for `microseconds` on `stream` -- a stand-in for foreign work that occupies CUs while a tokenizer launch runs on
 * another stream (tests/test_gpu_parity.py: the chained scan must complete with the right result whatever is resident). */
gtars_status gtars_debug_occupy_device(void *stream, uint32_t workgroups, uint32_t lds_bytes, uint32_t microseconds);

/* Test / A-B hook.  The library reads its GTARS_* environment switches (test and ablation knobs: GTARS_IGD_SWEEP_MIN,
 * GTARS_NO_LDS_PATH, GTARS_HOST_THREADS ...) ONCE, into an immutable snapshot taken at first use -- never with a getenv per
 * call, which races with a host program's setenv.  A process that changes a switch afterwards calls this to make the library take
 * a new snapshot; no other library call may be in flight. */
void gtars_debug_reload_env(void);

/* Test hook for the handles' device affinity (gtars_index_device): overwrite the device id a handle records -- of an index
 * (and its flat companion) when is_igd == 0, of an IGD (and its pieces view) otherwise -- and return the previous one.  The
 * handle's memory does not move: a forged id makes `*_device` entry points refuse the call and host-buffer entry points try
 * to switch to that device, which is what tests/test_gpu_parity.py asserts on a one-GPU box.  Put the real id back before
 * any other use. */
int gtars_debug_set_handle_device(void *handle, int is_igd, int device);
/* The same for the device image of an assembly handle (gtars_assembly_t *, include/gtars_amd_host.h): -1 when the image
 * is not built yet.  tests/test_gpu_vrs.py. */
int gtars_debug_set_assembly_device(void *assembly, int device);
/* The pinned staging blocks that the builds of assembly images have sent to the device so far, over all assemblies (csrc/
 * seqstats.hip: assembly_build; the block's size is GTARS_SEQ_STAGE_BYTES).  Never reset: tests/test_gpu_seq_stage.py reads it
 * around a build to prove that the build went round the fill loop as often as its block size says. */
uint64_t gtars_debug_seq_stage_blocks(void);

/* Test / measurement entry of the device-side DEFLATE decoder (csrc/inflate_dev.hip; the fused fragment pipeline's input stage,
 * gtars-fragsplit/src/split.rs:84-131 reads its files through flate2's MultiGzDecoder): n_streams raw DEFLATE streams (RFC 1951, no
 * gzip header or trailer), one wave each.  ALL pointers are device memory.  Stream i is comp[in_off[i] .. + in_len[i]) -- in_off a
 * multiple of 16, and 32 readable bytes behind every stream -- and is written to out[out_off[i] ..) -- out_off a multiple of 16,
 * capacity out_cap[i] bytes.  out_len[i] = bytes produced, consumed[i] = input bytes used, status[i] = 0 or the reason the decoder
 * refused the stream (1 block type / stored length, 2 code lengths, 3 symbol or distance, 4 input exhausted, 5 capacity).
 * Enqueued on `stream`; returns a gtars_status. */
int gtars_debug_inflate_streams(const void *comp, const uint64_t *in_off, const uint32_t *in_len, void *out, const uint64_t *out_off,
                                const uint32_t *out_cap, uint32_t n_streams, uint32_t *out_len, uint32_t *consumed, uint32_t *status,
                                void *stream);
/* The same decoder as the fused fragment pipeline launches it on the members of BGZF files (GTARS_FRAG_INFLATE=device): in_off and
 * out_off are ANY byte offsets -- the streams and their outputs may lie back to back --, comp is 16-byte aligned and readable for
 * 48 bytes behind the end of every stream, and no byte of out outside [out_off[i], out_off[i] + min(out_len[i], out_cap[i])) is
 * written.  ring_kib: 32 -- the whole window in LDS -- or 8 -- a match source the ring no longer holds is read back from out. */
int gtars_debug_inflate_members(const void *comp, const uint64_t *in_off, const uint32_t *in_len, void *out, const uint64_t *out_off,
                                const uint32_t *out_cap, uint32_t n_streams, uint32_t *out_len, uint32_t *consumed, uint32_t *status,
                                uint32_t ring_kib, void *stream);

/* Test entries of the three device primitives under every index build and set operation (tests/test_gpu_primitives.py).  All
 * pointers are HOST memory; the calls run on the current device's null stream and return when the result is in the caller's
 * buffer.  GTARS_ERR_NO_DEVICE without a device.
 *
 * gtars_debug_sort_perm: the stable radix sort as the index builds and set operations use it (csrc/sort.hip,
 * device_sort_perm_ws).  perm_out[p] = input row of sorted position p, ordered by (chrom, k1, k2, input row) ascending; k2 may
 * be NULL.  Every chrom[i] < n_chrom <= 2^31 - 1: only the bytes that n_chrom - 1 occupies take part in the order.
 *
 * gtars_debug_scan_u32: offsets_out[i] = counts[0] + ... + counts[i - 1] in u64 for i in [0, n] (csrc/kernels.hip,
 * launch_scan_u32_to_u64); offsets_out holds n + 1 values.
 *
 * gtars_debug_seg_max: the segmented max-scan of csrc/setops.hip (seg_max_pass).  A segment head is element 0 and every i with
 * seg[i] != seg[i - 1].  inclusive != 0: out[i] = max of val over [head of i's segment, i]; start is not read and may be NULL.
 * inclusive == 0: out[i] = 1 where i is a head or start[i] > min(max of val over [head, i) + gap, 2^32 - 1), else 0. */
gtars_status gtars_debug_sort_perm(const uint32_t *chrom, const uint32_t *k1, const uint32_t *k2, uint64_t n, uint32_t n_chrom,
                                   uint32_t *perm_out);
gtars_status gtars_debug_scan_u32(const uint32_t *counts, uint64_t n, uint64_t *offsets_out);
gtars_status gtars_debug_seg_max(const uint32_t *seg, const uint32_t *val, const uint32_t *start, uint64_t n, uint32_t gap,
                                 int inclusive, uint32_t *out);

/* Test hooks of the signal summary (csrc/signal.hip, K13; tests/test_gpu_signal.py).
 * gtars_debug_signal_sort_elems: the result columns are sorted in groups of conditions whose rows x conditions stay
 * at or under `elems` (the device sort takes a 32-bit count); sets it for every later summary of the process and
 * returns the previous value, 0 puts the default back.  No summary may be in flight.
 * gtars_debug_signal_split_hits: a query with MORE hits than this is folded by all waves of a workgroup, every wave a
 * slice of the hits, instead of by one lane group. */
uint32_t gtars_debug_signal_sort_elems(uint32_t elems);
uint32_t gtars_debug_signal_split_hits(void);

/* Test hook of the batched tokenizer (csrc/tokbatch.hip, K15; tests/test_gpu_tokbatch.py): the output ids a workgroup of
 * k_set_pack packs per step. */
uint32_t gtars_debug_tokbatch_tile(void);

/* Test hook of the grid-stride launches (csrc/pipeline.h grid_for, csrc/kernels.hip stream_grid; tests/test_gpu_grid_cap.py).
 * GTARS_GRID_CAP = C > 0 lowers the most workgroups either helper hands out to min(its own cap, C), so that an input of a
 * few hundred rows walks a kernel's grid-stride loop several times; unset or 0 changes nothing.  This counter rises by one
 * for every helper call in which the lowered cap, and not the helper's own, cut the grid short: a test reads it around a
 * call to prove that the call ran more than one trip.  Never reset. */
uint64_t gtars_debug_grid_clips(void);

/* (Stamp builds -- tools/build_variant.sh with -DGTARS_TOK_STAMPS=1 / -DIGD_STAMPS=1 -- additionally export
 * gtars_debug_tok_stamps / gtars_debug_route_stamps / gtars_debug_sweep_stamps: s_memtime at the phase boundaries of the tile
 * loops, read by tools/r03_tok_stamps.py, tools/r03_sweep_stamps.py, tools/r05_rank_stamps.py.  The shipped library has none.) */

#ifdef __cplusplus
}
#endif
#endif
