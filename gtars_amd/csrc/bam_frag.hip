// bam_frag.hip -- K26, device half: BAM to deduplicated fragments on K17's window pipeline (bam_pipe.h).
// Per window the rule of bam_frag_core.h for every record and the kept rows compacted into arrays that grow across windows;
// at the end of the file the distinct barcodes ranked (sort by hash, runs, one string per barcode to the host and its rank
// back) and the rows sorted and collapsed.  The handle's accessors, the text and the writer are host code (bam_frag.cpp).
#include "bam_frag.h"
#include "bam_frag_core.h"
#include "bam_pipe.h"

namespace gtars {
namespace {

// the kept rows of the file so far: 32 bytes per row and the barcode's bytes
struct FragView {
    const u32 *ref, *start, *end, *hhi, *hlo, *blen;
    const u64 *boff;  // the barcode's bytes in pool
    const u8 *pool;
};
// the columns of one window's records, before compaction: 8 arrays of n words in one allocation
struct FragTmp {
    u32 *keep, *blen, *ref, *start, *end, *boff, *hhi, *hlo;  // boff: in the window's bytes
};

// One lane per record: the rule, the outcome counters G[BF_KEPT .. BF_EMPTY], and the kept record's row.  err: a record
// whose aux data is malformed (nothing outside the record has been read to find that out).
__global__ void __launch_bounds__(256)
k_bam_frag_rows(const u8 *__restrict__ bytes, const u32 *__restrict__ offs, u32 n, BamFragParams prm, const u32 *__restrict__ ref_len, u32 n_ref,
                u64 hash_mask, FragTmp t, u64 *__restrict__ G, u32 *__restrict__ err) {
    u64 cnt[BF_N_OUTCOMES];
#pragma unroll
    for (int q = 0; q < BF_N_OUTCOMES; ++q) cnt[q] = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u8 *rec = bytes + offs[i];
        BamFragRow row;
        const i32 r = bam_frag_rule(rec, prm, ref_len, n_ref, &row);
        if (r == BF_MALFORMED) atomicOr(err, 1u);
#pragma unroll
        for (int q = 0; q < BF_N_OUTCOMES; ++q) cnt[q] += r == q;
        u32 keep = 0, bl = 0;
        if (r == BF_KEPT) {
            keep = 1, bl = row.cb_len;
            const u8 *cb = rec + row.cb_off;
            u64 h = 0xcbf29ce484222325ull;  // FNV-1a and a mix, as for the names of K17
            for (u32 k = 0; k < bl; ++k) h = (h ^ cb[k]) * 0x100000001b3ull;
            h ^= h >> 32;
            h *= 0xd6e8feb86659fd93ull;
            h ^= h >> 32;
            h &= hash_mask;
            t.ref[i] = (u32)row.ref, t.start[i] = row.start, t.end[i] = row.end;
            t.boff[i] = offs[i] + row.cb_off, t.hhi[i] = (u32)(h >> 32), t.hlo[i] = (u32)h;
        }
        t.keep[i] = keep, t.blen[i] = bl;
    }
#pragma unroll
    for (int q = 0; q < BF_N_OUTCOMES; ++q) wave_add(G + q, cnt[q]);
}

struct FragDst {
    u32 *ref, *start, *end, *hhi, *hlo, *blen;
    u64 *boff;
    u8 *pool;
};
// the window's kept rows behind the `rows` rows and `pool_n` barcode bytes already stored (koff, loff: the exclusive scans
// of keep and blen)
__global__ void __launch_bounds__(256)
k_bam_frag_append(const u8 *__restrict__ bytes, u32 n, FragTmp t, const u64 *__restrict__ koff, const u64 *__restrict__ loff, u64 rows, u64 pool_n,
                  FragDst d) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        if (!t.keep[i]) continue;
        const u64 j = rows + koff[i], o = pool_n + loff[i];
        const u32 bl = t.blen[i];
        d.ref[j] = t.ref[i], d.start[j] = t.start[i], d.end[j] = t.end[i], d.hhi[j] = t.hhi[i], d.hlo[j] = t.hlo[i], d.blen[j] = bl;
        d.boff[j] = o;
        const u8 *src = bytes + t.boff[i];
        for (u32 k = 0; k < bl; ++k) d.pool[o + k] = src[k];
    }
}

// bytewise, a prefix before the longer barcode
__device__ __forceinline__ int frag_cb_cmp(const FragView &v, u32 a, u32 b) {
    const u32 la = v.blen[a], lb = v.blen[b];
    const u8 *pa = v.pool + v.boff[a], *pb = v.pool + v.boff[b];
    const u32 l = min(la, lb);
    for (u32 k = 0; k < l; ++k)
        if (pa[k] != pb[k]) return pa[k] < pb[k] ? -1 : 1;
    return la < lb ? -1 : la > lb;
}

// Rows in hash order.  head[j]: sorted row j opens a run of equal hash; first[j]: it opens a run of one barcode, given that
// equal barcodes of a run stand together (they do once k_bam_frag_fix_runs has run, or when no run is mixed).  *mixed: some
// run of equal hash holds different barcodes.
__global__ void __launch_bounds__(256)
k_bam_frag_runs(const u32 *__restrict__ perm, FragView v, u32 m, u32 *__restrict__ head, u32 *__restrict__ first, u32 *__restrict__ mixed) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x) {
        bool h = j == 0, d = false;
        if (!h) {
            const u32 a = perm[j], b = perm[j - 1];
            h = v.hhi[a] != v.hhi[b] || v.hlo[a] != v.hlo[b];
            d = !h && frag_cb_cmp(v, a, b) != 0;
        }
        head[j] = h, first[j] = h || d;
        if (d) atomicOr(mixed, 1u);
    }
}

// The result may not depend on the hash: a run of equal hash that holds different barcodes is put into byte order by the lane
// of its head, as k_bam_fix_runs does for names.  A lane writes perm only inside its own run.
__global__ void __launch_bounds__(256) k_bam_frag_fix_runs(u32 *__restrict__ perm, const u32 *__restrict__ head, FragView v, u32 m) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x) {
        if (!head[j]) continue;
        u64 e = j + 1;
        bool mixed = false;
        for (; e < m && !head[e]; ++e) mixed = mixed || frag_cb_cmp(v, perm[j], perm[e]) != 0;
        if (!mixed) continue;
        for (u64 a = j + 1; a < e; ++a) {
            const u32 x = perm[a];
            u64 b = a;
            for (; b > j && frag_cb_cmp(v, perm[b - 1], x) > 0; --b) perm[b] = perm[b - 1];
            perm[b] = x;
        }
    }
}

// one representative row per distinct barcode d = doff[j] of a run's first row j, and its length
__global__ void __launch_bounds__(256)
k_bam_frag_reps(const u32 *__restrict__ perm, const u32 *__restrict__ first, const u64 *__restrict__ doff, FragView v, u32 m, u32 *__restrict__ rep,
                u32 *__restrict__ rep_len) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x) {
        if (!first[j]) continue;
        const u32 r = perm[j];
        rep[doff[j]] = r, rep_len[doff[j]] = v.blen[r];
    }
}
__global__ void __launch_bounds__(256)
k_bam_frag_rep_bytes(const u32 *__restrict__ rep, const u64 *__restrict__ roff, FragView v, u32 n_distinct, u8 *__restrict__ out) {
    for (u64 d = (u64)blockIdx.x * blockDim.x + threadIdx.x; d < n_distinct; d += (u64)gridDim.x * blockDim.x) {
        const u32 r = rep[d], bl = v.blen[r];
        const u8 *src = v.pool + v.boff[r];
        for (u32 k = 0; k < bl; ++k) out[roff[d] + k] = src[k];
    }
}
// every row's barcode id: the rank of its distinct barcode
__global__ void __launch_bounds__(256)
k_bam_frag_ids(const u32 *__restrict__ perm, const u64 *__restrict__ doff, const u32 *__restrict__ rank, u32 m, u32 *__restrict__ bid) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x) bid[perm[j]] = rank[doff[j + 1] - 1];
}

// rows in (ref, start, end, barcode id) order: head[j] = sorted row j opens a run of equal tuples
__global__ void __launch_bounds__(256)
k_bam_frag_tuple_heads(const u32 *__restrict__ perm, const u32 *__restrict__ ref, const u32 *__restrict__ start, const u32 *__restrict__ end,
                       const u32 *__restrict__ bid, u32 m, u32 *__restrict__ head) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x) {
        bool h = j == 0;
        if (!h) {
            const u32 a = perm[j], b = perm[j - 1];
            h = ref[a] != ref[b] || start[a] != start[b] || end[a] != end[b] || bid[a] != bid[b];
        }
        head[j] = h;
    }
}
// the output row toff[j] of every run's head j: its columns and where the run begins (at[n_rows] = m closes the last run)
__global__ void __launch_bounds__(256)
k_bam_frag_write(const u32 *__restrict__ perm, const u32 *__restrict__ head, const u64 *__restrict__ toff, const u32 *__restrict__ ref,
                 const u32 *__restrict__ start, const u32 *__restrict__ end, const u32 *__restrict__ bid, u32 m, u32 *__restrict__ o_ref,
                 u32 *__restrict__ o_start, u32 *__restrict__ o_end, u32 *__restrict__ o_bid, u32 *__restrict__ at) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x) {
        if (j == 0) at[toff[m]] = m;
        if (!head[j]) continue;
        const u64 r = toff[j];
        const u32 a = perm[j];
        o_ref[r] = ref[a], o_start[r] = start[a], o_end[r] = end[a], o_bid[r] = bid[a], at[r] = (u32)j;
    }
}
__global__ void __launch_bounds__(256) k_bam_frag_counts(const u32 *__restrict__ at, u32 n_rows, u32 *__restrict__ count) {
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (u64)gridDim.x * blockDim.x) count[r] = at[r + 1] - at[r];
}

struct FragState {
    hipStream_t st;
    const BamFile &f;
    BamFragParams prm;
    u64 hash_mask;
    Grow<u32> ref, start, end, hhi, hlo, blen;
    Grow<u64> boff;
    Grow<u8> pool;
    u64 rows = 0, pool_n = 0;
    DevBuf<u64> G;
    DevBuf<u32> err, ref_len;
    FragState(hipStream_t s, const BamFile &file, const BamFragParams &p) : st(s), f(file), prm(p) {
        const u64 bits = (u64)std::min<long>(std::max<long>(cfg_int("GTARS_BAM_CB_HASH_BITS", 64), 0), 64);
        hash_mask = bits >= 64 ? ~0ull : (1ull << bits) - 1ull;
    }

    FragView view() const { return FragView{ref.b.p, start.b.p, end.b.p, hhi.b.p, hlo.b.p, blen.b.p, boff.b.p, pool.b.p}; }

    gtars_status init() {
        GT_TRY(G.alloc(BF_N_OUTCOMES));
        GT_HIP(hipMemsetAsync(G.p, 0, BF_N_OUTCOMES * sizeof(u64), st));
        GT_TRY(err.alloc(1));
        GT_HIP(hipMemsetAsync(err.p, 0, 4, st));
        std::vector<u32> len(f.refs.size());
        for (size_t k = 0; k < len.size(); ++k) len[k] = f.refs[k].len;
        GT_TRY(ref_len.upload(len));
        return GTARS_OK;
    }

    // the n records of a window whose first record is record rec0 of the file
    gtars_status append(const u8 *d_bytes, const u32 *d_offs, u32 n, u64 rec0) {
        StreamFrame fr(st);
        u32 *tmp;
        GT_TRY(fr.alloc(&tmp, (size_t)n * 8));
        const size_t s = n;
        const FragTmp t{tmp, tmp + s, tmp + 2 * s, tmp + 3 * s, tmp + 4 * s, tmp + 5 * s, tmp + 6 * s, tmp + 7 * s};
        {
            ProfScope p("k_bam_frag_rows", st);
            GT_TRY(launch_over(st, n, k_bam_frag_rows, d_bytes, d_offs, n, prm, ref_len.p, (u32)f.refs.size(), hash_mask, t, G.p, err.p));
        }
        u32 e = 0;
        GT_TRY(fr.download(&e, err.p, 1));
        u64 *koff, *loff, kept = 0, nbytes = 0;
        GT_TRY(scan_total(fr, t.keep, n, &koff, &kept));
        if (e)
            return fail(GTARS_ERR_PARSE, f.path + ": a BAM record among records " + std::to_string(rec0) + " .. " + std::to_string(rec0 + n - 1) +
                                             " holds malformed aux data");
        if (!kept) return GTARS_OK;
        if (rows + kept > 0xFFFFFFFEull) return fail(GTARS_ERR_INVALID_ARG, f.path + ": more than 2^32 - 2 kept pairs");
        if (prm.use_tag) GT_TRY(scan_total(fr, t.blen, n, &loff, &nbytes));
        else loff = koff;  // (every length is 0: nothing is copied, and no offset is read afterwards)
        for (Grow<u32> *g : {&ref, &start, &end, &hhi, &hlo, &blen}) GT_TRY(g->ensure(rows + kept, rows, st));
        GT_TRY(boff.ensure(rows + kept, rows, st));
        GT_TRY(pool.ensure(pool_n + nbytes, pool_n, st));
        ProfScope p("k_bam_frag_append", st);
        GT_TRY(launch_over(st, n, k_bam_frag_append, d_bytes, n, t, koff, loff, rows, pool_n,
                           FragDst{ref.b.p, start.b.p, end.b.p, hhi.b.p, hlo.b.p, blen.b.p, boff.b.p, pool.b.p}));
        rows += kept, pool_n += nbytes;
        return fr.drain();
    }

    // the barcode id of every row into bid[rows], the barcodes in id order into names
    gtars_status rank_barcodes(u32 *bid, std::vector<std::string> &names) {
        const u32 m = (u32)rows;
        const FragView v = view();
        StreamFrame fr(st);
        u32 *perm, *head, *first, *mixed;
        {
            ProfScope p("bam_frag_sort_hash", st);
            GT_TRY(sort_perm(fr, v.hhi, v.hhi, v.hlo, m, 1, &perm));
        }
        GT_TRY(fr.alloc(&head, m));
        GT_TRY(fr.alloc(&first, m));
        GT_TRY(fr.alloc(&mixed, 1));
        GT_HIP(hipMemsetAsync(mixed, 0, 4, st));
        u64 *doff, n_distinct = 0;
        for (int round = 0;; ++round) {
            u32 mx = 0;
            {
                ProfScope p("k_bam_frag_runs", st);
                GT_TRY(launch_over(st, m, k_bam_frag_runs, perm, v, m, head, first, mixed));
            }
            GT_TRY(fr.download(&mx, mixed, 1));
            GT_TRY(scan_total(fr, first, m, &doff, &n_distinct));
            if (!mx || round == 1) break;
            // some run of equal hash is mixed: order those runs by their bytes, then find the barcode runs again
            ProfScope p("k_bam_frag_fix_runs", st);
            GT_TRY(launch_over(st, m, k_bam_frag_fix_runs, perm, head, v, m));
        }
        const u32 nd = (u32)n_distinct;
        u32 *rep, *rep_len, *rank;
        u64 *roff, rep_bytes = 0;
        u8 *rb;
        GT_TRY(fr.alloc(&rep, nd));
        GT_TRY(fr.alloc(&rep_len, nd));
        {
            ProfScope p("k_bam_frag_reps", st);
            GT_TRY(launch_over(st, m, k_bam_frag_reps, perm, first, doff, v, m, rep, rep_len));
        }
        GT_TRY(scan_total(fr, rep_len, nd, &roff, &rep_bytes));
        GT_TRY(fr.alloc(&rb, rep_bytes));
        {
            ProfScope p("k_bam_frag_rep_bytes", st);
            GT_TRY(launch_over(st, nd, k_bam_frag_rep_bytes, rep, roff, v, nd, rb));
        }
        std::vector<u64> h_off;
        std::vector<u8> h_bytes;
        GT_TRY(fr.download(h_off, roff, (size_t)nd + 1));
        GT_TRY(fr.download(h_bytes, rb, rep_bytes));
        GT_TRY(fr.drain());
        // the host puts the distinct barcodes into byte order (a prefix before the longer string): rank[d] is d's barcode id
        std::vector<u32> order(nd), h_rank(nd);
        for (u32 d = 0; d < nd; ++d) order[d] = d;
        auto less = [&](u32 a, u32 b) {
            const size_t la = h_off[a + 1] - h_off[a], lb = h_off[b + 1] - h_off[b];
            const int c = memcmp(h_bytes.data() + h_off[a], h_bytes.data() + h_off[b], std::min(la, lb));
            return c ? c < 0 : la < lb;
        };
        std::sort(order.begin(), order.end(), less);
        names.resize(nd);
        for (u32 k = 0; k < nd; ++k) {
            h_rank[order[k]] = k;
            names[k].assign((const char *)h_bytes.data() + h_off[order[k]], h_off[order[k] + 1] - h_off[order[k]]);
        }
        GT_TRY(fr.upload(&rank, h_rank.data(), nd));
        ProfScope p("k_bam_frag_ids", st);
        GT_TRY(launch_over(st, m, k_bam_frag_ids, perm, doff, rank, m, bid));
        return fr.drain();
    }

    // order, collapse and download: the handle's columns, barcodes and statistics
    gtars_status finish(gtars_bam_frags &out, const std::string &sample) {
        u64 Gh[BF_N_OUTCOMES];
        GT_HIP(hipMemcpyAsync(Gh, G.p, sizeof Gh, hipMemcpyDeviceToHost, st));
        GT_HIP(hipStreamSynchronize(st));
        u64 records = 0;
        for (int q = 0; q < BF_N_OUTCOMES; ++q) records += Gh[q];
        for (int q = BF_UNPLACED; q <= BF_EMPTY; ++q) out.stats[q] = Gh[q];  // (the reasons in the rule's order)
        out.stats[0] = records, out.stats[9] = Gh[BF_KEPT];
        if (Gh[BF_KEPT] != rows) return fail(GTARS_ERR_INTERNAL, "K26: the kept counter and the stored rows differ");
        const u32 m = (u32)rows;
        if (!m) return GTARS_OK;
        DevBuf<u32> bid;
        GT_TRY(bid.alloc(m));
        if (prm.use_tag) {
            GT_TRY(rank_barcodes(bid.p, out.barcodes));
        } else {
            GT_HIP(hipMemsetAsync(bid.p, 0, (size_t)m * 4, st));
            out.barcodes.assign(1, sample);
        }
        StreamFrame fr(st);
        // stable passes, the minor key first: the barcode id, then (ref as segment, start, end)
        const u32 *c_ref = ref.b.p, *c_start = start.b.p, *c_end = end.b.p, *c_bid = bid.p;
        if (out.barcodes.size() > 1) {
            ProfScope p("bam_frag_sort_rows", st);
            u32 *p1, *g[4];
            const u32 *src[4] = {c_ref, c_start, c_end, c_bid};
            GT_TRY(sort_perm(fr, c_bid, c_bid, nullptr, m, 1, &p1));
            for (int k = 0; k < 4; ++k) {
                GT_TRY(fr.alloc(&g[k], m));
                GT_TRY(device_gather_u32(src[k], p1, m, g[k], st));
            }
            c_ref = g[0], c_start = g[1], c_end = g[2], c_bid = g[3];
        }
        u32 *p2, *head;
        {
            ProfScope p("bam_frag_sort_rows", st);
            GT_TRY(sort_perm(fr, c_ref, c_start, c_end, m, (u32)f.refs.size(), &p2));
        }
        GT_TRY(fr.alloc(&head, m));
        {
            ProfScope p("k_bam_frag_tuple_heads", st);
            GT_TRY(launch_over(st, m, k_bam_frag_tuple_heads, p2, c_ref, c_start, c_end, c_bid, m, head));
        }
        u64 *toff, n_rows = 0;
        GT_TRY(scan_total(fr, head, m, &toff, &n_rows));
        const u32 R = (u32)n_rows;
        u32 *o[5], *at;
        for (int k = 0; k < 5; ++k) GT_TRY(fr.alloc(&o[k], R));
        GT_TRY(fr.alloc(&at, (size_t)R + 1));
        {
            ProfScope p("k_bam_frag_write", st);
            GT_TRY(launch_over(st, m, k_bam_frag_write, p2, head, toff, c_ref, c_start, c_end, c_bid, m, o[0], o[1], o[2], o[3], at));
            GT_TRY(launch_over(st, R, k_bam_frag_counts, at, R, o[4]));
        }
        out.ref.resize(R);
        GT_TRY(fr.download((u32 *)out.ref.data(), o[0], R));
        GT_TRY(fr.download(out.start, o[1], R));
        GT_TRY(fr.download(out.end, o[2], R));
        GT_TRY(fr.download(out.barcode, o[3], R));
        GT_TRY(fr.download(out.count, o[4], R));
        GT_TRY(fr.drain());
        out.stats[10] = R, out.stats[11] = out.barcodes.size();
        return GTARS_OK;
    }
};

gtars_status bam_fragments(const gtars_bam &h, const BamFragParams &prm, const std::string &sample, u64 max_window, unsigned threads,
                           gtars_bam_frags &out) {
    const double t_enter = now_s();
    GT_TRY(require_device());
    hipStream_t st = nullptr;
    FragState q(st, h.f, prm);  // (declared before the pipe, like the QC's state)
    GT_TRY(q.init());
    BamPipe pipe(h.f, max_window, threads, st);
    GT_TRY(pipe.run([&](const BamCols &, u32 n, const BamSegs &, u64 rec0, const u8 *d_bytes) -> gtars_status {
        return q.append(d_bytes, pipe.d_offs.p, n, rec0);
    }));
    GT_TRY(q.finish(out, sample));
    g_bam_stages[0] = h.t_open, g_bam_stages[5] = now_s() - t_enter;
    return GTARS_OK;
}

}  // namespace
}  // namespace gtars

using namespace gtars;

extern "C" {

gtars_status gtars_bam_fragments(const gtars_bam_t *b, const gtars_bam_frag_params *params, uint64_t max_window_bytes, uint32_t threads,
                                 gtars_bam_frags_t **out) {
    return guarded([&]() -> gtars_status {
        if (!b || !params || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        BamFragParams p;
        std::string sample;
        p.use_tag = params->use_barcode_tag != 0;
        p.tag[0] = (u8)params->barcode_tag[0], p.tag[1] = (u8)params->barcode_tag[1];
        if (p.use_tag && (!p.tag[0] || !p.tag[1])) return fail(GTARS_ERR_INVALID_ARG, "barcode_tag must be two bytes");
        if (!p.use_tag) {
            sample = params->sample ? params->sample : "";
            if (sample.empty() || sample.find_first_of(" \t\n\r\v\f") != std::string::npos)
                return fail(GTARS_ERR_INVALID_ARG, "sample must not be empty and must hold no white space");
        }
        if (params->min_mapq < 0) return fail(GTARS_ERR_INVALID_ARG, "min_mapq must not be negative");
        if (params->max_fragment_length < 1) return fail(GTARS_ERR_INVALID_ARG, "max_fragment_length must be at least 1");
        p.min_mapq = (u32)params->min_mapq, p.max_fragment_length = params->max_fragment_length;
        p.shift_left = params->shift_left, p.shift_right = params->shift_right;
        p.require_flags = params->require_flags, p.exclude_flags = params->exclude_flags;
        std::unique_ptr<gtars_bam_frags> h(new gtars_bam_frags);
        GT_TRY(bam_fragments(*b, p, sample, window_bytes(max_window_bytes), threads, *h));
        *out = h.release();
        return GTARS_OK;
    });
}

}  // extern "C"
