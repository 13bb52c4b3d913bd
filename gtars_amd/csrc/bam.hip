// bam.hip -- K17, device half: the window pipeline over a BAM file's inflated bytes, k_bam_decode (one lane
// per record) -- both in bam_pipe.h, which K26 (bam_frag.hip) shares -- and the library-complexity QC of
// gtars-uniwig/src/bamqc.rs:68-245 as decode, sort, run lengths and a join.
// The host threads inflate (bam.cpp) and walk the records' block_size chain; every other field is read here.
#include "bam_pipe.h"

namespace gtars {

thread_local double g_bam_stages[6];

namespace {

// ---- QC -----------------------------------------------------------------------------------------------------------------
// the counters, u64 on the device
enum { G_TOTAL, G_DUPS, G_MITO, G_PAIRS, G_DISTINCT, G_M1, G_M2, G_PAIRED, G_N1, G_N2, G_COUNT };
// what a record of the current chromosome is to the QC
enum : u32 { SEG_READ1 = 0, SEG_READ2 = 1, SEG_SINGLE = 2, SEG_DROPPED = 3 };

// bamqc.rs:99-142 for the records [r0, r1) of a window, all of one reference: the three totals, and per record its entry at
// base + (i - r0): seg (which table, or single / dropped), the two key words it contributes, its name hash and -- for a table
// entry -- nl[i - r0] = the name bytes to keep.  mito: the reference is mitochondrial, nothing is written.
__global__ void __launch_bounds__(256)
k_bam_classify(BamCols c, u32 r0, u32 r1, int mito, u64 base, u32 *__restrict__ seg, u32 *__restrict__ kpos, u32 *__restrict__ ka,
               u32 *__restrict__ hhi, u32 *__restrict__ hlo, u32 *__restrict__ nlen, u32 *__restrict__ nl, u64 *__restrict__ G) {
    u64 tot = 0, dup = 0, mt = 0, n1 = 0, n2 = 0, paired = 0;
    for (u64 i = (u64)r0 + (u64)blockIdx.x * blockDim.x + threadIdx.x; i < r1; i += (u64)gridDim.x * blockDim.x) {
        const u32 flag = c.flag[i];
        const i32 mapq = c.mapq[i], pos = c.pos[i];
        u32 sg = SEG_DROPPED, kp = 0, kb = 0, keep = 0;
        if (!(mapq != 255 && mapq < 30) && !(flag & 0x4u)) {
            ++tot;
            if (flag & 0x400u) ++dup;
            if (mito) {
                ++mt;
            } else if (pos != -1) {
                if (flag & 0x1u) {
                    paired = 1;
                    if (!(flag & FLAG_NAME_MISSING)) {
                        if (flag & 0x40u) sg = SEG_READ1, ++n1;
                        else if (flag & 0x80u) sg = SEG_READ2, ++n2;
                    }
                    if (sg != SEG_DROPPED) kp = (u32)pos + 1u, kb = (u32)c.tlen[i], keep = c.nlen[i];
                } else {
                    sg = SEG_SINGLE, kp = (u32)pos + 1u, kb = (u32)c.lseq[i];
                }
            }
        }
        if (!mito) {
            const u64 o = base + (i - r0);
            seg[o] = sg, kpos[o] = kp, ka[o] = kb, hhi[o] = c.hhi[i], hlo[o] = c.hlo[i], nlen[o] = keep;
            nl[i - r0] = keep;
        }
    }
    wave_add(G + G_TOTAL, tot);
    wave_add(G + G_DUPS, dup);
    wave_add(G + G_MITO, mt);
    wave_add(G + G_N1, n1);
    wave_add(G + G_N2, n2);
    wave_add(G + G_PAIRED, paired);
}

// the kept names of the records [r0, r0 + cnt) to names[name_base + off[j] ...), and where each went
__global__ void __launch_bounds__(256)
k_bam_names(const u8 *__restrict__ bytes, BamCols c, u32 r0, u32 cnt, const u64 *__restrict__ off, const u32 *__restrict__ nl, u64 name_base,
            u8 *__restrict__ names, u64 *__restrict__ noff) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < cnt; j += (u64)gridDim.x * blockDim.x) {
        const u64 o = name_base + off[j];
        noff[j] = o;
        const u8 *src = bytes + c.noff[r0 + j];
        for (u32 k = 0; k < nl[j]; ++k) names[o + k] = src[k];
    }
}

// the chromosome's entries and names as the kernels below see them
struct QcView {
    const u32 *seg, *kpos, *ka, *hhi, *hlo, *nlen;
    const u64 *noff;
    const u8 *names;
};
// bytewise, a prefix before the longer name
__device__ __forceinline__ int name_cmp(const QcView &v, u32 a, u32 b) {
    const u32 la = v.nlen[a], lb = v.nlen[b];
    const u8 *pa = v.names + v.noff[a], *pb = v.names + v.noff[b];
    const u32 l = min(la, lb);
    for (u32 k = 0; k < l; ++k)
        if (pa[k] != pb[k]) return pa[k] < pb[k] ? -1 : 1;
    return la < lb ? -1 : la > lb;
}
// (hash, name): the order inside a table once k_bam_fix_runs has run
__device__ __forceinline__ int entry_cmp(const QcView &v, u32 a, u32 b) {
    if (v.hhi[a] != v.hhi[b]) return v.hhi[a] < v.hhi[b] ? -1 : 1;
    if (v.hlo[a] != v.hlo[b]) return v.hlo[a] < v.hlo[b] ? -1 : 1;
    return name_cmp(v, a, b);
}

// head[j]: sorted table entry j opens a run of equal (table, hash)
__global__ void __launch_bounds__(256) k_bam_run_heads(const u32 *__restrict__ perm, QcView v, u32 m, u32 *__restrict__ head) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x) {
        bool h = j == 0;
        if (!h) {
            const u32 a = perm[j], b = perm[j - 1];
            h = v.seg[a] != v.seg[b] || v.hhi[a] != v.hhi[b] || v.hlo[a] != v.hlo[b];
        }
        head[j] = h;
    }
}

// The result may not depend on the hash: a run of equal hash that holds different names is put into name order (stable, so
// file order survives among equal names) by the lane of its head -- an insertion sort, such runs being rare and short.  A lane
// writes perm only inside its own run.
__global__ void __launch_bounds__(256) k_bam_fix_runs(u32 *__restrict__ perm, const u32 *__restrict__ head, QcView v, u32 m) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x) {
        if (!head[j]) continue;
        u64 e = j + 1;
        bool mixed = false;
        for (; e < m && !head[e]; ++e) mixed = mixed || name_cmp(v, perm[j], perm[e]) != 0;
        if (!mixed) continue;
        for (u64 a = j + 1; a < e; ++a) {
            const u32 x = perm[a];
            u64 b = a;
            for (; b > j && name_cmp(v, perm[b - 1], x) > 0; --b) perm[b] = perm[b - 1];
            perm[b] = x;
        }
    }
}

// the key of every record: a single-end read's (pos + 1, l_seq, 0, 0); nothing yet for the others (ks = 1: no key)
__global__ void __launch_bounds__(256)
k_bam_key_init(QcView v, u32 n, u32 *__restrict__ w0, u32 *__restrict__ w1, u32 *__restrict__ w2, u32 *__restrict__ w3, u32 *__restrict__ ks) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const bool single = v.seg[i] == SEG_SINGLE;
        w0[i] = single ? v.kpos[i] : 0u, w1[i] = single ? v.ka[i] : 0u, w2[i] = 0u, w3[i] = 0u;
        ks[i] = single ? 0u : 1u;
    }
}

// bamqc.rs:152-158.  Sorted positions [0, n1) are the read-1 table, [n1, m) the read-2 table, both in (hash, name, file)
// order: the last entry of a run of one name is what HashMap::insert left.  Every read-1 winner looks its name up among the
// read-2 entries (the last entry not behind it); a match is a joined pair, and its key goes to the read-1 record's slot.
__global__ void __launch_bounds__(256)
k_bam_join(const u32 *__restrict__ perm, const u32 *__restrict__ head, QcView v, u32 n1, u32 m, u32 *__restrict__ w0, u32 *__restrict__ w1,
           u32 *__restrict__ w2, u32 *__restrict__ w3, u32 *__restrict__ ks, u64 *__restrict__ G) {
    u64 pairs = 0;
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n1; j += (u64)gridDim.x * blockDim.x) {
        const u32 a = perm[j];
        if (!(j + 1 == n1 || head[j + 1] || name_cmp(v, a, perm[j + 1]) != 0)) continue;
        u32 lo = n1, hi = m;  // first read-2 entry behind a
        while (lo < hi) {
            const u32 mid = lo + ((hi - lo) >> 1);
            if (entry_cmp(v, perm[mid], a) > 0) hi = mid;
            else lo = mid + 1;
        }
        if (lo == n1) continue;
        const u32 b = perm[lo - 1];
        if (entry_cmp(v, b, a) != 0) continue;
        w0[a] = v.kpos[a], w1[a] = v.ka[a], w2[a] = v.kpos[b], w3[a] = v.ka[b];
        ks[a] = 0u;
        ++pairs;
    }
    wave_add(G + G_PAIRS, pairs);
}

// bamqc.rs:210-217 over the keys in sorted order (rows with a key first): a run is one distinct key, its length the count
__global__ void __launch_bounds__(256)
k_bam_key_runs(const u32 *__restrict__ perm, const u32 *__restrict__ ks, const u32 *__restrict__ w0, const u32 *__restrict__ w1,
               const u32 *__restrict__ w2, const u32 *__restrict__ w3, u32 n, u64 *__restrict__ G) {
    u64 distinct = 0, m1 = 0, m2 = 0;
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        const u32 r = perm[j];
        if (ks[r]) continue;
        auto same = [&](u64 k) {  // row k exists, has a key, and it is r's
            if (k >= n) return false;
            const u32 s = perm[k];
            return !ks[s] && w0[s] == w0[r] && w1[s] == w1[r] && w2[s] == w2[r] && w3[s] == w3[r];
        };
        if (j > 0 && same(j - 1)) continue;
        ++distinct;
        if (!same(j + 1)) ++m1;
        else if (!same(j + 2)) ++m2;
    }
    wave_add(G + G_DISTINCT, distinct);
    wave_add(G + G_M1, m1);
    wave_add(G + G_M2, m2);
}

struct QcState {
    hipStream_t st;
    Grow<u32> seg, kpos, ka, hhi, hlo, nlen;
    Grow<u64> noff;
    Grow<u8> names;
    u64 n_c = 0, names_n = 0;  // records and name bytes of the current chromosome
    int32_t cur_ref = INT32_MIN;
    DevBuf<u64> G;
    explicit QcState(hipStream_t s) : st(s) {}

    QcView view() const { return QcView{seg.b.p, kpos.b.p, ka.b.p, hhi.b.p, hlo.b.p, nlen.b.p, noff.b.p, names.b.p}; }

    // the records [r0, r1) of the window, all of reference `ref`
    gtars_status append(const BamFile &f, const BamCols &c, u32 r0, u32 r1, int32_t ref, const u8 *d_bytes) {
        if (ref != cur_ref) {
            GT_TRY(finish_chrom());
            cur_ref = ref;
        }
        if (ref < 0) return GTARS_OK;  // the unplaced tail belongs to no reference
        const u32 cnt = r1 - r0;
        const bool mito = f.mito[(size_t)ref] != 0;
        ProfScope p("bam_qc_append", st);
        if (mito) {
            hipLaunchKernelGGL(k_bam_classify, dim3(grid_for(cnt)), dim3(256), 0, st, c, r0, r1, 1, (u64)0, (u32 *)nullptr, (u32 *)nullptr,
                               (u32 *)nullptr, (u32 *)nullptr, (u32 *)nullptr, (u32 *)nullptr, (u32 *)nullptr, G.p);
            GT_HIP(hipGetLastError());
            return GTARS_OK;
        }
        const u64 need = n_c + cnt;
        if (need > 0xFFFFFFFEull)
            return fail(GTARS_ERR_INVALID_ARG, f.path + ": more than 2^32 - 2 records on reference " + f.refs[(size_t)ref].name);
        for (Grow<u32> *g : {&seg, &kpos, &ka, &hhi, &hlo, &nlen}) GT_TRY(g->ensure(need, n_c, st));
        GT_TRY(noff.ensure(need, n_c, st));
        StreamFrame fr(st);
        u32 *nl;
        GT_TRY(fr.alloc(&nl, cnt));
        hipLaunchKernelGGL(k_bam_classify, dim3(grid_for(cnt)), dim3(256), 0, st, c, r0, r1, 0, n_c, seg.b.p, kpos.b.p, ka.b.p, hhi.b.p, hlo.b.p,
                           nlen.b.p, nl, G.p);
        GT_HIP(hipGetLastError());
        u64 *off, total = 0;
        GT_TRY(scan_total(fr, nl, cnt, &off, &total));
        GT_TRY(names.ensure(names_n + total, names_n, st));
        hipLaunchKernelGGL(k_bam_names, dim3(grid_for(cnt)), dim3(256), 0, st, d_bytes, c, r0, cnt, off, nl, names_n, names.b.p, noff.b.p + n_c);
        GT_HIP(hipGetLastError());
        n_c = need, names_n += total;
        return fr.drain();
    }

    // the tables' join and the key counts of the chromosome that just ended (bamqc.rs:144-160, 210-217)
    gtars_status finish_chrom() {
        const u32 n = (u32)n_c;
        n_c = 0, names_n = 0;
        if (!n) return GTARS_OK;
        ProfScope p("bam_qc_finish", st);
        StreamFrame fr(st);
        u64 nn[2] = {0, 0};
        GT_TRY(fr.download(nn, G.p + G_N1, 2));
        GT_TRY(fr.drain());
        GT_HIP(hipMemsetAsync(G.p + G_N1, 0, 2 * sizeof(u64), st));
        const u32 n1 = (u32)nn[0], m = (u32)(nn[0] + nn[1]);
        const QcView v = view();
        u32 *w0, *w1, *w2, *w3, *ks;
        for (u32 **w : {&w0, &w1, &w2, &w3, &ks}) GT_TRY(fr.alloc(w, n));
        hipLaunchKernelGGL(k_bam_key_init, dim3(grid_for(n)), dim3(256), 0, st, v, n, w0, w1, w2, w3, ks);
        const bool join = n1 && m > n1;
        if (join) {
            u32 *perm, *head;
            GT_TRY(sort_perm(fr, v.seg, v.hhi, v.hlo, n, 4, &perm));
            GT_TRY(fr.alloc(&head, m));
            hipLaunchKernelGGL(k_bam_run_heads, dim3(grid_for(m)), dim3(256), 0, st, perm, v, m, head);
            hipLaunchKernelGGL(k_bam_fix_runs, dim3(grid_for(m)), dim3(256), 0, st, perm, head, v, m);
            hipLaunchKernelGGL(k_bam_join, dim3(grid_for(n1)), dim3(256), 0, st, perm, head, v, n1, m, w0, w1, w2, w3, ks, G.p);
            GT_HIP(hipGetLastError());
        }
        // the keys in (has a key, w0, w1, w2, w3) order: two stable passes, the minor words first -- they are all zero, and
        // their pass is skipped, when no pair was possible
        u32 *perm2;
        if (join) {
            u32 *p1, *g[5], *src[5] = {w0, w1, w2, w3, ks};
            GT_TRY(sort_perm(fr, w2, w2, w3, n, 1, &p1));
            for (int k = 0; k < 5; ++k) {
                GT_TRY(fr.alloc(&g[k], n));
                GT_TRY(device_gather_u32(src[k], p1, n, g[k], st));
            }
            w0 = g[0], w1 = g[1], w2 = g[2], w3 = g[3], ks = g[4];
        }
        GT_TRY(sort_perm(fr, ks, w0, w1, n, 2, &perm2));
        hipLaunchKernelGGL(k_bam_key_runs, dim3(grid_for(n)), dim3(256), 0, st, perm2, ks, w0, w1, w2, w3, n, G.p);
        GT_HIP(hipGetLastError());
        return fr.drain();
    }
};

gtars_status bam_qc(const gtars_bam &h, u64 max_window, unsigned threads, gtars_bam_qc_result *out) {
    const double t_enter = now_s();
    GT_TRY(require_device());
    hipStream_t st = nullptr;
    QcState q(st);  // (declared before the pipe: the pipe's destructor drains the stream while the state's memory is still there)
    GT_TRY(q.G.alloc(G_COUNT));
    GT_HIP(hipMemsetAsync(q.G.p, 0, G_COUNT * sizeof(u64), st));
    BamPipe pipe(h.f, max_window, threads, st);
    GT_TRY(pipe.run([&](const BamCols &c, u32 n, const BamSegs &sg, u64, const u8 *d_bytes) -> gtars_status {
        for (size_t k = 0; k < sg.ref.size(); ++k)
            GT_TRY(q.append(h.f, c, sg.start[k], k + 1 < sg.start.size() ? sg.start[k + 1] : n, sg.ref[k], d_bytes));
        return GTARS_OK;
    }));
    GT_TRY(q.finish_chrom());
    u64 G[G_COUNT];
    GT_HIP(hipMemcpyAsync(G, q.G.p, sizeof G, hipMemcpyDeviceToHost, st));
    GT_HIP(hipStreamSynchronize(st));
    // bamqc.rs:220-244
    const u64 effective = G[G_PAIRED] ? G[G_PAIRS] : G[G_TOTAL] - G[G_MITO];
    out->total_reads = effective, out->distinct = G[G_DISTINCT], out->m1 = G[G_M1], out->m2 = G[G_M2];
    out->dups = G[G_DUPS], out->mito_reads = G[G_MITO];
    out->nrf = (double)G[G_M1] / (double)std::max<u64>(effective, 1);
    out->pbc1 = (double)G[G_M1] / (double)std::max<u64>(G[G_DISTINCT], 1);
    out->pbc2 = (double)G[G_M1] / (double)std::max<u64>(G[G_M2], 1);
    g_bam_stages[0] = h.t_open, g_bam_stages[5] = now_s() - t_enter;
    return GTARS_OK;
}

gtars_status bam_decode(const gtars_bam &h, u64 first, u64 count, u64 max_window, unsigned threads, int32_t **cols, u64 *n_out) {
    const double t_enter = now_s();
    GT_TRY(require_device());
    hipStream_t st = nullptr;
    std::vector<i32> col[7];
    std::vector<i32> tmp;
    const u64 last = count > UINT64_MAX - first ? UINT64_MAX : first + count;
    BamPipe pipe(h.f, max_window, threads, st);
    GT_TRY(pipe.run([&](const BamCols &c, u32 n, const BamSegs &, u64 rec0, const u8 *) -> gtars_status {
        const u64 a = std::max(first, rec0), b = std::min<u64>(last, rec0 + n);
        if (a >= b) return GTARS_OK;
        const i32 *src[7] = {c.ref, c.pos, c.end, (const i32 *)c.flag, c.mapq, c.lseq, c.tlen};
        const size_t k = (size_t)(b - a);
        tmp.resize(7 * k);
        for (int j = 0; j < 7; ++j) GT_HIP(hipMemcpyAsync(tmp.data() + j * k, src[j] + (a - rec0), k * 4, hipMemcpyDeviceToHost, st));
        GT_HIP(hipStreamSynchronize(st));
        for (int j = 0; j < 7; ++j) col[j].insert(col[j].end(), tmp.begin() + j * k, tmp.begin() + (j + 1) * k);
        return GTARS_OK;
    }));
    const size_t n = col[0].size();
    i32 *res = (i32 *)malloc(std::max<size_t>(n * 7, 1) * sizeof(i32));
    if (!res) return fail(GTARS_ERR_INTERNAL, "out of host memory");
    for (int j = 0; j < 7; ++j)
        for (size_t i = 0; i < n; ++i) res[j * n + i] = j == 3 ? (i32)((u32)col[j][i] & 0xFFFFu) : col[j][i];
    *cols = res, *n_out = n;
    g_bam_stages[0] = h.t_open, g_bam_stages[5] = now_s() - t_enter;
    return GTARS_OK;
}

}  // namespace
}  // namespace gtars

using namespace gtars;

extern "C" {

gtars_status gtars_bam_open(const char *path, gtars_bam_t **out) {
    return guarded([&]() -> gtars_status {
        if (!path || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        const double t0 = now_s();
        std::unique_ptr<gtars_bam> h(new gtars_bam);
        GT_TRY(bam_open(path, h->f));
        h->t_open = now_s() - t0;
        *out = h.release();
        return GTARS_OK;
    });
}
void gtars_bam_close(gtars_bam_t *b) { delete b; }
const char *gtars_bam_header_text(const gtars_bam_t *b) { return b ? b->f.text.c_str() : ""; }
uint32_t gtars_bam_n_ref(const gtars_bam_t *b) { return b ? (uint32_t)b->f.refs.size() : 0; }
const char *gtars_bam_ref_name(const gtars_bam_t *b, uint32_t i) { return b && i < b->f.refs.size() ? b->f.refs[i].name.c_str() : nullptr; }
uint32_t gtars_bam_ref_len(const gtars_bam_t *b, uint32_t i) { return b && i < b->f.refs.size() ? b->f.refs[i].len : 0; }
uint64_t gtars_bam_n_blocks(const gtars_bam_t *b) { return b ? b->f.blocks.size() : 0; }
uint64_t gtars_bam_n_bytes(const gtars_bam_t *b) { return b ? b->f.n_bytes : 0; }
uint64_t gtars_bam_first_record(const gtars_bam_t *b) { return b ? b->f.first_record : 0; }

gtars_status gtars_bam_block_table(const gtars_bam_t *b, uint64_t *coff, uint32_t *csize, uint32_t *isize, uint32_t *crc, uint64_t *uoff) {
    return guarded([&]() -> gtars_status {
        if (!b) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        for (size_t i = 0; i < b->f.blocks.size(); ++i) {
            const BamBlock &k = b->f.blocks[i];
            if (coff) coff[i] = k.coff;
            if (csize) csize[i] = k.csize;
            if (isize) isize[i] = k.isize;
            if (crc) crc[i] = k.crc;
            if (uoff) uoff[i] = k.uoff;
        }
        return GTARS_OK;
    });
}

gtars_status gtars_bam_inflate(const gtars_bam_t *b, uint64_t block0, uint64_t block1, void *dst, uint64_t capacity, uint32_t threads) {
    return guarded([&]() -> gtars_status {
        if (!b) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        const size_t nb = b->f.blocks.size();
        if (block0 > block1 || block1 > nb) return fail(GTARS_ERR_INVALID_ARG, "block range out of bounds");
        const uint64_t need = (block1 < nb ? b->f.blocks[block1].uoff : b->f.n_bytes) - (block0 < nb ? b->f.blocks[block0].uoff : b->f.n_bytes);
        if (need > capacity) return fail(GTARS_ERR_CAPACITY, "inflate buffer too small: need " + std::to_string(need));
        if (need && !dst) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        return bam_inflate(b->f, block0, block1, (uint8_t *)dst, threads);
    });
}

gtars_status gtars_bam_record_offsets(const gtars_bam_t *b, const void *data, uint64_t n, uint64_t begin, int final, uint64_t **offsets,
                                      uint64_t *count, uint64_t *consumed) {
    return guarded([&]() -> gtars_status {
        if (!b || (!data && n) || !offsets || !count || begin > n) return fail(GTARS_ERR_INVALID_ARG, "NULL argument or begin > n");
        *offsets = nullptr, *count = 0;
        std::vector<uint64_t> offs;
        BamWalk w;
        uint64_t used = 0;
        GT_TRY(bam_walk((const uint8_t *)data, n, begin, final != 0, (int64_t)b->f.refs.size(), w, nullptr, &offs, 0, &used));
        uint64_t *res = (uint64_t *)malloc(std::max<size_t>(offs.size(), 1) * sizeof(uint64_t));
        if (!res) return fail(GTARS_ERR_INTERNAL, "out of host memory");
        if (!offs.empty()) memcpy(res, offs.data(), offs.size() * sizeof(uint64_t));
        *offsets = res, *count = offs.size();
        if (consumed) *consumed = used;
        return GTARS_OK;
    });
}

gtars_status gtars_bam_decode(const gtars_bam_t *b, uint64_t first, uint64_t count, uint64_t max_window_bytes, uint32_t threads, int32_t **cols,
                              uint64_t *n) {
    return guarded([&]() -> gtars_status {
        if (!b || !cols || !n) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *cols = nullptr, *n = 0;
        return bam_decode(*b, first, count, window_bytes(max_window_bytes), threads, cols, n);
    });
}

gtars_status gtars_bam_qc(const gtars_bam_t *b, uint64_t max_window_bytes, uint32_t threads, gtars_bam_qc_result *out) {
    return guarded([&]() -> gtars_status {
        if (!b || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        memset(out, 0, sizeof *out);
        return bam_qc(*b, window_bytes(max_window_bytes), threads, out);
    });
}

void gtars_bam_last_stages(double *out6) {
    if (out6) memcpy(out6, g_bam_stages, sizeof g_bam_stages);
}

}  // extern "C"
