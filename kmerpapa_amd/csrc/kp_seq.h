// kp_seq.h -- k-mer context counts of a genome and of its mutation sites (no reference
// counterpart: the reference starts from count files, and its README names an external tool
// for producing them).  Included by kp_hip.hip.  Semantics: include/kmerpapa_hip.h.
//
// Integer counts only, so the order of the adds does not matter and a device session equals the
// host session bit for bit.  The per-base code is __host__ __device__ and shared by both:
//   kp_s_class  a byte's nucleotide digit (A/a 0, C/c 1, G/g 2, T/t 3) or 4 = invalid
//   kp_s_step   one base appended to a rolling window: the forward code, the code of the reverse
//               complement, and the number of consecutive valid bases
//   kp_s_code   the counted code: with folding, the reverse complement where the centre is G or T
//
//   kp_seq_scan_kernel   a persistent grid over work items (first centre, count <= KP_S_TILE) the
//                        host cut from the merged regions, item s * gridDim.x + blockIdx.x at step
//                        s.  Each thread owns KP_S_RUN consecutive centres: it loads their bytes
//                        and the k - 1 halo as four aligned 16-byte words, rolls the window over
//                        them in registers and emits one code per complete window -- into uint32
//                        LDS counters of the workgroup (flushed at the end, one global 64-bit
//                        atomic per non-zero counter; a workgroup sees fewer than 2^32 centres,
//                        since a contig is shorter than that and regions are disjoint), or with
//                        global 64-bit atomics straight into the table: at each step of the
//                        roll the lanes that hold the same code as the wave's first emitting
//                        lane add once, together (low-complexity runs, where a whole wave
//                        holds one code), every other lane adds 1 on its own.  A session that counts
//                        both strands (kp_seq_begin_strands, kp_seq_begin_indel) runs builds of
//                        its own, <.., .., BOTH>, that emit the reverse complement's code as well
//   kp_seq_sites_kernel  one thread per site: the k bytes around it, the same classify / fold
//                        code, one global atomic per kept site
//
// Every device loop has a bound the host computed; there are no waits between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "kp_rt.h"

#define KP_S_MAXK 15
#define KP_S_THREADS 256
#define KP_S_RUN 32                            // centres per thread
#define KP_S_TILE (KP_S_THREADS * KP_S_RUN)    // centres per work item
#define KP_S_LDS_K 7                           // largest k with LDS counters: 4^7 * 4 B = 64 KiB, two workgroups per CU
// bytes allocated past a contig's end: a thread that owns centres loads aligned 16-byte words
// that begin before the last byte of its last window (< n), so no load reaches n + 15; a thread
// that owns none loads nothing
#define KP_S_PAD 64
// most items per workgroup and launch of a both-strand scan with LDS counters (kp_seq_scan_kernel)
#define KP_S_BOTH_STEPS (1u << 17)

__host__ __device__ inline uint32_t kp_s_class(uint32_t byte) {
    const uint32_t b = byte & 0xDFu;  // upper case
    return b == 'A' ? 0u : (b == 'C' ? 1u : (b == 'G' ? 2u : (b == 'T' ? 3u : 4u)));
}

struct kp_s_win {
    uint32_t fwd, rc, valid;
};

// mask = 4^k - 1, top = 2 (k - 1)
__host__ __device__ inline void kp_s_step(kp_s_win &w, uint32_t cls, uint32_t mask, int top) {
    const bool ok = cls < 4u;
    const uint32_t d = cls & 3u;
    w.fwd = ((w.fwd << 2) | d) & mask;
    w.rc = (w.rc >> 2) | ((3u - d) << top);
    w.valid = ok ? w.valid + 1u : 0u;  // (after an invalid byte k valid ones renew every bit of fwd and rc)
}

__host__ __device__ inline uint32_t kp_s_code(const kp_s_win &w, int k, int fold) {
    const uint32_t centre = (w.fwd >> (2 * (k - 1 - k / 2))) & 3u;
    return (fold && centre >= 2u) ? w.rc : w.fwd;
}

struct kp_s_item {
    uint32_t first, count;  // centres [first, first + count)
};

struct kp_s_args {
    const uint8_t *seq;      // the contig, KP_S_PAD readable bytes past its end
    const kp_s_item *items;  // [n_items]
    uint32_t n_items, steps;
    int32_t k, fold;
    uint32_t cells;           // 4^k
    unsigned long long *tab;  // [cells] the background column
    unsigned long long *stat; // [0] += windows counted
};

#ifdef __HIPCC__

// BOTH (a session that counts both strands, kp_seq_begin_strands / kp_seq_begin_indel; no folding):
// every window adds 1 at its forward code and 1 at its reverse complement's, a palindromic window
// 2 to one cell.  A build of its own, so the one-strand builds carry no branch for it.  Its uint32
// LDS counters take up to 2 per centre, so the host launches at most KP_S_BOTH_STEPS items per
// workgroup at a time: a counter holds at most 2 * KP_S_BOTH_STEPS * KP_S_TILE = 2^31 at the
// flush that ends a launch, whatever the contig and also with KP_SEQ_GRID=1.
template <bool LDS, bool MERGE, bool BOTH = false>
__global__ void __launch_bounds__(KP_S_THREADS) kp_seq_scan_kernel(kp_s_args A) {
    extern __shared__ uint32_t kp_s_cnt[];  // [cells] with LDS
    const uint32_t tid = threadIdx.x;
    if (LDS) {
        for (uint32_t e = tid; e < A.cells; e += KP_S_THREADS) kp_s_cnt[e] = 0;
        __syncthreads();
    }
    const int k = A.k, top = 2 * (A.k - 1), h = A.k / 2;
    const uint32_t mask = A.cells - 1u;
    uint32_t mine = 0;  // windows this thread counted
    for (uint32_t s = 0; s < A.steps; ++s) {
        const uint32_t item = s * gridDim.x + blockIdx.x;
        if (item >= A.n_items) break;
        const kp_s_item it = A.items[item];
        const uint32_t r0 = tid * KP_S_RUN;
        const uint32_t cnt = r0 < it.count ? min((uint32_t)KP_S_RUN, it.count - r0) : 0u;
        // bytes [s0, s0 + len) hold this thread's windows; a = s0 rounded down to 16
        const uint64_t s0 = (uint64_t)it.first + r0 - (uint32_t)h;
        const uint32_t len = cnt ? cnt + (uint32_t)k - 1u : 0u;
        const uint64_t a = s0 & ~(uint64_t)15;
        const uint32_t off = (uint32_t)(s0 - a), end = off + len;  // end <= 15 + 32 + 14
        uint32_t d[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint4 w = make_uint4(0, 0, 0, 0);
            // a thread without centres (cnt = 0: a short item) loads nothing: its s0 may lie far
            // past the contig; with cnt > 0, a + 16 q < s0 + len <= n, so the word ends before
            // n + 15 < n + KP_S_PAD
            if (cnt && 16u * q < end) w = *reinterpret_cast<const uint4 *>(A.seq + a + 16u * q);
            d[4 * q] = w.x;
            d[4 * q + 1] = w.y;
            d[4 * q + 2] = w.z;
            d[4 * q + 3] = w.w;
        }
        kp_s_win w{0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < 64; ++j) {
            const bool act = j >= off && j < end;
            if (act) kp_s_step(w, kp_s_class((d[j >> 2] >> (8u * (j & 3u))) & 0xffu), mask, top);
            const bool has = act && w.valid >= (uint32_t)k;
            mine += has;
#pragma unroll
            for (int strand = 0; strand < (BOTH ? 2 : 1); ++strand) {
                const uint32_t code = BOTH ? (strand ? w.rc : w.fwd) : kp_s_code(w, k, A.fold);
                if (LDS) {
                    if (has) atomicAdd(&kp_s_cnt[code], 1u);
                } else if (MERGE) {
                    // the lanes that hold the first emitting lane's code add once, together
                    const unsigned long long m = __ballot(has);
                    if (m) {
                        const int lead = __ffsll(m) - 1;
                        const uint32_t c0 = (uint32_t)__shfl((int)code, lead, 64);
                        const unsigned long long eq = __ballot(has && code == c0);
                        if ((int)(tid & 63u) == lead)
                            atomicAdd(&A.tab[c0], (unsigned long long)__popcll(eq));
                        else if (has && code != c0)
                            atomicAdd(&A.tab[code], 1ull);
                    }
                } else {
                    if (has) atomicAdd(&A.tab[code], 1ull);
                }
            }
        }
    }
    for (int o = 32; o; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((tid & 63u) == 0 && mine) atomicAdd(&A.stat[0], (unsigned long long)mine);
    if (LDS) {
        __syncthreads();
        for (uint32_t e = tid; e < A.cells; e += KP_S_THREADS) {
            const uint32_t v = kp_s_cnt[e];
            if (v) atomicAdd(&A.tab[e], (unsigned long long)v);
        }
    }
}

// tab = the positive column; stat[1] += sites counted, stat[2] += sites skipped
__global__ void __launch_bounds__(256) kp_seq_sites_kernel(const uint8_t *__restrict__ seq, uint64_t n,
                                                           const uint64_t *__restrict__ pos, uint64_t n_sites, int k,
                                                           int fold, uint32_t cells, unsigned long long *tab,
                                                           unsigned long long *stat) {
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    const bool act = i < n_sites;
    bool ok = false;
    if (act) {
        const uint64_t p = pos[i], h = (uint64_t)(k / 2);
        if (p >= h && p - h + (uint64_t)k <= n) {
            kp_s_win w{0u, 0u, 0u};
            for (int j = 0; j < k; ++j) kp_s_step(w, kp_s_class(seq[p - h + j]), cells - 1u, 2 * (k - 1));
            ok = w.valid == (uint32_t)k;
            if (ok) atomicAdd(&tab[kp_s_code(w, k, fold)], 1ull);
        }
    }
    const unsigned long long kept = __popcll(__ballot(ok)), skipped = __popcll(__ballot(act && !ok));
    if ((threadIdx.x & 63u) == 0) {  // one atomic per wave and counter
        if (kept) atomicAdd(&stat[1], kept);
        if (skipped) atomicAdd(&stat[2], skipped);
    }
}

#endif  // __HIPCC__

// ---------------------------------------------------------------------------
// sessions: the context's (device) or this thread's (host, ctx = NULL)
// ---------------------------------------------------------------------------

static thread_local kp_seq_sess g_seq_host;

static kp_seq_sess *seq_sess(kp_ctx *c) { return c ? &c->seq : &g_seq_host; }

// The work items of one contig: the regions (sorted and disjoint; none = the whole contig)
// clipped to the centres whose window lies inside the contig, cut into pieces of KP_S_TILE.
static std::vector<kp_s_item> seq_items(uint64_t n, int k, const uint64_t *rb, const uint64_t *re, uint64_t nr,
                                        uint64_t *centres) {
    std::vector<kp_s_item> items;
    *centres = 0;
    if (n < (uint64_t)k) return items;
    const uint64_t lo = (uint64_t)(k / 2), hi = n - (uint64_t)k + lo + 1;  // centres [lo, hi)
    const uint64_t whole_b = 0, whole_e = n;
    if (!nr) rb = &whole_b, re = &whole_e, nr = 1;
    for (uint64_t r = 0; r < nr; ++r) {
        const uint64_t b = std::max(rb[r], lo), e = std::min(re[r], hi);
        for (uint64_t f = b; f < e; f += KP_S_TILE) {
            const uint64_t cnt = std::min<uint64_t>(KP_S_TILE, e - f);
            items.push_back(kp_s_item{(uint32_t)f, (uint32_t)cnt});
            *centres += cnt;
        }
    }
    return items;
}

// kp_seq_begin and kp_seq_begin_strands (pcols = 1), kp_seq_begin_typed (pcols = 3) and
// kp_seq_begin_indel (pcols = 3, indel)
static int seq_begin(const std::string &w, kp_ctx *c, int k, int fold, int pcols, int both = 0, bool indel = false) {
    kp_seq_sess *s = seq_sess(c);
    if (s->active) return fail(KP_E_STATE, w + ": a session is open (kp_seq_end first)");
    if (c && c->pred.active) return fail(KP_E_STATE, w + ": a kp_pred session holds the context's arena (kp_pred_end first)");
    if (c && c->spec.active) return fail(KP_E_STATE, w + ": a kp_spec session holds the context's arena (kp_spec_end first)");
    if (c && c->ispec.active) return fail(KP_E_STATE, w + ": a kp_ispec session holds the context's arena (kp_ispec_end first)");
    if (indel && (k < 2 || k > 14 || k % 2))
        return fail(KP_E_ARG, w + ": k must be even and 2..14 (the window of a breakpoint has k/2 bases on each side)");
    if (k < 1 || k > KP_S_MAXK) return fail(KP_E_ARG, w + ": k must be 1..15 (a dense table of 4^k counters)");
    if (fold && k % 2 == 0) return fail(KP_E_ARG, w + ": strand folding needs an odd k (a centre base)");
    const uint64_t cells = 1ull << (2 * k), cols = (uint64_t)pcols + 1;
    if (c) {
        KP_HIP(hipSetDevice(c->device));
        const size_t need = g_up(cols * cells * 8) + g_up(64);
        if (need > c->arena.bytes) {
            size_t fr = 0, tot = 0;
            KP_HIP(hipMemGetInfo(&fr, &tot));
            if (need + (2ull << 30) > fr + c->arena.bytes)
                return fail(KP_E_NOMEM, w + ": the table of " + std::to_string(k) + "-mers needs " +
                                            std::to_string(need >> 20) + " MiB of device memory, " +
                                            std::to_string((fr + c->arena.bytes) >> 20) + " MiB are free (2 GiB stay free)");
        }
        int rc = c->arena.reserve(w.c_str(), need);
        if (rc) return rc;
        s->d_tab = (unsigned long long *)c->arena.take(cols * cells * 8);
        s->d_stat = (unsigned long long *)c->arena.take(64);
        if ((rc = c->arena.check(w.c_str()))) return rc;
        KP_HIP(hipMemsetAsync(s->d_tab, 0, cols * cells * 8, c->stream));
        KP_HIP(hipMemsetAsync(s->d_stat, 0, 64, c->stream));
        KP_HIP(hipStreamSynchronize(c->stream));
    } else {
        try {
            s->h_tab.assign(cols * cells, 0);
        } catch (const std::bad_alloc &) {
            return fail(KP_E_NOMEM, w + ": the host table of " + std::to_string(k) + "-mers does not fit memory");
        }
    }
    s->k = k;
    s->fold = fold ? 1 : 0;
    s->both = both ? 1 : 0;
    s->indel = indel;
    s->pcols = pcols;
    s->cells = cells;
    s->centres = 0;
    s->st = kp_seq_stats{};
    s->st.tile = KP_S_TILE;
    s->active = true;
    return KP_OK;
}

// kp_seq_end (pcols = 1) and kp_seq_end_typed (pcols = 3): pos_counts holds pcols columns
static int seq_end(const std::string &w, kp_ctx *c, int pcols, uint64_t *pos_counts, uint64_t *bg_counts) {
    kp_seq_sess *s = seq_sess(c);
    if (!s->active) return fail(KP_E_STATE, w + ": no session (kp_seq_begin first)");
    if (s->pcols != pcols)
        return fail(KP_E_STATE, w + (pcols == 1 ? ": the session is typed (kp_seq_end_typed)" : ": the session is not typed (kp_seq_end)"));
    s->active = false;  // whatever happens below, the session is over
    const size_t bytes = (size_t)s->cells * 8;
    if (c) {
        KP_HIP(hipSetDevice(c->device));
        if (pos_counts) KP_HIP(hipMemcpyAsync(pos_counts, s->d_tab, pcols * bytes, hipMemcpyDeviceToHost, c->stream));
        if (bg_counts) KP_HIP(hipMemcpyAsync(bg_counts, s->d_tab + pcols * s->cells, bytes, hipMemcpyDeviceToHost, c->stream));
        KP_HIP(hipStreamSynchronize(c->stream));
    } else {
        if (pos_counts) memcpy(pos_counts, s->h_tab.data(), pcols * bytes);
        if (bg_counts) memcpy(bg_counts, s->h_tab.data() + pcols * s->cells, bytes);
        std::vector<uint64_t>().swap(s->h_tab);
    }
    return KP_OK;
}

extern "C" {

int kp_seq_begin(kp_ctx *c, int k, int fold) { return seq_begin("kp_seq_begin", c, k, fold, 1); }

int kp_seq_begin_typed(kp_ctx *c, int k, int fold) { return seq_begin("kp_seq_begin_typed", c, k, fold, 3); }

int kp_seq_begin_strands(kp_ctx *c, int k, int both) { return seq_begin("kp_seq_begin_strands", c, k, 0, 1, both); }

int kp_seq_begin_indel(kp_ctx *c, int k, int both) { return seq_begin("kp_seq_begin_indel", c, k, 0, 3, both, true); }

int kp_seq_scan(kp_ctx *c, const uint8_t *seq, uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end,
                uint64_t n_regions) {
    kp_seq_sess *s = seq_sess(c);
    int rc = scan_check_contig("kp_seq_scan", s->active, seq, n, "kp_seq_begin");
    if (rc) return rc;
    if (n_regions && (!reg_begin || !reg_end)) return fail(KP_E_ARG, "kp_seq_scan: null regions");
    for (uint64_t r = 0; r < n_regions; ++r)
        if (reg_begin[r] > reg_end[r] || reg_end[r] > n || (r && reg_begin[r] < reg_end[r - 1]))
            return fail(KP_E_ARG, "kp_seq_scan: region " + std::to_string(r) +
                                      " is not sorted, overlaps the one before or lies outside the contig");
    const int k = s->k;
    uint64_t centres = 0;
    const std::vector<kp_s_item> items = seq_items(n, k, reg_begin, reg_end, n_regions, &centres);
    if (!c) {
        const uint32_t mask = (uint32_t)(s->cells - 1);
        uint64_t *bg = s->h_tab.data() + (uint64_t)s->pcols * s->cells;
        for (const kp_s_item &it : items) {
            kp_s_win w{0u, 0u, 0u};
            const uint64_t b0 = (uint64_t)it.first - (uint64_t)(k / 2);
            for (uint64_t p = b0; p < b0 + it.count + (uint64_t)k - 1; ++p) {
                kp_s_step(w, kp_s_class(seq[p]), mask, 2 * (k - 1));
                if (w.valid >= (uint32_t)k) {
                    if (s->both)
                        ++bg[w.fwd], ++bg[w.rc];
                    else
                        ++bg[kp_s_code(w, k, s->fold)];
                    ++s->st.windows;
                }
            }
        }
    } else if (!items.empty()) {
        KP_HIP(hipSetDevice(c->device));
        const long lds_k = env_int("KP_SEQ_LDS_K", KP_S_LDS_K);
        if (lds_k < 0 || lds_k > KP_S_LDS_K)
            return fail(KP_E_ARG, "kp_seq_scan: KP_SEQ_LDS_K must be 0..7 (4^k uint32 counters beside a second workgroup's)");
        const bool lds = env_int("KP_SEQ_GLOBAL", 0) == 0 && k <= lds_k;
        const size_t lds_bytes = lds ? (size_t)s->cells * 4 : 0;
        // a persistent grid: as many workgroups as are resident at once
        const int per_cu = !lds ? 8 : (lds_bytes <= 16u * 1024u ? 8 : (lds_bytes <= 40u * 1024u ? 4 : 2));
        const uint64_t grid = scan_grid(c, items.size(), per_cu, "KP_SEQ_GRID");
        const uint64_t steps = (items.size() + grid - 1) / grid;

        const size_t b_seq = g_up(n + KP_S_PAD), b_items = g_up(items.size() * sizeof(kp_s_item));
        if ((rc = c->seq_in.reserve("kp_seq_scan", b_seq + b_items))) return rc;
        uint8_t *d_seq = (uint8_t *)c->seq_in.take(b_seq);
        kp_s_item *d_items = (kp_s_item *)c->seq_in.take(b_items);
        if ((rc = c->seq_in.check("kp_seq_scan"))) return rc;
        hipStream_t st = c->stream;
        KP_HIP(hipMemcpyAsync(d_seq, seq, n, hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(kp_s_item), hipMemcpyHostToDevice, st));
        kp_s_args A;
        A.seq = d_seq;
        A.items = d_items;
        A.n_items = (uint32_t)items.size();
        A.steps = (uint32_t)steps;
        A.k = k;
        A.fold = s->fold;
        A.cells = (uint32_t)s->cells;
        A.tab = s->d_tab + (uint64_t)s->pcols * s->cells;
        A.stat = s->d_stat;
        const bool merge = env_int("KP_SEQ_MERGE", 1) != 0;  // (on by measurement: a quarter faster on a repeat-rich contig)
        KP_HIP(hipEventRecord(c->ev[0], st));
        if (s->both) {
            // LDS counters: at most max_steps items per workgroup and launch (kp_seq_scan_kernel)
            const long steps_env = env_int("KP_SEQ_BOTH_STEPS", KP_S_BOTH_STEPS);
            if (steps_env < 1 || steps_env > (long)KP_S_BOTH_STEPS)
                return fail(KP_E_ARG, "kp_seq_scan: KP_SEQ_BOTH_STEPS must be 1..131072 (a uint32 LDS counter takes 2 per centre)");
            const uint64_t max_steps = lds ? (uint64_t)steps_env : steps, per_launch = grid * max_steps;
            for (uint64_t i0 = 0; i0 < items.size(); i0 += per_launch) {
                const uint64_t cnt = std::min<uint64_t>(per_launch, items.size() - i0);
                A.items = d_items + i0;
                A.n_items = (uint32_t)cnt;
                A.steps = (uint32_t)((cnt + grid - 1) / grid);
                if (lds)
                    hipLaunchKernelGGL((kp_seq_scan_kernel<true, false, true>), dim3((unsigned)grid), dim3(KP_S_THREADS), lds_bytes, st, A);
                else if (merge)
                    hipLaunchKernelGGL((kp_seq_scan_kernel<false, true, true>), dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
                else
                    hipLaunchKernelGGL((kp_seq_scan_kernel<false, false, true>), dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
            }
        } else if (lds)
            hipLaunchKernelGGL((kp_seq_scan_kernel<true, false>), dim3((unsigned)grid), dim3(KP_S_THREADS), lds_bytes, st, A);
        else if (merge)
            hipLaunchKernelGGL((kp_seq_scan_kernel<false, true>), dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
        else
            hipLaunchKernelGGL((kp_seq_scan_kernel<false, false>), dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
        KP_HIP(hipGetLastError());
        KP_HIP(hipEventRecord(c->ev[1], st));
        unsigned long long h_stat[3] = {0, 0, 0};
        KP_HIP(hipMemcpyAsync(h_stat, s->d_stat, sizeof h_stat, hipMemcpyDeviceToHost, st));
        KP_HIP(hipStreamSynchronize(st));
        float ms = 0.f;
        KP_HIP(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        s->st.scan_ms += ms;
        s->st.path = lds ? 1u : 2u;
        s->st.windows = h_stat[0];
    }
    s->centres += centres;
    s->st.items += items.size();
    s->st.windows_invalid = s->centres - s->st.windows;
    return KP_OK;
}

int kp_seq_sites(kp_ctx *c, const uint8_t *seq, uint64_t n, const uint64_t *pos, uint64_t n_sites) {
    kp_seq_sess *s = seq_sess(c);
    int rc = scan_check_contig("kp_seq_sites", s->active, seq, n, "kp_seq_begin");
    if (rc) return rc;
    if (s->indel) return fail(KP_E_STATE, "kp_seq_sites: the session is an indel session (kp_seq_indels)");
    if (s->both) return fail(KP_E_STATE, "kp_seq_sites: the session counts both strands, which single-base sites have no rule for");
    if (s->pcols != 1) return fail(KP_E_STATE, "kp_seq_sites: the session is typed (kp_seq_sites_typed)");
    if (n_sites && !pos) return fail(KP_E_ARG, "kp_seq_sites: null positions");
    if (n_sites >= (1ull << 39)) return fail(KP_E_ARG, "kp_seq_sites: 2^39 sites or more in one call");
    for (uint64_t i = 0; i < n_sites; ++i)
        if (pos[i] >= n)
            return fail(KP_E_ARG, "kp_seq_sites: site " + std::to_string(i) + " at " + std::to_string(pos[i]) +
                                      " lies past the contig's " + std::to_string(n) + " bases");
    if (!n_sites) return KP_OK;
    const int k = s->k;
    if (!c) {
        const uint64_t h = (uint64_t)(k / 2);
        for (uint64_t i = 0; i < n_sites; ++i) {
            const uint64_t p = pos[i];
            bool ok = false;
            if (p >= h && p - h + (uint64_t)k <= n) {
                kp_s_win w{0u, 0u, 0u};
                for (int j = 0; j < k; ++j) kp_s_step(w, kp_s_class(seq[p - h + j]), (uint32_t)(s->cells - 1), 2 * (k - 1));
                ok = w.valid == (uint32_t)k;
                if (ok) ++s->h_tab[kp_s_code(w, k, s->fold)];
            }
            ++(ok ? s->st.sites : s->st.sites_skipped);
        }
        return KP_OK;
    }
    KP_HIP(hipSetDevice(c->device));
    const size_t b_seq = g_up(n + KP_S_PAD), b_pos = g_up(n_sites * 8);
    if ((rc = c->seq_in.reserve("kp_seq_sites", b_seq + b_pos))) return rc;
    uint8_t *d_seq = (uint8_t *)c->seq_in.take(b_seq);
    uint64_t *d_pos = (uint64_t *)c->seq_in.take(b_pos);
    if ((rc = c->seq_in.check("kp_seq_sites"))) return rc;
    hipStream_t st = c->stream;
    KP_HIP(hipMemcpyAsync(d_seq, seq, n, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_pos, pos, n_sites * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kp_seq_sites_kernel, dim3((unsigned)((n_sites + 255) / 256)), dim3(256), 0, st, d_seq, n, d_pos,
                       n_sites, k, s->fold, (uint32_t)s->cells, s->d_tab, s->d_stat);
    KP_HIP(hipGetLastError());
    unsigned long long h_stat[3] = {0, 0, 0};
    KP_HIP(hipMemcpyAsync(h_stat, s->d_stat, sizeof h_stat, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    s->st.sites = h_stat[1];
    s->st.sites_skipped = h_stat[2];
    return KP_OK;
}

int kp_seq_end(kp_ctx *c, uint64_t *pos_counts, uint64_t *bg_counts) {
    return seq_end("kp_seq_end", c, 1, pos_counts, bg_counts);
}

int kp_seq_end_typed(kp_ctx *c, uint64_t *pos_counts, uint64_t *bg_counts) {
    return seq_end("kp_seq_end_typed", c, 3, pos_counts, bg_counts);
}

int kp_seq_last_stats(kp_ctx *c, kp_seq_stats *out) {
    if (!out) return fail(KP_E_ARG, "kp_seq_last_stats: null out");
    *out = seq_sess(c)->st;
    return KP_OK;
}

int kp_seq_host(int k, int fold, const uint8_t *seq, uint64_t n, int scan, const uint64_t *reg_begin,
                const uint64_t *reg_end, uint64_t n_regions, const uint64_t *pos, uint64_t n_sites,
                uint64_t *pos_counts, uint64_t *bg_counts, kp_seq_stats *stats) {
    int rc = kp_seq_begin(nullptr, k, fold);
    if (rc) return rc;
    if (scan) rc = kp_seq_scan(nullptr, seq, n, reg_begin, reg_end, n_regions);
    if (!rc) rc = kp_seq_sites(nullptr, seq, n, pos, n_sites);
    const std::string err = g_err;
    const int rc_end = kp_seq_end(nullptr, rc ? nullptr : pos_counts, rc ? nullptr : bg_counts);
    if (rc) return fail(rc, err);
    if (stats) *stats = g_seq_host.st;
    return rc_end;
}

}  // extern "C"
