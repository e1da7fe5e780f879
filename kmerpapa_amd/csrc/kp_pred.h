// kp_pred.h -- a fitted partition taken back to the genome (no reference counterpart).  Included
// by kp_hip.hip.  Semantics: include/kmerpapa_hip.h.
//
// Windows, validity, the centre and folding are kp_seq.h's (kp_s_class / kp_s_step / kp_s_code),
// matching is kp_apply.h's (kp_a_onehot / kp_a_match), the aligned loads, the batched roll and the
// host's items, region check, uploads, arena and timed launch are kp_scan.h's.  Counts are integers
// and `expected` is a float64 sum in pattern order, so a device session equals the host session
// bit for bit.
//
//   kp_pred_lut_kernel    one k-mer code per thread against every pattern (staged through LDS in
//                         tiles, as kp_apply_assign stages them): lut[code] = the first and, the
//                         patterns being disjoint, only match, or -1.  Codes with G or T in the
//                         centre are not tested under folding: the scan cannot produce them.
//                         (int32 entries: a 16-bit table was measured and did not pay)
//   kp_pred_scan_kernel   kp_seq_scan_kernel's grid and roll over work items (first centre, count
//                         <= KP_S_TILE, region).  The roll goes in batches of KP_P_BATCH bytes:
//                         the codes of a batch first, then its gathers from lut together, then
//                         the adds -- into uint32 LDS counters that belong to the item (flushed
//                         to the region's row after it, one global 64-bit atomic per non-zero
//                         counter, and zeroed; a counter sees at most KP_S_TILE adds), or with
//                         global 64-bit atomics into the row.  other[region] gets one atomic per
//                         wave, item and counter
//   kp_pred_track_kernel  the same roll over KP_S_TILE consecutive positions of [begin, end) per
//                         item; a thread's 32 results go through LDS (transposed, so that writes
//                         do not collide) and leave as aligned 16-byte stores.  Positions outside
//                         the clipped centre range keep the -2 every slot starts with
//   kp_pred_sites_kernel  one thread per site, as kp_seq_sites_kernel
//   kp_pred_sums_kernel   one thread per region: expected, in pattern order
//
// Every device loop has a bound the host computed; there are no waits between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "kp_apply.h"
#include "kp_rt.h"
#include "kp_scan.h"
#include "kp_seq.h"

#define KP_P_LDS_P 16384   // most patterns with LDS counters: 64 KiB of uint32, two workgroups per CU
#define KP_P_LUT_TILE 1024 // patterns per LDS tile of the table build
#define KP_P_NONE (-1)
#define KP_P_INVALID (-2)

// the pattern of a one-hot word: the first match, or -1
__host__ __device__ inline int32_t kp_p_find(uint64_t oh, const uint64_t *pats, uint32_t P) {
    for (uint32_t j = 0; j < P; ++j)
        if (kp_a_match(oh, pats[j])) return (int32_t)j;
    return KP_P_NONE;
}

// a code the scan can produce: under folding the centre is A or C
__host__ __device__ inline bool kp_p_reachable(uint32_t code, int k, int fold) {
    return !fold || ((code >> (2 * (k - 1 - k / 2))) & 3u) < 2u;
}

// the code of the window centred at p, or false if it leaves the contig or holds an invalid byte
__host__ __device__ inline bool kp_p_window(const uint8_t *seq, uint64_t n, uint64_t p, int k, int fold, uint32_t mask,
                                            uint32_t *code) {
    const uint64_t h = (uint64_t)(k / 2);
    if (p < h || p - h + (uint64_t)k > n) return false;
    kp_s_win w{0u, 0u, 0u};
    for (int j = 0; j < k; ++j) kp_s_step(w, kp_s_class(seq[p - h + j]), mask, 2 * (k - 1));
    *code = kp_s_code(w, k, fold);
    return w.valid == (uint32_t)k;
}

struct kp_p_args {
    const uint8_t *seq;      // the contig, KP_S_PAD readable bytes past its end
    const kp_p_item *items;  // [n_items]
    uint32_t n_items, steps;
    int32_t k, fold;
    uint32_t mask;  // 4^k - 1
    uint32_t P;
    const int32_t *lut;         // [4^k]
    unsigned long long *hist;   // [n_regions][P]
    unsigned long long *other;  // [n_regions][2]: no pattern, invalid
};

struct kp_p_targs {
    const uint8_t *seq;
    uint32_t begin, len;  // positions [begin, begin + len)
    uint32_t lo, hi;      // centres whose window lies inside the contig
    uint32_t n_items, steps;
    int32_t k, fold;
    uint32_t mask;
    const int32_t *lut;
    int32_t *pid;  // [len], 256-byte aligned
};

#ifdef __HIPCC__

__global__ void __launch_bounds__(256) kp_pred_lut_kernel(const uint64_t *__restrict__ pats, uint32_t P, int k, int fold,
                                                          uint32_t cells, int32_t *__restrict__ lut) {
    __shared__ unsigned long long sT[KP_P_LUT_TILE];
    const uint32_t tid = threadIdx.x;
    const uint32_t code = blockIdx.x * 256u + tid;
    const bool act = code < cells && kp_p_reachable(code, k, fold);
    const uint64_t oh = act ? kp_a_onehot(code, k) : 0;
    int32_t found = KP_P_NONE;
    for (uint32_t t0 = 0; t0 < P; t0 += KP_P_LUT_TILE) {
        const uint32_t nt = P - t0 < KP_P_LUT_TILE ? P - t0 : KP_P_LUT_TILE;
        __syncthreads();  // the previous tile has been read by every wave
        for (uint32_t e = tid; e < nt; e += 256u) sT[e] = pats[t0 + e];
        __syncthreads();
        if (act && found < 0) {
#pragma unroll 8
            for (uint32_t j = 0; j < nt; ++j) found = (found < 0 && kp_a_match(oh, sT[j])) ? (int32_t)(t0 + j) : found;
        }
    }
    if (code < cells) lut[code] = found;
}

template <bool LDS>
__global__ void __launch_bounds__(KP_S_THREADS) kp_pred_scan_kernel(kp_p_args A) {
    extern __shared__ uint32_t kp_p_cnt[];  // [P] with LDS
    const uint32_t tid = threadIdx.x;
    if (LDS) {
        for (uint32_t e = tid; e < A.P; e += KP_S_THREADS) kp_p_cnt[e] = 0;
        __syncthreads();
    }
    const int k = A.k, top = 2 * (A.k - 1), h = A.k / 2;
    for (uint32_t s = 0; s < A.steps; ++s) {
        const uint32_t item = s * gridDim.x + blockIdx.x;
        if (item >= A.n_items) break;  // (the same for the whole workgroup)
        const kp_p_item it = A.items[item];
        const uint32_t r0 = tid * KP_S_RUN;
        const uint32_t cnt = r0 < it.count ? min((uint32_t)KP_S_RUN, it.count - r0) : 0u;
        uint32_t d[16], off, end;
        kp_p_load(A.seq, (uint64_t)it.first + r0 - (uint32_t)h, cnt ? cnt + (uint32_t)k - 1u : 0u, d, &off, &end);
        const uint32_t full0 = off + (uint32_t)k - 1u;  // the byte that completes the first window
        unsigned long long *row = A.hist + (uint64_t)it.region * A.P;
        uint32_t none = 0, inv = 0;
        kp_s_win w{0u, 0u, 0u};
#pragma unroll
        for (uint32_t jb = 0; jb < 64; jb += KP_P_BATCH) {
            uint32_t code[KP_P_BATCH];
            bool has[KP_P_BATCH];
            int32_t p[KP_P_BATCH];
            kp_scan_batch(w, d, jb, off, end, full0, k, A.fold, A.mask, top, code, has, inv);
#pragma unroll
            for (uint32_t q = 0; q < KP_P_BATCH; ++q) p[q] = has[q] ? A.lut[code[q]] : KP_P_INVALID;
#pragma unroll
            for (uint32_t q = 0; q < KP_P_BATCH; ++q) {
                if (p[q] >= 0) {
                    if (LDS)
                        atomicAdd(&kp_p_cnt[p[q]], 1u);
                    else
                        atomicAdd(&row[p[q]], 1ull);
                }
                none += p[q] == KP_P_NONE;
            }
        }
        for (int o = 32; o; o >>= 1) {
            none += __shfl_xor(none, o, 64);
            inv += __shfl_xor(inv, o, 64);
        }
        if ((tid & 63u) == 0) {
            if (none) atomicAdd(&A.other[2ull * it.region], (unsigned long long)none);
            if (inv) atomicAdd(&A.other[2ull * it.region + 1], (unsigned long long)inv);
        }
        if (LDS) {
            __syncthreads();  // every add of the item is in
            for (uint32_t e = tid; e < A.P; e += KP_S_THREADS) {
                const uint32_t v = kp_p_cnt[e];
                if (v) {
                    atomicAdd(&row[e], (unsigned long long)v);
                    kp_p_cnt[e] = 0;
                }
            }
            __syncthreads();  // zero again before the next item adds
        }
    }
}

__global__ void __launch_bounds__(KP_S_THREADS) kp_pred_track_kernel(kp_p_targs A) {
    __shared__ int32_t buf[KP_S_RUN * KP_P_ROW];  // [slot][thread]
    const uint32_t tid = threadIdx.x;
    const int k = A.k, top = 2 * (A.k - 1), h = A.k / 2;
    for (uint32_t s = 0; s < A.steps; ++s) {
        const uint32_t item = s * gridDim.x + blockIdx.x;
        if (item >= A.n_items) break;  // (the same for the whole workgroup)
        const uint64_t base = (uint64_t)item * KP_S_TILE;  // of the item in pid
        const uint64_t i0 = base + tid * KP_S_RUN;
        const uint32_t cnt = i0 >= A.len ? 0u : (A.len - i0 < KP_S_RUN ? (uint32_t)(A.len - i0) : (uint32_t)KP_S_RUN);
        // this thread's positions [c0, c0 + cnt), of which [cb, cb + nc) have a window inside the contig
        const uint64_t c0 = (uint64_t)A.begin + i0;
        const uint64_t cb = c0 > A.lo ? c0 : (uint64_t)A.lo, ce = c0 + cnt < A.hi ? c0 + cnt : (uint64_t)A.hi;
        const uint32_t nc = ce > cb ? (uint32_t)(ce - cb) : 0u;
#pragma unroll
        for (uint32_t q = 0; q < KP_S_RUN; ++q) buf[q * KP_P_ROW + tid] = KP_P_INVALID;
        uint32_t d[16], off, end;
        kp_p_load(A.seq, nc ? cb - (uint32_t)h : 0u, nc ? nc + (uint32_t)k - 1u : 0u, d, &off, &end);
        const uint32_t full0 = off + (uint32_t)k - 1u;
        const uint32_t slot0 = nc ? (uint32_t)(cb - c0) : 0u;  // slot of the first window: byte j fills slot0 + j - full0
        uint32_t inv = 0;  // (not reported: the slots of invalid windows keep their -2)
        kp_s_win w{0u, 0u, 0u};
#pragma unroll
        for (uint32_t jb = 0; jb < 64; jb += KP_P_BATCH) {
            uint32_t code[KP_P_BATCH];
            bool has[KP_P_BATCH];
            int32_t p[KP_P_BATCH];
            kp_scan_batch(w, d, jb, off, end, full0, k, A.fold, A.mask, top, code, has, inv);
#pragma unroll
            for (uint32_t q = 0; q < KP_P_BATCH; ++q) p[q] = has[q] ? A.lut[code[q]] : KP_P_INVALID;
#pragma unroll
            for (uint32_t q = 0; q < KP_P_BATCH; ++q)  // slot0 + j - full0 < slot0 + nc <= KP_S_RUN
                if (has[q]) buf[(slot0 + jb + q - full0) * KP_P_ROW + tid] = p[q];
        }
        __syncthreads();
        // the item's results leave in position order: vector v holds slots 4 (v % 8) .. + 3 of thread v / 8
#pragma unroll
        for (uint32_t q = 0; q < KP_S_RUN / 4; ++q) {
            const uint32_t v = q * KP_S_THREADS + tid, t = v >> 3, w0 = (v & 7u) * 4u;
            const uint64_t o = base + 4ull * v;
            if (o < A.len) {
                const int4 r = make_int4(buf[w0 * KP_P_ROW + t], buf[(w0 + 1) * KP_P_ROW + t], buf[(w0 + 2) * KP_P_ROW + t],
                                         buf[(w0 + 3) * KP_P_ROW + t]);
                if (o + 4 <= A.len) {
                    *reinterpret_cast<int4 *>(A.pid + o) = r;
                } else {  // the last positions of the range
                    A.pid[o] = r.x;
                    if (o + 1 < A.len) A.pid[o + 1] = r.y;
                    if (o + 2 < A.len) A.pid[o + 2] = r.z;
                }
            }
        }
        __syncthreads();  // read before the next item fills the slots
    }
}

__global__ void __launch_bounds__(256) kp_pred_sites_kernel(const uint8_t *__restrict__ seq, uint64_t n,
                                                            const uint64_t *__restrict__ pos, uint64_t n_sites, int k,
                                                            int fold, uint32_t mask, const int32_t *__restrict__ lut,
                                                            int32_t *__restrict__ pid) {
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n_sites) return;
    uint32_t code = 0;
    pid[i] = kp_p_window(seq, n, pos[i], k, fold, mask, &code) ? lut[code] : KP_P_INVALID;
}

__global__ void __launch_bounds__(64) kp_pred_sums_kernel(const unsigned long long *__restrict__ hist,
                                                          const double *__restrict__ rates, uint32_t P, uint64_t n_regions,
                                                          double *__restrict__ expected) {
    const uint64_t r = blockIdx.x * 64ull + threadIdx.x;
    if (r >= n_regions) return;
    const unsigned long long *row = hist + r * P;
    double acc = 0.0;
    for (uint32_t p = 0; p < P; ++p) acc = acc + (double)row[p] * rates[p];
    expected[r] = acc;
}

#endif  // __HIPCC__

// ---------------------------------------------------------------------------
// sessions: the context's (device) or this thread's (host, ctx = NULL)
// ---------------------------------------------------------------------------

static thread_local kp_pred_sess g_pred_host;

static kp_pred_sess *pred_sess(kp_ctx *c) { return c ? &c->pred : &g_pred_host; }

// scan_arena for the table of 4-byte entries: the table first, then `extra` bytes the caller takes
static int pred_arena(kp_ctx *c, const char *who, size_t extra) {
    kp_pred_sess *s = &c->pred;
    const uint32_t P = (uint32_t)s->pats.size();
    return scan_arena(c, s, who, "lookup", 4, g_up((size_t)P * 8), extra, [&]() -> int {
        uint64_t *d_pats = (uint64_t *)c->arena.take((size_t)P * 8);
        int rc = c->arena.check(who);
        if (rc) return rc;
        KP_HIP(hipMemcpyAsync(d_pats, s->pats.data(), (size_t)P * 8, hipMemcpyHostToDevice, c->stream));
        if ((rc = scan_mark(c, 0))) return rc;
        hipLaunchKernelGGL(kp_pred_lut_kernel, dim3((unsigned)((s->cells + 255) / 256)), dim3(256), 0, c->stream, d_pats, P,
                           s->k, s->fold, (uint32_t)s->cells, s->d_lut);
        return scan_launched(c, 1);
    });
}

// No two patterns share a k-mer.  A few patterns: every pair.  Many: every pattern's k-mers are
// marked in a bitmap of 4^k bits, which stops at the first k-mer marked twice, or before it starts
// if the patterns hold more than 4^k k-mers together -- at most 4^k marks where the pairs would
// be P^2 / 2 tests (5 * 10^9 for 10^5 patterns).
static bool pred_disjoint(const uint64_t *pats, uint32_t P, int k) {
    const uint64_t low = kp_a_low(k), cells = 1ull << (2 * k);
    if (P < 4096) {
        for (uint32_t i = 0; i < P; ++i)
            for (uint32_t j = i + 1; j < P; ++j)
                if (kp_a_overlap(pats[i], pats[j], low)) return false;
        return true;
    }
    uint64_t total = 0;
    for (uint32_t p = 0; p < P; ++p) {
        uint64_t size = 1;
        for (int i = 0; i < k; ++i) size *= (uint64_t)__builtin_popcountll((pats[p] >> (4 * i)) & 15u);
        if ((total += size) > cells) return false;
    }
    std::vector<uint64_t> seen((cells + 63) / 64, 0);
    for (uint32_t p = 0; p < P; ++p) {
        // the pattern's k-mers as an odometer over its positions: dig[i] = the digit of position i
        int dig[KP_S_MAXK];
        uint64_t code = 0;
        for (int i = 0; i < k; ++i) {
            dig[i] = __builtin_ctzll((pats[p] >> (4 * i)) & 15u);
            code |= (uint64_t)dig[i] << (2 * (k - 1 - i));
        }
        for (;;) {
            if (seen[code >> 6] >> (code & 63) & 1u) return false;
            seen[code >> 6] |= 1ull << (code & 63);
            int i = 0;
            for (; i < k; ++i) {  // the next digit of position i its mask allows, or back to its first and carry
                const uint32_t m = (uint32_t)(pats[p] >> (4 * i)) & 15u, up = m & ~((2u << dig[i]) - 1u);
                const int nd = up ? __builtin_ctz(up) : __builtin_ctz(m);
                code += ((uint64_t)nd - (uint64_t)dig[i]) << (2 * (k - 1 - i));
                dig[i] = nd;
                if (up) break;
            }
            if (i == k) break;
        }
    }
    return true;
}

extern "C" {

int kp_pred_begin(kp_ctx *c, int k, int fold, const uint64_t *patterns, uint32_t n_patterns, uint64_t super_word) {
    kp_pred_sess *s = pred_sess(c);
    if (s->active) return fail(KP_E_STATE, "kp_pred_begin: a session is open (kp_pred_end first)");
    if (c && c->seq.active)
        return fail(KP_E_STATE, "kp_pred_begin: a kp_seq session holds the context's arena (kp_seq_end first)");
    if (c && c->spec.active)
        return fail(KP_E_STATE, "kp_pred_begin: a kp_spec session holds the context's arena (kp_spec_end first)");
    if (c && c->ispec.active)
        return fail(KP_E_STATE, "kp_pred_begin: a kp_ispec session holds the context's arena (kp_ispec_end first)");
    if (k < 1 || k > KP_S_MAXK) return fail(KP_E_ARG, "kp_pred_begin: k must be 1..15 (a dense table of 4^k entries)");
    if (fold && k % 2 == 0) return fail(KP_E_ARG, "kp_pred_begin: strand folding needs an odd k (a centre base)");
    const uint32_t P = n_patterns;
    uint64_t dummy = 0;
    kp_apply_stats ast;
    int rc = apply_check("kp_pred_begin", k, patterns, P, super_word, nullptr, nullptr, nullptr, 0, 1, nullptr, &dummy,
                         &dummy, nullptr, &ast);
    if (rc) return rc;
    const uint64_t low = kp_a_low(k);
    const bool disjoint = pred_disjoint(patterns, P, k);
    for (uint32_t i = 0; i < P && !disjoint; ++i)  // (every pair only to name the first one)
        for (uint32_t j = i + 1; j < P; ++j)
            if (kp_a_overlap(patterns[i], patterns[j], low))
                return fail(KP_E_ARG, "kp_pred_begin: the patterns are not a partition: patterns " + std::to_string(i) +
                                          " and " + std::to_string(j) + " share k-mers");
    s->k = k;
    s->fold = fold ? 1 : 0;
    s->cells = 1ull << (2 * k);
    s->st = kp_pred_stats{};
    s->st.tile = KP_S_TILE;
    s->st.lut_bytes = s->cells * 4;
    try {
        s->pats.assign(patterns, patterns + P);
        if (!c) {
            s->h_lut.assign(s->cells, KP_P_NONE);
            for (uint64_t code = 0; code < s->cells; ++code)
                if (kp_p_reachable((uint32_t)code, k, s->fold))
                    s->h_lut[code] = kp_p_find(kp_a_onehot(code, k), patterns, P);
        }
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_pred_begin: the host table of " + std::to_string(k) + "-mers does not fit memory");
    }
    if (c) {
        KP_HIP(hipSetDevice(c->device));
        s->lut_ok = false;
        if ((rc = pred_arena(c, "kp_pred_begin", 0))) return rc;
    }
    s->active = true;
    return KP_OK;
}

int kp_pred_regions(kp_ctx *c, const uint8_t *seq, uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end,
                    uint64_t n_regions, const double *rates, uint64_t *hist, uint64_t *other, double *expected) {
    kp_pred_sess *s = pred_sess(c);
    int rc = scan_check_contig("kp_pred_regions", s->active, seq, n, "kp_pred_begin");
    if (rc) return rc;
    if (n_regions >= (1ull << 32)) return fail(KP_E_ARG, "kp_pred_regions: 2^32 regions or more in one call");
    if (n_regions && (!reg_begin || !reg_end || !other)) return fail(KP_E_ARG, "kp_pred_regions: null regions or counters");
    if (rates && n_regions && !expected) return fail(KP_E_ARG, "kp_pred_regions: rates without a place for the sums");
    if ((rc = scan_check_regions("kp_pred_regions", n, reg_begin, reg_end, n_regions, false))) return rc;
    if (!n_regions) return KP_OK;
    const int k = s->k;
    const uint32_t P = (uint32_t)s->pats.size();
    const uint32_t mask = (uint32_t)(s->cells - 1);
    uint64_t lo = 0, hi = 0;
    scan_centres(n, k, &lo, &hi);
    uint64_t n_items = 0;
    if (!c) {
        std::vector<uint64_t> row;
        try {
            row.resize(P);
        } catch (const std::bad_alloc &) {
            return fail(KP_E_NOMEM, "kp_pred_regions: a row of counters does not fit memory");
        }
        for (uint64_t r = 0; r < n_regions; ++r) {
            std::fill(row.begin(), row.end(), 0);
            uint64_t none = 0, inv = 0;
            for (uint64_t p = reg_begin[r]; p < reg_end[r]; ++p) {
                uint32_t code = 0;
                if (!kp_p_window(seq, n, p, k, s->fold, mask, &code)) {
                    ++inv;
                } else {
                    const int32_t j = s->h_lut[code];
                    if (j >= 0)
                        ++row[j];
                    else
                        ++none;
                }
            }
            n_items += scan_pieces(reg_begin[r], reg_end[r], lo, hi);
            other[2 * r] = none;
            other[2 * r + 1] = inv;
            s->st.unmatched += none;
            s->st.invalid += inv;
            s->st.assigned += reg_end[r] - reg_begin[r] - none - inv;
            if (hist) memcpy(hist + r * P, row.data(), (size_t)P * 8);
            if (rates) {
                double acc = 0.0;
                for (uint32_t p = 0; p < P; ++p) acc = acc + (double)row[p] * rates[p];
                expected[r] = acc;
            }
        }
        s->st.items += n_items;
        return KP_OK;
    }

    KP_HIP(hipSetDevice(c->device));
    const long lds_p = env_int("KP_PRED_LDS_P", KP_P_LDS_P);
    if (lds_p < 0 || lds_p > KP_P_LDS_P)
        return fail(KP_E_ARG, "kp_pred_regions: KP_PRED_LDS_P must be 0..16384 (uint32 counters beside a second workgroup's)");
    const bool lds = env_int("KP_PRED_GLOBAL", 0) == 0 && (long)P <= lds_p;
    std::vector<kp_p_item> items;
    std::vector<uint64_t> off_contig;  // per region: centres outside [lo, hi)
    try {
        off_contig.resize(n_regions);
        for (uint64_t r = 0; r < n_regions; ++r)
            off_contig[r] = reg_end[r] - reg_begin[r] - scan_cut(items, reg_begin[r], reg_end[r], lo, hi, (uint32_t)r);
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_pred_regions: the work items do not fit host memory");
    }
    if (items.size() >= (1ull << 32)) return fail(KP_E_ARG, "kp_pred_regions: 2^32 work items or more in one call");
    const size_t cnts = (size_t)n_regions * P;
    const size_t b_hist = g_up(cnts * 8), b_other = g_up(n_regions * 16);
    const size_t b_rates = rates ? g_up((size_t)P * 8) : 0, b_exp = rates ? g_up(n_regions * 8) : 0;
    if ((rc = pred_arena(c, "kp_pred_regions", b_hist + b_other + b_rates + b_exp))) return rc;
    unsigned long long *d_hist = (unsigned long long *)c->arena.take(cnts * 8);
    unsigned long long *d_other = (unsigned long long *)c->arena.take(n_regions * 16);
    double *d_rates = rates ? (double *)c->arena.take((size_t)P * 8) : nullptr;
    double *d_exp = rates ? (double *)c->arena.take(n_regions * 8) : nullptr;
    if ((rc = c->arena.check("kp_pred_regions"))) return rc;
    hipStream_t st = c->stream;
    KP_HIP(hipMemsetAsync(d_hist, 0, cnts * 8, st));
    KP_HIP(hipMemsetAsync(d_other, 0, n_regions * 16, st));
    if (!items.empty()) {
        uint8_t *d_seq = nullptr;
        kp_p_item *d_items = nullptr;
        if ((rc = scan_upload(c, "kp_pred_regions", seq, n, items, 0, &d_seq, &d_items))) return rc;
        const size_t lds_bytes = lds ? (size_t)P * 4 : 0;
        const uint64_t grid = scan_grid(c, items.size(), scan_per_cu(lds_bytes), "KP_PRED_GRID");
        kp_p_args A;
        A.seq = d_seq;
        A.items = d_items;
        A.n_items = (uint32_t)items.size();
        A.steps = (uint32_t)((items.size() + grid - 1) / grid);
        A.k = k;
        A.fold = s->fold;
        A.mask = mask;
        A.P = P;
        A.lut = s->d_lut;
        A.hist = d_hist;
        A.other = d_other;
        if ((rc = scan_mark(c, 0))) return rc;
        if (lds)
            hipLaunchKernelGGL((kp_pred_scan_kernel<true>), dim3((unsigned)grid), dim3(KP_S_THREADS), lds_bytes, st, A);
        else
            hipLaunchKernelGGL((kp_pred_scan_kernel<false>), dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
        if ((rc = scan_launched(c, 1))) return rc;
    }
    if (rates) {
        KP_HIP(hipMemcpyAsync(d_rates, rates, (size_t)P * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(kp_pred_sums_kernel, dim3((unsigned)((n_regions + 63) / 64)), dim3(64), 0, st, d_hist, d_rates, P,
                           n_regions, d_exp);
        KP_HIP(hipGetLastError());
        KP_HIP(hipMemcpyAsync(expected, d_exp, n_regions * 8, hipMemcpyDeviceToHost, st));
    }
    if (hist) KP_HIP(hipMemcpyAsync(hist, d_hist, cnts * 8, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(other, d_other, n_regions * 16, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    if (!items.empty()) {
        float ms = 0.f;
        if ((rc = scan_elapsed(c, 0, 1, &ms))) return rc;
        s->st.scan_ms += ms;
        s->st.path = lds ? 1u : 2u;
    }
    for (uint64_t r = 0; r < n_regions; ++r) {
        other[2 * r + 1] += off_contig[r];
        s->st.unmatched += other[2 * r];
        s->st.invalid += other[2 * r + 1];
        s->st.assigned += reg_end[r] - reg_begin[r] - other[2 * r] - other[2 * r + 1];
    }
    s->st.items += items.size();
    return KP_OK;
}

int kp_pred_track(kp_ctx *c, const uint8_t *seq, uint64_t n, uint64_t begin, uint64_t end, int32_t *pid) {
    kp_pred_sess *s = pred_sess(c);
    int rc = scan_check_contig("kp_pred_track", s->active, seq, n, "kp_pred_begin");
    if (rc) return rc;
    if (begin > end || end > n) return fail(KP_E_ARG, "kp_pred_track: begin > end or a range outside the contig");
    const uint64_t len = end - begin;
    if (!len) return KP_OK;
    if (!pid) return fail(KP_E_ARG, "kp_pred_track: null output");
    const int k = s->k;
    const uint32_t mask = (uint32_t)(s->cells - 1);
    const uint64_t n_items = scan_tiles(len);
    if (!c) {
        for (uint64_t i = 0; i < len; ++i) {
            uint32_t code = 0;
            pid[i] = kp_p_window(seq, n, begin + i, k, s->fold, mask, &code) ? s->h_lut[code] : KP_P_INVALID;
        }
        s->st.items += n_items;
        return KP_OK;
    }
    KP_HIP(hipSetDevice(c->device));
    if ((rc = pred_arena(c, "kp_pred_track", g_up(len * 4)))) return rc;
    int32_t *d_pid = (int32_t *)c->arena.take(len * 4);
    if ((rc = c->arena.check("kp_pred_track"))) return rc;
    uint8_t *d_seq = nullptr;
    if ((rc = scan_upload(c, "kp_pred_track", seq, n, {}, 0, &d_seq, nullptr))) return rc;
    hipStream_t st = c->stream;
    const uint64_t grid = scan_grid(c, n_items, 4, "KP_PRED_GRID");  // 33 KB of LDS per workgroup
    uint64_t lo = 0, hi = 0;
    scan_centres(n, k, &lo, &hi);
    kp_p_targs A;
    A.seq = d_seq;
    A.begin = (uint32_t)begin;
    A.len = (uint32_t)len;
    A.lo = (uint32_t)lo;
    A.hi = (uint32_t)hi;
    A.n_items = (uint32_t)n_items;
    A.steps = (uint32_t)((n_items + grid - 1) / grid);
    A.k = k;
    A.fold = s->fold;
    A.mask = mask;
    A.lut = s->d_lut;
    A.pid = d_pid;
    if ((rc = scan_mark(c, 0))) return rc;
    hipLaunchKernelGGL(kp_pred_track_kernel, dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
    if ((rc = scan_launched(c, 1))) return rc;
    KP_HIP(hipMemcpyAsync(pid, d_pid, len * 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    if ((rc = scan_elapsed(c, 0, 1, &ms))) return rc;
    s->st.scan_ms += ms;
    s->st.items += n_items;
    return KP_OK;
}

int kp_pred_sites(kp_ctx *c, const uint8_t *seq, uint64_t n, const uint64_t *pos, uint64_t n_sites, int32_t *pid) {
    kp_pred_sess *s = pred_sess(c);
    int rc = scan_check_contig("kp_pred_sites", s->active, seq, n, "kp_pred_begin");
    if (rc) return rc;
    if (n_sites && (!pos || !pid)) return fail(KP_E_ARG, "kp_pred_sites: null positions or output");
    if (n_sites >= (1ull << 39)) return fail(KP_E_ARG, "kp_pred_sites: 2^39 sites or more in one call");
    for (uint64_t i = 0; i < n_sites; ++i)
        if (pos[i] >= n)
            return fail(KP_E_ARG, "kp_pred_sites: site " + std::to_string(i) + " at " + std::to_string(pos[i]) +
                                      " lies past the contig's " + std::to_string(n) + " bases");
    if (!n_sites) return KP_OK;
    const int k = s->k;
    const uint32_t mask = (uint32_t)(s->cells - 1);
    if (!c) {
        for (uint64_t i = 0; i < n_sites; ++i) {
            uint32_t code = 0;
            pid[i] = kp_p_window(seq, n, pos[i], k, s->fold, mask, &code) ? s->h_lut[code] : KP_P_INVALID;
        }
        return KP_OK;
    }
    KP_HIP(hipSetDevice(c->device));
    if ((rc = pred_arena(c, "kp_pred_sites", g_up(n_sites * 4)))) return rc;
    int32_t *d_pid = (int32_t *)c->arena.take(n_sites * 4);
    if ((rc = c->arena.check("kp_pred_sites"))) return rc;
    uint8_t *d_seq = nullptr;
    if ((rc = scan_upload(c, "kp_pred_sites", seq, n, {}, g_up(n_sites * 8), &d_seq, nullptr))) return rc;
    uint64_t *d_pos = (uint64_t *)c->seq_in.take(n_sites * 8);
    if ((rc = c->seq_in.check("kp_pred_sites"))) return rc;
    hipStream_t st = c->stream;
    KP_HIP(hipMemcpyAsync(d_pos, pos, n_sites * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kp_pred_sites_kernel, dim3((unsigned)((n_sites + 255) / 256)), dim3(256), 0, st, d_seq, n, d_pos,
                       n_sites, k, s->fold, mask, s->d_lut, d_pid);
    KP_HIP(hipGetLastError());
    KP_HIP(hipMemcpyAsync(pid, d_pid, n_sites * 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    return KP_OK;
}

int kp_pred_end(kp_ctx *c) {
    kp_pred_sess *s = pred_sess(c);
    if (!s->active) return fail(KP_E_STATE, "kp_pred_end: no session (kp_pred_begin first)");
    s->active = false;
    s->lut_ok = false;
    std::vector<int32_t>().swap(s->h_lut);
    std::vector<uint64_t>().swap(s->pats);
    return KP_OK;
}

int kp_pred_last_stats(kp_ctx *c, kp_pred_stats *out) {
    if (!out) return fail(KP_E_ARG, "kp_pred_last_stats: null out");
    *out = pred_sess(c)->st;
    return KP_OK;
}

int kp_pred_host(int k, int fold, const uint64_t *patterns, uint32_t n_patterns, uint64_t super_word,
                 const uint8_t *seq, uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end, uint64_t n_regions,
                 const double *rates, uint64_t *hist, uint64_t *other, double *expected, uint64_t track_begin,
                 uint64_t track_end, int32_t *track_pid, const uint64_t *pos, uint64_t n_sites, int32_t *site_pid,
                 kp_pred_stats *stats) {
    int rc = kp_pred_begin(nullptr, k, fold, patterns, n_patterns, super_word);
    if (rc) return rc;
    rc = kp_pred_regions(nullptr, seq, n, reg_begin, reg_end, n_regions, rates, hist, other, expected);
    if (!rc && track_pid) rc = kp_pred_track(nullptr, seq, n, track_begin, track_end, track_pid);
    if (!rc) rc = kp_pred_sites(nullptr, seq, n, pos, n_sites, site_pid);
    const std::string err = g_err;
    const int rc_end = kp_pred_end(nullptr);
    if (rc) return fail(rc, err);
    if (stats) *stats = g_pred_host.st;
    return rc_end;
}

}  // extern "C"
