// kp_apply.h -- apply a fitted partition to a k-mer count table (no reference counterpart
// beyond papa.PatternPartition's constructor checks, src/kmerpapa/papa.py:53-107, and the
// per-pattern sums of pattern_utils.get_M_U :192-215).  Included by kp_hip.hip.
//
// Nothing is enumerated: a k-mer is a one-hot word (4 bits per position, position 0 lowest,
// A = 1, C = 2, G = 4, T = 8) and a pattern the word of 4-bit masks kp_greedy uses, so a k-mer
// matches a pattern when (onehot & ~mask) == 0.  The table may be sparse and needs no zero fill.
//
//   kp_apply_assign  one row per thread and step: the row's one-hot word against every
//                    pattern (staged through LDS in tiles, or read through the scalar cache
//                    with tile = 0); first match and number of matches, no early exit.  A row
//                    of exactly one match adds its count columns to that pattern's uint64
//                    totals -- in LDS counters of the workgroup, flushed with one global
//                    atomic per non-zero counter, or with global atomics directly (the host
//                    picks what takes fewer global atomics); any other row goes into the
//                    unmatched / multi error counters only
//   kp_apply_pairs   pattern pairs i < j that share a k-mer (every nibble of w_i & w_j
//                    non-zero), and patterns that are not sub-patterns of the super pattern
//   kp_apply_terms   xlogy(M, p) + xlog1py(U, -p) per (pattern, column), in parallel
//   kp_apply_sums    one thread per column: the terms added in pattern order from 0.0, then
//                    -2 * acc + 0.0 -- score_utils.get_loss with penalty 0, bit for bit
//
// Every count is a uint64 and every sum an integer sum (column totals below 2^63 are checked
// by the caller), so the order of the atomics does not matter.  Every device loop has a bound
// the host computed; there are no waits between workgroups.  kp_apply_host runs the same
// __host__ __device__ text serially on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp_core.h"
#include "kp_rt.h"

#define KP_A_MAXK 16
#define KP_A_THREADS 512
#define KP_A_TILE 1024  // patterns per LDS tile by default (KP_APPLY_TILE)

// the one-hot word of a KmerCounts code (2 bits per letter, first letter most significant)
__host__ __device__ inline uint64_t kp_a_onehot(uint64_t code, int k) {
    uint64_t w = 0;
    for (int i = 0; i < k; ++i) w |= 1ull << (4 * i + (int)((code >> (2 * (k - 1 - i))) & 3u));
    return w;
}

__host__ __device__ inline bool kp_a_match(uint64_t onehot, uint64_t pat) { return (onehot & ~pat) == 0; }

// 0x1111... over k positions
__host__ __device__ inline uint64_t kp_a_low(int k) { return 0x1111111111111111ull >> (4 * (KP_A_MAXK - k)); }

// every one of the k nibbles of w is non-zero
__host__ __device__ inline bool kp_a_full(uint64_t w, uint64_t low) {
    return (((w | (w >> 1) | (w >> 2) | (w >> 3)) & low) == low);
}

// two patterns share a k-mer
__host__ __device__ inline bool kp_a_overlap(uint64_t a, uint64_t b, uint64_t low) { return kp_a_full(a & b, low); }

// the term of one pattern in score_utils.get_loss :37-38
__host__ __device__ inline double kp_a_term(uint64_t M, uint64_t U, double p) {
    return kp_xlogy((double)M, p) + kp_xlog1py((double)U, -p);
}

// pid of a row from its first match and number of matches
__host__ __device__ inline int32_t kp_a_pid(uint32_t first, uint32_t cnt) {
    return cnt == 1 ? (int32_t)first : (cnt ? -2 : -1);
}

struct kp_a_args {
    const uint64_t *codes;  // [n]
    const int64_t *M, *U;   // [n][ncol]
    uint64_t n;
    int32_t k, ncol;
    const uint64_t *pats;  // [P]
    uint32_t P;
    uint32_t tile;   // patterns per LDS tile; 0 = no LDS, the patterns come through the scalar cache
    uint32_t steps;  // rows per thread: step s of workgroup b is row block s * gridDim.x + b
    int32_t *pid;    // [n] or null
    unsigned long long *tot;  // [2][P][ncol]: M totals, then U totals
    unsigned long long *err;  // [0] unmatched, [1] multi
};

#ifdef __HIPCC__

template <bool LDSC, bool TILED>
__global__ void __launch_bounds__(KP_A_THREADS) kp_apply_assign(kp_a_args A) {
    extern __shared__ unsigned long long kp_a_smem[];
    unsigned long long *sT = kp_a_smem;           // [tile]
    unsigned long long *sC = kp_a_smem + A.tile;  // [2][P][ncol] with LDSC
    const uint32_t tid = threadIdx.x;
    const uint32_t ncnt = 2u * A.P * (uint32_t)A.ncol;
    if (LDSC) {
        for (uint32_t e = tid; e < ncnt; e += KP_A_THREADS) sC[e] = 0;
        __syncthreads();
    }
    unsigned long long *C = LDSC ? sC : A.tot;
    uint32_t n_un = 0, n_mu = 0;  // of this wave (every lane holds the same numbers)
    for (uint32_t s = 0; s < A.steps; ++s) {
        const uint64_t row = ((uint64_t)s * gridDim.x + blockIdx.x) * KP_A_THREADS + tid;
        const bool act = row < A.n;
        const uint64_t oh = act ? kp_a_onehot(A.codes[row], A.k) : 0;
        uint32_t first = 0, cnt = 0;
        if (TILED) {
            for (uint32_t t0 = 0; t0 < A.P; t0 += A.tile) {
                const uint32_t nt = A.P - t0 < A.tile ? A.P - t0 : A.tile;
                __syncthreads();  // the previous tile has been read by every wave
                for (uint32_t e = tid; e < nt; e += KP_A_THREADS) sT[e] = A.pats[t0 + e];
                __syncthreads();
#pragma unroll 8
                for (uint32_t j = 0; j < nt; ++j) {
                    const bool m = kp_a_match(oh, sT[j]);
                    first = (m && !cnt) ? t0 + j : first;
                    cnt += m;
                }
            }
        } else {
#pragma unroll 8
            for (uint32_t j = 0; j < A.P; ++j) {
                const bool m = kp_a_match(oh, A.pats[j]);
                first = (m && !cnt) ? j : first;
                cnt += m;
            }
        }
        if (act && A.pid) A.pid[row] = kp_a_pid(first, cnt);
        if (act && cnt == 1) {
            const uint32_t half = A.P * (uint32_t)A.ncol;
            for (int c = 0; c < A.ncol; ++c) {
                const unsigned long long m = (unsigned long long)A.M[row * A.ncol + c];
                const unsigned long long u = (unsigned long long)A.U[row * A.ncol + c];
                const uint32_t d = first * (uint32_t)A.ncol + c;
                if (m) atomicAdd(&C[d], m);
                if (u) atomicAdd(&C[half + d], u);
            }
        }
        n_un += (uint32_t)__popcll(__ballot(act && cnt == 0));
        n_mu += (uint32_t)__popcll(__ballot(act && cnt > 1));
    }
    if ((tid & 63u) == 0) {  // one atomic per wave and counter
        if (n_un) atomicAdd(&A.err[0], (unsigned long long)n_un);
        if (n_mu) atomicAdd(&A.err[1], (unsigned long long)n_mu);
    }
    if (LDSC) {
        __syncthreads();
        for (uint32_t e = tid; e < ncnt; e += KP_A_THREADS) {
            const unsigned long long v = sC[e];
            if (v) atomicAdd(&A.tot[e], v);
        }
    }
}

// out[0] += pairs i < j that share a k-mer, out[1] += patterns outside the super pattern.
// Thread i runs j over [its block's first pattern + 1, P): the pattern of j is the same for
// the whole wave and comes through the scalar cache.
__global__ void __launch_bounds__(256) kp_apply_pairs(const uint64_t *__restrict__ pats, uint32_t P, int k,
                                                      uint64_t super_word, unsigned long long *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool act = i < P;
    const uint64_t wi = act ? pats[i] : 0;
    const uint64_t low = kp_a_low(k);
    unsigned long long pairs = 0;
    for (uint32_t j = blockIdx.x * 256u + 1; j < P; ++j) pairs += (act && j > i && kp_a_overlap(wi, pats[j], low)) ? 1u : 0u;
    unsigned long long outside = (act && (wi & ~super_word) != 0) ? 1u : 0u;
    for (int off = 32; off; off >>= 1) {
        pairs += __shfl_xor(pairs, off, 64);
        outside += __shfl_xor(outside, off, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (pairs) atomicAdd(&out[0], pairs);
        if (outside) atomicAdd(&out[1], outside);
    }
}

// terms[c][p] of pattern p and column c; tot as kp_a_args::tot
__global__ void __launch_bounds__(256) kp_apply_terms(const unsigned long long *__restrict__ tot,
                                                      const double *__restrict__ rates, uint32_t P, int ncol,
                                                      double *__restrict__ terms) {
    const uint64_t total = (uint64_t)P * (uint64_t)ncol;
    const uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (e >= total) return;
    const uint32_t p = (uint32_t)(e / (uint64_t)ncol);
    const int c = (int)(e % (uint64_t)ncol);
    terms[(uint64_t)c * P + p] = kp_a_term(tot[e], tot[total + e], rates[p]);
}

__global__ void __launch_bounds__(64) kp_apply_sums(const double *__restrict__ terms, uint32_t P, int ncol,
                                                    double *__restrict__ ll) {
    const int col = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (col >= ncol) return;
    const double *t = terms + (uint64_t)col * P;
    double s = 0.0;
    uint32_t i = 0;
    for (; i + 8 <= P; i += 8) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = t[i + q];
#pragma unroll
        for (int q = 0; q < 8; ++q) s += v[q];
    }
    for (; i < P; ++i) s += t[i];
    ll[col] = -2.0 * s + 0.0;  // get_loss :39 adds len(L) * 0: a -0.0 becomes 0.0
}

#endif  // __HIPCC__

// ---------------------------------------------------------------------------
// a fitted partition applied to a count table (kp_apply.h)
// ---------------------------------------------------------------------------

// every nibble of the k positions non-zero, nothing above them
static bool apply_word_ok(uint64_t w, int k) {
    return kp_a_full(w, kp_a_low(k)) && (k == KP_A_MAXK || (w >> (4 * k)) == 0);
}

// Arguments of kp_apply / kp_apply_host.
static int apply_check(const char *who, int k, const uint64_t *patterns, uint32_t P, uint64_t super_word,
                       const uint64_t *codes, const int64_t *M, const int64_t *U, uint64_t n, int ncol,
                       const double *rates, uint64_t *pat_M, uint64_t *pat_U, double *ll, kp_apply_stats *stats) {
    const std::string w(who);
    if (k < 1 || k > KP_A_MAXK) return fail(KP_E_ARG, w + ": k must be 1..16 (a pattern is a 64-bit word of 4-bit masks)");
    if (P == 0) return fail(KP_E_ARG, w + ": no patterns");
    if (!patterns || !pat_M || !pat_U || !stats || ncol < 1 || (n && (!codes || !M || !U)) || (rates && !ll))
        return fail(KP_E_ARG, w + ": bad arguments");
    if (2ull * P * (uint64_t)ncol >= (1ull << 31)) return fail(KP_E_ARG, w + ": patterns x columns of 2^30 or more");
    for (uint32_t i = 0; i < P; ++i)
        if (!apply_word_ok(patterns[i], k))
            return fail(KP_E_ARG, w + ": pattern " + std::to_string(i) + " has an empty position or bits above position k");
    if (!apply_word_ok(super_word, k)) return fail(KP_E_ARG, w + ": the super pattern has an empty position or bits above position k");
    const uint64_t lim = 1ull << 63;
    for (uint64_t i = 0; i < n; ++i)
        if (codes[i] >> (2 * k)) return fail(KP_E_ARG, w + ": k-mer code of row " + std::to_string(i) + " has bits above 2k");
    for (int c = 0; c < ncol; ++c) {
        uint64_t sm = 0, su = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const int64_t m = M[i * ncol + c], u = U[i * ncol + c];
            if (m < 0 || u < 0) return fail(KP_E_ARG, w + ": negative count in row " + std::to_string(i));
            sm += (uint64_t)m;
            su += (uint64_t)u;
            if (sm >= lim || su >= lim) return fail(KP_E_ARG, w + ": a column total of 2^63 or more");
        }
    }
    return KP_OK;
}

template <bool LDSC, bool TILED>
static int apply_launch(hipStream_t st, const kp_a_args &A, unsigned grid, size_t lds) {
    if (lds > 65536)
        KP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&kp_apply_assign<LDSC, TILED>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((kp_apply_assign<LDSC, TILED>), dim3(grid), dim3(KP_A_THREADS), lds, st, A);
    KP_HIP(hipGetLastError());
    return KP_OK;
}

extern "C" {

int kp_apply_host(int k, const uint64_t *patterns, uint32_t n_patterns, uint64_t super_word, const uint64_t *codes,
                  const int64_t *M, const int64_t *U, uint64_t n, int ncol, const double *rates, int32_t *pid,
                  uint64_t *pat_M, uint64_t *pat_U, double *ll, kp_apply_stats *stats) {
    const uint32_t P = n_patterns;
    int rc = apply_check("kp_apply_host", k, patterns, P, super_word, codes, M, U, n, ncol, rates, pat_M, pat_U, ll, stats);
    if (rc) return rc;
    *stats = kp_apply_stats{};
    for (uint64_t e = 0; e < (uint64_t)P * ncol; ++e) pat_M[e] = pat_U[e] = 0;
    for (uint64_t row = 0; row < n; ++row) {
        const uint64_t oh = kp_a_onehot(codes[row], k);
        uint32_t first = 0, cnt = 0;
        for (uint32_t j = 0; j < P; ++j) {
            const bool m = kp_a_match(oh, patterns[j]);
            first = (m && !cnt) ? j : first;
            cnt += m;
        }
        if (pid) pid[row] = kp_a_pid(first, cnt);
        if (cnt == 1) {
            for (int c = 0; c < ncol; ++c) {
                pat_M[(uint64_t)first * ncol + c] += (uint64_t)M[row * ncol + c];
                pat_U[(uint64_t)first * ncol + c] += (uint64_t)U[row * ncol + c];
            }
        } else if (cnt == 0) {
            ++stats->unmatched;
        } else {
            ++stats->multi;
        }
    }
    const uint64_t low = kp_a_low(k);
    for (uint32_t i = 0; i < P; ++i) {
        for (uint32_t j = i + 1; j < P; ++j) stats->overlap_pairs += kp_a_overlap(patterns[i], patterns[j], low);
        stats->outside_super += (patterns[i] & ~super_word) != 0;
    }
    if (rates)
        for (int c = 0; c < ncol; ++c) {
            double s = 0.0;
            for (uint32_t p = 0; p < P; ++p) s += kp_a_term(pat_M[(uint64_t)p * ncol + c], pat_U[(uint64_t)p * ncol + c], rates[p]);
            ll[c] = -2.0 * s + 0.0;
        }
    return KP_OK;
}

int kp_apply(kp_ctx *c, int k, const uint64_t *patterns, uint32_t n_patterns, uint64_t super_word,
             const uint64_t *codes, const int64_t *M, const int64_t *U, uint64_t n, int ncol, const double *rates,
             int32_t *pid, uint64_t *pat_M, uint64_t *pat_U, double *ll, kp_apply_stats *stats) {
    if (!c) return fail(KP_E_ARG, "kp_apply: null ctx");
    if (c->seq.active) return fail(KP_E_STATE, "kp_apply: a kp_seq session holds the context's arena (kp_seq_end first)");
    if (c->pred.active) return fail(KP_E_STATE, "kp_apply: a kp_pred session holds the context's arena (kp_pred_end first)");
    if (c->spec.active) return fail(KP_E_STATE, "kp_apply: a kp_spec session holds the context's arena (kp_spec_end first)");
    if (c->ispec.active) return fail(KP_E_STATE, "kp_apply: a kp_ispec session holds the context's arena (kp_ispec_end first)");
    const uint32_t P = n_patterns;
    int rc = apply_check("kp_apply", k, patterns, P, super_word, codes, M, U, n, ncol, rates, pat_M, pat_U, ll, stats);
    if (rc) return rc;
    *stats = kp_apply_stats{};
    KP_HIP(hipSetDevice(c->device));

    // launch shape: the tile, where the totals are summed, the grid (KP_APPLY_* knobs)
    const long tile_env = env_int("KP_APPLY_TILE", KP_A_TILE);
    if (tile_env < 0 || tile_env > 4096) return fail(KP_E_ARG, "kp_apply: KP_APPLY_TILE must be 0..4096 patterns");
    const uint32_t tile = (uint32_t)tile_env;
    const size_t cells = (size_t)P * (size_t)ncol;
    const size_t lds_all = (size_t)tile * 8 + 2 * cells * 8;
    const bool fits = lds_all <= c->lds_max;
    const bool force_global = env_int("KP_APPLY_GLOBAL", 0) != 0;
    const long lds_env = env_int("KP_APPLY_LDS", -1);
    if (lds_env > 0 && (force_global || !fits))
        return fail(KP_E_ARG, force_global ? "kp_apply: KP_APPLY_LDS=1 and KP_APPLY_GLOBAL=1 contradict each other"
                                           : "kp_apply: KP_APPLY_LDS=1, but the counters (" + std::to_string(lds_all) +
                                                 " bytes with the tile) do not fit LDS");
    const uint64_t blocks = (n + KP_A_THREADS - 1) / KP_A_THREADS;
    const long grid_env = env_int("KP_APPLY_GRID", 0);
    auto grid_for = [&](size_t lds_bytes) {  // a persistent grid: as many workgroups as are resident at once
        const int per_cu = lds_bytes <= 40u * 1024u ? 4 : (lds_bytes <= 80u * 1024u ? 2 : 1);
        uint64_t g = std::min<uint64_t>(blocks, (uint64_t)c->cus * per_cu);
        return grid_env > 0 ? std::min<uint64_t>(g, (uint64_t)grid_env) : g;
    };
    bool ldsc = !force_global && lds_env != 0 && fits;
    // unless forced: LDS counters only where they save global atomics -- every workgroup
    // flushes up to 2 P ncol counters, adding directly takes up to 2 ncol atomics per row
    // (a sparse table against many patterns: 1.31 against 1.83 ms)
    if (ldsc && lds_env < 0 && grid_for(lds_all) * 2 * cells > 2 * n * (uint64_t)ncol) ldsc = false;
    const size_t lds = ldsc ? lds_all : (size_t)tile * 8;
    const uint64_t grid = grid_for(lds);
    const uint64_t steps = grid ? (blocks + grid - 1) / grid : 0;
    if (steps >= (1ull << 32)) return fail(KP_E_ARG, "kp_apply: too many rows for the grid");

    // device buffers: one arena
    const size_t b_codes = g_up(n * 8), b_cnt = g_up(n * (size_t)ncol * 8), b_pid = pid ? g_up(n * 4) : 0;
    const size_t b_pats = g_up((size_t)P * 8), b_tot = g_up(2 * cells * 8), b_terms = rates ? g_up(cells * 8) : 0;
    const size_t b_ll = rates ? g_up((size_t)ncol * 8) : 0, b_rates = rates ? b_pats : 0;
    const size_t need = b_codes + 2 * b_cnt + b_pid + b_pats + b_tot + g_up(32) + b_rates + b_terms + b_ll;
    {
        size_t fr = 0, tot = 0;
        KP_HIP(hipMemGetInfo(&fr, &tot));
        if (need > fr + c->arena.bytes)
            return fail(KP_E_NOMEM, "kp_apply: the table and the partition need " + std::to_string(need >> 20) +
                                        " MiB of device memory, " + std::to_string((fr + c->arena.bytes) >> 20) + " MiB are free");
    }
    // (the arena shared with kp_greedy; every size above is already rounded as take() rounds)
    if ((rc = c->arena.reserve("kp_apply", need))) return rc;
    auto take = [&](size_t bytes) { return c->arena.take(bytes); };
    uint64_t *d_codes = (uint64_t *)take(b_codes);
    int64_t *dM = (int64_t *)take(b_cnt), *dU = (int64_t *)take(b_cnt);
    int32_t *d_pid = pid ? (int32_t *)take(b_pid) : nullptr;
    uint64_t *d_pats = (uint64_t *)take(b_pats);
    unsigned long long *d_tot = (unsigned long long *)take(b_tot);
    unsigned long long *d_err = (unsigned long long *)take(g_up(32));  // unmatched, multi, pairs, outside
    double *d_rates = rates ? (double *)take(b_rates) : nullptr;
    double *d_terms = rates ? (double *)take(b_terms) : nullptr;
    double *d_ll = rates ? (double *)take(b_ll) : nullptr;
    if ((rc = c->arena.check("kp_apply"))) return rc;

    hipStream_t st = c->stream;
    KP_HIP(hipMemcpyAsync(d_pats, patterns, (size_t)P * 8, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemsetAsync(d_tot, 0, 2 * cells * 8, st));
    KP_HIP(hipMemsetAsync(d_err, 0, 32, st));
    if (n) {
        KP_HIP(hipMemcpyAsync(d_codes, codes, n * 8, hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(dM, M, n * (size_t)ncol * 8, hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(dU, U, n * (size_t)ncol * 8, hipMemcpyHostToDevice, st));
        kp_a_args A;
        A.codes = d_codes;
        A.M = dM;
        A.U = dU;
        A.n = n;
        A.k = k;
        A.ncol = ncol;
        A.pats = d_pats;
        A.P = P;
        A.tile = tile;
        A.steps = (uint32_t)steps;
        A.pid = d_pid;
        A.tot = d_tot;
        A.err = d_err;
        KP_HIP(hipEventRecord(c->ev[0], st));
        if (ldsc)
            rc = tile ? apply_launch<true, true>(st, A, (unsigned)grid, lds) : apply_launch<true, false>(st, A, (unsigned)grid, lds);
        else
            rc = tile ? apply_launch<false, true>(st, A, (unsigned)grid, lds) : apply_launch<false, false>(st, A, (unsigned)grid, lds);
        if (rc) return rc;
        KP_HIP(hipEventRecord(c->ev[1], st));
    }
    hipLaunchKernelGGL(kp_apply_pairs, dim3((P + 255) / 256), dim3(256), 0, st, d_pats, P, k, super_word, d_err + 2);
    KP_HIP(hipGetLastError());
    if (rates) {
        KP_HIP(hipMemcpyAsync(d_rates, rates, (size_t)P * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(kp_apply_terms, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, d_tot, d_rates, P, ncol,
                           d_terms);
        KP_HIP(hipGetLastError());
        hipLaunchKernelGGL(kp_apply_sums, dim3((ncol + 63) / 64), dim3(64), 0, st, d_terms, P, ncol, d_ll);
        KP_HIP(hipGetLastError());
        KP_HIP(hipMemcpyAsync(ll, d_ll, (size_t)ncol * 8, hipMemcpyDeviceToHost, st));
    }
    unsigned long long h_err[4] = {0, 0, 0, 0};
    KP_HIP(hipMemcpyAsync(h_err, d_err, 32, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(pat_M, d_tot, cells * 8, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(pat_U, d_tot + cells, cells * 8, hipMemcpyDeviceToHost, st));
    if (pid && n) KP_HIP(hipMemcpyAsync(pid, d_pid, n * 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    stats->unmatched = h_err[0];
    stats->multi = h_err[1];
    stats->overlap_pairs = h_err[2];
    stats->outside_super = h_err[3];
    if (n) {
        float ms = 0.f;
        KP_HIP(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        stats->assign_ms = ms;
        stats->tiles = tile ? (uint32_t)((P + tile - 1) / tile) : 0;
        stats->lds_counters = ldsc ? 1u : 0u;
    }
    return KP_OK;
}
}  // extern "C"
