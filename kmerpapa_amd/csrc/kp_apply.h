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
