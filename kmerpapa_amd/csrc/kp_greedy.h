// kp_greedy.h -- the greedy top-down partition (reference
// src/kmerpapa/algorithms/greedy_penalty_plus_pseudo.py, v0.2.4: train_loss :18-25,
// test_logLik :28-35, greedy_res_kmer_table_ord :159-196).  Included by kp_hip.hip.
//
// There is no lattice: a lane is one tree grown from the general pattern over one count
// source (all data, or all data minus one fold) with its own (alpha, beta, penalty).  All
// lanes' trees grow breadth-first together, one depth per launch:
//
//   kp_greedy_tab        [n][nf] M / U  ->  tab[slot][row] = (M, U); slot nf' = all data
//   kp_greedy_hist       one wave per (node, chunk): H[pos][nuc] = (trM, trU, teM, teU) summed
//                        over the chunk's k-mers with 64-bit LDS atomics (a histogram per
//                        wave).  A node of one chunk is decided right there; a larger node's
//                        partial histograms are merged with integer atomics in global memory
//   kp_greedy_decide_big one wave per multi-chunk node: decide from the merged histogram
//   kp_greedy_finish     one workgroup per lane: leaf losses summed bottom-up as
//                        value(left) + value(right), leaf offsets top-down (left subtree
//                        first), the leaves' patterns and test terms written in that order
//   kp_greedy_chain      one thread per chain: the test terms added lane by lane, leaf by
//                        leaf, as the reference's `test_ll += this_ll` loop (:325-333)
//
// Every count is a uint64 and every histogram sum an integer sum, so the order of the
// atomics does not matter; the reference's float64 sums (get_M_U_kmer_table :86-92) are the
// same numbers while totals stay below 2^53 (larger totals are refused).  The decision of a
// node -- the two train_loss values of every (position, pair) candidate, their float64 sum,
// the first minimum in scan order, strict "<" against the node's own loss -- is the
// __host__ __device__ text below; kp_greedy_host runs the same text serially on the host.
// log is the C library's (kp_libm_log: numba lowers np.log to libm); float64 throughout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/kmerpapa_hip.h"
#include "kp_libm.h"

#define KP_G_MAXK 16
#define KP_G_MAXDEPTH (3 * KP_G_MAXK + 2)  // a split removes at least one nucleotide of one position
#define KP_G_WAVES 4
#define KP_G_HSIZE (KP_G_MAXK * 4 * 4)  // uint64 per histogram: [pos][nuc][trM, trU, teM, teU]
#define KP_G_ROWMASK 0x3fffffffu

// nucleotide bits of a position's mask: A = 1, C = 2, G = 4, T = 8
__host__ __device__ inline uint32_t kp_g_letter_mask(char c) {
    switch (c) {
    case 'A': return 1;
    case 'C': return 2;
    case 'G': return 4;
    case 'T': return 8;
    case 'M': return 3;
    case 'R': return 5;
    case 'S': return 6;
    case 'V': return 7;
    case 'W': return 9;
    case 'Y': return 10;
    case 'H': return 11;
    case 'K': return 12;
    case 'D': return 13;
    case 'B': return 14;
    case 'N': return 15;
    default: return 0;
    }
}

// The ordered two-way splits of a code (pattern_utils.py complements :48-57, the order of
// complements_tab_1/2): nibble j = first half of pair j (0 = no more pairs), the second
// half is the rest of the mask.
__host__ __device__ inline uint32_t kp_g_pairs(uint32_t mask) {
    switch (mask) {
    case 3: return 0x1;         // M: A C
    case 5: return 0x1;         // R: A G
    case 6: return 0x4;         // S: G C
    case 9: return 0x1;         // W: A T
    case 10: return 0x2;        // Y: C T
    case 12: return 0x4;        // K: G T
    case 7: return 0x421;       // V: A S, C R, G M
    case 11: return 0x821;      // H: A Y, C W, T M
    case 13: return 0x841;      // D: A K, G W, T R
    case 14: return 0x842;      // B: C K, G Y, T S
    case 15: return 0x84215c6;  // N: S W, K M, R Y, A B, C D, G H, T V
    default: return 0;
    }
}

// train_loss :18-25
__host__ __device__ inline double kp_g_train_loss(uint64_t Mi, uint64_t Ui, double alpha, double beta, double penalty) {
    const double M = (double)Mi, U = (double)Ui;
    const double p = (M + alpha) / (((M + U) + alpha) + beta);
    double s = penalty;
    if (M > 0) s += (-2.0 * M) * kp_libm_log(p);
    if (U > 0) s += (-2.0 * U) * kp_libm_log(1 - p);
    return s;
}

// test_logLik :28-35
__host__ __device__ inline double kp_g_test_ll(uint64_t trM, uint64_t trU, uint64_t teM, uint64_t teU, double alpha,
                                               double beta) {
    const double M = (double)trM, U = (double)trU;
    const double p = (M + alpha) / (((M + U) + alpha) + beta);
    double s = 0.0;
    if (teM > 0) s += (-2.0 * (double)teM) * kp_libm_log(p);
    if (teU > 0) s += (-2.0 * (double)teU) * kp_libm_log(1 - p);
    return s;
}

// out[0..4) = sum of H[pos][nuc][0..4) over the nucleotides of `mask`
__host__ __device__ inline void kp_g_sum(const uint64_t *H, int pos, uint32_t mask, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    for (int nuc = 0; nuc < 4; ++nuc)
        if (mask >> nuc & 1) {
            const uint64_t *h = H + (pos * 4 + nuc) * 4;
            out[0] += h[0];
            out[1] += h[1];
            out[2] += h[2];
            out[3] += h[3];
        }
}

// Candidate `code` = position * 8 + pair index (ascending code = the reference's scan order,
// :167-183).  False if the pattern has no such candidate; else the two halves' masks.
__host__ __device__ inline bool kp_g_cand(uint64_t pat, int k, int code, int *pos, uint32_t *a, uint32_t *b) {
    const int p = code >> 3, j = code & 7;
    if (p >= k || j >= 7) return false;
    const uint32_t mask = (uint32_t)(pat >> (4 * p)) & 15u;
    const uint32_t h = (kp_g_pairs(mask) >> (4 * j)) & 15u;
    if (!h) return false;
    *pos = p;
    *a = h;
    *b = mask ^ h;
    return true;
}

// s = loss1 + loss2 of a candidate (:175-178); +inf stands for "no candidate" and for a NaN
// sum, which the reference's `s < best_loss` never accepts either
__host__ __device__ inline double kp_g_cand_loss(const uint64_t *H, uint64_t pat, int k, int code, double alpha,
                                                 double beta, double penalty) {
    int pos;
    uint32_t a, b;
    if (!kp_g_cand(pat, k, code, &pos, &a, &b)) return __builtin_inf();
    uint64_t c1[4], c2[4];
    kp_g_sum(H, pos, a, c1);
    kp_g_sum(H, pos, b, c2);
    const double s = kp_g_train_loss(c1[0], c1[1], alpha, beta, penalty) +
                     kp_g_train_loss(c2[0], c2[1], alpha, beta, penalty);
    return s != s ? __builtin_inf() : s;
}

// the tie rule of the scan: the smaller value, then the earlier candidate
__host__ __device__ inline bool kp_g_better(double s1, int c1, double s2, int c2) {
    return s1 < s2 || (s1 == s2 && c1 < c2);
}

__host__ __device__ inline uint64_t kp_g_generality(uint64_t pat, int k) {
    uint64_t g = 1;
    for (int i = 0; i < k; ++i) g *= (uint64_t)__builtin_popcount((uint32_t)(pat >> (4 * i)) & 15u);
    return g;
}

// how the k-mers of the general pattern are numbered (KmerEnumeration = matches() order):
// row = sum_i dig[i][nuc_i] * cg[i], dig = the nucleotide's index in code[g_i]
struct kp_g_root {
    int32_t k;
    uint32_t cg[KP_G_MAXK];
    uint8_t dig[KP_G_MAXK][4];
    uint64_t pat;
};

// nuc = the d-th nucleotide of `mask` (ascending bit order)
__host__ __device__ inline int kp_g_nth_nuc(uint32_t mask, int d) {
    for (int nuc = 0; nuc < 4; ++nuc)
        if (mask >> nuc & 1) {
            if (!d) return nuc;
            --d;
        }
    return 0;
}

static bool kp_g_make_root(const char *gen_pat, kp_g_root *R) {
    const size_t k = strlen(gen_pat);
    if (k < 1 || k > KP_G_MAXK) return false;
    memset(R, 0, sizeof(*R));
    R->k = (int32_t)k;
    uint64_t w = 1;
    for (size_t i = 0; i < k; ++i) {
        const uint32_t m = kp_g_letter_mask(gen_pat[i]);
        if (!m) return false;
        R->pat |= (uint64_t)m << (4 * i);
        R->cg[i] = (uint32_t)w;
        int d = 0;
        for (int nuc = 0; nuc < 4; ++nuc) R->dig[i][nuc] = 0;
        if (m == 6) {  // code["S"] = "GC": G first
            R->dig[i][2] = 0;
            R->dig[i][1] = 1;
        } else {
            for (int nuc = 0; nuc < 4; ++nuc)
                if (m >> nuc & 1) R->dig[i][nuc] = (uint8_t)d++;
        }
        w *= (uint64_t)__builtin_popcount(m);
        if (w > (1ull << 30)) return false;
    }
    return true;
}

struct kp_g_node {
    uint64_t pat;
    uint64_t c[4];  // trM, trU, teM, teU of the pattern
    double value;   // own loss; after kp_greedy_finish the subtree's loss
    uint32_t left;  // first child (the second is left + 1); 0 = leaf
    uint32_t nl;    // leaves of the subtree
    uint32_t off;   // offset of the subtree's first leaf in the lane's partition
    uint32_t pad_;
};

struct kp_g_item {
    uint32_t lane, node, chunk, big;
};

struct kp_g_args {
    kp_g_root root;
    const ulonglong2 *tab;  // [nslots][n] (M, U); slot nslots - 1 = all data
    uint64_t n;
    int32_t nslots;
    uint32_t chunk;
    const kp_greedy_lane *lanes;
    kp_g_node *nodes;  // [lanes][node_cap]
    uint32_t node_cap;
    uint32_t *cnt;  // [lanes] nodes in use
    unsigned long long *Hbig;  // [big_cap][KP_G_HSIZE]
    uint2 *bigmeta_cur, *bigmeta_next;  // (lane, node) of a multi-chunk node's histogram slot
    kp_g_item *next;
    uint32_t item_cap, big_cap;
    // [0] items of the next depth, [1] its histogram slots, [2] error word; [4..5] one 64-bit
    // count: k-mers of every node put on a frontier (the histogram kernel's reads, for stats)
    uint32_t *counters;
};

#ifdef __HIPCC__

// Decide one node from its histogram (in LDS): all 64 lanes of the wave call this.
__device__ inline void kp_g_decide_wave(const kp_g_args &A, uint32_t L, uint32_t ndi, const uint64_t *H, int ln) {
    const kp_greedy_lane P = A.lanes[L];
    kp_g_node *nodes = A.nodes + (uint64_t)L * A.node_cap;
    const uint64_t pat = nodes[ndi].pat;
    const double own = nodes[ndi].value;
    const int k = A.root.k;
    double bs = __builtin_inf();
    int bc = 0x7fffffff;
    for (int r = 0; r < 2; ++r) {
        const int code = ln + 64 * r;
        const double s = kp_g_cand_loss(H, pat, k, code, P.alpha, P.beta, P.penalty);
        if (kp_g_better(s, code, bs, bc)) {
            bs = s;
            bc = code;
        }
    }
    for (int off = 32; off; off >>= 1) {
        const double os = __shfl_xor(bs, off, 64);
        const int oc = __shfl_xor(bc, off, 64);
        if (kp_g_better(os, oc, bs, bc)) {
            bs = os;
            bc = oc;
        }
    }
    if (!(bs < own)) return;  // a leaf (:195-196)
    uint32_t idx = 0;
    if (ln == 0) idx = atomicAdd(&A.cnt[L], 2u);
    idx = __shfl(idx, 0, 64);
    if ((uint64_t)idx + 2 > A.node_cap) {
        if (ln == 0) atomicOr(&A.counters[2], 1u);
        return;
    }
    if (ln == 0) nodes[ndi].left = idx;
    if (ln < 2) {
        int pos;
        uint32_t a, b;
        kp_g_cand(pat, k, bc, &pos, &a, &b);
        const uint32_t m = ln ? b : a;
        kp_g_node c;
        c.pat = (pat & ~(15ull << (4 * pos))) | ((uint64_t)m << (4 * pos));
        kp_g_sum(H, pos, m, c.c);
        c.value = kp_g_train_loss(c.c[0], c.c[1], P.alpha, P.beta, P.penalty);
        c.left = 0;
        c.nl = 1;
        c.off = 0;
        c.pad_ = 0;
        nodes[idx + ln] = c;
        const uint64_t gen = kp_g_generality(c.pat, k);
        if (gen >= 2) {
            atomicAdd(reinterpret_cast<unsigned long long *>(A.counters + 4), (unsigned long long)gen);
            const uint32_t nch = (uint32_t)((gen + A.chunk - 1) / A.chunk);
            const uint32_t base = atomicAdd(&A.counters[0], nch);
            uint32_t big = 0;
            bool ok = (uint64_t)base + nch <= A.item_cap;
            if (nch > 1) {
                big = atomicAdd(&A.counters[1], 1u);
                ok = ok && big < A.big_cap;
                if (ok) A.bigmeta_next[big] = make_uint2(L, idx + ln);
            }
            if (!ok) {
                atomicOr(&A.counters[2], 2u);
            } else {
                for (uint32_t q = 0; q < nch; ++q) {
                    kp_g_item it;
                    it.lane = L;
                    it.node = idx + ln;
                    it.chunk = q;
                    it.big = big;
                    A.next[base + q] = it;
                }
            }
        }
    }
}

__global__ void __launch_bounds__(256) kp_greedy_tab(const uint64_t *__restrict__ M, const uint64_t *__restrict__ U,
                                                     uint64_t n, int nfc, int nslots, ulonglong2 *__restrict__ tab) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        unsigned long long sm = 0, su = 0;
        for (int f = 0; f < nfc; ++f) {
            const unsigned long long m = M[i * nfc + f], u = U[i * nfc + f];
            sm += m;
            su += u;
            if (f < nslots - 1) tab[(uint64_t)f * n + i] = make_ulonglong2(m, u);
        }
        tab[(uint64_t)(nslots - 1) * n + i] = make_ulonglong2(sm, su);
    }
}

__global__ void __launch_bounds__(64 * KP_G_WAVES) kp_greedy_hist(kp_g_args A, const kp_g_item *__restrict__ items,
                                                                  uint32_t n_items) {
    __shared__ unsigned long long sH[KP_G_WAVES][KP_G_HSIZE];
    __shared__ uint32_t sDec[KP_G_WAVES][KP_G_MAXK * 4];
    const int w = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const uint32_t it = blockIdx.x * KP_G_WAVES + w;
    const bool act = it < n_items;
    kp_g_item I = {0, 0, 0, 0};
    if (act) I = items[it];
    const int k = A.root.k;
    const uint64_t pat = act ? A.nodes[(uint64_t)I.lane * A.node_cap + I.node].pat : 0;
    for (int e = ln; e < KP_G_HSIZE; e += 64) sH[w][e] = 0;
    {  // digit d of position i -> (row offset, nucleotide)
        const int i = ln >> 2, d = ln & 3;
        uint32_t v = 0;
        if (i < k) {
            const uint32_t m = (uint32_t)(pat >> (4 * i)) & 15u;
            if (d < __builtin_popcount(m)) {
                const int nuc = kp_g_nth_nuc(m, d);
                v = (uint32_t)A.root.dig[i][nuc] * A.root.cg[i] | (uint32_t)nuc << 30;
            }
        }
        sDec[w][ln] = v;
    }
    __syncthreads();
    uint64_t gen = 0;
    if (act) {
        gen = kp_g_generality(pat, k);
        const int fold = A.lanes[I.lane].fold;
        const ulonglong2 *all = A.tab + (uint64_t)(A.nslots - 1) * A.n;
        const ulonglong2 *ft = fold >= 0 ? A.tab + (uint64_t)fold * A.n : nullptr;
        const uint64_t j0 = (uint64_t)I.chunk * A.chunk;
        const uint64_t j1 = j0 + A.chunk < gen ? j0 + A.chunk : gen;
        for (uint64_t j = j0 + ln; j < j1; j += 64) {
            uint32_t t = (uint32_t)j, row = 0, nucs = 0;
            for (int i = 0; i < k; ++i) {
                const uint32_t r = __builtin_popcount((uint32_t)(pat >> (4 * i)) & 15u);
                uint32_t d = 0;
                switch (r) {
                case 2: d = t & 1u; t >>= 1; break;
                case 3: d = t % 3u; t /= 3u; break;
                case 4: d = t & 3u; t >>= 2; break;
                default: break;
                }
                const uint32_t e = sDec[w][i * 4 + d];
                row += e & KP_G_ROWMASK;
                nucs |= (e >> 30) << (2 * i);
            }
            ulonglong2 tr = all[row];
            ulonglong2 te = make_ulonglong2(0, 0);
            if (ft) {
                te = ft[row];
                tr.x -= te.x;
                tr.y -= te.y;
            }
            for (int i = 0; i < k; ++i) {
                if (__builtin_popcount((uint32_t)(pat >> (4 * i)) & 15u) < 2) continue;  // no split there
                unsigned long long *h = &sH[w][(i * 4 + ((nucs >> (2 * i)) & 3u)) * 4];
                if (tr.x) atomicAdd(h + 0, tr.x);
                if (tr.y) atomicAdd(h + 1, tr.y);
                if (ft) {
                    if (te.x) atomicAdd(h + 2, te.x);
                    if (te.y) atomicAdd(h + 3, te.y);
                }
            }
        }
    }
    __syncthreads();
    if (!act) return;
    if (gen <= A.chunk) {
        kp_g_decide_wave(A, I.lane, I.node, (const uint64_t *)sH[w], ln);
    } else if (I.big < A.big_cap) {
        unsigned long long *g = A.Hbig + (uint64_t)I.big * KP_G_HSIZE;
        for (int e = ln; e < k * 16; e += 64) {
            const unsigned long long v = sH[w][e];
            if (v) atomicAdd(g + e, v);
        }
    }
}

__global__ void __launch_bounds__(64 * KP_G_WAVES) kp_greedy_decide_big(kp_g_args A, uint32_t n_big) {
    __shared__ unsigned long long sH[KP_G_WAVES][KP_G_HSIZE];
    const int w = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const uint32_t slot = blockIdx.x * KP_G_WAVES + w;
    const bool act = slot < n_big;
    if (act) {
        unsigned long long *g = A.Hbig + (uint64_t)slot * KP_G_HSIZE;
        for (int e = ln; e < KP_G_HSIZE; e += 64) {
            sH[w][e] = g[e];
            g[e] = 0;  // the slot is clean for the next depth
        }
    }
    __syncthreads();
    if (!act) return;
    const uint2 m = A.bigmeta_cur[slot];
    kp_g_decide_wave(A, m.x, m.y, (const uint64_t *)sH[w], ln);
}

// dend[d * n_lanes + L] = nodes of lane L after depth d (level d = [dend[d - 1], dend[d]))
__global__ void __launch_bounds__(1024) kp_greedy_finish(kp_g_args A, const uint32_t *__restrict__ dend, int depths,
                                                         uint32_t n_lanes, uint64_t *__restrict__ leaf_pat,
                                                         double *__restrict__ leaf_term, double *__restrict__ loss,
                                                         uint64_t *__restrict__ n_leaves) {
    const uint32_t L = blockIdx.x;
    kp_g_node *nodes = A.nodes + (uint64_t)L * A.node_cap;
    const kp_greedy_lane P = A.lanes[L];
    for (int d = depths - 1; d >= 0; --d) {
        const uint32_t s = d ? dend[(uint64_t)(d - 1) * n_lanes + L] : 0, e = dend[(uint64_t)d * n_lanes + L];
        for (uint32_t i = s + threadIdx.x; i < e; i += blockDim.x) {
            const uint32_t l = nodes[i].left;
            if (l) {
                nodes[i].value = nodes[l].value + nodes[l + 1].value;  // s1 + s2 (:194)
                nodes[i].nl = nodes[l].nl + nodes[l + 1].nl;
            }
        }
        __syncthreads();
    }
    for (int d = 0; d < depths; ++d) {
        const uint32_t s = d ? dend[(uint64_t)(d - 1) * n_lanes + L] : 0, e = dend[(uint64_t)d * n_lanes + L];
        for (uint32_t i = s + threadIdx.x; i < e; i += blockDim.x) {
            const kp_g_node nd = nodes[i];
            if (nd.left) {
                nodes[nd.left].off = nd.off;  // papa1 + papa2: the left subtree's leaves first
                nodes[nd.left + 1].off = nd.off + nodes[nd.left].nl;
            } else {
                leaf_pat[(uint64_t)L * A.n + nd.off] = nd.pat;
                leaf_term[(uint64_t)L * A.n + nd.off] =
                    P.fold >= 0 ? kp_g_test_ll(nd.c[0], nd.c[1], nd.c[2], nd.c[3], P.alpha, P.beta) : 0.0;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[L] = nodes[0].value;
        n_leaves[L] = nodes[0].nl;
    }
}

// acc[c] += the test terms of the batch's lanes of chain c, lane by lane, leaf by leaf
__global__ void __launch_bounds__(64) kp_greedy_chain(const kp_greedy_lane *__restrict__ lanes, uint32_t n_lanes,
                                                      uint64_t n, const double *__restrict__ leaf_term,
                                                      const uint64_t *__restrict__ n_leaves, int n_chains,
                                                      double *__restrict__ acc) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= n_chains) return;
    double s = acc[c];
    for (uint32_t L = 0; L < n_lanes; ++L) {
        if (lanes[L].chain != c) continue;
        const double *t = leaf_term + (uint64_t)L * n;
        const uint64_t m = n_leaves[L];
        uint64_t i = 0;
        for (; i + 8 <= m; i += 8) {
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = t[i + q];
#pragma unroll
            for (int q = 0; q < 8; ++q) s += v[q];
        }
        for (; i < m; ++i) s += t[i];
    }
    acc[c] = s;
}

#endif  // __HIPCC__

// ---------------------------------------------------------------------------
// the same algorithm serially on the host (kp_greedy_host: parity and CPU tests)
// ---------------------------------------------------------------------------

struct kp_g_host_job {
    kp_g_root root;
    const uint64_t *M, *U;
    uint64_t n;
    int nfc;
    kp_greedy_lane P;
    std::vector<uint64_t> *leaves;
    double *chain;  // the lane's chain accumulator or nullptr
};

// counts of one k-mer row for the lane: (trM, trU, teM, teU)
static inline void kp_g_host_row(const kp_g_host_job &J, uint64_t row, uint64_t c[4]) {
    uint64_t sm = 0, su = 0;
    for (int f = 0; f < J.nfc; ++f) {
        sm += J.M[row * J.nfc + f];
        su += J.U[row * J.nfc + f];
    }
    c[2] = c[3] = 0;
    if (J.P.fold >= 0) {
        c[2] = J.M[row * J.nfc + J.P.fold];
        c[3] = J.U[row * J.nfc + J.P.fold];
    }
    c[0] = sm - c[2];
    c[1] = su - c[3];
}

static void kp_g_host_hist(const kp_g_host_job &J, uint64_t pat, uint64_t *H) {
    const int k = J.root.k;
    for (int e = 0; e < KP_G_HSIZE; ++e) H[e] = 0;
    const uint64_t gen = kp_g_generality(pat, k);
    for (uint64_t j = 0; j < gen; ++j) {
        uint64_t t = j, row = 0;
        int nucs[KP_G_MAXK];
        for (int i = 0; i < k; ++i) {
            const uint32_t m = (uint32_t)(pat >> (4 * i)) & 15u;
            const uint32_t r = __builtin_popcount(m);
            const int nuc = kp_g_nth_nuc(m, (int)(t % r));
            t /= r;
            nucs[i] = nuc;
            row += (uint64_t)J.root.dig[i][nuc] * J.root.cg[i];
        }
        uint64_t c[4];
        kp_g_host_row(J, row, c);
        for (int i = 0; i < k; ++i)
            for (int q = 0; q < 4; ++q) H[(i * 4 + nucs[i]) * 4 + q] += c[q];
    }
}

// greedy_res_kmer_table_ord :159-196 for one node with counts c; returns the subtree's loss
static double kp_g_host_node(const kp_g_host_job &J, uint64_t pat, const uint64_t c[4]) {
    const int k = J.root.k;
    const double own = kp_g_train_loss(c[0], c[1], J.P.alpha, J.P.beta, J.P.penalty);
    double bs = __builtin_inf();
    int bc = 0x7fffffff;
    std::vector<uint64_t> H;
    if (kp_g_generality(pat, k) >= 2) {
        H.resize(KP_G_HSIZE);
        kp_g_host_hist(J, pat, H.data());
        for (int code = 0; code < 8 * k; ++code) {
            const double s = kp_g_cand_loss(H.data(), pat, k, code, J.P.alpha, J.P.beta, J.P.penalty);
            if (kp_g_better(s, code, bs, bc)) {
                bs = s;
                bc = code;
            }
        }
    }
    if (!(bs < own)) {
        J.leaves->push_back(pat);
        if (J.chain && J.P.fold >= 0) *J.chain += kp_g_test_ll(c[0], c[1], c[2], c[3], J.P.alpha, J.P.beta);
        return own;
    }
    int pos;
    uint32_t a, b;
    kp_g_cand(pat, k, bc, &pos, &a, &b);
    uint64_t c1[4], c2[4];
    kp_g_sum(H.data(), pos, a, c1);
    kp_g_sum(H.data(), pos, b, c2);
    std::vector<uint64_t>().swap(H);
    const uint64_t keep = pat & ~(15ull << (4 * pos));
    const double s1 = kp_g_host_node(J, keep | ((uint64_t)a << (4 * pos)), c1);
    const double s2 = kp_g_host_node(J, keep | ((uint64_t)b << (4 * pos)), c2);
    return s1 + s2;
}
