// kp_bt.h -- the breadth-first backtrack of every lane at once (kp_bt_* kernels; see
// kp_hip.hip's header).  Launched by run_pass (kp_pass.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp_core.h"
#include "kp_dp_kernel.h"

// ---------------------------------------------------------------------------
// breadth-first backtrack
// ---------------------------------------------------------------------------

struct kp_node {
    uint64_t x;      // cell
    uint64_t dig;    // its packed digits
    uint32_t child;  // first child (the second is child + 1); 0 = leaf
    uint32_t nleaf;  // leaves of the subtree
    uint32_t off;    // position of the subtree's first leaf in backtrack order
    float test;      // test -2LL of the subtree, float32 sums along the tree
};

struct kp_bt_params {
    kp_geom g;
    kp_dev_tables T;
    const void *K;
    const float *S;
    const kp_group_dev *groups;
    const uint32_t *lanegrp;
    kp_node *nodes;    // [Ltot][cap]
    uint32_t cap;
    uint32_t *cnt;     // [Ltot] nodes allocated
    uint32_t *dend;    // [Ltot][KP_MAXDEPTH + 1] end of each depth's node range
    uint32_t *bad;     // [Ltot] 1 = no candidate, 2 = node pool full, 4 = score not reproduced
    float *root_train, *root_test;
    uint64_t *nleaves;
    uint64_t *leaves;  // [Ltot][leafcap]
    uint64_t leafcap;
    int depth;
    int maxdepth;
};

__device__ inline uint64_t kp_wave_sum(uint64_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__host__ __device__ inline uint64_t kp_s_off(const kp_geom &g, uint64_t h, uint32_t lane, uint32_t l) {
    return (h * g.Ltot + lane) * (uint64_t)g.Bpad + l;
}

__global__ void kp_bt_init(kp_bt_params P, uint64_t root_x, uint64_t root_dig) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= P.g.Ltot) return;
    kp_node *N = P.nodes + (uint64_t)lane * P.cap;
    N[0].x = root_x;
    N[0].dig = root_dig;
    N[0].child = 0;
    N[0].nleaf = 0;
    N[0].off = 0;
    N[0].test = 0.0f;
    P.cnt[lane] = 1;
    P.dend[(uint64_t)lane * (KP_MAXDEPTH + 1)] = 1;
    P.bad[lane] = 0;
}

__global__ void kp_bt_advance(kp_bt_params P) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= P.g.Ltot) return;
    P.dend[(uint64_t)lane * (KP_MAXDEPTH + 1) + P.depth + 1] = P.cnt[lane];
}

// one wave per node of depth P.depth; grid (waves, lanes)
template <typename CT>
__global__ void __launch_bounds__(256) kp_bt_level(kp_bt_params P) {
    const kp_geom &g = P.g;
    const uint32_t lane = blockIdx.y;
    const uint32_t lid = threadIdx.x & 63u;
    const uint32_t *de = P.dend + (uint64_t)lane * (KP_MAXDEPTH + 1);
    const uint32_t lo = P.depth ? de[P.depth - 1] : 0u, hi = de[P.depth];
    const kp_group_dev *G = P.groups + P.lanegrp[lane];
    const int fold = G->fold;
    const int jl = (int)(lane - (uint32_t)G->lane0);
    const double alpha = kp_lane_alpha(*G, jl), beta = kp_lane_beta(*G, jl);
    const double pen = G->pen[jl];
    const CT *K = reinterpret_cast<const CT *>(P.K);
    kp_node *N = P.nodes + (uint64_t)lane * P.cap;
    const uint32_t nw = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t n = lo + ((blockIdx.x * blockDim.x + threadIdx.x) >> 6); n < hi; n += nw) {
        const uint64_t x = N[n].x, dig = N[n].dig;
        const uint64_t h = x / g.B;
        const uint32_t l = (uint32_t)(x % g.B);
        const bool kmer = kp_dig_is_kmer(g, dig);
        // counts: the wave splits the k-mer-low rows of the cell, then reduces
        uint64_t mtr = 0, utr = 0, mte = 0, ute = 0;
        const uint32_t q0 = P.T.klofs[l], q1 = P.T.klofs[l + 1];
        for (uint32_t q = q0 + lid; q < q1; q += 64) {
            const kp_cnt c = kp_kl_counts<CT>(g, K, P.T.kpos[h], P.T.kllist[q], fold);
            mtr += c.mtr; utr += c.utr; mte += c.mte; ute += c.ute;
        }
        kp_cnt c;
        c.mtr = kp_wave_sum(mtr);
        c.utr = kp_wave_sum(utr);
        c.mte = kp_wave_sum(mte);
        c.ute = kp_wave_sum(ute);
        // split candidates: one (position, pair) per lane, scan order = code order
        float best = __builtin_huge_valf();
        uint32_t code = KP_NONE;
        if (!kmer) {
            uint32_t npt = 0;
            for (int i = 0; i < g.k; ++i) npt += P.T.tabs[i].np[kp_dig(dig, i)];
            for (uint32_t p = lid; p < npt; p += 64) {
                uint32_t rem = p, d = 0;
                int i = 0;
                for (; i < g.k; ++i) {
                    d = kp_dig(dig, i);
                    const uint32_t npi = P.T.tabs[i].np[d];
                    if (rem < npi) break;
                    rem -= npi;
                }
                const kp_postab &T = P.T.tabs[i];
                const uint32_t da = d - T.pa[d][rem], db = d - T.pb[d][rem];
                uint64_t o1, o2;
                if (i < g.t) {
                    const uint32_t cg = (uint32_t)g.cgl[i];
                    o1 = kp_s_off(g, h, lane, l - da * cg);
                    o2 = kp_s_off(g, h, lane, l - db * cg);
                } else {
                    o1 = kp_s_off(g, h - (uint64_t)da * g.hcg[i - g.t], lane, l);
                    o2 = kp_s_off(g, h - (uint64_t)db * g.hcg[i - g.t], lane, l);
                }
                const float v = P.S[o1] + P.S[o2];
                if (v < best) {  // a lane sees its pairs in increasing code order
                    best = v;
                    code = (uint32_t)((i << 3) | rem);
                }
            }
            // first minimum over the wave: smaller value, then smaller code (= earlier in scan)
            for (int off = 32; off > 0; off >>= 1) {
                const float ob = __shfl_xor(best, off, 64);
                const uint32_t oc = __shfl_xor(code, off, 64);
                if (ob < best || (ob == best && oc < code)) {
                    best = ob;
                    code = oc;
                }
            }
        }
        // single pattern term; the stored score must be reproduced exactly
        float value;
        float test = 0.0f;
        if (kmer) {
            value = kp_kmer_train(c, alpha, beta, pen);
            code = KP_SINGLE;
            if (fold >= 0) test = kp_kmer_test(c, alpha, beta);
        } else {
            const double pr = kp_rate(c, alpha, beta);
            const double lp = kp_libm_log(pr), l1p = kp_libm_log(1.0 - pr);  // the C library's (kp_libm.h)
            const double s = kp_single_train(c, lp, l1p, pen);
            value = best;
            if (s < (double)best) {
                value = (float)s;
                code = KP_SINGLE;
            }
            if (code == KP_SINGLE && fold >= 0) test = kp_single_test(c, lp, l1p);
        }
        if (lid == 0) {
            const float stored = P.S[kp_s_off(g, h, lane, l)];
            const bool same = (__float_as_uint(stored) == __float_as_uint(value)) || (stored != stored && value != value);
            uint32_t err = same ? 0u : 4u;
            if (code == KP_SINGLE) {
                N[n].child = 0;
                N[n].test = test;
            } else if (code == KP_NONE) {
                err |= 1u;
                N[n].child = 0;
                N[n].test = 0.0f;
            } else {
                const uint32_t base = atomicAdd(P.cnt + lane, 2u);
                if (base + 2 > P.cap) {
                    err |= 2u;
                    N[n].child = 0;
                } else {
                    const int i = (int)(code >> 3), j = (int)(code & 7u);
                    const uint32_t d = kp_dig(dig, i);
                    const kp_postab &T = P.T.tabs[i];
                    const uint64_t clear = ~(15ull << (4 * i));
                    kp_node a, b;
                    a.x = x - (uint64_t)(d - T.pa[d][j]) * g.cgl[i];
                    a.dig = (dig & clear) | ((uint64_t)T.pa[d][j] << (4 * i));
                    b.x = x - (uint64_t)(d - T.pb[d][j]) * g.cgl[i];
                    b.dig = (dig & clear) | ((uint64_t)T.pb[d][j] << (4 * i));
                    a.child = b.child = 0;
                    a.nleaf = b.nleaf = 0;
                    a.off = b.off = 0;
                    a.test = b.test = 0.0f;
                    N[base] = a;
                    N[base + 1] = b;
                    N[n].child = base;
                }
            }
            if (err) atomicOr(P.bad + lane, err);
        }
    }
}

// one workgroup per lane: float32 test sums bottom-up, then leaf order top-down
__global__ void __launch_bounds__(256) kp_bt_finish(kp_bt_params P) {
    const kp_geom &g = P.g;
    const uint32_t lane = blockIdx.x;
    const uint32_t *de = P.dend + (uint64_t)lane * (KP_MAXDEPTH + 1);
    kp_node *N = P.nodes + (uint64_t)lane * P.cap;
    for (int d = P.maxdepth; d >= 0; --d) {
        const uint32_t lo = d ? de[d - 1] : 0u, hi = de[d];
        for (uint32_t n = lo + threadIdx.x; n < hi; n += blockDim.x) {
            const uint32_t c = N[n].child;
            if (c) {
                N[n].test = N[c].test + N[c + 1].test;  // test[c1] + test[c2] (CV :47)
                N[n].nleaf = N[c].nleaf + N[c + 1].nleaf;
            } else {
                N[n].nleaf = 1;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) N[0].off = 0;
    __syncthreads();
    uint64_t *leaves = P.leaves + (uint64_t)lane * P.leafcap;
    for (int d = 0; d <= P.maxdepth; ++d) {
        const uint32_t lo = d ? de[d - 1] : 0u, hi = de[d];
        for (uint32_t n = lo + threadIdx.x; n < hi; n += blockDim.x) {
            const uint32_t c = N[n].child, off = N[n].off;
            if (c) {
                N[c].off = off;
                N[c + 1].off = off + N[c].nleaf;
            } else if (off < P.leafcap) {
                leaves[off] = N[n].x;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        P.root_train[lane] = P.S[kp_s_off(g, g.nblocks - 1, lane, g.B - 1)];
        P.root_test[lane] = N[0].test;
        P.nleaves[lane] = N[0].nleaf;
    }
}
