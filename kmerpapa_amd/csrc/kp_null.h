// kp_null.h -- per-region null tables: many replicates of kp_spec_simulate's draw, binned by
// region, in one pass (no reference counterpart).  Included by kp_hip.hip after kp_sim.h.
// Semantics: include/kmerpapa_hip.h.
//
// Column j of the table is what kp_spec_simulate draws with replicate = rep_first + j: the window,
// its validity, the table entry and kp_sm_cum are kp_sim.h's, and the uniform number is the same
// Philox4x32-10 output, computed in two parts and compared as an integer:
//   kp_nl_round1  the first round without the replicate (which only enters as an xor into x2), once
//                 per window
//   kp_nl_bits    the other nine rounds, written out, and the 53 bits m with u = m * 2^-53
//   kp_nl_thresh  T = ceil(c * 2^53): u < c exactly when m < T, for every 53-bit m and every double
//                 c in [0, 1] (c * 2^53 is exact, and an integer is below a real exactly when it is
//                 below its ceiling)
//   kp_nl_pick    kp_sm_pick on (m, T0, T1, T2)
// The host session runs the same four functions serially.
//
//   kp_null_kernel  kp_spec_scan_kernel's persistent grid over (item, replicate chunk) pairs, and
//                   per pair two phases per batch of KP_P_BATCH roll steps.  Roll: every thread rolls
//                   its run as kp_sim_roll does, gathers the batch's 16-byte entries and rates, and
//                   stages each window's thresholds, its centre in the run and its REF in LDS.  Draw:
//                   a wave takes every fourth staged window; the thresholds are wave-uniform, the
//                   lanes hold consecutive replicates of the chunk, and a window with T2 = 0 is
//                   skipped whole.  A hit adds 1 to the item's uint32 LDS counter [replicate][type],
//                   and after the item every non-zero counter goes to counts[region][replicate]
//                   with one global atomic (several items of a region share a row).  The type of a
//                   hit is 3 * REF + slot: kp_spec_begin admits a pattern only if its centre allows
//                   exactly the REF of its type, so this is ptype[pid].
//
// Every device loop has a bound the host computed; there are no waits between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <new>

#include "kp_pred.h"
#include "kp_rt.h"
#include "kp_seq.h"
#include "kp_sim.h"
#include "kp_spec.h"

#define KP_NL_WIN (KP_P_BATCH * KP_S_THREADS)  // windows staged per batch: 48 KB of thresholds, 2 KB of bytes
#define KP_NL_CNT 3072                         // uint32 counters of an item beside them: 62 KB in all

struct kp_nl_head {
    uint32_t a0, a1, a2, a3;  // the counter after round 1, but for x2 = a2 ^ replicate
};

__host__ __device__ inline kp_nl_head kp_nl_round1(uint64_t seed, uint32_t contig, uint64_t pos) {
    const uint64_t p0 = (uint64_t)KP_SM_M0 * (uint32_t)pos, p1 = (uint64_t)KP_SM_M1 * contig;
    return kp_nl_head{(uint32_t)(p1 >> 32) ^ (uint32_t)(pos >> 32) ^ (uint32_t)seed, (uint32_t)p1,
                      (uint32_t)(p0 >> 32) ^ (uint32_t)(seed >> 32), (uint32_t)p0};
}

// rounds 2..10 and the 53 bits of kp_sm_uniform before its scaling (the last round's p0 is dead code)
__host__ __device__ inline uint64_t kp_nl_bits(const kp_nl_head h, uint32_t replicate, uint64_t seed) {
    uint32_t x0 = h.a0, x1 = h.a1, x2 = h.a2 ^ replicate, x3 = h.a3;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 1; r < 10; ++r) {
        k0 += KP_SM_W0, k1 += KP_SM_W1;
        const uint64_t p0 = (uint64_t)KP_SM_M0 * x0, p1 = (uint64_t)KP_SM_M1 * x2;
        const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1;
        x0 = y0, x1 = (uint32_t)p1, x2 = y2, x3 = (uint32_t)p0;
    }
    return (((uint64_t)x1 << 32) | x0) >> 11;
}

// c in [0, 1]: the product is exact and at most 2^53
__host__ __device__ inline uint64_t kp_nl_thresh(double c) { return (uint64_t)ceil(c * 0x1p53); }

__host__ __device__ inline uint32_t kp_nl_pick(uint64_t m, uint64_t t0, uint64_t t1, uint64_t t2) {
    return m < t0 ? 0u : (m < t1 ? 1u : (m < t2 ? 2u : 3u));
}

struct kp_nl_args {
    const uint8_t *seq;      // the contig, KP_S_PAD readable bytes past its end
    const kp_p_item *items;  // [n_items]
    uint64_t n_units, steps; // units = (item, pass) pairs, item-major
    int32_t k, fold;
    uint32_t mask;  // 4^k - 1
    const int4 *lut;      // [4^k]
    const double *rates;  // [P]
    double scale;
    uint64_t seed;
    uint32_t contig, rep_first, n_reps;
    uint32_t rc, passes;         // replicates per pass (rc * types <= KP_NL_CNT), passes = ceil(n_reps / rc)
    uint32_t *counts;            // [n_regions][n_reps][1 or 12]
    unsigned long long *stat;    // [2] += valid windows, windows with c2 > 0 (pass 0 only)
};

#ifdef __HIPCC__

__device__ inline uint64_t kp_nl_uniform64(uint64_t v) {  // a value every lane holds, moved to scalar registers
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

template <bool TYPED>
__global__ void __launch_bounds__(KP_S_THREADS) kp_null_kernel(kp_nl_args A) {
    __shared__ unsigned long long s_thr[3][KP_NL_WIN];  // [slot][step of the batch][thread]
    __shared__ uint8_t s_meta[KP_NL_WIN];               // the centre's index in the thread's run, REF above it
    __shared__ uint32_t s_cnt[KP_NL_CNT];               // [replicate of the chunk][type]
    constexpr uint32_t NT = TYPED ? KP_SP_TYPES : 1;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint32_t e = tid; e < KP_NL_CNT; e += KP_S_THREADS) s_cnt[e] = 0;
    __syncthreads();
    const int k = A.k, top = 2 * (A.k - 1), h = A.k / 2, cshift = 2 * (A.k - 1 - A.k / 2);
    for (uint64_t s = 0; s < A.steps; ++s) {
        const uint64_t unit = s * gridDim.x + blockIdx.x;
        if (unit >= A.n_units) break;  // (the same for the whole workgroup)
        const uint32_t pass = (uint32_t)(unit % A.passes);
        const kp_p_item it = A.items[unit / A.passes];
        const uint32_t j0 = pass * A.rc;                   // the chunk's first column (< n_reps)
        const uint32_t rc = min(A.rc, A.n_reps - j0);      // and its columns
        const uint32_t rep0 = A.rep_first + j0;            // (rep_first + n_reps <= 2^32)
        const uint32_t r0 = tid * KP_S_RUN;
        const uint32_t cnt = r0 < it.count ? min((uint32_t)KP_S_RUN, it.count - r0) : 0u;
        uint32_t d[16], off, end;
        kp_p_load(A.seq, (uint64_t)it.first + r0 - (uint32_t)h, cnt ? cnt + (uint32_t)k - 1u : 0u, d, &off, &end);
        const uint32_t full0 = off + (uint32_t)k - 1u;  // the byte that completes the first window
        uint32_t nv = 0, nd = 0;
        kp_s_win w{0u, 0u, 0u};
#pragma unroll 1
        for (uint32_t b = 0; b < 64 / KP_P_BATCH; ++b) {  // (rolled: the draw phase stands once in the code)
            uint32_t lo = 0, hi = 0;  // the batch's eight bytes
#pragma unroll
            for (uint32_t i = 0; i < 64 / KP_P_BATCH; ++i) {
                lo = b == i ? d[2 * i] : lo;
                hi = b == i ? d[2 * i + 1] : hi;
            }
            const uint32_t jb = b * KP_P_BATCH;
            uint32_t code[KP_P_BATCH];
            bool has[KP_P_BATCH];
            int4 p[KP_P_BATCH];
            double c[KP_P_BATCH][3];
#pragma unroll
            for (uint32_t q = 0; q < KP_P_BATCH; ++q) {
                const uint32_t j = jb + q;
                const uint32_t byte = ((q < 4 ? lo : hi) >> (8u * (q & 3u))) & 0xffu;
                if (j >= off && j < end) kp_s_step(w, kp_s_class(byte), A.mask, top);
                has[q] = j >= full0 && j < end && w.valid >= (uint32_t)k;
                nv += has[q];
                code[q] = kp_s_code(w, k, A.fold);
            }
#pragma unroll
            for (uint32_t q = 0; q < KP_P_BATCH; ++q)  // (code <= mask: the entry lies inside the table)
                p[q] = has[q] ? A.lut[code[q]] : make_int4(KP_P_NONE, KP_P_NONE, KP_P_NONE, KP_P_NONE);
#pragma unroll
            for (uint32_t q = 0; q < KP_P_BATCH; ++q)  // (ids < P: the table holds indices of the pattern list only)
                kp_sm_cum(p[q].x, p[q].y, p[q].z, A.rates, A.scale, c[q]);
#pragma unroll
            for (uint32_t q = 0; q < KP_P_BATCH; ++q) {
                const uint32_t e = q * KP_S_THREADS + tid;  // < KP_NL_WIN
                const bool draws = c[q][2] > 0.0;           // (a window without has[q] has no id, so its c2 is 0.0)
                s_thr[2][e] = draws ? kp_nl_thresh(c[q][2]) : 0ull;
                if (draws) {
                    s_thr[0][e] = kp_nl_thresh(c[q][0]);
                    s_thr[1][e] = kp_nl_thresh(c[q][1]);
                    // jb + q - full0 < cnt <= KP_S_RUN = 32; the centre of the counted code is 0..3
                    s_meta[e] = (uint8_t)((jb + q - full0) | (((code[q] >> cshift) & 3u) << 5));
                    ++nd;
                }
            }
            __syncthreads();  // the batch is staged
            for (uint32_t e = wv; e < KP_NL_WIN; e += KP_S_THREADS / 64) {  // (e is the same for the whole wave)
                const uint64_t t2 = kp_nl_uniform64(s_thr[2][e]);
                if (t2 == 0) continue;
                const uint64_t t0 = kp_nl_uniform64(s_thr[0][e]), t1 = kp_nl_uniform64(s_thr[1][e]);
                const uint32_t m8 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_meta[e]);
                const uint64_t pos = (uint64_t)it.first + (e % KP_S_THREADS) * KP_S_RUN + (m8 & 31u);
                const kp_nl_head hd = kp_nl_round1(A.seed, A.contig, pos);
                const uint32_t tbase = TYPED ? 3u * (m8 >> 5) : 0u;
                for (uint32_t rb = 0; rb < rc; rb += 64) {
                    const uint32_t j = rb + lane;
                    if (j < rc) {  // (the last lanes of the chunk's last 64 replicates sit out)
                        const uint32_t slot = kp_nl_pick(kp_nl_bits(hd, rep0 + j, A.seed), t0, t1, t2);
                        // j < rc <= A.rc and type < NT: the counter lies below A.rc * NT <= KP_NL_CNT
                        if (slot < 3u) atomicAdd(&s_cnt[j * NT + (TYPED ? tbase + slot : 0u)], 1u);
                    }
                }
            }
            __syncthreads();  // read before the next batch is staged; every add of the batch is in
        }
        if (pass == 0) {
            for (int o = 32; o; o >>= 1) {
                nv += __shfl_xor(nv, o, 64);
                nd += __shfl_xor(nd, o, 64);
            }
            if (lane == 0) {
                if (nv) atomicAdd(&A.stat[0], (unsigned long long)nv);
                if (nd) atomicAdd(&A.stat[1], (unsigned long long)nd);
            }
        }
        uint32_t *row = A.counts + ((uint64_t)it.region * A.n_reps + j0) * NT;  // the chunk's rc * NT counters are contiguous
        for (uint32_t e = tid; e < rc * NT; e += KP_S_THREADS) {
            const uint32_t v = s_cnt[e];
            if (v) {
                atomicAdd(&row[e], v);
                s_cnt[e] = 0;
            }
        }
        __syncthreads();  // zero again before the next unit adds
    }
}

#endif  // __HIPCC__

// ---------------------------------------------------------------------------
// the call, in a kp_spec session
// ---------------------------------------------------------------------------

extern "C" {

int kp_spec_null(kp_ctx *c, const uint8_t *seq, uint64_t n, uint32_t contig_id, const uint64_t *reg_begin,
                 const uint64_t *reg_end, uint64_t n_regions, const double *rates, double scale, uint64_t seed,
                 uint32_t rep_first, uint32_t n_reps, int by_type, uint32_t *counts) {
    kp_spec_sess *s = spec_sess(c);
    int rc = scan_check_contig("kp_spec_null", s->active, seq, n, "kp_spec_begin");
    if (rc) return rc;
    if (!counts) return fail(KP_E_ARG, "kp_spec_null: null counts");
    if (!rates) return fail(KP_E_ARG, "kp_spec_null: null rates");
    if (n_regions >= (1ull << 32)) return fail(KP_E_ARG, "kp_spec_null: 2^32 regions or more in one call");
    if (n_regions && (!reg_begin || !reg_end)) return fail(KP_E_ARG, "kp_spec_null: null regions");
    if (n_reps == 0) return fail(KP_E_ARG, "kp_spec_null: no replicates");
    if ((uint64_t)rep_first + n_reps > (1ull << 32))
        return fail(KP_E_ARG, "kp_spec_null: replicates " + std::to_string(rep_first) + " .. " +
                                  std::to_string((uint64_t)rep_first + n_reps - 1) + " go past 2^32 - 1");
    if ((rc = sim_check_rates(s, rates, scale))) return rc;
    if ((rc = scan_check_regions("kp_spec_null", n, reg_begin, reg_end, n_regions, false))) return rc;
    s->null = kp_spec_null_stats{};
    if (!n_regions) return KP_OK;
    const int k = s->k;
    const uint32_t P = (uint32_t)s->pats.size();
    const uint32_t mask = (uint32_t)(s->cells - 1);
    const uint32_t NT = by_type ? (uint32_t)KP_SP_TYPES : 1u;
    const size_t n_cnt = (size_t)n_regions * n_reps * NT;
    uint64_t lo = 0, hi = 0;
    scan_centres(n, k, &lo, &hi);
    if (!c) {
        memset(counts, 0, n_cnt * 4);
        uint64_t windows = 0, drawing = 0, hits = 0, n_items = 0;
        for (uint64_t r = 0; r < n_regions; ++r) {
            const uint64_t b = std::max(reg_begin[r], lo), e = std::min(reg_end[r], hi);
            n_items += scan_pieces(reg_begin[r], reg_end[r], lo, hi);
            uint32_t *row = counts + r * n_reps * NT;
            for (uint64_t p = b; p < e; ++p) {
                uint32_t code = 0;
                if (!kp_p_window(seq, n, p, k, s->fold, mask, &code)) continue;
                ++windows;
                const int32_t *id = &s->h_lut[4ull * code];
                double cum[3];
                kp_sm_cum(id[0], id[1], id[2], rates, scale, cum);
                if (!(cum[2] > 0.0)) continue;
                ++drawing;
                const uint64_t t0 = kp_nl_thresh(cum[0]), t1 = kp_nl_thresh(cum[1]), t2 = kp_nl_thresh(cum[2]);
                const kp_nl_head hd = kp_nl_round1(seed, contig_id, p);
                for (uint32_t j = 0; j < n_reps; ++j) {
                    const uint32_t slot = kp_nl_pick(kp_nl_bits(hd, rep_first + j, seed), t0, t1, t2);
                    if (slot >= 3u) continue;
                    ++row[(size_t)j * NT + (by_type ? s->ptype[id[slot]] : 0u)];
                    ++hits;
                }
            }
        }
        s->null.windows = windows;
        s->null.draws = drawing * n_reps;
        s->null.hits = hits;
        s->null.items = n_items;
        s->null.passes = 1;
        s->null.reps_per_pass = n_reps;
        return KP_OK;
    }

    KP_HIP(hipSetDevice(c->device));
    const long reps_env = env_int("KP_NULL_REPS", 0);
    uint32_t chunk = std::min<uint32_t>(n_reps, (uint32_t)KP_NL_CNT / NT);
    if (reps_env > 0) chunk = (uint32_t)std::min<long>(chunk, reps_env);
    const uint32_t passes = (n_reps + chunk - 1) / chunk;
    s->null.passes = passes;
    s->null.reps_per_pass = chunk;
    std::vector<kp_p_item> items;
    try {
        for (uint64_t r = 0; r < n_regions; ++r) scan_cut(items, reg_begin[r], reg_end[r], lo, hi, (uint32_t)r);
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_spec_null: the work items do not fit host memory");
    }
    if (items.size() >= (1ull << 32)) return fail(KP_E_ARG, "kp_spec_null: 2^32 work items or more in one call");
    const size_t n_items = items.size();
    s->null.items = n_items;
    if ((rc = spec_arena(c, "kp_spec_null", g_up(n_cnt * 4) + g_up((size_t)P * 8) + g_up(16)))) return rc;
    uint32_t *d_counts = (uint32_t *)c->arena.take(n_cnt * 4);
    double *d_rates = (double *)c->arena.take((size_t)P * 8);
    unsigned long long *d_stat = (unsigned long long *)c->arena.take(16);
    if ((rc = c->arena.check("kp_spec_null"))) return rc;
    hipStream_t st = c->stream;
    KP_HIP(hipMemsetAsync(d_counts, 0, n_cnt * 4, st));
    KP_HIP(hipMemsetAsync(d_stat, 0, 16, st));
    if (n_items) {
        uint8_t *d_seq = nullptr;
        kp_p_item *d_items = nullptr;
        if ((rc = scan_upload(c, "kp_spec_null", seq, n, items, 0, &d_seq, &d_items))) return rc;
        KP_HIP(hipMemcpyAsync(d_rates, rates, (size_t)P * 8, hipMemcpyHostToDevice, st));
        kp_nl_args A;
        A.seq = d_seq;
        A.items = d_items;
        A.n_units = (uint64_t)n_items * passes;
        A.k = k;
        A.fold = s->fold;
        A.mask = mask;
        A.lut = (const int4 *)s->d_lut;
        A.rates = d_rates;
        A.scale = scale;
        A.seed = seed;
        A.contig = contig_id;
        A.rep_first = rep_first;
        A.n_reps = n_reps;
        A.rc = chunk;
        A.passes = passes;
        A.counts = d_counts;
        A.stat = d_stat;
        const uint64_t grid = scan_grid(c, A.n_units, 2, "KP_NULL_GRID");  // 62 KB of LDS per workgroup
        A.steps = (A.n_units + grid - 1) / grid;
        if ((rc = scan_mark(c, 0))) return rc;
        if (by_type)
            hipLaunchKernelGGL((kp_null_kernel<true>), dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
        else
            hipLaunchKernelGGL((kp_null_kernel<false>), dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
        if ((rc = scan_launched(c, 1))) return rc;
    }
    unsigned long long stat[2] = {0, 0};
    KP_HIP(hipMemcpyAsync(counts, d_counts, n_cnt * 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(stat, d_stat, 16, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    if (n_items) {
        float ms = 0.f;
        if ((rc = scan_elapsed(c, 0, 1, &ms))) return rc;
        s->null.null_ms = ms;
    }
    uint64_t hits = 0;
    for (size_t i = 0; i < n_cnt; ++i) hits += counts[i];
    s->null.windows = stat[0];
    s->null.draws = stat[1] * n_reps;
    s->null.hits = hits;
    return KP_OK;
}

int kp_spec_last_null(kp_ctx *c, kp_spec_null_stats *out) {
    if (!out) return fail(KP_E_ARG, "kp_spec_last_null: null out");
    *out = spec_sess(c)->null;
    return KP_OK;
}

}  // extern "C"
