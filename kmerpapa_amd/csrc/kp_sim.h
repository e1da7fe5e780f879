// kp_sim.h -- random mutation sets drawn from a spectrum model (no reference counterpart).
// Included by kp_hip.hip after kp_spec.h.  Semantics: include/kmerpapa_hip.h.
//
// A position's window, validity, centre and folding are kp_spec_regions' (kp_s_class / kp_s_step /
// kp_s_code, the 16-byte table of kp_spec_begin).  A valid window reads its three pattern ids,
// turns their rates into the cumulative c0 <= c1 <= c2 and compares them with one uniform number
// that depends on (seed, contig, position, replicate) only: Philox4x32-10 keyed by the seed, its
// counter the position, the contig id and the replicate.  Everything is integer arithmetic or
// IEEE double products, adds and compares, in __host__ __device__ functions both sessions share,
// so a device session equals the host session bit for bit:
//   kp_sm_philox   the ten rounds
//   kp_sm_uniform  the counter and key of a position, and the 53-bit fraction of the output
//   kp_sm_cum      the three rates of a table entry, cumulated
//   kp_sm_pick     the slot u falls into, or 3
//   kp_sm_alt      the ALT byte of a slot on the forward strand
//
// The hits leave in position order without a sort and without an atomic deciding a place:
//   kp_sim_count_kernel    kp_spec_scan_kernel's grid, roll and batches of 16-byte gathers, then the
//                          batch's rate gathers, then the draws (the rounds start after every gather
//                          of the batch has been issued).  A thread counts its hits, the workgroup
//                          adds them (wave shuffles, four wave totals in LDS) and one thread stores
//                          item_hits[item]
//   kp_sim_offsets_kernel  one workgroup walks item_hits in pieces of 1,024: the exclusive scan and
//                          the total, which the host reads back (more than `cap`: the call ends)
//   kp_sim_write_kernel    the same roll and draws for the items that have hits.  A thread stages its
//                          hits in LDS ([rank][thread], as the track kernel's buffer), the workgroup
//                          scans the threads' counts -- a thread owns consecutive centres, so thread
//                          order is position order -- and each hit goes to
//                          item offset + thread offset + rank
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
#include "kp_spec.h"

#define KP_SM_M0 0xD2511F53u
#define KP_SM_M1 0xCD9E8D57u
#define KP_SM_W0 0x9E3779B9u
#define KP_SM_W1 0xBB67AE85u
#define KP_SM_SCAN 1024  // threads of the offsets kernel

// Philox4x32-10: x0..x3 = the counter on entry, the output on return.  The rounds stay a loop: the
// draw stands 64 times in the unrolled roll, and ten rounds written out at each would make the
// kernels several times their size.
__host__ __device__ inline void kp_sm_philox(uint32_t &x0, uint32_t &x1, uint32_t &x2, uint32_t &x3, uint32_t k0,
                                             uint32_t k1) {
#pragma unroll 1
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)KP_SM_M0 * x0, p1 = (uint64_t)KP_SM_M1 * x2;
        const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1;
        x0 = y0, x1 = (uint32_t)p1, x2 = y2, x3 = (uint32_t)p0;
        k0 += KP_SM_W0, k1 += KP_SM_W1;
    }
}

// the uniform number of a position: 53 bits of the output, exactly, in [0, 1)
__host__ __device__ inline double kp_sm_uniform(uint64_t seed, uint32_t contig, uint64_t pos, uint32_t replicate) {
    uint32_t x0 = (uint32_t)pos, x1 = (uint32_t)(pos >> 32), x2 = contig, x3 = replicate;
    kp_sm_philox(x0, x1, x2, x3, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (double)((((uint64_t)x1 << 32) | x0) >> 11) * 0x1p-53;
}

// r_s = rates[id_s] * scale (0.0 without a pattern), cumulated in slot order
__host__ __device__ inline void kp_sm_cum(int32_t id0, int32_t id1, int32_t id2, const double *rates, double scale,
                                          double c[3]) {
    const double r0 = id0 >= 0 ? rates[id0] * scale : 0.0;
    const double r1 = id1 >= 0 ? rates[id1] * scale : 0.0;
    const double r2 = id2 >= 0 ? rates[id2] * scale : 0.0;
    c[0] = r0;
    c[1] = c[0] + r1;
    c[2] = c[1] + r2;
}

// the slot u falls into, 3 = no mutation
__host__ __device__ inline uint32_t kp_sm_pick(double u, double c0, double c1, double c2) {
    return u < c0 ? 0u : (u < c1 ? 1u : (u < c2 ? 2u : 3u));
}

// The ALT of a slot as a forward-strand base code: `ref` = the centre base as read (0..3).  Under
// folding a window with G or T in the centre was replaced by its reverse complement, so the slot
// counts among the bases other than the complemented REF and its base is complemented back.
__host__ __device__ inline uint32_t kp_sm_alt(uint32_t ref, int fold, uint32_t slot) {
    const bool flip = fold && ref >= 2u;
    const uint32_t r = flip ? 3u - ref : ref;
    const uint32_t a = slot < r ? slot : slot + 1u;
    return flip ? 3u - a : a;
}

__host__ __device__ inline uint8_t kp_sm_base(uint32_t code) {
    return code == 0u ? 'A' : (code == 1u ? 'C' : (code == 2u ? 'G' : 'T'));
}

struct kp_sm_args {
    const uint8_t *seq;      // the contig, KP_S_PAD readable bytes past its end
    const kp_p_item *items;  // [n_items]
    uint32_t n_items, steps;
    int32_t k, fold;
    uint32_t mask;  // 4^k - 1
    const int4 *lut;      // [4^k]
    const double *rates;  // [P]
    double scale;
    uint64_t seed;
    uint32_t contig, replicate;
    uint32_t *item_hits;            // [n_items]: written by the count kernel, read by the write kernel
    const uint32_t *item_off;       // [n_items]: the exclusive scan of item_hits
    unsigned long long *windows;    // [1] += valid windows (count kernel)
    uint64_t *out_pos;              // [n_out]
    uint8_t *out_alt;
    int32_t *out_pid;
    uint32_t n_out;  // the total of item_hits: no hit is written at or past it
};

#ifdef __HIPCC__

// One item's roll and draws for this thread.  Returns its hits; *valid += its valid windows.  With
// WRITE hit number r goes to s_pid / s_meta [r][tid]: the pattern, and the centre's index in the
// thread's run (5 bits) with the forward ALT code above it.
template <bool WRITE>
__device__ inline uint32_t kp_sim_roll(const kp_sm_args &A, const kp_p_item it, uint32_t tid, int32_t *s_pid,
                                       uint8_t *s_meta, uint32_t *valid) {
    const int k = A.k, top = 2 * (A.k - 1), h = A.k / 2, cshift = 2 * (A.k - 1 - A.k / 2);
    const uint32_t r0 = tid * KP_S_RUN;
    const uint32_t cnt = r0 < it.count ? min((uint32_t)KP_S_RUN, it.count - r0) : 0u;
    uint32_t d[16], off, end;
    kp_p_load(A.seq, (uint64_t)it.first + r0 - (uint32_t)h, cnt ? cnt + (uint32_t)k - 1u : 0u, d, &off, &end);
    const uint32_t full0 = off + (uint32_t)k - 1u;  // the byte that completes the first window
    const uint64_t pos0 = (uint64_t)it.first + r0;  // the centre of that window
    uint32_t nh = 0, nv = 0;
    kp_s_win w{0u, 0u, 0u};
#pragma unroll
    for (uint32_t jb = 0; jb < 64; jb += KP_P_BATCH) {
        uint32_t code[KP_P_BATCH], ref[KP_P_BATCH];
        bool has[KP_P_BATCH];
        int4 p[KP_P_BATCH];
        double c[KP_P_BATCH][3];
#pragma unroll
        for (uint32_t q = 0; q < KP_P_BATCH; ++q) {  // (kp_scan_batch with the REF as read kept beside the code)
            const uint32_t j = jb + q;
            if (j >= off && j < end) kp_s_step(w, kp_s_class((d[j >> 2] >> (8u * (j & 3u))) & 0xffu), A.mask, top);
            has[q] = j >= full0 && j < end && w.valid >= (uint32_t)k;
            nv += has[q];
            code[q] = kp_s_code(w, k, A.fold);
            ref[q] = (w.fwd >> cshift) & 3u;
        }
#pragma unroll
        for (uint32_t q = 0; q < KP_P_BATCH; ++q)  // (code <= mask: the entry lies inside the table)
            p[q] = has[q] ? A.lut[code[q]] : make_int4(KP_P_NONE, KP_P_NONE, KP_P_NONE, KP_P_NONE);
#pragma unroll
        for (uint32_t q = 0; q < KP_P_BATCH; ++q)  // (ids < P: the table holds indices of the pattern list only)
            kp_sm_cum(p[q].x, p[q].y, p[q].z, A.rates, A.scale, c[q]);
#pragma unroll
        for (uint32_t q = 0; q < KP_P_BATCH; ++q) {
            if (c[q][2] > 0.0) {  // (a window without has[q] has no id, so its c2 is 0.0)
                const uint32_t run = jb + q - full0;  // < cnt <= KP_S_RUN
                const double u = kp_sm_uniform(A.seed, A.contig, pos0 + run, A.replicate);
                const uint32_t slot = kp_sm_pick(u, c[q][0], c[q][1], c[q][2]);
                if (slot < 3u) {
                    if (WRITE && nh < (uint32_t)KP_S_RUN) {
                        s_pid[nh * KP_P_ROW + tid] = slot == 0u ? p[q].x : (slot == 1u ? p[q].y : p[q].z);
                        s_meta[nh * KP_P_ROW + tid] = (uint8_t)(run | (kp_sm_alt(ref[q], A.fold, slot) << 5));
                    }
                    ++nh;
                }
            }
        }
    }
    *valid += nv;
    return nh;
}

__global__ void __launch_bounds__(KP_S_THREADS) kp_sim_count_kernel(kp_sm_args A) {
    __shared__ uint32_t s_hits[KP_S_THREADS / 64], s_valid[KP_S_THREADS / 64];
    const uint32_t tid = threadIdx.x;
    for (uint32_t s = 0; s < A.steps; ++s) {
        const uint32_t item = s * gridDim.x + blockIdx.x;
        if (item >= A.n_items) break;  // (the same for the whole workgroup)
        uint32_t nv = 0;
        uint32_t nh = kp_sim_roll<false>(A, A.items[item], tid, nullptr, nullptr, &nv);
        for (int o = 32; o; o >>= 1) {
            nh += __shfl_xor(nh, o, 64);
            nv += __shfl_xor(nv, o, 64);
        }
        if ((tid & 63u) == 0) s_hits[tid >> 6] = nh, s_valid[tid >> 6] = nv;
        __syncthreads();
        if (tid == 0) {
            uint32_t th = 0, tv = 0;
            for (uint32_t x = 0; x < KP_S_THREADS / 64; ++x) th += s_hits[x], tv += s_valid[x];
            A.item_hits[item] = th;
            if (tv) atomicAdd(A.windows, (unsigned long long)tv);
        }
        __syncthreads();  // read before the next item's totals arrive
    }
}

// off[i] = hits[0] + .. + hits[i - 1], *total = their sum (below 2^32: at most one hit per
// position of a contig shorter than that).  One workgroup.
__global__ void __launch_bounds__(KP_SM_SCAN) kp_sim_offsets_kernel(const uint32_t *__restrict__ hits, uint32_t n_items,
                                                                    uint32_t *__restrict__ off, uint32_t *__restrict__ total) {
    __shared__ uint32_t s_wave[KP_SM_SCAN / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t b = 0; b < n_items; b += KP_SM_SCAN) {  // (b and carry are the same for every thread)
        const uint32_t i = b + tid;
        const uint32_t v = i < n_items ? hits[i] : 0u;
        uint32_t inc = v;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63u) s_wave[wv] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t x = 0; x < KP_SM_SCAN / 64; ++x) {
            const uint32_t t = s_wave[x];
            before += x < wv ? t : 0u;
            all += t;
        }
        if (i < n_items) off[i] = carry + before + inc - v;
        carry += all;
        __syncthreads();  // read before the next piece's wave totals arrive
    }
    if (tid == 0) *total = carry;
}

__global__ void __launch_bounds__(KP_S_THREADS) kp_sim_write_kernel(kp_sm_args A) {
    __shared__ int32_t s_pid[KP_S_RUN * KP_P_ROW];   // [rank][thread]
    __shared__ uint8_t s_meta[KP_S_RUN * KP_P_ROW];
    __shared__ uint32_t s_wave[KP_S_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint32_t s = 0; s < A.steps; ++s) {
        const uint32_t item = s * gridDim.x + blockIdx.x;
        if (item >= A.n_items) break;            // (the same for the whole workgroup)
        if (A.item_hits[item] == 0u) continue;   // (and so is this)
        const kp_p_item it = A.items[item];
        uint32_t nv = 0;
        const uint32_t nh = kp_sim_roll<true>(A, it, tid, s_pid, s_meta, &nv);
        uint32_t inc = nh;
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (lane == 63u) s_wave[wv] = inc;
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t x = 0; x < KP_S_THREADS / 64; ++x) before += x < wv ? s_wave[x] : 0u;
        const uint64_t base = (uint64_t)A.item_off[item] + before + inc - nh;
        const uint64_t pos0 = (uint64_t)it.first + tid * KP_S_RUN;
        for (uint32_t r = 0; r < nh && r < (uint32_t)KP_S_RUN; ++r) {  // (a thread reads the slots it wrote itself)
            const uint64_t o = base + r;
            if (o >= A.n_out) break;  // (never: the count kernel drew the same hits)
            const uint32_t m = s_meta[r * KP_P_ROW + tid];
            A.out_pos[o] = pos0 + (m & 31u);
            A.out_alt[o] = kp_sm_base(m >> 5);
            A.out_pid[o] = s_pid[r * KP_P_ROW + tid];
        }
        __syncthreads();  // the wave totals are read before the next item's arrive
    }
}

#endif  // __HIPCC__

// ---------------------------------------------------------------------------
// the call, in a kp_spec session
// ---------------------------------------------------------------------------

// finite rates >= 0, and per REF base the sum over its three types of the type's largest
// rates[p] * scale at most 1.0, so that c2 <= 1 at every window
static int sim_check_rates(const kp_spec_sess *s, const double *rates, double scale) {
    const uint32_t P = (uint32_t)s->pats.size();
    if (!std::isfinite(scale) || scale < 0.0)
        return fail(KP_E_ARG, "kp_spec_simulate: scale " + std::to_string(scale) + " is negative or not finite");
    for (uint32_t p = 0; p < P; ++p)
        if (!std::isfinite(rates[p]) || rates[p] < 0.0)
            return fail(KP_E_ARG, "kp_spec_simulate: the rate " + std::to_string(rates[p]) + " of pattern " + std::to_string(p) +
                                      " is negative or not finite");
    for (uint32_t ref = 0; ref < 4; ++ref) {
        double sum = 0.0;
        for (uint32_t slot = 0; slot < 3; ++slot) {
            const uint32_t t = 3 * ref + slot;
            double top = 0.0;
            for (uint32_t e = s->type_off[t]; e < s->type_off[t + 1]; ++e) top = std::max(top, rates[s->by_type[e]] * scale);
            sum = sum + top;
        }
        if (!(sum <= 1.0))
            return fail(KP_E_ARG, std::string("kp_spec_simulate: the largest rates of the three types with REF ") + "ACGT"[ref] +
                                      " times scale add up to " + std::to_string(sum) + ", more than 1");
    }
    return KP_OK;
}

extern "C" {

int kp_spec_simulate(kp_ctx *c, const uint8_t *seq, uint64_t n, uint32_t contig_id, const uint64_t *reg_begin,
                     const uint64_t *reg_end, uint64_t n_regions, const double *rates, double scale, uint64_t seed,
                     uint32_t replicate, uint64_t cap, uint64_t *out_pos, uint8_t *out_alt, int32_t *out_pid,
                     uint64_t *n_hits) {
    kp_spec_sess *s = spec_sess(c);
    int rc = scan_check_contig("kp_spec_simulate", s->active, seq, n, "kp_spec_begin");
    if (rc) return rc;
    if (!n_hits) return fail(KP_E_ARG, "kp_spec_simulate: null n_hits");
    if (!rates) return fail(KP_E_ARG, "kp_spec_simulate: null rates");
    if (n_regions >= (1ull << 32)) return fail(KP_E_ARG, "kp_spec_simulate: 2^32 regions or more in one call");
    if (n_regions && (!reg_begin || !reg_end)) return fail(KP_E_ARG, "kp_spec_simulate: null regions");
    if (cap && (!out_pos || !out_alt || !out_pid)) return fail(KP_E_ARG, "kp_spec_simulate: null outputs with cap > 0");
    if ((rc = sim_check_rates(s, rates, scale))) return rc;
    if ((rc = scan_check_regions("kp_spec_simulate", n, reg_begin, reg_end, n_regions, true))) return rc;
    s->sim = kp_spec_sim_stats{};
    *n_hits = 0;
    const int k = s->k;
    const uint32_t P = (uint32_t)s->pats.size();
    const uint32_t mask = (uint32_t)(s->cells - 1);
    uint64_t lo = 0, hi = 0;
    scan_centres(n, k, &lo, &hi);
    if (!c) {
        std::vector<uint64_t> h_pos;
        std::vector<uint8_t> h_alt;
        std::vector<int32_t> h_pid;
        uint64_t hits = 0, windows = 0, n_items = 0;
        try {
            for (uint64_t r = 0; r < n_regions; ++r) {
                const uint64_t b = std::max(reg_begin[r], lo), e = std::min(reg_end[r], hi);
                n_items += scan_pieces(reg_begin[r], reg_end[r], lo, hi);
                for (uint64_t p = b; p < e; ++p) {
                    uint32_t code = 0;
                    if (!kp_p_window(seq, n, p, k, s->fold, mask, &code)) continue;
                    ++windows;
                    const int32_t *id = &s->h_lut[4ull * code];
                    double cum[3];
                    kp_sm_cum(id[0], id[1], id[2], rates, scale, cum);
                    if (!(cum[2] > 0.0)) continue;
                    const uint32_t slot = kp_sm_pick(kp_sm_uniform(seed, contig_id, p, replicate), cum[0], cum[1], cum[2]);
                    if (slot >= 3u) continue;
                    if (hits < cap) {
                        h_pos.push_back(p);
                        h_alt.push_back(kp_sm_base(kp_sm_alt(kp_s_class(seq[p]) & 3u, s->fold, slot)));
                        h_pid.push_back(id[slot]);
                    }
                    ++hits;
                }
            }
        } catch (const std::bad_alloc &) {
            return fail(KP_E_NOMEM, "kp_spec_simulate: the hits do not fit host memory");
        }
        if (hits && hits <= cap) {
            memcpy(out_pos, h_pos.data(), hits * 8);
            memcpy(out_alt, h_alt.data(), hits);
            memcpy(out_pid, h_pid.data(), hits * 4);
        }
        *n_hits = hits;
        s->sim.windows = windows;
        s->sim.hits = hits;
        s->sim.items = n_items;
        return KP_OK;
    }

    KP_HIP(hipSetDevice(c->device));
    std::vector<kp_p_item> items;
    uint64_t centres = 0;
    try {
        for (uint64_t r = 0; r < n_regions; ++r) centres += scan_cut(items, reg_begin[r], reg_end[r], lo, hi, (uint32_t)r);
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_spec_simulate: the work items do not fit host memory");
    }
    if (items.size() >= (1ull << 32)) return fail(KP_E_ARG, "kp_spec_simulate: 2^32 work items or more in one call");
    s->sim.items = items.size();
    if (items.empty()) return KP_OK;
    const size_t n_items = items.size();
    const uint64_t room = std::min<uint64_t>(cap, centres);  // hits the outputs on the device hold
    const size_t extra = 2 * g_up(n_items * 4) + 2 * g_up(8) + g_up((size_t)P * 8) + g_up(room * 8) + g_up(room) + g_up(room * 4);
    if ((rc = spec_arena(c, "kp_spec_simulate", extra))) return rc;
    uint32_t *d_hits = (uint32_t *)c->arena.take(n_items * 4);
    uint32_t *d_off = (uint32_t *)c->arena.take(n_items * 4);
    uint32_t *d_total = (uint32_t *)c->arena.take(8);
    unsigned long long *d_windows = (unsigned long long *)c->arena.take(8);
    double *d_rates = (double *)c->arena.take((size_t)P * 8);
    uint64_t *d_pos = (uint64_t *)c->arena.take(room * 8);
    uint8_t *d_alt = (uint8_t *)c->arena.take(room);
    int32_t *d_pid = (int32_t *)c->arena.take(room * 4);
    if ((rc = c->arena.check("kp_spec_simulate"))) return rc;
    hipStream_t st = c->stream;
    uint8_t *d_seq = nullptr;
    kp_p_item *d_items = nullptr;
    if ((rc = scan_upload(c, "kp_spec_simulate", seq, n, items, 0, &d_seq, &d_items))) return rc;
    KP_HIP(hipMemcpyAsync(d_rates, rates, (size_t)P * 8, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemsetAsync(d_total, 0, 8, st));
    KP_HIP(hipMemsetAsync(d_windows, 0, 8, st));
    kp_sm_args A;
    A.seq = d_seq;
    A.items = d_items;
    A.n_items = (uint32_t)n_items;
    A.k = k;
    A.fold = s->fold;
    A.mask = mask;
    A.lut = (const int4 *)s->d_lut;
    A.rates = d_rates;
    A.scale = scale;
    A.seed = seed;
    A.contig = contig_id;
    A.replicate = replicate;
    A.item_hits = d_hits;
    A.item_off = d_off;
    A.windows = d_windows;
    A.out_pos = d_pos;
    A.out_alt = d_alt;
    A.out_pid = d_pid;
    A.n_out = 0;
    // persistent grids: as many workgroups as are resident at once
    uint64_t grid = scan_grid(c, n_items, 4, "KP_SIM_GRID");
    A.steps = (uint32_t)((n_items + grid - 1) / grid);
    if ((rc = scan_mark(c, 0))) return rc;
    hipLaunchKernelGGL(kp_sim_count_kernel, dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
    KP_HIP(hipGetLastError());
    hipLaunchKernelGGL(kp_sim_offsets_kernel, dim3(1), dim3(KP_SM_SCAN), 0, st, d_hits, (uint32_t)n_items, d_off, d_total);
    if ((rc = scan_launched(c, 1))) return rc;
    uint32_t total = 0;
    unsigned long long windows = 0;
    KP_HIP(hipMemcpyAsync(&total, d_total, 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(&windows, d_windows, 8, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    if ((rc = scan_elapsed(c, 0, 1, &ms))) return rc;
    s->sim.count_ms = ms;
    s->sim.windows = windows;
    s->sim.hits = total;
    *n_hits = total;
    if (total == 0 || total > cap) return KP_OK;
    if (total > room) return fail(KP_E_PARITY, "kp_spec_simulate: more hits than centres");
    A.n_out = total;
    grid = scan_grid(c, n_items, 3, "KP_SIM_GRID");  // 41 KB of LDS per workgroup
    A.steps = (uint32_t)((n_items + grid - 1) / grid);
    if ((rc = scan_mark(c, 2))) return rc;
    hipLaunchKernelGGL(kp_sim_write_kernel, dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
    if ((rc = scan_launched(c, 3))) return rc;
    KP_HIP(hipMemcpyAsync(out_pos, d_pos, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(out_alt, d_alt, (size_t)total, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(out_pid, d_pid, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    if ((rc = scan_elapsed(c, 2, 3, &ms))) return rc;
    s->sim.write_ms = ms;
    return KP_OK;
}

int kp_spec_last_sim(kp_ctx *c, kp_spec_sim_stats *out) {
    if (!out) return fail(KP_E_ARG, "kp_spec_last_sim: null out");
    *out = spec_sess(c)->sim;
    return KP_OK;
}

}  // extern "C"
