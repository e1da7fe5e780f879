// kp_spec.h -- the whole mutation spectrum in one genome pass (no reference counterpart).
// Included by kp_hip.hip.  Semantics: include/kmerpapa_hip.h.
//
// A mutation type is t = 3 * code(REF) + slot, slot = the rank of ALT among the bases != REF in
// ACGT order; a window's centre base is the (folded) REF, so the three slots of a k-mer code cover
// every type.  One pattern list holds every type's partition (ptype[p] = the type of pattern p),
// and one table of 16-byte entries {pattern of slot 0, 1, 2, -1} per code answers all three with
// one gather.  Windows, validity, the centre and folding are kp_seq.h's (kp_s_class / kp_s_step /
// kp_s_code), matching is kp_apply.h's (kp_a_onehot / kp_a_match), the window of a site is
// kp_pred.h's (kp_p_window), the scan's skeleton on device and host is kp_scan.h's.  Counts are
// integers and `expected` is a float64 sum in pattern order per type, so a device session equals
// the host session bit for bit.
//
//   kp_spec_lut_kernel        one k-mer code per thread against every pattern, staged through LDS
//                             in tiles with their slots (as kp_pred_lut_kernel): the first match
//                             of each slot; codes the scan cannot produce are not tested
//   kp_spec_scan_kernel       kp_pred_scan_kernel's grid, roll and batches; a valid window does one
//                             16-byte gather and up to three adds -- into the item's uint32 LDS
//                             counters (flushed to the region's row after it) or with global 64-bit
//                             atomics.  other[region][4] gets one atomic per wave, item and counter
//   kp_spec_track_kernel      kp_pred_track_kernel's roll and transposed LDS buffer, once per slot
//                             plane: the second and third pass gather lines the first one fetched
//   kp_spec_sites_kernel      one thread per site: the id in the slot of the (folded) ALT
//   kp_spec_sums_kernel       one thread per (region, type): expected, over the type's patterns in
//                             order (the host lists them per type, so a thread reads only its own)
//   kp_seq_sites_typed_kernel one thread per site, as kp_seq_sites_kernel: + 1 in column slot
//
// Every device loop has a bound the host computed; there are no waits between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "kp_apply.h"
#include "kp_pred.h"
#include "kp_rt.h"
#include "kp_seq.h"

#define KP_SP_TYPES 12
#define KP_SP_ALT_IS_REF (-3)

// the slot of ALT (0..3, != ref) among the bases other than ref
__host__ __device__ inline uint32_t kp_sp_slot(uint32_t ref, uint32_t alt) { return alt < ref ? alt : alt - 1u; }

// A site: the code of its window and the slot of its ALT byte on the counted strand.  Returns 0,
// KP_P_INVALID (the window leaves the contig or holds an invalid byte) or KP_SP_ALT_IS_REF.
// `alt` must be one of ACGTacgt (the host checks it).
__host__ __device__ inline int kp_sp_site(const uint8_t *seq, uint64_t n, uint64_t p, uint32_t alt, int k, int fold,
                                          uint32_t mask, uint32_t *code, uint32_t *slot) {
    if (!kp_p_window(seq, n, p, k, fold, mask, code)) return KP_P_INVALID;
    uint32_t ref = kp_s_class(seq[p]) & 3u, a = kp_s_class(alt) & 3u;
    if (fold && ref >= 2u) ref = 3u - ref, a = 3u - a;  // the window was replaced by its reverse complement
    if (a == ref) return KP_SP_ALT_IS_REF;
    *slot = kp_sp_slot(ref, a);
    return 0;
}

// the first pattern of each slot a one-hot word matches, or -1
__host__ __device__ inline void kp_sp_find(uint64_t oh, const uint64_t *pats, const uint32_t *ptype, uint32_t P,
                                           int32_t out[4]) {
    int32_t f0 = KP_P_NONE, f1 = KP_P_NONE, f2 = KP_P_NONE;
    for (uint32_t j = 0; j < P && (f0 < 0 || f1 < 0 || f2 < 0); ++j) {
        if (!kp_a_match(oh, pats[j])) continue;
        const uint32_t s = ptype[j] % 3u;
        if (s == 0u && f0 < 0) f0 = (int32_t)j;
        if (s == 1u && f1 < 0) f1 = (int32_t)j;
        if (s == 2u && f2 < 0) f2 = (int32_t)j;
    }
    out[0] = f0, out[1] = f1, out[2] = f2, out[3] = KP_P_NONE;
}

struct kp_sp_args {
    const uint8_t *seq;      // the contig, KP_S_PAD readable bytes past its end
    const kp_p_item *items;  // [n_items]
    uint32_t n_items, steps;
    int32_t k, fold;
    uint32_t mask;  // 4^k - 1
    uint32_t P;
    const int4 *lut;            // [4^k]
    unsigned long long *hist;   // [n_regions][P]
    unsigned long long *other;  // [n_regions][4]: no pattern in slot 0, 1, 2; invalid
};

struct kp_sp_offs {
    uint32_t off[KP_SP_TYPES + 1];  // by_type[off[t] .. off[t + 1]) are the patterns of type t, ascending
};

struct kp_sp_targs {
    const uint8_t *seq;
    uint32_t begin, len;  // positions [begin, begin + len)
    uint32_t lo, hi;      // centres whose window lies inside the contig
    uint32_t n_items, steps;
    int32_t k, fold;
    uint32_t mask;
    const int4 *lut;
    int32_t *pid;     // [3][plane], 256-byte aligned
    uint64_t plane;   // int32 between two planes, a multiple of 64
};

#ifdef __HIPCC__

__global__ void __launch_bounds__(256) kp_spec_lut_kernel(const uint64_t *__restrict__ pats,
                                                          const uint32_t *__restrict__ ptype, uint32_t P, int k, int fold,
                                                          uint32_t cells, int4 *__restrict__ lut) {
    __shared__ unsigned long long sT[KP_P_LUT_TILE];
    __shared__ uint32_t sS[KP_P_LUT_TILE];  // the slot of each staged pattern
    const uint32_t tid = threadIdx.x;
    const uint32_t code = blockIdx.x * 256u + tid;
    const bool act = code < cells && kp_p_reachable(code, k, fold);
    const uint64_t oh = act ? kp_a_onehot(code, k) : 0;
    int32_t f0 = KP_P_NONE, f1 = KP_P_NONE, f2 = KP_P_NONE;
    for (uint32_t t0 = 0; t0 < P; t0 += KP_P_LUT_TILE) {
        const uint32_t nt = P - t0 < KP_P_LUT_TILE ? P - t0 : KP_P_LUT_TILE;
        __syncthreads();  // the previous tile has been read by every wave
        for (uint32_t e = tid; e < nt; e += 256u) {
            sT[e] = pats[t0 + e];
            sS[e] = ptype[t0 + e] % 3u;
        }
        __syncthreads();
        if (act && (f0 < 0 || f1 < 0 || f2 < 0)) {
#pragma unroll 4
            for (uint32_t j = 0; j < nt; ++j) {
                const bool m = kp_a_match(oh, sT[j]);
                const uint32_t s = sS[j];
                const int32_t id = (int32_t)(t0 + j);
                f0 = (m && s == 0u && f0 < 0) ? id : f0;
                f1 = (m && s == 1u && f1 < 0) ? id : f1;
                f2 = (m && s == 2u && f2 < 0) ? id : f2;
            }
        }
    }
    if (code < cells) lut[code] = make_int4(f0, f1, f2, KP_P_NONE);
}

template <bool LDS>
__global__ void __launch_bounds__(KP_S_THREADS) kp_spec_scan_kernel(kp_sp_args A) {
    extern __shared__ uint32_t kp_sp_cnt[];  // [P] with LDS
    const uint32_t tid = threadIdx.x;
    if (LDS) {
        for (uint32_t e = tid; e < A.P; e += KP_S_THREADS) kp_sp_cnt[e] = 0;
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
        uint32_t none0 = 0, none1 = 0, none2 = 0, inv = 0;
        kp_s_win w{0u, 0u, 0u};
#pragma unroll
        for (uint32_t jb = 0; jb < 64; jb += KP_P_BATCH) {
            uint32_t code[KP_P_BATCH];
            bool has[KP_P_BATCH];
            int4 p[KP_P_BATCH];
            kp_scan_batch(w, d, jb, off, end, full0, k, A.fold, A.mask, top, code, has, inv);
#pragma unroll
            for (uint32_t q = 0; q < KP_P_BATCH; ++q)  // (code <= mask: the entry lies inside the table)
                p[q] = has[q] ? A.lut[code[q]] : make_int4(KP_P_INVALID, KP_P_INVALID, KP_P_INVALID, KP_P_INVALID);
#pragma unroll
            for (uint32_t q = 0; q < KP_P_BATCH; ++q) {
                const int32_t id[3] = {p[q].x, p[q].y, p[q].z};
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    if (id[e] >= 0) {  // (< P: the table holds indices of the pattern list only)
                        if (LDS)
                            atomicAdd(&kp_sp_cnt[id[e]], 1u);
                        else
                            atomicAdd(&row[id[e]], 1ull);
                    }
                }
                none0 += p[q].x == KP_P_NONE;
                none1 += p[q].y == KP_P_NONE;
                none2 += p[q].z == KP_P_NONE;
            }
        }
        for (int o = 32; o; o >>= 1) {
            none0 += __shfl_xor(none0, o, 64);
            none1 += __shfl_xor(none1, o, 64);
            none2 += __shfl_xor(none2, o, 64);
            inv += __shfl_xor(inv, o, 64);
        }
        if ((tid & 63u) == 0) {
            unsigned long long *o = A.other + 4ull * it.region;
            if (none0) atomicAdd(&o[0], (unsigned long long)none0);
            if (none1) atomicAdd(&o[1], (unsigned long long)none1);
            if (none2) atomicAdd(&o[2], (unsigned long long)none2);
            if (inv) atomicAdd(&o[3], (unsigned long long)inv);
        }
        if (LDS) {
            __syncthreads();  // every add of the item is in
            for (uint32_t e = tid; e < A.P; e += KP_S_THREADS) {
                const uint32_t v = kp_sp_cnt[e];
                if (v) {
                    atomicAdd(&row[e], (unsigned long long)v);
                    kp_sp_cnt[e] = 0;
                }
            }
            __syncthreads();  // zero again before the next item adds
        }
    }
}

__global__ void __launch_bounds__(KP_S_THREADS) kp_spec_track_kernel(kp_sp_targs A) {
    __shared__ int32_t buf[KP_S_RUN * KP_P_ROW];  // [slot of the run][thread]
    const uint32_t tid = threadIdx.x;
    const int k = A.k, top = 2 * (A.k - 1), h = A.k / 2;
    for (uint32_t s = 0; s < A.steps; ++s) {
        const uint32_t item = s * gridDim.x + blockIdx.x;
        if (item >= A.n_items) break;  // (the same for the whole workgroup)
        const uint64_t base = (uint64_t)item * KP_S_TILE;  // of the item in a plane
        const uint64_t i0 = base + tid * KP_S_RUN;
        const uint32_t cnt = i0 >= A.len ? 0u : (A.len - i0 < KP_S_RUN ? (uint32_t)(A.len - i0) : (uint32_t)KP_S_RUN);
        // this thread's positions [c0, c0 + cnt), of which [cb, cb + nc) have a window inside the contig
        const uint64_t c0 = (uint64_t)A.begin + i0;
        const uint64_t cb = c0 > A.lo ? c0 : (uint64_t)A.lo, ce = c0 + cnt < A.hi ? c0 + cnt : (uint64_t)A.hi;
        const uint32_t nc = ce > cb ? (uint32_t)(ce - cb) : 0u;
        uint32_t d[16], off, end;
        kp_p_load(A.seq, nc ? cb - (uint32_t)h : 0u, nc ? nc + (uint32_t)k - 1u : 0u, d, &off, &end);
        const uint32_t full0 = off + (uint32_t)k - 1u;
        const uint32_t slot0 = nc ? (uint32_t)(cb - c0) : 0u;  // of the first window: byte j fills slot0 + j - full0
        for (int plane = 0; plane < 3; ++plane) {
#pragma unroll
            for (uint32_t q = 0; q < KP_S_RUN; ++q) buf[q * KP_P_ROW + tid] = KP_P_INVALID;
            uint32_t inv = 0;  // (not reported: the slots of invalid windows keep their -2)
            kp_s_win w{0u, 0u, 0u};
#pragma unroll
            for (uint32_t jb = 0; jb < 64; jb += KP_P_BATCH) {
                uint32_t code[KP_P_BATCH];
                bool has[KP_P_BATCH];
                int4 p[KP_P_BATCH];
                kp_scan_batch(w, d, jb, off, end, full0, k, A.fold, A.mask, top, code, has, inv);
#pragma unroll
                for (uint32_t q = 0; q < KP_P_BATCH; ++q) p[q] = has[q] ? A.lut[code[q]] : make_int4(0, 0, 0, 0);
#pragma unroll
                for (uint32_t q = 0; q < KP_P_BATCH; ++q)  // slot0 + j - full0 < slot0 + nc <= KP_S_RUN
                    if (has[q])
                        buf[(slot0 + jb + q - full0) * KP_P_ROW + tid] = plane == 0 ? p[q].x : (plane == 1 ? p[q].y : p[q].z);
            }
            __syncthreads();
            // the item's results leave in position order: vector v holds slots 4 (v % 8) .. + 3 of thread v / 8
            int32_t *out = A.pid + (uint64_t)plane * A.plane;
#pragma unroll
            for (uint32_t q = 0; q < KP_S_RUN / 4; ++q) {
                const uint32_t v = q * KP_S_THREADS + tid, t = v >> 3, w0 = (v & 7u) * 4u;
                const uint64_t o = base + 4ull * v;
                if (o < A.len) {
                    const int4 r = make_int4(buf[w0 * KP_P_ROW + t], buf[(w0 + 1) * KP_P_ROW + t],
                                             buf[(w0 + 2) * KP_P_ROW + t], buf[(w0 + 3) * KP_P_ROW + t]);
                    if (o + 4 <= A.len) {
                        *reinterpret_cast<int4 *>(out + o) = r;
                    } else {  // the last positions of the range
                        out[o] = r.x;
                        if (o + 1 < A.len) out[o + 1] = r.y;
                        if (o + 2 < A.len) out[o + 2] = r.z;
                    }
                }
            }
            __syncthreads();  // read before the next plane or item fills the slots
        }
    }
}

__global__ void __launch_bounds__(256) kp_spec_sites_kernel(const uint8_t *__restrict__ seq, uint64_t n,
                                                            const uint64_t *__restrict__ pos,
                                                            const uint8_t *__restrict__ alt, uint64_t n_sites, int k,
                                                            int fold, uint32_t mask, const int32_t *__restrict__ lut,
                                                            int32_t *__restrict__ pid) {
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n_sites) return;
    uint32_t code = 0, slot = 0;
    const int rc = kp_sp_site(seq, n, pos[i], alt[i], k, fold, mask, &code, &slot);
    pid[i] = rc ? rc : lut[4ull * code + slot];
}

__global__ void __launch_bounds__(64) kp_spec_sums_kernel(const unsigned long long *__restrict__ hist,
                                                          const double *__restrict__ rates,
                                                          const uint32_t *__restrict__ by_type, kp_sp_offs T,
                                                          uint32_t P, uint64_t n_regions,
                                                          double *__restrict__ expected) {
    const uint64_t i = blockIdx.x * 64ull + threadIdx.x;
    if (i >= n_regions * KP_SP_TYPES) return;
    const uint64_t r = i / KP_SP_TYPES;
    const uint32_t t = (uint32_t)(i % KP_SP_TYPES);
    const unsigned long long *row = hist + r * P;
    double acc = 0.0;
    for (uint32_t e = T.off[t]; e < T.off[t + 1]; ++e) {  // (off[12] = P: e indexes by_type[P])
        const uint32_t p = by_type[e];
        acc = acc + (double)row[p] * rates[p];
    }
    expected[i] = acc;
}

// tab = the three positive columns; stat[1] += sites counted, stat[2] += sites skipped
__global__ void __launch_bounds__(256) kp_seq_sites_typed_kernel(const uint8_t *__restrict__ seq, uint64_t n,
                                                                 const uint64_t *__restrict__ pos,
                                                                 const uint8_t *__restrict__ alt, uint64_t n_sites, int k,
                                                                 int fold, uint32_t cells, unsigned long long *tab,
                                                                 unsigned long long *stat) {
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    const bool act = i < n_sites;
    bool ok = false;
    if (act) {
        uint32_t code = 0, slot = 0;
        ok = kp_sp_site(seq, n, pos[i], alt[i], k, fold, cells - 1u, &code, &slot) == 0;
        if (ok) atomicAdd(&tab[(uint64_t)slot * cells + code], 1ull);
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

static thread_local kp_spec_sess g_spec_host;

static kp_spec_sess *spec_sess(kp_ctx *c) { return c ? &c->spec : &g_spec_host; }

// positions on the contig and ALT bytes that are bases
static int spec_check_sites(const std::string &w, uint64_t n, const uint64_t *pos, const uint8_t *alt, uint64_t n_sites) {
    if (n_sites && (!pos || !alt)) return fail(KP_E_ARG, w + ": null positions or ALT bases");
    if (n_sites >= (1ull << 39)) return fail(KP_E_ARG, w + ": 2^39 sites or more in one call");
    for (uint64_t i = 0; i < n_sites; ++i) {
        if (pos[i] >= n)
            return fail(KP_E_ARG, w + ": site " + std::to_string(i) + " at " + std::to_string(pos[i]) +
                                      " lies past the contig's " + std::to_string(n) + " bases");
        if (kp_s_class(alt[i]) > 3u)
            return fail(KP_E_ARG, w + ": site " + std::to_string(i) + " has an ALT byte " + std::to_string((int)alt[i]) +
                                      " that is none of ACGTacgt");
    }
    return KP_OK;
}

// scan_arena for the table of 16-byte entries: the table first, then `extra` bytes the caller takes
static int spec_arena(kp_ctx *c, const char *who, size_t extra) {
    kp_spec_sess *s = &c->spec;
    const uint32_t P = (uint32_t)s->pats.size();
    return scan_arena(c, s, who, "spectrum", 16, g_up((size_t)P * 8) + g_up((size_t)P * 4), extra, [&]() -> int {
        uint64_t *d_pats = (uint64_t *)c->arena.take((size_t)P * 8);
        uint32_t *d_type = (uint32_t *)c->arena.take((size_t)P * 4);
        int rc = c->arena.check(who);
        if (rc) return rc;
        KP_HIP(hipMemcpyAsync(d_pats, s->pats.data(), (size_t)P * 8, hipMemcpyHostToDevice, c->stream));
        KP_HIP(hipMemcpyAsync(d_type, s->ptype.data(), (size_t)P * 4, hipMemcpyHostToDevice, c->stream));
        if ((rc = scan_mark(c, 0))) return rc;
        hipLaunchKernelGGL(kp_spec_lut_kernel, dim3((unsigned)((s->cells + 255) / 256)), dim3(256), 0, c->stream, d_pats,
                           d_type, P, s->k, s->fold, (uint32_t)s->cells, (int4 *)s->d_lut);
        return scan_launched(c, 1);
    });
}

extern "C" {

int kp_spec_begin(kp_ctx *c, int k, int fold, const uint64_t *patterns, const uint32_t *ptype, uint32_t n_patterns) {
    kp_spec_sess *s = spec_sess(c);
    if (s->active) return fail(KP_E_STATE, "kp_spec_begin: a session is open (kp_spec_end first)");
    if (c && c->seq.active)
        return fail(KP_E_STATE, "kp_spec_begin: a kp_seq session holds the context's arena (kp_seq_end first)");
    if (c && c->pred.active)
        return fail(KP_E_STATE, "kp_spec_begin: a kp_pred session holds the context's arena (kp_pred_end first)");
    if (c && c->ispec.active)
        return fail(KP_E_STATE, "kp_spec_begin: a kp_ispec session holds the context's arena (kp_ispec_end first)");
    if (k < 1 || k > KP_S_MAXK) return fail(KP_E_ARG, "kp_spec_begin: k must be 1..15 (a dense table of 4^k entries)");
    if (fold && k % 2 == 0) return fail(KP_E_ARG, "kp_spec_begin: strand folding needs an odd k (a centre base)");
    const uint32_t P = n_patterns;
    if (P == 0) return fail(KP_E_ARG, "kp_spec_begin: no patterns");
    if (!patterns || !ptype) return fail(KP_E_ARG, "kp_spec_begin: null patterns or types");
    if (P >= (1u << 30)) return fail(KP_E_ARG, "kp_spec_begin: 2^30 patterns or more");
    const uint32_t n_types = fold ? 6u : (uint32_t)KP_SP_TYPES;
    for (uint32_t p = 0; p < P; ++p) {
        if (!apply_word_ok(patterns[p], k))
            return fail(KP_E_ARG, "kp_spec_begin: pattern " + std::to_string(p) + " has an empty position or bits above position k");
        if (ptype[p] >= n_types)
            return fail(KP_E_ARG, "kp_spec_begin: pattern " + std::to_string(p) + " has type " + std::to_string(ptype[p]) +
                                      ", not 0.." + std::to_string(n_types - 1) + (fold ? " (strand folding)" : ""));
        if (((patterns[p] >> (4 * (k / 2))) & 15u) != (1u << (ptype[p] / 3u)))
            return fail(KP_E_ARG, "kp_spec_begin: the centre of pattern " + std::to_string(p) +
                                      " must allow exactly the REF base of its type " + std::to_string(ptype[p]));
    }
    const uint64_t low = kp_a_low(k);
    try {
        std::vector<uint64_t> of_type;
        for (uint32_t t = 0; t < n_types; ++t) {
            of_type.clear();
            for (uint32_t p = 0; p < P; ++p)
                if (ptype[p] == t) of_type.push_back(patterns[p]);
            if (of_type.empty() || pred_disjoint(of_type.data(), (uint32_t)of_type.size(), k)) continue;
            for (uint32_t i = 0; i < P; ++i)  // (every pair only to name the first one)
                for (uint32_t j = i + 1; ptype[i] == t && j < P; ++j)
                    if (ptype[j] == t && kp_a_overlap(patterns[i], patterns[j], low))
                        return fail(KP_E_ARG, "kp_spec_begin: the patterns of type " + std::to_string(t) +
                                                  " are not a partition: patterns " + std::to_string(i) + " and " +
                                                  std::to_string(j) + " share k-mers");
        }
        s->k = k;
        s->fold = fold ? 1 : 0;
        s->cells = 1ull << (2 * k);
        s->st = kp_spec_stats{};
        s->st.tile = KP_S_TILE;
        s->st.lut_bytes = s->cells * 16;
        s->pats.assign(patterns, patterns + P);
        s->ptype.assign(ptype, ptype + P);
        s->by_type.clear();
        for (uint32_t t = 0; t < KP_SP_TYPES; ++t) {
            s->type_off[t] = (uint32_t)s->by_type.size();
            for (uint32_t p = 0; p < P; ++p)
                if (ptype[p] == t) s->by_type.push_back(p);
        }
        s->type_off[KP_SP_TYPES] = (uint32_t)s->by_type.size();  // = P: every type is below 12
        if (!c) {
            s->h_lut.assign(4 * s->cells, KP_P_NONE);
            for (uint64_t code = 0; code < s->cells; ++code)
                if (kp_p_reachable((uint32_t)code, k, s->fold))
                    kp_sp_find(kp_a_onehot(code, k), patterns, ptype, P, &s->h_lut[4 * code]);
        }
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_spec_begin: the host table of " + std::to_string(k) + "-mers does not fit memory");
    }
    if (c) {
        KP_HIP(hipSetDevice(c->device));
        s->lut_ok = false;
        int rc = spec_arena(c, "kp_spec_begin", 0);
        if (rc) return rc;
    }
    s->active = true;
    return KP_OK;
}

int kp_spec_regions(kp_ctx *c, const uint8_t *seq, uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end,
                    uint64_t n_regions, const double *rates, uint64_t *hist, uint64_t *other, double *expected) {
    kp_spec_sess *s = spec_sess(c);
    int rc = scan_check_contig("kp_spec_regions", s->active, seq, n, "kp_spec_begin");
    if (rc) return rc;
    if (n_regions >= (1ull << 32)) return fail(KP_E_ARG, "kp_spec_regions: 2^32 regions or more in one call");
    if (n_regions && (!reg_begin || !reg_end || !other)) return fail(KP_E_ARG, "kp_spec_regions: null regions or counters");
    if (rates && n_regions && !expected) return fail(KP_E_ARG, "kp_spec_regions: rates without a place for the sums");
    if ((rc = scan_check_regions("kp_spec_regions", n, reg_begin, reg_end, n_regions, false))) return rc;
    if (!n_regions) return KP_OK;
    const int k = s->k;
    const uint32_t P = (uint32_t)s->pats.size();
    const uint32_t mask = (uint32_t)(s->cells - 1);
    uint64_t lo = 0, hi = 0;
    scan_centres(n, k, &lo, &hi);
    if (!c) {
        std::vector<uint64_t> row;
        try {
            row.resize(P);
        } catch (const std::bad_alloc &) {
            return fail(KP_E_NOMEM, "kp_spec_regions: a row of counters does not fit memory");
        }
        uint64_t n_items = 0;
        for (uint64_t r = 0; r < n_regions; ++r) {
            std::fill(row.begin(), row.end(), 0);
            uint64_t none[3] = {0, 0, 0}, inv = 0;
            for (uint64_t p = reg_begin[r]; p < reg_end[r]; ++p) {
                uint32_t code = 0;
                if (!kp_p_window(seq, n, p, k, s->fold, mask, &code)) {
                    ++inv;
                    continue;
                }
                for (int e = 0; e < 3; ++e) {
                    const int32_t j = s->h_lut[4ull * code + e];
                    if (j >= 0)
                        ++row[j];
                    else
                        ++none[e];
                }
            }
            n_items += scan_pieces(reg_begin[r], reg_end[r], lo, hi);
            for (int e3 = 0; e3 < 3; ++e3) other[4 * r + e3] = none[e3];
            other[4 * r + 3] = inv;
            s->st.unmatched += none[0] + none[1] + none[2];
            s->st.invalid += inv;
            s->st.assigned += 3 * (reg_end[r] - reg_begin[r] - inv) - none[0] - none[1] - none[2];
            if (hist) memcpy(hist + r * P, row.data(), (size_t)P * 8);
            if (rates) {
                for (uint32_t t = 0; t < KP_SP_TYPES; ++t) {
                    double acc = 0.0;
                    for (uint32_t e = s->type_off[t]; e < s->type_off[t + 1]; ++e)
                        acc = acc + (double)row[s->by_type[e]] * rates[s->by_type[e]];
                    expected[KP_SP_TYPES * r + t] = acc;
                }
            }
        }
        s->st.items += n_items;
        return KP_OK;
    }

    KP_HIP(hipSetDevice(c->device));
    const long lds_p = env_int("KP_SPEC_LDS_P", KP_P_LDS_P);
    if (lds_p < 0 || lds_p > KP_P_LDS_P)
        return fail(KP_E_ARG, "kp_spec_regions: KP_SPEC_LDS_P must be 0..16384 (uint32 counters beside a second workgroup's)");
    const bool lds = env_int("KP_SPEC_GLOBAL", 0) == 0 && (long)P <= lds_p;
    std::vector<kp_p_item> items;
    std::vector<uint64_t> off_contig;  // per region: centres outside [lo, hi)
    try {
        off_contig.resize(n_regions);
        for (uint64_t r = 0; r < n_regions; ++r)
            off_contig[r] = reg_end[r] - reg_begin[r] - scan_cut(items, reg_begin[r], reg_end[r], lo, hi, (uint32_t)r);
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_spec_regions: the work items do not fit host memory");
    }
    if (items.size() >= (1ull << 32)) return fail(KP_E_ARG, "kp_spec_regions: 2^32 work items or more in one call");
    const size_t cnts = (size_t)n_regions * P;
    const size_t b_hist = g_up(cnts * 8), b_other = g_up(n_regions * 32);
    const size_t b_rates = rates ? g_up((size_t)P * 8) + g_up((size_t)P * 4) : 0;
    const size_t b_exp = rates ? g_up(n_regions * KP_SP_TYPES * 8) : 0;
    if ((rc = spec_arena(c, "kp_spec_regions", b_hist + b_other + b_rates + b_exp))) return rc;
    unsigned long long *d_hist = (unsigned long long *)c->arena.take(cnts * 8);
    unsigned long long *d_other = (unsigned long long *)c->arena.take(n_regions * 32);
    double *d_rates = rates ? (double *)c->arena.take((size_t)P * 8) : nullptr;
    uint32_t *d_type = rates ? (uint32_t *)c->arena.take((size_t)P * 4) : nullptr;
    double *d_exp = rates ? (double *)c->arena.take(n_regions * KP_SP_TYPES * 8) : nullptr;
    if ((rc = c->arena.check("kp_spec_regions"))) return rc;
    hipStream_t st = c->stream;
    KP_HIP(hipMemsetAsync(d_hist, 0, cnts * 8, st));
    KP_HIP(hipMemsetAsync(d_other, 0, n_regions * 32, st));
    if (!items.empty()) {
        uint8_t *d_seq = nullptr;
        kp_p_item *d_items = nullptr;
        if ((rc = scan_upload(c, "kp_spec_regions", seq, n, items, 0, &d_seq, &d_items))) return rc;
        const size_t lds_bytes = lds ? (size_t)P * 4 : 0;
        const uint64_t grid = scan_grid(c, items.size(), scan_per_cu(lds_bytes), "KP_SPEC_GRID");
        kp_sp_args A;
        A.seq = d_seq;
        A.items = d_items;
        A.n_items = (uint32_t)items.size();
        A.steps = (uint32_t)((items.size() + grid - 1) / grid);
        A.k = k;
        A.fold = s->fold;
        A.mask = mask;
        A.P = P;
        A.lut = (const int4 *)s->d_lut;
        A.hist = d_hist;
        A.other = d_other;
        if ((rc = scan_mark(c, 0))) return rc;
        if (lds)
            hipLaunchKernelGGL((kp_spec_scan_kernel<true>), dim3((unsigned)grid), dim3(KP_S_THREADS), lds_bytes, st, A);
        else
            hipLaunchKernelGGL((kp_spec_scan_kernel<false>), dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
        if ((rc = scan_launched(c, 1))) return rc;
    }
    if (rates) {
        KP_HIP(hipMemcpyAsync(d_rates, rates, (size_t)P * 8, hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(d_type, s->by_type.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
        kp_sp_offs T;
        memcpy(T.off, s->type_off, sizeof T.off);
        hipLaunchKernelGGL(kp_spec_sums_kernel, dim3((unsigned)((n_regions * KP_SP_TYPES + 63) / 64)), dim3(64), 0, st, d_hist,
                           d_rates, d_type, T, P, n_regions, d_exp);
        KP_HIP(hipGetLastError());
        KP_HIP(hipMemcpyAsync(expected, d_exp, n_regions * KP_SP_TYPES * 8, hipMemcpyDeviceToHost, st));
    }
    if (hist) KP_HIP(hipMemcpyAsync(hist, d_hist, cnts * 8, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(other, d_other, n_regions * 32, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    if (!items.empty()) {
        float ms = 0.f;
        if ((rc = scan_elapsed(c, 0, 1, &ms))) return rc;
        s->st.scan_ms += ms;
        s->st.path = lds ? 1u : 2u;
    }
    for (uint64_t r = 0; r < n_regions; ++r) {
        uint64_t *o = other + 4 * r;
        o[3] += off_contig[r];
        s->st.unmatched += o[0] + o[1] + o[2];
        s->st.invalid += o[3];
        s->st.assigned += 3 * (reg_end[r] - reg_begin[r] - o[3]) - o[0] - o[1] - o[2];
    }
    s->st.items += items.size();
    return KP_OK;
}

int kp_spec_track(kp_ctx *c, const uint8_t *seq, uint64_t n, uint64_t begin, uint64_t end, int32_t *pid) {
    kp_spec_sess *s = spec_sess(c);
    int rc = scan_check_contig("kp_spec_track", s->active, seq, n, "kp_spec_begin");
    if (rc) return rc;
    if (begin > end || end > n) return fail(KP_E_ARG, "kp_spec_track: begin > end or a range outside the contig");
    const uint64_t len = end - begin;
    if (!len) return KP_OK;
    if (!pid) return fail(KP_E_ARG, "kp_spec_track: null output");
    const int k = s->k;
    const uint32_t mask = (uint32_t)(s->cells - 1);
    const uint64_t n_items = scan_tiles(len);
    if (!c) {
        for (uint64_t i = 0; i < len; ++i) {
            uint32_t code = 0;
            const bool ok = kp_p_window(seq, n, begin + i, k, s->fold, mask, &code);
            for (int e = 0; e < 3; ++e) pid[e * len + i] = ok ? s->h_lut[4ull * code + e] : KP_P_INVALID;
        }
        s->st.items += n_items;
        return KP_OK;
    }
    KP_HIP(hipSetDevice(c->device));
    const size_t plane = g_up(len * 4);  // bytes between two planes on the device
    if ((rc = spec_arena(c, "kp_spec_track", 3 * plane))) return rc;
    int32_t *d_pid = (int32_t *)c->arena.take(3 * plane);
    if ((rc = c->arena.check("kp_spec_track"))) return rc;
    uint8_t *d_seq = nullptr;
    if ((rc = scan_upload(c, "kp_spec_track", seq, n, {}, 0, &d_seq, nullptr))) return rc;
    hipStream_t st = c->stream;
    const uint64_t grid = scan_grid(c, n_items, 4, "KP_SPEC_GRID");  // 33 KB of LDS per workgroup
    uint64_t lo = 0, hi = 0;
    scan_centres(n, k, &lo, &hi);
    kp_sp_targs A;
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
    A.lut = (const int4 *)s->d_lut;
    A.pid = d_pid;
    A.plane = plane / 4;
    if ((rc = scan_mark(c, 0))) return rc;
    hipLaunchKernelGGL(kp_spec_track_kernel, dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
    if ((rc = scan_launched(c, 1))) return rc;
    for (int e = 0; e < 3; ++e)
        KP_HIP(hipMemcpyAsync(pid + e * len, d_pid + e * (plane / 4), len * 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    if ((rc = scan_elapsed(c, 0, 1, &ms))) return rc;
    s->st.scan_ms += ms;
    s->st.items += n_items;
    return KP_OK;
}

int kp_spec_sites(kp_ctx *c, const uint8_t *seq, uint64_t n, const uint64_t *pos, const uint8_t *alt, uint64_t n_sites,
                  int32_t *pid) {
    kp_spec_sess *s = spec_sess(c);
    int rc = scan_check_contig("kp_spec_sites", s->active, seq, n, "kp_spec_begin");
    if (rc) return rc;
    if ((rc = spec_check_sites("kp_spec_sites", n, pos, alt, n_sites))) return rc;
    if (!n_sites) return KP_OK;
    if (!pid) return fail(KP_E_ARG, "kp_spec_sites: null output");
    const int k = s->k;
    const uint32_t mask = (uint32_t)(s->cells - 1);
    if (!c) {
        for (uint64_t i = 0; i < n_sites; ++i) {
            uint32_t code = 0, slot = 0;
            const int r = kp_sp_site(seq, n, pos[i], alt[i], k, s->fold, mask, &code, &slot);
            pid[i] = r ? r : s->h_lut[4ull * code + slot];
        }
        return KP_OK;
    }
    KP_HIP(hipSetDevice(c->device));
    if ((rc = spec_arena(c, "kp_spec_sites", g_up(n_sites * 4)))) return rc;
    int32_t *d_pid = (int32_t *)c->arena.take(n_sites * 4);
    if ((rc = c->arena.check("kp_spec_sites"))) return rc;
    uint8_t *d_seq = nullptr;
    if ((rc = scan_upload(c, "kp_spec_sites", seq, n, {}, g_up(n_sites * 8) + g_up(n_sites), &d_seq, nullptr)))
        return rc;
    uint64_t *d_pos = (uint64_t *)c->seq_in.take(n_sites * 8);
    uint8_t *d_alt = (uint8_t *)c->seq_in.take(n_sites);
    if ((rc = c->seq_in.check("kp_spec_sites"))) return rc;
    hipStream_t st = c->stream;
    KP_HIP(hipMemcpyAsync(d_pos, pos, n_sites * 8, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_alt, alt, n_sites, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kp_spec_sites_kernel, dim3((unsigned)((n_sites + 255) / 256)), dim3(256), 0, st, d_seq, n, d_pos, d_alt,
                       n_sites, k, s->fold, mask, s->d_lut, d_pid);
    KP_HIP(hipGetLastError());
    KP_HIP(hipMemcpyAsync(pid, d_pid, n_sites * 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    return KP_OK;
}

int kp_spec_end(kp_ctx *c) {
    kp_spec_sess *s = spec_sess(c);
    if (!s->active) return fail(KP_E_STATE, "kp_spec_end: no session (kp_spec_begin first)");
    s->active = false;
    s->lut_ok = false;
    std::vector<int32_t>().swap(s->h_lut);
    std::vector<uint64_t>().swap(s->pats);
    std::vector<uint32_t>().swap(s->ptype);
    std::vector<uint32_t>().swap(s->by_type);
    return KP_OK;
}

int kp_spec_last_stats(kp_ctx *c, kp_spec_stats *out) {
    if (!out) return fail(KP_E_ARG, "kp_spec_last_stats: null out");
    *out = spec_sess(c)->st;
    return KP_OK;
}

int kp_spec_host(int k, int fold, const uint64_t *patterns, const uint32_t *ptype, uint32_t n_patterns, const uint8_t *seq,
                 uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end, uint64_t n_regions, const double *rates,
                 uint64_t *hist, uint64_t *other, double *expected, uint64_t track_begin, uint64_t track_end,
                 int32_t *track_pid, const uint64_t *pos, const uint8_t *alt, uint64_t n_sites, int32_t *site_pid,
                 kp_spec_stats *stats) {
    int rc = kp_spec_begin(nullptr, k, fold, patterns, ptype, n_patterns);
    if (rc) return rc;
    rc = kp_spec_regions(nullptr, seq, n, reg_begin, reg_end, n_regions, rates, hist, other, expected);
    if (!rc && track_pid) rc = kp_spec_track(nullptr, seq, n, track_begin, track_end, track_pid);
    if (!rc) rc = kp_spec_sites(nullptr, seq, n, pos, alt, n_sites, site_pid);
    const std::string err = g_err;
    const int rc_end = kp_spec_end(nullptr);
    if (rc) return fail(rc, err);
    if (stats) *stats = g_spec_host.st;
    return rc_end;
}

// typed counting (the kp_seq session with three positive columns, kp_seq.h)
int kp_seq_sites_typed(kp_ctx *c, const uint8_t *seq, uint64_t n, const uint64_t *pos, const uint8_t *alt,
                       uint64_t n_sites) {
    kp_seq_sess *s = seq_sess(c);
    int rc = scan_check_contig("kp_seq_sites_typed", s->active, seq, n, "kp_seq_begin");
    if (rc) return rc;
    if (s->indel) return fail(KP_E_STATE, "kp_seq_sites_typed: the session is an indel session (kp_seq_indels)");
    if (s->pcols != 3) return fail(KP_E_STATE, "kp_seq_sites_typed: the session is not typed (kp_seq_begin_typed)");
    if ((rc = spec_check_sites("kp_seq_sites_typed", n, pos, alt, n_sites))) return rc;
    if (!n_sites) return KP_OK;
    const int k = s->k;
    if (!c) {
        for (uint64_t i = 0; i < n_sites; ++i) {
            uint32_t code = 0, slot = 0;
            const bool ok = kp_sp_site(seq, n, pos[i], alt[i], k, s->fold, (uint32_t)(s->cells - 1), &code, &slot) == 0;
            if (ok) ++s->h_tab[(uint64_t)slot * s->cells + code];
            ++(ok ? s->st.sites : s->st.sites_skipped);
        }
        return KP_OK;
    }
    KP_HIP(hipSetDevice(c->device));
    const size_t b_seq = g_up(n + KP_S_PAD), b_pos = g_up(n_sites * 8), b_alt = g_up(n_sites);
    if ((rc = c->seq_in.reserve("kp_seq_sites_typed", b_seq + b_pos + b_alt))) return rc;
    uint8_t *d_seq = (uint8_t *)c->seq_in.take(b_seq);
    uint64_t *d_pos = (uint64_t *)c->seq_in.take(b_pos);
    uint8_t *d_alt = (uint8_t *)c->seq_in.take(b_alt);
    if ((rc = c->seq_in.check("kp_seq_sites_typed"))) return rc;
    hipStream_t st = c->stream;
    KP_HIP(hipMemcpyAsync(d_seq, seq, n, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_pos, pos, n_sites * 8, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_alt, alt, n_sites, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kp_seq_sites_typed_kernel, dim3((unsigned)((n_sites + 255) / 256)), dim3(256), 0, st, d_seq, n, d_pos,
                       d_alt, n_sites, k, s->fold, (uint32_t)s->cells, s->d_tab, s->d_stat);
    KP_HIP(hipGetLastError());
    unsigned long long h_stat[3] = {0, 0, 0};
    KP_HIP(hipMemcpyAsync(h_stat, s->d_stat, sizeof h_stat, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    s->st.sites = h_stat[1];
    s->st.sites_skipped = h_stat[2];
    return KP_OK;
}

}  // extern "C"
