// kp_ispec.h -- an insertion and a deletion partition taken back to the genome on both strands (no
// reference counterpart).  Included by kp_hip.hip after kp_spec.h and kp_indel.h.  Semantics:
// include/kmerpapa_hip.h.
//
// A breakpoint b of a contig has the window W(b) = seq[b - k/2, b + k/2), k even.  The partitions
// were fitted on both-strand tables (kp_seq_begin_indel with both), which are not rc-symmetric as
// partitions: the rate of an event at b needs the pattern of W(b) and that of rc(W(b)).  One pattern
// list holds both kinds (pkind[p] = 0 ins, 1 del), and one table of 16-byte entries {ins pattern of
// c, ins pattern of rc(c), del pattern of c, del pattern of rc(c)} per code c answers all four with
// one gather: the reverse complement is resolved when the table is built, the scan needs only the
// forward code.  Windows and validity are kp_seq.h's, matching is kp_apply.h's, the scan's skeleton
// on device and host is kp_scan.h's, a site's interval, placement and windows are kp_indel.h's
// (kp_i_left / kp_i_right / kp_i_place / kp_i_window).  Counts are integers and `expected` is a
// float64 sum in pattern order, so a device session equals the host session bit for bit.
//
//   kp_ispec_lut_kernel    one k-mer code per thread: its one-hot word and its reverse complement's
//                          against every pattern, staged through LDS in tiles with their kinds (as
//                          kp_spec_lut_kernel): four first matches
//   kp_ispec_scan_kernel   kp_spec_scan_kernel's grid, roll and batches with fold = 0; a valid window
//                          does one 16-byte gather and up to four adds -- into the item's 2 P uint32
//                          LDS counters (strand-major, flushed to the region's rows after it) or with
//                          global 64-bit atomics.  other[region][5] gets one atomic per wave, item and
//                          counter
//   kp_ispec_track_kernel  kp_spec_track_kernel with four planes
//   kp_ispec_sites_kernel  kp_seq_indels_kernel's wave-cooperative interval search (the loop is
//                          copied, so that kernel keeps its registers); then every lane places its
//                          own site, builds its one or two windows and reads two table entries.  No
//                          atomics on tables
//   kp_ispec_sums_kernel   one thread per (region, kind, strand): expected, over the kind's patterns
//                          in order
//
// Every device loop has a bound the host computed; there are no waits between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "kp_apply.h"
#include "kp_indel.h"
#include "kp_pred.h"
#include "kp_rt.h"
#include "kp_scan.h"
#include "kp_seq.h"

#define KP_IS_LDS_P (KP_P_LDS_P / 2)  // most patterns with LDS counters: 2 P uint32 in the spectrum scan's 64 KiB
#define KP_IS_INS 0
#define KP_IS_DEL 1

// the code of a k-mer's reverse complement
__host__ __device__ inline uint32_t kp_is_rc(uint32_t code, int k) {
    uint32_t r = 0;
    for (int i = 0; i < k; ++i) r = (r << 2) | (3u - ((code >> (2 * i)) & 3u));
    return r;
}

// the entry of a code: the first pattern of each kind its one-hot word and its reverse complement's match
__host__ __device__ inline void kp_is_find(uint64_t oh, uint64_t ohr, const uint64_t *pats, const uint32_t *pkind,
                                           uint32_t P, int32_t out[4]) {
    int32_t f[4] = {KP_P_NONE, KP_P_NONE, KP_P_NONE, KP_P_NONE};
    for (uint32_t j = 0; j < P && (f[0] < 0 || f[1] < 0 || f[2] < 0 || f[3] < 0); ++j) {
        const uint32_t t = 2u * pkind[j];
        if (f[t] < 0 && kp_a_match(oh, pats[j])) f[t] = (int32_t)j;
        if (f[t + 1] < 0 && kp_a_match(ohr, pats[j])) f[t + 1] = (int32_t)j;
    }
    out[0] = f[0], out[1] = f[1], out[2] = f[2], out[3] = f[3];
}

// The two patterns of a site placed at p: an insertion's are the ins patterns of W(p) and rc(W(p)); a
// deletion's are the del pattern of W(p), its start, and of rc(W(p + L)), its end read on the other
// strand.  Both KP_P_INVALID where kp_i_cells would skip the site whole.  lut = the table as int32 [4^k][4]
__host__ __device__ inline void kp_is_site(const uint8_t *seq, uint64_t n, uint32_t p, uint32_t L, bool del, int k,
                                           uint32_t mask, const int32_t *lut, int32_t out[2]) {
    kp_s_win w{0u, 0u, 0u}, e{0u, 0u, 0u};
    out[0] = out[1] = KP_P_INVALID;
    if (!kp_i_window(seq, n, p, k, mask, w)) return;
    if (!del) {
        out[0] = lut[4ull * w.fwd];
        out[1] = lut[4ull * w.fwd + 1];
        return;
    }
    if (!kp_i_window(seq, n, (uint64_t)p + L, k, mask, e)) return;
    out[0] = lut[4ull * w.fwd + 2];
    out[1] = lut[4ull * e.fwd + 3];
}

struct kp_is_args {
    const uint8_t *seq;      // the contig, KP_S_PAD readable bytes past its end
    const kp_p_item *items;  // [n_items]
    uint32_t n_items, steps;
    int32_t k;
    uint32_t mask;  // 4^k - 1
    uint32_t P;
    const int4 *lut;            // [4^k]
    unsigned long long *hist;   // [n_regions][2][P]
    unsigned long long *other;  // [n_regions][5]: no ins pattern fwd, rc; no del pattern fwd, rc; invalid
};

struct kp_is_offs {
    uint32_t off[3];  // by_kind[off[t] .. off[t + 1]) are the patterns of kind t, ascending
};

struct kp_is_targs {
    const uint8_t *seq;
    uint32_t begin, len;  // breakpoints [begin, begin + len)
    uint32_t lo, hi;      // breakpoints whose window lies inside the contig
    uint32_t n_items, steps;
    int32_t k;
    uint32_t mask;
    const int4 *lut;
    int32_t *pid;    // [4][plane], 256-byte aligned
    uint64_t plane;  // int32 between two planes, a multiple of 64
};

struct kp_is_sargs {
    const uint8_t *seq;  // the contig
    uint64_t n;
    const uint64_t *pos, *del_len, *key, *ins_off;  // as kp_i_args'
    const uint8_t *ins;
    uint64_t n_sites;
    uint32_t max_steps;  // n / 64 + 1
    int32_t k, place;
    uint32_t contig;
    uint64_t seed;
    uint32_t mask;
    const int32_t *lut;        // [4^k][4]
    unsigned long long *stat;  // [0] += sites kept, [1] += sites skipped
    uint64_t *resolved;        // [n_sites][3] lo, hi, chosen; or NULL
    int32_t *pid;              // [n_sites][2]
};

#ifdef __HIPCC__

__global__ void __launch_bounds__(256) kp_ispec_lut_kernel(const uint64_t *__restrict__ pats,
                                                           const uint32_t *__restrict__ pkind, uint32_t P, int k,
                                                           uint32_t cells, int4 *__restrict__ lut) {
    __shared__ unsigned long long sT[KP_P_LUT_TILE];
    __shared__ uint32_t sK[KP_P_LUT_TILE];  // the kind of each staged pattern
    const uint32_t tid = threadIdx.x;
    const uint32_t code = blockIdx.x * 256u + tid;
    const bool act = code < cells;
    const uint64_t oh = act ? kp_a_onehot(code, k) : 0, ohr = act ? kp_a_onehot(kp_is_rc(code, k), k) : 0;
    int32_t f0 = KP_P_NONE, f1 = KP_P_NONE, f2 = KP_P_NONE, f3 = KP_P_NONE;
    for (uint32_t t0 = 0; t0 < P; t0 += KP_P_LUT_TILE) {
        const uint32_t nt = P - t0 < KP_P_LUT_TILE ? P - t0 : KP_P_LUT_TILE;
        __syncthreads();  // the previous tile has been read by every wave
        for (uint32_t e = tid; e < nt; e += 256u) {
            sT[e] = pats[t0 + e];
            sK[e] = pkind[t0 + e];
        }
        __syncthreads();
        if (act && (f0 < 0 || f1 < 0 || f2 < 0 || f3 < 0)) {
#pragma unroll 4
            for (uint32_t j = 0; j < nt; ++j) {
                const unsigned long long pt = sT[j];
                const bool m = kp_a_match(oh, pt), mr = kp_a_match(ohr, pt);
                const bool del = sK[j] != 0u;
                const int32_t id = (int32_t)(t0 + j);
                f0 = (m && !del && f0 < 0) ? id : f0;
                f1 = (mr && !del && f1 < 0) ? id : f1;
                f2 = (m && del && f2 < 0) ? id : f2;
                f3 = (mr && del && f3 < 0) ? id : f3;
            }
        }
    }
    if (act) lut[code] = make_int4(f0, f1, f2, f3);
}

template <bool LDS>
__global__ void __launch_bounds__(KP_S_THREADS) kp_ispec_scan_kernel(kp_is_args A) {
    extern __shared__ uint32_t kp_is_cnt[];  // [2][P] with LDS
    const uint32_t tid = threadIdx.x;
    const uint32_t P = A.P, P2 = 2u * A.P;
    if (LDS) {
        for (uint32_t e = tid; e < P2; e += KP_S_THREADS) kp_is_cnt[e] = 0;
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
        unsigned long long *row = A.hist + (uint64_t)it.region * P2;
        uint32_t none0 = 0, none1 = 0, none2 = 0, none3 = 0, inv = 0;
        kp_s_win w{0u, 0u, 0u};
#pragma unroll
        for (uint32_t jb = 0; jb < 64; jb += KP_P_BATCH) {
            uint32_t code[KP_P_BATCH];
            bool has[KP_P_BATCH];
            int4 p[KP_P_BATCH];
            kp_scan_batch(w, d, jb, off, end, full0, k, 0, A.mask, top, code, has, inv);
#pragma unroll
            for (uint32_t q = 0; q < KP_P_BATCH; ++q)  // (code <= mask: the entry lies inside the table)
                p[q] = has[q] ? A.lut[code[q]] : make_int4(KP_P_INVALID, KP_P_INVALID, KP_P_INVALID, KP_P_INVALID);
#pragma unroll
            for (uint32_t q = 0; q < KP_P_BATCH; ++q) {
                const int32_t id[4] = {p[q].x, p[q].y, p[q].z, p[q].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (id[e] >= 0) {  // (< P: the table holds indices of the pattern list only)
                        const uint32_t cell = (e & 1 ? P : 0u) + (uint32_t)id[e];  // < 2 P
                        if (LDS)
                            atomicAdd(&kp_is_cnt[cell], 1u);
                        else
                            atomicAdd(&row[cell], 1ull);
                    }
                }
                none0 += p[q].x == KP_P_NONE;
                none1 += p[q].y == KP_P_NONE;
                none2 += p[q].z == KP_P_NONE;
                none3 += p[q].w == KP_P_NONE;
            }
        }
        for (int o = 32; o; o >>= 1) {
            none0 += __shfl_xor(none0, o, 64);
            none1 += __shfl_xor(none1, o, 64);
            none2 += __shfl_xor(none2, o, 64);
            none3 += __shfl_xor(none3, o, 64);
            inv += __shfl_xor(inv, o, 64);
        }
        if ((tid & 63u) == 0) {
            unsigned long long *o = A.other + 5ull * it.region;
            if (none0) atomicAdd(&o[0], (unsigned long long)none0);
            if (none1) atomicAdd(&o[1], (unsigned long long)none1);
            if (none2) atomicAdd(&o[2], (unsigned long long)none2);
            if (none3) atomicAdd(&o[3], (unsigned long long)none3);
            if (inv) atomicAdd(&o[4], (unsigned long long)inv);
        }
        if (LDS) {
            __syncthreads();  // every add of the item is in
            for (uint32_t e = tid; e < P2; e += KP_S_THREADS) {
                const uint32_t v = kp_is_cnt[e];
                if (v) {
                    atomicAdd(&row[e], (unsigned long long)v);
                    kp_is_cnt[e] = 0;
                }
            }
            __syncthreads();  // zero again before the next item adds
        }
    }
}

__global__ void __launch_bounds__(KP_S_THREADS) kp_ispec_track_kernel(kp_is_targs A) {
    __shared__ int32_t buf[KP_S_RUN * KP_P_ROW];  // [slot of the run][thread]
    const uint32_t tid = threadIdx.x;
    const int k = A.k, top = 2 * (A.k - 1), h = A.k / 2;
    for (uint32_t s = 0; s < A.steps; ++s) {
        const uint32_t item = s * gridDim.x + blockIdx.x;
        if (item >= A.n_items) break;  // (the same for the whole workgroup)
        const uint64_t base = (uint64_t)item * KP_S_TILE;  // of the item in a plane
        const uint64_t i0 = base + tid * KP_S_RUN;
        const uint32_t cnt = i0 >= A.len ? 0u : (A.len - i0 < KP_S_RUN ? (uint32_t)(A.len - i0) : (uint32_t)KP_S_RUN);
        // this thread's breakpoints [c0, c0 + cnt), of which [cb, cb + nc) have a window inside the contig
        const uint64_t c0 = (uint64_t)A.begin + i0;
        const uint64_t cb = c0 > A.lo ? c0 : (uint64_t)A.lo, ce = c0 + cnt < A.hi ? c0 + cnt : (uint64_t)A.hi;
        const uint32_t nc = ce > cb ? (uint32_t)(ce - cb) : 0u;
        uint32_t d[16], off, end;
        kp_p_load(A.seq, nc ? cb - (uint32_t)h : 0u, nc ? nc + (uint32_t)k - 1u : 0u, d, &off, &end);
        const uint32_t full0 = off + (uint32_t)k - 1u;
        const uint32_t slot0 = nc ? (uint32_t)(cb - c0) : 0u;  // of the first window: byte j fills slot0 + j - full0
        for (int plane = 0; plane < 4; ++plane) {
#pragma unroll
            for (uint32_t q = 0; q < KP_S_RUN; ++q) buf[q * KP_P_ROW + tid] = KP_P_INVALID;
            uint32_t inv = 0;  // (not reported: the slots of invalid windows keep their -2)
            kp_s_win w{0u, 0u, 0u};
#pragma unroll
            for (uint32_t jb = 0; jb < 64; jb += KP_P_BATCH) {
                uint32_t code[KP_P_BATCH];
                bool has[KP_P_BATCH];
                int4 p[KP_P_BATCH];
                kp_scan_batch(w, d, jb, off, end, full0, k, 0, A.mask, top, code, has, inv);
#pragma unroll
                for (uint32_t q = 0; q < KP_P_BATCH; ++q) p[q] = has[q] ? A.lut[code[q]] : make_int4(0, 0, 0, 0);
#pragma unroll
                for (uint32_t q = 0; q < KP_P_BATCH; ++q)  // slot0 + j - full0 < slot0 + nc <= KP_S_RUN
                    if (has[q])
                        buf[(slot0 + jb + q - full0) * KP_P_ROW + tid] =
                            plane == 0 ? p[q].x : (plane == 1 ? p[q].y : (plane == 2 ? p[q].z : p[q].w));
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

__global__ void __launch_bounds__(256) kp_ispec_sites_kernel(kp_is_sargs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    const bool act = i < A.n_sites;
    uint32_t b = 0, L = 1, off = 0;
    int del = 0;
    if (act) {
        const uint64_t dl = A.del_len[i], o = A.ins_off[i];
        b = (uint32_t)A.pos[i];
        del = dl != 0;
        off = (uint32_t)o;
        L = del ? (uint32_t)dl : (uint32_t)(A.ins_off[i + 1] - o);
    }
    // the wave's sites one after the other (its active lanes are lanes 0 .. n_live - 1), as in
    // kp_seq_indels_kernel
    const int n_live = __popcll(__ballot(act));
    uint32_t my_a = 0, my_c = 0;
    for (int j = 0; j < n_live; ++j) {
        const uint32_t jb = (uint32_t)__shfl((int)b, j, 64), jL = (uint32_t)__shfl((int)L, j, 64);
        const bool jdel = __shfl(del, j, 64) != 0;
        const uint8_t *jins = A.ins + (uint32_t)__shfl((int)off, j, 64);
        uint32_t a = 0, c = 0;
        bool more_a = true, more_c = true;
        for (uint32_t s = 0; s < A.max_steps && (more_a || more_c); ++s) {
            const uint32_t t = s * 64u + lane;
            const bool ml = more_a && kp_i_left(A.seq, jins, jb, jL, jdel, t);
            const bool mr = more_c && kp_i_right(A.seq, A.n, jins, jb, jL, jdel, t);
            const unsigned long long miss_l = ~__ballot(ml), miss_r = ~__ballot(mr);
            if (more_a && miss_l) a = s * 64u + (uint32_t)(__ffsll((long long)miss_l) - 1), more_a = false;
            if (more_c && miss_r) c = s * 64u + (uint32_t)(__ffsll((long long)miss_r) - 1), more_c = false;
        }
        if ((int)lane == j) my_a = a, my_c = c;
    }
    bool ok = false;
    if (act) {
        const uint32_t lo = b - my_a, hi = b + my_c;
        const uint32_t p = kp_i_place(lo, hi, A.place, A.seed, A.contig, A.key ? A.key[i] : i);
        int32_t id[2];
        kp_is_site(A.seq, A.n, p, L, del != 0, A.k, A.mask, A.lut, id);
        A.pid[2 * i] = id[0];
        A.pid[2 * i + 1] = id[1];
        ok = id[0] != KP_P_INVALID;
        if (A.resolved) {
            A.resolved[3 * i] = lo;
            A.resolved[3 * i + 1] = hi;
            A.resolved[3 * i + 2] = p;
        }
    }
    const unsigned long long kept = __popcll(__ballot(ok)), skipped = __popcll(__ballot(act && !ok));
    if (lane == 0) {  // one atomic per wave and counter
        if (kept) atomicAdd(&A.stat[0], kept);
        if (skipped) atomicAdd(&A.stat[1], skipped);
    }
}

__global__ void __launch_bounds__(64) kp_ispec_sums_kernel(const unsigned long long *__restrict__ hist,
                                                           const double *__restrict__ rates,
                                                           const uint32_t *__restrict__ by_kind, kp_is_offs T, uint32_t P,
                                                           uint64_t n_regions, double *__restrict__ expected) {
    const uint64_t i = blockIdx.x * 64ull + threadIdx.x;
    if (i >= n_regions * 4) return;
    const uint64_t r = i >> 2;
    const uint32_t kind = (uint32_t)(i >> 1) & 1u, strand = (uint32_t)i & 1u;
    const unsigned long long *row = hist + (2 * r + strand) * P;
    double acc = 0.0;
    for (uint32_t e = T.off[kind]; e < T.off[kind + 1]; ++e) {  // (off[2] = P: e indexes by_kind[P])
        const uint32_t p = by_kind[e];
        acc = acc + (double)row[p] * rates[p];
    }
    expected[i] = acc;
}

#endif  // __HIPCC__

// ---------------------------------------------------------------------------
// sessions: the context's (device) or this thread's (host, ctx = NULL)
// ---------------------------------------------------------------------------

static thread_local kp_ispec_sess g_ispec_host;

static kp_ispec_sess *ispec_sess(kp_ctx *c) { return c ? &c->ispec : &g_ispec_host; }

// scan_arena for the table of 16-byte entries: the table first, then `extra` bytes the caller takes
static int ispec_arena(kp_ctx *c, const char *who, size_t extra) {
    kp_ispec_sess *s = &c->ispec;
    const uint32_t P = (uint32_t)s->pats.size();
    return scan_arena(c, s, who, "indel model", 16, g_up((size_t)P * 8) + g_up((size_t)P * 4), extra, [&]() -> int {
        uint64_t *d_pats = (uint64_t *)c->arena.take((size_t)P * 8);
        uint32_t *d_kind = (uint32_t *)c->arena.take((size_t)P * 4);
        int rc = c->arena.check(who);
        if (rc) return rc;
        KP_HIP(hipMemcpyAsync(d_pats, s->pats.data(), (size_t)P * 8, hipMemcpyHostToDevice, c->stream));
        KP_HIP(hipMemcpyAsync(d_kind, s->pkind.data(), (size_t)P * 4, hipMemcpyHostToDevice, c->stream));
        if ((rc = scan_mark(c, 0))) return rc;
        hipLaunchKernelGGL(kp_ispec_lut_kernel, dim3((unsigned)((s->cells + 255) / 256)), dim3(256), 0, c->stream, d_pats,
                           d_kind, P, s->k, (uint32_t)s->cells, (int4 *)s->d_lut);
        return scan_launched(c, 1);
    });
}

extern "C" {

int kp_ispec_begin(kp_ctx *c, int k, const uint64_t *patterns, const uint32_t *pkind, uint32_t n_patterns) {
    kp_ispec_sess *s = ispec_sess(c);
    if (s->active) return fail(KP_E_STATE, "kp_ispec_begin: a session is open (kp_ispec_end first)");
    if (c && c->seq.active)
        return fail(KP_E_STATE, "kp_ispec_begin: a kp_seq session holds the context's arena (kp_seq_end first)");
    if (c && c->pred.active)
        return fail(KP_E_STATE, "kp_ispec_begin: a kp_pred session holds the context's arena (kp_pred_end first)");
    if (c && c->spec.active)
        return fail(KP_E_STATE, "kp_ispec_begin: a kp_spec session holds the context's arena (kp_spec_end first)");
    if (k < 2 || k > 14 || k % 2)
        return fail(KP_E_ARG, "kp_ispec_begin: k = " + std::to_string(k) +
                                  " must be even and 2..14 (the window of a breakpoint has k/2 bases on each side)");
    const uint32_t P = n_patterns;
    if (P == 0) return fail(KP_E_ARG, "kp_ispec_begin: no patterns (n_patterns = 0)");
    if (!patterns || !pkind) return fail(KP_E_ARG, "kp_ispec_begin: null patterns or kinds");
    if (P >= (1u << 30)) return fail(KP_E_ARG, "kp_ispec_begin: 2^30 patterns or more");
    for (uint32_t p = 0; p < P; ++p) {
        if (!apply_word_ok(patterns[p], k))
            return fail(KP_E_ARG, "kp_ispec_begin: pattern " + std::to_string(p) + " has an empty position or bits above position k");
        if (pkind[p] > 1u)
            return fail(KP_E_ARG, "kp_ispec_begin: pattern " + std::to_string(p) + " has kind " + std::to_string(pkind[p]) +
                                      ", not 0 (ins) or 1 (del)");
    }
    const uint64_t low = kp_a_low(k);
    try {
        std::vector<uint64_t> of_kind;
        for (uint32_t t = 0; t < 2; ++t) {
            of_kind.clear();
            for (uint32_t p = 0; p < P; ++p)
                if (pkind[p] == t) of_kind.push_back(patterns[p]);
            if (of_kind.empty() || pred_disjoint(of_kind.data(), (uint32_t)of_kind.size(), k)) continue;
            for (uint32_t i = 0; i < P; ++i)  // (every pair only to name the first one)
                for (uint32_t j = i + 1; pkind[i] == t && j < P; ++j)
                    if (pkind[j] == t && kp_a_overlap(patterns[i], patterns[j], low))
                        return fail(KP_E_ARG, std::string("kp_ispec_begin: the ") + (t ? "del" : "ins") +
                                                  " patterns are not a partition: patterns " + std::to_string(i) + " and " +
                                                  std::to_string(j) + " share k-mers");
        }
        s->k = k;
        s->cells = 1ull << (2 * k);
        s->st = kp_ispec_stats{};
        s->st.tile = KP_S_TILE;
        s->st.lut_bytes = s->cells * 16;
        s->pats.assign(patterns, patterns + P);
        s->pkind.assign(pkind, pkind + P);
        s->by_kind.clear();
        for (uint32_t t = 0; t < 2; ++t) {
            s->kind_off[t] = (uint32_t)s->by_kind.size();
            for (uint32_t p = 0; p < P; ++p)
                if (pkind[p] == t) s->by_kind.push_back(p);
        }
        s->kind_off[2] = (uint32_t)s->by_kind.size();  // = P: every kind is 0 or 1
        if (!c) {
            s->h_lut.assign(4 * s->cells, KP_P_NONE);
            for (uint64_t code = 0; code < s->cells; ++code)
                kp_is_find(kp_a_onehot(code, k), kp_a_onehot(kp_is_rc((uint32_t)code, k), k), patterns, pkind, P,
                           &s->h_lut[4 * code]);
        }
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_ispec_begin: the host table of " + std::to_string(k) + "-mers does not fit memory");
    }
    if (c) {
        KP_HIP(hipSetDevice(c->device));
        s->lut_ok = false;
        int rc = ispec_arena(c, "kp_ispec_begin", 0);
        if (rc) return rc;
    }
    s->active = true;
    return KP_OK;
}

int kp_ispec_regions(kp_ctx *c, const uint8_t *seq, uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end,
                     uint64_t n_regions, const double *rates, uint64_t *hist, uint64_t *other, double *expected) {
    kp_ispec_sess *s = ispec_sess(c);
    int rc = scan_check_contig("kp_ispec_regions", s->active, seq, n, "kp_ispec_begin");
    if (rc) return rc;
    if (n_regions >= (1ull << 32)) return fail(KP_E_ARG, "kp_ispec_regions: 2^32 regions or more in one call");
    if (n_regions && (!reg_begin || !reg_end || !other)) return fail(KP_E_ARG, "kp_ispec_regions: null regions or counters");
    if (rates && n_regions && !expected) return fail(KP_E_ARG, "kp_ispec_regions: rates without a place for the sums");
    if ((rc = scan_check_regions("kp_ispec_regions", n, reg_begin, reg_end, n_regions, false))) return rc;
    if (!n_regions) return KP_OK;
    const int k = s->k;
    const uint32_t P = (uint32_t)s->pats.size();
    const uint32_t mask = (uint32_t)(s->cells - 1);
    uint64_t lo = 0, hi = 0;
    scan_centres(n, k, &lo, &hi);
    if (!c) {
        std::vector<uint64_t> row;
        try {
            row.resize(2 * (size_t)P);
        } catch (const std::bad_alloc &) {
            return fail(KP_E_NOMEM, "kp_ispec_regions: a row of counters does not fit memory");
        }
        uint64_t n_items = 0;
        for (uint64_t r = 0; r < n_regions; ++r) {
            std::fill(row.begin(), row.end(), 0);
            uint64_t none[4] = {0, 0, 0, 0}, inv = 0;
            for (uint64_t b = reg_begin[r]; b < reg_end[r]; ++b) {
                kp_s_win w{0u, 0u, 0u};
                if (!kp_i_window(seq, n, b, k, mask, w)) {
                    ++inv;
                    continue;
                }
                for (int e = 0; e < 4; ++e) {
                    const int32_t j = s->h_lut[4ull * w.fwd + e];
                    if (j >= 0)
                        ++row[(e & 1 ? P : 0u) + (uint32_t)j];
                    else
                        ++none[e];
                }
            }
            n_items += scan_pieces(reg_begin[r], reg_end[r], lo, hi);
            for (int e = 0; e < 4; ++e) other[5 * r + e] = none[e];
            other[5 * r + 4] = inv;
            s->st.unmatched += none[0] + none[1] + none[2] + none[3];
            s->st.invalid += inv;
            s->st.assigned += 4 * (reg_end[r] - reg_begin[r] - inv) - none[0] - none[1] - none[2] - none[3];
            if (hist) memcpy(hist + r * 2 * P, row.data(), (size_t)P * 16);
            if (rates) {
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t kind = j >> 1, strand = j & 1u;
                    double acc = 0.0;
                    for (uint32_t e = s->kind_off[kind]; e < s->kind_off[kind + 1]; ++e)
                        acc = acc + (double)row[(size_t)strand * P + s->by_kind[e]] * rates[s->by_kind[e]];
                    expected[4 * r + j] = acc;
                }
            }
        }
        s->st.items += n_items;
        return KP_OK;
    }

    KP_HIP(hipSetDevice(c->device));
    const long lds_p = env_int("KP_ISPEC_LDS_P", KP_IS_LDS_P);
    if (lds_p < 0 || lds_p > KP_IS_LDS_P)
        return fail(KP_E_ARG, "kp_ispec_regions: KP_ISPEC_LDS_P must be 0..8192 (2 P uint32 counters beside a second workgroup's)");
    const bool lds = env_int("KP_ISPEC_GLOBAL", 0) == 0 && (long)P <= lds_p;
    std::vector<kp_p_item> items;
    std::vector<uint64_t> off_contig;  // per region: breakpoints outside [lo, hi)
    try {
        off_contig.resize(n_regions);
        for (uint64_t r = 0; r < n_regions; ++r)
            off_contig[r] = reg_end[r] - reg_begin[r] - scan_cut(items, reg_begin[r], reg_end[r], lo, hi, (uint32_t)r);
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_ispec_regions: the work items do not fit host memory");
    }
    if (items.size() >= (1ull << 32)) return fail(KP_E_ARG, "kp_ispec_regions: 2^32 work items or more in one call");
    const size_t cnts = (size_t)n_regions * 2 * P;
    const size_t b_hist = g_up(cnts * 8), b_other = g_up(n_regions * 40);
    const size_t b_rates = rates ? g_up((size_t)P * 8) + g_up((size_t)P * 4) : 0;
    const size_t b_exp = rates ? g_up(n_regions * 32) : 0;
    if ((rc = ispec_arena(c, "kp_ispec_regions", b_hist + b_other + b_rates + b_exp))) return rc;
    unsigned long long *d_hist = (unsigned long long *)c->arena.take(cnts * 8);
    unsigned long long *d_other = (unsigned long long *)c->arena.take(n_regions * 40);
    double *d_rates = rates ? (double *)c->arena.take((size_t)P * 8) : nullptr;
    uint32_t *d_kind = rates ? (uint32_t *)c->arena.take((size_t)P * 4) : nullptr;
    double *d_exp = rates ? (double *)c->arena.take(n_regions * 32) : nullptr;
    if ((rc = c->arena.check("kp_ispec_regions"))) return rc;
    hipStream_t st = c->stream;
    KP_HIP(hipMemsetAsync(d_hist, 0, cnts * 8, st));
    KP_HIP(hipMemsetAsync(d_other, 0, n_regions * 40, st));
    if (!items.empty()) {
        uint8_t *d_seq = nullptr;
        kp_p_item *d_items = nullptr;
        if ((rc = scan_upload(c, "kp_ispec_regions", seq, n, items, 0, &d_seq, &d_items))) return rc;
        const size_t lds_bytes = lds ? (size_t)P * 8 : 0;
        const uint64_t grid = scan_grid(c, items.size(), scan_per_cu(lds_bytes), "KP_ISPEC_GRID");
        kp_is_args A;
        A.seq = d_seq;
        A.items = d_items;
        A.n_items = (uint32_t)items.size();
        A.steps = (uint32_t)((items.size() + grid - 1) / grid);
        A.k = k;
        A.mask = mask;
        A.P = P;
        A.lut = (const int4 *)s->d_lut;
        A.hist = d_hist;
        A.other = d_other;
        if ((rc = scan_mark(c, 0))) return rc;
        if (lds)
            hipLaunchKernelGGL((kp_ispec_scan_kernel<true>), dim3((unsigned)grid), dim3(KP_S_THREADS), lds_bytes, st, A);
        else
            hipLaunchKernelGGL((kp_ispec_scan_kernel<false>), dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
        if ((rc = scan_launched(c, 1))) return rc;
    }
    if (rates) {
        KP_HIP(hipMemcpyAsync(d_rates, rates, (size_t)P * 8, hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(d_kind, s->by_kind.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
        kp_is_offs T;
        memcpy(T.off, s->kind_off, sizeof T.off);
        hipLaunchKernelGGL(kp_ispec_sums_kernel, dim3((unsigned)((n_regions * 4 + 63) / 64)), dim3(64), 0, st, d_hist, d_rates,
                           d_kind, T, P, n_regions, d_exp);
        KP_HIP(hipGetLastError());
        KP_HIP(hipMemcpyAsync(expected, d_exp, n_regions * 32, hipMemcpyDeviceToHost, st));
    }
    if (hist) KP_HIP(hipMemcpyAsync(hist, d_hist, cnts * 8, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(other, d_other, n_regions * 40, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    if (!items.empty()) {
        float ms = 0.f;
        if ((rc = scan_elapsed(c, 0, 1, &ms))) return rc;
        s->st.scan_ms += ms;
        s->st.path = lds ? 1u : 2u;
    }
    for (uint64_t r = 0; r < n_regions; ++r) {
        uint64_t *o = other + 5 * r;
        o[4] += off_contig[r];
        s->st.unmatched += o[0] + o[1] + o[2] + o[3];
        s->st.invalid += o[4];
        s->st.assigned += 4 * (reg_end[r] - reg_begin[r] - o[4]) - o[0] - o[1] - o[2] - o[3];
    }
    s->st.items += items.size();
    return KP_OK;
}

int kp_ispec_track(kp_ctx *c, const uint8_t *seq, uint64_t n, uint64_t begin, uint64_t end, int32_t *pid) {
    kp_ispec_sess *s = ispec_sess(c);
    int rc = scan_check_contig("kp_ispec_track", s->active, seq, n, "kp_ispec_begin");
    if (rc) return rc;
    if (begin > end || end > n) return fail(KP_E_ARG, "kp_ispec_track: begin > end or a range outside the contig");
    const uint64_t len = end - begin;
    if (!len) return KP_OK;
    if (!pid) return fail(KP_E_ARG, "kp_ispec_track: null output");
    const int k = s->k;
    const uint32_t mask = (uint32_t)(s->cells - 1);
    const uint64_t n_items = scan_tiles(len);
    if (!c) {
        for (uint64_t i = 0; i < len; ++i) {
            kp_s_win w{0u, 0u, 0u};
            const bool ok = kp_i_window(seq, n, begin + i, k, mask, w);
            for (int e = 0; e < 4; ++e) pid[e * len + i] = ok ? s->h_lut[4ull * w.fwd + e] : KP_P_INVALID;
        }
        s->st.items += n_items;
        return KP_OK;
    }
    KP_HIP(hipSetDevice(c->device));
    const size_t plane = g_up(len * 4);  // bytes between two planes on the device
    if ((rc = ispec_arena(c, "kp_ispec_track", 4 * plane))) return rc;
    int32_t *d_pid = (int32_t *)c->arena.take(4 * plane);
    if ((rc = c->arena.check("kp_ispec_track"))) return rc;
    uint8_t *d_seq = nullptr;
    if ((rc = scan_upload(c, "kp_ispec_track", seq, n, {}, 0, &d_seq, nullptr))) return rc;
    hipStream_t st = c->stream;
    const uint64_t grid = scan_grid(c, n_items, 4, "KP_ISPEC_GRID");  // 33 KB of LDS per workgroup
    uint64_t lo = 0, hi = 0;
    scan_centres(n, k, &lo, &hi);
    kp_is_targs A;
    A.seq = d_seq;
    A.begin = (uint32_t)begin;
    A.len = (uint32_t)len;
    A.lo = (uint32_t)lo;
    A.hi = (uint32_t)hi;
    A.n_items = (uint32_t)n_items;
    A.steps = (uint32_t)((n_items + grid - 1) / grid);
    A.k = k;
    A.mask = mask;
    A.lut = (const int4 *)s->d_lut;
    A.pid = d_pid;
    A.plane = plane / 4;
    if ((rc = scan_mark(c, 0))) return rc;
    hipLaunchKernelGGL(kp_ispec_track_kernel, dim3((unsigned)grid), dim3(KP_S_THREADS), 0, st, A);
    if ((rc = scan_launched(c, 1))) return rc;
    for (int e = 0; e < 4; ++e)
        KP_HIP(hipMemcpyAsync(pid + e * len, d_pid + e * (plane / 4), len * 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    if ((rc = scan_elapsed(c, 0, 1, &ms))) return rc;
    s->st.scan_ms += ms;
    s->st.items += n_items;
    return KP_OK;
}

int kp_ispec_sites(kp_ctx *c, const uint8_t *seq, uint64_t n, uint32_t contig, const uint64_t *pos,
                   const uint64_t *del_len, const uint64_t *key, const uint64_t *ins_off, const uint8_t *ins,
                   uint64_t n_sites, int place, uint64_t seed, uint64_t *resolved, int32_t *pid) {
    kp_ispec_sess *s = ispec_sess(c);
    int rc = scan_check_contig("kp_ispec_sites", s->active, seq, n, "kp_ispec_begin");
    if (rc) return rc;
    if ((rc = indel_check("kp_ispec_sites", n, pos, del_len, ins_off, ins, n_sites, place))) return rc;
    if (!n_sites) return KP_OK;
    if (!pid) return fail(KP_E_ARG, "kp_ispec_sites: null output");
    const int k = s->k;
    const uint32_t mask = (uint32_t)(s->cells - 1);
    if (!c) {
        for (uint64_t i = 0; i < n_sites; ++i) {
            const uint32_t b = (uint32_t)pos[i];
            const bool del = del_len[i] != 0;
            const uint32_t L = del ? (uint32_t)del_len[i] : (uint32_t)(ins_off[i + 1] - ins_off[i]);
            const uint8_t *in = ins ? ins + ins_off[i] : nullptr;
            uint32_t a = 0, e = 0;
            while (kp_i_left(seq, in, b, L, del, a)) ++a;
            while (kp_i_right(seq, n, in, b, L, del, e)) ++e;
            const uint32_t lo = b - a, hi = b + e;
            const uint32_t p = kp_i_place(lo, hi, place, seed, contig, key ? key[i] : i);
            kp_is_site(seq, n, p, L, del, k, mask, s->h_lut.data(), pid + 2 * i);
            ++(pid[2 * i] != KP_P_INVALID ? s->st.sites : s->st.sites_skipped);
            if (resolved) resolved[3 * i] = lo, resolved[3 * i + 1] = hi, resolved[3 * i + 2] = p;
        }
        return KP_OK;
    }
    KP_HIP(hipSetDevice(c->device));
    const size_t b_pid = g_up(n_sites * 8), b_res = resolved ? g_up(n_sites * 24) : 0, b_stat = g_up(16);
    if ((rc = ispec_arena(c, "kp_ispec_sites", b_pid + b_res + b_stat))) return rc;
    int32_t *d_pid = (int32_t *)c->arena.take(n_sites * 8);
    uint64_t *d_res = resolved ? (uint64_t *)c->arena.take(n_sites * 24) : nullptr;
    unsigned long long *d_stat = (unsigned long long *)c->arena.take(16);
    if ((rc = c->arena.check("kp_ispec_sites"))) return rc;
    const uint64_t pool = ins_off[n_sites];
    const size_t b_site = g_up(n_sites * 8), b_off = g_up((n_sites + 1) * 8), b_ins = g_up(pool + 1);
    uint8_t *d_seq = nullptr;
    if ((rc = scan_upload(c, "kp_ispec_sites", seq, n, {}, 3 * b_site + b_off + b_ins, &d_seq, nullptr))) return rc;
    uint64_t *d_pos = (uint64_t *)c->seq_in.take(b_site);
    uint64_t *d_del = (uint64_t *)c->seq_in.take(b_site);
    uint64_t *d_key = (uint64_t *)c->seq_in.take(b_site);
    uint64_t *d_off = (uint64_t *)c->seq_in.take(b_off);
    uint8_t *d_ins = (uint8_t *)c->seq_in.take(b_ins);
    if ((rc = c->seq_in.check("kp_ispec_sites"))) return rc;
    hipStream_t st = c->stream;
    KP_HIP(hipMemcpyAsync(d_pos, pos, n_sites * 8, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_del, del_len, n_sites * 8, hipMemcpyHostToDevice, st));
    if (key) KP_HIP(hipMemcpyAsync(d_key, key, n_sites * 8, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_off, ins_off, (n_sites + 1) * 8, hipMemcpyHostToDevice, st));
    if (pool) KP_HIP(hipMemcpyAsync(d_ins, ins, pool, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemsetAsync(d_stat, 0, 16, st));
    kp_is_sargs A;
    A.seq = d_seq;
    A.n = n;
    A.pos = d_pos;
    A.del_len = d_del;
    A.key = key ? d_key : nullptr;
    A.ins_off = d_off;
    A.ins = d_ins;
    A.n_sites = n_sites;
    A.max_steps = (uint32_t)(n / 64 + 1);
    A.k = k;
    A.place = place;
    A.contig = contig;
    A.seed = seed;
    A.mask = mask;
    A.lut = s->d_lut;
    A.stat = d_stat;
    A.resolved = d_res;
    A.pid = d_pid;
    if ((rc = scan_mark(c, 0))) return rc;
    hipLaunchKernelGGL(kp_ispec_sites_kernel, dim3((unsigned)((n_sites + 255) / 256)), dim3(256), 0, st, A);
    if ((rc = scan_launched(c, 1))) return rc;
    unsigned long long h_stat[2] = {0, 0};
    KP_HIP(hipMemcpyAsync(h_stat, d_stat, sizeof h_stat, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(pid, d_pid, n_sites * 8, hipMemcpyDeviceToHost, st));
    if (resolved) KP_HIP(hipMemcpyAsync(resolved, d_res, n_sites * 24, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    float ms = 0.f;
    if ((rc = scan_elapsed(c, 0, 1, &ms))) return rc;
    s->st.sites_ms += ms;
    s->st.sites += h_stat[0];
    s->st.sites_skipped += h_stat[1];
    return KP_OK;
}

int kp_ispec_end(kp_ctx *c) {
    kp_ispec_sess *s = ispec_sess(c);
    if (!s->active) return fail(KP_E_STATE, "kp_ispec_end: no session (kp_ispec_begin first)");
    s->active = false;
    s->lut_ok = false;
    std::vector<int32_t>().swap(s->h_lut);
    std::vector<uint64_t>().swap(s->pats);
    std::vector<uint32_t>().swap(s->pkind);
    std::vector<uint32_t>().swap(s->by_kind);
    return KP_OK;
}

int kp_ispec_last_stats(kp_ctx *c, kp_ispec_stats *out) {
    if (!out) return fail(KP_E_ARG, "kp_ispec_last_stats: null out");
    *out = ispec_sess(c)->st;
    return KP_OK;
}

int kp_ispec_host(int k, const uint64_t *patterns, const uint32_t *pkind, uint32_t n_patterns, const uint8_t *seq, uint64_t n,
                  uint32_t contig, const uint64_t *reg_begin, const uint64_t *reg_end, uint64_t n_regions,
                  const double *rates, uint64_t *hist, uint64_t *other, double *expected, uint64_t track_begin,
                  uint64_t track_end, int32_t *track_pid, const uint64_t *pos, const uint64_t *del_len, const uint64_t *key,
                  const uint64_t *ins_off, const uint8_t *ins, uint64_t n_sites, int place, uint64_t seed,
                  uint64_t *resolved, int32_t *site_pid, kp_ispec_stats *stats) {
    int rc = kp_ispec_begin(nullptr, k, patterns, pkind, n_patterns);
    if (rc) return rc;
    rc = kp_ispec_regions(nullptr, seq, n, reg_begin, reg_end, n_regions, rates, hist, other, expected);
    if (!rc && track_pid) rc = kp_ispec_track(nullptr, seq, n, track_begin, track_end, track_pid);
    if (!rc)
        rc = kp_ispec_sites(nullptr, seq, n, contig, pos, del_len, key, ins_off, ins, n_sites, place, seed, resolved, site_pid);
    const std::string err = g_err;
    const int rc_end = kp_ispec_end(nullptr);
    if (rc) return fail(rc, err);
    if (stats) *stats = g_ispec_host.st;
    return rc_end;
}

}  // extern "C"
