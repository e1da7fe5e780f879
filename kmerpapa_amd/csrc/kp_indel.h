// kp_indel.h -- breakpoint contexts of short insertions and deletions (no reference counterpart:
// the external counter the reference's README names has an indel mode; the semantics here are this
// project's own).  Included by kp_hip.hip after kp_seq.h (the session, bases, windows) and kp_sim.h
// (kp_sm_philox).  Semantics: include/kmerpapa_hip.h.
//
// An indel inside a repeat has no unique position, so every site's equivalence interval [lo, hi]
// is found on the contig before it is placed and counted.  Integer work only: a device session
// equals the host session bit for bit.  The per-base code is __host__ __device__ and shared:
//   kp_i_eq      two bytes are the same base (either case; an invalid byte equals nothing)
//   kp_i_left    may the site move t + 1 places to the left, given that it may move t?
//   kp_i_right   the same to the right
//   kp_i_place   the breakpoint chosen in [lo, hi]: left, right, or the Philox draw of the site's key
//   kp_i_cells   the two or four (column, code) cells a placed site adds 1 to, none if it is skipped
//
//   kp_seq_indels_kernel  a lane owns one site, a wave searches for one site at a time: lane l asks
//                         kp_i_left / kp_i_right at t = 64 step + l, a ballot finds the first
//                         mismatch, so a site inside a run of R bases costs R / 64 steps of two
//                         coalesced loads per side, not R dependent ones; the two sides advance in
//                         the same step.  Then each lane places its own site, builds its windows
//                         with kp_seq's roll and adds with global 64-bit atomics.  Kept and skipped
//                         sites are counted by a ballot per wave.
//
// Every device loop has a bound the host computed (n / 64 + 1 steps: kp_i_left is false at t = b <= n,
// kp_i_right at t = n - b); there are no waits between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp_rt.h"
#include "kp_seq.h"
#include "kp_sim.h"

#define KP_I_TAG 0x494E444Cu  // "INDL": the fourth counter word of a placement draw
#define KP_I_LEFT 0
#define KP_I_RIGHT 1
#define KP_I_SAMPLE 2
#define KP_I_INS 0        // the columns of an indel session
#define KP_I_DEL_START 1
#define KP_I_DEL_END 2

__host__ __device__ inline bool kp_i_eq(uint32_t a, uint32_t b) {
    const uint32_t ca = kp_s_class(a);
    return ca < 4u && ca == kp_s_class(b);
}

// A site: breakpoint b and a string of L >= 1 bases, seq[b, b + L) for a deletion (b + L <= n),
// ins[0, L) for an insertion.  Moving the site one place to the left rotates the string by one, so
// the placement t + 1 places to the left exists iff all of kp_i_left(0 .. t) hold.
__host__ __device__ inline bool kp_i_left(const uint8_t *seq, const uint8_t *ins, uint32_t b, uint32_t L, bool del,
                                          uint32_t t) {
    if (t >= b) return false;
    return kp_i_eq(seq[b - 1u - t], del ? seq[b + (L - 1u) - t] : ins[L - 1u - t % L]);
}

__host__ __device__ inline bool kp_i_right(const uint8_t *seq, uint64_t n, const uint8_t *ins, uint32_t b, uint32_t L,
                                           bool del, uint32_t t) {
    if ((uint64_t)b + (del ? L : 0u) + t >= n) return false;
    return kp_i_eq(seq[b + t], del ? seq[b + L + t] : ins[t % L]);
}

// The multiply-shift is not exactly uniform over the span hi - lo + 1: a placement's probability is
// off by less than 2^-32 * span (relative)
__host__ __device__ inline uint32_t kp_i_place(uint32_t lo, uint32_t hi, int place, uint64_t seed, uint32_t contig,
                                               uint64_t key) {
    if (place == KP_I_LEFT) return lo;
    if (place == KP_I_RIGHT) return hi;
    uint32_t x0 = (uint32_t)key, x1 = (uint32_t)(key >> 32), x2 = contig, x3 = KP_I_TAG;
    kp_sm_philox(x0, x1, x2, x3, (uint32_t)seed, (uint32_t)(seed >> 32));
    return lo + (uint32_t)(((uint64_t)x0 * ((uint64_t)hi - lo + 1u)) >> 32);
}

// the window of breakpoint p, seq[p - k/2, p + k/2): false if it runs off the contig or holds an
// invalid byte
__host__ __device__ inline bool kp_i_window(const uint8_t *seq, uint64_t n, uint64_t p, int k, uint32_t mask,
                                            kp_s_win &w) {
    const uint64_t r = (uint64_t)(k / 2);
    w = kp_s_win{0u, 0u, 0u};
    if (p < r || p + r > n) return false;
    for (int j = 0; j < k; ++j) kp_s_step(w, kp_s_class(seq[p - r + j]), mask, 2 * (k - 1));
    return w.valid == (uint32_t)k;
}

// cell[i] = column * cells + code of every add of the site placed at p (p + L <= n for a deletion);
// returns how many: 0 = the site is skipped, whole
__host__ __device__ inline int kp_i_cells(const uint8_t *seq, uint64_t n, uint32_t p, uint32_t L, bool del, int k,
                                          uint64_t cells, int both, uint64_t cell[4]) {
    const uint32_t mask = (uint32_t)(cells - 1);
    kp_s_win w{0u, 0u, 0u}, e{0u, 0u, 0u};
    if (!kp_i_window(seq, n, p, k, mask, w)) return 0;
    if (!del) {
        cell[0] = KP_I_INS * cells + w.fwd;
        cell[1] = KP_I_INS * cells + w.rc;  // an insertion is its own mirror
        return both ? 2 : 1;
    }
    if (!kp_i_window(seq, n, (uint64_t)p + L, k, mask, e)) return 0;
    cell[0] = KP_I_DEL_START * cells + w.fwd;
    cell[1] = KP_I_DEL_END * cells + e.fwd;
    cell[2] = KP_I_DEL_END * cells + w.rc;  // the start read on the other strand is an end
    cell[3] = KP_I_DEL_START * cells + e.rc;
    return both ? 4 : 2;
}

struct kp_i_args {
    const uint8_t *seq;  // the contig
    uint64_t n;
    const uint64_t *pos, *del_len, *key, *ins_off;  // [n_sites], ins_off [n_sites + 1]; key may be NULL (= the index)
    const uint8_t *ins;                            // the insertions' bytes
    uint64_t n_sites;
    uint32_t max_steps;  // n / 64 + 1
    int32_t k, both, place;
    uint32_t contig;
    uint64_t seed;
    uint64_t cells;
    unsigned long long *tab;   // [3][cells]: ins, del_start, del_end
    unsigned long long *stat;  // [1] += sites counted, [2] += sites skipped
    uint64_t *resolved;        // [n_sites][3] lo, hi, chosen; or NULL
};

#ifdef __HIPCC__

__global__ void __launch_bounds__(256) kp_seq_indels_kernel(kp_i_args A) {
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
    // the wave's sites one after the other (its active lanes are lanes 0 .. n_live - 1)
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
        uint64_t cell[4];
        const int adds = kp_i_cells(A.seq, A.n, p, L, del != 0, A.k, A.cells, A.both, cell);
        for (int q = 0; q < adds; ++q) atomicAdd(&A.tab[cell[q]], 1ull);
        ok = adds != 0;
        if (A.resolved) {
            A.resolved[3 * i] = lo;
            A.resolved[3 * i + 1] = hi;
            A.resolved[3 * i + 2] = p;
        }
    }
    const unsigned long long kept = __popcll(__ballot(ok)), skipped = __popcll(__ballot(act && !ok));
    if (lane == 0) {  // one atomic per wave and counter
        if (kept) atomicAdd(&A.stat[1], kept);
        if (skipped) atomicAdd(&A.stat[2], skipped);
    }
}

#endif  // __HIPCC__

static int indel_check(const std::string &w, uint64_t n, const uint64_t *pos, const uint64_t *del_len,
                       const uint64_t *ins_off, const uint8_t *ins, uint64_t n_sites, int place) {
    if (place != KP_I_LEFT && place != KP_I_RIGHT && place != KP_I_SAMPLE)
        return fail(KP_E_ARG, w + ": place must be 0 (left), 1 (right) or 2 (sample)");
    if (!n_sites) return KP_OK;
    if (!pos || !del_len || !ins_off) return fail(KP_E_ARG, w + ": null site arrays");
    if (n_sites >= (1ull << 32)) return fail(KP_E_ARG, w + ": 2^32 sites or more in one call");
    if (ins_off[n_sites] >= (1ull << 32)) return fail(KP_E_ARG, w + ": 4 GiB of inserted bases or more in one call");
    if (ins_off[n_sites] && !ins) return fail(KP_E_ARG, w + ": null insertion bytes");
    for (uint64_t i = 0; i < n_sites; ++i) {
        const std::string site = w + ": site " + std::to_string(i);
        if (ins_off[i] > ins_off[i + 1]) return fail(KP_E_ARG, site + ": the insertion offsets decrease");
        const uint64_t il = ins_off[i + 1] - ins_off[i];
        if (pos[i] > n)
            return fail(KP_E_ARG, site + " at " + std::to_string(pos[i]) + " lies past the contig's " + std::to_string(n) + " bases");
        if (del_len[i] > n - pos[i])
            return fail(KP_E_ARG, site + ": the deletion of " + std::to_string(del_len[i]) + " bases at " +
                                      std::to_string(pos[i]) + " runs past the contig's " + std::to_string(n) + " bases");
        if ((del_len[i] != 0) == (il != 0))
            return fail(KP_E_ARG, site + (il ? " is both an insertion and a deletion" : " is neither an insertion nor a deletion"));
        for (uint64_t q = ins_off[i]; q < ins_off[i + 1]; ++q)
            if (kp_s_class(ins[q]) >= 4u)
                return fail(KP_E_ARG, site + ": byte " + std::to_string(q - ins_off[i]) + " of the insertion is not a base");
    }
    return KP_OK;
}

extern "C" {

int kp_seq_indels(kp_ctx *c, const uint8_t *seq, uint64_t n, uint32_t contig, const uint64_t *pos,
                  const uint64_t *del_len, const uint64_t *key, const uint64_t *ins_off, const uint8_t *ins,
                  uint64_t n_sites, int place, uint64_t seed, uint64_t *resolved) {
    kp_seq_sess *s = seq_sess(c);
    int rc = scan_check_contig("kp_seq_indels", s->active, seq, n, "kp_seq_begin_indel");
    if (rc) return rc;
    if (!s->indel) return fail(KP_E_STATE, "kp_seq_indels: the session is not an indel session (kp_seq_begin_indel)");
    if ((rc = indel_check("kp_seq_indels", n, pos, del_len, ins_off, ins, n_sites, place))) return rc;
    if (!n_sites) return KP_OK;
    const int k = s->k;
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
            uint64_t cell[4];
            const int adds = kp_i_cells(seq, n, p, L, del, k, s->cells, s->both, cell);
            for (int q = 0; q < adds; ++q) ++s->h_tab[cell[q]];
            ++(adds ? s->st.sites : s->st.sites_skipped);
            if (resolved) resolved[3 * i] = lo, resolved[3 * i + 1] = hi, resolved[3 * i + 2] = p;
        }
        return KP_OK;
    }
    KP_HIP(hipSetDevice(c->device));
    const uint64_t pool = ins_off[n_sites];
    const size_t b_seq = g_up(n + KP_S_PAD), b_site = g_up(n_sites * 8), b_off = g_up((n_sites + 1) * 8),
                 b_ins = g_up(pool + 1), b_res = resolved ? g_up(n_sites * 24) : 0;
    if ((rc = c->seq_in.reserve("kp_seq_indels", b_seq + 3 * b_site + b_off + b_ins + b_res))) return rc;
    uint8_t *d_seq = (uint8_t *)c->seq_in.take(b_seq);
    uint64_t *d_pos = (uint64_t *)c->seq_in.take(b_site);
    uint64_t *d_del = (uint64_t *)c->seq_in.take(b_site);
    uint64_t *d_key = (uint64_t *)c->seq_in.take(b_site);
    uint64_t *d_off = (uint64_t *)c->seq_in.take(b_off);
    uint8_t *d_ins = (uint8_t *)c->seq_in.take(b_ins);
    uint64_t *d_res = resolved ? (uint64_t *)c->seq_in.take(b_res) : nullptr;
    if ((rc = c->seq_in.check("kp_seq_indels"))) return rc;
    hipStream_t st = c->stream;
    KP_HIP(hipMemcpyAsync(d_seq, seq, n, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_pos, pos, n_sites * 8, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_del, del_len, n_sites * 8, hipMemcpyHostToDevice, st));
    if (key) KP_HIP(hipMemcpyAsync(d_key, key, n_sites * 8, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_off, ins_off, (n_sites + 1) * 8, hipMemcpyHostToDevice, st));
    if (pool) KP_HIP(hipMemcpyAsync(d_ins, ins, pool, hipMemcpyHostToDevice, st));
    kp_i_args A;
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
    A.both = s->both;
    A.place = place;
    A.contig = contig;
    A.seed = seed;
    A.cells = s->cells;
    A.tab = s->d_tab;
    A.stat = s->d_stat;
    A.resolved = d_res;
    hipLaunchKernelGGL(kp_seq_indels_kernel, dim3((unsigned)((n_sites + 255) / 256)), dim3(256), 0, st, A);
    KP_HIP(hipGetLastError());
    unsigned long long h_stat[3] = {0, 0, 0};
    KP_HIP(hipMemcpyAsync(h_stat, s->d_stat, sizeof h_stat, hipMemcpyDeviceToHost, st));
    if (resolved) KP_HIP(hipMemcpyAsync(resolved, d_res, n_sites * 24, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    s->st.sites = h_stat[1];
    s->st.sites_skipped = h_stat[2];
    return KP_OK;
}

int kp_seq_indel_host(int k, int both, const uint8_t *seq, uint64_t n, uint32_t contig, int scan,
                      const uint64_t *reg_begin, const uint64_t *reg_end, uint64_t n_regions, const uint64_t *pos,
                      const uint64_t *del_len, const uint64_t *key, const uint64_t *ins_off, const uint8_t *ins,
                      uint64_t n_sites, int place, uint64_t seed, uint64_t *pos_counts, uint64_t *bg_counts,
                      uint64_t *resolved, kp_seq_stats *stats) {
    int rc = kp_seq_begin_indel(nullptr, k, both);
    if (rc) return rc;
    if (scan) rc = kp_seq_scan(nullptr, seq, n, reg_begin, reg_end, n_regions);
    if (!rc) rc = kp_seq_indels(nullptr, seq, n, contig, pos, del_len, key, ins_off, ins, n_sites, place, seed, resolved);
    const std::string err = g_err;
    const int rc_end = kp_seq_end_typed(nullptr, rc ? nullptr : pos_counts, rc ? nullptr : bg_counts);
    if (rc) return fail(rc, err);
    if (stats) *stats = g_seq_host.st;
    return rc_end;
}

}  // extern "C"
