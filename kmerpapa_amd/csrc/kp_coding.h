// kp_coding.h -- expected mutations per transcript by coding consequence (no reference
// counterpart).  Included by kp_hip.hip.  Semantics: include/kmerpapa_hip.h.
//
// A call of a kp_spec session (kp_spec.h): the window, folding, table gather and the float64 sums
// are that file's.  New here is the class of a (position, forward ALT) pair -- synonymous, missense,
// nonsense, stop-lost, essential splice -- from the codon the position belongs to on its
// transcript's strand.  The per-pair functions are __host__ __device__ and hold integer arithmetic
// only; a device session equals the host session bit for bit:
//   kp_cd_aa / kp_cd_class_of   the standard genetic code and the class of (REF codon, ALT codon)
//   kp_cd_tcodon / kp_cd_codons the transcript-strand codon of three digits in genomic order
//   kp_cd_is_splice             the essential splice positions of an intron
//   kp_cd_near / kp_cd_codon_at the codon of a position by a walk over the transcript's segments
//   kp_cd_site                  one (site, transcript) pair: segment search, class and codons
//
//   kp_coding_scan_kernel   kp_spec_scan_kernel's grid, loads, roll and batches over items that are
//                           pieces of one CDS segment or of one splice interval.  A record per
//                           segment (uniform for the workgroup) gives the transcript, strand, the
//                           spliced index of the first base and the two spliced bases before and
//                           after the segment, so a centre's codon is its neighbours within +-2
//                           inside the segment and those four bytes at its ends.  The roll keeps
//                           the classes of the last bytes in one 64-bit word (3 bits each, fed two
//                           bytes ahead of the window), from which the five bytes around a centre
//                           come by one uniform shift: no register is indexed dynamically.  The
//                           classes of a codon's nine changes are one byte per (codon, position)
//                           of a 192-byte table in LDS.  Each pair adds 1 to counter
//                           [class][pattern] -- uint32 LDS counters of the item, flushed to the
//                           transcript's rows, or global 64-bit atomics; other[transcript][8]
//                           gets one atomic per wave, item and counter
//   kp_coding_sites_kernel  one thread per (site, transcript) pair: kp_cd_site and kp_sp_site
//
// Every device loop has a bound the host computed; there are no waits between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "kp_spec.h"

#define KP_CD_CLASSES 5      // synonymous, missense, nonsense, stop-lost, splice
#define KP_CD_OTHER 8        // other[t][8]
#define KP_CD_SPLICE 4u      // the class of every pair of an essential splice position
#define KP_CD_MAX_SPLICE 8u
#define KP_CD_TAB_WORDS 48   // the class table: 64 codons x 3 positions, one byte each
#define KP_CD_LDS_P (65536 / (4 * KP_CD_CLASSES))  // most patterns with LDS counters: 5 P uint32 in 64 KiB
#define KP_CD_NOT_IN (-1)
#define KP_CD_NO_CLASS (-2)
#define KP_CD_F_STRAND 1u
#define KP_CD_F_SPLICE 2u

__host__ __device__ inline uint32_t kp_cd_comp(uint32_t digit) { return 3u - digit; }

// the amino acid of codon 16 b0 + 4 b1 + b2 (digits A 0, C 1, G 2, T 3), '*' = stop
__host__ __device__ inline uint32_t kp_cd_aa(uint32_t codon) {
    return (uint32_t)"KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"[codon & 63u];
}

// 0 synonymous (or stop to stop), 1 missense, 2 nonsense, 3 stop-lost
__host__ __device__ inline uint32_t kp_cd_class_of(uint32_t ref_codon, uint32_t alt_codon) {
    const uint32_t a = kp_cd_aa(ref_codon), b = kp_cd_aa(alt_codon);
    return a == b ? 0u : (b == (uint32_t)'*' ? 2u : (a == (uint32_t)'*' ? 3u : 1u));
}

// the codon on the transcript's strand of three digits in genomic order
__host__ __device__ inline uint32_t kp_cd_tcodon(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t strand) {
    return strand ? 16u * kp_cd_comp(x2) + 4u * kp_cd_comp(x1) + kp_cd_comp(x0) : 16u * x0 + 4u * x1 + x2;
}

// the transcript-strand REF and ALT codons of a change of genomic codon position i (0..2) into
// the forward digit alt
__host__ __device__ inline void kp_cd_codons(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t i, uint32_t alt,
                                             uint32_t strand, uint32_t *ref_codon, uint32_t *alt_codon) {
    *ref_codon = kp_cd_tcodon(x0, x1, x2, strand);
    *alt_codon = kp_cd_tcodon(i == 0u ? alt : x0, i == 1u ? alt : x1, i == 2u ? alt : x2, strand);
}

__host__ __device__ inline uint32_t kp_cd_class(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t i, uint32_t alt,
                                                uint32_t strand) {
    uint32_t r = 0, a = 0;
    kp_cd_codons(x0, x1, x2, i, alt, strand, &r, &a);
    return kp_cd_class_of(r, a);
}

// g is an essential splice position of the intron [a, b)
__host__ __device__ inline bool kp_cd_is_splice(uint64_t g, uint64_t a, uint64_t b, uint32_t splice) {
    return g >= a && g < b && (g - a < (uint64_t)splice || b - g <= (uint64_t)splice);
}

// The class (0..3, 4 = no base) of the byte d spliced bases (-2..2) from position g of segment e
// of a transcript with the non-empty segments [lo, hi); 4 outside the CDS.
__host__ __device__ inline uint32_t kp_cd_near(const uint8_t *seq, const uint64_t *sb, const uint64_t *se, uint64_t lo,
                                               uint64_t hi, uint64_t e, uint64_t g, int d) {
    for (; d < 0; ++d) {  // (at most two steps each way)
        if (g > sb[e]) {
            --g;
        } else {
            if (e == lo) return 4u;
            --e;
            g = se[e] - 1u;
        }
    }
    for (; d > 0; --d) {
        if (g + 1u < se[e]) {
            ++g;
        } else {
            if (e + 1u == hi) return 4u;
            ++e;
            g = sb[e];
        }
    }
    return kp_s_class(seq[g]);
}

// the codon of position g of segment e, spliced index j: three classes in genomic order and g's place
__host__ __device__ inline void kp_cd_codon_at(const uint8_t *seq, const uint64_t *sb, const uint64_t *se, uint64_t lo,
                                               uint64_t hi, uint64_t e, uint64_t g, uint64_t j, uint32_t x[3],
                                               uint32_t *i) {
    const int at = (int)(j % 3u);
    *i = (uint32_t)at;
    x[0] = kp_cd_near(seq, sb, se, lo, hi, e, g, -at);
    x[1] = kp_cd_near(seq, sb, se, lo, hi, e, g, 1 - at);
    x[2] = kp_cd_near(seq, sb, se, lo, hi, e, g, 2 - at);
}

// One (site, transcript) pair: the class 0..4, KP_CD_NOT_IN, KP_CD_NO_CLASS or KP_SP_ALT_IS_REF (in
// that order of precedence), and for classes 0..3 the packed codons (REF | ALT << 6).  sj0[e] = the
// spliced index of segment e's first base; `iters` bounds the segment search (2^iters > segments).
__host__ __device__ inline int kp_cd_site(const uint8_t *seq, const uint64_t *sb, const uint64_t *se, const uint64_t *sj0,
                                          uint64_t lo, uint64_t hi, uint32_t strand, uint32_t splice, uint32_t iters,
                                          uint64_t g, uint32_t alt, uint32_t *codons) {
    *codons = 0;
    uint64_t l = lo, r = hi;  // the first segment that ends after g
    for (uint32_t it = 0; it < iters && l < r; ++it) {
        const uint64_t m = l + (r - l) / 2u;
        if (se[m] > g)
            r = m;
        else
            l = m + 1u;
    }
    const uint32_t own = kp_s_class(seq[g]), a = kp_s_class(alt) & 3u;
    if (l < hi && sb[l] <= g) {
        uint32_t x[3], i = 0;
        kp_cd_codon_at(seq, sb, se, lo, hi, l, g, sj0[l] + (g - sb[l]), x, &i);
        if ((x[0] | x[1] | x[2]) > 3u) return KP_CD_NO_CLASS;
        if (a == own) return KP_SP_ALT_IS_REF;
        uint32_t rc = 0, ac = 0;
        kp_cd_codons(x[0], x[1], x[2], i, a, strand, &rc, &ac);
        *codons = rc | (ac << 6);
        return (int)kp_cd_class_of(rc, ac);
    }
    if (l > lo && l < hi && kp_cd_is_splice(g, se[l - 1u], sb[l], splice)) {
        if (own > 3u) return KP_CD_NO_CLASS;
        if (a == own) return KP_SP_ALT_IS_REF;
        return (int)KP_CD_SPLICE;
    }
    return KP_CD_NOT_IN;
}

// the byte of (transcript-strand codon, position) in the class table: 2 bits per transcript-strand
// ALT digit (0 where ALT is the codon's own base)
__host__ __device__ inline uint32_t kp_cd_tab_byte(uint32_t tcodon, uint32_t tpos) {
    const uint32_t sh = 2u * (2u - tpos), own = (tcodon >> sh) & 3u;
    uint32_t byte = 0;
    for (uint32_t a = 0; a < 4u; ++a)
        if (a != own) byte |= kp_cd_class_of(tcodon, (tcodon & ~(3u << sh)) | (a << sh)) << (2u * a);
    return byte;
}

struct kp_cd_rec {
    uint32_t begin, len;  // the segment or splice interval [begin, begin + len)
    uint32_t j0;          // the spliced index of its first base, mod 3 (a segment)
    uint32_t tx;
    uint32_t flags;       // KP_CD_F_STRAND, KP_CD_F_SPLICE
    uint32_t ctx;         // 3 bits each: the classes of the spliced bases j0 - 2, j0 - 1, j0 + len, j0 + len + 1
};

struct kp_cd_args {
    const uint8_t *seq;      // the contig, KP_S_PAD readable bytes past its end
    uint32_t n;
    const kp_p_item *items;  // [n_items]: region = the index of the item's record
    const kp_cd_rec *recs;
    const uint32_t *tab;     // [KP_CD_TAB_WORDS]
    uint32_t n_items, steps;
    int32_t k, fold;
    uint32_t mask;  // 4^k - 1
    uint32_t P;
    const int4 *lut;            // [4^k]
    unsigned long long *hist;   // [n_tx][5][P]
    unsigned long long *other;  // [n_tx][8]
};

struct kp_cd_sargs {
    const uint8_t *seq;
    uint64_t n;
    const uint64_t *sb, *se, *sj0;  // [n_segs]
    const uint64_t *tx_first;       // [n_tx + 1]
    const uint8_t *tx_strand;       // [n_tx]
    uint32_t splice, iters;
    const uint64_t *pos;  // [n_pairs]
    const uint8_t *alt;
    const uint32_t *tx;
    uint64_t n_pairs;
    int32_t k, fold;
    uint32_t mask;
    const int32_t *lut;
    int32_t *cls, *pid;
    uint32_t *codons;
};

#ifdef __HIPCC__

// the class of the byte dd (-2..2) bases from the centre at offset q of a segment of len bases:
// from the five classes around the centre (3 bits each, +2 lowest) or the record's context
__device__ inline uint32_t kp_cd_pick(uint32_t five, uint32_t ctx, int32_t q, int32_t len, int32_t dd) {
    const int32_t qd = q + dd;
    const bool inside = qd >= 0 && qd < len;
    const int32_t at = qd < 0 ? 2 + qd : 2 + qd - len;  // 0..3 outside
    return inside ? (five >> (3 * (2 - dd))) & 7u : (ctx >> (3 * (at & 3))) & 7u;
}

template <bool LDS>
__global__ void __launch_bounds__(KP_S_THREADS) kp_coding_scan_kernel(kp_cd_args A) {
    extern __shared__ uint32_t kp_cd_lds[];  // the class table, then [5][P] counters with LDS
    const uint8_t *tab = reinterpret_cast<const uint8_t *>(kp_cd_lds);
    uint32_t *cnt5 = kp_cd_lds + KP_CD_TAB_WORDS;
    const uint32_t tid = threadIdx.x;
    const uint32_t n_cnt = KP_CD_CLASSES * A.P;
    if (tid < KP_CD_TAB_WORDS) kp_cd_lds[tid] = A.tab[tid];
    if (LDS)
        for (uint32_t e = tid; e < n_cnt; e += KP_S_THREADS) cnt5[e] = 0;
    __syncthreads();
    const int k = A.k, top = 2 * (A.k - 1), h = A.k / 2;
    const uint32_t lag = (uint32_t)(k - 1 - h);  // bytes between a window's centre and its last byte
    const uint32_t halo = h > 2 ? (uint32_t)h : 2u;
    for (uint32_t s = 0; s < A.steps; ++s) {
        const uint32_t item = s * gridDim.x + blockIdx.x;
        if (item >= A.n_items) break;  // (the same for the whole workgroup)
        const kp_p_item it = A.items[item];
        const kp_cd_rec rec = A.recs[it.region];
        const uint32_t strand = rec.flags & KP_CD_F_STRAND;
        const bool splice = (rec.flags & KP_CD_F_SPLICE) != 0u;
        const uint32_t r0 = tid * KP_S_RUN;
        const uint32_t cnt = r0 < it.count ? min((uint32_t)KP_S_RUN, it.count - r0) : 0u;
        unsigned long long *row = A.hist + (uint64_t)rec.tx * n_cnt;
        // a wave whose 64 runs lie past the item's end has nothing to roll (wave-uniform): with
        // segments of a few hundred bases that is three waves of four
        if ((tid & ~63u) * KP_S_RUN < it.count) {
            // the bytes [s0, s1) of this thread: its centres with the halo, inside the contig (the item is
            // clipped to centres whose window lies inside it, so c0 >= h and the last window ends before n)
            const uint64_t c0 = (uint64_t)it.first + r0;
            const uint64_t s0 = c0 > halo ? c0 - halo : 0u;
            const uint64_t s1 = min(c0 + cnt + halo, (uint64_t)A.n);
            uint32_t d[16], off, end;
            kp_p_load(A.seq, s0, cnt ? (uint32_t)(s1 - s0) : 0u, d, &off, &end);
            const uint32_t full0 = off + (uint32_t)(c0 - (uint32_t)h - s0) + (uint32_t)k - 1u;  // completes the first window
            const uint32_t wend = cnt ? full0 + cnt : 0u;                                      // <= end
            const uint32_t w0 = full0 - ((uint32_t)k - 1u);
            // byte j is position a + j; the centre of the window byte j completes is a + j - lag, at
            // offset q0 + j of the record and codon position (m3 + j) % 3
            const int64_t a = (int64_t)s0 - off;
            const int32_t q0 = (int32_t)(a - (int64_t)lag - (int64_t)rec.begin);
            const uint32_t m3 = (uint32_t)(((int64_t)rec.j0 + q0 + 66) % 3);  // (q0 > -66)
            unsigned long long by_class = 0;  // 8 bits per class: at most 96 pairs of a thread
            uint32_t o5 = 0, o6 = 0, o7 = 0;
            kp_s_win w{0u, 0u, 0u};
            // the classes of the bytes up to j + 2, 3 bits each
            unsigned long long near = ((unsigned long long)kp_s_class(d[0] & 0xffu) << 3) | kp_s_class((d[0] >> 8) & 0xffu);
#pragma unroll
            for (uint32_t jb = 0; jb < 64; jb += KP_P_BATCH) {
                uint32_t code[KP_P_BATCH], info[KP_P_BATCH];
                bool has[KP_P_BATCH], full[KP_P_BATCH];
                int4 p[KP_P_BATCH];
#pragma unroll
                for (uint32_t q = 0; q < KP_P_BATCH; ++q) {
                    const uint32_t j = jb + q;
                    const uint32_t ahead = j + 2u < 64u ? kp_s_class((d[(j + 2u) >> 2 & 15u] >> (8u * ((j + 2u) & 3u))) & 0xffu) : 4u;
                    near = (near << 3) | ahead;
                    if (j >= w0 && j < wend) kp_s_step(w, kp_s_class((d[j >> 2] >> (8u * (j & 3u))) & 0xffu), A.mask, top);
                    full[q] = j >= full0 && j < wend;
                    code[q] = kp_s_code(w, k, A.fold);
                    // the centre's class and those of its three pairs, in slot order of the counted strand
                    const uint32_t five = (uint32_t)(near >> (3u * lag)) & 0x7fffu;
                    const uint32_t own = (five >> 6) & 7u;
                    const uint32_t t3 = m3 + j % 3u, i = t3 >= 3u ? t3 - 3u : t3;
                    const int32_t qc = q0 + (int32_t)j;
                    const uint32_t x0 = kp_cd_pick(five, rec.ctx, qc, (int32_t)rec.len, -(int32_t)i);
                    const uint32_t x1 = kp_cd_pick(five, rec.ctx, qc, (int32_t)rec.len, 1 - (int32_t)i);
                    const uint32_t x2 = kp_cd_pick(five, rec.ctx, qc, (int32_t)rec.len, 2 - (int32_t)i);
                    const bool ok = splice ? own < 4u : (x0 | x1 | x2) < 4u;
                    const uint32_t byte = tab[(kp_cd_tcodon(x0 & 3u, x1 & 3u, x2 & 3u, strand) & 63u) * 3u + (strand ? 2u - i : i)];
                    const bool flip = A.fold && own >= 2u;
                    const uint32_t ref = flip ? 3u - own : own;  // on the counted strand (own < 4 where ok)
                    uint32_t inf = ok ? 1u << 9 : 0u;
#pragma unroll
                    for (uint32_t e = 0; e < 3u; ++e) {
                        const uint32_t ac = e < ref ? e : e + 1u;      // the slot's ALT on the counted strand
                        const uint32_t af = (flip ? 3u - ac : ac) & 3u;  // ... on the forward strand
                        const uint32_t at = strand ? 3u - af : af;     // ... on the transcript's
                        inf |= (splice ? KP_CD_SPLICE : (byte >> (2u * at)) & 3u) << (3u * e);
                    }
                    info[q] = inf;
                    has[q] = full[q] && ok && w.valid >= (uint32_t)k;
                    o5 += (full[q] && ok && !has[q]) ? 3u : 0u;
                    o7 += full[q] && !ok;
                }
#pragma unroll
                for (uint32_t q = 0; q < KP_P_BATCH; ++q)  // (code <= mask: the entry lies inside the table)
                    p[q] = has[q] ? A.lut[code[q]] : make_int4(KP_P_INVALID, KP_P_INVALID, KP_P_INVALID, KP_P_INVALID);
#pragma unroll
                for (uint32_t q = 0; q < KP_P_BATCH; ++q) {
                    const int32_t id[3] = {p[q].x, p[q].y, p[q].z};
                    const bool counted = full[q] && (info[q] >> 9) != 0u;
#pragma unroll
                    for (uint32_t e = 0; e < 3u; ++e) {
                        const uint32_t cls = (info[q] >> (3u * e)) & 7u;  // 0..4
                        by_class += counted ? 1ull << (8u * cls) : 0ull;
                        if (id[e] >= 0) {  // (< P: the table holds indices of the pattern list only)
                            if (LDS)
                                atomicAdd(&cnt5[cls * A.P + (uint32_t)id[e]], 1u);
                            else
                                atomicAdd(&row[cls * A.P + (uint32_t)id[e]], 1ull);
                        }
                        o6 += id[e] == KP_P_NONE;
                    }
                }
            }
            // 16 bits per counter: a wave holds at most 64 * 96 pairs
            unsigned long long lo4 = (by_class & 0xffull) | ((by_class >> 8 & 0xffull) << 16) | ((by_class >> 16 & 0xffull) << 32) |
                                     ((by_class >> 24 & 0xffull) << 48);
            unsigned long long hi4 = (by_class >> 32 & 0xffull) | ((unsigned long long)o5 << 16) | ((unsigned long long)o6 << 32) |
                                     ((unsigned long long)o7 << 48);
            for (int o = 32; o; o >>= 1) {
                lo4 += __shfl_xor(lo4, o, 64);
                hi4 += __shfl_xor(hi4, o, 64);
            }
            if ((tid & 63u) == 0) {
                unsigned long long *o = A.other + (uint64_t)KP_CD_OTHER * rec.tx;
#pragma unroll
                for (uint32_t e = 0; e < 4u; ++e) {
                    const unsigned long long v = (lo4 >> (16u * e)) & 0xffffull, u = (hi4 >> (16u * e)) & 0xffffull;
                    if (v) atomicAdd(&o[e], v);
                    if (u) atomicAdd(&o[4u + e], u);
                }
            }
        }
        if (LDS) {
            __syncthreads();  // every add of the item is in
            // (a splice interval touches the counters of class 4 only, a segment never those)
            const uint32_t f0 = splice ? KP_CD_SPLICE * A.P : 0u, f1 = splice ? n_cnt : KP_CD_SPLICE * A.P;
            for (uint32_t e = f0 + tid; e < f1; e += KP_S_THREADS) {
                const uint32_t v = cnt5[e];
                if (v) {
                    atomicAdd(&row[e], (unsigned long long)v);
                    cnt5[e] = 0;
                }
            }
            __syncthreads();  // zero again before the next item adds
        }
    }
}

__global__ void __launch_bounds__(256) kp_coding_sites_kernel(kp_cd_sargs A) {
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= A.n_pairs) return;
    const uint32_t t = A.tx[i];
    uint32_t codons = 0, code = 0, slot = 0;
    A.cls[i] = kp_cd_site(A.seq, A.sb, A.se, A.sj0, A.tx_first[t], A.tx_first[t + 1], A.tx_strand[t], A.splice, A.iters,
                          A.pos[i], A.alt[i], &codons);
    A.codons[i] = codons;
    const int rc = kp_sp_site(A.seq, A.n, A.pos[i], A.alt[i], A.k, A.fold, A.mask, &code, &slot);
    A.pid[i] = rc ? rc : A.lut[4ull * code + slot];
}

#endif  // __HIPCC__

// ---------------------------------------------------------------------------
// the calls of a kp_spec session
// ---------------------------------------------------------------------------

// the transcript table of one call, checked; sj0[e] = the spliced index of segment e's first base
static int cd_check_table(const std::string &w, uint64_t n, const uint64_t *sb, const uint64_t *se, uint64_t n_segs,
                          const uint64_t *tx_first, const uint8_t *tx_strand, uint64_t n_tx, uint32_t splice,
                          std::vector<uint64_t> &sj0, uint32_t *iters) {
    if (n_tx >= (1ull << 32) / KP_CD_OTHER) return fail(KP_E_ARG, w + ": 2^29 transcripts or more in one call");
    if (n_segs >= (1ull << 32)) return fail(KP_E_ARG, w + ": 2^32 segments or more in one call");
    if (!tx_first || (n_tx && !tx_strand) || (n_segs && (!sb || !se))) return fail(KP_E_ARG, w + ": null transcript table");
    if (splice > KP_CD_MAX_SPLICE) return fail(KP_E_ARG, w + ": splice must be 0..8");
    if (tx_first[0] != 0 || tx_first[n_tx] != n_segs)
        return fail(KP_E_ARG, w + ": tx_first must run from 0 to the number of segments");
    sj0.resize(n_segs);
    uint64_t most = 0;
    for (uint64_t t = 0; t < n_tx; ++t) {
        if (tx_first[t] > tx_first[t + 1] || tx_first[t + 1] > n_segs)
            return fail(KP_E_ARG, w + ": tx_first is not ascending at transcript " + std::to_string(t));
        if (tx_strand[t] > 1) return fail(KP_E_ARG, w + ": transcript " + std::to_string(t) + " has a strand that is not 0 or 1");
        uint64_t len = 0;
        for (uint64_t e = tx_first[t]; e < tx_first[t + 1]; ++e) {
            if (sb[e] >= se[e] || se[e] > n)
                return fail(KP_E_ARG, w + ": segment " + std::to_string(e - tx_first[t]) + " of transcript " + std::to_string(t) +
                                          " is empty, has begin > end or lies outside the contig");
            if (e > tx_first[t] && sb[e] < se[e - 1])
                return fail(KP_E_ARG, w + ": the segments of transcript " + std::to_string(t) +
                                          " are not ascending and non-overlapping");
            sj0[e] = len;
            len += se[e] - sb[e];
        }
        if (len % 3u)
            return fail(KP_E_ARG, w + ": the segments of transcript " + std::to_string(t) + " hold " + std::to_string(len) +
                                      " bases, not a multiple of 3");
        most = std::max(most, tx_first[t + 1] - tx_first[t]);
    }
    uint32_t it = 1;
    while ((1ull << it) <= most) ++it;
    *iters = it;
    return KP_OK;
}

// the two splice intervals of the intron [a, b), each position once; the second may be empty
static void cd_splice_intervals(uint64_t a, uint64_t b, uint32_t splice, uint64_t iv[4]) {
    iv[0] = a;
    iv[1] = std::min(a + splice, b);
    iv[2] = std::max<uint64_t>(b > splice ? b - splice : 0, iv[1]);
    iv[3] = b;
}

// One position on the host: its pairs into other[8] and, where rated, into row[5][P] (row may be
// NULL if no pair of the position can be rated).  x: the codon (unused for a splice position).
static void cd_host_position(const kp_spec_sess *s, const uint8_t *seq, uint64_t n, uint64_t g, bool splice,
                             const uint32_t x[3], uint32_t i, uint32_t strand, uint64_t *row, uint64_t *other) {
    const uint32_t own = kp_s_class(seq[g]);
    const uint32_t P = (uint32_t)s->pats.size();
    if (splice ? own > 3u : (x[0] | x[1] | x[2]) > 3u) {
        ++other[7];
        return;
    }
    for (uint32_t a = 0; a < 4u; ++a) {
        if (a == own) continue;
        const uint32_t cls = splice ? KP_CD_SPLICE : kp_cd_class(x[0], x[1], x[2], i, a, strand);
        ++other[cls];
        uint32_t code = 0, slot = 0;
        if (kp_sp_site(seq, n, g, (uint32_t)"ACGT"[a], s->k, s->fold, (uint32_t)(s->cells - 1), &code, &slot)) {
            ++other[5];
            continue;
        }
        const int32_t id = s->h_lut[4ull * code + slot];
        if (id < 0)
            ++other[6];
        else
            ++row[(uint64_t)cls * P + (uint32_t)id];
    }
}

static long cd_lds_p() { return env_int("KP_CODING_LDS_P", KP_CD_LDS_P); }

extern "C" {

int kp_spec_coding(kp_ctx *c, const uint8_t *seq, uint64_t n, const uint64_t *seg_begin, const uint64_t *seg_end,
                   uint64_t n_segs, const uint64_t *tx_first, const uint8_t *tx_strand, uint64_t n_tx, uint32_t splice,
                   const double *rates, uint64_t *hist, uint64_t *other, double *expected) {
    kp_spec_sess *s = spec_sess(c);
    int rc = scan_check_contig("kp_spec_coding", s->active, seq, n, "kp_spec_begin");
    if (rc) return rc;
    if (n_tx && !other) return fail(KP_E_ARG, "kp_spec_coding: null counters");
    if (rates && n_tx && !expected) return fail(KP_E_ARG, "kp_spec_coding: rates without a place for the sums");
    std::vector<uint64_t> sj0;
    uint32_t iters = 0;
    try {
        if ((rc = cd_check_table("kp_spec_coding", n, seg_begin, seg_end, n_segs, tx_first, tx_strand, n_tx, splice, sj0,
                                 &iters)))
            return rc;
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_spec_coding: the segment table does not fit host memory");
    }
    s->coding = kp_spec_coding_stats{};
    if (!n_tx) return KP_OK;
    const int k = s->k;
    const uint32_t P = (uint32_t)s->pats.size();
    const uint32_t mask = (uint32_t)(s->cells - 1);
    const uint64_t n_rows = n_tx * KP_CD_CLASSES;
    uint64_t lo = 0, hi = 0;
    scan_centres(n, k, &lo, &hi);
    const uint64_t *sb = seg_begin, *se = seg_end;
    if (!c) {
        std::vector<uint64_t> rows;
        try {
            rows.resize((size_t)KP_CD_CLASSES * P);
        } catch (const std::bad_alloc &) {
            return fail(KP_E_NOMEM, "kp_spec_coding: a transcript's counters do not fit memory");
        }
        uint64_t n_items = 0, positions = 0, pairs = 0;
        for (uint64_t t = 0; t < n_tx; ++t) {
            std::fill(rows.begin(), rows.end(), 0);
            uint64_t *o = other + KP_CD_OTHER * t;
            std::fill(o, o + KP_CD_OTHER, 0);
            const uint64_t t0 = tx_first[t], t1 = tx_first[t + 1];
            for (uint64_t e = t0; e < t1; ++e) {
                for (uint64_t g = sb[e]; g < se[e]; ++g) {
                    uint32_t x[3], i = 0;
                    kp_cd_codon_at(seq, sb, se, t0, t1, e, g, sj0[e] + (g - sb[e]), x, &i);
                    cd_host_position(s, seq, n, g, false, x, i, tx_strand[t], rows.data(), o);
                }
                n_items += scan_pieces(sb[e], se[e], lo, hi);
                positions += se[e] - sb[e];
                if (e + 1 < t1) {
                    uint64_t iv[4];
                    cd_splice_intervals(se[e], sb[e + 1], splice, iv);
                    for (int v = 0; v < 4; v += 2) {
                        for (uint64_t g = iv[v]; g < iv[v + 1]; ++g)
                            cd_host_position(s, seq, n, g, true, nullptr, 0, tx_strand[t], rows.data(), o);
                        n_items += scan_pieces(iv[v], iv[v + 1], lo, hi);
                        positions += iv[v + 1] - iv[v];
                    }
                }
            }
            for (int e = 0; e < KP_CD_CLASSES; ++e) pairs += o[e];
            if (hist) memcpy(hist + t * KP_CD_CLASSES * P, rows.data(), rows.size() * 8);
            if (rates) {
                for (uint32_t cl = 0; cl < KP_CD_CLASSES; ++cl)
                    for (uint32_t ty = 0; ty < KP_SP_TYPES; ++ty) {
                        double acc = 0.0;
                        for (uint32_t e = s->type_off[ty]; e < s->type_off[ty + 1]; ++e)
                            acc = acc + (double)rows[(size_t)cl * P + s->by_type[e]] * rates[s->by_type[e]];
                        expected[(t * KP_CD_CLASSES + cl) * KP_SP_TYPES + ty] = acc;
                    }
            }
        }
        s->coding.items = n_items;
        s->coding.positions = positions;
        s->coding.pairs = pairs;
        return KP_OK;
    }

    KP_HIP(hipSetDevice(c->device));
    const long lds_p = cd_lds_p();
    if (lds_p < 0 || lds_p > KP_CD_LDS_P)
        return fail(KP_E_ARG, "kp_spec_coding: KP_CODING_LDS_P must be 0..3276 (5 P uint32 counters in 64 KiB)");
    const bool lds = env_int("KP_CODING_GLOBAL", 0) == 0 && (long)P <= lds_p;
    std::vector<kp_p_item> items;
    std::vector<kp_cd_rec> recs;
    std::vector<uint64_t> h_other;  // the clipped centres' share, added after the scan
    uint32_t h_tab[KP_CD_TAB_WORDS] = {};
    uint64_t positions = 0;
    try {
        h_other.assign(n_tx * KP_CD_OTHER, 0);
        // the centres of [b, e) whose window leaves the contig: the host's share
        auto clipped = [&](uint64_t b, uint64_t e, auto &&fn) {
            for (uint64_t g = b; g < std::min(e, lo); ++g) fn(g);
            for (uint64_t g = std::max(b, hi); g < e; ++g) fn(g);
        };
        for (uint64_t t = 0; t < n_tx; ++t) {
            const uint64_t t0 = tx_first[t], t1 = tx_first[t + 1];
            uint64_t *o = h_other.data() + KP_CD_OTHER * t;
            for (uint64_t e = t0; e < t1; ++e) {
                kp_cd_rec r;
                r.begin = (uint32_t)sb[e];
                r.len = (uint32_t)(se[e] - sb[e]);
                r.j0 = (uint32_t)(sj0[e] % 3u);
                r.tx = (uint32_t)t;
                r.flags = tx_strand[t] ? KP_CD_F_STRAND : 0u;
                r.ctx = kp_cd_near(seq, sb, se, t0, t1, e, sb[e], -2) | kp_cd_near(seq, sb, se, t0, t1, e, sb[e], -1) << 3 |
                        kp_cd_near(seq, sb, se, t0, t1, e, se[e] - 1, 1) << 6 |
                        kp_cd_near(seq, sb, se, t0, t1, e, se[e] - 1, 2) << 9;
                recs.push_back(r);
                scan_cut(items, sb[e], se[e], lo, hi, (uint32_t)(recs.size() - 1));
                positions += se[e] - sb[e];
                clipped(sb[e], se[e], [&](uint64_t g) {
                    uint32_t x[3], i = 0;
                    kp_cd_codon_at(seq, sb, se, t0, t1, e, g, sj0[e] + (g - sb[e]), x, &i);
                    cd_host_position(s, seq, n, g, false, x, i, tx_strand[t], nullptr, o);
                });
                if (e + 1 < t1) {
                    uint64_t iv[4];
                    cd_splice_intervals(se[e], sb[e + 1], splice, iv);
                    for (int v = 0; v < 4; v += 2) {
                        if (iv[v] >= iv[v + 1]) continue;
                        r.begin = (uint32_t)iv[v];
                        r.len = (uint32_t)(iv[v + 1] - iv[v]);
                        r.j0 = 0;
                        r.flags = (tx_strand[t] ? KP_CD_F_STRAND : 0u) | KP_CD_F_SPLICE;
                        r.ctx = 0;
                        recs.push_back(r);
                        scan_cut(items, iv[v], iv[v + 1], lo, hi, (uint32_t)(recs.size() - 1));
                        positions += iv[v + 1] - iv[v];
                        clipped(iv[v], iv[v + 1],
                                [&](uint64_t g) { cd_host_position(s, seq, n, g, true, nullptr, 0, tx_strand[t], nullptr, o); });
                    }
                }
            }
        }
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_spec_coding: the work items do not fit host memory");
    }
    if (items.size() >= (1ull << 32) || recs.size() >= (1ull << 32))
        return fail(KP_E_ARG, "kp_spec_coding: 2^32 work items or more in one call");
    for (uint32_t e = 0; e < 4u * KP_CD_TAB_WORDS; ++e) h_tab[e >> 2] |= kp_cd_tab_byte(e / 3u, e % 3u) << (8u * (e & 3u));
    const size_t cnts = (size_t)n_rows * P;
    const size_t b_hist = g_up(cnts * 8), b_other = g_up(n_tx * KP_CD_OTHER * 8);
    const size_t b_rates = rates ? g_up((size_t)P * 8) + g_up((size_t)P * 4) : 0;
    const size_t b_exp = rates ? g_up(n_rows * KP_SP_TYPES * 8) : 0;
    if ((rc = spec_arena(c, "kp_spec_coding", b_hist + b_other + b_rates + b_exp))) return rc;
    unsigned long long *d_hist = (unsigned long long *)c->arena.take(cnts * 8);
    unsigned long long *d_other = (unsigned long long *)c->arena.take(n_tx * KP_CD_OTHER * 8);
    double *d_rates = rates ? (double *)c->arena.take((size_t)P * 8) : nullptr;
    uint32_t *d_type = rates ? (uint32_t *)c->arena.take((size_t)P * 4) : nullptr;
    double *d_exp = rates ? (double *)c->arena.take(n_rows * KP_SP_TYPES * 8) : nullptr;
    if ((rc = c->arena.check("kp_spec_coding"))) return rc;
    hipStream_t st = c->stream;
    KP_HIP(hipMemsetAsync(d_hist, 0, cnts * 8, st));
    KP_HIP(hipMemsetAsync(d_other, 0, n_tx * KP_CD_OTHER * 8, st));
    if (!items.empty()) {
        const size_t b_recs = g_up(recs.size() * sizeof(kp_cd_rec)), b_tab = g_up(sizeof h_tab);
        uint8_t *d_seq = nullptr;
        kp_p_item *d_items = nullptr;
        if ((rc = scan_upload(c, "kp_spec_coding", seq, n, items, b_recs + b_tab, &d_seq, &d_items))) return rc;
        kp_cd_rec *d_recs = (kp_cd_rec *)c->seq_in.take(b_recs);
        uint32_t *d_tab = (uint32_t *)c->seq_in.take(b_tab);
        if ((rc = c->seq_in.check("kp_spec_coding"))) return rc;
        KP_HIP(hipMemcpyAsync(d_recs, recs.data(), recs.size() * sizeof(kp_cd_rec), hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(d_tab, h_tab, sizeof h_tab, hipMemcpyHostToDevice, st));
        const size_t lds_bytes = 4u * KP_CD_TAB_WORDS + (lds ? (size_t)KP_CD_CLASSES * P * 4 : 0);
        const uint64_t grid = scan_grid(c, items.size(), scan_per_cu(lds_bytes), "KP_CODING_GRID");
        kp_cd_args A;
        A.seq = d_seq;
        A.n = (uint32_t)n;
        A.items = d_items;
        A.recs = d_recs;
        A.tab = d_tab;
        A.n_items = (uint32_t)items.size();
        A.steps = (uint32_t)((items.size() + grid - 1) / grid);
        A.k = k;
        A.fold = s->fold;
        A.mask = mask;
        A.P = P;
        A.lut = (const int4 *)s->d_lut;
        A.hist = d_hist;
        A.other = d_other;
        if (lds_bytes > 65536)
            KP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&kp_coding_scan_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        if ((rc = scan_mark(c, 0))) return rc;
        if (lds)
            hipLaunchKernelGGL((kp_coding_scan_kernel<true>), dim3((unsigned)grid), dim3(KP_S_THREADS), lds_bytes, st, A);
        else
            hipLaunchKernelGGL((kp_coding_scan_kernel<false>), dim3((unsigned)grid), dim3(KP_S_THREADS), lds_bytes, st, A);
        if ((rc = scan_launched(c, 1))) return rc;
    }
    if (rates) {
        KP_HIP(hipMemcpyAsync(d_rates, rates, (size_t)P * 8, hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(d_type, s->by_type.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
        kp_sp_offs T;
        memcpy(T.off, s->type_off, sizeof T.off);
        hipLaunchKernelGGL(kp_spec_sums_kernel, dim3((unsigned)((n_rows * KP_SP_TYPES + 63) / 64)), dim3(64), 0, st, d_hist,
                           d_rates, d_type, T, P, n_rows, d_exp);
        KP_HIP(hipGetLastError());
        KP_HIP(hipMemcpyAsync(expected, d_exp, n_rows * KP_SP_TYPES * 8, hipMemcpyDeviceToHost, st));
    }
    if (hist) KP_HIP(hipMemcpyAsync(hist, d_hist, cnts * 8, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(other, d_other, n_tx * KP_CD_OTHER * 8, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    if (!items.empty()) {
        float ms = 0.f;
        if ((rc = scan_elapsed(c, 0, 1, &ms))) return rc;
        s->coding.scan_ms = ms;
        s->coding.path = lds ? 1u : 2u;
    }
    uint64_t pairs = 0;
    for (uint64_t t = 0; t < n_tx; ++t)
        for (int e = 0; e < KP_CD_OTHER; ++e) {
            other[KP_CD_OTHER * t + e] += h_other[KP_CD_OTHER * t + e];
            if (e < KP_CD_CLASSES) pairs += other[KP_CD_OTHER * t + e];
        }
    s->coding.items = items.size();
    s->coding.positions = positions;
    s->coding.pairs = pairs;
    return KP_OK;
}

int kp_spec_coding_sites(kp_ctx *c, const uint8_t *seq, uint64_t n, const uint64_t *seg_begin, const uint64_t *seg_end,
                         uint64_t n_segs, const uint64_t *tx_first, const uint8_t *tx_strand, uint64_t n_tx,
                         uint32_t splice, const uint64_t *pos, const uint8_t *alt, const uint32_t *tx, uint64_t n_pairs,
                         int32_t *cls, int32_t *pid, uint32_t *codons) {
    kp_spec_sess *s = spec_sess(c);
    int rc = scan_check_contig("kp_spec_coding_sites", s->active, seq, n, "kp_spec_begin");
    if (rc) return rc;
    std::vector<uint64_t> sj0;
    uint32_t iters = 0;
    try {
        if ((rc = cd_check_table("kp_spec_coding_sites", n, seg_begin, seg_end, n_segs, tx_first, tx_strand, n_tx, splice,
                                 sj0, &iters)))
            return rc;
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_spec_coding_sites: the segment table does not fit host memory");
    }
    if ((rc = spec_check_sites("kp_spec_coding_sites", n, pos, alt, n_pairs))) return rc;
    if (n_pairs && !tx) return fail(KP_E_ARG, "kp_spec_coding_sites: null transcripts of the pairs");
    for (uint64_t i = 0; i < n_pairs; ++i)
        if (tx[i] >= n_tx)
            return fail(KP_E_ARG, "kp_spec_coding_sites: pair " + std::to_string(i) + " names transcript " +
                                      std::to_string(tx[i]) + " of " + std::to_string(n_tx));
    if (!n_pairs) return KP_OK;
    if (!cls || !pid || !codons) return fail(KP_E_ARG, "kp_spec_coding_sites: null output");
    const int k = s->k;
    const uint32_t mask = (uint32_t)(s->cells - 1);
    if (!c) {
        for (uint64_t i = 0; i < n_pairs; ++i) {
            const uint32_t t = tx[i];
            cls[i] = kp_cd_site(seq, seg_begin, seg_end, sj0.data(), tx_first[t], tx_first[t + 1], tx_strand[t], splice, iters,
                                pos[i], alt[i], &codons[i]);
            uint32_t code = 0, slot = 0;
            const int r = kp_sp_site(seq, n, pos[i], alt[i], k, s->fold, mask, &code, &slot);
            pid[i] = r ? r : s->h_lut[4ull * code + slot];
        }
        return KP_OK;
    }
    KP_HIP(hipSetDevice(c->device));
    if ((rc = spec_arena(c, "kp_spec_coding_sites", 3 * g_up(n_pairs * 4)))) return rc;
    int32_t *d_cls = (int32_t *)c->arena.take(n_pairs * 4);
    int32_t *d_pid = (int32_t *)c->arena.take(n_pairs * 4);
    uint32_t *d_cod = (uint32_t *)c->arena.take(n_pairs * 4);
    if ((rc = c->arena.check("kp_spec_coding_sites"))) return rc;
    uint8_t *d_seq = nullptr;
    const size_t more = 3 * g_up(n_segs * 8) + g_up((n_tx + 1) * 8) + g_up(n_tx) + g_up(n_pairs * 8) + g_up(n_pairs) +
                        g_up(n_pairs * 4);
    if ((rc = scan_upload(c, "kp_spec_coding_sites", seq, n, {}, more, &d_seq, nullptr))) return rc;
    uint64_t *d_sb = (uint64_t *)c->seq_in.take(n_segs * 8);
    uint64_t *d_se = (uint64_t *)c->seq_in.take(n_segs * 8);
    uint64_t *d_sj = (uint64_t *)c->seq_in.take(n_segs * 8);
    uint64_t *d_first = (uint64_t *)c->seq_in.take((n_tx + 1) * 8);
    uint8_t *d_strand = (uint8_t *)c->seq_in.take(n_tx);
    uint64_t *d_pos = (uint64_t *)c->seq_in.take(n_pairs * 8);
    uint8_t *d_alt = (uint8_t *)c->seq_in.take(n_pairs);
    uint32_t *d_tx = (uint32_t *)c->seq_in.take(n_pairs * 4);
    if ((rc = c->seq_in.check("kp_spec_coding_sites"))) return rc;
    hipStream_t st = c->stream;
    if (n_segs) {
        KP_HIP(hipMemcpyAsync(d_sb, seg_begin, n_segs * 8, hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(d_se, seg_end, n_segs * 8, hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(d_sj, sj0.data(), n_segs * 8, hipMemcpyHostToDevice, st));
    }
    KP_HIP(hipMemcpyAsync(d_first, tx_first, (n_tx + 1) * 8, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_strand, tx_strand, n_tx, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_pos, pos, n_pairs * 8, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_alt, alt, n_pairs, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(d_tx, tx, n_pairs * 4, hipMemcpyHostToDevice, st));
    kp_cd_sargs A;
    A.seq = d_seq;
    A.n = n;
    A.sb = d_sb;
    A.se = d_se;
    A.sj0 = d_sj;
    A.tx_first = d_first;
    A.tx_strand = d_strand;
    A.splice = splice;
    A.iters = iters;
    A.pos = d_pos;
    A.alt = d_alt;
    A.tx = d_tx;
    A.n_pairs = n_pairs;
    A.k = k;
    A.fold = s->fold;
    A.mask = mask;
    A.lut = s->d_lut;
    A.cls = d_cls;
    A.pid = d_pid;
    A.codons = d_cod;
    hipLaunchKernelGGL(kp_coding_sites_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, A);
    KP_HIP(hipGetLastError());
    KP_HIP(hipMemcpyAsync(cls, d_cls, n_pairs * 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(pid, d_pid, n_pairs * 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(codons, d_cod, n_pairs * 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    return KP_OK;
}

int kp_spec_last_coding(kp_ctx *c, kp_spec_coding_stats *out) {
    if (!out) return fail(KP_E_ARG, "kp_spec_last_coding: null out");
    *out = spec_sess(c)->coding;
    return KP_OK;
}

}  // extern "C"
