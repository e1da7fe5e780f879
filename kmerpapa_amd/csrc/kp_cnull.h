// kp_cnull.h -- null tables per transcript by coding consequence: many replicates of
// kp_spec_simulate's draw, each hit classed as kp_spec_coding_sites classes it and counted in its
// transcript's row (no reference counterpart).  Included by kp_hip.hip after kp_null.h and
// kp_coding.h.  Semantics: include/kmerpapa_hip.h.
//
// Both halves exist as __host__ __device__ functions: the draw is kp_null.h's (kp_nl_thresh /
// round1 / bits / pick over kp_sm_cum of the window's table entry), the class of a (position,
// forward ALT) pair is kp_coding.h's (kp_cd_codons / kp_cd_class_of, kp_cd_is_splice).  The host
// session runs them serially per transcript, position and replicate.  On the device the work that
// does not depend on the replicate is done once and kept apart from the draws:
//
//   kp_cnull_stage_kernel  one thread per (transcript, position) record.  A binary search with a
//                          host-computed number of steps over the items' dense record offsets finds
//                          the thread's segment or splice interval (a kp_cd_rec, as the coding scan's);
//                          the thread reads its own window (kp_p_window), gathers the table entry and
//                          the three rates, and writes one 32-byte record: the integer thresholds
//                          T0 <= T1 <= T2 (T2 = 0: draws nothing), the position and the class of each
//                          slot (3 bits each, 7 = none).  The codon comes from the position's
//                          neighbours inside the segment and from the record's four context bytes at
//                          its ends.  A record's address is the item's base plus the index inside the
//                          item: no atomics, no compaction, a transcript's records are contiguous.
//                          One thread per position rather than the scan's roll: a record costs k byte
//                          loads instead of one, but an item of two splice bases costs two threads
//                          instead of a workgroup's roll over 8,192 mostly empty windows.
//   kp_cnull_draw_kernel   a persistent grid over (piece of a transcript's records, replicate chunk)
//                          units.  A wave reads its records with wave-uniform loads; its 64 lanes hold
//                          consecutive replicates.  kp_nl_round1 runs once per record on the scalar
//                          unit, kp_nl_bits once per lane.  A lane owns its replicate, so the five
//                          class counters are 12-bit fields of one 64-bit register (a piece holds at
//                          most KP_CN_PIECE = 4,095 records) and leave with one global atomic per
//                          non-zero (transcript, replicate, class).  A chunk holds at most KP_CN_REPS =
//                          256 replicates, one per thread; with 128 or fewer the four waves split the
//                          piece's records two or four ways instead of idling.  No LDS, no barrier.
//
// Every device loop has a bound the host computed; there are no waits between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "kp_coding.h"
#include "kp_null.h"

#define KP_CN_THREADS 256
#define KP_CN_REPS 256     // replicates of a chunk at most: one per thread of the draw kernel
#define KP_CN_PIECE 4095u  // records of a unit at most: a lane's class counters are 12-bit fields
#define KP_CN_NONE 7u      // the class of a slot without one

struct kp_cn_rec {
    uint64_t t0, t1, t2;  // kp_nl_thresh of c0 <= c1 <= c2; t2 = 0: the position draws nothing
    uint32_t pos;
    uint32_t cls;  // 3 bits per slot: 0..4, KP_CN_NONE
};

struct kp_cn_piece {
    uint64_t rec0;  // the first record
    uint32_t count, tx;
};

// the classes of the three slots of a position with REF class own (0..3): x = its codon in genomic
// order and i its place (a coding position), or splice
__host__ __device__ inline uint32_t kp_cn_classes(uint32_t own, bool splice, const uint32_t x[3], uint32_t i,
                                                  uint32_t strand, int fold) {
    uint32_t bits = 0;
    const bool none = !splice && (x[0] | x[1] | x[2]) > 3u;
    for (uint32_t e = 0; e < 3u; ++e) {
        uint32_t cls = KP_CD_SPLICE;
        if (none) {
            cls = KP_CN_NONE;
        } else if (!splice) {
            uint32_t rc = 0, ac = 0;
            kp_cd_codons(x[0], x[1], x[2], i, kp_sm_alt(own, fold, e), strand, &rc, &ac);
            cls = kp_cd_class_of(rc, ac);
        }
        bits |= cls << (3u * e);
    }
    return bits;
}

struct kp_cn_sargs {
    const uint8_t *seq;  // the contig, KP_S_PAD readable bytes past its end
    uint64_t n;
    const kp_cd_rec *items;  // [n_items]: segments and splice intervals, transcript by transcript
    const uint64_t *rec0;    // [n_items]: the dense offset of the item's first record, ascending
    uint64_t n_items, n_recs;
    uint32_t iters, steps;  // 2^iters > n_items; steps * grid * KP_CN_THREADS >= n_recs
    int32_t k, fold;
    uint32_t mask;
    const int4 *lut;
    const double *rates;
    double scale;
    kp_cn_rec *recs;           // [n_recs]
    unsigned long long *stat;  // [0] += records with t2 > 0
};

struct kp_cn_dargs {
    const kp_cn_rec *recs;
    const kp_cn_piece *pieces;  // [n_units / passes]
    uint64_t n_units, steps;    // units = (piece, pass) pairs, piece-major
    uint64_t seed;
    uint32_t contig, rep_first, n_reps;
    uint32_t rc, passes;       // replicates per pass (<= KP_CN_REPS), passes = ceil(n_reps / rc)
    uint32_t *counts;          // [n_tx][n_reps][5]
    unsigned long long *stat;  // [1] += hits without a class
};

#ifdef __HIPCC__

__global__ void __launch_bounds__(KP_CN_THREADS) kp_cnull_stage_kernel(kp_cn_sargs A) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t s = 0; s < A.steps; ++s) {
        const uint64_t r = ((uint64_t)s * gridDim.x + blockIdx.x) * KP_CN_THREADS + threadIdx.x;
        const bool live = r < A.n_recs;
        bool draws = false;
        if (live) {
            uint64_t lo = 0, hi = A.n_items;  // the first item that begins after record r
            for (uint32_t it = 0; it < A.iters && lo < hi; ++it) {
                const uint64_t m = lo + (hi - lo) / 2u;
                if (A.rec0[m] > r)
                    hi = m;
                else
                    lo = m + 1u;
            }
            // (rec0[0] = 0 <= r, so lo >= 1; r - rec0 < the item's len as r < n_recs)
            const kp_cd_rec rec = A.items[lo - 1u];
            const uint32_t q = (uint32_t)(r - A.rec0[lo - 1u]);
            const uint64_t g = (uint64_t)rec.begin + q;  // < n: the item lies inside the contig
            const bool splice = (rec.flags & KP_CD_F_SPLICE) != 0u;
            kp_cn_rec out{0ull, 0ull, 0ull, (uint32_t)g, 0u};
            uint32_t code = 0;
            if (kp_p_window(A.seq, A.n, g, A.k, A.fold, A.mask, &code)) {
                const int4 p = A.lut[code];  // (code <= mask: the entry lies inside the table)
                double c[3];
                kp_sm_cum(p.x, p.y, p.z, A.rates, A.scale, c);  // (ids < P)
                if (c[2] > 0.0) {
                    uint32_t x[3] = {0u, 0u, 0u};
                    const uint32_t i = (rec.j0 + q) % 3u;
                    if (!splice) {
                        for (int e = 0; e < 3; ++e) {  // the spliced bytes q - i .. q - i + 2 of the segment
                            const int64_t qd = (int64_t)q + e - (int64_t)i;
                            const bool inside = qd >= 0 && qd < (int64_t)rec.len;
                            const int64_t at = qd < 0 ? 2 + qd : 2 + qd - (int64_t)rec.len;  // 0..3 outside
                            x[e] = inside ? kp_s_class(A.seq[(uint64_t)rec.begin + (uint64_t)qd])
                                          : (rec.ctx >> (3u * ((uint32_t)at & 3u))) & 7u;
                        }
                    }
                    out.t0 = kp_nl_thresh(c[0]);
                    out.t1 = kp_nl_thresh(c[1]);
                    out.t2 = kp_nl_thresh(c[2]);
                    // (the window is valid, so the centre is a base)
                    out.cls = kp_cn_classes(kp_s_class(A.seq[g]) & 3u, splice, x, i, rec.flags & KP_CD_F_STRAND, A.fold);
                    draws = true;
                }
            }
            A.recs[r] = out;
        }
        const unsigned long long b = __ballot(draws);
        if (lane == 0 && b) atomicAdd(&A.stat[0], (unsigned long long)__popcll(b));
    }
}

__global__ void __launch_bounds__(KP_CN_THREADS) kp_cnull_draw_kernel(kp_cn_dargs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint64_t s = 0; s < A.steps; ++s) {
        const uint64_t unit = s * gridDim.x + blockIdx.x;
        if (unit >= A.n_units) break;
        const uint32_t pass = (uint32_t)(unit % A.passes);
        const kp_cn_piece pc = A.pieces[unit / A.passes];
        const uint32_t j0 = pass * A.rc;               // the chunk's first column (< n_reps)
        const uint32_t rc = min(A.rc, A.n_reps - j0);  // and its columns, 1..KP_CN_REPS
        const uint32_t rep0 = A.rep_first + j0;        // (rep_first + n_reps <= 2^32)
        // groups of 64 replicates, and the waves that share a group's records
        const uint32_t groups = (rc + 63u) / 64u, split = (KP_CN_THREADS / 64u) / groups;
        const uint32_t grp = wv / split, part = wv % split;
        if (grp >= groups) continue;  // (three groups leave the fourth wave without work)
        const uint32_t j = grp * 64u + lane;
        const bool active = j < rc;
        unsigned long long cnt = 0;  // 12 bits per class: at most KP_CN_PIECE hits
        uint32_t unc = 0;
        const kp_cn_rec *recs = A.recs + pc.rec0;
        kp_cn_rec next = part < pc.count ? recs[part] : kp_cn_rec{0ull, 0ull, 0ull, 0u, 0u};
        for (uint32_t e = part; e < pc.count; e += split) {  // (e is the same for the whole wave)
            const kp_cn_rec cur = next;
            if (e + split < pc.count) next = recs[e + split];  // in flight during this record's rounds
            const uint64_t t2 = kp_nl_uniform64(cur.t2);
            if (t2 == 0) continue;
            const uint64_t t0 = kp_nl_uniform64(cur.t0), t1 = kp_nl_uniform64(cur.t1);
            const uint32_t pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur.pos);
            const uint32_t bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur.cls);
            const kp_nl_head hd = kp_nl_round1(A.seed, A.contig, pos);
            const uint32_t slot = kp_nl_pick(kp_nl_bits(hd, rep0 + j, A.seed), t0, t1, t2);
            if (active && slot < 3u) {
                const uint32_t cls = (bits >> (3u * slot)) & 7u;
                if (cls < (uint32_t)KP_CD_CLASSES)
                    cnt += 1ull << (12u * cls);
                else
                    ++unc;
            }
        }
        // j < rc: the cell lies inside row pc.tx of the table
        uint32_t *cell = A.counts + ((uint64_t)pc.tx * A.n_reps + j0 + j) * KP_CD_CLASSES;
#pragma unroll
        for (uint32_t cl = 0; cl < (uint32_t)KP_CD_CLASSES; ++cl) {
            const uint32_t v = (uint32_t)(cnt >> (12u * cl)) & 0xfffu;
            if (v) atomicAdd(&cell[cl], v);  // (cnt is 0 in a lane that is not active)
        }
        for (int o = 32; o; o >>= 1) unc += __shfl_xor(unc, o, 64);
        if (lane == 0 && unc) atomicAdd(&A.stat[1], (unsigned long long)unc);
    }
}

#endif  // __HIPCC__

// ---------------------------------------------------------------------------
// the call, in a kp_spec session
// ---------------------------------------------------------------------------

extern "C" {

int kp_spec_coding_null(kp_ctx *c, const uint8_t *seq, uint64_t n, uint32_t contig_id, const uint64_t *seg_begin,
                        const uint64_t *seg_end, uint64_t n_segs, const uint64_t *tx_first, const uint8_t *tx_strand,
                        uint64_t n_tx, uint32_t splice, const double *rates, double scale, uint64_t seed, uint32_t rep_first,
                        uint32_t n_reps, uint32_t *counts) {
    const char *who = "kp_spec_coding_null";
    kp_spec_sess *s = spec_sess(c);
    int rc = scan_check_contig(who, s->active, seq, n, "kp_spec_begin");
    if (rc) return rc;
    if (!counts) return fail(KP_E_ARG, "kp_spec_coding_null: null counts");
    if (!rates) return fail(KP_E_ARG, "kp_spec_coding_null: null rates");
    if (n_reps == 0) return fail(KP_E_ARG, "kp_spec_coding_null: no replicates");
    if ((uint64_t)rep_first + n_reps > (1ull << 32))
        return fail(KP_E_ARG, "kp_spec_coding_null: replicates " + std::to_string(rep_first) + " .. " +
                                  std::to_string((uint64_t)rep_first + n_reps - 1) + " go past 2^32 - 1");
    if ((rc = sim_check_rates(s, rates, scale))) return rc;
    std::vector<uint64_t> sj0;
    uint32_t iters = 0;
    try {
        if ((rc = cd_check_table(who, n, seg_begin, seg_end, n_segs, tx_first, tx_strand, n_tx, splice, sj0, &iters)))
            return rc;
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_spec_coding_null: the segment table does not fit host memory");
    }
    s->cnull = kp_spec_coding_null_stats{};
    if (!n_tx) return KP_OK;
    const int k = s->k;
    const uint32_t P = (uint32_t)s->pats.size();
    const uint32_t mask = (uint32_t)(s->cells - 1);
    const uint64_t *sb = seg_begin, *se = seg_end;
    const size_t n_cnt = (size_t)n_tx * n_reps * KP_CD_CLASSES;
    if (!c) {
        memset(counts, 0, n_cnt * 4);
        uint64_t positions = 0, drawing = 0, hits = 0, unclassed = 0;
        for (uint64_t t = 0; t < n_tx; ++t) {
            const uint64_t t0 = tx_first[t], t1 = tx_first[t + 1];
            uint32_t *row = counts + t * n_reps * KP_CD_CLASSES;
            auto position = [&](uint64_t e, uint64_t g, bool spl) {
                ++positions;
                uint32_t code = 0;
                if (!kp_p_window(seq, n, g, k, s->fold, mask, &code)) return;
                const int32_t *id = &s->h_lut[4ull * code];
                double cum[3];
                kp_sm_cum(id[0], id[1], id[2], rates, scale, cum);
                if (!(cum[2] > 0.0)) return;
                ++drawing;
                uint32_t x[3] = {0u, 0u, 0u}, i = 0;
                if (!spl) kp_cd_codon_at(seq, sb, se, t0, t1, e, g, sj0[e] + (g - sb[e]), x, &i);
                const uint32_t bits = kp_cn_classes(kp_s_class(seq[g]) & 3u, spl, x, i, tx_strand[t], s->fold);
                const uint64_t th0 = kp_nl_thresh(cum[0]), th1 = kp_nl_thresh(cum[1]), th2 = kp_nl_thresh(cum[2]);
                const kp_nl_head hd = kp_nl_round1(seed, contig_id, g);
                for (uint32_t j = 0; j < n_reps; ++j) {
                    const uint32_t slot = kp_nl_pick(kp_nl_bits(hd, rep_first + j, seed), th0, th1, th2);
                    if (slot >= 3u) continue;
                    const uint32_t cls = (bits >> (3u * slot)) & 7u;
                    if (cls >= (uint32_t)KP_CD_CLASSES) {
                        ++unclassed;
                        continue;
                    }
                    ++row[(size_t)j * KP_CD_CLASSES + cls];
                    ++hits;
                }
            };
            for (uint64_t e = t0; e < t1; ++e) {
                for (uint64_t g = sb[e]; g < se[e]; ++g) position(e, g, false);
                if (e + 1 < t1) {
                    uint64_t iv[4];
                    cd_splice_intervals(se[e], sb[e + 1], splice, iv);
                    for (int v = 0; v < 4; v += 2)
                        for (uint64_t g = iv[v]; g < iv[v + 1]; ++g) position(e, g, true);
                }
            }
        }
        s->cnull.positions = positions;
        s->cnull.drawing = drawing;
        s->cnull.hits = hits;
        s->cnull.unclassed = unclassed;
        s->cnull.passes = 1;
        s->cnull.reps_per_pass = n_reps;
        return KP_OK;
    }

    KP_HIP(hipSetDevice(c->device));
    const long reps_env = env_int("KP_CNULL_REPS", 0);
    uint32_t chunk = std::min<uint32_t>(n_reps, (uint32_t)KP_CN_REPS);
    if (reps_env > 0) chunk = (uint32_t)std::min<long>(chunk, reps_env);
    const uint32_t passes = (n_reps + chunk - 1) / chunk;
    s->cnull.passes = passes;
    s->cnull.reps_per_pass = chunk;
    std::vector<kp_cd_rec> items;
    std::vector<uint64_t> rec0;
    std::vector<kp_cn_piece> pieces;
    uint64_t n_recs = 0;
    try {
        for (uint64_t t = 0; t < n_tx; ++t) {
            const uint64_t t0 = tx_first[t], t1 = tx_first[t + 1];
            const uint64_t first = n_recs;
            auto item = [&](const kp_cd_rec &r) {
                items.push_back(r);
                rec0.push_back(n_recs);
                n_recs += r.len;
            };
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
                item(r);
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
                        item(r);
                    }
                }
            }
            for (uint64_t f = first; f < n_recs; f += KP_CN_PIECE)
                pieces.push_back(kp_cn_piece{f, (uint32_t)std::min<uint64_t>(KP_CN_PIECE, n_recs - f), (uint32_t)t});
        }
    } catch (const std::bad_alloc &) {
        return fail(KP_E_NOMEM, "kp_spec_coding_null: the work items do not fit host memory");
    }
    if (items.size() >= (1ull << 32) || pieces.size() >= (1ull << 32))
        return fail(KP_E_ARG, "kp_spec_coding_null: 2^32 work items or more in one call");
    s->cnull.positions = n_recs;
    const size_t b_cnt = g_up(n_cnt * 4), b_recs = g_up((size_t)n_recs * sizeof(kp_cn_rec));
    if ((rc = spec_arena(c, who, b_cnt + b_recs + g_up((size_t)P * 8) + g_up(16)))) return rc;
    uint32_t *d_counts = (uint32_t *)c->arena.take(n_cnt * 4);
    kp_cn_rec *d_recs = (kp_cn_rec *)c->arena.take((size_t)n_recs * sizeof(kp_cn_rec));
    double *d_rates = (double *)c->arena.take((size_t)P * 8);
    unsigned long long *d_stat = (unsigned long long *)c->arena.take(16);
    if ((rc = c->arena.check(who))) return rc;
    hipStream_t st = c->stream;
    KP_HIP(hipMemsetAsync(d_counts, 0, n_cnt * 4, st));
    KP_HIP(hipMemsetAsync(d_stat, 0, 16, st));
    if (n_recs) {
        const size_t b_items = g_up(items.size() * sizeof(kp_cd_rec)), b_rec0 = g_up(rec0.size() * 8);
        const size_t b_pieces = g_up(pieces.size() * sizeof(kp_cn_piece));
        uint8_t *d_seq = nullptr;
        if ((rc = scan_upload(c, who, seq, n, {}, b_items + b_rec0 + b_pieces, &d_seq, nullptr))) return rc;
        kp_cd_rec *d_items = (kp_cd_rec *)c->seq_in.take(b_items);
        uint64_t *d_rec0 = (uint64_t *)c->seq_in.take(b_rec0);
        kp_cn_piece *d_pieces = (kp_cn_piece *)c->seq_in.take(b_pieces);
        if ((rc = c->seq_in.check(who))) return rc;
        KP_HIP(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(kp_cd_rec), hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(d_rec0, rec0.data(), rec0.size() * 8, hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(d_pieces, pieces.data(), pieces.size() * sizeof(kp_cn_piece), hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(d_rates, rates, (size_t)P * 8, hipMemcpyHostToDevice, st));
        kp_cn_sargs S;
        S.seq = d_seq;
        S.n = n;
        S.items = d_items;
        S.rec0 = d_rec0;
        S.n_items = items.size();
        S.n_recs = n_recs;
        S.iters = 1;
        while ((1ull << S.iters) <= items.size()) ++S.iters;
        S.k = k;
        S.fold = s->fold;
        S.mask = mask;
        S.lut = (const int4 *)s->d_lut;
        S.rates = d_rates;
        S.scale = scale;
        S.recs = d_recs;
        S.stat = d_stat;
        const uint64_t s_blocks = (n_recs + KP_CN_THREADS - 1) / KP_CN_THREADS, s_grid = scan_grid(c, s_blocks, 8, "KP_CNULL_GRID");  // no LDS
        const uint64_t s_steps = (s_blocks + s_grid - 1) / s_grid;
        if (s_steps >= (1ull << 32)) return fail(KP_E_ARG, "kp_spec_coding_null: too many positions for this grid");
        S.steps = (uint32_t)s_steps;
        kp_cn_dargs D;
        D.recs = d_recs;
        D.pieces = d_pieces;
        D.n_units = (uint64_t)pieces.size() * passes;
        D.seed = seed;
        D.contig = contig_id;
        D.rep_first = rep_first;
        D.n_reps = n_reps;
        D.rc = chunk;
        D.passes = passes;
        D.counts = d_counts;
        D.stat = d_stat;
        const uint64_t d_grid = scan_grid(c, D.n_units, 8, "KP_CNULL_GRID");
        D.steps = (D.n_units + d_grid - 1) / d_grid;
        if ((rc = scan_mark(c, 0))) return rc;
        hipLaunchKernelGGL(kp_cnull_stage_kernel, dim3((unsigned)s_grid), dim3(KP_CN_THREADS), 0, st, S);
        if ((rc = scan_launched(c, 1))) return rc;
        hipLaunchKernelGGL(kp_cnull_draw_kernel, dim3((unsigned)d_grid), dim3(KP_CN_THREADS), 0, st, D);
        if ((rc = scan_launched(c, 2))) return rc;
    }
    unsigned long long stat[2] = {0, 0};
    KP_HIP(hipMemcpyAsync(counts, d_counts, n_cnt * 4, hipMemcpyDeviceToHost, st));
    KP_HIP(hipMemcpyAsync(stat, d_stat, 16, hipMemcpyDeviceToHost, st));
    KP_HIP(hipStreamSynchronize(st));
    if (n_recs) {
        float ms = 0.f;
        if ((rc = scan_elapsed(c, 0, 1, &ms))) return rc;
        s->cnull.stage_ms = ms;
        if ((rc = scan_elapsed(c, 1, 2, &ms))) return rc;
        s->cnull.draw_ms = ms;
    }
    uint64_t hits = 0;
    for (size_t i = 0; i < n_cnt; ++i) hits += counts[i];
    s->cnull.drawing = stat[0];
    s->cnull.hits = hits;
    s->cnull.unclassed = stat[1];
    return KP_OK;
}

int kp_spec_last_coding_null(kp_ctx *c, kp_spec_coding_null_stats *out) {
    if (!out) return fail(KP_E_ARG, "kp_spec_last_coding_null: null out");
    *out = spec_sess(c)->cnull;
    return KP_OK;
}

}  // extern "C"
