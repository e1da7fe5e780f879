// kp_scan.h -- what the genome scans share (kp_pred.h, kp_spec.h, kp_sim.h, kp_null.h, kp_coding.h,
// kp_cnull.h).  Included by kp_hip.hip after kp_seq.h, whose windows (kp_s_class / kp_s_step /
// kp_s_code) and tile this builds on; the check of a contig and the persistent grid, which
// kp_seq.h needs too, are kp_rt.h's (scan_check_contig, scan_grid).
//
// Device side, pieces of a kernel, never a kernel:
//   kp_p_load      the four aligned 16-byte words that hold a thread's bytes
//   kp_scan_batch  KP_P_BATCH steps of the roll: the codes, which of them are valid windows, and the
//                  complete but invalid ones counted.  Both pred and both spec kernels use it and
//                  compile to the instructions they had with the loop written out.  The other rolls
//                  stay where they are: kp_sim_roll keeps the REF as read beside each code,
//                  kp_null_kernel's batch loop is rolled, so its bytes come from a select chain, and
//                  kp_coding_scan_kernel rolls over [w0, wend) inside a wider halo, two bytes ahead.
// The per-thread prologue around kp_p_load, the track kernels' write-out, the LDS counter flush and
// the wave sum are written out in each kernel: as helpers they change the kernels' instructions
// (profiles/refactor_scan/asm_compare.txt).
//
// Host side: the centres of a contig, a region clipped to them and cut into items of KP_S_TILE, the
// check of a list of regions, the upload of contig and items, the arena of a table session, and
// the events around a timed launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp_rt.h"
#include "kp_seq.h"

#define KP_P_BATCH 8  // bytes of the roll whose gathers are issued together
#define KP_P_ROW 257  // a track kernel's LDS row: KP_S_THREADS + 1, so a thread's slots spread over the banks

struct kp_p_item {
    uint32_t first, count, region;  // centres [first, first + count) of the region's row
};

// the four aligned 16-byte words that hold bytes [s0, s0 + len) of the contig, len <= 46; a thread
// with len = 0 loads nothing: its s0 may lie far past the contig.  With len > 0, s0 + len <= n,
// so every word loaded begins before n and ends before n + 15 < n + KP_S_PAD.
__device__ inline void kp_p_load(const uint8_t *seq, uint64_t s0, uint32_t len, uint32_t d[16], uint32_t *off,
                                 uint32_t *end) {
    const uint64_t a = s0 & ~(uint64_t)15;
    *off = (uint32_t)(s0 - a);
    *end = *off + len;  // <= 15 + 32 + 14
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint4 w = make_uint4(0, 0, 0, 0);
        if (len && 16u * q < *end) w = *reinterpret_cast<const uint4 *>(seq + a + 16u * q);
        d[4 * q] = w.x;
        d[4 * q + 1] = w.y;
        d[4 * q + 2] = w.z;
        d[4 * q + 3] = w.w;
    }
}

// Bytes jb .. jb + KP_P_BATCH - 1 of the roll (jb a constant of the caller's unrolled loop): code[q]
// and has[q] of the window byte jb + q completes, inv += the complete windows with an invalid byte
__device__ __forceinline__ void kp_scan_batch(kp_s_win &w, const uint32_t d[16], uint32_t jb, uint32_t off, uint32_t end,
                                              uint32_t full0, int k, int fold, uint32_t mask, int top,
                                              uint32_t code[KP_P_BATCH], bool has[KP_P_BATCH], uint32_t &inv) {
#pragma unroll
    for (uint32_t q = 0; q < KP_P_BATCH; ++q) {
        const uint32_t j = jb + q;
        if (j >= off && j < end) kp_s_step(w, kp_s_class((d[j >> 2] >> (8u * (j & 3u))) & 0xffu), mask, top);
        const bool full = j >= full0 && j < end;
        has[q] = full && w.valid >= (uint32_t)k;
        inv += full && !has[q];
        code[q] = kp_s_code(w, k, fold);
    }
}

// centres whose window lies inside a contig of n bases: [lo, hi)
static void scan_centres(uint64_t n, int k, uint64_t *lo, uint64_t *hi) {
    *lo = (uint64_t)(k / 2);
    *hi = n >= (uint64_t)k ? n - (uint64_t)k + *lo + 1 : *lo;
}

// the work items of `len` consecutive centres or positions
static uint64_t scan_tiles(uint64_t len) { return (len + KP_S_TILE - 1) / KP_S_TILE; }

// the work items of the positions [b, e) clipped to [lo, hi): how many, ...
static uint64_t scan_pieces(uint64_t b, uint64_t e, uint64_t lo, uint64_t hi) {
    b = std::max(b, lo), e = std::min(e, hi);
    return e > b ? scan_tiles(e - b) : 0;
}

// ... and the items themselves, appended with `tag` as their region; returns the centres they hold
static uint64_t scan_cut(std::vector<kp_p_item> &items, uint64_t b, uint64_t e, uint64_t lo, uint64_t hi, uint32_t tag) {
    b = std::max(b, lo), e = std::min(e, hi);
    for (uint64_t f = b; f < e; f += KP_S_TILE)
        items.push_back(kp_p_item{(uint32_t)f, (uint32_t)std::min<uint64_t>(KP_S_TILE, e - f), tag});
    return e > b ? e - b : 0;
}

static int scan_check_regions(const std::string &w, uint64_t n, const uint64_t *reg_begin, const uint64_t *reg_end,
                              uint64_t n_regions, bool ascending) {
    for (uint64_t r = 0; r < n_regions; ++r) {
        if (reg_begin[r] > reg_end[r] || reg_end[r] > n)
            return fail(KP_E_ARG, w + ": region " + std::to_string(r) + " has begin > end or lies outside the contig");
        if (ascending && r && reg_begin[r] < reg_end[r - 1])
            return fail(KP_E_ARG, w + ": region " + std::to_string(r) + " begins before region " + std::to_string(r - 1) +
                                      " ends (regions must be ascending and disjoint)");
    }
    return KP_OK;
}

// workgroups of a persistent grid resident at once beside `lds_bytes` of LDS each
static int scan_per_cu(size_t lds_bytes) { return lds_bytes <= 16u * 1024u ? 8 : (lds_bytes <= 40u * 1024u ? 4 : 2); }

// The contig on the device, in the allocation kp_seq_scan uses, then the items (none: d_items may
// be NULL), then `more` bytes the caller takes from c->seq_in (and checks)
static int scan_upload(kp_ctx *c, const char *who, const uint8_t *seq, uint64_t n, const std::vector<kp_p_item> &items,
                       size_t more, uint8_t **d_seq, kp_p_item **d_items) {
    const size_t b_items = items.size() * sizeof(kp_p_item);
    int rc = c->seq_in.reserve(who, g_up(n + KP_S_PAD) + g_up(b_items) + more);
    if (rc) return rc;
    *d_seq = (uint8_t *)c->seq_in.take(n + KP_S_PAD);
    kp_p_item *d_it = (kp_p_item *)c->seq_in.take(b_items);
    if ((rc = c->seq_in.check(who))) return rc;
    if (n) KP_HIP(hipMemcpyAsync(*d_seq, seq, n, hipMemcpyHostToDevice, c->stream));
    if (b_items) KP_HIP(hipMemcpyAsync(d_it, items.data(), b_items, hipMemcpyHostToDevice, c->stream));
    if (d_items) *d_items = d_it;
    return KP_OK;
}

// a timed launch: scan_mark, the launch, scan_launched, and after the stream's sync scan_elapsed
static int scan_mark(kp_ctx *c, int a) {
    KP_HIP(hipEventRecord(c->ev[a], c->stream));
    return KP_OK;
}

static int scan_launched(kp_ctx *c, int b) {
    KP_HIP(hipGetLastError());
    KP_HIP(hipEventRecord(c->ev[b], c->stream));
    return KP_OK;
}

static int scan_elapsed(kp_ctx *c, int a, int b, float *ms) {
    KP_HIP(hipEventElapsedTime(ms, c->ev[a], c->ev[b]));
    return KP_OK;
}

// The arena of a device session (kp_pred_sess or kp_spec_sess) laid out for one call: the table of
// `entry` bytes per k-mer first, then `extra` bytes the caller takes.  Grows the arena if it has
// to -- against free memory minus 2 GiB -- and then, or after a failed growth, builds the table
// again: `build` takes the `b_staged` bytes of its patterns from the arena, copies them and
// launches the table kernel between scan_mark(c, 0) and scan_launched(c, 1).
template <typename Sess, typename Build>
static int scan_arena(kp_ctx *c, Sess *s, const char *who, const char *table, size_t entry, size_t b_staged, size_t extra,
                      Build build) {
    const size_t b_lut = g_up((size_t)s->cells * entry);
    const size_t need = b_lut + std::max(extra, b_staged);
    if (need > c->arena.bytes) {
        size_t fr = 0, tot = 0;
        KP_HIP(hipMemGetInfo(&fr, &tot));
        if (need + (2ull << 30) > fr + c->arena.bytes)
            return fail(KP_E_NOMEM, std::string(who) + ": the " + table + " table of " + std::to_string(s->k) +
                                        "-mers and this call's buffers need " + std::to_string(need >> 20) +
                                        " MiB of device memory, " + std::to_string((fr + c->arena.bytes) >> 20) +
                                        " MiB are free (2 GiB stay free)");
        s->lut_ok = false;
    }
    int rc = c->arena.reserve(who, need);
    if (rc) return rc;
    s->d_lut = (int32_t *)c->arena.take((size_t)s->cells * entry);
    if (!s->lut_ok) {
        if ((rc = build())) return rc;
        KP_HIP(hipStreamSynchronize(c->stream));
        float ms = 0.f;
        if ((rc = scan_elapsed(c, 0, 1, &ms))) return rc;
        s->st.lut_ms = ms;
        s->lut_ok = true;
        c->arena.used = b_lut;  // the staged patterns are done with
    }
    return KP_OK;
}
