// kp_pass.h -- one pass of the sweep over every lane: the launch code of kp_dp_kernel
// (kp_dp_kernel.h), the score rows' allocator, the cut of user groups into device groups,
// run_pass, and kp_pass / kp_device_groups / kp_reserve_lanes with the stats getters and
// kp_fit_leaves.
#pragma once
#include "kp_bt.h"
#include "kp_dp_kernel.h"
#include "kp_plan_dev.h"

// dynamic LDS of kp_dp_kernel (carve order and rounding exactly as in the kernel)
static size_t dp_lds_bytes(const kp::host_plan &hp, int nl, size_t ct_bytes) {
    const kp_geom &g = hp.g;
    const size_t st = (size_t)nl * g.Bpad * 4;
    const size_t scratch = (((size_t)hp.pscratch_entries * 4 * ct_bytes) + 15) & ~(size_t)15;  // 2 build buffers
    const size_t ptab = ((((size_t)hp.ptab_entries * 2 + 3) & ~(size_t)3)) * ct_bytes;
    return std::max(st, scratch) + ptab + (size_t)(g.kh * 7 + 1) * sizeof(kp_hpair) +
           (((size_t)g.t * 16 + 15) & ~(size_t)15) + 16
#ifdef KP_STAMPS
           + 32 * sizeof(unsigned long long)
#endif
        ;
}

template <typename CT, int NL, bool HZ, bool MIX>
static int launch_dp_hz(hipStream_t st, const kp_dp_params &P, unsigned nb, unsigned ngroups, int threads, size_t lds) {
    if constexpr (kp_sdwa_on<NL, MIX>()) {  // its scan reads the row array at LDS address 0 (kp_at_bytes)
        static std::atomic<bool> checked{false};
        if (!checked.load(std::memory_order_relaxed)) {
            hipFuncAttributes fa;
            KP_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&kp_dp_kernel<CT, NL, HZ, MIX>)));
            if (fa.sharedSizeBytes != 0)
                return fail(KP_E_HIP, "kp_dp_kernel has static LDS: its dynamic LDS does not start at address 0");
            checked.store(true, std::memory_order_relaxed);
        }
    }
    if (lds > 65536)
        KP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&kp_dp_kernel<CT, NL, HZ, MIX>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((kp_dp_kernel<CT, NL, HZ, MIX>), dim3(nb, ngroups), dim3(threads), lds, st, P);
    KP_HIP(hipGetLastError());
    return KP_OK;
}

// Groups of 1-3 lanes (80 VGPRs at 6 waves per SIMD) run high levels >= 1 without the
// k-mer code (fewer spills: 1-lane pass 149 -> 144 ms); wider groups keep one kernel for
// every level (the split build measured slower there: 5 lanes 395 -> 402 ms)
// (the mixed builds always split: their k-mer code adds register spills at every width)
template <typename CT, int NL, bool MIX>
static int launch_dp(hipStream_t st, const kp_dp_params &P, unsigned nb, unsigned ngroups, int threads, size_t lds) {
    constexpr bool one_build = NL > 3 && !MIX;  // (mixed, one build for all levels: +1-2 ms)
    return (P.H == 0 || one_build) ? launch_dp_hz<CT, NL, true, MIX>(st, P, nb, ngroups, threads, lds)
                                : launch_dp_hz<CT, NL, false, MIX>(st, P, nb, ngroups, threads, lds);
}

// mixed groups (two (alpha, beta) sets) need at least 2 lanes
template <typename CT, int NL>
static int launch_dp_mix(bool mix, hipStream_t st, const kp_dp_params &P, unsigned nb, unsigned ngroups, int threads,
                         size_t lds) {
    if constexpr (NL >= 2) {
        if (mix) return launch_dp<CT, NL, true>(st, P, nb, ngroups, threads, lds);
    }
    return launch_dp<CT, NL, false>(st, P, nb, ngroups, threads, lds);
}

template <typename CT>
static int launch_dp_nl(int nl, bool mix, hipStream_t c, const kp_dp_params &P, unsigned nb, unsigned ngroups,
                        int threads, size_t lds) {
    switch (nl) {
        case 1: return launch_dp_mix<CT, 1>(mix, c, P, nb, ngroups, threads, lds);
        case 2: return launch_dp_mix<CT, 2>(mix, c, P, nb, ngroups, threads, lds);
        case 3: return launch_dp_mix<CT, 3>(mix, c, P, nb, ngroups, threads, lds);
        case 4: return launch_dp_mix<CT, 4>(mix, c, P, nb, ngroups, threads, lds);
        case 5: return launch_dp_mix<CT, 5>(mix, c, P, nb, ngroups, threads, lds);
        case 6: return launch_dp_mix<CT, 6>(mix, c, P, nb, ngroups, threads, lds);
        case 7: return launch_dp_mix<CT, 7>(mix, c, P, nb, ngroups, threads, lds);
        case 8: return launch_dp_mix<CT, 8>(mix, c, P, nb, ngroups, threads, lds);
    }
    return fail(KP_E_ARG, "lanes per workgroup must be 1..8");
}

static int dp_threads() {
    const int v = (int)env_int("KP_DP_THREADS", 512);
    return (v == 64 || v == 128 || v == 256 || v == 512 || v == 1024) ? v : 512;
}

// a wide group's lanes as full workgroups first (7 lanes as 5 + 2: 9-mer pass 603 -> 593
// ms, profiles/r03/experiments/wide_split.txt); KP_WIDE_SPLIT=0: near-equal (4 + 3)
static bool wide_split_greedy() { return env_int("KP_WIDE_SPLIT", 1) != 0; }

static int lanes_per_wg_default() {
    return std::min(std::max((int)env_int("KP_LANES_PER_WG", 5), 1), KP_GROUP_LANES);
}

// lanes per workgroup of the sweep: KP_LANES_PER_WG (default 5), fewer if two workgroups
// per CU would not fit LDS (KP_LDS_BUDGET: another per-workgroup budget; A/B only)
static int wg_lanes(const kp::host_plan &hp, size_t ct_bytes, size_t lds_max) {
    int per_wg = lanes_per_wg_default();
    const size_t lds_two = std::min<size_t>(lds_max, (size_t)env_int("KP_LDS_BUDGET", 160u * 1024u / 2u));
    while (per_wg > 1 && dp_lds_bytes(hp, per_wg, ct_bytes) > lds_two) --per_wg;
    return per_wg;
}

// Score rows + backtrack node pool for `lanes` lanes.  Grown only (a pass with fewer lanes
// uses the front of the buffers), never cleared: every pass writes every row of its lanes
// before any read.  Freeing and re-allocating a large buffer is slow on this platform
// (the driver wipes freed memory before handing it out again: ~4 s for 100-150 GB,
// tools/alloc_probe.hip), so callers reserve the largest pass up front (kp_reserve_lanes).
// ---- the score rows: the one very large allocation ----
// Plain hipMalloc.  A hipMalloc of HBM that was used before waits for the driver's wipe
// (~30 ms per GB); the device's stream-ordered pool does not, but re-serving a freed pool
// block for a larger request returned memory that does not hold what is written to it
// (tools/async_check.hip), so the pool is NOT used by default.  Opt-in only
// (KP_POOL_SCORES=1, for allocation-time experiments): then the FIRST score buffer of a
// process on a device comes from the pool (nothing was ever freed there) and is written
// with a pattern and read back before use; every later one comes from hipMalloc.
static std::atomic<bool> g_pool_touched[64];

__global__ void kp_fill_pattern(uint32_t *p, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        p[i] = (uint32_t)(i * 2654435761u) ^ 0x5bd1e995u;
}

__global__ void kp_check_pattern(const uint32_t *p, size_t n, unsigned long long *bad) {
    unsigned long long b = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        b += (p[i] != ((uint32_t)(i * 2654435761u) ^ 0x5bd1e995u));
    for (int off = 32; off > 0; off >>= 1) b += __shfl_xor(b, off, 64);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(bad, b);
}

static void free_scores(kp_plan *p) {
    if (!p->d_S) return;
    if (p->S_pool) {
        (void)hipFreeAsync(p->d_S, p->ctx->stream);
        (void)hipStreamSynchronize(p->ctx->stream);
    } else {
        (void)hipFree(p->d_S);
    }
    p->d_S = nullptr;
    p->S_pool = false;
}

static int alloc_scores(kp_plan *p, size_t bytes) {
    kp_ctx *c = p->ctx;
    const bool allow = env_int("KP_POOL_SCORES", 0) == 1 && c->device >= 0 && c->device < 64;
    if (allow && !g_pool_touched[c->device].exchange(true)) {
        void *q = nullptr;
        if (hipMallocAsync(&q, bytes, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess) {
            unsigned long long *d_bad = nullptr, bad = 1;
            const size_t n = bytes / 4;
            if (hipMalloc(&d_bad, sizeof(bad)) == hipSuccess &&
                hipMemsetAsync(d_bad, 0, sizeof(bad), c->stream) == hipSuccess) {
                hipLaunchKernelGGL(kp_fill_pattern, dim3(16384), dim3(256), 0, c->stream, (uint32_t *)q, n);
                hipLaunchKernelGGL(kp_check_pattern, dim3(16384), dim3(256), 0, c->stream, (const uint32_t *)q, n,
                                   d_bad);
                if (hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                    hipStreamSynchronize(c->stream) != hipSuccess)
                    bad = 1;
            }
            if (d_bad) (void)hipFree(d_bad);
            if (bad == 0) {
                p->d_S = static_cast<float *>(q);
                p->S_pool = true;
                return KP_OK;
            }
            (void)hipFreeAsync(q, c->stream);
            (void)hipStreamSynchronize(c->stream);
        }
        (void)hipGetLastError();  // fall back to hipMalloc below
    }
    KP_HIP(dmalloc(&p->d_S, bytes));
    p->S_pool = false;
    return KP_OK;
}

static int ensure_lanes(kp_plan *p, uint64_t lanes) {
    if (lanes <= p->lanes_cap) return KP_OK;
    const kp::host_plan &hp = p->hp;
    const uint32_t ncap = node_cap_of(hp);
    free_scores(p);
    dfree(p->d_nodes);
    p->d_S = nullptr;
    p->d_nodes = nullptr;
    p->lanes_cap = 0;
    size_t sb = hp.g.nblocks * (size_t)lanes * hp.g.Bpad * 4, nb = (size_t)lanes * ncap * sizeof(kp_node);
    size_t fr = 0, tot = 0;
    KP_HIP(hipMemGetInfo(&fr, &tot));
    if (sb + nb + (256u << 20) > fr)
        return fail(KP_E_NOMEM, "lanes need " + std::to_string(sb + nb) + " bytes, free " + std::to_string(fr));
    if (int rc = alloc_scores(p, sb)) return rc;
    KP_HIP(dmalloc(&p->d_nodes, nb));
    p->lanes_cap = lanes;
    p->node_cap = ncap;
    return KP_OK;
}

// The device groups of a pass (host code; kp_pass, and kp_device_groups for tests): user
// groups in order, lanes group-major, lane0 = first lane of each device group
static void plan_device_groups(const kp_group *groups, int n_groups, int per_wg, std::vector<kp_group_dev> &dg) {
    dg.clear();
    uint32_t lane = 0;
    // lanes [s, s + n) of the run of user groups g0.. (group-major) as one device group;
    // lanes of a second user group with another (alpha, beta) become the mixed set 2
    auto chunk = [&](int g0, int s, int n) -> bool {
        kp_group_dev d;
        memset(&d, 0, sizeof(d));
        d.fold = groups[g0].fold;
        d.lane0 = (int32_t)lane;
        d.nl = n;
        d.alpha = d.alpha2 = groups[g0].alpha;
        d.beta = d.beta2 = groups[g0].beta;
        int gi = g0, off = s;
        while (off >= groups[gi].n_lanes) off -= groups[gi++].n_lanes;
        const int first = gi;
        for (int j = 0; j < n; ++j, ++off) {
            if (off == groups[gi].n_lanes) {
                off = 0;
                ++gi;
            }
            const kp_group &u = groups[gi];
            if (j == 0) {
                d.alpha = d.alpha2 = u.alpha;
                d.beta = d.beta2 = u.beta;
            } else if (gi != first) {
                if (gi > first + 1) return false;  // at most two user groups per device group
                const bool same = u.alpha == groups[first].alpha && u.beta == groups[first].beta;
                if (!same && d.nl2 == 0) {
                    d.alpha2 = u.alpha;
                    d.beta2 = u.beta;
                }
                if (!same) ++d.nl2;
            }
            d.pen[j] = u.penalty[off];
        }
        dg.push_back(d);
        lane += (uint32_t)n;
        return true;
    };
    // Each user group becomes as few device groups as the workgroup width allows, full
    // workgroups first (wide_split_greedy).  Consecutive user groups of the same fold share their count tables: when
    // cutting the run's lanes together gives fewer device groups, they are cut together
    // (mixed groups, e.g. the 2 + 3 lanes of two alphas as one 5-lane group; at most two
    // (alpha, beta) sets each; KP_MIX_GROUPS=0 disables)
    const bool mixing = env_int("KP_MIX_GROUPS", 1) != 0;
    for (int i = 0; i < n_groups;) {
        int e = i + 1, tot = groups[i].n_lanes, sep = (groups[i].n_lanes + per_wg - 1) / per_wg;
        while (mixing && e < n_groups && groups[e].fold == groups[i].fold) {
            tot += groups[e].n_lanes;
            sep += (groups[e].n_lanes + per_wg - 1) / per_wg;
            ++e;
        }
        const int nd = (tot + per_wg - 1) / per_wg;
        bool merged = false;
        if (e > i + 1 && nd < sep) {
            const size_t dg0 = dg.size();
            const uint32_t lane0 = lane;
            merged = true;
            for (int q = 0, s = 0; q < nd && merged; ++q) {
                const int n = wide_split_greedy() ? std::min(per_wg, tot - s) : tot / nd + (q < tot % nd ? 1 : 0);
                merged = chunk(i, s, n);
                s += n;
            }
            if (!merged) {  // a chunk would span three user groups: cut them one by one
                dg.resize(dg0);
                lane = lane0;
            }
        }
        if (!merged)
            for (int q = i; q < e; ++q) {
                const kp_group &u = groups[q];
                const int nq = (u.n_lanes + per_wg - 1) / per_wg;
                for (int r = 0, s = 0; r < nq; ++r) {
                    const int n = wide_split_greedy() ? std::min(per_wg, u.n_lanes - s)
                                                      : u.n_lanes / nq + (r < u.n_lanes % nq ? 1 : 0);
                    chunk(q, s, n);
                    s += n;
                }
            }
        i = e;
    }
}

// ---------------------------------------------------------------------------
// run_pass and its steps
// ---------------------------------------------------------------------------

// The user groups are well-formed and the counts of their folds set; the pass's stream
// waits for the folds whose tables are still filling on the count stream.
static int pass_check_groups(kp_plan *p, const kp_group *groups, int n_groups) {
    for (int i = 0; i < n_groups; ++i) {
        const kp_group &u = groups[i];
        if (u.n_lanes < 1 || u.n_lanes > KP_GROUP_MAX_LANES) return fail(KP_E_ARG, "group lanes must be 1..8");
        if (u.fold >= p->nf || u.fold < -1) return fail(KP_E_ARG, "fold out of range");
        if (u.fold >= 0 && !p->fold_set[u.fold])
            return fail(KP_E_STATE, "counts of fold " + std::to_string(u.fold) + " are not set (kp_counts_fold)");
    }
    for (int i = 0; i < n_groups; ++i)
        if (groups[i].fold >= 0 && p->fold_async[groups[i].fold])
            KP_HIP(hipStreamWaitEvent(p->ctx->stream, p->fold_ev[groups[i].fold], 0));
    return KP_OK;
}

// threads per workgroup: every level of the block must fit KP_IPT cells per thread
static int pass_threads(const kp::host_plan &hp, int *out) {
    int max_level_cells = 0;
    for (int l = 0; l <= hp.lmax; ++l) max_level_cells = std::max(max_level_cells, hp.loff[l + 1] - hp.loff[l]);
    int threads = dp_threads();
    while (threads < KP_DP_MAX_THREADS && threads * KP_IPT < max_level_cells) threads *= 2;
    if (threads * KP_IPT < max_level_cells) return fail(KP_E_ARG, "block level too wide for one workgroup");
    *out = threads;
    return KP_OK;
}

// The small per-lane buffers (device groups, lane -> group, roots, backtrack counters and
// leaf lists), grown only: room for at least 64 lanes, which also bounds the device groups.
static int ensure_small(kp_plan *p, uint64_t lanes) {
    if (lanes <= p->small_cap) return KP_OK;
    const struct {
        void **ptr;
        size_t elem;  // bytes per lane
    } bufs[] = {
        {reinterpret_cast<void **>(&p->d_groups), sizeof(kp_group_dev)},
        {reinterpret_cast<void **>(&p->d_lanegrp), sizeof(uint32_t)},
        {reinterpret_cast<void **>(&p->d_rtrain), sizeof(float)},
        {reinterpret_cast<void **>(&p->d_rtest), sizeof(float)},
        {reinterpret_cast<void **>(&p->d_nleaves), sizeof(uint64_t)},
        {reinterpret_cast<void **>(&p->d_bad), sizeof(uint32_t)},
        {reinterpret_cast<void **>(&p->d_cnt), sizeof(uint32_t)},
        {reinterpret_cast<void **>(&p->d_dend), (KP_MAXDEPTH + 1) * sizeof(uint32_t)},
        {reinterpret_cast<void **>(&p->d_leaves), p->hp.n_kmers * sizeof(uint64_t)},
    };
    p->small_cap = 0;
    for (const auto &b : bufs) {
        dfree(*b.ptr);
        *b.ptr = nullptr;
    }
    const uint64_t cap = std::max<uint64_t>(lanes, 64);
    for (const auto &b : bufs) KP_HIP(dmalloc(b.ptr, cap * b.elem));
    p->small_cap = cap;
    return KP_OK;
}

// The device groups of the pass sorted into launch classes (device groups with equal lane
// counts share one launch per level, widest first), and each lane's device group.
static void pass_lanes(const kp_group *groups, int n_groups, int per_wg, std::vector<kp_group_dev> &dg,
                       std::vector<uint32_t> &lanegrp) {
    plan_device_groups(groups, n_groups, per_wg, dg);
    uint32_t ltot = 0;
    for (const kp_group_dev &d : dg) ltot += (uint32_t)d.nl;
    std::stable_sort(dg.begin(), dg.end(), [](const kp_group_dev &a, const kp_group_dev &b) { return a.nl > b.nl; });
    lanegrp.assign(ltot, 0);
    for (size_t i = 0; i < dg.size(); ++i)
        for (int j = 0; j < dg[i].nl; ++j) lanegrp[dg[i].lane0 + j] = (uint32_t)i;
}

// a lane class: the run [first, last) of device groups of one width (dg is sorted by width);
// mixed = one of them holds two (alpha, beta) sets
struct kp_lane_class {
    size_t first, last;
    int width;
    bool mixed;
};

static std::vector<kp_lane_class> lane_classes(const std::vector<kp_group_dev> &dg) {
    std::vector<kp_lane_class> classes;
    for (size_t i = 0; i < dg.size();) {
        kp_lane_class q = {i, i, dg[i].nl, false};
        for (; q.last < dg.size() && dg[q.last].nl == q.width; ++q.last) q.mixed = q.mixed || dg[q.last].nl2 > 0;
        classes.push_back(q);
        i = q.last;
    }
    return classes;
}

// What every launch of the pass shares of kp_dp_params: the plan's tables and sizes and the
// launch knobs (launch_params adds the per-launch fields).
static int pass_params(kp_plan *p, const kp_geom &g, kp_dp_params *out) {
    const kp::host_plan &hp = p->hp;
    kp_dp_params &P = *out;
    memset(&P, 0, sizeof(P));
    P.g = g;
    P.T = tables_of(p);
    P.K = p->d_K;
    P.S = p->d_S;
    P.groups = p->d_groups;
    P.lmax = hp.lmax;
    if (hp.lmax > KP_DP_MAX_LEVELS) return fail(KP_E_ARG, "too many low levels");
    for (int l = 0; l <= hp.lmax + 1; ++l) P.loffv[l] = hp.loff[l];
    for (int l = 0; l <= hp.lmax; ++l)  // (the sweep's descriptor loads assume every level holds a cell)
        if (hp.loff[l + 1] <= hp.loff[l]) return fail(KP_E_ARG, "empty low level");
    P.ptab_entries = hp.ptab_entries;
    P.pscratch_entries = hp.pscratch_entries;
#ifdef KP_ABLATION
    // timing-ablation build only (make ablation -> libkmerpapa_hip_ablation.so): phases
    // skipped by KP_DEBUG_SKIP give wrong scores, so the pass reports KP_E_STATE
    P.dbg = (int)env_int("KP_DEBUG_SKIP", 0);
#else
    P.dbg = 0;  // the product build has no phase-skipping path
#endif
    // runs of 36 consecutive blocks per XCD (workgroups are dealt round-robin over the 8
    // XCDs): neighbours in the reuse order share their L2; measured -1 % against none
    // (DESIGN.md §5), 16 against 8 -1.5 ms per 5-lane pass (12: -1.2, 32: -0.4), 24 against
    // 16 -1 ms (20: -0.5) and 40 against 24 -1 ms (32: +2, 64: +5; non-monotonic;
    // profiles/r04/experiments/remap_ab.txt), all under the plain block order.  Under the
    // class order (kp_plan.h) 36 against 40 -2.8 to -3.7 ms (24: -3.3, 64: +12), under the
    // plain one 36 and 40 tie (profiles/block_class/ab.txt).  The cache model gives 36 and
    // 40 the same traffic under the class order, so this step is measured, not modelled
    // 
    P.remap = (int)env_int("KP_XCD_REMAP", 36);
    P.lanesplit = (int)env_int("KP_LANE_SPLIT", 1);
    // KP_EXACT_LOGS=1: no fast device log at all (same results; exercises the exact path)
    P.exact = (int)env_int("KP_EXACT_LOGS", 0);
    P.ntstore = (int)env_int("KP_NT_STORE", 1);
    P.stamps = nullptr;
#ifdef KP_STAMPS
    static unsigned long long *d_stamps = nullptr;
    if (!d_stamps) KP_HIP(dmalloc(&d_stamps, 32 * sizeof(unsigned long long)));
    KP_HIP(hipMemsetAsync(d_stamps, 0, 32 * sizeof(unsigned long long), p->ctx->stream));
    P.stamps = d_stamps;
#endif
    return KP_OK;
}

// Per high level (launch), the high positions whose child rows are read non-temporally.
// Child rows along the KP_NT_SLOW slowest-varying high positions of the block order
// (default 3) are read non-temporally: under that order they are not re-read while
// still in the Infinity Cache, so they no longer evict the rows of the fast positions
// that are (9-mer pass 403-408 -> 397-398 ms; 2: 399-400, 4: 417)
// KP_NT_SLOW_H = comma list: a count per high level (launch), for per-launch tuning;
// levels past the list (or without it) take KP_NT_SLOW.
// KP_NT_SLOW is also read by kp::build_plan, where it sets the slab of the class order of
// the block list (the same slowest positions): changing it changes both the non-temporal
// reads and the list.  KP_NT_SLOW_H changes the reads only; the slab does not follow it.
static std::vector<uint32_t> nt_masks(const kp::host_plan &hp) {
    const kp_geom &g = hp.g;
    std::vector<uint32_t> ntmask_h(hp.hmax + 1, 0);
    std::vector<int> per(hp.hmax + 1, (int)env_int("KP_NT_SLOW", 3));
    if (const char *e = getenv("KP_NT_SLOW_H")) {
        int H = 0;
        for (const char *q = e; *q && H <= hp.hmax; ++H) {
            per[H] = atoi(q);
            while (*q && *q != ',') ++q;
            if (*q == ',') ++q;
        }
    }
    // (counted among the positions that have split pairs: a fixed base of the general
    // pattern, radix 1, sits last in the block order but has no child rows -- the 11-mer
    // super pattern ANNNNMNNNNA has one, which left it with two non-temporal positions)
    std::vector<int> slow_order;
    for (int q = (int)hp.perm.size() - 1; q >= 0; --q)
        if (g.r[g.t + hp.perm[q]] > 1) slow_order.push_back(hp.perm[q]);
    for (int H = 0; H <= hp.hmax; ++H)
        for (int q = 0; q < per[H] && q < (int)slow_order.size(); ++q) ntmask_h[H] |= 1u << slow_order[q];
    return ntmask_h;
}

// the parameters of the launch of high level H for the class whose first device group is `first`
static kp_dp_params launch_params(const kp_dp_params &P, const kp_plan *p, size_t first, int H, uint32_t ntmask) {
    kp_dp_params Q = P;
    Q.hbase = p->hp.hoff[H];
    Q.H = H;
    Q.groups = p->d_groups + first;
    Q.ntmask = ntmask;
    return Q;
}

// The sweep: one launch per (class, non-empty high level), H ascending.  With several
// classes and KP_CLASS_STREAMS=1, class q > 0 runs its whole launch sequence on side
// stream q - 1 and the pass's stream waits for them at the end.  Off by default: measured
// on one MI355X, 9-mer passes of 4+3 lanes (one 7-penalty group) 620 -> 603 ms and 5+1 /
// 4+2 (two groups) -0.5 %, but the 11-mer step (4+3 lanes, ANNNNMNNNNA) 606 -> 627 ms.
// timed (KP_LAUNCH_TIMES=1): HIP events around every launch (kp_last_launch_ms; tuning only)
template <typename CT>
static int pass_sweep(kp_plan *p, const kp_dp_params &P, const std::vector<kp_lane_class> &classes,
                      const std::vector<uint32_t> &ntmask_h, int threads, bool timed, uint64_t *n_launches) {
    kp_ctx *c = p->ctx;
    const kp::host_plan &hp = p->hp;
    const bool multi = classes.size() > 1 && env_int("KP_CLASS_STREAMS", 0) == 1;
    if (multi) {
        KP_HIP(hipEventRecord(c->ev[3], c->stream));
        for (size_t q = 1; q < classes.size() && q <= KP_SIDE_STREAMS; ++q)
            KP_HIP(hipStreamWaitEvent(c->side[q - 1], c->ev[3], 0));
    }
    uint64_t launches = 0;
    for (size_t q = 0; q < classes.size(); ++q) {
        const hipStream_t st = (multi && q > 0) ? c->side[(q - 1) % KP_SIDE_STREAMS] : c->stream;
        const kp_lane_class &cl = classes[q];
        size_t lds = dp_lds_bytes(hp, cl.width, sizeof(CT));
#ifdef KP_ABLATION
        // ablation build only: extra LDS per workgroup to force lower occupancy
        lds += (size_t)env_int("KP_LDS_PAD", 0);
#endif
        for (int H = 0; H <= hp.hmax; ++H) {
            const uint64_t nb = hp.hoff[H + 1] - hp.hoff[H];
            if (!nb) continue;
            if (timed) {
                while (p->lev.size() < 2 * (launches + 1)) {
                    hipEvent_t e;
                    KP_HIP(hipEventCreate(&e));
                    p->lev.push_back(e);
                }
                KP_HIP(hipEventRecord(p->lev[2 * launches], st));
            }
            if (int rc = launch_dp_nl<CT>(cl.width, cl.mixed, st, launch_params(P, p, cl.first, H, ntmask_h[H]),
                                          (unsigned)nb, (unsigned)(cl.last - cl.first), threads, lds))
                return rc;
            if (timed) KP_HIP(hipEventRecord(p->lev[2 * launches + 1], st));
            ++launches;
        }
    }
    if (multi)
        for (size_t q = 1; q < classes.size() && q <= KP_SIDE_STREAMS; ++q) {
            KP_HIP(hipEventRecord(c->side_ev[q - 1], c->side[q - 1]));
            KP_HIP(hipStreamWaitEvent(c->stream, c->side_ev[q - 1], 0));
        }
    *n_launches = launches;
    return KP_OK;
}

// breadth-first backtrack of every lane: depth d holds cells of level <= maxlev - d
template <typename CT>
static int pass_backtrack(kp_plan *p, const kp_geom &g, uint32_t Ltot) {
    const kp::host_plan &hp = p->hp;
    const hipStream_t st = p->ctx->stream;
    kp_bt_params B;
    memset(&B, 0, sizeof(B));
    B.g = g;
    B.T = tables_of(p);
    B.K = p->d_K;
    B.S = p->d_S;
    B.groups = p->d_groups;
    B.lanegrp = p->d_lanegrp;
    B.nodes = p->d_nodes;
    B.cap = p->node_cap;
    B.cnt = p->d_cnt;
    B.dend = p->d_dend;
    B.bad = p->d_bad;
    B.root_train = p->d_rtrain;
    B.root_test = p->d_rtest;
    B.nleaves = p->d_nleaves;
    B.leaves = p->d_leaves;
    B.leafcap = hp.n_kmers;
    B.maxdepth = hp.maxlev;
    const unsigned lb = (Ltot + 63) / 64;
    const uint64_t root = hp.npat - 1;
    hipLaunchKernelGGL(kp_bt_init, dim3(lb), dim3(64), 0, st, B, root, kp_cell_digits(g, root));
    KP_HIP(hipGetLastError());
    for (int d = 0; d <= hp.maxlev; ++d) {
        B.depth = d;
        hipLaunchKernelGGL(kp_bt_level<CT>, dim3(64, Ltot), dim3(256), 0, st, B);
        KP_HIP(hipGetLastError());
        hipLaunchKernelGGL(kp_bt_advance, dim3(lb), dim3(64), 0, st, B);
        KP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(kp_bt_finish, dim3(Ltot), dim3(256), 0, st, B);
    KP_HIP(hipGetLastError());
    return KP_OK;
}

// what the backtrack left per lane
struct kp_pass_roots {
    std::vector<uint32_t> bad;
    std::vector<float> train, test;
    std::vector<uint64_t> nleaves;
};

// read the roots back (nothing to read when the backtrack did not run) and wait for the pass
static int pass_read_back(kp_plan *p, uint32_t Ltot, bool bt, kp_pass_roots *R) {
    const hipStream_t st = p->ctx->stream;
    R->bad.assign(Ltot, 0);
    R->train.resize(Ltot);
    R->test.resize(Ltot);
    R->nleaves.resize(Ltot);
    if (bt) {
        KP_HIP(hipMemcpyAsync(R->train.data(), p->d_rtrain, Ltot * sizeof(float), hipMemcpyDeviceToHost, st));
        KP_HIP(hipMemcpyAsync(R->test.data(), p->d_rtest, Ltot * sizeof(float), hipMemcpyDeviceToHost, st));
        KP_HIP(hipMemcpyAsync(R->nleaves.data(), p->d_nleaves, Ltot * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        KP_HIP(hipMemcpyAsync(R->bad.data(), p->d_bad, Ltot * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    KP_HIP(hipStreamSynchronize(st));
    return KP_OK;
}

// every lane's backtrack reproduced its scores (KP_E_PARITY if not); the roots go to the caller
static int pass_deliver(const kp_pass_roots &R, float *root_train, float *root_test, uint64_t *n_leaves) {
    for (size_t i = 0; i < R.bad.size(); ++i) {
        if (R.bad[i])
            return fail(KP_E_PARITY, "backtrack of lane " + std::to_string(i) + " failed (flags " +
                                         std::to_string(R.bad[i]) +
                                         ": 1 no candidate, 2 node pool, 4 score not reproduced)");
        if (root_train) root_train[i] = R.train[i];
        if (root_test) root_test[i] = R.test[i];
        if (n_leaves) n_leaves[i] = R.nleaves[i];
    }
    return KP_OK;
}

// The stats of the pass that just ran (t0: its start on the host), from its events, and the
// per-launch times when they were taken.
static int pass_stats(kp_plan *p, const kp_dp_params &P, uint32_t Ltot, bool bt, bool timed, uint64_t launches,
                      std::chrono::steady_clock::time_point t0) {
    kp_ctx *c = p->ctx;
    const kp::host_plan &hp = p->hp;
    float dp_ms = 0, bt_ms = 0;
    KP_HIP(hipEventElapsedTime(&dp_ms, c->ev[0], c->ev[1]));
#ifdef KP_STAMPS
    {
        unsigned long long hs[32];
        KP_HIP(hipMemcpy(hs, P.stamps, sizeof(hs), hipMemcpyDeviceToHost));
        fprintf(stderr, "KP_STAMPS init %.4g gather %.4g store %.4g wg_ticks %.4g wg_real100MHz %.4g levels",
                (double)hs[0], (double)hs[1], (double)hs[2], (double)hs[30], (double)hs[31]);
        for (int l = 0; l <= hp.lmax; ++l) fprintf(stderr, " %.4g", (double)hs[3 + l]);
        fprintf(stderr, "\n");
    }
#endif
    KP_HIP(hipEventElapsedTime(&bt_ms, c->ev[1], c->ev[2]));
    p->launch_ms.clear();
    if (timed)
        for (uint64_t q = 0; q < launches; ++q) {
            float ms = 0;
            KP_HIP(hipEventElapsedTime(&ms, p->lev[2 * q], p->lev[2 * q + 1]));
            p->launch_ms.push_back(ms);
        }
    kp_pass_stats &s = p->stats;
    s.dp_ms = dp_ms;
    s.backtrack_ms = bt ? bt_ms : 0;
    s.units = hp.npat * (uint64_t)Ltot;
    s.dp_launches = launches;
    const double sz = (double)p->ct_bytes, npat = (double)hp.npat, nk = (double)hp.n_kmers;
    // 16 B per split pair, 8 B per cell write, 6s per aggregated cell, 2s per k-mer
    s.alg_bytes = (double)Ltot * (16.0 * hp.pairs_total + 8.0 * npat + 6.0 * sz * (npat - nk) + 2.0 * sz * nk);
    // compulsory HBM bytes of the blocked sweep: high-split gathers (2 x f32) + score writes
    const double padf = (double)P.g.Bpad / (double)P.g.B;
    s.gather_bytes = (double)Ltot * padf * (8.0 * hp.pairs_high + 4.0 * npat);
    s.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return KP_OK;
}

template <typename CT>
static int run_pass(kp_plan *p, const kp_group *groups, int n_groups, float *root_train, float *root_test,
                    uint64_t *n_leaves) {
    const auto t0 = std::chrono::steady_clock::now();
    kp_ctx *c = p->ctx;
    const kp::host_plan &hp = p->hp;
    // split user groups into device groups that fit two workgroups per CU in LDS when
    // possible (LDS is the occupancy limit of the sweep)
    const int per_wg = wg_lanes(hp, sizeof(CT), c->lds_max);
    if (dp_lds_bytes(hp, 1, sizeof(CT)) > c->lds_max) return fail(KP_E_ARG, "block does not fit LDS");
    if (int rc = pass_check_groups(p, groups, n_groups)) return rc;
    std::vector<kp_group_dev> dg;
    std::vector<uint32_t> lanegrp;
    pass_lanes(groups, n_groups, per_wg, dg, lanegrp);
    const uint32_t Ltot = (uint32_t)lanegrp.size();
    kp_geom g = hp.g;
    g.nf = p->nf;
    g.Ltot = Ltot;
    int threads = 0;
    if (int rc = pass_threads(hp, &threads)) return rc;
    // lane storage: scores and the backtrack node pool, then the small buffers
    if (int rc = ensure_lanes(p, Ltot)) return rc;
    if (int rc = ensure_small(p, Ltot)) return rc;
    KP_HIP(hipMemcpyAsync(p->d_groups, dg.data(), dg.size() * sizeof(kp_group_dev), hipMemcpyHostToDevice, c->stream));
    KP_HIP(hipMemcpyAsync(p->d_lanegrp, lanegrp.data(), lanegrp.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                          c->stream));
    kp_dp_params P;
    if (int rc = pass_params(p, g, &P)) return rc;
    const std::vector<uint32_t> ntmask_h = nt_masks(hp);
    const std::vector<kp_lane_class> classes = lane_classes(dg);
    const bool timed = env_int("KP_LAUNCH_TIMES", 0) == 1;
    uint64_t launches = 0;
    KP_HIP(hipEventRecord(c->ev[0], c->stream));
    if (int rc = pass_sweep<CT>(p, P, classes, ntmask_h, threads, timed, &launches)) return rc;
    KP_HIP(hipEventRecord(c->ev[1], c->stream));
    const bool bt = !P.dbg;  // (the ablation build's phase skipping leaves nothing to backtrack)
    if (bt)
        if (int rc = pass_backtrack<CT>(p, g, Ltot)) return rc;
    KP_HIP(hipEventRecord(c->ev[2], c->stream));
    kp_pass_roots R;
    if (int rc = pass_read_back(p, Ltot, bt, &R)) return rc;
    if (int rc = pass_stats(p, P, Ltot, bt, timed, launches, t0)) return rc;
    if (P.dbg)  // ablation build: timings only, never numbers
        return fail(KP_E_STATE, "KP_DEBUG_SKIP ablation pass: timings only, results are invalid");
    if (int rc = pass_deliver(R, root_train, root_test, n_leaves)) return rc;
    p->last_ltot = Ltot;
    p->last_groups = dg;
    p->last_lanegrp = lanegrp;
    return KP_OK;
}

extern "C" {

int kp_device_groups(const kp_group *groups, int n_groups, int lanes_per_workgroup, int32_t *lane0, int32_t *nl,
                     int32_t *nl2, int cap, int *n_out) {
    if (!groups || n_groups <= 0 || !n_out || lanes_per_workgroup < 1 || lanes_per_workgroup > KP_GROUP_LANES)
        return fail(KP_E_ARG, "bad arguments");
    for (int i = 0; i < n_groups; ++i)
        if (groups[i].n_lanes < 1 || groups[i].n_lanes > KP_GROUP_MAX_LANES)
            return fail(KP_E_ARG, "group lanes must be 1..8");
    std::vector<kp_group_dev> dg;
    plan_device_groups(groups, n_groups, lanes_per_workgroup, dg);
    *n_out = (int)dg.size();
    for (int i = 0; i < (int)dg.size() && i < cap; ++i) {
        if (lane0) lane0[i] = dg[i].lane0;
        if (nl) nl[i] = dg[i].nl;
        if (nl2) nl2[i] = dg[i].nl2;
    }
    return KP_OK;
}

int kp_pass(kp_plan *p, const kp_group *groups, int n_groups, float *root_train, float *root_test,
            uint64_t *n_leaves) {
    if (!p || !groups || n_groups <= 0) return fail(KP_E_ARG, "bad arguments");
    if (!p->d_K) return fail(KP_E_STATE, "kp_set_counts must come first");
    KP_HIP(hipSetDevice(p->ctx->device));
    if (p->ct_bytes == 4) return run_pass<uint32_t>(p, groups, n_groups, root_train, root_test, n_leaves);
    return run_pass<uint64_t>(p, groups, n_groups, root_train, root_test, n_leaves);
}

int kp_reserve_lanes(kp_plan *p, uint32_t lanes) {
    if (!p) return fail(KP_E_ARG, "null plan");
    KP_HIP(hipSetDevice(p->ctx->device));
    const uint64_t had = p->lanes_cap;
    if (int rc = ensure_lanes(p, lanes)) return rc;
    if (p->lanes_cap != had && !p->S_pool) {  // fault the new pages in now rather than in the first pass
        KP_HIP(hipMemsetAsync(p->d_S, 0, p->hp.g.nblocks * (size_t)p->lanes_cap * p->hp.g.Bpad * 4, p->ctx->stream));
        KP_HIP(hipStreamSynchronize(p->ctx->stream));
    }
    return KP_OK;
}

int kp_last_launch_ms(const kp_plan *p, float *ms, int cap, int *n) {
    if (!p || !n || (cap > 0 && !ms)) return fail(KP_E_ARG, "null argument");
    *n = (int)p->launch_ms.size();
    for (int i = 0; i < cap && i < *n; ++i) ms[i] = p->launch_ms[i];
    return KP_OK;
}

int kp_last_pass_stats(const kp_plan *p, kp_pass_stats *out) {
    if (!p || !out) return fail(KP_E_ARG, "null argument");
    *out = p->stats;
    return KP_OK;
}

int kp_fit_leaves(kp_plan *p, uint32_t lane, uint64_t *leaves, uint64_t cap, uint64_t *n_out) {
    if (!p || !n_out) return fail(KP_E_ARG, "null argument");
    if (lane >= p->last_ltot) return fail(KP_E_STATE, "lane not in last pass");
    KP_HIP(hipSetDevice(p->ctx->device));
    uint64_t n = 0;
    KP_HIP(hipMemcpy(&n, p->d_nleaves + lane, sizeof(uint64_t), hipMemcpyDeviceToHost));
    *n_out = n;
    uint64_t m = std::min(n, std::min(cap, p->hp.n_kmers));
    if (leaves && m)
        KP_HIP(hipMemcpy(leaves, p->d_leaves + (uint64_t)lane * p->hp.n_kmers, m * sizeof(uint64_t),
                         hipMemcpyDeviceToHost));
    return KP_OK;
}

}  // extern "C"
