// kp_plan_dev.h -- the device side of a plan: kp_plan (the device tables of kp_plan.h's
// host_plan, the count tables and the per-lane buffers), the kernels that build the block
// list and its high split pairs on the device, and kp_plan_create / _destroy / _get_info /
// _host* and the block-order checks.
#pragma once
#include "kp_bt.h"
#include "kp_dp_kernel.h"
#include "kp_plan.h"
#include "kp_rt.h"

// The high split pairs of every block of the block list, in scan order (positions
// ascending, pairs in table order: the order kp_dp_kernel's pair setup walks them), as
// child-block deltas: hpd[q][0 .. np) = kp_hpd_word, the rest of the hps-word row 0.  One
// thread per block, once per plan.
__global__ void kp_hpd_kernel(kp_geom g, const kp_postab *__restrict__ tabs, const uint64_t *__restrict__ hdig,
                              uint64_t nblocks, uint32_t hps, uint64_t *__restrict__ hpd) {
    for (uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; q < nblocks;
         q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t hd = hdig[q];
        uint64_t *row = hpd + q * hps;
        uint32_t n = 0;
        for (int i = 0; i < g.kh; ++i) {
            const kp_postab &T = tabs[g.t + i];
            const uint32_t d = (uint32_t)(hd >> (4 * i)) & 15u;
            for (uint32_t r = 0; r < T.np[d]; ++r)
                row[n++] = kp_hpd_word((uint64_t)(d - T.pa[d][r]) * g.hcg[i], (uint64_t)(d - T.pb[d][r]) * g.hcg[i],
                                       (uint32_t)i);
        }
        for (; n < hps; ++n) row[n] = 0;
    }
}

// The block list (hlist / kpos / hdig / hnp) of kp::build_plan's block order, built on the
// device from the plan's rank table instead of walked and uploaded by the host (2.3 M
// blocks at 9-mers: the walk was most of the plan's start-up, before the first pass).  One
// thread per block h; every slot is written once (kp_block_slot is a bijection).
__global__ void kp_blocks_kernel(kp_geom g, const kp_postab *__restrict__ tabs, kp_blockgen bg,
                                 const uint32_t *__restrict__ brank, const uint32_t *__restrict__ coff,
                                 const uint64_t *__restrict__ hoff, uint32_t *__restrict__ hlist, uint32_t *__restrict__ kpos, uint64_t *__restrict__ hdig,
                                 uint64_t *__restrict__ hnp) {
    for (uint64_t h = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; h < g.nblocks;
         h += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t hd, hn;
        const uint64_t q = kp_block_slot(g, tabs, bg, brank, coff, hoff, h, &hd, &hn);
        hlist[q] = (uint32_t)h;
        kpos[h] = (uint32_t)q;
        hdig[q] = hd;
        hnp[q] = hn;
    }
}

static kp_blockgen blockgen_of(const kp::host_plan &hp) {
    kp_blockgen bg;
    memset(&bg, 0, sizeof(bg));
    bg.hs = hp.hs;
    for (int j = 0; j < hp.g.kh; ++j) bg.perm[j] = (int8_t)hp.perm[j];
    bg.nfast = hp.nfast;
    for (int j = 0; j < hp.nfast; ++j) {  // the class order's level tables of the fast positions
        const int i = hp.g.t + hp.perm[j];
        const kp_postab &T = hp.tabs[i];
        // levels 0 .. n - 1: a position's digits are the non-empty subsets of its code's n
        // nucleotides, and a digit's level is its subset's size - 1 (kp_plan.h tabs.lev)
        bg.nlev[j] = (uint8_t)hp.g.n[i];
        for (uint32_t d = 0; d < hp.g.r[i]; ++d) bg.didx[j][d] = bg.lcnt[j][T.lev[d]]++;
        for (uint32_t d = 0; d < hp.g.r[i]; ++d)
            if (T.np[d] > 0 && bg.lcnt[j][T.lev[d]] > 1) bg.share[j] |= (uint8_t)(1u << T.lev[d]);
    }
    return bg;
}

struct kp_plan {
    kp_ctx *ctx = nullptr;
    kp::host_plan hp;
    uint32_t max_block = 4096;  // the block budget build_plan ran with (kp_plan_block_check rebuilds with it)
    // device tables
    kp_postab *d_tabs = nullptr;
    uint32_t *d_lowinfo = nullptr;
    int32_t *d_loff = nullptr;
    uint32_t *d_klofs = nullptr;
    uint16_t *d_kllist = nullptr;
    uint32_t *d_hlist = nullptr;
    uint32_t *d_kpos = nullptr;
    kp_lowdesc *d_ldesc = nullptr;
    uint64_t *d_hdig = nullptr;
    uint64_t *d_hnp = nullptr;
    uint64_t *d_hpd = nullptr;  // [nblocks][hps] high split pairs per block (kp_hpd_kernel)
    uint32_t hps = 0;
    uint8_t *d_lowmask = nullptr;
    uint32_t *d_lpairs = nullptr;
    // counts
    void *d_K = nullptr;     // [nf + 1][q][kl][2] CT, rows in block-list order (kp_core.h)
    int nf = 0;
    int ct_bytes = 0;
    std::vector<uint8_t> fold_set;  // fold f's slot holds counts (kp_counts_fold / kp_set_counts)
    // kp_counts_fold runs asynchronously on a stream of its own (a fold's table fills while
    // the previous fold's pass runs): pinned + device staging of one fold's counts, the
    // event that frees the pinned copy, and per fold the event its passes wait for
    hipStream_t cstream = nullptr;
    void *h_stage = nullptr, *d_stage = nullptr;
    size_t stage_bytes = 0;
    hipEvent_t stage_ev = nullptr;
    std::vector<hipEvent_t> fold_ev;
    std::vector<uint8_t> fold_async;  // fold f's table was filled on cstream (passes wait on fold_ev[f])
    // lanes
    float *d_S = nullptr;
    bool S_pool = false;  // d_S came from the device's stream-ordered pool (see alloc_scores)
    uint64_t lanes_cap = 0;
    kp_node *d_nodes = nullptr;
    uint32_t node_cap = 0;  // nodes per lane
    kp_group_dev *d_groups = nullptr;
    uint32_t *d_lanegrp = nullptr;
    float *d_rtrain = nullptr, *d_rtest = nullptr;
    uint64_t *d_nleaves = nullptr;
    uint32_t *d_bad = nullptr;
    uint32_t *d_cnt = nullptr;
    uint32_t *d_dend = nullptr;
    uint64_t *d_leaves = nullptr;
    uint64_t small_cap = 0;  // lanes the small buffers above can hold
    uint32_t last_ltot = 0;
    std::vector<kp_group_dev> last_groups;  // device groups of the last pass (dump)
    std::vector<uint32_t> last_lanegrp;
    kp_pass_stats stats{};
    std::vector<hipEvent_t> lev;     // per-launch events (KP_LAUNCH_TIMES=1)
    std::vector<float> launch_ms;    // per-launch times of the last pass (class-major, H ascending)
};

static void free_scores(kp_plan *p);  // the score rows (pool or hipMalloc), defined below

static kp_dev_tables tables_of(const kp_plan *p) {
    kp_dev_tables T;
    T.tabs = p->d_tabs;
    T.lowinfo = p->d_lowinfo;
    T.loff = p->d_loff;
    T.klofs = p->d_klofs;
    T.kllist = p->d_kllist;
    T.hlist = p->d_hlist;
    T.kpos = p->d_kpos;
    T.ldesc = p->d_ldesc;
    T.hdig = p->d_hdig;
    T.hnp = p->d_hnp;
    T.hpd = p->d_hpd;
    T.hps = p->hps;
    T.lowmask = p->d_lowmask;
    T.lpairs = reinterpret_cast<const uint4 *>(p->d_lpairs);
    return T;
}

// nodes of one lane's backtrack tree: at most 2 * leaves - 1 <= 2 * n_kmers - 1
static uint32_t node_cap_of(const kp::host_plan &hp) { return (uint32_t)(2 * hp.n_kmers + 2); }

// The plan's block list built on the device (kp_blocks_kernel): rank table and level
// offsets up, one launch, the small tables freed once it has run.
static int device_blocks(kp_plan *p) {
    const kp_geom &g = p->hp.g;
    uint32_t *d_brank = nullptr, *d_coff = nullptr;
    uint64_t *d_hoff = nullptr;
    int rc;
    if ((rc = upload(&d_brank, p->hp.brank)) || (rc = upload(&d_hoff, p->hp.hoff)) ||
        (p->hp.nfast > 0 && (rc = upload(&d_coff, p->hp.coff)))) {
        dfree(d_brank);
        dfree(d_coff);
        dfree(d_hoff);
        return rc;
    }
    hipError_t he = dmalloc(&p->d_hlist, g.nblocks * sizeof(uint32_t));
    if (he == hipSuccess) he = dmalloc(&p->d_kpos, g.nblocks * sizeof(uint32_t));
    if (he == hipSuccess) he = dmalloc(&p->d_hdig, g.nblocks * sizeof(uint64_t));
    if (he == hipSuccess) he = dmalloc(&p->d_hnp, g.nblocks * sizeof(uint64_t));
    if (he == hipSuccess) {
        const unsigned nb = (unsigned)std::min<uint64_t>((g.nblocks + 255) / 256, 16384);
        hipLaunchKernelGGL(kp_blocks_kernel, dim3(nb), dim3(256), 0, p->ctx->stream, g, p->d_tabs, blockgen_of(p->hp),
                           d_brank, d_coff, d_hoff, p->d_hlist, p->d_kpos, p->d_hdig, p->d_hnp);
        he = hipGetLastError();
        if (he == hipSuccess) he = hipStreamSynchronize(p->ctx->stream);
    }
    dfree(d_brank);
    dfree(d_coff);
    dfree(d_hoff);
    if (he == hipErrorOutOfMemory)  // the block-list tables do not fit: the lattice is too big here
        return fail(KP_E_NOMEM, "block list of " + p->hp.gp + " (" + std::to_string(g.nblocks) +
                                    " blocks): out of device memory");
    if (he != hipSuccess) return fail(KP_E_HIP, std::string("block list: ") + hipGetErrorString(he));
    return KP_OK;
}

extern "C" {

int kp_plan_create(kp_ctx *ctx, const char *gen_pat, uint32_t max_block, kp_plan **out) {
    if (!ctx || !gen_pat || !out) return fail(KP_E_ARG, "null argument");
    KP_HIP(hipSetDevice(ctx->device));
    kp_plan *p = new kp_plan();
    p->ctx = ctx;
    p->max_block = max_block ? max_block : 4096u;
    std::string err = kp::build_plan(gen_pat, p->max_block, p->hp, false);
    if (!err.empty()) {
        delete p;
        return fail(KP_E_ARG, err);
    }
    int rc;
    if ((rc = upload(&p->d_tabs, p->hp.tabs)) || (rc = upload(&p->d_lowinfo, p->hp.lowinfo)) ||
        (rc = upload(&p->d_loff, p->hp.loff)) || (rc = upload(&p->d_klofs, p->hp.klofs)) ||
        (rc = upload(&p->d_kllist, p->hp.kllist)) || (rc = upload(&p->d_ldesc, p->hp.ldesc)) ||
        (rc = upload(&p->d_lowmask, p->hp.lowmask)) || (rc = upload(&p->d_lpairs, p->hp.lpairs))) {
        kp_plan_destroy(p);
        return rc;
    }
    if (p->hp.blocks_on_host) {  // an experiment block order (KP_BLOCK_TILE / KP_BLOCK_ORDER)
        if ((rc = upload(&p->d_hlist, p->hp.hlist)) || (rc = upload(&p->d_kpos, p->hp.kpos)) ||
            (rc = upload(&p->d_hdig, p->hp.hdig)) || (rc = upload(&p->d_hnp, p->hp.hnp))) {
            kp_plan_destroy(p);
            return rc;
        }
    } else if ((rc = device_blocks(p))) {
        kp_plan_destroy(p);
        return rc;
    }
    // the blocks' high split pairs as child-block deltas (one load per pair in the sweep's
    // block setup); only when every block has at most 64 pairs (one wave) and the deltas
    // fit their 29-bit fields -- otherwise the sweep derives them from hdig and tabs
    {
        const kp_geom &g = p->hp.g;
        uint32_t most = 0;
        for (int i = 0; i < g.kh; ++i) {
            uint32_t m = 0;
            for (uint32_t d = 0; d < g.r[g.t + i]; ++d) m = std::max<uint32_t>(m, p->hp.tabs[g.t + i].np[d]);
            most += m;
        }
        if (env_int("KP_HPD", 1) != 0 && most >= 1 && most <= 64 && g.nblocks < (1ull << 29)) {
            // optional: if it cannot be set up (e.g. out of memory) the plan keeps the
            // hdig/tabs setup instead of failing
            hipError_t he = dmalloc(&p->d_hpd, g.nblocks * most * sizeof(uint64_t));
            if (he == hipSuccess) {
                const unsigned nb = (unsigned)std::min<uint64_t>((g.nblocks + 255) / 256, 16384);
                hipLaunchKernelGGL(kp_hpd_kernel, dim3(nb), dim3(256), 0, ctx->stream, g, p->d_tabs, p->d_hdig,
                                   (uint64_t)g.nblocks, most, p->d_hpd);
                he = hipGetLastError();
                if (he == hipSuccess) he = hipStreamSynchronize(ctx->stream);
            }
            if (he == hipSuccess) {
                p->hps = most;
            } else {
                (void)hipGetLastError();  // clear a sticky launch / allocation error
                dfree(p->d_hpd);
                p->d_hpd = nullptr;
                p->hps = 0;
            }
        }
    }
    *out = p;
    return KP_OK;
}

void kp_plan_destroy(kp_plan *p) {
    if (!p) return;
    if (p->ctx) (void)hipSetDevice(p->ctx->device);
    free_scores(p);
    void *bufs[] = {p->d_tabs,    p->d_lowinfo, p->d_loff,   p->d_klofs,   p->d_kllist, p->d_hlist, p->d_kpos, p->d_ldesc,
                    p->d_hdig,    p->d_hnp,     p->d_hpd,     p->d_lowmask, p->d_lpairs, p->d_K,      p->d_nodes, p->d_groups,
                    p->d_lanegrp, p->d_rtrain,  p->d_rtest,  p->d_nleaves, p->d_bad,    p->d_cnt,   p->d_dend,
                    p->d_leaves};
    if (p->cstream) (void)hipStreamSynchronize(p->cstream);
    for (void *b : bufs) dfree(b);
    dfree(p->d_stage);
    if (p->h_stage) (void)hipHostFree(p->h_stage);
    if (p->stage_ev) (void)hipEventDestroy(p->stage_ev);
    for (hipEvent_t e : p->fold_ev) (void)hipEventDestroy(e);
    if (p->cstream) (void)hipStreamDestroy(p->cstream);
    for (hipEvent_t e : p->lev) (void)hipEventDestroy(e);
    delete p;
}

static int wg_lanes(const kp::host_plan &hp, size_t ct_bytes, size_t lds_max);  // defined with the launch code

// ct_bytes / lds_max: the count width and LDS of the plan's device once counts are set
// (lanes_per_workgroup is then what kp_pass uses); 4 bytes and 160 KiB before that
static void info_of(const kp::host_plan &h, kp_plan_info *o, size_t ct_bytes = 4, size_t lds_max = 160u * 1024u) {
    o->npat = h.npat;
    o->nblocks = h.g.nblocks;
    o->n_kmers = h.n_kmers;
    o->block = h.g.B;
    o->block_pad = h.g.Bpad;
    o->k = h.g.k;
    o->low_positions = h.g.t;
    o->max_level = h.maxlev;
    o->high_levels = h.hmax + 1;
    o->pairs_total = h.pairs_total;
    o->pairs_high = h.pairs_high;
    // train scores + backtrack node pool + leaf list
    o->bytes_per_lane = h.g.nblocks * (uint64_t)h.g.Bpad * 4 + (uint64_t)node_cap_of(h) * sizeof(kp_node) +
                        h.n_kmers * 8 + 4096;
    o->lanes_per_workgroup = (uint32_t)wg_lanes(h, ct_bytes, lds_max);
    o->pad_ = 0;
}

int kp_plan_get_info(const kp_plan *p, kp_plan_info *o) {
    if (!p || !o) return fail(KP_E_ARG, "null argument");
    info_of(p->hp, o, p->ct_bytes ? (size_t)p->ct_bytes : 4u, p->ctx ? p->ctx->lds_max : 160u * 1024u);
    return KP_OK;
}

int kp_plan_host(const char *gen_pat, uint32_t max_block, kp_plan_info *o) {
    if (!gen_pat || !o) return fail(KP_E_ARG, "null argument");
    kp::host_plan hp;
    std::string err = kp::build_plan(gen_pat, max_block ? max_block : 4096u, hp, false);
    if (!err.empty()) return fail(KP_E_ARG, err);
    info_of(hp, o);
    return KP_OK;
}

int kp_plan_host_counts(const char *gen_pat, uint32_t max_block, int itype_bytes, kp_plan_info *o) {
    if (!gen_pat || !o || (itype_bytes != 4 && itype_bytes != 8)) return fail(KP_E_ARG, "bad arguments");
    kp::host_plan hp;
    std::string err = kp::build_plan(gen_pat, max_block ? max_block : 4096u, hp, false);
    if (!err.empty()) return fail(KP_E_ARG, err);
    info_of(hp, o, (size_t)itype_bytes);
    return KP_OK;
}

// Host-only (no GPU): the closed-form block order (kp_block_slot) against build_plan's
// block walk, every block of the lattice; *mismatches = blocks whose slot, digits or
// split-pair counts differ.
int kp_block_order_check(const char *gen_pat, uint32_t max_block, uint64_t *mismatches) {
    if (!gen_pat || !mismatches) return fail(KP_E_ARG, "null argument");
    kp::host_plan hp;
    std::string err = kp::build_plan(gen_pat, max_block ? max_block : 4096u, hp, true);
    if (!err.empty()) return fail(KP_E_ARG, err);
    const kp_blockgen bg = blockgen_of(hp);
    uint64_t bad = 0;
    std::vector<uint8_t> seen(hp.g.nblocks, 0);
    for (uint64_t h = 0; h < hp.g.nblocks; ++h) {
        uint64_t hd, hn;
        const uint64_t q = kp_block_slot(hp.g, hp.tabs.data(), bg, hp.brank.data(), hp.coff.data(), hp.hoff.data(), h, &hd, &hn);
        if (q >= hp.g.nblocks || seen[q] || hp.hlist[q] != h || hp.kpos[h] != q || hp.hdig[q] != hd || hp.hnp[q] != hn)
            ++bad;
        else
            seen[q] = 1;
    }
    *mismatches = bad;
    return KP_OK;
}

// Host-only (no GPU): the block list of build_plan's host walk, hlist[nblocks] (blocks in
// list order), and its level offsets hoff[high_levels + 1] (either may be null).
int kp_block_list_host(const char *gen_pat, uint32_t max_block, uint32_t *hlist, uint64_t *hoff) {
    if (!gen_pat) return fail(KP_E_ARG, "null argument");
    kp::host_plan hp;
    std::string err = kp::build_plan(gen_pat, max_block ? max_block : 4096u, hp, true);
    if (!err.empty()) return fail(KP_E_ARG, err);
    if (hlist) memcpy(hlist, hp.hlist.data(), hp.hlist.size() * sizeof(uint32_t));
    if (hoff) memcpy(hoff, hp.hoff.data(), hp.hoff.size() * sizeof(uint64_t));
    return KP_OK;
}

// The plan's device block list (kp_blocks_kernel, or the upload of an experiment order)
// against build_plan's host walk; *mismatches = differing entries of hlist, kpos, hdig
// and hnp together.
int kp_plan_block_check(kp_plan *p, uint64_t *mismatches) {
    if (!p || !mismatches) return fail(KP_E_ARG, "null argument");
    KP_HIP(hipSetDevice(p->ctx->device));
    kp::host_plan hp;  // the host walk with the plan's own block budget
    std::string err = kp::build_plan(p->hp.gp.c_str(), p->max_block, hp, true);
    if (!err.empty()) return fail(KP_E_ARG, err);
    if (hp.g.nblocks != p->hp.g.nblocks || hp.g.B != p->hp.g.B)
        return fail(KP_E_ARG, "the host walk does not rebuild the plan's block size");
    const uint64_t n = hp.g.nblocks;
    std::vector<uint32_t> hl(n), kp(n);
    std::vector<uint64_t> hd(n), hn(n);
    KP_HIP(hipStreamSynchronize(p->ctx->stream));
    KP_HIP(hipMemcpy(hl.data(), p->d_hlist, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    KP_HIP(hipMemcpy(kp.data(), p->d_kpos, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    KP_HIP(hipMemcpy(hd.data(), p->d_hdig, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    KP_HIP(hipMemcpy(hn.data(), p->d_hnp, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    uint64_t bad = 0;
    for (uint64_t q = 0; q < n; ++q)
        bad += (hl[q] != hp.hlist[q]) + (kp[q] != hp.kpos[q]) + (hd[q] != hp.hdig[q]) + (hn[q] != hp.hnp[q]);
    *mismatches = bad;
    return KP_OK;
}

}  // extern "C"
