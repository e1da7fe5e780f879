// kp_greedy_api.h -- the host drivers of the greedy top-down partition (kp_greedy.h):
// kp_greedy, kp_greedy_host, kp_greedy_leaves, kp_greedy_last_stats.
#pragma once
#include "kp_greedy.h"
#include "kp_rt.h"

static thread_local std::vector<std::vector<uint64_t>> g_greedy_host_leaves;  // kp_greedy_host's partitions

// Arguments of kp_greedy / kp_greedy_host: the root tables, the column totals (refused at
// 2^53, where the reference's float64 sums stop being exact) and the number of chains.
static int greedy_check(const char *who, const char *gen_pat, const uint64_t *M, const uint64_t *U, uint64_t n_kmers,
                        int nf, const kp_greedy_lane *lanes, int n_lanes, double *loss, uint64_t *n_leaves,
                        kp_g_root *R, std::vector<uint64_t> *totM, std::vector<uint64_t> *totU, int *n_chains) {
    const std::string w(who);
    if (!gen_pat || !M || !U || nf < 0 || n_lanes < 0 || (n_lanes && (!lanes || !loss || !n_leaves)))
        return fail(KP_E_ARG, w + ": bad arguments");
    if (strlen(gen_pat) > KP_G_MAXK)
        return fail(KP_E_ARG, w + ": patterns longer than 16 positions do not fit the 64-bit pattern word");
    if (!kp_g_make_root(gen_pat, R)) return fail(KP_E_ARG, w + ": bad general pattern (IUPAC codes, at most 2^30 k-mers)");
    if (kp_g_generality(R->pat, R->k) != n_kmers)
        return fail(KP_E_ARG, w + ": n_kmers is not the number of k-mers of the general pattern");
    const int nfc = nf > 1 ? nf : 1;
    totM->assign(nfc, 0);
    totU->assign(nfc, 0);
    const uint64_t lim = 1ull << 53;
    uint64_t am = 0, au = 0;
    for (int f = 0; f < nfc; ++f) {
        uint64_t sm = 0, su = 0;
        for (uint64_t i = 0; i < n_kmers; ++i) {
            const uint64_t m = M[i * nfc + f], u = U[i * nfc + f];
            if (m >= lim || u >= lim) return fail(KP_E_ARG, w + ": a count of 2^53 or more");
            sm += m;
            su += u;
            if (sm >= lim || su >= lim) return fail(KP_E_ARG, w + ": count totals of 2^53 or more are not exact in float64");
        }
        (*totM)[f] = sm;
        (*totU)[f] = su;
        am += sm;
        au += su;
        if (am >= lim || au >= lim || am + au >= lim)
            return fail(KP_E_ARG, w + ": count totals of 2^53 or more are not exact in float64");
    }
    *n_chains = 0;
    for (int i = 0; i < n_lanes; ++i) {
        if (lanes[i].fold < -1 || lanes[i].fold >= (nf > 1 ? nf : 0))
            return fail(KP_E_ARG, w + ": a lane's fold is not -1 or one of the fold tables");
        if (lanes[i].chain < -1) return fail(KP_E_ARG, w + ": a lane's chain is below -1");
        *n_chains = std::max(*n_chains, lanes[i].chain + 1);
    }
    return KP_OK;
}

static uint32_t greedy_chunk() {
    long v = env_int("KP_GREEDY_CHUNK", 0);
    if (v < 1) v = 4096;
    return (uint32_t)std::min<long>(v, 1l << 24);
}

extern "C" {

int kp_greedy_host(const char *gen_pat, const uint64_t *M, const uint64_t *U, uint64_t n_kmers, int nf,
                   const kp_greedy_lane *lanes, int n_lanes, double *loss, double *chain_test, uint64_t *n_leaves) {
    kp_g_root R;
    std::vector<uint64_t> totM, totU;
    int n_chains = 0;
    int rc = greedy_check("kp_greedy_host", gen_pat, M, U, n_kmers, nf, lanes, n_lanes, loss, n_leaves, &R, &totM, &totU,
                          &n_chains);
    if (rc) return rc;
    if (n_chains && !chain_test) return fail(KP_E_ARG, "kp_greedy_host: chain_test is null");
    for (int c = 0; c < n_chains; ++c) chain_test[c] = 0.0;
    const int nfc = nf > 1 ? nf : 1;
    uint64_t am = 0, au = 0;
    for (int f = 0; f < nfc; ++f) {
        am += totM[f];
        au += totU[f];
    }
    g_greedy_host_leaves.assign(n_lanes, {});
    for (int i = 0; i < n_lanes; ++i) {
        kp_g_host_job J;
        J.root = R;
        J.M = M;
        J.U = U;
        J.n = n_kmers;
        J.nfc = nfc;
        J.P = lanes[i];
        J.leaves = &g_greedy_host_leaves[i];
        J.chain = lanes[i].chain >= 0 ? &chain_test[lanes[i].chain] : nullptr;
        uint64_t c[4] = {am, au, 0, 0};
        if (lanes[i].fold >= 0) {
            c[2] = totM[lanes[i].fold];
            c[3] = totU[lanes[i].fold];
            c[0] -= c[2];
            c[1] -= c[3];
        }
        loss[i] = kp_g_host_node(J, R.pat, c);
        n_leaves[i] = J.leaves->size();
    }
    return KP_OK;
}

int kp_greedy_leaves(kp_ctx *c, uint32_t lane, uint64_t *patterns, uint64_t cap, uint64_t *n_out) {
    const std::vector<std::vector<uint64_t>> &all = c ? c->g_leaves : g_greedy_host_leaves;
    if (lane >= all.size()) return fail(KP_E_ARG, "kp_greedy_leaves: no such lane in the last greedy call");
    const std::vector<uint64_t> &v = all[lane];
    if (n_out) *n_out = v.size();
    if (patterns) memcpy(patterns, v.data(), std::min<uint64_t>(cap, v.size()) * sizeof(uint64_t));
    return KP_OK;
}

int kp_greedy_last_stats(kp_ctx *c, kp_greedy_stats *out) {
    if (!c || !out) return fail(KP_E_ARG, "kp_greedy_last_stats: bad arguments");
    *out = c->g_stats;
    return KP_OK;
}

int kp_greedy(kp_ctx *c, const char *gen_pat, const uint64_t *M, const uint64_t *U, uint64_t n_kmers, int nf,
              const kp_greedy_lane *lanes, int n_lanes, double *loss, double *chain_test, uint64_t *n_leaves) {
    if (!c) return fail(KP_E_ARG, "kp_greedy: null ctx");
    if (c->seq.active) return fail(KP_E_STATE, "kp_greedy: a kp_seq session holds the context's arena (kp_seq_end first)");
    if (c->pred.active) return fail(KP_E_STATE, "kp_greedy: a kp_pred session holds the context's arena (kp_pred_end first)");
    if (c->spec.active) return fail(KP_E_STATE, "kp_greedy: a kp_spec session holds the context's arena (kp_spec_end first)");
    if (c->ispec.active) return fail(KP_E_STATE, "kp_greedy: a kp_ispec session holds the context's arena (kp_ispec_end first)");
    kp_g_root R;
    std::vector<uint64_t> totM, totU;
    int n_chains = 0;
    int rc = greedy_check("kp_greedy", gen_pat, M, U, n_kmers, nf, lanes, n_lanes, loss, n_leaves, &R, &totM, &totU,
                          &n_chains);
    if (rc) return rc;
    if (n_chains && !chain_test) return fail(KP_E_ARG, "kp_greedy: chain_test is null");
    c->g_leaves.assign(n_lanes, {});
    c->g_stats = kp_greedy_stats{};
    const auto t_start = std::chrono::steady_clock::now();
    if (!n_lanes) return KP_OK;
    KP_HIP(hipSetDevice(c->device));
    const int nfc = nf > 1 ? nf : 1;
    const int nslots = nf > 1 ? nf + 1 : 1;
    const uint64_t n = n_kmers;
    const uint32_t chunk = greedy_chunk();
    uint64_t am = 0, au = 0;
    for (int f = 0; f < nfc; ++f) {
        am += totM[f];
        au += totU[f];
    }

    // memory: the tables, then per lane the worst-case node pool (2 n - 1 nodes), two item
    // lists, the histogram slots of multi-chunk nodes and the leaf outputs
    const uint64_t node_cap = 2 * n + 1;
    const uint64_t items_pl = n / 2 + n / chunk + 2;
    const uint64_t big_pl = n / chunk + 1;
    const size_t raw_bytes = g_up(n * (size_t)nfc * 8);
    const size_t fixed = 2 * raw_bytes + g_up((size_t)nslots * n * 16) + g_up((size_t)std::max(n_chains, 1) * 8) + 4096;
    const size_t per_lane = g_up(node_cap * sizeof(kp_g_node)) + 2 * g_up(items_pl * sizeof(kp_g_item)) +
                            g_up(big_pl * KP_G_HSIZE * 8) + 2 * g_up(big_pl * 8) + 2 * g_up(n * 8) +
                            (KP_G_MAXDEPTH + 4) * 4 + sizeof(kp_greedy_lane) + 16 + 1024;
    size_t budget = 0;
    if (const char *e = getenv("KP_GREEDY_MEM")) {
        budget = (size_t)strtoull(e, nullptr, 10);
    } else {
        size_t fr = 0, tot = 0;
        KP_HIP(hipMemGetInfo(&fr, &tot));
        fr += c->arena.bytes;  // the arena is ours to reuse
        budget = fr > (2ull << 30) ? fr - (2ull << 30) : 0;
    }
    if (budget < fixed + per_lane)
        return fail(KP_E_NOMEM, "kp_greedy: the count tables (" + std::to_string(fixed >> 20) + " MiB) and one lane's tree (" +
                                    std::to_string(per_lane >> 20) + " MiB) do not fit the device memory available (" +
                                    std::to_string(budget >> 20) + " MiB)");
    const uint32_t Lb = (uint32_t)std::min<uint64_t>((budget - fixed) / per_lane, (uint64_t)n_lanes);
    if ((uint64_t)Lb * items_pl >= (1ull << 32) || (uint64_t)Lb * big_pl >= (1ull << 32))
        return fail(KP_E_ARG, "kp_greedy: too many work items for one batch");
    const size_t need = fixed + (size_t)Lb * per_lane;
    if ((rc = c->arena.reserve("kp_greedy", need))) return rc;
    auto take = [&](size_t bytes) { return c->arena.take(bytes); };
    uint64_t *dM = (uint64_t *)take(raw_bytes), *dU = (uint64_t *)take(raw_bytes);
    ulonglong2 *d_tab = (ulonglong2 *)take((size_t)nslots * n * 16);
    double *d_acc = (double *)take((size_t)std::max(n_chains, 1) * 8);
    uint32_t *d_counters = (uint32_t *)take(64);
    kp_g_node *d_nodes = (kp_g_node *)take((size_t)Lb * node_cap * sizeof(kp_g_node));
    kp_g_item *d_items[2] = {(kp_g_item *)take((size_t)Lb * items_pl * sizeof(kp_g_item)),
                             (kp_g_item *)take((size_t)Lb * items_pl * sizeof(kp_g_item))};
    unsigned long long *d_H = (unsigned long long *)take((size_t)Lb * big_pl * KP_G_HSIZE * 8);
    uint2 *d_meta[2] = {(uint2 *)take((size_t)Lb * big_pl * 8), (uint2 *)take((size_t)Lb * big_pl * 8)};
    uint64_t *d_lpat = (uint64_t *)take((size_t)Lb * n * 8);
    double *d_lterm = (double *)take((size_t)Lb * n * 8);
    uint32_t *d_cnt = (uint32_t *)take((size_t)Lb * 4);
    uint32_t *d_dend = (uint32_t *)take((size_t)Lb * KP_G_MAXDEPTH * 4);
    kp_greedy_lane *d_lanes = (kp_greedy_lane *)take((size_t)Lb * sizeof(kp_greedy_lane));
    double *d_loss = (double *)take((size_t)Lb * 8);
    uint64_t *d_nl = (uint64_t *)take((size_t)Lb * 8);
    if ((rc = c->arena.check("kp_greedy"))) return rc;

    hipStream_t st = c->stream;
    KP_HIP(hipMemcpyAsync(dM, M, n * (size_t)nfc * 8, hipMemcpyHostToDevice, st));
    KP_HIP(hipMemcpyAsync(dU, U, n * (size_t)nfc * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kp_greedy_tab, dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 16384)), dim3(256), 0, st, dM, dU,
                       n, nfc, nslots, d_tab);
    KP_HIP(hipGetLastError());
    KP_HIP(hipMemsetAsync(d_acc, 0, (size_t)std::max(n_chains, 1) * 8, st));
    KP_HIP(hipMemsetAsync(d_H, 0, (size_t)Lb * big_pl * KP_G_HSIZE * 8, st));

    const uint32_t root_nch = n >= 2 ? (uint32_t)((n + chunk - 1) / chunk) : 0;
    for (int l0 = 0; l0 < n_lanes; l0 += (int)Lb) {
        const uint32_t nl = (uint32_t)std::min<int>((int)Lb, n_lanes - l0);
        ++c->g_stats.batches;
        kp_g_args A;
        A.root = R;
        A.tab = d_tab;
        A.n = n;
        A.nslots = nslots;
        A.chunk = chunk;
        A.lanes = d_lanes;
        A.nodes = d_nodes;
        A.node_cap = (uint32_t)node_cap;
        A.cnt = d_cnt;
        A.Hbig = d_H;
        A.item_cap = (uint32_t)(Lb * items_pl);
        A.big_cap = (uint32_t)(Lb * big_pl);
        A.counters = d_counters;
        // depth 0: every lane's root with its own loss, and its items
        std::vector<kp_g_item> items;
        std::vector<uint2> meta;
        std::vector<uint32_t> ones(nl, 1);
        std::vector<kp_g_node> roots(nl);
        for (uint32_t L = 0; L < nl; ++L) {
            const kp_greedy_lane &P = lanes[l0 + L];
            kp_g_node &r = roots[L];
            memset(&r, 0, sizeof(r));
            r.pat = R.pat;
            r.c[0] = am;
            r.c[1] = au;
            if (P.fold >= 0) {
                r.c[2] = totM[P.fold];
                r.c[3] = totU[P.fold];
                r.c[0] -= r.c[2];
                r.c[1] -= r.c[3];
            }
            r.value = kp_g_train_loss(r.c[0], r.c[1], P.alpha, P.beta, P.penalty);
            r.nl = 1;
            KP_HIP(hipMemcpyAsync(d_nodes + (uint64_t)L * node_cap, &r, sizeof(r), hipMemcpyHostToDevice, st));
            uint32_t big = 0;
            if (root_nch > 1) {
                big = (uint32_t)meta.size();
                meta.push_back(make_uint2(L, 0));
            }
            for (uint32_t q = 0; q < root_nch; ++q) items.push_back(kp_g_item{L, 0, q, big});
        }
        KP_HIP(hipMemcpyAsync(d_lanes, lanes + l0, nl * sizeof(kp_greedy_lane), hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(d_cnt, ones.data(), nl * 4, hipMemcpyHostToDevice, st));
        KP_HIP(hipMemcpyAsync(d_dend, ones.data(), nl * 4, hipMemcpyHostToDevice, st));
        if (!items.empty())
            KP_HIP(hipMemcpyAsync(d_items[0], items.data(), items.size() * sizeof(kp_g_item), hipMemcpyHostToDevice, st));
        if (!meta.empty()) KP_HIP(hipMemcpyAsync(d_meta[0], meta.data(), meta.size() * 8, hipMemcpyHostToDevice, st));
        KP_HIP(hipStreamSynchronize(st));
        uint32_t n_items = (uint32_t)items.size(), n_big = (uint32_t)meta.size();
        KP_HIP(hipMemsetAsync(d_counters, 0, 64, st));
        int depths = 1, cur = 0;
        while (n_items) {
            if (depths >= KP_G_MAXDEPTH) return fail(KP_E_PARITY, "kp_greedy: the tree is deeper than any pattern allows");
            KP_HIP(hipMemsetAsync(d_counters, 0, 12, st));
            KP_HIP(hipEventRecord(c->ev[0], st));
            A.next = d_items[cur ^ 1];
            A.bigmeta_cur = d_meta[cur];
            A.bigmeta_next = d_meta[cur ^ 1];
            hipLaunchKernelGGL(kp_greedy_hist, dim3((n_items + KP_G_WAVES - 1) / KP_G_WAVES), dim3(64 * KP_G_WAVES), 0, st, A,
                               d_items[cur], n_items);
            KP_HIP(hipGetLastError());
            KP_HIP(hipEventRecord(c->ev[1], st));
            if (n_big) {
                hipLaunchKernelGGL(kp_greedy_decide_big, dim3((n_big + KP_G_WAVES - 1) / KP_G_WAVES), dim3(64 * KP_G_WAVES), 0,
                                   st, A, n_big);
                KP_HIP(hipGetLastError());
            }
            KP_HIP(hipMemcpyAsync(d_dend + (uint64_t)depths * nl, d_cnt, nl * 4, hipMemcpyDeviceToDevice, st));
            uint32_t h[3] = {0, 0, 0};
            KP_HIP(hipMemcpyAsync(h, d_counters, 12, hipMemcpyDeviceToHost, st));
            KP_HIP(hipStreamSynchronize(st));
            if (h[2]) return fail(KP_E_PARITY, "kp_greedy: a node pool or work list overflowed (error word " +
                                                   std::to_string(h[2]) + ")");
            float ms = 0.f;
            KP_HIP(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
            c->g_stats.hist_ms += ms;
            c->g_stats.items += n_items;
            ++depths;
            n_items = h[0];
            n_big = h[1];
            cur ^= 1;
        }
        c->g_stats.depths = std::max<uint32_t>(c->g_stats.depths, (uint32_t)depths);
        {
            unsigned long long fk = 0;
            KP_HIP(hipMemcpyAsync(&fk, d_counters + 4, 8, hipMemcpyDeviceToHost, st));
            KP_HIP(hipStreamSynchronize(st));
            c->g_stats.frontier_kmers += fk + (n >= 2 ? (uint64_t)nl * n : 0);
        }
        hipLaunchKernelGGL(kp_greedy_finish, dim3(nl), dim3(1024), 0, st, A, d_dend, depths, nl, d_lpat, d_lterm, d_loss,
                           d_nl);
        KP_HIP(hipGetLastError());
        if (n_chains) {
            hipLaunchKernelGGL(kp_greedy_chain, dim3((n_chains + 63) / 64), dim3(64), 0, st, d_lanes, nl, n, d_lterm, d_nl,
                               n_chains, d_acc);
            KP_HIP(hipGetLastError());
        }
        KP_HIP(hipMemcpyAsync(loss + l0, d_loss, nl * 8, hipMemcpyDeviceToHost, st));
        KP_HIP(hipMemcpyAsync(n_leaves + l0, d_nl, nl * 8, hipMemcpyDeviceToHost, st));
        KP_HIP(hipStreamSynchronize(st));
        for (uint32_t L = 0; L < nl; ++L) {
            std::vector<uint64_t> &v = c->g_leaves[l0 + L];
            if (n_leaves[l0 + L] > n) return fail(KP_E_PARITY, "kp_greedy: more leaves than k-mers");
            v.resize(n_leaves[l0 + L]);
            KP_HIP(hipMemcpyAsync(v.data(), d_lpat + (uint64_t)L * n, v.size() * 8, hipMemcpyDeviceToHost, st));
        }
        KP_HIP(hipStreamSynchronize(st));
    }
    if (n_chains) KP_HIP(hipMemcpy(chain_test, d_acc, (size_t)n_chains * 8, hipMemcpyDeviceToHost));
    c->g_stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return KP_OK;
}

}  // extern "C"
