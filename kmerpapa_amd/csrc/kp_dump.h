// kp_dump.h -- parity dumps of the last pass: every cell's score and argmin code of one
// lane (kp_dump_lane) and the scores of chosen cells (kp_gather_cells).
#pragma once
#include "kp_bt.h"
#include "kp_plan_dev.h"

// float32 scores of the given cells of one lane (parity checks of a full-size pass: the
// cells of an embedded sub-lattice, against the oracle run on that sub-lattice alone)
__global__ void kp_gather_cells_kernel(kp_geom g, const float *__restrict__ S, uint32_t lane,
                                       const uint64_t *__restrict__ cells, uint64_t n, float *__restrict__ out) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t x = cells[i];
        out[i] = S[kp_s_off(g, x / g.B, lane, (uint32_t)(x % g.B))];
    }
}

// argmin code of every cell of one lane (parity dumps): the sequential decision of kp_core.h
template <typename CT>
__global__ void kp_codes_kernel(kp_geom g, kp_dev_tables T, const CT *K, const float *S, kp_group_dev G,
                                uint32_t lane, double pen, uint8_t *code) {
    const uint64_t npat = g.nblocks * g.B;
    for (uint64_t x = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; x < npat;
         x += (uint64_t)gridDim.x * blockDim.x) {
        const kp_cnt c = kp_cell_counts<CT>(g, T.klofs, T.kllist, K, x, G.fold, T.kpos);
        const uint64_t dig = kp_cell_digits(g, x);
        auto score = [&](uint64_t y) { return S[kp_s_off(g, y / g.B, lane, (uint32_t)(y % g.B))]; };
        float v;
        const int jl = (int)(lane - (uint32_t)G.lane0);
        code[x] = (uint8_t)kp_cell_decide(g, T.tabs, x, dig, score, c, kp_lane_alpha(G, jl), kp_lane_beta(G, jl), pen,
                                          &v);
    }
}

template <typename CT>
static int run_codes(kp_plan *p, uint32_t lane, uint8_t *code) {
    kp_ctx *c = p->ctx;
    const kp::host_plan &hp = p->hp;
    kp_geom g = hp.g;
    g.nf = p->nf;
    g.Ltot = p->last_ltot;
    const kp_group_dev &G = p->last_groups[p->last_lanegrp[lane]];
    const double pen = G.pen[lane - (uint32_t)G.lane0];
    uint8_t *d_code = nullptr;
    KP_HIP(dmalloc(&d_code, hp.npat));
    for (int f = 0; f < p->nf; ++f)  // a fold table refilled since the pass may still be filling
        if (p->fold_async[f]) KP_HIP(hipStreamWaitEvent(c->stream, p->fold_ev[f], 0));
    const unsigned nb = (unsigned)std::min<uint64_t>((hp.npat + 255) / 256, 65535);
    hipLaunchKernelGGL(kp_codes_kernel<CT>, dim3(nb), dim3(256), 0, c->stream, g, tables_of(p),
                       reinterpret_cast<const CT *>(p->d_K), p->d_S, G, lane, pen, d_code);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(code, d_code, hp.npat, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dfree(d_code);
    if (e != hipSuccess) return fail(KP_E_HIP, std::string("codes kernel: ") + hipGetErrorString(e));
    return KP_OK;
}

extern "C" {

int kp_dump_lane(kp_plan *p, uint32_t lane, float *score, uint8_t *code) {
    if (!p) return fail(KP_E_ARG, "null argument");
    if (lane >= p->last_ltot) return fail(KP_E_STATE, "lane not in last pass");
    KP_HIP(hipSetDevice(p->ctx->device));
    const kp_geom &g = p->hp.g;
    const uint64_t ltot = p->last_ltot;
    if (score) {
        std::vector<float> rowf(g.Bpad);
        for (uint64_t h = 0; h < g.nblocks; ++h) {
            uint64_t off = (h * ltot + lane) * (uint64_t)g.Bpad;
            KP_HIP(hipMemcpy(rowf.data(), p->d_S + off, g.Bpad * sizeof(float), hipMemcpyDeviceToHost));
            memcpy(score + h * g.B, rowf.data(), g.B * sizeof(float));
        }
    }
    if (code) return p->ct_bytes == 4 ? run_codes<uint32_t>(p, lane, code) : run_codes<uint64_t>(p, lane, code);
    return KP_OK;
}

int kp_gather_cells(kp_plan *p, uint32_t lane, const uint64_t *cells, uint64_t n, float *out) {
    if (!p || (n && (!cells || !out))) return fail(KP_E_ARG, "null argument");
    if (lane >= p->last_ltot) return fail(KP_E_STATE, "lane not in last pass");
    for (uint64_t i = 0; i < n; ++i)
        if (cells[i] >= p->hp.npat) return fail(KP_E_ARG, "cell " + std::to_string(cells[i]) + " out of range");
    if (!n) return KP_OK;
    KP_HIP(hipSetDevice(p->ctx->device));
    kp_ctx *c = p->ctx;
    kp_geom g = p->hp.g;
    g.Ltot = p->last_ltot;
    const uint64_t chunk = std::min<uint64_t>(n, 1ull << 26);
    uint64_t *d_cells = nullptr;
    float *d_out = nullptr;
    KP_HIP(dmalloc(&d_cells, chunk * sizeof(uint64_t)));
    hipError_t e = dmalloc(&d_out, chunk * sizeof(float));
    for (uint64_t i0 = 0; i0 < n && e == hipSuccess; i0 += chunk) {
        const uint64_t m = std::min(chunk, n - i0);
        e = hipMemcpyAsync(d_cells, cells + i0, m * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) break;
        const unsigned nb = (unsigned)std::min<uint64_t>((m + 255) / 256, 65536);
        hipLaunchKernelGGL(kp_gather_cells_kernel, dim3(nb), dim3(256), 0, c->stream, g, p->d_S, lane, d_cells, m,
                           d_out);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out + i0, d_out, m * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    dfree(d_cells);
    dfree(d_out);
    if (e != hipSuccess) return fail(KP_E_HIP, std::string("kp_gather_cells: ") + hipGetErrorString(e));
    return KP_OK;
}

}  // extern "C"
