// kp_math.h -- the device logs of kp_libm.h evaluated on arrays (kp_math_log / kp_math_libm;
// tests and the build-time guard's GPU twin).
#pragma once
#include "kp_libm.h"
#include "kp_rt.h"

// the C library's log (fn 1) or log1p (fn 2) as restated for the device (kp_libm.h), the
// device's own log (fn 0), the table-free fast log (fn 3, kp_fast_log) or its FMA form (fn 4, kp_fma_log)
__global__ void kp_libm_kernel(const double *__restrict__ x, double *__restrict__ y, uint64_t n, int fn) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        y[i] = fn == 1 ? kp_libm_log(x[i]) : fn == 2 ? kp_libm_log1p(x[i]) : fn == 3 ? kp_fast_log(x[i])
             : fn == 4 ? kp_fma_log(x[i]) : log(x[i]);
}

extern "C" {

int kp_math_log(kp_ctx *c, const double *x, double *y, uint64_t n) { return kp_math_libm(c, x, y, n, 0); }

int kp_math_libm(kp_ctx *c, const double *x, double *y, uint64_t n, int fn) {
    if (!c || (n && (!x || !y)) || fn < 0 || fn > 4) return fail(KP_E_ARG, "bad arguments");
    if (!n) return KP_OK;
    KP_HIP(hipSetDevice(c->device));
    double *dx = nullptr, *dy = nullptr;
    KP_HIP(dmalloc(&dx, n * sizeof(double)));
    hipError_t e = dmalloc(&dy, n * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(dx, x, n * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        const unsigned nb = (unsigned)std::min<uint64_t>((n + 255) / 256, 16384);
        hipLaunchKernelGGL(kp_libm_kernel, dim3(nb), dim3(256), 0, c->stream, dx, dy, n, fn);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(y, dy, n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dfree(dx);
    dfree(dy);
    if (e != hipSuccess) return fail(KP_E_HIP, std::string("kp_math_libm: ") + hipGetErrorString(e));
    return KP_OK;
}

}  // extern "C"
