// Squeeze-excite helpers on NCHW activations: per-plane mean (the "squeeze") and the sigmoid gate
// out = x * sigmoid(s[n,c]) with its backward (reference: models/efficientnet_pytorch/model.py:104-110 --
// `x_squeezed = F.adaptive_avg_pool2d(x, 1)` ... `x = torch.sigmoid(x_squeezed) * x`).  HBM streaming: one wave per
// (image, channel) plane, vector loads along the plane's contiguous memory.  The gate's backward makes
// dx = dout * sigmoid(s) and ds = sigmoid'(s) * sum_hw(dout * x) in ONE pass over (dout, x) -- stock autograd takes a
// multiply, another multiply plus a full-size temporary, and a reduction for the same two results.
#include "common.hpp"

namespace moma {
namespace {

constexpr int SE_WAVES = 4;

// out[plane] = mean over the plane (fp32 accumulation)
template <typename T, int VEC>
__global__ __launch_bounds__(SE_WAVES * 64) void plane_mean_kernel(const T* __restrict__ x, T* __restrict__ out, int NC, int HW) {
    const int lane = threadIdx.x & 63;
    const int nv = HW / VEC;
    for (int plane = blockIdx.x * SE_WAVES + (threadIdx.x >> 6); plane < NC; plane += gridDim.x * SE_WAVES) {
        const T* p = x + (size_t)plane * HW;
        float s = 0.f;
        for (int i = lane; i < nv; i += 64) {
            float v[VEC];
            PV<T, VEC>::ld(p + (size_t)i * VEC, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) s += v[j];
        }
        s = wave_sum(s);
        if (lane == 0) st1<T>(out + plane, s / (float)HW);
    }
}

// out = x * sigmoid(s[plane])
template <typename T, int VEC>
__global__ __launch_bounds__(SE_WAVES * 64) void se_gate_fwd_kernel(const T* __restrict__ x, const T* __restrict__ s,
                                                                  T* __restrict__ out, int NC, int HW) {
    const int lane = threadIdx.x & 63;
    const int nv = HW / VEC;
    for (int plane = blockIdx.x * SE_WAVES + (threadIdx.x >> 6); plane < NC; plane += gridDim.x * SE_WAVES) {
        const float g = 1.f / (1.f + __expf(-ld1<T>(s + plane)));
        const T* p = x + (size_t)plane * HW;
        T* o = out + (size_t)plane * HW;
        for (int i = lane; i < nv; i += 64) {
            float v[VEC];
            PV<T, VEC>::ld(p + (size_t)i * VEC, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] *= g;
            PV<T, VEC>::st(o + (size_t)i * VEC, v);
        }
    }
}

// dx = dout * sigmoid(s);  ds[plane] = sigmoid(s) * (1 - sigmoid(s)) * sum(dout * x)
template <typename T, int VEC>
__global__ __launch_bounds__(SE_WAVES * 64) void se_gate_bwd_kernel(const T* __restrict__ x, const T* __restrict__ s,
                                                                  const T* __restrict__ dout, T* __restrict__ dx,
                                                                  T* __restrict__ ds, int NC, int HW) {
    const int lane = threadIdx.x & 63;
    const int nv = HW / VEC;
    for (int plane = blockIdx.x * SE_WAVES + (threadIdx.x >> 6); plane < NC; plane += gridDim.x * SE_WAVES) {
        const float g = 1.f / (1.f + __expf(-ld1<T>(s + plane)));
        const T* p = x + (size_t)plane * HW;
        const T* d = dout + (size_t)plane * HW;
        T* o = dx + (size_t)plane * HW;
        float acc = 0.f;
        for (int i = lane; i < nv; i += 64) {
            float v[VEC], dv[VEC];
            PV<T, VEC>::ld(p + (size_t)i * VEC, v);
            PV<T, VEC>::ld(d + (size_t)i * VEC, dv);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                acc = fmaf(dv[j], v[j], acc);
                dv[j] *= g;
            }
            PV<T, VEC>::st(o + (size_t)i * VEC, dv);
        }
        acc = wave_sum(acc);
        if (lane == 0) st1<T>(ds + plane, acc * g * (1.f - g));
    }
}

unsigned se_grid(int NC) {
    long g = ((long)NC + SE_WAVES - 1) / SE_WAVES;
    if (g > 256 * 32) g = 256 * 32;
    return (unsigned)(g < 1 ? 1 : g);
}
// 16 bytes / 4 elements / 1 (never 2) along the plane; `bits` = the OR of the addresses accessed at that width
template <typename T, typename F> void se_launch(int NC, int HW, uintptr_t bits, F&& f) {
    const int vec = pick_vec(HW, sizeof(T), bits, {MAXVEC<T>, 4});
    with_vec<MAXVEC<T>, 8, 4, 1>(vec, [&](auto V) { f(V, dim3(se_grid(NC)), dim3(SE_WAVES * 64)); });
}
}  // namespace

hipError_t launch_plane_mean(const void* x, void* out, int NC, int HW, int dtype, hipStream_t st) {
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        se_launch<T>(NC, HW, (uintptr_t)x, [&](auto V, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((plane_mean_kernel<T, V>), grid, block, 0, st, (const T*)x, (T*)out, NC, HW);
        });
        return hipGetLastError();
    });
}
hipError_t launch_se_gate_fwd(const void* x, const void* s, void* out, int NC, int HW, int dtype, hipStream_t st) {
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        se_launch<T>(NC, HW, (uintptr_t)x | (uintptr_t)out, [&](auto V, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((se_gate_fwd_kernel<T, V>), grid, block, 0, st, (const T*)x, (const T*)s, (T*)out, NC, HW);
        });
        return hipGetLastError();
    });
}
hipError_t launch_se_gate_bwd(const void* x, const void* s, const void* dout, void* dx, void* ds, int NC, int HW, int dtype,
                              hipStream_t st) {
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        se_launch<T>(NC, HW, (uintptr_t)x | (uintptr_t)dout | (uintptr_t)dx, [&](auto V, dim3 grid, dim3 block) {
            hipLaunchKernelGGL((se_gate_bwd_kernel<T, V>), grid, block, 0, st, (const T*)x, (const T*)s, (const T*)dout, (T*)dx,
                               (T*)ds, NC, HW);
        });
        return hipGetLastError();
    });
}

}  // namespace moma
