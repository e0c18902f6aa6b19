// BN1 + activation applied INSIDE the squeeze-excite gate of an MBConv block, forward and backward.  With D the depthwise
// output, A1 = act(BN1(D)) rounded to the storage type, s the gate logits and G = A1 * sigmoid(s), the chain of bn.hip and se.hip
//   forward : bn_stats (read D), bn_apply_mean (read D, write A1 + pooled), se_gate_fwd (read A1, write G)       4 passes behind
//   backward: se_gate_bwd (read A1, dG, write dA1), bn_bwd_reduce (read D, dA1), bn_bwd_apply (read D, dA1,      the statistics,
//             write dD)                                                                                         8 passes
// becomes
//   forward : bn_stats (read D), bn_act_mean (read D -> pooled), bn_act_gate_fwd (read D, write G)               3 passes
//   backward: bn_gate_bwd_sums (read D, dG), bn_gate_bwd_apply (read D, dG, write dD)                            5 passes
//             (between the two: bn_gate_ds, one thread per plane, and bn_gate_bwd_finalize, one wave per channel)
// and A1 is neither written nor kept for the backward.  The forward's results are those of the old chain bit for bit: the
// read-only pass adds up the unrounded fp32 activations in the walk of bn_apply_mean_kernel, and the gate rounds every activation
// to the storage type before it multiplies.  The backward needs no dA1: BN's backward is linear in
//   dy = (dG * sigmoid(s) + dpooled / HW) * act'(y),
// and sigmoid(s) and dpooled are constant over a plane, so the channel sums of dy and dy * xhat follow from four sums per plane
// (P1 = sum dG act', P2 = sum act', P3 = sum dG act' xhat, P4 = sum act' xhat), taken before dpooled -- which depends on ds, a fifth
// sum of the same pass -- exists.  One wave per (image, channel) plane throughout, lane-strided vectors along the plane, no atomics.
#include "common.hpp"

namespace moma {
namespace {

constexpr int GW = 4;                     // waves (planes) per workgroup

template <typename T> __device__ __forceinline__ float round_storage(float v);
template <> __device__ __forceinline__ float round_storage<float>(float v) { return v; }
template <> __device__ __forceinline__ float round_storage<bf16_raw>(float v) { return bf16_to_f32(f32_to_bf16(v)); }

__device__ __forceinline__ float sigmoid_gate(float s) { return 1.f / (1.f + __expf(-s)); }      // se.hip's formula (forward)
// the backward's gate, once per plane: the derivative of the function, not of the forward's rounding of it (v_exp_f32 leaves
// ~1e-7 of sigmoid, which times a plane sum of sqrt(HW) terms would be the largest single error of dgamma / dbeta in fp32)
__device__ __forceinline__ double sigmoid_f64(float s) { return 1.0 / (1.0 + exp(-(double)s)); }

// Sum over the 64 lanes in DOUBLE, the same bits in every lane, without LDS: the butterfly of common.hpp's half32_sum (four DPP
// rotations inside the 16-lane rows, v_permlane16_swap across the rows of a half, v_permlane32_swap across the halves) on the
// two words of a double.  The lanes add up their own few elements in fp32; everything wider -- this tree, the plane sums in the
// workspace, the per-channel combine -- is double, so that re-associating BN's channel sums into plane sums (sigmoid(s) and
// dpooled are factored out of sums of their own) costs no accuracy against the one-level sums of bn.hip.
__device__ __forceinline__ double f64_of(unsigned lo, unsigned hi) { return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)); }
template <int CTRL>
__device__ __forceinline__ double dpp_row_f64(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, false);
    return f64_of(lo, hi);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
    v += dpp_row_f64<0x128>(v);            // row_ror:8
    v += dpp_row_f64<0x124>(v);            // row_ror:4
    v += dpp_row_f64<0x122>(v);            // row_ror:2
    v += dpp_row_f64<0x121>(v);            // row_ror:1
    unsigned long long u = (unsigned long long)__double_as_longlong(v);
    auto rl = __builtin_amdgcn_permlane16_swap((unsigned)u, (unsigned)u, false, false);           // [0]: even rows, [1]: odd rows
    auto rh = __builtin_amdgcn_permlane16_swap((unsigned)(u >> 32), (unsigned)(u >> 32), false, false);
    v = f64_of(rl[0], rh[0]) + f64_of(rl[1], rh[1]);
    u = (unsigned long long)__double_as_longlong(v);
    rl = __builtin_amdgcn_permlane32_swap((unsigned)u, (unsigned)u, false, false);                // [0]: low half, [1]: high half
    rh = __builtin_amdgcn_permlane32_swap((unsigned)(u >> 32), (unsigned)(u >> 32), false, false);
    return f64_of(rl[0], rh[0]) + f64_of(rl[1], rh[1]);
}

// the backward's view of one element: pre-activation y = x * scale + shift as the forward formed it, act(y) and act'(y).
// One reciprocal serves both (v_rcp_f32, 1 ulp: a gradient, not a result that has to reproduce another kernel's bits).
__device__ __forceinline__ void act_both(float y, int act, float& a, float& da) {
    if (act == MOMA_ACT_SILU) {
        const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-y));
        a = y * sg;
        da = sg * (1.f + y * (1.f - sg));
    } else if (act == MOMA_ACT_RELU) {
        a = fmaxf(y, 0.f);
        da = y > 0.f ? 1.f : 0.f;
    } else {
        a = y;
        da = 1.f;
    }
}

// pooled[plane] = mean_hw act(x * scale + shift): bn_apply_mean_kernel (bn.hip) without its store -- the same lanes add the same
// unrounded values in the same order
template <typename T, int VEC>
__global__ __launch_bounds__(GW * 64) void bn_act_mean_kernel(const T* __restrict__ x, T* __restrict__ pmean,
                                                               const float* __restrict__ scale_shift, int NC, int C, int HW,
                                                               int act) {
    const int lane = threadIdx.x & 63;
    const int nv = HW / VEC;
    for (int plane = blockIdx.x * GW + (threadIdx.x >> 6); plane < NC; plane += gridDim.x * GW) {
        const int c = plane % C;
        const float sc = scale_shift[2 * c], sh = scale_shift[2 * c + 1];
        const T* p = x + (size_t)plane * HW;
        float acc = 0.f;
        for (int i = lane; i < nv; i += 64) {
            float v[VEC];
            PV<T, VEC>::ld(p + (size_t)i * VEC, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                v[j] = act_fwd(fmaf(v[j], sc, sh), act);
                acc += v[j];
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) {
            float m[1] = {acc / (float)HW};
            PV<T, 1>::st(pmean + plane, m);
        }
    }
}

// out = round_T(act(x * scale + shift)) * sigmoid(s[plane])
template <typename T, int VEC>
__global__ __launch_bounds__(GW * 64) void bn_act_gate_fwd_kernel(const T* __restrict__ x, const T* __restrict__ s,
                                                                   T* __restrict__ out, const float* __restrict__ scale_shift,
                                                                   int NC, int C, int HW, int act) {
    const int lane = threadIdx.x & 63;
    const int nv = HW / VEC;
    for (int plane = blockIdx.x * GW + (threadIdx.x >> 6); plane < NC; plane += gridDim.x * GW) {
        const int c = plane % C;
        const float sc = scale_shift[2 * c], sh = scale_shift[2 * c + 1];
        const float g = sigmoid_gate(ld1<T>(s + plane));
        const T* p = x + (size_t)plane * HW;
        T* o = out + (size_t)plane * HW;
        for (int i = lane; i < nv; i += 64) {
            float v[VEC];
            PV<T, VEC>::ld(p + (size_t)i * VEC, v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) v[j] = round_storage<T>(act_fwd(fmaf(v[j], sc, sh), act)) * g;
            PV<T, VEC>::st(o + (size_t)i * VEC, v);
        }
    }
}

// per plane: psums[plane] = (P1, P2, P3, P4, sum dG * round_T(A1))
template <typename T, int VEC>
__global__ __launch_bounds__(GW * 64) void bn_gate_bwd_sums_kernel(const T* __restrict__ x, const T* __restrict__ dout,
                                                                    const float* __restrict__ scale_shift,
                                                                    const float* __restrict__ save_mean,
                                                                    const float* __restrict__ save_invstd,
                                                                    double* __restrict__ psums, int NC, int C, int HW, int act) {
    const int lane = threadIdx.x & 63;
    const int nv = HW / VEC;
    for (int plane = blockIdx.x * GW + (threadIdx.x >> 6); plane < NC; plane += gridDim.x * GW) {
        const int c = plane % C;
        const float sc = scale_shift[2 * c], sh = scale_shift[2 * c + 1];
        const float mean = save_mean[c], invstd = save_invstd[c];
        const T* p = x + (size_t)plane * HW;
        const T* d = dout + (size_t)plane * HW;
        // a lane's own sums: one level above the storage type, like everything behind them (fp32 tensors bring twice the bytes per
        // element, which pays for the double adds; under bf16 operands the fp32 sums' rounding does not show)
        using Acc = std::conditional_t<std::is_same<T, float>::value, double, float>;
        Acc p1 = 0, p2 = 0, p3 = 0, p4 = 0, acc = 0;
        for (int i = lane; i < nv; i += 64) {
            float xv[VEC], dv[VEC];
            PV<T, VEC>::ld(p + (size_t)i * VEC, xv);
            PV<T, VEC>::ld(d + (size_t)i * VEC, dv);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float xh = (xv[j] - mean) * invstd;
                const float y = fmaf(xv[j], sc, sh);
                float a, da;
                act_both(y, act, a, da);
                // fp32 storage keeps every bit of the forward's activation: its own formula (an IEEE division); under the bf16
                // rounding below the reciprocal's last bit does not show
                if constexpr (std::is_same<T, float>::value) a = act_fwd(y, act);
                const float u = dv[j] * da;
                p1 += (Acc)u;
                p2 += (Acc)da;
                p3 += (Acc)u * (Acc)xh;
                p4 += (Acc)da * (Acc)xh;
                acc += (Acc)dv[j] * (Acc)round_storage<T>(a);
            }
        }
        const double q1 = wave_sum_f64(p1), q2 = wave_sum_f64(p2), q3 = wave_sum_f64(p3), q4 = wave_sum_f64(p4);
        const double qa = wave_sum_f64(acc);
        if (lane == 0) {
            double* q = psums + (size_t)plane * 5;
            q[0] = q1; q[1] = q2; q[2] = q3; q[3] = q4; q[4] = qa;
        }
    }
}

// ds[plane] = sigmoid'(s) * sum dG * round_T(A1): one thread per plane, a launch of its own so that the double-precision exp stays out of
// the streaming kernel's register budget
template <typename T>
__global__ __launch_bounds__(256) void bn_gate_ds_kernel(const double* __restrict__ psums, const T* __restrict__ s, T* __restrict__ ds,
                                                          int NC) {
    const int plane = blockIdx.x * 256 + threadIdx.x;
    if (plane >= NC) return;
    const double g = sigmoid_f64(ld1<T>(s + plane));
    st1<T>(ds + plane, round_f32(psums[(size_t)plane * 5 + 4] * g * (1.0 - g)));
}

// per channel (one wave each): the plane terms summed over N in a fixed order (lane l takes images l, l + 64, ...; then the wave
// tree), dgamma, dbeta and the coefficients of dx = a * (dy - b1 - xhat * b2) as bn_bwd_finalize_kernel (bn.hip) leaves them;
// gate[plane] = (sigmoid(s), dpooled / HW) rounded once to fp32 for the apply pass
template <typename T>
__global__ __launch_bounds__(256) void bn_gate_bwd_finalize_kernel(const double* __restrict__ psums, const T* __restrict__ s,
                                                                    const T* __restrict__ dpl,
                                                                    const float* __restrict__ scale_shift,
                                                                    float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                    float* __restrict__ coef, float* __restrict__ gate, int N, int C,
                                                                    int HW, int training) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int n = lane; n < N; n += 64) {
        const size_t plane = (size_t)n * C + c;
        const double* q = psums + plane * 5;
        const double g = sigmoid_f64(ld1<T>(s + plane));
        const double add = dpl ? (double)ld1<T>(dpl + plane) / (double)HW : 0.0;
        gate[2 * plane] = (float)g;
        gate[2 * plane + 1] = (float)add;
        s1 += g * q[0] + add * q[1];
        s2 += g * q[2] + add * q[3];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane != 0) return;
    if (dgamma) dgamma[c] = (float)s2;
    if (dbeta) dbeta[c] = (float)s1;
    const double count = (double)N * (double)HW;
    coef[3 * c] = scale_shift[2 * c];                      // gamma * invstd
    coef[3 * c + 1] = training ? (float)(s1 / count) : 0.f;
    coef[3 * c + 2] = training ? (float)(s2 / count) : 0.f;
}

// dx = a * (dy - b1 - xhat * b2),  dy = (dG * sigmoid(s) + dpooled / HW) * act'(y)
template <typename T, int VEC>
__global__ __launch_bounds__(GW * 64) void bn_gate_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dout,
                                                                     const float* __restrict__ gate, T* __restrict__ dx,
                                                                     const float* __restrict__ scale_shift,
                                                                     const float* __restrict__ save_mean,
                                                                     const float* __restrict__ save_invstd,
                                                                     const float* __restrict__ coef, int NC, int C, int HW,
                                                                     int act) {
    const int lane = threadIdx.x & 63;
    const int nv = HW / VEC;
    for (int plane = blockIdx.x * GW + (threadIdx.x >> 6); plane < NC; plane += gridDim.x * GW) {
        const int c = plane % C;
        const float sc = scale_shift[2 * c], sh = scale_shift[2 * c + 1];
        const float mean = save_mean[c], invstd = save_invstd[c];
        const float a = coef[3 * c], b1 = coef[3 * c + 1], b2 = coef[3 * c + 2];
        const float g = gate[2 * (size_t)plane], add = gate[2 * (size_t)plane + 1];
        const T* p = x + (size_t)plane * HW;
        const T* d = dout + (size_t)plane * HW;
        T* o = dx + (size_t)plane * HW;
        for (int i = lane; i < nv; i += 64) {
            float xv[VEC], dv[VEC];
            PV<T, VEC>::ld(p + (size_t)i * VEC, xv);
            PV<T, VEC>::ld(d + (size_t)i * VEC, dv);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const float xh = (xv[j] - mean) * invstd;
                float av, da;
                act_both(fmaf(xv[j], sc, sh), act, av, da);
                const float dy = fmaf(dv[j], g, add) * da;
                xv[j] = a * (dy - b1 - xh * b2);
            }
            PV<T, VEC>::st(o + (size_t)i * VEC, xv);
        }
    }
}

unsigned plane_grid(long NC) {
    long g = (NC + GW - 1) / GW;
    if (g > 256 * 32) g = 256 * 32;
    return (unsigned)(g < 1 ? 1 : g);
}
// bn.hip's widths: 8 / 4 / 1 elements of either type
int gate_vec(int HW, int elem_bytes, const void* a, const void* b, const void* c) {
    return pick_vec(HW, elem_bytes, (uintptr_t)a | (uintptr_t)b | (uintptr_t)c, {8, 4});
}
}  // namespace

// [coef C*3 floats, rounded up to 16 bytes][plane sums N*C*5 doubles][gate N*C*2 floats]
size_t bn_gate_workspace_floats(int N, int C) { return (((size_t)C * 3 + 3) & ~(size_t)3) + (size_t)N * C * 12; }

hipError_t launch_bn_act_mean(const void* x, const float* gamma, const float* beta, float* rm, float* rv, float* save_mean,
                              float* save_invstd, float* scale_shift, void* pooled, float* ws, int N, int C, int HW, int dtype,
                              int act, int training, float momentum, float eps, hipStream_t st) {
    // statistics + finalize: launch_bn_prepare itself (the width of its walk is x's own, as below)
    const hipError_t e = launch_bn_prepare(x, gamma, beta, rm, rv, save_mean, save_invstd, scale_shift, ws, N, C, HW, dtype, training,
                                           momentum, eps, st);
    if (e != hipSuccess) return e;
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const int vec = gate_vec(HW, sizeof(T), x, nullptr, nullptr);
        with_vec<8, 8, 4, 1>(vec, [&](auto V) {
            hipLaunchKernelGGL((bn_act_mean_kernel<T, V>), dim3(plane_grid((long)N * C)), dim3(GW * 64), 0, st, (const T*)x,
                               (T*)pooled, scale_shift, N * C, C, HW, act);
        });
        return hipGetLastError();
    });
}

hipError_t launch_bn_act_gate_fwd(const void* x, const float* scale_shift, const void* s, void* out, int N, int C, int HW, int dtype,
                                  int act, hipStream_t st) {
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const int vec = gate_vec(HW, sizeof(T), x, out, nullptr);
        with_vec<8, 8, 4, 1>(vec, [&](auto V) {
            hipLaunchKernelGGL((bn_act_gate_fwd_kernel<T, V>), dim3(plane_grid((long)N * C)), dim3(GW * 64), 0, st, (const T*)x,
                               (const T*)s, (T*)out, scale_shift, N * C, C, HW, act);
        });
        return hipGetLastError();
    });
}

hipError_t launch_bn_gate_bwd_sums(const void* x, const void* dout, const void* s, const float* scale_shift, const float* save_mean,
                                   const float* save_invstd, void* ds, float* ws, int N, int C, int HW, int dtype, int act,
                                   hipStream_t st) {
    double* psums = reinterpret_cast<double*>(ws + (((size_t)C * 3 + 3) & ~(size_t)3));
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const int vec = gate_vec(HW, sizeof(T), x, dout, nullptr);
        with_vec<8, 8, 4, 1>(vec, [&](auto V) {
            hipLaunchKernelGGL((bn_gate_bwd_sums_kernel<T, V>), dim3(plane_grid((long)N * C)), dim3(GW * 64), 0, st, (const T*)x,
                               (const T*)dout, scale_shift, save_mean, save_invstd, psums, N * C, C, HW, act);
        });
        if (ds)
            hipLaunchKernelGGL((bn_gate_ds_kernel<T>), dim3((N * C + 255) / 256), dim3(256), 0, st, psums, (const T*)s, (T*)ds, N * C);
        return hipGetLastError();
    });
}

hipError_t launch_bn_gate_bwd(const void* x, const void* dout, const void* s, const void* dpl, const float* scale_shift,
                              const float* save_mean, const float* save_invstd, void* dx, float* dgamma, float* dbeta, float* ws,
                              int N, int C, int HW, int dtype, int act, int training, hipStream_t st) {
    float* coef = ws;
    const double* psums = reinterpret_cast<const double*>(ws + (((size_t)C * 3 + 3) & ~(size_t)3));
    float* gate = ws + (((size_t)C * 3 + 3) & ~(size_t)3) + (size_t)N * C * 10;
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((bn_gate_bwd_finalize_kernel<T>), dim3((C + 3) / 4), dim3(256), 0, st, psums, (const T*)s, (const T*)dpl,
                           scale_shift, dgamma, dbeta, coef, gate, N, C, HW, training);
        if (dx) {
            const int vec = gate_vec(HW, sizeof(T), x, dout, dx);
            with_vec<8, 8, 4, 1>(vec, [&](auto V) {
                hipLaunchKernelGGL((bn_gate_bwd_apply_kernel<T, V>), dim3(plane_grid((long)N * C)), dim3(GW * 64), 0, st, (const T*)x,
                                   (const T*)dout, gate, (T*)dx, scale_shift, save_mean, save_invstd, coef, N * C, C, HW, act);
            });
        }
        return hipGetLastError();
    });
}

}  // namespace moma
