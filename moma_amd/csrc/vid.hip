// Variational Information Distillation (`--distill vid`; reference distiller_zoo/VID.py, helper/loops_moma.py:145-149): the per-channel
// Gaussian negative log-likelihood of a regressor's output `mean` [B,C,H,W] against `target` [B,C,H,W], P = H W:
//     var_c = log(1 + exp(log_scale_c)) + eps      S_c = sum_{b,p} (mean - target)[b,c,p]^2
//     loss  = 0.5 / C * sum_c ( S_c / (B P var_c) + log var_c )
//     d_mean = g_loss (mean - target) / (var_c B C P)
//     d_var_c = 0.5 / C * ( 1 / var_c - S_c / (B P var_c^2) )      d_log_scale_c = d_var_c exp(log_scale_c) / (1 + exp(log_scale_c))
// in three kinds of launch, storage fp32 or bf16 and NCHW or channels_last, each chosen per side.  The walk over the maps and the
// finalize sums are mapwalk.hpp's (items of ONE image, so partials [B * nchunk, C]); this file says what happens to an element:
//   walk<VidFwd>  streams both maps once -> per item and channel sum (mean - target)^2, in fp32 chains of at most MAP_RUN = 16 squares
//             which are added to a double total: an NCHW thread has at most that many elements of an item, one chain, converted
//             once before the lanes meet; an NHWC thread's chain is cut every 16 of its pixels (the walk's cut()).
//   vid_finalize  the channel's partials -> sq, var, g_log_scale (the softplus, its logarithm and its derivative in double, in the
//             overflow-free form: finite for any finite log_scale, where the reference's fp32 exp is inf above 88) and the loss.
//   walk<VidBwd>  d_mean = round(double(mean - target) * (g_loss / (var_c B C P))), the factor formed in double per channel from var
//             (fp32) and g_loss, a DEVICE scalar; written in mean's dtype and layout.
// hipcc -O3, gfx950 (resource report, -Rpass-analysis=kernel-resource-usage), least .. most over the instantiations:
//   NCHW walk   forward 22 .. 50 VGPRs, backward 23 .. 58 (8 waves per SIMD throughout); no LDS
//   NHWC walk   forward 26 .. 98 VGPRs (8 chains and 8 double totals) and 16 KB of LDS at V = 8, backward 21 .. 88 (8 factors in double), no LDS
//   finalize    92 VGPRs and 128 B of LDS.       No kernel spills, none uses scratch.
#include "mapwalk.hpp"

namespace moma {
namespace {

static_assert(MAP_CHUNK == MOMA_VID_CHUNK, "the ABI's chunk is the walk's");

struct VidArgs {                            // the operands of the backward (forward: none)
    const float *var, *g_loss;
    double inv_n;                           // 1 / (B C P)
};

struct VidFwd {
    using Args = VidArgs;
    static constexpr int NS = 1;
    static constexpr bool READS_T = true, WRITES_DX = false, ONE_IMAGE = true;
    struct Ch {};
    static __device__ __forceinline__ Ch ch(const Args&, int, int) { return {}; }
    struct Acc {
        float chain = 0.f;
        double tot = 0.0;
        __device__ __forceinline__ float elem(float m, float t, const Ch&) {
            const float d = m - t;
            chain = fmaf(d, d, chain);
            return 0.f;
        }
        __device__ __forceinline__ void cut() { tot += (double)chain; chain = 0.f; }
        __device__ __forceinline__ void totals(double* s) const { s[0] = tot + (double)chain; }
    };
};

struct VidBwd {
    using Args = VidArgs;
    static constexpr int NS = 0;
    static constexpr bool READS_T = true, WRITES_DX = true, ONE_IMAGE = true;
    using Ch = double;                     // g_loss / (var_c B C P)
    static __device__ __forceinline__ Ch ch(const Args& a, int, int c) {
        double kc = (double)*a.g_loss * a.inv_n / (double)a.var[c];
        // the quotient is opaque to the scheduler: left free, it interleaves the 4 divisions of an NHWC thread at V = 4 and the
        // prologue then peaks at 66 VGPRs, one wave per SIMD less than the loop itself needs (50)
        asm("" : "+v"(kc));
        return kc;
    }
    struct Acc {
        __device__ __forceinline__ float elem(float m, float t, const Ch& kc) { return round_f32((double)(m - t) * kc); }
        __device__ __forceinline__ void cut() {}
    };
};

__global__ __launch_bounds__(MAP_FIN_THREADS) void vid_finalize_kernel(const double* __restrict__ partials, long long J, int C,
                                                                        const float* __restrict__ log_scale, double eps, double inv_bp,
                                                                        int lgL, float* __restrict__ sq, float* __restrict__ var,
                                                                        float* __restrict__ g_log_scale, float* __restrict__ loss) {
    double term = 0.0;
    map_fin_channels<1>(partials, J, C, lgL, [&](int c, const double* s) {
        const double ls = (double)log_scale[c];
        // softplus and sigmoid without overflow: exp of a non-positive number only
        const double en = exp(-fabs(ls));
        const double v = (ls > 0.0 ? ls : 0.0) + log1p(en) + eps;
        const double sig = ls >= 0.0 ? 1.0 / (1.0 + en) : en / (1.0 + en);
        const double m = s[0] * inv_bp;                                            // mean squared difference of the channel
        const double dv = (0.5 / (double)C) * (1.0 / v - m / (v * v));
        sq[c] = (float)s[0];
        var[c] = (float)v;
        g_log_scale[c] = (float)(dv * sig);
        term += m / v + log(v);
    });
    map_fin_loss(term, 0.5 / (double)C, loss);
}

}  // namespace

long long vid_partial_rows(int B, int P) { return (long long)B * ((P + MAP_CHUNK - 1) / MAP_CHUNK); }
size_t vid_workspace_bytes(int B, int C, int P) { return (size_t)vid_partial_rows(B, P) * (size_t)C * sizeof(double); }

hipError_t launch_vid_nll(const void* mean, const void* target, const float* log_scale, float eps, int B, int C, int P, int dt_m,
                          int lay_m, int dt_t, int lay_t, double* partials, float* sq, float* var, float* g_log_scale, float* loss,
                          hipStream_t st) {
    hipError_t e = map_launch<VidFwd>(mean, target, partials, VidArgs{}, nullptr, B, C, P, 1, dt_m, lay_m, dt_t, lay_t, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vid_finalize_kernel, dim3(1), dim3(MAP_FIN_THREADS), 0, st, (const double*)partials, vid_partial_rows(B, P), C,
                       log_scale, (double)eps, 1.0 / ((double)B * P), map_fin_lg(C), sq, var, g_log_scale, loss);
    return hipGetLastError();
}

hipError_t launch_vid_bwd(const void* mean, const void* target, const float* var, const float* g_loss, void* d_mean, int B, int C,
                          int P, int dt_m, int lay_m, int dt_t, int lay_t, hipStream_t st) {
    const VidArgs a{var, g_loss, 1.0 / ((double)B * C * P)};
    return map_launch<VidBwd>(mean, target, nullptr, a, d_mean, B, C, P, 1, dt_m, lay_m, dt_t, lay_t, st);
}

}  // namespace moma
