// FitNets hint (`--distill hint`; reference models/util.py ConvReg, distiller_zoo/FitNet.py HintLoss): what follows the regressor's
// convolution -- training-mode BatchNorm2d, ReLU and the mean squared error against the teacher's map -- on x (the convolution's
// output) and t, both [B,C,H,W], P = H W, M = B P, N = B C P:
//     mean_c = sum x / M    var_c = sum x^2 / M - mean_c^2 (biased)    invstd_c = 1 / sqrt(var_c + eps)    xh = (x - mean_c) invstd_c
//     y = max(0, gamma_c xh + beta_c)       loss = sum (y - t)^2 / N        g = (y - t) [y > 0]
//     A_c = sum_(b,p) g       B_c = sum_(b,p) g xh       k = 2 g_loss / N
//     d_beta_c = k A_c     d_gamma_c = k B_c     dx = k gamma_c invstd_c (g - A_c / M - xh B_c / M)
// in three streaming walks over the maps (x is read three times, t twice, dx written once; y, xh and g never reach memory), storage
// fp32 or bf16 and NCHW or channels_last, each chosen per side.  The walk and the finalize sums are mapwalk.hpp's; this file says
// what happens to an element:
//   walk<STATS>  reads x -> per item and channel sum x, sum x^2, both in DOUBLE from the first element on (x^2 is exact there, so
//             the variance does not cancel for off-centre inputs).
//   walk<LOSS>   reads x and t -> per item and channel sum (y - t)^2, sum g, sum g xh.  xh = round((double(x) - mean) invstd) with
//             mean and invstd in DOUBLE: an fp32 mean cancels against x for off-centre inputs or few values per channel (with
//             M = 2 the reference's own fp32 results are 1e-4 away from float64 for that reason), the double centring makes xh a
//             correctly rounded fp32 number at two more instructions per element of a memory-bound walk.  y, the difference and
//             the products are fp32, every sum double.  g_loss enters the backward only as the factor k, so A and B come from
//             THIS walk and the backward has no reduction.
//   walk<BWD>    reads x and t -> dx = round(double(g - A/M - xh B/M) * (k gamma invstd)), the inner term in fp32, the factor formed
//             in double per channel from g_loss, a DEVICE scalar (a power of two in g_loss scales dx exactly); written in x's dtype
//             and layout.
//   An item holds BI images: 1 for planes of a chunk and more, else the MAP_CHUNK / P images that fill one (7 x 7 planes: 20), so
//             that the partial rows -- what the one-workgroup finalize kernels walk -- stay near B P / MAP_CHUNK.
//   hint_stats_finalize / hint_loss_finalize   the channel's partials -> mean, invstd (double) and the running statistics in place
//             (unbiased variance M / (M - 1); conv_bias, nullable, is added to the mean for running_mean ONLY: a constant in front
//             of a BatchNorm moves nothing else) / A, B (double) and the loss.
//   hint_dparam       [C] threads: d_gamma = k B, d_beta = k A.
// hipcc -O3, gfx950 (resource report, -Rpass-analysis=kernel-resource-usage), least .. most over the instantiations:
//   NCHW walk   STATS 22 .. 34 VGPRs, LOSS 38 .. 65, BWD 39 .. 68 (7 waves per SIMD at least); no LDS
//   NHWC walk   STATS 20 .. 66 VGPRs and 32 KB of LDS at V = 8; LOSS 40 .. 179 (V = 8: 8 channels x (3 double sums + mean + invstd in
//               double + gamma + beta), 2 waves per SIMD) and 48 KB of LDS; BWD 37 .. 157, no LDS.  V = 4 and 1 stay below 100.
//   finalize    stats 84 VGPRs, loss 102 VGPRs and 128 B of LDS; d_param 8.       No kernel spills, none uses scratch.
#include "mapwalk.hpp"

namespace moma {
namespace {

static_assert(MAP_CHUNK == MOMA_HINT_CHUNK, "the ABI's chunk is the walk's");
enum { HINT_STATS = 0, HINT_LOSS = 1, HINT_BWD = 2 };

struct HintVecs {                           // the [C] operands of a walk (STATS: none; LOSS: the first four; BWD: all)
    const float *gamma, *beta;
    const double *mean, *invstd;
    const double* sums;                     // A [C] then B [C]
    const float* g_loss;
    double inv_m, two_inv_n;                // 1 / M, 2 / N
};

struct HintCh {                             // one channel's constants in registers
    double mu, is, kc;
    float ga, be, a, b;
};

template <int MODE>
__device__ __forceinline__ HintCh hint_ch(const HintVecs& v, int C, int c) {
    HintCh h{};
    if constexpr (MODE != HINT_STATS) {
        h.mu = v.mean[c]; h.is = v.invstd[c]; h.ga = v.gamma[c]; h.be = v.beta[c];
    }
    if constexpr (MODE == HINT_BWD) {
        h.a = (float)(v.sums[c] * v.inv_m);
        h.b = (float)(v.sums[C + c] * v.inv_m);
        h.kc = (double)*v.g_loss * v.two_inv_n * (double)h.ga * h.is;
    }
    return h;
}

// one element: STATS and LOSS add to s[], BWD returns dx
template <int MODE>
__device__ __forceinline__ float hint_elem(float x, float t, const HintCh& h, double* s) {
    if constexpr (MODE == HINT_STATS) {
        const double xd = (double)x;
        s[0] += xd;
        s[1] = fma(xd, xd, s[1]);
        return 0.f;
    } else {
        const float xh = round_f32(((double)x - h.mu) * h.is);
        const float y = fmaxf(fmaf(h.ga, xh, h.be), 0.f);
        const float d = y - t;
        const float g = y > 0.f ? d : 0.f;                                         // (strictly: ReLU's derivative at 0 is 0)
        if constexpr (MODE == HINT_LOSS) {
            s[0] += (double)(d * d);
            s[1] += (double)g;
            s[2] += (double)(g * xh);
            return 0.f;
        } else {
            return round_f32((double)(g - h.a - xh * h.b) * h.kc);
        }
    }
}

template <int MODE>
struct HintOp {                             // the three as mapwalk.hpp's policy
    using Args = HintVecs;
    static constexpr int NS = MODE == HINT_STATS ? 2 : MODE == HINT_LOSS ? 3 : 0;
    static constexpr bool READS_T = MODE != HINT_STATS, WRITES_DX = MODE == HINT_BWD, ONE_IMAGE = false;
    using Ch = HintCh;
    static __device__ __forceinline__ Ch ch(const Args& v, int C, int c) { return hint_ch<MODE>(v, C, c); }
    struct Acc {
        double s[NS ? NS : 1] = {};
        __device__ __forceinline__ float elem(float x, float t, const Ch& h) { return hint_elem<MODE>(x, t, h, s); }
        __device__ __forceinline__ void cut() {}           // (every sum is double from the first element on)
        __device__ __forceinline__ void totals(double* o) const {
#pragma unroll
            for (int n = 0; n < NS; ++n) o[n] = s[n];
        }
    };
};

__global__ __launch_bounds__(MAP_FIN_THREADS) void hint_stats_finalize_kernel(const double* __restrict__ partials, long long J, int C,
                                                                              int lgL, const float* __restrict__ conv_bias,
                                                                              float* __restrict__ running_mean,
                                                                              float* __restrict__ running_var, double momentum,
                                                                              double eps, double M, double unbias,
                                                                              double* __restrict__ mean, double* __restrict__ invstd) {
    map_fin_channels<2>(partials, J, C, lgL, [&](int c, const double* s) {
        const double m = s[0] / M;                                                 // (divisions: a constant channel has var = 0 exactly)
        const double var = fmax(s[1] / M - m * m, 0.0);
        mean[c] = m;
        invstd[c] = 1.0 / sqrt(var + eps);
        if (running_mean)
            running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] +
                                      momentum * (m + (conv_bias ? (double)conv_bias[c] : 0.0)));
        if (running_var) running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * var * unbias);
    });
}

__global__ __launch_bounds__(MAP_FIN_THREADS) void hint_loss_finalize_kernel(const double* __restrict__ partials, long long J, int C,
                                                                             int lgL, double inv_n, double* __restrict__ sums,
                                                                             float* __restrict__ loss) {
    double term = 0.0;
    map_fin_channels<3>(partials, J, C, lgL, [&](int c, const double* s) {
        term += s[0];
        sums[c] = s[1];
        sums[C + c] = s[2];
    });
    map_fin_loss(term, inv_n, loss);
}

__global__ void hint_dparam_kernel(const double* __restrict__ sums, const float* __restrict__ g_loss, double two_inv_n, int C,
                                   float* __restrict__ d_gamma, float* __restrict__ d_beta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double k = (double)*g_loss * two_inv_n;
    if (d_beta) d_beta[c] = (float)(k * sums[c]);
    if (d_gamma) d_gamma[c] = (float)(k * sums[C + c]);
}

// images of one item: a plane shorter than a chunk shares its item with as many further images as fill one (7 x 7 planes: 20 images),
// so the partial rows -- what the one-workgroup finalize kernels walk -- stay near B P / MAP_CHUNK
int hint_images_per_item(int B, int P) { return max(1, min(B, MAP_CHUNK / P)); }

template <int MODE>
hipError_t hint_launch(const void* x, const void* t, double* partials, const HintVecs& vecs, void* dx, int B, int C, int P, int dt_x,
                       int lay_x, int dt_t, int lay_t, hipStream_t st) {
    return map_launch<HintOp<MODE>>(x, t, partials, vecs, dx, B, C, P, hint_images_per_item(B, P), dt_x, lay_x, dt_t, lay_t, st);
}

}  // namespace

long long hint_partial_rows(int B, int P) {
    const int bi = hint_images_per_item(B, P);
    return (long long)((B + bi - 1) / bi) * ((P + MAP_CHUNK - 1) / MAP_CHUNK);
}
size_t hint_workspace_bytes(int B, int C, int P) { return (size_t)hint_partial_rows(B, P) * (size_t)C * 3 * sizeof(double); }

hipError_t launch_hint_fwd(const void* x, const void* t, const float* gamma, const float* beta, const float* conv_bias,
                           float* running_mean, float* running_var, float momentum, float eps, int B, int C, int P, int dt_x,
                           int lay_x, int dt_t, int lay_t, double* partials, double* mean, double* invstd, double* sums, float* loss,
                           hipStream_t st) {
    const double M = (double)B * P;
    const long long J = hint_partial_rows(B, P);
    const int lgL = map_fin_lg(C);
    HintVecs v{};
    hipError_t e = hint_launch<HINT_STATS>(x, nullptr, partials, v, nullptr, B, C, P, dt_x, lay_x, dt_x, lay_x, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hint_stats_finalize_kernel, dim3(1), dim3(MAP_FIN_THREADS), 0, st, (const double*)partials, J, C, lgL, conv_bias,
                       running_mean, running_var, (double)momentum, (double)eps, M, M / (M - 1.0), mean, invstd);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    v.gamma = gamma; v.beta = beta; v.mean = mean; v.invstd = invstd;
    e = hint_launch<HINT_LOSS>(x, t, partials, v, nullptr, B, C, P, dt_x, lay_x, dt_t, lay_t, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hint_loss_finalize_kernel, dim3(1), dim3(MAP_FIN_THREADS), 0, st, (const double*)partials, J, C, lgL,
                       1.0 / (M * C), sums, loss);
    return hipGetLastError();
}

hipError_t launch_hint_bwd(const void* x, const void* t, const float* gamma, const float* beta, const double* mean,
                           const double* invstd, const double* sums, const float* g_loss, void* dx, float* d_gamma, float* d_beta,
                           int B, int C, int P, int dt_x, int lay_x, int dt_t, int lay_t, hipStream_t st) {
    const double M = (double)B * P;
    HintVecs v{gamma, beta, mean, invstd, sums, g_loss, 1.0 / M, 2.0 / (M * C)};
    if (dx) {
        const hipError_t e = hint_launch<HINT_BWD>(x, t, nullptr, v, dx, B, C, P, dt_x, lay_x, dt_t, lay_t, st);
        if (e != hipSuccess) return e;
    }
    if (d_gamma || d_beta) {
        hipLaunchKernelGGL(hint_dparam_kernel, dim3((C + 255) / 256), dim3(256), 0, st, sums, g_loss, v.two_inv_n, C, d_gamma, d_beta);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace moma
