// SRRL (`--distill srrl`; reference models/util.py SRRL, train_student_moma.py:365-371, nn.MSELoss twice): what follows the connector's
// 1 x 1 convolution -- training-mode BatchNorm2d, ReLU, the mean squared error against the teacher's pooled feature, the TEACHER'S
// classifier on the activation and the mean squared error of its output against the teacher's logits -- on x (the convolution's
// output) and t, both [B, C], W [K, C], b [K], l [B, K]:
//     mean_c = sum_b x / B    var_c = sum_b x^2 / B - mean_c^2 (biased)    invstd_c = 1 / sqrt(var_c + eps)    xh = (x - mean_c) invstd_c
//     y = max(0, gamma_c xh + beta_c)      p = y W^T + b      loss = sum (y - t)^2 / (B C) + sum (p - l)^2 / (B K)
//     dY = 2 / (B C) (y - t) + 2 / (B K) (p - l) W            g = dY [y > 0]
//     A_c = sum_b g     B_c = sum_b g xh     d_beta = A     d_gamma = B     dx = gamma_c invstd_c (g - A_c / B - xh B_c / B)
// Everything is linear in the upstream gradient g_loss, so the FORWARD forms A, B and the whole of dx for g_loss = 1 (`dxu`, fp32)
// and the backward is one elementwise launch that scales them by the device scalar: x, t, W and l are read in the forward only,
// the batch reductions and both GEMMs run once per step, and nothing but dxu [B, C] and sums [2 C] is kept for the backward.
//   srrl_bn_kernel     one workgroup per SRRL_TC = 16 channels, 16 row lanes each: thread (tr, tc) walks rows tr, tr + 16, ... of channel
//             tc (16 neighbouring channels of a row in one request: element accesses, so no alignment beyond the element and no
//             divisibility of C is needed).  sum x and sum x^2 in DOUBLE from the first element on (x^2 is exact there: the variance does
//             not cancel for off-centre inputs, hint.hip), the sixteen row lanes added in the order of tr -> mean, invstd (double) and the
//             running statistics in place (unbiased variance B / (B - 1)).  The workgroup owns every row of its channels, so a second
//             walk follows at once: xh = round((double(x) - mean) invstd), y = max(0, fma(gamma, xh, beta)) in fp32 -> y [B, C] and the
//             channel's sum of (y - t)^2 in double.
//   srrl_gemm_kernel<NT>   p's partial sums: the 64 x 64 tile product of tile64.hpp (fp32 FMA over a SEGMENT of 32 channels, the segment's
//             sum added to a DOUBLE total) on y and W.  Shapes with few tiles split the channels over blockIdx.z (tile64_segs: a
//             function of the shape alone, about one workgroup per compute unit): partials [splits, B, K] in double.
//   srrl_pred_kernel   one workgroup per row: p = the splits added in order + b, rounded ONCE to fp32 (what the reference holds), e = p - l
//             -> e [B, K] fp32 and the row's sum of e^2 in double.
//   srrl_gemm_kernel<NN>   q = e W, the same kernel with W walked along its rows: partials [splits, B, C] in double.
//   srrl_grad_kernel   srrl_bn_kernel's walk again: recomputes xh and y from x, dY = (y - t) 2 / (B C) + q 2 / (B K) and g in double,
//             A and B in double in the order of the rows, then the second walk writes dxu = round(gamma invstd (g - A / B - xh B / B)) over
//             y.  Workgroup 0 also adds the channels' and the rows' squared errors in order (tile64.hpp's ordered sum) -> loss.
//   srrl_scale_kernel  (backward) dx = round(dxu g_loss) in x's dtype, d_gamma = g_loss B, d_beta = g_loss A: a power of two in g_loss
//             scales every gradient exactly.
// Five launches forward, one backward.  No atomics, every sum in a fixed order that depends on the shape alone: bitwise repeatable.
// hipcc -O3, gfx950 (resource report, -Rpass-analysis=kernel-resource-usage), least .. most over the instantiations:
//   srrl_bn_kernel 32 .. 36 VGPRs, 2304 B of LDS; srrl_gemm_kernel 138 (NT), 130 (NN) VGPRs (16 double and 16 fp32 accumulators, 16
//   values of the next segment in flight: 3 waves per SIMD) and 16.5 KB of LDS; srrl_pred_kernel 18 VGPRs, 32 B of LDS;
//   srrl_grad_kernel 40 VGPRs, 4352 B of LDS; srrl_scale_kernel 10 VGPRs, no LDS.  8 waves per SIMD but for the GEMM.
//   No kernel spills, none uses scratch.
#include "tile64.hpp"

namespace moma {
namespace {

constexpr int SRRL_THREADS = T64_THREADS;           // (the loss in srrl_grad_kernel is tile64.hpp's ordered sum)
constexpr int SRRL_TC = 16;                         // channels of a workgroup of the two batch walks
constexpr int SRRL_RL = SRRL_THREADS / SRRL_TC;     // row lanes per channel

// the SRRL_RL row lanes of a channel meet in the order of tr; thread (0, tc) returns the sum
__device__ __forceinline__ double srrl_rows_sum(double (*sh)[SRRL_TC], int tr, int tc, double v) {
    __syncthreads();                                                               // (the previous use has been read)
    sh[tr][tc] = v;
    __syncthreads();
    double u = 0.0;
    if (tr == 0)
#pragma unroll
        for (int r = 0; r < SRRL_RL; ++r) u += sh[r][tc];
    return u;
}

template <typename TX, typename TT>
__global__ __launch_bounds__(SRRL_THREADS) void srrl_bn_kernel(const TX* __restrict__ x, const TT* __restrict__ t,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               float* __restrict__ running_mean, float* __restrict__ running_var,
                                                               double momentum, double eps, int B, int C, double* __restrict__ mean,
                                                               double* __restrict__ invstd, double* __restrict__ colsum,
                                                               float* __restrict__ y, float* __restrict__ y_out) {
    __shared__ double sh[SRRL_RL][SRRL_TC];
    __shared__ double stat[2][SRRL_TC];
    const int tid = threadIdx.x, tc = tid % SRRL_TC, tr = tid / SRRL_TC, c = blockIdx.x * SRRL_TC + tc;
    const bool ok = c < C;
    double s0 = 0.0, s1 = 0.0;
    if (ok)
#pragma unroll 4
        for (int b = tr; b < B; b += SRRL_RL) {
            const double xd = (double)ld1<TX>(x + (size_t)b * C + c);
            s0 += xd;
            s1 = fma(xd, xd, s1);
        }
    s0 = srrl_rows_sum(sh, tr, tc, s0);
    s1 = srrl_rows_sum(sh, tr, tc, s1);
    if (tr == 0) {
        const double m = s0 / (double)B;                                           // (divisions: a constant channel has var = 0 exactly)
        const double var = fmax(s1 / (double)B - m * m, 0.0);
        const double is = 1.0 / sqrt(var + eps);
        stat[0][tc] = m;
        stat[1][tc] = is;
        if (ok) {
            mean[c] = m;
            invstd[c] = is;
            if (running_mean) running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * m);
            if (running_var)
                running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * var * ((double)B / (double)(B - 1)));
        }
    }
    __syncthreads();
    const double mu = stat[0][tc], is = stat[1][tc];
    double l = 0.0;
    if (ok) {
        const float ga = gamma[c], be = beta[c];
        for (int b = tr; b < B; b += SRRL_RL) {
            const size_t at = (size_t)b * C + c;
            const float xh = round_f32(((double)ld1<TX>(x + at) - mu) * is);
            const float yv = fmaxf(fmaf(ga, xh, be), 0.f);
            const double d = (double)(yv - ld1<TT>(t + at));
            l = fma(d, d, l);
            y[at] = yv;
            if (y_out) y_out[at] = yv;
        }
    }
    l = srrl_rows_sum(sh, tr, tc, l);
    if (tr == 0 && ok) colsum[c] = l;
}

// out[s, m, n] = sum over the split's k of A[m, k] Bm(n, k), Bm(n, k) = NN ? Bm[k N + n] : Bm[n Kr + k]; A [M, Kr] dense: one tile of
// tile64.hpp per workgroup, split s = blockIdx.z over `segs` segments of the reduction
template <bool NN>
__global__ __launch_bounds__(T64_THREADS) void srrl_gemm_kernel(const float* __restrict__ A, const float* __restrict__ Bm,
                                                                double* __restrict__ out, int M, int N, int Kr, int segs) {
    __shared__ float As[T64_LDS], Bs[T64_LDS];
    const int n0 = blockIdx.x * T64_TILE, m0 = blockIdx.y * T64_TILE, s = blockIdx.z;
    const int kbeg = s * segs * T64_SEG, kend = min(Kr, kbeg + segs * T64_SEG);
    double dacc[4][4];
    tile64_zero(dacc);
    tile64<false, NN, false, float, float>(A, Bm, As, Bs, M, N, Kr, kbeg, kend, m0, n0, dacc);
    tile64_each(dacc, m0, n0, M, N, [=](int m, int n, double v) { out[((size_t)s * M + m) * N + n] = v; });
}

// one workgroup per row b
__global__ __launch_bounds__(SRRL_THREADS) void srrl_pred_kernel(const double* __restrict__ P, int splits, const float* __restrict__ bias,
                                                                 const float* __restrict__ logits, int B, int K, float* __restrict__ e,
                                                                 double* __restrict__ rowsum, float* __restrict__ pred_out) {
    __shared__ double sh[SRRL_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    double l = 0.0;
    for (int k = tid; k < K; k += SRRL_THREADS) {
        const size_t at = (size_t)b * K + k;
        double p = 0.0;
        for (int s = 0; s < splits; ++s) p += P[(size_t)s * B * K + at];
        const float pf = round_f32(p + (bias ? (double)bias[k] : 0.0));
        const float ev = pf - logits[at];
        e[at] = ev;
        if (pred_out) pred_out[at] = pf;
        l = fma((double)ev, (double)ev, l);
    }
    l = wave_sum(l);
    if ((tid & 63) == 0) sh[tid >> 6] = l;
    __syncthreads();
    if (tid == 0) {
        double u = 0.0;
#pragma unroll
        for (int w = 0; w < SRRL_THREADS / 64; ++w) u += sh[w];
        rowsum[b] = u;
    }
}

struct SrrlGradArgs {
    const float *gamma, *beta;
    const double *mean, *invstd, *Q, *colsum, *rowsum;
    int splits, B, C;
    double k1, k2, inv_b, inv_bc, inv_bk;           // 2 / (B C), 2 / (B K), 1 / B, 1 / (B C), 1 / (B K)
    double* sums;
    float *dxu, *loss;
};

struct SrrlElem { float xh; double g; };

template <typename TX, typename TT>
__device__ __forceinline__ SrrlElem srrl_elem(const TX* __restrict__ x, const TT* __restrict__ t, const SrrlGradArgs& a, int b, int c,
                                              double mu, double is, float ga, float be) {
    const size_t at = (size_t)b * a.C + c;
    SrrlElem r;
    r.xh = round_f32(((double)ld1<TX>(x + at) - mu) * is);
    const float yv = fmaxf(fmaf(ga, r.xh, be), 0.f);
    const float d = yv - ld1<TT>(t + at);
    double q = 0.0;
    for (int s = 0; s < a.splits; ++s) q += a.Q[(size_t)s * a.B * a.C + at];
    r.g = yv > 0.f ? fma((double)d, a.k1, q * a.k2) : 0.0;                         // (strictly: ReLU's derivative at 0 is 0)
    return r;
}

template <typename TX, typename TT>
__global__ __launch_bounds__(SRRL_THREADS) void srrl_grad_kernel(const TX* __restrict__ x, const TT* __restrict__ t,
                                                                 const SrrlGradArgs a) {
    __shared__ double sh[SRRL_RL][SRRL_TC];
    __shared__ double stat[2][SRRL_TC];
    const int tid = threadIdx.x, tc = tid % SRRL_TC, tr = tid / SRRL_TC, c = blockIdx.x * SRRL_TC + tc;
    const int B = a.B, C = a.C;
    const bool ok = c < C;
    double mu = 0.0, is = 0.0, sa = 0.0, sb = 0.0;
    float ga = 0.f, be = 0.f;
    if (ok) {
        mu = a.mean[c]; is = a.invstd[c]; ga = a.gamma[c]; be = a.beta[c];
        for (int b = tr; b < B; b += SRRL_RL) {
            const SrrlElem r = srrl_elem<TX, TT>(x, t, a, b, c, mu, is, ga, be);
            sa += r.g;
            sb = fma(r.g, (double)r.xh, sb);
        }
    }
    sa = srrl_rows_sum(sh, tr, tc, sa);
    sb = srrl_rows_sum(sh, tr, tc, sb);
    if (tr == 0) {
        stat[0][tc] = sa;
        stat[1][tc] = sb;
        if (ok) {
            a.sums[c] = sa;
            a.sums[C + c] = sb;
        }
    }
    __syncthreads();
    if (ok) {
        const double am = stat[0][tc] * a.inv_b, bm = stat[1][tc] * a.inv_b, f = (double)ga * is;
        for (int b = tr; b < B; b += SRRL_RL) {
            const SrrlElem r = srrl_elem<TX, TT>(x, t, a, b, c, mu, is, ga, be);
            a.dxu[(size_t)b * C + c] = round_f32(f * (r.g - am - (double)r.xh * bm));
        }
    }
    if (blockIdx.x == 0) {                                                         // the loss: both weighted sums per thread, then in order
        const double u = strided_sum(a.colsum, C), v = strided_sum(a.rowsum, B);
        const double w = ordered_sum(u * a.inv_bc + v * a.inv_bk);
        if (tid == 0) *a.loss = (float)w;
    }
}

template <typename TX>
__global__ __launch_bounds__(SRRL_THREADS) void srrl_scale_kernel(const float* __restrict__ dxu, const double* __restrict__ sums,
                                                                  const float* __restrict__ g_loss, TX* __restrict__ dx,
                                                                  float* __restrict__ d_gamma, float* __restrict__ d_beta, long long n,
                                                                  int C) {
    const double gl = (double)*g_loss;
    const long long i0 = (long long)blockIdx.x * SRRL_THREADS + threadIdx.x;
    if (dx)
        for (long long i = i0; i < n; i += (long long)gridDim.x * SRRL_THREADS) st1<TX>(dx + i, round_f32((double)dxu[i] * gl));
    if (i0 < C) {
        if (d_beta) d_beta[i0] = (float)(gl * sums[i0]);
        if (d_gamma) d_gamma[i0] = (float)(gl * sums[C + i0]);
    }
}

// segments of 32 along the reduction that one workgroup of a GEMM [M, N] adds, and the splits that makes
int srrl_segs(int M, int N, int Kr) { return tile64_segs(tile64_tiles(M, N), ceil_div(Kr, T64_SEG)); }
int srrl_splits(int M, int N, int Kr) { return ceil_div(ceil_div(Kr, T64_SEG), srrl_segs(M, N, Kr)); }

template <bool NN>
hipError_t srrl_gemm(const float* A, const float* Bm, double* out, int M, int N, int Kr, hipStream_t st) {
    const dim3 grid(ceil_div(N, T64_TILE), ceil_div(M, T64_TILE), srrl_splits(M, N, Kr));
    hipLaunchKernelGGL((srrl_gemm_kernel<NN>), grid, dim3(T64_THREADS), 0, st, A, Bm, out, M, N, Kr, srrl_segs(M, N, Kr));
    return hipGetLastError();
}

// the workspace: doubles first
struct SrrlWs {
    double *mean, *invstd, *colsum, *rowsum, *P, *Q;
    float* e;
};
size_t srrl_ws_doubles(int B, int C, int K) {
    return (size_t)3 * C + B + (size_t)srrl_splits(B, K, C) * B * K + (size_t)srrl_splits(B, C, K) * B * C;
}
SrrlWs srrl_ws(void* base, int B, int C, int K) {
    SrrlWs w{};
    double* d = (double*)base;
    w.mean = d; d += C;
    w.invstd = d; d += C;
    w.colsum = d; d += C;
    w.rowsum = d; d += B;
    w.P = d; d += (size_t)srrl_splits(B, K, C) * B * K;
    w.Q = d;
    w.e = (float*)((double*)base + srrl_ws_doubles(B, C, K));
    return w;
}

}  // namespace

size_t srrl_workspace_bytes(int B, int C, int K) {
    return srrl_ws_doubles(B, C, K) * sizeof(double) + (size_t)B * K * sizeof(float);
}

hipError_t launch_srrl_fwd(const void* x, const void* t, const float* W, const float* bias, const float* logits, const float* gamma,
                           const float* beta, float* running_mean, float* running_var, float momentum, float eps, int B, int C, int K,
                           int dt_x, int dt_t, void* workspace, double* sums, float* dxu, float* loss, float* y_out, float* pred_out,
                           hipStream_t st) {
    const SrrlWs w = srrl_ws(workspace, B, C, K);
    const unsigned cgrid = (unsigned)ceil_div(C, SRRL_TC);
    with_dtype(dt_x, [&](auto tx) {
        return with_dtype(dt_t, [&](auto tt) {
            using TX = typename decltype(tx)::type;
            using TT = typename decltype(tt)::type;
            hipLaunchKernelGGL((srrl_bn_kernel<TX, TT>), dim3(cgrid), dim3(SRRL_THREADS), 0, st, (const TX*)x, (const TT*)t, gamma, beta,
                               running_mean, running_var, (double)momentum, (double)eps, B, C, w.mean, w.invstd, w.colsum, dxu, y_out);
            return 0;
        });
    });
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    err = srrl_gemm<false>(dxu, W, w.P, B, K, C, st);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(srrl_pred_kernel, dim3(B), dim3(SRRL_THREADS), 0, st, (const double*)w.P, srrl_splits(B, K, C), bias, logits, B, K,
                       w.e, w.rowsum, pred_out);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    err = srrl_gemm<true>(w.e, W, w.Q, B, C, K, st);
    if (err != hipSuccess) return err;
    const double bc = (double)B * C, bk = (double)B * K;
    const SrrlGradArgs a{gamma, beta, w.mean, w.invstd, w.Q, w.colsum, w.rowsum, srrl_splits(B, C, K), B, C,
                         2.0 / bc, 2.0 / bk, 1.0 / B, 1.0 / bc, 1.0 / bk, sums, dxu, loss};
    with_dtype(dt_x, [&](auto tx) {
        return with_dtype(dt_t, [&](auto tt) {
            using TX = typename decltype(tx)::type;
            using TT = typename decltype(tt)::type;
            hipLaunchKernelGGL((srrl_grad_kernel<TX, TT>), dim3(cgrid), dim3(SRRL_THREADS), 0, st, (const TX*)x, (const TT*)t, a);
            return 0;
        });
    });
    return hipGetLastError();
}

hipError_t launch_srrl_bwd(const float* dxu, const double* sums, const float* g_loss, void* dx, float* d_gamma, float* d_beta, int B,
                           int C, int dt_x, hipStream_t st) {
    const long long n = (long long)B * C;
    const long long need = dx ? n : C;
    const unsigned grid = (unsigned)max((long long)ceil_div(C, SRRL_THREADS), min((need + SRRL_THREADS - 1) / SRRL_THREADS, 2048LL));
    with_dtype(dt_x, [&](auto tx) {
        using TX = typename decltype(tx)::type;
        hipLaunchKernelGGL((srrl_scale_kernel<TX>), dim3(grid), dim3(SRRL_THREADS), 0, st, dxu, sums, g_loss, (TX*)dx, d_gamma, d_beta, n,
                           C);
        return 0;
    });
    return hipGetLastError();
}

}  // namespace moma
