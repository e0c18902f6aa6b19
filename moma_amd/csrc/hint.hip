// FitNets hint (`--distill hint`; reference models/util.py ConvReg, distiller_zoo/FitNet.py HintLoss): what follows the regressor's
// convolution -- training-mode BatchNorm2d, ReLU and the mean squared error against the teacher's map -- on x (the convolution's
// output) and t, both [B,C,H,W], P = H W, M = B P, N = B C P:
//     mean_c = sum x / M    var_c = sum x^2 / M - mean_c^2 (biased)    invstd_c = 1 / sqrt(var_c + eps)    xh = (x - mean_c) invstd_c
//     y = max(0, gamma_c xh + beta_c)       loss = sum (y - t)^2 / N        g = (y - t) [y > 0]
//     A_c = sum_(b,p) g       B_c = sum_(b,p) g xh       k = 2 g_loss / N
//     d_beta_c = k A_c     d_gamma_c = k B_c     dx = k gamma_c invstd_c (g - A_c / M - xh B_c / M)
// in three streaming walks over the maps (x is read three times, t twice, dx written once; y, xh and g never reach memory), storage
// fp32 or bf16 and NCHW or channels_last, each chosen per side:
//   hint_walk<STATS>  reads x -> per item and channel sum x, sum x^2, both in DOUBLE from the first element on (x^2 is exact there, so
//             the variance does not cancel for off-centre inputs).
//   hint_walk<LOSS>   reads x and t -> per item and channel sum (y - t)^2, sum g, sum g xh.  xh = round((double(x) - mean) invstd) with
//             mean and invstd in DOUBLE: an fp32 mean cancels against x for off-centre inputs or few values per channel (with
//             M = 2 the reference's own fp32 results are 1e-4 away from float64 for that reason), the double centring makes xh a
//             correctly rounded fp32 number at two more instructions per element of a memory-bound walk.  y, the difference and
//             the products are fp32, every sum double.  g_loss enters the backward only as the factor k, so A and B come from
//             THIS walk and the backward has no reduction.
//   hint_walk<BWD>    reads x and t -> dx = round(double(g - A/M - xh B/M) * (k gamma invstd)), the inner term in fp32, the factor formed
//             in double per channel from g_loss, a DEVICE scalar (a power of two in g_loss scales dx exactly); written in x's dtype
//             and layout.
//   The walk is vid.hip's: the work is cut into ITEMS whose shape follows the layout of x:
//             NCHW  (BI images, block of R = 256 / G channel rows, chunk of HINT_CHUNK pixels); BI = 1 for planes of a chunk and more,
//                   else the HINT_CHUNK / P images that fill one (7 x 7 planes: 20), so that the partial rows -- what the
//                   one-workgroup finalize kernels walk -- stay near B P / HINT_CHUNK; G = 1 .. 64 lanes walk one row, G the
//                   power of two that covers min(P, HINT_CHUNK) / V vectors; the G lanes meet in double by xor shuffles.
//             NHWC  (BI images, tile of TW <= 64 / V channel vectors, chunk of HINT_CHUNK pixels); thread (tr, tc) walks pixels tr, tr + RP,
//                   ... of channel vector tc, RP = 256 / TW; all sums go to LDS at once and one thread per (sum, channel) adds the RP pixel
//                   rows in the order of tr.
//             Each item writes one double per sum and channel it covers: partials [sums, ceil(B / BI) * nchunk, C].  The grid is capped at
//             HINT_MAX_GRID workgroups which stride over the items; what a partial holds depends on the item alone, never on the grid.
//             A t in the OTHER layout than x is read element by element at the same (b, c, p): correct, not fast.
//   hint_stats_finalize / hint_loss_finalize   ONE workgroup of 16 waves each: L = 1 .. 64 lanes per channel add the partials l, l + L,
//             ... in order, then a xor tree, all in double -> mean, invstd (double) and the running statistics in place (unbiased
//             variance M / (M - 1); conv_bias, nullable, is added to the mean for running_mean ONLY: a constant in front of a
//             BatchNorm moves nothing else) / A, B (double) and the loss, the channels' terms added per wave, then over the waves in order.
//   hint_dparam       [C] threads: d_gamma = k B, d_beta = k A.
// 16-byte accesses (two for 8 fp32) where the address and the contiguous extent (P, or C) allow on every side that is walked in
// vectors, 4 elements where only that divides, element accesses otherwise.  No atomics: bitwise repeatable.
// hipcc -O3, gfx950 (resource report, -Rpass-analysis=kernel-resource-usage), least .. most over the instantiations:
//   NCHW walk   STATS 22 .. 34 VGPRs, LOSS 38 .. 65, BWD 39 .. 68 (7 waves per SIMD at least); no LDS
//   NHWC walk   STATS 20 .. 66 VGPRs and 32 KB of LDS at V = 8; LOSS 40 .. 179 (V = 8: 8 channels x (3 double sums + mean + invstd in
//               double + gamma + beta), 2 waves per SIMD) and 48 KB of LDS; BWD 37 .. 157, no LDS.  V = 4 and 1 stay below 100.
//   finalize    stats 84 VGPRs, loss 103 VGPRs and 128 B of LDS; d_param 8.       No kernel spills, none uses scratch.
#include "common.hpp"

namespace moma {
namespace {

constexpr int HINT_THREADS = 256;
constexpr int HINT_CHUNK = MOMA_HINT_CHUNK;  // pixels of one item
constexpr int HINT_MAX_GRID = 2048;          // 256 compute units x 8 workgroups
constexpr int HINT_FIN_THREADS = 1024;
constexpr int HINT_FIN_BATCH = 8;            // partials a lane of a finalize kernel requests before it adds them
static_assert(HINT_CHUNK % (64 * 8) == 0, "a chunk is whole vectors for whole waves");

enum { HINT_STATS = 0, HINT_LOSS = 1, HINT_BWD = 2 };
template <int MODE> constexpr int HINT_NS = MODE == HINT_STATS ? 2 : MODE == HINT_LOSS ? 3 : 0;   // sums per channel of a walk

struct HintShape {
    int B, C, P;
    int nhwc_t;                             // memory [B, P, C] instead of [B, C, P] on t's side
    int t_other;                            // t lies in the other layout than x: element accesses at (b, c, p)
    int nchunk;                             // ceil(P / HINT_CHUNK)
    int BI, nbg;                            // images of one item (planes below a chunk: as many as fill one), ceil(B / BI)
    int lgG, ctiles;                        // NCHW walk: log2 of the lanes per row; ceil(C / (256 >> lgG))
    int TW, RP, ntile;                      // NHWC walk: channel vectors per tile, pixel rows per pass, ceil(C / V / TW)
    long long items, rows;                  // rows = nbg * nchunk: partial rows per sum
};

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

template <typename TT>
__device__ __forceinline__ float hint_target1(const TT* __restrict__ t, const HintShape& q, int b, int c, int p) {
    return ld1<TT>(t + (q.nhwc_t ? ((size_t)b * q.P + p) * q.C + c : ((size_t)b * q.C + c) * q.P + p));
}

// x in NCHW.  grid-stride over items (image b, rows [ct R, ct R + R), pixels [k CHUNK, k CHUNK + len))
template <typename TX, typename TT, int V, int MODE>
__global__ __launch_bounds__(HINT_THREADS) void hint_nchw_kernel(const TX* __restrict__ x, const TT* __restrict__ t,
                                                                 double* __restrict__ partials, const HintVecs v,
                                                                 TX* __restrict__ dx, const HintShape q) {
    constexpr int NS = HINT_NS<MODE>;
    const int tid = threadIdx.x, G = 1 << q.lgG, R = HINT_THREADS >> q.lgG, r = tid >> q.lgG, i = tid & (G - 1);
    const int C = q.C, P = q.P;
    for (long long it = blockIdx.x; it < q.items; it += gridDim.x) {
        const int k = (int)(it % q.nchunk);
        const long long rest = it / q.nchunk;
        const int ct = (int)(rest % q.ctiles), bg = (int)(rest / q.ctiles);
        const int c = ct * R + r, p0 = k * HINT_CHUNK, len = min(HINT_CHUNK, P - p0);
        double s[NS ? NS : 1];
#pragma unroll
        for (int n = 0; n < NS; ++n) s[n] = 0.0;
        if (c < C) {
            const HintCh h = hint_ch<MODE>(v, C, c);
            for (int b = bg * q.BI, be = min(q.B, b + q.BI); b < be; ++b) {
            const size_t base = ((size_t)b * C + c) * P + p0;
            for (int pv = i * V; pv < len; pv += G * V) {                          // (P % V == 0: all V inside)
                float xv[V], tv[V];
                PV<TX, V>::ld(x + base + pv, xv);
                if constexpr (MODE != HINT_STATS) {
                    if (!q.t_other) PV<TT, V>::ld(t + base + pv, tv);
                    else {
#pragma unroll
                        for (int e = 0; e < V; ++e) tv[e] = hint_target1<TT>(t, q, b, c, p0 + pv + e);
                    }
                }
#pragma unroll
                for (int e = 0; e < V; ++e) xv[e] = hint_elem<MODE>(xv[e], MODE != HINT_STATS ? tv[e] : 0.f, h, s);
                if constexpr (MODE == HINT_BWD) PV<TX, V>::st(dx + base + pv, xv);
            }
            }
        }
#pragma unroll
        for (int n = 0; n < NS; ++n) {
            double u = s[n];
            for (int o = G >> 1; o > 0; o >>= 1) u += __shfl_xor(u, o, 64);          // (G divides 64: a row's lanes share a wave)
            if (i == 0 && c < C) partials[((size_t)n * q.rows + (size_t)bg * q.nchunk + k) * C + c] = u;
        }
    }
}

// x in channels_last.  grid-stride over items (image b, channel vectors [ti TW, ti TW + TW), pixels [k CHUNK, k CHUNK + len))
template <typename TX, typename TT, int V, int MODE>
__global__ __launch_bounds__(HINT_THREADS) void hint_nhwc_kernel(const TX* __restrict__ x, const TT* __restrict__ t,
                                                                 double* __restrict__ partials, const HintVecs v,
                                                                 TX* __restrict__ dx, const HintShape q) {
    constexpr int NS = HINT_NS<MODE>;
    __shared__ double sh[NS ? NS : 1][NS ? V : 1][NS ? HINT_THREADS : 1];
    const int tid = threadIdx.x, TW = q.TW, RP = q.RP, tc = tid % TW, tr = tid / TW;
    const int C = q.C, P = q.P, ncv = C / V;
    for (long long it = blockIdx.x; it < q.items; it += gridDim.x) {
        const int k = (int)(it % q.nchunk);
        const long long rest = it / q.nchunk;
        const int ti = (int)(rest % q.ntile), bg = (int)(rest / q.ntile);
        const int cv = ti * TW + tc, c0 = cv * V, p0 = k * HINT_CHUNK, pe = p0 + min(HINT_CHUNK, P - p0);
        double s[V][NS ? NS : 1];
#pragma unroll
        for (int e = 0; e < V; ++e)
#pragma unroll
            for (int n = 0; n < NS; ++n) s[e][n] = 0.0;
        if (tr < RP && cv < ncv) {
            HintCh h[V];
#pragma unroll
            for (int e = 0; e < V; ++e) h[e] = hint_ch<MODE>(v, C, c0 + e);
            for (int b = bg * q.BI, be = min(q.B, b + q.BI); b < be; ++b)
            for (int p = p0 + tr; p < pe; p += RP) {
                const size_t at = ((size_t)b * P + p) * C + c0;
                float xv[V], tv[V];
                PV<TX, V>::ld(x + at, xv);
                if constexpr (MODE != HINT_STATS) {
                    if (!q.t_other) PV<TT, V>::ld(t + at, tv);
                    else {
#pragma unroll
                        for (int e = 0; e < V; ++e) tv[e] = hint_target1<TT>(t, q, b, c0 + e, p);
                    }
                }
#pragma unroll
                for (int e = 0; e < V; ++e) xv[e] = hint_elem<MODE>(xv[e], MODE != HINT_STATS ? tv[e] : 0.f, h[e], s[e]);
                if constexpr (MODE == HINT_BWD) PV<TX, V>::st(dx + at, xv);
            }
        }
        if constexpr (NS > 0) {
            __syncthreads();                                                       // the sums of the previous item have been read
#pragma unroll
            for (int n = 0; n < NS; ++n)
#pragma unroll
                for (int e = 0; e < V; ++e) sh[n][e][tid] = s[e][n];
            __syncthreads();
            // one thread per (sum, element, channel vector) of the tile adds the RP pixel rows in the order of tr
            for (int j = tid; j < NS * V * TW; j += HINT_THREADS) {
                const int n = j / (V * TW), e = (j / TW) % V, t2 = j % TW, cv2 = ti * TW + t2;
                if (cv2 < ncv) {
                    double u = 0.0;
                    for (int rr = 0; rr < RP; ++rr) u += sh[n][e][rr * TW + t2];
                    partials[((size_t)n * q.rows + (size_t)bg * q.nchunk + k) * C + cv2 * V + e] = u;
                }
            }
        }
    }
}

// the finalize kernels' sums: the L = 1 << lgL lanes of channel c add partial rows i, i + L, ... of each of the NS sums in order
// (HINT_FIN_BATCH requests in flight) and meet over the lane bits above the channel's; lane = i * cpw + cw, cpw = 64 >> lgL
template <int NS>
__device__ __forceinline__ void hint_fin_sums(const double* __restrict__ partials, long long J, int C, int c, int i, int lgL, double* s) {
    const int L = 1 << lgL, cpw = 64 >> lgL;
#pragma unroll
    for (int n = 0; n < NS; ++n) {
        double u = 0.0;
        const double* pn = partials + (size_t)n * J * C;
        if (c < C)
            for (long long j0 = i; j0 < J; j0 += (long long)HINT_FIN_BATCH * L) {
                double w[HINT_FIN_BATCH];
#pragma unroll
                for (int b = 0; b < HINT_FIN_BATCH; ++b) {
                    const long long j = j0 + (long long)b * L;
                    w[b] = j < J ? pn[(size_t)j * C + c] : 0.0;
                }
#pragma unroll
                for (int b = 0; b < HINT_FIN_BATCH; ++b) u += w[b];
            }
        for (int o = 32; o >= cpw; o >>= 1) u += __shfl_xor(u, o, 64);
        s[n] = u;
    }
}

// one workgroup.  Wave w owns channels [w cpw, w cpw + cpw), then 16 cpw further, ...
__global__ __launch_bounds__(HINT_FIN_THREADS) void hint_stats_finalize_kernel(const double* __restrict__ partials, long long J, int C,
                                                                               int lgL, const float* __restrict__ conv_bias,
                                                                               float* __restrict__ running_mean,
                                                                               float* __restrict__ running_var, double momentum,
                                                                               double eps, double M, double unbias,
                                                                               double* __restrict__ mean, double* __restrict__ invstd) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int cpw = 64 >> lgL, cw = lane & (cpw - 1), i = lane >> (6 - lgL);
    for (int cb = w * cpw; cb < C; cb += (HINT_FIN_THREADS / 64) * cpw) {          // (wave-uniform)
        const int c = cb + cw;
        double s[2];
        hint_fin_sums<2>(partials, J, C, c, i, lgL, s);
        if (i == 0 && c < C) {
            const double m = s[0] / M;                                             // (divisions: a constant channel has var = 0 exactly)
            const double var = fmax(s[1] / M - m * m, 0.0);
            mean[c] = m;
            invstd[c] = 1.0 / sqrt(var + eps);
            if (running_mean)
                running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] +
                                          momentum * (m + (conv_bias ? (double)conv_bias[c] : 0.0)));
            if (running_var) running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * var * unbias);
        }
    }
}

__global__ __launch_bounds__(HINT_FIN_THREADS) void hint_loss_finalize_kernel(const double* __restrict__ partials, long long J, int C,
                                                                              int lgL, double inv_n, double* __restrict__ sums,
                                                                              float* __restrict__ loss) {
    __shared__ double sh[HINT_FIN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int cpw = 64 >> lgL, cw = lane & (cpw - 1), i = lane >> (6 - lgL);
    double term = 0.0;
    for (int cb = w * cpw; cb < C; cb += (HINT_FIN_THREADS / 64) * cpw) {
        const int c = cb + cw;
        double s[3];
        hint_fin_sums<3>(partials, J, C, c, i, lgL, s);
        if (i == 0 && c < C) {
            term += s[0];
            sums[c] = s[1];
            sums[C + c] = s[2];
        }
    }
    term = wave_sum(term);
    if (lane == 0) sh[w] = term;
    __syncthreads();
    if (tid == 0) {
        double u = 0.0;
        for (int z = 0; z < HINT_FIN_THREADS / 64; ++z) u += sh[z];
        *loss = (float)(u * inv_n);
    }
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
// so the partial rows -- what the one-workgroup finalize kernels walk -- stay near B P / HINT_CHUNK
int hint_images_per_item(int B, int P) { return max(1, min(B, HINT_CHUNK / P)); }

int hint_pow2_ceil_lg(long long n) {          // smallest lg with (1 << lg) >= n
    int lg = 0;
    while ((1LL << lg) < n) ++lg;
    return lg;
}

// the widest of 8, 4, 1 elements that divides the contiguous extent and whose accesses (16 bytes at most each) are aligned
int hint_side_vec(const void* p, int extent, int dtype) {
    if (dtype == MOMA_DT_BF16) return pick_vec(extent, 2, (uintptr_t)p, {8, 4});
    const int v = pick_vec(extent, 4, (uintptr_t)p, {4});
    return v == 4 && extent % 8 == 0 ? 8 : v;                                      // (8 fp32: two 16-byte accesses)
}

// the walk of a launch: t (nullable: the statistics) is read, dx (nullable) is accessed like x
HintShape hint_shape(const void* x, const void* t, const void* dx, int B, int C, int P, int dt_x, int lay_x, int dt_t, int lay_t,
                     int* vec) {
    HintShape q{};
    q.B = B; q.C = C; q.P = P;
    const int nhwc_x = lay_x == MOMA_LAYOUT_NHWC;
    q.nhwc_t = lay_t == MOMA_LAYOUT_NHWC;
    q.t_other = t != nullptr && nhwc_x != q.nhwc_t;
    q.nchunk = (P + HINT_CHUNK - 1) / HINT_CHUNK;
    q.BI = hint_images_per_item(B, P);
    q.nbg = (B + q.BI - 1) / q.BI;
    const int extent = nhwc_x ? C : P;
    int V = hint_side_vec(x, extent, dt_x);
    if (dx) V = min(V, hint_side_vec(dx, extent, dt_x));
    if (t && !q.t_other) V = min(V, hint_side_vec(t, extent, dt_t));
    *vec = V;
    const int vecs = (min(P, HINT_CHUNK) + V - 1) / V;                             // vectors of the longest row piece
    q.lgG = min(6, hint_pow2_ceil_lg(vecs));
    const int R = HINT_THREADS >> q.lgG;
    q.ctiles = (C + R - 1) / R;
    const int ncv = C / V;                                                         // (channels_last: C % V == 0)
    q.TW = max(1, min(ncv, 64 / V));
    q.RP = HINT_THREADS / q.TW;
    q.ntile = (ncv + q.TW - 1) / q.TW;
    q.rows = (long long)q.nbg * q.nchunk;
    q.items = q.rows * (nhwc_x ? q.ntile : q.ctiles);
    return q;
}

template <int MODE>
hipError_t hint_launch(const void* x, const void* t, double* partials, const HintVecs& vecs, void* dx, int B, int C, int P, int dt_x,
                       int lay_x, int dt_t, int lay_t, hipStream_t st) {
    int vec = 1;
    const HintShape q = hint_shape(x, t, dx, B, C, P, dt_x, lay_x, dt_t, lay_t, &vec);
    const unsigned grid = (unsigned)min(q.items, (long long)HINT_MAX_GRID);
    const bool nhwc_x = lay_x == MOMA_LAYOUT_NHWC;
    with_dtype(dt_x, [&](auto tx) {
        return with_dtype(MODE == HINT_STATS ? dt_x : dt_t, [&](auto tt) {         // (the statistics read no t: one instantiation)
            using TX = typename decltype(tx)::type;
            using TT = typename decltype(tt)::type;
            with_vec<8, 8, 4, 1>(vec, [&](auto w) {
                constexpr int V = decltype(w)::value;
                if (nhwc_x)
                    hipLaunchKernelGGL((hint_nhwc_kernel<TX, TT, V, MODE>), dim3(grid), dim3(HINT_THREADS), 0, st, (const TX*)x,
                                       (const TT*)t, partials, vecs, (TX*)dx, q);
                else
                    hipLaunchKernelGGL((hint_nchw_kernel<TX, TT, V, MODE>), dim3(grid), dim3(HINT_THREADS), 0, st, (const TX*)x,
                                       (const TT*)t, partials, vecs, (TX*)dx, q);
            });
            return 0;
        });
    });
    return hipGetLastError();
}

// lanes per channel of a finalize kernel: the power of two (1 .. 64) with which C channels fill the workgroup
int hint_fin_lg(int C) { return max(0, min(6, 10 - hint_pow2_ceil_lg(C))); }

}  // namespace

long long hint_partial_rows(int B, int P) {
    const int bi = hint_images_per_item(B, P);
    return (long long)((B + bi - 1) / bi) * ((P + HINT_CHUNK - 1) / HINT_CHUNK);
}
size_t hint_workspace_bytes(int B, int C, int P) { return (size_t)hint_partial_rows(B, P) * (size_t)C * 3 * sizeof(double); }

hipError_t launch_hint_fwd(const void* x, const void* t, const float* gamma, const float* beta, const float* conv_bias,
                           float* running_mean, float* running_var, float momentum, float eps, int B, int C, int P, int dt_x,
                           int lay_x, int dt_t, int lay_t, double* partials, double* mean, double* invstd, double* sums, float* loss,
                           hipStream_t st) {
    const double M = (double)B * P;
    const long long J = hint_partial_rows(B, P);
    const int lgL = hint_fin_lg(C);
    HintVecs v{};
    hipError_t e = hint_launch<HINT_STATS>(x, nullptr, partials, v, nullptr, B, C, P, dt_x, lay_x, dt_x, lay_x, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hint_stats_finalize_kernel, dim3(1), dim3(HINT_FIN_THREADS), 0, st, (const double*)partials, J, C, lgL, conv_bias,
                       running_mean, running_var, (double)momentum, (double)eps, M, M / (M - 1.0), mean, invstd);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    v.gamma = gamma; v.beta = beta; v.mean = mean; v.invstd = invstd;
    e = hint_launch<HINT_LOSS>(x, t, partials, v, nullptr, B, C, P, dt_x, lay_x, dt_t, lay_t, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hint_loss_finalize_kernel, dim3(1), dim3(HINT_FIN_THREADS), 0, st, (const double*)partials, J, C, lgL,
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
