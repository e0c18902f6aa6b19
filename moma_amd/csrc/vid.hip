// Variational Information Distillation (`--distill vid`; reference distiller_zoo/VID.py, helper/loops_moma.py:145-149): the per-channel
// Gaussian negative log-likelihood of a regressor's output `mean` [B,C,H,W] against `target` [B,C,H,W], P = H W:
//     var_c = log(1 + exp(log_scale_c)) + eps      S_c = sum_{b,p} (mean - target)[b,c,p]^2
//     loss  = 0.5 / C * sum_c ( S_c / (B P var_c) + log var_c )
//     d_mean = g_loss (mean - target) / (var_c B C P)
//     d_var_c = 0.5 / C * ( 1 / var_c - S_c / (B P var_c^2) )      d_log_scale_c = d_var_c exp(log_scale_c) / (1 + exp(log_scale_c))
// in three kinds of launch, storage fp32 or bf16 and NCHW or channels_last, each chosen per side:
//   vid_map<.., BWD = false>  streams both maps once.  The work is cut into ITEMS whose shape follows the layout of `mean`:
//             NCHW  (image, block of R = 256 / G channel rows, chunk of VID_CHUNK pixels); G = 1 .. 64 lanes walk one row, G the
//                   power of two that covers min(P, VID_CHUNK) / V vectors -- a 16 x 16 plane takes 32 lanes of 8 elements and a
//                   workgroup holds 8 rows, a 128 x 128 plane takes whole waves.  A thread's fp32 sum is at most VID_CHUNK / 64
//                   squares long; the G lanes meet in double by xor shuffles (no LDS, no barrier).
//             NHWC  (image, tile of TW <= 64 / V channel vectors, chunk of VID_CHUNK pixels); thread (tr, tc) walks pixels tr, tr + RP,
//                   ... of channel vector tc, RP = 256 / TW: with TW = C / V the pixels of a pass are one contiguous range.  A thread's
//                   fp32 sums are cut every 16 pixels and added to double totals; the RP threads of a channel meet through LDS, in
//                   the order of tr.
//             Each item writes one double per channel it covers: partials [B * nchunk, C], nchunk = ceil(P / VID_CHUNK).  The grid is
//             capped at VID_MAX_GRID workgroups which stride over the items, so neither 1280 channels x 64 planes of 256 pixels
//             (10240 / 1280 items) nor 24 channels x 64 planes of 16384 pixels (6144 / 1024 items) leaves compute units idle; what
//             a partial holds depends on the item alone, never on the grid.
//             A `target` in the OTHER layout than `mean` is read element by element at the same (b, c, p): correct, not fast.
//   vid_finalize  ONE workgroup of 16 waves: L = 1 .. 64 lanes per channel (the power of two that fills 1024 threads) add partials
//             l, l + L, ... in order (eight requests in flight), then a xor tree, all in double -> sq, var, g_log_scale (the
//             softplus, its logarithm and its derivative in double, in the overflow-free form: finite for any finite log_scale,
//             where the reference's fp32 exp is inf above 88); the channels' terms meet per wave, then over the 16 waves in
//             order -> loss.
//   vid_map<.., BWD = true>  the same walk; d_mean = round(double(mean - target) * (g_loss / (var_c B C P))), the factor formed in
//             double per channel from var (fp32) and g_loss, a DEVICE scalar; written in mean's dtype and layout.
// 16-byte accesses (two for 8 fp32) where the address and the contiguous extent (P, or C) allow on every side that is walked in
// vectors, 4 elements where only that divides, element accesses otherwise.  No atomics: bitwise repeatable.
// hipcc -O3, gfx950: 24 .. 56 VGPRs (NCHW map), 22 .. 102 (NHWC map, 8 double totals and 8 factors), no spill, no scratch; LDS
// 16 KB at most (NHWC forward only).
#include "common.hpp"

namespace moma {
namespace {

constexpr int VID_THREADS = 256;
constexpr int VID_CHUNK = MOMA_VID_CHUNK;   // pixels of one item
constexpr int VID_RUN = 16;                 // pixels of one fp32 chain (NHWC map)
constexpr int VID_MAX_GRID = 2048;          // 256 compute units x 8 workgroups
constexpr int VID_FIN_THREADS = 1024;
constexpr int VID_FIN_BATCH = 8;            // partials a lane of the finalize kernel requests before it adds them
static_assert(VID_CHUNK % (64 * 8) == 0, "a chunk is whole vectors for whole waves");

struct VidShape {
    int B, C, P;
    int nhwc_t;                             // memory [B, P, C] instead of [B, C, P] on the target's side
    int t_other;                            // the target lies in the other layout than mean: element accesses at (b, c, p)
    int nchunk;                             // ceil(P / VID_CHUNK)
    int lgG, ctiles;                        // NCHW map: log2 of the lanes per row; ceil(C / (256 >> lgG))
    int TW, RP, ntile;                      // NHWC map: channel vectors per tile, pixel rows per pass, ceil(C / V / TW)
    long long items;
};

template <typename TT>
__device__ __forceinline__ float vid_target1(const TT* __restrict__ target, const VidShape& q, int b, int c, int p) {
    return ld1<TT>(target + (q.nhwc_t ? ((size_t)b * q.P + p) * q.C + c : ((size_t)b * q.C + c) * q.P + p));
}

// mean in NCHW.  grid-stride over items (image b, rows [ct R, ct R + R), pixels [k CHUNK, k CHUNK + len))
template <typename TM, typename TT, int V, bool BWD>
__global__ __launch_bounds__(VID_THREADS) void vid_nchw_kernel(const TM* __restrict__ mean, const TT* __restrict__ target,
                                                               double* __restrict__ partials, const float* __restrict__ var,
                                                               const float* __restrict__ g_loss, TM* __restrict__ d_mean,
                                                               const VidShape q, double inv_n) {
    const int tid = threadIdx.x, G = 1 << q.lgG, R = VID_THREADS >> q.lgG, r = tid >> q.lgG, i = tid & (G - 1);
    const int C = q.C, P = q.P;
    for (long long it = blockIdx.x; it < q.items; it += gridDim.x) {
        const int k = (int)(it % q.nchunk);
        const long long rest = it / q.nchunk;
        const int ct = (int)(rest % q.ctiles), b = (int)(rest / q.ctiles);
        const int c = ct * R + r, p0 = k * VID_CHUNK, len = min(VID_CHUNK, P - p0);
        float acc = 0.f;
        if (c < C) {
            const size_t base = ((size_t)b * C + c) * P + p0;
            double kc = 0.0;
            if constexpr (BWD) kc = (double)*g_loss * inv_n / (double)var[c];
            for (int pv = i * V; pv < len; pv += G * V) {                          // (P % V == 0: all V inside)
                float m[V], t[V];
                PV<TM, V>::ld(mean + base + pv, m);
                if (!q.t_other) PV<TT, V>::ld(target + base + pv, t);
                else {
#pragma unroll
                    for (int e = 0; e < V; ++e) t[e] = vid_target1<TT>(target, q, b, c, p0 + pv + e);
                }
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float d = m[e] - t[e];
                    if constexpr (BWD) m[e] = round_f32((double)d * kc);
                    else acc = fmaf(d, d, acc);
                }
                if constexpr (BWD) PV<TM, V>::st(d_mean + base + pv, m);
            }
        }
        if constexpr (!BWD) {
            double s = (double)acc;
            for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);          // (G divides 64: a row's lanes share a wave)
            if (i == 0 && c < C) partials[((size_t)b * q.nchunk + k) * C + c] = s;
        }
    }
}

// mean in channels_last.  grid-stride over items (image b, channel vectors [ti TW, ti TW + TW), pixels [k CHUNK, k CHUNK + len))
template <typename TM, typename TT, int V, bool BWD>
__global__ __launch_bounds__(VID_THREADS) void vid_nhwc_kernel(const TM* __restrict__ mean, const TT* __restrict__ target,
                                                               double* __restrict__ partials, const float* __restrict__ var,
                                                               const float* __restrict__ g_loss, TM* __restrict__ d_mean,
                                                               const VidShape q, double inv_n) {
    __shared__ double sh[BWD ? 1 : V][BWD ? 1 : VID_THREADS];
    const int tid = threadIdx.x, TW = q.TW, RP = q.RP, tc = tid % TW, tr = tid / TW;
    const int C = q.C, P = q.P, ncv = C / V;
    for (long long it = blockIdx.x; it < q.items; it += gridDim.x) {
        const int k = (int)(it % q.nchunk);
        const long long rest = it / q.nchunk;
        const int ti = (int)(rest % q.ntile), b = (int)(rest / q.ntile);
        const int cv = ti * TW + tc, c0 = cv * V, p0 = k * VID_CHUNK, pe = p0 + min(VID_CHUNK, P - p0);
        double tot[V];
#pragma unroll
        for (int e = 0; e < V; ++e) tot[e] = 0.0;
        if (tr < RP && cv < ncv) {
            double kc[V];
#pragma unroll
            for (int e = 0; e < V; ++e) kc[e] = BWD ? (double)*g_loss * inv_n / (double)var[c0 + e] : 0.0;
            for (int p = p0 + tr; p < pe;) {
                float acc[V];
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] = 0.f;
                for (int n = 0; n < VID_RUN && p < pe; ++n, p += RP) {
                    const size_t at = ((size_t)b * P + p) * C + c0;
                    float m[V], t[V];
                    PV<TM, V>::ld(mean + at, m);
                    if (!q.t_other) PV<TT, V>::ld(target + at, t);
                    else {
#pragma unroll
                        for (int e = 0; e < V; ++e) t[e] = vid_target1<TT>(target, q, b, c0 + e, p);
                    }
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const float d = m[e] - t[e];
                        if constexpr (BWD) m[e] = round_f32((double)d * kc[e]);
                        else acc[e] = fmaf(d, d, acc[e]);
                    }
                    if constexpr (BWD) PV<TM, V>::st(d_mean + at, m);
                }
#pragma unroll
                for (int e = 0; e < V; ++e) tot[e] += (double)acc[e];
            }
        }
        if constexpr (!BWD) {
            __syncthreads();                                                       // the sums of the previous item have been read
#pragma unroll
            for (int e = 0; e < V; ++e) sh[e][tid] = tot[e];
            __syncthreads();
            if (tid < TW && cv < ncv) {                                            // (tr = 0, tc = tid)
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    double s = 0.0;
                    for (int rr = 0; rr < RP; ++rr) s += sh[e][rr * TW + tid];
                    partials[((size_t)b * q.nchunk + k) * C + c0 + e] = s;
                }
            }
        }
    }
}

// one workgroup.  Wave w owns channels [w cpw, w cpw + cpw), then 16 cpw further, ...; cpw = 64 >> lgL channels per wave and pass,
// lane = i * cpw + cw: the L = 1 << lgL lanes of a channel add partials i, i + L, ... and meet over the lane bits above cw
__global__ __launch_bounds__(VID_FIN_THREADS) void vid_finalize_kernel(const double* __restrict__ partials, long long J, int C,
                                                                        const float* __restrict__ log_scale, double eps, double inv_bp,
                                                                        int lgL, float* __restrict__ sq, float* __restrict__ var,
                                                                        float* __restrict__ g_log_scale, float* __restrict__ loss) {
    __shared__ double sh[VID_FIN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int L = 1 << lgL, cpw = 64 >> lgL, cw = lane & (cpw - 1), i = lane >> (6 - lgL);
    double term = 0.0;
    for (int cb = w * cpw; cb < C; cb += (VID_FIN_THREADS / 64) * cpw) {          // (wave-uniform)
        const int c = cb + cw;
        double s = 0.0;
        if (c < C)
            for (long long j0 = i; j0 < J; j0 += (long long)VID_FIN_BATCH * L) {   // VID_FIN_BATCH loads in flight, added in order
                double v[VID_FIN_BATCH];
#pragma unroll
                for (int u = 0; u < VID_FIN_BATCH; ++u) {
                    const long long j = j0 + (long long)u * L;
                    v[u] = j < J ? partials[(size_t)j * C + c] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < VID_FIN_BATCH; ++u) s += v[u];
            }
        for (int o = 32; o >= cpw; o >>= 1) s += __shfl_xor(s, o, 64);
        if (i == 0 && c < C) {
            const double ls = (double)log_scale[c];
            // softplus and sigmoid without overflow: exp of a non-positive number only
            const double en = exp(-fabs(ls));
            const double v = (ls > 0.0 ? ls : 0.0) + log1p(en) + eps;
            const double sig = ls >= 0.0 ? 1.0 / (1.0 + en) : en / (1.0 + en);
            const double m = s * inv_bp;                                           // mean squared difference of the channel
            const double dv = (0.5 / (double)C) * (1.0 / v - m / (v * v));
            sq[c] = (float)s;
            var[c] = (float)v;
            g_log_scale[c] = (float)(dv * sig);
            term += m / v + log(v);
        }
    }
    term = wave_sum(term);
    if (lane == 0) sh[w] = term;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int x = 0; x < VID_FIN_THREADS / 64; ++x) t += sh[x];
        *loss = (float)(0.5 / (double)C * t);
    }
}

int vid_pow2_ceil_lg(long long n) {          // smallest lg with (1 << lg) >= n
    int lg = 0;
    while ((1LL << lg) < n) ++lg;
    return lg;
}

// the widest of 8, 4, 1 elements that divides the contiguous extent and whose accesses (16 bytes at most each) are aligned
int vid_side_vec(const void* p, int extent, int dtype) {
    if (dtype == MOMA_DT_BF16) return pick_vec(extent, 2, (uintptr_t)p, {8, 4});
    const int v = pick_vec(extent, 4, (uintptr_t)p, {4});
    return v == 4 && extent % 8 == 0 ? 8 : v;                                      // (8 fp32: two 16-byte accesses)
}

// the walk of a launch: d_mean (nullable) is accessed like mean
VidShape vid_shape(const void* mean, const void* target, const void* d_mean, int B, int C, int P, int dt_m, int lay_m, int dt_t,
                   int lay_t, int* vec) {
    VidShape q{};
    q.B = B; q.C = C; q.P = P;
    const int nhwc_m = lay_m == MOMA_LAYOUT_NHWC;
    q.nhwc_t = lay_t == MOMA_LAYOUT_NHWC;
    q.t_other = nhwc_m != q.nhwc_t;
    q.nchunk = (P + VID_CHUNK - 1) / VID_CHUNK;
    const int extent = nhwc_m ? C : P;
    int V = vid_side_vec(mean, extent, dt_m);
    if (d_mean) V = min(V, vid_side_vec(d_mean, extent, dt_m));
    if (!q.t_other) V = min(V, vid_side_vec(target, extent, dt_t));
    *vec = V;
    const int vecs = (min(P, VID_CHUNK) + V - 1) / V;                              // vectors of the longest row piece
    q.lgG = min(6, vid_pow2_ceil_lg(vecs));
    const int R = VID_THREADS >> q.lgG;
    q.ctiles = (C + R - 1) / R;
    const int ncv = C / V;                                                         // (channels_last: C % V == 0)
    q.TW = max(1, min(ncv, 64 / V));
    q.RP = VID_THREADS / q.TW;
    q.ntile = (ncv + q.TW - 1) / q.TW;
    q.items = (long long)B * q.nchunk * (nhwc_m ? q.ntile : q.ctiles);
    return q;
}

template <bool BWD>
hipError_t vid_launch(const void* mean, const void* target, double* partials, const float* var, const float* g_loss, void* d_mean,
                      int B, int C, int P, int dt_m, int lay_m, int dt_t, int lay_t, hipStream_t st) {
    int vec = 1;
    const VidShape q = vid_shape(mean, target, d_mean, B, C, P, dt_m, lay_m, dt_t, lay_t, &vec);
    const unsigned grid = (unsigned)min(q.items, (long long)VID_MAX_GRID);
    const double inv_n = 1.0 / ((double)B * C * P);
    const bool nhwc_m = lay_m == MOMA_LAYOUT_NHWC;
    with_dtype(dt_m, [&](auto tm) {
        return with_dtype(dt_t, [&](auto tt) {
            using TM = typename decltype(tm)::type;
            using TT = typename decltype(tt)::type;
            with_vec<8, 8, 4, 1>(vec, [&](auto v) {
                constexpr int V = decltype(v)::value;
                if (nhwc_m)
                    hipLaunchKernelGGL((vid_nhwc_kernel<TM, TT, V, BWD>), dim3(grid), dim3(VID_THREADS), 0, st, (const TM*)mean,
                                       (const TT*)target, partials, var, g_loss, (TM*)d_mean, q, inv_n);
                else
                    hipLaunchKernelGGL((vid_nchw_kernel<TM, TT, V, BWD>), dim3(grid), dim3(VID_THREADS), 0, st, (const TM*)mean,
                                       (const TT*)target, partials, var, g_loss, (TM*)d_mean, q, inv_n);
            });
            return 0;
        });
    });
    return hipGetLastError();
}

}  // namespace

long long vid_partial_rows(int B, int P) { return (long long)B * ((P + VID_CHUNK - 1) / VID_CHUNK); }
size_t vid_workspace_bytes(int B, int C, int P) { return (size_t)vid_partial_rows(B, P) * (size_t)C * sizeof(double); }

hipError_t launch_vid_nll(const void* mean, const void* target, const float* log_scale, float eps, int B, int C, int P, int dt_m,
                          int lay_m, int dt_t, int lay_t, double* partials, float* sq, float* var, float* g_log_scale, float* loss,
                          hipStream_t st) {
    hipError_t e = vid_launch<false>(mean, target, partials, nullptr, nullptr, nullptr, B, C, P, dt_m, lay_m, dt_t, lay_t, st);
    if (e != hipSuccess) return e;
    // lanes per channel: the power of two (1 .. 64) with which C channels fill the workgroup
    const int lgL = max(0, min(6, 10 - vid_pow2_ceil_lg(C)));
    hipLaunchKernelGGL(vid_finalize_kernel, dim3(1), dim3(VID_FIN_THREADS), 0, st, (const double*)partials, vid_partial_rows(B, P), C,
                       log_scale, (double)eps, 1.0 / ((double)B * P), lgL, sq, var, g_log_scale, loss);
    return hipGetLastError();
}

hipError_t launch_vid_bwd(const void* mean, const void* target, const float* var, const float* g_loss, void* d_mean, int B, int C,
                          int P, int dt_m, int lay_m, int dt_t, int lay_t, hipStream_t st) {
    return vid_launch<true>(mean, target, nullptr, var, g_loss, d_mean, B, C, P, dt_m, lay_m, dt_t, lay_t, st);
}

}  // namespace moma
