// Attention Transfer (`--distill attention`; reference distiller_zoo/AT.py, helper/loops_moma.py:287-292) for p = 2 on one pair of
// feature maps f_s [B,Cs,Hs,Ws], f_t [B,Ct,Ht,Wt]:
//     a[b, y w + x] = (1/C) sum_c pool(f)[b,c,y,x]^2        ah = a / max(|a|_2, 1e-12)        loss = mean (ah_s - ah_t)^2
// in three kinds of launch:
//   at_map   one read of f -> a (fp32).  HBM streaming; NCHW: lanes along the contiguous pixels, the 4 waves of a workgroup share the
//            channels (and, where (b, pixel tiles) alone would leave compute units idle, so do several workgroups: their partial
//            maps meet in a second launch in split order); channels_last: LPP lanes along the channels of one pixel with vector
//            loads, 64 / LPP pixels per wave, an xor-shuffle reduction per pixel.  An integer-ratio average pool is folded in (the
//            window is averaged per channel, then squared).
//   at_pair  the two [B, n] maps -> row norms, the row's share of the loss, g_a = d loss / d a per side (normalisation Jacobian and
//            2 / (B n) applied).  One workgroup per batch row, double arithmetic: the maps are C times smaller than the features,
//            and ah_s - ah_t cancels.  A second launch adds the B row sums in a fixed order.
//   at_bwd   one read of f (+ g_a) -> dF in f's dtype and layout: dF = g_loss * g_a * (2 / (C r^2)) * pool(f), g_loss a DEVICE scalar.
// No atomics: every sum has an order that depends on the shapes alone -- bitwise repeatable.  Plain C++ (no inline asm).
#include "common.hpp"

namespace moma {
namespace {

constexpr int AT_WAVES = 4;
constexpr int AT_THREADS = AT_WAVES * 64;
constexpr long AT_MAX_BLOCKS = 2048;          // 8 workgroups of 4 waves per compute unit; the kernels stride over the rest

struct AtShape {
    int B, C, H, W, oh, ow, rh, rw;
};

// ---- NCHW ----------------------------------------------------------------------------------------------------------------------
// work item = (b, tile of 64 * VEC output pixels, channel split s); wave w of the workgroup takes channels c0 + w, c0 + w + 4, ...
// out = a (S == 1, scale = 1 / C) or the partial maps [S, B, oh * ow] (scale = 1)
template <typename T, int VEC, bool POOL>
__global__ __launch_bounds__(AT_THREADS) void at_map_nchw_kernel(const T* __restrict__ f, float* __restrict__ out, const AtShape q,
                                                                 int tiles, int S, int cps, float scale, long long items) {
    __shared__ float sh[AT_WAVES][64 * VEC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ohw = q.oh * q.ow;
    const size_t HW = (size_t)q.H * q.W;
    const float inv_win = 1.f / (float)(q.rh * q.rw);
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {         // (workgroup-uniform: the barriers below are safe)
        const int s = (int)(it % S);
        const long long r = it / S;
        const int tile = (int)(r % tiles), b = (int)(r / tiles);
        const int p0 = (tile * 64 + lane) * VEC;                           // VEC > 1 only where ohw % VEC == 0: all or nothing
        const bool act = p0 < ohw;
        const int c0 = s * cps, c1 = min(q.C, c0 + cps);
        float acc[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
        if (act) {
            if constexpr (!POOL) {
                const T* p = f + ((size_t)b * q.C + c0 + w) * HW + p0;
#pragma unroll 4
                for (int c = c0 + w; c < c1; c += AT_WAVES, p += AT_WAVES * HW) {
                    float v[VEC];
                    PV<T, VEC>::ld(p, v);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) acc[j] = fmaf(v[j], v[j], acc[j]);
                }
            } else {
                const int oy = p0 / q.ow, ox = p0 % q.ow;
                const T* p = f + ((size_t)b * q.C + c0 + w) * HW + (size_t)oy * q.rh * q.W + (size_t)ox * q.rw;
                for (int c = c0 + w; c < c1; c += AT_WAVES, p += AT_WAVES * HW) {
                    float sum = 0.f;
                    for (int wy = 0; wy < q.rh; ++wy)
                        for (int wx = 0; wx < q.rw; ++wx) sum += ld1<T>(p + (size_t)wy * q.W + wx);
                    sum *= inv_win;
                    acc[0] = fmaf(sum, sum, acc[0]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) sh[w][lane * VEC + j] = acc[j];
        __syncthreads();
        if (w == 0 && act) {
            float* o = out + ((size_t)s * q.B + b) * ohw + p0;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int k = lane * VEC + j;
                o[j] = ((sh[0][k] + sh[1][k]) + (sh[2][k] + sh[3][k])) * scale;
            }
        }
        __syncthreads();
    }
}

// a[i] = (part[0][i] + part[1][i] + ... + part[S-1][i]) / C, in split order
__global__ __launch_bounds__(AT_THREADS) void at_map_combine_kernel(const float* __restrict__ part, float* __restrict__ a, int S,
                                                                    long long n, float inv_C) {
    for (long long i = (long long)blockIdx.x * AT_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * AT_THREADS) {
        float t = part[i];
        for (int s = 1; s < S; ++s) t += part[(size_t)s * n + i];
        a[i] = t * inv_C;
    }
}

// work item = (b, tile, channel chunk): dF[b,c,window of p] = (g_loss * g_a[b,p] * k) * pool(f)[b,c,p],  k = 2 / (C rh rw)
template <typename T, int VEC, bool POOL>
__global__ __launch_bounds__(AT_THREADS) void at_bwd_nchw_kernel(const T* __restrict__ f, const float* __restrict__ g_a,
                                                                 const float* __restrict__ g_loss, T* __restrict__ dF, const AtShape q,
                                                                 int tiles, int nchunk, int cpc, float k, long long items) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ohw = q.oh * q.ow;
    const size_t HW = (size_t)q.H * q.W;
    const float inv_win = 1.f / (float)(q.rh * q.rw);
    const float gl = *g_loss;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int chunk = (int)(it % nchunk);
        const long long r = it / nchunk;
        const int tile = (int)(r % tiles), b = (int)(r / tiles);
        const int p0 = (tile * 64 + lane) * VEC;
        if (p0 >= ohw) continue;                                           // (no barrier in this kernel)
        float gv[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) gv[j] = gl * g_a[(size_t)b * ohw + p0 + j] * k;
        const int c0 = chunk * cpc, c1 = min(q.C, c0 + cpc);
        if constexpr (!POOL) {
            size_t off = ((size_t)b * q.C + c0 + w) * HW + p0;
            for (int c = c0 + w; c < c1; c += AT_WAVES, off += AT_WAVES * HW) {
                float v[VEC];
                PV<T, VEC>::ld(f + off, v);
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[j] *= gv[j];
                PV<T, VEC>::st(dF + off, v);
            }
        } else {
            const int oy = p0 / q.ow, ox = p0 % q.ow;
            size_t off = ((size_t)b * q.C + c0 + w) * HW + (size_t)oy * q.rh * q.W + (size_t)ox * q.rw;
            for (int c = c0 + w; c < c1; c += AT_WAVES, off += AT_WAVES * HW) {
                float sum = 0.f;
                for (int wy = 0; wy < q.rh; ++wy)
                    for (int wx = 0; wx < q.rw; ++wx) sum += ld1<T>(f + off + (size_t)wy * q.W + wx);
                const float v = gv[0] * (sum * inv_win);
                for (int wy = 0; wy < q.rh; ++wy)
                    for (int wx = 0; wx < q.rw; ++wx) st1<T>(dF + off + (size_t)wy * q.W + wx, v);
            }
        }
    }
}

// ---- channels_last (memory [B, H, W, C]) -----------------------------------------------------------------------------------------
// LPP = 1 << lpp_log2 lanes share the C / VEC channel vectors of one output pixel; a wave carries 64 / LPP pixels side by side
template <typename T, int VEC>
__global__ __launch_bounds__(AT_THREADS) void at_map_nhwc_kernel(const T* __restrict__ f, float* __restrict__ a, const AtShape q,
                                                                 int lpp_log2, float inv_C, long long npix) {
    const int lane = threadIdx.x & 63;
    const int LPP = 1 << lpp_log2, ppw = 64 >> lpp_log2;
    const int g = lane >> lpp_log2, l = lane & (LPP - 1);
    const int nvc = q.C / VEC;
    const float inv_win = 1.f / (float)(q.rh * q.rw);
    const long long wave = (long long)blockIdx.x * AT_WAVES + (threadIdx.x >> 6), nwave = (long long)gridDim.x * AT_WAVES;
    for (long long base = wave * ppw; base < npix; base += nwave * ppw) {   // (wave-uniform: every lane reaches the shuffles)
        const long long pix = base + g;
        float acc = 0.f;
        if (pix < npix) {
            const int ox = (int)(pix % q.ow);
            const long long r = pix / q.ow;
            const int oy = (int)(r % q.oh), b = (int)(r / q.oh);
            const T* p = f + (((size_t)b * q.H + (size_t)oy * q.rh) * q.W + (size_t)ox * q.rw) * q.C;
            for (int v = l; v < nvc; v += LPP) {
                float s[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) s[j] = 0.f;
                for (int wy = 0; wy < q.rh; ++wy)
                    for (int wx = 0; wx < q.rw; ++wx) {
                        float t[VEC];
                        PV<T, VEC>::ld(p + ((size_t)wy * q.W + wx) * q.C + (size_t)v * VEC, t);
#pragma unroll
                        for (int j = 0; j < VEC; ++j) s[j] += t[j];
                    }
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float m = s[j] * inv_win;
                    acc = fmaf(m, m, acc);
                }
            }
        }
        for (int o = LPP >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (pix < npix && l == 0) a[pix] = acc * inv_C;
    }
}

template <typename T, int VEC>
__global__ __launch_bounds__(AT_THREADS) void at_bwd_nhwc_kernel(const T* __restrict__ f, const float* __restrict__ g_a,
                                                                 const float* __restrict__ g_loss, T* __restrict__ dF, const AtShape q,
                                                                 int lpp_log2, float k, long long npix) {
    const int lane = threadIdx.x & 63;
    const int LPP = 1 << lpp_log2, ppw = 64 >> lpp_log2;
    const int g = lane >> lpp_log2, l = lane & (LPP - 1);
    const int nvc = q.C / VEC;
    const float inv_win = 1.f / (float)(q.rh * q.rw);
    const float gl = *g_loss;
    const long long wave = (long long)blockIdx.x * AT_WAVES + (threadIdx.x >> 6), nwave = (long long)gridDim.x * AT_WAVES;
    for (long long base = wave * ppw; base < npix; base += nwave * ppw) {
        const long long pix = base + g;
        if (pix >= npix) continue;
        const int ox = (int)(pix % q.ow);
        const long long r = pix / q.ow;
        const int oy = (int)(r % q.oh), b = (int)(r / q.oh);
        const size_t off0 = (((size_t)b * q.H + (size_t)oy * q.rh) * q.W + (size_t)ox * q.rw) * q.C;
        const float gv = gl * g_a[pix] * k;
        for (int v = l; v < nvc; v += LPP) {
            float s[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) s[j] = 0.f;
            for (int wy = 0; wy < q.rh; ++wy)
                for (int wx = 0; wx < q.rw; ++wx) {
                    float t[VEC];
                    PV<T, VEC>::ld(f + off0 + ((size_t)wy * q.W + wx) * q.C + (size_t)v * VEC, t);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) s[j] += t[j];
                }
#pragma unroll
            for (int j = 0; j < VEC; ++j) s[j] = gv * (s[j] * inv_win);
            for (int wy = 0; wy < q.rh; ++wy)
                for (int wx = 0; wx < q.rw; ++wx) PV<T, VEC>::st(dF + off0 + ((size_t)wy * q.W + wx) * q.C + (size_t)v * VEC, s);
        }
    }
}

// ---- the pair ----------------------------------------------------------------------------------------------------------------------
// sum over the workgroup's 256 threads in an order that depends on nothing but the thread index; result in every thread
__device__ __forceinline__ double at_block_sum(double v, double* sh) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return r;
}

// grid (B): row b of both maps.  kk = 2 / (B n).  g_s / g_t / ah_s / ah_t may be NULL.
__global__ __launch_bounds__(AT_THREADS) void at_pair_kernel(const float* __restrict__ a_s, const float* __restrict__ a_t, int n,
                                                             float* __restrict__ norms, float* __restrict__ partials,
                                                             float* __restrict__ g_s, float* __restrict__ g_t,
                                                             float* __restrict__ ah_s, float* __restrict__ ah_t, double kk) {
    __shared__ double sh[AT_WAVES];
    constexpr double EPS = 1e-12;                                          // F.normalize's clamp of the norm
    const size_t row = (size_t)blockIdx.x * n;
    const float* __restrict__ ps = a_s + row;
    const float* __restrict__ pt = a_t + row;
    double ss = 0.0, tt = 0.0;
    for (int i = threadIdx.x; i < n; i += AT_THREADS) {
        const double x = ps[i], y = pt[i];
        ss = fma(x, x, ss);
        tt = fma(y, y, tt);
    }
    const double ns = sqrt(at_block_sum(ss, sh)), nt = sqrt(at_block_sum(tt, sh));
    const double ds = fmax(ns, EPS), dt = fmax(nt, EPS);
    double lp = 0.0, dot_s = 0.0, dot_t = 0.0;
    for (int i = threadIdx.x; i < n; i += AT_THREADS) {
        const double hs = ps[i] / ds, ht = pt[i] / dt, d = hs - ht;
        lp = fma(d, d, lp);
        dot_s = fma(hs, d, dot_s);
        dot_t = fma(ht, d, dot_t);
    }
    lp = at_block_sum(lp, sh);
    // the Jacobian of a / |a| takes the component along ah out; under the clamp the denominator is a constant: nothing to take out
    dot_s = at_block_sum(dot_s, sh);
    dot_t = at_block_sum(dot_t, sh);
    const double proj_s = ns >= EPS ? kk * dot_s : 0.0;
    const double proj_t = nt >= EPS ? -kk * dot_t : 0.0;
    for (int i = threadIdx.x; i < n; i += AT_THREADS) {
        const double hs = ps[i] / ds, ht = pt[i] / dt, ga = kk * (hs - ht);
        if (g_s) g_s[row + i] = (float)((ga - hs * proj_s) / ds);
        if (g_t) g_t[row + i] = (float)((-ga - ht * proj_t) / dt);
        if (ah_s) ah_s[row + i] = (float)hs;
        if (ah_t) ah_t[row + i] = (float)ht;
    }
    if (threadIdx.x == 0) {
        norms[2 * (size_t)blockIdx.x] = (float)ns;
        norms[2 * (size_t)blockIdx.x + 1] = (float)nt;
        partials[blockIdx.x] = (float)lp;
    }
}

// loss = (partials[0] + ... + partials[B-1]) / (B n): thread t adds rows t, t + 256, ... in order, then the fixed tree.  grid (1)
__global__ __launch_bounds__(AT_THREADS) void at_loss_kernel(const float* __restrict__ partials, float* __restrict__ loss, int B,
                                                             double inv_count) {
    __shared__ double sh[AT_WAVES];
    double t = 0.0;
    for (int i = threadIdx.x; i < B; i += AT_THREADS) t += (double)partials[i];
    t = at_block_sum(t, sh);
    if (threadIdx.x == 0) *loss = (float)(t * inv_count);
}

// ---- plans (host) ----------------------------------------------------------------------------------------------------------------
// 16 bytes / 4 elements / 1 (never 2) for `n_div` contiguous elements at an address with the low bits `bits`
int at_pick(long n_div, int elem_bytes, uintptr_t bits) { return pick_vec(n_div, elem_bytes, bits, {16 / elem_bytes, 4}); }
unsigned at_grid(long long items) {
    return (unsigned)(items < 1 ? 1 : (items > AT_MAX_BLOCKS ? AT_MAX_BLOCKS : items));
}
int at_lpp_log2(int nvc) {
    int l = 0;
    while ((1 << l) < nvc && l < 6) ++l;
    return l;
}
// NCHW forward: channel splits.  (b, tiles) alone fill the chip from 512 workgroups on; below that the channels are cut so that about
// 1024 workgroups exist, none with fewer than 32 channels.  Decided on the shape alone (not on the vector width the pointers allow).
int at_map_splits(const AtShape& q) {
    const long long ohw = (long long)q.oh * q.ow;
    const long long items0 = (long long)q.B * ((ohw + 255) / 256);
    if (items0 >= 512) return 1;
    long long S = (1024 + items0 - 1) / items0;
    const long long maxS = q.C / 32 > 1 ? q.C / 32 : 1;
    if (S > maxS) S = maxS;
    if (S > 64) S = 64;
    return (int)S;
}

}  // namespace

size_t at_workspace_bytes(int B, int C, int H, int W, int oh, int ow, int layout) {
    if (layout != MOMA_LAYOUT_NCHW) return 0;
    const AtShape q{B, C, H, W, oh, ow, H / oh, W / ow};
    const int S = at_map_splits(q);
    return S == 1 ? 0 : (size_t)S * B * oh * ow * sizeof(float);
}

// launch NCHW<T, V, POOL> (the pooling kernels are scalar) or NHWC<T, V> for the run-time (dtype, vec): f(kernel type tag, V[, POOL])
template <typename F> void at_nchw_dispatch(int dtype, bool pool, int vec, F&& f) {
    with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        if (pool) f(t, std::integral_constant<int, 1>{}, std::true_type{});
        else with_vec<MAXVEC<T>, 8, 4, 1>(vec, [&](auto V) { f(t, V, std::false_type{}); });
        return 0;
    });
}
template <typename F> void at_nhwc_dispatch(int dtype, int vec, F&& f) {
    with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        with_vec<MAXVEC<T>, 8, 4, 1>(vec, [&](auto V) { f(t, V); });
        return 0;
    });
}

hipError_t launch_at_map(const void* f, float* a, int B, int C, int H, int W, int oh, int ow, int dtype, int layout, void* ws,
                         hipStream_t st) {
    const AtShape q{B, C, H, W, oh, ow, H / oh, W / ow};
    const bool pool = q.rh * q.rw > 1;
    const int eb = dtype == MOMA_DT_BF16 ? 2 : 4;
    const long long ohw = (long long)oh * ow;
    const float inv_C = (float)(1.0 / (double)C);
    if (layout == MOMA_LAYOUT_NCHW) {
        const int vec = pool ? 1 : at_pick((long)ohw, eb, (uintptr_t)f);
        const int tiles = (int)((ohw + 64LL * vec - 1) / (64LL * vec));
        const int S = at_map_splits(q);
        const int cps = (C + S - 1) / S;
        const long long items = (long long)B * tiles * S;
        float* out = S == 1 ? a : (float*)ws;
        const float scale = S == 1 ? inv_C : 1.f;
        const dim3 grid(at_grid(items));
        at_nchw_dispatch(dtype, pool, vec, [&](auto t, auto V, auto POOL) {
            using T = typename decltype(t)::type;
            hipLaunchKernelGGL((at_map_nchw_kernel<T, V, POOL>), grid, dim3(AT_THREADS), 0, st, (const T*)f, out, q, tiles, S, cps, scale,
                               items);
        });
        hipError_t e = hipGetLastError();
        if (e != hipSuccess || S == 1) return e;
        const long long n = (long long)B * ohw;
        hipLaunchKernelGGL(at_map_combine_kernel, dim3(at_grid((n + AT_THREADS - 1) / AT_THREADS)), dim3(AT_THREADS), 0, st,
                           (const float*)ws, a, S, n, inv_C);
        return hipGetLastError();
    }
    const int vec = at_pick(C, eb, (uintptr_t)f);
    const int lpp_log2 = at_lpp_log2(C / vec);
    const long long npix = (long long)B * ohw;
    const long long ppb = (long long)AT_WAVES * (64 >> lpp_log2);
    const dim3 grid(at_grid((npix + ppb - 1) / ppb));
    at_nhwc_dispatch(dtype, vec, [&](auto t, auto V) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((at_map_nhwc_kernel<T, V>), grid, dim3(AT_THREADS), 0, st, (const T*)f, a, q, lpp_log2, inv_C, npix);
    });
    return hipGetLastError();
}

hipError_t launch_at_pair(const float* a_s, const float* a_t, int B, int n, float* norms, float* partials, float* loss, float* g_s,
                          float* g_t, float* ah_s, float* ah_t, hipStream_t st) {
    const double count = (double)B * (double)n;
    hipLaunchKernelGGL(at_pair_kernel, dim3(B), dim3(AT_THREADS), 0, st, a_s, a_t, n, norms, partials, g_s, g_t, ah_s, ah_t, 2.0 / count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(at_loss_kernel, dim3(1), dim3(AT_THREADS), 0, st, (const float*)partials, loss, B, 1.0 / count);
    return hipGetLastError();
}

hipError_t launch_at_bwd(const void* f, const float* g_a, const float* g_loss, void* dF, int B, int C, int H, int W, int oh, int ow,
                         int dtype, int layout, hipStream_t st) {
    const AtShape q{B, C, H, W, oh, ow, H / oh, W / ow};
    const bool pool = q.rh * q.rw > 1;
    const int eb = dtype == MOMA_DT_BF16 ? 2 : 4;
    const long long ohw = (long long)oh * ow;
    const float k = (float)(2.0 / ((double)C * q.rh * q.rw));
    const uintptr_t bits = (uintptr_t)f | (uintptr_t)dF;
    if (layout == MOMA_LAYOUT_NCHW) {
        const int vec = pool ? 1 : at_pick((long)ohw, eb, bits);
        const int tiles = (int)((ohw + 64LL * vec - 1) / (64LL * vec));
        // about 2048 workgroups over (b, tile, channel chunk), every wave of a chunk with a channel of its own where C allows
        const long long items0 = (long long)B * tiles;
        long long nchunk = (AT_MAX_BLOCKS + items0 - 1) / items0;
        const long long maxc = (C + AT_WAVES - 1) / AT_WAVES;
        if (nchunk > maxc) nchunk = maxc;
        const int cpc = (int)((C + nchunk - 1) / nchunk);
        nchunk = (C + cpc - 1) / cpc;
        const long long items = items0 * nchunk;
        const dim3 grid(at_grid(items));
        at_nchw_dispatch(dtype, pool, vec, [&](auto t, auto V, auto POOL) {
            using T = typename decltype(t)::type;
            hipLaunchKernelGGL((at_bwd_nchw_kernel<T, V, POOL>), grid, dim3(AT_THREADS), 0, st, (const T*)f, g_a, g_loss, (T*)dF, q, tiles,
                               (int)nchunk, cpc, k, items);
        });
        return hipGetLastError();
    }
    const int vec = at_pick(C, eb, bits);
    const int lpp_log2 = at_lpp_log2(C / vec);
    const long long npix = (long long)B * ohw;
    const long long ppb = (long long)AT_WAVES * (64 >> lpp_log2);
    const dim3 grid(at_grid((npix + ppb - 1) / ppb));
    at_nhwc_dispatch(dtype, vec, [&](auto t, auto V) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((at_bwd_nhwc_kernel<T, V>), grid, dim3(AT_THREADS), 0, st, (const T*)f, g_a, g_loss, (T*)dF, q, lpp_log2, k, npix);
    });
    return hipGetLastError();
}

}  // namespace moma
