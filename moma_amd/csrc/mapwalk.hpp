// What the losses that stream [B,C,H,W] maps share (vid.hip, hint.hip): ONE walk over x (and t, and dx), P = H W, storage fp32 or
// bf16 and NCHW or channels_last, each chosen per side, and the one-workgroup finalize sums behind it.  The including file says
// what happens to an element through a policy struct OP:
//     OP::Args                 the [C] operands of a launch, passed to the kernel by value
//     OP::NS                   sums per channel an item writes (0: none, the backward passes)
//     OP::READS_T, WRITES_DX   whether t is read, whether dx is written (in x's dtype and layout)
//     OP::ONE_IMAGE            the launch's BI is 1, known to the compiler: the image loop costs 7 .. 13 VGPRs, for vid's kernels a wave
//     OP::Ch, OP::ch(args, C, c)   one channel's constants in registers
//     OP::Acc                  a thread's accumulator for one channel of one item, zero when constructed:
//                              elem(x, t, ch) -> float (what goes to dx), totals(double s[NS]), and cut(), which the NHWC
//                              walk calls after every MAP_RUN of the thread's pixels (an fp32 chain ends there; an NCHW
//                              thread has at most MAP_CHUNK / 64 = MAP_RUN elements of an image and is never cut)
// The work is cut into ITEMS whose shape follows the layout of x:
//     NCHW  (BI images, block of R = 256 / G channel rows, chunk of MAP_CHUNK pixels); G = 1 .. 64 lanes walk one row, G the power of
//           two that covers min(P, MAP_CHUNK) / V vectors -- a 16 x 16 plane takes 32 lanes of 8 elements and a workgroup holds 8
//           rows, a 128 x 128 plane takes whole waves; the G lanes meet in double by xor shuffles (no LDS, no barrier).
//     NHWC  (BI images, tile of TW <= 64 / V channel vectors, chunk of MAP_CHUNK pixels); thread (tr, tc) walks pixels tr, tr + RP, ...
//           of channel vector tc, RP = 256 / TW: with TW = C / V the pixels of a pass are one contiguous range.  All sums go to LDS
//           at once and one thread per (sum, channel) adds the RP pixel rows in the order of tr.
// BI, the images of one item, is the caller's: 1 (vid), or as many as fill a chunk (hint).  Each item writes one double per sum and
// channel it covers: partials [NS, rows, C], rows = ceil(B / BI) * nchunk, nchunk = ceil(P / MAP_CHUNK); item (bg, k) owns row
// bg * nchunk + k.  The grid is capped at MAP_MAX_GRID workgroups which stride over the items, so neither 1280 channels x 64 planes
// of 256 pixels nor 24 channels x 64 planes of 16384 pixels leaves compute units idle; what a partial holds depends on the item
// alone, never on the grid.  A t in the OTHER layout than x is read element by element at the same (b, c, p): correct, not fast.
// 16-byte accesses (two for 8 fp32) where the address and the contiguous extent (P, or C) allow on every side that is walked in
// vectors, 4 elements where only that divides, element accesses otherwise.  No atomics: bitwise repeatable.
// The finalize kernels are ONE workgroup of 16 waves: L = 1 .. 64 lanes per channel (the power of two that fills 1024 threads) add
// the partial rows l, l + L, ... in order (eight requests in flight), then a xor tree, all in double; the channels' terms of a loss
// meet per wave, then over the 16 waves in order.
#pragma once
#include "common.hpp"

namespace moma {

constexpr int MAP_THREADS = 256;
constexpr int MAP_CHUNK = MOMA_VID_CHUNK;    // pixels of one item
constexpr int MAP_RUN = 16;                  // pixels of an NHWC thread between two cut()
constexpr int MAP_MAX_GRID = 2048;           // 256 compute units x 8 workgroups
constexpr int MAP_FIN_THREADS = 1024;
constexpr int MAP_FIN_BATCH = 8;             // partials a lane of a finalize kernel requests before it adds them
static_assert(MOMA_HINT_CHUNK == MAP_CHUNK, "the chunk is a compile-time constant of the one walk");
static_assert(MAP_CHUNK % (64 * 8) == 0 && MAP_CHUNK / 64 == MAP_RUN, "a chunk is whole vectors for whole waves");

struct MapShape {
    int B, C, P;
    int nhwc_t;                             // memory [B, P, C] instead of [B, C, P] on t's side
    int t_other;                            // t lies in the other layout than x: element accesses at (b, c, p)
    int nchunk;                             // ceil(P / MAP_CHUNK)
    int BI, nbg;                            // images of one item, ceil(B / BI)
    int lgG, ctiles;                        // NCHW walk: log2 of the lanes per row; ceil(C / (256 >> lgG))
    int TW, RP, ntile;                      // NHWC walk: channel vectors per tile, pixel rows per pass, ceil(C / V / TW)
    long long items, rows;                  // rows = nbg * nchunk: partial rows per sum
};

template <typename TT>
__device__ __forceinline__ float map_target1(const TT* __restrict__ t, const MapShape& q, int b, int c, int p) {
    return ld1<TT>(t + (q.nhwc_t ? ((size_t)b * q.P + p) * q.C + c : ((size_t)b * q.C + c) * q.P + p));
}

// x in NCHW.  grid-stride over items (images [bg BI, bg BI + BI), rows [ct R, ct R + R), pixels [k CHUNK, k CHUNK + len))
template <typename TX, typename TT, int V, typename OP>
__global__ __launch_bounds__(MAP_THREADS) void map_nchw_kernel(const TX* __restrict__ x, const TT* __restrict__ t,
                                                               double* __restrict__ partials, const typename OP::Args v,
                                                               TX* __restrict__ dx, const MapShape q) {
    constexpr int NS = OP::NS;
    const int tid = threadIdx.x, G = 1 << q.lgG, R = MAP_THREADS >> q.lgG, r = tid >> q.lgG, i = tid & (G - 1);
    const int C = q.C, P = q.P;
    for (long long it = blockIdx.x; it < q.items; it += gridDim.x) {
        const int k = (int)(it % q.nchunk);
        const long long rest = it / q.nchunk;
        const int ct = (int)(rest % q.ctiles), bg = (int)(rest / q.ctiles);
        const int c = ct * R + r, p0 = k * MAP_CHUNK, len = min(MAP_CHUNK, P - p0);
        typename OP::Acc acc;
        if (c < C) {
            const typename OP::Ch h = OP::ch(v, C, c);
            for (int b = bg * q.BI, be = OP::ONE_IMAGE ? b + 1 : min(q.B, b + q.BI); b < be; ++b) {
                const size_t base = ((size_t)b * C + c) * P + p0;
                for (int pv = i * V; pv < len; pv += G * V) {                      // (P % V == 0: all V inside)
                    float xv[V], tv[V];
                    PV<TX, V>::ld(x + base + pv, xv);
                    if constexpr (OP::READS_T) {
                        if (!q.t_other) PV<TT, V>::ld(t + base + pv, tv);
                        else {
#pragma unroll
                            for (int e = 0; e < V; ++e) tv[e] = map_target1<TT>(t, q, b, c, p0 + pv + e);
                        }
                    }
#pragma unroll
                    for (int e = 0; e < V; ++e) xv[e] = acc.elem(xv[e], OP::READS_T ? tv[e] : 0.f, h);
                    if constexpr (OP::WRITES_DX) PV<TX, V>::st(dx + base + pv, xv);
                }
            }
        }
        if constexpr (NS > 0) {
            double s[NS];
            acc.totals(s);
#pragma unroll
            for (int n = 0; n < NS; ++n) {
                double u = s[n];
                for (int o = G >> 1; o > 0; o >>= 1) u += __shfl_xor(u, o, 64);      // (G divides 64: a row's lanes share a wave)
                if (i == 0 && c < C) partials[((size_t)n * q.rows + (size_t)bg * q.nchunk + k) * C + c] = u;
            }
        }
    }
}

// x in channels_last.  grid-stride over items (images [bg BI, bg BI + BI), channel vectors [ti TW, ti TW + TW), pixels [k CHUNK,
// k CHUNK + len))
template <typename TX, typename TT, int V, typename OP>
__global__ __launch_bounds__(MAP_THREADS) void map_nhwc_kernel(const TX* __restrict__ x, const TT* __restrict__ t,
                                                               double* __restrict__ partials, const typename OP::Args v,
                                                               TX* __restrict__ dx, const MapShape q) {
    constexpr int NS = OP::NS;
    __shared__ double sh[NS ? NS : 1][NS ? V : 1][NS ? MAP_THREADS : 1];
    const int tid = threadIdx.x, TW = q.TW, RP = q.RP, tc = tid % TW, tr = tid / TW;
    const int C = q.C, P = q.P, ncv = C / V;
    for (long long it = blockIdx.x; it < q.items; it += gridDim.x) {
        const int k = (int)(it % q.nchunk);
        const long long rest = it / q.nchunk;
        const int ti = (int)(rest % q.ntile), bg = (int)(rest / q.ntile);
        const int cv = ti * TW + tc, c0 = cv * V, p0 = k * MAP_CHUNK, pe = p0 + min(MAP_CHUNK, P - p0);
        typename OP::Acc acc[V];
        int run = 0;
        if (tr < RP && cv < ncv) {
            typename OP::Ch h[V];
#pragma unroll
            for (int e = 0; e < V; ++e) h[e] = OP::ch(v, C, c0 + e);
            for (int b = bg * q.BI, be = OP::ONE_IMAGE ? b + 1 : min(q.B, b + q.BI); b < be; ++b)
                for (int p = p0 + tr; p < pe; p += RP) {
                    const size_t at = ((size_t)b * P + p) * C + c0;
                    float xv[V], tv[V];
                    PV<TX, V>::ld(x + at, xv);
                    if constexpr (OP::READS_T) {
                        if (!q.t_other) PV<TT, V>::ld(t + at, tv);
                        else {
#pragma unroll
                            for (int e = 0; e < V; ++e) tv[e] = map_target1<TT>(t, q, b, c0 + e, p);
                        }
                    }
#pragma unroll
                    for (int e = 0; e < V; ++e) xv[e] = acc[e].elem(xv[e], OP::READS_T ? tv[e] : 0.f, h[e]);
                    if constexpr (OP::WRITES_DX) PV<TX, V>::st(dx + at, xv);
                    if (++run == MAP_RUN) {
                        run = 0;
#pragma unroll
                        for (int e = 0; e < V; ++e) acc[e].cut();
                    }
                }
        }
        if constexpr (NS > 0) {
            double s[V][NS];
#pragma unroll
            for (int e = 0; e < V; ++e) acc[e].totals(s[e]);
            __syncthreads();                                                       // the sums of the previous item have been read
#pragma unroll
            for (int n = 0; n < NS; ++n)
#pragma unroll
                for (int e = 0; e < V; ++e) sh[n][e][tid] = s[e][n];
            __syncthreads();
            // one thread per (sum, element, channel vector) of the tile adds the RP pixel rows in the order of tr
            for (int j = tid; j < NS * V * TW; j += MAP_THREADS) {
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

inline int pow2_ceil_lg(long long n) {       // smallest lg with (1 << lg) >= n
    int lg = 0;
    while ((1LL << lg) < n) ++lg;
    return lg;
}

// the walk of a launch: t (nullable) is read, dx (nullable) is accessed like x; BI images share an item.  *vec: the least
// side_vec of the sides walked in vectors
inline MapShape map_shape(const void* x, const void* t, const void* dx, int B, int C, int P, int BI, int dt_x, int lay_x, int dt_t,
                          int lay_t, int* vec) {
    MapShape q{};
    q.B = B; q.C = C; q.P = P;
    const int nhwc_x = lay_x == MOMA_LAYOUT_NHWC;
    q.nhwc_t = lay_t == MOMA_LAYOUT_NHWC;
    q.t_other = t != nullptr && nhwc_x != q.nhwc_t;
    q.nchunk = (P + MAP_CHUNK - 1) / MAP_CHUNK;
    q.BI = BI;
    q.nbg = (B + BI - 1) / BI;
    const int extent = nhwc_x ? C : P;
    int V = side_vec(x, extent, dt_x);
    if (dx) V = min(V, side_vec(dx, extent, dt_x));
    if (t && !q.t_other) V = min(V, side_vec(t, extent, dt_t));
    *vec = V;
    const int vecs = (min(P, MAP_CHUNK) + V - 1) / V;                              // vectors of the longest row piece
    q.lgG = min(6, pow2_ceil_lg(vecs));
    const int R = MAP_THREADS >> q.lgG;
    q.ctiles = (C + R - 1) / R;
    const int ncv = C / V;                                                         // (channels_last: C % V == 0)
    q.TW = max(1, min(ncv, 64 / V));
    q.RP = MAP_THREADS / q.TW;
    q.ntile = (ncv + q.TW - 1) / q.TW;
    q.rows = (long long)q.nbg * q.nchunk;
    q.items = q.rows * (nhwc_x ? q.ntile : q.ctiles);
    return q;
}

// one walk under OP.  An OP that reads no t is given t = nullptr and x's dtype for it: one instantiation
template <typename OP>
hipError_t map_launch(const void* x, const void* t, double* partials, const typename OP::Args& args, void* dx, int B, int C, int P,
                      int BI, int dt_x, int lay_x, int dt_t, int lay_t, hipStream_t st) {
    if (OP::ONE_IMAGE && BI != 1) return hipErrorInvalidValue;
    int vec = 1;
    const MapShape q = map_shape(x, t, dx, B, C, P, BI, dt_x, lay_x, dt_t, lay_t, &vec);
    const unsigned grid = (unsigned)min(q.items, (long long)MAP_MAX_GRID);
    const bool nhwc_x = lay_x == MOMA_LAYOUT_NHWC;
    with_dtype(dt_x, [&](auto tx) {
        return with_dtype(dt_t, [&](auto tt) {
            using TX = typename decltype(tx)::type;
            using TT = typename decltype(tt)::type;
            with_vec<8, 8, 4, 1>(vec, [&](auto w) {
                constexpr int V = decltype(w)::value;
                if (nhwc_x)
                    hipLaunchKernelGGL((map_nhwc_kernel<TX, TT, V, OP>), dim3(grid), dim3(MAP_THREADS), 0, st, (const TX*)x,
                                       (const TT*)t, partials, args, (TX*)dx, q);
                else
                    hipLaunchKernelGGL((map_nchw_kernel<TX, TT, V, OP>), dim3(grid), dim3(MAP_THREADS), 0, st, (const TX*)x,
                                       (const TT*)t, partials, args, (TX*)dx, q);
            });
            return 0;
        });
    });
    return hipGetLastError();
}

// ---- the finalize kernels: one workgroup of MAP_FIN_THREADS ------------------------------------------------------------------
// lanes per channel: the power of two (1 .. 64) with which C channels fill the workgroup
inline int map_fin_lg(int C) { return max(0, min(6, 10 - pow2_ceil_lg(C))); }

// the L = 1 << lgL lanes of channel c add partial rows i, i + L, ... of each of the NS sums in order (MAP_FIN_BATCH requests in
// flight) and meet over the lane bits above the channel's; lane = i * cpw + cw, cpw = 64 >> lgL
template <int NS>
__device__ __forceinline__ void map_fin_sums(const double* __restrict__ partials, long long J, int C, int c, int i, int lgL, double* s) {
    const int L = 1 << lgL, cpw = 64 >> lgL;
#pragma unroll
    for (int n = 0; n < NS; ++n) {
        double u = 0.0;
        const double* pn = partials + (size_t)n * J * C;
        if (c < C)
            for (long long j0 = i; j0 < J; j0 += (long long)MAP_FIN_BATCH * L) {
                double w[MAP_FIN_BATCH];
#pragma unroll
                for (int b = 0; b < MAP_FIN_BATCH; ++b) {
                    const long long j = j0 + (long long)b * L;
                    w[b] = j < J ? pn[(size_t)j * C + c] : 0.0;
                }
#pragma unroll
                for (int b = 0; b < MAP_FIN_BATCH; ++b) u += w[b];
            }
        for (int o = 32; o >= cpw; o >>= 1) u += __shfl_xor(u, o, 64);
        s[n] = u;
    }
}

// wave w owns channels [w cpw, w cpw + cpw), then 16 cpw further, ...: body(c, s) once per channel, s its NS sums over the J rows
template <int NS, typename F>
__device__ __forceinline__ void map_fin_channels(const double* __restrict__ partials, long long J, int C, int lgL, F body) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int cpw = 64 >> lgL, cw = lane & (cpw - 1), i = lane >> (6 - lgL);
    for (int cb = w * cpw; cb < C; cb += (MAP_FIN_THREADS / 64) * cpw) {           // (wave-uniform)
        const int c = cb + cw;
        double s[NS];
        map_fin_sums<NS>(partials, J, C, c, i, lgL, s);
        if (i == 0 && c < C) body(c, s);
    }
}

// the threads' terms meet per wave, then over the 16 waves in order -> *loss = sum * scale
__device__ __forceinline__ void map_fin_loss(double term, double scale, float* __restrict__ loss) {
    __shared__ double sh[MAP_FIN_THREADS / 64];
    term = wave_sum(term);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) {
        double u = 0.0;
        for (int z = 0; z < MAP_FIN_THREADS / 64; ++z) u += sh[z];
        *loss = (float)(u * scale);
    }
}

}  // namespace moma
