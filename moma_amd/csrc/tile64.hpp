// What the small dense products on plain FMA share (srrl.hip: y W^T and e W; cc.hip: the forward product of both heads and the three
// backward products): ONE 64 x 64 tile of outputs per workgroup of 256 threads, 4 x 4 outputs per thread from LDS tiles of both
// operands, one SEGMENT of 32 elements of the reduction at a time, the next segment's 16 values per thread requested while the
// current one is multiplied.  F64 = false: plain fp32 FMA over the segment, the segment's sum then added to a DOUBLE total (gfx950
// has no xf32; 1280 channels are 40 segments).  F64 = true: multiply and add in double from the first element on (the product of two
// fp32 values is exact in double; cc.hip says why its forward needs that).  Element accesses (fp32 or bf16 per operand): no
// alignment beyond the element, no divisibility asked.  Around the product: the accumulators' zeroing, the bounds-checked walk over
// a thread's outputs, the planner that splits a reduction over about one workgroup per compute unit, and the ordered sum of an
// array by one workgroup.  One copy, so a change to the tile (the LDS strides, the request depth) is made and measured once.
// hipcc -O3, gfx950: 2 x 8448 B of LDS; F64 = false 130 .. 138 VGPRs (16 double and 16 fp32 accumulators, 16 values in flight), F64 =
// true 166 (16 double accumulators, 8 double operands of four steps, 16 values in flight): 3 waves per SIMD either way.
#pragma once
#include "common.hpp"

namespace moma {

constexpr int T64_THREADS = 256;
constexpr int T64_TILE = 64;                        // outputs of a tile per side (4 x 4 per thread)
constexpr int T64_SEG = 32;                         // elements of the reduction in one segment
constexpr int T64_LD = T64_SEG + 1, T64_LN = T64_TILE + 1;      // LDS strides of a [row][k] and of a [k][column] tile
constexpr int T64_PER = T64_TILE * T64_SEG / T64_THREADS;       // values per thread and operand in one request
constexpr int T64_LDS = T64_TILE * T64_LD;          // floats of one operand's tile (the [k][column] form is smaller)
constexpr int T64_TARGET_WG = 256;                  // workgroups a product aims at when it splits its reduction (one per compute unit)
static_assert(T64_SEG * T64_LN <= T64_LDS, "both layouts fit one tile");

// dacc[i][j] += sum over k in [kbeg, kend) of A(m0 + ty + 16 i, k) Bm(k, n0 + tx + 16 j), rows past M and columns past N read as 0:
//     A(m, k)  = AT ? A[k M + m]  : A[m Kr + k]            Bm(k, n) = BN ? Bm[k N + n] : Bm[n Kr + k]
// The tiles lie in LDS as [row][k] with a stride of 33 (the BN form of Bm as [k][n], stride 65): the 16 columns of a wave's read fall
// into 16 banks and its 4 rows are broadcasts.  As, Bs: T64_LDS floats each.
template <bool AT, bool BN, bool F64, typename TA, typename TB>
__device__ __forceinline__ void tile64(const TA* __restrict__ A, const TB* __restrict__ Bm, float* As, float* Bs, int M, int N, int Kr,
                                       int kbeg, int kend, int m0, int n0, double (&dacc)[4][4]) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    float ra[T64_PER], rb[T64_PER];
    auto request = [&](int k0) {
#pragma unroll
        for (int r = 0; r < T64_PER; ++r) {
            const int idx = tid + r * T64_THREADS;
            if constexpr (AT) {
                const int gk = k0 + idx / T64_TILE, gm = m0 + idx % T64_TILE;
                ra[r] = gk < kend && gm < M ? ld1<TA>(A + (size_t)gk * M + gm) : 0.f;
            } else {
                const int gm = m0 + idx / T64_SEG, gk = k0 + idx % T64_SEG;
                ra[r] = gm < M && gk < kend ? ld1<TA>(A + (size_t)gm * Kr + gk) : 0.f;
            }
            if constexpr (BN) {
                const int gk = k0 + idx / T64_TILE, gn = n0 + idx % T64_TILE;
                rb[r] = gk < kend && gn < N ? ld1<TB>(Bm + (size_t)gk * N + gn) : 0.f;
            } else {
                const int gn = n0 + idx / T64_SEG, gk = k0 + idx % T64_SEG;
                rb[r] = gn < N && gk < kend ? ld1<TB>(Bm + (size_t)gn * Kr + gk) : 0.f;
            }
        }
    };
    request(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += T64_SEG) {
#pragma unroll
        for (int r = 0; r < T64_PER; ++r) {
            const int idx = tid + r * T64_THREADS;
            if constexpr (AT) As[(idx % T64_TILE) * T64_LD + idx / T64_TILE] = ra[r];
            else As[(idx / T64_SEG) * T64_LD + idx % T64_SEG] = ra[r];
            if constexpr (BN) Bs[(idx / T64_TILE) * T64_LN + idx % T64_TILE] = rb[r];
            else Bs[(idx / T64_SEG) * T64_LD + idx % T64_SEG] = rb[r];
        }
        __syncthreads();
        if (k0 + T64_SEG < kend) request(k0 + T64_SEG);
        if constexpr (F64) {
#pragma unroll 4
            for (int kk = 0; kk < T64_SEG; ++kk) {
                double av[4], bv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) av[i] = (double)As[(ty + 16 * i) * T64_LD + kk];
#pragma unroll
                for (int j = 0; j < 4; ++j) bv[j] = (double)(BN ? Bs[kk * T64_LN + tx + 16 * j] : Bs[(tx + 16 * j) * T64_LD + kk]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) dacc[i][j] = fma(av[i], bv[j], dacc[i][j]);
            }
            __syncthreads();
            continue;
        }
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
#pragma unroll 8
        for (int kk = 0; kk < T64_SEG; ++kk) {
            float av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = As[(ty + 16 * i) * T64_LD + kk];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = BN ? Bs[kk * T64_LN + tx + 16 * j] : Bs[(tx + 16 * j) * T64_LD + kk];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) dacc[i][j] += (double)acc[i][j];
        __syncthreads();
    }
}

__device__ __forceinline__ void tile64_zero(double (&dacc)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) dacc[i][j] = 0.0;
}

// the epilogue: f(m, n, total) for each of the thread's 4 x 4 outputs that lies inside [M, N].  Let f capture BY VALUE: through
// reference captures of kernel arguments hipcc forms every store's address from scratch (114 more instructions in srrl's kernel)
template <typename F>
__device__ __forceinline__ void tile64_each(const double (&dacc)[4][4], int m0, int n0, int M, int N, F f) {
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + ty + 16 * i, n = n0 + tx + 16 * j;
            if (m < M && n < N) f(m, n, dacc[i][j]);
        }
}

inline int tile64_tiles(int M, int N) { return ceil_div(M, T64_TILE) * ceil_div(N, T64_TILE); }

// segments that one workgroup adds when `tiles` tiles share a reduction of `nseg` segments: all of them where the tiles alone fill
// the device.  A function of the shape alone: the workspace layouts and the order of every sum hang on it.
inline int tile64_segs(int tiles, int nseg) {
    const int want = max(1, min(nseg, T64_TARGET_WG / tiles));
    return ceil_div(nseg, want);
}

// ---- the ordered sum of an array by ONE workgroup of T64_THREADS: thread i adds terms i, i + 256, ... in order (strided_sum), then
//      thread 0 adds the 256 threads' values in order and is the one that gets the total (ordered_sum).  Two steps, so that a caller
//      can put several arrays into a thread's value first (srrl.hip's loss).
__device__ __forceinline__ double strided_sum(const double* __restrict__ v, int n) {
    double u = 0.0;
    for (int i = threadIdx.x; i < n; i += T64_THREADS) u += v[i];
    return u;
}
__device__ __forceinline__ double ordered_sum(double u) {
    __shared__ double ls[T64_THREADS];
    ls[threadIdx.x] = u;
    __syncthreads();
    double w = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < T64_THREADS; ++i) w += ls[i];
    return w;
}

}  // namespace moma
