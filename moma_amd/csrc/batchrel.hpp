// What the losses on a B x B batch relation share (rkd.hip, pkt.hip, sp.hip): the fixed-order sums of a workgroup, and for rkd and pkt
// the staging of a slab of f [B, D] as double and the backward dX = g M X' on v_mfma_f64_16x16x4_f64.  All of it assumes workgroups
// of REL_THREADS = 256 threads (four waves).
#pragma once
#include "common.hpp"

namespace moma {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int REL_THREADS = 256;
constexpr int REL_T = 16;                    // rows / columns of a tile of a B x B matrix
constexpr int REL_KD = 128;                  // columns of one staged slab of f
constexpr int REL_LDD = REL_KD + 1;          // its row stride (doubles): the 8 columns of a wave's lanes in disjoint banks
constexpr int REL_BR = 32, REL_BC = 64;      // rows / columns of dX of one rel_bwd workgroup
constexpr int REL_BJ = 16;                   // its slab of the summation index
constexpr int REL_LDM = REL_BJ + 1;          // row stride of the M slab (doubles)
constexpr int REL_LDX = REL_BC + 16;         // row stride of the X slab: two consecutive k rows in disjoint halves of the banks

// sum over the workgroup in a fixed order (butterfly inside a wave, then waves 0, 1, 2, 3), the result in every thread.
// Not the block sums of attention.hip ((s0 + s1) + (s2 + s3)), crd.hip (an LDS tree) or bnse.hip (DPP): those give other bits.
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    __syncthreads();                                              // (sh may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
// sum of n doubles: thread t adds entries t, t + 256, ... in order, then the fixed tree
__device__ __forceinline__ double array_sum(const double* __restrict__ a, int n, double* sh) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += REL_THREADS) s += a[i];
    return block_sum(s, sh);
}

// rows [r0, r0 + 16) x columns [k0, k0 + 128) of f [B, D] -> lds[r * REL_LDD + kk] as double; zero past B and past D.
// vec: D is a multiple of the vector width and the base is 16-byte aligned (k0 is a multiple of 128)
template <typename T>
__device__ __forceinline__ void rel_stage(const T* __restrict__ f, int B, int D, int vec, int r0, long long k0, double* __restrict__ lds) {
    constexpr int V = MAXVEC<T>, VPR = REL_KD / V;             // vectors per row of the slab
    const int tid = threadIdx.x;
    if (vec) {
        for (int idx = tid; idx < REL_T * VPR; idx += REL_THREADS) {
            const int r = idx / VPR, kv = idx % VPR, row = r0 + r;
            const long long k = k0 + kv * V;
            float v[V];
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = 0.f;
            if (row < B && k < D) PV<T, V>::ld(f + (size_t)row * D + k, v);          // (D % V == 0: all V inside)
            double* o = lds + r * REL_LDD + kv * V;
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = (double)v[e];
        }
    } else {
        for (int idx = tid; idx < REL_T * REL_KD; idx += REL_THREADS) {
            const int r = idx / REL_KD, kk = idx % REL_KD, row = r0 + r;
            const long long k = k0 + kk;
            lds[r * REL_LDD + kk] = (row < B && k < D) ? (double)ld1<T>(f + (size_t)row * D + k) : 0.0;
        }
    }
}

// grid (ceil(D / 64), ceil(B / 32)): rows [32 by, +32) x columns [64 bx, +64) of dX = g M X' on v_mfma_f64_16x16x4_f64.  Wave w owns
// columns 16 w .. 16 w + 15 (two accumulators of 4 doubles); j streams in slabs of 16 through Ml [REL_BR * REL_LDM] and Xl
// [REL_BJ * REL_LDX].  m_of(i, j, r) is M_ij for i, j < B (r = i - 32 by), x_of(x, c) is X'_jc from the widened X_jc (c = column in the
// block).  The first barrier comes before any use of the callables: what the caller wrote to LDS in front of the call is visible.
// g is read from device memory and folded in before the one rounding double -> fp32 (-> bf16 in a second step).
// pkt_bwd is this call.  rkd_bwd carries the same body written out behind its prologue (rkd.hip says why): change both.
template <typename T, typename MOf, typename XOf>
__device__ __forceinline__ void rel_bwd(const T* __restrict__ X, const float* __restrict__ g_loss, T* __restrict__ dX, int B, int D,
                                        double* __restrict__ Ml, double* __restrict__ Xl, MOf m_of, XOf x_of) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int i0 = blockIdx.y * REL_BR;
    const size_t d0 = (size_t)blockIdx.x * REL_BC;
    f64x4 acc[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[rt][r] = 0.0;
    for (int j0 = 0; j0 < B; j0 += REL_BJ) {
        __syncthreads();                                          // the slab of the previous turn has been read
        for (int idx = tid; idx < REL_BR * REL_BJ; idx += REL_THREADS) {
            const int r = idx >> 4, jj = idx & 15, i = i0 + r, j = j0 + jj;
            Ml[r * REL_LDM + jj] = (i < B && j < B) ? m_of(i, j, r) : 0.0;
        }
        for (int idx = tid; idx < REL_BJ * REL_BC; idx += REL_THREADS) {
            const int jj = idx >> 6, c = idx & 63, j = j0 + jj;
            Xl[jj * REL_LDX + c] = (j < B && d0 + c < (size_t)D) ? x_of((double)ld1<T>(X + (size_t)j * D + d0 + c), c) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < REL_BJ / 4; ++s) {
            const int k = 4 * s + l4;
            const double bv = Xl[k * REL_LDX + 16 * w + l15];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
                acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ml[(16 * rt + l15) * REL_LDM + k], bv, acc[rt], 0, 0, 0);
        }
    }
    const double g = (double)*g_loss;
    const size_t c = d0 + 16 * w + l15;
    if (c >= (size_t)D) return;                                   // (no barrier below)
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 16 * rt + l4 + 4 * r;              // C/D layout of the f64 MFMA: row = (lane >> 4) + 4 reg
            if (i < B) st1<T>(dX + (size_t)i * D + c, round_f32(g * acc[rt][r]));
        }
}

}  // namespace moma
