// Probabilistic Knowledge Transfer (`--distill pkt`; reference distiller_zoo/PKT.py, helper/loops_moma.py:159-162) on feat[-1] of both
// networks, student X [B, Ds], teacher Y [B, Dt], eps = 1e-7.  Everything is a function of the two raw B x B Gram matrices; per side
//     G = F F^T   n_i = sqrt(G_ii)   C_ij = G_ij / ((n_i + eps)(n_j + eps))   K = (C + 1) / 2   r_i = sum_j K_ij   P_ij = K_ij / r_i
//     loss = (1/B^2) sum_ij T_ij log((T_ij + eps) / (P_ij + eps))                       (P from the student, T from the teacher)
//     U_ij = -(1/B^2) T_ij / (P_ij + eps)   s_i = sum_k U_ik P_ik   W_ij = (U_ij - s_i) / (2 r_i) = d loss / d C^s_ij (entries independent)
//     M = W + W^T   c_i = sum_j M_ij C^s_ij   M'_ij = M_ij / ((n_i + eps)(n_j + eps)) - [i = j] c_i / (n_i (n_i + eps))   dX = g M' X
// The diagonal term is 0 where n_i = 0: an all-zero student row gets the derivative of x / (|x| + eps) at 0 (the reference's autograd
// returns NaN for that row).  No normalised copy of X or Y exists.  All arithmetic in double; fp32 / bf16 inputs are exact once widened.
// Forward: three launches (pkt_gram_pair, pkt_rows, pkt_m; four where the caller asks for one pkt_gram per side); backward: one (pkt_bwd).
//   pkt_gram   grid (nt, nt), nt = ceil(B / 16) for one side; pkt_gram_pair: grid (nt, nt, 2), the side in blockIdx.z (the sides may
//              differ in D and dtype: four instantiations) -- the same device function, the same bits.
//              The workgroups with ti <= tj each own one 16 x 16 tile of G on v_mfma_f64_16x16x4_f64
//              and write every entry together with its mirror image from the same value (inside the diagonal tile the entries with
//              i <= j): G is symmetric bit for bit, its diagonal is n^2.  D streams through LDS in slabs of 128 columns of both row
//              tiles (double, row stride 129, zero past B and past D); wave w takes columns 32 w .. 32 w + 31 of every slab in 8 MFMA
//              steps; the four waves' tiles meet in LDS in the order 0, 1, 2, 3.  16-byte loads where the base address and D allow,
//              element loads otherwise.
//              hipcc -O3, gfx950: pkt_gram 36 VGPRs (fp32) / 40 (bf16), pkt_gram_pair 36 (both fp32) / 38 (any bf16), each + 8 AGPRs
//              (the accumulator), no spill, no scratch; LDS 41216 B (32.3 KB slabs + 8 KB partial tiles), three waves per SIMD.
//   pkt_rows   grid B: row i of both sides -- n (the diagonal of G is read, not recomputed), C, K, r, P, T; the row's KL sum into the
//              workspace; U, s_i and W[i, :] into the workspace; n^s_i into the workspace.  A thread owns columns t, t + 256, ...
//              (at most 4), every row sum is the fixed tree of the workgroup.
//              hipcc -O3, gfx950: 55 VGPRs, no AGPRs, no spill, no scratch; LDS 32 B.
//   pkt_m      grid (nt, nt): tile (ti, tj) of M' from W_ij, W_ji (the transposed tile through LDS) and the norms; both positions of
//              a pair take the same two operands, so M' is symmetric bit for bit.  c_i needs column i of W, i.e. every row's s and r:
//              it is computed HERE, by the diagonal tiles, for their 16 rows (16 threads per row over j in order, their sums added in
//              order) before the diagonal entry is written -- not in pkt_rows, and not in a launch of its own.  Workgroup (0, 0) also
//              adds the B row sums of the KL terms in a fixed order and writes the loss.
//              hipcc -O3, gfx950: 30 VGPRs, no AGPRs, no spill, no scratch; LDS 4256 B (2.1 KB tile + 2 KB sums + 32 B).
//   pkt_bwd    grid (ceil(D / 64), ceil(B / 32)): dX[32 rows, 64 columns] = g M' X on v_mfma_f64_16x16x4_f64 (wave w owns columns
//              16 w .. 16 w + 15, two accumulators of 4 doubles); j streams in slabs of 16.  No mean subtraction (the difference from
//              rkd_bwd).  g is read from device memory and folded in before the one rounding double -> fp32 (-> bf16 in a second
//              step: a bf16 dF_s is the fp32 dF_s rounded once, bit for bit).
//              hipcc -O3, gfx950: 42 VGPRs + 16 AGPRs (the accumulators), no spill, no scratch; LDS 14592 B (4.3 KB M' + 10 KB X).
// None of the launches spills or uses scratch (the compiler's kernel-resource-usage report).
// No atomics: every sum has an order that depends on the shapes alone -- bitwise repeatable.
#include "common.hpp"

namespace moma {
namespace {

typedef __attribute__((ext_vector_type(4))) double f64x4;

constexpr int PKT_THREADS = 256;
constexpr int PKT_T = 16;                    // rows / columns of a tile of G and of M'
constexpr int PKT_KD = 128;                  // columns of one pkt_gram slab
constexpr int PKT_LDD = PKT_KD + 1;          // its row stride (doubles)
constexpr int PKT_RJ = MOMA_PKT_MAX_B / PKT_THREADS;      // columns a pkt_rows thread owns at most
constexpr int PKT_BR = 32, PKT_BC = 64;      // rows / columns of one pkt_bwd workgroup
constexpr int PKT_BJ = 16;                   // its slab of the summation index
constexpr int PKT_LDM = PKT_BJ + 1;          // row stride of the M' slab (doubles)
constexpr int PKT_LDX = PKT_BC + 16;         // row stride of the X slab: two consecutive k rows in disjoint halves of the banks
constexpr double PKT_EPS = 1e-7;             // the reference's single constant

// sum over the workgroup in a fixed order (butterfly inside a wave, then waves 0, 1, 2, 3), the result in every thread
__device__ __forceinline__ double pkt_block_sum(double v, double* sh) {
    v = wave_sum(v);
    __syncthreads();                                              // (sh may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// rows [r0, r0 + 16) x columns [k0, k0 + 128) of f [B, D] -> lds[r * PKT_LDD + kk] as double; zero past B and past D.
// vec: D is a multiple of the vector width and the base is 16-byte aligned (k0 is a multiple of 128)
template <typename T>
__device__ __forceinline__ void pkt_stage(const T* __restrict__ f, int B, int D, int vec, int r0, long long k0, double* __restrict__ lds) {
    constexpr int V = MAXVEC<T>, VPR = PKT_KD / V;             // vectors per row of the slab
    const int tid = threadIdx.x;
    if (vec) {
        for (int idx = tid; idx < PKT_T * VPR; idx += PKT_THREADS) {
            const int r = idx / VPR, kv = idx % VPR, row = r0 + r;
            const long long k = k0 + kv * V;
            float v[V];
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = 0.f;
            if (row < B && k < D) PV<T, V>::ld(f + (size_t)row * D + k, v);          // (D % V == 0: all V inside)
            double* o = lds + r * PKT_LDD + kv * V;
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = (double)v[e];
        }
    } else {
        for (int idx = tid; idx < PKT_T * PKT_KD; idx += PKT_THREADS) {
            const int r = idx / PKT_KD, kk = idx % PKT_KD, row = r0 + r;
            const long long k = k0 + kk;
            lds[r * PKT_LDD + kk] = (row < B && k < D) ? (double)ld1<T>(f + (size_t)row * D + k) : 0.0;
        }
    }
}

// one tile (ti = blockIdx.y, tj = blockIdx.x), ti <= tj, of one side's G: THE body of both Gram kernels, so a side's bits do not
// depend on which of them computed it
template <typename T>
__device__ __forceinline__ void pkt_gram_tile(const T* __restrict__ f, double* __restrict__ G, int B, int D, int vec,
                                              double* __restrict__ Xi, double* __restrict__ Xj, double (*part)[PKT_T * PKT_T]) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;                                          // (uniform: before any barrier)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const double* xj_tile = ti == tj ? Xi : Xj;                   // the diagonal tile stages its rows once
    f64x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = 0.0;
    for (long long k0 = 0; k0 < D; k0 += PKT_KD) {
        __syncthreads();                                          // the slab of the previous turn has been read
        pkt_stage<T>(f, B, D, vec, ti * PKT_T, k0, Xi);
        if (ti != tj) pkt_stage<T>(f, B, D, vec, tj * PKT_T, k0, Xj);
        __syncthreads();
        const double* xi = Xi + l15 * PKT_LDD + 32 * w + l4;      // A: row l15 of the tile's rows, k = lane >> 4
        const double* xj = xj_tile + l15 * PKT_LDD + 32 * w + l4; // B: row l15 of the tile's columns, k = lane >> 4
#pragma unroll
        for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xi[4 * s], xj[4 * s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) part[w][(l4 + 4 * r) * PKT_T + l15] = acc[r];      // C/D layout: row = (lane >> 4) + 4 reg, col = lane & 15
    __syncthreads();
    const double s = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    const int li = tid >> 4, lj = tid & 15;
    const int i = ti * PKT_T + li, j = tj * PKT_T + lj;
    if (i < B && j < B && (ti != tj || li <= lj)) {
        G[(size_t)i * B + j] = s;
        if (i != j) G[(size_t)j * B + i] = s;
    }
}

// grid (nt, nt): one side
template <typename T>
__global__ __launch_bounds__(PKT_THREADS) void pkt_gram_kernel(const T* __restrict__ f, double* __restrict__ G, int B, int D, int vec) {
    __shared__ double Xi[PKT_T * PKT_LDD], Xj[PKT_T * PKT_LDD];
    __shared__ double part[4][PKT_T * PKT_T];
    pkt_gram_tile<T>(f, G, B, D, vec, Xi, Xj, part);
}

// grid (nt, nt, 2): both sides in one launch, the side in blockIdx.z (uniform per workgroup)
template <typename TS, typename TT>
__global__ __launch_bounds__(PKT_THREADS) void pkt_gram_pair_kernel(const TS* __restrict__ fs, const TT* __restrict__ ft,
                                                                    double* __restrict__ Gs, double* __restrict__ Gt, int B, int Ds,
                                                                    int Dt, int vec_s, int vec_t) {
    __shared__ double Xi[PKT_T * PKT_LDD], Xj[PKT_T * PKT_LDD];
    __shared__ double part[4][PKT_T * PKT_T];
    if (blockIdx.z == 0) pkt_gram_tile<TS>(fs, Gs, B, Ds, vec_s, Xi, Xj, part);
    else pkt_gram_tile<TT>(ft, Gt, B, Dt, vec_t, Xi, Xj, part);
}

__device__ __forceinline__ double pkt_norm(const double* __restrict__ G, int B, int i) { return sqrt(G[(size_t)i * B + i]); }

// grid B: row i -> W[i, :], kl[i], ns[i]
__global__ __launch_bounds__(PKT_THREADS) void pkt_rows_kernel(const double* __restrict__ Gs, const double* __restrict__ Gt,
                                                               double* __restrict__ W, double* __restrict__ kl,
                                                               double* __restrict__ ns, int B) {
    __shared__ double sh[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const double inv_b2 = 1.0 / ((double)B * B);
    const double ni_s = pkt_norm(Gs, B, i), ni_t = pkt_norm(Gt, B, i);
    double ks[PKT_RJ], kt[PKT_RJ];
    double rs = 0.0, rt = 0.0;
#pragma unroll
    for (int q = 0; q < PKT_RJ; ++q) {
        const int j = tid + q * PKT_THREADS;
        ks[q] = kt[q] = 0.0;
        if (j < B) {
            const double cs = Gs[(size_t)i * B + j] / ((ni_s + PKT_EPS) * (pkt_norm(Gs, B, j) + PKT_EPS));
            const double ct = Gt[(size_t)i * B + j] / ((ni_t + PKT_EPS) * (pkt_norm(Gt, B, j) + PKT_EPS));
            ks[q] = (cs + 1.0) * 0.5;
            kt[q] = (ct + 1.0) * 0.5;
            rs += ks[q];
            rt += kt[q];
        }
    }
    rs = pkt_block_sum(rs, sh);
    rt = pkt_block_sum(rt, sh);
    double l = 0.0, s = 0.0;
#pragma unroll
    for (int q = 0; q < PKT_RJ; ++q) {
        const int j = tid + q * PKT_THREADS;
        if (j < B) {
            const double p = ks[q] / rs, t = kt[q] / rt;
            const double u = -inv_b2 * t / (p + PKT_EPS);
            l += t * log((t + PKT_EPS) / (p + PKT_EPS));
            s += u * p;
            ks[q] = u;                                            // (K_s is not needed again)
        }
    }
    l = pkt_block_sum(l, sh);
    s = pkt_block_sum(s, sh);
#pragma unroll
    for (int q = 0; q < PKT_RJ; ++q) {
        const int j = tid + q * PKT_THREADS;
        if (j < B) W[(size_t)i * B + j] = (ks[q] - s) / (2.0 * rs);
    }
    if (tid == 0) { kl[i] = l; ns[i] = ni_s; }
}

// grid (nt, nt): rows i of tile blockIdx.y, columns j of tile blockIdx.x
__global__ __launch_bounds__(PKT_THREADS) void pkt_m_kernel(const double* __restrict__ Gs, const double* __restrict__ W,
                                                            const double* __restrict__ kl, const double* __restrict__ ns,
                                                            double* __restrict__ M, float* __restrict__ loss, int B) {
    __shared__ double Wt[PKT_T][PKT_T + 1];                       // the tile (tj, ti) of W: Wt[lj][li] = W[j, i]
    __shared__ double red[PKT_T][PKT_T];
    __shared__ double sh[4];
    const int tid = threadIdx.x, li = tid >> 4, lj = tid & 15;
    const int i0 = blockIdx.y * PKT_T, j0 = blockIdx.x * PKT_T, i = i0 + li, j = j0 + lj;
    {
        const int r = j0 + li, c = i0 + lj;                       // row li of the transposed tile, read along its rows
        Wt[li][lj] = (r < B && c < B) ? W[(size_t)r * B + c] : 0.0;
    }
    double c_i = 0.0;
    if (i0 == j0) {
        // c_r = sum_j (W_rj + W_jr) C_rj for the 16 rows of this diagonal tile: thread (t, r) adds j = t, t + 16, ... in order
        const int r = i0 + lj, t = li;
        double s = 0.0;
        if (r < B) {
            const double nr = ns[r] + PKT_EPS;
            for (int jj = t; jj < B; jj += PKT_T) {
                const double m = W[(size_t)r * B + jj] + W[(size_t)jj * B + r];
                s += m * (Gs[(size_t)r * B + jj] / (nr * (ns[jj] + PKT_EPS)));
            }
        }
        red[t][lj] = s;
    }
    __syncthreads();
    if (i0 == j0) {
        for (int t = 0; t < PKT_T; ++t) c_i += red[t][li];        // (row li of the tile: every thread of the row, same order)
    }
    if (i < B && j < B) {
        const double n_i = ns[i], n_j = ns[j];
        const double m = W[(size_t)i * B + j] + Wt[lj][li];
        double v = m / ((n_i + PKT_EPS) * (n_j + PKT_EPS));
        if (i == j && n_i > 0.0) v -= c_i / (n_i * (n_i + PKT_EPS));
        M[(size_t)i * B + j] = v;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0) {                     // (uniform)
        double s = 0.0;
        for (int k = tid; k < B; k += PKT_THREADS) s += kl[k];
        s = pkt_block_sum(s, sh);
        if (tid == 0) *loss = (float)(s / ((double)B * B));
    }
}

// grid (ceil(D / 64), ceil(B / 32)): rows [32 by, +32) x columns [64 bx, +64) of dX
template <typename T>
__global__ __launch_bounds__(PKT_THREADS) void pkt_bwd_kernel(const T* __restrict__ X, const double* __restrict__ M,
                                                              const float* __restrict__ g_loss, T* __restrict__ dX, int B, int D) {
    __shared__ double Ml[PKT_BR * PKT_LDM];
    __shared__ double Xl[PKT_BJ * PKT_LDX];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int i0 = blockIdx.y * PKT_BR;
    const size_t d0 = (size_t)blockIdx.x * PKT_BC;
    f64x4 acc[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[rt][r] = 0.0;
    for (int j0 = 0; j0 < B; j0 += PKT_BJ) {
        __syncthreads();                                          // the slab of the previous turn has been read
        for (int idx = tid; idx < PKT_BR * PKT_BJ; idx += PKT_THREADS) {
            const int r = idx >> 4, jj = idx & 15, i = i0 + r, j = j0 + jj;
            Ml[r * PKT_LDM + jj] = (i < B && j < B) ? M[(size_t)i * B + j] : 0.0;
        }
        for (int idx = tid; idx < PKT_BJ * PKT_BC; idx += PKT_THREADS) {
            const int jj = idx >> 6, c = idx & 63, j = j0 + jj;
            Xl[jj * PKT_LDX + c] = (j < B && d0 + c < (size_t)D) ? (double)ld1<T>(X + (size_t)j * D + d0 + c) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < PKT_BJ / 4; ++s) {
            const int k = 4 * s + l4;
            const double bv = Xl[k * PKT_LDX + 16 * w + l15];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
                acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ml[(16 * rt + l15) * PKT_LDM + k], bv, acc[rt], 0, 0, 0);
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

int pkt_tiles(int B) { return (B + PKT_T - 1) / PKT_T; }

}  // namespace

// workspace (doubles): W [B, B], kl [B], ns [B]
size_t pkt_workspace_bytes(int B) { return ((size_t)B * B + 2 * (size_t)B) * sizeof(double); }

hipError_t launch_pkt_gram(const void* f, int B, long long D, int dtype, double* G, hipStream_t st) {
    const int nt = pkt_tiles(B);
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const int vec = pick_vec(D, sizeof(T), (uintptr_t)f, {MAXVEC<T>}) > 1;      // 16 bytes or nothing
        hipLaunchKernelGGL(pkt_gram_kernel<T>, dim3(nt, nt), dim3(PKT_THREADS), 0, st, (const T*)f, G, B, (int)D, vec);
        return hipGetLastError();
    });
}

hipError_t launch_pkt_gram_pair(const void* f_s, long long Ds, int dt_s, const void* f_t, long long Dt, int dt_t, int B, double* G_s,
                                double* G_t, hipStream_t st) {
    const int nt = pkt_tiles(B);
    return with_dtype(dt_s, [&](auto a) {
        return with_dtype(dt_t, [&](auto b) {
            using TS = typename decltype(a)::type;
            using TT = typename decltype(b)::type;
            const int vec_s = pick_vec(Ds, sizeof(TS), (uintptr_t)f_s, {MAXVEC<TS>}) > 1;
            const int vec_t = pick_vec(Dt, sizeof(TT), (uintptr_t)f_t, {MAXVEC<TT>}) > 1;
            hipLaunchKernelGGL((pkt_gram_pair_kernel<TS, TT>), dim3(nt, nt, 2), dim3(PKT_THREADS), 0, st, (const TS*)f_s, (const TT*)f_t,
                               G_s, G_t, B, (int)Ds, (int)Dt, vec_s, vec_t);
            return hipGetLastError();
        });
    });
}

hipError_t launch_pkt_terms(const double* G_s, const double* G_t, int B, void* ws, double* M, float* loss, hipStream_t st) {
    const int nt = pkt_tiles(B);
    double* W = (double*)ws;
    double *kl = W + (size_t)B * B, *ns = kl + B;
    hipLaunchKernelGGL(pkt_rows_kernel, dim3(B), dim3(PKT_THREADS), 0, st, G_s, G_t, W, kl, ns, B);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pkt_m_kernel, dim3(nt, nt), dim3(PKT_THREADS), 0, st, G_s, (const double*)W, (const double*)kl, (const double*)ns,
                       M, loss, B);
    return hipGetLastError();
}

hipError_t launch_pkt_bwd(const void* f_s, const double* M, const float* g_loss, void* dF, int B, long long D, int dtype,
                          hipStream_t st) {
    const dim3 grid((unsigned)((D + PKT_BC - 1) / PKT_BC), (unsigned)((B + PKT_BR - 1) / PKT_BR));
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(pkt_bwd_kernel<T>, grid, dim3(PKT_THREADS), 0, st, (const T*)f_s, M, g_loss, (T*)dF, B, (int)D);
        return hipGetLastError();
    });
}

}  // namespace moma
