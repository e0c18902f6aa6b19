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
//              tiles (rel_stage of batchrel.hpp, shared with rkd_dist); wave w takes columns 32 w .. 32 w + 31 of every slab in 8 MFMA
//              steps; the four waves' tiles meet in LDS in the order 0, 1, 2, 3.
//              hipcc -O3, gfx950: pkt_gram 36 VGPRs (fp32) / 40 (bf16), pkt_gram_pair 36 (both fp32) / 38 (any bf16), each + 8 AGPRs
//              (the accumulator), no spill, no scratch; LDS 41216 B (32.3 KB slabs + 8 KB partial tiles), three waves per SIMD.
//   pkt_rows   grid B: row i of both sides -- n (the diagonal of G is read, not recomputed), C, K, r, P, T; the row's KL sum into the
//              workspace; U, s_i and W[i, :] into the workspace; n^s_i into the workspace.  A thread owns columns t, t + 256, ...
//              (at most 4), every row sum is the fixed tree of the workgroup (block_sum of batchrel.hpp).
//              hipcc -O3, gfx950: 55 VGPRs, no AGPRs, no spill, no scratch; LDS 32 B.
//   pkt_m      grid (nt, nt): tile (ti, tj) of M' from W_ij, W_ji (the transposed tile through LDS) and the norms; both positions of
//              a pair take the same two operands, so M' is symmetric bit for bit.  c_i needs column i of W, i.e. every row's s and r:
//              it is computed HERE, by the diagonal tiles, for their 16 rows (16 threads per row over j in order, their sums added in
//              order) before the diagonal entry is written -- not in pkt_rows, and not in a launch of its own.  Workgroup (0, 0) also
//              adds the B row sums of the KL terms in a fixed order and writes the loss.
//              hipcc -O3, gfx950: 30 VGPRs, no AGPRs, no spill, no scratch; LDS 4256 B (2.1 KB tile + 2 KB sums + 32 B).
//   pkt_bwd    grid (ceil(D / 64), ceil(B / 32)): dX[32 rows, 64 columns] = g M' X, rel_bwd of batchrel.hpp (shared with rkd_bwd) with
//              M' read as it is and X taken as it is (no mean subtraction: the difference from rkd_bwd).  A bf16 dF_s is the fp32
//              dF_s rounded once, bit for bit.
//              hipcc -O3, gfx950: 42 VGPRs + 16 AGPRs (the accumulators), no spill, no scratch; LDS 14592 B (4.3 KB M' + 10 KB X).
// None of the launches spills or uses scratch (the compiler's kernel-resource-usage report).
// No atomics: every sum has an order that depends on the shapes alone -- bitwise repeatable.
#include "batchrel.hpp"

namespace moma {
namespace {

constexpr int PKT_RJ = MOMA_PKT_MAX_B / REL_THREADS;      // columns a pkt_rows thread owns at most
constexpr double PKT_EPS = 1e-7;             // the reference's single constant

// one tile (ti = blockIdx.y, tj = blockIdx.x), ti <= tj, of one side's G: THE body of both Gram kernels, so a side's bits do not
// depend on which of them computed it
template <typename T>
__device__ __forceinline__ void pkt_gram_tile(const T* __restrict__ f, double* __restrict__ G, int B, int D, int vec,
                                              double* __restrict__ Xi, double* __restrict__ Xj, double (*part)[REL_T * REL_T]) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;                                          // (uniform: before any barrier)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const double* xj_tile = ti == tj ? Xi : Xj;                   // the diagonal tile stages its rows once
    f64x4 acc;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = 0.0;
    for (long long k0 = 0; k0 < D; k0 += REL_KD) {
        __syncthreads();                                          // the slab of the previous turn has been read
        rel_stage<T>(f, B, D, vec, ti * REL_T, k0, Xi);
        if (ti != tj) rel_stage<T>(f, B, D, vec, tj * REL_T, k0, Xj);
        __syncthreads();
        const double* xi = Xi + l15 * REL_LDD + 32 * w + l4;      // A: row l15 of the tile's rows, k = lane >> 4
        const double* xj = xj_tile + l15 * REL_LDD + 32 * w + l4; // B: row l15 of the tile's columns, k = lane >> 4
#pragma unroll
        for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xi[4 * s], xj[4 * s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) part[w][(l4 + 4 * r) * REL_T + l15] = acc[r];      // C/D layout: row = (lane >> 4) + 4 reg, col = lane & 15
    __syncthreads();
    const double s = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    const int li = tid >> 4, lj = tid & 15;
    const int i = ti * REL_T + li, j = tj * REL_T + lj;
    if (i < B && j < B && (ti != tj || li <= lj)) {
        G[(size_t)i * B + j] = s;
        if (i != j) G[(size_t)j * B + i] = s;
    }
}

// grid (nt, nt): one side
template <typename T>
__global__ __launch_bounds__(REL_THREADS) void pkt_gram_kernel(const T* __restrict__ f, double* __restrict__ G, int B, int D, int vec) {
    __shared__ double Xi[REL_T * REL_LDD], Xj[REL_T * REL_LDD];
    __shared__ double part[4][REL_T * REL_T];
    pkt_gram_tile<T>(f, G, B, D, vec, Xi, Xj, part);
}

// grid (nt, nt, 2): both sides in one launch, the side in blockIdx.z (uniform per workgroup)
template <typename TS, typename TT>
__global__ __launch_bounds__(REL_THREADS) void pkt_gram_pair_kernel(const TS* __restrict__ fs, const TT* __restrict__ ft,
                                                                    double* __restrict__ Gs, double* __restrict__ Gt, int B, int Ds,
                                                                    int Dt, int vec_s, int vec_t) {
    __shared__ double Xi[REL_T * REL_LDD], Xj[REL_T * REL_LDD];
    __shared__ double part[4][REL_T * REL_T];
    if (blockIdx.z == 0) pkt_gram_tile<TS>(fs, Gs, B, Ds, vec_s, Xi, Xj, part);
    else pkt_gram_tile<TT>(ft, Gt, B, Dt, vec_t, Xi, Xj, part);
}

__device__ __forceinline__ double pkt_norm(const double* __restrict__ G, int B, int i) { return sqrt(G[(size_t)i * B + i]); }

// grid B: row i -> W[i, :], kl[i], ns[i]
__global__ __launch_bounds__(REL_THREADS) void pkt_rows_kernel(const double* __restrict__ Gs, const double* __restrict__ Gt,
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
        const int j = tid + q * REL_THREADS;
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
    rs = block_sum(rs, sh);
    rt = block_sum(rt, sh);
    double l = 0.0, s = 0.0;
#pragma unroll
    for (int q = 0; q < PKT_RJ; ++q) {
        const int j = tid + q * REL_THREADS;
        if (j < B) {
            const double p = ks[q] / rs, t = kt[q] / rt;
            const double u = -inv_b2 * t / (p + PKT_EPS);
            l += t * log((t + PKT_EPS) / (p + PKT_EPS));
            s += u * p;
            ks[q] = u;                                            // (K_s is not needed again)
        }
    }
    l = block_sum(l, sh);
    s = block_sum(s, sh);
#pragma unroll
    for (int q = 0; q < PKT_RJ; ++q) {
        const int j = tid + q * REL_THREADS;
        if (j < B) W[(size_t)i * B + j] = (ks[q] - s) / (2.0 * rs);
    }
    if (tid == 0) { kl[i] = l; ns[i] = ni_s; }
}

// grid (nt, nt): rows i of tile blockIdx.y, columns j of tile blockIdx.x
__global__ __launch_bounds__(REL_THREADS) void pkt_m_kernel(const double* __restrict__ Gs, const double* __restrict__ W,
                                                            const double* __restrict__ kl, const double* __restrict__ ns,
                                                            double* __restrict__ M, float* __restrict__ loss, int B) {
    __shared__ double Wt[REL_T][REL_T + 1];                       // the tile (tj, ti) of W: Wt[lj][li] = W[j, i]
    __shared__ double red[REL_T][REL_T];
    __shared__ double sh[4];
    const int tid = threadIdx.x, li = tid >> 4, lj = tid & 15;
    const int i0 = blockIdx.y * REL_T, j0 = blockIdx.x * REL_T, i = i0 + li, j = j0 + lj;
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
            for (int jj = t; jj < B; jj += REL_T) {
                const double m = W[(size_t)r * B + jj] + W[(size_t)jj * B + r];
                s += m * (Gs[(size_t)r * B + jj] / (nr * (ns[jj] + PKT_EPS)));
            }
        }
        red[t][lj] = s;
    }
    __syncthreads();
    if (i0 == j0) {
        for (int t = 0; t < REL_T; ++t) c_i += red[t][li];        // (row li of the tile: every thread of the row, same order)
    }
    if (i < B && j < B) {
        const double n_i = ns[i], n_j = ns[j];
        const double m = W[(size_t)i * B + j] + Wt[lj][li];
        double v = m / ((n_i + PKT_EPS) * (n_j + PKT_EPS));
        if (i == j && n_i > 0.0) v -= c_i / (n_i * (n_i + PKT_EPS));
        M[(size_t)i * B + j] = v;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0) {                     // (uniform)
        const double s = array_sum(kl, B, sh);
        if (tid == 0) *loss = (float)(s / ((double)B * B));
    }
}

// grid (ceil(D / 64), ceil(B / 32)): rows [32 by, +32) x columns [64 bx, +64) of dX
template <typename T>
__global__ __launch_bounds__(REL_THREADS) void pkt_bwd_kernel(const T* __restrict__ X, const double* __restrict__ M,
                                                              const float* __restrict__ g_loss, T* __restrict__ dX, int B, int D) {
    __shared__ double Ml[REL_BR * REL_LDM];
    __shared__ double Xl[REL_BJ * REL_LDX];
    rel_bwd<T>(X, g_loss, dX, B, D, Ml, Xl, [=](int i, int j, int) { return M[(size_t)i * B + j]; },
               [](double x, int) { return x; });
}

int pkt_tiles(int B) { return (B + REL_T - 1) / REL_T; }

}  // namespace

// workspace (doubles): W [B, B], kl [B], ns [B]
size_t pkt_workspace_bytes(int B) { return ((size_t)B * B + 2 * (size_t)B) * sizeof(double); }

hipError_t launch_pkt_gram(const void* f, int B, long long D, int dtype, double* G, hipStream_t st) {
    const int nt = pkt_tiles(B);
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const int vec = pick_vec(D, sizeof(T), (uintptr_t)f, {MAXVEC<T>}) > 1;      // 16 bytes or nothing
        hipLaunchKernelGGL(pkt_gram_kernel<T>, dim3(nt, nt), dim3(REL_THREADS), 0, st, (const T*)f, G, B, (int)D, vec);
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
            hipLaunchKernelGGL((pkt_gram_pair_kernel<TS, TT>), dim3(nt, nt, 2), dim3(REL_THREADS), 0, st, (const TS*)f_s, (const TT*)f_t,
                               G_s, G_t, B, (int)Ds, (int)Dt, vec_s, vec_t);
            return hipGetLastError();
        });
    });
}

hipError_t launch_pkt_terms(const double* G_s, const double* G_t, int B, void* ws, double* M, float* loss, hipStream_t st) {
    const int nt = pkt_tiles(B);
    double* W = (double*)ws;
    double *kl = W + (size_t)B * B, *ns = kl + B;
    hipLaunchKernelGGL(pkt_rows_kernel, dim3(B), dim3(REL_THREADS), 0, st, G_s, G_t, W, kl, ns, B);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pkt_m_kernel, dim3(nt, nt), dim3(REL_THREADS), 0, st, G_s, (const double*)W, (const double*)kl, (const double*)ns,
                       M, loss, B);
    return hipGetLastError();
}

hipError_t launch_pkt_bwd(const void* f_s, const double* M, const float* g_loss, void* dF, int B, long long D, int dtype,
                          hipStream_t st) {
    const dim3 grid((unsigned)((D + REL_BC - 1) / REL_BC), (unsigned)((B + REL_BR - 1) / REL_BR));
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(pkt_bwd_kernel<T>, grid, dim3(REL_THREADS), 0, st, (const T*)f_s, M, g_loss, (T*)dF, B, (int)D);
        return hipGetLastError();
    });
}

}  // namespace moma
