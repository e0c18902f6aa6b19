// Relational Knowledge Distillation (`--distill rkd`; reference distiller_zoo/RKD.py, helper/loops_moma.py:155-158) on feat[-1] of both
// networks, student X [B, Ds], teacher Y [B, Dt], w_d = 25, w_a = 50.  Everything is a function of the B x B matrices of pairwise
// SQUARED distances, per side S_ij = sum_k (x_ik - x_jk)^2 (summed from the differences: exactly 0 on the diagonal and for equal rows):
//     d_ij = sqrt(max(S_ij, 1e-12)) (0 for i = j)   mu = sum d / (B (B - 1))   l_d = (1/B^2) sum_ij sl1(d^s_ij / mu^s - d^t_ij / mu^t)
//     n_ab = max(sqrt(S_ab), 1e-12)   A_a[b,c] = (S_ab + S_ac - S_bc) / (2 n_ab n_ac)   (the law of cosines; 0 where S_ab or S_ac is 0)
//     l_a = (1/B^3) sum_abc sl1(A^s - A^t)   loss = w_d l_d + w_a l_a   sl1(z) = z^2 / 2 for |z| < 1, |z| - 1/2 otherwise
//     Q_ij = d loss / d S^s_ij (the B^2 entries independent)   dX = g M (X - mean),  M = -2 (Q + Q^T) off the diagonal, rows summing to 0
// No [B, B, D] object exists, nothing of size B^3 is stored.  All arithmetic in double; fp32 / bf16 inputs are exact once widened.
//   rkd_dist   grid (nt, nt), nt = ceil(B / 16); the workgroups with ti <= tj each own one 16 x 16 tile of S and write it and its
//              mirror image from the same values.  D streams through LDS in slabs of 128 columns of both row tiles (rel_stage of
//              batchrel.hpp, shared with pkt_gram); wave w sums columns 32 w .. 32 w + 31 of every slab, each lane a 2 x 2 block of
//              the tile; the four waves' sums meet in LDS in the order 0, 1, 2, 3.  A row is read ceil(B / 16) times.
//              hipcc -O3, gfx950: 100 VGPRs (fp32) / 104 (bf16), no AGPRs, no spill, no scratch; LDS 32.3 KB slabs + 8 KB partial sums.
//   rkd_terms  four launches (their sums over a workgroup and over an array: block_sum, array_sum of batchrel.hpp):
//     rkd_rows   grid B: row i of both sides -> 1 / n (0 where S = 0) into the workspace, the row's sums of d.             32 VGPRs
//     rkd_drow   grid B: mu of both sides (every workgroup adds the B row sums in the same order), the row's sums of sl1 and of
//                sl1' d / mu.                                                                                             44 VGPRs
//     rkd_angle  grid (nt, nt): thread (i, j) of a 16 x 16 tile loops over the third index k in order; per k it evaluates the triple
//                (anchor k; i, j), whose S_ij role feeds Q_ij, and the triple (anchor i; j, k), whose S_ij role (doubled: the b <-> c
//                symmetry) feeds Q_ij and whose sl1 is the thread's share of l_a.  Rows i and j of S and 1 / n of both sides stream
//                through LDS in slabs of 32 k (8 arrays [32][16] double, read by the symmetry of S as columns: 128-byte segments).
//                The distance term's part of Q_ij, with its dependence through mu, is added at the end.  Writes Q and one partial
//                sum per workgroup.                                              123 VGPRs, four waves per SIMD, LDS 32 KB + 32 B
//     rkd_final  one workgroup adds the row sums and the partials in a fixed order -> terms (l_d, l_a), loss.              24 VGPRs
//   rkd_bwd    grid (ceil(D / 64), ceil(B / 32)): dX[32 rows, 64 columns] = g M . (X - mean) on v_mfma_f64_16x16x4_f64 (wave w owns
//              columns 16 w .. 16 w + 15, two accumulators of 4 doubles).  Prologue: the column means of its 64 columns (double, fixed
//              order) and the diagonal of M for its 32 rows.  j streams in slabs of 16: M from Q and Q^T, X - mean in double.
//              dF_s is written in f_s's dtype, rounded double -> fp32 (-> bf16).  The part behind the prologue is rel_bwd of
//              batchrel.hpp (pkt_bwd) written out: see the kernel for why.
//              hipcc -O3, gfx950: 50 VGPRs + 16 AGPRs (the accumulators), no spill, no scratch; LDS 4.3 KB M + 10 KB X + 2.8 KB.
// None of the launches spills or uses scratch (the compiler's kernel-resource-usage report).
// No atomics: every sum has an order that depends on the shapes alone -- bitwise repeatable.
#include "batchrel.hpp"

namespace moma {
namespace {

constexpr int RKD_KC = 32;                   // third indices of one rkd_angle slab
constexpr double RKD_EPS = 1e-12;

__device__ __forceinline__ double rkd_sl1(double z) {
    const double a = fabs(z);
    return a < 1.0 ? 0.5 * z * z : a - 0.5;
}
__device__ __forceinline__ double rkd_clip(double z) { return fmin(fmax(z, -1.0), 1.0); }

// grid (nt, nt): tile (ti = blockIdx.y, tj = blockIdx.x), ti <= tj
template <typename T>
__global__ __launch_bounds__(REL_THREADS) void rkd_dist_kernel(const T* __restrict__ f, double* __restrict__ S, int B, int D, int vec) {
    __shared__ double Xi[REL_T * REL_LDD], Xj[REL_T * REL_LDD];
    __shared__ double part[4][REL_T * REL_T];
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;                                          // (uniform: before any barrier)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, lr = lane >> 3, lc = lane & 7;
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;            // rows lr, lr + 8 x columns lc, lc + 8 of the tile
    for (long long k0 = 0; k0 < D; k0 += REL_KD) {
        __syncthreads();                                          // the slab of the previous turn has been read
        rel_stage<T>(f, B, D, vec, ti * REL_T, k0, Xi);
        rel_stage<T>(f, B, D, vec, tj * REL_T, k0, Xj);
        __syncthreads();
        const double* xi = Xi + lr * REL_LDD + 32 * w;
        const double* xj = Xj + lc * REL_LDD + 32 * w;
#pragma unroll 8
        for (int kk = 0; kk < 32; ++kk) {
            const double p0 = xi[kk], p1 = xi[8 * REL_LDD + kk], q0 = xj[kk], q1 = xj[8 * REL_LDD + kk];
            const double d00 = p0 - q0, d01 = p0 - q1, d10 = p1 - q0, d11 = p1 - q1;
            a00 = fma(d00, d00, a00);
            a01 = fma(d01, d01, a01);
            a10 = fma(d10, d10, a10);
            a11 = fma(d11, d11, a11);
        }
    }
    part[w][lr * REL_T + lc] = a00;
    part[w][lr * REL_T + lc + 8] = a01;
    part[w][(lr + 8) * REL_T + lc] = a10;
    part[w][(lr + 8) * REL_T + lc + 8] = a11;
    __syncthreads();
    const double s = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    const int i = ti * REL_T + (tid >> 4), j = tj * REL_T + (tid & 15);
    if (i < B && j < B) {
        S[(size_t)i * B + j] = s;
        if (ti != tj) S[(size_t)j * B + i] = s;
    }
}

// 1 / n of one entry: n = max(sqrt(S), 1e-12), 0 where S = 0 (that pair spans no angle)
__device__ __forceinline__ double rkd_recip(double s) { return s > 0.0 ? 1.0 / fmax(sqrt(s), RKD_EPS) : 0.0; }

// grid B: row i -> R_s, R_t [i, :], rd_s[i], rd_t[i]
__global__ __launch_bounds__(REL_THREADS) void rkd_rows_kernel(const double* __restrict__ Ss, const double* __restrict__ St,
                                                               double* __restrict__ Rs, double* __restrict__ Rt,
                                                               double* __restrict__ rd_s, double* __restrict__ rd_t, int B) {
    __shared__ double sh[4];
    const int i = blockIdx.x;
    double ds = 0.0, dt = 0.0;
    for (int j = threadIdx.x; j < B; j += REL_THREADS) {
        const double s = Ss[(size_t)i * B + j], t = St[(size_t)i * B + j];
        Rs[(size_t)i * B + j] = rkd_recip(s);
        Rt[(size_t)i * B + j] = rkd_recip(t);
        if (j != i) {
            ds += sqrt(fmax(s, RKD_EPS));
            dt += sqrt(fmax(t, RKD_EPS));
        }
    }
    ds = block_sum(ds, sh);
    dt = block_sum(dt, sh);
    if (threadIdx.x == 0) { rd_s[i] = ds; rd_t[i] = dt; }
}

// grid B: row i -> rl[i] = sum_j sl1(z_ij), rE[i] = sum_j sl1'(z_ij) d^s_ij / mu^s, z = d^s / mu^s - d^t / mu^t
__global__ __launch_bounds__(REL_THREADS) void rkd_drow_kernel(const double* __restrict__ Ss, const double* __restrict__ St,
                                                               const double* __restrict__ rd_s, const double* __restrict__ rd_t,
                                                               double* __restrict__ rl, double* __restrict__ rE, int B) {
    __shared__ double sh[4];
    const int i = blockIdx.x;
    const double pairs = (double)B * (B - 1);
    const double mu_s = array_sum(rd_s, B, sh) / pairs, mu_t = array_sum(rd_t, B, sh) / pairs;
    double l = 0.0, e = 0.0;
    for (int j = threadIdx.x; j < B; j += REL_THREADS) {
        if (j == i) continue;
        const double ds = sqrt(fmax(Ss[(size_t)i * B + j], RKD_EPS)) / mu_s, dt = sqrt(fmax(St[(size_t)i * B + j], RKD_EPS)) / mu_t;
        const double z = ds - dt;
        l += rkd_sl1(z);
        e += rkd_clip(z) * ds;
    }
    l = block_sum(l, sh);
    e = block_sum(e, sh);
    if (threadIdx.x == 0) { rl[i] = l; rE[i] = e; }
}

// grid (nt, nt): rows i of tile blockIdx.y, columns j of tile blockIdx.x
__global__ __launch_bounds__(REL_THREADS) void rkd_angle_kernel(const double* __restrict__ Ss, const double* __restrict__ St,
                                                                const double* __restrict__ Rs, const double* __restrict__ Rt,
                                                                const double* __restrict__ rd_s, const double* __restrict__ rd_t,
                                                                const double* __restrict__ rE, double* __restrict__ Q,
                                                                double* __restrict__ partials, int B, double w_d, double w_a) {
    __shared__ double tile[8][RKD_KC][REL_T];                     // S_s, S_t, R_s, R_t for the rows i (0 .. 3) and the rows j (4 .. 7)
    __shared__ double sh[4];
    const int tid = threadIdx.x, li = tid >> 4, lj = tid & 15;
    const int i0 = blockIdx.y * REL_T, j0 = blockIdx.x * REL_T, i = i0 + li, j = j0 + lj;
    const bool in = i < B && j < B;
    const double pairs = (double)B * (B - 1), B2 = (double)B * B;
    const double mu_s = array_sum(rd_s, B, sh) / pairs, mu_t = array_sum(rd_t, B, sh) / pairs;
    const double E = array_sum(rE, B, sh) / B2;
    const double sij = in ? Ss[(size_t)i * B + j] : 0.0, tij = in ? St[(size_t)i * B + j] : 0.0;
    const double rij = in ? Rs[(size_t)i * B + j] : 0.0, rtij = in ? Rt[(size_t)i * B + j] : 0.0;
    const double own = sqrt(sij) >= RKD_EPS ? rij * rij : 0.0;    // 1 / n_ij^2 where n_ij follows S_ij (not clamped)
    const double* src[4] = {Ss, St, Rs, Rt};
    double q3 = 0.0, ql = 0.0, la = 0.0;
    for (int k0 = 0; k0 < B; k0 += RKD_KC) {
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const int c0 = a < 4 ? i0 : j0;
            const double* m = src[a & 3];
            for (int idx = tid; idx < RKD_KC * REL_T; idx += REL_THREADS) {
                const int kk = idx >> 4, r = idx & 15, k = k0 + kk, c = c0 + r;
                tile[a][kk][r] = (k < B && c < B) ? m[(size_t)k * B + c] : 0.0;          // (S and R are symmetric: row c as a column)
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < RKD_KC; ++kk) {
            const double si = tile[0][kk][li], ti = tile[1][kk][li], ri = tile[2][kk][li], rti = tile[3][kk][li];
            const double sj = tile[4][kk][lj], tj = tile[5][kk][lj], rj = tile[6][kk][lj], rtj = tile[7][kk][lj];
            // anchor k, legs to i and j: S_ij is the side opposite the anchor
            const double rr = ri * rj;
            const double z3 = (si + sj - sij) * 0.5 * rr - (ti + tj - tij) * 0.5 * (rti * rtj);
            q3 = fma(rkd_clip(z3), rr, q3);
            // anchor i, legs to j and k: S_ij is a leg
            const double rl_ = rij * ri;
            const double as = (sij + si - sj) * 0.5 * rl_;
            const double zl = as - (tij + ti - tj) * 0.5 * (rtij * rti);
            la += rkd_sl1(zl);
            ql = fma(rkd_clip(zl), rl_ - as * own, ql);
        }
    }
    if (in) {
        double q = (w_a / (B2 * B)) * (ql - 0.5 * q3);
        if (i != j && sij >= RKD_EPS) {
            const double d = sqrt(sij);
            const double z = d / mu_s - sqrt(fmax(tij, RKD_EPS)) / mu_t;
            q += w_d * (rkd_clip(z) / B2 - E / pairs) / mu_s / (2.0 * d);
        }
        Q[(size_t)i * B + j] = q;
    }
    la = block_sum(la, sh);
    if (tid == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = la;
}

__global__ __launch_bounds__(REL_THREADS) void rkd_final_kernel(const double* __restrict__ rl, const double* __restrict__ partials,
                                                                int B, int np, double w_d, double w_a, float* __restrict__ terms,
                                                                float* __restrict__ loss) {
    __shared__ double sh[4];
    const double B2 = (double)B * B;
    const double l_d = array_sum(rl, B, sh) / B2, l_a = array_sum(partials, np, sh) / (B2 * B);
    if (threadIdx.x == 0) {
        terms[0] = (float)l_d;
        terms[1] = (float)l_a;
        *loss = (float)(w_d * l_d + w_a * l_a);
    }
}

// grid (ceil(D / 64), ceil(B / 32)): rows [32 by, +32) x columns [64 bx, +64) of dX
template <typename T>
__global__ __launch_bounds__(REL_THREADS) void rkd_bwd_kernel(const T* __restrict__ X, const double* __restrict__ Q,
                                                              const float* __restrict__ g_loss, T* __restrict__ dX, int B, int D) {
    __shared__ double Ml[REL_BR * REL_LDM];
    __shared__ double Xl[REL_BJ * REL_LDX];
    __shared__ double red[4][REL_BC], mean[REL_BC], diag[REL_BR];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int i0 = blockIdx.y * REL_BR;
    const size_t d0 = (size_t)blockIdx.x * REL_BC;
    {   // the batch mean of this workgroup's columns: rows w, w + 4, ... in order, then the four sums in order
        const size_t c = d0 + lane;
        double s = 0.0;
        if (c < (size_t)D)
            for (int j = w; j < B; j += 4) s += (double)ld1<T>(X + (size_t)j * D + c);
        red[w][lane] = s;
    }
    {   // the diagonal of M: minus the sum of its row off the diagonal, eight threads per row
        const int r = tid >> 3, t8 = tid & 7, i = i0 + r;
        double s = 0.0;
        if (i < B)
            for (int j = t8; j < B; j += 8)
                if (j != i) s += -2.0 * (Q[(size_t)i * B + j] + Q[(size_t)j * B + i]);
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        if (t8 == 0) diag[r] = -s;
    }
    __syncthreads();
    if (tid < REL_BC) mean[tid] = (((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]) / (double)B;
    // From here on this is rel_bwd of batchrel.hpp with M from diag, Q and Q^T and X' = X - mean, written out: called through
    // rel_bwd the kernel compiles to other code (the same instructions but one, another order) that measured 0.3 - 0.8 % slower
    // (profiles/batchrel_unify.txt).  A change to either body belongs in both.
    f64x4 acc[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[rt][r] = 0.0;
    for (int j0 = 0; j0 < B; j0 += REL_BJ) {
        __syncthreads();                                          // (first turn: mean and diag are written)
        for (int idx = tid; idx < REL_BR * REL_BJ; idx += REL_THREADS) {
            const int r = idx >> 4, jj = idx & 15, i = i0 + r, j = j0 + jj;
            double v = 0.0;
            if (i < B && j < B) v = i == j ? diag[r] : -2.0 * (Q[(size_t)i * B + j] + Q[(size_t)j * B + i]);
            Ml[r * REL_LDM + jj] = v;
        }
        for (int idx = tid; idx < REL_BJ * REL_BC; idx += REL_THREADS) {
            const int jj = idx >> 6, c = idx & 63, j = j0 + jj;
            Xl[jj * REL_LDX + c] = (j < B && d0 + c < (size_t)D) ? (double)ld1<T>(X + (size_t)j * D + d0 + c) - mean[c] : 0.0;
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

int rkd_tiles(int B) { return (B + REL_T - 1) / REL_T; }

}  // namespace

// workspace (doubles): R_s [B, B], R_t [B, B], rd_s [B], rd_t [B], rl [B], rE [B], partials [ceil(B / 16)^2]
size_t rkd_workspace_bytes(int B) {
    const size_t nt = (size_t)rkd_tiles(B);
    return (2 * (size_t)B * B + 4 * (size_t)B + nt * nt) * sizeof(double);
}

hipError_t launch_rkd_dist(const void* f, int B, long long D, int dtype, double* S, hipStream_t st) {
    const int nt = rkd_tiles(B);
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const int vec = pick_vec(D, sizeof(T), (uintptr_t)f, {MAXVEC<T>}) > 1;      // 16 bytes or nothing
        hipLaunchKernelGGL(rkd_dist_kernel<T>, dim3(nt, nt), dim3(REL_THREADS), 0, st, (const T*)f, S, B, (int)D, vec);
        return hipGetLastError();
    });
}

hipError_t launch_rkd_terms(const double* S_s, const double* S_t, int B, double w_d, double w_a, void* ws, double* Q, float* terms,
                            float* loss, hipStream_t st) {
    const int nt = rkd_tiles(B);
    const size_t BB = (size_t)B * B;
    double* Rs = (double*)ws;
    double *Rt = Rs + BB, *rd_s = Rt + BB, *rd_t = rd_s + B, *rl = rd_t + B, *rE = rl + B, *partials = rE + B;
    hipLaunchKernelGGL(rkd_rows_kernel, dim3(B), dim3(REL_THREADS), 0, st, S_s, S_t, Rs, Rt, rd_s, rd_t, B);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rkd_drow_kernel, dim3(B), dim3(REL_THREADS), 0, st, S_s, S_t, (const double*)rd_s, (const double*)rd_t, rl, rE, B);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(rkd_angle_kernel, dim3(nt, nt), dim3(REL_THREADS), 0, st, S_s, S_t, (const double*)Rs, (const double*)Rt,
                       (const double*)rd_s, (const double*)rd_t, (const double*)rE, Q, partials, B, w_d, w_a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(rkd_final_kernel, dim3(1), dim3(REL_THREADS), 0, st, (const double*)rl, (const double*)partials, B, nt * nt, w_d,
                       w_a, terms, loss);
    return hipGetLastError();
}

hipError_t launch_rkd_bwd(const void* f_s, const double* Q, const float* g_loss, void* dF, int B, long long D, int dtype,
                          hipStream_t st) {
    const dim3 grid((unsigned)((D + REL_BC - 1) / REL_BC), (unsigned)((B + REL_BR - 1) / REL_BR));
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(rkd_bwd_kernel<T>, grid, dim3(REL_THREADS), 0, st, (const T*)f_s, Q, g_loss, (T*)dF, B, (int)D);
        return hipGetLastError();
    });
}

}  // namespace moma
