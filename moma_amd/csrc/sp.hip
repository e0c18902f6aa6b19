// Similarity-Preserving distillation (`--distill similarity`; reference distiller_zoo/SP.py, helper/loops_moma.py:140-144) on feat[-2] of
// both networks.  X = f_s as [B, Ks], Y = f_t as [B, Kt] (Ks != Kt allowed), every index runs over the batch:
//     G = X X^T   n_i = max(|G_i|, 1e-12)   H = G / n (row-wise)   (per side)          loss = (1/B^2) sum_ij (H^t_ij - H^s_ij)^2
//     E = -(2/B^2) (H^t - H^s)   Q_i = (E_i - (E_i . H^s_i) H^s_i) / n^s_i  (the projection only where |G^s_i| >= 1e-12)
//     dX = g (Q + Q^T) X = g M X
// G does not change when the K columns are permuted (the same way in every row): a map is read IN STORAGE ORDER as [B, K] with row
// stride K, NCHW and channels_last alike, and dF_s is written in that order.  No layout flag exists.
//   sp_gram   one launch per side, grid (tile pairs, splits): 64 x 64 tiles of G, the nt (nt + 1) / 2 pairs with ti <= tj, nt =
//             ceil(B / 64); K is cut into slabs (fp32: 64 columns, bf16: 128) and split s owns slabs [s per, (s + 1) per), per =
//             ceil(slabs / splits), splits = min(ceil(K / 128), ceil(512 / pairs)) -- a function of B and K alone (a split past the
//             last slab writes zeros).  A slab of both row tiles is staged in LDS in its storage type (fp32, row stride 65; bf16, row
//             stride 136: 16-byte fragment reads); wave w owns the 32 x 32 subtile (w >> 1, w & 1) on v_mfma_f32_32x32x2_f32 /
//             v_mfma_f32_32x32x16_bf16 (products of bf16 are exact in the fp32 accumulator).  The fp32 chain ends with every slab (64
//             columns for fp32 storage, 128 for bf16): it is added to a double total, and that total is rounded once to fp32 when
//             the split's partial is written (sp_rows adds the partials in double).  A diagonal tile stages one row tile and leaves subtile (1, 0) out.  Only entries with
//             i <= j are written, each together with its mirror image: the partial [splits, B, B] (fp32) is symmetric bit for bit.
//             16-byte loads where the base address and K allow, element loads otherwise; zero past B and past K.
//             hipcc -O3, gfx950: 69 VGPRs (fp32) / 82 (bf16) + 16 AGPRs (the accumulator), no spill, no scratch; LDS 32.5 KB / 34 KB.
//   sp_terms  three launches, all in double:
//     sp_rows   grid B: row i of both sides: G = the split partials added in the order 0, 1, ...; n; H; r_i = E_i . H^s_i; the row's
//               sum of (H^t - H^s)^2; the sums over the workgroup: block_sum of batchrel.hpp.       50 VGPRs, LDS 32 B
//     sp_m      grid ceil(B / 16)^2: M_ij = Q_ij + Q_ji (the same sum for (i, j) and (j, i): symmetric bit for bit).   24 VGPRs
//     sp_final  one workgroup adds the B row sums in a fixed order (array_sum of batchrel.hpp) -> loss (fp32).   13 VGPRs, LDS 32 B
//   sp_gram_sum  (moma_sp_gram_sum, `--distill semckd`: ops.batch_gram) G of ONE side on its own as fp32: sp_rows' sum of the split
//             partials (sp_split_sum: one copy), one thread per entry, grid ceil(B^2 / 256).
//   sp_bwd    grid (ceil(K / 64), ceil(B / 128)): dF_s[128 rows, 64 columns] = g M X[:, 64 columns] on v_mfma_f32_32x32x2_f32 for both
//             storages (bf16 widened while it is staged; M rounded to fp32 once per use: every workgroup reads its
//             [128, B] block of M as double and converts it -- B^2 8 bytes of L2 reads per 64 columns, 0.5 GB at B = 256, K = 62720,
//             which the HBM bound does not show).  j streams in slabs of 32; wave w owns column half
//             w & 1 and the row tiles (w >> 1) and (w >> 1) + 2; every slab's chain of 32 products is added to a double total.  g is
//             a DEVICE scalar, folded in in double before the one rounding double -> fp32 (-> bf16).  X is read ceil(B / 128) times,
//             dF_s written once.
//             hipcc -O3, gfx950: 119 VGPRs (fp32) / 106 (bf16) + 32 AGPRs (the accumulators), no spill, no scratch; LDS 16.5 KB M + 12 KB X.
// None of the launches spills or uses scratch (the compiler's kernel-resource-usage report).
// No atomics: every sum has an order that depends on the shapes alone -- bitwise repeatable.
#include "batchrel.hpp"

namespace moma {
namespace {

constexpr int SP_T = 64;                     // rows / columns of a workgroup's tile of G
constexpr int SP_TARGET = 512;               // workgroups sp_gram aims at (two per compute unit)
constexpr int SP_TM = 16;                    // rows / columns of a tile of M
constexpr int SP_BR = 128, SP_BC = 64;       // rows / columns of one sp_bwd workgroup
constexpr int SP_BJ = 32;                    // its slab of the summation index
constexpr int SP_LDM = SP_BJ + 1;            // row stride of the M slab (floats): 32 consecutive rows fall in 32 banks
constexpr int SP_LDX = SP_BC + 32;           // row stride of the X slab: the two k rows of an MFMA step in disjoint banks
constexpr double SP_EPS = 1e-12;             // F.normalize's clamp of the norm

// the staged slab of sp_gram per storage type: KS columns, row stride LD elements
template <typename T> struct SpSlab;
template <> struct SpSlab<float> { static constexpr int KS = 64, LD = 65; };          // odd stride: 32 consecutive rows in 32 banks
template <> struct SpSlab<bf16_raw> { static constexpr int KS = 128, LD = 136; };     // 272-byte rows: 16-byte aligned fragments

// row of accumulator register `reg` in a 32 x 32 MFMA result (the column is lane & 31)
__device__ __forceinline__ int sp_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// rows [r0, r0 + 64) x columns [k0, k0 + KS) of f [B, K] -> lds[r * LD + kk] in the storage type; zero past B and past K.
// vec: K is a multiple of the vector width and the base is 16-byte aligned (k0 is a multiple of KS)
template <typename T>
__device__ __forceinline__ void sp_stage(const T* __restrict__ f, int B, long long K, int vec, int r0, long long k0, T* __restrict__ lds) {
    constexpr int KS = SpSlab<T>::KS, LD = SpSlab<T>::LD, V = MAXVEC<T>, VPR = KS / V;      // vectors per row of the slab
    const int tid = threadIdx.x;
    if (vec) {
        for (int idx = tid; idx < SP_T * VPR; idx += REL_THREADS) {
            const int r = idx / VPR, kv = idx % VPR, row = r0 + r;
            const long long k = k0 + kv * V;
            const bool in = row < B && k < K;                                               // (K % V == 0: all V inside)
            if constexpr (std::is_same<T, float>::value) {
                float v[V] = {0.f, 0.f, 0.f, 0.f};
                if (in) PV<float, V>::ld(f + (size_t)row * K + k, v);
                float* o = lds + r * LD + kv * V;
#pragma unroll
                for (int e = 0; e < V; ++e) o[e] = v[e];
            } else {                                                                        // (bf16 stays bf16: no widening)
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (in) v = *reinterpret_cast<const uint4*>(f + (size_t)row * K + k);
                *reinterpret_cast<uint4*>(lds + r * LD + kv * V) = v;
            }
        }
    } else {
        for (int idx = tid; idx < SP_T * KS; idx += REL_THREADS) {
            const int r = idx / KS, kk = idx % KS, row = r0 + r;
            const long long k = k0 + kk;
            lds[r * LD + kk] = (row < B && k < K) ? f[(size_t)row * K + k] : (T)0;
        }
    }
}

// one slab of a 32 x 32 subtile: acc += Xi[rows] . Xj[rows]^T
__device__ __forceinline__ void sp_slab_mma(const float* __restrict__ xi, const float* __restrict__ xj, int h, f32x16& acc) {
#pragma unroll 8
    for (int kk = 0; kk < SpSlab<float>::KS; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xi[kk + h], xj[kk + h], acc, 0, 0, 0);
}
__device__ __forceinline__ void sp_slab_mma(const bf16_raw* __restrict__ xi, const bf16_raw* __restrict__ xj, int h, f32x16& acc) {
#pragma unroll
    for (int kk = 0; kk < SpSlab<bf16_raw>::KS; kk += 16) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(xi + kk + 8 * h), b = *reinterpret_cast<const bf16x8*>(xj + kk + 8 * h);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
}

// grid (nt (nt + 1) / 2, splits): tile pair blockIdx.x (ti <= tj, row by row), split blockIdx.y
template <typename T>
__global__ __launch_bounds__(REL_THREADS) void sp_gram_kernel(const T* __restrict__ f, float* __restrict__ P, int B, long long K, int vec,
                                                              int nt, long long per, long long nslabs) {
    constexpr int KS = SpSlab<T>::KS, LD = SpSlab<T>::LD;
    __shared__ __attribute__((aligned(16))) T Xi[SP_T * LD];
    __shared__ __attribute__((aligned(16))) T Xj[SP_T * LD];
    int ti = 0, rest = (int)blockIdx.x;
    while (rest >= nt - ti) { rest -= nt - ti; ++ti; }
    const int tj = ti + rest;
    const bool diag = ti == tj;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5, si = w >> 1, sj = w & 1;
    const bool work = !(diag && si == 1 && sj == 0);              // (wave-uniform) the mirror image of subtile (0, 1)
    const T* xj_tile = diag ? Xi : Xj;
    f32x16 acc;
    double tot[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.f; tot[r] = 0.0; }
    const long long s0 = (long long)blockIdx.y * per, s1 = s0 + per < nslabs ? s0 + per : nslabs;
    for (long long s = s0; s < s1; ++s) {
        __syncthreads();                                          // the slab of the previous turn has been read
        sp_stage<T>(f, B, K, vec, ti * SP_T, s * KS, Xi);
        if (!diag) sp_stage<T>(f, B, K, vec, tj * SP_T, s * KS, Xj);
        __syncthreads();
        if (work) {
            sp_slab_mma(Xi + (32 * si + l31) * LD, xj_tile + (32 * sj + l31) * LD, h, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) { tot[r] += (double)acc[r]; acc[r] = 0.f; }
        }
    }
    if (!work) return;                                            // (no barrier below)
    float* Ps = P + (size_t)blockIdx.y * B * B;
    const int j = tj * SP_T + 32 * sj + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = ti * SP_T + 32 * si + sp_row(r, h);
        if (i <= j && j < B) {
            const float v = (float)tot[r];
            Ps[(size_t)i * B + j] = v;
            Ps[(size_t)j * B + i] = v;
        }
    }
}

// entry o of G: the split partials added in double in the order 0, 1, ...  (unrolled: the loads of eight splits are in flight
// together, the additions keep the order; one load per addition made sp_rows 234 us at B = 64, K = 62720, where 64 workgroups
// add 490 partials per side).  THE sum of sp_rows (moma_sp_terms) and of sp_gram_sum (moma_sp_gram_sum)
__device__ __forceinline__ double sp_split_sum(const float* __restrict__ P, int splits, size_t BB, size_t o) {
    double g = 0.0;
#pragma unroll 8
    for (int s = 0; s < splits; ++s) g += (double)P[s * BB + o];
    return g;
}

// grid ceil(B^2 / 256): G [B, B] fp32 of one side.  The partials are symmetric bit for bit and every entry adds them in the same
// order, so G is
__global__ __launch_bounds__(REL_THREADS) void sp_gram_sum_kernel(const float* __restrict__ P, int splits, int B, float* __restrict__ G) {
    const size_t BB = (size_t)B * B, o = (size_t)blockIdx.x * REL_THREADS + threadIdx.x;
    if (o < BB) G[o] = (float)sp_split_sum(P, splits, BB, o);
}

// grid B: row i of both sides.  rows = [n_s | n_t | r | lp], each [B]
__global__ __launch_bounds__(REL_THREADS) void sp_rows_kernel(const float* __restrict__ Ps, int splits_s, const float* __restrict__ Pt,
                                                              int splits_t, int B, double* __restrict__ G, double* __restrict__ H,
                                                              double* __restrict__ rows) {
    __shared__ double sh[4];
    constexpr int PER = MOMA_SP_MAX_B / REL_THREADS;               // entries of a row per thread
    const int i = blockIdx.x;
    const size_t BB = (size_t)B * B;
    double gs[PER], gt[PER], qs = 0.0, qt = 0.0;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int j = threadIdx.x + u * REL_THREADS;
        gs[u] = 0.0;
        gt[u] = 0.0;
        if (j < B) {
            const size_t o = (size_t)i * B + j;
            gs[u] = sp_split_sum(Ps, splits_s, BB, o);
            gt[u] = sp_split_sum(Pt, splits_t, BB, o);
            G[o] = gs[u];
            G[BB + o] = gt[u];
            qs = fma(gs[u], gs[u], qs);
            qt = fma(gt[u], gt[u], qt);
        }
    }
    const double n_s = sqrt(block_sum(qs, sh)), n_t = sqrt(block_sum(qt, sh));
    const double c_s = fmax(n_s, SP_EPS), c_t = fmax(n_t, SP_EPS), e = -2.0 / ((double)B * B);
    double r = 0.0, lp = 0.0;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int j = threadIdx.x + u * REL_THREADS;
        if (j < B) {
            const size_t o = (size_t)i * B + j;
            const double hs = gs[u] / c_s, ht = gt[u] / c_t, d = ht - hs;
            H[o] = hs;
            H[BB + o] = ht;
            r = fma(e * d, hs, r);
            lp = fma(d, d, lp);
        }
    }
    r = block_sum(r, sh);
    lp = block_sum(lp, sh);
    if (threadIdx.x == 0) {
        rows[i] = n_s;
        rows[B + i] = n_t;
        rows[2 * B + i] = r;
        rows[3 * B + i] = lp;
    }
}

// Q_ij = d loss / d G^s_ij: F.normalize's backward, the projection only where the norm is not clamped
__device__ __forceinline__ double sp_q(double hs, double ht, double n, double r, double e) {
    const double E = e * (ht - hs);
    return n >= SP_EPS ? (E - r * hs) / n : E / SP_EPS;
}

// grid (ceil(B / 16), ceil(B / 16)): thread (i, j)
__global__ __launch_bounds__(REL_THREADS) void sp_m_kernel(const double* __restrict__ H, const double* __restrict__ rows, int B,
                                                           double* __restrict__ M) {
    const int i = blockIdx.y * SP_TM + (threadIdx.x >> 4), j = blockIdx.x * SP_TM + (threadIdx.x & 15);
    if (i >= B || j >= B) return;
    const size_t BB = (size_t)B * B, ij = (size_t)i * B + j, ji = (size_t)j * B + i;
    const double e = -2.0 / ((double)B * B);
    const double a = sp_q(H[ij], H[BB + ij], rows[i], rows[2 * B + i], e), b = sp_q(H[ji], H[BB + ji], rows[j], rows[2 * B + j], e);
    M[ij] = i <= j ? a + b : b + a;                               // (the same two operands in the same order for (i, j) and (j, i))
}

__global__ __launch_bounds__(REL_THREADS) void sp_final_kernel(const double* __restrict__ lp, int B, float* __restrict__ loss) {
    __shared__ double sh[4];
    const double s = array_sum(lp, B, sh);
    if (threadIdx.x == 0) *loss = (float)(s / ((double)B * B));
}

// grid (ceil(K / 64), ceil(B / 128)): rows [128 by, +128) x columns [64 bx, +64) of dX
template <typename T>
__global__ __launch_bounds__(REL_THREADS) void sp_bwd_kernel(const T* __restrict__ X, const double* __restrict__ M,
                                                             const float* __restrict__ g_loss, T* __restrict__ dX, int B, long long K,
                                                             int vec) {
    __shared__ float Ml[SP_BR * SP_LDM];
    __shared__ float Xl[SP_BJ * SP_LDX];
    constexpr int V = MAXVEC<T>, VPR = SP_BC / V;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5, ch = w & 1, rt0 = w >> 1;
    const int i0 = blockIdx.y * SP_BR;
    const long long c0 = (long long)blockIdx.x * SP_BC;
    f32x16 acc[2];
    double tot[2][16];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[t][r] = 0.f; tot[t][r] = 0.0; }
    for (int j0 = 0; j0 < B; j0 += SP_BJ) {
        __syncthreads();                                          // the slab of the previous turn has been read
        for (int idx = tid; idx < SP_BR * SP_BJ; idx += REL_THREADS) {
            const int r = idx / SP_BJ, jj = idx % SP_BJ, i = i0 + r, j = j0 + jj;
            Ml[r * SP_LDM + jj] = (i < B && j < B) ? (float)M[(size_t)i * B + j] : 0.f;
        }
        if (vec) {
            for (int idx = tid; idx < SP_BJ * VPR; idx += REL_THREADS) {
                const int jj = idx / VPR, cv = idx % VPR, j = j0 + jj;
                const long long c = c0 + cv * V;
                float v[V];
#pragma unroll
                for (int e = 0; e < V; ++e) v[e] = 0.f;
                if (j < B && c < K) PV<T, V>::ld(X + (size_t)j * K + c, v);                 // (K % V == 0: all V inside)
                float* o = Xl + jj * SP_LDX + cv * V;
#pragma unroll
                for (int e = 0; e < V; ++e) o[e] = v[e];
            }
        } else {
            for (int idx = tid; idx < SP_BJ * SP_BC; idx += REL_THREADS) {
                const int jj = idx / SP_BC, cc = idx % SP_BC, j = j0 + jj;
                const long long c = c0 + cc;
                Xl[jj * SP_LDX + cc] = (j < B && c < K) ? ld1<T>(X + (size_t)j * K + c) : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < SP_BJ; kk += 2) {
            const float bx = Xl[(kk + h) * SP_LDX + 32 * ch + l31];
#pragma unroll
            for (int t = 0; t < 2; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ml[(32 * (rt0 + 2 * t) + l31) * SP_LDM + kk + h], bx, acc[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) { tot[t][r] += (double)acc[t][r]; acc[t][r] = 0.f; }
    }
    const double g = (double)*g_loss;
    const long long c = c0 + 32 * ch + l31;
    if (c >= K) return;                                           // (no barrier below)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + 32 * (rt0 + 2 * t) + sp_row(r, h);
            if (i < B) st1<T>(dX + (size_t)i * K + c, round_f32(g * tot[t][r]));
        }
}

int sp_tiles(int B) { return (B + SP_T - 1) / SP_T; }
long long sp_slabs(long long K, int dtype) {
    const int ks = dtype == MOMA_DT_BF16 ? SpSlab<bf16_raw>::KS : SpSlab<float>::KS;
    return (K + ks - 1) / ks;
}
static_assert(SpSlab<float>::KS <= 128 && SpSlab<bf16_raw>::KS <= 128, "sp_splits: no more splits than slabs of either storage type");

}  // namespace

// K splits of sp_gram: a function of B and K alone (the same for both storage types)
long long sp_splits(int B, long long K) {
    const long long nt = sp_tiles(B), pairs = nt * (nt + 1) / 2, want = (SP_TARGET + pairs - 1) / pairs, cap = (K + 127) / 128;
    return want < cap ? want : cap;
}

// the split partials of one side: [splits, B, B] fp32
size_t sp_workspace_bytes(int B, long long K) { return (size_t)sp_splits(B, K) * B * B * sizeof(float); }

hipError_t launch_sp_gram(const void* f, int B, long long K, int dtype, float* P, hipStream_t st) {
    const int nt = sp_tiles(B);
    const long long splits = sp_splits(B, K), slabs = sp_slabs(K, dtype), per = (slabs + splits - 1) / splits;
    const dim3 grid((unsigned)(nt * (nt + 1) / 2), (unsigned)splits);
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const int vec = pick_vec(K, sizeof(T), (uintptr_t)f, {MAXVEC<T>}) > 1;      // 16 bytes or nothing
        hipLaunchKernelGGL(sp_gram_kernel<T>, grid, dim3(REL_THREADS), 0, st, (const T*)f, P, B, K, vec, nt, per, slabs);
        return hipGetLastError();
    });
}

hipError_t launch_sp_gram_sum(const float* P, int splits, int B, float* G, hipStream_t st) {
    const size_t BB = (size_t)B * B;
    hipLaunchKernelGGL(sp_gram_sum_kernel, dim3((unsigned)((BB + REL_THREADS - 1) / REL_THREADS)), dim3(REL_THREADS), 0, st, P, splits, B, G);
    return hipGetLastError();
}

hipError_t launch_sp_terms(const float* P_s, int splits_s, const float* P_t, int splits_t, int B, double* G, double* H, double* rows,
                           double* M, float* loss, hipStream_t st) {
    const int nm = (B + SP_TM - 1) / SP_TM;
    hipLaunchKernelGGL(sp_rows_kernel, dim3(B), dim3(REL_THREADS), 0, st, P_s, splits_s, P_t, splits_t, B, G, H, rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sp_m_kernel, dim3(nm, nm), dim3(REL_THREADS), 0, st, (const double*)H, (const double*)rows, B, M);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(sp_final_kernel, dim3(1), dim3(REL_THREADS), 0, st, (const double*)(rows + 3 * (size_t)B), B, loss);
    return hipGetLastError();
}

hipError_t launch_sp_bwd(const void* f_s, const double* M, const float* g_loss, void* dF, int B, long long K, int dtype, hipStream_t st) {
    const dim3 grid((unsigned)((K + SP_BC - 1) / SP_BC), (unsigned)((B + SP_BR - 1) / SP_BR));
    return with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        const int vec = (pick_vec(K, sizeof(T), (uintptr_t)f_s, {MAXVEC<T>}) > 1);  // 16 bytes or nothing
        hipLaunchKernelGGL(sp_bwd_kernel<T>, grid, dim3(REL_THREADS), 0, st, (const T*)f_s, M, g_loss, (T*)dF, B, K, vec);
        return hipGetLastError();
    });
}

}  // namespace moma
