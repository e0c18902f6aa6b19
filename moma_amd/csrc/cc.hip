// Correlation Congruence (`--distill correlation`; reference distiller_zoo/CC.py behind two LinearEmbed heads of models/util.py,
// train_student_comparison.py:388-395, helper/loops_moma.py:168-171): both embeddings, their difference, the product of neighbouring
// rows and the whole backward -- on x_s [B, Cs], x_t [B, Ct] (each side's feat[-1], flattened; the teacher's detached), W_s [D, Cs],
// b_s [D], W_t [D, Ct], b_t [D]:
//     d = x_s W_s^T + b_s - (x_t W_t^T + b_t)   [B, D]      delta = |d|      loss = sum_{i < B - 1} sum_k delta[i,k] delta[i+1,k] / (B - 1)
//     G[i,k] = sign(d[i,k]) (delta[i-1,k] + delta[i+1,k]) / (B - 1)        (a missing neighbour counts 0; sign(0) = 0, as torch's abs)
//     dx_s = g G W_s      dW_s = g G^T x_s      db_s = g colsum(G)      dW_t = -g G^T x_t      db_t = -db_s      (x_t gets none)
// G does not depend on the upstream gradient g, so the FORWARD writes it (`gu`, fp32 [B, D]) and the backward is three products on it.
//   cc_tile<AT, BN, F64>  what the three GEMM-shaped kernels share, srrl_gemm_kernel's tile loop: a 64 x 64 tile of outputs, 4 x 4 per
//             thread from LDS tiles of both operands, one SEGMENT of 32 elements of the reduction at a time, the next segment
//             requested while the current one is multiplied.  The backward products (F64 = false) use srrl's arithmetic: plain fp32
//             FMA over the segment, the segment's sum then added to a DOUBLE total (gfx950 has no xf32).  The forward product
//             (F64 = true) multiplies and adds in double from the first element on: d is the DIFFERENCE of two sums that are each
//             several times larger, so an fp32 partial sum's rounding, harmless relative to a side, is not relative to d, and the loss
//             of a case with few terms (B = 2, D = 2) then misses twice the reference's own distance (seen: 1.33 x); the product of two
//             fp32 values is exact in double, so d is the exact difference but for its one rounding.  Element accesses (fp32 or bf16
//             per operand): no alignment beyond the element, no divisibility asked.
//   cc_diff_kernel     d's partial sums as ONE product over the concatenated reduction of Cs + Ct elements: blockIdx.z is a split of
//             `segs` segments that lies wholly inside one side (the first splits_s belong to x_s W_s^T, the others to x_t W_t^T);
//             segs is a function of the shape alone (about one workgroup per compute unit): partials [splits_s + splits_t, B, D] in
//             double.
//   cc_finalize_kernel one workgroup per CC_TC = 4 columns of d, 64 row lanes: each side's splits added in order, the two totals
//             subtracted, b_s - b_t added, d rounded ONCE to fp32 (-> the workspace, and d_out); behind a barrier the same lanes write
//             gu = round(sign(d) (|d above| + |d below|) / (B - 1)) from double, and lane 0 of a column walks down its rows in row
//             order adding |d[i]| |d[i+1]| in double -> one double per column.
//   cc_loss_kernel     one workgroup adds the columns' sums in a fixed order -> loss = total / (B - 1).
//   cc_bwd_kernel      ONE grouped launch over a flat list of work items: the 64 x 64 tiles of dx_s [B, Cs] (reduction over D), of
//             dW_s [D, Cs] and of dW_t [D, Ct] (reduction over B, whole: no split, nothing to add up afterwards), then items of 256
//             columns of the bias sums (rows added in row order in double).  Every total is multiplied by g_loss (a DEVICE scalar) in
//             double and rounded once: a power of two in g_loss scales every bit pattern exactly; db_t is db_s with the sign bit
//             flipped.  Outputs that are not asked for have no items.
// Three launches forward, one backward.  No atomics, every sum in a fixed order that depends on the shape alone: bitwise repeatable.
// Identical sides (the same x, W, b; Cs = Ct) split alike, so both totals are the same bits: d, the loss and every gradient are 0.
// hipcc -O3, gfx950 (resource report, -Rpass-analysis=kernel-resource-usage), the same over all four instantiations:
//   cc_diff_kernel 166 VGPRs (16 double accumulators, 8 double operands of four steps in flight, 16 values of the next segment: 3 waves
//   per SIMD) and 16.5 KB of LDS; cc_finalize_kernel 30 VGPRs, no LDS; cc_loss_kernel 34 VGPRs, 2 KB of LDS; cc_bwd_kernel 132 VGPRs
//   (16 double and 16 fp32 accumulators, 16 values of the next segment in flight: 3 waves per SIMD) and 16.5 KB of LDS.
//   No kernel spills, none uses scratch.
#include "common.hpp"

namespace moma {
namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_TILE = 64;                         // outputs of a tile per side (4 x 4 per thread)
constexpr int CC_SEG = 32;                          // elements of the reduction in one fp32 segment
constexpr int CC_TARGET_WG = 256;                   // workgroups the forward product aims at when it splits its reduction
constexpr int CC_TC = 4;                            // columns of a workgroup of the finalize (few: D / 4 workgroups share the partial sums)
constexpr int CC_RL = CC_THREADS / CC_TC;           // row lanes per column
constexpr int CC_LD = CC_SEG + 1, CC_LN = CC_TILE + 1, CC_PER = CC_TILE * CC_SEG / CC_THREADS;
constexpr int CC_LDS = CC_TILE * CC_LD;             // floats of one operand's tile ([row][k], stride 33; the BN form [k][n], stride 65, is smaller)
static_assert(CC_SEG * CC_LN <= CC_LDS, "both layouts fit one tile");

// dacc[i][j] += sum over k in [kbeg, kend) of A(m0 + ty + 16 i, k) Bm(k, n0 + tx + 16 j), rows past M and columns past N read as 0:
//     A(m, k)  = AT ? A[k M + m]  : A[m Kr + k]            Bm(k, n) = BN ? Bm[k N + n] : Bm[n Kr + k]
// The tiles lie in LDS as [row][k] with a stride of 33 (the BN form of Bm as [k][n], stride 65): the 16 columns of a wave's read fall
// into 16 banks and its 4 rows are broadcasts.
template <bool AT, bool BN, bool F64, typename TA, typename TB>
__device__ __forceinline__ void cc_tile(const TA* __restrict__ A, const TB* __restrict__ Bm, float* As, float* Bs, int M, int N, int Kr,
                                        int kbeg, int kend, int m0, int n0, double (&dacc)[4][4]) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    float ra[CC_PER], rb[CC_PER];
    auto request = [&](int k0) {
#pragma unroll
        for (int r = 0; r < CC_PER; ++r) {
            const int idx = tid + r * CC_THREADS;
            if constexpr (AT) {
                const int gk = k0 + idx / CC_TILE, gm = m0 + idx % CC_TILE;
                ra[r] = gk < kend && gm < M ? ld1<TA>(A + (size_t)gk * M + gm) : 0.f;
            } else {
                const int gm = m0 + idx / CC_SEG, gk = k0 + idx % CC_SEG;
                ra[r] = gm < M && gk < kend ? ld1<TA>(A + (size_t)gm * Kr + gk) : 0.f;
            }
            if constexpr (BN) {
                const int gk = k0 + idx / CC_TILE, gn = n0 + idx % CC_TILE;
                rb[r] = gk < kend && gn < N ? ld1<TB>(Bm + (size_t)gk * N + gn) : 0.f;
            } else {
                const int gn = n0 + idx / CC_SEG, gk = k0 + idx % CC_SEG;
                rb[r] = gn < N && gk < kend ? ld1<TB>(Bm + (size_t)gn * Kr + gk) : 0.f;
            }
        }
    };
    request(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += CC_SEG) {
#pragma unroll
        for (int r = 0; r < CC_PER; ++r) {
            const int idx = tid + r * CC_THREADS;
            if constexpr (AT) As[(idx % CC_TILE) * CC_LD + idx / CC_TILE] = ra[r];
            else As[(idx / CC_SEG) * CC_LD + idx % CC_SEG] = ra[r];
            if constexpr (BN) Bs[(idx / CC_TILE) * CC_LN + idx % CC_TILE] = rb[r];
            else Bs[(idx / CC_SEG) * CC_LD + idx % CC_SEG] = rb[r];
        }
        __syncthreads();
        if (k0 + CC_SEG < kend) request(k0 + CC_SEG);
        if constexpr (F64) {
#pragma unroll 4
            for (int kk = 0; kk < CC_SEG; ++kk) {
                double av[4], bv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) av[i] = (double)As[(ty + 16 * i) * CC_LD + kk];
#pragma unroll
                for (int j = 0; j < 4; ++j) bv[j] = (double)(BN ? Bs[kk * CC_LN + tx + 16 * j] : Bs[(tx + 16 * j) * CC_LD + kk]);
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
        for (int kk = 0; kk < CC_SEG; ++kk) {
            float av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = As[(ty + 16 * i) * CC_LD + kk];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = BN ? Bs[kk * CC_LN + tx + 16 * j] : Bs[(tx + 16 * j) * CC_LD + kk];
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

__device__ __forceinline__ void cc_zero(double (&dacc)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) dacc[i][j] = 0.0;
}

// out[z, b, k]: split z of the concatenated reduction, the first splits_s of them over x_s W_s^T, the others over x_t W_t^T
template <typename TS, typename TT>
__global__ __launch_bounds__(CC_THREADS) void cc_diff_kernel(const TS* __restrict__ xs, const TT* __restrict__ xt,
                                                             const float* __restrict__ Ws, const float* __restrict__ Wt,
                                                             double* __restrict__ out, int B, int Cs, int Ct, int D, int segs,
                                                             int splits_s) {
    __shared__ float As[CC_LDS], Bs[CC_LDS];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.x * CC_TILE, m0 = blockIdx.y * CC_TILE, z = blockIdx.z;
    double dacc[4][4];
    cc_zero(dacc);
    if (z < splits_s) {                                                            // (uniform over the workgroup)
        const int kbeg = z * segs * CC_SEG, kend = min(Cs, kbeg + segs * CC_SEG);
        cc_tile<false, false, true, TS, float>(xs, Ws, As, Bs, B, D, Cs, kbeg, kend, m0, n0, dacc);
    } else {
        const int kbeg = (z - splits_s) * segs * CC_SEG, kend = min(Ct, kbeg + segs * CC_SEG);
        cc_tile<false, false, true, TT, float>(xt, Wt, As, Bs, B, D, Ct, kbeg, kend, m0, n0, dacc);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + ty + 16 * i, n = n0 + tx + 16 * j;
            if (m < B && n < D) out[((size_t)z * B + m) * D + n] = dacc[i][j];
        }
}

// one workgroup per CC_TC columns; thread (tr, tc) owns rows tr, tr + 16, ... of column tc.  d is written and read again by the same
// workgroup (its neighbours in a column belong to other lanes): plain pointers, a barrier in between.
__global__ __launch_bounds__(CC_THREADS) void cc_finalize_kernel(const double* __restrict__ P, int splits_s, int splits_t,
                                                                 const float* __restrict__ bs, const float* __restrict__ bt, int B, int D,
                                                                 float* d, float* __restrict__ d_out, float* __restrict__ gu,
                                                                 double* __restrict__ colsum) {
    const int tid = threadIdx.x, tc = tid % CC_TC, tr = tid / CC_TC, k = blockIdx.x * CC_TC + tc;
    const bool ok = k < D;
    const size_t plane = (size_t)B * D;
    if (ok) {
        const double bias = (double)bs[k] - (double)bt[k];
        for (int i = tr; i < B; i += CC_RL) {
            const size_t at = (size_t)i * D + k;
            double us = 0.0, ut = 0.0;
            for (int s = 0; s < splits_s; ++s) us += P[(size_t)s * plane + at];
            for (int s = 0; s < splits_t; ++s) ut += P[(size_t)(splits_s + s) * plane + at];
            const float dv = round_f32((us - ut) + bias);
            d[at] = dv;
            if (d_out) d_out[at] = dv;
        }
    }
    __syncthreads();
    if (!ok) return;
    const double bm1 = (double)(B - 1);
    for (int i = tr; i < B; i += CC_RL) {
        const size_t at = (size_t)i * D + k;
        const float dv = d[at];
        const double up = i > 0 ? (double)fabsf(d[at - D]) : 0.0, dn = i + 1 < B ? (double)fabsf(d[at + D]) : 0.0;
        const double sg = dv > 0.f ? 1.0 : dv < 0.f ? -1.0 : 0.0;
        gu[at] = round_f32(sg * (up + dn) / bm1);
    }
    if (tr == 0) {
        double l = 0.0, prev = (double)fabsf(d[k]);
        for (int i = 1; i < B; ++i) {
            const double cur = (double)fabsf(d[(size_t)i * D + k]);
            l = fma(prev, cur, l);
            prev = cur;
        }
        colsum[k] = l;
    }
}

// one workgroup: thread i adds columns i, i + 256, ... in order, thread 0 the 256 sums in order
__global__ __launch_bounds__(CC_THREADS) void cc_loss_kernel(const double* __restrict__ colsum, int B, int D, float* __restrict__ loss) {
    __shared__ double ls[CC_THREADS];
    const int tid = threadIdx.x;
    double u = 0.0;
    for (int i = tid; i < D; i += CC_THREADS) u += colsum[i];
    ls[tid] = u;
    __syncthreads();
    if (tid == 0) {
        double w = 0.0;
        for (int i = 0; i < CC_THREADS; ++i) w += ls[i];
        *loss = (float)(w / (double)(B - 1));
    }
}

struct CcBwdArgs {
    const float* gu;
    const void *xs, *xt;
    const float *Ws, *g_loss;
    void* dxs;
    float *dWs, *dbs, *dWt, *dbt;
    int B, Cs, Ct, D;
    int first[5];                                   // items in front of: the tiles of dx_s, of dW_s, of dW_t, the bias items, the end
};

template <typename TS, typename TT>
__global__ __launch_bounds__(CC_THREADS) void cc_bwd_kernel(const CcBwdArgs a) {
    __shared__ float As[CC_LDS], Bs[CC_LDS];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, it = blockIdx.x;
    const int B = a.B, D = a.D;
    const double gl = (double)*a.g_loss;
    if (it >= a.first[3]) {                                                        // the bias sums: one column per thread, rows in order
        const int k = (it - a.first[3]) * CC_THREADS + tid;
        if (k < D) {
            double s = 0.0;
            for (int i = 0; i < B; ++i) s += (double)a.gu[(size_t)i * D + k];
            const float v = round_f32(s * gl);
            if (a.dbs) a.dbs[k] = v;
            if (a.dbt) a.dbt[k] = -v;
        }
        return;
    }
    double dacc[4][4];
    cc_zero(dacc);
    if (it < a.first[1]) {                                                         // dx_s [B, Cs] = G W_s, reduction over D
        const int Cs = a.Cs, nt = (Cs + CC_TILE - 1) / CC_TILE, t = it - a.first[0];
        const int m0 = (t / nt) * CC_TILE, n0 = (t % nt) * CC_TILE;
        cc_tile<false, true, false, float, float>(a.gu, a.Ws, As, Bs, B, Cs, D, 0, D, m0, n0, dacc);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int m = m0 + ty + 16 * i, n = n0 + tx + 16 * j;
                if (m < B && n < Cs) st1<TS>((TS*)a.dxs + (size_t)m * Cs + n, round_f32(dacc[i][j] * gl));
            }
        return;
    }
    const bool teacher = it >= a.first[2];                                         // dW [D, C] = +- G^T x, reduction over B
    const int Cc = teacher ? a.Ct : a.Cs, nt = (Cc + CC_TILE - 1) / CC_TILE, t = it - a.first[teacher ? 2 : 1];
    const int m0 = (t / nt) * CC_TILE, n0 = (t % nt) * CC_TILE;
    if (teacher) cc_tile<true, true, false, float, TT>(a.gu, (const TT*)a.xt, As, Bs, D, Cc, B, 0, B, m0, n0, dacc);
    else cc_tile<true, true, false, float, TS>(a.gu, (const TS*)a.xs, As, Bs, D, Cc, B, 0, B, m0, n0, dacc);
    float* dW = teacher ? a.dWt : a.dWs;
    const double f = teacher ? -gl : gl;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + ty + 16 * i, n = n0 + tx + 16 * j;
            if (m < D && n < Cc) dW[(size_t)m * Cc + n] = round_f32(dacc[i][j] * f);
        }
}

int cc_ceil(int a, int b) { return (a + b - 1) / b; }

// segments of 32 along the concatenated reduction that one workgroup of the forward product adds: all of a side where the tiles alone
// fill the device
int cc_segs(int B, int Cs, int Ct, int D) {
    const int tiles = cc_ceil(B, CC_TILE) * cc_ceil(D, CC_TILE), nseg = cc_ceil(Cs, CC_SEG) + cc_ceil(Ct, CC_SEG);
    const int want = max(1, min(nseg, CC_TARGET_WG / tiles));
    return cc_ceil(nseg, want);
}
int cc_splits(int B, int Cs, int Ct, int D, int Cside) { return cc_ceil(cc_ceil(Cside, CC_SEG), cc_segs(B, Cs, Ct, D)); }

// the workspace: the partial sums and the columns' sums in double, then d in fp32
size_t cc_ws_doubles(int B, int Cs, int Ct, int D) {
    return (size_t)(cc_splits(B, Cs, Ct, D, Cs) + cc_splits(B, Cs, Ct, D, Ct)) * B * D + (size_t)D;
}

}  // namespace

size_t cc_workspace_bytes(int B, int Cs, int Ct, int D) {
    return cc_ws_doubles(B, Cs, Ct, D) * sizeof(double) + (size_t)B * D * sizeof(float);
}

hipError_t launch_cc_fwd(const void* x_s, const void* x_t, const float* W_s, const float* b_s, const float* W_t, const float* b_t, int B,
                         int Cs, int Ct, int D, int dt_s, int dt_t, void* workspace, float* gu, float* loss, float* d_out,
                         hipStream_t st) {
    const int segs = cc_segs(B, Cs, Ct, D), ns = cc_splits(B, Cs, Ct, D, Cs), nt = cc_splits(B, Cs, Ct, D, Ct);
    double* P = (double*)workspace;
    double* colsum = P + (size_t)(ns + nt) * B * D;
    float* d = (float*)((double*)workspace + cc_ws_doubles(B, Cs, Ct, D));
    const dim3 grid(cc_ceil(D, CC_TILE), cc_ceil(B, CC_TILE), ns + nt);
    with_dtype(dt_s, [&](auto ts) {
        return with_dtype(dt_t, [&](auto tt) {
            using TS = typename decltype(ts)::type;
            using TT = typename decltype(tt)::type;
            hipLaunchKernelGGL((cc_diff_kernel<TS, TT>), grid, dim3(CC_THREADS), 0, st, (const TS*)x_s, (const TT*)x_t, W_s, W_t, P, B, Cs,
                               Ct, D, segs, ns);
            return 0;
        });
    });
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(cc_finalize_kernel, dim3(cc_ceil(D, CC_TC)), dim3(CC_THREADS), 0, st, (const double*)P, ns, nt, b_s, b_t, B, D, d,
                       d_out, gu, colsum);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(cc_loss_kernel, dim3(1), dim3(CC_THREADS), 0, st, (const double*)colsum, B, D, loss);
    return hipGetLastError();
}

hipError_t launch_cc_bwd(const float* gu, const void* x_s, const void* x_t, const float* W_s, const float* g_loss, void* dx_s, float* dW_s,
                         float* db_s, float* dW_t, float* db_t, int B, int Cs, int Ct, int D, int dt_s, int dt_t, hipStream_t st) {
    CcBwdArgs a{gu, x_s, x_t, W_s, g_loss, dx_s, dW_s, db_s, dW_t, db_t, B, Cs, Ct, D, {}};
    const int td = cc_ceil(D, CC_TILE);
    int n = 0;
    a.first[0] = n; n += dx_s ? cc_ceil(B, CC_TILE) * cc_ceil(Cs, CC_TILE) : 0;
    a.first[1] = n; n += dW_s ? td * cc_ceil(Cs, CC_TILE) : 0;
    a.first[2] = n; n += dW_t ? td * cc_ceil(Ct, CC_TILE) : 0;
    a.first[3] = n; n += db_s || db_t ? cc_ceil(D, CC_THREADS) : 0;
    a.first[4] = n;
    if (n == 0) return hipSuccess;
    with_dtype(dt_s, [&](auto ts) {
        return with_dtype(dt_t, [&](auto tt) {
            using TS = typename decltype(ts)::type;
            using TT = typename decltype(tt)::type;
            hipLaunchKernelGGL((cc_bwd_kernel<TS, TT>), dim3(n), dim3(CC_THREADS), 0, st, a);
            return 0;
        });
    });
    return hipGetLastError();
}

}  // namespace moma
