// Correlation Congruence (`--distill correlation`; reference distiller_zoo/CC.py behind two LinearEmbed heads of models/util.py,
// train_student_comparison.py:388-395, helper/loops_moma.py:168-171): both embeddings, their difference, the product of neighbouring
// rows and the whole backward -- on x_s [B, Cs], x_t [B, Ct] (each side's feat[-1], flattened; the teacher's detached), W_s [D, Cs],
// b_s [D], W_t [D, Ct], b_t [D]:
//     d = x_s W_s^T + b_s - (x_t W_t^T + b_t)   [B, D]      delta = |d|      loss = sum_{i < B - 1} sum_k delta[i,k] delta[i+1,k] / (B - 1)
//     G[i,k] = sign(d[i,k]) (delta[i-1,k] + delta[i+1,k]) / (B - 1)        (a missing neighbour counts 0; sign(0) = 0, as torch's abs)
//     dx_s = g G W_s      dW_s = g G^T x_s      db_s = g colsum(G)      dW_t = -g G^T x_t      db_t = -db_s      (x_t gets none)
// G does not depend on the upstream gradient g, so the FORWARD writes it (`gu`, fp32 [B, D]) and the backward is three products on it.
//   tile64<AT, BN, F64>   (tile64.hpp) what the three GEMM-shaped kernels run, srrl_gemm_kernel's tile product: a 64 x 64 tile of
//             outputs, segments of 32 elements of the reduction.  The backward products (F64 = false) use srrl's arithmetic: plain
//             fp32 FMA over the segment, the segment's sum then added to a DOUBLE total (gfx950 has no xf32).  The forward product
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
//   cc_loss_kernel     one workgroup adds the columns' sums in a fixed order (tile64.hpp's ordered sum) -> loss = total / (B - 1).
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
#include "tile64.hpp"

namespace moma {
namespace {

constexpr int CC_THREADS = T64_THREADS;
constexpr int CC_TC = 4;                            // columns of a workgroup of the finalize (few: D / 4 workgroups share the partial sums)
constexpr int CC_RL = CC_THREADS / CC_TC;           // row lanes per column

// out[z, b, k]: split z of the concatenated reduction, the first splits_s of them over x_s W_s^T, the others over x_t W_t^T
template <typename TS, typename TT>
__global__ __launch_bounds__(CC_THREADS) void cc_diff_kernel(const TS* __restrict__ xs, const TT* __restrict__ xt,
                                                             const float* __restrict__ Ws, const float* __restrict__ Wt,
                                                             double* __restrict__ out, int B, int Cs, int Ct, int D, int segs,
                                                             int splits_s) {
    __shared__ float As[T64_LDS], Bs[T64_LDS];
    const int n0 = blockIdx.x * T64_TILE, m0 = blockIdx.y * T64_TILE, z = blockIdx.z;
    double dacc[4][4];
    tile64_zero(dacc);
    if (z < splits_s) {                                                            // (uniform over the workgroup)
        const int kbeg = z * segs * T64_SEG, kend = min(Cs, kbeg + segs * T64_SEG);
        tile64<false, false, true, TS, float>(xs, Ws, As, Bs, B, D, Cs, kbeg, kend, m0, n0, dacc);
    } else {
        const int kbeg = (z - splits_s) * segs * T64_SEG, kend = min(Ct, kbeg + segs * T64_SEG);
        tile64<false, false, true, TT, float>(xt, Wt, As, Bs, B, D, Ct, kbeg, kend, m0, n0, dacc);
    }
    tile64_each(dacc, m0, n0, B, D, [=](int m, int n, double v) { out[((size_t)z * B + m) * D + n] = v; });
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

// one workgroup: tile64.hpp's ordered sum over the columns
__global__ __launch_bounds__(CC_THREADS) void cc_loss_kernel(const double* __restrict__ colsum, int B, int D, float* __restrict__ loss) {
    const double w = ordered_sum(strided_sum(colsum, D));
    if (threadIdx.x == 0) *loss = (float)(w / (double)(B - 1));
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
    __shared__ float As[T64_LDS], Bs[T64_LDS];
    const int tid = threadIdx.x, it = blockIdx.x;
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
    tile64_zero(dacc);
    if (it < a.first[1]) {                                                         // dx_s [B, Cs] = G W_s, reduction over D
        const int Cs = a.Cs, nt = ceil_div(Cs, T64_TILE), t = it - a.first[0];
        const int m0 = (t / nt) * T64_TILE, n0 = (t % nt) * T64_TILE;
        tile64<false, true, false, float, float>(a.gu, a.Ws, As, Bs, B, Cs, D, 0, D, m0, n0, dacc);
        tile64_each(dacc, m0, n0, B, Cs, [=](int m, int n, double v) { st1<TS>((TS*)a.dxs + (size_t)m * Cs + n, round_f32(v * gl)); });
        return;
    }
    const bool teacher = it >= a.first[2];                                         // dW [D, C] = +- G^T x, reduction over B
    const int Cc = teacher ? a.Ct : a.Cs, nt = ceil_div(Cc, T64_TILE), t = it - a.first[teacher ? 2 : 1];
    const int m0 = (t / nt) * T64_TILE, n0 = (t % nt) * T64_TILE;
    if (teacher) tile64<true, true, false, float, TT>(a.gu, (const TT*)a.xt, As, Bs, D, Cc, B, 0, B, m0, n0, dacc);
    else tile64<true, true, false, float, TS>(a.gu, (const TS*)a.xs, As, Bs, D, Cc, B, 0, B, m0, n0, dacc);
    float* dW = teacher ? a.dWt : a.dWs;
    const double f = teacher ? -gl : gl;
    tile64_each(dacc, m0, n0, D, Cc, [=](int m, int n, double v) { dW[(size_t)m * Cc + n] = round_f32(v * f); });
}

// segments of 32 along the concatenated reduction (both sides' segments) that one workgroup of the forward product adds, and the
// splits of one side that makes
int cc_segs(int B, int Cs, int Ct, int D) { return tile64_segs(tile64_tiles(B, D), ceil_div(Cs, T64_SEG) + ceil_div(Ct, T64_SEG)); }
int cc_splits(int B, int Cs, int Ct, int D, int Cside) { return ceil_div(ceil_div(Cside, T64_SEG), cc_segs(B, Cs, Ct, D)); }

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
    const dim3 grid(ceil_div(D, T64_TILE), ceil_div(B, T64_TILE), ns + nt);
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
    hipLaunchKernelGGL(cc_finalize_kernel, dim3(ceil_div(D, CC_TC)), dim3(CC_THREADS), 0, st, (const double*)P, ns, nt, b_s, b_t, B, D, d,
                       d_out, gu, colsum);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(cc_loss_kernel, dim3(1), dim3(CC_THREADS), 0, st, (const double*)colsum, B, D, loss);
    return hipGetLastError();
}

hipError_t launch_cc_bwd(const float* gu, const void* x_s, const void* x_t, const float* W_s, const float* g_loss, void* dx_s, float* dW_s,
                         float* db_s, float* dW_t, float* db_t, int B, int Cs, int Ct, int D, int dt_s, int dt_t, hipStream_t st) {
    CcBwdArgs a{gu, x_s, x_t, W_s, g_loss, dx_s, dW_s, db_s, dW_t, db_t, B, Cs, Ct, D, {}};
    const int td = ceil_div(D, T64_TILE);
    int n = 0;
    a.first[0] = n; n += dx_s ? ceil_div(B, T64_TILE) * ceil_div(Cs, T64_TILE) : 0;
    a.first[1] = n; n += dW_s ? td * ceil_div(Cs, T64_TILE) : 0;
    a.first[2] = n; n += dW_t ? td * ceil_div(Ct, T64_TILE) : 0;
    a.first[3] = n; n += db_s || db_t ? ceil_div(D, CC_THREADS) : 0;
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
