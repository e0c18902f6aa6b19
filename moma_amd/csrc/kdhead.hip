// The student's head of every `--distill` step (reference helper/loops_moma.py:278-279 and the accuracy call behind them):
// nn.CrossEntropyLoss(logit_s, y), DistillKL(T)(logit_s, logit_t) (distiller_zoo/KD.py) and helper/util.accuracy (top-1) as two launches
// forward and one backward -- on z_s, z_t [B, K] (each fp32 or bf16, dense, independently), labels [B] int64 and a host float T > 0.
// With a = z / T:
//     m_b = max_k z_s[b,k]     pred_b = the LOWEST k with z_s[b,k] = m_b       (one maximum serves z_s and a_s: T > 0)
//     lse_b  = m_b + log1p(sum_{k != pred_b} exp(z_s[b,k] - m_b))                 ce_b = lse_b - z_s[b,y_b]    (a valid row: 0 <= y_b < K)
//     lseS_b = m_b / T + log1p(SS_b),  SS_b = sum_{k != pred_b} exp((z_s[b,k] - m_b) / T)          and lseT_b, ST_b likewise from z_t
//     kl_b = sum_k p_t (log p_t - log p_s) = W_b / (1 + ST_b) + (log1p(SS_b) - log1p(ST_b)),
//            W_b = sum_k e_t[k] (d_t[k] - d_s[k]),  d = (z - its row's maximum) / T,  e_t = exp(d_t)    (a term with e_t = 0 counts 0)
//     loss_cls = sum_valid ce_b / n_valid       loss_div = T^2 sum_b kl_b / B       acc = 100 #{pred_b == y_b} / B
//     dz_s[b,k] = g_cls (exp(z_s[b,k] - lse_b) - [k == y_b]) / n_valid                              (zero for a row that is not valid)
//               + g_div T (exp(a_s[b,k] - lseS_b) - exp(a_t[b,k] - lseT_b)) / B
// The KL sum is written on the rows' SHIFTED values: the two maxima cancel against the two lse analytically, so W adds terms of order
// e_t d and not differences of logits of order 4, it accumulates beside ST in the same walk (no third pass over memory), and rows with
// z_t = z_s give d_t - d_s = 0 and SS = ST bit for bit: kl_b is exactly 0, and so is the KL part of their gradient.  As in ce.hip, and
// for the reasons given at its top: the maximum's own term is left out of every sum and log1p adds it back; sums, exp, log1p and the
// saved lse values are double; no floating-point atomics, so results repeat bit for bit.  No gradient to z_t.
//   kd_rows_kernel<TS, TT, VEC, ONE>  256 threads; G lanes per row as ce.hip (rowhead.hpp), 256 / G rows per workgroup.  ONE (K <= 16 G
//             <= 1024): both rows are read ONCE, 16 elements per lane and operand in registers; both maxima by xor shuffles inside the G
//             lanes, then S, SS, ST and W from the registers.  !ONE: two walks over both rows.  VEC (8, 4 or 1 elements) is the width
//             BOTH operands allow (rowhead.hpp's ce_vec per operand, the smaller).  Lane 0 of a row writes lse, lseS, lseT, the row's CE
//             and KL terms and its flags (valid / hit / bad label).  A label outside [0, K) is never used as an index.
//   kd_finalize_kernel                ONE workgroup: thread t adds the rows [t c, (t + 1) c), c = ceil(B / 256), in row order in double;
//             thread 0 adds the 256 sums in order -> loss_cls (NaN without a valid row and with a bad label), loss_div, acc, 1 / n_valid.
//   kd_bwd_kernel<TS, TT, VEC>        one thread per VEC elements of dz; no reduction.  g_cls and g_div are DEVICE scalars, either may be
//             NULL (= 0, and its exponentials are not evaluated); both parts are multiplied and added in double before the one rounding
//             to fp32 (and, for bf16, one more to the storage type): a power of two in both scales every bit pattern exactly.
// hipcc -O3, gfx950 (-Rpass-analysis=kernel-resource-usage): see DESIGN.md, section KD head; no kernel spills, none uses scratch.
#include "rowhead.hpp"

namespace moma {
namespace {

static_assert(CE_ONE_WALK == MOMA_KDHEAD_ONE_WALK_K, "header and kernel agree on the one-walk limit");
static_assert(MOMA_KDHEAD_MAX_B == MOMA_CE_MAX_B && MOMA_KDHEAD_MAX_K == MOMA_CE_MAX_K, "the caps are the CE head's");
constexpr int KD_VALID = 1, KD_HIT = 2, KD_BAD = 4;

// the maximum of a row in registers (ONE) or in memory, with its lowest index, inside the G lanes of the row
template <typename T, int VEC, bool ONE>
__device__ __forceinline__ void kd_row_max(const T* __restrict__ zr, bool active, int K, int G, int lane, float* v, float& bv, int& bi) {
    bv = -INFINITY;
    bi = INT32_MAX;
    if constexpr (ONE) {
#pragma unroll
        for (int c = 0; c < CE_PER_LANE / VEC; ++c) {
            const int k0 = (c * G + lane) * VEC;                 // (K % VEC == 0: an access lies wholly inside the row or outside)
            if (active && k0 < K) PV<T, VEC>::ld(zr + k0, v + c * VEC);
            else
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[c * VEC + e] = -INFINITY;
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (k0 + e < K) ce_take(bv, bi, v[c * VEC + e], k0 + e);
        }
    } else {
        if (active)
            for (int k0 = lane * VEC; k0 < K; k0 += G * VEC) {
                PV<T, VEC>::ld(zr + k0, v);
#pragma unroll
                for (int e = 0; e < VEC; ++e) ce_take(bv, bi, v[e], k0 + e);
            }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, WAVE);
        const int oi = __shfl_xor(bi, o, WAVE);
        ce_take(bv, bi, ov, oi);
    }
}

// one element's share of the four sums: S (z_s at temperature 1), SS, ST and W
__device__ __forceinline__ void kd_add(float zs, float zt, int k, int is, int it, double ms, double mt, double inv_T, double& S, double& SS,
                                       double& ST, double& W) {
    const double ds0 = (double)zs - ms, ds = ds0 * inv_T, dt = ((double)zt - mt) * inv_T;
    if (k != is) {
        S += exp(ds0);
        SS += exp(ds);
    }
    const double et = k != it ? exp(dt) : 1.0;
    if (k != it) ST += et;
    if (et != 0.0) W += et * (dt - ds);                          // (p_t = 0: the term counts 0, whatever log p_s is)
}

template <typename TS, typename TT, int VEC, bool ONE>
__global__ __launch_bounds__(CE_THREADS) void kd_rows_kernel(const TS* __restrict__ z_s, const TT* __restrict__ z_t,
                                                             const long long* __restrict__ labels, int B, int K, int G, double inv_T,
                                                             double* __restrict__ saved, double* __restrict__ row_ce,
                                                             double* __restrict__ row_kl, int* __restrict__ row_flag) {
    const int tid = threadIdx.x, lane = tid & (G - 1);
    const int r = blockIdx.x * (CE_THREADS / G) + tid / G;
    const bool active = r < B;                                   // (no early return: every lane of a wave takes part in the shuffles)
    const TS* sr = z_s + (size_t)(active ? r : 0) * K;
    const TT* tr = z_t + (size_t)(active ? r : 0) * K;
    float vs[CE_PER_LANE], vt[CE_PER_LANE];
    float bs, bt;
    int is, it;
    kd_row_max<TS, VEC, ONE>(sr, active, K, G, lane, vs, bs, is);
    kd_row_max<TT, VEC, ONE>(tr, active, K, G, lane, vt, bt, it);
    const double ms = (double)bs, mt = (double)bt;
    double S = 0.0, SS = 0.0, ST = 0.0, W = 0.0;
    if constexpr (ONE) {
#pragma unroll
        for (int c = 0; c < CE_PER_LANE / VEC; ++c) {
            const int k0 = (c * G + lane) * VEC;
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (k0 + e < K) kd_add(vs[c * VEC + e], vt[c * VEC + e], k0 + e, is, it, ms, mt, inv_T, S, SS, ST, W);
        }
    } else {
        if (active)
            for (int k0 = lane * VEC; k0 < K; k0 += G * VEC) {
                PV<TS, VEC>::ld(sr + k0, vs);
                PV<TT, VEC>::ld(tr + k0, vt);
#pragma unroll
                for (int e = 0; e < VEC; ++e) kd_add(vs[e], vt[e], k0 + e, is, it, ms, mt, inv_T, S, SS, ST, W);
            }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {
        S += __shfl_xor(S, o, WAVE);
        SS += __shfl_xor(SS, o, WAVE);
        ST += __shfl_xor(ST, o, WAVE);
        W += __shfl_xor(W, o, WAVE);
    }
    if (!active || lane != 0) return;
    const int pred = is < K ? is : 0;                            // (a row of NaNs has no maximum: its sums are NaN)
    const double l1 = log1p(S), l1s = log1p(SS), l1t = log1p(ST);
    const long long y = labels[r];
    const bool valid = y >= 0 && y < (long long)K;
    int flag = valid ? KD_VALID : (y == CE_IGNORE ? 0 : KD_BAD);
    double ce = 0.0;
    if (valid) {
        ce = l1 + (ms - (double)ld1<TS>(sr + (int)y));
        if ((int)y == pred) flag |= KD_HIT;
    }
    saved[r] = ms + l1;
    saved[B + r] = ms * inv_T + l1s;
    saved[2 * B + r] = mt * inv_T + l1t;
    row_ce[r] = ce;
    row_kl[r] = W / (1.0 + ST) + (l1s - l1t);
    row_flag[r] = flag;
}

__global__ __launch_bounds__(CE_THREADS) void kd_finalize_kernel(const double* __restrict__ row_ce, const double* __restrict__ row_kl,
                                                                 const int* __restrict__ row_flag, int B, double T,
                                                                 float* __restrict__ out, double* __restrict__ inv_n) {
    __shared__ double lc[CE_THREADS], lk[CE_THREADS];
    __shared__ int lh[CE_THREADS], lv[CE_THREADS], lb[CE_THREADS];
    const int tid = threadIdx.x, chunk = (B + CE_THREADS - 1) / CE_THREADS;
    const int beg = min(B, tid * chunk), end = min(B, beg + chunk);
    double u = 0.0, q = 0.0;
    int hits = 0, nv = 0, nb = 0;
    for (int r = beg; r < end; ++r) {
        const int f = row_flag[r];
        if (f & KD_VALID) {
            u += row_ce[r];
            ++nv;
            hits += (f & KD_HIT) ? 1 : 0;
        }
        nb += (f & KD_BAD) ? 1 : 0;
        q += row_kl[r];                                                         // (the KL term does not look at labels)
    }
    lc[tid] = u; lk[tid] = q; lh[tid] = hits; lv[tid] = nv; lb[tid] = nb;
    __syncthreads();
    if (tid != 0) return;
    double w = 0.0, d = 0.0;
    int h = 0, n = 0, b = 0;
    for (int i = 0; i < CE_THREADS; ++i) { w += lc[i]; d += lk[i]; h += lh[i]; n += lv[i]; b += lb[i]; }
    out[0] = b > 0 ? __builtin_nanf("") : (float)(w / (double)n);              // (n = 0: 0 / 0 = NaN, as nn.CrossEntropyLoss)
    out[1] = (float)(T * T * d / (double)B);
    out[2] = (float)(100.0 * (double)h / (double)B);                            // (helper/util.accuracy divides by the batch size)
    *inv_n = 1.0 / (double)n;                                                   // (n = 0: no row reads it)
}

template <typename TS, typename TT, int VEC>
__global__ __launch_bounds__(CE_THREADS) void kd_bwd_kernel(const TS* __restrict__ z_s, const TT* __restrict__ z_t,
                                                            const long long* __restrict__ labels, const double* __restrict__ saved,
                                                            const float* __restrict__ g_cls, const float* __restrict__ g_div,
                                                            TS* __restrict__ dz, int B, int K, double inv_T, double T_over_B) {
    const size_t at = ((size_t)blockIdx.x * CE_THREADS + threadIdx.x) * VEC;     // (K % VEC == 0: the VEC elements share a row)
    if (at >= (size_t)B * K) return;
    const int r = (int)(at / K), k0 = (int)(at % K);
    const long long y = labels[r];
    const bool with_cls = g_cls != nullptr && y >= 0 && y < (long long)K, with_div = g_div != nullptr;
    float vs[VEC], vt[VEC];
    double acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
    if (with_cls || with_div) PV<TS, VEC>::ld(z_s + at, vs);
    if (with_cls) {
        const double l = saved[r], f = saved[3 * (size_t)B], g = (double)*g_cls;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = (exp((double)vs[e] - l) - (k0 + e == (int)y ? 1.0 : 0.0)) * f * g;
    }
    if (with_div) {
        PV<TT, VEC>::ld(z_t + at, vt);
        const double ls = saved[B + r], lt = saved[2 * (size_t)B + r], g = (double)*g_div;
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            acc[e] += (exp((double)vs[e] * inv_T - ls) - exp((double)vt[e] * inv_T - lt)) * T_over_B * g;
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) vs[e] = round_f32(acc[e]);
    PV<TS, VEC>::st(dz + at, vs);
}

// the width both operands allow
template <typename TS, typename TT> int kd_vec(int K, uintptr_t low_s, uintptr_t low_t) {
    const int a = ce_vec<TS>(K, low_s), b = ce_vec<TT>(K, low_t);
    return a < b ? a : b;
}
template <typename TS, typename TT> constexpr int KD_MAXVEC = MAXVEC<TS> < MAXVEC<TT> ? MAXVEC<TS> : MAXVEC<TT>;

}  // namespace

// the workspace: the rows' CE and KL terms in double, then their flags
size_t kdhead_workspace_bytes(int B) { return (size_t)B * 2 * sizeof(double) + (((size_t)B * sizeof(int) + 7) & ~(size_t)7); }

hipError_t launch_kdhead_fwd(const void* z_s, const void* z_t, const int64_t* labels, int B, int K, int dt_s, int dt_t, float T,
                             void* workspace, float* out, double* saved, hipStream_t st) {
    double* row_ce = (double*)workspace;
    double* row_kl = row_ce + B;
    int* row_flag = (int*)(row_kl + B);
    const int G = ce_lanes(K);
    const dim3 grid(ceil_div(B, CE_THREADS / G));
    const double inv_T = 1.0 / (double)T;
    with_dtype(dt_s, [&](auto ts) {
        using TS = typename decltype(ts)::type;
        with_dtype(dt_t, [&](auto tt) {
            using TT = typename decltype(tt)::type;
            with_vec<KD_MAXVEC<TS, TT>, 8, 4, 1>(kd_vec<TS, TT>(K, (uintptr_t)z_s, (uintptr_t)z_t), [&](auto vec) {
                constexpr int VEC = decltype(vec)::value;
                if (K <= CE_ONE_WALK)
                    hipLaunchKernelGGL((kd_rows_kernel<TS, TT, VEC, true>), grid, dim3(CE_THREADS), 0, st, (const TS*)z_s, (const TT*)z_t,
                                       (const long long*)labels, B, K, G, inv_T, saved, row_ce, row_kl, row_flag);
                else
                    hipLaunchKernelGGL((kd_rows_kernel<TS, TT, VEC, false>), grid, dim3(CE_THREADS), 0, st, (const TS*)z_s, (const TT*)z_t,
                                       (const long long*)labels, B, K, G, inv_T, saved, row_ce, row_kl, row_flag);
            });
            return 0;
        });
        return 0;
    });
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(kd_finalize_kernel, dim3(1), dim3(CE_THREADS), 0, st, (const double*)row_ce, (const double*)row_kl,
                       (const int*)row_flag, B, (double)T, out, saved + 3 * (size_t)B);
    return hipGetLastError();
}

hipError_t launch_kdhead_bwd(const void* z_s, const void* z_t, const int64_t* labels, const double* saved, const float* g_cls,
                             const float* g_div, void* dz, int B, int K, int dt_s, int dt_t, float T, hipStream_t st) {
    const double inv_T = 1.0 / (double)T, T_over_B = (double)T / (double)B;
    with_dtype(dt_s, [&](auto ts) {
        using TS = typename decltype(ts)::type;
        with_dtype(dt_t, [&](auto tt) {
            using TT = typename decltype(tt)::type;
            with_vec<KD_MAXVEC<TS, TT>, 8, 4, 1>(kd_vec<TS, TT>(K, (uintptr_t)z_s | (uintptr_t)dz, (uintptr_t)z_t), [&](auto vec) {
                constexpr int VEC = decltype(vec)::value;
                const size_t threads = (size_t)B * K / VEC;
                hipLaunchKernelGGL((kd_bwd_kernel<TS, TT, VEC>), dim3((unsigned)((threads + CE_THREADS - 1) / CE_THREADS)),
                                   dim3(CE_THREADS), 0, st, (const TS*)z_s, (const TT*)z_t, (const long long*)labels, saved, g_cls, g_div,
                                   (TS*)dz, B, K, inv_T, T_over_B);
            });
            return 0;
        });
        return 0;
    });
    return hipGetLastError();
}

}  // namespace moma
