// The classification head of the teacher trainer (`train_teacher.py`; reference helper/loops_moma.py:13-65 and the validation that ends
// at :444): nn.CrossEntropyLoss, helper/util.accuracy (top-1) and the confusion matrix of process_accumulated_output as two launches
// forward and one backward -- on logits z [B, K] (fp32 or bf16, dense) and labels [B] int64:
//     m_b = max_k z[b,k]      pred_b = the LOWEST k with z[b,k] = m_b      T_b = sum_{k != pred_b} exp(z[b,k] - m_b)
//     lse_b = m_b + log1p(T_b)                 row_b = log1p(T_b) + (m_b - z[b,y_b])          (a valid row: 0 <= y_b < K)
//     loss = sum_valid row_b / n_valid         hit_b = [pred_b == y_b]
//     dz[b,k] = g_loss (exp(z[b,k] - lse_b) - [k == y_b]) / n_valid                          (a row that is not valid: exact zeros)
// The sum leaves out the term of the maximum itself (it is exactly 1) and log1p adds it back: where the label's logit dominates, row_b
// is log1p of a small sum and not the logarithm of a sum that has already rounded to 1.  Every sum, the logarithm and both exponentials
// are double (ocml's exp / log1p: the fast fp32 intrinsic's 2^-21 would use the whole allowance of the tests by itself; z - m is exact
// in double), so lse is kept in double too: an fp32 lse near 5 is uncertain by 2.4e-7, which exp(z - lse) hands on to every
// probability of the row.
//   ce_rows_kernel<T, VEC, ONE>   256 threads; G lanes per row, G the power of two (1 .. 64) that covers ceil(K / 16), so 256 / G rows
//             per workgroup: a 4-class head takes one lane per row, not a wave.  ONE (K <= 16 G <= 1024): the row is read ONCE, 16
//             elements per lane in registers as 16 / VEC accesses of VEC elements (lane l takes the accesses l, l + G, ...); the
//             maximum and its lowest index by xor shuffles inside the G lanes, then the sum of exponentials from the registers.
//             !ONE (longer rows; G = 64): two walks over the row, the same arithmetic.  VEC (8, 4 or 1 elements, at most 16 bytes) is
//             common.hpp's pick_vec over K and the base address, so K = 5 in fp32 (rows on 20-byte boundaries) takes the element
//             accesses.  Lane 0 of a row writes lse, pred, the row's loss and its flags (valid / hit / bad label) to the workspace.  A
//             label outside [0, K) is never used as an index.
//   ce_finalize_kernel            ONE workgroup: thread t adds the rows [t c, (t + 1) c), c = ceil(B / 256), in row order in double and
//             counts them; thread 0 adds the 256 sums in order -> loss (rounded once; NaN without a valid row, as torch, and with a bad
//             label), 1 / n_valid, stats += (sum of valid row losses, hits, valid rows, bad labels).  conf[y_b, pred_b] += 1 per valid
//             row by integer vector atomics (exact in any order).  No floating-point atomics: bitwise repeatable.
//   ce_bwd_kernel<T, VEC>         one thread per VEC elements of dz; no reduction.  g_loss is a DEVICE scalar multiplied in double before
//             the one rounding to fp32 (and, for bf16, one more to the storage type): a power of two scales every bit pattern exactly.
// hipcc -O3, gfx950 (-Rpass-analysis=kernel-resource-usage): see DESIGN.md, section CE; no kernel spills, none uses scratch.
#include "rowhead.hpp"

namespace moma {
namespace {

// (rowhead.hpp: CE_THREADS, CE_PER_LANE, CE_ONE_WALK, CE_IGNORE, ce_lanes, ce_take, ce_vec -- shared with kdhead.hip)
static_assert(CE_ONE_WALK == MOMA_CE_ONE_WALK_K, "header and kernel agree on the one-walk limit");
constexpr int CE_VALID = 1, CE_HIT = 2, CE_BAD = 4;

template <typename T, int VEC, bool ONE>
__global__ __launch_bounds__(CE_THREADS) void ce_rows_kernel(const T* __restrict__ z, const long long* __restrict__ labels, int B, int K,
                                                             int G, double* __restrict__ lse, double* __restrict__ row_loss,
                                                             int* __restrict__ row_pred, int* __restrict__ row_flag,
                                                             int* __restrict__ pred_out) {
    const int tid = threadIdx.x, lane = tid & (G - 1);
    const int r = blockIdx.x * (CE_THREADS / G) + tid / G;
    const bool active = r < B;                                   // (no early return: every lane of a wave takes part in the shuffles)
    const T* zr = z + (size_t)(active ? r : 0) * K;
    float v[CE_PER_LANE];
    float bv = -INFINITY;
    int bi = INT32_MAX;
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
    const int pred = bi < K ? bi : 0;                            // (a row of NaNs has no maximum: its sum below is NaN)
    const double m = (double)bv;
    double s = 0.0;
    if constexpr (ONE) {
#pragma unroll
        for (int c = 0; c < CE_PER_LANE / VEC; ++c) {
            const int k0 = (c * G + lane) * VEC;
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (k0 + e < K && k0 + e != bi) s += exp((double)v[c * VEC + e] - m);
        }
    } else {
        if (active)
            for (int k0 = lane * VEC; k0 < K; k0 += G * VEC) {
                PV<T, VEC>::ld(zr + k0, v);
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (k0 + e != bi) s += exp((double)v[e] - m);
            }
    }
    for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, WAVE);
    if (!active || lane != 0) return;
    const double l1p = log1p(s);
    const long long y = labels[r];
    const bool valid = y >= 0 && y < (long long)K;
    int flag = valid ? CE_VALID : (y == CE_IGNORE ? 0 : CE_BAD);
    double row = 0.0;
    if (valid) {
        row = l1p + (m - (double)ld1<T>(zr + (int)y));
        if ((int)y == pred) flag |= CE_HIT;
    }
    lse[r] = m + l1p;
    row_loss[r] = row;
    row_pred[r] = pred;
    row_flag[r] = flag;
    if (pred_out) pred_out[r] = pred;
}

__global__ __launch_bounds__(CE_THREADS) void ce_finalize_kernel(const double* __restrict__ row_loss, const int* __restrict__ row_pred,
                                                                 const int* __restrict__ row_flag, const long long* __restrict__ labels,
                                                                 int B, int K, float* __restrict__ loss, double* __restrict__ inv_n,
                                                                 double* __restrict__ stats, unsigned long long* __restrict__ conf) {
    __shared__ double ls[CE_THREADS];
    __shared__ int lh[CE_THREADS], lv[CE_THREADS], lb[CE_THREADS];
    const int tid = threadIdx.x, chunk = (B + CE_THREADS - 1) / CE_THREADS;
    const int beg = min(B, tid * chunk), end = min(B, beg + chunk);
    double u = 0.0;
    int hits = 0, nv = 0, nb = 0;
    for (int r = beg; r < end; ++r) {
        const int f = row_flag[r];
        if (f & CE_VALID) {
            u += row_loss[r];
            ++nv;
            hits += (f & CE_HIT) ? 1 : 0;
            if (conf) atomicAdd(conf + (size_t)labels[r] * K + row_pred[r], 1ULL);       // (valid: 0 <= label < K; 0 <= pred < K)
        }
        nb += (f & CE_BAD) ? 1 : 0;
    }
    ls[tid] = u; lh[tid] = hits; lv[tid] = nv; lb[tid] = nb;
    __syncthreads();
    if (tid != 0) return;
    double w = 0.0;
    int h = 0, n = 0, b = 0;
    for (int i = 0; i < CE_THREADS; ++i) { w += ls[i]; h += lh[i]; n += lv[i]; b += lb[i]; }
    *loss = b > 0 ? __builtin_nanf("") : (float)(w / (double)n);              // (n = 0: 0 / 0 = NaN, as nn.CrossEntropyLoss)
    *inv_n = 1.0 / (double)n;                                                   // (n = 0: no row reads it)
    if (stats) {
        stats[0] += w;
        stats[1] += (double)h;
        stats[2] += (double)n;
        stats[3] += (double)b;
    }
}

template <typename T, int VEC>
__global__ __launch_bounds__(CE_THREADS) void ce_bwd_kernel(const T* __restrict__ z, const long long* __restrict__ labels,
                                                            const double* __restrict__ lse, const double* __restrict__ inv_n,
                                                            const float* __restrict__ g_loss, T* __restrict__ dz, int B, int K) {
    const size_t at = ((size_t)blockIdx.x * CE_THREADS + threadIdx.x) * VEC;     // (K % VEC == 0: the VEC elements share a row)
    if (at >= (size_t)B * K) return;
    const int r = (int)(at / K), k0 = (int)(at % K);
    const long long y = labels[r];
    float v[VEC];
    if (y >= 0 && y < (long long)K) {
        PV<T, VEC>::ld(z + at, v);
        const double l = lse[r], f = *inv_n, g = (double)*g_loss;
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = round_f32((exp((double)v[e] - l) - (k0 + e == (int)y ? 1.0 : 0.0)) * f * g);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = 0.f;
    }
    PV<T, VEC>::st(dz + at, v);
}

}  // namespace

// the workspace: the rows' losses in double, then their predictions and flags
size_t ce_workspace_bytes(int B) { return (size_t)B * (sizeof(double) + 2 * sizeof(int)); }

hipError_t launch_ce_fwd(const void* z, const int64_t* labels, int B, int K, int dtype, void* workspace, float* loss, double* lse,
                         double* inv_n, int32_t* pred, double* stats, int64_t* conf, hipStream_t st) {
    double* row_loss = (double*)workspace;
    int* row_pred = (int*)(row_loss + B);
    int* row_flag = row_pred + B;
    const int G = ce_lanes(K);
    const dim3 grid(ceil_div(B, CE_THREADS / G));
    with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        with_vec<MAXVEC<T>, 8, 4, 1>(ce_vec<T>(K, (uintptr_t)z), [&](auto vec) {
            constexpr int VEC = decltype(vec)::value;
            if (K <= CE_ONE_WALK)
                hipLaunchKernelGGL((ce_rows_kernel<T, VEC, true>), grid, dim3(CE_THREADS), 0, st, (const T*)z, (const long long*)labels, B,
                                   K, G, lse, row_loss, row_pred, row_flag, pred);
            else
                hipLaunchKernelGGL((ce_rows_kernel<T, VEC, false>), grid, dim3(CE_THREADS), 0, st, (const T*)z, (const long long*)labels, B,
                                   K, G, lse, row_loss, row_pred, row_flag, pred);
        });
        return 0;
    });
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(CE_THREADS), 0, st, (const double*)row_loss, (const int*)row_pred,
                       (const int*)row_flag, (const long long*)labels, B, K, loss, inv_n, stats, (unsigned long long*)conf);
    return hipGetLastError();
}

hipError_t launch_ce_bwd(const void* z, const int64_t* labels, const double* lse, const double* inv_n, const float* g_loss, void* dz,
                         int B, int K, int dtype, hipStream_t st) {
    with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        with_vec<MAXVEC<T>, 8, 4, 1>(ce_vec<T>(K, (uintptr_t)z | (uintptr_t)dz), [&](auto vec) {
            constexpr int VEC = decltype(vec)::value;
            const size_t threads = (size_t)B * K / VEC;
            hipLaunchKernelGGL((ce_bwd_kernel<T, VEC>), dim3((unsigned)((threads + CE_THREADS - 1) / CE_THREADS)), dim3(CE_THREADS), 0, st,
                               (const T*)z, (const long long*)labels, lse, inv_n, g_loss, (T*)dz, B, K);
        });
        return 0;
    });
    return hipGetLastError();
}

}  // namespace moma
