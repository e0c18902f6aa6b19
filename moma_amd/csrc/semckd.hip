// Cross-Layer Distillation with Semantic Calibration (`--distill semckd`; reference distiller_zoo/SemCKD.py, models/util.py SelfA): the
// tail behind the projections -- the per-sample mean squared error of EVERY (student map i, teacher map j) pair, weighted by the
// attention w [B,S,T] -- as ONE grouped forward call and ONE grouped backward call over all pairs p = i T + j (n_pairs <= 64):
//     ind[b,p]  = (1/n_p) sum_k (x_p[b,k] - t_p[b,k])^2          loss = (1/(B S)) sum_b sum_p w[b,p] ind[b,p]
//     dx_p[b,k] = g 2 w[b,p] / (n_p B S) (x_p[b,k] - t_p[b,k])   (dw = g ind / (B S) is a stock multiply of ind by the caller)
// Both maps of a pair lie in the same memory format, so each side is read in storage order as [B, n_p] rows (the sum of squares does
// not depend on the order of the columns); storage fp32 or bf16 per side and per pair.
//   The work list: the pairs differ widely in n_p (64 x between the 56 x 56 and the 7 x 7 grids of EfficientNet-B0), so the work is
//             not a grid over (pair, sample) but a flat list of ITEMS (pair p, sample b, chunk c of SEMCKD_CHUNK elements), item =
//             first_p + b nchunk_p + c with first_p the prefix sum of B nchunk_p that the host fills into the kernel's argument
//             table.  Workgroups stride over the list (at most SEMCKD_MAX_GRID of them); a workgroup finds the pair of its item by a
//             binary search of the prefix table, which is uniform over the workgroup.  What an item computes depends on the item
//             alone, never on the grid.
//   semckd_fwd       per item: thread i walks vectors i, i + 256, ... of the chunk; difference and square in fp32, the thread's sum,
//             the workgroup's sum (block_sum of batchrel.hpp: a fixed order) in DOUBLE -> one double partial per item.
//   semckd_finalize  ONE workgroup of 1024 threads: thread i adds the nchunk_p partials of the entries (b,p) = i, i + 1024, ... in
//             chunk order -> ind[b,p] (fp32) and its term w[b,p] ind[b,p] in double (from the unrounded double ind); the terms are
//             added per thread in order, then butterfly per wave, then the waves in order -> loss (fp32).
//   semckd_bwd       the same list; per item the factor g 2 w[b,p] / (n_p B S) in double (g a DEVICE scalar), dx = round_f32(double(x - t)
//             factor) in x's dtype.  Items of a pair whose dx is null are skipped.  No reduction.
// 16-byte accesses (two for 8 fp32) where the base addresses of a pair and n_p allow, 4 elements where only that divides, element
// accesses otherwise -- chosen per pair.  No atomics: bitwise repeatable.
// hipcc -O3, gfx950 (resource report, -Rpass-analysis=kernel-resource-usage): fwd 50 VGPRs, 32 B of LDS; finalize 26 VGPRs, 128 B;
// bwd 48 VGPRs, no LDS.  No kernel spills, none uses scratch (the argument table stays in the kernarg segment).
#include "batchrel.hpp"

namespace moma {
namespace {

constexpr int SEMCKD_CHUNK = MOMA_SEMCKD_CHUNK;
constexpr int SEMCKD_MAX_GRID = 4096;        // 256 compute units x 16 workgroups
constexpr int SEMCKD_FIN_THREADS = 1024;
static_assert(SEMCKD_CHUNK % (REL_THREADS * 8) == 0, "a chunk is whole vectors for the whole workgroup");

struct SemPair {
    const void* x;
    const void* t;
    void* dx;
    long long n;                             // elements of one sample
    long long first;                         // items in front of this pair
    int nchunk;                              // ceil(n / SEMCKD_CHUNK)
    int code;                                // dtype_x | dtype_t << 1 | vec << 2
};
struct SemTable {                            // the kernels' argument: 48 bytes per pair, 3 KB
    SemPair p[MOMA_SEMCKD_MAX_PAIRS];
    long long items;
    int n_pairs, B;
    double inv_bs;                           // 1 / (B S)
};

// the pair of item `it`: the last p with first_p <= it (uniform over the workgroup)
__device__ __forceinline__ int semckd_find(const SemTable& tb, long long it) {
    int lo = 0, hi = tb.n_pairs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tb.p[mid].first <= it) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// one item: elements [e0, e0 + len) of a row.  BWD: dx = round_f32(double(x - t) coef); else the thread's sum of squares
template <typename TX, typename TT, int V, bool BWD>
__device__ __forceinline__ double semckd_item(const TX* __restrict__ x, const TT* __restrict__ t, TX* __restrict__ dx, int len,
                                              double coef) {
    double s = 0.0;
    for (int e = threadIdx.x * V; e < len; e += REL_THREADS * V) {                 // (n % V == 0: all V inside)
        float xv[V], tv[V];
        PV<TX, V>::ld(x + e, xv);
        PV<TT, V>::ld(t + e, tv);
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const float d = xv[u] - tv[u];
            if constexpr (BWD) xv[u] = round_f32((double)d * coef);
            else s += (double)(d * d);
        }
        if constexpr (BWD) PV<TX, V>::st(dx + e, xv);
    }
    return s;
}

// code -> the instantiation, by the dispatchers the host uses elsewhere
template <bool BWD>
__device__ __forceinline__ double semckd_dispatch(const SemPair& q, size_t at, int len, double coef) {
    double s = 0.0;
    with_dtype(q.code & 1, [&](auto tx) {
        return with_dtype((q.code >> 1) & 1, [&](auto tt) {
            using TX = typename decltype(tx)::type;
            using TT = typename decltype(tt)::type;
            with_vec<8, 8, 4, 1>(q.code >> 2, [&](auto w) {
                constexpr int V = decltype(w)::value;
                s = semckd_item<TX, TT, V, BWD>((const TX*)q.x + at, (const TT*)q.t + at, BWD ? (TX*)q.dx + at : nullptr, len, coef);
            });
            return 0;
        });
    });
    return s;
}

__global__ __launch_bounds__(REL_THREADS) void semckd_fwd_kernel(const SemTable tb, double* __restrict__ partials) {
    __shared__ double sh[4];
    for (long long it = blockIdx.x; it < tb.items; it += gridDim.x) {
        const int p = semckd_find(tb, it);
        const SemPair& q = tb.p[p];
        const long long r = it - q.first;
        const int b = (int)(r / q.nchunk), c = (int)(r % q.nchunk);
        const long long e0 = (long long)c * SEMCKD_CHUNK;
        const int len = (int)(q.n - e0 < SEMCKD_CHUNK ? q.n - e0 : SEMCKD_CHUNK);
        const double s = block_sum(semckd_dispatch<false>(q, (size_t)b * q.n + e0, len, 0.0), sh);
        if (threadIdx.x == 0) partials[it] = s;
    }
}

// one workgroup.  ind is [B, n_pairs]: entry = b n_pairs + p
__global__ __launch_bounds__(SEMCKD_FIN_THREADS) void semckd_finalize_kernel(const SemTable tb, const double* __restrict__ partials,
                                                                             const float* __restrict__ w, float* __restrict__ ind,
                                                                             float* __restrict__ loss) {
    __shared__ double sh[SEMCKD_FIN_THREADS / 64];
    const long long entries = (long long)tb.B * tb.n_pairs;
    double term = 0.0;
    for (long long i = threadIdx.x; i < entries; i += SEMCKD_FIN_THREADS) {
        const int b = (int)(i / tb.n_pairs), p = (int)(i % tb.n_pairs);
        const SemPair& q = tb.p[p];
        const double* pp = partials + q.first + (long long)b * q.nchunk;
        double u = 0.0;
        for (int c = 0; c < q.nchunk; ++c) u += pp[c];
        u /= (double)q.n;
        ind[i] = (float)u;
        term += (double)w[i] * u;
    }
    term = wave_sum(term);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) {
        double u = 0.0;
        for (int z = 0; z < SEMCKD_FIN_THREADS / 64; ++z) u += sh[z];
        *loss = (float)(u * tb.inv_bs);
    }
}

__global__ __launch_bounds__(REL_THREADS) void semckd_bwd_kernel(const SemTable tb, const float* __restrict__ w,
                                                                 const float* __restrict__ g_loss) {
    const double g2 = 2.0 * (double)*g_loss * tb.inv_bs;
    for (long long it = blockIdx.x; it < tb.items; it += gridDim.x) {
        const int p = semckd_find(tb, it);
        const SemPair& q = tb.p[p];
        if (q.dx == nullptr) continue;                                             // (uniform over the workgroup)
        const long long r = it - q.first;
        const int b = (int)(r / q.nchunk), c = (int)(r % q.nchunk);
        const long long e0 = (long long)c * SEMCKD_CHUNK;
        const int len = (int)(q.n - e0 < SEMCKD_CHUNK ? q.n - e0 : SEMCKD_CHUNK);
        const double coef = g2 * (double)w[(size_t)b * tb.n_pairs + p] / (double)q.n;
        semckd_dispatch<true>(q, (size_t)b * q.n + e0, len, coef);
    }
}

long long semckd_chunks(long long n) { return (n + SEMCKD_CHUNK - 1) / SEMCKD_CHUNK; }

SemTable semckd_table(const moma_semckd_pair_t* pairs, int n_pairs, int S, int B, bool with_dx) {
    SemTable tb{};
    long long first = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const moma_semckd_pair_t& a = pairs[p];
        int v = min(side_vec(a.x, a.n, a.dtype_x), side_vec(a.t, a.n, a.dtype_t));
        if (with_dx && a.dx) v = min(v, side_vec(a.dx, a.n, a.dtype_x));
        tb.p[p] = SemPair{a.x, a.t, with_dx ? a.dx : nullptr, a.n, first, (int)semckd_chunks(a.n),
                          (a.dtype_x == MOMA_DT_BF16 ? 1 : 0) | (a.dtype_t == MOMA_DT_BF16 ? 2 : 0) | (v << 2)};
        first += (long long)B * tb.p[p].nchunk;
    }
    tb.items = first;
    tb.n_pairs = n_pairs;
    tb.B = B;
    tb.inv_bs = 1.0 / ((double)B * S);
    return tb;
}

}  // namespace

// one double per item
size_t semckd_workspace_bytes(const moma_semckd_pair_t* pairs, int n_pairs, int B) {
    long long items = 0;
    for (int p = 0; p < n_pairs; ++p) items += (long long)B * semckd_chunks(pairs[p].n);
    return (size_t)items * sizeof(double);
}

hipError_t launch_semckd_fwd(const moma_semckd_pair_t* pairs, int n_pairs, int S, int B, const float* w, double* partials, float* ind,
                             float* loss, hipStream_t st) {
    const SemTable tb = semckd_table(pairs, n_pairs, S, B, false);
    const unsigned grid = (unsigned)min(tb.items, (long long)SEMCKD_MAX_GRID);
    hipLaunchKernelGGL(semckd_fwd_kernel, dim3(grid), dim3(REL_THREADS), 0, st, tb, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(semckd_finalize_kernel, dim3(1), dim3(SEMCKD_FIN_THREADS), 0, st, tb, (const double*)partials, w, ind, loss);
    return hipGetLastError();
}

hipError_t launch_semckd_bwd(const moma_semckd_pair_t* pairs, int n_pairs, int S, int B, const float* w, const float* g_loss,
                             hipStream_t st) {
    const SemTable tb = semckd_table(pairs, n_pairs, S, B, true);
    const unsigned grid = (unsigned)min(tb.items, (long long)SEMCKD_MAX_GRID);
    hipLaunchKernelGGL(semckd_bwd_kernel, dim3(grid), dim3(REL_THREADS), 0, st, tb, w, g_loss);
    return hipGetLastError();
}

}  // namespace moma
