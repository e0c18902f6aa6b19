// CRD (Contrastive Representation Distillation) over two n_data x d memory banks addressed by sample index (reference
// crd/memory.py:23-79, crd/criterion.py:57-74): one gather core in four modes -- statistics for Z, the fused loss + gradient pass,
// the materialised scores and their backward -- plus the fixed-order combine launches and the momentum update of the banks.
//
// The gather is latency bound (every (b, j) fetches one row of 4 d bytes from a random place of the bank), so the loop is built to
// keep loads in flight: a wave owns one b and a contiguous range of j, carries 64 / LPR rows side by side (LPR lanes per row, one
// 16-byte load per lane and 4 LPR columns), issues U such groups of row loads AND the indices of the next U groups before it
// consumes the first, and uses the row it still holds for the gradient accumulation: every bank row is fetched once per
// (b, j, side).  Arithmetic is plain fp32 FMA (each row meets exactly one vector: nothing for an MFMA); the per-wave sums that the
// second launch adds in a fixed order are kept in double where that is free (one add per row).  No atomics: bitwise repeatable.
#include "common.hpp"

namespace moma {
namespace {

enum { CRD_STATS = 0, CRD_FUSED = 1, CRD_SCORES = 2, CRD_SBWD = 3 };

struct CrdArgs {
    const float* v[2];       // side 0: v1 (student embedding), side 1: v2 (teacher embedding)               [B, d]
    const float* mem[2];     // side 0: memory_v2,              side 1: memory_v1                             [n_data, d]
    const int64_t* idx;      // [B, K1], column 0 = the sample's own index
    const float* Z;          // [2] normalisation constants (FUSED, SCORES)
    float* out[2];           // SCORES: x [B, K1] per side
    const float* dout[2];    // SBWD: gradient of the scores
    const float* xin[2];     // SBWD: the scores the forward wrote
    float* part_dv;          // [2, B, nchunk, d] per-wave slices of dv
    double* part_sum;        // [2, B, nchunk]    per-wave loss sums (FUSED) / sums of e (STATS)
    int32_t* bad;            // set to 1 when an index outside [0, n_data) was met
    int64_t n_data;
    int B, d, K1, nchunk, rpc, want_dv;
    float T, c, ce, eps, inv_B;   // c = nce_k / n_data, ce = c + eps
};

template <int LPR>
__device__ __forceinline__ float group_sum(float v) {      // sum over the LPR lanes of a row group, result in each of them
    if constexpr (LPR == 64) {
        v = half32_sum(v);
        return v + other_half(v);
    } else if constexpr (LPR == 32) {
        return half32_sum(v);
    } else {
        v += dpp_row<0x128>(v);
        v += dpp_row<0x124>(v);
        v += dpp_row<0x122>(v);
        v += dpp_row<0x121>(v);
        return v;
    }
}


// grid (ceil(nchunk / 4), B, 2 sides), 256 threads = 4 waves, one chunk of j each
template <int LPR, int VPL, int U, int MODE>
__global__ __launch_bounds__(256) void crd_gather_kernel(const CrdArgs a) {
    constexpr int R = 64 / LPR;                      // rows a wave carries side by side
    const int lane = threadIdx.x & 63;
    const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= a.nchunk) return;                   // (wave-uniform; no barrier in this kernel)
    const int b = blockIdx.y, side = blockIdx.z;
    const int g = lane / LPR, l = lane % LPR;
    const int d = a.d, d4 = d >> 2;
    const int jbeg = chunk * a.rpc;
    const int jend = min(a.K1, jbeg + a.rpc);
    const float* __restrict__ M = a.mem[side];
    const int64_t* __restrict__ idxb = a.idx + (int64_t)b * a.K1;
    const float* __restrict__ dob = MODE == CRD_SBWD ? a.dout[side] + (int64_t)b * a.K1 : nullptr;
    const float* __restrict__ xib = MODE == CRD_SBWD ? a.xin[side] + (int64_t)b * a.K1 : nullptr;

    bool act[VPL];
    f32x4 vr[VPL], acc[VPL];
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
        const int col4 = l + k * LPR;
        act[k] = col4 < d4;
        vr[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (MODE != CRD_SBWD && act[k]) vr[k] = *reinterpret_cast<const f32x4*>(a.v[side] + (int64_t)b * d + col4 * 4);
    }
    float Zs = 1.f;
    if (MODE == CRD_FUSED || MODE == CRD_SCORES) Zs = a.Z[side];
    double lsum = 0.0;

    // index (and, for the scores' backward, coefficient) of row slot u of the group of rows that starts at j0: -1 = nothing to
    // fetch (past the end of the chunk, or an index that is not a row of the bank: flagged, never turned into an address)
    int64_t cur[U];
    float cco[U];
#define CRD_LOAD_IDS(J0, IDS, CO)                                                      \
    _Pragma("unroll") for (int u = 0; u < U; ++u) {                                    \
        const int j = (J0) + u * R + g;                                                \
        int64_t id = -1;                                                               \
        float co = 0.f;                                                                \
        if (j < jend) {                                                                \
            id = idxb[j];                                                              \
            if (id < 0 || id >= a.n_data) {                                            \
                if (l == 0) *a.bad = 1;                                                \
                id = -1;                                                               \
            } else if (MODE == CRD_SBWD) {                                             \
                co = dob[j] * xib[j] / a.T;                                            \
            }                                                                          \
        }                                                                              \
        IDS[u] = id;                                                                   \
        CO[u] = co;                                                                    \
    }
    CRD_LOAD_IDS(jbeg, cur, cco)

    for (int j0 = jbeg; j0 < jend; j0 += R * U) {
        f32x4 row[U][VPL];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int k = 0; k < VPL; ++k) {
                row[u][k] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (cur[u] >= 0 && act[k]) row[u][k] = *reinterpret_cast<const f32x4*>(M + cur[u] * d + (l + k * LPR) * 4);
            }
        int64_t nxt[U];
        float nco[U];
        CRD_LOAD_IDS(j0 + R * U, nxt, nco)

        float s[U];
        if (MODE != CRD_SBWD) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float p = 0.f;
#pragma unroll
                for (int k = 0; k < VPL; ++k) {
                    p = fmaf(row[u][k].x, vr[k].x, p);
                    p = fmaf(row[u][k].y, vr[k].y, p);
                    p = fmaf(row[u][k].z, vr[k].z, p);
                    p = fmaf(row[u][k].w, vr[k].w, p);
                }
                s[u] = group_sum<LPR>(p);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * R + g;
            const bool ok = cur[u] >= 0;
            float coef = 0.f;
            if (MODE == CRD_STATS) {
                if (ok) lsum += (double)expf(s[u] / a.T);
            } else if (MODE == CRD_SCORES) {
                const float x = ok ? expf(s[u] / a.T) / Zs : 0.f;
                if (l == 0 && j < jend) a.out[side][(int64_t)b * a.K1 + j] = x;
            } else if (MODE == CRD_FUSED) {
                if (ok) {
                    const float x = expf(s[u] / a.T) / Zs;
                    float lt, gx;
                    if (j == 0) {            // log(x / (x + c + eps)),  g x = -(c + eps) / (x + c + eps)
                        lt = -log1pf(a.ce / x);
                        gx = -a.ce / (x + a.ce);
                    } else {                 // log(c / (x + c + eps)),  g x = x / (x + c + eps)
                        lt = -log1pf((x + a.eps) / a.c);
                        gx = x / (x + a.ce);
                    }
                    lsum += (double)lt;
                    coef = gx / a.T * a.inv_B;
                }
            } else {
                coef = cco[u];
            }
            if ((MODE == CRD_FUSED && a.want_dv) || MODE == CRD_SBWD) {
#pragma unroll
                for (int k = 0; k < VPL; ++k) {
                    acc[k].x = fmaf(coef, row[u][k].x, acc[k].x);
                    acc[k].y = fmaf(coef, row[u][k].y, acc[k].y);
                    acc[k].z = fmaf(coef, row[u][k].z, acc[k].z);
                    acc[k].w = fmaf(coef, row[u][k].w, acc[k].w);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cur[u] = nxt[u];
            cco[u] = nco[u];
        }
    }
#undef CRD_LOAD_IDS

    const int64_t slot = ((int64_t)side * a.B + b) * a.nchunk + chunk;
    if (MODE == CRD_STATS || MODE == CRD_FUSED) {
        const double t = wave_sum(l == 0 ? lsum : 0.0);        // every lane of a row group holds the same sum: count it once
        if (lane == 0) a.part_sum[slot] = t;
    }
    if ((MODE == CRD_FUSED && a.want_dv) || MODE == CRD_SBWD) {
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
#pragma unroll
            for (int o = LPR; o < 64; o <<= 1) {                   // the R row groups of the wave, in a fixed order
                acc[k].x += __shfl_xor(acc[k].x, o, 64);
                acc[k].y += __shfl_xor(acc[k].y, o, 64);
                acc[k].z += __shfl_xor(acc[k].z, o, 64);
                acc[k].w += __shfl_xor(acc[k].w, o, 64);
            }
            if (g == 0 && act[k]) *reinterpret_cast<f32x4*>(a.part_dv + slot * d + (l + k * LPR) * 4) = acc[k];
        }
    }
}

// sum of n doubles by one workgroup of 256 threads in an order that depends on n alone; result valid in thread 0
__device__ __forceinline__ double block_sum_f64(const double* __restrict__ p, int64_t n, double* sh) {
    double t = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) t += p[i];
    sh[threadIdx.x] = t;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// Z[side] = mean(e) * n_data (crd/memory.py:50-57) from the per-wave sums of the statistics pass.  grid (2)
__global__ __launch_bounds__(256) void crd_z_kernel(const double* __restrict__ part_sum, float* __restrict__ Z, int B, int K1,
                                                    int nchunk, int64_t n_data) {
    __shared__ double sh[256];
    const int64_t n = (int64_t)B * nchunk;
    const double t = block_sum_f64(part_sum + blockIdx.x * n, n, sh);
    if (threadIdx.x == 0) Z[blockIdx.x] = (float)(t / ((double)B * (double)K1) * (double)n_data);
}

// grid (B + 1, 2): blocks 0 .. B-1 add the nchunk slices of dv[b] in chunk order, block B the loss sums of the side
__global__ __launch_bounds__(256) void crd_combine_kernel(const float* __restrict__ part_dv, const double* __restrict__ part_sum,
                                                          float* __restrict__ dv1, float* __restrict__ dv2, float* __restrict__ loss,
                                                          int B, int d, int nchunk) {
    __shared__ double sh[256];
    const int side = blockIdx.y;
    if ((int)blockIdx.x == B) {
        if (loss == nullptr) return;
        const int64_t n = (int64_t)B * nchunk;
        const double t = block_sum_f64(part_sum + side * n, n, sh);
        if (threadIdx.x == 0) loss[side] = (float)(-t / (double)B);
        return;
    }
    float* __restrict__ dv = side == 0 ? dv1 : dv2;
    if (dv == nullptr) return;
    const int b = blockIdx.x;
    const float* __restrict__ p = part_dv + ((int64_t)side * B + b) * nchunk * d;
    for (int c = threadIdx.x; c < d; c += 256) {
        double t = 0.0;
        for (int k = 0; k < nchunk; ++k) t += (double)p[(int64_t)k * d + c];
        dv[(int64_t)b * d + c] = (float)t;
    }
}

// Momentum update of both banks (crd/memory.py:64-77): r = M[y_i] m + v_i (1 - m);  M[y_i] = r / sqrt(sum r^2).   grid (B, 2).
// It reads the PRE-update row.  A y that occurs again later in the batch is skipped: the last writer in batch order wins, as in a
// serial index_copy_, and no two workgroups touch the same row.  A y outside [0, n_data) is flagged and skipped.
__global__ __launch_bounds__(256) void crd_update_kernel(float* __restrict__ mem1, float* __restrict__ mem2,
                                                         const float* __restrict__ v1, const float* __restrict__ v2,
                                                         const int64_t* __restrict__ y, int B, int d, int64_t n_data, float m,
                                                         float om, int32_t* __restrict__ bad) {
    __shared__ float sh[4];
    const int i = blockIdx.x;
    const int64_t yi = y[i];
    if (yi < 0 || yi >= n_data) {                        // (block-uniform)
        if (threadIdx.x == 0) *bad = 1;
        return;
    }
    int later = 0;
    for (int k = i + 1 + threadIdx.x; k < B; k += 256) later |= (y[k] == yi);
    if (__syncthreads_or(later)) return;
    float* __restrict__ M = (blockIdx.y == 0 ? mem1 : mem2) + yi * d;
    const float* __restrict__ v = (blockIdx.y == 0 ? v1 : v2) + (int64_t)i * d;
    float r[8];                                          // d <= 2048
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = threadIdx.x + k * 256;
        r[k] = 0.f;
        if (c < d) r[k] = __fadd_rn(__fmul_rn(M[c], m), __fmul_rn(v[c], om));
        ss = fmaf(r[k], r[k], ss);
    }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float norm = sqrtf((sh[0] + sh[1]) + (sh[2] + sh[3]));
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = threadIdx.x + k * 256;
        if (c < d) M[c] = r[k] / norm;
    }
}

template <int MODE>
hipError_t launch_gather(const CrdArgs& a, hipStream_t st) {
    const dim3 grid((a.nchunk + 3) / 4, a.B, 2), block(256);
    const int d4 = a.d / 4;
#define CRD_L(LPR, VPL, U) hipLaunchKernelGGL((crd_gather_kernel<LPR, VPL, U, MODE>), grid, block, 0, st, a)
    if (d4 <= 16) CRD_L(16, 1, 4);
    else if (d4 <= 32) CRD_L(32, 1, 4);
    else switch ((d4 + 63) / 64) {
        case 1: CRD_L(64, 1, 4); break;
        case 2: CRD_L(64, 2, 4); break;
        case 3: CRD_L(64, 3, 2); break;
        case 4: CRD_L(64, 4, 2); break;
        case 5: CRD_L(64, 5, 2); break;
        case 6: CRD_L(64, 6, 2); break;
        case 7: CRD_L(64, 7, 2); break;
        default: CRD_L(64, 8, 2); break;
    }
#undef CRD_L
    return hipGetLastError();
}

struct CrdPlan {
    int nchunk, rpc;
    size_t off_sum, bytes;      // part_dv at 0, part_sum at off_sum
};

CrdPlan crd_plan(int B, int d, int K1) {
    // about 8192 waves over (side, b, chunk) -- 8 per SIMD of the 256 compute units -- but no wave with fewer than 64 rows
    long nc = (8192 + 2L * B - 1) / (2L * B);
    const long maxc = (K1 + 63) / 64;
    if (nc > maxc) nc = maxc;
    if (nc > 1024) nc = 1024;
    if (nc < 1) nc = 1;
    CrdPlan p;
    p.rpc = (int)((K1 + nc - 1) / nc);
    p.nchunk = (K1 + p.rpc - 1) / p.rpc;
    const size_t dv = (size_t)2 * B * p.nchunk * d * sizeof(float);
    p.off_sum = (dv + 255) / 256 * 256;
    p.bytes = p.off_sum + ((size_t)2 * B * p.nchunk * sizeof(double) + 255) / 256 * 256;
    return p;
}

CrdArgs crd_args(const float* v1, const float* v2, const float* memory_v1, const float* memory_v2, const int64_t* idx, int B,
                 int d, int K1, int64_t n_data, float T, const float* Z, int32_t* bad, void* ws) {
    const CrdPlan p = crd_plan(B, d, K1);
    CrdArgs a{};
    a.v[0] = v1; a.v[1] = v2;
    a.mem[0] = memory_v2; a.mem[1] = memory_v1;
    a.idx = idx; a.Z = Z; a.bad = bad; a.n_data = n_data;
    a.part_dv = (float*)ws;
    a.part_sum = (double*)((char*)ws + p.off_sum);
    a.B = B; a.d = d; a.K1 = K1; a.nchunk = p.nchunk; a.rpc = p.rpc; a.want_dv = 0;
    const double c = (double)(K1 - 1) / (double)n_data;
    a.T = T; a.c = (float)c; a.ce = (float)(c + 1e-7); a.eps = 1e-7f; a.inv_B = (float)(1.0 / (double)B);
    return a;
}

hipError_t crd_set_z(const CrdArgs& a, float* Z, hipStream_t st) {
    hipError_t e = launch_gather<CRD_STATS>(a, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crd_z_kernel, dim3(2), dim3(256), 0, st, a.part_sum, Z, a.B, a.K1, a.nchunk, a.n_data);
    return hipGetLastError();
}
}  // namespace

size_t crd_workspace_bytes(int B, int d, int K1) { return crd_plan(B, d, K1).bytes; }

hipError_t launch_crd_fused(const float* v1, const float* v2, const float* memory_v1, const float* memory_v2, const int64_t* idx,
                            int B, int d, int K1, int64_t n_data, float T, float* Z, int set_z, float* loss, float* dv1, float* dv2,
                            int32_t* bad, void* ws, hipStream_t st) {
    CrdArgs a = crd_args(v1, v2, memory_v1, memory_v2, idx, B, d, K1, n_data, T, Z, bad, ws);
    if (set_z) {
        hipError_t e = crd_set_z(a, Z, st);
        if (e != hipSuccess) return e;
    }
    a.want_dv = dv1 != nullptr;
    hipError_t e = launch_gather<CRD_FUSED>(a, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crd_combine_kernel, dim3(B + 1, 2), dim3(256), 0, st, a.part_dv, a.part_sum, dv1, dv2, loss, B, d, a.nchunk);
    return hipGetLastError();
}

hipError_t launch_crd_scores(const float* v1, const float* v2, const float* memory_v1, const float* memory_v2, const int64_t* idx,
                             int B, int d, int K1, int64_t n_data, float T, float* Z, int set_z, float* out_v1, float* out_v2,
                             int32_t* bad, void* ws, hipStream_t st) {
    CrdArgs a = crd_args(v1, v2, memory_v1, memory_v2, idx, B, d, K1, n_data, T, Z, bad, ws);
    if (set_z) {
        hipError_t e = crd_set_z(a, Z, st);
        if (e != hipSuccess) return e;
    }
    a.out[0] = out_v1; a.out[1] = out_v2;
    return launch_gather<CRD_SCORES>(a, st);
}

hipError_t launch_crd_scores_bwd(const float* dout_v1, const float* dout_v2, const float* out_v1, const float* out_v2,
                                 const float* memory_v1, const float* memory_v2, const int64_t* idx, int B, int d, int K1,
                                 int64_t n_data, float T, float* dv1, float* dv2, int32_t* bad, void* ws, hipStream_t st) {
    CrdArgs a = crd_args(nullptr, nullptr, memory_v1, memory_v2, idx, B, d, K1, n_data, T, nullptr, bad, ws);
    a.dout[0] = dout_v1; a.dout[1] = dout_v2;
    a.xin[0] = out_v1; a.xin[1] = out_v2;
    hipError_t e = launch_gather<CRD_SBWD>(a, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crd_combine_kernel, dim3(B + 1, 2), dim3(256), 0, st, a.part_dv, a.part_sum, dv1, dv2, (float*)nullptr, B, d,
                       a.nchunk);
    return hipGetLastError();
}

hipError_t launch_crd_update(float* memory_v1, float* memory_v2, const float* v1, const float* v2, const int64_t* y, int B, int d,
                             int64_t n_data, float momentum, int32_t* bad, hipStream_t st) {
    const float om = (float)(1.0 - (double)momentum);
    hipLaunchKernelGGL(crd_update_kernel, dim3(B, 2), dim3(256), 0, st, memory_v1, memory_v2, v1, v2, y, B, d, n_data, momentum, om,
                       bad);
    return hipGetLastError();
}

}  // namespace moma
