// Generic batched MFMA GEMM used by the non-fused stages (projection linears, their gradients, the
// per-head score / context products and the materialised-logits compatibility path).
//   C[m,n] (+)= alpha * sum_k A(m,k) * B(n,k) + bias[n]
// TM x TM output tile per 256-thread workgroup, TM = 64 (4 waves as 2x2, each wave 2x2 MFMA 16x16 tiles) or TM = 32 (each
// wave one 16x16 tile) for problems with few output tiles: the M = 256-class linears of the attention module then cover
// the chip WITHOUT splitting K, so every result is a fixed-order sum (bitwise reproducible; no atomics).  K in steps of 32
// through fp32 LDS tiles.  Two arithmetic policies on the same tiles:
//   MOMA_PREC_F32  : v_mfma_f32_16x16x4_f32  (exact fp32 fma chain = the reference's arithmetic)
//   MOMA_PREC_BF16 : v_mfma_f32_16x16x32_bf16 (operands rounded to bf16 at fragment load, fp32 accumulate)
#include "common.hpp"
#include <mutex>

namespace moma {

namespace {
// K step per LDS tile: 32 with the 64 x 64 tile, 128 with the 32 x 32 tile.  The M = 256-class linears are latency- and
// L2-traffic-bound (a T x T tile reloads M*N*K*4*(2/T) bytes from L2: 50 MB for the qkv linear at T = 32): measured on MI355X
// (rocprofv3, [256 x 1536 x 512]) BK = 128 -> 14.6 us average, the whole K panel at once (BK = 512) -> 18.9 us, BK = 32 -> 17.0 us.
// Rows padded by 4 floats (16-B aligned, banks).
// One TM x BK operand tile travels global -> registers -> LDS.  The two halves are split so that the global loads
// of tile k+1 are in flight while tile k is multiplied.
//   X(row,k) = trans ? X[k*ld + row] : X[row*ld + k]; out-of-range elements read as zero.
// VEC: 16-byte loads along the contiguous dimension (needs fp32 data, ld % 4 == 0, 16-B aligned base).
template <int N>
struct TileRegs {
    float v[N];
};

template <typename T, bool VEC, int TM, int BK>
__device__ __forceinline__ void load_tile(TileRegs<TM * BK / 256>& t, const T* __restrict__ X, long ld, int trans, int r0, int rows,
                                          int k0, int kend, int tid) {
    constexpr int NS = TM * BK / 256;           // scalars per thread   (TM x BK elements over 256 threads)
    constexpr int NV = NS / 4;                  // float4 per thread
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * 256;
            int gr, gk;
            if (!trans) { gr = r0 + idx / (BK / 4); gk = k0 + (idx % (BK / 4)) * 4; }   // 4 consecutive k of one row
            else { gk = k0 + idx / (TM / 4); gr = r0 + (idx % (TM / 4)) * 4; }      // 4 consecutive rows of one k
            const long off = trans ? (long)gk * ld + gr : (long)gr * ld + gk;
            const int lim = trans ? rows - gr : kend - gk;                          // valid elements along the vector
            const bool other_ok = trans ? (gk < kend) : (gr < rows);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (other_ok && lim >= 4) v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(X) + off);
            else if (other_ok && lim > 0) {
                const float* p = reinterpret_cast<const float*>(X) + off;
                v.x = p[0];
                if (lim > 1) v.y = p[1];
                if (lim > 2) v.z = p[2];
            }
            t.v[4 * i + 0] = v.x; t.v[4 * i + 1] = v.y; t.v[4 * i + 2] = v.z; t.v[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int idx = tid + i * 256;
            int gr, gk;
            if (!trans) { gr = r0 + idx / BK; gk = k0 + (idx % BK); }
            else { gk = k0 + idx / TM; gr = r0 + (idx % TM); }
            float v = 0.f;
            if (gr < rows && gk < kend) v = ld1<T>(X + (trans ? (long)gk * ld + gr : (long)gr * ld + gk));
            t.v[i] = v;
        }
    }
}

template <bool VEC, int TM, int BK>
__device__ __forceinline__ void store_tile(float (*S)[BK + 4], const TileRegs<TM * BK / 256>& t, int trans, int tid) {
    constexpr int NS = TM * BK / 256, NV = NS / 4;
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * 256;
            if (!trans) {
                *reinterpret_cast<float4*>(&S[idx / (BK / 4)][(idx % (BK / 4)) * 4]) =
                    make_float4(t.v[4 * i], t.v[4 * i + 1], t.v[4 * i + 2], t.v[4 * i + 3]);
            } else {
                const int kr = idx / (TM / 4), c = (idx % (TM / 4)) * 4;
#pragma unroll
                for (int j = 0; j < 4; ++j) S[c + j][kr] = t.v[4 * i + j];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int idx = tid + i * 256;
            if (!trans) S[idx / BK][idx % BK] = t.v[i];
            else S[idx % TM][idx / TM] = t.v[i];
        }
    }
}

template <int PREC, typename TB, bool VECA, bool VECB, int TM>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs g) {
    constexpr int BK = TM == 32 ? 128 : 32, LDK = BK + 4;
    constexpr int BM = TM, BN = TM, WT = TM / 2, NF = TM / 32;   // wave sub-tile WT x WT = NF x NF MFMA tiles of 16 x 16
    extern __shared__ __attribute__((aligned(16))) float gemm_smem[];
    float (*As)[LDK] = reinterpret_cast<float (*)[LDK]>(gemm_smem);
    float (*Bs)[LDK] = reinterpret_cast<float (*)[LDK]>(gemm_smem + BM * LDK);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
    const int batch = blockIdx.z / g.splitk, split = blockIdx.z % g.splitk;
    const float* A = g.A + (long)batch * g.strideA;
    const TB* B = reinterpret_cast<const TB*>(g.B) + (long)batch * g.strideB;
    float* C = g.C + (long)batch * g.strideC + (g.atomic ? 0L : (long)split * g.splitC);

    const int ktiles = (g.K + BK - 1) / BK;
    const int per = (ktiles + g.splitk - 1) / g.splitk;
    const int kbeg = split * per * BK;
    const int kend = min(g.K, kbeg + per * BK);

    f32x4 acc[NF][NF];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fg = lane >> 4;
    TileRegs<TM * BK / 256> ra, rb;
    if (kbeg < kend) {
        load_tile<float, VECA, TM, BK>(ra, A, g.lda, g.transA, m0, g.M, kbeg, kend, tid);
        load_tile<TB, VECB, TM, BK>(rb, B, g.ldb, g.transB, n0, g.N, kbeg, kend, tid);
    }
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        store_tile<VECA, TM, BK>(As, ra, g.transA, tid);
        store_tile<VECB, TM, BK>(Bs, rb, g.transB, tid);
        __syncthreads();
        if (k0 + BK < kend) {                      // next tile's loads fly while this one is multiplied
            load_tile<float, VECA, TM, BK>(ra, A, g.lda, g.transA, m0, g.M, k0 + BK, kend, tid);
            load_tile<TB, VECB, TM, BK>(rb, B, g.ldb, g.transB, n0, g.N, k0 + BK, kend, tid);
        }
        if constexpr (PREC == MOMA_PREC_BF16) {
#pragma unroll
            for (int k32 = 0; k32 < BK / 32; ++k32) {
                bf16x8 af[NF], bf[NF];
#pragma unroll
                for (int i = 0; i < NF; ++i) {
                    const float* pa = &As[wm * WT + i * 16 + fr][k32 * 32 + fg * 8];
                    const float* pb = &Bs[wn * WT + i * 16 + fr][k32 * 32 + fg * 8];
                    const float4 a0 = *reinterpret_cast<const float4*>(pa), a1 = *reinterpret_cast<const float4*>(pa + 4);
                    const float4 b0 = *reinterpret_cast<const float4*>(pb), b1 = *reinterpret_cast<const float4*>(pb + 4);
                    af[i] = bf16x8{(__bf16)a0.x, (__bf16)a0.y, (__bf16)a0.z, (__bf16)a0.w,
                                   (__bf16)a1.x, (__bf16)a1.y, (__bf16)a1.z, (__bf16)a1.w};
                    bf[i] = bf16x8{(__bf16)b0.x, (__bf16)b0.y, (__bf16)b0.z, (__bf16)b0.w,
                                   (__bf16)b1.x, (__bf16)b1.y, (__bf16)b1.z, (__bf16)b1.w};
                }
#pragma unroll
                for (int i = 0; i < NF; ++i)
#pragma unroll
                    for (int j = 0; j < NF; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < BK / 4; ++kk) {
                float af[NF], bf[NF];
#pragma unroll
                for (int i = 0; i < NF; ++i) {
                    af[i] = As[wm * WT + i * 16 + fr][kk * 4 + fg];
                    bf[i] = Bs[wn * WT + i * 16 + fr][kk * 4 + fg];
                }
#pragma unroll
                for (int i = 0; i < NF; ++i)
#pragma unroll
                    for (int j = 0; j < NF; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // C/D layout of the 16x16 tile: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const int col = n0 + wn * WT + j * 16 + fr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * WT + i * 16 + fg * 4 + r;
                if (row < g.M && col < g.N) {
                    float v = acc[i][j][r] * g.alpha;
                    if (g.bias != nullptr && split == 0) v += g.bias[col];
                    float* dst = C + (long)row * g.ldc + col;
                    if (g.atomic) atomicAdd(dst, v);
                    else *dst = v;
                }
            }
        }
}
}  // namespace

namespace {
// ---- small linears of the attention module under the bf16 policy (M = 256-class: x.W^T, dY.W, dY^T.X) ----------------------
// The tiled kernel above pays one global-load round trip per K tile (4 at K = 512) and next to no arithmetic in between:
// 14.6 us for [256 x 1536 x 512].  Here a workgroup owns one 32 x 32 output tile and its four waves split K: every wave
// requests ALL fragments of its K quarter straight into registers in MFMA operand order -- 2 x 16 B per lane and k-step for
// an operand stored K-contiguous, 8 x 4 B (32 consecutive rows per k: coalesced) for one stored K-major -- so the whole
// kernel is ONE load round trip, 8 MFMAs per wave, and a fixed-order sum of the four partial tiles through LDS
// (bitwise reproducible, no atomics).  No LDS staging, no transposition pass for the gradient products.
// (Tried: the K-contiguous panels loaded in full rows, converted and staged through 16 KiB of LDS per wave, fragments read back
//  with ds_read_b128 -- 8 cache lines per load instead of 64.  Slower, 15.0 vs 12.9 us on the qkv linear: the 64 KiB of LDS
//  halve the workgroups per CU and the extra LDS round trip outweighs the cheaper loads.)
template <bool TRA, bool TRB>
__global__ __launch_bounds__(256) void linear_ksplit_kernel(GemmArgs g) {
    __shared__ float red[4][16][64];
    __shared__ float csum[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r32 = lane & 31, kh = lane >> 5;
    const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
    // batched products (the per-head products of the staged attention path): one batch entry per blockIdx.z
    g.A += (long)blockIdx.z * g.strideA;
    g.B = reinterpret_cast<const float*>(g.B) + (long)blockIdx.z * g.strideB;
    g.C += (long)blockIdx.z * g.strideC;
    const int steps = g.K / 16;                                     // k-steps of 16 (K % 16 == 0 by dispatch)
    const int base = steps / 4, rem = steps % 4;
    const int sb = wave * base + min(wave, rem), ns = base + (wave < rem ? 1 : 0);
    const long arow = min(m0 + r32, g.M - 1), brow = min(n0 + r32, g.N - 1);       // clamped: masked at the store
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // sum_k A(m, k) of this tile's 32 rows next to the product (the bias gradient beside dW = dY^T X): first column tile only
    const bool want_cs = TRA && g.colsum_a != nullptr && blockIdx.x == 0;
    float cs = 0.f;
    constexpr int CH = 8;                                           // k-steps in flight per chunk
    for (int c0 = 0; c0 < ns; c0 += CH) {
        float fa[CH][8], fb[CH][8];
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            if (c0 + s < ns) {
                const long k0 = (long)(sb + c0 + s) * 16 + 8 * kh;
                if constexpr (!TRA) {
                    const float4* p = reinterpret_cast<const float4*>(g.A + arow * g.lda + k0);
                    const float4 v0 = p[0], v1 = p[1];
                    fa[s][0] = v0.x; fa[s][1] = v0.y; fa[s][2] = v0.z; fa[s][3] = v0.w;
                    fa[s][4] = v1.x; fa[s][5] = v1.y; fa[s][6] = v1.z; fa[s][7] = v1.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) fa[s][j] = g.A[(k0 + j) * g.lda + arow];
                }
                const float* B = reinterpret_cast<const float*>(g.B);
                if constexpr (!TRB) {
                    const float4* p = reinterpret_cast<const float4*>(B + brow * g.ldb + k0);
                    const float4 v0 = p[0], v1 = p[1];
                    fb[s][0] = v0.x; fb[s][1] = v0.y; fb[s][2] = v0.z; fb[s][3] = v0.w;
                    fb[s][4] = v1.x; fb[s][5] = v1.y; fb[s][6] = v1.z; fb[s][7] = v1.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) fb[s][j] = B[(k0 + j) * g.ldb + brow];
                }
            }
        }
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            if (c0 + s < ns) {
                if (want_cs) cs += ((fa[s][0] + fa[s][1]) + (fa[s][2] + fa[s][3])) + ((fa[s][4] + fa[s][5]) + (fa[s][6] + fa[s][7]));
                const bf16x8 a = bf16x8{(__bf16)fa[s][0], (__bf16)fa[s][1], (__bf16)fa[s][2], (__bf16)fa[s][3],
                                        (__bf16)fa[s][4], (__bf16)fa[s][5], (__bf16)fa[s][6], (__bf16)fa[s][7]};
                const bf16x8 b = bf16x8{(__bf16)fb[s][0], (__bf16)fb[s][1], (__bf16)fb[s][2], (__bf16)fb[s][3],
                                        (__bf16)fb[s][4], (__bf16)fb[s][5], (__bf16)fb[s][6], (__bf16)fb[s][7]};
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
    csum[wave][lane] = cs;
    __syncthreads();
    if (want_cs && threadIdx.x < 32 && m0 + (int)threadIdx.x < g.M) {                // fixed order: K quarters, lane halves
        const int r = threadIdx.x;
        g.colsum_a[m0 + r] = (((csum[0][r] + csum[0][r + 32]) + (csum[1][r] + csum[1][r + 32])) +
                              ((csum[2][r] + csum[2][r + 32]) + (csum[3][r] + csum[3][r + 32])));
    }
    // D layout of the 32 x 32 tile: column = lane & 31, row = 8*(r>>2) + 4*(lane>>5) + (r&3); the K quarters in a fixed order
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = wave * 4 + i;
        const float v = ((red[0][r][lane] + red[1][r][lane]) + red[2][r][lane]) + red[3][r][lane];
        const int row = m0 + 8 * (r >> 2) + 4 * kh + (r & 3), col = n0 + r32;
        if (row < g.M && col < g.N) {
            float o = v * g.alpha;
            if (g.bias != nullptr) o += g.bias[col];
            g.C[(long)row * g.ldc + col] = o;
        }
    }
}

bool linear_ksplit_ok(const GemmArgs& a) {
    if (a.prec != MOMA_PREC_BF16 || a.b_dtype != MOMA_DT_F32 || a.batch < 1 || a.batch > 65535 || a.splitk != 1 || a.atomic) return false;
    if (a.K < 64 || a.K % 16 != 0) return false;
    const bool batched = a.batch > 1;
    if (batched && (a.bias != nullptr || a.colsum_a != nullptr)) return false;
    if (!a.transA && !(((uintptr_t)a.A % 16) == 0 && a.lda % 4 == 0 && (!batched || a.strideA % 4 == 0))) return false;
    if (!a.transB && !(((uintptr_t)a.B % 16) == 0 && a.ldb % 4 == 0 && (!batched || a.strideB % 4 == 0))) return false;
    const long tiles = (long)((a.N + 31) / 32) * ((a.M + 31) / 32) * a.batch;
    return tiles <= 1024;                                           // past that the 64 x 64 tiles re-read less from L2
}
}  // namespace

namespace {
template <int PREC, typename TB, bool VA, bool VB, int TM>
void launch_one(const GemmArgs& a, dim3 grid, hipStream_t s) {
    constexpr int BK = TM == 32 ? 128 : 32;
    constexpr size_t lds = (size_t)2 * TM * (BK + 4) * sizeof(float);
    if constexpr (lds > 64 * 1024) {                       // dynamic-LDS opt-in, once per process and instantiation
        static std::once_flag once;
        std::call_once(once, [] {
            (void)hipFuncSetAttribute((const void*)gemm_kernel<PREC, TB, VA, VB, TM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        });
    }
    hipLaunchKernelGGL((gemm_kernel<PREC, TB, VA, VB, TM>), grid, dim3(256), lds, s, a);
}
template <int PREC, typename TB, int TM>
void launch_variant(const GemmArgs& a, dim3 grid, bool va, bool vb, hipStream_t s) {
    if (va && vb) launch_one<PREC, TB, true, true, TM>(a, grid, s);
    else if (va) launch_one<PREC, TB, true, false, TM>(a, grid, s);
    else if (vb) launch_one<PREC, TB, false, true, TM>(a, grid, s);
    else launch_one<PREC, TB, false, false, TM>(a, grid, s);
}
inline bool vec_ok(const void* p, long ld, long stride, int batch) {
    return ((uintptr_t)p % 16) == 0 && ld % 4 == 0 && (batch == 1 || stride % 4 == 0);
}
template <int TM>
void launch_tm(const GemmArgs& a, hipStream_t s) {
    dim3 grid((a.N + TM - 1) / TM, (a.M + TM - 1) / TM, a.batch * a.splitk);
    const bool va = vec_ok(a.A, a.lda, a.strideA, a.batch);
    const bool vb = a.b_dtype == MOMA_DT_F32 && vec_ok(a.B, a.ldb, a.strideB, a.batch);
    if (a.prec == MOMA_PREC_BF16) {
        if (a.b_dtype == MOMA_DT_BF16) launch_variant<MOMA_PREC_BF16, bf16_raw, TM>(a, grid, va, false, s);
        else launch_variant<MOMA_PREC_BF16, float, TM>(a, grid, va, vb, s);
    } else {
        if (a.b_dtype == MOMA_DT_BF16) launch_variant<MOMA_PREC_F32, bf16_raw, TM>(a, grid, va, false, s);
        else launch_variant<MOMA_PREC_F32, float, TM>(a, grid, va, vb, s);
    }
}
}  // namespace

bool gemm_fuses_colsum(const GemmArgs& a) { return a.transA && a.alpha == 1.f && linear_ksplit_ok(a); }

hipError_t launch_gemm(const GemmArgs& a, hipStream_t s) {
    if (a.M <= 0 || a.N <= 0 || a.batch <= 0) return hipSuccess;
    // Few 64 x 64 output tiles (the M = 256-class linears): 32 x 32 tiles give 4x the workgroups instead of a K split --
    // every output element stays ONE fixed-order sum, so the results are bitwise reproducible.  (A caller that wants a K
    // split over workgroups asks for it explicitly with splitk / atomic: only the materialised-logits gradient does.)
    if (linear_ksplit_ok(a)) {
        const dim3 grid((a.N + 31) / 32, (a.M + 31) / 32, a.batch);
        if (a.transA && a.transB) hipLaunchKernelGGL((linear_ksplit_kernel<true, true>), grid, dim3(256), 0, s, a);
        else if (a.transA) hipLaunchKernelGGL((linear_ksplit_kernel<true, false>), grid, dim3(256), 0, s, a);
        else if (a.transB) hipLaunchKernelGGL((linear_ksplit_kernel<false, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((linear_ksplit_kernel<false, false>), grid, dim3(256), 0, s, a);
        return hipGetLastError();
    }
    const long tiles64 = (long)((a.N + 63) / 64) * ((a.M + 63) / 64) * a.batch * a.splitk;
    if (tiles64 < 192) launch_tm<32>(a, s);
    else launch_tm<64>(a, s);
    return hipGetLastError();
}

}  // namespace moma
