// Shared device helpers and internal launch declarations for libmoma_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
#include <type_traits>
#include "../../include/moma_hip.h"

namespace moma {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef unsigned short bf16_raw;  // storage type of a bf16 queue element

constexpr int WAVE = 64;

constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }

__device__ __forceinline__ float bf16_to_f32(bf16_raw v) {
    return __uint_as_float(((unsigned)v) << 16);
}
__device__ __forceinline__ bf16_raw f32_to_bf16(float f) {
    // plain cast -> v_cvt_pk_bf16_f32 (round to nearest even, NaN stays NaN)
    __bf16 b = (__bf16)f;
    return *reinterpret_cast<bf16_raw*>(&b);
}

// the activation that follows a BatchNorm (MOMA_ACT_*): THE formula of bn.hip's apply kernels and of the depthwise kernels'
// pre-activation prologue (dwconv.hip), which must reproduce the former bit for bit
__device__ __forceinline__ float act_fwd(float y, int act) {
    if (act == MOMA_ACT_SILU) return y / (1.f + __expf(-y));
    if (act == MOMA_ACT_RELU) return fmaxf(y, 0.f);
    return y;
}

// two floats -> one word of two bf16 (lo in bits 0..15), round to nearest even: ONE v_cvt_pk_bf16_f32.  Written as
// `f32_to_bf16(lo) | f32_to_bf16(hi) << 16` hipcc pairs the conversions of a 16-byte store the wrong way round (values 0,2 / 1,3)
// and puts the words together again with v_and / v_lshl / 2 x v_or_sdwa: 20 VALU instructions per store instead of 12 -- seen
// in round 4 in the partial stores of the one-pass K2 kernel, whose last tile took 2.9 us instead of ~1
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}

// value of lane l ^ 32 (the other half of the wave) by one v_permlane32_swap -- a VALU instruction; __shfl_xor(v, 32) is a
// ds_bpermute, i.e. an LDS round trip with a wait
__device__ __forceinline__ float other_half(float v) {
    const unsigned u = __float_as_uint(v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);     // r[0] = {lo, lo}, r[1] = {hi, hi}
    return __uint_as_float((threadIdx.x & 32) ? r[0] : r[1]);
}

// Reductions over the 32 lanes of a wave HALF (lanes 0-31 / 32-63), result in every lane, without LDS: four DPP rotations inside
// the 16-lane rows (x op= ror 8, 4, 2, 1: a butterfly, so every lane of a row ends with the same bits) and one v_permlane16_swap
// across the two rows of the half.  __shfl_xor is a ds_bpermute each -- five dependent LDS round trips per reduction.
template <int CTRL>
__device__ __forceinline__ float dpp_row(float v) {
    return __uint_as_float((unsigned)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float half32_sum(float v) {
    v += dpp_row<0x128>(v);            // row_ror:8
    v += dpp_row<0x124>(v);            // row_ror:4
    v += dpp_row<0x122>(v);            // row_ror:2
    v += dpp_row<0x121>(v);            // row_ror:1
    const unsigned u = __float_as_uint(v);
    const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);     // r[0] = rows {0, 0, 2, 2}, r[1] = rows {1, 1, 3, 3}
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float half32_max(float v) {
    v = fmaxf(v, dpp_row<0x128>(v));
    v = fmaxf(v, dpp_row<0x124>(v));
    v = fmaxf(v, dpp_row<0x122>(v));
    v = fmaxf(v, dpp_row<0x121>(v));
    const unsigned u = __float_as_uint(v);
    const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// double -> float as a rounding of its own: written as a plain cast in front of a bf16 store the compiler merges the two roundings
// into one double -> bf16 conversion, and a value that is a tie in fp32 then lands on the other side of what the fp32 output rounds to
__device__ __forceinline__ float round_f32(double d) {
    float f = (float)d;
    asm("" : "+v"(f));
    return f;
}

// ---- typed vector access: VEC elements of storage type T (float or bf16_raw) <-> fp32 registers, one memory instruction of up to
//      16 bytes (PV<float, 8>: two); the pointer must be aligned to VEC elements.  THE accessor of every kernel file but the
//      InfoNCE / K1 ones, which have operand layouts of their own --------------------------------------------------------------
template <typename T> constexpr int MAXVEC = 16 / sizeof(T);        // elements of T in 16 bytes
template <typename T, int VEC> struct PV;
template <> struct PV<float, 8> {
    static __device__ void ld(const float* p, float* v) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    static __device__ void st(float* p, const float* v) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
};
template <> struct PV<float, 4> {
    static __device__ void ld(const float* p, float* v) { const float4 a = *reinterpret_cast<const float4*>(p); v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }
    static __device__ void st(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct PV<float, 2> {
    static __device__ void ld(const float* p, float* v) { const float2 a = *reinterpret_cast<const float2*>(p); v[0] = a.x; v[1] = a.y; }
    static __device__ void st(float* p, const float* v) { *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]); }
};
template <> struct PV<float, 1> {
    static __device__ void ld(const float* p, float* v) { v[0] = *p; }
    static __device__ void st(float* p, const float* v) { *p = v[0]; }
};
template <> struct PV<bf16_raw, 8> {
    static __device__ void ld(const bf16_raw* p, float* v) {
        const uint4 a = *reinterpret_cast<const uint4*>(p);
        const unsigned w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
    }
    static __device__ void st(bf16_raw* p, const float* v) {
        uint4 a;
        a.x = (unsigned)f32_to_bf16(v[0]) | ((unsigned)f32_to_bf16(v[1]) << 16);
        a.y = (unsigned)f32_to_bf16(v[2]) | ((unsigned)f32_to_bf16(v[3]) << 16);
        a.z = (unsigned)f32_to_bf16(v[4]) | ((unsigned)f32_to_bf16(v[5]) << 16);
        a.w = (unsigned)f32_to_bf16(v[6]) | ((unsigned)f32_to_bf16(v[7]) << 16);
        *reinterpret_cast<uint4*>(p) = a;
    }
};
template <> struct PV<bf16_raw, 4> {
    static __device__ void ld(const bf16_raw* p, float* v) {
        const uint2 a = *reinterpret_cast<const uint2*>(p);
        v[0] = __uint_as_float(a.x << 16); v[1] = __uint_as_float(a.x & 0xffff0000u);
        v[2] = __uint_as_float(a.y << 16); v[3] = __uint_as_float(a.y & 0xffff0000u);
    }
    static __device__ void st(bf16_raw* p, const float* v) {
        uint2 a;
        a.x = (unsigned)f32_to_bf16(v[0]) | ((unsigned)f32_to_bf16(v[1]) << 16);
        a.y = (unsigned)f32_to_bf16(v[2]) | ((unsigned)f32_to_bf16(v[3]) << 16);
        *reinterpret_cast<uint2*>(p) = a;
    }
};
template <> struct PV<bf16_raw, 2> {          // (load only: no kernel stores two bf16)
    static __device__ void ld(const bf16_raw* p, float* v) {
        const unsigned a = *reinterpret_cast<const unsigned*>(p);
        v[0] = __uint_as_float(a << 16); v[1] = __uint_as_float(a & 0xffff0000u);
    }
};
template <> struct PV<bf16_raw, 1> {
    static __device__ void ld(const bf16_raw* p, float* v) { v[0] = bf16_to_f32(*p); }
    static __device__ void st(bf16_raw* p, const float* v) { *p = f32_to_bf16(v[0]); }
};
template <typename T> __device__ __forceinline__ float ld1(const T* p) { float v; PV<T, 1>::ld(p, &v); return v; }
template <typename T> __device__ __forceinline__ void st1(T* p, float v) { PV<T, 1>::st(p, &v); }

// ---- the vector width of a launch (host) ------------------------------------------------------------------------------------
// The first of `widths` (widest first) that divides `extent`, the run of contiguous elements, and whose byte size divides
// `low_bits`, the OR of the addresses accessed at that width; else 1.  Every kernel family passes a list of its own, ON PURPOSE:
// the width decides which elements one thread adds up, so it fixes the summation order of that family's reductions and with it
// the bits of the results.  The static_asserts state what tells the lists apart.
constexpr int pick_vec(long extent, int elem_bytes, uintptr_t low_bits, std::initializer_list<int> widths) {
    for (const int v : widths)
        if (extent % v == 0 && low_bits % (uintptr_t)(v * elem_bytes) == 0) return v;
    return 1;
}
// bn.hip {8, 4} for both types: fp32 at 8 is two 16-byte accesses and asks for 32-byte alignment
static_assert(pick_vec(56 * 56, 4, 0x20, {8, 4}) == 8 && pick_vec(56 * 56, 4, 0x10, {8, 4}) == 4, "bn");
// se.hip, attention.hip {16 / eb, 4}: never 2
static_assert(pick_vec(6, 2, 0, {8, 4}) == 1 && pick_vec(8, 4, 0, {4, 4}) == 4, "se / at");
// dwconv.hip {16 / eb, 4, 2}: every power of two down to 2
static_assert(pick_vec(6, 2, 0, {8, 4, 2}) == 2 && pick_vec(112, 2, 4, {8, 4, 2}) == 2, "dw");
// nst.hip, rkd.hip, sp.hip {16 / eb}: 16 bytes or nothing
static_assert(pick_vec(12, 2, 0, {8}) == 1 && pick_vec(16, 2, 0, {8}) == 8 && pick_vec(16, 2, 8, {8}) == 1, "nst / rkd / sp");
// mapwalk.hpp (vid.hip, hint.hip) and semckd.hip, per side: the widest of 8, 4, 1 elements that divides the contiguous extent and
// whose accesses (16 bytes at most each) are aligned
inline int side_vec(const void* p, long long extent, int dtype) {
    if (dtype == MOMA_DT_BF16) return pick_vec((long)extent, 2, (uintptr_t)p, {8, 4});
    const int v = pick_vec((long)extent, 4, (uintptr_t)p, {4});
    return v == 4 && extent % 8 == 0 ? 8 : v;                                      // (8 fp32: two 16-byte accesses)
}

// ---- run-time (dtype, vec) -> template arguments (host; semckd.hip also on the device, per pair of a grouped launch) ---------
// f(TypeTag<bf16_raw>{}) or f(TypeTag<float>{}) by MOMA_DT_*; inside a generic lambda: using T = typename decltype(t)::type
template <typename T> struct TypeTag { using type = T; };
template <typename F> __host__ __device__ auto with_dtype(int dtype, F&& f) {
    return dtype == MOMA_DT_BF16 ? f(TypeTag<bf16_raw>{}) : f(TypeTag<float>{});
}
// f(std::integral_constant<int, V>{}) for the V of the list V, REST... (widest first) that equals `vec`, the last one for any other
// `vec`.  Widths above CAP (at most call sites MAXVEC<T>) are left out of the list: they get no instantiation.
template <int CAP, int V, int... REST, typename F> __host__ __device__ void with_vec(int vec, F&& f) {
    if constexpr (V > CAP) with_vec<CAP, REST...>(vec, f);
    else if constexpr (sizeof...(REST) == 0) f(std::integral_constant<int, V>{});
    else if (vec == V) f(std::integral_constant<int, V>{});
    else with_vec<CAP, REST...>(vec, f);
}

// ---- generic batched GEMM:  C[m,n] (+)= alpha * sum_k A(m,k) * B(n,k) + bias[n] ----------------
//   A(m,k) = transA ? A[k*lda + m] : A[m*lda + k]      (fp32)
//   B(n,k) = transB ? B[k*ldb + n] : B[n*ldb + k]      (fp32 or bf16 storage)
//   batch b adds b*strideX elements to each base pointer; split-K partial sums are combined with
//   fp32 atomics into a C the caller has initialised (atomic != 0).
struct GemmArgs {
    const float* A;
    const void* B;
    float* C;
    const float* bias;   // nullable, length N
    int M, N, K;
    long lda, ldb, ldc;
    long strideA, strideB, strideC;
    int batch;
    int transA, transB;
    float alpha;
    int splitk;          // >= 1
    int atomic;          // 1: atomicAdd into C
    long splitC;         // splitk > 1 without atomics: split s writes its partial product to C + s * splitC (the caller sums them)
    int b_dtype;         // MOMA_DT_*
    int prec;            // MOMA_PREC_*
    float* colsum_a;     // nullable: also write sum_k A(m,k) for every m (the bias gradient next to dW = dY^T X); only honoured
                         // where gemm_fuses_colsum(args) holds, zero-initialised by value-initialisation otherwise ignored
};
hipError_t launch_gemm(const GemmArgs& a, hipStream_t s);
bool gemm_fuses_colsum(const GemmArgs& a);     // true: launch_gemm fills a.colsum_a itself (no separate column-sum launch)

// ---- row-wise helpers (rowops.hip) ---------------------------------------------------------------
hipError_t launch_softmax_rows(float* s, long rows, int cols, hipStream_t st);
hipError_t launch_softmax_bwd_rows(const float* p, float* dp, long rows, int cols, float scale, hipStream_t st);
hipError_t launch_colsum(const float* x, float* out, int rows, int cols, long ld, hipStream_t st);
hipError_t launch_pos_logit(const float* q, const float* k, float* out, long ld_out, int B, int d, float inv_T, hipStream_t st);
hipError_t launch_infonce_rows(float* logits, int B, int ncols, float* loss_rows, float* lse, int32_t* top1,
                               int write_probs, hipStream_t st);
// dst[i] = ((dst[i] + parts[i]) + parts[stride + i]) + ... over nparts partial arrays: the fixed-order end of a split-K product
hipError_t launch_add_partials(float* dst, const float* parts, int nparts, long n, long stride, hipStream_t st);
hipError_t launch_pos_grad_init(const float* dlogits, long ld, const float* k, float* dq, int B, int d, float inv_T,
                                hipStream_t st);

// ---- queue.hip -----------------------------------------------------------------------------------
hipError_t launch_enqueue(void* queue, const float* rows, int n, int64_t index, int K, int d, int qdtype, hipStream_t st);
hipError_t launch_enqueue_mirror(float* queue, void* mirror, const float* rows, int n, int64_t index, int K, int d, hipStream_t st);
hipError_t launch_prefetch(const void* p, size_t bytes, hipStream_t st);
hipError_t launch_widen_bf16(const void* src, float* dst, size_t n, hipStream_t st);      // bf16 -> fp32, n elements (src 16-B aligned)
hipError_t launch_ema(const int64_t* table, int n_tensors, int64_t total_blocks, float m, float om, hipStream_t st);

// ---- crd.hip (CRD: gather-contrast over two sample-indexed memory banks) ---------------------------
size_t crd_workspace_bytes(int B, int d, int K1);
hipError_t launch_crd_fused(const float* v1, const float* v2, const float* memory_v1, const float* memory_v2, const int64_t* idx,
                            int B, int d, int K1, int64_t n_data, float T, float* Z, int set_z, float* loss, float* dv1, float* dv2,
                            int32_t* bad, void* ws, hipStream_t st);
hipError_t launch_crd_scores(const float* v1, const float* v2, const float* memory_v1, const float* memory_v2, const int64_t* idx,
                             int B, int d, int K1, int64_t n_data, float T, float* Z, int set_z, float* out_v1, float* out_v2,
                             int32_t* bad, void* ws, hipStream_t st);
hipError_t launch_crd_scores_bwd(const float* dout_v1, const float* dout_v2, const float* out_v1, const float* out_v2,
                                 const float* memory_v1, const float* memory_v2, const int64_t* idx, int B, int d, int K1,
                                 int64_t n_data, float T, float* dv1, float* dv2, int32_t* bad, void* ws, hipStream_t st);
hipError_t launch_crd_update(float* memory_v1, float* memory_v2, const float* v1, const float* v2, const int64_t* y, int B, int d,
                             int64_t n_data, float momentum, int32_t* bad, hipStream_t st);

// ---- attention.hip (Attention Transfer: spatial attention maps, the pair loss, the feature gradient) ----------------------
size_t at_workspace_bytes(int B, int C, int H, int W, int oh, int ow, int layout);
hipError_t launch_at_map(const void* f, float* a, int B, int C, int H, int W, int oh, int ow, int dtype, int layout, void* ws,
                         hipStream_t st);
hipError_t launch_at_pair(const float* a_s, const float* a_t, int B, int n, float* norms, float* partials, float* loss, float* g_s,
                          float* g_t, float* ah_s, float* ah_t, hipStream_t st);
hipError_t launch_at_bwd(const void* f, const float* g_a, const float* g_loss, void* dF, int B, int C, int H, int W, int oh, int ow,
                         int dtype, int layout, hipStream_t st);

// ---- nst.hip (Neuron Selectivity Transfer: per-image normalised Gram of a feature pair, its loss, the student's gradient) ------
size_t nst_workspace_bytes(int B, int Cs, int Ct);
long long nst_row_blocks(int Cs);
long long nst_pixel_tiles(int P);
hipError_t launch_nst_gram(const void* fs, const void* ft, int B, int Cs, int Ct, int P, int dt_s, int lay_s, int dt_t, int lay_t,
                           float* G, float* norms, float* rows, float* partials, float* terms, float* loss, hipStream_t st);
hipError_t launch_nst_bwd(const void* fs, const void* ft, const float* G, const float* norms, const float* rows, const float* g_loss,
                          void* dF, int B, int Cs, int Ct, int P, int dt_s, int lay_s, int dt_t, int lay_t, hipStream_t st);

// ---- vid.hip (Variational Information Distillation: the per-channel Gaussian NLL of a regressor's output, its gradients) --------
long long vid_partial_rows(int B, int P);
size_t vid_workspace_bytes(int B, int C, int P);
hipError_t launch_vid_nll(const void* mean, const void* target, const float* log_scale, float eps, int B, int C, int P, int dt_m,
                          int lay_m, int dt_t, int lay_t, double* partials, float* sq, float* var, float* g_log_scale, float* loss,
                          hipStream_t st);
hipError_t launch_vid_bwd(const void* mean, const void* target, const float* var, const float* g_loss, void* d_mean, int B, int C,
                          int P, int dt_m, int lay_m, int dt_t, int lay_t, hipStream_t st);

// ---- hint.hip (FitNets hint: training-mode BatchNorm, ReLU and the squared error behind the regressor's convolution, their gradients) --
long long hint_partial_rows(int B, int P);
size_t hint_workspace_bytes(int B, int C, int P);
hipError_t launch_hint_fwd(const void* x, const void* t, const float* gamma, const float* beta, const float* conv_bias,
                           float* running_mean, float* running_var, float momentum, float eps, int B, int C, int P, int dt_x,
                           int lay_x, int dt_t, int lay_t, double* partials, double* mean, double* invstd, double* sums, float* loss,
                           hipStream_t st);
hipError_t launch_hint_bwd(const void* x, const void* t, const float* gamma, const float* beta, const double* mean,
                           const double* invstd, const double* sums, const float* g_loss, void* dx, float* d_gamma, float* d_beta,
                           int B, int C, int P, int dt_x, int lay_x, int dt_t, int lay_t, hipStream_t st);

// ---- srrl.hip (SRRL: training-mode BatchNorm, ReLU, the teacher's classifier and both squared errors behind the connector's convolution) --
size_t srrl_workspace_bytes(int B, int C, int K);
hipError_t launch_srrl_fwd(const void* x, const void* t, const float* W, const float* bias, const float* logits, const float* gamma,
                           const float* beta, float* running_mean, float* running_var, float momentum, float eps, int B, int C, int K,
                           int dt_x, int dt_t, void* workspace, double* sums, float* dxu, float* loss, float* y_out, float* pred_out,
                           hipStream_t st);
hipError_t launch_srrl_bwd(const float* dxu, const double* sums, const float* g_loss, void* dx, float* d_gamma, float* d_beta, int B,
                           int C, int dt_x, hipStream_t st);

// ---- cc.hip (Correlation Congruence: both LinearEmbed heads as one product, the neighbouring-row product of |difference|, every gradient) --
size_t cc_workspace_bytes(int B, int Cs, int Ct, int D);
hipError_t launch_cc_fwd(const void* x_s, const void* x_t, const float* W_s, const float* b_s, const float* W_t, const float* b_t, int B,
                         int Cs, int Ct, int D, int dt_s, int dt_t, void* workspace, float* gu, float* loss, float* d_out,
                         hipStream_t st);
hipError_t launch_cc_bwd(const float* gu, const void* x_s, const void* x_t, const float* W_s, const float* g_loss, void* dx_s, float* dW_s,
                         float* db_s, float* dW_t, float* db_t, int B, int Cs, int Ct, int D, int dt_s, int dt_t, hipStream_t st);

// ---- ce.hip (the teacher trainer's classification head: cross-entropy, top-1 and the confusion matrix, the logits' gradient) ----------
size_t ce_workspace_bytes(int B);
hipError_t launch_ce_fwd(const void* z, const int64_t* labels, int B, int K, int dtype, void* workspace, float* loss, double* lse,
                         double* inv_n, int32_t* pred, double* stats, int64_t* conf, hipStream_t st);
hipError_t launch_ce_bwd(const void* z, const int64_t* labels, const double* lse, const double* inv_n, const float* g_loss, void* dz,
                         int B, int K, int dtype, hipStream_t st);

// ---- kdhead.hip (the student's head: cross-entropy, the KD divergence at temperature T and top-1, the student logits' gradient) ------
size_t kdhead_workspace_bytes(int B);
hipError_t launch_kdhead_fwd(const void* z_s, const void* z_t, const int64_t* labels, int B, int K, int dt_s, int dt_t, float T,
                             void* workspace, float* out, double* saved, hipStream_t st);
hipError_t launch_kdhead_bwd(const void* z_s, const void* z_t, const int64_t* labels, const double* saved, const float* g_cls,
                             const float* g_div, void* dz, int B, int K, int dt_s, int dt_t, float T, hipStream_t st);

// ---- rkd.hip (Relational Knowledge Distillation: pairwise squared distances, the distance and angle terms, the student's gradient) --
size_t rkd_workspace_bytes(int B);
hipError_t launch_rkd_dist(const void* f, int B, long long D, int dtype, double* S, hipStream_t st);
hipError_t launch_rkd_terms(const double* S_s, const double* S_t, int B, double w_d, double w_a, void* ws, double* Q, float* terms,
                            float* loss, hipStream_t st);
hipError_t launch_rkd_bwd(const void* f_s, const double* Q, const float* g_loss, void* dF, int B, long long D, int dtype,
                          hipStream_t st);

// ---- sp.hip (Similarity-Preserving distillation: split-K batch Gram per side, the row-normalised terms, the student's gradient) ------
long long sp_splits(int B, long long K);
size_t sp_workspace_bytes(int B, long long K);
hipError_t launch_sp_gram(const void* f, int B, long long K, int dtype, float* P, hipStream_t st);
hipError_t launch_sp_terms(const float* P_s, int splits_s, const float* P_t, int splits_t, int B, double* G, double* H, double* rows,
                           double* M, float* loss, hipStream_t st);
hipError_t launch_sp_bwd(const void* f_s, const double* M, const float* g_loss, void* dF, int B, long long K, int dtype, hipStream_t st);
hipError_t launch_sp_gram_sum(const float* P, int splits, int B, float* G, hipStream_t st);

// ---- semckd.hip (SemCKD: the attention-weighted per-sample MSE of every (student, teacher) pair as one grouped call each way) -------
size_t semckd_workspace_bytes(const moma_semckd_pair_t* pairs, int n_pairs, int B);
hipError_t launch_semckd_fwd(const moma_semckd_pair_t* pairs, int n_pairs, int S, int B, const float* w, double* partials, float* ind,
                             float* loss, hipStream_t st);
hipError_t launch_semckd_bwd(const moma_semckd_pair_t* pairs, int n_pairs, int S, int B, const float* w, const float* g_loss,
                             hipStream_t st);

// ---- pkt.hip (Probabilistic Knowledge Transfer: the raw batch Gram per side in double, the cosine / KL terms, the student's gradient) --
size_t pkt_workspace_bytes(int B);
hipError_t launch_pkt_gram(const void* f, int B, long long D, int dtype, double* G, hipStream_t st);
hipError_t launch_pkt_gram_pair(const void* f_s, long long Ds, int dt_s, const void* f_t, long long Dt, int dt_t, int B, double* G_s,
                                double* G_t, hipStream_t st);
hipError_t launch_pkt_terms(const double* G_s, const double* G_t, int B, void* ws, double* M, float* loss, hipStream_t st);
hipError_t launch_pkt_bwd(const void* f_s, const double* M, const float* g_loss, void* dF, int B, long long D, int dtype,
                          hipStream_t st);

// ---- infonce_fused.hip (one-pass flash-style kernel) ----------------------------------------------
bool infonce_flash_supported(int B, int d, int K, int qdtype, int prec);
size_t infonce_flash_workspace_bytes(int B, int d, int K);
int set_k2_target_wg(int n);                            // debug knob of the K2 plan (moma_debug_set_k2_target_wg)
// the enqueue that follows a K2 call (MoMA/mem_moco.py:97-99), carried by the call's LAST launch where there is one to carry it
struct EnqueueJob {
    void* queue16;        // bf16 queue rows are rounded into (the queue K2 has just read), or nullptr
    float* queue32;       // fp32 queue (alone, or next to its bf16 mirror `queue16`), or nullptr
    const float* rows;    // [n, d] fp32
    int n;                // 0: nothing to enqueue
    int64_t index;        // ring pointer: rows[i] -> slot (index + i) mod K
    int K, d;
};
hipError_t launch_infonce_flash(const float* q, const float* k, const void* queue, int B, int d, int K, float inv_T,
                                float* loss_rows, float* lse, int32_t* top1, float* dq, void* ws, int qdtype,
                                hipStream_t st, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr,
                                const void* q_packed = nullptr, hipEvent_t ev_call_end = nullptr,
                                const EnqueueJob* enq = nullptr);
size_t infonce_qpack_bytes(int B, int d);
bool infonce_multi_supported(int n_terms, int B, int d, int K, int qdtype, int prec);
size_t infonce_multi_workspace_bytes(int n_terms, int B, int d, int K);
hipError_t launch_infonce_multi(const moma_infonce_term_t* terms, int n_terms, int B, int d, int K, float inv_T, void* ws,
                                hipStream_t st);

// ---- infonce_f32.hip (one pass over an fp32 queue in exact fp32 arithmetic) ------------------------
bool infonce_f32_flash_supported(int B, int d, int K, int qdtype, int prec);
size_t infonce_f32_flash_workspace_bytes(int B, int d, int K);
hipError_t launch_infonce_f32_flash(const float* q, const float* k, const float* queue, int B, int d, int K, float inv_T,
                                    float* loss_rows, float* lse, int32_t* top1, float* dq, void* ws, hipStream_t st,
                                    hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);

// ---- k1_fast.hip (batch-token attention, bf16 fast path) -------------------------------------------
bool mha_fast_supported(int N, int d, int H, int prec);
hipError_t launch_mha_pack(const float* w_qkv, const float* w_proj, void* pack, int d, int with_t, hipStream_t st);
hipError_t launch_mha_fwd_fast(const moma_mha_module_t* mods, int n_modules, int N, int d, int H, hipStream_t st);
size_t mha_bwd_fast_workspace_bytes(int N, int d);
hipError_t launch_mha_bwd_fast(const void* pack, const void* x, int x_dtype, const void* qkv16, const void* attn16, const float* lse,
                               const float* dy, float* dx, float* dw_qkv, float* db_qkv, float* dw_proj, float* db_proj,
                               void* workspace, int N, int d, int H, hipStream_t st);

// ---- bn.hip (BatchNorm2d + activation, NCHW) ------------------------------------------------------
size_t bn_workspace_floats(int C);
hipError_t launch_bn_fwd(const void* x, void* out, const float* gamma, const float* beta, float* rm, float* rv,
                         float* save_mean, float* save_invstd, float* ws, int N, int C, int HW, int dtype, int act,
                         int training, float momentum, float eps, void* plane_mean, hipStream_t st);
hipError_t launch_bn_prepare(const void* x, const float* gamma, const float* beta, float* rm, float* rv, float* save_mean,
                             float* save_invstd, float* scale_shift, float* ws, int N, int C, int HW, int dtype, int training,
                             float momentum, float eps, hipStream_t st);
hipError_t launch_bn_bwd(const void* x, const void* dout, const float* gamma, const float* beta, const float* save_mean,
                         const float* save_invstd, void* dx, float* dgamma, float* dbeta, float* ws, int N, int C, int HW,
                         int dtype, int act, int training, const void* dplane_mean, hipStream_t st);

// ---- bnse.hip (BN + activation inside the squeeze-excite gate: no materialised activation, forward and backward) ----------
size_t bn_gate_workspace_floats(int N, int C);
hipError_t launch_bn_act_mean(const void* x, const float* gamma, const float* beta, float* rm, float* rv, float* save_mean,
                              float* save_invstd, float* scale_shift, void* pooled, float* ws, int N, int C, int HW, int dtype,
                              int act, int training, float momentum, float eps, hipStream_t st);
hipError_t launch_bn_act_gate_fwd(const void* x, const float* scale_shift, const void* s, void* out, int N, int C, int HW, int dtype,
                                  int act, hipStream_t st);
hipError_t launch_bn_gate_bwd_sums(const void* x, const void* dout, const void* s, const float* scale_shift, const float* save_mean,
                                   const float* save_invstd, void* ds, float* ws, int N, int C, int HW, int dtype, int act,
                                   hipStream_t st);
hipError_t launch_bn_gate_bwd(const void* x, const void* dout, const void* s, const void* dpl, const float* scale_shift,
                              const float* save_mean, const float* save_invstd, void* dx, float* dgamma, float* dbeta, float* ws,
                              int N, int C, int HW, int dtype, int act, int training, hipStream_t st);

// ---- dwconv.hip (depthwise convolution, NCHW) -----------------------------------------------------
bool dwconv_supported(int K, int S);
size_t dwconv_workspace_floats(int C, int K);
// scale_shift (nullable, [C][2] fp32): the x the kernels see is act(x * scale[c] + shift[c]) rounded to the storage type, applied
// while the tile is filled (forward and backward-weight only; the padding stays zero)
hipError_t launch_dw_fwd(const void* x, const float* w, void* y, int N, int C, int H, int W, int OH, int OW, int K, int S,
                         int pt, int pl, int dtype, const float* scale_shift, int act, hipStream_t st);
hipError_t launch_dw_bwd_data(const void* dy, const float* w, void* dx, int N, int C, int H, int W, int OH, int OW, int K,
                              int S, int pt, int pl, int dtype, hipStream_t st);
hipError_t launch_dw_bwd_weight(const void* x, const void* dy, float* dw, float* ws, size_t ws_floats, int N, int C, int H,
                                int W, int OH, int OW, int K, int S, int pt, int pl, int dtype, const float* scale_shift, int act,
                                hipStream_t st);

// ---- pwconv.hip (pointwise convolution, NCHW: the weight gradient as a split-K bf16 MFMA product) ---------
size_t pwconv_workspace_floats(int N, int Cin, int Cout, int HW);
hipError_t launch_pw_bwd_weight(const void* x, const void* dy, void* dw, float* ws, int N, int Cin, int Cout, int HW,
                                hipStream_t st);

// ---- pwstream.hip (pointwise convolution, NCHW: forward and input gradient as one streaming bf16 MFMA product) ---------
hipError_t launch_pw_stream(const void* x, const void* w, void* y, int N, int Cin, int Cout, int HW, int transposed, hipStream_t st);

// ---- se.hip (squeeze-excite: per-plane mean, sigmoid gate) ----------------------------------------------
hipError_t launch_plane_mean(const void* x, void* out, int NC, int HW, int dtype, hipStream_t st);
hipError_t launch_se_gate_fwd(const void* x, const void* s, void* out, int NC, int HW, int dtype, hipStream_t st);
hipError_t launch_se_gate_bwd(const void* x, const void* s, const void* dout, void* dx, void* ds, int NC, int HW, int dtype,
                              hipStream_t st);

// ---- input.hip (the input batch: uint8 rows of a data pack -> normalised fp32 / bf16 images, NCHW or channels_last) -------------
hipError_t launch_input_batch(const uint8_t* src, const int64_t* idx, const uint8_t* flip, const int32_t* box, const float* lut,
                              void* out, int N, int H, int W, int B, int Sh, int Sw, int resample, int dtype, int layout,
                              hipStream_t st);

}  // namespace moma
