// extern "C" entry points of libmoma_hip.so (see include/moma_hip.h for the contract of each).
#include "common.hpp"

using namespace moma;

namespace {
inline int hip_rc(hipError_t e) { return e == hipSuccess ? MOMA_OK : (int)e; }
inline bool bad_prec(int p) { return p != MOMA_PREC_F32 && p != MOMA_PREC_BF16; }
inline bool bad_dt(int t) { return t != MOMA_DT_F32 && t != MOMA_DT_BF16; }
inline bool misaligned(const void* p, size_t a) { return ((uintptr_t)p % a) != 0; }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

#define MOMA_TRY(expr)                         \
    do {                                       \
        hipError_t _e = (expr);                \
        if (_e != hipSuccess) return (int)_e;  \
    } while (0)

GemmArgs gemm(const float* A, const void* B, float* C, int M, int N, int K, long lda, long ldb, long ldc, int tA,
              int tB, float alpha, int prec) {
    GemmArgs g{};
    g.A = A; g.B = B; g.C = C; g.bias = nullptr;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
    g.strideA = g.strideB = g.strideC = 0; g.batch = 1;
    g.transA = tA; g.transB = tB; g.alpha = alpha; g.splitk = 1; g.atomic = 0; g.splitC = 0;
    g.b_dtype = MOMA_DT_F32; g.prec = prec;
    return g;
}
}  // namespace

extern "C" {

int moma_version(void) { return MOMA_ABI_VERSION; }

int moma_debug_set_k2_target_wg(int n) { return set_k2_target_wg(n); }

const char* moma_error_string(int code) {
    switch (code) {
        case MOMA_OK: return "ok";
        case MOMA_E_NULL: return "moma: required pointer is NULL";
        case MOMA_E_SHAPE: return "moma: bad or inconsistent dimension";
        case MOMA_E_DTYPE: return "moma: unknown precision / queue dtype";
        case MOMA_E_ALIGN: return "moma: pointer not aligned to its element size";
        case MOMA_E_WORKSPACE: return "moma: workspace too small";
        case MOMA_E_UNSUPPORTED: return "moma: unsupported configuration";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "moma: unknown error";
    }
}

int moma_ema_multi(const int64_t* table, int n_tensors, int64_t total_blocks, float m, float one_minus_m,
                   moma_stream_t stream) {
    if (n_tensors == 0) return MOMA_OK;
    if (!table) return MOMA_E_NULL;
    if (n_tensors < 0 || total_blocks < 0 || total_blocks > 0x7fffffffLL) return MOMA_E_SHAPE;
    return hip_rc(launch_ema(table, n_tensors, total_blocks, m, one_minus_m, (hipStream_t)stream));
}

int moma_enqueue(void* queue, const float* rows, int n, int64_t index, int K, int d, int qdtype,
                 moma_stream_t stream) {
    if (n == 0) return MOMA_OK;
    if (!queue || !rows) return MOMA_E_NULL;
    if (n < 0 || K <= 0 || d <= 0 || index < 0 || index >= K) return MOMA_E_SHAPE;
    if (bad_dt(qdtype)) return MOMA_E_DTYPE;
    if (misaligned(rows, 4) || misaligned(queue, qdtype == MOMA_DT_BF16 ? 2 : 4)) return MOMA_E_ALIGN;
    return hip_rc(launch_enqueue(queue, rows, n, index, K, d, qdtype, (hipStream_t)stream));
}

int moma_enqueue_mirror(float* queue, void* mirror_bf16, const float* rows, int n, int64_t index, int K, int d,
                        moma_stream_t stream) {
    if (n == 0) return MOMA_OK;
    if (!queue || !mirror_bf16 || !rows) return MOMA_E_NULL;
    if (n < 0 || K <= 0 || d <= 0 || index < 0 || index >= K) return MOMA_E_SHAPE;
    if (misaligned(rows, 4) || misaligned(queue, 4) || misaligned(mirror_bf16, 2)) return MOMA_E_ALIGN;
    return hip_rc(launch_enqueue_mirror(queue, mirror_bf16, rows, n, index, K, d, (hipStream_t)stream));
}

int moma_queue_prefetch(const void* queue, size_t bytes, moma_stream_t stream) {
    if (bytes == 0) return MOMA_OK;
    if (!queue) return MOMA_E_NULL;
    if (misaligned(queue, 16)) return MOMA_E_ALIGN;
    return hip_rc(launch_prefetch(queue, bytes, (hipStream_t)stream));
}

int moma_infonce_logits(const float* q, const float* k, const void* queue, float* out, int B, int d, int K,
                        float inv_T, int qdtype, int prec, moma_stream_t stream) {
    if (!q || !k || !queue || !out) return MOMA_E_NULL;
    if (B <= 0 || d <= 0 || K <= 0) return MOMA_E_SHAPE;
    if (bad_dt(qdtype) || bad_prec(prec)) return MOMA_E_DTYPE;
    hipStream_t st = (hipStream_t)stream;
    const long ld = (long)K + 1;
    MOMA_TRY(launch_pos_logit(q, k, out, ld, B, d, inv_T, st));
    GemmArgs g = gemm(q, queue, out + 1, B, K, d, d, d, ld, 0, 0, inv_T, prec);   // neg = q . queue^T
    g.b_dtype = qdtype;
    return hip_rc(launch_gemm(g, st));
}

// dq = dlogits[:,0] k inv_T + dlogits[:,1:] . queue inv_T: the contraction over K is split over workgroups (B x d is a handful of
// output tiles).  With `parts` (splitk x B x d floats) every split writes its own partial product and a last launch adds them in
// split order -- bitwise reproducible; without it the splits meet in fp32 atomics (equal up to the order of the additions).
static int logits_bwd_splitk(int B, int d, int K) {
    const int tiles = ((B + 63) / 64) * ((d + 63) / 64);
    int splitk = (1024 + tiles - 1) / tiles;
    const int ktiles = (K + 31) / 32;
    if (splitk > ktiles) splitk = ktiles;
    return splitk < 1 ? 1 : splitk;
}
static size_t logits_bwd_parts_bytes(int B, int d, int K) {
    const int sk = logits_bwd_splitk(B, d, K);
    return sk > 1 ? align_up((size_t)sk * B * d * sizeof(float), 256) : 0;
}
static int logits_bwd_impl(const float* dlogits, const float* k, const void* queue, float* dq, int B, int d, int K, float inv_T,
                           int qdtype, int prec, hipStream_t st, float* parts) {
    const long ld = (long)K + 1;
    MOMA_TRY(launch_pos_grad_init(dlogits, ld, k, dq, B, d, inv_T, st));
    GemmArgs g = gemm(dlogits + 1, queue, dq, B, d, K, ld, d, d, 0, 1, inv_T, prec);
    g.b_dtype = qdtype;
    g.splitk = logits_bwd_splitk(B, d, K);
    if (parts != nullptr && g.splitk > 1) {
        g.C = parts;
        g.splitC = (long)B * d;
        MOMA_TRY(launch_gemm(g, st));
        return hip_rc(launch_add_partials(dq, parts, g.splitk, (long)B * d, (long)B * d, st));
    }
    g.atomic = 1;                     // (also splitk == 1: one split adds its product to the initialised dq)
    return hip_rc(launch_gemm(g, st));
}

int moma_infonce_logits_bwd(const float* dlogits, const float* k, const void* queue, float* dq, int B, int d,
                            int K, float inv_T, int qdtype, int prec, moma_stream_t stream) {
    if (!dlogits || !k || !queue || !dq) return MOMA_E_NULL;
    if (B <= 0 || d <= 0 || K <= 0) return MOMA_E_SHAPE;
    if (bad_dt(qdtype) || bad_prec(prec)) return MOMA_E_DTYPE;
    return logits_bwd_impl(dlogits, k, queue, dq, B, d, K, inv_T, qdtype, prec, (hipStream_t)stream, nullptr);
}

size_t moma_infonce_logits_bwd_workspace_bytes(int B, int d, int K) {
    if (B <= 0 || d <= 0 || K <= 0) return 0;
    const size_t b = logits_bwd_parts_bytes(B, d, K);
    return b ? b : 256;               // (never 0 for a valid shape: 0 is the error value of the *_bytes functions)
}

int moma_infonce_logits_bwd_ws(const float* dlogits, const float* k, const void* queue, float* dq, int B, int d, int K,
                               float inv_T, int qdtype, int prec, void* workspace, size_t workspace_bytes,
                               moma_stream_t stream) {
    if (!dlogits || !k || !queue || !dq || !workspace) return MOMA_E_NULL;
    if (B <= 0 || d <= 0 || K <= 0) return MOMA_E_SHAPE;
    if (bad_dt(qdtype) || bad_prec(prec)) return MOMA_E_DTYPE;
    if (workspace_bytes < moma_infonce_logits_bwd_workspace_bytes(B, d, K)) return MOMA_E_WORKSPACE;
    if (misaligned(workspace, 16)) return MOMA_E_ALIGN;
    return logits_bwd_impl(dlogits, k, queue, dq, B, d, K, inv_T, qdtype, prec, (hipStream_t)stream, (float*)workspace);
}

int moma_infonce_logits_bwd_kq(const float* dlogits, const float* q, float* dk, float* dqueue, int B, int d, int K,
                               float inv_T, int prec, moma_stream_t stream) {
    if (!dlogits || !q) return MOMA_E_NULL;
    if (B <= 0 || d <= 0 || K <= 0) return MOMA_E_SHAPE;
    if (bad_prec(prec)) return MOMA_E_DTYPE;
    hipStream_t st = (hipStream_t)stream;
    const long ld = (long)K + 1;
    if (dk) MOMA_TRY(launch_pos_grad_init(dlogits, ld, q, dk, B, d, inv_T, st));
    if (dqueue) {
        // dqueue[j,c] = sum_b dlogits[b,1+j] * q[b,c]
        GemmArgs g = gemm(dlogits + 1, q, dqueue, K, d, B, ld, d, d, 1, 1, inv_T, prec);
        MOMA_TRY(launch_gemm(g, st));
    }
    return MOMA_OK;
}

// Exact-fp32 policy over a bf16-STORED queue at a width the one-pass fp32 kernel takes: the queue is widened (bf16 -> fp32 is
// exact) into the workspace and that kernel streams the copy -- 64 MB read + 128 MB written at K x d = 65536 x 512 (~35 us) in front
// of a 378 us pass, against 807 us for the staged path with its [B,K+1] logits (round 5).  The copy lives for the call only.
static bool f32_policy_widens_queue(int B, int d, int K, int qdtype, int prec) {
    return prec == MOMA_PREC_F32 && qdtype == MOMA_DT_BF16 && infonce_f32_flash_supported(B, d, K, MOMA_DT_F32, prec);
}

size_t moma_infonce_fused_workspace_bytes(int B, int d, int K, int qdtype, int prec) {
    if (B <= 0 || d <= 0 || K <= 0) return 0;
    if (infonce_flash_supported(B, d, K, qdtype, prec)) return infonce_flash_workspace_bytes(B, d, K);
    if (infonce_f32_flash_supported(B, d, K, qdtype, prec)) return infonce_f32_flash_workspace_bytes(B, d, K);
    if (f32_policy_widens_queue(B, d, K, qdtype, prec))
        return align_up((size_t)K * d * sizeof(float), 256) + infonce_f32_flash_workspace_bytes(B, d, K);
    return align_up((size_t)B * ((size_t)K + 1) * sizeof(float), 256) + logits_bwd_parts_bytes(B, d, K);     // logits | split-K partials of dq
}

int moma_infonce_fused(const float* q, const float* k, const void* queue, int B, int d, int K, float inv_T,
                       float* loss_rows, float* lse, int32_t* top1, float* dq, void* workspace,
                       size_t workspace_bytes, int qdtype, int prec, moma_stream_t stream) {
    return moma_infonce_fused_ex(q, k, queue, B, d, K, inv_T, loss_rows, lse, top1, dq, workspace, workspace_bytes,
                                 qdtype, prec, stream, nullptr, nullptr);
}

int moma_infonce_fused_ex(const float* q, const float* k, const void* queue, int B, int d, int K, float inv_T,
                          float* loss_rows, float* lse, int32_t* top1, float* dq, void* workspace,
                          size_t workspace_bytes, int qdtype, int prec, moma_stream_t stream, void* ev_begin,
                          void* ev_end) {
    return moma_infonce_fused_q(q, nullptr, k, queue, B, d, K, inv_T, loss_rows, lse, top1, dq, workspace, workspace_bytes,
                                qdtype, prec, stream, ev_begin, ev_end, nullptr);
}

size_t moma_infonce_qpack_bytes(int B, int d) { return infonce_qpack_bytes(B, d); }

// K2 (+ K3 when `job` names rows): the enqueue rides on the call's last launch where the path has a combine launch to carry it
// (*carried = 1), else the caller launches it behind the call
static int fused_impl(const float* q, const void* q_packed, const float* k, const void* queue, int B, int d, int K,
                      float inv_T, float* loss_rows, float* lse, int32_t* top1, float* dq, void* workspace,
                      size_t workspace_bytes, int qdtype, int prec, moma_stream_t stream, void* ev_begin, void* ev_end,
                      void* ev_call_end, const EnqueueJob* job, int* carried) {
    if (carried) *carried = 0;
    if (!q || !k || !queue || !loss_rows || !lse || !top1 || !workspace) return MOMA_E_NULL;
    if (B <= 0 || d <= 0 || K <= 0) return MOMA_E_SHAPE;
    if (bad_dt(qdtype) || bad_prec(prec)) return MOMA_E_DTYPE;
    if (workspace_bytes < moma_infonce_fused_workspace_bytes(B, d, K, qdtype, prec)) return MOMA_E_WORKSPACE;
    if (misaligned(workspace, 16)) return MOMA_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    if (q_packed && (misaligned(q_packed, 16) || infonce_qpack_bytes(B, d) == 0 || !infonce_flash_supported(B, d, K, qdtype, prec)))
        return q_packed && misaligned(q_packed, 16) ? MOMA_E_ALIGN : MOMA_E_UNSUPPORTED;
    // the one-pass kernels move q / k / dq in 16-byte pieces and the queue by 16-byte LDS-DMA: operands that start inside a vector
    // (an element-granular view of a larger buffer) are refused here instead of faulting there
    const bool one_pass = infonce_flash_supported(B, d, K, qdtype, prec) || infonce_f32_flash_supported(B, d, K, qdtype, prec) ||
                          f32_policy_widens_queue(B, d, K, qdtype, prec);
    if (one_pass && (misaligned(q, 16) || misaligned(k, 16) || misaligned(queue, 16) || (dq && misaligned(dq, 16)))) return MOMA_E_ALIGN;
    if (!one_pass && (misaligned(q, 4) || misaligned(k, 4) || misaligned(queue, qdtype == MOMA_DT_BF16 ? 2 : 4) || (dq && misaligned(dq, 4))))
        return MOMA_E_ALIGN;
    if (infonce_flash_supported(B, d, K, qdtype, prec)) {
        if (carried) *carried = 1;
        return hip_rc(launch_infonce_flash(q, k, queue, B, d, K, inv_T, loss_rows, lse, top1, dq, workspace, qdtype, st,
                                           (hipEvent_t)ev_begin, (hipEvent_t)ev_end, q_packed, (hipEvent_t)ev_call_end, job));
    }
    if (infonce_f32_flash_supported(B, d, K, qdtype, prec))      // exact fp32, fp32 queue: one pass, no [B,K+1] logits
    {
        const int rc = hip_rc(launch_infonce_f32_flash(q, k, (const float*)queue, B, d, K, inv_T, loss_rows, lse, top1, dq, workspace, st,
                                                       (hipEvent_t)ev_begin, (hipEvent_t)ev_end));
        if (ev_call_end) (void)hipEventRecord((hipEvent_t)ev_call_end, st);
        return rc;
    }
    if (f32_policy_widens_queue(B, d, K, qdtype, prec)) {
        if (misaligned(queue, 16)) return MOMA_E_ALIGN;
        float* wide = (float*)workspace;
        void* ws2 = (char*)workspace + align_up((size_t)K * d * sizeof(float), 256);
        // (the measurement span opens IN FRONT of the widening pass: 64 MB read + 128 MB written per call at the bench shape belong
        //  to what this policy costs -- ADVICE r5)
        if (ev_begin) (void)hipEventRecord((hipEvent_t)ev_begin, st);
        MOMA_TRY(launch_widen_bf16(queue, wide, (size_t)K * d, st));
        const int rc = hip_rc(launch_infonce_f32_flash(q, k, wide, B, d, K, inv_T, loss_rows, lse, top1, dq, ws2, st,
                                                       (hipEvent_t) nullptr, (hipEvent_t)ev_end));
        if (ev_call_end) (void)hipEventRecord((hipEvent_t)ev_call_end, st);
        return rc;
    }
    // staged path (any shape, exact fp32 available): logits -> row reduction -> gradient product
    float* logits = (float*)workspace;
    if (ev_begin) (void)hipEventRecord((hipEvent_t)ev_begin, st);
    int rc = moma_infonce_logits(q, k, queue, logits, B, d, K, inv_T, qdtype, prec, stream);
    if (ev_end) (void)hipEventRecord((hipEvent_t)ev_end, st);
    if (rc != MOMA_OK) return rc;
    MOMA_TRY(launch_infonce_rows(logits, B, K + 1, loss_rows, lse, top1, dq != nullptr, st));
    if (dq) {
        float* parts = (float*)((char*)workspace + align_up((size_t)B * ((size_t)K + 1) * sizeof(float), 256));
        rc = logits_bwd_impl(logits, k, queue, dq, B, d, K, inv_T, qdtype, prec, st, logits_bwd_parts_bytes(B, d, K) ? parts : nullptr);
    }
    if (ev_call_end) (void)hipEventRecord((hipEvent_t)ev_call_end, st);
    return rc;
}

int moma_infonce_fused_q(const float* q, const void* q_packed, const float* k, const void* queue, int B, int d, int K,
                         float inv_T, float* loss_rows, float* lse, int32_t* top1, float* dq, void* workspace,
                         size_t workspace_bytes, int qdtype, int prec, moma_stream_t stream, void* ev_begin, void* ev_end,
                         void* ev_call_end) {
    return fused_impl(q, q_packed, k, queue, B, d, K, inv_T, loss_rows, lse, top1, dq, workspace, workspace_bytes, qdtype, prec, stream,
                      ev_begin, ev_end, ev_call_end, nullptr, nullptr);
}

int moma_infonce_fused_enqueue(const float* q, const void* q_packed, const float* k, void* queue, int B, int d, int K,
                               float inv_T, float* loss_rows, float* lse, int32_t* top1, float* dq, void* workspace,
                               size_t workspace_bytes, int qdtype, int prec, const float* rows, int n, int64_t index,
                               float* queue_f32, moma_stream_t stream, void* ev_begin, void* ev_end, void* ev_call_end) {
    if (n < 0 || K <= 0 || index < 0 || index >= K) return MOMA_E_SHAPE;
    if (n > 0 && !rows) return MOMA_E_NULL;
    if (bad_dt(qdtype)) return MOMA_E_DTYPE;
    if (queue_f32 && qdtype != MOMA_DT_BF16) return MOMA_E_DTYPE;          // (a mirror is the bf16 image of an fp32 queue)
    if (n > 0 && (misaligned(rows, 4) || misaligned(queue, qdtype == MOMA_DT_BF16 ? 2 : 4) || (queue_f32 && misaligned(queue_f32, 4))))
        return MOMA_E_ALIGN;
    EnqueueJob job{qdtype == MOMA_DT_BF16 ? queue : nullptr, qdtype == MOMA_DT_BF16 ? queue_f32 : (float*)queue, rows, n, index, K, d};
    int carried = 0;
    const int rc = fused_impl(q, q_packed, k, queue, B, d, K, inv_T, loss_rows, lse, top1, dq, workspace, workspace_bytes, qdtype, prec,
                              stream, ev_begin, ev_end, ev_call_end, n > 0 ? &job : nullptr, &carried);
    if (rc != MOMA_OK || carried || n == 0) return rc;
    // a path without a combine launch (exact fp32, staged): the enqueue as its own launch, behind the call on the stream
    if (queue_f32) return hip_rc(launch_enqueue_mirror(queue_f32, queue, rows, n, index, K, d, (hipStream_t)stream));
    return hip_rc(launch_enqueue(queue, rows, n, index, K, d, qdtype, (hipStream_t)stream));
}

size_t moma_infonce_fused_multi_workspace_bytes(int n_terms, int B, int d, int K, int qdtype, int prec) {
    if (n_terms < 1 || n_terms > 4 || B <= 0 || d <= 0 || K <= 0 || bad_dt(qdtype) || bad_prec(prec)) return 0;
    if (infonce_multi_supported(n_terms, B, d, K, qdtype, prec)) return infonce_multi_workspace_bytes(n_terms, B, d, K);
    // no one-sweep kernel for this configuration (wide rows, exact fp32, fp32 queue under the bf16 policy): the terms go through
    // moma_infonce_fused's own path one after the other on the stream and share ONE workspace of that call's size
    return moma_infonce_fused_workspace_bytes(B, d, K, qdtype, prec);
}

int moma_infonce_fused_multi(const moma_infonce_term_t* terms, int n_terms, int B, int d, int K, float inv_T, void* workspace,
                             size_t workspace_bytes, int qdtype, int prec, moma_stream_t stream) {
    if (!terms || !workspace) return MOMA_E_NULL;
    if (n_terms < 1 || n_terms > 4 || B <= 0 || d <= 0 || K <= 0) return MOMA_E_SHAPE;
    if (bad_dt(qdtype) || bad_prec(prec)) return MOMA_E_DTYPE;
    for (int i = 0; i < n_terms; ++i) {
        const moma_infonce_term_t& t = terms[i];
        if (!t.q || !t.k || !t.queue || !t.loss_rows || !t.lse || !t.top1) return MOMA_E_NULL;
        if ((t.dq != nullptr) != (terms[0].dq != nullptr)) return MOMA_E_UNSUPPORTED;     // every term with dq, or none
        if (misaligned(t.q, 16) || misaligned(t.k, 4) || misaligned(t.queue, 16)) return MOMA_E_ALIGN;
    }
    if (workspace_bytes < moma_infonce_fused_multi_workspace_bytes(n_terms, B, d, K, qdtype, prec)) return MOMA_E_WORKSPACE;
    if (misaligned(workspace, 16)) return MOMA_E_ALIGN;
    if (infonce_multi_supported(n_terms, B, d, K, qdtype, prec))
        return hip_rc(launch_infonce_multi(terms, n_terms, B, d, K, inv_T, workspace, (hipStream_t)stream));
    // term by term (stream order makes the shared workspace safe).  At these shapes every term's passes already fill the chip and
    // are bound by the matrix pipe / L2 delivery, not by HBM (d = 1280 bf16: 1.2 TB/s; exact fp32: 0.35 TB/s): merging the terms'
    // launches would not read the queues any less
    for (int i = 0; i < n_terms; ++i) {
        const moma_infonce_term_t& t = terms[i];
        const int rc = moma_infonce_fused_q(t.q, nullptr, t.k, t.queue, B, d, K, inv_T, t.loss_rows, t.lse, t.top1, t.dq, workspace,
                                            workspace_bytes, qdtype, prec, stream, nullptr, nullptr, nullptr);
        if (rc != MOMA_OK) return rc;
    }
    return MOMA_OK;
}

int moma_mha_saved_state(int N, int d, int H, int prec) {
    if (N <= 0 || d <= 0 || H <= 0 || d % H != 0 || bad_prec(prec)) return MOMA_E_SHAPE;
    return mha_fast_supported(N, d, H, prec) ? MOMA_MHA_SAVE_LSE : MOMA_MHA_SAVE_PROBS;
}

int moma_mha_fwd(const float* x, const float* w_qkv, const float* b_qkv, const float* w_proj, const float* b_proj,
                 float* y, float* qkv, float* probs, float* attn_out, int N, int d, int H, int prec,
                 moma_stream_t stream) {
    if (!x || !w_qkv || !w_proj || !b_proj || !y || !qkv || !attn_out || !probs) return MOMA_E_NULL;
    if (N <= 0 || d <= 0 || H <= 0 || d % H != 0) return MOMA_E_SHAPE;
    if (bad_prec(prec)) return MOMA_E_DTYPE;
    hipStream_t st = (hipStream_t)stream;
    const int hd = d / H;
    const float scale = 1.0f / sqrtf((float)hd);
    // qkv = x Wqkv^T + b                                   (MoMA/criterion_moco_att.py:156)
    GemmArgs g = gemm(x, w_qkv, qkv, N, 3 * d, d, d, d, 3L * d, 0, 0, 1.f, prec);
    g.bias = b_qkv;
    MOMA_TRY(launch_gemm(g, st));
    // per head: S = (q k^T) * scale                          (:159)
    g = gemm(qkv, qkv + d, probs, N, N, hd, 3L * d, 3L * d, N, 0, 0, scale, prec);
    g.batch = H; g.strideA = hd; g.strideB = hd; g.strideC = (long)N * N;
    MOMA_TRY(launch_gemm(g, st));
    MOMA_TRY(launch_softmax_rows(probs, (long)H * N, N, st));                      // :160
    // per head: a[:, h*hd:(h+1)*hd] = P v                   (:163)
    g = gemm(probs, qkv + 2 * d, attn_out, N, hd, N, N, 3L * d, d, 0, 1, 1.f, prec);
    g.batch = H; g.strideA = (long)N * N; g.strideB = hd; g.strideC = hd;
    MOMA_TRY(launch_gemm(g, st));
    // y = a Wproj^T + b                                      (:164)
    g = gemm(attn_out, w_proj, y, N, d, d, d, d, d, 0, 0, 1.f, prec);
    g.bias = b_proj;
    return hip_rc(launch_gemm(g, st));
}

size_t moma_mha_bwd_workspace_bytes(int N, int d, int H, int prec) {
    if (N <= 0 || d <= 0 || H <= 0 || d % H != 0 || bad_prec(prec)) return 0;
    // dA [N,d] + dP [H,N,N] + dqkv [N,3d]
    return align_up(((size_t)N * d + (size_t)H * N * N + (size_t)N * 3 * d) * sizeof(float), 256);
}

int moma_mha_bwd(const float* x, const float* w_qkv, const float* w_proj, const float* qkv, const float* probs,
                 const float* attn_out, const float* dy, float* dx, float* dw_qkv, float* db_qkv,
                 float* dw_proj, float* db_proj, void* workspace, size_t workspace_bytes, int N, int d, int H, int prec,
                 moma_stream_t stream) {
    if (!x || !w_qkv || !w_proj || !qkv || !attn_out || !dy || !workspace || !probs) return MOMA_E_NULL;
    if (N <= 0 || d <= 0 || H <= 0 || d % H != 0) return MOMA_E_SHAPE;
    if (bad_prec(prec)) return MOMA_E_DTYPE;
    if (workspace_bytes < moma_mha_bwd_workspace_bytes(N, d, H, prec)) return MOMA_E_WORKSPACE;
    if (misaligned(workspace, 16)) return MOMA_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int hd = d / H;
    const float scale = 1.0f / sqrtf((float)hd);
    float* dA = (float*)workspace;
    float* dP = dA + (size_t)N * d;
    float* dqkv = dP + (size_t)H * N * N;
    GemmArgs g;
    // proj: dWproj = dy^T a ; dbproj = colsum(dy) ; dA = dy Wproj
    bool db_done = false;
    if (dw_proj) {
        g = gemm(dy, attn_out, dw_proj, d, d, N, d, d, d, 1, 1, 1.f, prec);
        if (db_proj && gemm_fuses_colsum(g)) { g.colsum_a = db_proj; db_done = true; }       // the bias gradient rides along
        MOMA_TRY(launch_gemm(g, st));
    }
    if (db_proj && !db_done) MOMA_TRY(launch_colsum(dy, db_proj, N, d, d, st));
    g = gemm(dy, w_proj, dA, N, d, d, d, d, d, 0, 1, 1.f, prec);
    MOMA_TRY(launch_gemm(g, st));
    // per head: dV = P^T dA_h  -> dqkv[:, 2d + h*hd ...]
    g = gemm(probs, dA, dqkv + 2 * d, N, hd, N, N, d, 3L * d, 1, 1, 1.f, prec);
    g.batch = H; g.strideA = (long)N * N; g.strideB = hd; g.strideC = hd;
    MOMA_TRY(launch_gemm(g, st));
    // per head: dP = dA_h V^T
    g = gemm(dA, qkv + 2 * d, dP, N, N, hd, d, 3L * d, N, 0, 0, 1.f, prec);
    g.batch = H; g.strideA = hd; g.strideB = hd; g.strideC = (long)N * N;
    MOMA_TRY(launch_gemm(g, st));
    // dS = P * (dP - rowsum(dP*P)) * scale   (in place on dP)
    MOMA_TRY(launch_softmax_bwd_rows(probs, dP, (long)H * N, N, scale, st));
    // per head: dQ = dS K ; dK = dS^T Q
    g = gemm(dP, qkv + d, dqkv, N, hd, N, N, 3L * d, 3L * d, 0, 1, 1.f, prec);
    g.batch = H; g.strideA = (long)N * N; g.strideB = hd; g.strideC = hd;
    MOMA_TRY(launch_gemm(g, st));
    g = gemm(dP, qkv, dqkv + d, N, hd, N, N, 3L * d, 3L * d, 1, 1, 1.f, prec);
    g.batch = H; g.strideA = (long)N * N; g.strideB = hd; g.strideC = hd;
    MOMA_TRY(launch_gemm(g, st));
    // qkv linear: dWqkv = dqkv^T x ; dbqkv = colsum(dqkv) ; dx = dqkv Wqkv
    db_done = false;
    if (dw_qkv) {
        g = gemm(dqkv, x, dw_qkv, 3 * d, d, N, 3L * d, d, d, 1, 1, 1.f, prec);
        if (db_qkv && gemm_fuses_colsum(g)) { g.colsum_a = db_qkv; db_done = true; }
        MOMA_TRY(launch_gemm(g, st));
    }
    if (db_qkv && !db_done) MOMA_TRY(launch_colsum(dqkv, db_qkv, N, 3 * d, 3L * d, st));
    if (dx) {
        g = gemm(dqkv, w_qkv, dx, N, d, 3 * d, 3L * d, d, d, 0, 1, 1.f, prec);
        MOMA_TRY(launch_gemm(g, st));
    }
    return MOMA_OK;
}

// ---- K1 fast path (k1_fast.hip) ----------------------------------------------------------------------------------
size_t moma_mha_pack_bytes(int d) { return d > 0 ? (size_t)16 * d * d : 0; }

int moma_mha_pack_weights(const float* w_qkv, const float* w_proj, void* pack, int d, int with_transposed,
                          moma_stream_t stream) {
    if (!w_qkv || !w_proj || !pack) return MOMA_E_NULL;
    if (d <= 0 || d % 16 != 0) return MOMA_E_SHAPE;
    if (misaligned(pack, 16) || misaligned(w_qkv, 4) || misaligned(w_proj, 4)) return MOMA_E_ALIGN;
    return hip_rc(launch_mha_pack(w_qkv, w_proj, pack, d, with_transposed != 0, (hipStream_t)stream));
}

int moma_mha_fwd_fast(const moma_mha_module_t* mods, int n_modules, int N, int d, int H, moma_stream_t stream) {
    if (!mods) return MOMA_E_NULL;
    if (n_modules < 1 || n_modules > 4 || N <= 0 || d <= 0 || H <= 0 || d % H != 0) return MOMA_E_SHAPE;
    if (!mha_fast_supported(N, d, H, MOMA_PREC_BF16)) return MOMA_E_UNSUPPORTED;
    for (int i = 0; i < n_modules; ++i) {
        const moma_mha_module_t& m = mods[i];
        if (!m.x || !m.pack || !m.b_proj || !m.y || !m.qkv16 || !m.attn16) return MOMA_E_NULL;
        if (bad_dt(m.x_dtype)) return MOMA_E_DTYPE;
        if (misaligned(m.x, 16) || misaligned(m.pack, 16) || misaligned(m.y, 16) || misaligned(m.qkv16, 16) ||
            misaligned(m.attn16, 16) || misaligned(m.b_proj, 16) || (m.b_qkv && misaligned(m.b_qkv, 16)) ||
            (m.qpack && misaligned(m.qpack, 16)))
            return MOMA_E_ALIGN;
    }
    return hip_rc(launch_mha_fwd_fast(mods, n_modules, N, d, H, (hipStream_t)stream));
}

size_t moma_mha_bwd_fast_workspace_bytes(int N, int d, int H) {
    if (N <= 0 || d <= 0 || H <= 0 || d % H != 0) return 0;
    return mha_bwd_fast_workspace_bytes(N, d);
}

int moma_mha_bwd_fast(const void* pack, const void* x, int x_dtype, const void* qkv16, const void* attn16, const float* lse,
                      const float* dy, float* dx, float* dw_qkv, float* db_qkv, float* dw_proj, float* db_proj,
                      void* workspace, size_t workspace_bytes, int N, int d, int H, moma_stream_t stream) {
    if (!pack || !x || !qkv16 || !attn16 || !lse || !dy || !workspace) return MOMA_E_NULL;
    if (N <= 0 || d <= 0 || H <= 0 || d % H != 0) return MOMA_E_SHAPE;
    if (!mha_fast_supported(N, d, H, MOMA_PREC_BF16)) return MOMA_E_UNSUPPORTED;
    if (bad_dt(x_dtype)) return MOMA_E_DTYPE;
    if ((db_qkv && !dw_qkv) || (db_proj && !dw_proj)) return MOMA_E_UNSUPPORTED;      // a bias gradient rides on its weight gradient
    if (workspace_bytes < mha_bwd_fast_workspace_bytes(N, d)) return MOMA_E_WORKSPACE;
    if (misaligned(workspace, 16) || misaligned(pack, 16) || misaligned(x, 16) || misaligned(qkv16, 16) ||
        misaligned(attn16, 16) || misaligned(dy, 16) || (dx && misaligned(dx, 16)) || (dw_qkv && misaligned(dw_qkv, 8)) ||
        (dw_proj && misaligned(dw_proj, 8)))
        return MOMA_E_ALIGN;
    return hip_rc(launch_mha_bwd_fast(pack, x, x_dtype, qkv16, attn16, lse, dy, dx, dw_qkv, db_qkv, dw_proj, db_proj, workspace, N, d,
                                      H, (hipStream_t)stream));
}

size_t moma_bn_workspace_bytes(int C) { return C > 0 ? align_up(bn_workspace_floats(C) * sizeof(float), 256) : 0; }

static int bn_check(int N, int C, int HW, int dtype, int act, const void* ws, size_t ws_bytes) {
    if (N <= 0 || C <= 0 || HW <= 0 || (long)N * C > 0x7fffffffL || (long)N * HW > 0x7fffffffL) return MOMA_E_SHAPE;
    if (dtype != MOMA_DT_F32 && dtype != MOMA_DT_BF16) return MOMA_E_DTYPE;
    if (act != MOMA_ACT_NONE && act != MOMA_ACT_SILU && act != MOMA_ACT_RELU) return MOMA_E_DTYPE;
    if (!ws) return MOMA_E_NULL;
    if (ws_bytes < moma_bn_workspace_bytes(C)) return MOMA_E_WORKSPACE;
    return MOMA_OK;
}

int moma_bn_fwd(const void* x, void* out, const float* gamma, const float* beta, float* running_mean,
                float* running_var, float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes,
                int N, int C, int HW, int dtype, int act, int training, float momentum, float eps, void* plane_mean,
                moma_stream_t stream) {
    if (!x || !out) return MOMA_E_NULL;
    if (!training && (!running_mean || !running_var)) return MOMA_E_NULL;
    const int rc = bn_check(N, C, HW, dtype, act, workspace, workspace_bytes);
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_bn_fwd(x, out, gamma, beta, running_mean, running_var, save_mean, save_invstd,
                                (float*)workspace, N, C, HW, dtype, act, training, momentum, eps, plane_mean, (hipStream_t)stream));
}

int moma_bn_prepare(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                    float* save_mean, float* save_invstd, float* scale_shift, void* workspace, size_t workspace_bytes, int N,
                    int C, int HW, int dtype, int training, float momentum, float eps, moma_stream_t stream) {
    if (!x || !save_mean || !save_invstd || !scale_shift) return MOMA_E_NULL;
    if (!training && (!running_mean || !running_var)) return MOMA_E_NULL;
    const int rc = bn_check(N, C, HW, dtype, MOMA_ACT_NONE, workspace, workspace_bytes);
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_bn_prepare(x, gamma, beta, running_mean, running_var, save_mean, save_invstd, scale_shift,
                                    (float*)workspace, N, C, HW, dtype, training, momentum, eps, (hipStream_t)stream));
}

int moma_bn_bwd(const void* x, const void* dout, const float* gamma, const float* beta, const float* save_mean,
                const float* save_invstd, void* dx, float* dgamma, float* dbeta, void* workspace,
                size_t workspace_bytes, int N, int C, int HW, int dtype, int act, int training,
                const void* dplane_mean, moma_stream_t stream) {
    if (!x || !dout || !save_mean || !save_invstd) return MOMA_E_NULL;
    const int rc = bn_check(N, C, HW, dtype, act, workspace, workspace_bytes);
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_bn_bwd(x, dout, gamma, beta, save_mean, save_invstd, dx, dgamma, dbeta, (float*)workspace, N,
                                C, HW, dtype, act, training, dplane_mean, (hipStream_t)stream));
}

// ---- BN + activation inside the squeeze-excite gate (bnse.hip) --------------------------------------------------------------
size_t moma_bn_gate_workspace_bytes(int N, int C) {
    return (N > 0 && C > 0 && (long)N * C <= 0x7fffffffL / 4) ? align_up(bn_gate_workspace_floats(N, C) * sizeof(float), 256) : 0;
}

static int bn_gate_check(int N, int C, int HW, int dtype, int act, const void* ws, size_t ws_bytes) {
    if (N <= 0 || C <= 0 || HW <= 0 || (long)N * C > 0x7fffffffL / 4 || (long)N * HW > 0x7fffffffL) return MOMA_E_SHAPE;
    if (dtype != MOMA_DT_F32 && dtype != MOMA_DT_BF16) return MOMA_E_DTYPE;
    if (act != MOMA_ACT_NONE && act != MOMA_ACT_SILU && act != MOMA_ACT_RELU) return MOMA_E_DTYPE;
    if (!ws) return MOMA_E_NULL;
    if (misaligned(ws, 16)) return MOMA_E_ALIGN;
    if (ws_bytes < moma_bn_gate_workspace_bytes(N, C)) return MOMA_E_WORKSPACE;
    return MOMA_OK;
}

int moma_bn_act_mean(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                     float* save_mean, float* save_invstd, float* scale_shift, void* pooled, void* workspace,
                     size_t workspace_bytes, int N, int C, int HW, int dtype, int act, int training, float momentum, float eps,
                     moma_stream_t stream) {
    if (!x || !save_mean || !save_invstd || !scale_shift || !pooled) return MOMA_E_NULL;
    if (!training && (!running_mean || !running_var)) return MOMA_E_NULL;
    const int rc = bn_check(N, C, HW, dtype, act, workspace, workspace_bytes);
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_bn_act_mean(x, gamma, beta, running_mean, running_var, save_mean, save_invstd, scale_shift, pooled,
                                     (float*)workspace, N, C, HW, dtype, act, training, momentum, eps, (hipStream_t)stream));
}

int moma_bn_act_gate_fwd(const void* x, const float* scale_shift, const void* s, void* out, int N, int C, int HW, int dtype,
                         int act, moma_stream_t stream) {
    if (!x || !scale_shift || !s || !out) return MOMA_E_NULL;
    if (N <= 0 || C <= 0 || HW <= 0 || (long)N * C > 0x7fffffffL) return MOMA_E_SHAPE;
    if (dtype != MOMA_DT_F32 && dtype != MOMA_DT_BF16) return MOMA_E_DTYPE;
    if (act != MOMA_ACT_NONE && act != MOMA_ACT_SILU && act != MOMA_ACT_RELU) return MOMA_E_DTYPE;
    return hip_rc(launch_bn_act_gate_fwd(x, scale_shift, s, out, N, C, HW, dtype, act, (hipStream_t)stream));
}

int moma_bn_gate_bwd_sums(const void* x, const void* dout, const void* s, const float* scale_shift, const float* save_mean,
                          const float* save_invstd, void* ds, void* workspace, size_t workspace_bytes, int N, int C, int HW,
                          int dtype, int act, moma_stream_t stream) {
    if (!x || !dout || !s || !scale_shift || !save_mean || !save_invstd) return MOMA_E_NULL;
    const int rc = bn_gate_check(N, C, HW, dtype, act, workspace, workspace_bytes);
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_bn_gate_bwd_sums(x, dout, s, scale_shift, save_mean, save_invstd, ds, (float*)workspace, N, C, HW, dtype,
                                          act, (hipStream_t)stream));
}

int moma_bn_gate_bwd(const void* x, const void* dout, const void* s, const void* dpooled, const float* scale_shift,
                     const float* save_mean, const float* save_invstd, void* dx, float* dgamma, float* dbeta, void* workspace,
                     size_t workspace_bytes, int N, int C, int HW, int dtype, int act, int training, moma_stream_t stream) {
    if (!x || !dout || !s || !scale_shift || !save_mean || !save_invstd) return MOMA_E_NULL;
    const int rc = bn_gate_check(N, C, HW, dtype, act, workspace, workspace_bytes);
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_bn_gate_bwd(x, dout, s, dpooled, scale_shift, save_mean, save_invstd, dx, dgamma, dbeta, (float*)workspace,
                                     N, C, HW, dtype, act, training, (hipStream_t)stream));
}

size_t moma_dwconv_workspace_bytes(int C, int K) {
    return (C > 0 && K > 0) ? align_up(dwconv_workspace_floats(C, K) * sizeof(float), 256) : 0;
}

static int dw_check(int N, int C, int H, int W, int OH, int OW, int K, int S, int pt, int pl, int dtype) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || (long)N * C > 0x7fffffffL) return MOMA_E_SHAPE;
    if (!dwconv_supported(K, S)) return MOMA_E_SHAPE;
    if (pt < 0 || pl < 0 || pt >= K || pl >= K) return MOMA_E_SHAPE;
    // every output must read at least its first tap row/column inside the padded image
    if ((long)(OH - 1) * S - pt >= H || (long)(OW - 1) * S - pl >= W) return MOMA_E_SHAPE;
    if (dtype != MOMA_DT_F32 && dtype != MOMA_DT_BF16) return MOMA_E_DTYPE;
    return MOMA_OK;
}

int moma_dwconv_fwd(const void* x, const float* w, void* y, int N, int C, int H, int W, int OH, int OW, int K, int stride,
                    int pad_top, int pad_left, int dtype, moma_stream_t stream) {
    if (!x || !w || !y) return MOMA_E_NULL;
    const int rc = dw_check(N, C, H, W, OH, OW, K, stride, pad_top, pad_left, dtype);
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_dw_fwd(x, w, y, N, C, H, W, OH, OW, K, stride, pad_top, pad_left, dtype, nullptr, MOMA_ACT_NONE,
                                (hipStream_t)stream));
}

static bool bad_act(int act) { return act != MOMA_ACT_NONE && act != MOMA_ACT_SILU && act != MOMA_ACT_RELU; }

int moma_dwconv_fwd_pre(const void* x, const float* w, void* y, int N, int C, int H, int W, int OH, int OW, int K, int stride,
                        int pad_top, int pad_left, int dtype, const float* scale_shift, int act, moma_stream_t stream) {
    if (!x || !w || !y || !scale_shift) return MOMA_E_NULL;
    const int rc = dw_check(N, C, H, W, OH, OW, K, stride, pad_top, pad_left, dtype);
    if (rc != MOMA_OK) return rc;
    if (bad_act(act)) return MOMA_E_DTYPE;
    return hip_rc(launch_dw_fwd(x, w, y, N, C, H, W, OH, OW, K, stride, pad_top, pad_left, dtype, scale_shift, act,
                                (hipStream_t)stream));
}

int moma_dwconv_bwd_data(const void* dy, const float* w, void* dx, int N, int C, int H, int W, int OH, int OW, int K,
                         int stride, int pad_top, int pad_left, int dtype, moma_stream_t stream) {
    if (!dy || !w || !dx) return MOMA_E_NULL;
    const int rc = dw_check(N, C, H, W, OH, OW, K, stride, pad_top, pad_left, dtype);
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_dw_bwd_data(dy, w, dx, N, C, H, W, OH, OW, K, stride, pad_top, pad_left, dtype, (hipStream_t)stream));
}

int moma_dwconv_bwd_weight(const void* x, const void* dy, float* dw, void* workspace, size_t workspace_bytes, int N, int C,
                           int H, int W, int OH, int OW, int K, int stride, int pad_top, int pad_left, int dtype,
                           moma_stream_t stream) {
    if (!x || !dy || !dw || !workspace) return MOMA_E_NULL;
    const int rc = dw_check(N, C, H, W, OH, OW, K, stride, pad_top, pad_left, dtype);
    if (rc != MOMA_OK) return rc;
    if (workspace_bytes < moma_dwconv_workspace_bytes(C, K)) return MOMA_E_WORKSPACE;
    return hip_rc(launch_dw_bwd_weight(x, dy, dw, (float*)workspace, workspace_bytes / sizeof(float), N, C, H, W, OH, OW, K,
                                       stride, pad_top, pad_left, dtype, nullptr, MOMA_ACT_NONE, (hipStream_t)stream));
}

int moma_dwconv_bwd_weight_pre(const void* x, const void* dy, float* dw, void* workspace, size_t workspace_bytes, int N, int C,
                               int H, int W, int OH, int OW, int K, int stride, int pad_top, int pad_left, int dtype,
                               const float* scale_shift, int act, moma_stream_t stream) {
    if (!x || !dy || !dw || !workspace || !scale_shift) return MOMA_E_NULL;
    const int rc = dw_check(N, C, H, W, OH, OW, K, stride, pad_top, pad_left, dtype);
    if (rc != MOMA_OK) return rc;
    if (bad_act(act)) return MOMA_E_DTYPE;
    if (workspace_bytes < moma_dwconv_workspace_bytes(C, K)) return MOMA_E_WORKSPACE;
    return hip_rc(launch_dw_bwd_weight(x, dy, dw, (float*)workspace, workspace_bytes / sizeof(float), N, C, H, W, OH, OW, K,
                                       stride, pad_top, pad_left, dtype, scale_shift, act, (hipStream_t)stream));
}

static bool pw_bad_shape(int N, int Cin, int Cout, int HW) {
    return N <= 0 || Cin <= 0 || Cout <= 0 || HW <= 0 || Cin > 65536 || Cout > 65536 || (long)N * HW > 0x7fffffffL;
}

size_t moma_pwconv_workspace_bytes(int N, int Cin, int Cout, int HW) {
    return pw_bad_shape(N, Cin, Cout, HW) ? 0 : align_up(pwconv_workspace_floats(N, Cin, Cout, HW) * sizeof(float), 256);
}

int moma_pwconv_bwd_weight(const void* x, const void* dy, void* dw, void* workspace, size_t workspace_bytes, int N, int Cin,
                           int Cout, int HW, int dtype, moma_stream_t stream) {
    if (!x || !dy || !dw || !workspace) return MOMA_E_NULL;
    if (pw_bad_shape(N, Cin, Cout, HW)) return MOMA_E_SHAPE;
    if (dtype != MOMA_DT_BF16) return MOMA_E_DTYPE;          // (MOMA_DT_F32 included: the caller keeps its stock path for fp32)
    if (misaligned(x, 2) || misaligned(dy, 2) || misaligned(dw, 2) || misaligned(workspace, 16)) return MOMA_E_ALIGN;
    if (workspace_bytes < moma_pwconv_workspace_bytes(N, Cin, Cout, HW)) return MOMA_E_WORKSPACE;
    return hip_rc(launch_pw_bwd_weight(x, dy, dw, (float*)workspace, N, Cin, Cout, HW, (hipStream_t)stream));
}

static int pw_stream_call(const void* x, const void* w, void* y, int N, int Cin, int Cout, int HW, int dtype, int transposed,
                          moma_stream_t stream) {
    if (!x || !w || !y) return MOMA_E_NULL;
    if (pw_bad_shape(N, Cin, Cout, HW)) return MOMA_E_SHAPE;
    if (dtype != MOMA_DT_BF16) return MOMA_E_DTYPE;          // (MOMA_DT_F32 included: the caller keeps its stock path for fp32)
    if (misaligned(x, 2) || misaligned(w, 2) || misaligned(y, 2)) return MOMA_E_ALIGN;
    return hip_rc(launch_pw_stream(x, w, y, N, Cin, Cout, HW, transposed, (hipStream_t)stream));
}

int moma_pwconv_fwd(const void* x, const void* w, void* y, int N, int Cin, int Cout, int HW, int dtype, moma_stream_t stream) {
    return pw_stream_call(x, w, y, N, Cin, Cout, HW, dtype, 0, stream);
}

int moma_pwconv_bwd_data(const void* dy, const void* w, void* dx, int N, int Cin, int Cout, int HW, int dtype,
                         moma_stream_t stream) {
    return pw_stream_call(dy, w, dx, N, Cin, Cout, HW, dtype, 1, stream);
}

static int se_check(int NC, int HW, int dtype) {
    if (NC <= 0 || HW <= 0) return MOMA_E_SHAPE;
    if (dtype != MOMA_DT_F32 && dtype != MOMA_DT_BF16) return MOMA_E_DTYPE;
    return MOMA_OK;
}
int moma_plane_mean(const void* x, void* mean, int NC, int HW, int dtype, moma_stream_t stream) {
    if (!x || !mean) return MOMA_E_NULL;
    const int rc = se_check(NC, HW, dtype);
    return rc != MOMA_OK ? rc : hip_rc(launch_plane_mean(x, mean, NC, HW, dtype, (hipStream_t)stream));
}
int moma_se_gate_fwd(const void* x, const void* s, void* out, int NC, int HW, int dtype, moma_stream_t stream) {
    if (!x || !s || !out) return MOMA_E_NULL;
    const int rc = se_check(NC, HW, dtype);
    return rc != MOMA_OK ? rc : hip_rc(launch_se_gate_fwd(x, s, out, NC, HW, dtype, (hipStream_t)stream));
}
int moma_se_gate_bwd(const void* x, const void* s, const void* dout, void* dx, void* ds, int NC, int HW, int dtype,
                     moma_stream_t stream) {
    if (!x || !s || !dout || !dx || !ds) return MOMA_E_NULL;
    const int rc = se_check(NC, HW, dtype);
    return rc != MOMA_OK ? rc : hip_rc(launch_se_gate_bwd(x, s, dout, dx, ds, NC, HW, dtype, (hipStream_t)stream));
}

// ---- CRD ------------------------------------------------------------------------------------------------------------------
static int crd_check(int B, int d, int K1, int64_t n_data, float T) {
    if (B <= 0 || d < 4 || d % 4 != 0 || K1 < 2 || n_data <= 0 || !(T > 0.f)) return MOMA_E_SHAPE;
    if (d > 2048 || B > 65535) return MOMA_E_UNSUPPORTED;
    return MOMA_OK;
}
static bool crd_misaligned(const void* a, const void* b, const void* c, const void* d, const void* e = nullptr,
                           const void* f = nullptr, const void* g = nullptr, const void* h = nullptr) {
    return misaligned(a, 16) || misaligned(b, 16) || misaligned(c, 16) || misaligned(d, 16) || misaligned(e, 16) ||
           misaligned(f, 16) || misaligned(g, 16) || misaligned(h, 16);
}

size_t moma_crd_workspace_bytes(int B, int d, int K1) {
    if (crd_check(B, d, K1, 1, 1.f) != MOMA_OK) return 0;
    return crd_workspace_bytes(B, d, K1);
}

int moma_crd_fused(const float* v1, const float* v2, const float* memory_v1, const float* memory_v2, const int64_t* idx,
                   int B, int d, int K1, int64_t n_data, float T, float* Z, int set_z, float* loss, float* dv1, float* dv2,
                   int32_t* bad_index, void* workspace, size_t workspace_bytes, moma_stream_t stream) {
    if (!v1 || !v2 || !memory_v1 || !memory_v2 || !idx || !Z || !loss || !bad_index || !workspace) return MOMA_E_NULL;
    if ((dv1 == nullptr) != (dv2 == nullptr)) return MOMA_E_NULL;
    const int rc = crd_check(B, d, K1, n_data, T);
    if (rc != MOMA_OK) return rc;
    if (crd_misaligned(v1, v2, memory_v1, memory_v2, dv1, dv2, workspace) || misaligned(idx, 8) || misaligned(Z, 4) ||
        misaligned(loss, 4) || misaligned(bad_index, 4))
        return MOMA_E_ALIGN;
    if (workspace_bytes < crd_workspace_bytes(B, d, K1)) return MOMA_E_WORKSPACE;
    return hip_rc(launch_crd_fused(v1, v2, memory_v1, memory_v2, idx, B, d, K1, n_data, T, Z, set_z, loss, dv1, dv2, bad_index,
                                   workspace, (hipStream_t)stream));
}

int moma_crd_scores(const float* v1, const float* v2, const float* memory_v1, const float* memory_v2, const int64_t* idx,
                    int B, int d, int K1, int64_t n_data, float T, float* Z, int set_z, float* out_v1, float* out_v2,
                    int32_t* bad_index, void* workspace, size_t workspace_bytes, moma_stream_t stream) {
    if (!v1 || !v2 || !memory_v1 || !memory_v2 || !idx || !Z || !out_v1 || !out_v2 || !bad_index || !workspace) return MOMA_E_NULL;
    const int rc = crd_check(B, d, K1, n_data, T);
    if (rc != MOMA_OK) return rc;
    if (crd_misaligned(v1, v2, memory_v1, memory_v2, workspace) || misaligned(idx, 8) || misaligned(Z, 4) ||
        misaligned(out_v1, 4) || misaligned(out_v2, 4) || misaligned(bad_index, 4))
        return MOMA_E_ALIGN;
    if (workspace_bytes < crd_workspace_bytes(B, d, K1)) return MOMA_E_WORKSPACE;
    return hip_rc(launch_crd_scores(v1, v2, memory_v1, memory_v2, idx, B, d, K1, n_data, T, Z, set_z, out_v1, out_v2, bad_index,
                                    workspace, (hipStream_t)stream));
}

int moma_crd_scores_bwd(const float* dout_v1, const float* dout_v2, const float* out_v1, const float* out_v2,
                        const float* memory_v1, const float* memory_v2, const int64_t* idx, int B, int d, int K1,
                        int64_t n_data, float T, float* dv1, float* dv2, int32_t* bad_index, void* workspace,
                        size_t workspace_bytes, moma_stream_t stream) {
    if (!dout_v1 || !dout_v2 || !out_v1 || !out_v2 || !memory_v1 || !memory_v2 || !idx || !dv1 || !dv2 || !bad_index || !workspace)
        return MOMA_E_NULL;
    const int rc = crd_check(B, d, K1, n_data, T);
    if (rc != MOMA_OK) return rc;
    if (crd_misaligned(memory_v1, memory_v2, dv1, dv2, workspace) || misaligned(idx, 8) || misaligned(dout_v1, 4) ||
        misaligned(dout_v2, 4) || misaligned(out_v1, 4) || misaligned(out_v2, 4) || misaligned(bad_index, 4))
        return MOMA_E_ALIGN;
    if (workspace_bytes < crd_workspace_bytes(B, d, K1)) return MOMA_E_WORKSPACE;
    return hip_rc(launch_crd_scores_bwd(dout_v1, dout_v2, out_v1, out_v2, memory_v1, memory_v2, idx, B, d, K1, n_data, T, dv1, dv2,
                                        bad_index, workspace, (hipStream_t)stream));
}

int moma_crd_update(float* memory_v1, float* memory_v2, const float* v1, const float* v2, const int64_t* y, int B, int d,
                    int64_t n_data, float momentum, int32_t* bad_index, moma_stream_t stream) {
    if (!memory_v1 || !memory_v2 || !v1 || !v2 || !y || !bad_index) return MOMA_E_NULL;
    if (B <= 0 || d <= 0 || n_data <= 0) return MOMA_E_SHAPE;
    if (d > 2048 || B > 65535) return MOMA_E_UNSUPPORTED;
    if (misaligned(memory_v1, 4) || misaligned(memory_v2, 4) || misaligned(v1, 4) || misaligned(v2, 4) || misaligned(y, 8) ||
        misaligned(bad_index, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_crd_update(memory_v1, memory_v2, v1, v2, y, B, d, n_data, momentum, bad_index, (hipStream_t)stream));
}

// ---- Attention Transfer ----------------------------------------------------------------------------------------------------
static int at_check(int B, int C, int H, int W, int oh, int ow, int dtype, int layout) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0) return MOMA_E_SHAPE;
    if (bad_dt(dtype)) return MOMA_E_DTYPE;
    if (layout != MOMA_LAYOUT_NCHW && layout != MOMA_LAYOUT_NHWC) return MOMA_E_UNSUPPORTED;
    if (H % oh != 0 || W % ow != 0) return MOMA_E_SHAPE;
    if ((int64_t)oh * ow > INT32_MAX / 8) return MOMA_E_UNSUPPORTED;          // (pixel indices of one image are ints)
    return MOMA_OK;
}

size_t moma_at_workspace_bytes(int B, int C, int H, int W, int oh, int ow, int dtype, int layout) {
    if (at_check(B, C, H, W, oh, ow, dtype, layout) != MOMA_OK) return 0;
    return at_workspace_bytes(B, C, H, W, oh, ow, layout);
}

int moma_at_map(const void* f, float* a, int B, int C, int H, int W, int oh, int ow, int dtype, int layout, void* workspace,
                size_t workspace_bytes, moma_stream_t stream) {
    if (!f || !a) return MOMA_E_NULL;
    const int rc = at_check(B, C, H, W, oh, ow, dtype, layout);
    if (rc != MOMA_OK) return rc;
    const size_t need = at_workspace_bytes(B, C, H, W, oh, ow, layout);
    if (need != 0 && !workspace) return MOMA_E_NULL;
    if (workspace_bytes < need) return MOMA_E_WORKSPACE;
    if (misaligned(f, dtype == MOMA_DT_BF16 ? 2 : 4) || misaligned(a, 4) || (need != 0 && misaligned(workspace, 16))) return MOMA_E_ALIGN;
    return hip_rc(launch_at_map(f, a, B, C, H, W, oh, ow, dtype, layout, workspace, (hipStream_t)stream));
}

int moma_at_pair(const float* a_s, const float* a_t, int B, int n, float* norms, float* partials, float* loss, float* g_s,
                 float* g_t, float* ah_s, float* ah_t, moma_stream_t stream) {
    if (!a_s || !a_t || !norms || !partials || !loss) return MOMA_E_NULL;
    if (B <= 0 || n <= 0) return MOMA_E_SHAPE;
    if (misaligned(a_s, 4) || misaligned(a_t, 4) || misaligned(norms, 4) || misaligned(partials, 4) || misaligned(loss, 4) ||
        misaligned(g_s, 4) || misaligned(g_t, 4) || misaligned(ah_s, 4) || misaligned(ah_t, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_at_pair(a_s, a_t, B, n, norms, partials, loss, g_s, g_t, ah_s, ah_t, (hipStream_t)stream));
}

int moma_at_bwd(const void* f, const float* g_a, const float* g_loss, void* dF, int B, int C, int H, int W, int oh, int ow,
                int dtype, int layout, moma_stream_t stream) {
    if (!f || !g_a || !g_loss || !dF) return MOMA_E_NULL;
    const int rc = at_check(B, C, H, W, oh, ow, dtype, layout);
    if (rc != MOMA_OK) return rc;
    const size_t eb = dtype == MOMA_DT_BF16 ? 2 : 4;
    if (misaligned(f, eb) || misaligned(dF, eb) || misaligned(g_a, 4) || misaligned(g_loss, 4)) return MOMA_E_ALIGN;
    return hip_rc(launch_at_bwd(f, g_a, g_loss, dF, B, C, H, W, oh, ow, dtype, layout, (hipStream_t)stream));
}

// ---- Neuron Selectivity Transfer -----------------------------------------------------------------------------------------------
static int nst_check(int B, int Cs, int Ct, int P, int dtype_s, int layout_s, int dtype_t, int layout_t) {
    if (B <= 0 || Cs <= 0 || Ct <= 0 || P <= 0) return MOMA_E_SHAPE;
    if (bad_dt(dtype_s) || bad_dt(dtype_t)) return MOMA_E_DTYPE;
    if ((layout_s != MOMA_LAYOUT_NCHW && layout_s != MOMA_LAYOUT_NHWC) || (layout_t != MOMA_LAYOUT_NCHW && layout_t != MOMA_LAYOUT_NHWC))
        return MOMA_E_UNSUPPORTED;
    if (Cs > MOMA_NST_MAX_C || Ct > MOMA_NST_MAX_C) return MOMA_E_UNSUPPORTED;
    if (P > INT32_MAX / 2) return MOMA_E_UNSUPPORTED;                          // (pixel indices of one image are ints)
    if ((long long)B * nst_row_blocks(Cs) > INT32_MAX || (long long)B * nst_pixel_tiles(P) > INT32_MAX) return MOMA_E_UNSUPPORTED;
    return MOMA_OK;
}

size_t moma_nst_workspace_bytes(int B, int Cs, int Ct) {
    if (B <= 0 || Cs <= 0 || Ct <= 0 || Cs > MOMA_NST_MAX_C || Ct > MOMA_NST_MAX_C) return 0;
    return nst_workspace_bytes(B, Cs, Ct);
}

int moma_nst_gram(const void* f_s, const void* f_t, int B, int Cs, int Ct, int P, int dtype_s, int layout_s, int dtype_t,
                  int layout_t, void* workspace, size_t workspace_bytes, float* norms, float* rows, float* partials, float* terms,
                  float* loss, moma_stream_t stream) {
    if (!f_s || !f_t || !workspace || !norms || !rows || !partials || !terms || !loss) return MOMA_E_NULL;
    const int rc = nst_check(B, Cs, Ct, P, dtype_s, layout_s, dtype_t, layout_t);
    if (rc != MOMA_OK) return rc;
    if (workspace_bytes < nst_workspace_bytes(B, Cs, Ct)) return MOMA_E_WORKSPACE;
    if (misaligned(f_s, dtype_s == MOMA_DT_BF16 ? 2 : 4) || misaligned(f_t, dtype_t == MOMA_DT_BF16 ? 2 : 4) || misaligned(workspace, 4) ||
        misaligned(norms, 4) || misaligned(rows, 4) || misaligned(partials, 4) || misaligned(terms, 4) || misaligned(loss, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_nst_gram(f_s, f_t, B, Cs, Ct, P, dtype_s, layout_s, dtype_t, layout_t, (float*)workspace, norms, rows, partials,
                                  terms, loss, (hipStream_t)stream));
}

int moma_nst_bwd(const void* f_s, const void* f_t, const void* workspace, size_t workspace_bytes, const float* norms,
                 const float* rows, const float* g_loss, void* dF_s, int B, int Cs, int Ct, int P, int dtype_s, int layout_s,
                 int dtype_t, int layout_t, moma_stream_t stream) {
    if (!f_s || !f_t || !workspace || !norms || !rows || !g_loss || !dF_s) return MOMA_E_NULL;
    const int rc = nst_check(B, Cs, Ct, P, dtype_s, layout_s, dtype_t, layout_t);
    if (rc != MOMA_OK) return rc;
    if (workspace_bytes < nst_workspace_bytes(B, Cs, Ct)) return MOMA_E_WORKSPACE;
    const size_t eb = dtype_s == MOMA_DT_BF16 ? 2 : 4;
    if (misaligned(f_s, eb) || misaligned(dF_s, eb) || misaligned(f_t, dtype_t == MOMA_DT_BF16 ? 2 : 4) || misaligned(workspace, 4) ||
        misaligned(norms, 4) || misaligned(rows, 4) || misaligned(g_loss, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_nst_bwd(f_s, f_t, (const float*)workspace, norms, rows, g_loss, dF_s, B, Cs, Ct, P, dtype_s, layout_s, dtype_t,
                                 layout_t, (hipStream_t)stream));
}

// ---- Variational Information Distillation ---------------------------------------------------------------------------------------
static int vid_check(int B, int C, int P, int dtype_m, int layout_m, int dtype_t, int layout_t) {
    if (B <= 0 || C <= 0 || P <= 0) return MOMA_E_SHAPE;
    if (bad_dt(dtype_m) || bad_dt(dtype_t)) return MOMA_E_UNSUPPORTED;
    if ((layout_m != MOMA_LAYOUT_NCHW && layout_m != MOMA_LAYOUT_NHWC) || (layout_t != MOMA_LAYOUT_NCHW && layout_t != MOMA_LAYOUT_NHWC))
        return MOMA_E_UNSUPPORTED;
    if (P > INT32_MAX / 2 || C > INT32_MAX / 2) return MOMA_E_UNSUPPORTED;      // (pixel and channel indices of one image are ints)
    return MOMA_OK;
}

size_t moma_vid_workspace_bytes(int B, int C, int P, int dtype_m, int layout_m, int dtype_t, int layout_t) {
    if (vid_check(B, C, P, dtype_m, layout_m, dtype_t, layout_t) != MOMA_OK) return 0;
    return vid_workspace_bytes(B, C, P);
}

int moma_vid_nll(const void* mean, const void* target, const float* log_scale, float eps, int B, int C, int P, int dtype_m,
                 int layout_m, int dtype_t, int layout_t, void* workspace, size_t workspace_bytes, float* sq, float* var,
                 float* g_log_scale, float* loss, moma_stream_t stream) {
    if (!mean || !target || !log_scale || !workspace || !sq || !var || !g_log_scale || !loss) return MOMA_E_NULL;
    const int rc = vid_check(B, C, P, dtype_m, layout_m, dtype_t, layout_t);
    if (rc != MOMA_OK) return rc;
    if (workspace_bytes < vid_workspace_bytes(B, C, P)) return MOMA_E_WORKSPACE;
    if (misaligned(mean, dtype_m == MOMA_DT_BF16 ? 2 : 4) || misaligned(target, dtype_t == MOMA_DT_BF16 ? 2 : 4) ||
        misaligned(workspace, 8) || misaligned(log_scale, 4) || misaligned(sq, 4) || misaligned(var, 4) || misaligned(g_log_scale, 4) ||
        misaligned(loss, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_vid_nll(mean, target, log_scale, eps, B, C, P, dtype_m, layout_m, dtype_t, layout_t, (double*)workspace, sq,
                                 var, g_log_scale, loss, (hipStream_t)stream));
}

int moma_vid_bwd(const void* mean, const void* target, const float* var, const float* g_loss, void* d_mean, int B, int C, int P,
                 int dtype_m, int layout_m, int dtype_t, int layout_t, moma_stream_t stream) {
    if (!mean || !target || !var || !g_loss || !d_mean) return MOMA_E_NULL;
    const int rc = vid_check(B, C, P, dtype_m, layout_m, dtype_t, layout_t);
    if (rc != MOMA_OK) return rc;
    const size_t eb = dtype_m == MOMA_DT_BF16 ? 2 : 4;
    if (misaligned(mean, eb) || misaligned(d_mean, eb) || misaligned(target, dtype_t == MOMA_DT_BF16 ? 2 : 4) || misaligned(var, 4) ||
        misaligned(g_loss, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_vid_bwd(mean, target, var, g_loss, d_mean, B, C, P, dtype_m, layout_m, dtype_t, layout_t, (hipStream_t)stream));
}

// ---- FitNets hint -----------------------------------------------------------------------------------------------------------------
static int hint_check(int B, int C, int P, int dtype_x, int layout_x, int dtype_t, int layout_t) {
    if (B <= 0 || C <= 0 || P <= 0) return MOMA_E_SHAPE;
    if ((long long)B * P < 2) return MOMA_E_SHAPE;                   // one value per channel has no variance
    if (bad_dt(dtype_x) || bad_dt(dtype_t)) return MOMA_E_UNSUPPORTED;
    if ((layout_x != MOMA_LAYOUT_NCHW && layout_x != MOMA_LAYOUT_NHWC) || (layout_t != MOMA_LAYOUT_NCHW && layout_t != MOMA_LAYOUT_NHWC))
        return MOMA_E_UNSUPPORTED;
    return MOMA_OK;
}

size_t moma_hint_workspace_bytes(int B, int C, int P, int dtype_x, int layout_x, int dtype_t, int layout_t) {
    if (hint_check(B, C, P, dtype_x, layout_x, dtype_t, layout_t) != MOMA_OK) return 0;
    return hint_workspace_bytes(B, C, P);
}

int moma_hint_fwd(const void* x, const void* t, const float* gamma, const float* beta, const float* conv_bias, float* running_mean,
                  float* running_var, float momentum, float eps, int B, int C, int P, int dtype_x, int layout_x, int dtype_t,
                  int layout_t, void* workspace, size_t workspace_bytes, double* mean, double* invstd, double* sums, float* loss,
                  moma_stream_t stream) {
    if (!x || !t || !gamma || !beta || !workspace || !mean || !invstd || !sums || !loss) return MOMA_E_NULL;
    const int rc = hint_check(B, C, P, dtype_x, layout_x, dtype_t, layout_t);
    if (rc != MOMA_OK) return rc;
    if (workspace_bytes < hint_workspace_bytes(B, C, P)) return MOMA_E_WORKSPACE;
    if (misaligned(x, dtype_x == MOMA_DT_BF16 ? 2 : 4) || misaligned(t, dtype_t == MOMA_DT_BF16 ? 2 : 4) || misaligned(workspace, 8) ||
        misaligned(sums, 8) || misaligned(gamma, 4) || misaligned(beta, 4) || misaligned(conv_bias, 4) || misaligned(running_mean, 4) ||
        misaligned(running_var, 4) || misaligned(mean, 8) || misaligned(invstd, 8) || misaligned(loss, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_hint_fwd(x, t, gamma, beta, conv_bias, running_mean, running_var, momentum, eps, B, C, P, dtype_x, layout_x,
                                  dtype_t, layout_t, (double*)workspace, mean, invstd, sums, loss, (hipStream_t)stream));
}

int moma_hint_bwd(const void* x, const void* t, const float* gamma, const float* beta, const double* mean, const double* invstd,
                  const double* sums, const float* g_loss, void* dx, float* d_gamma, float* d_beta, int B, int C, int P, int dtype_x,
                  int layout_x, int dtype_t, int layout_t, moma_stream_t stream) {
    if (!x || !t || !gamma || !beta || !mean || !invstd || !sums || !g_loss) return MOMA_E_NULL;
    if (!dx && !d_gamma && !d_beta) return MOMA_E_NULL;
    const int rc = hint_check(B, C, P, dtype_x, layout_x, dtype_t, layout_t);
    if (rc != MOMA_OK) return rc;
    const size_t eb = dtype_x == MOMA_DT_BF16 ? 2 : 4;
    if (misaligned(x, eb) || misaligned(dx, eb) || misaligned(t, dtype_t == MOMA_DT_BF16 ? 2 : 4) || misaligned(sums, 8) ||
        misaligned(gamma, 4) || misaligned(beta, 4) || misaligned(mean, 8) || misaligned(invstd, 8) || misaligned(g_loss, 4) ||
        misaligned(d_gamma, 4) || misaligned(d_beta, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_hint_bwd(x, t, gamma, beta, mean, invstd, sums, g_loss, dx, d_gamma, d_beta, B, C, P, dtype_x, layout_x,
                                  dtype_t, layout_t, (hipStream_t)stream));
}

// ---- SRRL --------------------------------------------------------------------------------------------------------------------------
static int srrl_check(int B, int C, int K) {
    if (B <= 0 || C <= 0 || K <= 0) return MOMA_E_SHAPE;
    if (B < 2) return MOMA_E_SHAPE;                                  // one value per channel has no variance
    if (B > MOMA_SRRL_MAX_B || C > MOMA_SRRL_MAX_C || K > MOMA_SRRL_MAX_K) return MOMA_E_UNSUPPORTED;
    return MOMA_OK;
}

size_t moma_srrl_workspace_bytes(int B, int C, int K) {
    if (srrl_check(B, C, K) != MOMA_OK) return 0;
    return srrl_workspace_bytes(B, C, K);
}

int moma_srrl_fwd(const void* x, const void* t, const float* W, const float* bias, const float* logits, const float* gamma,
                  const float* beta, float* running_mean, float* running_var, float momentum, float eps, int B, int C, int K,
                  int dtype_x, int dtype_t, void* workspace, size_t workspace_bytes, double* sums, float* dxu, float* loss,
                  float* y_out, float* pred_out, moma_stream_t stream) {
    if (!x || !t || !W || !logits || !gamma || !beta || !workspace || !sums || !dxu || !loss) return MOMA_E_NULL;
    const int rc = srrl_check(B, C, K);
    if (rc != MOMA_OK) return rc;
    if (bad_dt(dtype_x) || bad_dt(dtype_t)) return MOMA_E_DTYPE;
    if (workspace_bytes < srrl_workspace_bytes(B, C, K)) return MOMA_E_WORKSPACE;
    if (misaligned(x, dtype_x == MOMA_DT_BF16 ? 2 : 4) || misaligned(t, dtype_t == MOMA_DT_BF16 ? 2 : 4) || misaligned(W, 4) ||
        misaligned(bias, 4) || misaligned(logits, 4) || misaligned(gamma, 4) || misaligned(beta, 4) || misaligned(running_mean, 4) ||
        misaligned(running_var, 4) || misaligned(workspace, 8) || misaligned(sums, 8) || misaligned(dxu, 4) || misaligned(loss, 4) ||
        misaligned(y_out, 4) || misaligned(pred_out, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_srrl_fwd(x, t, W, bias, logits, gamma, beta, running_mean, running_var, momentum, eps, B, C, K, dtype_x,
                                  dtype_t, workspace, sums, dxu, loss, y_out, pred_out, (hipStream_t)stream));
}

int moma_srrl_bwd(const float* dxu, const double* sums, const float* g_loss, void* dx, float* d_gamma, float* d_beta, int B, int C,
                  int dtype_x, moma_stream_t stream) {
    if (!dxu || !sums || !g_loss) return MOMA_E_NULL;
    if (!dx && !d_gamma && !d_beta) return MOMA_E_NULL;
    const int rc = srrl_check(B, C, 1);
    if (rc != MOMA_OK) return rc;
    if (bad_dt(dtype_x)) return MOMA_E_DTYPE;
    if (misaligned(dxu, 4) || misaligned(sums, 8) || misaligned(g_loss, 4) || misaligned(dx, dtype_x == MOMA_DT_BF16 ? 2 : 4) ||
        misaligned(d_gamma, 4) || misaligned(d_beta, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_srrl_bwd(dxu, sums, g_loss, dx, d_gamma, d_beta, B, C, dtype_x, (hipStream_t)stream));
}

// ---- Correlation Congruence --------------------------------------------------------------------------------------------------------
static int cc_check(int B, int Cs, int Ct, int D) {
    if (B <= 0 || Cs <= 0 || Ct <= 0 || D <= 0) return MOMA_E_SHAPE;
    if (B < 2) return MOMA_E_SHAPE;                                  // no pair of neighbouring rows: the reference's mean is NaN
    if (B > MOMA_CC_MAX_B || Cs > MOMA_CC_MAX_C || Ct > MOMA_CC_MAX_C || D > MOMA_CC_MAX_D) return MOMA_E_UNSUPPORTED;
    return MOMA_OK;
}

size_t moma_cc_workspace_bytes(int B, int Cs, int Ct, int D) {
    if (cc_check(B, Cs, Ct, D) != MOMA_OK) return 0;
    return cc_workspace_bytes(B, Cs, Ct, D);
}

int moma_cc_fwd(const void* x_s, const void* x_t, const float* W_s, const float* b_s, const float* W_t, const float* b_t, int B, int Cs,
                int Ct, int D, int dtype_s, int dtype_t, void* workspace, size_t workspace_bytes, float* gu, float* loss, float* d_out,
                moma_stream_t stream) {
    if (!x_s || !x_t || !W_s || !b_s || !W_t || !b_t || !workspace || !gu || !loss) return MOMA_E_NULL;
    const int rc = cc_check(B, Cs, Ct, D);
    if (rc != MOMA_OK) return rc;
    if (bad_dt(dtype_s) || bad_dt(dtype_t)) return MOMA_E_DTYPE;
    if (workspace_bytes < cc_workspace_bytes(B, Cs, Ct, D)) return MOMA_E_WORKSPACE;
    if (misaligned(x_s, dtype_s == MOMA_DT_BF16 ? 2 : 4) || misaligned(x_t, dtype_t == MOMA_DT_BF16 ? 2 : 4) || misaligned(W_s, 4) ||
        misaligned(b_s, 4) || misaligned(W_t, 4) || misaligned(b_t, 4) || misaligned(workspace, 8) || misaligned(gu, 4) ||
        misaligned(loss, 4) || misaligned(d_out, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_cc_fwd(x_s, x_t, W_s, b_s, W_t, b_t, B, Cs, Ct, D, dtype_s, dtype_t, workspace, gu, loss, d_out,
                                (hipStream_t)stream));
}

int moma_cc_bwd(const float* gu, const void* x_s, const void* x_t, const float* W_s, const float* g_loss, void* dx_s, float* dW_s,
                float* db_s, float* dW_t, float* db_t, int B, int Cs, int Ct, int D, int dtype_s, int dtype_t, moma_stream_t stream) {
    if (!gu || !g_loss) return MOMA_E_NULL;
    if (!dx_s && !dW_s && !db_s && !dW_t && !db_t) return MOMA_E_NULL;
    if ((dx_s && !W_s) || (dW_s && !x_s) || (dW_t && !x_t)) return MOMA_E_NULL;      // an input is needed only by its output
    const int rc = cc_check(B, Cs, Ct, D);
    if (rc != MOMA_OK) return rc;
    if (bad_dt(dtype_s) || bad_dt(dtype_t)) return MOMA_E_DTYPE;
    const size_t es = dtype_s == MOMA_DT_BF16 ? 2 : 4;
    if (misaligned(gu, 4) || misaligned(x_s, es) || misaligned(x_t, dtype_t == MOMA_DT_BF16 ? 2 : 4) || misaligned(W_s, 4) ||
        misaligned(g_loss, 4) || misaligned(dx_s, es) || misaligned(dW_s, 4) || misaligned(db_s, 4) || misaligned(dW_t, 4) ||
        misaligned(db_t, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_cc_bwd(gu, x_s, x_t, W_s, g_loss, dx_s, dW_s, db_s, dW_t, db_t, B, Cs, Ct, D, dtype_s, dtype_t,
                                (hipStream_t)stream));
}

// ---- The classification head (cross-entropy, top-1, confusion matrix) ---------------------------------------------------------------
static int ce_check(int B, int K, int dtype) {
    if (B < 1 || K < 1) return MOMA_E_SHAPE;
    if (bad_dt(dtype)) return MOMA_E_DTYPE;
    if (B > MOMA_CE_MAX_B || K > MOMA_CE_MAX_K) return MOMA_E_UNSUPPORTED;
    return MOMA_OK;
}

size_t moma_ce_workspace_bytes(int B, int K) {
    if (ce_check(B, K, MOMA_DT_F32) != MOMA_OK) return 0;
    return ce_workspace_bytes(B);
}

int moma_ce_fwd(const void* z, const int64_t* labels, int B, int K, int dtype, void* workspace, size_t workspace_bytes, float* loss,
                double* lse, double* inv_n, int32_t* pred, double* stats, int64_t* conf, moma_stream_t stream) {
    if (!z || !labels || !workspace || !loss || !lse || !inv_n) return MOMA_E_NULL;
    const int rc = ce_check(B, K, dtype);
    if (rc != MOMA_OK) return rc;
    if (workspace_bytes < ce_workspace_bytes(B)) return MOMA_E_WORKSPACE;
    if (misaligned(z, dtype == MOMA_DT_BF16 ? 2 : 4) || misaligned(labels, 8) || misaligned(workspace, 8) || misaligned(loss, 4) ||
        misaligned(lse, 8) || misaligned(inv_n, 8) || misaligned(pred, 4) || misaligned(stats, 8) || misaligned(conf, 8))
        return MOMA_E_ALIGN;
    return hip_rc(launch_ce_fwd(z, labels, B, K, dtype, workspace, loss, lse, inv_n, pred, stats, conf, (hipStream_t)stream));
}

int moma_ce_bwd(const void* z, const int64_t* labels, const double* lse, const double* inv_n, const float* g_loss, void* dz, int B,
                int K, int dtype, moma_stream_t stream) {
    if (!z || !labels || !lse || !inv_n || !g_loss || !dz) return MOMA_E_NULL;
    const int rc = ce_check(B, K, dtype);
    if (rc != MOMA_OK) return rc;
    const size_t eb = dtype == MOMA_DT_BF16 ? 2 : 4;
    if (misaligned(z, eb) || misaligned(dz, eb) || misaligned(labels, 8) || misaligned(lse, 8) || misaligned(inv_n, 8) ||
        misaligned(g_loss, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_ce_bwd(z, labels, lse, inv_n, g_loss, dz, B, K, dtype, (hipStream_t)stream));
}

// ---- The student's head (cross-entropy, KD divergence at temperature T, top-1) ------------------------------------------------------
static int kdhead_check(int B, int K, int dtype_s, int dtype_t, float T) {
    if (B < 1 || K < 1 || !(T > 0.f) || !(T <= 3.402823466e+38f)) return MOMA_E_SHAPE;      // (a NaN fails both comparisons)
    if (bad_dt(dtype_s) || bad_dt(dtype_t)) return MOMA_E_DTYPE;
    if (B > MOMA_KDHEAD_MAX_B || K > MOMA_KDHEAD_MAX_K) return MOMA_E_UNSUPPORTED;
    return MOMA_OK;
}

size_t moma_kdhead_workspace_bytes(int B, int K) {
    if (kdhead_check(B, K, MOMA_DT_F32, MOMA_DT_F32, 1.f) != MOMA_OK) return 0;
    return kdhead_workspace_bytes(B);
}

int moma_kdhead_fwd(const void* z_s, const void* z_t, const int64_t* labels, int B, int K, int dtype_s, int dtype_t, float T,
                    void* workspace, size_t workspace_bytes, float* out, double* saved, moma_stream_t stream) {
    if (!z_s || !z_t || !labels || !workspace || !out || !saved) return MOMA_E_NULL;
    const int rc = kdhead_check(B, K, dtype_s, dtype_t, T);
    if (rc != MOMA_OK) return rc;
    if (workspace_bytes < kdhead_workspace_bytes(B)) return MOMA_E_WORKSPACE;
    if (misaligned(z_s, dtype_s == MOMA_DT_BF16 ? 2 : 4) || misaligned(z_t, dtype_t == MOMA_DT_BF16 ? 2 : 4) || misaligned(labels, 8) ||
        misaligned(workspace, 8) || misaligned(out, 4) || misaligned(saved, 8))
        return MOMA_E_ALIGN;
    return hip_rc(launch_kdhead_fwd(z_s, z_t, labels, B, K, dtype_s, dtype_t, T, workspace, out, saved, (hipStream_t)stream));
}

int moma_kdhead_bwd(const void* z_s, const void* z_t, const int64_t* labels, const double* saved, const float* g_cls, const float* g_div,
                    void* dz, int B, int K, int dtype_s, int dtype_t, float T, moma_stream_t stream) {
    if (!z_s || !z_t || !labels || !saved || !dz || (!g_cls && !g_div)) return MOMA_E_NULL;
    const int rc = kdhead_check(B, K, dtype_s, dtype_t, T);
    if (rc != MOMA_OK) return rc;
    const size_t es = dtype_s == MOMA_DT_BF16 ? 2 : 4;
    if (misaligned(z_s, es) || misaligned(dz, es) || misaligned(z_t, dtype_t == MOMA_DT_BF16 ? 2 : 4) || misaligned(labels, 8) ||
        misaligned(saved, 8) || misaligned(g_cls, 4) || misaligned(g_div, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_kdhead_bwd(z_s, z_t, labels, saved, g_cls, g_div, dz, B, K, dtype_s, dtype_t, T, (hipStream_t)stream));
}

// ---- The losses on a B x B batch relation (rkd, sp, pkt): the guards they share ---------------------------------------------------
// f [B, D] of `dtype` with lo <= B <= hi
static int rel_check(int B, long long D, int dtype, int lo, int hi) {
    if (B <= 0 || D <= 0) return MOMA_E_SHAPE;
    if (bad_dt(dtype)) return MOMA_E_DTYPE;
    if (B < lo || B > hi) return MOMA_E_UNSUPPORTED;
    return MOMA_OK;
}

// f [B, D] -> a B x B matrix of doubles (moma_rkd_dist, moma_pkt_gram); rc: the entry point's shape check
static int rel_side_guard(const void* f, const double* out, int dtype, int rc) {
    if (!f || !out) return MOMA_E_NULL;
    if (rc != MOMA_OK) return rc;
    if (misaligned(f, dtype == MOMA_DT_BF16 ? 2 : 4) || misaligned(out, 8)) return MOMA_E_ALIGN;
    return MOMA_OK;
}

// dF_s from f_s, the B x B matrix M and the device scalar g_loss (the three *_bwd); rc: the entry point's shape check
static int rel_bwd_guard(const void* f_s, const double* M, const float* g_loss, const void* dF_s, int dtype, int rc) {
    if (!f_s || !M || !g_loss || !dF_s) return MOMA_E_NULL;
    if (rc != MOMA_OK) return rc;
    const size_t eb = dtype == MOMA_DT_BF16 ? 2 : 4;
    if (misaligned(f_s, eb) || misaligned(dF_s, eb) || misaligned(M, 8) || misaligned(g_loss, 4)) return MOMA_E_ALIGN;
    return MOMA_OK;
}

// ---- Relational Knowledge Distillation ------------------------------------------------------------------------------------------

size_t moma_rkd_workspace_bytes(int B) {
    if (B < 2 || B > MOMA_RKD_MAX_B) return 0;
    return rkd_workspace_bytes(B);
}

int moma_rkd_dist(const void* f, int B, int D, int dtype, double* S, moma_stream_t stream) {
    const int rc = rel_side_guard(f, S, dtype, rel_check(B, D, dtype, 2, MOMA_RKD_MAX_B));
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_rkd_dist(f, B, D, dtype, S, (hipStream_t)stream));
}

int moma_rkd_terms(const double* S_s, const double* S_t, int B, float w_d, float w_a, void* workspace, size_t workspace_bytes,
                   double* Q, float* terms, float* loss, moma_stream_t stream) {
    if (!S_s || !S_t || !workspace || !Q || !terms || !loss) return MOMA_E_NULL;
    const int rc = rel_check(B, 1, MOMA_DT_F32, 2, MOMA_RKD_MAX_B);
    if (rc != MOMA_OK) return rc;
    if (workspace_bytes < rkd_workspace_bytes(B)) return MOMA_E_WORKSPACE;
    if (misaligned(S_s, 8) || misaligned(S_t, 8) || misaligned(workspace, 8) || misaligned(Q, 8) || misaligned(terms, 4) ||
        misaligned(loss, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_rkd_terms(S_s, S_t, B, (double)w_d, (double)w_a, workspace, Q, terms, loss, (hipStream_t)stream));
}

int moma_rkd_bwd(const void* f_s, const double* Q, const float* g_loss, void* dF_s, int B, int D, int dtype, moma_stream_t stream) {
    const int rc = rel_bwd_guard(f_s, Q, g_loss, dF_s, dtype, rel_check(B, D, dtype, 2, MOMA_RKD_MAX_B));
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_rkd_bwd(f_s, Q, g_loss, dF_s, B, D, dtype, (hipStream_t)stream));
}

// ---- Similarity-Preserving distillation ------------------------------------------------------------------------------------------
static int sp_check(int B, long long K, int dtype) {
    const int rc = rel_check(B, K, dtype, 1, MOMA_SP_MAX_B);
    if (rc != MOMA_OK) return rc;
    if ((K + 63) / 64 > INT32_MAX) return MOMA_E_UNSUPPORTED;                    // (sp_bwd's grid)
    return MOMA_OK;
}

size_t moma_sp_workspace_bytes(int B, long long K) {
    if (sp_check(B, K, MOMA_DT_F32) != MOMA_OK) return 0;
    return sp_workspace_bytes(B, K);
}

int moma_sp_gram(const void* f, int B, long long K, int dtype, void* workspace, size_t workspace_bytes, moma_stream_t stream) {
    if (!f || !workspace) return MOMA_E_NULL;
    const int rc = sp_check(B, K, dtype);
    if (rc != MOMA_OK) return rc;
    if (workspace_bytes < sp_workspace_bytes(B, K)) return MOMA_E_WORKSPACE;
    if (misaligned(f, dtype == MOMA_DT_BF16 ? 2 : 4) || misaligned(workspace, 4)) return MOMA_E_ALIGN;
    return hip_rc(launch_sp_gram(f, B, K, dtype, (float*)workspace, (hipStream_t)stream));
}

int moma_sp_terms(const void* workspace_s, size_t workspace_s_bytes, long long Ks, const void* workspace_t, size_t workspace_t_bytes,
                  long long Kt, int B, double* G, double* H, double* rows, double* M, float* loss, moma_stream_t stream) {
    if (!workspace_s || !workspace_t || !G || !H || !rows || !M || !loss) return MOMA_E_NULL;
    int rc = sp_check(B, Ks, MOMA_DT_F32);
    if (rc == MOMA_OK) rc = sp_check(B, Kt, MOMA_DT_F32);
    if (rc != MOMA_OK) return rc;
    if (workspace_s_bytes < sp_workspace_bytes(B, Ks) || workspace_t_bytes < sp_workspace_bytes(B, Kt)) return MOMA_E_WORKSPACE;
    if (misaligned(workspace_s, 4) || misaligned(workspace_t, 4) || misaligned(G, 8) || misaligned(H, 8) || misaligned(rows, 8) ||
        misaligned(M, 8) || misaligned(loss, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_sp_terms((const float*)workspace_s, (int)sp_splits(B, Ks), (const float*)workspace_t, (int)sp_splits(B, Kt), B, G,
                                  H, rows, M, loss, (hipStream_t)stream));
}

int moma_sp_bwd(const void* f_s, const double* M, const float* g_loss, void* dF_s, int B, long long K, int dtype, moma_stream_t stream) {
    const int rc = rel_bwd_guard(f_s, M, g_loss, dF_s, dtype, sp_check(B, K, dtype));
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_sp_bwd(f_s, M, g_loss, dF_s, B, K, dtype, (hipStream_t)stream));
}

int moma_sp_gram_sum(const void* workspace, size_t workspace_bytes, long long K, int B, float* G, moma_stream_t stream) {
    if (!workspace || !G) return MOMA_E_NULL;
    const int rc = sp_check(B, K, MOMA_DT_F32);
    if (rc != MOMA_OK) return rc;
    if (workspace_bytes < sp_workspace_bytes(B, K)) return MOMA_E_WORKSPACE;
    if (misaligned(workspace, 4) || misaligned(G, 4)) return MOMA_E_ALIGN;
    return hip_rc(launch_sp_gram_sum((const float*)workspace, (int)sp_splits(B, K), B, G, (hipStream_t)stream));
}

// ---- SemCKD: the grouped weighted per-sample MSE ----------------------------------------------------------------------------------
static int semckd_check(const moma_semckd_pair_t* pairs, int n_pairs, int S, int B, bool with_dx) {
    if (!pairs) return MOMA_E_NULL;
    if (n_pairs < 1 || n_pairs > MOMA_SEMCKD_MAX_PAIRS || S < 1 || n_pairs % S != 0 || B < 1) return MOMA_E_SHAPE;
    for (int p = 0; p < n_pairs; ++p)
        if (pairs[p].n < 1) return MOMA_E_SHAPE;
    for (int p = 0; p < n_pairs; ++p)
        if (bad_dt(pairs[p].dtype_x) || bad_dt(pairs[p].dtype_t)) return MOMA_E_UNSUPPORTED;
    for (int p = 0; p < n_pairs; ++p) {
        if (!pairs[p].x || !pairs[p].t) return MOMA_E_NULL;
        const size_t ex = pairs[p].dtype_x == MOMA_DT_BF16 ? 2 : 4;
        if (misaligned(pairs[p].x, ex) || misaligned(pairs[p].t, pairs[p].dtype_t == MOMA_DT_BF16 ? 2 : 4) ||
            (with_dx && misaligned(pairs[p].dx, ex)))
            return MOMA_E_ALIGN;
    }
    return MOMA_OK;
}

size_t moma_semckd_workspace_bytes(const moma_semckd_pair_t* pairs, int n_pairs, int B) {
    if (!pairs || n_pairs < 1 || n_pairs > MOMA_SEMCKD_MAX_PAIRS || B < 1) return 0;
    for (int p = 0; p < n_pairs; ++p)
        if (pairs[p].n < 1) return 0;
    return semckd_workspace_bytes(pairs, n_pairs, B);
}

int moma_semckd_fwd(const moma_semckd_pair_t* pairs, int n_pairs, int S, int B, const float* w, void* workspace,
                    size_t workspace_bytes, float* ind, float* loss, moma_stream_t stream) {
    if (!w || !workspace || !ind || !loss) return MOMA_E_NULL;
    const int rc = semckd_check(pairs, n_pairs, S, B, false);
    if (rc != MOMA_OK) return rc;
    if (workspace_bytes < semckd_workspace_bytes(pairs, n_pairs, B)) return MOMA_E_WORKSPACE;
    if (misaligned(w, 4) || misaligned(workspace, 8) || misaligned(ind, 4) || misaligned(loss, 4)) return MOMA_E_ALIGN;
    return hip_rc(launch_semckd_fwd(pairs, n_pairs, S, B, w, (double*)workspace, ind, loss, (hipStream_t)stream));
}

int moma_semckd_bwd(const moma_semckd_pair_t* pairs, int n_pairs, int S, int B, const float* w, const float* g_loss,
                    moma_stream_t stream) {
    if (!w || !g_loss) return MOMA_E_NULL;
    const int rc = semckd_check(pairs, n_pairs, S, B, true);
    if (rc != MOMA_OK) return rc;
    if (misaligned(w, 4) || misaligned(g_loss, 4)) return MOMA_E_ALIGN;
    return hip_rc(launch_semckd_bwd(pairs, n_pairs, S, B, w, g_loss, (hipStream_t)stream));
}

// ---- Probabilistic Knowledge Transfer ---------------------------------------------------------------------------------------------
size_t moma_pkt_workspace_bytes(int B) {
    if (B < 1 || B > MOMA_PKT_MAX_B) return 0;
    return pkt_workspace_bytes(B);
}

int moma_pkt_gram(const void* f, int B, int D, int dtype, double* G, moma_stream_t stream) {
    const int rc = rel_side_guard(f, G, dtype, rel_check(B, D, dtype, 1, MOMA_PKT_MAX_B));
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_pkt_gram(f, B, D, dtype, G, (hipStream_t)stream));
}

int moma_pkt_gram_pair(const void* f_s, int Ds, int dtype_s, const void* f_t, int Dt, int dtype_t, int B, double* G_s, double* G_t,
                       moma_stream_t stream) {
    if (!f_s || !f_t || !G_s || !G_t) return MOMA_E_NULL;
    int rc = rel_check(B, Ds, dtype_s, 1, MOMA_PKT_MAX_B);
    if (rc == MOMA_OK) rc = rel_check(B, Dt, dtype_t, 1, MOMA_PKT_MAX_B);
    if (rc != MOMA_OK) return rc;
    if (misaligned(f_s, dtype_s == MOMA_DT_BF16 ? 2 : 4) || misaligned(f_t, dtype_t == MOMA_DT_BF16 ? 2 : 4) || misaligned(G_s, 8) ||
        misaligned(G_t, 8))
        return MOMA_E_ALIGN;
    return hip_rc(launch_pkt_gram_pair(f_s, Ds, dtype_s, f_t, Dt, dtype_t, B, G_s, G_t, (hipStream_t)stream));
}

int moma_pkt_terms(const double* G_s, const double* G_t, int B, void* workspace, size_t workspace_bytes, double* M, float* loss,
                   moma_stream_t stream) {
    if (!G_s || !G_t || !workspace || !M || !loss) return MOMA_E_NULL;
    const int rc = rel_check(B, 1, MOMA_DT_F32, 1, MOMA_PKT_MAX_B);
    if (rc != MOMA_OK) return rc;
    if (workspace_bytes < pkt_workspace_bytes(B)) return MOMA_E_WORKSPACE;
    if (misaligned(G_s, 8) || misaligned(G_t, 8) || misaligned(workspace, 8) || misaligned(M, 8) || misaligned(loss, 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_pkt_terms(G_s, G_t, B, workspace, M, loss, (hipStream_t)stream));
}

int moma_pkt_bwd(const void* f_s, const double* M, const float* g_loss, void* dF_s, int B, int D, int dtype, moma_stream_t stream) {
    const int rc = rel_bwd_guard(f_s, M, g_loss, dF_s, dtype, rel_check(B, D, dtype, 1, MOMA_PKT_MAX_B));
    if (rc != MOMA_OK) return rc;
    return hip_rc(launch_pkt_bwd(f_s, M, g_loss, dF_s, B, D, dtype, (hipStream_t)stream));
}

// ---- The input batch (uint8 rows of a data pack -> the normalised image tensor) -----------------------------------------------------
int moma_input_batch(const uint8_t* src, const int64_t* idx, const uint8_t* flip, const int32_t* box, const float* lut, void* out,
                     int N, int H, int W, int B, int S_h, int S_w, int resample, int dtype, int layout, moma_stream_t stream) {
    if (!src || !lut || !out) return MOMA_E_NULL;
    if (N < 0 || H < 0 || W < 0 || B < 0 || S_h < 0 || S_w < 0 || (resample != 0 && resample != 1)) return MOMA_E_SHAPE;
    if (bad_dt(dtype) || (layout != MOMA_LAYOUT_NCHW && layout != MOMA_LAYOUT_NHWC)) return MOMA_E_DTYPE;
    if (B == 0) return MOMA_OK;
    if (N < 1 || H < 1 || W < 1 || S_h < 1 || S_w < 1) return MOMA_E_SHAPE;
    if (H > MOMA_INPUT_MAX_SIDE || W > MOMA_INPUT_MAX_SIDE || S_h > MOMA_INPUT_MAX_SIDE || S_w > MOMA_INPUT_MAX_SIDE)
        return MOMA_E_UNSUPPORTED;
    if (!box) resample = 0;                                    // (the centred window at its own size: nothing to resample)
    if (!resample && (S_h > H || S_w > W)) return MOMA_E_SHAPE;
    if (resample && (S_h > MOMA_INPUT_MAX_RESAMPLE || S_w > MOMA_INPUT_MAX_RESAMPLE)) return MOMA_E_UNSUPPORTED;
    if (misaligned(idx, 8) || misaligned(box, 4) || misaligned(lut, 4) || misaligned(out, dtype == MOMA_DT_BF16 ? 2 : 4))
        return MOMA_E_ALIGN;
    return hip_rc(launch_input_batch(src, idx, flip, box, lut, out, N, H, W, B, S_h, S_w, resample, dtype, layout, (hipStream_t)stream));
}

}  // extern "C"
