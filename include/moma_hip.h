/*
 * moma_hip.h -- C ABI of libmoma_hip.so: the MI355X (gfx950) kernels behind MoMA's
 * contrastive-distillation training step.
 *
 * The reference (trinhvg/MoMA) is pure Python on PyTorch and has no native interface of its own, so
 * every entry point below replaces a *chain of ATen ops* at a reference call site; the call site is
 * cited per function (paths relative to the reference root).  A maintainer binds these with ctypes
 * (see INTEGRATION.md); moma_amd/_lib.py is that binding.
 *
 * Conventions
 *   - all pointers are DEVICE pointers owned by the caller (torch tensors' data_ptr()); nothing is
 *     retained past the call; the library allocates no device memory: workspaces are caller-provided
 *     and sized by the *_workspace_bytes() queries;
 *   - every launch function takes the hipStream_t to enqueue on (as void*), is asynchronous on it and
 *     performs no host synchronisation (safe under hipGraph capture);
 *   - return value: 0 = ok, <0 = argument check failed (MOMA_E_*), >0 = hipError_t of a failed launch;
 *     nothing throws; no environment variable is read; no mutable global state apart from once-per-process kernel-attribute
 *     setups (dynamic-LDS opt-ins) behind std::call_once and the debug knob moma_debug_set_k2_target_wg() -- they are made for the device that is current at the first call:
 *     ONE DEVICE PER PROCESS (the DDP model: one host thread per process / GPU); re-entrant within that;
 *   - matrices are row-major and dense unless a leading dimension is given;
 *   - `prec`   : arithmetic of the contractions. MOMA_PREC_F32 = f32-input MFMA (exact fp32 fma chain,
 *                the reference's arithmetic), MOMA_PREC_BF16 = bf16-input MFMA with fp32 accumulate;
 *   - `qdtype` : storage type of the K x d feature queue (MOMA_DT_F32 = reference storage,
 *                MOMA_DT_BF16 = 2-byte rows).
 */
#ifndef MOMA_HIP_H
#define MOMA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOMA_ABI_VERSION 4

enum { MOMA_PREC_F32 = 0, MOMA_PREC_BF16 = 1 };
enum { MOMA_DT_F32 = 0, MOMA_DT_BF16 = 1 };

enum {
    MOMA_OK = 0,
    MOMA_E_NULL = -1,      /* a required pointer is NULL                        */
    MOMA_E_SHAPE = -2,     /* a dimension is <= 0 or inconsistent               */
    MOMA_E_DTYPE = -3,     /* unknown prec / qdtype                             */
    MOMA_E_ALIGN = -4,     /* pointer not aligned to its element size -- or, for the operands the fast paths move in 16-byte pieces (K1 fast
                              path, one-pass K2: q, k, queue, dq), not to 16 bytes */
    MOMA_E_WORKSPACE = -5, /* workspace too small                               */
    MOMA_E_UNSUPPORTED = -6
};

typedef void* moma_stream_t; /* hipStream_t */

/* ABI version (== MOMA_ABI_VERSION of the header the library was built from). */
int moma_version(void);
/* Human-readable text for a return code of this library (static storage). */
const char* moma_error_string(int code);
/* DEBUG knob, for plan sweeps only (scripts/sweep_k2_plan.sh): cut the K2 passes over the queue into about `n` workgroups instead
 * of the product's own plan (one per compute unit, fewer for short passes).  n = 0 restores the plan; 8 <= n <= 1024 otherwise.
 * Returns the previous value, or -1 when n is refused.  Process-wide and not synchronised with calls in flight: the launch plan AND
 * moma_infonce_fused*_workspace_bytes() follow it, so set it once, before the first workspace query, and size every workspace
 * after that.  This is the one piece of caller-set state in the library and the reason it reads no environment variable. */
int moma_debug_set_k2_target_wg(int n);

/* ---------------------------------------------------------------------------------------------
 * K4  multi-tensor EMA -- replaces ContrastTrainer.momentum_update
 *     (learning/contrast_trainer.py:207-211: per-tensor p2.mul_(m).add_(p1, alpha=1-m)).
 *     One launch for the whole parameter list:  ema = fma(fl32(1-m), p, fl32(ema*fl32(m))).
 *     `table` is a device array of n_tensors records {int64 ema_ptr, int64 p_ptr, int64 numel,
 *     int64 first_block}; first_block = exclusive prefix sum of ceil(numel / MOMA_EMA_BLOCK_ELEMS);
 *     total_blocks = that sum.  The table is built once per model pair by the host.
 * ------------------------------------------------------------------------------------------- */
#define MOMA_EMA_BLOCK_ELEMS 4096
int moma_ema_multi(const int64_t* table, int n_tensors, int64_t total_blocks,
                   float m, float one_minus_m, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K3  ring-buffer enqueue -- replaces BaseMoCo._update_memory (MoMA/mem_moco.py:17-27:
 *     arange+index -> fmod(K) -> index_copy_).   queue[(index+i) mod K, :] = rows[i, :], i in [0,n).
 *     n > K (duplicate slots) is last-writer-wins like a serial index_copy_.  The pointer update
 *     index = (index+n) mod K (MoMA/mem_moco.py:14-15) stays a host integer in the caller.
 *     rows are fp32 [n,d]; queue is [K,d] in `qdtype` (bf16 rows are rounded to nearest even).
 * ------------------------------------------------------------------------------------------- */
int moma_enqueue(void* queue, const float* rows, int n, int64_t index, int K, int d,
                 int qdtype, moma_stream_t stream);
/* The same enqueue into an fp32 queue (the reference's storage) AND its bf16 mirror (what the bf16-policy one-pass K2 streams:
 * half the HBM bytes per step, no conversion pass over the K x d queue) in ONE launch from one read of the rows. */
int moma_enqueue_mirror(float* queue, void* mirror_bf16, const float* rows, int n, int64_t index, int K, int d,
                        moma_stream_t stream);

/* Cache hint for K2: streams `bytes` of the queue once (16-B loads, data dropped) so that it sits in the 256 MiB memory-side
 * Infinity Cache when moma_infonce_fused reads it next.  In the training step the K x d queue was last touched a whole step
 * (gigabytes of activations) ago; issued on a second stream under the latency-bound attention launches that precede K2, the
 * sweep costs no step time and K2 then runs at its cache-resident rate.  Purely a performance hint: no result depends on it.
 * (Round 5: the training loop no longer issues it by default -- a second read of the queue per step for 0.6 us of K2 at B = 256.) */
int moma_queue_prefetch(const void* queue, size_t bytes, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K2  InfoNCE over the queue.
 *
 * moma_infonce_logits -- replaces BaseMoCo._compute_logit (MoMA/mem_moco.py:29-49):
 *     out[b,0] = <q_b,k_b>*inv_T ; out[b,1+j] = <queue_j,q_b>*inv_T ; out is [B,K+1] fp32 contiguous.
 * moma_infonce_logits_bwd -- the autograd backward of the above w.r.t. q:
 *     dq[b,:] = (dlogits[b,0]*k_b + sum_j dlogits[b,1+j]*queue_j) * inv_T          (dq is [B,d] fp32)
 *     The contraction over K is split over workgroups.  moma_infonce_logits_bwd_ws (round 6) keeps one partial product per split
 *     in a caller-owned workspace (moma_infonce_logits_bwd_workspace_bytes()) and adds them in split order: bitwise reproducible,
 *     like every other result of this library.  moma_infonce_logits_bwd, the form without a workspace, lets the splits meet in
 *     fp32 atomics: equal up to the order of the additions (last bits differ from run to run).
 * moma_infonce_fused -- replaces the whole chain MoCo.forward (MoMA/mem_moco.py:77-100, minus the
 *     enqueue) + nn.CrossEntropyLoss(logits, 0) + top-1 accuracy (helper/loops_moma.py:322,331-335,
 *     learning/contrast_trainer.py:189-205) and its backward, in one pass over the queue:
 *       lse[b]       = logsumexp_j out[b,j]
 *       loss_rows[b] = lse[b] - out[b,0]                  (loss_kd = mean_b loss_rows[b])
 *       top1[b]      = 1 if out[b,0] >= max_j out[b,j] else 0
 *       dq[b,:]      = d(sum_b loss_rows)/dq_b = ((p_b0-1)*k_b + sum_j p_bj*queue_j)*inv_T
 *     dq may be NULL (forward only).  workspace: moma_infonce_fused_workspace_bytes() -- it depends on (qdtype, prec): under
 *     prec = fp32 with a bf16-stored queue it includes room for a widened (fp32, exact) copy of the queue, made and dropped inside
 *     the call, at the widths the one-pass fp32 kernel takes.
 * ------------------------------------------------------------------------------------------- */
int moma_infonce_logits(const float* q, const float* k, const void* queue, float* out,
                        int B, int d, int K, float inv_T, int qdtype, int prec, moma_stream_t stream);
int moma_infonce_logits_bwd(const float* dlogits, const float* k, const void* queue, float* dq,
                            int B, int d, int K, float inv_T, int qdtype, int prec,
                            moma_stream_t stream);
size_t moma_infonce_logits_bwd_workspace_bytes(int B, int d, int K);
int moma_infonce_logits_bwd_ws(const float* dlogits, const float* k, const void* queue, float* dq,
                               int B, int d, int K, float inv_T, int qdtype, int prec,
                               void* workspace, size_t workspace_bytes, moma_stream_t stream);
/* gradients of the logits w.r.t. the key / queue operands (needed by the MoCoAtt cross-attention variants,
 * MoMA/mem_moco.py:103-161, where k and the queue are attention outputs that carry gradient):
 *     dk[b,:]     = dlogits[b,0] * q_b * inv_T                          (may be NULL)
 *     dqueue[j,:] = sum_b dlogits[b,1+j] * q_b * inv_T   ([K,d] fp32)    (may be NULL) */
int moma_infonce_logits_bwd_kq(const float* dlogits, const float* q, float* dk, float* dqueue,
                               int B, int d, int K, float inv_T, int prec, moma_stream_t stream);
size_t moma_infonce_fused_workspace_bytes(int B, int d, int K, int qdtype, int prec);
int moma_infonce_fused(const float* q, const float* k, const void* queue, int B, int d, int K,
                       float inv_T, float* loss_rows, float* lse, int32_t* top1, float* dq,
                       void* workspace, size_t workspace_bytes, int qdtype, int prec,
                       moma_stream_t stream);
/* Same, with an optional measurement hook: ev_begin / ev_end are hipEvent_t handles (or NULL) recorded on
 * `stream` immediately before / after the dominant kernel of the call (the one pass over the queue), so a
 * benchmark can time exactly the kernel its roofline is quoted for.  No synchronisation is performed. */
int moma_infonce_fused_ex(const float* q, const float* k, const void* queue, int B, int d, int K,
                          float inv_T, float* loss_rows, float* lse, int32_t* top1, float* dq,
                          void* workspace, size_t workspace_bytes, int qdtype, int prec,
                          moma_stream_t stream, void* ev_begin, void* ev_end);
/* Same, with the query ALSO handed over pre-packed: q_packed (nullable) holds q * inv_T * log2(e) rounded to bf16 in the
 * MFMA-operand order the one pass over the queue loads it in,
 *     unit[((row / 32) * (d / 16) + col / 16) * 64 + ((col / 8) & 1) * 32 + row % 32] = 8 bf16 = columns 8 * (col / 8) .. + 7 of row,
 * 16 bytes per unit, rows padded to a multiple of 128 with zeros: moma_infonce_qpack_bytes(B, d) bytes (0 = this width takes
 * no pre-packed query: d must be 128 / 256 / 384 / 512).  The producer of q writes it -- moma_mha_fwd_fast does when asked
 * (moma_mha_module_t.qpack) -- and the call then runs no pre-pack launch.  q itself (fp32) is still read for the exact positive
 * logit.  The results are bit-identical to moma_infonce_fused_ex on the same q.
 * ev_call_end (hipEvent_t or NULL): recorded when the LAST kernel of the call has finished (on its dispatch), so that
 * ev_begin .. ev_call_end spans the kernels of the call without the latency of event packets around it. */
size_t moma_infonce_qpack_bytes(int B, int d);
int moma_infonce_fused_q(const float* q, const void* q_packed, const float* k, const void* queue, int B, int d, int K,
                         float inv_T, float* loss_rows, float* lse, int32_t* top1, float* dq,
                         void* workspace, size_t workspace_bytes, int qdtype, int prec,
                         moma_stream_t stream, void* ev_begin, void* ev_end, void* ev_call_end);
/* K2 + K3 in one call: moma_infonce_fused_q(...) followed by the enqueue of `rows` [n,d] at ring pointer `index`
 * (MoCo.forward, MoMA/mem_moco.py:77-100: logits from the PRE-enqueue queue, then _update_memory).  Where the call ends in the
 * combine launch (the bf16 policy's one-pass and two-pass paths) the enqueue rides on THAT launch -- extra workgroups behind every
 * read of the queue -- instead of a launch of its own; elsewhere it is issued behind the call.  Same results as the two calls.
 *   queue     : what K2 reads, written in place: fp32 rows (qdtype F32) or rows rounded to bf16 (qdtype BF16);
 *   queue_f32 : NULL, or -- qdtype BF16 only -- the fp32 queue whose bf16 mirror `queue` is: both take the rows (moma_enqueue_mirror).
 * The ring pointer stays with the caller (a host integer: bit-exact contract); n = 0 is K2 alone. */
int moma_infonce_fused_enqueue(const float* q, const void* q_packed, const float* k, void* queue, int B, int d, int K,
                               float inv_T, float* loss_rows, float* lse, int32_t* top1, float* dq, void* workspace,
                               size_t workspace_bytes, int qdtype, int prec, const float* rows, int n, int64_t index,
                               float* queue_f32, moma_stream_t stream, void* ev_begin, void* ev_end, void* ev_call_end);

/* Several InfoNCE terms over queues of the same shape in ONE sweep -- replaces the 2 / 4 `_compute_logit` calls + CrossEntropy of
 * the dual-queue memories MoCoST.forward / MoCoSSTT.forward (MoMA/mem_moco.py:165-253):
 *     (q, k, memory_s), (q, k_t, memory_t) [, (q_t, k, memory_s), (q_t, k_t, memory_t)]
 * One pre-pack launch over the distinct q pointers, ONE launch of the one-pass kernel over every (term, query tile, key chunk) --
 * sized to one workgroup per compute unit over all terms, the queues streamed back to back --, one combine launch: 3 launches
 * for any number of terms (<= 4).  Per term the outputs of moma_infonce_fused; dq either for every term or for none (a query
 * shared by two terms gets two dq buffers: the caller adds them).  The one-sweep kernel takes the bf16 policy with bf16 queues and
 * d in {128, 256, 384, 512}; every other configuration moma_infonce_fused accepts (wide rows, exact fp32, fp32 queues) is served
 * by the same entry point term by term on the stream, through ONE workspace of moma_infonce_fused's size -- at those shapes a
 * term's own passes fill the chip and are not HBM-bound, so there is no sweep to share.  Queues are bf16 or fp32 per `qdtype`. */
typedef struct moma_infonce_term {
    const float* q;        /* [B,d] fp32  */
    const float* k;        /* [B,d] fp32  */
    const void* queue;     /* [K,d] bf16 / fp32 (qdtype) */
    float* loss_rows;      /* [B] out     */
    float* lse;            /* [B] out     */
    int32_t* top1;         /* [B] out     */
    float* dq;             /* [B,d] out or NULL */
} moma_infonce_term_t;
size_t moma_infonce_fused_multi_workspace_bytes(int n_terms, int B, int d, int K, int qdtype, int prec);
int moma_infonce_fused_multi(const moma_infonce_term_t* terms, int n_terms, int B, int d, int K, float inv_T,
                             void* workspace, size_t workspace_bytes, int qdtype, int prec, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * CRD  Contrastive Representation Distillation (`--distill crd`) over two n_data x d memory banks addressed by sample index
 *      -- replaces ContrastMemory.forward (crd/memory.py:23-79: index_select -> [B,K1,d] copy -> bmm -> exp -> div, per side,
 *      then the momentum update of the banks) and ContrastLoss.forward (crd/criterion.py:57-74) with their autograd backward.
 *
 *   K1 = nce_k + 1;  idx [B,K1] int64, column 0 = the sample's own index;  c = nce_k / n_data;  eps = 1e-7;
 *   side 1 = (v1 = student embedding, bank memory_v2), side 2 = (v2 = teacher embedding, bank memory_v1).  Per side:
 *       s[b,j] = <M[idx[b,j]], v[b]>      e[b,j] = exp(s[b,j] / T)      x[b,j] = e[b,j] / Z
 *       loss   = -( sum_b log(x[b,0] / (x[b,0] + c + eps)) + sum_b sum_{j>=1} log(c / (x[b,j] + c + eps)) ) / B
 *       dv[b,:] = d loss / d v[b] = sum_j g[b,j] x[b,j] / T * M[idx[b,j],:],
 *                 g[b,0] = -(1/x[b,0] - 1/(x[b,0] + c + eps)) / B,   g[b,j>=1] = 1 / (x[b,j] + c + eps) / B
 *   All operands fp32; v*, memory_*, dv*, out_*, dout_* 16-byte aligned; d a multiple of 4, 4 <= d <= 2048; B <= 65535;
 *   K1 >= 2; T > 0.  Z [2] (side 1, side 2) is a DEVICE pair: with set_z != 0 a statistics pass over the same gather writes
 *   Z = mean(e) * n_data per side first (crd/memory.py:50-57) and the main pass reads it; with set_z == 0 Z is read as it stands.
 *   Indices are data: an entry of idx (or y) outside [0, n_data) never becomes an address -- it contributes nothing (its score is
 *   written as 0) and 1 is stored into *bad_index, which the caller zeroes and reads where it synchronises anyway.
 *   workspace: moma_crd_workspace_bytes(B, d, K1) for each of the three gather calls.  Per-wave partial sums meet in a second
 *   launch in a fixed order: no atomics, bitwise reproducible.
 *
 * moma_crd_fused      both sides in one pass: loss [2] (side 1, side 2; the CRD loss is their sum) and dv1 / dv2 [B,d] (both or
 *                     neither: NULL, NULL = forward only).  Every bank row is fetched once per (b, j, side).
 * moma_crd_scores     the materialised form ContrastMemory.forward returns: out_v1 = x of side 1, out_v2 = x of side 2, [B,K1].
 * moma_crd_scores_bwd its backward: dv[b,:] = sum_j dout[b,j] * out[b,j] / T * M[idx[b,j],:] per side.
 * moma_crd_update     crd/memory.py:64-77 for both banks in one launch: for i < B, r = M[y[i]] * momentum + v[i] * (1 - momentum),
 *                     M[y[i]] = r / sqrt(sum r^2) with (memory_v1, v1) and (memory_v2, v2).  It reads the PRE-update row: issue it
 *                     behind the gather of the same step (same stream).  A y repeated inside the batch: the last one in batch
 *                     order wins, as in a serial index_copy_.
 * ------------------------------------------------------------------------------------------- */
size_t moma_crd_workspace_bytes(int B, int d, int K1);
int moma_crd_fused(const float* v1, const float* v2, const float* memory_v1, const float* memory_v2, const int64_t* idx,
                   int B, int d, int K1, int64_t n_data, float T, float* Z, int set_z, float* loss, float* dv1, float* dv2,
                   int32_t* bad_index, void* workspace, size_t workspace_bytes, moma_stream_t stream);
int moma_crd_scores(const float* v1, const float* v2, const float* memory_v1, const float* memory_v2, const int64_t* idx,
                    int B, int d, int K1, int64_t n_data, float T, float* Z, int set_z, float* out_v1, float* out_v2,
                    int32_t* bad_index, void* workspace, size_t workspace_bytes, moma_stream_t stream);
int moma_crd_scores_bwd(const float* dout_v1, const float* dout_v2, const float* out_v1, const float* out_v2,
                        const float* memory_v1, const float* memory_v2, const int64_t* idx, int B, int d, int K1,
                        int64_t n_data, float T, float* dv1, float* dv2, int32_t* bad_index, void* workspace,
                        size_t workspace_bytes, moma_stream_t stream);
int moma_crd_update(float* memory_v1, float* memory_v2, const float* v1, const float* v2, const int64_t* y, int B, int d,
                    int64_t n_data, float momentum, int32_t* bad_index, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * AT   Attention Transfer (`--distill attention`, p = 2) on one pair of feature maps -- replaces Attention.at_loss
 *      (distiller_zoo/AT.py: adaptive_avg_pool2d -> pow(2) -> mean(1) -> F.normalize -> (a_s - a_t).pow(2).mean()) and its
 *      autograd backward.  For f [B,C,H,W] and an output grid oh x ow with H % oh == 0 and W % ow == 0 (window rh x rw =
 *      H/oh x W/ow; 1 x 1 = no pooling):
 *          pool(f)[b,c,y,x] = mean of the window      a[b, y ow + x] = (1/C) sum_c pool(f)[b,c,y,x]^2
 *          ah = a / max(|a|_2, 1e-12) per batch row    loss = sum_b sum_i (ah_s - ah_t)[b,i]^2 / (B n),   n = oh ow
 *          g_ah = +-2 (ah_s - ah_t) / (B n)            g_a = (g_ah - ah <ah, g_ah>) / |a|_2   (g_ah / 1e-12 under the clamp)
 *          dF[b,c,Y,X] = g_loss * g_a[b, (Y/rh) ow + X/rw] * 2 / (C rh rw) * pool(f)[b,c,Y/rh,X/rw]
 *      f, dF: MOMA_DT_F32 or MOMA_DT_BF16 (dtype), dense in MOMA_LAYOUT_NCHW or MOMA_LAYOUT_NHWC (channels_last memory
 *      [B,H,W,C]; the shape arguments are the logical B, C, H, W either way), aligned to their element size -- 16-byte accesses
 *      are used where the address and the contiguous extent (H W, or C) allow, element accesses otherwise.  Everything else
 *      (a, norms, partials, loss, g_*, ah_*, g_loss) is fp32.  Accumulation over the channels in fp32; the pair in double.
 *      No atomics: partial sums meet in a fixed order, results are bitwise reproducible.
 *
 * moma_at_map   a [B, oh ow] from one read of f.  workspace: moma_at_workspace_bytes() bytes (0 for most shapes: NULL is
 *               accepted then), 16-byte aligned -- small NCHW maps are cut along the channels over several workgroups.
 * moma_at_pair  both maps [B, n] -> norms [B, 2] (student, teacher), partials [B] (the row's sum of squared differences),
 *               loss [1], and, each nullable, g_s / g_t [B, n] (d loss / d a_s, d loss / d a_t) and ah_s / ah_t [B, n].
 *               A row with |a| = 0 gives ah = 0 and a finite g (no 0/0).
 * moma_at_bwd   dF (dtype and layout of f) from one read of f and g_a [B, oh ow]; g_loss is a DEVICE scalar (the upstream
 *               gradient of the loss, e.g. a GradScaler factor): nothing is read back to the host.
 *      A grid that does not divide the map: MOMA_E_SHAPE (pool with other means first); unknown layout: MOMA_E_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_LAYOUT_NCHW = 0, MOMA_LAYOUT_NHWC = 1 };
size_t moma_at_workspace_bytes(int B, int C, int H, int W, int oh, int ow, int dtype, int layout);
int moma_at_map(const void* f, float* a, int B, int C, int H, int W, int oh, int ow, int dtype, int layout, void* workspace,
                size_t workspace_bytes, moma_stream_t stream);
int moma_at_pair(const float* a_s, const float* a_t, int B, int n, float* norms, float* partials, float* loss, float* g_s,
                 float* g_t, float* ah_s, float* ah_t, moma_stream_t stream);
int moma_at_bwd(const void* f, const float* g_a, const float* g_loss, void* dF, int B, int C, int H, int W, int oh, int ow,
                int dtype, int layout, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * NST  Neuron Selectivity Transfer (`--distill nst`) on one pair of feature maps on a COMMON grid -- replaces NSTLoss.nst_loss
 *      behind its pooling (distiller_zoo/NST.py: view -> F.normalize(dim=2) -> poly_kernel(f_s, f_s).mean()
 *      - 2 poly_kernel(f_s, f_t).mean(), the reference's full_loss = False branch) and its autograd backward to f_s.
 *      For f_s [B,Cs,H,W], f_t [B,Ct,H,W], P = H W, per image X = f_s[b] as [Cs,P], Y = f_t[b] as [Ct,P]:
 *          n_i = max(|X_i|_2, 1e-12)    m_j = max(|Y_j|_2, 1e-12)
 *          G[b,i,j] = X_i . X_j / (n_i n_j) for j < Cs (Gss),  X_i . Y_(j-Cs) / (n_i m_(j-Cs)) for j >= Cs (Gst)
 *          t1 = mean_(b,i,j) Gss^2    t2 = mean_(b,i,j) Gst^2    loss = t1 - 2 t2
 *          dX_i = g_loss (1/n_i) [ sum_j (a Gss_ij / n_j) X_j - sum_j (c Gst_ij / m_j) Y_j - (r_i / n_i) X_i ]
 *          a = 4 / (B Cs^2)   c = 4 / (B Cs Ct)   r_i = a sum_j Gss_ij^2 - c sum_j Gst_ij^2     (a row with |X_i| = 0: dX_i = 0)
 *      f_s, f_t, dF_s: MOMA_DT_F32 or MOMA_DT_BF16 and MOMA_LAYOUT_NCHW or MOMA_LAYOUT_NHWC, each chosen per side (dF_s as
 *      f_s), dense, aligned to their element size -- 16-byte accesses where the address and the contiguous extent (P, or C) allow,
 *      element accesses otherwise.  Everything else is fp32.  All products in fp32 on the f32-input MFMA whatever the storage; the
 *      normalisation is applied to the raw Gram in its epilogue (no normalised copy of a map exists).  Cs, Ct <= MOMA_NST_MAX_C
 *      (wider maps: MOMA_E_UNSUPPORTED).  No atomics: results are bitwise reproducible.
 *
 * workspace     G [B, Cs, Cs + Ct] fp32 = moma_nst_workspace_bytes() = B Cs (Cs + Ct) 4 bytes, 4-byte aligned; moma_nst_gram
 *               writes it, moma_nst_bwd reads it.
 * moma_nst_gram both maps, requested once per block of MOMA_NST_ROW_BLOCK student rows (ceil(Cs / 32) times) -> G, norms
 *               [B, Cs + Ct] (n then m, clamped), rows [B, Cs, 2] (sum_j Gss_ij^2, sum_j Gst_ij^2), partials
 *               [B, ceil(Cs / MOMA_NST_ROW_BLOCK), 2] (a workgroup's sums of both), terms [2] = (t1, t2), loss [1].
 * moma_nst_bwd  dF_s from one read of both maps, G, norms and rows; g_loss is a DEVICE scalar (the upstream gradient of the loss,
 *               e.g. a GradScaler factor): nothing is read back to the host.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_NST_MAX_C = 256, MOMA_NST_ROW_BLOCK = 32 };
size_t moma_nst_workspace_bytes(int B, int Cs, int Ct);
int moma_nst_gram(const void* f_s, const void* f_t, int B, int Cs, int Ct, int P, int dtype_s, int layout_s, int dtype_t,
                  int layout_t, void* workspace, size_t workspace_bytes, float* norms, float* rows, float* partials, float* terms,
                  float* loss, moma_stream_t stream);
int moma_nst_bwd(const void* f_s, const void* f_t, const void* workspace, size_t workspace_bytes, const float* norms,
                 const float* rows, const float* g_loss, void* dF_s, int B, int Cs, int Ct, int P, int dtype_s, int layout_s,
                 int dtype_t, int layout_t, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * VID  Variational Information Distillation (`--distill vid`) on one pair of maps on a COMMON grid -- replaces the Gaussian negative
 *      log-likelihood at the end of VIDLoss.forward (distiller_zoo/VID.py: softplus(log_scale) + eps -> 0.5 ((pred_mean - target)^2
 *      / pred_var + log pred_var) -> mean) and its autograd backward to pred_mean and log_scale.  For mean (the regressor's output)
 *      and target, both [B,C,H,W], P = H W, log_scale [C]:
 *          var_c  = log(1 + exp(log_scale_c)) + eps                  (evaluated in double)
 *          S_c    = sum_(b,p) (mean - target)[b,c,p]^2
 *          loss   = 0.5 / C * sum_c ( S_c / (B P var_c) + log var_c )
 *          d_mean = g_loss * (mean - target) / (var_c * B C P)
 *          d_var_c       = 0.5 / C * ( 1 / var_c - S_c / (B P var_c^2) )
 *          d_log_scale_c = d_var_c * exp(log_scale_c) / (1 + exp(log_scale_c))      (before g_loss: the caller multiplies)
 *      mean, target, d_mean: MOMA_DT_F32 or MOMA_DT_BF16 and MOMA_LAYOUT_NCHW or MOMA_LAYOUT_NHWC, each chosen per side (d_mean as
 *      mean), dense, aligned to their element size -- 16-byte accesses where the address and the contiguous extent (P, or C) allow,
 *      element accesses otherwise; a target in the other layout than mean is read element by element.  Everything else is fp32.
 *      Differences and squares in fp32; a thread's fp32 sum is at most 16 squares long, everything across lanes, waves, workgroups
 *      and partials is added in double, as is all [C] arithmetic.  No atomics: partial sums meet in a fixed order in a second
 *      launch, results are bitwise reproducible.  The target gets no gradient.
 *      DEVIATION: the softplus is evaluated in double in its overflow-free form, so var, loss and d_log_scale stay finite for any
 *      finite log_scale; the reference's fp32 exp(log_scale) is inf for log_scale above about 88.
 *
 * workspace     moma_vid_workspace_bytes() = B ceil(P / MOMA_VID_CHUNK) C 8 bytes, 8-byte aligned: one double per image, chunk of
 *               MOMA_VID_CHUNK pixels and channel, written by the streaming kernel and added in order by the finalize kernel.
 * moma_vid_nll  one read of mean and of target -> sq [C] (S_c), var [C], g_log_scale [C], loss [1].  Two launches.
 * moma_vid_bwd  d_mean from one read of mean, target and var [C]; g_loss is a DEVICE scalar (the upstream gradient of the loss,
 *               e.g. a GradScaler factor): nothing is read back to the host.
 *      Unknown dtype or layout: MOMA_E_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_VID_CHUNK = 1024 };
size_t moma_vid_workspace_bytes(int B, int C, int P, int dtype_m, int layout_m, int dtype_t, int layout_t);
int moma_vid_nll(const void* mean, const void* target, const float* log_scale, float eps, int B, int C, int P, int dtype_m,
                 int layout_m, int dtype_t, int layout_t, void* workspace, size_t workspace_bytes, float* sq, float* var,
                 float* g_log_scale, float* loss, moma_stream_t stream);
int moma_vid_bwd(const void* mean, const void* target, const float* var, const float* g_loss, void* d_mean, int B, int C, int P,
                 int dtype_m, int layout_m, int dtype_t, int layout_t, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * HINT FitNets hint (`--distill hint`) on one pair of maps on a COMMON grid -- replaces what follows the convolution in
 *      ConvReg.forward (models/util.py: BatchNorm2d in training mode -> ReLU) together with HintLoss (distiller_zoo/FitNet.py:
 *      MSELoss) and their autograd backward.  For x (the convolution's output) and t (the teacher's map), both [B,C,H,W], P = H W,
 *      M = B P, N = B C P, gamma and beta [C]:
 *          mean_c = sum x / M       var_c = sum x^2 / M - mean_c^2   (biased; sums and variance in double)
 *          invstd_c = 1 / sqrt(var_c + eps)       xh = (x - mean_c) invstd_c   (centred and scaled in double, rounded to fp32)
 *          y = max(0, gamma_c xh + beta_c)        loss = sum (y - t)^2 / N
 *          g = (y - t) [y > 0]                    (strictly greater: ReLU's derivative at 0 is 0, as in torch)
 *          A_c = sum_(b,p) g        B_c = sum_(b,p) g xh        k = 2 g_loss / N
 *          d_beta_c = k A_c         d_gamma_c = k B_c           dx = k gamma_c invstd_c (g - A_c / M - xh B_c / M)
 *          running_mean_c <- (1 - momentum) running_mean_c + momentum (mean_c + conv_bias_c)
 *          running_var_c  <- (1 - momentum) running_var_c  + momentum var_c M / (M - 1)
 *      x, t, dx: MOMA_DT_F32 or MOMA_DT_BF16, MOMA_LAYOUT_NCHW or MOMA_LAYOUT_NHWC, each chosen per side, dense, aligned to their
 *      element size (16-byte accesses where the base address and the contiguous extent allow); dx has x's dtype and layout.
 *      gamma, beta, conv_bias, the running statistics, d_gamma, d_beta, loss and g_loss are fp32; mean, invstd, sums (A [C] then
 *      B [C]) and the workspace are double, 8-byte aligned.  The arithmetic on an element is fp32 behind the double centring,
 *      every sum double; a bf16 dx is rounded from the fp32 value.  No atomics: bitwise reproducible.  t gets no gradient.
 *      conv_bias (nullable) is the bias of the convolution in front, which the caller has NOT added to x: in training mode a
 *      per-channel constant in front of a BatchNorm changes running_mean and nothing else, so it enters there only, and its
 *      gradient is exactly 0 (the reference's autograd returns rounding noise there).
 *
 * workspace      moma_hint_workspace_bytes() = 3 ceil(B / BI) ceil(P / MOMA_HINT_CHUNK) C 8 bytes, BI = max(1, min(B,
 *                MOMA_HINT_CHUNK / P)): one double per sum, group of BI images (planes shorter than a chunk share one), chunk of
 *                MOMA_HINT_CHUNK pixels and channel, written by the streaming kernels and added in order by the finalize kernels.
 * moma_hint_fwd  two reads of x, one of t -> mean [C], invstd [C], sums [2 C] (A, B), loss [1]; running_mean / running_var
 *                (each nullable) updated in place.  Four launches.
 * moma_hint_bwd  dx (nullable) from one read of x and t and the saved [C] vectors, with no reduction of its own; d_gamma, d_beta
 *                (each nullable) from sums.  g_loss is a DEVICE scalar (the upstream gradient of the loss, e.g. a GradScaler
 *                factor): nothing is read back to the host.
 *      M < 2: MOMA_E_SHAPE, nothing is launched (torch refuses "more than 1 value per channel" likewise); unknown dtype or layout:
 *      MOMA_E_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_HINT_CHUNK = 1024 };
size_t moma_hint_workspace_bytes(int B, int C, int P, int dtype_x, int layout_x, int dtype_t, int layout_t);
int moma_hint_fwd(const void* x, const void* t, const float* gamma, const float* beta, const float* conv_bias, float* running_mean,
                  float* running_var, float momentum, float eps, int B, int C, int P, int dtype_x, int layout_x, int dtype_t,
                  int layout_t, void* workspace, size_t workspace_bytes, double* mean, double* invstd, double* sums, float* loss,
                  moma_stream_t stream);
int moma_hint_bwd(const void* x, const void* t, const float* gamma, const float* beta, const double* mean, const double* invstd,
                  const double* sums, const float* g_loss, void* dx, float* d_gamma, float* d_beta, int B, int C, int P, int dtype_x,
                  int layout_x, int dtype_t, int layout_t, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SRRL Softmax Regression Representation Learning (`--distill srrl`) on one pair of pooled features -- replaces what follows the
 *      convolution in SRRL.forward (models/util.py: BatchNorm2d in training mode -> ReLU, then the TEACHER'S classifier on the result)
 *      together with the two nn.MSELoss of train_student_moma.py:365-371 / helper/loops_moma.py:340-342 and their autograd backward.
 *      For x (the convolution's output) and t (the teacher's feat[-1]), both [B, C], W [K, C] and bias [K] the teacher classifier's
 *      Linear, logits [B, K] the teacher's, gamma and beta [C]:
 *          mean_c = sum_b x / B     var_c = sum_b x^2 / B - mean_c^2   (biased; sums and variance in double)
 *          invstd_c = 1 / sqrt(var_c + eps)       xh = (x - mean_c) invstd_c   (centred and scaled in double, rounded to fp32)
 *          y = max(0, gamma_c xh + beta_c)        p = y W^T + bias     (fp32 FMA over 32 channels, those sums added in double; p
 *                                                                       rounded once to fp32)
 *          loss = sum (y - t)^2 / (B C) + sum (p - logits)^2 / (B K)
 *          dY = 2 / (B C) (y - t) + 2 / (B K) (p - logits) W           g = dY [y > 0]   (strictly greater, as in torch)
 *          A_c = sum_b g        B_c = sum_b g xh
 *          d_beta_c = g_loss A_c     d_gamma_c = g_loss B_c     dx = g_loss gamma_c invstd_c (g - A_c / B - xh B_c / B)
 *          running_mean_c <- (1 - momentum) running_mean_c + momentum mean_c
 *          running_var_c  <- (1 - momentum) running_var_c  + momentum var_c B / (B - 1)
 *      x, t, dx: MOMA_DT_F32 or MOMA_DT_BF16, chosen per side, rows contiguous and dense, aligned to their element size only (element
 *      accesses of 32 neighbouring channels: no row length or base address is special); dx has x's dtype.  W, bias, logits, gamma,
 *      beta, the running statistics, dxu, d_gamma, d_beta, loss and g_loss are fp32; sums (A [C] then B [C]) and the workspace are
 *      double, 8-byte aligned.  Every sum over the batch is double.  No atomics: bitwise reproducible, independent of the grid.
 *      t, logits, W and bias get no gradient (the classifier is the teacher's and constant).
 *
 * workspace      moma_srrl_workspace_bytes(B, C, K): mean, invstd, the per-channel and per-row squared errors, the split partial sums
 *                of both products in double and p - logits [B, K] in fp32; written and read by moma_srrl_fwd alone.
 * moma_srrl_fwd  -> loss [1], sums [2 C] and dxu [B, C] = dx for g_loss = 1 (everything is linear in g_loss, so the forward forms
 *                the whole gradient and x, t, W, logits are not read again); running_mean / running_var / bias (each nullable);
 *                y_out [B, C] and pred_out [B, K] (each nullable, fp32): y and p as the loss saw them.  Five launches.
 * moma_srrl_bwd  dx (nullable) = round(dxu g_loss) in x's dtype; d_gamma, d_beta (each nullable) from sums.  One launch.  g_loss is a
 *                DEVICE scalar (the upstream gradient of the loss, e.g. a GradScaler factor): nothing is read back to the host.
 *      B < 2: MOMA_E_SHAPE (one value per channel has no variance; torch refuses likewise); B > MOMA_SRRL_MAX_B, C > MOMA_SRRL_MAX_C or
 *      K > MOMA_SRRL_MAX_K: MOMA_E_UNSUPPORTED; unknown dtype: MOMA_E_DTYPE.  Nothing is launched in either case.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_SRRL_MAX_B = 1024, MOMA_SRRL_MAX_C = 4096, MOMA_SRRL_MAX_K = 1024 };
size_t moma_srrl_workspace_bytes(int B, int C, int K);
int moma_srrl_fwd(const void* x, const void* t, const float* W, const float* bias, const float* logits, const float* gamma,
                  const float* beta, float* running_mean, float* running_var, float momentum, float eps, int B, int C, int K,
                  int dtype_x, int dtype_t, void* workspace, size_t workspace_bytes, double* sums, float* dxu, float* loss,
                  float* y_out, float* pred_out, moma_stream_t stream);
int moma_srrl_bwd(const float* dxu, const double* sums, const float* g_loss, void* dx, float* d_gamma, float* d_beta, int B, int C,
                  int dtype_x, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * CC   Correlation Congruence (`--distill correlation`) on one pair of flattened features -- replaces both LinearEmbed heads
 *      (models/util.py: nn.Linear on each side's feat[-1]), Correlation.forward (distiller_zoo/CC.py: |f_s - f_t|, the product of
 *      neighbouring rows, summed over the columns, averaged over the B - 1 pairs) and their autograd backward.  For x_s [B, Cs],
 *      x_t [B, Ct] (the teacher's, constant), W_s [D, Cs], b_s [D], W_t [D, Ct], b_t [D]:
 *          d = x_s W_s^T + b_s - (x_t W_t^T + b_t)      (products and sums in double: exact products; each side's total formed
 *                                                        separately, subtracted, the bias difference added; d rounded ONCE to
 *                                                        fp32)
 *          delta = |d|     loss = sum_{i < B - 1} sum_k delta[i,k] delta[i+1,k] / (B - 1)     (down the rows of a column, in double)
 *          G[i,k] = sign(d[i,k]) (delta[i-1,k] + delta[i+1,k]) / (B - 1)        (a missing neighbour counts 0; sign(0) = 0)
 *          dx_s = g_loss G W_s     dW_s = g_loss G^T x_s     db_s = g_loss colsum(G)     dW_t = -g_loss G^T x_t     db_t = -db_s
 *                                                       (fp32 FMA over 32 elements, those sums added in double)
 *      x_s, x_t, dx_s: MOMA_DT_F32 or MOMA_DT_BF16, chosen per side, rows contiguous and dense, aligned to their element size only
 *      (element accesses: no row length or base address is special); dx_s has x_s's dtype.  The weights, the biases, their gradients,
 *      gu, d_out, loss and g_loss are fp32; the workspace is 8-byte aligned.  Every reduction total is double.  No atomics: bitwise
 *      reproducible, independent of the allocation.  x_t gets no gradient.  BOTH heads are trained: W_t and b_t get theirs.
 *
 * workspace      moma_cc_workspace_bytes(B, Cs, Ct, D): the split partial sums of d and the columns' sums in double, d in fp32;
 *                written and read by moma_cc_fwd alone.
 * moma_cc_fwd    -> loss [1] and gu [B, D] = G (it does not depend on g_loss); d_out [B, D] (nullable, fp32): d as the loss saw it.
 *                Three launches.
 * moma_cc_bwd    ONE grouped launch over the output tiles of dx_s (needs W_s), dW_s (needs x_s), dW_t (needs x_t) and the bias sums;
 *                every output is nullable (at least one must be asked for), an input is needed only by its output.  g_loss is a
 *                DEVICE scalar, multiplied in double before the one rounding: a power of two scales every bit pattern exactly.
 *                db_t is db_s with the sign bit flipped.
 *      B < 2: MOMA_E_SHAPE (the reference's mean over an empty slice is NaN); B > MOMA_CC_MAX_B, Cs or Ct > MOMA_CC_MAX_C or
 *      D > MOMA_CC_MAX_D: MOMA_E_UNSUPPORTED; unknown dtype: MOMA_E_DTYPE.  Nothing is launched in either case.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_CC_MAX_B = 1024, MOMA_CC_MAX_C = 4096, MOMA_CC_MAX_D = 4096 };
size_t moma_cc_workspace_bytes(int B, int Cs, int Ct, int D);
int moma_cc_fwd(const void* x_s, const void* x_t, const float* W_s, const float* b_s, const float* W_t, const float* b_t, int B, int Cs,
                int Ct, int D, int dtype_s, int dtype_t, void* workspace, size_t workspace_bytes, float* gu, float* loss, float* d_out,
                moma_stream_t stream);
int moma_cc_bwd(const float* gu, const void* x_s, const void* x_t, const float* W_s, const float* g_loss, void* dx_s, float* dW_s,
                float* db_s, float* dW_t, float* db_t, int B, int Cs, int Ct, int D, int dtype_s, int dtype_t, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * CE   The classification head of the teacher trainer (`train_teacher.py`) -- replaces nn.CrossEntropyLoss (mean over the rows,
 *      ignore_index -100), helper/util.accuracy (top-1) and, in validation, the argmax and confusion matrix of
 *      process_accumulated_output, with their autograd backward.  For logits z [B, K] and labels y [B]:
 *          m_b = max_k z[b,k]     pred_b = the LOWEST k with z[b,k] = m_b     lse_b = m_b + log1p(sum_{k != pred_b} exp(z[b,k] - m_b))
 *          row_b = lse_b - z[b,y_b] (formed as log1p(..) + (m_b - z[b,y_b]))  for a VALID row, 0 <= y_b < K
 *          loss = sum_valid row_b / n_valid                                   (n_valid = 0: NaN, as nn.CrossEntropyLoss)
 *          dz[b,k] = g_loss (exp(z[b,k] - lse_b) - [k == y_b]) / n_valid      (a row that is not valid: exact zeros)
 *      Every sum, exponential and logarithm is double; lse and 1 / n_valid are kept in double.
 *      z, dz: MOMA_DT_F32 or MOMA_DT_BF16, rows contiguous and dense, aligned to their element size (16-byte or 4-element accesses
 *      where the base address and K allow, element accesses otherwise: K = 5 is as legal as K = 8); dz has z's dtype.  labels: int64.
 *      A label of -100 is ignored: no loss, left out of the mean, no gradient, never a hit, nothing in conf.  ANY OTHER label outside
 *      [0, K) is never used as an index: it makes loss NaN, its row of dz zero, and is counted in stats[3] (stock torch answers it
 *      with a device-side assert that ends the process: a deliberate deviation).
 *
 * workspace      moma_ce_workspace_bytes(B, K) (8-byte aligned): the rows' losses, predictions and flags between the two launches.
 * moma_ce_fwd    -> loss [1] fp32; lse [B] and inv_n [1] = 1 / n_valid, double, for moma_ce_bwd; and, each nullable:
 *                pred [B] int32; stats [4] double, to which it ADDS (sum of the valid rows' losses, hits, valid rows, rows with a bad
 *                label); conf [K, K] int64 (row = label, column = prediction), to which it adds 1 at [y_b, pred_b] per valid row.
 *                Two launches: the rows (G lanes per row, G the power of two in 1 .. 64 that covers ceil(K / 16); rows of up to
 *                MOMA_CE_ONE_WALK_K elements are read once, longer ones twice), then ONE workgroup that adds the rows' losses in row
 *                order (256 consecutive runs of rows, their sums in order) and rounds loss once.  conf takes integer atomics (exact);
 *                no floating-point total does: bitwise reproducible, independent of the allocation (the access width follows the
 *                base address's alignment, and with it the last bits of lse).  Nothing happens on the host but the argument checks.
 * moma_ce_bwd    -> dz.  One launch, no reduction.  g_loss is a DEVICE scalar (fp32), multiplied in double before the one rounding:
 *                a power of two scales every bit pattern exactly.
 *      B < 1 or K < 1: MOMA_E_SHAPE; unknown dtype: MOMA_E_DTYPE; B > MOMA_CE_MAX_B or K > MOMA_CE_MAX_K: MOMA_E_UNSUPPORTED (the
 *      caps keep every element index, B K and K K, below 2^31).  Nothing is launched and nothing written in any of these cases.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_CE_MAX_B = 16384, MOMA_CE_MAX_K = 32768, MOMA_CE_ONE_WALK_K = 1024 };
size_t moma_ce_workspace_bytes(int B, int K);
int moma_ce_fwd(const void* z, const int64_t* labels, int B, int K, int dtype, void* workspace, size_t workspace_bytes, float* loss,
                double* lse, double* inv_n, int32_t* pred, double* stats, int64_t* conf, moma_stream_t stream);
int moma_ce_bwd(const void* z, const int64_t* labels, const double* lse, const double* inv_n, const float* g_loss, void* dz, int B,
                int K, int dtype, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * KDHEAD   The student's head of every `--distill` step -- replaces nn.CrossEntropyLoss(logit_s, y), DistillKL(T)(logit_s, logit_t)
 *      (distiller_zoo/KD.py: two divisions, log_softmax, softmax, kl_div batchmean, times T^2), helper/util.accuracy (top-1) and the
 *      .float() cast in front of them (helper/loops_moma.py:278-279), with their autograd backward to the student's logits.  For
 *      z_s, z_t [B, K], labels y [B] and a host float T > 0, with a = z / T and p = softmax(a) per row:
 *          m_b = max_k z_s[b,k]     pred_b = the LOWEST k with z_s[b,k] = m_b     (one maximum serves z_s and a_s: T > 0)
 *          lse_b = logsumexp z_s[b,:]     lseS_b = logsumexp a_s[b,:]     lseT_b = logsumexp a_t[b,:]
 *          ce_b = lse_b - z_s[b,y_b]                                              for a VALID row, 0 <= y_b < K
 *          kl_b = sum_k p_t[b,k] (log p_t[b,k] - log p_s[b,k])                    (a term with p_t = 0 counts 0)
 *          loss_cls = sum_valid ce_b / n_valid     loss_div = T^2 sum_b kl_b / B     acc = 100 #{b : pred_b == y_b} / B
 *          dz_s[b,k] = g_cls (softmax(z_s)[b,k] - [k == y_b]) / n_valid           (zero for a row that is not valid)
 *                    + g_div T (p_s[b,k] - p_t[b,k]) / B
 *      Every logsumexp leaves the maximum's own term out of its sum and adds it back with log1p; kl_b is summed on the rows' shifted
 *      values beside the teacher's sum of exponentials (no third walk over memory), so rows with z_t = z_s give exactly 0, in the loss
 *      and in the KL part of dz_s.  Every sum, exponential and logarithm is double; the three lse and 1 / n_valid are kept in double.
 *      z_s, z_t: MOMA_DT_F32 or MOMA_DT_BF16 INDEPENDENTLY, rows contiguous and dense, aligned to their element size (16-byte or
 *      4-element accesses where both base addresses and K allow, element accesses otherwise); dz_s has z_s's dtype; z_t gets no
 *      gradient.  labels: int64, by the rule of CE above: -100 is ignored (no CE term, left out of its mean, no CE gradient, never a
 *      hit); ANY OTHER label outside [0, K) is never used as an index: it makes loss_cls NaN and its row's CE gradient zero.  The KL
 *      term does not look at labels; acc divides by B, as helper/util.accuracy does.
 *
 * workspace        moma_kdhead_workspace_bytes(B, K) (8-byte aligned): the rows' CE and KL terms and flags between the two launches.
 * moma_kdhead_fwd  -> out [3] fp32 = (loss_cls, loss_div, acc); saved [3 B + 1] double = lse [B], lseS [B], lseT [B], 1 / n_valid, for
 *                  moma_kdhead_bwd.  Two launches: the rows (G lanes per row as CE; rows of up to MOMA_KDHEAD_ONE_WALK_K elements are
 *                  read once for BOTH operands, longer ones twice), then ONE workgroup that adds the rows' terms in row order (256
 *                  consecutive runs of rows, their sums in order) and rounds each result once.  No floating-point atomics: bitwise
 *                  reproducible.  Nothing happens on the host but the argument checks.
 * moma_kdhead_bwd  -> dz_s.  One launch, no reduction.  g_cls and g_div are DEVICE scalars (fp32); either may be NULL (= 0: that part
 *                  is not evaluated), not both.  Both parts are multiplied and added in double before the one rounding: a power of two
 *                  in both scales every bit pattern exactly.
 *      B < 1, K < 1, or T not finite or <= 0: MOMA_E_SHAPE; unknown dtype: MOMA_E_DTYPE; B > MOMA_KDHEAD_MAX_B or K > MOMA_KDHEAD_MAX_K:
 *      MOMA_E_UNSUPPORTED (CE's caps).  Nothing is launched and nothing written in any of these cases.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_KDHEAD_MAX_B = 16384, MOMA_KDHEAD_MAX_K = 32768, MOMA_KDHEAD_ONE_WALK_K = 1024 };
size_t moma_kdhead_workspace_bytes(int B, int K);
int moma_kdhead_fwd(const void* z_s, const void* z_t, const int64_t* labels, int B, int K, int dtype_s, int dtype_t, float T,
                    void* workspace, size_t workspace_bytes, float* out, double* saved, moma_stream_t stream);
int moma_kdhead_bwd(const void* z_s, const void* z_t, const int64_t* labels, const double* saved, const float* g_cls, const float* g_div,
                    void* dz, int B, int K, int dtype_s, int dtype_t, float T, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * RKDRelational Knowledge Distillation (`--distill rkd`) on one pair of feature rows -- replaces RKDLoss.forward
 *      (distiller_zoo/RKD.py: pdist -> smooth L1 of the mean-normalised distances, and unsqueeze-difference -> F.normalize -> bmm ->
 *      smooth L1 of the angles) and its autograd backward to f_s, without any [B, B, D] temporary.  For f_s [B, Ds], f_t [B, Dt]
 *      (each side's feat[-1] flattened), per side S_ij = sum_k (x_ik - x_jk)^2, summed from the differences in double: exactly 0
 *      on the diagonal and for equal rows, S_ij and S_ji the same bits.  Then
 *          d_ij = sqrt(max(S_ij, 1e-12)) (0 for i = j)    mu = sum_ij d_ij / (B (B - 1))
 *          l_d = (1/B^2) sum_ij sl1(d^s_ij / mu^s - d^t_ij / mu^t)        sl1(z) = z^2 / 2 for |z| < 1, |z| - 1/2 otherwise
 *          n_ab = max(sqrt(S_ab), 1e-12)    A_a[b,c] = (S_ab + S_ac - S_bc) / (2 n_ab n_ac), 0 wherever S_ab = 0 or S_ac = 0
 *          l_a = (1/B^3) sum_abc sl1(A^s_a[b,c] - A^t_a[b,c])             loss = w_d l_d + w_a l_a
 *          Q_ij = d loss / d S^s_ij, the B^2 entries taken as independent (no gradient from d_ij where S_ij < 1e-12: the clamp)
 *          dF_s = g_loss M (f_s - batch mean),  M = -2 (Q + Q^T) off the diagonal, each diagonal entry minus its row's other entries
 *      A pair of EXACTLY equal student rows contributes value 0 and gradient 0 to the angle term (the reference's autograd divides
 *      by F.normalize's clamp 1e-12 there and returns gradients of 1e10).  The gradient goes to f_s only.
 *      f, f_s, dF_s: MOMA_DT_F32 or MOMA_DT_BF16, rows contiguous, aligned to their element size (16-byte loads where the base
 *      address and D allow); S, Q and the workspace are double, 8-byte aligned; terms, loss and g_loss fp32.  All arithmetic in
 *      double.  2 <= B <= MOMA_RKD_MAX_B (else MOMA_E_UNSUPPORTED, nothing is launched), any D >= 1.  No atomics: bitwise reproducible.
 *
 * workspace       moma_rkd_workspace_bytes(B) = (2 B^2 + 4 B + ceil(B / 16)^2) 8 bytes: 1 / n of both sides, four row sums per row and
 *                 one partial sum per 16 x 16 tile; written and read by moma_rkd_terms alone.
 * moma_rkd_dist   one side: f [B, D] -> S [B, B].  Call it once for f_s and once for f_t (Ds and Dt may differ).
 * moma_rkd_terms  S_s, S_t -> Q [B, B], terms [2] = (l_d, l_a), loss [1].
 * moma_rkd_bwd    f_s, Q -> dF_s [B, D] in f_s's dtype; g_loss is a DEVICE scalar (the upstream gradient of the loss, e.g. a GradScaler
 *                 factor): nothing is read back to the host.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_RKD_MAX_B = 1024 };
size_t moma_rkd_workspace_bytes(int B);
int moma_rkd_dist(const void* f, int B, int D, int dtype, double* S, moma_stream_t stream);
int moma_rkd_terms(const double* S_s, const double* S_t, int B, float w_d, float w_a, void* workspace, size_t workspace_bytes,
                   double* Q, float* terms, float* loss, moma_stream_t stream);
int moma_rkd_bwd(const void* f_s, const double* Q, const float* g_loss, void* dF_s, int B, int D, int dtype, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SP  Similarity-Preserving distillation (`--distill similarity`) on one pair of feature maps -- replaces Similarity.similarity_loss
 *     (distiller_zoo/SP.py: view(bsz, -1) -> mm with its transpose -> F.normalize(dim=1) per side -> mean squared difference) and
 *     its autograd backward to f_s.  X = f_s as [B, Ks], Y = f_t as [B, Kt] (Ks and Kt may differ), all indices over the batch:
 *         G = X X^T    n_i = max(|G_i|_2, 1e-12)    H = G / n (row-wise)    (per side)
 *         loss = (1/B^2) sum_ij (H^t_ij - H^s_ij)^2
 *         E = -(2/B^2) (H^t - H^s)    Q_i = (E_i - (E_i . H^s_i) H^s_i) / n^s_i   (the projection only where |G^s_i| >= 1e-12: the clamp)
 *         M = Q + Q^T    dF_s = g_loss M X
 *     G is invariant under a permutation of the K columns applied to every row alike, so f is read IN STORAGE ORDER as [B, K] with
 *     row stride K and dF_s is written in that order: an NCHW-contiguous map and a channels_last map are both passed as they lie in
 *     memory, no layout flag exists.  Required: sample 0 is dense and every sample has the same strides.
 *     f, f_s, dF_s: MOMA_DT_F32 or MOMA_DT_BF16, aligned to their element size (16-byte loads where the base address and K allow,
 *     element loads otherwise).  The products run on the f32-input MFMA (fp32 storage) or the bf16-input MFMA (bf16 storage: the
 *     products of two bf16 are exact in its fp32 accumulator); an fp32 accumulation chain is one staged slab long -- 64 columns for
 *     fp32 storage, 128 for bf16 -- and is then added to a double total.  A split's double total is rounded ONCE to fp32 when the
 *     partial is written (half an fp32 ulp of the partial at most); moma_sp_terms adds the partials of a side in double, in the order
 *     of the splits.  G, H, rows, M are double, 8-byte aligned; loss and g_loss fp32.  1 <= B <= MOMA_SP_MAX_B (else
 *     MOMA_E_UNSUPPORTED, nothing is launched), any K >= 1.  No atomics: bitwise reproducible.
 *
 * workspace      of ONE side: moma_sp_workspace_bytes(B, K) = splits(B, K) B^2 4 bytes, splits = min(ceil(K / 128), ceil(512 / pairs)),
 *                pairs = nt (nt + 1) / 2, nt = ceil(B / 64): the split-K partial Gram matrices, written by moma_sp_gram and read by
 *                moma_sp_terms.  4-byte aligned.
 * moma_sp_gram   one side: f [B, K] -> its workspace.  Call it once for f_s and once for f_t, each with a workspace of its own.
 * moma_sp_terms  both workspaces (with the K each was written for) -> G [2, B, B] (student, teacher), H [2, B, B], rows [4, B]
 *                (n^s, n^t -- not clamped --, E_i . H^s_i, the row's sum of (H^t - H^s)^2), M [B, B], loss [1].
 * moma_sp_bwd    f_s, M -> dF_s [B, K] in f_s's dtype and storage order; g_loss is a DEVICE scalar (the upstream gradient of the loss,
 *                e.g. a GradScaler factor): nothing is read back to the host.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_SP_MAX_B = 1024 };
size_t moma_sp_workspace_bytes(int B, long long K);
int moma_sp_gram(const void* f, int B, long long K, int dtype, void* workspace, size_t workspace_bytes, moma_stream_t stream);
int moma_sp_terms(const void* workspace_s, size_t workspace_s_bytes, long long Ks, const void* workspace_t, size_t workspace_t_bytes,
                  long long Kt, int B, double* G, double* H, double* rows, double* M, float* loss, moma_stream_t stream);
int moma_sp_bwd(const void* f_s, const double* M, const float* g_loss, void* dF_s, int B, long long K, int dtype, moma_stream_t stream);
/* moma_sp_gram_sum  the first half of moma_sp_terms on its own (`--distill semckd`: ops.batch_gram): the workspace of ONE side that
 *                moma_sp_gram wrote for (B, K) -> G [B, B] fp32 = the split partials added in double in the order of the splits (the
 *                very sum of moma_sp_terms, one copy of the code), rounded once to fp32.  Both triangles hold the same bits.  With
 *                the rounding of each split's partial, G lies within (splits + 1) 2^-24 of |X| |X|^T (entry-wise, |.| the absolute
 *                values) of the product of the stored values; where every partial sum is exact in fp32 it IS that product.  With
 *                M = dG + dG^T (double) and a device scalar 1, moma_sp_bwd is its backward.  Same guards as moma_sp_terms. */
int moma_sp_gram_sum(const void* workspace, size_t workspace_bytes, long long K, int B, float* G, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SEMCKD  Cross-Layer Distillation with Semantic Calibration (`--distill semckd`) -- replaces SemCKDLoss.forward
 *      (distiller_zoo/SemCKD.py: S x T times MSELoss(reduction='none') -> reshape -> mean -> a strided write into ind_loss, then the
 *      weighted sum) and its autograd backward, for ALL pairs of (student map i, teacher map j) in ONE grouped call each way.
 *      Pair p = i T + j has x_p (the projection's output) and t_p (the pooled teacher map), both [B, n_p], n_p = C h w; with the
 *      attention w [B,S,T] fp32:
 *          ind[b,p]  = (1/n_p) sum_k (x_p[b,k] - t_p[b,k])^2
 *          loss      = (1/(B S)) sum_b sum_p w[b,p] ind[b,p]
 *          dx_p[b,k] = g_loss 2 w[b,p] / (n_p B S) (x_p[b,k] - t_p[b,k])        (in x_p's dtype)
 *          dw[b,p]   = g_loss ind[b,p] / (B S)                                  (left to the caller: a multiply of ind)
 *      Both maps of a pair lie on a common grid and in the SAME memory format; each side is read in storage order as B rows of n_p
 *      elements (dense, row stride n_p), NCHW and channels_last alike: the sum of squares does not depend on the order of the
 *      columns, and dx_p is written in that order.  No layout flag exists.  Per side and per pair the dtype is MOMA_DT_F32 or
 *      MOMA_DT_BF16, the pointers aligned to the element size (16-byte accesses where the base addresses of the pair and n_p allow,
 *      element accesses otherwise).  The difference and the square are fp32, every sum double; a bf16 dx is rounded from the fp32
 *      value.  No atomics: bitwise reproducible.  t gets no gradient.
 *      `pairs` is a HOST array, read during the call (as moma_infonce_fused_multi and moma_mha_fwd_fast read theirs).
 *
 * workspace        moma_semckd_workspace_bytes() = B sum_p ceil(n_p / MOMA_SEMCKD_CHUNK) 8 bytes: one double per work item (pair,
 *                  sample, chunk of MOMA_SEMCKD_CHUNK elements).  The pairs differ widely in n_p, so the launches run over this flat
 *                  list (the host fills a prefix table of chunk counts, a workgroup finds its pair in it), not over a grid of pairs.
 *                  8-byte aligned.  0 for arguments moma_semckd_fwd refuses.
 * moma_semckd_fwd  one read of every x_p and t_p -> ind [B,S,T] fp32, loss [1] fp32.  Two launches: the streaming one writes one
 *                  double partial per item, the finalize one adds the partials of a (b,p) in chunk order.  `dx` is ignored.
 * moma_semckd_bwd  one launch over the same list: writes every non-null pairs[p].dx, with no reduction of its own.  g_loss is a
 *                  DEVICE scalar (the upstream gradient of the loss, e.g. a GradScaler factor): nothing is read back to the host.
 *      n_pairs outside 1 .. MOMA_SEMCKD_MAX_PAIRS, S < 1, n_pairs % S != 0, B < 1 or any n_p < 1: MOMA_E_SHAPE; an unknown dtype:
 *      MOMA_E_UNSUPPORTED; nothing is launched and nothing written in either case.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_SEMCKD_MAX_PAIRS = 64, MOMA_SEMCKD_CHUNK = 4096 };
typedef struct moma_semckd_pair {
    const void* x;         /* [B, n] dtype_x */
    const void* t;         /* [B, n] dtype_t */
    void* dx;              /* [B, n] dtype_x out (moma_semckd_bwd) or NULL */
    long long n;           /* elements of one sample: C h w */
    int dtype_x, dtype_t;  /* MOMA_DT_* */
} moma_semckd_pair_t;
size_t moma_semckd_workspace_bytes(const moma_semckd_pair_t* pairs, int n_pairs, int B);
int moma_semckd_fwd(const moma_semckd_pair_t* pairs, int n_pairs, int S, int B, const float* w, void* workspace,
                    size_t workspace_bytes, float* ind, float* loss, moma_stream_t stream);
int moma_semckd_bwd(const moma_semckd_pair_t* pairs, int n_pairs, int S, int B, const float* w, const float* g_loss,
                    moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * PKT  Probabilistic Knowledge Transfer (`--distill pkt`) on one pair of feature rows -- replaces PKT.cosine_similarity_loss
 *      (distiller_zoo/PKT.py: rows / (norm + eps) -> mm with the transpose -> (. + 1) / 2 -> rows / row sums per side -> mean of
 *      T log((T + eps) / (P + eps))) and its autograd backward to f_s, without a normalised copy of either side.  For f_s [B, Ds],
 *      f_t [B, Dt] (each side's feat[-1] flattened), eps = 1e-7, per side
 *          G = F F^T    n_i = sqrt(G_ii)    C_ij = G_ij / ((n_i + eps)(n_j + eps))    K = (C + 1) / 2    r_i = sum_j K_ij
 *          P_ij = K_ij / r_i (student: P, teacher: T)        loss = (1/B^2) sum_ij T_ij log((T_ij + eps) / (P_ij + eps))
 *          U_ij = -(1/B^2) T_ij / (P_ij + eps)    s_i = sum_k U_ik P_ik    W_ij = (U_ij - s_i) / (2 r_i)    M = W + W^T
 *          c_i = sum_j M_ij C^s_ij    M'_ij = M_ij / ((n_i + eps)(n_j + eps)) - [i = j] c_i / (n_i (n_i + eps))    dF_s = g_loss M' f_s
 *      The diagonal term is 0 where n_i = 0: an ALL-ZERO student row gets the finite derivative of x / (|x| + eps) at 0 (the
 *      reference's autograd returns NaN for that row).  Nothing is clamped (K may fall a few ulps below 0; P + eps stays
 *      positive).  The gradient goes to f_s only.
 *      f, f_s, dF_s: MOMA_DT_F32 or MOMA_DT_BF16, rows contiguous, aligned to their element size (16-byte loads where the base
 *      address and D allow); G, M and the workspace are double, 8-byte aligned; loss and g_loss fp32.  All arithmetic in double on
 *      the f64 MFMA.  1 <= B <= MOMA_PKT_MAX_B (else MOMA_E_UNSUPPORTED, nothing is launched), any D >= 1.  G and M (= M' above) are
 *      symmetric bit for bit.  No atomics: bitwise reproducible.  Three launches forward (four with one moma_pkt_gram per side), one
 *      backward.
 *
 * workspace       moma_pkt_workspace_bytes(B) = (B^2 + 2 B) 8 bytes: W, one KL row sum and the student's norm per row; written and read
 *                 by moma_pkt_terms alone.  0 for B < 1 and B > MOMA_PKT_MAX_B.
 * moma_pkt_gram   one side: f [B, D] -> G [B, B].  Call it once for f_s and once for f_t (Ds and Dt may differ).
 * moma_pkt_gram_pair  both sides in ONE launch (the side in the grid's third dimension): the same bits in G_s and G_t as two
 *                 moma_pkt_gram calls.  With it the forward is three launches.
 * moma_pkt_terms  G_s, G_t -> M [B, B] (the M' above), loss [1].
 * moma_pkt_bwd    f_s, M -> dF_s [B, D] in f_s's dtype; g_loss is a DEVICE scalar (the upstream gradient of the loss, e.g. a GradScaler
 *                 factor): nothing is read back to the host.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_PKT_MAX_B = 1024 };
size_t moma_pkt_workspace_bytes(int B);
int moma_pkt_gram(const void* f, int B, int D, int dtype, double* G, moma_stream_t stream);
int moma_pkt_gram_pair(const void* f_s, int Ds, int dtype_s, const void* f_t, int Dt, int dtype_t, int B, double* G_s, double* G_t,
                       moma_stream_t stream);
int moma_pkt_terms(const double* G_s, const double* G_t, int B, void* workspace, size_t workspace_bytes, double* M, float* loss,
                   moma_stream_t stream);
int moma_pkt_bwd(const void* f_s, const double* M, const float* g_loss, void* dF_s, int B, int D, int dtype, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K1  batch-token multi-head attention -- replaces Attention.forward
 *     (MoMA/criterion_moco_att.py:153-167) and its autograd backward.
 *     x [N,d] -> qkv = x Wqkv^T + bqkv -> per head softmax(q k^T * hd^-1/2) v -> y = a Wproj^T + bproj.
 *
 *   Two families of entry points; moma_mha_saved_state() says which one a configuration takes:
 *
 *   MOMA_MHA_SAVE_LSE  ->  the FAST path (moma_mha_pack_weights / moma_mha_fwd_fast / moma_mha_bwd_fast): MOMA_PREC_BF16 with a
 *     head dim that is a multiple of 16: up to 128 (every `--head mlp` configuration) at any N, wider heads up to 1024
 *     (`--head None`: EfficientNet-B0 1280 / 4 = 320, ResNet-50 2048 / 4 = 512) at N <= 1024.  Flash-style: the forward keeps the
 *     row log-sum-exp lse [H,N] (log2 units, scale included) and the backward recomputes P per tile, so no [H,N,N] array
 *     exists at any N (attn = 'all' runs over N = 2B + K tokens).  Everything a launch reads more than once is bf16:
 *       pack    caller-owned, moma_mha_pack_bytes(d) bytes: [Wqkv | Wproj | Wqkv^T | Wproj^T] as bf16, written by
 *               moma_mha_pack_weights (one launch; with_transposed = 0 fills only the first half -- enough for a forward);
 *               the caller refreshes it when the fp32 weights change (after optimizer.step());
 *       qkv16   [N,3d] bf16, the Q third pre-scaled by hd^-1/2 * log2(e);  attn16 [N,d] bf16  (both saved for the backward,
 *               together with x, lse and the pack);
 *     moma_mha_fwd_fast runs n_modules <= 4 modules of equal (N, d, H) in the SAME three launches (qkv linear, per-head core,
 *     proj linear: blockIdx selects the module) -- the loop's atts_k and atts_queue (helper/loops_moma.py:327-329) run as one
 *     group.  A module with qpack != NULL also gets y * qpack_scale in the packed bf16 MFMA-operand layout that
 *     moma_infonce_fused_q consumes (so K2 needs no pre-pack launch; the buffer has moma_infonce_qpack_bytes(N, d) bytes and
 *     its pad rows must be zero -- zero it once).
 *     moma_mha_bwd_fast: 3 launches -- {dA = dy Wproj with the row dots D, dWproj, dbproj} -> core (dQ | dK | dV) ->
 *     {dWqkv, dbqkv, dx}.  dx / (dw_qkv, db_qkv) / (dw_proj, db_proj) may be NULL to skip them; a bias gradient is only
 *     produced together with its weight gradient.  workspace: moma_mha_bwd_fast_workspace_bytes().
 *
 *   MOMA_MHA_SAVE_PROBS  ->  the STAGED path (moma_mha_fwd / moma_mha_bwd): the reference's op chain on one generic MFMA GEMM
 *     plus row softmax kernels -- exact fp32 under MOMA_PREC_F32 (f32-input MFMA), any N, d, H; keeps qkv [N,3d],
 *     attn_out [N,d] and probs [H,N,N] in fp32 for the backward.
 *     bwd writes dx [N,d], dw_qkv [3d,d], db_qkv [3d], dw_proj [d,d], db_proj [d]; any of the five may be NULL to skip it.
 *     bwd workspace: moma_mha_bwd_workspace_bytes().
 *   No atomics anywhere: results are bitwise reproducible run to run.  One device per process (kernel attributes are set once).
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_MHA_SAVE_PROBS = 0, MOMA_MHA_SAVE_LSE = 1 };
int moma_mha_saved_state(int N, int d, int H, int prec);
int moma_mha_fwd(const float* x, const float* w_qkv, const float* b_qkv, const float* w_proj,
                 const float* b_proj, float* y, float* qkv, float* probs, float* attn_out,
                 int N, int d, int H, int prec, moma_stream_t stream);
size_t moma_mha_bwd_workspace_bytes(int N, int d, int H, int prec);
int moma_mha_bwd(const float* x, const float* w_qkv, const float* w_proj, const float* qkv,
                 const float* probs, const float* attn_out, const float* dy, float* dx,
                 float* dw_qkv, float* db_qkv, float* dw_proj, float* db_proj, void* workspace,
                 size_t workspace_bytes, int N, int d, int H, int prec, moma_stream_t stream);

typedef struct moma_mha_module {
    const void* x;        /* [N,d] input, fp32 or bf16 (x_dtype)                           */
    const void* pack;     /* bf16 weight pack (moma_mha_pack_weights)                      */
    const float* b_qkv;   /* [3d] or NULL                                                  */
    const float* b_proj;  /* [d]                                                           */
    float* y;             /* [N,d] fp32 output                                             */
    void* qkv16;          /* [N,3d] bf16 out (saved for the backward / scratch)            */
    void* attn16;         /* [N,d]  bf16 out (saved for the backward / scratch)            */
    float* lse;           /* [H,N] out, or NULL for a forward without backward             */
    void* qpack;          /* NULL, or moma_infonce_qpack_bytes(N,d) bytes: packed y * qpack_scale for moma_infonce_fused_q */
    float qpack_scale;
    int x_dtype;          /* MOMA_DT_F32 / MOMA_DT_BF16: storage type of x (a bf16 x -- the output of a bf16-autocast head -- is
                             consumed as it stands: the products round x to bf16 either way, the values are identical)        */
} moma_mha_module_t;
size_t moma_mha_pack_bytes(int d);
int moma_mha_pack_weights(const float* w_qkv, const float* w_proj, void* pack, int d, int with_transposed,
                          moma_stream_t stream);
int moma_mha_fwd_fast(const moma_mha_module_t* modules, int n_modules, int N, int d, int H, moma_stream_t stream);
size_t moma_mha_bwd_fast_workspace_bytes(int N, int d, int H);
int moma_mha_bwd_fast(const void* pack, const void* x, int x_dtype, const void* qkv16, const void* attn16, const float* lse,
                      const float* dy, float* dx, float* dw_qkv, float* db_qkv, float* dw_proj, float* db_proj,
                      void* workspace, size_t workspace_bytes, int N, int d, int H, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * BN  BatchNorm2d + fused activation on NCHW activations -- the `_swish(_bn(conv(x)))` pairs of the
 *     backbones inside the step (models/efficientnet_pytorch/model.py:96-102,114; nn.BatchNorm2d
 *     semantics: batch statistics + running-stat update (momentum, unbiased variance) when
 *     training != 0, running statistics otherwise).  Not one of the KD-term kernels: an HBM-streaming
 *     helper for the step's throughput (3 passes forward, 5 backward instead of 5 + 8 unfused).
 *     x, out, dout, dx: [N, C, HW] contiguous, MOMA_DT_F32 or MOMA_DT_BF16; gamma/beta/running/save: fp32 [C]
 *     (gamma, beta, running_* may be NULL when training).  act: MOMA_ACT_*.  The backward recomputes the
 *     pre-activation from x and save_mean/save_invstd (written by the forward, eval mode included).
 *     workspace >= moma_bn_workspace_bytes(C) for either call.
 *     plane_mean (nullable, [N*C], activation dtype): the forward also emits mean_hw(out[n,c]) -- the squeeze of
 *     a squeeze-excite block that follows (replaces a separate F.adaptive_avg_pool2d pass); dplane_mean (nullable)
 *     is its gradient, folded into the backward as dout + dplane_mean / HW.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_ACT_NONE = 0, MOMA_ACT_SILU = 1, MOMA_ACT_RELU = 2 };
size_t moma_bn_workspace_bytes(int C);
int moma_bn_fwd(const void* x, void* out, const float* gamma, const float* beta, float* running_mean,
                float* running_var, float* save_mean, float* save_invstd, void* workspace,
                size_t workspace_bytes, int N, int C, int HW, int dtype, int act, int training,
                float momentum, float eps, void* plane_mean, moma_stream_t stream);
int moma_bn_bwd(const void* x, const void* dout, const float* gamma, const float* beta,
                const float* save_mean, const float* save_invstd, void* dx, float* dgamma, float* dbeta,
                void* workspace, size_t workspace_bytes, int N, int C, int HW, int dtype, int act,
                int training, const void* dplane_mean, moma_stream_t stream);
/*     The forward without its apply pass, for a consumer that applies the normalisation itself while it reads x
 *     (the _pre entry points of the depthwise convolution below): the statistics, the running-statistics update,
 *     save_mean / save_invstd and scale_shift [C][2] fp32 (caller-owned) with
 *       act(BN(x))[n,c,:] = act(x[n,c,:] * scale_shift[c][0] + scale_shift[c][1]),
 *     bit-identical to what the forward call computes for the same x (training == 0: from the running statistics).
 *     Same workspace as the forward call; moma_bn_bwd takes x and the saved statistics as after a forward call. */
int moma_bn_prepare(const void* x, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, float* save_mean, float* save_invstd, float* scale_shift,
                    void* workspace, size_t workspace_bytes, int N, int C, int HW, int dtype, int training,
                    float momentum, float eps, moma_stream_t stream);
/*     BN + activation applied inside the squeeze-excite gate that consumes it (the _bn1 -> SE pair of an MBConv block):
 *     a = act(BN(x)) is neither written nor kept.  All tensors as above; pooled, s, ds, dpooled: [N*C] of the activation dtype.
 *       moma_bn_act_mean       the statistics and finalize of moma_bn_prepare (save_*, running_*, scale_shift [C][2], same
 *                              workspace) and pooled[n,c] = mean_hw a[n,c,:] from one read-only pass: pooled, the saved and the
 *                              running statistics are bit-identical to moma_bn_fwd(..., plane_mean)
 *       moma_bn_act_gate_fwd   out = round(a) * sigmoid(s[n,c]), a rounded to the activation dtype first: bit-identical to
 *                              moma_se_gate_fwd on the a that moma_bn_fwd stores
 *       moma_bn_gate_bwd_sums  one pass over (x, dout = d out): five sums per plane (double) into the workspace, and from the
 *                              fifth ds[n,c] = sigmoid'(s) * sum_hw dout * round(a) (ds nullable); from the other four ...
 *       moma_bn_gate_bwd       ... forms dgamma, dbeta (nullable) per channel once dpooled (nullable: the gradient of pooled) is
 *                              known, and writes dx (nullable) = BN's input gradient for
 *                              dy = (dout * sigmoid(s) + dpooled / HW) * act'(y); training as in moma_bn_bwd
 *     The two backward calls share ONE workspace >= moma_bn_gate_workspace_bytes(N, C), 16-byte aligned, untouched in between.
 *     No atomics: bitwise reproducible.  (The vector width of the read-only pass follows x's alignment alone; moma_bn_fwd's
 *     follows x and out: pooled has moma_bn_fwd's bits where out is aligned as x is, e.g. both to 32 bytes.) */
size_t moma_bn_gate_workspace_bytes(int N, int C);
int moma_bn_act_mean(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                     float* save_mean, float* save_invstd, float* scale_shift, void* pooled, void* workspace,
                     size_t workspace_bytes, int N, int C, int HW, int dtype, int act, int training, float momentum,
                     float eps, moma_stream_t stream);
int moma_bn_act_gate_fwd(const void* x, const float* scale_shift, const void* s, void* out, int N, int C, int HW,
                         int dtype, int act, moma_stream_t stream);
int moma_bn_gate_bwd_sums(const void* x, const void* dout, const void* s, const float* scale_shift,
                          const float* save_mean, const float* save_invstd, void* ds, void* workspace,
                          size_t workspace_bytes, int N, int C, int HW, int dtype, int act, moma_stream_t stream);
int moma_bn_gate_bwd(const void* x, const void* dout, const void* s, const void* dpooled, const float* scale_shift,
                     const float* save_mean, const float* save_invstd, void* dx, float* dgamma, float* dbeta,
                     void* workspace, size_t workspace_bytes, int N, int C, int HW, int dtype, int act, int training,
                     moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * DW  depthwise convolution (groups == channels) on NCHW activations -- the MBConv `_depthwise_conv`
 *     layers of the backbones inside the step (models/efficientnet_pytorch/model.py:59-64,100; TF "SAME"
 *     padding, possibly asymmetric: pad_top / pad_left are given, bottom / right follow from OH / OW).
 *     Like BN a throughput helper for the step, not a KD-term kernel.  K in {3,5}, stride in {1,2}.
 *       y[n,c,oy,ox] = sum_{ky,kx} w[c,ky,kx] * x[n,c, oy*S+ky-pad_top, ox*S+kx-pad_left]   (zero outside)
 *     x, dx [N,C,H,W]; y, dy [N,C,OH,OW]: MOMA_DT_F32 or MOMA_DT_BF16;  w, dw [C,K,K] fp32.
 *     bwd_weight needs workspace >= moma_dwconv_workspace_bytes(C, K).
 * ------------------------------------------------------------------------------------------- */
size_t moma_dwconv_workspace_bytes(int C, int K);
int moma_dwconv_fwd(const void* x, const float* w, void* y, int N, int C, int H, int W, int OH, int OW,
                    int K, int stride, int pad_top, int pad_left, int dtype, moma_stream_t stream);
int moma_dwconv_bwd_data(const void* dy, const float* w, void* dx, int N, int C, int H, int W, int OH,
                         int OW, int K, int stride, int pad_top, int pad_left, int dtype,
                         moma_stream_t stream);
int moma_dwconv_bwd_weight(const void* x, const void* dy, float* dw, void* workspace,
                           size_t workspace_bytes, int N, int C, int H, int W, int OH, int OW, int K,
                           int stride, int pad_top, int pad_left, int dtype, moma_stream_t stream);
/*     The same two calls on a = act(BN(x)) without a materialised a: x is the BatchNorm's input and scale_shift
 *     [C][2] fp32 comes from moma_bn_prepare; every element is normalised, activated (act: MOMA_ACT_*) and rounded
 *     to the storage dtype as it is read, the zero padding is that of a.  Results are bit-identical to
 *     moma_bn_fwd followed by the plain call.  (The gradient w.r.t. a is moma_dwconv_bwd_data as it is; moma_bn_bwd
 *     then turns it into the gradient w.r.t. x.)  An act outside MOMA_ACT_* is answered with MOMA_E_DTYPE, as by the BN calls. */
int moma_dwconv_fwd_pre(const void* x, const float* w, void* y, int N, int C, int H, int W, int OH, int OW,
                        int K, int stride, int pad_top, int pad_left, int dtype, const float* scale_shift,
                        int act, moma_stream_t stream);
int moma_dwconv_bwd_weight_pre(const void* x, const void* dy, float* dw, void* workspace,
                               size_t workspace_bytes, int N, int C, int H, int W, int OH, int OW, int K,
                               int stride, int pad_top, int pad_left, int dtype, const float* scale_shift,
                               int act, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * PW  weight gradient of a pointwise (1 x 1, stride 1, no padding, groups 1) convolution on NCHW activations -- the MBConv
 *     `_expand_conv` / `_project_conv` / `_se_reduce` / `_se_expand` layers and `_conv_head` of the backbones inside the step
 *     (models/efficientnet_pytorch/model.py, MBConvBlock).  A throughput helper like BN / DW: replaces MIOpen's transpose -> fill ->
 *     split-K product -> cast chain with one read of both operands as they lie.
 *       dw[co, ci] = sum_{n, p} dy[n, co, p] * x[n, ci, p]
 *     x [N, Cin, HW], dy [N, Cout, HW], dw [Cout, Cin]: dense, MOMA_DT_BF16, aligned to 2 bytes (16- and 8-byte loads where the
 *     addresses and HW allow, element loads otherwise).  MOMA_DT_F32 is answered with MOMA_E_DTYPE: the caller keeps its stock
 *     path for fp32.  HW = 1 (the squeeze-excite layers) is the same call.  Products are exact in fp32 (bf16-input MFMA);
 *     K = N HW is split over workgroups, the fp32 partials go to the workspace (moma_pwconv_workspace_bytes(), 16-byte
 *     aligned) and are added in the order of the splits, then rounded once to bf16.  No atomics: bitwise reproducible.
 * ------------------------------------------------------------------------------------------- */
size_t moma_pwconv_workspace_bytes(int N, int Cin, int Cout, int HW);
int moma_pwconv_bwd_weight(const void* x, const void* dy, void* dw, void* workspace, size_t workspace_bytes, int N, int Cin,
                           int Cout, int HW, int dtype, moma_stream_t stream);

/*     Forward and input gradient of the same convolution on one streaming bf16 MFMA kernel (csrc/pwstream.hip): x is read once
 *     in 16-byte rows as it lies in NCHW, transposed on the way out of LDS, and y is written in 16-byte pieces of 8 pixels.
 *       moma_pwconv_fwd       y [N, Cout, HW] :  y[n, co, p]  = sum_ci w[co, ci] * x[n, ci, p]       (no bias)
 *       moma_pwconv_bwd_data  dx [N, Cin, HW] :  dx[n, ci, p] = sum_co w[co, ci] * dy[n, co, p]
 *     w [Cout, Cin] in both (the input gradient reads it transposed in place).  All operands dense, MOMA_DT_BF16, aligned to
 *     2 bytes (16- / 8-byte accesses where HW and the addresses allow, element accesses otherwise: any N, Cin, Cout, HW >= 1 is
 *     computed).  fp32 accumulation, one rounding to bf16.  No workspace, no atomics, no host synchronisation: bitwise
 *     reproducible, safe under graph capture.  MOMA_DT_F32 is answered with MOMA_E_DTYPE; a refused call writes nothing. */
int moma_pwconv_fwd(const void* x, const void* w, void* y, int N, int Cin, int Cout, int HW, int dtype, moma_stream_t stream);
int moma_pwconv_bwd_data(const void* dy, const void* w, void* dx, int N, int Cin, int Cout, int HW, int dtype,
                         moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * SE  squeeze-excite helpers on NCHW activations (models/efficientnet_pytorch/model.py:104-110):
 *     moma_plane_mean     mean[n,c] = mean_hw x[n,c,:,:]                       (F.adaptive_avg_pool2d(x, 1))
 *     moma_se_gate_fwd    out = x * sigmoid(s[n,c])                            (torch.sigmoid(x_squeezed) * x)
 *     moma_se_gate_bwd    dx = dout * sigmoid(s);  ds = sigmoid'(s) * sum_hw(dout * x)   -- one pass
 *     x, out, dout, dx: [NC, HW] contiguous; mean, s, ds: [NC]; all of dtype MOMA_DT_F32 or MOMA_DT_BF16.
 *     Throughput helpers of the step like BN / DW, not KD-term kernels.
 * ------------------------------------------------------------------------------------------- */
int moma_plane_mean(const void* x, void* mean, int NC, int HW, int dtype, moma_stream_t stream);
int moma_se_gate_fwd(const void* x, const void* s, void* out, int NC, int HW, int dtype, moma_stream_t stream);
int moma_se_gate_bwd(const void* x, const void* s, const void* dout, void* dx, void* ds, int NC, int HW,
                     int dtype, moma_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * IN   the input batch: raw uint8 rows of a data pack -> the tensor the backbones read -- replaces, per batch, the tail of the
 *      reference's transforms (dataset/histo_dataset.py:194-239 and :1054-1058: RandomHorizontalFlip, CenterCrop,
 *      RandomResizedCrop, ToTensor, Normalize) and the layout / dtype passes behind them.  One launch, no workspace, no atomics.
 *          src   uint8 [N, H, W, 3]                         idx   int64 [B], or NULL: sample b is row b of src
 *          flip  uint8 [B], or NULL: none                   box   int32 [B, 4] = (top, left, h, w), or NULL: the centred S_h x S_w
 *          lut   fp32 [3, 256]: lut[c][v] = ((v / 255) - mean_c) / std_c, built by the caller in ToTensor's and Normalize's order
 *          out   [B, 3, S_h, S_w] of `dtype`, dense in MOMA_LAYOUT_NCHW or MOMA_LAYOUT_NHWC (channels_last memory)
 *      The centred window has CenterCrop's offsets: (H - S_h) / 2 and (W - S_w) / 2, a half rounded to the even neighbour.
 *      resample = 0   out[b, c, y, x] = lut[c][ src[idx_b, top + y, left + x', c] ],  x' = S_w - 1 - x where flip[b], else x; the
 *                     box's h, w are not read.  S_h > H or S_w > W: MOMA_E_SHAPE.
 *      resample = 1   bilinear over the box onto S_h x S_w with half-pixel centres: the source coordinate of output o is
 *                     (o + 0.5) h / S - 0.5 clamped to [0, h - 1], the second tap clamped to h - 1, columns likewise.  The taps'
 *                     weights are kept as integers over 2 S (exact); the four products are summed in fp32 (at most five roundings
 *                     of a value <= 255: 7.7e-5) and the result becomes a level by floor(v + 0.5), which then goes through lut.
 *                     Flip mirrors the output column.  h, w are taken into [1, H], [1, W].  A NULL box is the centred window, so
 *                     the same as resample = 0.
 *      Every read is clamped into sample idx_b's own image (rows to [0, H - 1], columns to [0, W - 1]; idx_b to [0, N - 1]).  Every
 *      output element is a value of lut, or its bf16 rounded to nearest even.  src needs no alignment; out is aligned to its element
 *      size (16-byte stores wherever an output row allows, element stores at its unaligned ends).
 *      B == 0: MOMA_OK, nothing done.  Any other size < 1, or resample not 0 / 1: MOMA_E_SHAPE; unknown dtype or layout: MOMA_E_DTYPE;
 *      H, W, S_h or S_w above MOMA_INPUT_MAX_SIDE, or S_h or S_w above MOMA_INPUT_MAX_RESAMPLE with resample = 1: MOMA_E_UNSUPPORTED.
 *      Nothing is launched in any of these cases.
 * ------------------------------------------------------------------------------------------- */
enum { MOMA_INPUT_MAX_SIDE = 16384, MOMA_INPUT_MAX_RESAMPLE = 4096 };
int moma_input_batch(const uint8_t* src, const int64_t* idx, const uint8_t* flip, const int32_t* box, const float* lut, void* out,
                     int N, int H, int W, int B, int S_h, int S_w, int resample, int dtype, int layout, moma_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MOMA_HIP_H */
