// Neuron Selectivity Transfer (`--distill nst`; reference distiller_zoo/NST.py, helper/loops_moma.py:150-154) on one pair of feature
// maps on a common grid, f_s [B,Cs,H,W], f_t [B,Ct,H,W], P = H W.  Per image, X = f_s[b] as [Cs,P], Y = f_t[b] as [Ct,P]:
//     n_i = max(|X_i|, 1e-12)   m_j = max(|Y_j|, 1e-12)   Gss_ij = X_i.X_j / (n_i n_j)   Gst_ij = X_i.Y_j / (n_i m_j)
//     t1 = mean_{b,i,j} Gss^2   t2 = mean_{b,i,j} Gst^2   loss = t1 - 2 t2
//     dX_i = (1/n_i) [ sum_j (a Gss_ij / n_j) X_j - sum_j (c Gst_ij / m_j) Y_j - (r_i / n_i) X_i ],
//     a = 4 / (B Cs^2), c = 4 / (B Cs Ct), r_i = a sum_j Gss_ij^2 - c sum_j Gst_ij^2
// in three kinds of launch, all arithmetic in fp32 on v_mfma_f32_32x32x2_f32 whatever the storage (fp32 or bf16, NCHW or
// channels_last, each chosen per side); no normalised copy of a map is ever stored:
//   nst_gram  one workgroup per (image, block of 32 student rows).  P streams through LDS in slabs of 16 .. 128 pixels (the power of
//             two whose image fits 34 KB: 128 up to 64 rows, 16 from 257 rows on): the WHOLE [Cs + Ct, slab] piece of both maps
//             (fp32, odd row stride), of which the workgroup's 32 rows are the A operand and every
//             32-row tile a B operand; wave w owns column tiles w, w + 4, w + 8, w + 12 (Cs + Ct <= 512: at most 4 x 16 accumulator
//             registers).  The squared norms of all rows are summed from the staged slab by the threads, in the order of the
//             MFMA's own fmaf chain.  fp32 chains are cut every 128 pixels and added to a second set of accumulators.
//             Epilogue: G = raw / (n n) in double, rounded once -> G [B, Cs, Cs + Ct], norms [B, Cs + Ct], the rows' sums of
//             Gss^2 and Gst^2 [B, Cs, 2], and the workgroup's partial sums of both [B, blocks, 2].
//             Every one of an image's ceil(Cs / 32) workgroups stages both maps whole and sums all norms: the maps are REQUESTED
//             1 / 2 / 4 / 8 times at up to 32 / 64 / 128 / 256 student channels (an image's workgroups are neighbours in the grid, so
//             the repeats can meet in L2; G is written once).
//             hipcc -O3, gfx950: 156 VGPRs + 64 AGPRs (the accumulators; the totals are VGPRs), two workgroups per compute unit, no
//             spill, no scratch; LDS 34 KB slab + 4 KB reciprocal norms + 1 KB.
//   nst_loss  one workgroup adds the partials in a fixed order in double -> terms (t1, t2) and loss.
//   nst_bwd   one workgroup per (image, tile of 64 pixels): dX[:, tile] = Coef [Cs, Cs + Ct] . [X ; Y][:, tile], the right operand the
//             RAW maps, streamed once in slabs of 16 channels; the coefficients of a slab are formed from G, the norms and the row
//             sums (double, rounded once; the upstream gradient, a DEVICE scalar, folded in) while they are staged.  Wave w owns the
//             output tiles (row tile, pixel half) w, w + 4, ...: all Cs rows stay in accumulators (<= 4 x 16; every slab's chain of
//             16 products is added to a double total: for maps far from zero mean the sum cancels to a tenth of its terms).
//             dF_s is written in f_s's dtype and layout.
//             Both maps and G are read once, dF_s is written once.
//             hipcc -O3, gfx950: 232 - 236 VGPRs (128 of them the double totals) + 64 AGPRs (the accumulators), one workgroup per
//             compute unit, no spill, no scratch; LDS 17 KB coefficients + 6 KB slab + 8 KB factors.
// Workspace of a pair: G, B Cs (Cs + Ct) 4 bytes.  Cs, Ct <= 256.  16-byte loads where the address and the contiguous extent (P, or
// C) allow, element loads otherwise.  No atomics: every sum has an order that depends on the shapes alone -- bitwise repeatable.
#include "common.hpp"

namespace moma {
namespace {

constexpr int NST_THREADS = 256;
constexpr int NST_MAXC = 256;
constexpr int NST_MAXN = 2 * NST_MAXC;
constexpr int NST_BK = 16;                  // pixels (nst_gram) / channels (nst_bwd) of one staged slab
constexpr int NST_LDA = NST_BK + 1;         // row stride of a [rows, 16] LDS image: 32 consecutive rows fall in 32 banks
constexpr int NST_CHUNK = 8;                // slabs per fp32 accumulation chain
constexpr int NST_BP = 64;                  // pixels of one nst_bwd workgroup
constexpr int NST_LDZ = NST_BP + 32;        // row stride of the [16, 64] slab: the two k rows of an MFMA step in disjoint banks
constexpr double NST_EPS = 1e-12;           // F.normalize's clamp of the norm

struct NstShape {
    int B, Cs, Ct, P;
    int nhwc_s, nhwc_t;                     // memory [B, P, C] instead of [B, C, P]
    int vec_s, vec_t;                       // 16-byte loads are possible on that side
};

// row of accumulator register `reg` in a 32 x 32 MFMA result (the column is lane & 31)
__device__ __forceinline__ int nst_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

// channels [c0, c0 + nc) x pixels [p0, p0 + 2^lg) of one image -> lds[(c - c0) * ld + (p - p0)] as fp32, zero where p >= P.
// vec: c0 and nc are multiples of the vector width (channels_last), p0 is (NCHW), and the side's base is 16-byte aligned
template <typename T>
__device__ __forceinline__ void nst_stage(const T* __restrict__ fb, int C, int P, int nhwc, int vec, int c0, int nc, int p0, int lg,
                                          float* __restrict__ lds, int ld) {
    constexpr int V = MAXVEC<T>, LGV = V == 8 ? 3 : 2;
    const int tid = threadIdx.x, TP = 1 << lg;                     // tile width in pixels: 16 .. 128
    if (!nhwc) {
        if (vec) {
            const int lgvp = lg - LGV, VP = 1 << lgvp;
            for (int idx = tid; idx < nc * VP; idx += NST_THREADS) {
                const int r = idx >> lgvp, pv = idx & (VP - 1), p = p0 + pv * V;
                float v[V];
#pragma unroll
                for (int e = 0; e < V; ++e) v[e] = 0.f;
                if (p < P) PV<T, V>::ld(fb + (size_t)(c0 + r) * P + p, v);          // (P % V == 0: all V inside)
                float* o = lds + r * ld + pv * V;
#pragma unroll
                for (int e = 0; e < V; ++e) o[e] = v[e];
            }
        } else {
            for (int idx = tid; idx < nc * TP; idx += NST_THREADS) {
                const int r = idx >> lg, pp = idx & (TP - 1), p = p0 + pp;
                lds[r * ld + pp] = p < P ? ld1<T>(fb + (size_t)(c0 + r) * P + p) : 0.f;
            }
        }
    } else {
        if (vec) {
            const int ncv = nc / V;
            for (int idx = tid; idx < TP * ncv; idx += NST_THREADS) {
                const int pp = idx / ncv, cv = idx % ncv, p = p0 + pp;
                float v[V];
#pragma unroll
                for (int e = 0; e < V; ++e) v[e] = 0.f;
                if (p < P) PV<T, V>::ld(fb + (size_t)p * C + c0 + cv * V, v);
#pragma unroll
                for (int e = 0; e < V; ++e) lds[(cv * V + e) * ld + pp] = v[e];
            }
        } else {
            for (int idx = tid; idx < TP * nc; idx += NST_THREADS) {
                const int pp = idx / nc, r = idx % nc, p = p0 + pp;
                lds[r * ld + pp] = p < P ? ld1<T>(fb + (size_t)p * C + c0 + r) : 0.f;
            }
        }
    }
}

// grid (B * nrb): image b, student rows [32 rb, 32 rb + 32)
template <typename TS, typename TT>
__global__ __launch_bounds__(NST_THREADS) void nst_gram_kernel(const TS* __restrict__ fs, const TT* __restrict__ ft,
                                                               float* __restrict__ G, float* __restrict__ norms,
                                                               float* __restrict__ rows, float* __restrict__ partials,
                                                               const NstShape q, int nrb, int lgk) {
    __shared__ float tile[NST_MAXN * NST_LDA];
    __shared__ double inv[NST_MAXN];
    __shared__ float red[4][32][2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.x / nrb, rb = blockIdx.x % nrb, r0 = rb * 32;
    const int Cs = q.Cs, Ct = q.Ct, P = q.P;
    const int N = Cs + Ct, Npad = (N + 31) & ~31, NT = Npad >> 5;
    const int BK = 1 << lgk, LDA = BK + 1;                        // pixels per slab: as many as the LDS image holds for Npad rows
    const int every = BK >= NST_CHUNK * NST_BK ? 1 : (NST_CHUNK * NST_BK) >> lgk;      // slabs per fp32 chain (128 pixels)
    for (int idx = N * LDA + tid; idx < Npad * LDA; idx += NST_THREADS) tile[idx] = 0.f;          // rows the staging never writes
    f32x16 acc[4], tot[4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[s][r] = 0.f; tot[s][r] = 0.f; }
    float sq[2] = {0.f, 0.f}, sqt[2] = {0.f, 0.f};                // |row tid|^2 and |row tid + 256|^2: chain and total
    const TS* fsb = fs + (size_t)b * Cs * P;
    const TT* ftb = ft + (size_t)b * Ct * P;
    const int nk = (P + BK - 1) >> lgk;
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();                                                           // the slab of the previous turn has been read
        nst_stage<TS>(fsb, Cs, P, q.nhwc_s, q.vec_s, 0, Cs, kt << lgk, lgk, tile, LDA);
        nst_stage<TT>(ftb, Ct, P, q.nhwc_t, q.vec_t, 0, Ct, kt << lgk, lgk, tile + Cs * LDA, LDA);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int row = tid + u * NST_THREADS;
            if (row < N) {
                const float* t = tile + row * LDA;
                for (int k0 = 0; k0 < BK; k0 += NST_BK)
#pragma unroll
                    for (int kk = 0; kk < NST_BK; ++kk) sq[u] = fmaf(t[k0 + kk], t[k0 + kk], sq[u]);
            }
        }
        for (int k0 = 0; k0 < BK; k0 += NST_BK)
#pragma unroll
            for (int kk = 0; kk < NST_BK; kk += 2) {
                const float a = tile[(r0 + l31) * LDA + k0 + kk + h];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int t = w + 4 * s;
                    if (t < NT) {                                                  // (wave-uniform)
                        const float bv = tile[(32 * t + l31) * LDA + k0 + kk + h];
                        acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[s], 0, 0, 0);
                    }
                }
            }
        if (kt % every == every - 1 || kt == nk - 1) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int r = 0; r < 16; ++r) { tot[s][r] += acc[s][r]; acc[s][r] = 0.f; }
#pragma unroll
            for (int u = 0; u < 2; ++u) { sqt[u] += sq[u]; sq[u] = 0.f; }
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int row = tid + u * NST_THREADS;
        if (row < N) {
            const double n = fmax(sqrt((double)sqt[u]), NST_EPS);
            inv[row] = 1.0 / n;
            if (rb == 0) norms[(size_t)b * N + row] = (float)n;
        }
    }
    __syncthreads();
    float rs[16], rt[16];                                        // this lane's share of sum_j Gss^2 / Gst^2 of its 16 rows
#pragma unroll
    for (int r = 0; r < 16; ++r) { rs[r] = 0.f; rt[r] = 0.f; }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int t = w + 4 * s;
        if (t < NT) {
            const int j = 32 * t + l31;
            if (j < N) {
                const double ij = inv[j];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int i = r0 + nst_row(r, h);
                    if (i < Cs) {
                        const float g = (float)((double)tot[s][r] * inv[i] * ij);
                        G[((size_t)b * Cs + i) * N + j] = g;
                        if (j < Cs) rs[r] = fmaf(g, g, rs[r]);
                        else rt[r] = fmaf(g, g, rt[r]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float a = half32_sum(rs[r]), c = half32_sum(rt[r]);
        if (l31 == 0) { red[w][nst_row(r, h)][0] = a; red[w][nst_row(r, h)][1] = c; }
    }
    __syncthreads();
    if (tid < 32) {
        const float v0 = (red[0][tid][0] + red[1][tid][0]) + (red[2][tid][0] + red[3][tid][0]);
        const float v1 = (red[0][tid][1] + red[1][tid][1]) + (red[2][tid][1] + red[3][tid][1]);
        if (r0 + tid < Cs) {
            rows[((size_t)b * Cs + r0 + tid) * 2] = v0;
            rows[((size_t)b * Cs + r0 + tid) * 2 + 1] = v1;
        }
        red[0][tid][0] = v0;                                     // (rows past Cs carry 0)
        red[0][tid][1] = v1;
    }
    __syncthreads();
    if (tid == 0) {
        double p0 = 0.0, p1 = 0.0;
        for (int r = 0; r < 32; ++r) { p0 += (double)red[0][r][0]; p1 += (double)red[0][r][1]; }
        partials[(size_t)blockIdx.x * 2] = (float)p0;
        partials[(size_t)blockIdx.x * 2 + 1] = (float)p1;
    }
}

// terms = (t1, t2), loss = t1 - 2 t2 from the n workgroup partials: thread t adds partials t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(NST_THREADS) void nst_loss_kernel(const float* __restrict__ partials, long long n, float* __restrict__ terms,
                                                               float* __restrict__ loss, double inv1, double inv2) {
    __shared__ double sh[2][4];
    double s0 = 0.0, s1 = 0.0;
    for (long long i = threadIdx.x; i < n; i += NST_THREADS) { s0 += (double)partials[2 * i]; s1 += (double)partials[2 * i + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s0; sh[1][threadIdx.x >> 6] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t1 = ((sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3])) * inv1;
        const double t2 = ((sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3])) * inv2;
        terms[0] = (float)t1;
        terms[1] = (float)t2;
        *loss = (float)(t1 - 2.0 * t2);
    }
}

// grid (B * ptiles): image b, pixels [64 pt, 64 pt + 64).  The sum runs over the student's channels in slabs of 16, then the teacher's
template <typename TS, typename TT>
__global__ __launch_bounds__(NST_THREADS) void nst_bwd_kernel(const TS* __restrict__ fs, const TT* __restrict__ ft,
                                                              const float* __restrict__ G, const float* __restrict__ norms,
                                                              const float* __restrict__ rows, const float* __restrict__ g_loss,
                                                              TS* __restrict__ dF, const NstShape q, int vec_out, int ptiles,
                                                              double alpha, double beta) {
    __shared__ float Cl[NST_MAXC * NST_LDA];
    __shared__ float Zl[NST_BK * NST_LDZ];
    __shared__ double rowf[NST_MAXC], rdiag[NST_MAXC], colf[NST_MAXN];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.x / ptiles, p0 = (blockIdx.x % ptiles) * NST_BP;
    const int Cs = q.Cs, Ct = q.Ct, P = q.P;
    const int N = Cs + Ct, CsPad = (Cs + 31) & ~31, NT = 2 * (CsPad >> 5);
    const double gl = (double)*g_loss;
    const float* nb = norms + (size_t)b * N;
    for (int i = tid; i < CsPad; i += NST_THREADS) {
        double rf = 0.0, rd = 0.0;
        if (i < Cs) {
            const double n = (double)nb[i];
            const double r = alpha * (double)rows[((size_t)b * Cs + i) * 2] - beta * (double)rows[((size_t)b * Cs + i) * 2 + 1];
            rf = gl / n;
            rd = r / n;
        }
        rowf[i] = rf;
        rdiag[i] = rd;
    }
    for (int j = tid; j < N; j += NST_THREADS) colf[j] = (j < Cs ? alpha : -beta) / (double)nb[j];
    f32x16 acc[4];
    double tot[4][16];                                            // the slabs' fp32 chains meet in double: the sum cancels (below)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[s][r] = 0.f; tot[s][r] = 0.0; }
    const TS* fsb = fs + (size_t)b * Cs * P;
    const TT* ftb = ft + (size_t)b * Ct * P;
    const float* Gb = G + (size_t)b * Cs * N;
    const int nxb = (Cs + NST_BK - 1) / NST_BK, nit = nxb + (Ct + NST_BK - 1) / NST_BK;
    const int pt = w & 1;                                         // (tiles w, w + 4, ...: all in the same half of the 64 pixels)
    for (int it = 0; it < nit; ++it) {
        const bool sx = it < nxb;
        const int c0 = (sx ? it : it - nxb) * NST_BK;
        const int nc = min(NST_BK, (sx ? Cs : Ct) - c0);
        const int g0 = sx ? c0 : Cs + c0;                         // first column of G of this slab
        __syncthreads();                                          // (first turn: the factors above are written)
        if (sx) nst_stage<TS>(fsb, Cs, P, q.nhwc_s, q.vec_s, c0, nc, p0, 6, Zl, NST_LDZ);
        else nst_stage<TT>(ftb, Ct, P, q.nhwc_t, q.vec_t, c0, nc, p0, 6, Zl, NST_LDZ);
        for (int idx = nc * NST_BP + tid; idx < NST_BK * NST_BP; idx += NST_THREADS) Zl[(idx / NST_BP) * NST_LDZ + idx % NST_BP] = 0.f;
        for (int idx = tid; idx < CsPad * NST_BK; idx += NST_THREADS) {
            const int i = idx / NST_BK, jj = idx % NST_BK;
            float v = 0.f;
            if (i < Cs && jj < nc) {
                double gv = (double)Gb[(size_t)i * N + g0 + jj] * colf[g0 + jj];
                if (sx && c0 + jj == i) gv -= rdiag[i];
                v = (float)(rowf[i] * gv);
            }
            Cl[i * NST_LDA + jj] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < NST_BK; kk += 2) {
            const float bz = Zl[(kk + h) * NST_LDZ + 32 * pt + l31];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int t = w + 4 * s;
                if (t < NT) {
                    const float a = Cl[(32 * (t >> 1) + l31) * NST_LDA + kk + h];
                    acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bz, acc[s], 0, 0, 0);
                }
            }
        }
        // where the channels resemble each other (maps far from zero mean) dX_i is what is left of sum_j c_ij Z_j after its
        // component along X_i cancels against the diagonal term: chains of 16 products, then double
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (w + 4 * s < NT) {
#pragma unroll
                for (int r = 0; r < 16; ++r) { tot[s][r] += (double)acc[s][r]; acc[s][r] = 0.f; }
            }
    }
    const int p = p0 + 32 * pt + l31;
    if (p >= P) return;                                           // (no barrier below)
    TS* dFb = dF + (size_t)b * Cs * P;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int t = w + 4 * s;
        if (t >= NT) continue;
        const int i0 = 32 * (t >> 1);
        if (!q.nhwc_s) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + nst_row(r, h);
                if (i < Cs) st1<TS>(dFb + (size_t)i * P + p, round_f32(tot[s][r]));
            }
        } else if (vec_out) {                                     // Cs % 4 == 0: registers 4g .. 4g + 3 are four neighbouring channels
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = i0 + 8 * g + 4 * h;
                if (i < Cs) {
                    const float v[4] = {round_f32(tot[s][4 * g]), round_f32(tot[s][4 * g + 1]), round_f32(tot[s][4 * g + 2]), round_f32(tot[s][4 * g + 3])};
                    PV<TS, 4>::st(dFb + (size_t)p * Cs + i, v);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + nst_row(r, h);
                if (i < Cs) st1<TS>(dFb + (size_t)p * Cs + i, round_f32(tot[s][r]));
            }
        }
    }
}

// 16-byte accesses along the contiguous extent (P in NCHW, C in channels_last) of a side, or element accesses
int nst_wide(const void* p, int extent, int dtype) {
    const int eb = dtype == MOMA_DT_BF16 ? 2 : 4;
    return pick_vec(extent, eb, (uintptr_t)p, {16 / eb}) > 1;
}
NstShape nst_shape(const void* fs, const void* ft, int B, int Cs, int Ct, int P, int dt_s, int lay_s, int dt_t, int lay_t) {
    NstShape q;
    q.B = B; q.Cs = Cs; q.Ct = Ct; q.P = P;
    q.nhwc_s = lay_s == MOMA_LAYOUT_NHWC;
    q.nhwc_t = lay_t == MOMA_LAYOUT_NHWC;
    q.vec_s = nst_wide(fs, q.nhwc_s ? Cs : P, dt_s);
    q.vec_t = nst_wide(ft, q.nhwc_t ? Ct : P, dt_t);
    return q;
}

}  // namespace

size_t nst_workspace_bytes(int B, int Cs, int Ct) { return (size_t)B * Cs * ((size_t)Cs + Ct) * sizeof(float); }
long long nst_row_blocks(int Cs) { return (Cs + MOMA_NST_ROW_BLOCK - 1) / MOMA_NST_ROW_BLOCK; }
long long nst_pixel_tiles(int P) { return ((long long)P + NST_BP - 1) / NST_BP; }

template <typename TS, typename TT>
void nst_gram_t(const void* fs, const void* ft, float* G, float* norms, float* rows, float* partials, const NstShape& q, int nrb,
                hipStream_t st) {
    // pixels per slab: the power of two (16 .. 128) whose [Npad, 2^lgk + 1] image fits the LDS array, no wider than the map
    const int Npad = (q.Cs + q.Ct + 31) & ~31;
    int lgk = 4;
    while (lgk < 7 && Npad * ((2 << lgk) + 1) <= NST_MAXN * NST_LDA && (1 << lgk) < q.P) ++lgk;
    hipLaunchKernelGGL((nst_gram_kernel<TS, TT>), dim3((unsigned)((long long)q.B * nrb)), dim3(NST_THREADS), 0, st, (const TS*)fs,
                       (const TT*)ft, G, norms, rows, partials, q, nrb, lgk);
}
template <typename TS, typename TT>
void nst_bwd_t(const void* fs, const void* ft, const float* G, const float* norms, const float* rows, const float* g_loss, void* dF,
               const NstShape& q, int vec_out, int ptiles, double alpha, double beta, hipStream_t st) {
    hipLaunchKernelGGL((nst_bwd_kernel<TS, TT>), dim3((unsigned)((long long)q.B * ptiles)), dim3(NST_THREADS), 0, st, (const TS*)fs,
                       (const TT*)ft, G, norms, rows, g_loss, (TS*)dF, q, vec_out, ptiles, alpha, beta);
}
// f(TypeTag<TS>, TypeTag<TT>) for the storage types of the two sides
template <typename F> void nst_dispatch(int dt_s, int dt_t, F&& f) {
    with_dtype(dt_s, [&](auto ts) { return with_dtype(dt_t, [&](auto tt) { f(ts, tt); return 0; }); });
}

hipError_t launch_nst_gram(const void* fs, const void* ft, int B, int Cs, int Ct, int P, int dt_s, int lay_s, int dt_t, int lay_t,
                           float* G, float* norms, float* rows, float* partials, float* terms, float* loss, hipStream_t st) {
    const NstShape q = nst_shape(fs, ft, B, Cs, Ct, P, dt_s, lay_s, dt_t, lay_t);
    const int nrb = (int)nst_row_blocks(Cs);
    nst_dispatch(dt_s, dt_t, [&](auto ts, auto tt) {
        nst_gram_t<typename decltype(ts)::type, typename decltype(tt)::type>(fs, ft, G, norms, rows, partials, q, nrb, st);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nst_loss_kernel, dim3(1), dim3(NST_THREADS), 0, st, (const float*)partials, (long long)B * nrb, terms, loss,
                       1.0 / ((double)B * Cs * Cs), 1.0 / ((double)B * Cs * Ct));
    return hipGetLastError();
}

hipError_t launch_nst_bwd(const void* fs, const void* ft, const float* G, const float* norms, const float* rows, const float* g_loss,
                          void* dF, int B, int Cs, int Ct, int P, int dt_s, int lay_s, int dt_t, int lay_t, hipStream_t st) {
    const NstShape q = nst_shape(fs, ft, B, Cs, Ct, P, dt_s, lay_s, dt_t, lay_t);
    const int ptiles = (int)nst_pixel_tiles(P);
    const int vec_out = q.nhwc_s && Cs % 4 == 0 && (uintptr_t)dF % 16 == 0;
    const double alpha = 4.0 / ((double)B * Cs * Cs), beta = 4.0 / ((double)B * Cs * Ct);
    nst_dispatch(dt_s, dt_t, [&](auto ts, auto tt) {
        nst_bwd_t<typename decltype(ts)::type, typename decltype(tt)::type>(fs, ft, G, norms, rows, g_loss, dF, q, vec_out, ptiles, alpha,
                                                                            beta, st);
    });
    return hipGetLastError();
}

}  // namespace moma
