// The input batch (moma_input_batch): uint8 [N, H, W, 3] rows of a data pack -> [B, 3, Sh, Sw] fp32 / bf16, NCHW or channels_last, in one
// launch: the gather through idx, the crop window or the bilinear resample of a box, the horizontal flip, ToTensor + Normalize (a
// [3][256] table of the caller's, so every output is a table value or its bf16) and the layout.  A pure stream: 1 byte read and 2 - 4
// bytes written per output element, nothing reduced, no atomics, no workspace.
//
// The work is cut into ITEMS of IN_ROWS (or fewer: what fits LDS) consecutive output rows of one sample; the grid is capped at
// IN_MAX_GRID workgroups which stride over the items.  An item has two phases with a barrier between them:
//   fill    window mode: the source bytes of the item's rows -- 3 * (columns of the window inside the image) bytes per row, at any
//           byte alignment because of `left` -- go to LDS in aligned 16-byte loads: row r is copied from its start rounded DOWN to
//           16 bytes, so its first needed byte sits at (address & 15) of its LDS row.  A 16-byte piece that is not wholly inside
//           src (the first of a misaligned src, the last of the last row of the last sample) is read byte by byte, each inside.
//           resample mode: the columns' taps, one (x0, x1, weight) record per output column, shared by the item's rows; the four
//           taps of an element are then read from global memory (a box is a gather; the taps of neighbours share cache lines).
//   write   a ROW-PLANE is a contiguous run of the output: the Sw elements of one row of one channel (NCHW: 3 per row), or the
//           3 Sw interleaved elements of one row (channels_last).  G = 2^lgG lanes (the power of two that covers a row-plane's
//           16-byte stores, at most a wave) own one row-plane at a time: 16-byte stores over its aligned middle, one lane the
//           elements in front of the first 16-byte boundary, one lane those behind the last.
// Both phases clamp every source row to [0, H - 1] and column to [0, W - 1] of the sample's own image, and idx to [0, N - 1].
#include "common.hpp"

namespace moma {
namespace {

constexpr int IN_THREADS = 256;
constexpr int IN_MAX_GRID = 2048;            // 256 compute units x 8 workgroups (as mapwalk.hpp)
constexpr int IN_ROWS = 8;                   // output rows of an item
constexpr int IN_LUT = 3 * 256;              // floats of the table, at the front of LDS (3072 bytes: the rest stays 16-byte aligned)
constexpr int IN_LDS_BYTES = 60 * 1024;      // of the 64 KiB a workgroup may ask for without an attribute

struct InputShape {
    int N, H, W, B, Sh, Sw;
    int R, nrg;                              // output rows per item, ceil(Sh / R)
    int stride;                              // window mode: bytes of one staged row in LDS (a multiple of 16)
    int lgG;                                 // log2 of the lanes that share a row-plane
    int top0, left0;                         // the centred window (box == NULL)
    long long items;                         // B * nrg
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <typename T, bool NHWC, bool RESAMPLE>
__global__ __launch_bounds__(IN_THREADS) void input_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ idx,
                                                           const uint8_t* __restrict__ flip, const int32_t* __restrict__ box,
                                                           const float* __restrict__ lut, T* __restrict__ out, const InputShape q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* slut = reinterpret_cast<float*>(smem);
    unsigned char* stage = smem + IN_LUT * sizeof(float);
    int2* cols = reinterpret_cast<int2*>(stage);
    constexpr int VEC = MAXVEC<T>;
    constexpr int PLANES = NHWC ? 1 : 3;
    const int tid = threadIdx.x, G = 1 << q.lgG, grp = tid >> q.lgG, li = tid & (G - 1), ngrp = IN_THREADS >> q.lgG;
    const int H = q.H, W = q.W, Sh = q.Sh, Sw = q.Sw, E = NHWC ? 3 * Sw : Sw;
    const uintptr_t src_lo = (uintptr_t)src, src_hi = src_lo + (size_t)q.N * H * W * 3;
    for (int i = tid; i < IN_LUT; i += IN_THREADS) slut[i] = lut[i];

    for (long long it = blockIdx.x; it < q.items; it += gridDim.x) {
        const int b = (int)(it / q.nrg), y_first = (int)(it % q.nrg) * q.R, rcount = min(q.R, Sh - y_first);
        long long n = idx ? idx[b] : b;
        n = n < 0 ? 0 : (n >= q.N ? q.N - 1 : n);
        const bool fl = flip != nullptr && flip[b] != 0;
        int top = q.top0, left = q.left0, bh = Sh, bw = Sw;
        if (box) {
            top = box[4 * b]; left = box[4 * b + 1];
            if constexpr (RESAMPLE) { bh = clampi(box[4 * b + 2], 1, H); bw = clampi(box[4 * b + 3], 1, W); }
        }
        // (a box far outside the image: every read is clamped anyway; keep the sums below inside int)
        top = clampi(top, -MOMA_INPUT_MAX_SIDE, 2 * MOMA_INPUT_MAX_SIDE);
        left = clampi(left, -MOMA_INPUT_MAX_SIDE, 2 * MOMA_INPUT_MAX_SIDE);
        const uint8_t* img = src + (size_t)n * H * W * 3;
        const int lo = clampi(left, 0, W - 1), hi = clampi(left + Sw - 1, 0, W - 1), span = 3 * (hi - lo + 1);

        __syncthreads();                                         // the table is in LDS; the previous item's fill has been read
        if constexpr (!RESAMPLE) {
            const int CH = q.stride >> 4;                        // 16-byte pieces of a staged row
            for (int t = tid; t < rcount * CH; t += IN_THREADS) {
                const int r = t / CH, k = t - r * CH;
                const int row = clampi(top + y_first + r, 0, H - 1);
                const uintptr_t a0 = (uintptr_t)(img + ((size_t)row * W + lo) * 3);
                const int off = (int)(a0 & 15);
                if (16 * k < off + span) {
                    const uintptr_t ca = a0 - off + 16 * (uintptr_t)k;
                    unsigned char* dst = stage + r * q.stride + 16 * k;
                    if (ca >= src_lo && ca + 16 <= src_hi) {
                        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(ca);
                    } else {
                        for (int j = 0; j < 16; ++j) {
                            const uintptr_t a = ca + j;
                            dst[j] = (a >= src_lo && a < src_hi) ? *reinterpret_cast<const uint8_t*>(a) : (unsigned char)0;
                        }
                    }
                }
            }
        } else {
            // output column x: n = (2 x + 1) w - Sw over d = 2 Sw is its source coordinate (clamped to [0, w - 1]); x0 = n / d, the
            // weight of x1 is (n mod d) / d, kept as the integer n mod d
            const int d = 2 * Sw;
            for (int x = tid; x < Sw; x += IN_THREADS) {
                const int nx = clampi((2 * x + 1) * bw - Sw, 0, (bw - 1) * d);
                const int x0 = nx / d, x1 = min(x0 + 1, bw - 1);
                cols[x] = make_int2(clampi(left + x0, 0, W - 1) | (clampi(left + x1, 0, W - 1) << 16), nx - x0 * d);
            }
        }
        __syncthreads();

        for (int rp = grp; rp < rcount * PLANES; rp += ngrp) {
            const int r = NHWC ? rp : rp / 3, c0 = NHWC ? 0 : rp - 3 * r, y = y_first + r;
            T* p = out + (NHWC ? ((size_t)b * Sh + y) * Sw * 3 : (((size_t)b * 3 + c0) * Sh + y) * Sw);
            // the row's source: its staged bytes (window), or its two tap rows and their weights (resample)
            const unsigned char* srow = stage;
            const uint8_t *p0 = img, *p1 = img;
            float gy = 0.f, fy = 0.f, inv = 0.f;
            if constexpr (!RESAMPLE) {
                const int row = clampi(top + y, 0, H - 1);
                srow = stage + r * q.stride + (int)((uintptr_t)(img + ((size_t)row * W + lo) * 3) & 15);
            } else {
                const int d = 2 * Sh, ny = clampi((2 * y + 1) * bh - Sh, 0, (bh - 1) * d);
                const int y0 = ny / d, y1 = min(y0 + 1, bh - 1), ry = ny - y0 * d;
                p0 = img + (size_t)clampi(top + y0, 0, H - 1) * W * 3;
                p1 = img + (size_t)clampi(top + y1, 0, H - 1) * W * 3;
                fy = (float)ry; gy = (float)(d - ry);
                inv = (float)d * (float)(2 * Sw);
            }
            auto value = [&](int e) -> float {
                const int x = NHWC ? e / 3 : e, c = NHWC ? e - 3 * x : c0, xs = fl ? Sw - 1 - x : x;
                int level;
                if constexpr (!RESAMPLE) {
                    level = srow[3 * (clampi(left + xs, 0, W - 1) - lo) + c];
                } else {
                    const int2 t = cols[xs];
                    const int x0 = 3 * (t.x & 0xffff) + c, x1 = 3 * (t.x >> 16) + c;
                    const float fx = (float)t.y, gx = (float)(2 * Sw - t.y);
                    // integers below 2^24: both row sums are exact; then a product, a fused product-sum, the denominator, the
                    // quotient and the + 0.5 round: five roundings of at most half an ulp of 255 each
                    const float ht = (float)p0[x0] * gx + (float)p0[x1] * fx, hb = (float)p1[x0] * gx + (float)p1[x1] * fx;
                    const float v = fmaf(ht, gy, hb * fy) / inv;
                    level = clampi((int)floorf(v + 0.5f), 0, 255);
                }
                return slut[c * 256 + level];
            };
            const int head = min(E, (int)(((16 - ((uintptr_t)p & 15)) & 15) / sizeof(T)));
            const int nbody = (E - head) / VEC, tail = head + nbody * VEC;
            for (int u = li; u < nbody + 2; u += G) {
                if (u < nbody) {
                    const int e0 = head + u * VEC;
                    float v[VEC];
#pragma unroll
                    for (int e = 0; e < VEC; ++e) v[e] = value(e0 + e);
                    PV<T, VEC>::st(p + e0, v);
                } else if (u == nbody) {
                    for (int e = 0; e < head; ++e) st1<T>(p + e, value(e));
                } else {
                    for (int e = tail; e < E; ++e) st1<T>(p + e, value(e));
                }
            }
        }
    }
}

// CenterCrop's offset int(round((H - S) / 2.0)): a half goes to the even neighbour
inline int centre_offset(int full, int s) {
    const int d = full - s, k = d >> 1;
    return (d & 1) ? k + (k & 1) : k;
}

}  // namespace

hipError_t launch_input_batch(const uint8_t* src, const int64_t* idx, const uint8_t* flip, const int32_t* box, const float* lut,
                              void* out, int N, int H, int W, int B, int Sh, int Sw, int resample, int dtype, int layout,
                              hipStream_t st) {
    InputShape q{};
    q.N = N; q.H = H; q.W = W; q.B = B; q.Sh = Sh; q.Sw = Sw;
    const bool nhwc = layout == MOMA_LAYOUT_NHWC;
    const size_t lut_bytes = IN_LUT * sizeof(float);
    size_t lds;
    if (resample) {
        q.R = min(IN_ROWS, Sh);
        q.stride = 0;
        lds = lut_bytes + (size_t)Sw * sizeof(int2);
    } else {
        q.stride = (3 * Sw + 15 + 15) / 16 * 16;                                  // any start inside the first 16 bytes
        q.R = max(1, min(min(IN_ROWS, Sh), (int)((IN_LDS_BYTES - lut_bytes) / q.stride)));
        lds = lut_bytes + (size_t)q.R * q.stride;
    }
    if (lds > IN_LDS_BYTES) return hipErrorInvalidValue;                           // (the entry point's caps rule this out)
    q.nrg = (Sh + q.R - 1) / q.R;
    q.items = (long long)B * q.nrg;
    q.top0 = centre_offset(H, Sh);
    q.left0 = centre_offset(W, Sw);
    const int vec = dtype == MOMA_DT_BF16 ? MAXVEC<bf16_raw> : MAXVEC<float>;
    const int units = (nhwc ? 3 * Sw : Sw) / vec + 2;                              // 16-byte stores of a row-plane, head, tail
    int lg = 0;
    while (lg < 6 && (1 << lg) < units) ++lg;
    q.lgG = lg;
    const unsigned grid = (unsigned)min(q.items, (long long)IN_MAX_GRID);
    with_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(IN_THREADS), lds, st, src, idx, flip, box, lut, (T*)out, q); };
        if (nhwc) { if (resample) go(input_kernel<T, true, true>); else go(input_kernel<T, true, false>); }
        else { if (resample) go(input_kernel<T, false, true>); else go(input_kernel<T, false, false>); }
        return 0;
    });
    return hipGetLastError();
}

}  // namespace moma
