// Weight gradient of a pointwise (1 x 1, stride 1) convolution on NCHW activations:
//     dW[co, ci] = sum_n sum_p dY[n, co, p] * X[n, ci, p]            (x [N, Cin, HW], dy [N, Cout, HW], bf16; dW bf16)
// MIOpen's winning solver for these problems transposes both operands into an NHWC workspace, zero-fills, runs a small
// split-K product and casts -- passes over memory the result does not need.  In NCHW both operands already lie as the bf16
// MFMA wants them: row = channel, K = pixel, K contiguous.  v_mfma_f32_16x16x32_bf16 takes from lane l the 8 k-values
// 8 (l >> 4) .. + 7 of row l & 15 for A and for B alike, so a fragment is one 16-byte load per lane and nothing is staged.
//   * K = N HW is cut into units of 64 pixels of one image (a unit never crosses an image: the tail of a plane is padded with
//     zeros in registers).  Lane (r, q) = (l & 15, l >> 4) loads the 16 pixels 16 q .. + 15 of its row -- the wave covers 128
//     contiguous bytes of each row -- and feeds the first 8 to one MFMA step and the second 8 to the next; A and B use the
//     same assignment of pixels to k slots, which is all the sum needs.
//   * one wave owns TM x TN tiles of 16 x 16 outputs (TM, TN in {1, 2, 4}: 4 .. 64 accumulator registers) over a contiguous
//     range of units; the four waves of a workgroup own neighbouring tiles over the SAME range, so what they share is
//     fetched once.  Outputs of up to 64 x 64 (the 112^2 / 56^2 layers, where the bytes are) are one wave's tile: x and dy are
//     read from memory once.  No LDS, no barriers.  Two register sets: the loads of the next unit are in flight while the
//     MFMAs of this one run.
//   * split s writes its fp32 partial [Cout, Cin] to the workspace; the finalize kernel adds the partials in the order of
//     the splits, rounds once to bf16 and writes dW.  No atomics: bitwise reproducible.
//   * access width VEC in {8, 4, 1} elements by pick_vec from HW and the operands' addresses (49-pixel planes: element loads).
//     The 1 x 1-plane form (the squeeze-excite convolutions: K = N, rows strided by the channel count) runs as ONE image of
//     N "pixels" with pixel stride C on the element-load instantiation.
// Every load address is clamped into the operand (rows to C - 1, pixel groups to 0) and masked afterwards, so the loads stay
// unconditional and in bounds; rows past C only reach accumulators that are never stored.
#include "common.hpp"

namespace moma {
namespace {

constexpr int PW_WAVES = 4;          // waves per workgroup: neighbouring wave tiles over one range of K
constexpr int PW_UNIT = 64;          // pixels per K unit: two MFMA steps of 32
constexpr int PW_TARGET_WAVES = 4096;
constexpr int PW_MAX_SPLITS = 2048;

struct PwPlan {
    int tm, tn;                      // 16 x 16 tiles per wave, each in {1, 2, 4}
    int mt, nt;                      // wave tiles along Cout / Cin
    int imgs, hwk;                   // images and pixels per image along K (the 1 x 1-plane form: 1 image of N pixels)
    int cpp;                         // units per image
    long units;                      // imgs * cpp
    int splits;
};

int pw_tiles_per_wave(int tiles) { return tiles >= 3 ? 4 : tiles; }

PwPlan pw_plan(int N, int Cin, int Cout, int HW) {
    PwPlan p{};
    const int tiles_m = (Cout + 15) / 16, tiles_n = (Cin + 15) / 16;
    p.tm = pw_tiles_per_wave(tiles_m);
    p.tn = pw_tiles_per_wave(tiles_n);
    p.mt = (tiles_m + p.tm - 1) / p.tm;
    p.nt = (tiles_n + p.tn - 1) / p.tn;
    p.imgs = HW == 1 ? 1 : N;
    p.hwk = HW == 1 ? N : HW;
    p.cpp = (p.hwk + PW_UNIT - 1) / PW_UNIT;
    p.units = (long)p.imgs * p.cpp;
    const long wave_tiles = (long)p.mt * p.nt;
    // enough waves to fill the chip, at most one per unit, and no more partial bytes than half of what the operands hold
    const long in_bytes = (long)N * HW * ((long)Cin + Cout) * 2, out_bytes = (long)Cout * Cin * 4;
    long s = (PW_TARGET_WAVES + wave_tiles - 1) / wave_tiles;
    if (s > in_bytes / (2 * out_bytes)) s = in_bytes / (2 * out_bytes);
    if (s > p.units) s = p.units;
    if (s > PW_MAX_SPLITS) s = PW_MAX_SPLITS;
    if (s < 1) s = 1;
    p.splits = (int)s;
    return p;
}

struct PwArgs {
    const bf16_raw* x;
    const bf16_raw* dy;
    float* part;                     // [splits][Cout][Cin]
    int Cin, Cout, hwk, cpp, mt, nt, splits;
    long units;
    long x_img, dy_img;              // element strides: image, row (channel), pixel
    long x_row, dy_row;
    long x_pix, dy_pix;
};

// the 16 pixels pl .. pl + 15 of one row as two MFMA fragments (w[0..3], w[4..7]).  Pixels >= hwk must read as zero: the vector
// forms load them from the row's start instead (in bounds) and leave the zeroing to pw_mask16, which runs where the fragments are
// consumed -- a select right behind the load would make the wave wait for it there; the element form masks as it packs.
template <int VEC>
__device__ __forceinline__ void pw_load16(const bf16_raw* __restrict__ row, long pix, int pl, int hwk, unsigned (&w)[8]) {
    if constexpr (VEC == 8) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const uint4 v = *reinterpret_cast<const uint4*>(row + (pl + 8 * g < hwk ? pl + 8 * g : 0));
            w[4 * g] = v.x; w[4 * g + 1] = v.y; w[4 * g + 2] = v.z; w[4 * g + 3] = v.w;
        }
    } else if constexpr (VEC == 4) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint2 v = *reinterpret_cast<const uint2*>(row + (pl + 4 * g < hwk ? pl + 4 * g : 0));
            w[2 * g] = v.x; w[2 * g + 1] = v.y;
        }
    } else {
        unsigned e[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const bool ok = pl + i < hwk;
            const unsigned v = row[ok ? (long)(pl + i) * pix : 0];
            e[i] = ok ? v : 0u;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = e[2 * i] | (e[2 * i + 1] << 16);
    }
}
template <int VEC>
__device__ __forceinline__ void pw_mask16(int pl, int hwk, unsigned (&w)[8]) {
    if constexpr (VEC > 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = pl + (2 * i / VEC) * VEC < hwk ? w[i] : 0u;
    }
}

__device__ __forceinline__ bf16x8 pw_frag(const unsigned* w) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const u4 v = {w[0], w[1], w[2], w[3]};
    return __builtin_bit_cast(bf16x8, v);
}

template <int TM, int TN, int VEC>
__global__ __launch_bounds__(PW_WAVES * 64) void pw_wgrad_kernel(PwArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int wt = blockIdx.x * PW_WAVES + wave;
    if (wt >= a.mt * a.nt) return;                       // (the whole wave: no barrier follows)
    const int wm = wt / a.nt, wn = wt - wm * a.nt;
    const int s = blockIdx.y;
    const long u0 = a.units * s / a.splits, u1 = a.units * (s + 1) / a.splits;

    long aoff[TM], boff[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) aoff[i] = (long)min((wm * TM + i) * 16 + r, a.Cout - 1) * a.dy_row;
#pragma unroll
    for (int j = 0; j < TN; ++j) boff[j] = (long)min((wn * TN + j) * 16 + r, a.Cin - 1) * a.x_row;

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // two register sets: the loads of the next unit are in flight while the MFMAs of this one run
    int n = (int)(u0 / a.cpp), c = (int)(u0 - (long)n * a.cpp);
    unsigned af0[TM][8], bf0[TN][8], af1[TM][8], bf1[TN][8];
    int pl0 = 0, pl1 = 0;                                // first pixel of this lane in the unit each set holds
    auto load = [&](unsigned (&af)[TM][8], unsigned (&bf)[TN][8], int& pl) {      // the unit (n, c); then on to the next one
        pl = c * PW_UNIT + 16 * q;
        const bf16_raw* ap = a.dy + (long)n * a.dy_img;
        const bf16_raw* bp = a.x + (long)n * a.x_img;
#pragma unroll
        for (int i = 0; i < TM; ++i) pw_load16<VEC>(ap + aoff[i], a.dy_pix, pl, a.hwk, af[i]);
#pragma unroll
        for (int j = 0; j < TN; ++j) pw_load16<VEC>(bp + boff[j], a.x_pix, pl, a.hwk, bf[j]);
        if (++c == a.cpp) { c = 0; ++n; }
    };
    auto mma = [&](unsigned (&af)[TM][8], unsigned (&bf)[TN][8], int pl) {
        if (pl + 16 > a.hwk) {                           // (only the last unit of a plane, and only some lanes of it)
#pragma unroll
            for (int i = 0; i < TM; ++i) pw_mask16<VEC>(pl, a.hwk, af[i]);
#pragma unroll
            for (int j = 0; j < TN; ++j) pw_mask16<VEC>(pl, a.hwk, bf[j]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pw_frag(af[i] + 4 * h), pw_frag(bf[j] + 4 * h), acc[i][j],
                                                                        0, 0, 0);
    };
    long u = u0;
    if (u < u1) load(af0, bf0, pl0);
    while (u < u1) {
        const bool more0 = u + 1 < u1;
        if (more0) load(af1, bf1, pl1);
        mma(af0, bf0, pl0);
        if (!more0) break;
        ++u;
        const bool more1 = u + 1 < u1;
        if (more1) load(af0, bf0, pl0);
        mma(af1, bf1, pl1);
        if (!more1) break;
        ++u;
    }

    // acc[i][j][v] = dW[co = 16 (wm TM + i) + 4 q + v][ci = 16 (wn TN + j) + r]
    float* part = a.part + (size_t)s * a.Cout * a.Cin;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int ci = (wn * TN + j) * 16 + r;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int co = (wm * TM + i) * 16 + 4 * q + v;
                if (co < a.Cout && ci < a.Cin) part[(size_t)co * a.Cin + ci] = acc[i][j][v];
            }
        }
}

// dw[e] = bf16(part[0][e] + part[1][e] + ...).  G = 1: one thread per output adds the splits in order.  G = 64 (many splits): 64
// threads per output, thread g adds the splits g, g + 64, ... in order, the 64 sums meet in LDS and are added in the order of g.
// Eight loads are in flight per thread: the sums are short chains of long-latency reads, not bandwidth.
template <int G>
__global__ __launch_bounds__(G == 1 ? 256 : 16 * G) void pw_finalize_kernel(const float* __restrict__ part,
                                                                           bf16_raw* __restrict__ dw, long total, int splits) {
    constexpr int E = G == 1 ? 256 : 16;                 // outputs per workgroup
    const int el = threadIdx.x % E, g = threadIdx.x / E;
    const long e = (long)blockIdx.x * E + el;
    const long ec = e < total ? e : total - 1;
    float sum = 0.f;
    for (int s0 = g; s0 < splits; s0 += 8 * G) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = part[(size_t)min(s0 + i * G, splits - 1) * total + ec];
#pragma unroll
        for (int i = 0; i < 8; ++i) sum += s0 + i * G < splits ? v[i] : 0.f;
    }
    if constexpr (G > 1) {
        __shared__ float sm[G][E];
        sm[g][el] = sum;
        __syncthreads();
        if (g != 0) return;
        sum = sm[0][el];
#pragma unroll
        for (int k = 1; k < G; ++k) sum += sm[k][el];
    }
    if (e < total) dw[e] = f32_to_bf16(sum);
}

template <int TM, int TN>
void pw_launch_tile(const PwArgs& a, int vec, dim3 grid, hipStream_t st) {
    with_vec<8, 8, 4, 1>(vec, [&](auto V) {
        hipLaunchKernelGGL((pw_wgrad_kernel<TM, TN, V>), grid, dim3(PW_WAVES * 64), 0, st, a);
    });
}

}  // namespace

size_t pwconv_workspace_floats(int N, int Cin, int Cout, int HW) {
    return (size_t)pw_plan(N, Cin, Cout, HW).splits * Cout * Cin;
}

hipError_t launch_pw_bwd_weight(const void* x, const void* dy, void* dw, float* ws, int N, int Cin, int Cout, int HW,
                                hipStream_t st) {
    const PwPlan p = pw_plan(N, Cin, Cout, HW);
    PwArgs a{};
    a.x = (const bf16_raw*)x; a.dy = (const bf16_raw*)dy; a.part = ws;
    a.Cin = Cin; a.Cout = Cout; a.hwk = p.hwk; a.cpp = p.cpp; a.mt = p.mt; a.nt = p.nt; a.splits = p.splits; a.units = p.units;
    int vec = 1;
    if (HW == 1) {                   // x [N, Cin], dy [N, Cout]: one image, N pixels a channel count apart
        a.x_img = a.dy_img = 0; a.x_row = a.dy_row = 1; a.x_pix = Cin; a.dy_pix = Cout;
    } else {
        a.x_img = (long)Cin * HW; a.dy_img = (long)Cout * HW; a.x_row = a.dy_row = HW; a.x_pix = a.dy_pix = 1;
        vec = pick_vec(HW, 2, (uintptr_t)x | (uintptr_t)dy, {8, 4});
    }
    const dim3 grid((unsigned)(((long)p.mt * p.nt + PW_WAVES - 1) / PW_WAVES), (unsigned)p.splits);
#define MOMA_PW_ROW(TMV)                                             \
    if (p.tn == 1) pw_launch_tile<TMV, 1>(a, vec, grid, st);         \
    else if (p.tn == 2) pw_launch_tile<TMV, 2>(a, vec, grid, st);    \
    else pw_launch_tile<TMV, 4>(a, vec, grid, st);
    if (p.tm == 1) { MOMA_PW_ROW(1) }
    else if (p.tm == 2) { MOMA_PW_ROW(2) }
    else { MOMA_PW_ROW(4) }
#undef MOMA_PW_ROW
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const long total = (long)Cout * Cin;
    if (p.splits > 32)
        hipLaunchKernelGGL(pw_finalize_kernel<64>, dim3((unsigned)((total + 15) / 16)), dim3(1024), 0, st, ws, (bf16_raw*)dw, total,
                           p.splits);
    else
        hipLaunchKernelGGL(pw_finalize_kernel<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws, (bf16_raw*)dw, total,
                           p.splits);
    return hipGetLastError();
}

}  // namespace moma
