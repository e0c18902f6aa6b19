// Forward and input gradient of a pointwise (1 x 1, stride 1) convolution on NCHW activations as ONE streaming product
//     Y[n, o, p] = sum_k Wm[o, k] * X[n, k, p]                       (x [N, K, HW], y [N, O, HW], bf16; fp32 accumulation)
// forward:        K = Cin,  O = Cout, Wm[o, k] = w[o * Cin + k]     (w [Cout, Cin] as it lies: a B fragment is one 16-byte load)
// input gradient: K = Cout, O = Cin,  Wm[o, k] = w[k * Cin + o]     (the weight read transposed by element loads: it is small and
//                                                                    stays in L2; no activation-sized pass, no workspace)
// K is 16 .. 112 (expand) or 96 .. 672 (project) channels strided by HW, the pixel axis is the contiguous one of x and y, and the
// bf16 MFMA wants K contiguous per lane.  So:
//   * a workgroup (4 waves) owns a tile of PT = 64 or 128 pixels of ONE image (no tile crosses an image) and a block of up to
//     CB = 16 NT WC output channels -- all of O for O <= 256, so x leaves memory once -- and walks K in chunks of 64 channels.
//   * a chunk [64 channels][PT pixels] of x is staged into LDS with 16-byte row loads (8-byte / element loads by pick_vec); the
//     loads of the next chunk are in flight while the MFMAs of this one run.  Rows at and past K are written as zeros (K tails).
//   * v_mfma_f32_16x16x32_bf16 with A = x^T (row = pixel, k = channel) and B = Wm^T (k = channel, column = output channel).  The
//     A fragments are read from the LDS slab with gfx950's transposed read: one instruction hands lane i of a 16-lane group
//     the 4 channels of column i of a 4-row block whose four 8-byte column chunks the lanes address freely.  MFMA row m of tile
//     t (t = 0, 1) is pixel 8 (m >> 2) + 4 t + (m & 3) of a 32-pixel group, so the accumulator rows 4 q .. 4 q + 3 of lane
//     (c, q) = (l & 15, l >> 4) in the two tiles are the 8 CONSECUTIVE pixels 8 q .. 8 q + 7 of output channel c: one 16-byte store.
//     The transposed read needs EXEC all ones and 8-byte-aligned addresses: no lane leaves the kernel early, every branch around
//     it is workgroup-uniform, rows are 2 PT + 64 bytes (the 64-byte pad spreads the 4 rows of a block over the banks; the two
//     blocks of a 32-lane half, 8 rows apart, remain 2-way).
//   * WC waves split the output-channel tiles, 4 / WC waves the 32-pixel groups; the accumulators (NT x PG x 2 tiles) stay in
//     registers over the whole K loop.  Fragments of Wm are (re)loaded per chunk from L2 and masked to zero past K and past O.
// Every global load address is clamped into the operand and the value masked afterwards (loads are never lane-conditional; whole
// staging rows past K are skipped workgroup-uniformly and zero-filled); stores are masked by o < O and pixel < HW.
// No atomics, no workspace, no host synchronisation: bitwise reproducible and safe under graph capture.
#include "common.hpp"

namespace moma {
namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_KC = 64;            // channels per staged chunk: two MFMA steps of 32
constexpr int PS_PAD = 64;           // bytes added to an LDS row

struct PsArgs {
    const bf16_raw* x;
    const bf16_raw* w;
    bf16_raw* y;
    int K, O, HW;
    int tpi, ncb;                    // pixel tiles per image, output-channel blocks
    long tiles;                      // N * tpi
    long w_os, w_ks;                 // element strides of Wm along o and along k
};

typedef __attribute__((address_space(3))) void* ps_lds_ptr;
typedef short ps_s4 __attribute__((ext_vector_type(4)));

// 8 pixels pix .. pix + 7 of one row (pix a multiple of 8) as 4 words.  VEC 8 / 4: raw loads from clamped addresses, masked later
// by ps_mask8 (a select right behind the load would make the wave wait for it there); VEC 1 masks as it packs.
template <int VEC>
__device__ __forceinline__ void ps_load8(const bf16_raw* __restrict__ row, int pix, int hw, bool rowok, unsigned (&v)[4]) {
    if constexpr (VEC == 8) {
        const uint4 a = *reinterpret_cast<const uint4*>(row + (pix < hw ? pix : 0));
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else if constexpr (VEC == 4) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const uint2 a = *reinterpret_cast<const uint2*>(row + (pix + 4 * g < hw ? pix + 4 * g : 0));
            v[2 * g] = a.x; v[2 * g + 1] = a.y;
        }
    } else {
        unsigned e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool ok = rowok && pix + i < hw;
            const unsigned t = row[pix + i < hw ? pix + i : 0];
            e[i] = ok ? t : 0u;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = e[2 * i] | (e[2 * i + 1] << 16);
    }
}
template <int VEC>
__device__ __forceinline__ void ps_mask8(int pix, int hw, bool rowok, unsigned (&v)[4]) {
    if constexpr (VEC > 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (rowok && pix + (2 * i / VEC) * VEC < hw) ? v[i] : 0u;
    }
}

// the B fragment of lane (c, q): Wm[o][k .. k + 7], zero where o >= O or k + j >= K.  WV 8: one 16-byte load (w_ks == 1, K a multiple
// of 8, w 16-byte aligned); WV 1: eight element loads (the transposed weight of the input gradient, odd K)
template <int WV>
__device__ __forceinline__ bf16x8 ps_wfrag(const PsArgs& a, int o, int k) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const bool ook = o < a.O;
    const bf16_raw* row = a.w + (long)(ook ? o : a.O - 1) * a.w_os;
    u4 r;
    if constexpr (WV == 8) {
        const bool ok = ook && k < a.K;
        const uint4 v = *reinterpret_cast<const uint4*>(row + (k < a.K ? k : 0));
        r = u4{ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u};
    } else {
        unsigned e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool kok = k + j < a.K;
            const unsigned t = row[(long)(kok ? k + j : 0) * a.w_ks];
            e[j] = (ook && kok) ? t : 0u;
        }
        r = u4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
    }
    return __builtin_bit_cast(bf16x8, r);
}

// raw words of the B fragment Wm[o][k .. k + 7] by one 16-byte load from a clamped address (WV 8), to be masked by ps_wmask where
// they are consumed: the loads of the next chunk's fragments stay in flight behind this chunk's MFMAs
__device__ __forceinline__ void ps_wload(const PsArgs& a, int o, int k, unsigned (&r)[4]) {
    const uint4 v = *reinterpret_cast<const uint4*>(a.w + (long)min(o, a.O - 1) * a.w_os + (k < a.K ? k : 0));
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
}
__device__ __forceinline__ bf16x8 ps_wmask(const PsArgs& a, int o, int k, const unsigned (&r)[4]) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const bool ok = o < a.O && k < a.K;
    const u4 v = {ok ? r[0] : 0u, ok ? r[1] : 0u, ok ? r[2] : 0u, ok ? r[3] : 0u};
    return __builtin_bit_cast(bf16x8, v);
}

// NT output-channel tiles per wave, WC waves along the output channels (4 / WC along the pixels), PG 32-pixel groups per wave.
// The grid is ncb x (as many workgroups as the chip holds at once): a workgroup walks the pixel tiles pt0, pt0 + stride, ... of its
// channel block, and the (tile, chunk) steps form ONE software pipeline -- the loads of the next step, of the next tile where this
// one ends, are in flight while this step's MFMAs and stores run.  With K <= 64 (the expand layers) the fragments of Wm are loaded
// once and stay in registers over the whole walk.
template <int NT, int WC, int PG, int VEC, int WV>
__global__ __launch_bounds__(PS_THREADS) void pw_stream_kernel(PsArgs a) {
    constexpr int WP = 4 / WC, PT = 32 * WP * PG, CB = 16 * NT * WC;
    constexpr int S = 2 * PT + PS_PAD;                   // bytes per LDS row
    constexpr int OPR = PT / 8;                          // 16-byte octets per row
    constexpr int RPI = PS_THREADS / OPR;                // rows per staging pass
    constexpr int NI = PS_KC / RPI;                      // staging passes per chunk
    __shared__ __attribute__((aligned(16))) unsigned char slab[PS_KC * S];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wc = wave % WC, wp = wave / WC;
    const int cb = (int)(blockIdx.x % (unsigned)a.ncb);
    const long pt0 = blockIdx.x / (unsigned)a.ncb, stride = gridDim.x / (unsigned)a.ncb;

    const int srow = tid / OPR, scol = (tid % OPR) * 8;  // this thread's row of a staging pass and its 8 pixels of the tile
    unsigned char* const sdst = slab + srow * S + scol * 2;

    unsigned xs[NI][4];
    auto stage_load = [&](long pt, int kc) {
        const int n = (int)(pt / a.tpi), spix = (int)(pt - (long)n * a.tpi) * PT + scol;
        const bf16_raw* xin = a.x + (long)n * a.K * a.HW;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (kc + RPI * i < a.K) {                    // (workgroup-uniform)
                const int ch = kc + RPI * i + srow;
                ps_load8<VEC>(xin + (long)min(ch, a.K - 1) * a.HW, spix, a.HW, ch < a.K, xs[i]);
            } else {
                xs[i][0] = xs[i][1] = xs[i][2] = xs[i][3] = 0u;
            }
        }
    };
    auto stage_store = [&](int p0, int kc) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            ps_mask8<VEC>(p0 + scol, a.HW, kc + RPI * i + srow < a.K, xs[i]);
            *reinterpret_cast<uint4*>(sdst + RPI * i * S) = make_uint4(xs[i][0], xs[i][1], xs[i][2], xs[i][3]);
        }
    };

    // transposed read: lane 4 q' + p of group g addresses row 8 g + q' (+ 4 for the second half of the fragment), the 4 pixels
    // 8 p + 4 t .. + 3 of the 32-pixel group; lane i of the group receives pixel 8 (i >> 2) + 4 t + (i & 3) of those 4 rows
    const int c = lane & 15, q = lane >> 4;
    const unsigned char* const rbase = slab + (8 * q + (c >> 2)) * S + 16 * (c & 3) + 64 * (wp * PG);
    const int ocol = cb * CB + 16 * wc + c;              // + 16 WC t: this lane's output channel in tile t

    const bool single = a.K <= PS_KC;                    // one chunk per tile: Wm stays in registers
    constexpr bool WPRE = WV == 8;                       // 16-byte fragments are prefetched raw, element-loaded ones are not
    bf16x8 wf[NT][2];
    unsigned wr[WPRE ? NT : 1][2][4];
    auto w_prefetch = [&](int kc) {
        if constexpr (WPRE) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                ps_wload(a, ocol + 16 * WC * t, kc + 8 * q, wr[t][0]);
                if (a.K - kc > 32) ps_wload(a, ocol + 16 * WC * t, kc + 32 + 8 * q, wr[t][1]);
            }
        }
    };
    auto w_take = [&](int kc) {
        const bool two = a.K - kc > 32;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if constexpr (WPRE) {
                wf[t][0] = ps_wmask(a, ocol + 16 * WC * t, kc + 8 * q, wr[t][0]);
                wf[t][1] = two ? ps_wmask(a, ocol + 16 * WC * t, kc + 32 + 8 * q, wr[t][1]) : wf[t][0];
            } else {
                wf[t][0] = ps_wfrag<WV>(a, ocol + 16 * WC * t, kc + 8 * q);
                wf[t][1] = two ? ps_wfrag<WV>(a, ocol + 16 * WC * t, kc + 32 + 8 * q) : wf[t][0];
            }
        }
    };

    if (pt0 < a.tiles) {
        stage_load(pt0, 0);
        w_prefetch(0);
        if (single) w_take(0);
    }
    for (long pt = pt0; pt < a.tiles; pt += stride) {
        const int n = (int)(pt / a.tpi), p0 = (int)(pt - (long)n * a.tpi) * PT;
        f32x4 acc[NT][PG][2];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < PG; ++i) acc[t][i][0] = acc[t][i][1] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int kc = 0; kc < a.K; kc += PS_KC) {
            const bool two = a.K - kc > 32;              // a second MFMA step in this chunk
            if (!single) w_take(kc);
            stage_store(p0, kc);
            __syncthreads();
            {                                            // the next step of the pipeline: its loads fly behind this step's work
                const bool last = kc + PS_KC >= a.K;
                const long npt = last ? pt + stride : pt;
                const int nkc = last ? 0 : kc + PS_KC;
                if (npt < a.tiles) {
                    stage_load(npt, nkc);
                    if (!single) w_prefetch(nkc);
                }
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (ks == 0 || two) {                    // (workgroup-uniform: EXEC stays all ones)
#pragma unroll
                    for (int i = 0; i < PG; ++i)
#pragma unroll
                        for (int t2 = 0; t2 < 2; ++t2) {
                            const unsigned char* p = rbase + 32 * ks * S + 64 * i + 8 * t2;
                            const ps_s4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ps_s4*)(ps_lds_ptr)p);
                            const ps_s4 hi =
                                __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ps_s4*)(ps_lds_ptr)(p + 4 * S));
                            typedef short s8 __attribute__((ext_vector_type(8)));
                            const s8 f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                            const bf16x8 af = __builtin_bit_cast(bf16x8, f);
#pragma unroll
                            for (int t = 0; t < NT; ++t)
                                acc[t][i][t2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wf[t][ks], acc[t][i][t2], 0, 0, 0);
                        }
                }
            }
            __syncthreads();
        }

        // acc[t][i][t2][v] = y[o = ocol + 16 WC t][pixel p0 + 32 (wp PG + i) + 8 q + 4 t2 + v]
        bf16_raw* yout = a.y + (long)n * a.O * a.HW;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int o = ocol + 16 * WC * t;
#pragma unroll
            for (int i = 0; i < PG; ++i) {
                const int pix = p0 + 32 * (wp * PG + i) + 8 * q;
                const f32x4 lo = acc[t][i][0], hi = acc[t][i][1];
                bf16_raw* dst = yout + (long)min(o, a.O - 1) * a.HW + pix;
                if (o < a.O) {
                    if constexpr (VEC == 8) {
                        if (pix < a.HW)
                            *reinterpret_cast<uint4*>(dst) = make_uint4(pack_bf16x2(lo[0], lo[1]), pack_bf16x2(lo[2], lo[3]),
                                                                         pack_bf16x2(hi[0], hi[1]), pack_bf16x2(hi[2], hi[3]));
                    } else if constexpr (VEC == 4) {
                        if (pix < a.HW) *reinterpret_cast<uint2*>(dst) = make_uint2(pack_bf16x2(lo[0], lo[1]), pack_bf16x2(lo[2], lo[3]));
                        if (pix + 4 < a.HW)
                            *reinterpret_cast<uint2*>(dst + 4) = make_uint2(pack_bf16x2(hi[0], hi[1]), pack_bf16x2(hi[2], hi[3]));
                    } else {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            if (pix + v < a.HW) dst[v] = f32_to_bf16(lo[v]);
                            if (pix + 4 + v < a.HW) dst[4 + v] = f32_to_bf16(hi[v]);
                        }
                    }
                }
            }
        }
    }
}

// compute units of the CURRENT device (a process may drive several); asked once per device
int ps_compute_units() {
    constexpr int MAXDEV = 64;
    static int cached[MAXDEV] = {};                      // 0: not asked yet (benign race: every thread writes the same value)
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev >= 0 && dev < MAXDEV && cached[dev] > 0) return cached[dev];
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    if (dev >= 0 && dev < MAXDEV) cached[dev] = cus;
    return cus;
}

// the grid: ncb x min(tiles, what the chip holds at once / ncb) workgroups.  The occupancy of an instantiation is a property of the
// code object and the architecture (the library is built for gfx950 only), the same on every device of the process; the query is a
// host-side calculation, no stream operation, so a first call inside a graph capture is harmless.  A wrong figure would cost
// balance, never correctness: the walk covers all tiles with any grid.
template <int NT, int WC, int PG>
void ps_launch(const PsArgs& a, int vec, int wv, hipStream_t st) {
    with_vec<8, 8, 4, 1>(vec, [&](auto V) {
        with_vec<8, 8, 1>(wv, [&](auto WVV) {
            auto kernel = pw_stream_kernel<NT, WC, PG, V, WVV>;
            static const int per_cu = [&] {
                int n = 0;
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, PS_THREADS, 0) != hipSuccess) n = 0;
                return n > 0 ? n : 1;
            }();
            long walkers = (long)per_cu * ps_compute_units() / a.ncb;
            if (walkers < 1) walkers = 1;
            if (walkers > a.tiles) walkers = a.tiles;
            hipLaunchKernelGGL(kernel, dim3((unsigned)(walkers * a.ncb)), dim3(PS_THREADS), 0, st, a);
        });
    });
}

}  // namespace

// transposed = 0: y [N, Cout, HW] = w x (the forward); 1: y [N, Cin, HW] = w^T x with x [N, Cout, HW] (the input gradient).
// w is [Cout, Cin] in both.
hipError_t launch_pw_stream(const void* x, const void* w, void* y, int N, int Cin, int Cout, int HW, int transposed, hipStream_t st) {
    PsArgs a{};
    a.x = (const bf16_raw*)x; a.w = (const bf16_raw*)w; a.y = (bf16_raw*)y;
    a.K = transposed ? Cout : Cin;
    a.O = transposed ? Cin : Cout;
    a.HW = HW;
    a.w_os = transposed ? 1 : Cin;
    a.w_ks = transposed ? Cin : 1;
    // (NT, WC, PG) by the number of output channels: pixel tile 128 with the waves along the pixels for few channels, 64 pixels and
    // the waves along the channels for many.  Above 256 channels: blocks of 256 whose workgroups are neighbours in the grid (the
    // later ones find the x tile in L2); 8 tiles per wave would cover 512 at one wave per SIMD, too few to hide the loads
    int nt, wc, pg;
    if (a.O <= 16) { nt = 1; wc = 1; pg = 1; }
    else if (a.O <= 32) { nt = 2; wc = 1; pg = 1; }
    else if (a.O <= 64) { nt = 4; wc = 1; pg = 1; }
    else if (a.O <= 128) { nt = 4; wc = 2; pg = 1; }
    else { nt = 4; wc = 4; pg = 2; }
    const int ptile = 32 * (4 / wc) * pg, cblock = 16 * nt * wc;
    a.tpi = (HW + ptile - 1) / ptile;
    a.ncb = (a.O + cblock - 1) / cblock;
    a.tiles = (long)N * a.tpi;
    const int vec = pick_vec(HW, 2, (uintptr_t)x | (uintptr_t)y, {8, 4});
    const int wv = transposed ? 1 : pick_vec(Cin, 2, (uintptr_t)w, {8});
    if (nt == 1) ps_launch<1, 1, 1>(a, vec, wv, st);
    else if (nt == 2) ps_launch<2, 1, 1>(a, vec, wv, st);
    else if (nt == 4 && wc == 1) ps_launch<4, 1, 1>(a, vec, wv, st);
    else if (nt == 4 && wc == 2) ps_launch<4, 2, 1>(a, vec, wv, st);
    else ps_launch<4, 4, 2>(a, vec, wv, st);
    return hipGetLastError();
}

}  // namespace moma
