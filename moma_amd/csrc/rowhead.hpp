// What the two heads over a [B, K] logit matrix share (ce.hip: the teacher trainer's cross-entropy head; kdhead.hip: the student's
// CE + KD-divergence head): the shape of the work -- 256 threads, G lanes per row, 16 elements of a row per lane in registers --, the
// (value, index) maximum and the vector width of a launch.  One copy, so the two heads cut a row the same way.
#pragma once
#include "common.hpp"

namespace moma {

constexpr int CE_THREADS = 256;
constexpr int CE_PER_LANE = 16;                     // elements of a row one lane keeps in registers (per operand)
constexpr int CE_ONE_WALK = WAVE * CE_PER_LANE;     // longest row that is read once (MOMA_CE_ONE_WALK_K, MOMA_KDHEAD_ONE_WALK_K)
constexpr long long CE_IGNORE = -100;               // nn.CrossEntropyLoss's ignore_index

// lanes per row: the power of two (1 .. 64) that covers ceil(K / 16)
inline int ce_lanes(int K) {
    int g = 1;
    while (g < WAVE && g * CE_PER_LANE < K) g *= 2;
    return g;
}

// (value, index) of the larger value, the LOWER index among equals; a NaN never wins
__device__ __forceinline__ void ce_take(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// the widths of a launch: 16 bytes (8 bf16 / 4 fp32), 4 elements, else element accesses
template <typename T> int ce_vec(int K, uintptr_t low_bits) { return pick_vec(K, sizeof(T), low_bits, {MAXVEC<T>, 4}); }

}  // namespace moma
