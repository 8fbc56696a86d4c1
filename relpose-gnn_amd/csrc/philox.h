// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) with the standard constants,
// and the counter layout of the Monte-Carlo pose heads (mc_heads.hip).  Plain C++ that the host compiler takes as it is
// (tests/philox_check.cpp) and hipcc compiles for the device: the host and the kernel run the same text.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RPG_HD __host__ __device__ __forceinline__
#else
#define RPG_HD inline
#endif

namespace rpg {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;      // multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;      // Weyl increments of the key

struct Philox4 {
    uint32_t w[4];
};

// Ten rounds; the key is bumped between rounds (nine times).
RPG_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// The node tag: the second id of a NODE row (an edge row carries its target's id there).
constexpr uint32_t kMcNodeTag = 0xFFFFFFFFu;

// The dropout mask of the Monte-Carlo heads is a pure function of (seed, draw, ids, column, sample): the four words serve the
// four elements of float4 column chunk k (columns 4k .. 4k+3) of one row for sample s; element j is KEPT iff w[j] >= T with
// T = floor(p 2^32).  key = (seed_lo, seed_hi); counter = (a, b, k | s << 16, draw).  A node row has a = its global node id and
// b = kMcNodeTag; an edge row has a = the global id of its source and b = that of its target.  Global node id = node_base + the
// node's row in the call's node list.  Limits: k < 65536, s < 65536 (the launcher takes S <= 1024), ids below 2^31 (so no edge's
// target id is the node tag); draw is 32 bits and wraps.
//
// What follows from that: a row's masks do not depend on its position in the call, on the stream slot or micro-batch that
// computes it, on the order of the edge list, on whether the graph is fully connected or a kNN graph, or on the output mode
// ("query" or "all") -- and two copies of the same (source, target) edge share their masks.
RPG_HD Philox4 mc_mask_words(uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, uint32_t a, uint32_t b, uint32_t k, uint32_t s) {
    return philox4x32_10(a, b, k | (s << 16), draw, seed_lo, seed_hi);
}

}  // namespace rpg
