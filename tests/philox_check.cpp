// Host check of csrc/philox.h: includes nothing of the project but that header (which needs no HIP), prints the three
// known-answer vectors of Philox4x32-10 and the mask words of a few (a, b, k, s, draw, seed) tuples; tests/test_mc_dropout_cpu.py
// compares both with its own numpy statement.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>

#include "../relpose-gnn_amd/csrc/philox.h"

int main() {
    struct Kat { uint32_t c[4], k[2]; };
    const Kat kats[3] = {{{0u, 0u, 0u, 0u}, {0u, 0u}},
                         {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}},
                         {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}}};
    for (const Kat& t : kats) {
        const rpg::Philox4 r = rpg::philox4x32_10(t.c[0], t.c[1], t.c[2], t.c[3], t.k[0], t.k[1]);
        printf("kat %08x %08x %08x %08x\n", r.w[0], r.w[1], r.w[2], r.w[3]);
    }
    struct Tup { uint32_t a, b, k, s, draw; uint64_t seed; };
    const Tup tups[] = {{0u, rpg::kMcNodeTag, 0u, 0u, 0u, 0ull},
                        {5u, rpg::kMcNodeTag, 511u, 15u, 3u, 1234ull},
                        {7u, 3u, 1u, 1u, 0u, 0ull},
                        {3u, 7u, 1u, 1u, 0u, 0ull},
                        {0x7fffffffu, 0x7ffffffeu, 65535u, 1023u, 0xffffffffu, 0xfedcba9876543210ull},
                        {1000000u, rpg::kMcNodeTag, 17u, 0u, 42u, 0x100000000ull}};
    for (const Tup& t : tups) {
        const rpg::Philox4 r = rpg::mc_mask_words((uint32_t)t.seed, (uint32_t)(t.seed >> 32), t.draw, t.a, t.b, t.k, t.s);
        printf("mask %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu64 " : %08x %08x %08x %08x\n", t.a, t.b, t.k, t.s,
               t.draw, t.seed, r.w[0], r.w[1], r.w[2], r.w[3]);
    }
    printf("philox: ok\n");
    return 0;
}
