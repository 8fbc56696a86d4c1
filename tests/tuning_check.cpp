// Stand-alone host check of csrc/tuning.h (built and run by tests/test_host.py; no GPU, no HIP).
// (a) every key's raw default against the list below, which restates the initialisers the launchers' globals carried before the
//     table existed (it is NOT read from the table);  (b) the state those defaults decode to, field by field;  (c) the keys that
//     pack several values into one int, decoded at chosen values as the former switch of rpg_set_tuning and its setters did.
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "../relpose-gnn_amd/csrc/tuning.h"

namespace {

int g_failures = 0;
#define EXPECT(cond, ...)                                            \
    do {                                                             \
        if (!(cond)) {                                               \
            ++g_failures;                                            \
            fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                            \
            fprintf(stderr, "\n");                                   \
        }                                                            \
    } while (0)

struct Default { const char* name; int key, value; };
const Default kDefaults[] = {
    {"TILE", 0, -1}, {"BK", 1, 0}, {"EPILOGUE", 2, 1}, {"STREAMK", 3, 1}, {"WINOGRAD", 4, 1}, {"GNN_SPLIT", 5, 1}, {"BF16_BK", 6, 32},
    {"FAST_LOADER", 7, 1}, {"WINO_SPLIT", 8, 1}, {"BF16_FAST", 9, 1}, {"FUSED_STEM", 10, 1}, {"WAVES8", 11, 1}, {"WINO_SHORT", 12, 0},
    {"GNN_FUSE_AGG", 13, 1}, {"WINO_PERSIST", 14, 1}, {"BF16_TILE", 15, -1}, {"BF16_DMA", 16, 1}, {"BF16_PATCH", 17, 1},
    {"BF16_WS64", 18, 0}, {"SK_MIN_ITS", 19, 8}, {"INKERNEL_FIXUP", 20, 0}, {"BF16_CHUNK", 21, 0}, {"WINO2D", 22, 0},
    {"BF16_LEAN_EPI", 23, 1}, {"BF16_LINEAR_DMA", 24, 0}, {"BF16_PERSIST", 25, 0}, {"FOLD_K", 26, 256}, {"BF16_FUSE_BLOCK", 27, 3},
    {"BF16_TAIL", 28, 1}, {"LIN112", 29, 3}, {"FIXUP_PRIO", 30, 0}, {"BF16_PAIR", 31, 1},
};
constexpr int kKeys = (int)(sizeof(kDefaults) / sizeof(kDefaults[0]));

// every field of the default state, as the globals' initialisers had it
void expect_default_state(const char* when) {
    const rpg::Tuning& t = rpg::tuning();
    EXPECT(t.gemm.force_tile == -1 && t.gemm.bk == 0 && t.gemm.epi_lds == 1 && t.gemm.streamk == 1 && t.gemm.fast == 1 && t.gemm.waves8 == 1,
           "%s", when);
    EXPECT(t.gemm.sk_min_its == 8 && t.gemm.fold_k == 256 && t.gemm.lin112 == 3 && t.gemm.inkernel_fixup == 0 && t.gemm.fixup_prio == 0, "%s", when);
    EXPECT(t.gnn.split == 1 && t.gnn.fuse_agg == 1, "%s", when);
    EXPECT(t.wino.on == 1 && t.wino.min_blocks == 16 && t.wino.split == 1 && t.wino.split_steps == 3 && t.wino.persist == 1 &&
           t.wino.combine_max == 8 && t.wino.wino2d == 0, "%s", when);
    EXPECT(t.bf16.bk == 32 && t.bf16.fast == 1 && t.bf16.tile == -1 && t.bf16.dma == 1 && t.bf16.linear_dma == 0 && t.bf16.lean_epi == 1 &&
           t.bf16.pair == 1 && t.bf16.persist == 0 && t.bf16.tail == 1, "%s", when);
    EXPECT(t.bf16.patch == 1 && t.bf16.stages == 4 && t.bf16.chunk == 0 && t.bf16.chunk_mb == 64 && t.bf16.fuse_block == 3 && t.bf16.ws64 == 0,
           "%s", when);
    EXPECT(t.bf16.fused_stem == 1 && t.bf16.stem_strip == 9 && t.bf16.stem_strip_bh == 0, "%s", when);
    EXPECT(t.stem.fused == 1 && t.stem.strip == 0 && t.stem.strip_bh == 0, "%s", when);
}

void reset() {
    for (int k = 0; k < kKeys; ++k) EXPECT(rpg::set_tuning(k, kDefaults[k].value) == RPG_OK, "%s", kDefaults[k].name);
}

const rpg::Tuning& set(int key, int value) {
    EXPECT(rpg::set_tuning(key, value) == RPG_OK, "key %d value %d", key, value);
    int raw = INT_MIN;
    EXPECT(rpg::get_tuning(key, &raw, nullptr) == RPG_OK && raw == value, "key %d value %d reads back %d", key, value, raw);
    return rpg::tuning();
}

void check_defaults() {
    EXPECT(rpg::kTuningKeys == kKeys, "%d rows, %d keys", rpg::kTuningKeys, kKeys);
    for (int k = 0; k < kKeys; ++k) {
        const rpg::TuningRow* row = rpg::tuning_row(k);
        EXPECT(row && row->key == kDefaults[k].key && k == kDefaults[k].key, "row %d", k);
        if (!row) continue;
        EXPECT(strcmp(row->name, kDefaults[k].name) == 0, "row %d is %s, not %s", k, row->name, kDefaults[k].name);
        EXPECT(row->def == kDefaults[k].value, "%s: default %d, not %d", row->name, row->def, kDefaults[k].value);
        EXPECT(row->valid(row->def), "%s refuses its default", row->name);
        int raw = INT_MIN, def = INT_MIN;
        EXPECT(rpg::get_tuning(k, &raw, &def) == RPG_OK && raw == kDefaults[k].value && def == kDefaults[k].value, "%s: %d / %d", row->name, raw, def);
        EXPECT(rpg::get_tuning(k, nullptr, nullptr) == RPG_OK, "%s", row->name);
    }
    for (int bad : {-1, kKeys, 12345, INT_MIN, INT_MAX}) {
        EXPECT(!rpg::tuning_row(bad) && rpg::set_tuning(bad, 0) == RPG_ERR_BAD_ARG && rpg::get_tuning(bad, nullptr, nullptr) == RPG_ERR_BAD_ARG,
               "key %d", bad);
    }
    expect_default_state("before any set");
}

void check_packed_keys() {
    // FUSED_STEM: bit 0 both stems; bf16: bit 1 the tile kernel (mode 0), bit 5 one half per wave (mode 1), else mode 9; fp32: bit 7 strips;
    // value >> 8 the band rows of both
    struct Stem { int value, fused, strip, bh, bf16_mode; };
    for (const Stem& c : {Stem{0, 0, 0, 0, 9}, Stem{1, 1, 0, 0, 9}, Stem{2, 0, 0, 0, 0}, Stem{3, 1, 0, 0, 0}, Stem{33, 1, 0, 0, 1},
                          Stem{129, 1, 1, 0, 9}, Stem{129 | (5 << 8), 1, 1, 5, 9}}) {
        const rpg::Tuning& t = set(RPG_TUNE_FUSED_STEM, c.value);
        EXPECT(t.stem.fused == c.fused && t.stem.strip == c.strip && t.stem.strip_bh == c.bh, "FUSED_STEM %d (fp32)", c.value);
        EXPECT(t.bf16.fused_stem == c.fused && t.bf16.stem_strip == c.bf16_mode && t.bf16.stem_strip_bh == c.bh, "FUSED_STEM %d (bf16)", c.value);
    }
    // WINOGRAD: below 16 the mode; from 16 up automatic with that many blocks as the least
    struct Wino { int value, on, min_blocks; };
    for (const Wino& c : {Wino{0, 0, 16}, Wino{2, 2, 16}, Wino{3, 3, 16}, Wino{16, 1, 16}, Wino{40, 1, 40}, Wino{1, 1, 16}}) {
        const rpg::Tuning& t = set(RPG_TUNE_WINOGRAD, c.value);
        EXPECT(t.wino.on == c.on && t.wino.min_blocks == c.min_blocks, "WINOGRAD %d", c.value);
    }
    // WINO_SPLIT: from 2 up, on with that step count
    struct Split { int value, split, steps; };
    for (const Split& c : {Split{0, 0, 3}, Split{1, 1, 3}, Split{2, 1, 2}, Split{96, 1, 96}}) {
        const rpg::Tuning& t = set(RPG_TUNE_WINO_SPLIT, c.value);
        EXPECT(t.wino.split == c.split && t.wino.split_steps == c.steps, "WINO_SPLIT %d", c.value);
    }
    // BF16_PATCH: + 10 = three weight stages
    struct Patch { int value, patch, stages; };
    for (const Patch& c : {Patch{0, 0, 4}, Patch{2, 2, 4}, Patch{4, 4, 4}, Patch{10, 0, 3}, Patch{14, 4, 3}}) {
        const rpg::Tuning& t = set(RPG_TUNE_BF16_PATCH, c.value);
        EXPECT(t.bf16.patch == c.patch && t.bf16.stages == c.stages, "BF16_PATCH %d", c.value);
    }
    // BF16_CHUNK: images | MB << 12, 0 MB = 64
    struct Chunk { int value, images, mb; };
    for (const Chunk& c : {Chunk{8, 8, 64}, Chunk{8 | (128 << 12), 8, 128}, Chunk{4095, 4095, 64}, Chunk{1 << 12, 0, 1}}) {
        const rpg::Tuning& t = set(RPG_TUNE_BF16_CHUNK, c.value);
        EXPECT(t.bf16.chunk == c.images && t.bf16.chunk_mb == c.mb, "BF16_CHUNK %d", c.value);
    }
    // INKERNEL_FIXUP: bits 0-1 who combines in the kernel, bit 2 the Winograd combine limit
    for (int v = 0; v <= 7; ++v) {
        const rpg::Tuning& t = set(RPG_TUNE_INKERNEL_FIXUP, v);
        EXPECT(t.gemm.inkernel_fixup == (v & 3) && t.wino.combine_max == (v >= 4 ? 32 : 8), "INKERNEL_FIXUP %d", v);
    }
    // masked: BF16_FUSE_BLOCK takes any int and keeps three bits; the raw value reads back as passed (set() checks)
    EXPECT(set(RPG_TUNE_BF16_FUSE_BLOCK, 11).bf16.fuse_block == 3, "BF16_FUSE_BLOCK 11");
    EXPECT(set(RPG_TUNE_BF16_FUSE_BLOCK, 5).bf16.fuse_block == 5, "BF16_FUSE_BLOCK 5");
    EXPECT(set(RPG_TUNE_BF16_TAIL, 6).bf16.tail == 6, "BF16_TAIL 6");
    EXPECT(rpg::set_tuning(RPG_TUNE_BF16_TAIL, 8) == RPG_ERR_BAD_ARG && rpg::tuning().bf16.tail == 6, "BF16_TAIL 8 is refused and changes nothing");
    // flags keep 0 / 1 whatever was passed
    EXPECT(set(RPG_TUNE_FIXUP_PRIO, 7).gemm.fixup_prio == 1 && set(RPG_TUNE_BF16_PERSIST, -2).bf16.persist == 1, "flags");
    // WINO_SHORT: accepted from 0 up, decodes to nothing
    EXPECT(rpg::set_tuning(RPG_TUNE_WINO_SHORT, 64) == RPG_OK && rpg::set_tuning(RPG_TUNE_WINO_SHORT, -1) == RPG_ERR_BAD_ARG, "WINO_SHORT");
    // the probe-only keys: a build without the probe kernels accepts 0 only
#ifndef RPG_PROBE_WS64
    EXPECT(rpg::set_tuning(RPG_TUNE_BF16_WS64, 1) == RPG_ERR_BAD_ARG && rpg::set_tuning(RPG_TUNE_BF16_WS64, 0) == RPG_OK, "BF16_WS64");
#endif
#ifndef RPG_PROBE_WINO2D
    EXPECT(rpg::set_tuning(RPG_TUNE_WINO2D, 1) == RPG_ERR_BAD_ARG && rpg::set_tuning(RPG_TUNE_WINO2D, 0) == RPG_OK, "WINO2D");
#endif
    reset();
    expect_default_state("after setting every key back to its default");
}

}  // namespace

int main() {
    check_defaults();
    check_packed_keys();
    if (g_failures) {
        fprintf(stderr, "tuning: %d failure(s)\n", g_failures);
        return 1;
    }
    printf("tuning: ok (%d keys)\n", kKeys);
    return 0;
}
