// The tuning keys (RPG_TUNE_*, rpg_set_tuning / rpg_get_tuning): every key's default, accepted values and decoding, stated once,
// and the process-wide state the launchers read.  What each key's values MEAN is documented at its #define in the C header; this
// table is how a raw value becomes the fields below.  Host-only: nothing of HIP is needed, so tests/tuning_check.cpp compiles it
// with a plain host compiler.
#pragma once
#include "../../include/relpose_gnn_hip.h"

namespace rpg {

// The decoded fields, as the launchers read them (plain loads; a key is set between launches, by the thread that launches).
struct Tuning {
    struct Gemm {              // gemm_f32.hip / gemm_engine.inc
        int force_tile;        // -1 = automatic, else a TileShape
        int bk;                // 0 = automatic: 32 for the 128-row tiles on K >= 256, else 16
        int epi_lds, streamk;
        int fast;              // buffer-load loaders + interleaved main loop where eligible
        int waves8;            // 8-wave workgroups for the 128-row tiles where the fast path applies
        int sk_min_its;        // at least this many k-steps per stream-K workgroup
        int fold_k;            // two-level accumulation of the Linears (gemm_engine.inc), 0 = one sequential chain
        int lin112;            // bit 0 the exact-fit kernel, bit 1 its eight-wave form for launches of about one tile per CU
        int inkernel_fixup;    // bit 0: stream-K, bit 1: Winograd: partial tiles combined by the last-arriving workgroup
        int fixup_prio;        // fix-up launches on the high-priority companion stream
    } gemm;
    struct Gnn {               // forward.hip
        int split, fuse_agg;
        int mean_first;        // fused aggregation only: mlp.2 runs on the node means of the hidden rows, not per edge
    } gnn;
    struct Wino {              // winograd.hip
        int on;                // 0 off | 1 auto | 2 / 3: always the 4-wave / 8-wave kernel
        int min_blocks;        // auto: Winograd from this many blocks of 64 tiles x 64 channels up
        int split;             // split-K tail of the 8-wave kernel
        int split_steps;       // ... and the least number of K steps a part of a tile gets in the one-workgroup-per-tile form
        int persist;           // the persistent 8-wave kernel when a launch has more tiles than CUs (2: always)
        int combine_max;       // most parts of a tail tile that its last-arriving workgroup adds up itself
        int wino2d;            // probe builds (tools/probes/winograd2d.hip): 0 off | 1 by shape | 2 wherever eligible
    } wino;
    struct Bf16 {              // conv_bf16.hip, block_bf16.inc, stem_bf16.hip
        int bk, fast, tile, dma, linear_dma, lean_epi, pair, persist, tail;
        int patch, stages;     // the patch kernel: 0 off | 1 by shape | 2.. wherever eligible; its weight stages (3 = never the prefetching form)
        int chunk, chunk_mb;   // images per depth-first group (0 = off), for activation tensors of at least this many MB
        int fuse_block;        // 64-channel identity BasicBlocks as one kernel (bit 1: persistent, bit 2: two-group schedule)
        int ws64;              // probe builds (tools/probes/conv3x3_bf16_ws64.inc): 0 off | 1: 384-pixel tiles | 2: 256
        int fused_stem;
        int stem_strip;        // 0: the tile kernel | bit 0: the strip-march kernel, + bit 3: both 32-channel halves in one wave
        int stem_strip_bh;     // pooled rows per band; 0 = by the launch's size
    } bf16;
    struct Stem {              // stem.hip (fp32)
        int fused;
        int strip, strip_bh;   // the strip-march kernel and its pooled rows per band (0: by the launch's size)
    } stem;
};

struct TuningRow {
    int key;
    const char* name;                 // the header's name without RPG_TUNE_
    int def;                          // raw default
    bool (*valid)(int);               // which raw values rpg_set_tuning accepts
    void (*decode)(Tuning&, int);     // writes the fields a (valid) raw value stands for
};

constexpr int kTuningKeys = 32;

#define RPG_TUNING_ROW(NAME, def, valid, decode) \
    {RPG_TUNE_##NAME, #NAME, def, [](int v) -> bool { (void)v; return valid; }, [](Tuning& t, int v) { (void)t; (void)v; decode; }}

// One row per key, in key order.
inline constexpr TuningRow kTuningRows[kTuningKeys] = {
    RPG_TUNING_ROW(TILE, -1, true, t.gemm.force_tile = v),
    RPG_TUNING_ROW(BK, 0, v == 0 || v == 16 || v == 32, t.gemm.bk = v),
    RPG_TUNING_ROW(EPILOGUE, 1, true, t.gemm.epi_lds = v != 0),
    RPG_TUNING_ROW(STREAMK, 1, true, t.gemm.streamk = v != 0),
    RPG_TUNING_ROW(WINOGRAD, 1, v >= 0 && !(v > 3 && v < 16),      // n >= 16: auto with the min-blocks rule
                   if (v >= 16) { t.wino.on = 1; t.wino.min_blocks = v; } else { t.wino.on = v; t.wino.min_blocks = 16; }),
    RPG_TUNING_ROW(GNN_SPLIT, 1, true, t.gnn.split = v != 0),
    RPG_TUNING_ROW(BF16_BK, 32, v == 32 || v == 64, t.bf16.bk = v),
    RPG_TUNING_ROW(FAST_LOADER, 1, true, t.gemm.fast = v != 0),
    RPG_TUNING_ROW(WINO_SPLIT, 1, v >= 0 && v <= 96,               // n >= 2: on, with n as the step count
                   t.wino.split = v != 0; t.wino.split_steps = v >= 2 ? v : 3),
    RPG_TUNING_ROW(BF16_FAST, 1, true, t.bf16.fast = v != 0),
    RPG_TUNING_ROW(FUSED_STEM, 1, true,                            // bit 0: both stems; bits 1, 5: bf16 kernel; bit 7: fp32 strips; >> 8: band rows
                   t.stem.fused = (v & 1) != 0; t.stem.strip = (v & 128) != 0; t.stem.strip_bh = (v >> 8) > 0 ? (v >> 8) : 0;
                   t.bf16.fused_stem = (v & 1) != 0; t.bf16.stem_strip = (v & 2) ? 0 : ((v & 32) ? 1 : 9);
                   t.bf16.stem_strip_bh = (v >> 8) > 0 ? (v >> 8) : 0),
    RPG_TUNING_ROW(WAVES8, 1, true, t.gemm.waves8 = v != 0),
    RPG_TUNING_ROW(WINO_SHORT, 0, v >= 0, ),                       // retired with the short-K kernel: accepted, ignored
    RPG_TUNING_ROW(GNN_FUSE_AGG, 1, true,                          // 2: fused, but mlp.2 still per edge (the form before mean-first)
                   t.gnn.fuse_agg = v != 0; t.gnn.mean_first = v != 0 && v != 2),
    RPG_TUNING_ROW(WINO_PERSIST, 1, v >= 0 && v <= 2, t.wino.persist = v),
    RPG_TUNING_ROW(BF16_TILE, -1, v >= -1 && v <= 3, t.bf16.tile = v),
    RPG_TUNING_ROW(BF16_DMA, 1, v >= 0 && v <= 40, t.bf16.dma = v),
    RPG_TUNING_ROW(BF16_PATCH, 1, v >= 0 && v % 10 <= 4 && v <= 14,      // + 10: three weight stages
                   t.bf16.stages = v >= 10 ? 3 : 4; t.bf16.patch = v % 10),
#ifdef RPG_PROBE_WS64
    RPG_TUNING_ROW(BF16_WS64, 0, v >= 0 && v <= 2, t.bf16.ws64 = v),
#else
    RPG_TUNING_ROW(BF16_WS64, 0, v == 0, t.bf16.ws64 = v),         // the probe kernel is not in this build
#endif
    RPG_TUNING_ROW(SK_MIN_ITS, 8, v >= 1 && v <= 4096, t.gemm.sk_min_its = v),
    RPG_TUNING_ROW(INKERNEL_FIXUP, 0, v >= 0 && v <= 7,            // + 4: the Winograd combine takes up to 32 parts
                   t.gemm.inkernel_fixup = v & 3; t.wino.combine_max = (v & 4) ? 32 : 8),
    RPG_TUNING_ROW(BF16_CHUNK, 0, v >= 0,                          // images | MB << 12 (0 MB = 64)
                   t.bf16.chunk = v & 4095; t.bf16.chunk_mb = (v >> 12) ? (v >> 12) : 64),
#ifdef RPG_PROBE_WINO2D
    RPG_TUNING_ROW(WINO2D, 0, v >= 0 && v <= 2, t.wino.wino2d = v),
#else
    RPG_TUNING_ROW(WINO2D, 0, v == 0, t.wino.wino2d = v),          // the probe kernel is not in this build
#endif
    RPG_TUNING_ROW(BF16_LEAN_EPI, 1, true, t.bf16.lean_epi = v != 0),
    RPG_TUNING_ROW(BF16_LINEAR_DMA, 0, v == 0 || (v >= 10 && v <= 19), t.bf16.linear_dma = v),
    RPG_TUNING_ROW(BF16_PERSIST, 0, true, t.bf16.persist = v != 0),
    RPG_TUNING_ROW(FOLD_K, 256, v >= 0 && v % 64 == 0, t.gemm.fold_k = v),
    RPG_TUNING_ROW(BF16_FUSE_BLOCK, 3, true, t.bf16.fuse_block = v & 7),
    RPG_TUNING_ROW(BF16_TAIL, 1, v >= 0 && v <= 7, t.bf16.tail = v & 7),
    RPG_TUNING_ROW(LIN112, 3, v >= 0 && v <= 3, t.gemm.lin112 = v),
    RPG_TUNING_ROW(FIXUP_PRIO, 0, true, t.gemm.fixup_prio = v != 0),
    RPG_TUNING_ROW(BF16_PAIR, 1, true, t.bf16.pair = v != 0),
};
#undef RPG_TUNING_ROW

constexpr bool tuning_rows_in_key_order() {
    for (int k = 0; k < kTuningKeys; ++k)
        if (kTuningRows[k].key != k) return false;
    return true;
}
static_assert(tuning_rows_in_key_order(), "kTuningRows[k] must be the row of key k");

// The raw value of every key as last accepted, and what those values decode to.
struct TuningState {
    int raw[kTuningKeys];
    Tuning decoded;
};

// The state before any set: every default, decoded.
constexpr TuningState default_tuning_state() {
    TuningState s{};
    for (int k = 0; k < kTuningKeys; ++k) {
        s.raw[k] = kTuningRows[k].def;
        kTuningRows[k].decode(s.decoded, s.raw[k]);
    }
    return s;
}

inline TuningState g_tuning_state = default_tuning_state();      // constant-initialised

inline const Tuning& tuning() { return g_tuning_state.decoded; }

inline const TuningRow* tuning_row(int key) { return key >= 0 && key < kTuningKeys ? &kTuningRows[key] : nullptr; }

inline int set_tuning(int key, int value) {
    const TuningRow* row = tuning_row(key);
    if (!row || !row->valid(value)) return RPG_ERR_BAD_ARG;
    g_tuning_state.raw[key] = value;
    row->decode(g_tuning_state.decoded, value);
    return RPG_OK;
}

inline int get_tuning(int key, int* value, int* default_value) {
    const TuningRow* row = tuning_row(key);
    if (!row) return RPG_ERR_BAD_ARG;
    if (value) *value = g_tuning_state.raw[key];
    if (default_value) *default_value = row->def;
    return RPG_OK;
}

}  // namespace rpg
