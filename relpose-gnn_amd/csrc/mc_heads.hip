// Monte-Carlo pose heads for gfx950: S evaluations of the 6-wide heads under S dropout masks, from ONE read of every feature row.
//
// Reference ops replaced (python/niantic/modules/posenet.py:1073-1086): F.dropout without `training=` (always
// on, so with the default --droprate 0.5 every pose is one sample of a random estimator) followed by fc_xyz / fc_wpqr on the
// node features and fc_xyz_R / fc_wpqr_R on the edge features.  Here the S samples, their mean and their unbiased variance
// come out of one launch; the masks are Philox4x32-10 words keyed by (seed, draw, node ids, column, sample) (philox.h), so a
// row's result does not depend on where in which call it is computed.
//
// Shape of the kernel.  One wave per row, as rpg_pose_heads_f32 (gnn_ops.hip): lane l owns the float4 column chunks l, l + 64,
// ...  A tile of 64 * MC_CH chunks of the row is loaded into registers ONCE (d <= 2048 is one tile; a longer row takes one tile
// after the other, each read once) and stays there for all S samples.  Samples go in blocks of MC_SB: per chunk the six weight
// float4s are fetched once per block (L1 / L2 hits after the chip's first rows: 24 d bytes in all, never HBM per sample) and
// feed MC_SB masked accumulations, each of which costs one Philox call (ten rounds of two 32 x 32 -> 64 multiplies) and
// 4 selects + 24 FMAs.  The butterfly reduction of the block's 6 MC_SB sums follows -- once per block and tile, not per chunk --
// and lanes 0..5 put the sums into the row's LDS slab [S][6].  Lanes 0..5 then walk the slab in sample order: scale, bias, the
// sequential sum for the mean, and a second pass for the variance.  No atomics, no workgroup barrier (a wave only ever touches
// the slab of its own row; LDS operations of one wave execute in order).  A row's arithmetic is the same wherever it runs: the
// lane -> chunk map, the block and tile order and the butterfly depend on (d, S) alone.
// Measured (profiles/mc_heads_bench.json): the kernel is bound by the integer VALU work of the Philox rounds, not by memory.
#include "rpg_common.h"
#include "philox.h"

namespace {

constexpr int MC_CH = 8;        // float4 chunks per lane held in registers: one tile = 512 chunks = 2048 columns
constexpr int MC_SB = 4;        // samples per block
constexpr int MC_MAX_S = 1024;
constexpr int MC_SLAB_S = 256;  // up to this many samples four rows share a workgroup (24 KB of LDS); above it one row each

struct McArgs {
    const float4* x;
    const float4* w6;
    const float* b6;
    int R, d4, S;
    uint32_t thr;               // keep iff word >= thr
    float scale;
    uint32_t seed_lo, seed_hi;
    const uint32_t* state;      // {draw, node_base}
    const int64_t* id_a;
    const int64_t* id_b;
    int64_t id_offset;
    float* mean;
    float* var;
    float* samples;
};

// SB samples s0 .. s0 + SB - 1 over the register tile xv (chunks tile0 + c * 64 + lane): their six sums, reduced over the wave.
template <int SB>
__device__ __forceinline__ void mc_block(const McArgs& g, const float4 (&xv)[MC_CH], int tile0, int lane, int s0, uint32_t a,
                                         uint32_t b, uint32_t draw, float* ys, bool first_tile) {
    float acc[SB][6];
#pragma unroll
    for (int j = 0; j < SB; ++j)
#pragma unroll
        for (int o = 0; o < 6; ++o) acc[j][o] = 0.f;
#pragma unroll
    for (int c = 0; c < MC_CH; ++c) {
        const int k = tile0 + c * 64 + lane;
        if (tile0 + c * 64 >= g.d4) break;                    // wave-uniform: the tile's chunks past the row's end
        if (k < g.d4) {
            float4 wv[6];
#pragma unroll
            for (int o = 0; o < 6; ++o) wv[o] = g.w6[(size_t)o * g.d4 + k];
#pragma unroll
            for (int j = 0; j < SB; ++j) {
                const rpg::Philox4 m = rpg::mc_mask_words(g.seed_lo, g.seed_hi, draw, a, b, (uint32_t)k, (uint32_t)(s0 + j));
                // the mask SELECTS: a dropped feature is replaced by +0 before the products (F.dropout multiplies by 0 instead,
                // which turns a dropped Inf / NaN into NaN)
                const float x0 = m.w[0] >= g.thr ? xv[c].x : 0.f, x1 = m.w[1] >= g.thr ? xv[c].y : 0.f;
                const float x2 = m.w[2] >= g.thr ? xv[c].z : 0.f, x3 = m.w[3] >= g.thr ? xv[c].w : 0.f;
#pragma unroll
                for (int o = 0; o < 6; ++o)
                    acc[j][o] = __fmaf_rn(x3, wv[o].w, __fmaf_rn(x2, wv[o].z, __fmaf_rn(x1, wv[o].y, __fmaf_rn(x0, wv[o].x, acc[j][o]))));
            }
        }
    }
#pragma unroll
    for (int j = 0; j < SB; ++j)
#pragma unroll
        for (int o = 0; o < 6; ++o)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc[j][o] += __shfl_xor(acc[j][o], off);
    if (lane < 6) {
#pragma unroll
        for (int j = 0; j < SB; ++j) {
            float v = acc[j][0];
#pragma unroll
            for (int o = 1; o < 6; ++o) v = lane == o ? acc[j][o] : v;
            float* p = ys + (size_t)(s0 + j) * 6 + lane;
            *p = first_tile ? v : *p + v;
        }
    }
}

__global__ __launch_bounds__(256) void pose_heads_mc_kernel(McArgs g) {
    extern __shared__ float s_y[];                            // [rows of the workgroup][S][6]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * (blockDim.x >> 6) + wave;
    if (row >= g.R) return;                                   // whole waves leave; there is no workgroup barrier below
    float* ys = s_y + (size_t)wave * g.S * 6;
    const uint32_t draw = g.state[0], base = g.state[1];
    const uint32_t off = base + (uint32_t)g.id_offset;
    const uint32_t a = off + (uint32_t)(g.id_a ? g.id_a[row] : (int64_t)row);
    const uint32_t b = g.id_b ? off + (uint32_t)g.id_b[row] : rpg::kMcNodeTag;
    const float4* xr = g.x + (size_t)row * g.d4;

    for (int tile0 = 0; tile0 < g.d4; tile0 += 64 * MC_CH) {
        float4 xv[MC_CH];
#pragma unroll
        for (int c = 0; c < MC_CH; ++c) {
            const int k = tile0 + c * 64 + lane;
            xv[c] = k < g.d4 ? xr[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const bool first = tile0 == 0;
        int s = 0;
        for (; s + MC_SB <= g.S; s += MC_SB) mc_block<MC_SB>(g, xv, tile0, lane, s, a, b, draw, ys, first);
        for (; s < g.S; ++s) mc_block<1>(g, xv, tile0, lane, s, a, b, draw, ys, first);
    }
    __builtin_amdgcn_wave_barrier();

    // lanes 0..5: y_s = scale * sum + b in place, the sequential sum in sample order, then the second pass
    if (lane < 6) {
        const float bias = g.b6[lane];
        float sum = 0.f;
        for (int s = 0; s < g.S; ++s) {
            const float y = g.scale * ys[(size_t)s * 6 + lane] + bias;
            ys[(size_t)s * 6 + lane] = y;
            sum += y;
        }
        const float mu = sum / (float)g.S;
        float ss = 0.f;
        for (int s = 0; s < g.S; ++s) {
            const float dv = ys[(size_t)s * 6 + lane] - mu;
            ss += dv * dv;
        }
        g.mean[(size_t)row * 6 + lane] = mu;
        g.var[(size_t)row * 6 + lane] = g.S > 1 ? ss / (float)(g.S - 1) : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    if (g.samples)
        for (int i = lane; i < g.S * 6; i += 64)
            g.samples[((size_t)(i / 6) * g.R + row) * 6 + (i % 6)] = ys[i];
}

__global__ void mc_advance_kernel(uint32_t* state) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[0] = state[0] + 1u;
}

}  // namespace

extern "C" int rpg_pose_heads_mc_f32(const float* x, const float* w6, const float* b6, int r, int d, double p, int s, uint64_t seed,
                                     const uint32_t* state, const int64_t* id_a, const int64_t* id_b, int64_t id_offset,
                                     float* mean, float* var, float* samples, void* stream) {
    if (!x || !w6 || !b6 || !state || !mean || !var || r <= 0 || d <= 0 || (d & 3) || d / 4 >= 65536 || !(p > 0.0 && p < 1.0) ||
        s < 1 || s > MC_MAX_S || id_offset < 0 || id_offset + (int64_t)r > ((int64_t)1 << 31) || !rpg::aligned16(x) ||
        !rpg::aligned16(w6))
        return RPG_ERR_BAD_ARG;
    McArgs g;
    g.x = reinterpret_cast<const float4*>(x);
    g.w6 = reinterpret_cast<const float4*>(w6);
    g.b6 = b6;
    g.R = r; g.d4 = d / 4; g.S = s;
    const double t = p * 4294967296.0;                        // floor(p 2^32), in double: < 2^32 for p < 1
    g.thr = (uint32_t)(uint64_t)t;
    g.scale = 1.0f / (1.0f - (float)p);
    g.seed_lo = (uint32_t)seed; g.seed_hi = (uint32_t)(seed >> 32);
    g.state = state; g.id_a = id_a; g.id_b = id_b; g.id_offset = id_offset;
    g.mean = mean; g.var = var; g.samples = samples;
    const int rows = s <= MC_SLAB_S ? 4 : 1;                  // rows (waves) per workgroup: the slab is rows * S * 24 bytes <= 24 KB
    hipLaunchKernelGGL(pose_heads_mc_kernel, dim3((r + rows - 1) / rows), dim3(64 * rows), (size_t)rows * s * 6 * sizeof(float),
                       rpg::as_stream(stream), g);
    RPG_CHECK_LAUNCH("pose_heads_mc");
    return RPG_OK;
}

extern "C" int rpg_mc_advance(uint32_t* state, void* stream) {
    if (!state) return RPG_ERR_BAD_ARG;
    hipLaunchKernelGGL(mc_advance_kernel, dim3(1), dim3(64), 0, rpg::as_stream(stream), state);
    RPG_CHECK_LAUNCH("mc_advance");
    return RPG_OK;
}
