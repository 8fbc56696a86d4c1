// Node assembly of the map path (PoseNetX_R2.forward_map): the node features of G graphs, each one query followed by K database
// images whose features were encoded once into a feature map.  Replaces the `x = torch.cat((query, db_batch))` of the
// reference's graph construction (dataset_7Scenes_multi.py:340-345) one level down, on encoder OUTPUT instead of pixels: the
// encoder is per image (eval-mode BatchNorm), so assembling features is the same as encoding the assembled images.
//
// One workgroup per output row (grid-strided over rows): the source row is resolved once per row by the scalar unit, then the
// workgroup copies its d floats as 16-byte loads / stores (d = 2048: 512 float4, two per lane).  HBM-bound and tiny: 64 KB per
// 8-node graph at d = 2048.
#include "rpg_common.h"

namespace {

constexpr int GN_NT = 256;

__global__ __launch_bounds__(GN_NT) void gather_graph_nodes_kernel(const float4* __restrict__ query, const float4* __restrict__ map,
                                                                   const int64_t* __restrict__ nbr, int k, int64_t m, int d4,
                                                                   float4* __restrict__ out, int32_t* __restrict__ status,
                                                                   int64_t rows) {
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const int64_t g = r / (k + 1);
        const int j = (int)(r - g * (k + 1));
        const float4* src;
        if (j == 0) {
            src = query + g * d4;
        } else {
            int64_t idx = nbr[g * k + (j - 1)];
            if (idx < 0 || idx >= m) {                  // counted once per row, clamped: nothing below reads out of bounds
                if (threadIdx.x == 0) atomicAdd(status, 1);
                idx = idx < 0 ? 0 : m - 1;
            }
            src = map + idx * d4;                       // 64-bit row offset: maps past 2 GiB
        }
        float4* dst = out + r * d4;
        for (int c = threadIdx.x; c < d4; c += GN_NT) dst[c] = src[c];
    }
}

}  // namespace

extern "C" int rpg_gather_graph_nodes_f32(const float* query_feat, const float* map_feat, const int64_t* neighbours, int g, int k,
                                          int64_t m, int d, float* out, int32_t* status, void* stream) {
    if (!query_feat || !map_feat || !neighbours || !out || !status || g <= 0 || k <= 0 || m <= 0 || d <= 0 || (d & 3) ||
        !rpg::aligned16(query_feat) || !rpg::aligned16(map_feat) || !rpg::aligned16(out) ||
        (reinterpret_cast<uintptr_t>(neighbours) & 7u) || (reinterpret_cast<uintptr_t>(status) & 3u))
        return RPG_ERR_BAD_ARG;
    const int64_t rows = (int64_t)g * (k + 1);
    const int grid = (int)(rows < 8192 ? rows : 8192);
    hipLaunchKernelGGL(gather_graph_nodes_kernel, dim3(grid), dim3(GN_NT), 0, rpg::as_stream(stream),
                       reinterpret_cast<const float4*>(query_feat), reinterpret_cast<const float4*>(map_feat), neighbours, k, m,
                       d / 4, reinterpret_cast<float4*>(out), status, rows);
    RPG_CHECK_LAUNCH("gather_graph_nodes");
    return RPG_OK;
}
