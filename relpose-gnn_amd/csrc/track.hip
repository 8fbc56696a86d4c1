// The update launch of the tracking loop (tracking.Tracker): behind a frame's map step and pose rule, one thread per tracked
// camera decides whether the frame's pose is accepted and writes the prior the NEXT frame's retrieval is gated by (retrieve.hip).
// The rule itself is rpg::track_update_one (pose_gate.h), plain C++ that tests/pose_gate_check.cpp runs on the host.
// One launch on the caller's stream, no allocation, no synchronisation: it is captured with the step.
#include "rpg_common.h"
#include "pose_gate.h"

namespace {

constexpr int TU_NT = 64;

__global__ __launch_bounds__(TU_NT) void track_update_kernel(const double* __restrict__ rows, const int32_t* __restrict__ inliers, int s,
                                                             int min_inliers, double min_ratio, int max_lost,
                                                             double* __restrict__ prior, int32_t* __restrict__ lost,
                                                             int32_t* __restrict__ accepted) {
    const int i = blockIdx.x * TU_NT + threadIdx.x;
    if (i >= s) return;
    accepted[i] = rpg::track_update_one(rows + (int64_t)i * 16, inliers[2 * (int64_t)i], inliers[2 * (int64_t)i + 1], min_inliers,
                                        min_ratio, max_lost, prior + (int64_t)i * 7, lost + i);
}

}  // namespace

extern "C" int rpg_track_update_f64(const double* rows, const int32_t* inliers, int s, int min_inliers, double min_ratio,
                                    int max_lost, double* prior, int32_t* lost, int32_t* accepted, void* stream) {
    if (!rows || !inliers || !prior || !lost || !accepted || s < 1 || min_ratio != min_ratio ||
        (reinterpret_cast<uintptr_t>(rows) & 7u) || (reinterpret_cast<uintptr_t>(prior) & 7u) ||
        (reinterpret_cast<uintptr_t>(inliers) & 3u) || (reinterpret_cast<uintptr_t>(lost) & 3u) ||
        (reinterpret_cast<uintptr_t>(accepted) & 3u))
        return RPG_ERR_BAD_ARG;
    hipLaunchKernelGGL(track_update_kernel, dim3((unsigned)((s + TU_NT - 1) / TU_NT)), dim3(TU_NT), 0, rpg::as_stream(stream), rows,
                       inliers, s, min_inliers, min_ratio, max_lost, prior, lost, accepted);
    RPG_CHECK_LAUNCH("track_update");
    return RPG_OK;
}
