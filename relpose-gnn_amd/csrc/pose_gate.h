// The pose gate of retrieval (retrieve.hip) and the accept rule of the tracking loop (track.hip).  Plain C++ that the host compiler
// takes as it is (tests/pose_gate_check.cpp) and hipcc compiles for the device: the host and the kernels run the same text.
//
// A gate entry is seven doubles, (t[3], q[4]): the un-normalised translation and the unit quaternion (w, x, y, z) -- what the pose
// rule's rows hold in their first seven columns (query_pose.hip).  Everything is double, every product and sum rounded on its
// own (no contraction), in the order written here; tests/pose_gate_ref.py states the same order in numpy.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#ifndef RPG_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RPG_HD __host__ __device__ __forceinline__
#else
#define RPG_HD inline
#endif
#endif

namespace rpg {

// all seven finite (a NaN compares false, an infinity is above DBL_MAX)
RPG_HD bool pose_gate_finite7(const double* p) {
    bool ok = true;
    for (int i = 0; i < 7; ++i) ok = ok && (fabs(p[i]) <= DBL_MAX);
    return ok;
}

// Whether the map row `row` lies inside the gate around `prior` (both finite7 or the row is outside; the caller has checked the
// prior): squared distance <= r2, and with `rot` |<q_row, q_prior>| >= cos_half, i.e. a rotation of at most max_deg between
// them, q and -q being one rotation.  Both comparisons are inclusive.
RPG_HD bool pose_gate_inside(const double* row, const double* prior, double r2, double cos_half, bool rot) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (!pose_gate_finite7(row)) return false;
    const double dx = row[0] - prior[0], dy = row[1] - prior[1], dz = row[2] - prior[2];
    const double d2 = ((dx * dx + dy * dy) + dz * dz);
    if (!(d2 <= r2)) return false;
    if (!rot) return true;
    const double dot = ((row[3] * prior[3] + row[4] * prior[4]) + row[5] * prior[5]) + row[6] * prior[6];
    return fabs(dot) >= cos_half;
}

// The accept rule of one tracked camera: `pose` is the pose rule's (t, q) of this frame, (inliers, used) its consensus integers.
// Accepted: the pose becomes the prior of the next frame and `lost` returns to 0.  Otherwise `lost` counts one more frame
// (saturating), and once it is above max_lost the prior is forgotten (NaN: the next frame is ranked against the whole map).
// Returns 1 / 0 = accepted / not.
RPG_HD int track_update_one(const double* pose, int32_t inliers, int32_t used, int32_t min_inliers, double min_ratio,
                            int32_t max_lost, double* prior, int32_t* lost) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const bool ok = pose_gate_finite7(pose) && inliers >= min_inliers && (double)inliers >= min_ratio * (double)used;
    if (ok) {
        for (int i = 0; i < 7; ++i) prior[i] = pose[i];
        *lost = 0;
        return 1;
    }
    const int32_t l = *lost < INT32_MAX ? *lost + 1 : INT32_MAX;
    *lost = l;
    if (l > max_lost) {
        const double nan = (double)NAN;
        for (int i = 0; i < 7; ++i) prior[i] = nan;
    }
    return 0;
}

}  // namespace rpg
