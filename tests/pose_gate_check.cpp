// Host check of csrc/pose_gate.h: includes nothing of the project but that header (which needs no HIP) and runs the very text the
// kernels run.  Cases come on stdin, one per line, every double as the 16 hex digits of its bits:
//   g <r2> <cos_half> <rot 0|1> <row x7> <prior x7>                               -> "g <prior finite 0|1> <inside 0|1>"
//   u <min_inliers> <min_ratio> <max_lost> <inliers> <used> <lost> <pose x7> <prior x7>
//                                                                                  -> "u <accepted> <lost> <prior x7>"
// tests/test_pose_gate_cpu.py compares the output with tests/pose_gate_ref.py, bit for bit.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../relpose-gnn_amd/csrc/pose_gate.h"

static bool read_double(double* d) {
    uint64_t u;
    if (scanf("%" SCNx64, &u) != 1) return false;
    memcpy(d, &u, sizeof u);
    return true;
}

static uint64_t bits(double d) {
    uint64_t u;
    memcpy(&u, &d, sizeof u);
    return u;
}

int main() {
    char tag[4];
    long n = 0;
    while (scanf("%3s", tag) == 1) {
        if (tag[0] == 'g') {
            double r2, cos_half, row[7], prior[7];
            int rot;
            if (!read_double(&r2) || !read_double(&cos_half) || scanf("%d", &rot) != 1) return 2;
            for (double& v : row)
                if (!read_double(&v)) return 2;
            for (double& v : prior)
                if (!read_double(&v)) return 2;
            const bool has = rpg::pose_gate_finite7(prior);
            printf("g %d %d\n", has ? 1 : 0, has && rpg::pose_gate_inside(row, prior, r2, cos_half, rot != 0) ? 1 : 0);
        } else if (tag[0] == 'u') {
            int32_t min_inliers, max_lost, inliers, used, lost;
            double min_ratio, pose[7], prior[7];
            if (scanf("%" SCNd32, &min_inliers) != 1 || !read_double(&min_ratio) ||
                scanf("%" SCNd32 "%" SCNd32 "%" SCNd32 "%" SCNd32, &max_lost, &inliers, &used, &lost) != 4)
                return 2;
            for (double& v : pose)
                if (!read_double(&v)) return 2;
            for (double& v : prior)
                if (!read_double(&v)) return 2;
            const int acc = rpg::track_update_one(pose, inliers, used, min_inliers, min_ratio, max_lost, prior, &lost);
            printf("u %d %" PRId32, acc, lost);
            for (double v : prior) printf(" %016" PRIx64, bits(v));
            printf("\n");
        } else {
            return 2;
        }
        ++n;
    }
    printf("pose_gate: ok %ld\n", n);
    return 0;
}
