// Pose recovery of the evaluation streams: per graph of one forward's output the reference edge, the query's absolute pose
// (t, q) and its translation / rotation error -- what eval_RP does on the host with the model outputs (testing/test.py:213-267:
// the first edge into the query node, `target[source] - rel_pose`, qexp, translation * std + mean, the two losses;
// evaluate.query_pose / evaluate.errors restate it in numpy).  float64 arithmetic on the fp32 inputs, like the host code.
//
// Three rules, two kernels, one set of pieces.  Shared by both kernels and stated once below: a graph's node span and clamped
// column span (graph_span), the query's own target row and a source node's pose row in either graph form (target_row,
// source_row), a row turned into (t, q) (pose_of), the two errors (trans_dist, quat_angle) and the row of 16 doubles written as
// eight 16-byte stores (store_row, store_nan_row, store_void_row).  On the host one function checks the arguments the three
// entry points share and fills QpArgs (qp_args); the fused launcher adds only what is its own.
//
// The single reference edge (query_pose_kernel): one wave per graph.  The wave steps over the graph's columns 64 at a time:
// every lane tests one column's target against the graph's first node, a ballot gathers the 64 answers in COLUMN order,
// popcounts are accumulated until the `ref_node`-th hit is inside the current step, and the wave stops there.  Which column is
// chosen is a function of the column order only (a self-edge counts here; the fused rules skip it).  Lane 0 then does the few
// dozen double operations of one pose and stores the row.  No LDS, no barrier.  The only atomic is the integer count of bad
// graphs.  One launch, no allocation, no synchronisation.  The fused rules (query_pose_fused_kernel) are described above it.
#include "rpg_common.h"

#include <math.h>

namespace {

constexpr int QP_NT = 256;            // 4 waves = 4 graphs per workgroup

struct QpArgs {
    const float* rel_pose;            // [e][6]
    const int64_t* edge_src;          // [e]
    const int64_t* edge_dst;          // [e]
    int64_t e;
    const int64_t* node_first;        // [g + 1] (targets form) | null (map form: graph i owns nodes [i (k+1), (i+1)(k+1)))
    const int64_t* edge_first;        // [g + 1] | null: the graph's columns are those whose target lies in its node range
    int g;
    const float* node_targets;        // [n][6] | null
    int64_t n;
    const float* map_poses;           // [m][6] | null
    int64_t m;
    const int64_t* neighbours;        // [g][k]
    int k;
    const float* query_targets;       // [g][6] | null (zeros)
    double pose_m[3], pose_s[3];
    int ref_node;
    double* out;                      // [g][16]
    int32_t* status;
};

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// (cos|v|, sin|v| / |v| * v), (1, 0, 0, 0) at |v| = 0   (pose_utils.py:340-348).  Non-finite input: |v| is NaN or inf, cos and
// sin / |v| are NaN, and NaN * v is NaN in every component -- what numpy gives.
__device__ __forceinline__ void qexp(const double* v, double* q) {
#pragma clang fp contract(off)
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double s = n == 0.0 ? 1.0 : sin(n) / n;
    q[0] = cos(n);
    q[1] = s * v[0];
    q[2] = s * v[1];
    q[3] = s * v[2];
}

// ---- what both kernels share ---------------------------------------------------------------------------------------------------
struct QpSpan {
    int64_t first, last;              // the graph's nodes [first, last); `first` is the query
    int64_t lo, hi;                   // its columns [lo, hi), clamped: a wrong offset gives a wrong or bad row, never a read outside [0, e)
};

__device__ __forceinline__ QpSpan graph_span(const QpArgs& a, int64_t gi) {
    QpSpan s;
    s.first = a.node_first ? a.node_first[gi] : gi * (a.k + 1);
    s.last = a.node_first ? a.node_first[gi + 1] : s.first + a.k + 1;
    s.lo = a.edge_first ? clamp_i64(a.edge_first[gi], 0, a.e) : 0;
    s.hi = a.edge_first ? clamp_i64(a.edge_first[gi + 1], 0, a.e) : a.e;
    return s;
}

// targets form: whether the graph's nodes lie outside node_targets (no row of such a graph is read)
__device__ __forceinline__ bool outside_targets(const QpArgs& a, const QpSpan& s) {
    return a.node_targets && (s.first < 0 || s.last > a.n);
}

// the query's own target row (null: zeros)
__device__ __forceinline__ const float* target_row(const QpArgs& a, int64_t gi, const QpSpan& s) {
    if (a.node_targets) return a.node_targets + s.first * 6;
    return a.query_targets ? a.query_targets + gi * 6 : nullptr;
}

// the pose row of source node `src` in [first, last): its target, or in the map form the query's own row (`trow`) for src == first
// and else the map row of its neighbour -- forward_map has counted a neighbour outside [0, m) already; here it is clamped like there
__device__ __forceinline__ const float* source_row(const QpArgs& a, int64_t gi, const QpSpan& s, int64_t src, const float* trow) {
    if (a.node_targets) return a.node_targets + src * 6;
    if (src == s.first) return trow;
    return a.map_poses + clamp_i64(a.neighbours[gi * a.k + (src - s.first - 1)], 0, a.m - 1) * 6;
}

// (t, q) of the normalised [t, log q] row `row` (null: zeros) minus, when given, the relative pose `rel`: test.py:231, 248-251
__device__ __forceinline__ void pose_of(const QpArgs& a, const float* row, const float* rel, double* t, double* q) {
#pragma clang fp contract(off)
    double v[6];
    for (int i = 0; i < 6; ++i) {
        v[i] = row ? (double)row[i] : 0.0;
        if (rel) v[i] = v[i] - (double)rel[i];
    }
    for (int i = 0; i < 3; ++i) t[i] = v[i] * a.pose_s[i] + a.pose_m[i];
    qexp(v + 3, q);
}

// 2 acos(|<p, q>|) in degrees (pose_utils.py:420-431); the clamp is Python's min(1.0, max(-1.0, d)): max keeps -1.0 unless
// d > -1.0, so a NaN dot becomes -1 and the error 360
__device__ __forceinline__ double quat_angle(const double* p, const double* q) {
#pragma clang fp contract(off)
    double d = fabs(q[0] * p[0] + q[1] * p[1] + q[2] * p[2] + q[3] * p[3]);
    d = d > -1.0 ? d : -1.0;
    d = d < 1.0 ? d : 1.0;
    return 2.0 * acos(d) * 180.0 / M_PI;
}

__device__ __forceinline__ double trans_dist(const double* p, const double* t) {
#pragma clang fp contract(off)
    const double dx = p[0] - t[0], dy = p[1] - t[1], dz = p[2] - t[2];
    return sqrt(dx * dx + dy * dy + dz * dz);
}

__device__ __forceinline__ void store_row(double* row, const double* pt, const double* pq, const double* tt, const double* tq,
                                          double t_err, double q_err) {
    double2* orow = reinterpret_cast<double2*>(row);
    orow[0] = make_double2(pt[0], pt[1]);
    orow[1] = make_double2(pt[2], pq[0]);
    orow[2] = make_double2(pq[1], pq[2]);
    orow[3] = make_double2(pq[3], tt[0]);
    orow[4] = make_double2(tt[1], tt[2]);
    orow[5] = make_double2(tq[0], tq[1]);
    orow[6] = make_double2(tq[2], tq[3]);
    orow[7] = make_double2(t_err, q_err);
}

__device__ __forceinline__ void store_nan_row(double* row) {
    const double nan = __builtin_nan("");
    double2* orow = reinterpret_cast<double2*>(row);
    for (int i = 0; i < 8; ++i) orow[i] = make_double2(nan, nan);
}

// a row whose pose and errors are NaN behind a target that stands
__device__ __forceinline__ void store_void_row(double* row, const double* tt, const double* tq) {
    const double nan = __builtin_nan("");
    const double nt[3] = {nan, nan, nan}, nq[4] = {nan, nan, nan, nan};
    store_row(row, nt, nq, tt, tq, nan, nan);
}

// ---- the single reference edge --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(QP_NT) void query_pose_kernel(const QpArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int64_t gi = (int64_t)blockIdx.x * (QP_NT / 64) + (threadIdx.x >> 6);
    if (gi >= a.g) return;                                // (the whole wave)
    const QpSpan s = graph_span(a, gi);
    // the ref_node-th column, in column order, whose target is the graph's first node (test.py:227-229); a self-edge counts
    int64_t ref = -1;
    if (s.last > s.first) {                               // (a graph without nodes owns no column)
        int need = a.ref_node;
        for (int64_t c0 = s.lo; c0 < s.hi; c0 += 64) {
            const int64_t c = c0 + lane;
            const bool hit = c < s.hi && a.edge_dst[c] == s.first;
            unsigned long long mask = __ballot(hit);
            const int cnt = __popcll(mask);
            if (cnt > need) {
                for (int i = 0; i < need; ++i) mask &= mask - 1;      // drop the hits before the wanted one
                ref = c0 + (__ffsll((long long)mask) - 1);
                break;
            }
            need -= cnt;
        }
    }
    if (lane != 0) return;

    bool bad = ref < 0;
    int64_t src = s.first;
    if (!bad) {
        src = a.edge_src[ref];
        bad = src < s.first || src >= s.last;             // the reference edge's source lies outside the graph
    }
    if (bad || outside_targets(a, s)) {
        atomicAdd(a.status, 1);
        store_nan_row(a.out + gi * 16);
        return;
    }
    const float* trow = target_row(a, gi, s);
    double pt[3], pq[4], tt[3], tq[4];
    pose_of(a, source_row(a, gi, s, src, trow), a.rel_pose + ref * 6, pt, pq);
    pose_of(a, trow, nullptr, tt, tq);
    store_row(a.out + gi * 16, pt, pq, tt, tq, trans_dist(pt, tt), quat_angle(pq, tq));
}

// ---- all of a query's reference edges fused into one pose ---------------------------------------------------------------------
// Every column into the query node is one estimate of its pose (the single-edge rule above keeps one and drops the rest).  One
// wave per graph again.  The wave steps over the graph's columns 64 at a time; a hit whose source is not the query itself takes
// the next candidate slot (ballot + popcounts in column order) until `max_edges` slots are filled, and the scan goes on to the
// end so that `count` tells what the limit cut.  Lane c then computes candidate c -- the sin / cos / sqrt of the candidates run
// side by side -- and writes its 7 doubles to LDS (4 waves x 64 x 7 doubles = 14 KB, plus 2 KB of column indices).  Every
// reduction is a function of the column order only: the sums of `mean` run sequentially over LDS in lane 0 (mean_of, over a
// slot mask: the low C bits here, the inlier mask for `consensus`); for `median` every
// lane ranks its own value (smaller values, ties by slot) and the lane(s) of the middle rank(s) are read with a cross-lane move;
// for the medoid lane c adds up its own row of angles in slot order and a butterfly of cross-lane moves takes the lexicographic
// minimum of (sum, c).  No floating-point atomics; the only atomic is the integer count of bad graphs.
//
// `consensus` (rpg_query_pose_consensus_f64) is the third mode: the candidates vote.  Lane c walks the slots in order over LDS and
// counts, as an integer, the finite candidates within `inlier_t` and `inlier_deg` of its own (itself included, by c == d and not by
// an angle test); the same kind of butterfly takes the lexicographic maximum of (support, lowest c); every lane then tests itself
// against that winner, one ballot is the inlier mask in slot order and its popcount the inlier count; lane 0 runs the mean's
// sequential sums over the masked slots.  A non-finite candidate is an outlier here, it does not void the pose.
//
// Inverse-variance weights (rpg_query_pose_weighted_f64) are a further mode of `mean` and of `consensus`, not a rule of their own:
// lane c reads its column's six variances where it makes candidate c, turns them into three translation weights and one rotation
// weight, 1 / (v + var_floor), and writes the four beside the candidate in LDS (4 waves x 64 x 4 doubles = 8 KB more); whether the
// six can be used (none NaN, negative or +inf) is one more ballot next to the finite one, and an unusable variance counts wherever
// a non-finite candidate does.  The voting is unchanged and unweighted.  Lane 0 then runs mean_of_weighted in place of mean_of over
// the same slot mask, again sequentially in slot order, and writes the two predicted deviations of the fused pose (`spread`) with
// one 16-byte store.  Without weights none of this is read or written and mean_of is what runs.
constexpr int QF_MEAN = 0, QF_MEDIAN = 1, QF_CONSENSUS = 2;
constexpr int QF_MAX = 64;            // candidates per graph: one per lane

struct QfArgs {
    QpArgs q;                         // (ref_node unused)
    int fuse, max_edges;
    double* cand;                     // [g][max_edges][16] | null
    int32_t* count;                   // [g] | null
    double inlier_t, inlier_deg;      // consensus: the two thresholds
    int32_t* inliers;                 // consensus: [g][2] = (inliers, used) | null
    const float* rel_var;             // weighted: [e][6], row for row with rel_pose | null = unweighted
    double var_floor;                 // weighted: added to every variance before the division
    double* spread;                   // weighted: [g][2] = (sigma_t, sigma_q) | null
};

// the two predicted deviations of a fused pose from its weight sums W[3] and Wq
__device__ __forceinline__ void spread_of(const double* sw, double swq, const double* pose_s, double* sp) {
#pragma clang fp contract(off)
    sp[0] = sqrt((pose_s[0] * pose_s[0] / sw[0] + pose_s[1] * pose_s[1] / sw[1]) + pose_s[2] * pose_s[2] / sw[2]);
    sp[1] = sqrt(1.0 / swq);
}

// `spread` of graph gi (when asked for): one 16-byte store; NaN where the pose has a NaN component
__device__ __forceinline__ void store_spread(double* spread, int64_t gi, const double* pt, const double* pq, const double* sp) {
    if (!spread) return;
    bool nan = false;
    for (int i = 0; i < 3; ++i) nan = nan || isnan(pt[i]);
    for (int i = 0; i < 4; ++i) nan = nan || isnan(pq[i]);
    const double v = __builtin_nan("");
    *reinterpret_cast<double2*>(spread + gi * 2) = nan ? make_double2(v, v) : make_double2(sp[0], sp[1]);
}

__device__ __forceinline__ void store_nan_spread(double* spread, int64_t gi) {
    const double v = __builtin_nan("");
    if (spread) *reinterpret_cast<double2*>(spread + gi * 2) = make_double2(v, v);
}

// The `mean` of the candidates (t[3], q[4]) whose slot is set in `mask` (never empty), every sum sequential in slot order:
// t = the sum / n; q = S / |S| with S the sum of q_c where <q_c, q_0> >= 0 and of -q_c elsewhere, q_0 = the first set slot, and
// q_0 itself where |S| = 0.
__device__ __forceinline__ void mean_of(const double (*cand)[7], unsigned long long mask, double* ft, double* fq) {
#pragma clang fp contract(off)
    const double* c0 = cand[__ffsll((long long)mask) - 1];
    double st[3] = {0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};
    for (unsigned long long rest = mask; rest != 0ull; rest &= rest - 1ull) {
        const double* cd = cand[__ffsll((long long)rest) - 1];
        for (int i = 0; i < 3; ++i) st[i] = st[i] + cd[i];
        const double dot = cd[3] * c0[3] + cd[4] * c0[4] + cd[5] * c0[5] + cd[6] * c0[6];
        for (int i = 0; i < 4; ++i) sq[i] = dot >= 0.0 ? sq[i] + cd[3 + i] : sq[i] - cd[3 + i];
    }
    for (int i = 0; i < 3; ++i) ft[i] = st[i] / (double)__popcll(mask);
    const double norm = sqrt(sq[0] * sq[0] + sq[1] * sq[1] + sq[2] * sq[2] + sq[3] * sq[3]);
    for (int i = 0; i < 4; ++i) fq[i] = norm == 0.0 ? c0[3 + i] : sq[i] / norm;
}

// The weighted form of mean_of over the same kind of mask (two or more slots): `wt` holds per slot the translation weights w[3] and
// the rotation weight wq.  t_j = (sum w_j t_j) / W_j with W_j = sum w_j; q = S / |S| with S the sum of +/- wq q_c, the sign as in
// mean_of; every sum sequential in slot order.  sp = (sqrt((s_0 s_0 / W_0 + s_1 s_1 / W_1) + s_2 s_2 / W_2), sqrt(1 / Wq)), s = pose_s.
__device__ __forceinline__ void mean_of_weighted(const double (*cand)[7], const double (*wt)[4], unsigned long long mask,
                                                 const double* pose_s, double* ft, double* fq, double* sp) {
#pragma clang fp contract(off)
    const double* c0 = cand[__ffsll((long long)mask) - 1];
    double st[3] = {0.0, 0.0, 0.0}, sw[3] = {0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0}, swq = 0.0;
    for (unsigned long long rest = mask; rest != 0ull; rest &= rest - 1ull) {
        const int c = __ffsll((long long)rest) - 1;
        const double* cd = cand[c];
        const double* w = wt[c];
        for (int i = 0; i < 3; ++i) {
            st[i] = st[i] + w[i] * cd[i];
            sw[i] = sw[i] + w[i];
        }
        const double dot = cd[3] * c0[3] + cd[4] * c0[4] + cd[5] * c0[5] + cd[6] * c0[6];
        for (int i = 0; i < 4; ++i) sq[i] = dot >= 0.0 ? sq[i] + w[3] * cd[3 + i] : sq[i] - w[3] * cd[3 + i];
        swq = swq + w[3];
    }
    for (int i = 0; i < 3; ++i) ft[i] = st[i] / sw[i];
    const double norm = sqrt(sq[0] * sq[0] + sq[1] * sq[1] + sq[2] * sq[2] + sq[3] * sq[3]);
    for (int i = 0; i < 4; ++i) fq[i] = norm == 0.0 ? c0[3 + i] : sq[i] / norm;
    spread_of(sw, swq, pose_s, sp);
}

// whether two FINITE candidates (t[3], q[4]) support each other: symmetric bit for bit -- the squares and the products of the dot
// are the same numbers either way round
__device__ __forceinline__ bool cons_support(const double* c, const double* d, double inlier_t, double inlier_deg) {
#pragma clang fp contract(off)
    return trans_dist(c, d) <= inlier_t && quat_angle(c + 3, d + 3) <= inlier_deg;
}

__global__ __launch_bounds__(QP_NT) void query_pose_fused_kernel(const QfArgs f) {
#pragma clang fp contract(off)
    __shared__ double s_cand[QP_NT / 64][QF_MAX][7];      // per wave: candidate c = t[3], q[4]
    __shared__ long long s_col[QP_NT / 64][QF_MAX];       // per wave: the column of candidate c
    __shared__ double s_wt[QP_NT / 64][QF_MAX][4];        // per wave, weighted only: candidate c's weights w[3], wq
    const QpArgs& a = f.q;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t gi = (int64_t)blockIdx.x * (QP_NT / 64) + w;
    const bool active = gi < a.g;                         // (wave-uniform; no wave leaves before the last barrier)
    const bool weighted = f.rel_var != nullptr;

    // ---- the usable columns, in column order: target = the graph's first node, source != that node -------------------------------
    QpSpan s = {0, 0, 0, 0};
    int64_t found = 0;
    if (active) {
        s = graph_span(a, gi);
        if (s.last > s.first) {
            for (int64_t c0 = s.lo; c0 < s.hi; c0 += 64) {
                const int64_t c = c0 + lane;
                const bool hit = c < s.hi && a.edge_dst[c] == s.first && a.edge_src[c] != s.first;
                const unsigned long long mask = __ballot(hit);
                if (hit) {
                    const int64_t slot = found + __popcll(mask & ((1ull << lane) - 1ull));
                    if (slot < f.max_edges) s_col[w][slot] = c;
                }
                found += __popcll(mask);
            }
        }
    }
    __syncthreads();

    // ---- lane c: candidate c --------------------------------------------------------------------------------------------------------
    const int cn = (int)(found < f.max_edges ? found : f.max_edges);      // C, the candidates used
    const bool mine = active && lane < cn;
    bool bad = false, void_row = false;
    unsigned long long finite = 0ull;                     // the used candidates without a non-finite component, by slot
    unsigned long long unusable_any = 0ull;               // weighted: the used candidates whose variance cannot be used, by slot
    double pt[3], pq[4], tt[3], tq[4], t_err = 0.0, q_err = 0.0;
    for (int i = 0; i < 3; ++i) pt[i] = tt[i] = 0.0;
    for (int i = 0; i < 4; ++i) pq[i] = tq[i] = 0.0;
    if (active) {
        int64_t col = 0, src = s.first;
        bool bad_lane = false;
        if (mine) {
            col = s_col[w][lane];
            src = a.edge_src[col];
            bad_lane = src < s.first || src >= s.last;    // a used edge's source lies outside the graph
        }
        bad = cn == 0 || __ballot(bad_lane) != 0ull || outside_targets(a, s);
        if (!bad) {
            const float* trow = target_row(a, gi, s);
            pose_of(a, trow, nullptr, tt, tq);
            bool nf_lane = false;
            if (mine) {                                   // (the query's own node is never a source here)
                pose_of(a, source_row(a, gi, s, src, trow), a.rel_pose + col * 6, pt, pq);
                t_err = trans_dist(pt, tt);
                q_err = quat_angle(pq, tq);
                for (int i = 0; i < 3; ++i) {
                    s_cand[w][lane][i] = pt[i];
                    nf_lane = nf_lane || !isfinite(pt[i]);
                }
                for (int i = 0; i < 4; ++i) {
                    s_cand[w][lane][3 + i] = pq[i];
                    nf_lane = nf_lane || !isfinite(pq[i]);
                }
            }
            unsigned long long nf = __ballot(nf_lane);
            if (weighted) {                               // an unusable variance counts wherever a non-finite candidate does
                bool unusable = false;
                if (mine) {
                    const float* vrow = f.rel_var + col * 6;
                    double v[6];
                    for (int i = 0; i < 6; ++i) {
                        v[i] = (double)vrow[i];
                        unusable = unusable || !(v[i] >= 0.0) || v[i] == __builtin_inf();
                    }
                    for (int i = 0; i < 3; ++i) s_wt[w][lane][i] = 1.0 / (v[i] + f.var_floor);
                    s_wt[w][lane][3] = 1.0 / (((v[3] + v[4]) + v[5]) + f.var_floor);
                }
                unusable_any = __ballot(unusable);
                if (f.fuse == QF_CONSENSUS) nf |= unusable_any;
            }
            finite = __ballot(mine) & ~nf;
            void_row = cn > 1 && (nf | unusable_any) != 0ull;     // a non-finite candidate voids the fused pose (not C = 1)
        }
        if (f.cand && lane < f.max_edges) {
            double* crow = f.cand + (gi * f.max_edges + lane) * 16;
            if (mine && !bad) {
                store_row(crow, pt, pq, tt, tq, t_err, q_err);
            } else {
                store_nan_row(crow);
            }
        }
        if (f.count && lane == 0) f.count[gi] = (int32_t)(found < 0x7fffffff ? found : 0x7fffffff);
    }
    __syncthreads();
    if (!active) return;
    if (bad) {
        if (lane == 0) {
            atomicAdd(a.status, 1);
            store_nan_row(a.out + gi * 16);
            store_nan_spread(f.spread, gi);
            if (f.inliers) *reinterpret_cast<int2*>(f.inliers + gi * 2) = make_int2(0, cn);
        }
        return;
    }
    // ---- the fused pose (the whole wave is here: cross-lane moves below; lane 0 stores it) -----------------------------------------
    double ft[3], fq[4], sp[2] = {0.0, 0.0};
    if (f.fuse == QF_CONSENSUS) {                         // the candidates vote
        const bool fin = ((finite >> lane) & 1ull) != 0ull;
        double me[7];
        for (int i = 0; i < 3; ++i) me[i] = pt[i];
        for (int i = 0; i < 4; ++i) me[3 + i] = pq[i];
        int support = 0, best = lane;
        if (fin) {
            for (int d = 0; d < cn; ++d) {
                if (d == lane) {
                    ++support;
                } else if ((finite >> d) & 1ull) {
                    support += cons_support(me, s_cand[w][d], f.inlier_t, f.inlier_deg) ? 1 : 0;
                }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {          // the lexicographic maximum of (support, lowest c)
            const int so = __shfl_xor(support, off);
            const int bo = __shfl_xor(best, off);
            if (so > support || (so == support && bo < best)) {
                support = so;
                best = bo;
            }
        }
        // (support == 0: no finite candidate at all, and `best` is lane 0 -- nobody is an inlier)
        const bool inl = fin && support > 0 && (lane == best || cons_support(me, s_cand[w][best], f.inlier_t, f.inlier_deg));
        const unsigned long long mask = __ballot(inl);
        if (lane != 0) return;
        const int ni = __popcll(mask);
        if (f.inliers) *reinterpret_cast<int2*>(f.inliers + gi * 2) = make_int2(ni, cn);
        if (ni == 0) {                                    // every candidate is non-finite
            store_void_row(a.out + gi * 16, tt, tq);
            store_nan_spread(f.spread, gi);
            return;
        }
        if (ni == 1) {                                    // one inlier as it is
            const int c = __ffsll((long long)mask) - 1;
            const double* c0 = s_cand[w][c];
            for (int i = 0; i < 3; ++i) ft[i] = c0[i];
            for (int i = 0; i < 4; ++i) fq[i] = c0[3 + i];
            if (weighted) spread_of(s_wt[w][c], s_wt[w][c][3], a.pose_s, sp);
        } else if (weighted) {
            mean_of_weighted(s_cand[w], s_wt[w], mask, a.pose_s, ft, fq, sp);
        } else {
            mean_of(s_cand[w], mask, ft, fq);
        }
    } else if (cn == 1) {                                 // the candidate as it is: the single-edge rule's row
        if (lane == 0) {
            store_row(a.out + gi * 16, pt, pq, tt, tq, t_err, q_err);
            if (weighted && unusable_any == 0ull) {
                spread_of(s_wt[w][0], s_wt[w][0][3], a.pose_s, sp);
                store_spread(f.spread, gi, pt, pq, sp);
            } else {
                store_nan_spread(f.spread, gi);
            }
        }
        return;
    } else if (void_row) {
        if (lane == 0) {
            store_void_row(a.out + gi * 16, tt, tq);
            store_nan_spread(f.spread, gi);
        }
        return;
    } else if (f.fuse == QF_MEAN) {
        if (lane != 0) return;
        if (weighted) {
            mean_of_weighted(s_cand[w], s_wt[w], ~0ull >> (64 - cn), a.pose_s, ft, fq, sp);
        } else {
            mean_of(s_cand[w], ~0ull >> (64 - cn), ft, fq);    // slots 0 .. cn - 1 (cn can be 64: no 1ull << cn)
        }
    } else {
        // component-wise median of t: every lane ranks its own value, ties by slot, and the middle rank(s) are read
        for (int j = 0; j < 3; ++j) {
            const double v = pt[j];
            int rank = 0;
            for (int d = 0; d < cn; ++d) {
                const double vd = s_cand[w][d][j];
                rank += (vd < v || (vd == v && d < lane)) ? 1 : 0;
            }
            const unsigned long long m_lo = __ballot(mine && rank == (cn - 1) / 2);
            const unsigned long long m_hi = __ballot(mine && rank == cn / 2);
            const double v_lo = __shfl(v, __ffsll((long long)m_lo) - 1);
            const double v_hi = __shfl(v, __ffsll((long long)m_hi) - 1);
            ft[j] = (cn & 1) ? v_lo : (v_lo + v_hi) / 2.0;
        }
        // medoid of q: lane c's sum of angles to the others in slot order, then the lexicographic minimum of (sum, c)
        double sum = __builtin_inf();
        int best = lane;
        if (mine) {
            sum = 0.0;
            for (int d = 0; d < cn; ++d)
                if (d != lane) sum = sum + quat_angle(pq, &s_cand[w][d][3]);
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double so = __shfl_xor(sum, off);
            const int bo = __shfl_xor(best, off);
            if (so < sum || (so == sum && bo < best)) {
                sum = so;
                best = bo;
            }
        }
        if (lane != 0) return;
        for (int i = 0; i < 4; ++i) fq[i] = s_cand[w][best][3 + i];
    }
    store_row(a.out + gi * 16, ft, fq, tt, tq, trans_dist(ft, tt), quat_angle(fq, tq));
    store_spread(f.spread, gi, ft, fq, sp);
}

inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// what the four entry points share, as they declare it and as they hand it on
#define QP_SHARED_PARAMS                                                                                                        \
    const float *rel_pose, const int64_t *edge_src, const int64_t *edge_dst, int64_t e, const int64_t *node_first,             \
        const int64_t *edge_first, int g, const float *node_targets, int64_t n, const float *map_poses, int64_t m,              \
        const int64_t *neighbours, int k, const float *query_targets, double pose_m0, double pose_m1, double pose_m2,           \
        double pose_s0, double pose_s1, double pose_s2
#define QP_SHARED                                                                                                               \
    rel_pose, edge_src, edge_dst, e, node_first, edge_first, g, node_targets, n, map_poses, m, neighbours, k, query_targets,   \
        pose_m0, pose_m1, pose_m2, pose_s0, pose_s1, pose_s2

// The shared arguments checked (null, range, the two forms, alignment) and `a` filled from them; false: RPG_ERR_BAD_ARG.
bool qp_args(QpArgs& a, QP_SHARED_PARAMS, int ref_node, double* out, int32_t* status) {
    if (!rel_pose || !edge_src || !edge_dst || !out || !status || e < 1 || g < 1 || ref_node < 0) return false;
    if ((node_targets == nullptr) == (map_poses == nullptr)) return false;                // one source of poses, not both
    if (node_targets) {
        if (!node_first || n < 1 || neighbours || query_targets) return false;
    } else {
        if (node_first || !neighbours || m < 1 || k < 1) return false;
    }
    if (misaligned(rel_pose, 3) || misaligned(node_targets, 3) || misaligned(map_poses, 3) || misaligned(query_targets, 3) ||
        misaligned(edge_src, 7) || misaligned(edge_dst, 7) || misaligned(node_first, 7) || misaligned(edge_first, 7) ||
        misaligned(neighbours, 7) || misaligned(status, 3) || !rpg::aligned16(out))
        return false;
    a = QpArgs{rel_pose, edge_src, edge_dst, e, node_first, edge_first, g, node_targets, n, map_poses, m, neighbours, k,
               query_targets, {pose_m0, pose_m1, pose_m2}, {pose_s0, pose_s1, pose_s2}, ref_node, out, status};
    return true;
}

inline unsigned qp_grid(int g) { return (unsigned)((g + QP_NT / 64 - 1) / (QP_NT / 64)); }

// the fused kernel over `f`, whose `q` qp_args has filled: what is the fused rule's own is checked and set here
// (`weighted`: rel_var [e][6] and var_floor are read and spread may be written; otherwise the three are null / 0 / null)
int launch_fused(QfArgs& f, int fuse, int max_edges, double inlier_t, double inlier_deg, double* cand, int32_t* count,
                 int32_t* inliers, bool weighted, const float* rel_var, double var_floor, double* spread, void* stream) {
    if (max_edges < 1 || max_edges > QF_MAX) return RPG_ERR_BAD_ARG;
    if (misaligned(count, 3) || misaligned(inliers, 7) || (cand && !rpg::aligned16(cand))) return RPG_ERR_BAD_ARG;
    if (weighted) {                                       // (written so that a NaN floor fails the test too)
        if (!rel_var || misaligned(rel_var, 3) || (spread && !rpg::aligned16(spread))) return RPG_ERR_BAD_ARG;
        if (!(var_floor >= 1e-30 && var_floor < __builtin_inf())) return RPG_ERR_BAD_ARG;
    }
    f.rel_var = weighted ? rel_var : nullptr;
    f.var_floor = weighted ? var_floor : 0.0;
    f.spread = weighted ? spread : nullptr;
    f.fuse = fuse;
    f.max_edges = max_edges;
    f.cand = cand;
    f.count = count;
    f.inlier_t = inlier_t;
    f.inlier_deg = inlier_deg;
    f.inliers = inliers;
    hipLaunchKernelGGL(query_pose_fused_kernel, dim3(qp_grid(f.q.g)), dim3(QP_NT), 0, rpg::as_stream(stream), f);
    RPG_CHECK_LAUNCH("query_pose_fused");
    return RPG_OK;
}

}  // namespace

extern "C" int rpg_query_pose_f64(QP_SHARED_PARAMS, int ref_node, double* out, int32_t* status, void* stream) {
    QpArgs a;
    if (!qp_args(a, QP_SHARED, ref_node, out, status)) return RPG_ERR_BAD_ARG;
    hipLaunchKernelGGL(query_pose_kernel, dim3(qp_grid(g)), dim3(QP_NT), 0, rpg::as_stream(stream), a);
    RPG_CHECK_LAUNCH("query_pose");
    return RPG_OK;
}

extern "C" int rpg_query_pose_fused_f64(QP_SHARED_PARAMS, int fuse, int max_edges, double* out, double* cand, int32_t* count,
                                        int32_t* status, void* stream) {
    QfArgs f;
    if ((fuse != QF_MEAN && fuse != QF_MEDIAN) || !qp_args(f.q, QP_SHARED, 0, out, status)) return RPG_ERR_BAD_ARG;
    return launch_fused(f, fuse, max_edges, 0.0, 0.0, cand, count, nullptr, false, nullptr, 0.0, nullptr, stream);
}

extern "C" int rpg_query_pose_consensus_f64(QP_SHARED_PARAMS, int max_edges, double inlier_t, double inlier_deg, double* out,
                                            double* cand, int32_t* count, int32_t* inliers, int32_t* status, void* stream) {
    // (written so that a NaN threshold fails the test too)
    if (!(inlier_t >= 0.0 && inlier_t < __builtin_inf()) || !(inlier_deg >= 0.0 && inlier_deg <= 360.0)) return RPG_ERR_BAD_ARG;
    QfArgs f;
    if (!qp_args(f.q, QP_SHARED, 0, out, status)) return RPG_ERR_BAD_ARG;
    return launch_fused(f, QF_CONSENSUS, max_edges, inlier_t, inlier_deg, cand, count, inliers, false, nullptr, 0.0, nullptr, stream);
}

extern "C" int rpg_query_pose_weighted_f64(QP_SHARED_PARAMS, int max_edges, double inlier_t, double inlier_deg, const float* rel_var,
                                           double var_floor, int consensus, double* out, double* cand, int32_t* count,
                                           int32_t* inliers, double* spread, int32_t* status, void* stream) {
    if (!(inlier_t >= 0.0 && inlier_t < __builtin_inf()) || !(inlier_deg >= 0.0 && inlier_deg <= 360.0)) return RPG_ERR_BAD_ARG;
    if ((consensus != 0 && consensus != 1) || (consensus == 0 && inliers)) return RPG_ERR_BAD_ARG;
    QfArgs f;
    if (!qp_args(f.q, QP_SHARED, 0, out, status)) return RPG_ERR_BAD_ARG;
    return launch_fused(f, consensus ? QF_CONSENSUS : QF_MEAN, max_edges, inlier_t, inlier_deg, cand, count, consensus ? inliers : nullptr,
                        true, rel_var, var_floor, spread, stream);
}
