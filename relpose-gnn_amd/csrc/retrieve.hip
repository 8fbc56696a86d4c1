// Image retrieval against a feature map: for every query descriptor the database rows at given positions of the order
// (cosine similarity descending, row index ascending) over the rows its exclusion group allows -- the selection step of the
// reference's obtain_KNNs (dataset_7Scenes_multi.py:238-264) with everything random moved into `ranks` (retrieval.py).
//
// Three launches on the caller's stream, no allocation, no synchronisation:
//   1. row_inv_norms_kernel     1 / |q_g| into the workspace (and 1 / |d_m| when the caller has not cached them)
//   2. retrieve_dot_kernel<NQ>  <q_g, d_m> on the f32 matrix pipe (v_mfma_f32_16x16x4_f32).  A workgroup owns 16 database rows and
//                               up to 64 queries, so the database is read from HBM once per 64 queries; its four waves take
//                               every fourth 64-column block and are summed through LDS in wave order; the column range is cut
//                               in `split` slices (grid.y) whose partial products go to the workspace and are summed in slice
//                               order by the next kernel.  ONE code path for every g: a single query runs as a tile of 16 with 15
//                               zero rows (still bandwidth-bound: 16 x the flop of a matrix-vector pass is a quarter of the time
//                               the bytes take), and the slice count depends on (m, d) only -- so the bits of a similarity depend
//                               on the two rows and on d, never on where the rows sit, on the tile, or on the batch.
//   3. retrieve_select_kernel   one workgroup per query: similarity -> ordered 32-bit key (excluded rows and non-finite
//                               similarities get the two largest keys), radix select of the R-th smallest (key, row) pair
//                               (R = largest rank + 1 <= R_MAX), the R pairs collected and sorted in LDS, ranks read off.
// The LDS atomics of (3) count integers (histogram bins, list slots whose order the sort erases): the result does not depend on
// their arrival order.  No floating-point atomics anywhere.
//
// The pose gate (rpg_retrieve_cosine_gated_f32; pose_gate.h) is a second instantiation of (3): with a finite prior pose, query g's
// select workgroup first counts the allowed rows inside the gate -- one more sweep over m, ahead of the key-writing pass -- and,
// when they cover its largest rank, gives the rows outside the key of an excluded row.  Null gate pointers launch the
// instantiation without any of it.
//
// Scene scopes (rpg_retrieve_cosine_scoped_f32): a map that holds several scenes back to back gives every query a row range
// [lo, hi) = its scene's rows.  The rows outside rank as rows of the query's own group do -- not at all -- so the plain entry with
// an emulated group array is an exact oracle; what the scope adds is that they cost nothing: a dot workgroup whose 16 rows lie
// outside the scope of every query of its chunk returns before it loads a database byte, a workgroup that computes stores only
// the (query, row) pairs inside a scope, and every sweep of the select kernel runs over [lo, hi) alone (so it never reads a
// product that was not written).  The column slices stay a function of (m, d) of the whole map: the bits of a similarity do not
// depend on whether the call was scoped.  Null scope pointers launch the instantiations without any of it.
//
// Finding the scene (rpg_retrieve_cosine_elect_f32): a query that is not told its scene elects it.  Its products are computed
// against every row (the unscoped dot instantiation when every query elects; otherwise a scoped one in which an electing query's
// range is [0, m)), and retrieve_vote_kernel, a launch of its own between (2) and (3), one workgroup per query, reads them
// without writing them: unfiltered keys of all m rows go to a workspace region of their own, the same radix select takes the
// vote_top best (key, row) pairs, each finds its scene by binary search in scene_first, and the scene with the most voters -- the
// best-placed voter's among tied ones -- goes into q_scene.  Then (3) is the scoped selection as it stands, on that q_scene.
// With RPG_ELECT_LOST a one-thread-per-query mark launch ahead of (2) writes -1 into q_scene where the prior is not finite, so
// that every kernel of the call decides "elects" by the same test, q_scene[g] == -1.
#include "rpg_common.h"
#include "pose_gate.h"

#include <float.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RT_NT = 256;            // dot kernel: 4 waves
constexpr int RT_ROWS = 16;           // database rows per workgroup (one MFMA tile column block)
constexpr int RT_BLK = 64;            // columns per wave step: 4 float4 per lane
constexpr int RT_QCHUNK = 64;         // queries per workgroup (grid.z chunks beyond that re-read the database)
constexpr int RS_NT = 1024;           // select kernel
constexpr int R_MAX = 512;            // largest rank + 1 the select kernel serves
constexpr int K_MAX = 64;
constexpr int NORM_NT = 256;
constexpr uint32_t KEY_NONFINITE = 0xFFFFFFFEu;
constexpr uint32_t KEY_EXCLUDED = 0xFFFFFFFFu;

// ---- 1 / |row| ------------------------------------------------------------------------------------------------------------
// One workgroup per row (grid-strided).  Lane-strided float4 partial sums, then a shuffle tree per wave and the four wave sums
// added in wave order: the same order for every row.  A zero row gives 0 (similarity 0, sklearn's normalize), NaN stays NaN.
__global__ __launch_bounds__(NORM_NT) void row_inv_norms_kernel(const float4* __restrict__ x, int64_t rows, int d4,
                                                                float* __restrict__ inv) {
    __shared__ float wsum[NORM_NT / 64];
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const float4* src = x + r * d4;
        float s = 0.f;
        for (int c = threadIdx.x; c < d4; c += NORM_NT) {
            const float4 v = src[c];
            s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            const float ss = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
            inv[r] = ss == 0.f ? 0.f : 1.f / sqrtf(ss);
        }
        __syncthreads();
    }
}

// ---- <q, d> ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 ld4_or_zero(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// ---- scene scopes ----------------------------------------------------------------------------------------------------------
struct ScopeOn {
    const int64_t* first;      // [n + 1]: scene s owns rows [first[s], first[s + 1])
    const int32_t* q_scene;    // [g]
    int n;
};
struct ScopeOff {};
template <bool SCOPED>
struct ScopeArgs { typedef ScopeOff type; };
template <>
struct ScopeArgs<true> { typedef ScopeOn type; };

// Rows [lo, hi) of query gi, clamped into [0, m] with hi >= lo whatever the two arrays hold; -> false (and an empty range) for a
// scene outside [0, n).
__device__ __forceinline__ bool scope_of(const ScopeOn& sc, int gi, int64_t m, int64_t* lo, int64_t* hi) {
    const int s = sc.q_scene[gi];
    if (s < 0 || s >= sc.n) {
        *lo = *hi = 0;
        return false;
    }
    int64_t a = sc.first[s], b = sc.first[s + 1];
    a = a < 0 ? 0 : (a > m ? m : a);
    b = b < a ? a : (b > m ? m : b);
    *lo = a;
    *hi = b;
    return true;
}

// A = queries (tile rows i), B = database rows (tile columns j).  Lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15];
// a lane's float4 at column 16 u + 4 (l >> 4) feeds four MFMAs (.x .y .z .w), so one wave step of 64 columns is 16 MFMAs per
// query tile, in a fixed column order.  D[i = 4 (l >> 4) + reg][j = l & 15].
// SCOPED: the chunk's scopes go to LDS first, and the workgroup returns when none of them meets its 16 rows.  ELECT (with
// SCOPED): a query with q_scene -1 votes over every row, so its range is [0, m).
template <int NQ, bool SCOPED, bool ELECT = false>
__global__ __launch_bounds__(RT_NT) void retrieve_dot_kernel(const float* __restrict__ q, const float* __restrict__ db, int g,
                                                             int64_t m, int d, int blocks_per_split,
                                                             float* __restrict__ part,
                                                             const typename ScopeArgs<SCOPED>::type sc) {
    __shared__ float red[RT_NT / 64][NQ][4][64];
    __shared__ int64_t s_lo[SCOPED ? RT_QCHUNK : 1], s_hi[SCOPED ? RT_QCHUNK : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, c4 = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * RT_ROWS;
    const int split = blockIdx.y;
    const int g0 = blockIdx.z * RT_QCHUNK;
    if constexpr (SCOPED) {
        int meets = 0;
        if (threadIdx.x < RT_QCHUNK) {
            int64_t lo = 0, hi = 0;
            const int gi = g0 + (int)threadIdx.x;
            if (gi < g) {
                if (ELECT && sc.q_scene[gi] == -1)
                    hi = m;
                else
                    scope_of(sc, gi, m, &lo, &hi);
            }
            s_lo[threadIdx.x] = lo;
            s_hi[threadIdx.x] = hi;
            meets = lo < m0 + RT_ROWS && hi > m0;         // (an empty range meets nothing)
        }
        if (!__syncthreads_or(meets)) return;             // uniform: no query of this chunk ranks any of these 16 rows
    }

    int64_t row = m0 + r16;
    if (row >= m) row = m - 1;                            // a tail tile reads a valid row again; its column is not stored
    const float* brow = db + row * d;                     // 64-bit row offset
    const float* arow[NQ];
    bool aok[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        const int gi = g0 + 16 * t + r16;
        aok[t] = gi < g;
        arow[t] = q + (int64_t)(aok[t] ? gi : 0) * d;
    }
    const int nblk = (d + RT_BLK - 1) / RT_BLK;
    const int b_begin = split * blocks_per_split;
    const int b_end = b_begin + blocks_per_split < nblk ? b_begin + blocks_per_split : nblk;

    f32x4 acc[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int b = b_begin + wave; b < b_end; b += RT_NT / 64) {
        const int col = b * RT_BLK + 4 * c4;
        float4 bv[4], av[NQ][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = col + 16 * u;
            const bool in = c < d;                        // d % 4 == 0: a float4 is inside or outside as a whole
            bv[u] = ld4_or_zero(brow + c, in);
#pragma unroll
            for (int t = 0; t < NQ; ++t) av[t][u] = ld4_or_zero(arow[t] + c, in && aok[t]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int t = 0; t < NQ; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][u].x, bv[u].x, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NQ; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][u].y, bv[u].y, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NQ; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][u].z, bv[u].z, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NQ; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][u].w, bv[u].w, acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < NQ; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][t][r][lane] = acc[t][r];
    __syncthreads();
    const int reg = threadIdx.x >> 6;                     // this thread sums (tile t, reg, lane) over the waves, in wave order
#pragma unroll
    for (int t = 0; t < NQ; ++t) {
        const float s = ((red[0][t][reg][lane] + red[1][t][reg][lane]) + red[2][t][reg][lane]) + red[3][t][reg][lane];
        const int gi = g0 + 16 * t + 4 * c4 + reg;
        const int64_t mm = m0 + r16;
        bool store = gi < g && mm < m;
        if constexpr (SCOPED) store = store && mm >= s_lo[gi - g0] && mm < s_hi[gi - g0];
        if (store) part[((int64_t)split * g + gi) * m + mm] = s;
    }
}

// ---- selection -------------------------------------------------------------------------------------------------------------
// Larger similarity -> smaller key; -0 and +0 share a key; NaN / inf order after every finite value.
__device__ __forceinline__ uint32_t sim_key(float s) {
    if (!(fabsf(s) <= FLT_MAX)) return KEY_NONFINITE;
    // -0 takes +0's key, by its bits.  (Not `s += 0.0f`: that add was contracted with the product that made s into one fma, and
    // the fma's single rounding of a negative product that underflows is -0 -- a key of its own, one below +0's.)
    uint32_t u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;
    const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;
}

__device__ __forceinline__ float key_sim(uint32_t key) {
    if (key >= KEY_NONFINITE) return __builtin_nanf("");
    const uint32_t asc = ~key;
    return __uint_as_float((asc & 0x80000000u) ? (asc & 0x7FFFFFFFu) : ~asc);
}

// ---- the pose gate of the selection ---------------------------------------------------------------------------------------------
struct GateOn {
    const double* db_gate;     // [m][7]
    const double* prior;       // [g][7]
    double r2, cos_half;
    int rot;
    int32_t* info;             // [g][2]
};
struct GateOff {};
template <bool GATED>
struct GateArgs { typedef GateOff type; };
template <>
struct GateArgs<true> { typedef GateOn type; };

constexpr int GATE_ROW = 7;                               // doubles per gate row
constexpr int GATE_UNROLL = 4;                            // rows a thread has in flight in a sweep over the gate rows

// GATED = false is the kernel as it was before the gate existed (an empty struct more in its arguments): rpg_retrieve_cosine_f32
// and the new entry point with null gate pointers launch that one.  SCOPED = false likewise: [lo, hi) is [0, m) at compile time.
template <bool GATED, bool SCOPED>
__global__ __launch_bounds__(RS_NT) void retrieve_select_kernel(float* __restrict__ part, int nsplit,
                                                                const float* __restrict__ q_inv, const float* __restrict__ db_inv,
                                                                const int64_t* __restrict__ q_group,
                                                                const int64_t* __restrict__ db_group,
                                                                const int32_t* __restrict__ ranks, int g, int k, int64_t m,
                                                                int64_t* __restrict__ nbrs, float* __restrict__ sims,
                                                                int32_t* __restrict__ status, const typename GateArgs<GATED>::type ga,
                                                                const typename ScopeArgs<SCOPED>::type sc) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long list[R_MAX];
    __shared__ int s_rank[K_MAX];
    __shared__ unsigned s_allowed, s_cnt, s_bucket, s_need;
    __shared__ int s_r;
    const int tid = threadIdx.x;
    const int gi = blockIdx.x;
    // slice 0 of this query's row becomes its keys, in place: element mm is read and written by the same thread in every pass
    uint32_t* keys = reinterpret_cast<uint32_t*>(part) + (int64_t)gi * m;

    if (tid == 0) {
        s_allowed = 0;
        s_cnt = 0;
    }
    __syncthreads();
    const int64_t qg = q_group ? q_group[gi] : -1;
    const float qi = q_inv[gi];
    // the rows this query ranks: every sweep below runs over [lo, hi) (uniform over the workgroup)
    int64_t lo = 0, hi = m;
    bool scene_ok = true;
    if constexpr (SCOPED) scene_ok = scope_of(sc, gi, m, &lo, &hi);
    // similarity -> key of row mm, or KEY_EXCLUDED for a row the query does not rank; -> whether it is ranked
    auto write_key = [&](int64_t mm, bool allowed) {
        float dot = part[(int64_t)gi * m + mm];
        for (int s = 1; s < nsplit; ++s) dot += part[((int64_t)s * g + gi) * m + mm];          // slice order
        const float sim = dot * qi * db_inv[mm];
        keys[mm] = allowed ? sim_key(sim) : KEY_EXCLUDED;
    };
    bool gated = false;
    if constexpr (GATED) {
        // state 1 = no prior (a non-finite component), 0 = gated, 2 = fewer allowed rows inside than the largest rank needs: ranked
        // by the groups alone.  Every branch here is uniform over the workgroup.
        __shared__ unsigned s_inside;
        double p[GATE_ROW];
        for (int i = 0; i < GATE_ROW; ++i) p[i] = ga.prior[(int64_t)gi * GATE_ROW + i];
        // One sweep over the gate rows: body(mm, inside) for this thread's rows mm = tid, tid + RS_NT, ... (the rows whose keys it
        // owns).  The map's 56 bytes per row come from beyond the L2 and one workgroup has little else to hide that latency with,
        // so a thread loads GATE_UNROLL rows before it judges the first (a row past the end reads row `base` again, unused).
        auto sweep = [&](auto&& body) {
            for (int64_t base = lo + tid; base < hi; base += (int64_t)GATE_UNROLL * RS_NT) {
                double r[GATE_UNROLL][GATE_ROW];
#pragma unroll
                for (int u = 0; u < GATE_UNROLL; ++u) {
                    const int64_t mm = base + (int64_t)u * RS_NT;
                    const double* src = ga.db_gate + (mm < hi ? mm : base) * GATE_ROW;
#pragma unroll
                    for (int c = 0; c < GATE_ROW; ++c) r[u][c] = src[c];
                }
#pragma unroll
                for (int u = 0; u < GATE_UNROLL; ++u) {
                    const int64_t mm = base + (int64_t)u * RS_NT;
                    if (mm < hi) body(mm, rpg::pose_gate_inside(r[u], p, ga.r2, ga.cos_half, ga.rot != 0));
                }
            }
        };
        int state = 1;
        unsigned inside = 0;
        if (rpg::pose_gate_finite7(p)) {
            if (tid == 0) s_inside = 0;
            __syncthreads();
            unsigned local = 0;
            sweep([&](int64_t mm, bool in) { local += in && !(qg != -1 && db_group[mm] == qg); });
            if (local) atomicAdd(&s_inside, local);
            __syncthreads();
            inside = s_inside;
            int64_t need = (int64_t)ranks[(int64_t)gi * k] + 1;
            for (int j = 1; j < k; ++j) {
                const int64_t r = (int64_t)ranks[(int64_t)gi * k + j] + 1;
                need = r > need ? r : need;
            }
            gated = (int64_t)inside >= need;
            state = gated ? 0 : 2;
        }
        if (tid == 0) {
            ga.info[2 * (int64_t)gi] = state;
            ga.info[2 * (int64_t)gi + 1] = (int32_t)inside;
        }
        if (gated) {                                      // the key-writing pass of a gated query: the rows outside are excluded
            unsigned local = 0;
            sweep([&](int64_t mm, bool in) {
                const bool allowed = in && !(qg != -1 && db_group[mm] == qg);
                write_key(mm, allowed);
                local += allowed;
            });
            if (local) atomicAdd(&s_allowed, local);
        }
    }
    if (!gated) {
        unsigned local = 0;
        for (int64_t mm = lo + tid; mm < hi; mm += RS_NT) {
            const bool allowed = !(qg != -1 && db_group[mm] == qg);
            write_key(mm, allowed);
            local += allowed;
        }
        if (local) atomicAdd(&s_allowed, local);
    }
    __syncthreads();
    if (tid == 0) {
        // ranks of this query: each clamped below min(allowed rows, R_MAX); bad entries and a non-ascending row are counted
        const unsigned n_allowed = s_allowed;
        const int lim = (int)(n_allowed < (unsigned)R_MAX ? n_allowed : (unsigned)R_MAX);
        int bad = 0, top = -1, prev = 0;
        bool ascending = true;
        for (int j = 0; j < k; ++j) {
            const int raw = ranks[(int64_t)gi * k + j];
            if (j > 0 && raw <= prev) ascending = false;
            prev = raw;
            int r = raw;
            if (r < 0 || r >= lim) {
                ++bad;
                r = r < 0 ? 0 : lim - 1;
                if (r < 0) r = 0;
            }
            s_rank[j] = r;
            if (r > top) top = r;
        }
        if (!ascending) ++bad;
        if (!scene_ok) bad = 1;                           // a scene that does not exist: counted once, nothing ranked
        if (bad) atomicAdd(status, bad);
        s_r = lim > 0 ? top + 1 : 0;
    }
    __syncthreads();
    const int R = s_r;
    if (R == 0) {                                         // no allowed row: nothing to pick, row 0 keeps the output inside [0, m)
        if (tid < k) {
            nbrs[(int64_t)gi * k + tid] = 0;
            if (sims) sims[(int64_t)gi * k + tid] = __builtin_nanf("");
        }
        return;
    }

    // radix select of the R-th smallest (key << 32 | row): the pairs are distinct, so the last digit leaves exactly one
    unsigned long long prefix = 0, mask = 0;
    unsigned need = (unsigned)R;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (shift < 32 && ((unsigned long long)(hi - 1) >> shift) == 0) {     // every row index has digit 0 here (R > 0: hi >= 1)
            mask |= 0xFFull << shift;
            continue;
        }
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int64_t mm = lo + tid; mm < hi; mm += RS_NT) {
            const unsigned long long comp = ((unsigned long long)keys[mm] << 32) | (unsigned long long)mm;
            if ((comp & mask) == prefix) atomicAdd(&hist[(unsigned)(comp >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned cum = 0;
            int b = 0;
            for (; b < 255; ++b) {
                const unsigned h = hist[b];
                if (cum + h >= need) break;
                cum += h;
            }
            s_bucket = (unsigned)b;
            s_need = need - cum;
        }
        __syncthreads();
        prefix |= (unsigned long long)s_bucket << shift;
        mask |= 0xFFull << shift;
        need = s_need;
    }
    // collect the R pairs <= the threshold (slot order is arbitrary: the sort below fixes it), pad, sort ascending
    if (tid < R_MAX) list[tid] = ~0ull;
    __syncthreads();
    for (int64_t mm = lo + tid; mm < hi; mm += RS_NT) {
        const unsigned long long comp = ((unsigned long long)keys[mm] << 32) | (unsigned long long)mm;
        if (comp <= prefix) {
            const unsigned slot = atomicAdd(&s_cnt, 1u);
            if (slot < (unsigned)R_MAX) list[slot] = comp;
        }
    }
    for (int size = 2; size <= R_MAX; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            if (tid < R_MAX / 2) {
                const int i = 2 * tid - (tid & (stride - 1));
                const int j = i + stride;
                const bool up = (i & size) == 0;
                const unsigned long long a = list[i], b = list[j];
                if ((a > b) == up) {
                    list[i] = b;
                    list[j] = a;
                }
            }
        }
    }
    __syncthreads();
    if (tid < k) {
        const unsigned long long comp = list[s_rank[tid]];
        int64_t row = (int64_t)(comp & 0xFFFFFFFFull);
        if (row >= m) row = m - 1;                        // (a padding entry cannot be reached: ranks are clamped below R)
        nbrs[(int64_t)gi * k + tid] = row;
        if (sims) sims[(int64_t)gi * k + tid] = key_sim((uint32_t)(comp >> 32));
    }
}

// ---- the vote ---------------------------------------------------------------------------------------------------------------------
constexpr int ELECT_ALL = 1, ELECT_LOST = 2;              // RPG_ELECT_ALL, RPG_ELECT_LOST

// RPG_ELECT_LOST, ahead of the dot launch: a query without a finite prior elects, which every later kernel reads as q_scene -1.
__global__ __launch_bounds__(NORM_NT) void retrieve_mark_lost_kernel(const double* __restrict__ prior, int g,
                                                                     int32_t* __restrict__ q_scene) {
    const int gi = blockIdx.x * NORM_NT + threadIdx.x;
    if (gi >= g) return;
    double p[GATE_ROW];
    for (int i = 0; i < GATE_ROW; ++i) p[i] = prior[(int64_t)gi * GATE_ROW + i];
    if (!rpg::pose_gate_finite7(p)) q_scene[gi] = -1;
}

// The scene that owns `row`, or -1: the last s with clamp(first[s]) <= row by binary search (boundaries that do not descend
// are what a map has; whatever they hold, s stays inside [0, n) and the owner is confirmed with the clamping of scope_of).
__device__ __forceinline__ int scene_of_row(const int64_t* __restrict__ first, int n, int64_t m, int64_t row) {
    auto clamped = [&](int s) {
        const int64_t a = first[s];
        return a < 0 ? 0 : (a > m ? m : a);
    };
    int lo = 0, hi = n;                                   // the answer is in [lo, hi); first[n] only bounds the last scene
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (clamped(mid) <= row)
            lo = mid;
        else
            hi = mid;
    }
    const int64_t a = clamped(lo);
    int64_t b = first[lo + 1];
    b = b < a ? a : (b > m ? m : b);
    return row >= a && row < b ? lo : -1;
}

// One workgroup per query, between the dot launch and the selection.  It reads `part` and never writes it (the selection turns
// slice 0 into keys in place afterwards): the keys of all m rows -- the sums of write_key, unfiltered -- go to `vkeys`, the
// radix select of the selection takes the V-th smallest (key << 32 | row), the V pairs are sorted in LDS, and the voters are
// counted per scene by comparing the V scenes with one another (no table of n counters, so n is unbounded).  The one LDS
// atomic that decides is an integer max.  all == 0: a query whose q_scene is not -1 is held, scene_info = (its scene, 0).
__global__ __launch_bounds__(RS_NT) void retrieve_vote_kernel(const float* __restrict__ part, int nsplit,
                                                              const float* __restrict__ q_inv, const float* __restrict__ db_inv,
                                                              int g, int64_t m, int vote_top, int all,
                                                              const int64_t* __restrict__ first, int n, uint32_t* __restrict__ vkeys,
                                                              int32_t* __restrict__ q_scene, int32_t* __restrict__ scene_info) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long list[K_MAX];
    __shared__ int s_scene[K_MAX];
    __shared__ unsigned s_cnt, s_bucket, s_need, s_best;
    const int tid = threadIdx.x;
    const int gi = blockIdx.x;
    if (!all) {                                           // uniform over the workgroup
        const int32_t held = q_scene[gi];
        if (held != -1) {
            if (tid == 0) {
                scene_info[2 * (int64_t)gi] = held;
                scene_info[2 * (int64_t)gi + 1] = 0;
            }
            return;
        }
    }
    uint32_t* keys = vkeys + (int64_t)gi * m;             // element mm is written and read by the same thread in every pass
    const float qi = q_inv[gi];
    for (int64_t mm = tid; mm < m; mm += RS_NT) {
        float dot = part[(int64_t)gi * m + mm];
        for (int s = 1; s < nsplit; ++s) dot += part[((int64_t)s * g + gi) * m + mm];          // slice order, as write_key
        const float sim = dot * qi * db_inv[mm];
        keys[mm] = sim_key(sim);
    }
    if (tid == 0) {
        s_cnt = 0;
        s_best = 0;
    }
    if (tid < K_MAX) {
        list[tid] = ~0ull;
        s_scene[tid] = -1;
    }
    // radix select of the V-th smallest pair (1 <= V <= m: it exists), as in retrieve_select_kernel
    unsigned long long prefix = 0, mask = 0;
    unsigned need = (unsigned)vote_top;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (shift < 32 && ((unsigned long long)(m - 1) >> shift) == 0) {
            mask |= 0xFFull << shift;
            continue;
        }
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int64_t mm = tid; mm < m; mm += RS_NT) {
            const unsigned long long comp = ((unsigned long long)keys[mm] << 32) | (unsigned long long)mm;
            if ((comp & mask) == prefix) atomicAdd(&hist[(unsigned)(comp >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            unsigned cum = 0;
            int b = 0;
            for (; b < 255; ++b) {
                const unsigned h = hist[b];
                if (cum + h >= need) break;
                cum += h;
            }
            s_bucket = (unsigned)b;
            s_need = need - cum;
        }
        __syncthreads();
        prefix |= (unsigned long long)s_bucket << shift;
        mask |= 0xFFull << shift;
        need = s_need;
    }
    __syncthreads();                                      // (every digit skipped, m == 1: the initialisation above still lands)
    for (int64_t mm = tid; mm < m; mm += RS_NT) {
        const unsigned long long comp = ((unsigned long long)keys[mm] << 32) | (unsigned long long)mm;
        if (comp <= prefix) {
            const unsigned slot = atomicAdd(&s_cnt, 1u);
            if (slot < (unsigned)K_MAX) list[slot] = comp;
        }
    }
    for (int size = 2; size <= K_MAX; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            if (tid < K_MAX / 2) {
                const int i = 2 * tid - (tid & (stride - 1));
                const int j = i + stride;
                const bool up = (i & size) == 0;
                const unsigned long long a = list[i], b = list[j];
                if ((a > b) == up) {
                    list[i] = b;
                    list[j] = a;
                }
            }
        }
    }
    __syncthreads();
    // voter tid (position tid of the order) finds its scene; then counts the voters of that scene and the best-placed of them
    if (tid < vote_top && list[tid] != ~0ull) {
        int64_t row = (int64_t)(list[tid] & 0xFFFFFFFFull);
        if (row >= m) row = m - 1;
        s_scene[tid] = scene_of_row(first, n, m, row);
    }
    __syncthreads();
    if (tid < vote_top && s_scene[tid] >= 0) {
        const int mine = s_scene[tid];
        unsigned votes = 0;
        int best = K_MAX - 1;
        for (int i = K_MAX - 1; i >= 0; --i)
            if (s_scene[i] == mine) {
                ++votes;
                best = i;
            }
        atomicMax(&s_best, votes * (unsigned)K_MAX + (unsigned)(K_MAX - 1 - best));       // most votes, then the earliest position
    }
    __syncthreads();
    if (tid == 0) {
        const unsigned best = s_best;
        const int32_t votes = (int32_t)(best / (unsigned)K_MAX);
        const int32_t scene = votes ? s_scene[K_MAX - 1 - (int)(best % (unsigned)K_MAX)] : -1;
        q_scene[gi] = scene;
        scene_info[2 * (int64_t)gi] = scene;
        scene_info[2 * (int64_t)gi + 1] = votes;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Column slices of the dot kernel: enough workgroups to keep every CU streaming when the map has few 16-row tiles, at least 8
// column blocks per slice.  A function of (m, d) ONLY: the slice count is part of the summation order.
void split_plan(int64_t m, int d, int* nsplit, int* blocks_per_split) {
    const int64_t tiles = (m + RT_ROWS - 1) / RT_ROWS;
    const int nblk = (d + RT_BLK - 1) / RT_BLK;
    int64_t s = (1024 + tiles - 1) / tiles;
    const int cap = nblk / 8 < 1 ? 1 : nblk / 8;
    if (s > cap) s = cap;
    if (s > 16) s = 16;
    if (s < 1) s = 1;
    const int bps = (int)((nblk + s - 1) / s);
    *blocks_per_split = bps;
    *nsplit = (nblk + bps - 1) / bps;
}

struct WsLayout {
    size_t q_inv, db_inv, part, total;
};

WsLayout ws_layout(int g, int64_t m, int d) {
    int ns, bps;
    split_plan(m, d, &ns, &bps);
    WsLayout w;
    w.q_inv = 0;
    w.db_inv = round_up((size_t)g * sizeof(float), 256);
    w.part = w.db_inv + round_up((size_t)m * sizeof(float), 256);
    w.total = w.part + round_up((size_t)ns * (size_t)g * (size_t)m * sizeof(float), 256);
    return w;
}

int launch_inv_norms(const float* x, int64_t rows, int d, float* inv, hipStream_t s) {
    const int grid = (int)(rows < 65536 ? rows : 65536);
    hipLaunchKernelGGL(row_inv_norms_kernel, dim3(grid), dim3(NORM_NT), 0, s, reinterpret_cast<const float4*>(x), rows, d / 4, inv);
    RPG_CHECK_LAUNCH("row_inv_norms");
    return RPG_OK;
}

// Query tiling of the dot kernel: chunks of RT_QCHUNK queries (grid.z), and the 16-query tiles of the fullest chunk, which pick
// the NQ instantiation (1, 2, or 4 for three and four tiles).
int query_chunks(int g) { return (g + RT_QCHUNK - 1) / RT_QCHUNK; }
int query_tiles(int g) { return ((g < RT_QCHUNK ? g : RT_QCHUNK) + 15) / 16; }

template <bool SCOPED, bool ELECT>
int launch_dot(const float* q, const float* db, int g, int64_t m, int d, float* part, const typename ScopeArgs<SCOPED>::type sc,
               hipStream_t s) {
    int ns, bps;
    split_plan(m, d, &ns, &bps);
    const dim3 grid((unsigned)((m + RT_ROWS - 1) / RT_ROWS), (unsigned)ns, (unsigned)query_chunks(g));
    const int tiles = query_tiles(g);
    if (tiles <= 1)
        hipLaunchKernelGGL((retrieve_dot_kernel<1, SCOPED, ELECT>), grid, dim3(RT_NT), 0, s, q, db, g, m, d, bps, part, sc);
    else if (tiles == 2)
        hipLaunchKernelGGL((retrieve_dot_kernel<2, SCOPED, ELECT>), grid, dim3(RT_NT), 0, s, q, db, g, m, d, bps, part, sc);
    else
        hipLaunchKernelGGL((retrieve_dot_kernel<4, SCOPED, ELECT>), grid, dim3(RT_NT), 0, s, q, db, g, m, d, bps, part, sc);
    RPG_CHECK_LAUNCH("retrieve_dot");
    return RPG_OK;
}

template <bool SCOPED>
int launch_select(const float* q_inv, const float* db_inv_norm, const int64_t* q_group, const int64_t* db_group,
                  const int32_t* ranks, int g, int k, int64_t m, int d, const double* db_gate, const double* prior, double r2,
                  double cos_half, int rot_gate, int32_t* gate_info, int64_t* neighbours, float* sims, float* part, int32_t* status,
                  const typename ScopeArgs<SCOPED>::type sc, hipStream_t s) {
    int ns, bps;
    split_plan(m, d, &ns, &bps);
    if (db_gate) {
        const GateOn ga = {db_gate, prior, r2, cos_half, rot_gate, gate_info};
        hipLaunchKernelGGL((retrieve_select_kernel<true, SCOPED>), dim3(g), dim3(RS_NT), 0, s, part, ns, q_inv, db_inv_norm, q_group,
                           db_group, ranks, g, k, m, neighbours, sims, status, ga, sc);
    } else {
        hipLaunchKernelGGL((retrieve_select_kernel<false, SCOPED>), dim3(g), dim3(RS_NT), 0, s, part, ns, q_inv, db_inv_norm, q_group,
                           db_group, ranks, g, k, m, neighbours, sims, status, GateOff{}, sc);
    }
    RPG_CHECK_LAUNCH("retrieve_select");
    return RPG_OK;
}

template <bool SCOPED>
int launch_dot_select(const float* q, const float* db, const float* q_inv, const float* db_inv_norm, const int64_t* q_group,
                      const int64_t* db_group, const int32_t* ranks, int g, int k, int64_t m, int d, const double* db_gate,
                      const double* prior, double r2, double cos_half, int rot_gate, int32_t* gate_info, int64_t* neighbours,
                      float* sims, float* part, int32_t* status, const typename ScopeArgs<SCOPED>::type sc, hipStream_t s) {
    const int rc = launch_dot<SCOPED, false>(q, db, g, m, d, part, sc, s);
    if (rc != RPG_OK) return rc;
    return launch_select<SCOPED>(q_inv, db_inv_norm, q_group, db_group, ranks, g, k, m, d, db_gate, prior, r2, cos_half, rot_gate,
                                 gate_info, neighbours, sims, part, status, sc, s);
}

// What every retrieval entry refuses before a launch: the shapes and alignments, the gate's three pointers together or not at
// all with a radius that is a number, the scopes' two pointers together or not at all with at least one scene.
bool retrieve_args_ok(const float* q, const float* db, const float* db_inv_norm, const int64_t* q_group, const int64_t* db_group,
                      const int32_t* ranks, int g, int k, int64_t m, int d, const double* db_gate, const double* prior, double r2,
                      double cos_half, const int32_t* gate_info, const int64_t* scene_first, const int32_t* q_scene, int n_scenes,
                      const int64_t* neighbours, const float* sims, const void* workspace, const int32_t* status) {
    if (!q || !db || !ranks || !neighbours || !workspace || !status || g < 1 || k < 1 || k > K_MAX || m < k ||
        m >= ((int64_t)1 << 31) || d <= 0 || (d & 3) || !rpg::aligned16(q) || !rpg::aligned16(db) || !rpg::aligned16(workspace) ||
        ((q_group == nullptr) != (db_group == nullptr)) || (reinterpret_cast<uintptr_t>(neighbours) & 7u) ||
        (reinterpret_cast<uintptr_t>(q_group) & 7u) || (reinterpret_cast<uintptr_t>(db_group) & 7u) ||
        (reinterpret_cast<uintptr_t>(ranks) & 3u) || (reinterpret_cast<uintptr_t>(status) & 3u) ||
        (reinterpret_cast<uintptr_t>(sims) & 3u) || (reinterpret_cast<uintptr_t>(db_inv_norm) & 3u) ||
        (g + RT_QCHUNK - 1) / RT_QCHUNK > 65535)
        return false;
    if ((db_gate == nullptr) != (prior == nullptr) || (db_gate == nullptr) != (gate_info == nullptr) ||
        (reinterpret_cast<uintptr_t>(db_gate) & 7u) || (reinterpret_cast<uintptr_t>(prior) & 7u) ||
        (reinterpret_cast<uintptr_t>(gate_info) & 3u) || (db_gate && (!(r2 >= 0.0) || cos_half != cos_half)))
        return false;
    if ((scene_first == nullptr) != (q_scene == nullptr) || (reinterpret_cast<uintptr_t>(scene_first) & 7u) ||
        (reinterpret_cast<uintptr_t>(q_scene) & 3u) || (scene_first && n_scenes < 1))
        return false;
    return true;
}

// The electing call's workspace: the scoped call's, then the vote's keys uint32 [g][m].
struct ElectLayout {
    WsLayout w;
    size_t vkeys, total;
};

ElectLayout elect_layout(int g, int64_t m, int d) {
    ElectLayout e;
    e.w = ws_layout(g, m, d);
    e.vkeys = e.w.total;
    e.total = e.vkeys + round_up((size_t)g * (size_t)m * sizeof(uint32_t), 256);
    return e;
}

}  // namespace

extern "C" int rpg_retrieve_max_rank(void) { return R_MAX; }

extern "C" size_t rpg_retrieve_workspace_bytes(int g, int64_t m, int d) {
    if (g <= 0 || m <= 0 || d <= 0) return 0;
    return ws_layout(g, m, d).total;
}

// HOST: what launch_dot would launch for (g, m, d), from split_plan and the tile rule it uses itself.  No launch.
extern "C" int rpg_retrieve_plan(int g, int64_t m, int d, int32_t out[4]) {
    if (!out || g < 1 || m < 1 || m >= ((int64_t)1 << 31) || d <= 0 || (d & 3)) return RPG_ERR_BAD_ARG;
    int ns, bps;
    split_plan(m, d, &ns, &bps);
    const int tiles = query_tiles(g);
    out[0] = ns;
    out[1] = bps;
    out[2] = tiles <= 1 ? 1 : (tiles == 2 ? 2 : 4);
    out[3] = query_chunks(g);
    return RPG_OK;
}

extern "C" int rpg_row_inv_norms_f32(const float* x, int64_t m, int d, float* inv_norm, void* stream) {
    if (!x || !inv_norm || m <= 0 || d <= 0 || (d & 3) || !rpg::aligned16(x) || (reinterpret_cast<uintptr_t>(inv_norm) & 3u))
        return RPG_ERR_BAD_ARG;
    return launch_inv_norms(x, m, d, inv_norm, rpg::as_stream(stream));
}

extern "C" int rpg_retrieve_cosine_scoped_f32(const float* q, const float* db, const float* db_inv_norm, const int64_t* q_group,
                                             const int64_t* db_group, const int32_t* ranks, int g, int k, int64_t m, int d,
                                             const double* db_gate, const double* prior, double r2, double cos_half, int rot_gate,
                                             int32_t* gate_info, const int64_t* scene_first, const int32_t* q_scene, int n_scenes,
                                             int64_t* neighbours, float* sims, void* workspace, size_t workspace_bytes,
                                             int32_t* status, void* stream) {
    if (!retrieve_args_ok(q, db, db_inv_norm, q_group, db_group, ranks, g, k, m, d, db_gate, prior, r2, cos_half, gate_info,
                          scene_first, q_scene, n_scenes, neighbours, sims, workspace, status))
        return RPG_ERR_BAD_ARG;
    const WsLayout w = ws_layout(g, m, d);
    if (workspace_bytes < w.total) return RPG_ERR_WORKSPACE;
    hipStream_t s = rpg::as_stream(stream);
    char* base = static_cast<char*>(workspace);
    float* q_inv = reinterpret_cast<float*>(base + w.q_inv);
    float* part = reinterpret_cast<float*>(base + w.part);
    int rc = launch_inv_norms(q, g, d, q_inv, s);
    if (rc != RPG_OK) return rc;
    if (!db_inv_norm) {
        float* db_inv = reinterpret_cast<float*>(base + w.db_inv);
        rc = launch_inv_norms(db, m, d, db_inv, s);
        if (rc != RPG_OK) return rc;
        db_inv_norm = db_inv;
    }
    if (scene_first)
        return launch_dot_select<true>(q, db, q_inv, db_inv_norm, q_group, db_group, ranks, g, k, m, d, db_gate, prior, r2, cos_half,
                                       rot_gate, gate_info, neighbours, sims, part, status, ScopeOn{scene_first, q_scene, n_scenes}, s);
    return launch_dot_select<false>(q, db, q_inv, db_inv_norm, q_group, db_group, ranks, g, k, m, d, db_gate, prior, r2, cos_half,
                                    rot_gate, gate_info, neighbours, sims, part, status, ScopeOff{}, s);
}

extern "C" size_t rpg_retrieve_elect_workspace_bytes(int g, int64_t m, int d) {
    if (g <= 0 || m <= 0 || d <= 0) return 0;
    return elect_layout(g, m, d).total;
}

extern "C" int rpg_retrieve_cosine_elect_f32(const float* q, const float* db, const float* db_inv_norm, const int64_t* q_group,
                                            const int64_t* db_group, const int32_t* ranks, int g, int k, int64_t m, int d,
                                            const double* db_gate, const double* prior, double r2, double cos_half, int rot_gate,
                                            int32_t* gate_info, const int64_t* scene_first, int32_t* q_scene, int n_scenes,
                                            int vote_top, int elect_mode, int32_t* scene_info, int64_t* neighbours, float* sims,
                                            void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
    if (!scene_first || !q_scene || !scene_info || (reinterpret_cast<uintptr_t>(scene_info) & 3u) || vote_top < 1 ||
        vote_top > K_MAX || vote_top > m || (elect_mode != ELECT_ALL && elect_mode != ELECT_LOST) ||
        !retrieve_args_ok(q, db, db_inv_norm, q_group, db_group, ranks, g, k, m, d, db_gate, prior, r2, cos_half, gate_info,
                          scene_first, q_scene, n_scenes, neighbours, sims, workspace, status))
        return RPG_ERR_BAD_ARG;
    const ElectLayout e = elect_layout(g, m, d);
    if (workspace_bytes < e.total) return RPG_ERR_WORKSPACE;
    hipStream_t s = rpg::as_stream(stream);
    char* base = static_cast<char*>(workspace);
    float* q_inv = reinterpret_cast<float*>(base + e.w.q_inv);
    float* part = reinterpret_cast<float*>(base + e.w.part);
    uint32_t* vkeys = reinterpret_cast<uint32_t*>(base + e.vkeys);
    int rc = launch_inv_norms(q, g, d, q_inv, s);
    if (rc != RPG_OK) return rc;
    if (!db_inv_norm) {
        float* db_inv = reinterpret_cast<float*>(base + e.w.db_inv);
        rc = launch_inv_norms(db, m, d, db_inv, s);
        if (rc != RPG_OK) return rc;
        db_inv_norm = db_inv;
    }
    const ScopeOn sc = {scene_first, q_scene, n_scenes};
    if (elect_mode == ELECT_ALL) {
        rc = launch_dot<false, false>(q, db, g, m, d, part, ScopeOff{}, s);
    } else {
        if (prior) {
            hipLaunchKernelGGL(retrieve_mark_lost_kernel, dim3((unsigned)((g + NORM_NT - 1) / NORM_NT)), dim3(NORM_NT), 0, s, prior, g,
                               q_scene);
            RPG_CHECK_LAUNCH("retrieve_mark_lost");
        }
        rc = launch_dot<true, true>(q, db, g, m, d, part, sc, s);
    }
    if (rc != RPG_OK) return rc;
    int ns, bps;
    split_plan(m, d, &ns, &bps);
    hipLaunchKernelGGL(retrieve_vote_kernel, dim3(g), dim3(RS_NT), 0, s, part, ns, q_inv, db_inv_norm, g, m, vote_top,
                       elect_mode == ELECT_ALL ? 1 : 0, scene_first, n_scenes, vkeys, q_scene, scene_info);
    RPG_CHECK_LAUNCH("retrieve_vote");
    return launch_select<true>(q_inv, db_inv_norm, q_group, db_group, ranks, g, k, m, d, db_gate, prior, r2, cos_half, rot_gate,
                               gate_info, neighbours, sims, part, status, sc, s);
}

extern "C" int rpg_retrieve_cosine_gated_f32(const float* q, const float* db, const float* db_inv_norm, const int64_t* q_group,
                                             const int64_t* db_group, const int32_t* ranks, int g, int k, int64_t m, int d,
                                             const double* db_gate, const double* prior, double r2, double cos_half, int rot_gate,
                                             int32_t* gate_info, int64_t* neighbours, float* sims, void* workspace,
                                             size_t workspace_bytes, int32_t* status, void* stream) {
    return rpg_retrieve_cosine_scoped_f32(q, db, db_inv_norm, q_group, db_group, ranks, g, k, m, d, db_gate, prior, r2, cos_half,
                                          rot_gate, gate_info, nullptr, nullptr, 0, neighbours, sims, workspace, workspace_bytes,
                                          status, stream);
}

extern "C" int rpg_retrieve_cosine_f32(const float* q, const float* db, const float* db_inv_norm, const int64_t* q_group,
                                       const int64_t* db_group, const int32_t* ranks, int g, int k, int64_t m, int d,
                                       int64_t* neighbours, float* sims, void* workspace, size_t workspace_bytes,
                                       int32_t* status, void* stream) {
    return rpg_retrieve_cosine_gated_f32(q, db, db_inv_norm, q_group, db_group, ranks, g, k, m, d, nullptr, nullptr, 0.0, 0.0, 0,
                                         nullptr, neighbours, sims, workspace, workspace_bytes, status, stream);
}
