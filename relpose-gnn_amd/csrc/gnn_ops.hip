// GNN-side kernels for gfx950 that are not GEMM shaped: edge-index preparation (CSR by target node),
// pair-feature gather, the AttentionBlock softmax core, scatter-mean aggregation and the 6-wide pose heads.
// All are HBM/LDS/VALU kernels: coalesced 16-byte-per-lane row reads, LDS broadcast of the small per-row
// vectors, wave64 shuffle reductions; no MFMA.
//
// Reference ops replaced (all under /root/reference/python/niantic/modules/):
//   posenet.py:999-1019 compute_edge_features; att.py:20-31; my_gnn_layer.py:279,301 (PyG propagate ->
//   torch_scatter scatter(reduce='mean')); posenet.py:1077-1091 (fc_xyz/fc_wpqr/fc_xyz_R/fc_wpqr_R).
#include "rpg_common.h"

namespace {

constexpr int NT = 256;

// ------------------------------------------------------------------------------------------------
// graph_prepare: one workgroup of 1024 lanes.  Counting sort of the edges by target node followed by a
// per-node insertion sort of the (short) segments, so that perm lists edge ids in ascending order per
// target: the summation order of torch_scatter's sequential CPU kernel, and a deterministic one.
// ------------------------------------------------------------------------------------------------
constexpr int GP_NT = 1024;

__global__ __launch_bounds__(GP_NT) void graph_prepare_kernel(const int64_t* __restrict__ esrc,
                                                              const int64_t* __restrict__ edst, int64_t node_off, int E,
                                                              int N, int64_t* __restrict__ ends, int* rowptr, int* cursor,
                                                              int* perm, int* status) {
    __shared__ int s_scan[GP_NT];
    __shared__ int s_bad;
    __shared__ int s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) { s_bad = 0; s_carry = 0; }
    for (int i = tid; i <= N; i += GP_NT) rowptr[i] = 0;
    for (int i = tid; i < N; i += GP_NT) cursor[i] = 0;
    __syncthreads();

    // pass 1: sanitised endpoints, min/max endpoints, in-degree histogram (rowptr[t+1] += 1)
    int bad = 0;
    for (int e = tid; e < E; e += GP_NT) {
        const int64_t s = esrc[e] - node_off, t = edst[e] - node_off;
        const bool ok = ((uint64_t)s < (uint64_t)N) && ((uint64_t)t < (uint64_t)N);
        const int64_t sc = s < 0 ? 0 : (s >= N ? N - 1 : s);
        const int64_t tc = t < 0 ? 0 : (t >= N ? N - 1 : t);
        ends[e] = sc;
        ends[(size_t)E + e] = tc;
        ends[2 * (size_t)E + e] = sc < tc ? sc : tc;
        ends[3 * (size_t)E + e] = sc < tc ? tc : sc;
        if (ok) atomicAdd(&rowptr[t + 1], 1);
        else ++bad;
    }
    if (bad) atomicAdd(&s_bad, bad);
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the histogram was built by L2 atomics

    // inclusive scan of rowptr[1..N] in chunks of 1024 (Hillis-Steele in LDS)
    for (int base = 1; base <= N; base += GP_NT) {
        const int i = base + tid;
        int v = (i <= N) ? rowptr[i] : 0;
        s_scan[tid] = v;
        __syncthreads();
        for (int off = 1; off < GP_NT; off <<= 1) {
            const int add = (tid >= off) ? s_scan[tid - off] : 0;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        const int carry = s_carry;
        if (i <= N) rowptr[i] = carry + s_scan[tid];
        __syncthreads();
        if (tid == GP_NT - 1) s_carry = carry + s_scan[tid];
        __syncthreads();
    }
    __syncthreads();

    // pass 2: claim a slot inside the target's segment (arbitrary order) ...
    for (int e = tid; e < E; e += GP_NT) {
        const int64_t s = esrc[e] - node_off, t = edst[e] - node_off;
        if (((uint64_t)s < (uint64_t)N) && ((uint64_t)t < (uint64_t)N)) {
            const int slot = atomicAdd(&cursor[t], 1);
            perm[rowptr[t] + slot] = e;
        }
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // ... then order every segment by edge id (segments are in-degree long: 7 for the FC-8 graphs)
    for (int v = tid; v < N; v += GP_NT) {
        const int b = rowptr[v], n = rowptr[v + 1] - b;
        for (int i = 1; i < n; ++i) {
            const int key = perm[b + i];
            int j = i - 1;
            while (j >= 0 && perm[b + j] > key) { perm[b + j + 1] = perm[b + j]; --j; }
            perm[b + j + 1] = key;
        }
    }
    if (tid == 0 && s_bad) atomicAdd(status, s_bad);     // accumulates: the host zeroes it when it wants a fresh count
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void edge_concat_kernel(const float4* __restrict__ x, const int64_t* __restrict__ ei,
                                                         int E, int d4, float4* __restrict__ out, long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int c = (int)(i % (2 * d4));
        const long e = i / (2 * d4);
        const int64_t s = ei[e], t = ei[(size_t)E + e];
        const int64_t node = (c < d4) ? (s < t ? s : t) : (s < t ? t : s);
        out[i] = x[node * d4 + (c < d4 ? c : c - d4)];
    }
}

// out[e] = relu(pq[lo[e]][0:d] + pq[hi[e]][d:2d] + bias): proj_edge after splitting its weight into the two node
// halves (W [x_lo, x_hi] = W_lo x_lo + W_hi x_hi, each product computed once per NODE instead of once per edge).
__global__ __launch_bounds__(NT) void gather_add2_relu_kernel(const float4* __restrict__ pq, const int64_t* __restrict__ lo,
                                                              const int64_t* __restrict__ hi, const float4* __restrict__ bias,
                                                              float4* __restrict__ out, int d4, long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int c = (int)(i % d4);
        const long e = i / d4;
        const float4 a = pq[(size_t)lo[e] * (2 * d4) + c];
        const float4 b = pq[(size_t)hi[e] * (2 * d4) + d4 + c];
        const float4 bb = bias[c];
        float4 v;
        v.x = rpg::relu(a.x + b.x + bb.x); v.y = rpg::relu(a.y + b.y + bb.y);
        v.z = rpg::relu(a.z + b.z + bb.z); v.w = rpg::relu(a.w + b.w + bb.w);
        out[i] = v;
    }
}

__global__ __launch_bounds__(NT) void relu_inplace_kernel(float4* __restrict__ x, long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        float4 v = x[i];
        v = rpg::relu4(v);
        x[i] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// AttentionBlock core.  One workgroup per row; theta and g are staged in LDS and read back as
// broadcast float4; lane i owns output channel i:  y_i = sum_j exp(phi_i theta_j - m_i) g_j / sum_j exp(.)
// with m_i = max_j(phi_i theta_j) = phi_i * (phi_i >= 0 ? max theta : min theta) (rounding is monotone).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void attention_rows_kernel(const float* __restrict__ gtp, int C, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float sm[];   // theta[C], g[C], red[8]
    float* s_th = sm;
    float* s_g = sm + C;
    float* s_red = sm + 2 * C;
    const int tid = threadIdx.x;
    const float* row = gtp + (size_t)blockIdx.x * 3 * C;
    float tmax = -INFINITY, tmin = INFINITY;
    for (int j = tid; j < C; j += NT) {
        const float th = row[C + j];
        s_th[j] = th;
        s_g[j] = row[j];
        tmax = fmaxf(tmax, th);
        tmin = fminf(tmin, th);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        tmax = fmaxf(tmax, __shfl_xor(tmax, off));
        tmin = fminf(tmin, __shfl_xor(tmin, off));
    }
    if ((tid & 63) == 0) { s_red[tid >> 6] = tmax; s_red[4 + (tid >> 6)] = tmin; }
    __syncthreads();
    tmax = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    tmin = fminf(fminf(s_red[4], s_red[5]), fminf(s_red[6], s_red[7]));

    for (int i = tid; i < C; i += NT) {
        const float phi = row[2 * C + i];
        const float m = __fmul_rn(phi, (phi >= 0.f ? tmax : tmin));
        float den = 0.f, num = 0.f;
        for (int j = 0; j < C; j += 4) {
            const float4 th = *reinterpret_cast<const float4*>(&s_th[j]);
            const float4 g = *reinterpret_cast<const float4*>(&s_g[j]);
            // product and subtraction rounded separately (no FMA contraction), as the reference's
            // matmul-then-softmax does, so the arg-max term is exactly exp(0)
            const float p0 = __expf(__fsub_rn(__fmul_rn(phi, th.x), m)), p1 = __expf(__fsub_rn(__fmul_rn(phi, th.y), m));
            const float p2 = __expf(__fsub_rn(__fmul_rn(phi, th.z), m)), p3 = __expf(__fsub_rn(__fmul_rn(phi, th.w), m));
            den += p0; num += p0 * g.x;
            den += p1; num += p1 * g.y;
            den += p2; num += p2 * g.z;
            den += p3; num += p3 * g.w;
        }
        y[(size_t)blockIdx.x * C + i] = num / den;
    }
}

// ------------------------------------------------------------------------------------------------
// AttentionBlock core + mean aggregation in one kernel (the message path of my_gnn_layer.py:304-307 followed by PyG's
// aggr='mean', :279,301).  The reference computes, per edge, att = W y + b + msg with y = the attention rows of above, and
// then averages att over the edges into a node.  W y + b + msg is linear in (y, msg), so the mean commutes with it:
//   mean_e(att) = W mean_e(y) + (b + mean_e(msg))            (summation order changes only)
// and the E-row Linear att.W becomes an N-row one.  This kernel produces the two means for a node directly:
//   ybar[v][i] = (1/cnt) sum_{e -> v} y_e[i],   mbar[v][:] = (1/cnt) sum_{e -> v} msg[e][:] (+ bias if cnt > 0)
// (mbar without bias is BIT-EXACT scatter-mean of msg: ascending edge order, the order of torch_scatter's CPU kernel), so
// neither the per-edge y [E][C], nor att [E][D], nor a separate scatter launch exist any more.
//
// Round 5 form.  The kernel is bound by its 65,536 exponentials per edge (v_exp_f32 is quarter rate), so everything else is
// taken off the vector unit's critical path: workgroup (node v, 64-channel quarter s) = 8 waves, and the node's incoming
// EDGES ARE PROCESSED IN PARALLEL, ONE PER WAVE (round 4 walked them serially with three workgroup barriers each).  Lane = output
// channel i; the wave's theta / g rows are wave-uniform, so they come through the SCALAR unit (s_load from the read-only
// gtp: no LDS staging, no barrier, one scalar operand per VALU instruction).  Per (i, j): one v_fma (phi_i log2e theta_j -
// m_i log2e, single rounding), v_exp_f32, v_add, v_fma.  m_i = max_j(phi_i theta_j) = phi_i * (phi_i >= 0 ? max theta :
// min theta); softmax is shift invariant, so any m_i close to the maximum does.  The per-edge rows y_e meet in LDS and wave 0
// adds them in ascending edge order (a node with more than 8 incoming edges: wave w takes edges w, w + 8, ... and the
// wave partials are added in wave order).  Threads 0 .. D/16/quarters - 1 also carry one float4 column of mbar, all of the
// node's message rows in flight at once.  An isolated node (cnt = 0) gives zeros, like scatter-mean.
// ------------------------------------------------------------------------------------------------
constexpr int AA_NT = 512, AA_W = AA_NT / 64;

// SPLIT_BIAS (the mean-first form, rpg_attention_aggregate_hidden_f32): `msg` holds the message MLP's HIDDEN rows, whose mean goes
// out without the bias, and the bias goes to a row of its own, `res` = bias where cnt > 0, zeros otherwise: the node-level Linear
// that follows (mlp.2 | att.W on [mbar ; ybar]) takes it as its residual operand, so an isolated node's aggregate stays exactly 0.
template <bool SPLIT_BIAS>
__global__ __launch_bounds__(AA_NT) void attention_aggregate_kernel(const float* __restrict__ gtp, const float4* __restrict__ msg,
                                                                    const int* __restrict__ rowptr, const int* __restrict__ perm,
                                                                    const float4* __restrict__ bias, int C, int d4,
                                                                    float* __restrict__ ybar, float4* __restrict__ mbar,
                                                                    float4* __restrict__ res) {
    __shared__ float s_y[AA_W][64];
    const int v = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = 64 * s + lane;                          // this lane's output channel (valid if < C)
    const int beg = rowptr[v], end = rowptr[v + 1];
    const int dq = (d4 + gridDim.y - 1) / gridDim.y;      // float4 columns of mbar per quarter
    const int mc = s * dq + tid;                          // this thread's mbar column (valid if tid < dq && mc < d4)
    const bool m_ok = tid < dq && mc < d4;
    constexpr float LOG2E = 1.4426950408889634f;

    // ---- mbar: ascending edge order, up to 8 rows in flight
    float4 macc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m_ok) {
        for (int p0 = beg; p0 < end; p0 += 8) {
            float4 mv[8];
#pragma unroll
            for (int t = 0; t < 8; ++t)
                mv[t] = (p0 + t < end) ? msg[(size_t)perm[p0 + t] * d4 + mc] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < 8; ++t)
                if (p0 + t < end) { macc.x += mv[t].x; macc.y += mv[t].y; macc.z += mv[t].z; macc.w += mv[t].w; }
        }
    }

    // ---- attention rows: wave w takes edges beg + w, beg + w + 8, ...
    float ysum = 0.f;
    for (int p = beg + wave; p < end; p += AA_W) {
        const int e = __builtin_amdgcn_readfirstlane(perm[p]);
        const float* __restrict__ row = gtp + (size_t)e * 3 * C;      // wave-uniform: g | theta | phi
        float tmax = -INFINITY, tmin = INFINITY;
        for (int j = 4 * lane; j < C; j += 256) {
            const float4 th = *reinterpret_cast<const float4*>(row + C + j);
            tmax = fmaxf(fmaxf(tmax, fmaxf(th.x, th.y)), fmaxf(th.z, th.w));
            tmin = fminf(fminf(tmin, fminf(th.x, th.y)), fminf(th.z, th.w));
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            tmax = fmaxf(tmax, __shfl_xor(tmax, off));
            tmin = fminf(tmin, __shfl_xor(tmin, off));
        }
        const float phi = (i < C) ? row[2 * C + i] : 0.f;
        const float pl = phi * LOG2E;
        const float nm = -(pl * (phi >= 0.f ? tmax : tmin));
        float den0 = 0.f, num0 = 0.f, den1 = 0.f, num1 = 0.f;
        const float* __restrict__ gr = row;
        const float* __restrict__ tr = row + C;
#pragma unroll 8
        for (int j = 0; j < C; j += 2) {
            const float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(pl, tr[j], nm));
            const float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(pl, tr[j + 1], nm));
            den0 += p0; num0 = __builtin_fmaf(p0, gr[j], num0);
            den1 += p1; num1 = __builtin_fmaf(p1, gr[j + 1], num1);
        }
        ysum += (num0 + num1) / (den0 + den1);
    }
    s_y[wave][lane] = ysum;
    __syncthreads();
    const int cnt = end - beg;
    const float dv = (float)(cnt > 0 ? cnt : 1);
    if (wave == 0 && i < C) {
        float y = s_y[0][lane];
#pragma unroll
        for (int w = 1; w < AA_W; ++w) y += s_y[w][lane];
        ybar[(size_t)v * C + i] = y / dv;
    }
    if (m_ok) {
        float4 o = make_float4(macc.x / dv, macc.y / dv, macc.z / dv, macc.w / dv);
        if constexpr (SPLIT_BIAS) {
            res[(size_t)v * d4 + mc] = cnt > 0 ? bias[mc] : make_float4(0.f, 0.f, 0.f, 0.f);
        } else if (bias && cnt > 0) {
            const float4 b = bias[mc];
            o.x += b.x; o.y += b.y; o.z += b.z; o.w += b.w;
        }
        mbar[(size_t)v * d4 + mc] = o;
    }
}

// ------------------------------------------------------------------------------------------------
// scatter-mean: one workgroup per (target node, 1024-column slab); every lane streams its float4 column of
// the node's incoming messages in ascending edge order (4 independent loads in flight) and divides by the
// in-degree.  Algorithmic bytes: E*D*4 (messages) + N*D*4 (output) + indices.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void scatter_mean_kernel(const float4* __restrict__ msg, const int* __restrict__ rowptr,
                                                          const int* __restrict__ perm, int d4, float4* __restrict__ out) {
    const int v = blockIdx.x;
    const int c = blockIdx.y * NT + threadIdx.x;
    if (c >= d4) return;
    const int beg = rowptr[v], end = rowptr[v + 1];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int p = beg;
    for (; p + 4 <= end; p += 4) {
        const float4 a = msg[(size_t)perm[p] * d4 + c];
        const float4 b = msg[(size_t)perm[p + 1] * d4 + c];
        const float4 cc = msg[(size_t)perm[p + 2] * d4 + c];
        const float4 dd = msg[(size_t)perm[p + 3] * d4 + c];
        acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
        acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
        acc.x += cc.x; acc.y += cc.y; acc.z += cc.z; acc.w += cc.w;
        acc.x += dd.x; acc.y += dd.y; acc.z += dd.z; acc.w += dd.w;
    }
    for (; p < end; ++p) {
        const float4 a = msg[(size_t)perm[p] * d4 + c];
        acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
    }
    const int cnt = end - beg;
    const float dv = (float)(cnt > 0 ? cnt : 1);
    out[(size_t)v * d4 + c] = make_float4(acc.x / dv, acc.y / dv, acc.z / dv, acc.w / dv);
}

// ------------------------------------------------------------------------------------------------
// pose heads: one wave per row, six dot products of length d, butterfly reduction over the 64 lanes.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void pose_heads_kernel(const float4* __restrict__ x, const float4* __restrict__ w6,
                                                        const float* __restrict__ b6, int R, int d4,
                                                        float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (row >= R) return;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float4* xr = x + (size_t)row * d4;
    for (int k = lane; k < d4; k += 64) {
        const float4 xv = xr[k];
#pragma unroll
        for (int o = 0; o < 6; ++o) {
            const float4 wv = w6[(size_t)o * d4 + k];
            acc[o] += xv.x * wv.x + xv.y * wv.y + xv.z * wv.z + xv.w * wv.w;
        }
    }
#pragma unroll
    for (int o = 0; o < 6; ++o)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[o] += __shfl_xor(acc[o], off);
    if (lane == 0) {
#pragma unroll
        for (int o = 0; o < 6; ++o) out[(size_t)row * 6 + o] = acc[o] + b6[o];
    }
}

// ------------------------------------------------------------------------------------------------
// kNN graph (torch_cluster.knn_graph(x, k, batch, loop=False), posenet.py:1043-1050): brute force per graph.
// One workgroup per query node i: its 4 waves take the candidates j of i's graph in turn and reduce
// sum_c (x_i[c] - x_j[c])^2 over the 64 lanes (float4 reads); lane 0 of wave 0 then picks the k+1 nearest by
// (distance, index) -- candidates in index order, strict '<', like torch_cluster's kernel -- and drops the self
// match (`row != col` mask).  Output: cand[i][0..k] (neighbour ids, -1 = unused), cnt[i].
// ------------------------------------------------------------------------------------------------
constexpr int KNN_MAX_GRAPH = 2048;   // nodes per graph (LDS distance row)
constexpr int KNN_MAX_K = 64;

__global__ __launch_bounds__(NT) void knn_candidates_kernel(const float* __restrict__ x, const int64_t* __restrict__ batch,
                                                            int n, int d4, int k, int* __restrict__ cand,
                                                            int* __restrict__ cnt, int* __restrict__ status) {
    __shared__ float s_dist[KNN_MAX_GRAPH];
    __shared__ int s_seg[2];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        int lo = 0, hi = n;
        if (batch) {            // nodes of one graph are contiguous (PyG batching): scan outwards from i
            const int64_t b = batch[i];
            lo = i; hi = i + 1;
            while (lo > 0 && batch[lo - 1] == b) --lo;
            while (hi < n && batch[hi] == b) ++hi;
        }
        s_seg[0] = lo; s_seg[1] = hi;
    }
    __syncthreads();
    const int lo = s_seg[0], hi = s_seg[1], m = hi - lo;
    if (m > KNN_MAX_GRAPH) {
        if (tid == 0) { atomicAdd(status, 1); cnt[i] = 0; }
        return;
    }
    const float4* xi = reinterpret_cast<const float4*>(x) + (size_t)i * d4;
    for (int j = lo + wave; j < hi; j += NT / 64) {
        const float4* xj = reinterpret_cast<const float4*>(x) + (size_t)j * d4;
        float acc = 0.f;
        for (int c = lane; c < d4; c += 64) {
            const float4 a = xi[c], b = xj[c];
            const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, dw = a.w - b.w;
            acc += dx * dx + dy * dy + dz * dz + dw * dw;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) s_dist[j - lo] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        // k+1 nearest (self included), insertion into a sorted list; strict '<' keeps the earlier index on ties
        float bd[KNN_MAX_K + 1];
        int bi[KNN_MAX_K + 1];
        const int kk = k + 1;
        int have = 0;
        for (int j = 0; j < m; ++j) {
            const float dj = s_dist[j];
            if (have < kk || dj < bd[have - 1]) {
                int p = have < kk ? have : kk - 1;
                while (p > 0 && dj < bd[p - 1]) { bd[p] = bd[p - 1]; bi[p] = bi[p - 1]; --p; }
                bd[p] = dj; bi[p] = lo + j;
                if (have < kk) ++have;
            }
        }
        int c = 0;
        for (int t = 0; t < have; ++t)
            if (bi[t] != i) cand[(size_t)i * kk + c++] = bi[t];
        for (int t = c; t < kk; ++t) cand[(size_t)i * kk + t] = -1;
        cnt[i] = c;
    }
}

// Compaction: edge e of node i goes to offset prefix(cnt)[i] + t; row 0 = neighbour (source), row 1 = i (target).
// Single workgroup (n up to 2^20), serial prefix per 1024-node chunk.
__global__ __launch_bounds__(GP_NT) void knn_compact_kernel(const int* __restrict__ cand, const int* __restrict__ cnt,
                                                            int n, int kk, int e_cap, int64_t* __restrict__ ei,
                                                            int* __restrict__ total) {
    __shared__ int s_scan[GP_NT];
    __shared__ int s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += GP_NT) {
        const int i = base + tid;
        const int c = (i < n) ? cnt[i] : 0;
        s_scan[tid] = c;
        __syncthreads();
        for (int off = 1; off < GP_NT; off <<= 1) {
            const int add = (tid >= off) ? s_scan[tid - off] : 0;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        const int start = s_carry + s_scan[tid] - c;
        if (i < n)
            for (int t = 0; t < c; ++t) {
                ei[start + t] = cand[(size_t)i * kk + t];
                ei[(size_t)e_cap + start + t] = i;
            }
        __syncthreads();
        if (tid == GP_NT - 1) s_carry += s_scan[tid];
        __syncthreads();
    }
    if (tid == 0) *total = s_carry;
}

// ------------------------------------------------------------------------------------------------
// kNN graph of g graphs of n_per nodes each, at fixed positions (rpg_knn_graph_uniform_f32): every node has k' = min(k, n_per - 1)
// incoming edges, so column (v k' + t) is known before anything runs and no count goes to the host.  The per-pair sum is
// knn_candidates_kernel's, operation for operation (lane c adds float4 columns c, c + 64, ..., then the xor tree 32..1), and so is
// the selection, so the neighbours and their order are that kernel's on every input.
// ------------------------------------------------------------------------------------------------
constexpr int KNN_SMALL = 64;         // nodes per graph up to which one workgroup holds the graph's whole distance matrix in LDS

__device__ __forceinline__ float knn_pair_dist(const float4* __restrict__ xi, const float4* __restrict__ xj, int d4, int lane) {
    float acc = 0.f;
    for (int c = lane; c < d4; c += 64) {
        const float4 a = xi[c], b = xj[c];
        const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z, dw = a.w - b.w;
        acc += dx * dx + dy * dy + dz * dz + dw * dw;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    return acc;
}

// Node v (id within its graph) of graph gi picks from its distance row (stride 1, m = n_per entries) like knn_candidates_kernel's
// thread 0 and writes its k' columns.  A list without the self match holds k' + 1 other nodes (the reference keeps them all): the
// first k' go out and the node is counted.
__device__ __forceinline__ void knn_uniform_select(const float* __restrict__ dist, int m, int v, int gi, int k, int kp,
                                                   int64_t node_offset, int64_t* __restrict__ src, int64_t* __restrict__ dst,
                                                   int64_t* __restrict__ q_src, int64_t* __restrict__ q_dst,
                                                   int* __restrict__ irregular) {
    float bd[KNN_MAX_K + 1];
    int bi[KNN_MAX_K + 1];
    const int kk = k + 1;
    int have = 0;
    for (int j = 0; j < m; ++j) {
        const float dj = dist[j];
        if (have < kk || dj < bd[have - 1]) {
            int p = have < kk ? have : kk - 1;
            while (p > 0 && dj < bd[p - 1]) { bd[p] = bd[p - 1]; bi[p] = bi[p - 1]; --p; }
            bd[p] = dj; bi[p] = j;
            if (have < kk) ++have;
        }
    }
    const int64_t first = (int64_t)gi * m + node_offset;       // id of the graph's node 0
    const size_t col = ((size_t)gi * m + v) * kp;
    int c = 0;
    for (int t = 0; t < have; ++t) {
        if (bi[t] == v) continue;
        if (c < kp) {
            src[col + c] = first + bi[t];
            dst[col + c] = first + v;
            if (q_src && v == 0) {
                q_src[(size_t)gi * kp + c] = first + bi[t];
                q_dst[(size_t)gi * kp + c] = first;
            }
        }
        ++c;
    }
    if (c != kp) atomicAdd(irregular, 1);
}

// n_per <= KNN_SMALL: one workgroup per graph; its waves take the unordered pairs in turn ((a - b)^2 is (b - a)^2 bit for bit),
// then thread v selects for node v.  Row stride n_per + 1 keeps the selecting threads on different LDS banks.
__global__ __launch_bounds__(NT) void knn_uniform_graph_kernel(const float* __restrict__ x, int n_per, int d4, int k, int kp,
                                                               int64_t node_offset, int64_t* __restrict__ src,
                                                               int64_t* __restrict__ dst, int64_t* __restrict__ q_src,
                                                               int64_t* __restrict__ q_dst, int* __restrict__ irregular) {
    __shared__ float s_dist[KNN_SMALL * (KNN_SMALL + 1)];
    const int gi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ld = n_per + 1;
    const float4* xg = reinterpret_cast<const float4*>(x) + (size_t)gi * n_per * d4;
    const int pairs = n_per * (n_per - 1) / 2;
    for (int p = wave; p < pairs; p += NT / 64) {
        int i = 0, rem = p;
        while (rem >= n_per - 1 - i) { rem -= n_per - 1 - i; ++i; }
        const int j = i + 1 + rem;
        const float acc = knn_pair_dist(xg + (size_t)i * d4, xg + (size_t)j * d4, d4, lane);
        if (lane == 0) { s_dist[i * ld + j] = acc; s_dist[j * ld + i] = acc; }
    }
    for (int i = wave; i < n_per; i += NT / 64) {     // the self match, evaluated like any pair: x - x is NaN for a non-finite x
        const float acc = knn_pair_dist(xg + (size_t)i * d4, xg + (size_t)i * d4, d4, lane);
        if (lane == 0) s_dist[i * ld + i] = acc;
    }
    __syncthreads();
    if (tid < n_per) knn_uniform_select(s_dist + tid * ld, n_per, tid, gi, k, kp, node_offset, src, dst, q_src, q_dst, irregular);
}

// n_per > KNN_SMALL: one workgroup per node, knn_candidates_kernel's shape with the graph's range computed instead of scanned.
__global__ __launch_bounds__(NT) void knn_uniform_node_kernel(const float* __restrict__ x, int n_per, int d4, int k, int kp,
                                                              int64_t node_offset, int64_t* __restrict__ src,
                                                              int64_t* __restrict__ dst, int64_t* __restrict__ q_src,
                                                              int64_t* __restrict__ q_dst, int* __restrict__ irregular) {
    __shared__ float s_dist[KNN_MAX_GRAPH];
    const int node = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gi = node / n_per, v = node - gi * n_per;
    const float4* xg = reinterpret_cast<const float4*>(x) + (size_t)gi * n_per * d4;
    const float4* xi = xg + (size_t)v * d4;
    for (int j = wave; j < n_per; j += NT / 64) {
        const float acc = knn_pair_dist(xi, xg + (size_t)j * d4, d4, lane);
        if (lane == 0) s_dist[j] = acc;
    }
    __syncthreads();
    if (tid == 0) knn_uniform_select(s_dist, n_per, v, gi, k, kp, node_offset, src, dst, q_src, q_dst, irregular);
}

inline int capped_grid(long items) {
    long g = (items + NT - 1) / NT;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

namespace rpg {
int launch_gather_add2_relu(const float* pq, const int64_t* lo, const int64_t* hi, const float* bias, float* out, int e,
                            int d, hipStream_t s) {
    if (!pq || !lo || !hi || !bias || !out || e <= 0 || d <= 0 || (d & 3)) return RPG_ERR_BAD_ARG;
    const long total = (long)e * (d / 4);
    hipLaunchKernelGGL(gather_add2_relu_kernel, dim3(capped_grid(total)), dim3(NT), 0, s, reinterpret_cast<const float4*>(pq),
                       lo, hi, reinterpret_cast<const float4*>(bias), reinterpret_cast<float4*>(out), d / 4, total);
    RPG_CHECK_LAUNCH("gather_add2_relu");
    return RPG_OK;
}
int launch_relu_inplace(float* x, long n_floats, hipStream_t s) {
    if (!x || n_floats <= 0 || (n_floats & 3)) return RPG_ERR_BAD_ARG;
    hipLaunchKernelGGL(relu_inplace_kernel, dim3(capped_grid(n_floats / 4)), dim3(NT), 0, s,
                       reinterpret_cast<float4*>(x), n_floats / 4);
    RPG_CHECK_LAUNCH("relu_inplace");
    return RPG_OK;
}
}  // namespace rpg

extern "C" int rpg_graph_prepare(const int64_t* src, const int64_t* dst, int64_t node_offset, int e, int n, int64_t* ends,
                                 int32_t* rowptr, int32_t* cursor, int32_t* perm, int32_t* status, void* stream) {
    if (!src || !dst || !ends || !rowptr || !cursor || !perm || !status || e <= 0 || n <= 0 || e > (1 << 20) ||
        n > (1 << 20))
        return RPG_ERR_BAD_ARG;
    hipLaunchKernelGGL(graph_prepare_kernel, dim3(1), dim3(GP_NT), 0, rpg::as_stream(stream), src, dst, node_offset, e, n, ends,
                       rowptr, cursor, perm, status);
    RPG_CHECK_LAUNCH("graph_prepare");
    return RPG_OK;
}

extern "C" int rpg_edge_concat_gather_f32(const float* x, const int64_t* edge_index, int e, int d, float* out,
                                          void* stream) {
    if (!x || !edge_index || !out || e <= 0 || d <= 0 || (d & 3) || !rpg::aligned16(x) || !rpg::aligned16(out))
        return RPG_ERR_BAD_ARG;
    const long total = (long)e * (d / 2);
    hipLaunchKernelGGL(edge_concat_kernel, dim3(capped_grid(total)), dim3(NT), 0, rpg::as_stream(stream),
                       reinterpret_cast<const float4*>(x), edge_index, e, d / 4, reinterpret_cast<float4*>(out), total);
    RPG_CHECK_LAUNCH("edge_concat_gather");
    return RPG_OK;
}

extern "C" int rpg_gather_add2_relu_f32(const float* pq, const int64_t* lo, const int64_t* hi, const float* bias, int e, int d,
                                        float* out, void* stream) {
    if (!rpg::aligned16(pq) || !rpg::aligned16(bias) || !rpg::aligned16(out)) return RPG_ERR_BAD_ARG;
    return rpg::launch_gather_add2_relu(pq, lo, hi, bias, out, e, d, rpg::as_stream(stream));
}

extern "C" int rpg_attention_rows_f32(const float* gtp, int r, int c, float* y, void* stream) {
    if (!gtp || !y || r <= 0 || c <= 0 || (c & 3) || c > 8192 || !rpg::aligned16(gtp)) return RPG_ERR_BAD_ARG;
    hipStream_t s = rpg::as_stream(stream);
    const int slot = rpg::timing_begin(RPG_TIMER_ATTENTION, s);
    hipLaunchKernelGGL(attention_rows_kernel, dim3(r), dim3(NT), (2 * c + 8) * sizeof(float), s, gtp, c, y);
    rpg::timing_end(slot, (double)r * c * (double)c * 4.0, s);
    RPG_CHECK_LAUNCH("attention_rows");
    return RPG_OK;
}

extern "C" int rpg_attention_aggregate_f32(const float* gtp, const float* msg, const int32_t* rowptr, const int32_t* perm,
                                           const float* bias, int n, int e, int c, int d, float* ybar, float* mbar,
                                           void* stream) {
    if (!gtp || !msg || !rowptr || !perm || !ybar || !mbar || n <= 0 || e <= 0 || c <= 0 || d <= 0 || (c & 3) || (d & 3) ||
        c > 4096 || !rpg::aligned16(gtp) || !rpg::aligned16(msg) || !rpg::aligned16(mbar) || (bias && !rpg::aligned16(bias)))
        return RPG_ERR_BAD_ARG;
    hipStream_t s = rpg::as_stream(stream);
    const int quarters = (c + 63) / 64;                       // 64 output channels per workgroup
    if ((d / 4 + quarters - 1) / quarters > AA_NT) return RPG_ERR_BAD_ARG;   // one mbar column per thread
    const int slot = rpg::timing_begin(RPG_TIMER_ATT_AGG, s);
    hipLaunchKernelGGL(attention_aggregate_kernel<false>, dim3(n, quarters), dim3(AA_NT), 0, s, gtp,
                       reinterpret_cast<const float4*>(msg), rowptr, perm, reinterpret_cast<const float4*>(bias), c, d / 4, ybar,
                       reinterpret_cast<float4*>(mbar), nullptr);
    // algorithmic bytes: the scatter-mean of SURVEY 8(a) A9 (messages E*D*4 + targets E*8 + output N*D*4) plus the attention
    // operands it now reads itself (E*3C*4) and the N*C*4 it writes
    rpg::timing_end(slot, (double)e * d * 4.0 + (double)e * 8.0 + (double)n * d * 4.0 + (double)e * 3.0 * c * 4.0 + (double)n * c * 4.0, s);
    RPG_CHECK_LAUNCH("attention_aggregate");
    return RPG_OK;
}

extern "C" int rpg_attention_aggregate_hidden_f32(const float* gtp, const float* hid, const int32_t* rowptr, const int32_t* perm,
                                                  const float* bias, int n, int e, int c, int d, float* ybar, float* hbar, float* res,
                                                  void* stream) {
    if (!gtp || !hid || !rowptr || !perm || !bias || !ybar || !hbar || !res || n <= 0 || e <= 0 || c <= 0 || d <= 0 || (c & 3) ||
        (d & 3) || c > 4096 || !rpg::aligned16(gtp) || !rpg::aligned16(hid) || !rpg::aligned16(hbar) || !rpg::aligned16(res) ||
        !rpg::aligned16(bias))
        return RPG_ERR_BAD_ARG;
    hipStream_t s = rpg::as_stream(stream);
    const int quarters = (c + 63) / 64;
    if ((d / 4 + quarters - 1) / quarters > AA_NT) return RPG_ERR_BAD_ARG;   // one hbar column per thread
    const int slot = rpg::timing_begin(RPG_TIMER_ATT_AGG, s);
    hipLaunchKernelGGL(attention_aggregate_kernel<true>, dim3(n, quarters), dim3(AA_NT), 0, s, gtp,
                       reinterpret_cast<const float4*>(hid), rowptr, perm, reinterpret_cast<const float4*>(bias), c, d / 4, ybar,
                       reinterpret_cast<float4*>(hbar), reinterpret_cast<float4*>(res));
    // algorithmic bytes: as rpg_attention_aggregate_f32, plus the residual rows (N*D*4)
    rpg::timing_end(slot, (double)e * d * 4.0 + (double)e * 8.0 + 2.0 * n * d * 4.0 + (double)e * 3.0 * c * 4.0 + (double)n * c * 4.0, s);
    RPG_CHECK_LAUNCH("attention_aggregate_hidden");
    return RPG_OK;
}

extern "C" int rpg_scatter_mean_f32(const float* msg, const int32_t* rowptr, const int32_t* perm, int n, int e, int d,
                                    float* out, void* stream) {
    if (!msg || !rowptr || !perm || !out || n <= 0 || e <= 0 || d <= 0 || (d & 3) || !rpg::aligned16(msg) || !rpg::aligned16(out))
        return RPG_ERR_BAD_ARG;
    hipStream_t s = rpg::as_stream(stream);
    const int d4 = d / 4;
    const int slot = rpg::timing_begin(RPG_TIMER_SCATTER, s);
    hipLaunchKernelGGL(scatter_mean_kernel, dim3(n, (d4 + NT - 1) / NT), dim3(NT), 0, s,
                       reinterpret_cast<const float4*>(msg), rowptr, perm, d4, reinterpret_cast<float4*>(out));
    // algorithmic bytes: messages E*D*4 + int64 targets E*8 + output N*D*4
    rpg::timing_end(slot, (double)e * d * 4.0 + (double)e * 8.0 + (double)n * d * 4.0, s);
    RPG_CHECK_LAUNCH("scatter_mean");
    return RPG_OK;
}

extern "C" int rpg_pose_heads_f32(const float* x, const float* w6, const float* b6, int r, int d, float* out,
                                  void* stream) {
    if (!x || !w6 || !b6 || !out || r <= 0 || d <= 0 || (d & 3) || !rpg::aligned16(x) || !rpg::aligned16(w6))
        return RPG_ERR_BAD_ARG;
    hipLaunchKernelGGL(pose_heads_kernel, dim3((r + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, rpg::as_stream(stream),
                       reinterpret_cast<const float4*>(x), reinterpret_cast<const float4*>(w6), b6, r, d / 4, out);
    RPG_CHECK_LAUNCH("pose_heads");
    return RPG_OK;
}

extern "C" int rpg_knn_graph_f32(const float* x, const int64_t* batch, int n, int d, int k, int64_t* edge_index,
                                 int32_t* cand, int32_t* cnt, int32_t* total, int32_t* status, void* stream) {
    if (!x || !edge_index || !cand || !cnt || !total || !status || n <= 0 || d <= 0 || (d & 3) || k <= 0 ||
        k > KNN_MAX_K || n > (1 << 20) || !rpg::aligned16(x))
        return RPG_ERR_BAD_ARG;
    hipStream_t s = rpg::as_stream(stream);
    hipLaunchKernelGGL(knn_candidates_kernel, dim3(n), dim3(NT), 0, s, x, batch, n, d / 4, k, cand, cnt, status);
    hipLaunchKernelGGL(knn_compact_kernel, dim3(1), dim3(GP_NT), 0, s, cand, cnt, n, k + 1, n * (k + 1), edge_index, total);
    RPG_CHECK_LAUNCH("knn_graph");
    return RPG_OK;
}

extern "C" int rpg_knn_graph_uniform_f32(const float* x, int g, int n_per, int d, int k, int64_t node_offset, int64_t* src,
                                         int64_t* dst, int64_t* q_src, int64_t* q_dst, int32_t* irregular, void* stream) {
    if (!x || !src || !dst || !irregular || (q_src == nullptr) != (q_dst == nullptr) || g <= 0 || n_per < 2 ||
        n_per > KNN_MAX_GRAPH || d <= 0 || (d & 3) || k <= 0 || k > KNN_MAX_K || node_offset < 0 ||
        (long)g * n_per > (1 << 20) || !rpg::aligned16(x))
        return RPG_ERR_BAD_ARG;
    hipStream_t s = rpg::as_stream(stream);
    const int kp = k < n_per - 1 ? k : n_per - 1;
    if (n_per <= KNN_SMALL)
        hipLaunchKernelGGL(knn_uniform_graph_kernel, dim3(g), dim3(NT), 0, s, x, n_per, d / 4, k, kp, node_offset, src, dst, q_src,
                           q_dst, irregular);
    else
        hipLaunchKernelGGL(knn_uniform_node_kernel, dim3(g * n_per), dim3(NT), 0, s, x, n_per, d / 4, k, kp, node_offset, src, dst,
                           q_src, q_dst, irregular);
    RPG_CHECK_LAUNCH("knn_graph_uniform");
    return RPG_OK;
}
