// The query-only output mode of the GNN composite (rpg_gnn_forward_query_*): what the last recursion needs besides the
// existing kernels.  The pose rule of the map path reads the relative poses on the edges INTO a query node (and the query's
// own absolute pose), and the last recursion of simpleConvEdge_upt (my_gnn_layer.py:293-311) has no consumer after it, so its
// E-row work is needed on the selected columns only and its N-row work on the query rows only.
//
//   query_select   one workgroup of 1024 lanes, the shape of graph_prepare: checks the selection against the contract
//                  (counted into status, everything clamped), writes the selected columns' end points and builds the CSR of
//                  the selection by query row, ascending position inside a row -- for an ascending selection the
//                  ascending-edge order of rpg_graph_prepare, so a query's mean adds the same edges in the same order.
//   gather_rows16  the compaction: out[i] = in[idx[i]] as 16-byte copies (fp32 or bf16 rows, any row pitch).
#include "rpg_common.h"

namespace {

constexpr int QS_NT = 1024;
constexpr int NT = 256;

__global__ __launch_bounds__(QS_NT) void query_select_kernel(const int64_t* __restrict__ esrc, const int64_t* __restrict__ edst,
                                                             int64_t node_off, int E, int N, const int64_t* __restrict__ ends,
                                                             const int64_t* __restrict__ sel, int ES, const int64_t* __restrict__ qnodes,
                                                             int Q, int* qrow, int* selc, int64_t* ssrc, int64_t* sdst, int* srow,
                                                             int* qn, int* rowptr, int* cursor, int* perm, int* status) {
    __shared__ int s_scan[QS_NT];
    __shared__ int s_bad;
    __shared__ int s_into;
    __shared__ int s_carry;
    const int tid = threadIdx.x;
    if (tid == 0) { s_bad = 0; s_into = 0; s_carry = 0; }
    for (int i = tid; i < N; i += QS_NT) qrow[i] = -1;
    for (int i = tid; i <= Q; i += QS_NT) rowptr[i] = 0;
    for (int i = tid; i < Q; i += QS_NT) cursor[i] = 0;
    __syncthreads();

    // the query nodes: in range, strictly ascending (so distinct); clamped; node -> query row (the highest row of a repeated node)
    int bad = 0;
    for (int i = tid; i < Q; i += QS_NT) {
        const int64_t v = qnodes[i] - node_off;
        const bool ok = ((uint64_t)v < (uint64_t)N) && (i == 0 || qnodes[i - 1] < qnodes[i]);
        const int vc = (int)(v < 0 ? 0 : (v >= N ? N - 1 : v));
        qn[i] = vc;
        atomicMax(&qrow[vc], i);
        if (!ok) ++bad;
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

    // how many valid columns of the whole list enter a query node: the selection must hold exactly these
    int into = 0;
    for (int e = tid; e < E; e += QS_NT) {
        const int64_t s = esrc[e] - node_off, t = edst[e] - node_off;
        if (((uint64_t)s < (uint64_t)N) && ((uint64_t)t < (uint64_t)N) && qrow[t] >= 0) ++into;
    }
    if (into) atomicAdd(&s_into, into);

    // the selected columns: in range, kept by graph_prepare, into a query node, ascending; end points from the sanitised copy
    for (int i = tid; i < ES; i += QS_NT) {
        const int64_t c = sel[i];
        bool ok = (uint64_t)c < (uint64_t)E;
        const int cc = (int)(c < 0 ? 0 : (c >= E ? E - 1 : c));
        const int64_t s = esrc[cc] - node_off, t = edst[cc] - node_off;
        ok = ok && ((uint64_t)s < (uint64_t)N) && ((uint64_t)t < (uint64_t)N);
        const int64_t sc = ends[cc], tc = ends[(size_t)E + cc];
        const int r = ok ? qrow[tc] : -1;
        const bool asc = i == 0 || sel[i - 1] < c;
        selc[i] = cc;
        ssrc[i] = sc;
        sdst[i] = tc;
        srow[i] = r;
        if (r >= 0) atomicAdd(&rowptr[r + 1], 1);
        if (r < 0 || !asc) ++bad;
    }
    if (bad) atomicAdd(&s_bad, bad);
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

    // inclusive scan of rowptr[1..Q] in chunks of 1024 (as graph_prepare)
    for (int base = 1; base <= Q; base += QS_NT) {
        const int i = base + tid;
        const int v = (i <= Q) ? rowptr[i] : 0;
        s_scan[tid] = v;
        __syncthreads();
        for (int off = 1; off < QS_NT; off <<= 1) {
            const int add = (tid >= off) ? s_scan[tid - off] : 0;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        const int carry = s_carry;
        if (i <= Q) rowptr[i] = carry + s_scan[tid];
        __syncthreads();
        if (tid == QS_NT - 1) s_carry = carry + s_scan[tid];
        __syncthreads();
    }
    __syncthreads();

    // a slot inside the query row's segment (arbitrary order), then every segment ordered by position in the selection
    for (int i = tid; i < ES; i += QS_NT) {
        const int r = srow[i];
        if (r >= 0) {
            const int slot = atomicAdd(&cursor[r], 1);
            perm[rowptr[r] + slot] = i;
        }
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    for (int v = tid; v < Q; v += QS_NT) {
        const int b = rowptr[v], n = rowptr[v + 1] - b;
        for (int i = 1; i < n; ++i) {
            const int key = perm[b + i];
            int j = i - 1;
            while (j >= 0 && perm[b + j] > key) { perm[b + j + 1] = perm[b + j]; --j; }
            perm[b + j + 1] = key;
        }
    }
    if (tid == 0) {
        const int total = s_bad + (s_into != ES ? 1 : 0);
        if (total) atomicAdd(status, total);             // accumulates, like graph_prepare's count
    }
}

// out[i][0 .. cols16) = in[idx[i]][0 .. cols16) in 16-byte units; row pitches ld_in16 / ld_out16 (16-byte units)
__global__ __launch_bounds__(NT) void gather_rows16_kernel(const uint4* __restrict__ in, int ld_in16, const int* __restrict__ idx,
                                                           uint4* __restrict__ out, int ld_out16, int cols16, long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int c = (int)(i % cols16);
        const long r = i / cols16;
        out[r * ld_out16 + c] = in[(size_t)idx[r] * ld_in16 + c];
    }
}

}  // namespace

namespace rpg {

int launch_query_select(const int64_t* esrc, const int64_t* edst, int64_t node_off, int e, int n, const int64_t* ends,
                        const int64_t* sel, int e_sel, const int64_t* qnodes, int q, int32_t* qrow, int32_t* selc, int64_t* ssrc,
                        int64_t* sdst, int32_t* srow, int32_t* qn, int32_t* rowptr, int32_t* cursor, int32_t* perm, int32_t* status,
                        hipStream_t s) {
    if (!esrc || !edst || !ends || !sel || !qnodes || !qrow || !selc || !ssrc || !sdst || !srow || !qn || !rowptr || !cursor ||
        !perm || !status || e <= 0 || n <= 0 || e_sel <= 0 || q <= 0 || e > (1 << 20) || n > (1 << 20) || e_sel > (1 << 20) ||
        q > n)
        return RPG_ERR_BAD_ARG;
    hipLaunchKernelGGL(query_select_kernel, dim3(1), dim3(QS_NT), 0, s, esrc, edst, node_off, e, n, ends, sel, e_sel, qnodes, q, qrow,
                       selc, ssrc, sdst, srow, qn, rowptr, cursor, perm, status);
    RPG_CHECK_LAUNCH("query_select");
    return RPG_OK;
}

int launch_gather_rows16(const void* in, int ld_in_bytes, const int32_t* idx, void* out, int ld_out_bytes, int row_bytes, long rows,
                         hipStream_t s) {
    if (!in || !idx || !out || rows <= 0 || row_bytes <= 0 || (row_bytes & 15) || (ld_in_bytes & 15) || (ld_out_bytes & 15) ||
        ld_in_bytes < row_bytes || ld_out_bytes < row_bytes || !aligned16(in) || !aligned16(out))
        return RPG_ERR_BAD_ARG;
    const long total = rows * (row_bytes / 16);
    long g = (total + NT - 1) / NT;
    g = g < 1 ? 1 : (g > 8192 ? 8192 : g);
    hipLaunchKernelGGL(gather_rows16_kernel, dim3((int)g), dim3(NT), 0, s, reinterpret_cast<const uint4*>(in), ld_in_bytes / 16, idx,
                       reinterpret_cast<uint4*>(out), ld_out_bytes / 16, row_bytes / 16, total);
    RPG_CHECK_LAUNCH("gather_rows16");
    return RPG_OK;
}

}  // namespace rpg
