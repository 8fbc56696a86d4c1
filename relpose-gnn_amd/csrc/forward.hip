// Composite forwards: the whole ResNet (BasicBlock) encoder and the whole GNN + heads, as sequences of the
// kernels in gemm_f32.hip / encoder_ops.hip / gnn_ops.hip on one stream.  No allocation, no synchronisation:
// the caller passes a workspace sized by rpg_*_workspace_bytes().
//
// Reference control flow restated here:
//   encoder  torchvision 0.9.1 ResNet._forward_impl with BasicBlock (call site posenet.py:1037)
//   GNN      /root/reference/python/niantic/modules/posenet.py:1052-1091 and my_gnn_layer.py:293-311
#include <initializer_list>

#include "rpg_common.h"

namespace rpg {
int launch_relu_inplace(float* x, long n_floats, hipStream_t s);
bool stem_pool_supported(int h, int w, int cout);
int launch_stem_pool(const float* x_nchw, const float* wpack, const float* shift, float* out, int n, int h, int w, hipStream_t s);
}

using rpg::Carver;
using rpg::ResnetWalk;
typedef rpg::ResnetBuffers<float> ResnetBuffersF32;      // NHWC4 input; the last buffer holds the split-K partial tiles

extern "C" size_t rpg_resnet_workspace_bytes(int n, int h, int w, const int* planes) {
    if (n <= 0 || h <= 0 || w <= 0 || !planes) return 0;
    return rpg::planned_bytes<ResnetBuffersF32>(n, h, w, planes, 4, rpg::split_scratch_bytes());
}

extern "C" int rpg_resnet_forward_f32(const float* const* tensors, int n_tensors, const int* blocks, const int* planes,
                                      int feat_dim, const float* x_nchw, int n, int h, int w, float* feat,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!tensors || !blocks || !planes || !x_nchw || !feat || !workspace || n <= 0 || h <= 0 || w <= 0 || feat_dim <= 0)
        return RPG_ERR_BAD_ARG;
    // tensor count: stem 4 + per block 8 (+4 with downsample) + fc 2; every 4th entry (u_wino43) may be NULL
    int expect = 4 + 2;
    for (ResnetWalk b(blocks, planes, 1, 1); !b.done(); b.next()) expect += b.ds ? 12 : 8;      // (whatever the extent)
    if (n_tensors != expect) return RPG_ERR_BAD_ARG;
    for (int i = 0; i < n_tensors; ++i)
        if (!tensors[i] && !((i & 3) == 3 && i < n_tensors - 2)) return RPG_ERR_BAD_ARG;
    const size_t scratch_bytes = rpg::split_scratch_bytes();
    Carver cv{reinterpret_cast<char*>(workspace), 0};
    ResnetBuffersF32 B;
    B.carve(cv, n, h, w, planes, 4, scratch_bytes);
    if (workspace_bytes < cv.off) return RPG_ERR_WORKSPACE;      // before any pointer of B is used
    hipStream_t s = rpg::as_stream(stream);
    float* const* buf = B.buf;
    rpg::ScratchScope scratch(B.scratch, scratch_bytes, s);  // split-K partial tiles of this call

    int rc;
    int ti = 0;
    if (tensors[3] && rpg::stem_pool_supported(h, w, planes[0])) {
        // the fused stem: NCHW input -> conv7x7/2 + BN + ReLU + maxpool3x3/2 -> pooled NHWC, one kernel (csrc/stem.hip);
        // tensors[3] = its packed weight operands (BN scale folded in), tensors[2] = the BN shift
        if ((rc = rpg::launch_stem_pool(x_nchw, tensors[3], tensors[2], buf[0], n, h, w, s)) != RPG_OK) return rc;
    } else {
        if ((rc = rpg_nchw3_to_nhwc4_f32(x_nchw, B.in, n, h, w, stream)) != RPG_OK) return rc;
        // stem: conv7x7/2 pad 3 (3 -> planes[0], input channels padded to 4 with zero weights) + BN + ReLU
        if ((rc = rpg::launch_conv(B.in, tensors[ti], tensors[ti + 1], tensors[ti + 2], nullptr, B.stem, n, h, w, 4,
                                   planes[0], 7, 7, 2, 3, 1, s, 3)) != RPG_OK)
            return rc;
        if ((rc = rpg_maxpool3x3s2_nhwc_f32(B.stem, buf[0], n, B.h1, B.w1, planes[0], stream)) != RPG_OK) return rc;
    }
    ti += 4;

    int cur = 0;
    ResnetWalk b(blocks, planes, B.h2, B.w2);
    for (; !b.done(); b.next()) {
        const int c = b.c;
        float* X = buf[cur];
        float* T = buf[(cur + 1) & 3];
        float* Y = buf[(cur + 2) & 3];
        float* D = buf[(cur + 3) & 3];
        // conv1 3x3/stride + BN + ReLU
        // Winograd where it pays (rpg::wino_pays: addressable with 32-bit buffer offsets and enough workgroups)
        const bool wino1 = b.stride == 1 && tensors[ti + 3] && rpg::wino_pays(n, b.h, b.w, b.cin, c);
        const bool wino2 = tensors[ti + 7] && rpg::wino_pays(n, b.ho, b.wo, c, c);
        if (wino1)
            rc = rpg::launch_conv_wino(X, tensors[ti + 3], tensors[ti + 1], tensors[ti + 2], nullptr, T, n, b.h, b.w, b.cin, c, 1, s);
        else
            rc = rpg::launch_conv(X, tensors[ti], tensors[ti + 1], tensors[ti + 2], nullptr, T, n, b.h, b.w, b.cin, c, 3, 3,
                                  b.stride, 1, 1, s);
        if (rc != RPG_OK) return rc;
        const float* identity = X;
        if (b.ds) {   // downsample: conv1x1/stride + BN (no activation)
            if ((rc = rpg::launch_conv(X, tensors[ti + 8], tensors[ti + 9], tensors[ti + 10], nullptr, D, n, b.h, b.w, b.cin, c, 1,
                                       1, b.stride, 0, 0, s)) != RPG_OK)
                return rc;
            identity = D;
        }
        // conv2 3x3/1 + BN + identity + ReLU
        if (wino2)
            rc = rpg::launch_conv_wino(T, tensors[ti + 7], tensors[ti + 5], tensors[ti + 6], identity, Y, n, b.ho, b.wo, c, c, 1, s);
        else
            rc = rpg::launch_conv(T, tensors[ti + 4], tensors[ti + 5], tensors[ti + 6], identity, Y, n, b.ho, b.wo, c, c, 3, 3, 1,
                                  1, 1, s);
        if (rc != RPG_OK) return rc;
        ti += b.ds ? 12 : 8;
        cur = (cur + 2) & 3;
    }
    // the walk has ended: b.cin x b.h x b.w is the last activation tensor
    if ((rc = rpg_global_avgpool_nhwc_f32(buf[cur], B.pool, n, b.h * b.w, b.cin, stream)) != RPG_OK) return rc;
    rpg::GatherSrc src{};
    src.n = 1; src.a[0] = B.pool; src.idx[0] = nullptr; src.ld[0] = b.cin; src.width[0] = b.cin;
    return rpg::launch_linear(src, tensors[ti], tensors[ti + 1], nullptr, feat, n, feat_dim, 0, s);
}

// ------------------------------------------------------------------------------------------------------------
// GNN + heads
// ------------------------------------------------------------------------------------------------------------
namespace {
enum GnnTensor {
    T_PROJ_W, T_PROJ_B, T_EDGE0_W, T_EDGE0_B, T_EDGE2_W, T_EDGE2_B, T_MSG0_W, T_MSG0_B, T_MSG2_W, T_MSG2_B,
    T_GTP_W, T_GTP_B, T_ATTW_W, T_ATTW_B, T_UPD0_W, T_UPD0_B, T_UPD2_W, T_UPD2_B, T_HEADN_W, T_HEADN_B,
    T_HEADE_W, T_HEADE_B, T_COUNT,
    // optional node/edge split of the concatenated-input Linears (enables the per-node precompute path):
    T_PROJN_W = T_COUNT,   // [2D][D]  = rows cat(proj_edge.W[:, :D], proj_edge.W[:, D:])
    T_NODE3_W,             // [3D][D]  = rows cat(edge_mlp.0.W[:, :D], edge_mlp.0.W[:, D:2D], mlp.0.W[:, :D])
    T_EDGE0E_W,            // [D][D]   = edge_mlp.0.W[:, 2D:]
    T_MSG0E_W,             // [D][D]   = mlp.0.W[:, D:]
    T_COUNT_SPLIT,
    // optional products / concatenations around mlp.2 (enable the mean-first message path of layers_general; c = D / 8):
    T_GTPM_W = T_COUNT_SPLIT,   // [3c][D]     = att.gtp.W mlp.2.W (float64 product, rounded once); T_GTPM_B follows it as a bias does
    T_GTPM_B,                   // [3c]        = att.gtp.W mlp.2.b + att.gtp.b
    T_MSG2ATT_W,                // [D][D + c]  = cat(mlp.2.W, att.W.W) along the input dimension
    T_MSG2ATT_B,                // [D]         = att.W.b + mlp.2.b: the residual row of nodes with incoming edges, never a bias operand
    T_COUNT_MEAN
};

// The query-only output mode (rpg_gnn_forward_query_*): the selection.  The pruned last recursion reuses the buffers of
// GnnBuffers at e_sel / q rows and keeps the rest in GnnQueryBuffers.
struct QuerySel {
    const int64_t* sel;        // [e_sel] ascending columns of the edge list: every valid column whose target is a query node
    int e_sel;
    const int64_t* qnodes;     // [q] ascending node ids, in the numbering of the edge list (node_offset is subtracted)
    int q;
};
}  // namespace

extern "C" size_t rpg_gnn_workspace_bytes(int n, int e, int d) {
    if (n <= 0 || e <= 0 || d <= 0 || (d & 31)) return 0;
    return rpg::planned_bytes<rpg::GnnBuffers>(n, e, d, rpg::split_scratch_bytes());
}

extern "C" size_t rpg_gnn_query_workspace_bytes(int n, int e, int d, int e_sel, int q) {
    if (n <= 0 || e <= 0 || d <= 0 || (d & 31) || e_sel <= 0 || e_sel > e || q <= 0 || q > n) return 0;
    return rpg::planned_bytes<rpg::GnnBuffers>(n, e, d, rpg::split_scratch_bytes()) + rpg::planned_bytes<rpg::GnnQueryBuffers>(d, e_sel, q);
}

namespace {
// wb: null (every Linear in fp32), or the bf16 images of the 10 GEMM weights of the split formulation, in the order
// of BfWeight (then the Linears run on v_mfma_f32_32x32x16_bf16 with bf16 inputs / weights, fp32 accumulation, fp32
// bias / residual / output; everything that is not a GEMM stays fp32)
enum BfWeight { B_PROJN, B_NODE3, B_EDGE0E, B_EDGE2, B_MSG0E, B_MSG2, B_GTP, B_ATTW, B_UPD0, B_UPD2, B_COUNT };

int check_bf16_table(const void* const* weights_bf16, int n_bf16, int d) {
    if (!weights_bf16 || n_bf16 != B_COUNT || (d & 63)) return RPG_ERR_BAD_ARG;
    for (int i = 0; i < B_COUNT; ++i)
        if (!weights_bf16[i]) return RPG_ERR_BAD_ARG;
    return RPG_OK;
}

// What every step of one GNN forward needs.
struct GnnCall {
    const float* const* tensors;
    const void* const* wb;
    int n, e, d, c, recursion;           // c = d / 8, the width of the attention vector
    bool split;                          // the concatenated-input Linears run in their node / edge split form
    bool mean_first;                     // fp32, fused aggregation: mlp.2 runs behind the mean (needs T_COUNT_MEAN tensors)
    const QuerySel* qs;                  // null: full outputs
    int es, nq;                          // qs ? its e_sel, q : 0
    hipStream_t s;
    rpg::GnnBuffers g;
    rpg::GnnQueryBuffers q;
    const int64_t *src, *dst, *lo, *hi;  // the prepared end points of every edge (g.ends)
    const float* x;                      // current node features ...
    float* ecur;                         // ... and edge features: left by the layers for finish()
};

// Argument checks and carving: nothing is launched and nothing written when it refuses.
int prepare(GnnCall& k, const float* const* tensors, int n_tensors, const void* const* wb, const float* feat, const int64_t* esrc,
            const int64_t* edst, int n, int e, int d, int gnn_recursion, const float* abs_pose, const float* rel_pose, const int32_t* status,
            void* workspace, size_t workspace_bytes, size_t scratch_bytes, void* stream, const QuerySel* qs) {
    if (!tensors || (n_tensors != T_COUNT && n_tensors != T_COUNT_SPLIT && n_tensors != T_COUNT_MEAN) || !feat || !esrc || !edst || !abs_pose || !rel_pose || !status || !workspace ||
        n <= 0 || e <= 0 || d <= 0 || (d & 31) || gnn_recursion < 0)
        return RPG_ERR_BAD_ARG;
    for (int i = 0; i < n_tensors; ++i)
        if (!tensors[i]) return RPG_ERR_BAD_ARG;
    if (qs && (!qs->sel || !qs->qnodes || qs->e_sel <= 0 || qs->e_sel > e || qs->q <= 0 || qs->q > n)) return RPG_ERR_BAD_ARG;
    Carver cv{reinterpret_cast<char*>(workspace), 0};
    k.g.carve(cv, n, e, d, scratch_bytes);
    if (qs) k.q.carve(cv, d, qs->e_sel, qs->q);
    if (workspace_bytes < cv.off) return RPG_ERR_WORKSPACE;      // before any pointer of k.g / k.q is used
    k.tensors = tensors; k.wb = wb;
    k.n = n; k.e = e; k.d = d; k.c = d / 8; k.recursion = gnn_recursion;
    k.split = (n_tensors >= T_COUNT_SPLIT) && (wb || rpg::tuning().gnn.split != 0);
    k.mean_first = (n_tensors == T_COUNT_MEAN) && !wb && rpg::tuning().gnn.mean_first != 0;      // implies fuse_agg
    if (wb && !k.split) return RPG_ERR_BAD_ARG;            // the bf16 Linears exist for the split formulation only
    k.qs = qs; k.es = qs ? qs->e_sel : 0; k.nq = qs ? qs->q : 0;
    k.s = rpg::as_stream(stream);
    k.x = feat; k.ecur = k.g.ebuf[0];
    return RPG_OK;
}

// The graph's index arrays and, in query-only mode, the selection's: the first launches of the call.
int prepare_graph(GnnCall& k, const int64_t* esrc, const int64_t* edst, int64_t node_offset, int32_t* status) {
    const rpg::GnnBuffers& g = k.g;
    const rpg::GnnQueryBuffers& q = k.q;
    int rc;
    if ((rc = rpg_graph_prepare(esrc, edst, node_offset, k.e, k.n, g.ends, g.rowptr, g.cursor, g.perm, status, k.s)) != RPG_OK) return rc;
    k.src = g.ends;
    k.dst = g.ends + k.e;
    k.lo = g.ends + 2 * (size_t)k.e;
    k.hi = g.ends + 3 * (size_t)k.e;
    // the selection: checked against its contract (counted into status, clamped), its end points, its CSR by query row.  `cursor`
    // is free once graph_prepare has run: it holds the node -> query row table.
    if (k.qs) rc = rpg::launch_query_select(esrc, edst, node_offset, k.e, k.n, g.ends, k.qs->sel, k.es, k.qs->qnodes, k.nq, g.cursor, q.selc,
                                            q.ssrc, q.sdst, q.srow, q.qn, q.rowptr_q, q.cursor_q, q.perm_q, status, k.s);
    return rc;
}

// The rows recursion r runs on.  Query-only mode, last recursion: nothing reads its output but the heads, so the edge rows are the
// selected columns and the node rows the query nodes (the three node terms stay n rows: a selected edge's source is any node).
struct GnnRows {
    bool prune;
    int me, mn;                          // edge rows, node rows
    const int64_t *src, *dst;            // end points of the edge rows
    const int32_t *rowptr, *perm;        // their CSR by node row
};
GnnRows rows_of(const GnnCall& k, int r) {
    if (k.qs && r + 1 == k.recursion) return {true, k.es, k.nq, k.q.ssrc, k.q.sdst, k.q.rowptr_q, k.q.perm_q};
    return {false, k.e, k.n, k.src, k.dst, k.g.rowptr, k.g.perm};
}

// One Linear of the general route on the concatenation of up to three sources (idx: rows gathered by node / edge id), weight
// tensors[wt], bias tensors[wt + 1].  bf16 Linears: at most two ungathered sources (all the split formulation leaves), converted
// and concatenated in bf16 first; no dual-store epilogue.
struct LinSrc {
    const float* a;
    const int64_t* idx;
    int width;
};
int linear(const GnnCall& k, std::initializer_list<LinSrc> srcs, int wt, const float* residual, float* out, int m, int n_out, int relu,
           float* out_relu = nullptr, bool with_bias = true) {
    const float* bias = with_bias ? k.tensors[wt + 1] : nullptr;
    if (k.wb) {
        int bw = -1;
        switch (wt) {
            case T_EDGE2_W: bw = B_EDGE2; break;
            case T_MSG2_W: bw = B_MSG2; break;
            case T_GTP_W: bw = B_GTP; break;
            case T_ATTW_W: bw = B_ATTW; break;
            case T_UPD0_W: bw = B_UPD0; break;
            case T_UPD2_W: bw = B_UPD2; break;
            default: return RPG_ERR_BAD_ARG;
        }
        if (srcs.size() > 2) return RPG_ERR_BAD_ARG;
        int kk = 0, col = 0, rc;
        for (const LinSrc& sr : srcs) {
            if (sr.idx) return RPG_ERR_BAD_ARG;
            kk += sr.width;
        }
        for (const LinSrc& sr : srcs) {
            if ((rc = rpg::launch_f32_to_bf16(sr.a, sr.width, k.g.abf, kk, col, m, sr.width, k.s)) != RPG_OK) return rc;
            col += sr.width;
        }
        if (out_relu) return RPG_ERR_BAD_ARG;          // the bf16 Linears have no dual-store epilogue
        return rpg::launch_linear_bf16(k.g.abf, k.wb[bw], bias, residual, nullptr, nullptr, nullptr, n_out, out, m, kk, n_out, relu, k.s);
    }
    rpg::GatherSrc g{};
    for (const LinSrc& sr : srcs) {
        const int i = g.n++;
        g.a[i] = sr.a; g.idx[i] = sr.idx; g.ld[i] = sr.width; g.width[i] = sr.width;
        g.rows[i] = sr.idx ? (k.n > k.e ? k.n : k.e) : 0;       // node / edge ids index n- or e-row arrays
    }
    return rpg::launch_linear(g, k.tensors[wt], bias, residual, out, m, n_out, relu, k.s, nullptr, out_relu);
}

// A Linear fed by cat[x[a], x[b], e] splits as W_a x[a] + W_b x[b] + W_e e: the node terms are computed once per
// NODE (n rows) and added as gathered rows in the edge GEMM's epilogue (summation order changes only).
int node_gemm(const GnnCall& k, const float* xin, int wt, int n_out) {
    const int n = k.n, d = k.d;
    if (k.wb) {
        int rc;
        if ((rc = rpg::launch_f32_to_bf16(xin, d, k.g.abf, d, 0, n, d, k.s)) != RPG_OK) return rc;
        return rpg::launch_linear_bf16(k.g.abf, k.wb[wt == T_PROJN_W ? B_PROJN : B_NODE3], nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                       k.g.node3, n, d, n_out, 0, k.s);
    }
    rpg::GatherSrc g{};
    g.n = 1; g.a[0] = xin; g.idx[0] = nullptr; g.ld[0] = d; g.width[0] = d;
    return rpg::launch_linear(g, k.tensors[wt], nullptr, nullptr, k.g.node3, n, n_out, 0, k.s);
}
int edge_gemm(const GnnCall& k, const float* ein, int wt, int bias_t, const float* r1, const int64_t* i1, const float* r2,
              const int64_t* i2, float* out, int m) {
    const int d = k.d;
    if (k.wb) {
        int rc;
        if ((rc = rpg::launch_f32_to_bf16(ein, d, k.g.abf, d, 0, m, d, k.s)) != RPG_OK) return rc;
        return rpg::launch_linear_bf16(k.g.abf, k.wb[wt == T_EDGE0E_W ? B_EDGE0E : B_MSG0E], k.tensors[bias_t], r1, i1, r2, i2, 3 * d, out,
                                       m, d, d, 1, k.s);
    }
    rpg::GatherSrc g{};
    g.n = 1; g.a[0] = ein; g.idx[0] = nullptr; g.ld[0] = d; g.width[0] = d;
    const rpg::GatherRes gr{r1, i1, r2, i2, 3 * d};
    return rpg::launch_linear(g, k.tensors[wt], k.tensors[bias_t], nullptr, out, m, d, 1, k.s, &gr);
}

// ---- bf16 Linears, round 3: every GEMM hands its result to the next GEMM in bf16 FROM ITS EPILOGUE (EpiB::out2 /
// a bf16 primary output); the 21 separate f32 -> bf16 passes and the 2 in-place ReLU passes per forward of round 2
// are down to 4 conversions (encoder features, proj_edge output, 2 x the n x D/8 attention vector).  The bf16
// tensors live in the fp32 buffers this mode does not use (raw edge update, hidden, node hidden, agg).
int layers_bf16_chained(GnnCall& k) {
    typedef unsigned short bf;
    const rpg::GnnBuffers& g = k.g;
    const rpg::GnnQueryBuffers& q = k.q;
    const int n = k.n, e = k.e, d = k.d, c = k.c;
    // the bf16 tensors below are ALIASED onto fp32 buffers of GnnBuffers: check that every one fits the buffer it is placed in
    // (all four are exact fits today; a change to the layout must not silently overlap)
    if (2 * (size_t)e * d * sizeof(bf) > g.edge_bytes ||          // eb | enb in eraw, hb | mb in hid
        (size_t)n * 2 * d * sizeof(bf) > g.node_bytes ||          // xab [n][2d] in nhid
        (size_t)n * d * sizeof(bf) > g.node_bytes ||              // nhb [n][d] in agg
        (size_t)n * c * sizeof(bf) > g.abf_bytes)                 // yb [n][c] in abf
        return RPG_ERR_WORKSPACE;
    bf* eb = reinterpret_cast<bf*>(g.eraw);               // [e][d]   current edge features (A of edge_mlp.0's edge block)
    bf* enb = eb + (size_t)e * d;                         // [e][d]   raw edge update (A of mlp.0's edge block)
    bf* hb = reinterpret_cast<bf*>(g.hid);                // [e][d]   hidden activations of edge_mlp / mlp
    bf* mb = hb + (size_t)e * d;                          // [e][d]   messages (A of g|theta|phi)
    bf* xab = reinterpret_cast<bf*>(g.nhid);              // [n][2d]  x | aggregated messages (A of mlp_updating.0; x alone: lda = 2d)
    bf* nhb = reinterpret_cast<bf*>(g.agg);               // [n][d]   hidden activations of mlp_updating
    bf* yb = g.abf;                                       // [n][c]   attention vector
    auto gemm = [&](const void* a, int lda, int kk, int bw, const float* bias, const float* r1, const int64_t* i1, const float* r2,
                    const int64_t* i2, int ldr, void* out, int out_f32, void* out2, int ld2, int relu2, int m, int n_out, int relu) {
        rpg::LinearBf16Out o{};
        o.out = out; o.out_f32 = out_f32; o.out2 = out2; o.ld2 = ld2; o.relu2 = relu2;
        return rpg::launch_linear_bf16_ex(a, lda, k.wb[bw], bias, r1, i1, r2, i2, ldr, o, m, kk, n_out, relu, k.s);
    };
    auto gather16 = [&](const void* in, int ld_in, const int32_t* idx, void* out, int ld_out, int row_bytes, int rows) {
        return rpg::launch_gather_rows16(in, ld_in, idx, out, ld_out, row_bytes, rows, k.s);
    };
    int rc;
    if ((rc = rpg::launch_f32_to_bf16(k.x, d, xab, 2 * d, 0, n, d, k.s)) != RPG_OK) return rc;
    // edge_feat = relu(proj_edge(cat[x[min], x[max]]))                               posenet.py:1053-1055
    if ((rc = gemm(xab, 2 * d, d, B_PROJN, nullptr, nullptr, nullptr, nullptr, nullptr, 0, g.node3, 1, nullptr, 0, 0, n, 2 * d, 0)) != RPG_OK) return rc;
    if ((rc = rpg::launch_gather_add2_relu(g.node3, k.lo, k.hi, k.tensors[T_PROJ_B], k.ecur, e, d, k.s)) != RPG_OK) return rc;
    if ((rc = rpg::launch_f32_to_bf16(k.ecur, d, eb, d, 0, e, d, k.s)) != RPG_OK) return rc;
    for (int r = 0; r < k.recursion; ++r) {                                         // posenet.py:1061-1069
        const bool last = r + 1 == k.recursion;
        const GnnRows rw = rows_of(k, r);
        const int me = rw.me, mn = rw.mn;
        float* xnew = g.xbuf[r & 1];
        // edge update                                                              my_gnn_layer.py:296-297
        if ((rc = gemm(xab, 2 * d, d, B_NODE3, nullptr, nullptr, nullptr, nullptr, nullptr, 0, g.node3, 1, nullptr, 0, 0, n, 3 * d, 0)) != RPG_OK) return rc;
        const bf* ein = eb;
        if (rw.prune) {
            if ((rc = gather16(eb, d * 2, q.selc, q.ebs, d * 2, d * 2, me)) != RPG_OK) return rc;
            ein = q.ebs;
        }
        if ((rc = gemm(ein, d, d, B_EDGE0E, k.tensors[T_EDGE0_B], g.node3, rw.src, g.node3 + d, rw.dst, 3 * d, hb, 0, nullptr, 0, 0, me, d, 1)) != RPG_OK) return rc;
        // raw update -> enb (consumed by the message MLP); relu(update) (posenet.py:1065) -> the next recursion's bf16 edge
        // features, or on the last recursion the fp32 ones the heads read
        if (last) rc = gemm(hb, d, d, B_EDGE2, k.tensors[T_EDGE2_B], nullptr, nullptr, nullptr, nullptr, 0, g.ebuf[1], 1, enb, d, 0, me, d, 1);
        else rc = gemm(hb, d, d, B_EDGE2, k.tensors[T_EDGE2_B], nullptr, nullptr, nullptr, nullptr, 0, eb, 0, enb, d, 0, e, d, 1);
        if (rc != RPG_OK) return rc;
        if (last) k.ecur = g.ebuf[1];
        // message MLP, attention, aggregation                                      my_gnn_layer.py:301,304-307
        if ((rc = gemm(enb, d, d, B_MSG0E, k.tensors[T_MSG0_B], g.node3 + 2 * d, rw.src, nullptr, nullptr, 3 * d, hb, 0, nullptr, 0, 0, me, d, 1)) != RPG_OK) return rc;
        if ((rc = gemm(hb, d, d, B_MSG2, k.tensors[T_MSG2_B], nullptr, nullptr, nullptr, nullptr, 0, g.msg, 1, mb, d, 0, me, d, 0)) != RPG_OK) return rc;
        if ((rc = gemm(mb, d, d, B_GTP, k.tensors[T_GTP_B], nullptr, nullptr, nullptr, nullptr, 0, g.gtp, 1, nullptr, 0, 0, me, 3 * c, 0)) != RPG_OK) return rc;
        if ((rc = rpg_attention_aggregate_f32(g.gtp, g.msg, rw.rowptr, rw.perm, k.tensors[T_ATTW_B], mn, me, c, d, g.yat, g.att, k.s)) != RPG_OK)
            return rc;
        if ((rc = rpg::launch_f32_to_bf16(g.yat, c, yb, c, 0, mn, c, k.s)) != RPG_OK) return rc;
        bf* xa = xab;                                     // [mn][2d]: x | aggregate, the input of mlp_updating.0
        if (rw.prune) {
            if ((rc = gather16(xab, 4 * d, q.qn, q.xabq, 4 * d, 2 * d, mn)) != RPG_OK) return rc;
            xa = q.xabq;
        }
        // att.W on node rows; the aggregate goes straight to the right half of mlp_updating.0's bf16 input
        if ((rc = gemm(yb, c, c, B_ATTW, nullptr, g.att, nullptr, nullptr, nullptr, d, nullptr, 0, xa + d, 2 * d, 0, mn, d, 0)) != RPG_OK) return rc;
        // node update                                                              my_gnn_layer.py:309-311
        if ((rc = gemm(xa, 2 * d, 2 * d, B_UPD0, k.tensors[T_UPD0_B], nullptr, nullptr, nullptr, nullptr, 0, nhb, 0, nullptr, 0, 0, mn, d, 1)) != RPG_OK) return rc;
        if ((rc = gemm(nhb, d, d, B_UPD2, k.tensors[T_UPD2_B], nullptr, nullptr, nullptr, nullptr, 0, xnew, 1, rw.prune ? nullptr : xab,
                       rw.prune ? 0 : 2 * d, 1, mn, d, 1)) != RPG_OK)
            return rc;
        k.x = xnew;
    }
    return RPG_OK;
}

// Every other form: fp32 split / unsplit (RPG_TUNE_GNN_SPLIT), fused / unfused aggregation and, with the T_COUNT_MEAN table, the mean
// before or after mlp.2 (RPG_TUNE_GNN_FUSE_AGG), and the bf16 Linears that convert their input per Linear (bf16 with unfused aggregation).
int layers_general(GnnCall& k) {
    const rpg::GnnBuffers& g = k.g;
    const rpg::GnnQueryBuffers& q = k.q;
    const int e = k.e, d = k.d, c = k.c;
    const bool split = k.split, fuse_agg = rpg::tuning().gnn.fuse_agg != 0;
    int rc;
    // edge_feat = relu(proj_edge(cat[x[min], x[max]]))                                   posenet.py:1053-1055
    const float* x = k.x;
    float* ecur = k.ecur;
    if (split) {
        if ((rc = node_gemm(k, x, T_PROJN_W, 2 * d)) != RPG_OK) return rc;               // [n][2d] = [W_lo x | W_hi x]
        if ((rc = rpg::launch_gather_add2_relu(g.node3, k.lo, k.hi, k.tensors[T_PROJ_B], ecur, e, d, k.s)) != RPG_OK) return rc;
    } else if ((rc = linear(k, {{x, k.lo, d}, {x, k.hi, d}}, T_PROJ_W, nullptr, ecur, e, d, 1)) != RPG_OK) {
        return rc;
    }

    const bool dual = !k.wb;               // fp32: the edge update is stored twice, raw (for the message) and rectified
    for (int r = 0; r < k.recursion; ++r) {                                             // posenet.py:1061-1069
        const GnnRows rw = rows_of(k, r);
        const int me = rw.me, mn = rw.mn;
        float* enext = (ecur == g.ebuf[0]) ? g.ebuf[1] : g.ebuf[0];    // relu(edge update): the next recursion's / the heads' input
        float* enew = dual ? g.eraw : enext;                          // the raw edge update (consumed by the message MLP)
        float* xnew = g.xbuf[r & 1];
        const float* ein = ecur;
        if (rw.prune) {
            if ((rc = rpg::launch_gather_rows16(ecur, d * 4, q.selc, q.esel, d * 4, d * 4, me, k.s)) != RPG_OK) return rc;
            ein = q.esel;
        }
        // edge update: edge_mlp(cat[x[src], x[dst], e])                                 my_gnn_layer.py:296-297
        if (split) {
            if ((rc = node_gemm(k, x, T_NODE3_W, 3 * d)) != RPG_OK) return rc;           // [n][3d] = [Ws x | Wd x | Wm x]
            if ((rc = edge_gemm(k, ein, T_EDGE0E_W, T_EDGE0_B, g.node3, rw.src, g.node3 + d, rw.dst, g.hid, me)) != RPG_OK) return rc;
        } else if ((rc = linear(k, {{x, rw.src, d}, {x, rw.dst, d}, {ein, nullptr, d}}, T_EDGE0_W, nullptr, g.hid, me, d, 1)) != RPG_OK) {
            return rc;
        }
        // edge_feat = relu(edge_feat) of posenet.py:1065 is the second output of this Linear's epilogue (fp32 path)
        if ((rc = linear(k, {{g.hid, nullptr, d}}, T_EDGE2_W, nullptr, enew, me, d, 0, dual ? enext : nullptr)) != RPG_OK) return rc;
        // message: mlp(cat[x[src], e_new]) then AttentionBlock                          my_gnn_layer.py:304-307
        if (split) {
            if ((rc = edge_gemm(k, enew, T_MSG0E_W, T_MSG0_B, g.node3 + 2 * d, rw.src, nullptr, nullptr, g.hid, me)) != RPG_OK) return rc;
        } else if ((rc = linear(k, {{x, rw.src, d}, {enew, nullptr, d}}, T_MSG0_W, nullptr, g.hid, me, d, 1)) != RPG_OK) {
            return rc;
        }
        if (k.mean_first) {
            // mlp.2 has no activation behind it and feeds a Linear (g|theta|phi) and the mean, so it moves behind the mean:
            // g|theta|phi reads the hidden rows through the product weight, the aggregate kernel averages the hidden rows and ONE
            // node-row Linear applies cat(mlp.2.W, att.W) to [hbar ; ybar].  The biases b_att + b_mlp2 come in as the residual
            // row, which the kernel leaves zero for a node without incoming edges.  g.msg stays unused.  The three node-row
            // tensors live in NODE-sized buffers that are free here (an [e][d] buffer is too small for them where n > e): hbar
            // in nhid (written next by mlp_updating.0, which reads agg), the residual rows and ybar in node3 (its three
            // per-node terms were consumed by the two edge GEMMs above).
            float* hbar = g.nhid;
            float* res = g.node3;
            float* ybar = g.node3 + (size_t)k.n * d;
            if ((rc = linear(k, {{g.hid, nullptr, d}}, T_GTPM_W, nullptr, g.gtp, me, 3 * c, 0)) != RPG_OK) return rc;
            if ((rc = rpg_attention_aggregate_hidden_f32(g.gtp, g.hid, rw.rowptr, rw.perm, k.tensors[T_MSG2ATT_B], mn, me, c, d, ybar, hbar,
                                                         res, k.s)) != RPG_OK)
                return rc;
            if ((rc = linear(k, {{hbar, nullptr, d}, {ybar, nullptr, c}}, T_MSG2ATT_W, res, g.agg, mn, d, 0, nullptr, false)) != RPG_OK)
                return rc;
        } else if (fuse_agg) {
            if ((rc = linear(k, {{g.hid, nullptr, d}}, T_MSG2_W, nullptr, g.msg, me, d, 0)) != RPG_OK) return rc;
            if ((rc = linear(k, {{g.msg, nullptr, d}}, T_GTP_W, nullptr, g.gtp, me, 3 * c, 0)) != RPG_OK) return rc;
            // aggregate FIRST (att = W y + b + msg is linear in (y, msg): mean(att) = W mean(y) + b + mean(msg)), in the
            // attention kernel itself, then att.W on the n node rows                    my_gnn_layer.py:301,304-307; att.py:32-33
            if ((rc = rpg_attention_aggregate_f32(g.gtp, g.msg, rw.rowptr, rw.perm, k.tensors[T_ATTW_B], mn, me, c, d, g.yat, g.att, k.s)) != RPG_OK)
                return rc;
            if ((rc = linear(k, {{g.yat, nullptr, c}}, T_ATTW_W, g.att, g.agg, mn, d, 0, nullptr, false)) != RPG_OK) return rc;
        } else {
            if ((rc = linear(k, {{g.hid, nullptr, d}}, T_MSG2_W, nullptr, g.msg, me, d, 0)) != RPG_OK) return rc;
            if ((rc = linear(k, {{g.msg, nullptr, d}}, T_GTP_W, nullptr, g.gtp, me, 3 * c, 0)) != RPG_OK) return rc;
            if ((rc = rpg_attention_rows_f32(g.gtp, me, c, g.yat, k.s)) != RPG_OK) return rc;
            if ((rc = linear(k, {{g.yat, nullptr, c}}, T_ATTW_W, g.msg, g.att, me, d, 0)) != RPG_OK) return rc;
            // aggregate (mean over incoming edges)                                       my_gnn_layer.py:301
            if ((rc = rpg_scatter_mean_f32(g.att, rw.rowptr, rw.perm, mn, me, d, g.agg, k.s)) != RPG_OK) return rc;
        }
        // node update                                                                   my_gnn_layer.py:309-311
        const float* xin = x;
        if (rw.prune) {
            if ((rc = rpg::launch_gather_rows16(x, d * 4, q.qn, q.xq, d * 4, d * 4, mn, k.s)) != RPG_OK) return rc;
            xin = q.xq;
        }
        if ((rc = linear(k, {{xin, nullptr, d}, {g.agg, nullptr, d}}, T_UPD0_W, nullptr, g.nhid, mn, d, 1)) != RPG_OK) return rc;
        if ((rc = linear(k, {{g.nhid, nullptr, d}}, T_UPD2_W, nullptr, xnew, mn, d, 1)) != RPG_OK) return rc;
        // x = relu(x) is fused above; edge_feat = relu(edge_feat): dual-stored above, or in place now that the message has
        // consumed the raw one (bf16 Linears)
        if (!dual && (rc = rpg::launch_relu_inplace(enext, (long)me * d, k.s)) != RPG_OK) return rc;
        x = xnew;
        ecur = enext;
    }
    k.x = x; k.ecur = ecur;
    return RPG_OK;
}

// The optional feature outputs and the heads (droprate == 0, use_AP)                     posenet.py:1077-1091
int finish(const GnnCall& k, float* abs_pose, float* rel_pose, float* node_out, float* edge_out) {
    const int d = k.d;
    // rows of the heads' inputs: all of them, or the query nodes and the selected columns
    const int n_head = k.qs ? k.nq : k.n, e_head = k.qs ? k.es : k.e;
    const float* x = k.x;
    const float* ecur = k.ecur;
    int rc;
    if (k.qs && k.recursion == 0) {                           // no recursion to prune: the heads read rows of the inputs
        if ((rc = rpg::launch_gather_rows16(ecur, d * 4, k.q.selc, k.q.esel, d * 4, d * 4, k.es, k.s)) != RPG_OK) return rc;
        if ((rc = rpg::launch_gather_rows16(x, d * 4, k.q.qn, k.q.xq, d * 4, d * 4, k.nq, k.s)) != RPG_OK) return rc;
        ecur = k.q.esel; x = k.q.xq;
    }
    if (node_out && hipMemcpyAsync(node_out, x, (size_t)n_head * d * 4, hipMemcpyDeviceToDevice, k.s) != hipSuccess) {
        rpg::set_last_error("gnn_forward node_out", hipGetLastError());
        return RPG_ERR_LAUNCH;
    }
    if (edge_out && hipMemcpyAsync(edge_out, ecur, (size_t)e_head * d * 4, hipMemcpyDeviceToDevice, k.s) != hipSuccess) {
        rpg::set_last_error("gnn_forward edge_out", hipGetLastError());
        return RPG_ERR_LAUNCH;
    }
    if ((rc = rpg_pose_heads_f32(x, k.tensors[T_HEADN_W], k.tensors[T_HEADN_B], n_head, d, abs_pose, k.s)) != RPG_OK) return rc;
    return rpg_pose_heads_f32(ecur, k.tensors[T_HEADE_W], k.tensors[T_HEADE_B], e_head, d, rel_pose, k.s);
}

int gnn_forward_impl(const float* const* tensors, int n_tensors, const void* const* wb, const float* feat, const int64_t* esrc,
                     const int64_t* edst, int64_t node_offset, int n, int e, int d, int gnn_recursion, float* abs_pose,
                     float* rel_pose, float* node_out, float* edge_out, int32_t* status, void* workspace,
                     size_t workspace_bytes, void* stream, const QuerySel* qs = nullptr) {
    GnnCall k;
    const size_t scratch_bytes = rpg::split_scratch_bytes();
    int rc = prepare(k, tensors, n_tensors, wb, feat, esrc, edst, n, e, d, gnn_recursion, abs_pose, rel_pose, status, workspace,
                     workspace_bytes, scratch_bytes, stream, qs);
    if (rc != RPG_OK) return rc;
    rpg::ScratchScope scratch(k.g.scratch, scratch_bytes, k.s);      // stream-K partial tiles; its memset precedes every launch
    if ((rc = prepare_graph(k, esrc, edst, node_offset, status)) != RPG_OK) return rc;
    rc = (wb && rpg::tuning().gnn.fuse_agg != 0) ? layers_bf16_chained(k) : layers_general(k);
    if (rc != RPG_OK) return rc;
    return finish(k, abs_pose, rel_pose, node_out, edge_out);
}
}  // namespace

extern "C" int rpg_gnn_forward_f32(const float* const* tensors, int n_tensors, const float* feat, const int64_t* esrc,
                                   const int64_t* edst, int64_t node_offset, int n, int e, int d, int gnn_recursion, float* abs_pose,
                                   float* rel_pose, float* node_out, float* edge_out, int32_t* status, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    return gnn_forward_impl(tensors, n_tensors, nullptr, feat, esrc, edst, node_offset, n, e, d, gnn_recursion, abs_pose, rel_pose,
                            node_out, edge_out, status, workspace, workspace_bytes, stream);
}

extern "C" int rpg_gnn_forward_bf16(const float* const* tensors, int n_tensors, const void* const* weights_bf16, int n_bf16,
                                    const float* feat, const int64_t* esrc, const int64_t* edst, int64_t node_offset, int n, int e,
                                    int d, int gnn_recursion, float* abs_pose, float* rel_pose, float* node_out, float* edge_out,
                                    int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (check_bf16_table(weights_bf16, n_bf16, d) != RPG_OK) return RPG_ERR_BAD_ARG;
    return gnn_forward_impl(tensors, n_tensors, weights_bf16, feat, esrc, edst, node_offset, n, e, d, gnn_recursion, abs_pose,
                            rel_pose, node_out, edge_out, status, workspace, workspace_bytes, stream);
}

// The query-only output mode: abs_pose [q][6] of `qnodes`, rel_pose [e_sel][6] of the columns `sel` (node_out [q][d], edge_out
// [e_sel][d]).  Everything up to the last recursion runs as in rpg_gnn_forward_*; the last recursion runs its edge rows on the
// selection and its node rows on the query nodes (see query_select.hip).
extern "C" int rpg_gnn_forward_query_f32(const float* const* tensors, int n_tensors, const float* feat, const int64_t* esrc,
                                         const int64_t* edst, int64_t node_offset, int n, int e, int d, int gnn_recursion,
                                         const int64_t* sel, int e_sel, const int64_t* qnodes, int q, float* abs_pose, float* rel_pose,
                                         float* node_out, float* edge_out, int32_t* status, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    const QuerySel qs{sel, e_sel, qnodes, q};
    return gnn_forward_impl(tensors, n_tensors, nullptr, feat, esrc, edst, node_offset, n, e, d, gnn_recursion, abs_pose, rel_pose,
                            node_out, edge_out, status, workspace, workspace_bytes, stream, &qs);
}

extern "C" int rpg_gnn_forward_query_bf16(const float* const* tensors, int n_tensors, const void* const* weights_bf16, int n_bf16,
                                          const float* feat, const int64_t* esrc, const int64_t* edst, int64_t node_offset, int n, int e,
                                          int d, int gnn_recursion, const int64_t* sel, int e_sel, const int64_t* qnodes, int q,
                                          float* abs_pose, float* rel_pose, float* node_out, float* edge_out, int32_t* status,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    if (check_bf16_table(weights_bf16, n_bf16, d) != RPG_OK) return RPG_ERR_BAD_ARG;
    const QuerySel qs{sel, e_sel, qnodes, q};
    return gnn_forward_impl(tensors, n_tensors, weights_bf16, feat, esrc, edst, node_offset, n, e, d, gnn_recursion, abs_pose,
                            rel_pose, node_out, edge_out, status, workspace, workspace_bytes, stream, &qs);
}
