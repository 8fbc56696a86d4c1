/*
 * relpose_gnn_hip.h -- C ABI of the MI355X (gfx950) hot path of relpose-gnn.
 *
 * The reference has no FFI of its own: its "plugin API" for this path is the PyTorch
 * nn.Module contract of PoseNetX_R2 (/root/reference/python/niantic/modules/posenet.py:920-1091)
 * and all native arithmetic lives in third-party wheels (torchvision / aten conv+BN+ReLU,
 * torch_geometric MessagePassing.propagate, torch_scatter scatter-mean).  Each entry point below
 * names the reference interface it replaces.  The host-side mirror of the nn.Module contract
 * (relpose-gnn_amd/posenet.py) binds these symbols with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to caller-owned, 16-byte aligned memory (except where
 *     marked HOST, and the uint8 frames of rpg_frames_u8_to_*, which may start at any byte); no call synchronises the device (except rpg_timing_read* and
 *     rpg_release_scratch);
 *   - the composite forwards (rpg_resnet_forward_*, rpg_gnn_forward_*) allocate nothing: all their
 *     memory, including the partial-tile scratch of the split-K / stream-K launches, is the
 *     caller's workspace (rpg_*_workspace_bytes), so they can be captured into a HIP graph as is.
 *     The fine-grained convolution / Linear entry points have no workspace argument: when a shape
 *     calls for a split-K pass they use a library-owned scratch block per (device, stream) that
 *     only grows (old blocks stay valid; never grown while the stream is being captured -- the
 *     launch then simply does not split); rpg_release_scratch() frees the pool;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *   - tensors are dense fp32, indices are int64 (the dtype of PyG's edge_index);
 *   - return value: 0 = RPG_OK, negative = error, never throws across the ABI.
 *   - activations inside the encoder are NHWC ("channels last"): x[n][h][w][c].
 */
#ifndef RELPOSE_GNN_HIP_H
#define RELPOSE_GNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPG_OK 0
#define RPG_ERR_BAD_ARG (-1)      /* null pointer, non-positive size, unsupported shape/alignment */
#define RPG_ERR_LAUNCH (-2)       /* hipLaunch / runtime error (hipGetLastError text via rpg_last_error) */
#define RPG_ERR_WORKSPACE (-3)    /* workspace_bytes smaller than rpg_*_workspace_bytes() */

#define RPG_ABI_VERSION 1

int rpg_abi_version(void);
/* HOST: static string describing the last RPG_ERR_LAUNCH on this thread ("" if none). */
const char* rpg_last_error(void);
/* Synchronises the device and frees the library-owned split-K scratch pool (see conventions). */
int rpg_release_scratch(void);

/* ------------------------------------------------------------------------------------------- */
/* Encoder primitives (replace aten conv2d + batch_norm + relu + max_pool2d + adaptive_avg_pool */
/* as reached from torchvision resnet34, call site posenet.py:1037)                              */
/* ------------------------------------------------------------------------------------------- */

/* data.x.view(N,3,H,-1) (posenet.py:1035, NCHW) -> NHWC with the channel dim padded 3 -> 4 (zero). */
int rpg_nchw3_to_nhwc4_f32(const float* x_nchw, float* y_nhwc4, int n, int h, int w, void* stream);

/* y = act( conv(x, w) * scale[c] + shift[c] (+ residual) ),  implicit GEMM on f32 MFMA.
 *   x        [n][h][w][cin]           NHWC, cin % 4 == 0
 *   w_ohwi   [cout][kh][kw][cin]      (PyTorch OIHW weight permuted once at load time)
 *   scale/shift [cout]                folded eval-mode BatchNorm: scale = gamma/sqrt(var+eps),
 *                                     shift = beta - mean*scale; scale may be NULL (=1)
 *   residual [n][ho][wo][cout] or NULL; relu != 0 applies max(.,0) last
 *   y        [n][ho][wo][cout],  ho = (h + 2*pad - kh)/stride + 1 (floor), same for wo        */
int rpg_conv2d_bn_act_nhwc_f32(const float* x, const float* w_ohwi, const float* scale, const float* shift,
                               const float* residual, float* y, int n, int h, int w, int cin, int cout,
                               int kh, int kw, int stride, int pad, int relu, void* stream);

/* The same op for the 3x3 / stride 1 / pad 1 case as a 1-D Winograd F(4,3) along the width: half the f32 MFMA work.
 *   u  [6][cout][3][cin]   transformed weights from rpg_wino43_transform_weights_f32 (once per weight load);
 *      rpg_wino43_weights_floats(cout, cin) floats = 18 * cout * cin (42 * cout * cin in a probe build that carries the nested
 *      F(4x2, 3x3) experiment of round 4, tools/probes/winograd2d.hip: its image [24][cout][cin] follows the 1-D one)
 *   cin % 4 == 0, cout % 4 == 0; x [n][h][w][cin] -> y [n][h][w][cout]; other arguments as above.            */
size_t rpg_wino43_weights_floats(int cout, int cin);
int rpg_wino43_transform_weights_f32(const float* w_ohwi /* [cout][3][3][cin] */, float* u, int cout, int cin,
                                     void* stream);
int rpg_conv3x3_wino43_bn_act_nhwc_f32(const float* x, const float* u, const float* scale, const float* shift,
                                       const float* residual, float* y, int n, int h, int w, int cin, int cout,
                                       int relu, void* stream);

/* The whole ResNet stem in one kernel: conv1 (7x7, stride 2, pad 3, 3 -> 64 channels, no bias) + bn1 (eval) + ReLU +
 * MaxPool2d(3, stride 2, padding 1) of torchvision's resnet34 (call site posenet.py:1037), straight from the NCHW input
 * of posenet.py:1035 to the pooled NHWC tensor:  x_nchw [n][3][h][w] -> y [n][hp][wp][64],
 * hc = (h - 1) / 2 + 1, hp = (hc - 1) / 2 + 1 (same for w).
 *   wpack [74][2][64]  the weight operands of the kernel's 74 tap pairs with the BatchNorm scale folded in:
 *                      wpack[kp][nf][l] = scale[ch] * W[ch][tap], ch = 32 nf + (l & 31), tap = tap_a[kp] for l < 32 and
 *                      tap_b[kp] (0 if tap_b[kp].c == -1) for l >= 32, with the table of rpg_stem_pair_table
 *                      (relpose-gnn_amd/params.py pack_stem_pairs builds it)
 *   shift [64]         folded BatchNorm shift
 * rpg_stem_pair_table: HOST arrays tap_a[74][3], tap_b[74][3] = (c, kh, kw) of the two taps of every pair.            */
int rpg_stem_conv7x7s2_bn_relu_maxpool_f32(const float* x_nchw, const float* wpack, const float* shift, float* y_nhwc,
                                           int n, int h, int w, void* stream);
int rpg_stem_pair_table(int* tap_a, int* tap_b);

/* nn.MaxPool2d(3, stride 2, padding 1), NHWC, c % 4 == 0. */
int rpg_maxpool3x3s2_nhwc_f32(const float* x, float* y, int n, int h, int w, int c, void* stream);

/* nn.AdaptiveAvgPool2d(1) + flatten: [n][hw][c] -> [n][c]. */
int rpg_global_avgpool_nhwc_f32(const float* x, float* y, int n, int hw, int c, void* stream);

/* Whole encoder: torchvision-0.9.1 ResNet (BasicBlock) forward incl. the replaced fc
 * (posenet.py:942-945, :1037).  `tensors` is a HOST array of device pointers laid out as
 * documented in relpose-gnn_amd/params.py (stem, then per block conv1/conv2/(downsample), each
 * as {w_ohwi, scale, shift, u_wino43}, then fc weight [feat][512] and bias).  u_wino43 may be NULL
 * (always for strided and 1x1 convolutions): that convolution then takes the direct implicit-GEMM
 * kernel.  The stem's fourth slot holds the wpack of rpg_stem_conv7x7s2_bn_relu_maxpool_f32 (planes[0]
 * == 64) or NULL (= re-layout + generic convolution + max-pool kernels).  `blocks[4]`/`planes[4]` HOST.
 * x_nchw [n][3][h][w] -> feat [n][feat_dim].                                                     */
size_t rpg_resnet_workspace_bytes(int n, int h, int w, const int* planes);
int rpg_resnet_forward_f32(const float* const* tensors, int n_tensors, const int* blocks, const int* planes,
                           int feat_dim, const float* x_nchw, int n, int h, int w, float* feat,
                           void* workspace, size_t workspace_bytes, void* stream);

/* bf16 encoder (BASELINE.json configs[2]: bf16 activations + bf16 MFMA convolutions, fp32 accumulate / BN epilogue).
 *   rpg_conv2d_bn_act_nhwc_bf16: x, w_ohwi, residual, y are bf16 (y is fp32 when out_f32 != 0); scale/shift fp32;
 *                                cin % 8 == 0, cout % 4 == 0; other arguments as rpg_conv2d_bn_act_nhwc_f32.
 *   rpg_resnet_forward_bf16:     tensors = per conv {w_ohwi bf16 (stem Cin padded 3 -> 8), scale f32, shift f32}, then
 *                                fc weight bf16 [feat][512], fc bias f32, then OPTIONALLY the wpack of the fused bf16 stem
 *                                below (64-channel stems; without it: re-layout + generic convolution + max-pool kernels);
 *                                x_nchw fp32 -> feat fp32 [n][feat_dim].
 *   rpg_stem_conv7x7s2_bn_relu_maxpool_bf16: the stem of the bf16 encoder in one kernel (same op chain and shapes as
 *                                rpg_stem_conv7x7s2_bn_relu_maxpool_f32; torchvision conv1 / bn1 / relu / maxpool reached from
 *                                posenet.py:1037): x_nchw fp32 [n][3][h][w] -> y bf16 [n][hp][wp][64]; inputs and weights
 *                                rounded to bf16, fp32 accumulation on v_mfma_f32_32x32x16_bf16, fp32 scale / shift / ReLU /
 *                                max, one bf16 rounding at the store.
 *                                wpack_bf16: two operand images back to back (23,552 bf16).  [11][2][64][8]: element
 *                                [s][nf][l][j] = W[ch = 32 nf + (l & 31)][c][kh][kw = j] with (c, kh) = divmod(2 s + (l >> 5), 7);
 *                                zero for j == 7 and for the 22nd (c, kh) row (the tile kernel of rounds 3-5,
 *                                RPG_TUNE_FUSED_STEM = 3).  Then [2][3][4][64][8]: element [nf][c][j][l][t] =
 *                                W[ch = 32 nf + (l & 31)][c][kh = 2 j + (l >> 5)][kw = t - 1]; zero for t == 0 and kh == 7 (the
 *                                strip-march kernel of round 6, the default).  relpose-gnn_amd/params.py pack_stem_bf16
 *                                builds both.                                                                             */
int rpg_stem_conv7x7s2_bn_relu_maxpool_bf16(const float* x_nchw, const void* wpack_bf16, const float* scale, const float* shift,
                                            void* y_nhwc_bf16, int n, int h, int w, void* stream);
/* ... and on node images that are ALREADY bf16 [n][3][h][w] (the reference's fp32 `data.x`, posenet.py:1034-1035, rounded to bf16
 * on the host so that the host-to-device copy is half the size): the kernel above rounds its fp32 input to bf16 first thing, so the
 * result is bit-identical. */
int rpg_stem_conv7x7s2_bn_relu_maxpool_bf16_xbf16(const void* x_nchw_bf16, const void* wpack_bf16, const float* scale, const float* shift,
                                                  void* y_nhwc_bf16, int n, int h, int w, void* stream);
int rpg_conv2d_bn_act_nhwc_bf16(const void* x, const void* w_ohwi, const float* scale, const float* shift,
                                const void* residual, void* y, int n, int h, int w, int cin, int cout, int kh, int kw,
                                int stride, int pad, int relu, int out_f32, void* stream);
size_t rpg_resnet_bf16_workspace_bytes(int n, int h, int w, const int* planes);
int rpg_resnet_forward_bf16(const void* const* tensors, int n_tensors, const int* blocks, const int* planes, int feat_dim,
                            const float* x_nchw, int n, int h, int w, float* feat, void* workspace,
                            size_t workspace_bytes, void* stream);
/* the same forward on bf16 node images (see rpg_stem_conv7x7s2_bn_relu_maxpool_bf16_xbf16).  Works with either stem: the fused
 * kernel (wpack as the optional last tensor, RPG_TUNE_FUSED_STEM on) or the three-kernel stem, whose re-layout pass reads the
 * bf16 pixels as they are (round 4; it used to return RPG_ERR_BAD_ARG, so a tuning knob could break a caller that stages bf16).
 * Non-finite pixels: the fused stem's padded K slots (8th kernel column, 22nd (channel, row) pair) multiply a ZERO weight with a
 * real neighbouring pixel, so an Inf / NaN pixel just outside a 7x7 window yields NaN where the reference's conv2d stays finite;
 * finite inputs (every image) are unaffected. */
int rpg_resnet_forward_bf16_xbf16(const void* const* tensors, int n_tensors, const int* blocks, const int* planes, int feat_dim,
                                  const void* x_nchw_bf16, int n, int h, int w, float* feat, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------- */
/* GNN primitives                                                                                */
/* ------------------------------------------------------------------------------------------- */

/* Index preparation for one edge list given as its two rows src[e] (message source) and dst[e] (target) -- for a
 * contiguous edge_index [2][E] pass edge_index and edge_index + E; for a column slice [e0, e1) of a batched edge_index
 * pass edge_index + e0 and edge_index + E + e0 with node_offset = first node id of the slice (ids are stored
 * relative to the whole batch, the kernels work on ids - node_offset in [0, n)):
 *   ends [4][e]    int64: sanitised source, sanitised target, min(s,t), max(s,t)
 *                  (the last two are compute_edge_features' gather indices, posenet.py:1014-1017)
 *   rowptr [n+1], perm [e]   CSR of edges grouped by TARGET node, edge ids ascending inside a
 *                  group (the order torch_scatter's CPU kernel accumulates in)
 *   cursor [n]     scratch
 *   status [1]     += number of edges with an endpoint outside [0, n) (the caller zeroes it; a
 *                  counter that several calls share accumulates); such edges are left out of the
 *                  CSR and their endpoints clamped, so no later kernel reads out of bounds.  The
 *                  host mirror raises IndexError when it reads a non-zero count back.
 * Single workgroup; e and n up to 2^20.                                                          */
int rpg_graph_prepare(const int64_t* src, const int64_t* dst, int64_t node_offset, int e, int n, int64_t* ends,
                      int32_t* rowptr, int32_t* cursor, int32_t* perm, int32_t* status, void* stream);

/* Node assembly from a pre-encoded map (the map path, PoseNetX_R2.forward_map): `x = torch.cat((query, db_batch))` of
 * dataset_7Scenes_multi.py:340-345 on encoder OUTPUT -- graph g is its query followed by its K database images, in
 * retrieval order:
 *   out[g*(K+1)]       = query_feat[g]                       query_feat [g][d]
 *   out[g*(K+1) + j]   = map_feat[neighbours[g][j-1]]        map_feat [m][d], neighbours [g][k] int64, j = 1..K
 * Index contract of rpg_graph_prepare: status [1] += number of neighbours outside [0, m) (the caller zeroes it; the host
 * mirror raises IndexError on a non-zero count); such rows are clamped into [0, m), so nothing reads out of bounds.
 * d % 4 == 0, 16-byte aligned features (RPG_ERR_BAD_ARG otherwise); row offsets are 64-bit (maps past 2 GiB).
 * One launch, no allocation, no synchronisation (graph-capturable).                                            */
int rpg_gather_graph_nodes_f32(const float* query_feat, const float* map_feat, const int64_t* neighbours, int g, int k,
                               int64_t m, int d, float* out, int32_t* status, void* stream);

/* Image retrieval against a map of descriptors: the selection step of the reference's obtain_KNNs
 * (dataset_7Scenes_multi.py:238-264) with its random draws moved into `ranks` (made on the host, retrieval.py).
 * For query g (descriptor q [g][d]) and database rows db [m][d]:
 *   s[g][r]  = <q_g, db_r> / (|q_g| |db_r|); a zero-norm vector gives 0 (sklearn's normalize)
 *   row r is allowed unless db_group[r] == q_group[g]; q_group[g] == -1, or both group arrays NULL, allows every row
 *   the allowed rows are ordered by (s descending, r ascending), a non-finite s after every finite one
 *   neighbours[g][j] = the row at position ranks[g][j] of that order; sims[g][j] (may be NULL) its similarity (NaN for a
 *   non-finite one).  ranks int32 [g][k], strictly ascending per query.
 * fp32 accumulation on the f32 matrix pipe in a fixed order that depends on d (and on the column slicing, a function of m and
 * d) only: rows with equal bits get equal similarities wherever they sit in the map, a query's result does not depend on the
 * other queries of the call, and two calls give the same bits.  The database is read once per 64 queries.
 * db_inv_norm [m]: 1 / |db_r| from rpg_row_inv_norms_f32 (cached by the caller), or NULL to have it computed into the workspace.
 * status [1] += the number of (g, j) whose rank is negative, not below query g's allowed-row count or not below
 * rpg_retrieve_max_rank(), plus the number of queries whose ranks are not strictly ascending (the caller zeroes it; the host
 * mirror raises IndexError on a non-zero count); such ranks are clamped, so nothing reads out of bounds and every written
 * neighbour is in [0, m) (row 0 for a query with no allowed row).
 * 1 <= g, 1 <= k <= 64, k <= m < 2^31, d % 4 == 0, q / db / workspace 16-byte aligned (RPG_ERR_BAD_ARG otherwise); row
 * offsets are 64-bit (maps past 2 GiB).  workspace: rpg_retrieve_workspace_bytes(g, m, d) bytes, contents irrelevant on
 * entry.  Three or four launches, no allocation, no synchronisation (graph-capturable).                               */
size_t rpg_retrieve_workspace_bytes(int g, int64_t m, int d);
int rpg_retrieve_max_rank(void);
/* HOST, no launch: what the product launch of every retrieval entry does with (g, m, d), from the launchers' own planner --
 * plan4 = (column slices, 64-column blocks per slice, 16-query tiles per workgroup NQ in {1, 2, 4}, 64-query chunks).  The
 * first two depend on (m, d) only and are part of the summation order.  RPG_ERR_BAD_ARG outside 1 <= g, 1 <= m < 2^31,
 * d > 0, d % 4 == 0.                                                                                                   */
int rpg_retrieve_plan(int g, int64_t m, int d, int32_t* plan4);
/* inv_norm[r] = 1 / |x_r| (0 for a zero row), x [m][d], d % 4 == 0, 16-byte aligned rows. */
int rpg_row_inv_norms_f32(const float* x, int64_t m, int d, float* inv_norm, void* stream);
int rpg_retrieve_cosine_f32(const float* q, const float* db, const float* db_inv_norm, const int64_t* q_group,
                            const int64_t* db_group, const int32_t* ranks, int g, int k, int64_t m, int d,
                            int64_t* neighbours, float* sims, void* workspace, size_t workspace_bytes, int32_t* status,
                            void* stream);
/* rpg_retrieve_cosine_f32 with a pose gate: retrieval restricted to the map rows near a prior pose (no counterpart in the
 * reference, whose obtain_KNNs, dataset_7Scenes_multi.py:238-264, ranks the whole split; the quaternion test is the angular
 * error of pose_utils.py:420-431, 2 acos |<p, q>| <= max_deg, stated on the cosine).  db_gate float64 [m][7] and prior float64
 * [g][7] hold (t[3], q[4] = w x y z): the un-normalised translation and the unit quaternion, the first seven columns of the
 * rows of rpg_query_pose_*_f64.  For query g:
 *   a non-finite prior component: ranked as by rpg_retrieve_cosine_f32, gate_info[g] = (1, 0)
 *   row r is inside when all 7 of db_gate[r] are finite, ((dx dx + dy dy) + dz dz) <= r2 and, with rot_gate != 0,
 *     fabs(((w1 w2 + x1 x2) + y1 y2) + z1 z2) >= cos_half -- in double, every product and sum rounded on its own
 *   rows_inside = the rows inside that the group filter allows; need = the largest of ranks[g] + 1
 *   rows_inside >= need: the rows outside are excluded like rows of the query's group, gate_info[g] = (0, rows_inside)
 *   otherwise: ranked by the group filter alone, gate_info[g] = (2, rows_inside)
 * status counts bad ranks against the rows actually ranked.  db_gate, prior and gate_info (int32 [g][2]) are given together
 * or all NULL (then this IS rpg_retrieve_cosine_f32: same launches, same bits); r2 >= 0, cos_half a number (RPG_ERR_BAD_ARG
 * otherwise).  One more sweep over m per gated query inside the selection launch; no further launch, workspace as before. */
int rpg_retrieve_cosine_gated_f32(const float* q, const float* db, const float* db_inv_norm, const int64_t* q_group,
                                  const int64_t* db_group, const int32_t* ranks, int g, int k, int64_t m, int d,
                                  const double* db_gate, const double* prior, double r2, double cos_half, int rot_gate,
                                  int32_t* gate_info, int64_t* neighbours, float* sims, void* workspace, size_t workspace_bytes,
                                  int32_t* status, void* stream);
/* rpg_retrieve_cosine_gated_f32 on a map that holds several scenes back to back (the reference evaluates scene by scene, each
 * against its own database: dataset_7Scenes_multi.py:273-345).  scene_first int64 [n_scenes + 1] (device): scene s owns the map
 * rows [scene_first[s], scene_first[s + 1]); q_scene int32 [g] (device): the scene of every query.  Query g gets, bit for bit
 * (neighbours, sims, gate_info, its share of status), what rpg_retrieve_cosine_gated_f32 gives when every row outside its scene
 * is excluded as a row of its group is: the group filter applies inside the scene, the gate counts the scene's allowed rows,
 * a query with no allowed row keeps row 0 and NaN.  The rows outside cost nothing: the product launch skips the 16-row tiles
 * no query of a 64-query chunk ranks and stores only the pairs inside a scope, the selection sweeps [lo, hi) only.  lo and hi
 * are clamped into [0, m] with hi >= lo on the device (nothing is read out of bounds whatever the arrays hold; boundaries need
 * not be multiples of 16); a q_scene[g] outside [0, n_scenes) adds 1 to status and ranks nothing for that query (row 0, NaN).
 * scene_first and q_scene both NULL: this IS rpg_retrieve_cosine_gated_f32 (same launches, same bits); exactly one NULL, or
 * n_scenes < 1 with both given: RPG_ERR_BAD_ARG.  Workspace rpg_retrieve_workspace_bytes(g, m, d) with m the whole map's row
 * count (the column slices, and with them the summation order, stay a function of (m, d)); no further launch, allocation or
 * synchronisation.                                                                                                       */
int rpg_retrieve_cosine_scoped_f32(const float* q, const float* db, const float* db_inv_norm, const int64_t* q_group,
                                   const int64_t* db_group, const int32_t* ranks, int g, int k, int64_t m, int d,
                                   const double* db_gate, const double* prior, double r2, double cos_half, int rot_gate,
                                   int32_t* gate_info, const int64_t* scene_first, const int32_t* q_scene, int n_scenes,
                                   int64_t* neighbours, float* sims, void* workspace, size_t workspace_bytes, int32_t* status,
                                   void* stream);
/* rpg_retrieve_cosine_scoped_f32 for queries that are not told their scene: they elect it (no counterpart in the reference,
 * which is handed one scene at a time).  For a query g that elects, with V = vote_top:
 *   voters     the rows at positions 0 .. V-1 of the order rpg_retrieve_cosine_f32 defines over all m rows (similarity
 *              descending, row ascending, non-finite similarities last) -- no group filter (group ids mean something inside a
 *              scene only) and no gate: the rows that call returns for ranks 0 .. V-1 without groups
 *   scene      voter row r belongs to the scene s with scene_first[s] <= r < scene_first[s + 1], the boundaries clamped into
 *              [0, m] as the scoped entry clamps them; s is found by binary search, so scene_first is expected not to descend
 *              (if it does, some voters find no owner; nothing is read out of bounds).  A row no scene owns does not vote
 *   election   the scene with the most voters; among tied scenes the one that owns the best-placed voter (NOT the lowest
 *              index); -1 with no voter
 *   output     scene_info[g] = (elected scene, its votes), q_scene[g] = elected scene
 *   retrieval  bit for bit (neighbours, sims, gate_info, share of status) what rpg_retrieve_cosine_scoped_f32 gives with
 *              q_scene[g] = the elected scene: groups and gate apply inside it; an elected -1 is an out-of-range scene there
 * A NaN query needs no special case: all its similarities are non-finite, its voters are rows 0 .. V-1.
 * elect_mode RPG_ELECT_ALL: every query elects; q_scene is an output only.  RPG_ELECT_LOST: query g elects when q_scene[g] ==
 * -1 on entry or, with a gate, when prior[g] has a non-finite component; any other query is held: scoped by q_scene[g] exactly
 * as the scoped entry does it (out-of-range values counted likewise), scene_info[g] = (q_scene[g], 0).  Elected entries of
 * q_scene are overwritten, so the next call (or replay of a captured one) holds them.
 * RPG_ERR_BAD_ARG before any launch: scene_first, q_scene or scene_info NULL or misaligned, n_scenes < 1, vote_top outside
 * [1, 64] or above m, an unknown mode, and everything the scoped entry refuses.  Workspace
 * rpg_retrieve_elect_workspace_bytes(g, m, d) >= rpg_retrieve_workspace_bytes(g, m, d): the vote keeps its keys uint32 [g][m]
 * beside the products, which it reads and never writes.  Launches: the scoped entry's, plus the vote launch (one workgroup per
 * query) between the product launch and the selection, plus with RPG_ELECT_LOST and a gate a mark launch ahead of the
 * product launch that writes -1 into q_scene where the prior is not finite.  With RPG_ELECT_ALL the product launch is the
 * unscoped one; with RPG_ELECT_LOST a scoped one in which an electing query's range is [0, m): a 16-row tile no query of the
 * 64-query chunk ranks or votes over is still skipped before its first load.  The column slices stay a function of (m, d).
 * No allocation, no synchronisation (graph-capturable).                                                                  */
#define RPG_ELECT_ALL 1
#define RPG_ELECT_LOST 2
size_t rpg_retrieve_elect_workspace_bytes(int g, int64_t m, int d);
int rpg_retrieve_cosine_elect_f32(const float* q, const float* db, const float* db_inv_norm, const int64_t* q_group,
                                  const int64_t* db_group, const int32_t* ranks, int g, int k, int64_t m, int d,
                                  const double* db_gate, const double* prior, double r2, double cos_half, int rot_gate,
                                  int32_t* gate_info, const int64_t* scene_first, int32_t* q_scene, int n_scenes, int vote_top,
                                  int elect_mode, int32_t* scene_info, int64_t* neighbours, float* sims, void* workspace,
                                  size_t workspace_bytes, int32_t* status, void* stream);
/* The update launch of a tracking loop (no counterpart in the reference, which relocalises every frame on its own,
 * testing/test.py:192-267): for each of s cameras, from this frame's pose-rule row rows [s][16] (its first seven doubles the
 * predicted (t, q)) and the consensus integers inliers int32 [s][2] = (inliers, used) of rpg_query_pose_consensus_f64:
 *   accepted when the 7 doubles are finite, inliers >= min_inliers and (double)inliers >= min_ratio * (double)used:
 *     prior[i] = rows[i][0:7], lost[i] = 0, accepted[i] = 1
 *   otherwise accepted[i] = 0, lost[i] += 1 (saturating at INT32_MAX), and once lost[i] > max_lost prior[i] = NaN (7 of them)
 * prior float64 [s][7], lost / accepted int32 [s].  One launch, one thread per camera; graph-capturable.               */
int rpg_track_update_f64(const double* rows, const int32_t* inliers, int s, int min_inliers, double min_ratio, int max_lost,
                         double* prior, int32_t* lost, int32_t* accepted, void* stream);

/* Pose recovery of an evaluation stream: per graph of ONE forward's output the query's pose and its errors, what eval_RP does
 * on the host with the model outputs (testing/test.py:213-267; pose_utils.py:340-348 qexp, :420-431 the angular error).  In
 * float64 arithmetic on the fp32 inputs, for graph i of g:
 *   ref     = the ref_node-th column, in column order, whose target is the graph's first node          (test.py:227-229)
 *   o       = pose[source of ref] - rel_pose[ref]                                                          (test.py:231)
 *   pred    = (o[:3] * pose_s + pose_m, qexp(o[3:])),  targ = the same map of the query's own target row   (test.py:248-251)
 *   out[i]  = pred[7], targ[7], |pred_t - targ_t|, 2 acos(min(1.0, max(-1.0, |<q_pred, q_targ>|))) * 180 / pi   (16 doubles)
 * with Python's min / max (a NaN dot gives -1 and an error of 360); other non-finite inputs propagate as in numpy.
 *   edge_src, edge_dst [e] int64  the two rows of the edge list the forward used (stored, or model-built), batch node ids
 *   edge_first [g + 1] or NULL    graph i's columns are [edge_first[i], edge_first[i + 1]) (clamped into [0, e]); NULL: a column
 *                                 belongs to the graph whose node range holds its target (a model-built kNN list)
 * The graphs' nodes and poses come in one of two forms:
 *   targets  node_first [g + 1] int64 (graph i owns nodes [node_first[i], node_first[i + 1])) and node_targets [n][6] fp32, the
 *            collated `data.y`; map_poses, neighbours and query_targets NULL
 *   map      node_first and node_targets NULL: graph i owns nodes [i (k + 1), (i + 1)(k + 1)), its node j >= 1 has the pose
 *            map_poses[neighbours[i][j - 1]] (map_poses [m][6] fp32, neighbours [g][k] int64; an index outside [0, m) is
 *            clamped -- rpg_gather_graph_nodes_f32 has counted it), its node 0 query_targets[i] ([g][6] fp32, or NULL: zeros)
 * A graph with fewer than ref_node + 1 edges into its first node, with a reference edge whose source lies outside the graph, or
 * (targets form) with nodes outside [0, n) gets a row of NaN and status [1] += 1 (the caller zeroes it; the host mirror raises
 * ValueError on a non-zero count, the error evaluate.reference_edge raises).  Nothing reads out of bounds.
 * out 16-byte aligned, e >= 1, g >= 1, ref_node >= 0 (RPG_ERR_BAD_ARG otherwise).  One wave per graph stepping over its columns
 * 64 at a time (ballot + popcount, stops at the hit); no floating-point atomics: the chosen column and the bits of the row do
 * not depend on arrival order.  One launch, no allocation, no synchronisation (graph-capturable).                        */
int rpg_query_pose_f64(const float* rel_pose, const int64_t* edge_src, const int64_t* edge_dst, int64_t e,
                       const int64_t* node_first, const int64_t* edge_first, int g, const float* node_targets, int64_t n,
                       const float* map_poses, int64_t m, const int64_t* neighbours, int k, const float* query_targets,
                       double pose_m0, double pose_m1, double pose_m2, double pose_s0, double pose_s1, double pose_s2,
                       int ref_node, double* out, int32_t* status, void* stream);

/* All of a query's reference edges fused into one pose.  rpg_query_pose_f64 keeps one of the edges into the query node; here every
 * such edge is one estimate of the query's pose and the row holds their combination.  Arguments, the two forms of the graphs,
 * arithmetic (float64 on the fp32 inputs, no contraction) and the row layout are those of rpg_query_pose_f64.  For graph i:
 *   used    = the first max_edges columns, in column order, whose target is the graph's first node and whose source is NOT that
 *             node (a self-edge would carry the query's own target into its estimate); C of them
 *   t_c, q_c = the pred part of the single-edge rule for used column c;  targ is unchanged
 *   fuse 0 (mean)    t = (t_0 + .. + t_{C-1}) / C;  q = S / |S| with S = sum of (q_c if <q_c, q_0> >= 0 else -q_c), both sums in
 *                    column order; q_0 where |S| = 0
 *   fuse 1 (median)  t = the component-wise median (the mean of the two middle values for even C);  q = q_c* , the medoid: c*
 *                    minimises the sum over d != c, in column order, of the angular error between q_c and q_d; ties: the lowest c
 *   C = 1            the candidate as it is: the row of rpg_query_pose_f64 at ref_node = 0, bit for bit
 *   C >= 2 and a used candidate with a non-finite component: pred[7] and both errors NaN (targ as always); not a bad graph
 *   the errors are those of the fused pose against targ, by the formulas of rpg_query_pose_f64
 * A graph without a usable edge, with a used edge whose source lies outside the graph, or (targets form) with nodes outside
 * [0, n) gets a row of NaN and status [1] += 1.  Nothing reads out of bounds.
 *   cand  [g][max_edges][16] float64 or NULL  used candidate c as a full row (pred, targ, its own errors): the row of
 *                                             rpg_query_pose_f64 at ref_node = c on a graph without self-edges; NaN past C and
 *                                             for a bad graph
 *   count [g] int32 or NULL                   the usable edges found BEFORE the cut at max_edges
 * out and cand 16-byte aligned, e >= 1, g >= 1, fuse 0 or 1, 1 <= max_edges <= 64 (RPG_ERR_BAD_ARG otherwise).  One wave per
 * graph, lane c computes candidate c; every reduction is a function of the column order only (sequential sums, ranks with ties
 * by slot, a lexicographic minimum through cross-lane moves); no floating-point atomics.  One launch, no allocation, no
 * synchronisation (graph-capturable).                                                                                    */
int rpg_query_pose_fused_f64(const float* rel_pose, const int64_t* edge_src, const int64_t* edge_dst, int64_t e,
                             const int64_t* node_first, const int64_t* edge_first, int g, const float* node_targets, int64_t n,
                             const float* map_poses, int64_t m, const int64_t* neighbours, int k, const float* query_targets,
                             double pose_m0, double pose_m1, double pose_m2, double pose_s0, double pose_s1, double pose_s2,
                             int fuse, int max_edges, double* out, double* cand, int32_t* count, int32_t* status, void* stream);

/* A query's reference edges fused by consensus, with the inlier count: the third mode of the kernel behind
 * rpg_query_pose_fused_f64 (whose `fuse` stays 0 or 1).  Candidates (used, C, t_c, q_c), the graphs' two forms, arithmetic, row
 * layout, cand, count, bad graphs and status are those of rpg_query_pose_fused_f64.  With the thresholds inlier_t (in the unit of
 * the un-normalised translation, i.e. compared after `* pose_s + pose_m`) and inlier_deg (degrees), for graph i:
 *   a candidate with a non-finite component supports nothing and is supported by nothing (support 0); a finite one supports itself
 *   finite c != d support each other when sqrt((dx dx + dy dy) + dz dz) <= inlier_t, d* = t_c - t_d, AND the angular error of
 *                    rpg_query_pose_f64 between q_c and q_d <= inlier_deg -- symmetric bit for bit
 *   support_c        the number of candidates that support c;  c* = the lowest c among those of largest support
 *   I                the candidates that support c*, in column order
 *   pred             fuse 0 (mean) over the candidates of I alone, in column order, sign-aligned to the first of them; one inlier
 *                    as it is; the errors are those of that pose against targ
 *   every used candidate non-finite: pred[7] and both errors NaN (targ as always), 0 inliers; not a bad graph.  A non-finite
 *                    candidate next to finite ones is an outlier and voids nothing, and there is no separate C = 1 case
 *   inliers [g][2] int32 or NULL   (|I|, min(count, max_edges)) per graph; (0, that minimum) for a bad graph
 * inliers 8-byte aligned, inlier_t finite and >= 0, 0 <= inlier_deg <= 360, 1 <= max_edges <= 64 (RPG_ERR_BAD_ARG otherwise).
 * Lane c counts its support as an integer over the slots in order, a butterfly of cross-lane moves takes the lexicographic maximum
 * of (support, lowest c), one ballot of every lane's test against c* is the inlier mask and its popcount |I|, lane 0 runs the
 * mean's sequential sums over the masked slots; no floating-point atomics.  One launch, no allocation, no synchronisation
 * (graph-capturable).                                                                                                    */
int rpg_query_pose_consensus_f64(const float* rel_pose, const int64_t* edge_src, const int64_t* edge_dst, int64_t e,
                                 const int64_t* node_first, const int64_t* edge_first, int g, const float* node_targets, int64_t n,
                                 const float* map_poses, int64_t m, const int64_t* neighbours, int k, const float* query_targets,
                                 double pose_m0, double pose_m1, double pose_m2, double pose_s0, double pose_s1, double pose_s2,
                                 int max_edges, double inlier_t, double inlier_deg, double* out, double* cand, int32_t* count,
                                 int32_t* inliers, int32_t* status, void* stream);

/* A query's reference edges weighted by their Monte-Carlo variance, with the predicted deviation of the fused pose: a further mode
 * of the kernel behind rpg_query_pose_fused_f64, for its fuse 0 (consensus = 0) and for rpg_query_pose_consensus_f64 (consensus =
 * 1).  Candidates (used, C, t_c, q_c), the graphs' two forms, arithmetic, row layout, cand, count, bad graphs, status, the voting,
 * I and inliers are those of the two; the thresholds are checked always and read with consensus = 1.  Beyond them:
 *   rel_var [e][6] fp32   row for row with rel_pose: the variance of ONE dropout sample of that relative pose (what
 *                         rpg_pose_heads_mc_f32 leaves); v_c[0..5] = its row at used column c, read as float64
 *   var_floor             added to every variance before the division; finite, >= 1e-30
 *   w_cj   = 1.0 / (v_c[j] + var_floor), j = 0..2                     the translation weights, per component
 *   wq_c   = 1.0 / (((v_c[3] + v_c[4]) + v_c[5]) + var_floor)         the rotation weight, one scalar
 *   v_c is UNUSABLE when one of its six values is NaN, negative or +inf
 *   over a slot set I of two or more, every sum sequential in column order:
 *            W_j = sum w_cj,  t_j = (sum w_cj t_cj) / W_j;   Wq = sum wq_c,  q = S / |S| with S = sum of (wq_c q_c if <q_c, q_first>
 *            >= 0 else -wq_c q_c), q_first the first slot of I, and q_first itself where |S| = 0
 *   over a set I of one slot the candidate as it is, W_j and Wq its own weights
 *   consensus 0   I = all C used candidates.  C >= 2 and a used candidate with a non-finite component OR an unusable variance: pred[7]
 *                 and both errors NaN (targ as always); not a bad graph.  C = 1: the candidate as it is, whatever its variance
 *   consensus 1   a candidate with an unusable variance is treated like one with a non-finite component: it supports nothing and is
 *                 supported by nothing.  The voting itself is unweighted; I = the inliers, and the weighted mean replaces the plain one
 *   spread [g][2] float64 or NULL   (sigma_t, sigma_q) = (sqrt((s_0 s_0 / W_0 + s_1 s_1 / W_1) + s_2 s_2 / W_2), sqrt(1.0 / Wq)) with
 *                 s = pose_s: the predicted standard deviation of the fused translation in the un-normalised unit and of the fused
 *                 rotation in log-quaternion units (2 sigma_q radians ~ the deviation of the rotation angle).  Both NaN where a
 *                 component of pred is NaN, for a bad graph, and for C = 1 under consensus 0 with an unusable variance
 *   when every v + var_floor of the used candidates is the same power of two, pred and the errors are those of the unweighted
 *                 mode bit for bit (scaling by a power of two commutes with every operation above)
 * rel_var not NULL and 4-byte aligned, spread 16-byte aligned, var_floor finite and >= 1e-30, consensus 0 or 1, inliers NULL with
 * consensus 0 (RPG_ERR_BAD_ARG otherwise).  Lane c reads its six variances where it makes candidate c and writes its four weights
 * to LDS beside it; usability is one more ballot next to the finite one; lane 0 runs the weighted sums over the masked slots in
 * slot order; the row goes out by the same eight 16-byte stores and spread by one more.  No floating-point atomics.  One launch,
 * no allocation, no synchronisation (graph-capturable).                                                                    */
int rpg_query_pose_weighted_f64(const float* rel_pose, const int64_t* edge_src, const int64_t* edge_dst, int64_t e,
                                const int64_t* node_first, const int64_t* edge_first, int g, const float* node_targets, int64_t n,
                                const float* map_poses, int64_t m, const int64_t* neighbours, int k, const float* query_targets,
                                double pose_m0, double pose_m1, double pose_m2, double pose_s0, double pose_s1, double pose_s2,
                                int max_edges, double inlier_t, double inlier_deg, const float* rel_var, double var_floor,
                                int consensus, double* out, double* cand, int32_t* count, int32_t* inliers, double* spread,
                                int32_t* status, void* stream);

/* torch_cluster.knn_graph(x, k, batch, loop=False, flow='source_to_target') (posenet.py:1043-1050): for every node
 * the k nearest OTHER nodes of its graph by squared Euclidean distance (k+1 nearest including itself by
 * (distance, index), self match dropped).  x [n][d]; batch [n] int64 graph id per node, nodes of a graph contiguous,
 * NULL = one graph.  edge_index: capacity [2][n*(k+1)], row stride n*(k+1); the first *total columns are valid:
 * row 0 = neighbour (source), row 1 = query node (target), grouped by target in node order, nearest first.
 * cand [n][k+1], cnt [n] scratch; total [1]; status [1] += graphs larger than 2048 nodes (unsupported).
 * k <= 64.                                                                                                   */
int rpg_knn_graph_f32(const float* x, const int64_t* batch, int n, int d, int k, int64_t* edge_index,
                      int32_t* cand, int32_t* cnt, int32_t* total, int32_t* status, void* stream);

/* The same graph for g graphs of n_per nodes each (x [g*n_per][d], graph after graph), with every column at a position known
 * before the call: k' = min(k, n_per - 1), column (v k' + t) of node v (id within the batch, 0 .. g n_per) holds its t-th nearest
 * other node in src and v in dst, both plus node_offset; src / dst [g*n_per*k'] each.  The neighbours and their order are those
 * rpg_knn_graph_f32 writes for the same x with a batch vector of g blocks of n_per: the per-pair sum rounds like that kernel's
 * (lane c adds float4 columns c, c + 64, ..., then the xor-shuffle tree 32..1), near ties included.  q_src / q_dst (both NULL or
 * both set): [g*k'], the columns into node 0 of every graph, i.e. columns g n_per k' + [0, k') of src / dst.
 * A node whose self match is not among its k+1 nearest by (distance, index) -- k+1 or more lower-numbered nodes of its graph
 * with a bit-identical row, or non-finite rows; only possible with n_per - 1 > k -- keeps k'+1 edges in the reference
 * ("irregular").  Here it gets the first k' entries of that list, which is a valid graph but not the reference's, and
 * irregular[0] += 1 per such node: a caller that needs the reference's graph reads the counter and takes rpg_knn_graph_f32.
 * Limits (RPG_ERR_BAD_ARG otherwise): g >= 1, 2 <= n_per <= 2048, g*n_per <= 2^20, 1 <= k <= 64, d % 4 == 0, x 16-byte aligned,
 * node_offset >= 0.  One workgroup per graph up to 64 nodes per graph (every unordered pair evaluated once), one per node above.
 * One launch, no allocation, no synchronisation, no count for the host (graph-capturable).                                   */
int rpg_knn_graph_uniform_f32(const float* x, int g, int n_per, int d, int k, int64_t node_offset, int64_t* src, int64_t* dst,
                              int64_t* q_src, int64_t* q_dst, int32_t* irregular, void* stream);

/* compute_edge_features (posenet.py:999-1019): out[e] = [x[min(s,t)], x[max(s,t)]], [e][2d]. */
int rpg_edge_concat_gather_f32(const float* x, const int64_t* edge_index, int e, int d, float* out, void* stream);

/* proj_edge (posenet.py:1053-1055) after its weight is split into the two node halves, W [x_lo, x_hi] = W_lo x_lo + W_hi x_hi
 * with both products computed once per node: out[e][:] = relu((pq[lo[e]][0:d] + pq[hi[e]][d:2d]) + bias), in that association.
 * pq [rows][2d] = [W_lo x | W_hi x] per node, lo / hi [e] int64 row ids in [0, rows) (NOT checked: the composite forward passes
 * the clamped end points of rpg_graph_prepare), bias [d], out [e][d]; d % 4 == 0, all float pointers 16-byte aligned.      */
int rpg_gather_add2_relu_f32(const float* pq, const int64_t* lo, const int64_t* hi, const float* bias, int e, int d, float* out,
                             void* stream);

/* out[m][n_out] = act( cat_k( a_k[idx_k[m]] ) @ W^T + bias ) (+ residual): nn.Linear over a row-wise
 * concatenation of up to three gathered sources that is never materialised
 * (my_gnn_layer.py:238, :305, :310; posenet.py:1053-1055).  idx_k == NULL means row m itself.
 *   a_k [rows_k][ld_k] uses its first width_k columns, width_k % 4 == 0, ld_k % 4 == 0
 *   W   [n_out][sum width_k] (PyTorch Linear layout), bias [n_out] or NULL
 *   residual [m][n_out] or NULL (added before the activation)                                   */
int rpg_linear_gather_f32(int n_src, const float* const* a, const int64_t* const* idx, const int* ld,
                          const int* width, const float* weight, const float* bias, const float* residual,
                          float* out, int m, int n_out, int relu, void* stream);

/* The same Linear with the epilogue the composite GNN forward uses for the split formulation of the concatenated-input
 * Linears (W [x_a, x_b, e] = W_a x_a + W_b x_b + W_e e, node terms computed once per node; my_gnn_layer.py:236-239,304-311
 * -- the reference materialises the torch.cat): the residual rows may be GATHERED,
 *   out[r] = act( cat_k(a_k[idx_k[r]]) W^T + bias + residual[(res_idx ? res_idx[r] : r) * ldr + :]
 *                                                 + residual2[res2_idx[r] * ldr + :] ),
 * and out_relu (or NULL) receives max(out, 0) as a second tensor of the same shape (the caller-side ReLU of
 * posenet.py:1064-1065 next to the un-activated value).  rows[k]: row count of a gathered source k (its index range; 0 /
 * NULL for plain sources); ldr >= n_out: row pitch of residual / residual2 (floats); res_idx == NULL and residual2 == NULL
 * = rpg_linear_gather_f32 (ldr 0 or n_out); residual2 needs res_idx AND res2_idx.  RPG_ERR_BAD_ARG: residual2 without both
 * index arrays, index arrays without residual, ldr < n_out, mis-aligned out_relu.                                        */
int rpg_linear_gather_ex_f32(int n_src, const float* const* a, const int64_t* const* idx, const int* ld,
                             const int* width, const long* rows, const float* weight, const float* bias,
                             const float* residual, const int64_t* res_idx, const float* residual2,
                             const int64_t* res2_idx, int ldr, float* out, float* out_relu, int m, int n_out, int relu,
                             void* stream);

/* HOST: what the launcher did with the last fp32 GEMM of the calling thread (rpg_linear_gather_f32 / _ex_f32,
 * rpg_conv2d_bn_act_nhwc_f32 and the composite forwards' Linears and direct convolutions; the Winograd and bf16 kernels
 * do not record).  Writes the first min(n, 15) of these ints to out and returns 15 (RPG_ERR_BAD_ARG: out NULL or n < 0):
 *    0 kernel    0 nothing launched yet | 1 tile engine | 2 linear112 (4 waves) | 3 linear112k2 (8 waves)
 *    1 BM, 2 BN, 3 BK   the workgroup tile and its K step
 *    4 waves     4 | 8 per workgroup
 *    5 loader    A operand: 0 general (64-bit row pointers, any K) | 1 buffer loads (32-bit row offsets) | 2 one tap per slot
 *    6 epi_lds   1: the epilogue transposes through LDS (16-byte accesses) | 0: direct, one float per lane
 *    7 occ       resident workgroups per CU the launcher planned with
 *    8 tiles, 9 t_dp    output tiles, and how many of them whole workgroups ran over all of K
 *   10 g_sk, 11 rem, 12 its_per   stream-K: workgroups that share the rem = tiles - t_dp other tiles, K steps each (0 0 0: none)
 *   13 combine   of the split tiles: 0 none | 1 the fix-up launch | 2 the last-arriving workgroup (RPG_TUNE_INKERNEL_FIXUP bit 0)
 *   14 fold_k    two-level accumulation period in force for this launch (0: one sequential chain; RPG_TUNE_FOLD_K)
 * A diagnostic for tests and tools: a few integer stores per launch, no effect on any launch.                           */
int rpg_gemm_last_route(int* out, int n);

/* AttentionBlock core (att.py:20-31) on rows: gtp [r][3c] = [g | theta | phi] projections,
 * y[r][i] = sum_j softmax_j(phi_i * theta_j) * g_j.                                            */
int rpg_attention_rows_f32(const float* gtp, int r, int c, float* y, void* stream);

/* torch_scatter.scatter(msg, target, dim=0, dim_size=n, reduce='mean') through the CSR of
 * rpg_graph_prepare: out[v] = sum_{p in rowptr[v]..rowptr[v+1]} msg[perm[p]] / max(count,1).
 * msg [e][d], d % 4 == 0.  (my_gnn_layer.py:279,301)                                                        */
int rpg_scatter_mean_f32(const float* msg, const int32_t* rowptr, const int32_t* perm, int n, int e, int d,
                         float* out, void* stream);

/* AttentionBlock core + mean aggregation fused (att.py:20-31, my_gnn_layer.py:279,301,304-307).  att = W y + b + msg is
 * linear in (y, msg), so mean_e(att) = W mean_e(y) + (b + mean_e(msg)): this entry point produces the two means per
 * target node through the CSR of rpg_graph_prepare, in ascending edge order,
 *   ybar[v][i] = mean_{e -> v} y_e[i]   (y_e = the attention row of gtp[e], as rpg_attention_rows_f32)       [n][c]
 *   mbar[v][:] = mean_{e -> v} msg[e][:] (+ bias[:] if the node has an incoming edge; bias may be NULL)       [n][d]
 * (mbar without bias is bit-exact rpg_scatter_mean_f32 of msg; nodes without incoming edges give zeros) and the composite
 * forward then runs att.W on n rows: agg = ybar W^T + mbar.  gtp [e][3c], msg [e][d]; c % 4 == 0, d % 4 == 0,
 * d <= 1024 * ceil(c / 64).                                                                                   */
int rpg_attention_aggregate_f32(const float* gtp, const float* msg, const int32_t* rowptr, const int32_t* perm,
                                const float* bias, int n, int e, int c, int d, float* ybar, float* mbar, void* stream);

/* The same kernel for the mean-first formulation of rpg_gnn_forward_f32: `hid` [e][d] holds the message MLP's hidden rows
 * relu(mlp.0(.)) instead of the messages, and the bias is kept apart so that the Linear behind it cannot put it on an isolated node:
 *   ybar[v][i] = as above                                                                                    [n][c]
 *   hbar[v][:] = mean_{e -> v} hid[e][:]         (bit-exact rpg_scatter_mean_f32 of hid: the same order)     [n][d]
 *   res[v][:]  = bias[:] if the node has an incoming edge, else zeros      (bias [d], required)              [n][d]
 * The composite forward then runs ONE n-row Linear, agg = [hbar ; ybar] cat(W_mlp2, W_att)^T + res, without a bias operand: a node
 * without incoming edges has hbar = ybar = res = 0 and gets agg = 0 exactly.  Shapes and limits as rpg_attention_aggregate_f32.  */
int rpg_attention_aggregate_hidden_f32(const float* gtp, const float* hid, const int32_t* rowptr, const int32_t* perm,
                                       const float* bias, int n, int e, int c, int d, float* ybar, float* hbar, float* res,
                                       void* stream);

/* Two 3-output Linear heads on the same rows, concatenated: out[r][0:3] = x W1^T + b1,
 * out[r][3:6] = x W2^T + b2 (posenet.py:1077-1091).  w6 [6][d] = cat(W1, W2), b6 [6].           */
int rpg_pose_heads_f32(const float* x, const float* w6, const float* b6, int r, int d, float* out, void* stream);

/* Monte-Carlo pose heads (csrc/mc_heads.hip): the reference's always-on F.dropout (posenet.py:1073-1075, no `training=`) and the
 * heads behind it (posenet.py:1077-1086), evaluated under s masks from ONE read of x [r][d]; the weights come from cache.
 *   y_k[o]  = scale * (sum over the KEPT columns c of x[c] w6[o][c]) + b6[o],   scale = 1.0f / (1.0f - (float)p), applied once
 *   mean[o] = (the fp32 sum of y_0 .. y_{s-1} in that order) / s
 *   var[o]  = sum_k (y_k[o] - mean[o])^2 / (s - 1), two passes in fp32; exactly 0 for s = 1
 *   samples [s][r][6] or NULL: every y_k
 * The mask is a pure function of (seed, draw, node ids, column, sample) -- Philox4x32-10, csrc/philox.h: key = (seed low, seed
 * high), counter = (a, b, k | sample << 16, draw); its four words serve columns 4k .. 4k+3, and element j is kept iff word[j] >=
 * floor(p 2^32) (evaluated in double).  state: DEVICE uint32 [2] = {draw, node_base}, read by the kernel, so that a captured graph
 * sees new values at every replay.  With off = node_base + id_offset:  a = off + (id_a ? id_a[row] : row);  b = id_b ? off +
 * id_b[row] : 0xFFFFFFFF (the node tag).  A node row passes its node id (or its row index) and no id_b; an edge row passes the
 * ids of its source and target.  So a row's masks do not depend on its position, stream slot, micro-batch, the edge order, FC
 * versus kNN graph or the "query" / "all" output mode, and two copies of the same (source, target) edge share a mask.
 * The mask SELECTS: a dropped column enters the sum as +0 whatever x holds there, so a NaN / Inf feature poisons exactly the
 * samples that keep it (and the mean and variance with them), where F.dropout, which multiplies by 0, poisons all of them.
 * Limits (RPG_ERR_BAD_ARG otherwise): 0 < p < 1, 1 <= s <= 1024, d % 4 == 0, d / 4 < 65536, id_offset >= 0, id_offset + r <=
 * 2^31 (node ids stay below 2^31: the caller's business for id_a / id_b, which are only read on the device), x and w6 16-byte
 * aligned.  One launch, no allocation, no synchronisation (graph-capturable).                                          */
int rpg_pose_heads_mc_f32(const float* x, const float* w6, const float* b6, int r, int d, double p, int s, uint64_t seed,
                          const uint32_t* state, const int64_t* id_a, const int64_t* id_b, int64_t id_offset, float* mean,
                          float* var, float* samples, void* stream);
/* state[0] += 1 (the draw counter; wraps) by a one-thread kernel: queued once behind a forward's heads, and part of a captured
 * step, so that every call / replay draws the next set of masks.                                                          */
int rpg_mc_advance(uint32_t* state, void* stream);

/* Everything after the encoder for use_gnn=True, use_AP=True, knn<=0 (posenet.py:1052-1091).
 * `tensors` HOST array of device pointers, order in params.py: 22 tensors (reference formulation) or 26 (adds the
 * node/edge column blocks of proj_edge, edge_mlp.0 and mlp.0 as separate matrices, which lets the node terms be
 * computed once per node and gathered in the edge GEMM epilogues), or 30 (adds four more, which let the fp32 forward take the
 * mean over a node's incoming edges BEFORE the message MLP's second Linear instead of after it; c = d / 8):
 *   tensors[26] [3c][d]      W_gtp W_mlp2, the product evaluated in float64 and rounded once
 *   tensors[27] [3c]         W_gtp b_mlp2 + b_gtp, likewise
 *   tensors[28] [d][d + c]   cat(W_mlp2, W_att) along the input dimension
 *   tensors[29] [d]          b_att + b_mlp2
 * mlp.2 has no activation behind it and its output is read only by g|theta|phi (a Linear) and by the mean, so
 *   gtp_k = (W_gtp W_mlp2) h_k + (W_gtp b_mlp2 + b_gtp),   agg_i = W_mlp2 hbar_i + W_att ybar_i + (b_att + b_mlp2)   (in-degree > 0)
 * with h_k = relu(mlp.0(.)) of edge k and hbar_i / ybar_i the means over the edges into node i: the e-row Linear mlp.2 goes away and
 * att.W becomes one n-row Linear over [hbar ; ybar] (rpg_attention_aggregate_hidden_f32).  Rounding changes, nothing else.  Used by
 * the fp32 forwards (the query-only one too) with RPG_TUNE_GNN_FUSE_AGG = 1; the bf16 forwards accept the 30-tensor table and keep
 * the 26-tensor formulation.
 * feat [n][d], edge rows src[e] / dst[e] with node_offset (see rpg_graph_prepare) -> abs_pose [n][6], rel_pose [e][6].
 * node_out [n][d] / edge_out [e][d]: optional (NULL to skip) copies of the final ReLU'd node and
 * edge features, i.e. the inputs of the heads; the host mirror uses them to apply the reference's
 * always-on F.dropout (posenet.py:1073-1075) before calling rpg_pose_heads_f32 itself.
 * status: device int32, see rpg_graph_prepare.                                                  */
size_t rpg_gnn_workspace_bytes(int n, int e, int d);
int rpg_gnn_forward_f32(const float* const* tensors, int n_tensors, const float* feat, const int64_t* src,
                        const int64_t* dst, int64_t node_offset, int n, int e, int d, int gnn_recursion,
                        float* abs_pose, float* rel_pose,
                        float* node_out, float* edge_out, int32_t* status, void* workspace,
                        size_t workspace_bytes, void* stream);

/* The same forward with the Linears on the bf16 matrix pipe (BASELINE configs[2]/[4] "bf16 activations"): a Linear's
 * input is rounded to bf16 on the fly, its weight is read from weights_bf16, accumulation / bias / residual / output
 * stay fp32, and everything that is not a GEMM (attention rows, scatter-mean, heads) is the fp32 kernel of above.
 * Needs the 26-tensor (split) table and d % 64 == 0.  weights_bf16: HOST array of 10 device pointers to bf16 [out][in]
 * matrices, in this order (params.pack_gnn_bf16): tensors[22] (proj node blocks), tensors[23] (edge_mlp.0 | mlp.0 node
 * blocks), tensors[24] (edge_mlp.0 edge block), edge_mlp.2, tensors[25] (mlp.0 edge block), mlp.2, att.{g|theta|phi},
 * att.W, mlp_updating.0, mlp_updating.2.  Not part of the fp32 parity claim: tolerance in tests/test_hip_bf16.py.   */
int rpg_gnn_forward_bf16(const float* const* tensors, int n_tensors, const void* const* weights_bf16, int n_bf16,
                         const float* feat, const int64_t* src, const int64_t* dst, int64_t node_offset, int n, int e, int d,
                         int gnn_recursion, float* abs_pose, float* rel_pose, float* node_out, float* edge_out,
                         int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* The query-only output mode of the two forwards above, for callers whose pose rule reads only the relative poses on the edges
 * INTO some nodes (the queries) and those nodes' own absolute poses (test.py:227-232).  The last recursion of simpleConvEdge_upt
 * (my_gnn_layer.py:293-311) has no consumer behind it, so its edge update, message MLP, attention and aggregation run on the
 * e_sel selected columns only and att.W / mlp_updating on the q query rows only; every recursion before it, proj_edge and the
 * last recursion's three per-node terms run in full.  Dead-code elimination: every value still computed is the value of the full
 * forward up to the summation order of the differently tiled GEMMs.
 *   sel    [e_sel] int64, ascending columns of the edge list: exactly the valid columns (those rpg_graph_prepare keeps) whose
 *          target is in qnodes, so that every query node's aggregate is complete
 *   qnodes [q] int64, ascending and distinct node ids in the edge list's numbering (node_offset is subtracted)
 * -> abs_pose [q][6] of qnodes, rel_pose [e_sel][6] of the sel columns in sel order; node_out [q][d] / edge_out [e_sel][d]
 * optional, the heads' inputs.  The selection's CSR keeps rpg_graph_prepare's ascending-edge order.  Index contract, as
 * rpg_graph_prepare: status += violations -- a column outside [0, e), one rpg_graph_prepare left out, one whose target is no query
 * node, a column that does not ascend, a qnode out of range or not ascending, and one more if the number of valid columns into
 * the query nodes is not e_sel; everything is clamped, so nothing reads out of bounds.  1 <= e_sel <= e, 1 <= q <= n.
 * No allocation, no synchronisation, capturable; workspace of rpg_gnn_query_workspace_bytes().                                  */
size_t rpg_gnn_query_workspace_bytes(int n, int e, int d, int e_sel, int q);
int rpg_gnn_forward_query_f32(const float* const* tensors, int n_tensors, const float* feat, const int64_t* src,
                              const int64_t* dst, int64_t node_offset, int n, int e, int d, int gnn_recursion, const int64_t* sel,
                              int e_sel, const int64_t* qnodes, int q, float* abs_pose, float* rel_pose, float* node_out,
                              float* edge_out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int rpg_gnn_forward_query_bf16(const float* const* tensors, int n_tensors, const void* const* weights_bf16, int n_bf16,
                               const float* feat, const int64_t* src, const int64_t* dst, int64_t node_offset, int n, int e, int d,
                               int gnn_recursion, const int64_t* sel, int e_sel, const int64_t* qnodes, int q, float* abs_pose,
                               float* rel_pose, float* node_out, float* edge_out, int32_t* status, void* workspace,
                               size_t workspace_bytes, void* stream);

/* One 64-channel identity BasicBlock of the bf16 encoder as a single kernel (round 5): y = relu(bn2(conv2(relu(bn1(conv1(x))))) + x),
 * both convolutions 3x3 / stride 1 / pad 1, 64 -> 64 channels, x / y bf16 NHWC [n][h][w][64] (y must not alias x), weights bf16
 * [64][3][3][64] (OHWI), folded BatchNorm scale / shift fp32 [64] (16-byte aligned).  Replaces the two aten conv2d + batch_norm +
 * relu (+ add) sequences of torchvision's BasicBlock.forward (reference call site: modules/posenet.py:1037) for ResNet34's
 * layer 1.  The intermediate activation is rounded to bf16 exactly where the two-launch path stores it: outputs are bit-identical
 * to rpg_conv2d_bn_act_nhwc_bf16 called twice.  Maps up to 62 pixels wide as they are, up to 120 (round 6: the 64 x 86 maps of the
 * 256 x 341 evaluation shape, dataset_7Scenes_multi.py:341,434) as two column strips per image whose two columns next to the cut are
 * recomputed; RPG_ERR_BAD_ARG for shapes it does not take (w < 4, w > 120, a strip's activations beyond 2^31 bytes: the caller then
 * uses two convolution calls).  No workspace, no allocation, no synchronisation. */
int rpg_basicblock64_bf16(const void* x, const void* w1_ohwi, const float* scale1, const float* shift1, const void* w2_ohwi,
                          const float* scale2, const float* shift2, void* y, int n, int h, int w, void* stream);

/* Building blocks of the above.  rpg_f32_to_bf16: dst[r][col_off + c] = bf16(src[r][c]) for c < cols (cols, col_off,
 * ld_dst % 8 == 0).  rpg_linear_bf16: out[m][n_out] (fp32) = act(a[m][k] (bf16) * weight[n_out][k]^T (bf16) + bias +
 * residual[(res_idx ? res_idx[r] : r) * ldr + :] + residual2[res2_idx[r] * ldr + :]); k % 8 == 0, n_out % 4 == 0.
 * Replaces nn.Linear (+ the gathered node terms of the split formulation), my_gnn_layer.py:236-239,304-311.         */
int rpg_f32_to_bf16(const float* src, int ld_src, void* dst, int ld_dst, int col_off, long rows, int cols, void* stream);
int rpg_linear_bf16(const void* a, const void* weight, const float* bias, const float* residual, const int64_t* res_idx,
                    const float* residual2, const int64_t* res2_idx, int ldr, float* out, int m, int k, int n_out,
                    int relu, void* stream);

/* rpg_linear_bf16_ex: the general form rpg_gnn_forward_bf16 uses -- a rows with pitch lda >= k (lda % 8 == 0), primary output `out`
 * fp32 (out_f32 = 1) or bf16 (0) or none (null, when out2 is given), and an optional second output out2 (bf16, row pitch ld2 >= n_out,
 * ld2 % 4 == 0) = bf16(relu2 ? max(y, 0) : y) with y the sum BEFORE the primary's ReLU; both rounded once, to nearest even.
 * rpg_conv_pair_bf16: the two convolutions that read the input of a down-sampling BasicBlock (torchvision BasicBlock.conv1 and
 * .downsample, reference call site modules/posenet.py:1037) as one launch: ya = relu(bn_a(conv k x k / stride / pad (x))),
 * yb = bn_b(conv 1 x 1 / stride / pad 0 (x)), both bf16 NHWC [n][ho][wo][cout]; the arithmetic of two rpg_conv2d_bn_act_nhwc_bf16
 * calls.  RPG_ERR_BAD_ARG where the pair is not taken (fewer than 8192 output pixels, cin % 32 != 0, RPG_TUNE_BF16_PAIR = 0 or
 * RPG_TUNE_BF16_DMA != 1): the caller launches the two convolutions one by one. */
int rpg_linear_bf16_ex(const void* a, int lda, const void* weight, const float* bias, const float* residual, const int64_t* res_idx,
                       const float* residual2, const int64_t* res2_idx, int ldr, void* out, int out_f32, void* out2, int ld2,
                       int relu2, int m, int k, int n_out, int relu, void* stream);
int rpg_conv_pair_bf16(const void* x, const void* wa_ohwi, const float* scale_a, const float* shift_a, void* ya, const void* wb_ohwi,
                       const float* scale_b, const float* shift_b, void* yb, int n, int h, int w, int cin, int cout, int k,
                       int stride, int pad, void* stream);

/* The streaming kernels of rpg_resnet_forward_bf16 as entry points of their own (the composite runs the same launches):
 * rpg_nchw3_to_nhwc8_bf16: images [n][3][h][w], fp32 (x_is_bf16 = 0) or bf16 (1), -> bf16 NHWC [n][h][w][8], channels 3..7 zero,
 * rounded to nearest even (the first step of the three-kernel stem, RPG_TUNE_FUSED_STEM = 0).  rpg_maxpool3x3s2_nhwc_bf16:
 * nn.MaxPool2d(3, 2, 1) on bf16 NHWC [n][h][w][c] -> [n][(h-1)/2+1][(w-1)/2+1][c], c % 8 == 0, NaN propagated.
 * rpg_global_avgpool_nhwc_bf16: nn.AdaptiveAvgPool2d(1) on bf16 [n][hw][c] -> bf16 [n][c]: the pixels summed in fp32 in ascending
 * order, one division by hw, one rounding.  Tensors 16-byte aligned; h w < 2^31 (RPG_ERR_BAD_ARG otherwise).                                                            */
int rpg_nchw3_to_nhwc8_bf16(const void* x_nchw, int x_is_bf16, void* y_nhwc8, int n, int h, int w, void* stream);
int rpg_maxpool3x3s2_nhwc_bf16(const void* x, void* y, int n, int h, int w, int c, void* stream);
int rpg_global_avgpool_nhwc_bf16(const void* x, void* y, int n, int hw, int c, void* stream);

/* HOST: what the launchers did with the last bf16 convolution, paired launch, fused BasicBlock or bf16 Linear of the calling thread
 * (rpg_conv2d_bn_act_nhwc_bf16, rpg_conv_pair_bf16, rpg_basicblock64_bf16, rpg_linear_bf16 / _ex; after a composite forward: its
 * last launch, the fc).  The dispatcher falls back from kernel to kernel silently; tests read here which one ran.
 *    family    0 nothing launched (the shape was refused) | 1 general buffer-load kernel | 2 interleaved buffer-load kernel |
 *              3 LDS-DMA kernel | 4 patch kernel | 5 patch kernel, persistent | 6 paired LDS-DMA launch | 7 fused BasicBlock |
 *              8 fused BasicBlock, persistent | 9 fused BasicBlock, two-group schedule
 *    bm, bn    the workgroup tile of the first kernel launched
 *    detail    families 1, 2: the K step; 3, 6: the LDS-DMA configuration (RPG_TUNE_BF16_DMA - 10); 4, 5, 7-9: weight stages
 *    launches  kernels launched: 2 where the tail re-tiling (RPG_TUNE_BF16_TAIL) split the rows; 3 if the main patch launch ran and
 *              every tail tile then refused the shape -- the launcher runs a second kernel family over ALL rows, while family, bm,
 *              bn and detail still name the first kernel
 * A diagnostic for tests and tools: a few integer stores per launch, no effect on any launch.  RPG_ERR_BAD_ARG: a null pointer.  */
int rpg_conv_bf16_last_route(int* family, int* bm, int* bn, int* detail, int* launches);

/* ------------------------------------------------------------------------------------------- */
/* Per-kernel timing with HIP events on the launch stream (used by bench.py for the roofline).  */
/* ------------------------------------------------------------------------------------------- */
#define RPG_TIMER_CONV 0          /* direct implicit-GEMM convolutions (stem, strided 3x3, 1x1)     */
#define RPG_TIMER_LINEAR 1        /* gathered Linear GEMMs                                         */
#define RPG_TIMER_SCATTER 2       /* scatter-mean                                                  */
#define RPG_TIMER_ATTENTION 3     /* attention rows                                                */
#define RPG_TIMER_CONV_WINO 4     /* Winograd F(4,3) 3x3/stride-1 convolutions (work = direct-conv FLOP) */
#define RPG_TIMER_ATT_AGG 5       /* fused attention rows + mean aggregation (work = algorithmic bytes)   */
#define RPG_TIMER_COUNT 6
/* enable != 0: every launch of the listed kernel classes is bracketed by hipEventRecord. */
int rpg_timing_enable(int enable);
/* Synchronises, sums the elapsed time of all bracketed launches since the last read.
 * HOST outputs, arrays of RPG_TIMER_COUNT: total milliseconds, launches, algorithmic work
 * (FLOP for CONV/LINEAR/ATTENTION, bytes for SCATTER).                                          */
int rpg_timing_read(double* ms, long long* launches, double* work);
/* The same plus executed[k]: the FLOP the matrix pipe really issues for those launches (whole padded
 * tiles; for the Winograd kernels workgroups x K steps x 48 MFMAs x waves x 4096, i.e. about half of
 * the algorithmic direct-convolution FLOP).  executed may be NULL.                               */
int rpg_timing_read_ex(double* ms, long long* launches, double* work, double* executed);

/* Measurement aid for the bf16 roofline (no counterpart in the reference, which has no bf16 path and no
 * benchmark harness -- /root/reference/python/niantic/testing/test.py:192-211 is the only caller): one launch of `workgroups` x 8
 * waves, each issuing iters x 16 v_mfma_f32_32x32x16_bf16 on registers only (no LDS / L2 / HBM traffic), operands taken from
 * `operands` (device, 65,536 x 16 bytes of bf16 values chosen by the caller: the sustained clock of the matrix pipe depends on
 * them -- on MI355X 2.50 PFLOP/s on zeros, 1.8 on random data, 2.1 on ReLU-like data).  The caller times the launch on `stream`;
 * FLOP = workgroups * 8 * iters * 16 * 32768.  `sink`: one float of device memory (never written in practice).
 * RPG_ERR_BAD_ARG: null / misaligned operands, iters outside 1 .. 2^24, workgroups outside 1 .. 65536. */
int rpg_probe_mfma_bf16(const void* operands, long iters, int workgroups, float* sink, void* stream);

/* Tuning knobs of the f32 MFMA tile engine (benchmarking aid; defaults are the tuned choice).
 *   RPG_TUNE_TILE      -1 automatic (default) | 0: 128x128 | 1: 256x64 | 2: 64x64 | 3: 128x64 workgroup tile
 *   RPG_TUNE_BK        K-step: 0 automatic (default: 32 for the 128x128 tile, else 16) | 16 | 32
 *   RPG_TUNE_EPILOGUE  1: LDS-transposed 16-byte epilogue (default) | 0: direct 4-byte epilogue
 *   RPG_TUNE_STREAMK   1: stream-K pass for the tiles that do not fill a round of resident workgroups
 *                      (default; partial tiles go to the caller's workspace / the scratch pool) | 0: off  */
#define RPG_TUNE_TILE 0
#define RPG_TUNE_BK 1
#define RPG_TUNE_EPILOGUE 2
#define RPG_TUNE_STREAMK 3
#define RPG_TUNE_GNN_SPLIT 5      /* 1: per-node precompute of the split concatenated-input Linears (default, needs
                                     the 26-tensor table) | 0: reference formulation (gathered 3-source GEMMs) */
#define RPG_TUNE_BF16_BK 6        /* K step of the bf16 convolution kernel: 32 (default) | 64 */
#define RPG_TUNE_BF16_FAST 9      /* 1: interleaved buffer-load bf16 conv kernel where Cin % 64 == 0 (default) | 0: general kernel */
#define RPG_TUNE_GNN_FUSE_AGG 13  /* 1: attention rows + mean aggregation in one kernel, att.W on node rows (default) | 0: per-edge
                                     attention rows, att.W on edge rows, separate scatter-mean (the reference's order).  With the 30-tensor
                                     table the fp32 forward also takes the mean BEFORE mlp.2 (see rpg_gnn_forward_f32): 2 = as 1, but
                                     mlp.2 stays on the edge rows (the 26-tensor formulation, for A/B in one binary).  Any other value: 1. */
#define RPG_TUNE_WAVES8 11        /* 1: 8-wave workgroups (two waves per SIMD) for the 128x128 / 128x64 tiles of the f32 tile engine where
                                     the buffer-load path applies (default) | 0: always 4-wave workgroups */
#define RPG_TUNE_FUSED_STEM 10    /* bit 0: one-kernel stem (conv7x7 + BN + ReLU + max-pool) where its operands are given (default 1) | 0: three kernels.
                                     bf16 stem only: bit 1 = the tile kernel of rounds 3-5 instead of the strip-march kernel of round 6; bit 5 = the
                                     strip-march kernel with one 32-channel half per wave and three waves per SIMD (default: both halves in one wave,
                                     two waves per SIMD; the register-weight and four-wave variants were measured slower and removed); value >> 8 =
                                     pooled rows per band
                                     (0, the default: by the launch's size).  fp32 stem: bit 7 = the strip-march kernel (round 6; opt-in: 6-12 % faster
                                     than the tile kernel, every fp32 bar holds, but it re-rolls the rounding noise of the noise-floor ratio test) */
#define RPG_TUNE_WINO_SPLIT 8     /* 1: split-K tail + fix-up for the 8-wave Winograd kernel (default) | 0: whole tiles only | n >= 2: as 1, and a part of a
                                     tile gets at least n K steps in the one-workgroup-per-tile form (default 3: one 8-node graph 1.50 ms per forward, 1.63 with 4) */
#define RPG_TUNE_FAST_LOADER 7    /* 1: buffer-load loaders + interleaved main loop where eligible (default) | 0: general loaders */
#define RPG_TUNE_WINOGRAD 4       /* 0: always the direct kernel | 1: use u_wino43 where given, kernel by size (default) |
                                     2 / 3: as 1 but always the 4-wave single-image / the 8-wave Winograd kernel | n >= 16: as 1 with the
                                     Winograd kernels from n blocks of 64 tiles x 64 channels per layer up (default 16; larger: the small layers of
                                     a small batch go to the direct kernel, which reads half the weight bytes) */
#define RPG_TUNE_WINO_SHORT 12    /* retired in round 3 with the short-K Winograd kernel it selected (measured: no gain); the key is
                                     still accepted (values >= 0) and ignored */
#define RPG_TUNE_WINO_PERSIST 14  /* 1: launches with more 8-wave tiles than CUs run the persistent kernel (one workgroup per CU walks its
                                     tiles, loads pipelined across tiles; needs Cin % 16 == 0) (default) | 2: also launches of at most one
                                     tile per CU (measured equal) | 0: one workgroup per tile */
#define RPG_TUNE_BF16_TILE 15     /* tile of the interleaved bf16 convolution kernel: -1 by shape (default) | 0: 64x64 | 1: 128x128 | 2: 256x64 | 3: 128x64 */
#define RPG_TUNE_BF16_DMA 16      /* the LDS-DMA bf16 convolution kernel (buffer_load ... lds, counted vmcnt, up to 256 x 256 tiles on 8 waves):
                                     0: off | 1: by shape (default) | 10 + i: configuration i wherever eligible (experiments) */
#define RPG_TUNE_BF16_PATCH 17    /* the patch kernel of the bf16 encoder's 3x3 / stride-1 convolutions (input patch resident in LDS, nine taps
                                     read it at shifted slots; Cin % 64 == 0): 0: off | 1: for more than 64 output channels on >= 8192
                                     pixels (default) | 2: on any eligible size | 3: as 2 with the 256 x 128 tile for every width;
                                     + 10: always three weight stages (without: four where the LDS allows -- the next step's weight fragments
                                     are then read before the barrier) */
#define RPG_TUNE_BF16_WS64 18     /* probe builds only (-DRPG_PROBE_WS64, tools/probes/conv3x3_bf16_ws64.inc: the weights-stationary layer-1
                                     experiment of round 3, correct and not faster): 1 / 2 select it.  The product library accepts 0 and
                                     returns RPG_ERR_BAD_ARG for anything else */
/* HOST: fp32 -> bf16 (round to nearest even, NaN -> quiet NaN: what the device's conversion and torch's .bfloat16() do) of a
 * contiguous host array; thread-safe, called by evaluate_stream's staging threads for the bf16 encoder's node images. */
int rpg_host_f32_to_bf16(const float* src, void* dst_bf16, size_t count);
/* HOST: the same with the instruction set named (round 6: the conversion runs on 8 / 16 lanes where the CPU has AVX2 / AVX-512F,
 * chosen once at run time by rpg_host_f32_to_bf16; every variant is the same integer arithmetic, bit-identical).  isa: 0 = what
 * rpg_host_f32_to_bf16 uses on this CPU | 1 = scalar | 2 = AVX2 | 3 = AVX-512F.  RPG_ERR_BAD_ARG for an unknown index or an
 * instruction set this CPU lacks (tests compare every available variant with the scalar one). */
int rpg_host_f32_to_bf16_isa(const float* src, void* dst_bf16, size_t count, int isa);

#define RPG_TUNE_SK_MIN_ITS 19    /* least K steps a stream-K workgroup of the fp32 GEMM engine gets (default 8) */
#define RPG_TUNE_INKERNEL_FIXUP 20  /* experiment of round 4, OFF by default (measured slower on MI355X): the partial tiles of a
                                     split launch are combined by the LAST-ARRIVING workgroup of each tile inside the producing kernel (per-tile
                                     arrival counter in the scratch block, agent-scope slab stores / loads, slabs summed in ascending k order:
                                     same bits whoever comes last) instead of by a separate fix-up launch.  Bit 0: stream-K tiles of the fp32 GEMM
                                     engine; bit 1: Winograd tail tiles of up to 8 parts (wino43_conv8_kernel only); + 4: up to 32 parts */
#define RPG_TUNE_BF16_CHUNK 21     /* bf16 encoder: runs of identity blocks on activation tensors of >= M MB are walked depth-first, `value & 4095`
                                     images at a time (their intermediates then come back from the Infinity Cache instead of HBM); M = value >> 12
                                     (0: 64 MB); 0 = off */
#define RPG_TUNE_WINO2D 22         /* probe builds only (-DRPG_PROBE_WINO2D: the nested 2-D Winograd F(4x2, 3x3) kernel, 3 instead of 4.5 multiplies per
                                     output -- correct and 13-34 % slower, profiles/r4_wino2d_nested_kernel.txt): 1 by shape | 2 wherever
                                     eligible.  The product library accepts 0 and returns RPG_ERR_BAD_ARG for anything else */
#define RPG_TUNE_BF16_LEAN_EPI 23   /* bf16 convolutions (bf16 output, optional bf16 residual): 1 (default) the branch-free epilogue of round 4 (raw buffer
                                     accesses with out-of-range offsets instead of a branch per row, 32-bit offsets, residual as a template
                                     parameter: -7..-12 % on the convolution kernels) | 0: the general epilogue of rounds 1-3 */
#define RPG_TUNE_BF16_LINEAR_DMA 24 /* bf16 GNN Linears on the edge rows (>= 192 tiles of 128 x 128): 0 the interleaved buffer-load kernel | 10 + i:
                                     configuration i of the LDS-DMA convolution kernel (a Linear is a 1 x 1 convolution over an m-pixel image) */
#define RPG_TUNE_BF16_PERSIST 25    /* bf16 3x3 / stride-1 convolutions with <= 64 output channels (layer 1) on more than one round of tiles: 1 = the persistent
                                     form of the patch kernel (one workgroup per CU walks its tiles; the next tile's first patch chunk and weights are
                                     loaded during the current tile's last chunk and epilogue).  The kernel is 10 % (in the model) to 15 % (stand-alone)
                                     faster; the default two-stream step is 2 % SLOWER with it (resident workgroups leave the other stream no gaps), so
                                     the default is 0 = one workgroup per tile.  For single-stream use */
#define RPG_TUNE_FOLD_K 26          /* fp32 Linears (rpg_linear_gather_f32 and the GNN composite): two-level accumulation -- the v_mfma_f32_32x32x2_f32
                                     accumulator is folded into a second one and restarted every `value` of K (a multiple of 64; default 256; 0 = one
                                     sequential chain over all of K as in rounds 1-4).  Summation order only: cuts the rounding noise of the K = 2048..4096
                                     GNN Linears (reference: addmm in my_gnn_layer.py:236-239,304-311 through oneDNN's blocked sums) */
#define RPG_TUNE_BF16_FUSE_BLOCK 27  /* bf16 encoder: 64-channel identity BasicBlocks (ResNet34 layer 1) run as ONE kernel, conv1 + BN + ReLU + conv2 +
                                     BN + identity + ReLU with the intermediate activation in LDS (rpg_basicblock64_bf16; bit-identical to the two
                                     convolution launches): 3 (default) = persistent form (one workgroup per CU walks the tiles, the next tile's
                                     first loads under the current tile's last steps and epilogue; launches of more than one round of tiles) |
                                     1 = one tile per workgroup (rounds 5-6a) | 5 = one tile per workgroup in the two-group schedule (waves 4-7 one
                                     barrier behind waves 0-3: load / compute phases alternate on every SIMD; experiment, not faster) | 0 = two launches */
#define RPG_TUNE_BF16_TAIL 28        /* bf16 3x3 / stride-1 convolutions on more than one round of tiles: the rows beyond the last FULL round of workgroups
                                     go to a second launch of the patch kernel with smaller tiles instead of a mostly empty round of full-size ones
                                     (49 * 2^k pixels: 3.06 / 1.53 rounds at 512 images); same arithmetic per output, bit-identical.  Bit 0 (default
                                     on): 512 x 128 -> 256 x 128 tiles (layer 2: -4..5 %); bit 1 (off): 256 x 256 -> 160 x 256 (layer 3: measured
                                     no gain); bit 2 (off, round 6): layer 2's tail on 128 x 128 tiles instead of 256 x 128 (measured: no gain,
                                     0.350 vs 0.351); 0 = always one launch */
#define RPG_TUNE_LIN112 29           /* fp32 Linears with a plain A operand, M % 112 == 0, N % 64 == 0, K % 32 == 0 and at least one 112 x 64 tile per CU (the
                                     GNN's edge GEMMs: M = 56 edges x graphs = 7 * 2^k rows): bit 0 = the exact-fit kernel on v_mfma_f32_16x16x4_f32
                                     (no stream-K split, no fix-up launch), bit 1 = its eight-wave form (the two k halves of a step on two wave
                                     groups) for launches of about one tile per CU; default 3; 0 = the 32x32x2 tile engine */
#define RPG_TUNE_FIXUP_PRIO 30       /* experiment of round 6, OFF by default: 1 = the fix-up launches of split tiles (Winograd tail, stream-K) run on a
                                     high-priority companion of the launch stream (event hand-off there and back), so that under two concurrent
                                     streams they are dispatched ahead of the other stream's queued convolution workgroups */
#define RPG_TUNE_BF16_PAIR 31        /* bf16 encoder: 1 (default) = the 3x3 / stride-2 convolution and the 1x1 / stride-2 shortcut of a down-sampling BasicBlock
                                     run as ONE launch of the LDS-DMA kernel (their tiles side by side in the grid; same arithmetic) | 0 = two launches */
/* RPG_ERR_BAD_ARG for an unknown key or a value the key does not accept (nothing changes then).  Process-wide; set keys between
 * launches, from the thread that launches. */
int rpg_set_tuning(int key, int value);
/* Read-back: *value = the value last accepted for `key`, exactly as it was passed to rpg_set_tuning (the default before any set);
 * *default_value = the key's default.  Either pointer may be NULL.  RPG_ERR_BAD_ARG for an unknown key. */
int rpg_get_tuning(int key, int* value, int* default_value);

/* ------------------------------------------------------------------------------------------- */
/* Input transform (replaces the reference's CPU transform of every node image,                 */
/* dataset_7Scenes_multi.py:290-298: torchvision-0.9.1 Resize(256) on a PIL RGB image, ToTensor, */
/* Normalize(mean = stats[0], std = sqrt(stats[1])); images from torchvision's default_loader)   */
/* ------------------------------------------------------------------------------------------- */

/* HOST: Pillow's 8-bit bilinear resampling table of one axis, in -> out samples (Image.resize(..., BILINEAR), the resampler
 * behind Resize(256)): scale = in / out, support = max(scale, 1), ksize = 2 * ceil(support) + 1; for output index o
 * bounds[2 o] = first source index, bounds[2 o + 1] = tap count, weights[o * ksize + j] = the normalised bilinear weight of tap j
 * as int32 with 22 fraction bits (zero beyond the tap count).  Returns ksize (rpg_resize_table_ksize) or RPG_ERR_BAD_ARG
 * (non-positive size, downscale beyond 31x).  bounds [2 * out], weights [out * ksize].                                    */
int rpg_resize_table_ksize(int in, int out);
int rpg_resize_table_bilinear(int in, int out, int32_t* bounds, int32_t* weights);

/* uint8 RGB frames [n][in_h][in_w][3] (HWC, what PIL's convert("RGB") holds) -> the encoder's input [n][3][out_h][out_w]:
 * the resize of rpg_resize_table_bilinear bit for bit (horizontal pass first, over the source rows the vertical pass reads; an
 * axis whose size does not change is not resampled: its tables may be NULL), then ((float)u / 255 - mean_c) / std_c in fp32
 * with correctly rounded divisions (torch's ToTensor + Normalize on the CPU); the bf16 form rounds that value to nearest even
 * (the rounding the bf16 encoder applies to fp32 input, so both give the same poses).
 *   frames    DEVICE, any byte alignment (a frame tensor may start anywhere); 64-bit offsets throughout
 *   h_*, v_*  DEVICE copies of the tables of (in_w -> out_w) and (in_h -> out_h), built once per geometry by the caller
 *   mean*, std*  per channel, by value (std = sqrt(var) rounded to fp32)
 *   out       fp32 (4-byte aligned) or bf16 (2-byte aligned)
 * One launch, no allocation, no synchronisation (graph-capturable).  rpg_frames_workspace_bytes: workspace of the launch;
 * the fused kernel keeps its intermediate in LDS, so it is 0 for every geometry taken today.                              */
size_t rpg_frames_workspace_bytes(int n, int in_h, int in_w, int out_h, int out_w);
/* HOST: the tile plan rpg_frames_u8_to_* launches this geometry with (the launcher's own planner; no device needed):
 * plan8 = {tile rows, tile columns, row tiles, column tiles per frame, source rows a tile stages (max over tiles), LDS bytes
 * per staged row, LDS bytes of a workgroup, horizontal pass | vertical pass << 1}.  RPG_ERR_BAD_ARG for the sizes the launch
 * refuses (non-positive, downscale beyond 31x, frames beyond 2^40 bytes or 2^36 output pixels).                          */
int rpg_frames_plan(int in_h, int in_w, int out_h, int out_w, int32_t* plan8);
int rpg_frames_u8_to_f32(const uint8_t* frames, int n, int in_h, int in_w, int out_h, int out_w, const int32_t* h_bounds,
                         const int32_t* h_weights, const int32_t* v_bounds, const int32_t* v_weights, float mean0, float mean1,
                         float mean2, float std0, float std1, float std2, float* out, void* workspace, size_t workspace_bytes,
                         void* stream);
int rpg_frames_u8_to_bf16(const uint8_t* frames, int n, int in_h, int in_w, int out_h, int out_w, const int32_t* h_bounds,
                          const int32_t* h_weights, const int32_t* v_bounds, const int32_t* v_weights, float mean0, float mean1,
                          float mean2, float std0, float std1, float std2, void* out_bf16, void* workspace, size_t workspace_bytes,
                          void* stream);
/* The two launches above with the statistics per frame, for a batch whose frames come from several scenes (the reference
 * reads one stats.txt per sequence, dataset_7Scenes_multi.py:290-298): scene_stats fp32 [n_scenes][6] = mean[3], std[3]
 * (device), frame_scene int32 [n] (device).  A frame of scene s equals the launch above with scene s's six floats, bit for bit.
 * status (int32, device) is incremented by the number of frames whose scene is outside [0, n_scenes); such a frame is
 * transformed with scene 0's statistics.  The statistics are on the device, so the launch cannot check them: their maker does
 * (std finite and non-zero, mean finite).  Tile plan, tables and alignment rules as above.                                */
int rpg_frames_u8_to_f32_scenes(const uint8_t* frames, int n, int in_h, int in_w, int out_h, int out_w, const int32_t* h_bounds,
                                const int32_t* h_weights, const int32_t* v_bounds, const int32_t* v_weights,
                                const float* scene_stats, const int32_t* frame_scene, int n_scenes, int32_t* status, float* out,
                                void* workspace, size_t workspace_bytes, void* stream);
int rpg_frames_u8_to_bf16_scenes(const uint8_t* frames, int n, int in_h, int in_w, int out_h, int out_w, const int32_t* h_bounds,
                                 const int32_t* h_weights, const int32_t* v_bounds, const int32_t* v_weights,
                                 const float* scene_stats, const int32_t* frame_scene, int n_scenes, int32_t* status,
                                 void* out_bf16, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RELPOSE_GNN_HIP_H */
