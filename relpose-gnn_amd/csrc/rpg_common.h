// Shared host-side helpers for the gfx950 kernels of the relpose-gnn hot path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/relpose_gnn_hip.h"

#include "tuning.h"            // the tuning keys' table and the state the launchers read, rpg::tuning() (host-only)
#include "composite_plan.h"    // kWorkspaceSkew, align_up / conv_out, the workspace layouts and the block walk of the composite forwards (host-only)
#include "rpg_coherent.h"      // agent-scope partial-slab accesses + arrival ticket (device code of winograd.hip / gemm_engine.inc)

namespace rpg {

// Last launch error text (thread local), exposed through rpg_last_error().
void set_last_error(const char* where, hipError_t e);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// Kernel timing hooks (timing.hip).  begin() returns a slot (or -1 when timing is disabled).
int timing_begin(int klass, hipStream_t s);
// work = algorithmic work of the launch (FLOP / bytes); executed = FLOP the matrix pipe really issues for it
// (padded tiles, Winograd's reduced multiply count); 0 = same as work
void timing_end(int slot, double work, hipStream_t s, double executed = 0.0);

#define RPG_CHECK_LAUNCH(where)                         \
    do {                                                \
        hipError_t _e = hipGetLastError();              \
        if (_e != hipSuccess) {                         \
            rpg::set_last_error(where, _e);             \
            return RPG_ERR_LAUNCH;                      \
        }                                               \
    } while (0)

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- NaN-propagating activation and pooling (the reference's torch semantics: relu(NaN) = NaN, max_pool2d propagates NaN) ----
// fmaxf is IEEE maxNum: fmaxf(NaN, 0) = 0 swallows a NaN, and fmaxf(NaN, -inf) = -inf.  __builtin_elementwise_maximum is IEEE
// 754-2019 maximum (NaN in -> NaN out, -0 < +0), one v_maximum3_f32 on gfx950.  Every ReLU and max-pool of the library goes
// through these.  relu4_if, an optional ReLU, is ONE maximum per element, with 0 or -inf: under IEEE maximum -inf is the identity
// for every input, NaN included (a select after the ReLU would add a v_cndmask per element to the convolution epilogues).
__device__ __forceinline__ float nan_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ float nan_max3(float a, float b, float c) { return nan_max(nan_max(a, b), c); }
__device__ __forceinline__ float relu(float y) { return nan_max(y, 0.f); }
__device__ __forceinline__ float4 relu4(float4 v) { return make_float4(relu(v.x), relu(v.y), relu(v.z), relu(v.w)); }
__device__ __forceinline__ float4 nan_max4(float4 a, float4 b) {
    return make_float4(nan_max(a.x, b.x), nan_max(a.y, b.y), nan_max(a.z, b.z), nan_max(a.w, b.w));
}
__device__ __forceinline__ float4 relu4_if(bool on, float4 v) {
    const float f = on ? 0.f : -__builtin_inff();
    return nan_max4(v, make_float4(f, f, f, f));
}


// ---- internal launchers shared between the fine-grained C ABI and the composite forwards ----
struct GatherSrc {
    const float* a[3];
    const int64_t* idx[3];
    int ld[3];
    int width[3];
    int n;
    long rows[3];          // rows of a[i] when idx[i] is given (0 = unknown: the 32-bit-offset fast path is not used)
};

int launch_conv(const float* x, const float* w, const float* scale, const float* shift, const float* residual,
                float* y, int n, int h, int wd, int cin, int cout, int kh, int kw, int stride, int pad, int relu,
                hipStream_t s, int alg_cin = 0 /* channels counted as algorithmic work; 0 = cin */);
int launch_conv_wino(const float* x, const float* u, const float* scale, const float* shift, const float* residual,
                     float* y, int n, int h, int w, int cin, int cout, int relu, hipStream_t s);
// Scratch for split-K / stream-K partial tiles (consumers run in stream order).  Inside a composite forward it is a
// slice of the CALLER's workspace (ScratchScope, set for the duration of the host-side call; a request that does not fit
// returns null and the launcher simply does not split).  The fine-grained entry points have no workspace argument:
// they draw on a library-owned pool, one block per (device, stream), which only ever grows, never while the stream is
// being captured into a HIP graph, and whose old blocks stay alive until rpg_release_scratch().
// counters (optional out): the block's arrival counters -- 4096 unsigned, zero between launches (see gemm_f32.hip) -- for the
// in-kernel combine of split tiles by the last-arriving workgroup
float* stream_scratch(hipStream_t s, size_t bytes, unsigned** counters = nullptr);
// RPG_TUNE_FIXUP_PRIO: the stream a split tile's fix-up launch goes to (s itself when off; else the high-priority companion of s,
// already waiting for what s has enqueued) and the hand-back (s waits for the companion)
hipStream_t fixup_hop_begin(hipStream_t s);
void fixup_hop_end(hipStream_t s, hipStream_t used);
struct ScratchScope {
    ScratchScope(void* p, size_t bytes, hipStream_t s);       // zeroes the slice's counter header on s (one memset node per call)
    ~ScratchScope();
    ScratchScope(const ScratchScope&) = delete;
    ScratchScope& operator=(const ScratchScope&) = delete;
};
// upper bound of what one launch asks stream_scratch for (stream-K: < 2 partial tiles of 64 KB per resident workgroup,
// <= 3 workgroups per CU; Winograd split-K tail: <= one 128-KB partial tile per CU)
size_t split_scratch_bytes();
int num_cus();
// true if the composite forward should route this 3x3/stride-1 convolution to launch_conv_wino (enabled, shape
// addressable, and large enough that the un-split K loop is not latency-bound)
bool wino_pays(int n, int h, int w, int cin, int cout);
// nested 2-D Winograd F(4x2, 3x3) (tools/probes/winograd2d.hip, probe builds)
size_t wino_weight_floats(int cout, int cin);
int launch_wino2d_weights(const float* w_ohwi, float* u2, int cout, int cin, hipStream_t s);
bool wino2d_takes(int n, int h, int w, int cin, int cout);
int launch_conv_wino2d(const float* x, const float* u2, const float* scale, const float* shift, const float* residual, float* y,
                       int n, int h, int w, int cin, int cout, int relu, hipStream_t s);
bool stem_pool_bf16_supported(int n, int h, int w, int cout);      // incl. the ranges the kernel's magic divisions are exact for
int launch_stem_pool_bf16(const void* x_nchw, int x_is_bf16, const void* wpack, const float* scale, const float* shift, void* out, int n, int h,
                          int w, hipStream_t s);
int launch_f32_to_bf16(const float* src, int ld_src, void* dst, int ld_dst, int col_off, long rows, int cols, hipStream_t s);
int launch_linear_bf16(const void* a, const void* w, const float* bias, const float* res, const int64_t* res_idx,
                       const float* res2, const int64_t* res2_idx, int ldr, float* out, int m, int k, int n_out, int relu,
                       hipStream_t s);
struct LinearBf16Out {
    void* out = nullptr;       // primary output [m][n_out]: fp32 (out_f32) or bf16; may be null when out2 is given
    int out_f32 = 1;
    void* out2 = nullptr;      // optional second output, bf16, pitch ld2 elements: bf16(relu2 ? max(y, 0) : y), y = before the primary's ReLU
    int ld2 = 0;
    int relu2 = 0;
};
int launch_linear_bf16_ex(const void* a, int lda, const void* w, const float* bias, const float* res, const int64_t* res_idx,
                          const float* res2, const int64_t* res2_idx, int ldr, const LinearBf16Out& o, int m, int k, int n_out,
                          int relu, hipStream_t s);
// Gathered residual rows added in the epilogue: out[m] += res1[idx1[m]] (+ res2[idx2[m]]), row pitch ld.
struct GatherRes {
    const float* res1;
    const int64_t* idx1;
    const float* res2;
    const int64_t* idx2;
    int ld;
};
// out_relu: optional second output of the same shape, = max(out, 0)
int launch_linear(const GatherSrc& src, const float* weight, const float* bias, const float* residual, float* out,
                  int m, int n_out, int relu, hipStream_t s, const GatherRes* gres = nullptr, float* out_relu = nullptr);
int launch_gather_add2_relu(const float* pq, const int64_t* lo, const int64_t* hi, const float* bias, float* out, int e,
                            int d, hipStream_t s);
// query_select.hip: the query-only output mode of the GNN composite.  launch_query_select checks a selection of edge columns and
// query nodes against its contract (violations counted into status, everything clamped) and builds its CSR by query row;
// launch_gather_rows16 copies rows out[i] = in[idx[i]] in 16-byte units (row pitches and width in bytes, multiples of 16).
int launch_query_select(const int64_t* esrc, const int64_t* edst, int64_t node_off, int e, int n, const int64_t* ends,
                        const int64_t* sel, int e_sel, const int64_t* qnodes, int q, int32_t* qrow, int32_t* selc, int64_t* ssrc,
                        int64_t* sdst, int32_t* srow, int32_t* qn, int32_t* rowptr, int32_t* cursor, int32_t* perm, int32_t* status,
                        hipStream_t s);
int launch_gather_rows16(const void* in, int ld_in_bytes, const int32_t* idx, void* out, int ld_out_bytes, int row_bytes, long rows,
                         hipStream_t s);

}  // namespace rpg
