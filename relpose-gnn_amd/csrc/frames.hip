// uint8 camera frames -> the encoder's normalised NCHW input, on the GPU.
//
// Replaces the reference's CPU transform of every node image (dataset_7Scenes_multi.py:290-298: torchvision 0.9.1
// Resize(256) on a PIL RGB image = Pillow Image.resize(BILINEAR), ToTensor, Normalize(mean = stats[0], std = sqrt(stats[1])))
// bit for bit:
//   - the resize is Pillow's 8-bit two-pass resampler: per axis a table of (first source index, tap count) and int32 weights
//     with 22 fraction bits (rpg_resize_table_bilinear builds it exactly as Pillow's precompute_coeffs + normalize_coeffs_8bpc
//     do), acc = 2^21 + sum(src * w) in int32, clamp(acc >> 22, 0, 255); the horizontal pass runs first over the source rows
//     the vertical pass reads, the vertical pass then runs on that uint8 intermediate; a pass whose size does not change is
//     skipped;
//   - ToTensor + Normalize as CPU torch evaluates them: x = ((float)u / 255.0f - mean_c) / std_c, both divisions correctly
//     rounded (a 256-entry table per channel, built in LDS by every workgroup); the bf16 output is that value rounded to
//     nearest even, the rounding the bf16 encoder applies to fp32 input.
//
// One fused kernel: a workgroup owns a tile of output rows x columns of one frame, stages the source bytes the tile reads into
// LDS (16-byte loads for the aligned interior of every row segment, byte loads at its ends: a frame may start at any byte),
// runs the horizontal pass into an LDS intermediate and the vertical pass + normalisation from there, and stores the planes
// of [n][3][out_h][out_w] (consecutive lanes, consecutive columns).  The intermediate never leaves LDS, so the launch needs
// no workspace.  Tiles are sized on the host so that a workgroup's LDS stays within kLdsBudget (full-width tiles where the
// rows fit, narrower ones for large frames); the workgroups walk the tiles grid-stride.
//
// rpg_frames_u8_to_*_scenes: the same launch with the statistics per frame -- a device table [n_scenes][6] and one scene index per
// frame -- for batches whose frames come from several scenes.  A workgroup crosses frames as it walks its tiles, so it rebuilds
// the normalisation table when the next tile's frame is of another scene than the one the table was built for (768 divisions
// per change, a few per workgroup when a batch is sorted or mixed alike); the arithmetic of an entry is the one above.
#include "rpg_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int kPrec = 22;                        // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)
constexpr size_t kLdsBudget = 48 * 1024;         // workgroup LDS (3 workgroups per CU); see make_plan for why it always suffices
constexpr int kMaxTaps = 64;                     // host-side weight buffer of one output index (downscale <= 31x)

// ---- host: Pillow's coefficient rule (Resample.c precompute_coeffs, bilinear filter, support 1) ----------------------
int ksize_of(int in, int out) {
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return (int)ceil(fs) * 2 + 1;
}

void bounds_of(int in, int out, int o, int* xmin, int* cnt) {
    const double scale = (double)in / out;
    const double support = scale < 1.0 ? 1.0 : scale;
    const double center = (o + 0.5) * scale;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > in) hi = in;
    *xmin = lo;
    *cnt = hi - lo;
}

bool size_ok(int in, int out) { return in > 0 && out > 0 && ksize_of(in, out) <= kMaxTaps; }

// source index range [lo, hi) read by the outputs [o0, o1) of one axis (both bounds are monotonic in o)
void span_of(int in, int out, int o0, int o1, int* lo, int* hi) {
    int a, na, b, nb;
    bounds_of(in, out, o0, &a, &na);
    bounds_of(in, out, o1 - 1, &b, &nb);
    *lo = a;
    *hi = b + nb;
}

struct Plan {
    int tr = 0, tc = 0;          // tile: output rows x output columns
    int rows_max = 0;            // source rows a tile stages (max over tiles)
    int pitch = 0;               // LDS bytes per staged row (16-byte chunks)
    int hk = 0, vk = 0;          // taps per output index of the horizontal / vertical table
    bool need_h = false, need_v = false;
    size_t off_htab = 0, off_vtab = 0, off_stage = 0, off_tmp = 0, lds = 0;
    long tiles_y = 0, tiles_x = 0;
};

inline size_t up16(size_t v) { return (v + 15) & ~size_t(15); }

bool plan_for(int in_h, int in_w, int out_h, int out_w, size_t budget, int tr, int tc, Plan* p) {
    Plan q;
    q.need_h = in_w != out_w;
    q.need_v = in_h != out_h;
    q.hk = ksize_of(in_w, out_w);
    q.vk = ksize_of(in_h, out_h);
    q.tr = tr;
    q.tc = tc;
    int rows_max = 0, cols_max = 0;
    for (int y0 = 0; y0 < out_h; y0 += tr) {
        const int y1 = y0 + tr < out_h ? y0 + tr : out_h;
        int lo = y0, hi = y1;
        if (q.need_v) span_of(in_h, out_h, y0, y1, &lo, &hi);
        if (hi - lo > rows_max) rows_max = hi - lo;
    }
    for (int x0 = 0; x0 < out_w; x0 += tc) {
        const int x1 = x0 + tc < out_w ? x0 + tc : out_w;
        int lo = x0, hi = x1;
        if (q.need_h) span_of(in_w, out_w, x0, x1, &lo, &hi);
        if (hi - lo > cols_max) cols_max = hi - lo;
    }
    q.rows_max = rows_max;
    // a row segment of 3 * cols bytes starting anywhere inside a 16-byte chunk spans at most this many chunks
    q.pitch = 16 * ((3 * cols_max + 15 + 15) / 16);
    size_t off = 768 * sizeof(float);                                        // normalisation table (fp32 or bf16 entries)
    q.off_htab = off;
    off = up16(off + (q.need_h ? (size_t)tc * (2 + q.hk) * 4 : 0));
    q.off_vtab = off;
    off = up16(off + (q.need_v ? (size_t)tr * (2 + q.vk) * 4 : 0));
    q.off_stage = off;
    off = up16(off + (size_t)rows_max * q.pitch);
    q.off_tmp = off;
    off = up16(off + (q.need_h ? (size_t)3 * rows_max * tc : 0));
    q.lds = off;
    q.tiles_y = (out_h + tr - 1) / tr;
    q.tiles_x = (out_w + tc - 1) / tc;
    if (q.lds > budget) return false;
    *p = q;
    return true;
}

// Widest tiles first (full output rows: every store instruction writes contiguous columns), then the most rows per tile.
// The search ends at a 1 x 1 tile, which fits kLdsBudget for every geometry size_ok admits: at most kMaxTaps - 1 = 63 source
// rows of 63 columns (pitch 208) are staged, 3072 + 260 + 260 + 63 * 208 + 189 bytes in all, about 17 KiB.  So there is no
// second, larger budget, and the final return is never taken for sizes that passed size_ok.
bool make_plan(int in_h, int in_w, int out_h, int out_w, Plan* p) {
    static const int kRows[] = {16, 8, 4, 2, 1};
    for (int tc = out_w;; tc = (tc + 1) / 2) {
        for (int tr : kRows)
            if (plan_for(in_h, in_w, out_h, out_w, kLdsBudget, tr < out_h ? tr : out_h, tc, p)) return true;
        if (tc == 1) break;
    }
    return false;
}

// the geometries launch_frames takes (the tables, the pointers and the statistics are its own business)
bool geometry_ok(int in_h, int in_w, int out_h, int out_w) {
    if (!size_ok(in_h, out_h) || !size_ok(in_w, out_w)) return false;
    return (long)in_h * in_w * 3 <= (1L << 40) && (long)out_h * out_w <= (1L << 36);
}

// ---- device ----------------------------------------------------------------------------------------------------------
template <typename OutT>
struct Norm;
template <>
struct Norm<float> {
    __device__ static float make(float v) { return v; }
};
template <>
struct Norm<uint16_t> {                          // bf16 bits, round to nearest even (inputs are finite)
    __device__ static uint16_t make(float v) {
        const uint32_t u = __float_as_uint(v);
        return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
    }
};

struct Geometry {
    const uint8_t* frames;
    long n;
    int in_h, in_w, out_h, out_w;
    const int* hb;
    const int* hw;
    const int* vb;
    const int* vw;
};
// the launch's arguments: the geometry and where the statistics come from -- by value (one set for the launch; the layout the
// kernel has always had), or per frame from a device table (the *_scenes entries)
struct ArgsByValue : Geometry {
    float mean[3], stdv[3];
};
struct ArgsByScene : Geometry {
    const float* scene_stats;                    // [n_scenes][6] = mean[3], std[3]
    const int32_t* frame_scene;                  // [n]
    int n_scenes;
    int32_t* status;
};
template <bool SCENES>
struct FrameArgs { typedef ArgsByValue type; };
template <>
struct FrameArgs<true> { typedef ArgsByScene type; };

__device__ inline int clip8(int acc) {
    const int v = acc >> kPrec;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

template <typename OutT, bool SCENES>
__global__ __launch_bounds__(NT) void frames_kernel(const typename FrameArgs<SCENES>::type a, Plan p, OutT* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    OutT* lut = reinterpret_cast<OutT*>(lds);
    int* htab = reinterpret_cast<int*>(lds + p.off_htab);         // [tc][2] bounds (xmin relative to the staged columns), [tc][hk] weights
    int* vtab = reinterpret_cast<int*>(lds + p.off_vtab);         // [tr][2] bounds (ymin relative to the staged rows), [tr][vk] weights
    uint8_t* stage = lds + p.off_stage;
    uint8_t* tmp = lds + p.off_tmp;
    const int tid = threadIdx.x;

    if constexpr (!SCENES) {
        for (int i = tid; i < 768; i += NT) {
            const int c = i >> 8;
            const float x = ((float)(i & 255) / 255.0f - a.mean[c]) / a.stdv[c];     // ToTensor, Normalize (CPU fp32 semantics)
            lut[i] = Norm<OutT>::make(x);
        }
    }
    [[maybe_unused]] int lut_scene = -1;          // SCENES: the scene the table holds (uniform over the workgroup)

    const long row_bytes = 3L * a.in_w;
    const long frame_bytes = row_bytes * a.in_h;
    const long per_frame = p.tiles_y * p.tiles_x;
    const long total = a.n * per_frame;
    for (long wi = blockIdx.x; wi < total; wi += gridDim.x) {
        const long f = wi / per_frame;
        const long t = wi - f * per_frame;
        const int ty = (int)(t / p.tiles_x), tx = (int)(t - (long)ty * p.tiles_x);
        const int oy0 = ty * p.tr, oy1 = min(oy0 + p.tr, a.out_h);
        const int ox0 = tx * p.tc, ox1 = min(ox0 + p.tc, a.out_w);
        const int th = oy1 - oy0, tw = ox1 - ox0;
        int scene = 0;
        if constexpr (SCENES) {
            scene = a.frame_scene[f];
            if (scene < 0 || scene >= a.n_scenes) {       // counted once per frame, by the workgroup of its first tile
                if (t == 0 && tid == 0) atomicAdd(a.status, 1);
                scene = 0;
            }
        }
        int r0 = oy0, r1 = oy1, c0 = ox0, c1 = ox1;
        if (p.need_v) {
            r0 = a.vb[2 * oy0];
            r1 = a.vb[2 * (oy1 - 1)] + a.vb[2 * (oy1 - 1) + 1];
        }
        if (p.need_h) {
            c0 = a.hb[2 * ox0];
            c1 = a.hb[2 * (ox1 - 1)] + a.hb[2 * (ox1 - 1) + 1];
        }
        // tables that do not belong to this geometry: nothing is read outside the frame or the LDS image
        if (r0 < 0 || r1 > a.in_h || r1 - r0 > p.rows_max || r1 <= r0 || c0 < 0 || c1 > a.in_w || c1 <= c0 ||
            16 * ((3 * (c1 - c0) + 30) / 16) > p.pitch)
            continue;
        const int nrows = r1 - r0;
        const uint8_t* base = a.frames + f * frame_bytes + (long)r0 * row_bytes + 3L * c0;
        const int seg = 3 * (c1 - c0);

        __syncthreads();                          // the previous tile's readers are done with the LDS image
        if constexpr (SCENES) {
            if (scene != lut_scene) {                 // visible to the readers after the barrier that follows the staging
                const float* ms = a.scene_stats + 6 * (long)scene;
                for (int i = tid; i < 768; i += NT) {
                    const int c = i >> 8;
                    const float x = ((float)(i & 255) / 255.0f - ms[c]) / ms[3 + c];
                    lut[i] = Norm<OutT>::make(x);
                }
                lut_scene = scene;
            }
        }
        // ---- tables of this tile, relative to the staged rows / columns
        if (p.need_h) {
            for (int i = tid; i < tw; i += NT) {
                htab[2 * i] = a.hb[2 * (ox0 + i)] - c0;
                htab[2 * i + 1] = a.hb[2 * (ox0 + i) + 1];
            }
            int* w = htab + 2 * p.tc;
            for (int i = tid; i < tw * p.hk; i += NT) w[i] = a.hw[(long)ox0 * p.hk + i];
        }
        if (p.need_v) {
            for (int i = tid; i < th; i += NT) {
                vtab[2 * i] = a.vb[2 * (oy0 + i)] - r0;
                vtab[2 * i + 1] = a.vb[2 * (oy0 + i) + 1];
            }
            int* w = vtab + 2 * p.tr;
            for (int i = tid; i < th * p.vk; i += NT) w[i] = a.vw[(long)oy0 * p.vk + i];
        }
        // ---- stage the row segments: staged row r holds bytes [g & ~15, ...) of its segment g at LDS r * pitch
        const int nch = p.pitch / 16;
        for (int i = tid; i < nrows * nch; i += NT) {
            const int r = i / nch, q = i - r * nch;
            const uint8_t* g = base + (long)r * row_bytes;
            const uintptr_t ga = reinterpret_cast<uintptr_t>(g);
            const uintptr_t A = (ga & ~uintptr_t(15)) + 16u * (uintptr_t)q;
            const uintptr_t gend = ga + (uintptr_t)seg;
            if (A >= gend) continue;
            uint8_t* d = stage + r * p.pitch + 16 * q;
            if (A >= ga && A + 16 <= gend) {
                *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(A);
            } else {
                for (int k = 0; k < 16; ++k)
                    if (A + k >= ga && A + k < gend) d[k] = *reinterpret_cast<const uint8_t*>(A + k);
            }
        }
        __syncthreads();
        // byte (column x of the staged segment, channel c) of staged row r
        auto src_at = [&](int r, int x, int c) -> int {
            const int sh = (int)(reinterpret_cast<uintptr_t>(base + (long)r * row_bytes) & 15);
            return stage[r * p.pitch + sh + 3 * x + c];
        };
        // ---- horizontal pass into the planar intermediate tmp[c][nrows][tw]
        if (p.need_h) {
            const int* w = htab + 2 * p.tc;
            for (int i = tid; i < nrows * tw; i += NT) {
                const int r = i / tw, x = i - r * tw;
                const int xmin = htab[2 * x], cnt = htab[2 * x + 1];
                const int sh = (int)(reinterpret_cast<uintptr_t>(base + (long)r * row_bytes) & 15);
                const uint8_t* s = stage + r * p.pitch + sh + 3 * xmin;
                const int* k = w + x * p.hk;
                int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
                for (int j = 0; j < cnt; ++j) {
                    const int kj = k[j];
                    a0 += (int)s[3 * j] * kj;
                    a1 += (int)s[3 * j + 1] * kj;
                    a2 += (int)s[3 * j + 2] * kj;
                }
                tmp[(0 * nrows + r) * tw + x] = (uint8_t)clip8(a0);
                tmp[(1 * nrows + r) * tw + x] = (uint8_t)clip8(a1);
                tmp[(2 * nrows + r) * tw + x] = (uint8_t)clip8(a2);
            }
            __syncthreads();
        }
        // ---- vertical pass + normalisation, stored plane by plane
        const int* vw = vtab + 2 * p.tr;
        for (int i = tid; i < 3 * th * tw; i += NT) {
            const int c = i / (th * tw);
            const int rem = i - c * th * tw;
            const int y = rem / tw, x = rem - y * tw;
            int u;
            if (p.need_v) {
                const int ymin = vtab[2 * y], cnt = vtab[2 * y + 1];
                const int* k = vw + y * p.vk;
                int acc = 1 << (kPrec - 1);
                if (p.need_h) {
                    const uint8_t* s = tmp + (c * nrows + ymin) * tw + x;
                    for (int j = 0; j < cnt; ++j) acc += (int)s[j * tw] * k[j];
                } else {
                    for (int j = 0; j < cnt; ++j) acc += src_at(ymin + j, x, c) * k[j];
                }
                u = clip8(acc);
            } else {
                u = p.need_h ? (int)tmp[(c * nrows + y) * tw + x] : src_at(y, x, c);
            }
            out[((f * 3 + c) * a.out_h + (oy0 + y)) * (long)a.out_w + (ox0 + x)] = lut[(c << 8) + u];
        }
    }
}

bool stats_ok(const ArgsByValue& st) {
    for (int c = 0; c < 3; ++c)
        if (!(st.stdv[c] != 0.0f) || !isfinite(st.stdv[c]) || !isfinite(st.mean[c])) return false;
    return true;
}

// the statistics are on the device, checked by their maker: here only the pointers
bool stats_ok(const ArgsByScene& st) {
    return st.scene_stats && st.frame_scene && st.status && st.n_scenes >= 1 && !(reinterpret_cast<uintptr_t>(st.scene_stats) & 3u) &&
           !(reinterpret_cast<uintptr_t>(st.frame_scene) & 3u) && !(reinterpret_cast<uintptr_t>(st.status) & 3u);
}

template <typename OutT, bool SCENES>
int launch_frames(const uint8_t* frames, int n, int in_h, int in_w, int out_h, int out_w, const int32_t* hb, const int32_t* hw,
                  const int32_t* vb, const int32_t* vw, typename FrameArgs<SCENES>::type a, OutT* out, hipStream_t s) {
    if (!frames || !out || n <= 0 || !geometry_ok(in_h, in_w, out_h, out_w) ||
        (reinterpret_cast<uintptr_t>(out) % sizeof(OutT)) != 0)
        return RPG_ERR_BAD_ARG;
    if ((in_w != out_w && (!hb || !hw)) || (in_h != out_h && (!vb || !vw))) return RPG_ERR_BAD_ARG;
    if (!stats_ok(a)) return RPG_ERR_BAD_ARG;
    Plan p;
    if (!make_plan(in_h, in_w, out_h, out_w, &p)) return RPG_ERR_BAD_ARG;
    a.frames = frames;
    a.n = n;
    a.in_h = in_h;
    a.in_w = in_w;
    a.out_h = out_h;
    a.out_w = out_w;
    a.hb = hb;
    a.hw = hw;
    a.vb = vb;
    a.vw = vw;
    const long tiles = (long)n * p.tiles_y * p.tiles_x;
    const long per_cu = (long)(160 * 1024 / p.lds) < 8 ? (long)(160 * 1024 / p.lds) : 8;
    long grid = (long)rpg::num_cus() * (per_cu < 1 ? 1 : per_cu);
    if (grid > tiles) grid = tiles;
    hipLaunchKernelGGL((frames_kernel<OutT, SCENES>), dim3((unsigned)grid), dim3(NT), p.lds, s, a, p, out);
    RPG_CHECK_LAUNCH("frames_u8");
    return RPG_OK;
}

}  // namespace

extern "C" int rpg_resize_table_ksize(int in, int out) { return size_ok(in, out) ? ksize_of(in, out) : RPG_ERR_BAD_ARG; }

extern "C" int rpg_frames_plan(int in_h, int in_w, int out_h, int out_w, int32_t* plan8) {
    Plan p;
    if (!plan8 || !geometry_ok(in_h, in_w, out_h, out_w) || !make_plan(in_h, in_w, out_h, out_w, &p)) return RPG_ERR_BAD_ARG;
    const int32_t v[8] = {p.tr, p.tc, (int32_t)p.tiles_y, (int32_t)p.tiles_x, p.rows_max, p.pitch, (int32_t)p.lds,
                          (int32_t)p.need_h | (int32_t)p.need_v << 1};
    for (int i = 0; i < 8; ++i) plan8[i] = v[i];
    return RPG_OK;
}

extern "C" int rpg_resize_table_bilinear(int in, int out, int32_t* bounds, int32_t* weights) {
    if (!bounds || !weights || !size_ok(in, out)) return RPG_ERR_BAD_ARG;
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double ss = 1.0 / fs;
    const int ks = ksize_of(in, out);
    double k[kMaxTaps];
    for (int o = 0; o < out; ++o) {
        const double center = (o + 0.5) * scale;
        int xmin, cnt;
        bounds_of(in, out, o, &xmin, &cnt);
        double ww = 0.0;
        for (int x = 0; x < cnt; ++x) {
            double t = (x + xmin - center + 0.5) * ss;          // bilinear filter: max(0, 1 - |t|)
            if (t < 0.0) t = -t;
            const double w = t < 1.0 ? 1.0 - t : 0.0;
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < cnt; ++x)
            if (ww != 0.0) k[x] /= ww;
        for (int x = cnt; x < ks; ++x) k[x] = 0.0;
        for (int x = 0; x < ks; ++x)
            weights[(long)o * ks + x] = k[x] < 0 ? (int32_t)(-0.5 + k[x] * (1 << kPrec)) : (int32_t)(0.5 + k[x] * (1 << kPrec));
        bounds[2 * o] = xmin;
        bounds[2 * o + 1] = cnt;
    }
    return ks;
}

extern "C" size_t rpg_frames_workspace_bytes(int n, int in_h, int in_w, int out_h, int out_w) {
    (void)n;
    (void)in_h;
    (void)in_w;
    (void)out_h;
    (void)out_w;
    return 0;                                   // the fused kernel keeps its intermediate in LDS
}

extern "C" int rpg_frames_u8_to_f32(const uint8_t* frames, int n, int in_h, int in_w, int out_h, int out_w, const int32_t* h_bounds,
                                    const int32_t* h_weights, const int32_t* v_bounds, const int32_t* v_weights, float mean0,
                                    float mean1, float mean2, float std0, float std1, float std2, float* out, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    (void)workspace;
    if (workspace_bytes < rpg_frames_workspace_bytes(n, in_h, in_w, out_h, out_w)) return RPG_ERR_WORKSPACE;
    ArgsByValue st;                              // (the launcher fills in the geometry)
    st.mean[0] = mean0, st.mean[1] = mean1, st.mean[2] = mean2;
    st.stdv[0] = std0, st.stdv[1] = std1, st.stdv[2] = std2;
    return launch_frames<float, false>(frames, n, in_h, in_w, out_h, out_w, h_bounds, h_weights, v_bounds, v_weights, st, out,
                                       rpg::as_stream(stream));
}

extern "C" int rpg_frames_u8_to_bf16(const uint8_t* frames, int n, int in_h, int in_w, int out_h, int out_w, const int32_t* h_bounds,
                                     const int32_t* h_weights, const int32_t* v_bounds, const int32_t* v_weights, float mean0,
                                     float mean1, float mean2, float std0, float std1, float std2, void* out, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    (void)workspace;
    if (workspace_bytes < rpg_frames_workspace_bytes(n, in_h, in_w, out_h, out_w)) return RPG_ERR_WORKSPACE;
    ArgsByValue st;                              // (the launcher fills in the geometry)
    st.mean[0] = mean0, st.mean[1] = mean1, st.mean[2] = mean2;
    st.stdv[0] = std0, st.stdv[1] = std1, st.stdv[2] = std2;
    return launch_frames<uint16_t, false>(frames, n, in_h, in_w, out_h, out_w, h_bounds, h_weights, v_bounds, v_weights, st,
                                          static_cast<uint16_t*>(out), rpg::as_stream(stream));
}

extern "C" int rpg_frames_u8_to_f32_scenes(const uint8_t* frames, int n, int in_h, int in_w, int out_h, int out_w,
                                           const int32_t* h_bounds, const int32_t* h_weights, const int32_t* v_bounds,
                                           const int32_t* v_weights, const float* scene_stats, const int32_t* frame_scene,
                                           int n_scenes, int32_t* status, float* out, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    (void)workspace;
    if (workspace_bytes < rpg_frames_workspace_bytes(n, in_h, in_w, out_h, out_w)) return RPG_ERR_WORKSPACE;
    ArgsByScene st;                              // (the launcher fills in the geometry)
    st.scene_stats = scene_stats, st.frame_scene = frame_scene, st.n_scenes = n_scenes, st.status = status;
    return launch_frames<float, true>(frames, n, in_h, in_w, out_h, out_w, h_bounds, h_weights, v_bounds, v_weights, st, out,
                                      rpg::as_stream(stream));
}

extern "C" int rpg_frames_u8_to_bf16_scenes(const uint8_t* frames, int n, int in_h, int in_w, int out_h, int out_w,
                                            const int32_t* h_bounds, const int32_t* h_weights, const int32_t* v_bounds,
                                            const int32_t* v_weights, const float* scene_stats, const int32_t* frame_scene,
                                            int n_scenes, int32_t* status, void* out, void* workspace, size_t workspace_bytes,
                                            void* stream) {
    (void)workspace;
    if (workspace_bytes < rpg_frames_workspace_bytes(n, in_h, in_w, out_h, out_w)) return RPG_ERR_WORKSPACE;
    ArgsByScene st;                              // (the launcher fills in the geometry)
    st.scene_stats = scene_stats, st.frame_scene = frame_scene, st.n_scenes = n_scenes, st.status = status;
    return launch_frames<uint16_t, true>(frames, n, in_h, in_w, out_h, out_w, h_bounds, h_weights, v_bounds, v_weights, st,
                                         static_cast<uint16_t*>(out), rpg::as_stream(stream));
}
