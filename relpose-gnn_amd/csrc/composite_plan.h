// The plan of a composite forward (forward.hip, the end of conv_bf16.hip): how its workspace is laid out and how the ResNet's
// blocks are walked.  Each is stated once here; the size functions of the C ABI and the forwards both read it.  Host-only: nothing
// of HIP is needed, so tests/composite_plan_check.cpp compiles it with a plain host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rpg {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int conv_out(int x, int k, int s, int p) { return (x + 2 * p - k) / s + 1; }

// Workspace carving: every sub-buffer is followed by this many bytes of padding.  The activation buffers of a layer are
// whole MiB apart otherwise (256 images x 28 x 28 x 128 x 4 B = 98 MiB), so the input, residual and output streams of
// a convolution hit the same HBM channels in lock-step: measured on the layer-2 Winograd convolution, 323 us with
// 2-MiB-congruent buffers vs 272 us with >= 68 KB of skew between them (tools/probes/alias_probe.py).
constexpr size_t kWorkspaceSkew = 260 * 1024 + 4096;

// Hands out consecutive 256-byte-aligned sub-buffers of `base`, each followed by the skew.  A null base is the dry run: every take
// returns null and, once a buffer set has carved itself, `off` is the number of bytes it needs.
struct Carver {
    char* base;
    size_t off;
    template <class T>
    T* take(size_t count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += align_up(count * sizeof(T), 256) + kWorkspaceSkew;
        return p;
    }
};

// What a buffer set B needs for the given shape: B carves itself from a null base.
template <class B, class... Shape>
size_t planned_bytes(Shape... shape) {
    Carver dry{nullptr, 0};
    B b;
    b.carve(dry, shape...);
    return dry.off;
}

// The BasicBlocks of the encoder in execution order, from the stem's pooled output (h2 x w2, planes[0] channels):
//     for (ResnetWalk b(blocks, planes, h2, w2); !b.done(); b.next()) ...
// A plain value: copy it and advance the copy to look ahead.  Once done(), cin x h x w is the shape of the encoder's last
// activation tensor.
struct ResnetWalk {
    const int* blocks;
    const int* planes;
    int layer, index;      // block `index` of layer `layer`
    int stride, cin, c;    // conv1's stride, input channels, output channels
    bool ds;               // the shortcut is a 1x1 convolution (downsample) rather than the identity
    int h, w, ho, wo;      // input and output extent

    ResnetWalk(const int* blocks_, const int* planes_, int h2, int w2)
        : blocks(blocks_), planes(planes_), layer(0), index(-1), stride(1), cin(planes_[0]), c(planes_[0]), ds(false), h(h2), w(w2),
          ho(h2), wo(w2) {
        next();
    }
    bool done() const { return layer >= 4; }
    void next() {
        cin = c; h = ho; w = wo;
        ++index;
        while (layer < 4 && index >= blocks[layer]) { ++layer; index = 0; }
        if (done()) return;
        c = planes[layer];
        stride = (layer > 0 && index == 0) ? 2 : 1;
        ds = stride != 1 || cin != c;
        ho = conv_out(h, 3, stride, 1); wo = conv_out(w, 3, stride, 1);
    }
};

// Encoder: input re-laid out as NHWC with `cin_pad` channels, stem output, 4 rotating block buffers, pooled vector, and (fp32:
// scratch_bytes > 0) the split-K partial tiles.  T is the element type of the activations.
template <class T>
struct ResnetBuffers {
    int h1, w1, h2, w2;    // extent after the stem's convolution / after its max-pool
    T* in;
    T* stem;
    T* buf[4];
    T* pool;
    char* scratch;

    void carve(Carver& cv, int n, int h, int w, const int* planes, int cin_pad, size_t scratch_bytes) {
        h1 = conv_out(h, 7, 2, 3); w1 = conv_out(w, 7, 2, 3);
        h2 = conv_out(h1, 3, 2, 1); w2 = conv_out(w1, 3, 2, 1);
        // a block buffer holds the output of any block: the largest is the first block's of some layer, whatever `blocks` is
        static const int one_each[4] = {1, 1, 1, 1};
        size_t blk = 0;
        for (ResnetWalk b(one_each, planes, h2, w2); !b.done(); b.next()) {
            const size_t sz = (size_t)n * b.ho * b.wo * b.c;
            if (sz > blk) blk = sz;
        }
        in = cv.take<T>((size_t)n * h * w * cin_pad);
        stem = cv.take<T>((size_t)n * h1 * w1 * planes[0]);
        for (int i = 0; i < 4; ++i) buf[i] = cv.take<T>(blk);
        pool = cv.take<T>((size_t)n * planes[3]);
        scratch = scratch_bytes ? cv.take<char>(scratch_bytes) : nullptr;
    }
};

// GNN + heads on n nodes, e edges, d features.
struct GnnBuffers {
    int64_t* ends;                       // [4][e] src, dst, min, max end point of every edge
    int32_t *rowptr, *cursor, *perm;     // CSR by target node
    float* ebuf[2];                      // [e][d] edge features, ping-pong
    float *eraw, *hid, *msg, *att;       // [e][d] raw edge update, hidden, messages, attended (fused aggregation: [n][d] mean) messages
    float *gtp, *yat;                    // [e][3d/8] g|theta|phi, [e][d/8] attention vector
    float *agg, *nhid;                   // [n][d] aggregate, node hidden
    float* xbuf[2];                      // [n][d] node features, ping-pong
    float* node3;                        // [n][3d] per-node partial products of the split Linears
    unsigned short* abf;                 // bf16 image of a Linear's input (bf16 GNN only)
    char* scratch;                       // stream-K partial tiles
    size_t edge_bytes, node_bytes, abf_bytes;      // of one [e][d] fp32 buffer, one [n][d] fp32 buffer, abf

    void carve(Carver& cv, int n, int e, int d, size_t scratch_bytes) {
        const size_t ed = (size_t)e * d, nd = (size_t)n * d, c = d / 8;
        const size_t a_rows = e > 2 * n ? e : 2 * n;
        edge_bytes = ed * sizeof(float); node_bytes = nd * sizeof(float); abf_bytes = a_rows * d * sizeof(unsigned short);
        ends = cv.take<int64_t>((size_t)4 * e);
        rowptr = cv.take<int32_t>((size_t)n + 1);
        cursor = cv.take<int32_t>((size_t)n);
        perm = cv.take<int32_t>((size_t)e);
        ebuf[0] = cv.take<float>(ed); ebuf[1] = cv.take<float>(ed);
        eraw = cv.take<float>(ed); hid = cv.take<float>(ed); msg = cv.take<float>(ed); att = cv.take<float>(ed);
        gtp = cv.take<float>((size_t)e * 3 * c);
        yat = cv.take<float>((size_t)e * c);
        agg = cv.take<float>(nd); nhid = cv.take<float>(nd);
        xbuf[0] = cv.take<float>(nd); xbuf[1] = cv.take<float>(nd);
        node3 = cv.take<float>(3 * nd);
        abf = cv.take<unsigned short>(a_rows * d);
        scratch = cv.take<char>(scratch_bytes);
    }
};

// What the query-only output mode keeps beside GnnBuffers (carved behind it, so the full forward's layout is the same with and
// without it): the selection of e_sel edge columns and q query nodes, and the rows the pruned last recursion reads.
struct GnnQueryBuffers {
    // all null until carved from a real base (a full forward never carves them)
    int32_t *selc = nullptr, *srow = nullptr, *perm_q = nullptr;         // [e_sel] clamped columns, query row per column, CSR permutation
    int32_t *qn = nullptr, *cursor_q = nullptr, *rowptr_q = nullptr;     // [q] query nodes, [q] CSR cursor, [q + 1] CSR row pointers
    int64_t *ssrc = nullptr, *sdst = nullptr;                            // [e_sel] end points of the selected columns
    float* esel = nullptr;                                               // [e_sel][d] the selected rows of the edge features
    unsigned short* ebs = nullptr;                                       // ... and their bf16 image (bf16 Linears)
    float* xq = nullptr;                                                 // [q][d] the query rows of x
    unsigned short* xabq = nullptr;                                      // [q][2d] bf16 x | aggregate of the query rows (bf16 Linears)

    void carve(Carver& cv, int d, int e_sel, int q) {
        const size_t es = e_sel, nq = q;
        selc = cv.take<int32_t>(3 * es + 3 * nq + 1);
        ssrc = cv.take<int64_t>(2 * es);
        if (selc) { srow = selc + es; perm_q = srow + es; qn = perm_q + es; cursor_q = qn + nq; rowptr_q = cursor_q + nq; sdst = ssrc + es; }
        esel = cv.take<float>(es * d);
        ebs = cv.take<unsigned short>(es * d);
        xq = cv.take<float>(nq * d);
        xabq = cv.take<unsigned short>(nq * 2 * d);
    }
};

}  // namespace rpg
