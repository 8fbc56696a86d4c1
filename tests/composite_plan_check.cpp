// Stand-alone host check of csrc/composite_plan.h (built and run by tests/test_host.py; no GPU, no HIP).
// For every buffer set: the dry run's size, then a carve of a host buffer of exactly that size.  Every carved buffer is filled over
// the extent its user needs (restated here from the kernels' shapes, not read back from the header) with a tag of its own; all tags
// are then read again, which fails if two buffers overlap.  Every carved buffer must start 256-byte aligned (relative to the base) and end
// within the size.  ResnetWalk is compared with the nested loops it replaced.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../relpose-gnn_amd/csrc/composite_plan.h"

namespace {

int g_failures = 0;
#define EXPECT(cond, ...)                                            \
    do {                                                             \
        if (!(cond)) {                                               \
            ++g_failures;                                            \
            fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                            \
            fprintf(stderr, "\n");                                   \
        }                                                            \
    } while (0)

struct Region {
    const char* name;
    void* p;
    size_t bytes;
    size_t align = 256;      // every carved buffer; the arrays packed into one carved buffer: that of their elements
};

// Tags every region, re-reads every tag, checks alignment and bounds against [base, base + size).
void check_regions(const char* what, unsigned char* base, size_t size, const std::vector<Region>& regions) {
    for (size_t i = 0; i < regions.size(); ++i) {
        const Region& r = regions[i];
        unsigned char* p = static_cast<unsigned char*>(r.p);
        EXPECT(p != nullptr, "%s.%s is null", what, r.name);
        if (!p) continue;
        const size_t off = (size_t)(p - base);
        EXPECT(p >= base && off % r.align == 0, "%s.%s at offset %zu is not %zu-byte aligned", what, r.name, off, r.align);
        EXPECT(off + r.bytes <= size, "%s.%s ends at %zu, past the %zu bytes of the dry run", what, r.name, off + r.bytes, size);
        if (p < base || off + r.bytes > size) continue;      // reported; never written or read outside the buffer
        memset(p, (int)(i + 1), r.bytes);
    }
    for (size_t i = 0; i < regions.size(); ++i) {
        const Region& r = regions[i];
        const unsigned char* p = static_cast<const unsigned char*>(r.p);
        if (!p || p < base || (size_t)(p - base) + r.bytes > size) continue;
        const bool intact = r.bytes == 0 || (p[0] == (unsigned char)(i + 1) && memcmp(p, p + 1, r.bytes - 1) == 0);
        EXPECT(intact, "%s.%s was overwritten by another buffer", what, r.name);
    }
}

// exactly `size` bytes, uninitialised: only what a check writes is ever touched
struct HostBuffer {
    unsigned char* p;
    explicit HostBuffer(size_t size) : p(static_cast<unsigned char*>(malloc(size))) {
        if (!p) { fprintf(stderr, "out of memory (%zu bytes)\n", size); exit(2); }
    }
    ~HostBuffer() { free(p); }
    HostBuffer(const HostBuffer&) = delete;
    HostBuffer& operator=(const HostBuffer&) = delete;
};

const size_t kScratch = 1000;      // a small stand-in for the split-K scratch (odd on purpose)

template <class T>
void check_resnet(const int* planes, int n, int h, int w, int cin_pad, size_t scratch_bytes) {
    char what[96];
    snprintf(what, sizeof what, "resnet<%zu>(%d,%d,%d | %d..%d)", sizeof(T), n, h, w, planes[0], planes[3]);
    const size_t size = rpg::planned_bytes<rpg::ResnetBuffers<T>>(n, h, w, planes, cin_pad, scratch_bytes);
    HostBuffer host(size);
    rpg::Carver cv{reinterpret_cast<char*>(host.p), 0};
    rpg::ResnetBuffers<T> b;
    b.carve(cv, n, h, w, planes, cin_pad, scratch_bytes);
    EXPECT(cv.off == size, "%s: carving took %zu bytes, the dry run %zu", what, cv.off, size);
    // the extents, from the layers' shapes: conv7x7/2 pad 3, max-pool 3x3/2 pad 1, then one 3x3/2 pad 1 per later layer
    const int h1 = (h + 6 - 7) / 2 + 1, w1 = (w + 6 - 7) / 2 + 1;
    int hh = (h1 + 2 - 3) / 2 + 1, ww = (w1 + 2 - 3) / 2 + 1;
    EXPECT(b.h1 == h1 && b.w1 == w1 && b.h2 == hh && b.w2 == ww, "%s: stem extents %d %d %d %d", what, b.h1, b.w1, b.h2, b.w2);
    size_t blk = 0;
    for (int l = 0; l < 4; ++l) {
        if (l > 0) { hh = (hh + 2 - 3) / 2 + 1; ww = (ww + 2 - 3) / 2 + 1; }
        const size_t sz = (size_t)n * hh * ww * planes[l];
        if (sz > blk) blk = sz;
    }
    std::vector<Region> r = {{"in", b.in, (size_t)n * h * w * cin_pad * sizeof(T)},
                             {"stem", b.stem, (size_t)n * h1 * w1 * planes[0] * sizeof(T)},
                             {"buf0", b.buf[0], blk * sizeof(T)}, {"buf1", b.buf[1], blk * sizeof(T)},
                             {"buf2", b.buf[2], blk * sizeof(T)}, {"buf3", b.buf[3], blk * sizeof(T)},
                             {"pool", b.pool, (size_t)n * planes[3] * sizeof(T)}};
    if (scratch_bytes) r.push_back({"scratch", b.scratch, scratch_bytes});
    else EXPECT(b.scratch == nullptr, "%s: a scratch buffer without scratch bytes", what);
    check_regions(what, host.p, size, r);
}

void check_gnn(int n, int e, int d, int e_sel, int q) {      // e_sel = 0: without the query buffers
    char what[96];
    snprintf(what, sizeof what, "gnn(%d,%d,%d | %d,%d)", n, e, d, e_sel, q);
    const size_t size_g = rpg::planned_bytes<rpg::GnnBuffers>(n, e, d, kScratch);
    const size_t size = size_g + (e_sel ? rpg::planned_bytes<rpg::GnnQueryBuffers>(d, e_sel, q) : 0);
    HostBuffer host(size);
    rpg::Carver cv{reinterpret_cast<char*>(host.p), 0};
    rpg::GnnBuffers g;
    rpg::GnnQueryBuffers s;
    g.carve(cv, n, e, d, kScratch);
    EXPECT(cv.off == size_g, "%s: carving took %zu bytes, the dry run %zu", what, cv.off, size_g);
    if (e_sel) s.carve(cv, d, e_sel, q);
    EXPECT(cv.off == size, "%s: carving took %zu bytes, the dry run %zu", what, cv.off, size);
    const size_t ed = (size_t)e * d * 4, nd = (size_t)n * d * 4, c = d / 8;
    const size_t a_rows = e > 2 * n ? e : 2 * n;
    EXPECT(g.edge_bytes == ed && g.node_bytes == nd && g.abf_bytes == a_rows * d * 2, "%s: recorded sizes", what);
    std::vector<Region> r = {{"ends", g.ends, (size_t)4 * e * 8}, {"rowptr", g.rowptr, ((size_t)n + 1) * 4}, {"cursor", g.cursor, (size_t)n * 4},
                             {"perm", g.perm, (size_t)e * 4}, {"ebuf0", g.ebuf[0], ed}, {"ebuf1", g.ebuf[1], ed}, {"eraw", g.eraw, ed},
                             {"hid", g.hid, ed}, {"msg", g.msg, ed}, {"att", g.att, ed}, {"gtp", g.gtp, (size_t)e * 3 * c * 4},
                             {"yat", g.yat, (size_t)e * c * 4}, {"agg", g.agg, nd}, {"nhid", g.nhid, nd}, {"xbuf0", g.xbuf[0], nd},
                             {"xbuf1", g.xbuf[1], nd}, {"node3", g.node3, 3 * nd}, {"abf", g.abf, a_rows * d * 2},
                             {"scratch", g.scratch, kScratch}};
    if (e_sel) {
        const size_t es = e_sel, nq = q;
        const std::vector<Region> rq = {{"selc", s.selc, es * 4}, {"srow", s.srow, es * 4, 4}, {"perm_q", s.perm_q, es * 4, 4},
                                        {"qn", s.qn, nq * 4, 4}, {"cursor_q", s.cursor_q, nq * 4, 4}, {"rowptr_q", s.rowptr_q, (nq + 1) * 4, 4},
                                        {"ssrc", s.ssrc, es * 8}, {"sdst", s.sdst, es * 8, 8}, {"esel", s.esel, es * d * 4}, {"ebs", s.ebs, es * d * 2},
                                        {"xq", s.xq, nq * d * 4}, {"xabq", s.xabq, nq * 2 * d * 2}};
        r.insert(r.end(), rq.begin(), rq.end());
    } else {
        EXPECT(!s.selc && !s.srow && !s.perm_q && !s.qn && !s.cursor_q && !s.rowptr_q && !s.ssrc && !s.sdst && !s.esel && !s.ebs && !s.xq && !s.xabq,
               "%s: query buffers that were never carved are not null", what);
    }
    // the bf16 GNN places [e][2d], [n][2d], [n][d] and [n][d/8] bf16 tensors in eraw / hid, nhid, agg and abf
    EXPECT((size_t)2 * e * d * 2 <= g.edge_bytes && (size_t)n * 2 * d * 2 <= g.node_bytes && (size_t)n * c * 2 <= g.abf_bytes, "%s: aliased bf16 tensors", what);
    check_regions(what, host.p, size, r);
}

// the dry run hands out no pointers
void check_dry_run() {
    rpg::Carver dry{nullptr, 0};
    EXPECT(dry.take<float>(10) == nullptr && dry.take<char>(1) == nullptr, "a dry take returned a pointer");
    EXPECT(dry.off == 2 * (256 + rpg::kWorkspaceSkew), "dry offset %zu", dry.off);
    rpg::GnnBuffers g;
    rpg::GnnQueryBuffers s;
    g.carve(dry, 8, 56, 64, kScratch);
    s.carve(dry, 64, 7, 1);
    EXPECT(!g.ends && !g.scratch && !g.abf && !s.selc && !s.sdst && !s.rowptr_q && !s.xabq, "a dry carve produced a pointer");
}

void check_walk(const int* blocks, const int* planes, int h2, int w2) {
    rpg::ResnetWalk b(blocks, planes, h2, w2);
    int cin = planes[0], hh = h2, ww = w2, count = 0;
    for (int l = 0; l < 4; ++l)
        for (int i = 0; i < blocks[l]; ++i) {
            const int stride = (l > 0 && i == 0) ? 2 : 1, c = planes[l];
            const int ho = (hh + 2 - 3) / stride + 1, wo = (ww + 2 - 3) / stride + 1;
            EXPECT(!b.done(), "walk ended after %d blocks", count);
            if (b.done()) return;
            EXPECT(b.layer == l && b.index == i && b.stride == stride && b.cin == cin && b.c == c && b.ds == (stride != 1 || cin != c) &&
                       b.h == hh && b.w == ww && b.ho == ho && b.wo == wo,
                   "block %d.%d: walk says %d.%d stride %d %d->%d ds %d %dx%d->%dx%d", l, i, b.layer, b.index, b.stride, b.cin, b.c, (int)b.ds,
                   b.h, b.w, b.ho, b.wo);
            rpg::ResnetWalk ahead = b;      // a copy advances on its own
            ahead.next();
            EXPECT(b.layer == l && b.index == i, "advancing a copy moved the original");
            cin = c; hh = ho; ww = wo;
            ++count;
            b.next();
        }
    EXPECT(b.done(), "walk goes on after %d blocks", count);
    EXPECT(b.cin == cin && b.h == hh && b.w == ww, "after the walk: %d x %d x %d, expected %d x %d x %d", b.cin, b.h, b.w, cin, hh, ww);
}

}  // namespace

int main() {
    check_dry_run();

    const int resnet34[4] = {64, 128, 256, 512}, tiny[4] = {8, 16, 32, 64}, steep[4] = {8, 64, 512, 4096};
    const int shapes34[4][3] = {{1, 224, 224}, {8, 256, 341}, {256, 224, 224}, {3, 33, 47}};
    for (const int* s : shapes34) {
        check_resnet<float>(resnet34, s[0], s[1], s[2], 4, kScratch);
        check_resnet<unsigned short>(resnet34, s[0], s[1], s[2], 8, 0);
    }
    check_resnet<float>(tiny, 2, 32, 40, 4, kScratch);
    check_resnet<unsigned short>(tiny, 2, 32, 40, 8, 0);
    check_resnet<float>(steep, 2, 64, 64, 4, kScratch);            // the LAST layer owns the largest block buffer
    check_resnet<unsigned short>(steep, 2, 64, 64, 8, 0);

    const int gnn[6][3] = {{8, 56, 2048}, {256, 1792, 2048}, {8, 56, 64}, {3, 1, 32}, {2000, 100, 64}, {1, 1, 32}};      // incl. e < 2n
    for (const int* s : gnn) check_gnn(s[0], s[1], s[2], 0, 0);
    const int query[3][5] = {{8, 56, 64, 7, 1}, {256, 1792, 2048, 224, 32}, {8, 56, 64, 56, 8}};
    for (const int* s : query) check_gnn(s[0], s[1], s[2], s[3], s[4]);

    const int block_sets[5][4] = {{3, 4, 6, 3}, {1, 1, 1, 1}, {2, 2, 2, 2}, {1, 0, 2, 1}, {0, 0, 0, 0}};
    const int flat[4] = {64, 64, 64, 64};
    for (const int* bl : block_sets) {
        check_walk(bl, resnet34, 56, 56);
        check_walk(bl, steep, 9, 12);
        check_walk(bl, flat, 7, 5);
    }

    if (g_failures) {
        fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    printf("composite_plan: ok\n");
    return 0;
}
