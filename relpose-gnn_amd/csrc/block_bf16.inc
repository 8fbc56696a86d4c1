// Fused 64-channel BasicBlock of the bf16 encoder (round 5): conv3x3 + BN + ReLU -> conv3x3 + BN + identity + ReLU of a
// torchvision BasicBlock (reached from /root/reference/python/niantic/modules/posenet.py:1037; layer 1 of ResNet34: 3 blocks
// on 56x56x64 maps) as ONE kernel, the intermediate activation never leaving the CU.  Included by conv_bf16.hip (shares its
// epilogue, LDS-DMA helpers and the patch kernel's conventions); not a translation unit of its own.
//
// Why: layer 1 is bound by neither pipe (r4: matrix pipe 0.26 busy, HBM 0.34 of 8 TB/s) -- 64 output channels make every byte
// moved worth 52 FLOP, and every kernel tried on it (im2col, patch-resident, weights-stationary, persistent) landed at
// 170-260 us for 517 MB of compulsory traffic per convolution.  Per block the unfused pair moves x in, t out, t in, x in
// (residual), y out = 5 x 205 MB (512 images); fused: x in (+ the halo rows neighbouring tiles share), x again from L2 for the
// residual, y out.
//
// Structure (the patch kernel's, run twice over one LDS image):
//   * a tile = BM2 consecutive output pixels (raster order over all images) of conv2.  conv2 needs the intermediate t on
//     [m0 - W - 1, m0 + BM2 + W + 1); conv1 therefore produces t for BM1 = BM2 + 128 consecutive pixels from m0 - 64 (56-wide
//     maps: W + 1 = 57 <= 64), from an input patch [rows][P slots][32 ch] per 32-channel chunk exactly as in the patch kernel
//     (virtual rows with zero rows between images, zero halo slots, all zeros from out-of-range DMA lanes);
//   * conv1 = 2 chunks x 9 taps on patch buffers 0 / 1 with the weights streaming through NS LDS stages; its MFMAs are issued with
//     the operands SWAPPED (weights as A, pixels as B: D[channel][pixel]), so that a lane ends up with 4 consecutive channels of
//     ONE pixel per accumulator quad: BN1 + ReLU + rounding to bf16 happen in registers, and the result is written back INTO
//     THE INPUT PATCH'S OWN SLOTS (ds_write_b64, same swizzle): pixel (r, c) of t replaces pixel (r, c) of x, halo slots and the
//     rows between images stay zero -- conv2's padding.  (x is dead by then: the residual is re-read from global memory / L2.)
//     Rounding t to bf16 exactly where the unfused path stores it keeps the block's output bit-identical to the two launches;
//   * conv2 = 2 more chunks x 9 taps on the same buffers (wave wn wrote channels 32 wn ..: chunk wn = buffer wn), operands in the
//     usual order, then the lean epilogue (BN2 + identity + ReLU, bf16 stores) on slabs laid over the dead patch.
//   The step sequence is ONE stream of 36 steps for the counted waits: every step issues one patch-slot load (conv1 chunk 0: the
//   pieces of chunk 1; afterwards dummies) and one weight-slot load, weights AHEAD steps early, conv2's first weights during
//   conv1's last taps.
// 8 waves as 4 (pixels) x 2 (channels): conv1 wave tile 32 ch x 160 px (FM1 = 5), conv2 128 px x 32 ch (FM2 = 4).
// LDS: 2 x 68 KB patch + 4 x 4 KB weight stages + 1 KB dummy = 153 KB at BM2 = 512 on 56-wide maps.
// Maps wider than 62 pixels (round 6: the 64 x 86 maps of the 256 x 341 evaluation shape) run as TWO column strips per image, each a
// "virtual image" of W = ceil(Wfull / 2) + 2 columns that ends at its image edge and overlaps the other by 4 columns: the kernel
// works on virtual images throughout (pixel raster, patch, conv1 / conv2 ranges); only the patch loads (row pitch Wfull, column offset
// x01 of strip 1) and the epilogue (real addresses; the 2 halo columns next to the cut are computed and NOT stored: their conv1 inputs
// saw zero padding where the neighbouring strip has pixels) know about the real image.  S = 1: W = Wfull, everything stored.
// Round 6 forms of the same kernel (template flags): PS = persistent (default for launches of more than one round of tiles: the next
// tile's first loads under the current tile's last nine steps and epilogue), PP = the two-group schedule (experiment, bit-identical,
// not faster); the LDS swizzle carries the patch kernel's row-parity term (bank conflicts -80 %, time unchanged).  What bounds all of
// them is the chip-wide power cap: DESIGN.md section 7 (registers-only MFMA stream: 1.8-2.1 PFLOP/s on non-zero operands).
#if defined(RPG_BLOCK_ABL) && (RPG_BLOCK_ABL & 2)   // diagnostic builds (timing only, wrong results): the steps do not wait for their loads
#define RPG_BLK_NOWAIT 1
#else
#define RPG_BLK_NOWAIT 0
#endif
#if defined(RPG_BLOCK_ABL) && (RPG_BLOCK_ABL & 4)   // diagnostic builds (timing only, wrong results): no fragment reads inside the steps
#define RPG_BLK_NOREAD 1
#else
#define RPG_BLK_NOREAD 0
#endif
#ifdef RPG_BLOCK_NOPARITY          // probe builds: the swizzle without its row-parity term (A/B of the LDS bank conflicts; same results)
#define RPG_BLK_PAR 0
#else
#define RPG_BLK_PAR 1
#endif
struct BlockArgs {
    const __bf16* x;
    int H, W, Nimg, M, n_tiles;          // W: virtual width; Nimg: virtual images (N * S); M = Nimg * H * W
    int P, PR, patch_bytes, n_pieces;
    unsigned mg_hv, mg_hw, mg_w, mg_p16;
    const float* scale1;
    const float* shift1;
    int S, Wfull, x01;                   // strips per image (1 | 2), real width, first real column of strip 1
    int st0_hi, st1_lo;                  // strip 0 stores virtual columns < st0_hi, strip 1 those >= st1_lo
};

// The lean epilogue (conv_bf16.hip bf16_tile_epilogue_lean_body, FN = 1, residual) for two-strip launches: row m of the tile is
// pixel (virtual image, row, virtual column); it is stored -- and its residual read -- at its REAL address, if the column belongs
// to the strip's share.  Offsets from the tensors' bases (checked < 2^31 bytes by the launcher); invalid rows carry an out-of-range
// offset (loads return zero, stores are dropped).
template <int FM, int NWAVES>
__device__ __forceinline__ void block64_strip_epilogue(f32x16 (&acc)[FM][1], unsigned char* lds_raw, const EpiB& ep, const BlockArgs& a, int m0,
                                                       int wm, int wn, int lane, int wave) {
    constexpr int EW = 32, EPITCH = EW + 4, C4 = EW / 4, RPI = 64 / C4, NIT = 32 / RPI, C = 64;
    constexpr unsigned OOB = 0x80000000u;
    float* slab = reinterpret_cast<float*>(lds_raw) + wave * (32 * EPITCH);
    const int c4 = lane % C4, r_in = lane / C4;
    const int nb = wn * EW + 4 * c4;
    const float4 sc = *reinterpret_cast<const float4*>(ep.scale + nb);
    const float4 sh = *reinterpret_cast<const float4*>(ep.shift + nb);
    const int mw = m0 + wm * FM * 32;
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<__bf16*>(ep.out), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(ep.residual), 0, 0x7fffffff, 0x00020000);
    const int HW = a.H * a.W;
    const int n0 = m0 / HW, r0 = m0 - n0 * HW;                // (m0 is uniform: one exact division per tile)
    unsigned offs[FM][NIT];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int t = 0; t < NIT; ++t) {
            const int m = mw + i * 32 + r_in + RPI * t;
            const int mc = m < a.M ? m : a.M - 1;
            // the magic division is exact only for dividends < 2^32 / HW (the launcher checks (HW + BM1) * HW < 2^32): divide the
            // tile-relative pixel, not m itself (M reaches millions: the last pixel of an image came out one image too high)
            const int rel = r0 + (mc - m0), nr = div_magic(rel, a.mg_hw);
            const int vn = n0 + nr, rem = rel - nr * HW, row = div_magic(rem, a.mg_w), vc = rem - row * a.W;
            const int strip = vn & 1, n = vn >> 1;
            const bool ok = m < a.M && (strip ? vc >= a.st1_lo : vc < a.st0_hi);
            offs[i][t] = ok ? 2u * (unsigned)(((n * a.H + row) * a.Wfull + vc + (strip ? a.x01 : 0)) * C + nb) : OOB;
        }
    const bool relu = ep.relu != 0;
    u32x2e rs_cur[NIT], rs_nxt[NIT];
#pragma unroll
    for (int t = 0; t < NIT; ++t) rs_cur[t] = __builtin_bit_cast(u32x2e, __builtin_amdgcn_raw_buffer_load_b64(rr, offs[0][t], 0, 0));
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        if (i + 1 < FM) {
#pragma unroll
            for (int t = 0; t < NIT; ++t) rs_nxt[t] = __builtin_bit_cast(u32x2e, __builtin_amdgcn_raw_buffer_load_b64(rr, offs[i + 1 < FM ? i + 1 : i][t], 0, 0));
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) slab[((e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)) * EPITCH + (lane & 31)] = acc[i][0][e];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < NIT; ++t) {
            const float4 v = *reinterpret_cast<const float4*>(&slab[(r_in + RPI * t) * EPITCH + 4 * c4]);
            float4 y;
            y.x = v.x * sc.x + sh.x; y.y = v.y * sc.y + sh.y; y.z = v.z * sc.z + sh.z; y.w = v.w * sc.w + sh.w;
            const bf16x4 rs = __builtin_bit_cast(bf16x4, rs_cur[t]);
            y.x += (float)rs[0]; y.y += (float)rs[1]; y.z += (float)rs[2]; y.w += (float)rs[3];
            const float4 yr = rpg::relu4_if(relu, y);
            const bf16x4 ob = {(__bf16)yr.x, (__bf16)yr.y, (__bf16)yr.z, (__bf16)yr.w};
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2e, ob), ro, offs[i][t], 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < NIT; ++t) rs_cur[t] = rs_nxt[t];
    }
}

// PS (round 6, RPG_TUNE_BF16_FUSE_BLOCK bit 1, default on): PERSISTENT form -- one workgroup per CU walks the tiles b, b + grid, ...;
// during a tile's last nine steps (conv2, chunk 1: patch buffer 0 is dead) the patch slot loads the NEXT tile's chunk 0 and the
// last three weight slots its first three weight stages, the epilogue's slabs lie over buffer 1, and the next tile's address set-up
// runs under the acknowledgement of this tile's stores (one vmcnt(0) in front of its first step: stores count in vmcnt on gfx950).
// PP (round 6 experiment, RPG_TUNE_BF16_FUSE_BLOCK bit 2): TWO-GROUP schedule.  The ablations (DESIGN.md) say a step costs ~1000 cycles
// for 512-640 cycles of MFMAs per SIMD even with no operand reads and no load waits: both waves of a SIMD leave every barrier together,
// fight for the matrix pipe together and reach the next barrier together.  Here a step is two phases, LOAD (all 12 fragments of the step
// into registers, the step's two DMA issues) and COMPUTE (its 8-10 MFMAs back to back), each followed by a workgroup barrier; waves 4..7
// run the SAME instruction stream one barrier behind waves 0..3 (one extra s_barrier at the start, one for waves 0..3 at the end), so at
// any time one wave of every SIMD owns the matrix pipe while the other one reads its next operands.  Five weight stages (a stage is read
// by the late group half a step after the early one), the chunk-1 patch pieces three steps earlier; same MFMA order per accumulator:
// bit-identical.  One tile per workgroup (PS = false).
template <int BM2, int NS, bool PS, bool PP = false>
__global__ __launch_bounds__(512) void block64_bf16_fused_kernel(BlockArgs a, const __bf16* __restrict__ W1, const __bf16* __restrict__ W2,
                                                                 EpiB ep) {
    static_assert((NS == 4 && !PP) || (NS == 5 && PP && !PS), "four weight stages (five in the two-group schedule)");
    constexpr int NW = 8, WM = 4, WN = 2, C = 64;
    constexpr int BM1 = BM2 + 128, LEAD = 64;                 // conv1 range: [m0 - LEAD, m0 - LEAD + BM1)
    constexpr int FM1 = BM1 / WM / 32, FM2 = BM2 / WM / 32;
    constexpr int BSTAGE = C * 64;                            // bytes per weight stage: 64 rows x 32 channels
    constexpr int NPT = 9;                                    // patch pieces per wave (1 KB each): up to 72 per buffer
    constexpr unsigned OOB = 0x80000000u;
    constexpr int NL = 2;                                     // loads per wave and step: one patch-slot piece + one weight-slot piece
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];

    const int nwg = gridDim.x, bid = blockIdx.x;
    // logical tile of (virtual) block vb among n_tiles: contiguous runs of tiles per XCD (vb & 7 is the XCD of every block vb + k * grid)
    auto tile_of = [&](int vb) {
        const int xcd = vb & 7, loc = vb >> 3, q8 = a.n_tiles >> 3, r8 = a.n_tiles & 7;
        return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + loc;
    };
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int H = a.H, W = a.W, HW = a.H * a.W, P = a.P, HV = a.H + 2;
    const unsigned off_b1 = (unsigned)a.patch_bytes;
    const unsigned off_st = 2u * (unsigned)a.patch_bytes;
    const unsigned dummy_off = off_st + (unsigned)NS * BSTAGE;
    const int img = H * a.Wfull * C;                          // a REAL image, elements
    const __amdgpu_buffer_rsrc_t rsw1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(W1), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(W2), 0, 0x7fffffff, 0x00020000);

    // ---- per-tile geometry (patch kernel): first output pixel, conv1's range, first image, the row above the first pixel, this
    // wave's pieces (16 slots = one piece, P % 16 == 0: a piece lies inside one patch row, so row / image / validity are wave-uniform)
    int m0, m1_0, mf, n_first, rem_first, v0;
    unsigned pvoff[NPT];
    __amdgpu_buffer_rsrc_t rs_p;
    auto geometry = [&](int tile, bool live) {
        m0 = tile * BM2;                                      // first output pixel of the tile
        m1_0 = m0 - LEAD;                                     // first pixel of conv1's range (may be < 0)
        mf = m1_0 > 0 ? m1_0 : 0;                             // the patch is laid out from this pixel's row
        n_first = mf / HW;
        rem_first = mf - n_first * HW;
        v0 = n_first * HV + div_magic(rem_first, a.mg_w);
        const int s_l = lane >> 2;
        const int lc0 = (lane & 3) ^ ((s_l >> 2) & 3);
        const int p16 = P >> 4;
        const int vbase = v0 - n_first * HV;
#pragma unroll
        for (int t = 0; t < NPT; ++t) {
            const int q = wave + NW * t;
            const int prow = div_magic(q, a.mg_p16);
            const int col0 = (q - prow * p16) * 16;
            // (row-parity term of the swizzle, as in the patch kernel: physical chunk = logical ^ ((slot >> 2) & 3) ^ 2 (patch row & 1) --
            // a fragment's 32 consecutive pixels wrap into the next patch row P - W = 8 slots further on 56-wide maps, two swizzle
            // blocks: without the term the lanes behind the wrap land on the banks of lanes in front of it)
            const int lc8 = 8 * (lc0 ^ (2 * RPG_BLK_PAR * (prow & 1)));
            const int vrel = vbase + prow;
            const int nrel = div_magic(vrel, a.mg_hv);
            const int rr = vrel - nrel * HV - 1;
            const bool rowok = live && q < a.n_pieces && prow < a.PR && (unsigned)rr < (unsigned)H && n_first + nrel < a.Nimg;
            // virtual image n_first + nrel = real image (..) / S, strip (..) % S; offsets relative to the real image of n_first
            const int vn = n_first + nrel;
            const int nreal = a.S == 2 ? (vn >> 1) - (n_first >> 1) : nrel;
            const int x0 = (a.S == 2 && (vn & 1)) ? a.x01 : 0;
            const int rowbase = ((nreal * H + rr) * a.Wfull + x0 - 1) * C;
            const int pcol = col0 + s_l;
            const unsigned off = 2u * (unsigned)(rowbase + __mul24(pcol, C) + lc8);
            pvoff[t] = (rowok && (unsigned)(pcol - 1) < (unsigned)W) ? off : OOB;
        }
        rs_p = __builtin_amdgcn_make_buffer_rsrc(const_cast<__bf16*>(a.x) + (size_t)(a.S == 2 ? n_first >> 1 : n_first) * img, 0, 0x7fffffff, 0x00020000);
    };
    int vb = bid;
    geometry(PS ? tile_of(vb) : tile_of(bid), true);
    bool has_next = false;                                    // (PS) the tile after the current one exists: its first loads ride on this tile's last steps
    // weight piece of this wave: waves 0..3 carry rows 16 wave .. + 15 of the stage (64 rows), waves 4..7 a dummy
    unsigned woff;
    {
        const int r_in = lane >> 2;
        const int lc = (lane & 3) ^ ((r_in >> 2) & 3);
        const int n = wave * 16 + r_in;
        woff = wave < 4 ? 2u * (unsigned)(n * 9 * C + 8 * lc) : OOB;
    }
    auto issue_patch = [&](int t, int buf, int chunk) {
        const bool real = (wave + NW * t) < a.n_pieces;
        const unsigned dst = real ? (buf ? off_b1 : 0u) + (unsigned)((wave + NW * t) * 1024) : dummy_off;
        dma_piece16_raw(rs_p, dst, lds_raw, pvoff[t], chunk * 64);
    };
    auto issue_dummy = [&]() { dma_piece16_raw(rsw1, dummy_off, lds_raw, OOB, 0); };
    // the weights of global step gs (0..35: conv gs / 18, chunk (gs / 9) % 2, tap gs % 9) -> stage gs % NS; past the end: zero pieces
    auto issue_w = [&](int gs) {
        const int g36 = gs % 36;                              // (PS: steps 36..38 are the next tile's 0..2 -- 36 % NS == 0, same stages)
        const int conv = g36 / 18, chunk = (g36 / 9) & 1, tap = g36 % 9;
        const unsigned dst = wave < 4 ? off_st + (unsigned)((gs % NS) * BSTAGE + wave * 1024) : dummy_off;
        dma_piece16_raw(conv == 0 ? rsw1 : rsw2, dst, lds_raw, (gs < 36 || (PS && has_next)) ? woff : OOB, (tap * C + chunk * 32) * 2);
    };

    // ---- prologue: chunk 0 of the input patch, the weights of steps 0..2 (a dummy in front of the last two sets: the loads a
    // step's wait leaves outstanding are then whole steps' worth, NL each)
#pragma unroll
    for (int t = 0; t < NPT; ++t) issue_patch(t, 0, 0);
    issue_w(0);
    if constexpr (PP) {
        // (PP) pairs "-3 .. -1" of the step stream: chunk-1 pieces 0..2 and the weights of steps 1..3 (LOAD(s) issues pair s - 1 =
        // chunk-1 piece s + 2 | dummy, weights of step s + 3)
        issue_patch(0, 1, 1); issue_w(1);
        issue_patch(1, 1, 1); issue_w(2);
        issue_patch(2, 1, 1); issue_w(3);
    } else {
        issue_dummy();
        issue_w(1);
        issue_dummy();
        issue_w(2);
    }

    const int half = lane >> 5;
    unsigned cb[2];                                           // weight fragment addresses inside stage 0 (rows 32 wn ..)
    {
        const int lrow = lane & 31, sw = (lrow >> 2) & 3;
#pragma unroll
        for (int g = 0; g < 2; ++g) cb[g] = off_st + (unsigned)(wn * 32 * 64 + lrow * 64 + 16 * ((2 * g + half) ^ sw));
    }
    // pixel m (clamped into [mf, M)) -> its patch slot s0 = (row above it) * P + column, as in the patch kernel
    auto slot_of = [&](int m, int& prow) {                    // prow: the slot's patch row (for the swizzle's parity term)
        m = m < mf ? mf : (m < a.M ? m : a.M - 1);
        const int rel = rem_first + (m - mf);
        const int nr = div_magic(rel, a.mg_hw), rem = rel - nr * HW, r = div_magic(rem, a.mg_w), c = rem - r * W;
        prow = (n_first + nr) * HV + r - v0;
        return prow * P + c;
    };

    bf16x8 fr[2][FM1 + 1];                                    // [set][0 = weight fragment, 1 + i = pixel fragment i] (shared by both convolutions)
    // One step of `FM` pixel fragments: two k groups of FM MFMAs; group 1's fragments are read behind group 0's MFMAs, the next
    // tap's group-0 pixel fragments and (unless `last`) the next step's group-0 weight fragment behind group 1's (the patch of a
    // chunk is complete from its first tap on; with four stages the next step's weights were waited for at this step's barrier).
    // SWAP: weights as the A operand (conv1).  `pl` = what the step's patch slot loads (piece index into buffer 1, or -1: dummy).
#define RPG_BLK_STEP(FM, SWAP, ACC, A3, GS, TAP, FIRST, LAST, PL, PBUF)                                                          \
    do {                                                                                                                 \
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(RPG_BLK_NOWAIT ? 63 : (((GS) == 9) ? 1 : NL)) : "memory");    \
        __builtin_amdgcn_s_barrier();                                                                                    \
        asm volatile("" ::: "memory");                                                                                   \
        constexpr int st_ = (GS) & 3, st1_ = ((GS) + 1) & 3;                                                             \
        const unsigned aoff_ = (unsigned)(((TAP) / 3) * P * 64);                                                         \
        const unsigned aoff1_ = (unsigned)((((TAP) + 1) / 3) * P * 64);                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
        if ((TAP) == 0) {                                                                                                \
            _Pragma("unroll") for (int i = 0; i < FM; ++i)                                                               \
                fr[0][1 + i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds_raw + (A3[i][0][0] + aoff_))); \
        }                                                                                                                \
        if (FIRST) fr[0][0] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds_raw + cb[0] + st_ * BSTAGE)); \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
        _Pragma("unroll") for (int ms = 0; ms < FM; ++ms) {                                                              \
            if (SWAP) ACC[ms][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[0][0], fr[0][1 + ms], ACC[ms][0], 0, 0, 0);          \
            else ACC[ms][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[0][1 + ms], fr[0][0], ACC[ms][0], 0, 0, 0);               \
            if (ms == 0 && !RPG_BLK_NOREAD) fr[1][0] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds_raw + cb[1] + st_ * BSTAGE)); \
            if (!RPG_BLK_NOREAD) fr[1][1 + ms] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds_raw + (A3[ms][(TAP) % 3][1 ^ (((TAP) / 3) & RPG_BLK_PAR)] + aoff_))); \
            if (ms == 0) {                                                                                               \
                if ((PL) >= 0) issue_patch((PL) >= 0 ? (PL) : 0, (PBUF), (PBUF));   /* chunk 1 -> buffer 1 | (PS) the next tile's chunk 0 -> buffer 0 */ \
                else issue_dummy();                                                                                      \
            }                                                                                                            \
            __builtin_amdgcn_sched_barrier(0);                                                                           \
        }                                                                                                                \
        _Pragma("unroll") for (int ms = 0; ms < FM; ++ms) {                                                              \
            if (SWAP) ACC[ms][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[1][0], fr[1][1 + ms], ACC[ms][0], 0, 0, 0);          \
            else ACC[ms][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[1][1 + ms], fr[1][0], ACC[ms][0], 0, 0, 0);               \
            if (ms == 0) issue_w((GS) + NS - 1);                                                                         \
            if ((TAP) < 8 && !RPG_BLK_NOREAD) fr[0][1 + ms] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds_raw + (A3[ms][((TAP) + 1) % 3][(((TAP) + 1) / 3) & RPG_BLK_PAR] + aoff1_))); \
            if (!(LAST) && ms == FM - 1 && !RPG_BLK_NOREAD) fr[0][0] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds_raw + cb[0] + st1_ * BSTAGE)); \
            __builtin_amdgcn_sched_barrier(0);                                                                           \
        }                                                                                                                \
    } while (0)
#define RPG_BLK_CHUNK(FM, SWAP, ACC, A3, GS0, FIRST, LAST, PATCH, PBUF)                                                    \
    do {                                                                                                                 \
        RPG_BLK_STEP(FM, SWAP, ACC, A3, (GS0) + 0, 0, FIRST, false, (PATCH) ? 0 : -1, PBUF);                              \
        RPG_BLK_STEP(FM, SWAP, ACC, A3, (GS0) + 1, 1, false, false, (PATCH) ? 1 : -1, PBUF);                              \
        RPG_BLK_STEP(FM, SWAP, ACC, A3, (GS0) + 2, 2, false, false, (PATCH) ? 2 : -1, PBUF);                              \
        RPG_BLK_STEP(FM, SWAP, ACC, A3, (GS0) + 3, 3, false, false, (PATCH) ? 3 : -1, PBUF);                              \
        RPG_BLK_STEP(FM, SWAP, ACC, A3, (GS0) + 4, 4, false, false, (PATCH) ? 4 : -1, PBUF);                              \
        RPG_BLK_STEP(FM, SWAP, ACC, A3, (GS0) + 5, 5, false, false, (PATCH) ? 5 : -1, PBUF);                              \
        RPG_BLK_STEP(FM, SWAP, ACC, A3, (GS0) + 6, 6, false, false, (PATCH) ? 6 : -1, PBUF);                              \
        RPG_BLK_STEP(FM, SWAP, ACC, A3, (GS0) + 7, 7, false, false, (PATCH) ? 7 : -1, PBUF);                              \
        RPG_BLK_STEP(FM, SWAP, ACC, A3, (GS0) + 8, 8, false, LAST, (PATCH) ? 8 : -1, PBUF);                               \
    } while (0)
    // A fragment address table of a pixel range: tap (kh, kw) of pixel slot s0 reads slot s0 + kh P + kw, k group g the 16-byte
    // chunk (2 g + half) ^ ((slot >> 2) & 3) ^ 2 (patch row & 1); P % 16 == 0, so the slot term depends on kw only, and the parity
    // term is XOR-decomposable over the kernel row: the entries carry the parity of row kh = 0, an odd kh reads the OTHER k group's
    // entry (RPG_BLK_STEP: [g ^ (kh & 1)]) -- no extra registers or instructions
#define RPG_BLK_ATABLE(FM, A3, MBASE)                                                                                     \
    _Pragma("unroll") for (int i = 0; i < FM; ++i) {                                                                     \
        int pr_;                                                                                                         \
        const int s0_ = slot_of((MBASE) + (wm * FM + i) * 32 + (lane & 31), pr_);                                        \
        _Pragma("unroll") for (int kw = 0; kw < 3; ++kw) {                                                               \
            const int t_ = s0_ + kw;                                                                                     \
            const int e_ = half ^ ((t_ >> 2) & 3) ^ (2 * RPG_BLK_PAR * (pr_ & 1));                                                     \
            A3[i][kw][0] = (unsigned)(t_ * 64 + 16 * e_);                                                                \
            A3[i][kw][1] = (unsigned)(t_ * 64 + 16 * (e_ ^ 2));                                                          \
        }                                                                                                                \
    }

#define RPG_PP_SYNC()                                                                                                    \
    do {                                                                                                                 \
        asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");                                                       \
        __builtin_amdgcn_s_barrier();                                                                                    \
        asm volatile("" ::: "memory");                                                                                   \
    } while (0)
    // LOAD(GS): the step's 2 weight + 2 FM pixel fragments, pair GS - 1 of the DMA stream; COMPUTE(GS): its MFMAs
#define RPG_PP_STEP(FM, SWAP, ACC, A3, GS, TAP)                                                                           \
    do {                                                                                                                 \
        constexpr int st_ = (GS) % NS, ko_ = ((TAP) / 3) & RPG_BLK_PAR;                                                  \
        const unsigned aoff_ = (unsigned)(((TAP) / 3) * P * 64);                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
        fr[0][0] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds_raw + cb[0] + st_ * BSTAGE));          \
        fr[1][0] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds_raw + cb[1] + st_ * BSTAGE));          \
        _Pragma("unroll") for (int i = 0; i < FM; ++i) {                                                                 \
            fr[0][1 + i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds_raw + (A3[i][(TAP) % 3][0 ^ ko_] + aoff_))); \
            fr[1][1 + i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(lds_raw + (A3[i][(TAP) % 3][1 ^ ko_] + aoff_))); \
        }                                                                                                                \
        if ((GS) >= 1) {                                                                                                 \
            if ((GS) + 2 <= 8) issue_patch(((GS) + 2 <= 8) ? (GS) + 2 : 0, 1, 1);                                        \
            else issue_dummy();                                                                                          \
            issue_w((GS) + 3);                                                                                           \
        }                                                                                                                \
        RPG_PP_SYNC();                                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
        _Pragma("unroll") for (int ms = 0; ms < FM; ++ms) {                                                              \
            if (SWAP) ACC[ms][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[0][0], fr[0][1 + ms], ACC[ms][0], 0, 0, 0);          \
            else ACC[ms][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[0][1 + ms], fr[0][0], ACC[ms][0], 0, 0, 0);               \
        }                                                                                                                \
        _Pragma("unroll") for (int ms = 0; ms < FM; ++ms) {                                                              \
            if (SWAP) ACC[ms][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[1][0], fr[1][1 + ms], ACC[ms][0], 0, 0, 0);          \
            else ACC[ms][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[1][1 + ms], fr[1][0], ACC[ms][0], 0, 0, 0);               \
        }                                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
        RPG_PP_SYNC();                                                                                                   \
    } while (0)
#define RPG_PP_CHUNK(FM, SWAP, ACC, A3, GS0)                                                                              \
    do {                                                                                                                 \
        RPG_PP_STEP(FM, SWAP, ACC, A3, (GS0) + 0, 0); RPG_PP_STEP(FM, SWAP, ACC, A3, (GS0) + 1, 1);                       \
        RPG_PP_STEP(FM, SWAP, ACC, A3, (GS0) + 2, 2); RPG_PP_STEP(FM, SWAP, ACC, A3, (GS0) + 3, 3);                       \
        RPG_PP_STEP(FM, SWAP, ACC, A3, (GS0) + 4, 4); RPG_PP_STEP(FM, SWAP, ACC, A3, (GS0) + 5, 5);                       \
        RPG_PP_STEP(FM, SWAP, ACC, A3, (GS0) + 6, 6); RPG_PP_STEP(FM, SWAP, ACC, A3, (GS0) + 7, 7);                       \
        RPG_PP_STEP(FM, SWAP, ACC, A3, (GS0) + 8, 8);                                                                     \
    } while (0)
    if constexpr (PP) {
        const int grp = wave >> 2;                            // 0: waves 0..3 (early), 1: waves 4..7 (one barrier behind)
        f32x16 acc2[FM2][1];
        {
            unsigned a1[FM1][3][2];
            f32x16 acc1[FM1][1];
            RPG_BLK_ATABLE(FM1, a1, m1_0);
#pragma unroll
            for (int i = 0; i < FM1; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc1[i][0][e] = 0.f;
            // patch chunk 0 and the weights of step 0 have landed (16 loads issued: the three pairs may be in flight)
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (grp) __builtin_amdgcn_s_barrier();
            RPG_PP_CHUNK(FM1, true, acc1, a1, 0);
#pragma unroll
            for (int i = 0; i < FM1; ++i)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) { a1[i][kw][0] += off_b1; a1[i][kw][1] += off_b1; }
            RPG_PP_CHUNK(FM1, true, acc1, a1, 9);
            // write-back phase: nobody reads x any more (the late group is in COMPUTE(17): registers only); BN1 + ReLU + bf16 -> t into
            // the pixels' own slots.  The late group writes one phase later, the early group's LOAD(18) comes one phase after that.
            float4 sc[4], sh[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                sc[q] = *reinterpret_cast<const float4*>(a.scale1 + wn * 32 + 8 * q + 4 * half);
                sh[q] = *reinterpret_cast<const float4*>(a.shift1 + wn * 32 + 8 * q + 4 * half);
            }
            unsigned char* tbuf = lds_raw + (wn ? off_b1 : 0u);
#pragma unroll
            for (int i = 0; i < FM1; ++i) {
                const int m = m1_0 + (wm * FM1 + i) * 32 + (lane & 31);
                int pr0;
                const int slot = slot_of(m, pr0) + P + 1;
                const int sw = ((slot >> 2) & 3) ^ (2 * RPG_BLK_PAR * ((pr0 + 1) & 1));
                if (m >= mf && m < a.M) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        float4 y;
                        y.x = acc1[i][0][4 * q + 0] * sc[q].x + sh[q].x; y.y = acc1[i][0][4 * q + 1] * sc[q].y + sh[q].y;
                        y.z = acc1[i][0][4 * q + 2] * sc[q].z + sh[q].z; y.w = acc1[i][0][4 * q + 3] * sc[q].w + sh[q].w;
                        const float4 yr = rpg::relu4(y);
                        const bf16x4 ob = {(__bf16)yr.x, (__bf16)yr.y, (__bf16)yr.z, (__bf16)yr.w};
                        *reinterpret_cast<u32x2e*>(tbuf + slot * 64 + 16 * (q ^ sw) + 8 * half) = __builtin_bit_cast(u32x2e, ob);
                    }
                }
            }
            RPG_PP_SYNC();
        }
        // empty phase of the early group (the late group writes t): conv2's fragment addresses and accumulators
        unsigned a2[FM2][3][2];
        RPG_BLK_ATABLE(FM2, a2, m0);
#pragma unroll
        for (int i = 0; i < FM2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc2[i][0][e] = 0.f;
        RPG_PP_SYNC();
        RPG_PP_CHUNK(FM2, false, acc2, a2, 18);
#pragma unroll
        for (int i = 0; i < FM2; ++i)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) { a2[i][kw][0] += off_b1; a2[i][kw][1] += off_b1; }
        RPG_PP_CHUNK(FM2, false, acc2, a2, 27);
        if (!grp) __builtin_amdgcn_s_barrier();               // (the late group's last COMPUTE)
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (a.S == 1) bf16_tile_epilogue_lean_body<FM2, 1, NW, true>(acc2, lds_raw, ep, m0, 0, a.M, C, wm, wn, lane, wave);
        else block64_strip_epilogue<FM2, NW>(acc2, lds_raw, ep, a, m0, wm, wn, lane, wave);
        return;
    }
    bool first_tile = true;
    for (;;) {                                                // (one pass unless PS)
    unsigned a2[FM2][3][2];
    // ================= conv1 (operands swapped: D[channel][pixel]) over [m1_0, m1_0 + BM1) =================
    {
        unsigned a1[FM1][3][2];
        f32x16 acc1[FM1][1];
        RPG_BLK_ATABLE(FM1, a1, m1_0);
#pragma unroll
        for (int i = 0; i < FM1; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc1[i][0][e] = 0.f;
        if (PS && !first_tile) {
            // the previous tile's stores are acknowledged and this tile's chunk 0 + first weights (issued during its last steps) have
            // landed: the counted waits of the steps start from zero again.  (Behind the address set-up above: that ran under the wait.)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        RPG_BLK_CHUNK(FM1, true, acc1, a1, 0, true, false, true, 1);
#pragma unroll
        for (int i = 0; i < FM1; ++i)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) { a1[i][kw][0] += off_b1; a1[i][kw][1] += off_b1; }
        RPG_BLK_CHUNK(FM1, true, acc1, a1, 9, false, false, false, 1);
        // conv2's fragment addresses now, under conv1's last MFMAs and the wait for the other waves (left to itself hipcc sinks these
        // ~150 instructions behind conv2's first barrier, in front of its first MFMA)
        RPG_BLK_ATABLE(FM2, a2, m0);
#pragma unroll
        for (int i = 0; i < FM2; ++i)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) { asm volatile("" : "+v"(a2[i][kw][0])); asm volatile("" : "+v"(a2[i][kw][1])); }
        // every wave is done reading x (both buffers): t goes into the same slots
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // BN1 + ReLU + bf16, in registers: the lane holds pixel (lane & 31) of fragment i, channels 32 wn + 8 q + 4 half + 0..3 in
        // accumulator elements 4 q .. 4 q + 3
        float4 sc[4], sh[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sc[q] = *reinterpret_cast<const float4*>(a.scale1 + wn * 32 + 8 * q + 4 * half);
            sh[q] = *reinterpret_cast<const float4*>(a.shift1 + wn * 32 + 8 * q + 4 * half);
        }
        unsigned char* tbuf = lds_raw + (wn ? off_b1 : 0u);
#pragma unroll
        for (int i = 0; i < FM1; ++i) {
            const int m = m1_0 + (wm * FM1 + i) * 32 + (lane & 31);
            int pr0;
            const int slot = slot_of(m, pr0) + P + 1;         // the pixel's own slot: one row down, one column right of its (kh, kw) = (0, 0) tap
            const int sw = ((slot >> 2) & 3) ^ (2 * RPG_BLK_PAR * ((pr0 + 1) & 1));
            if (m >= mf && m < a.M) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float4 y;
                    y.x = acc1[i][0][4 * q + 0] * sc[q].x + sh[q].x; y.y = acc1[i][0][4 * q + 1] * sc[q].y + sh[q].y;
                    y.z = acc1[i][0][4 * q + 2] * sc[q].z + sh[q].z; y.w = acc1[i][0][4 * q + 3] * sc[q].w + sh[q].w;
                    const float4 yr = rpg::relu4(y);
                    const bf16x4 ob = {(__bf16)yr.x, (__bf16)yr.y, (__bf16)yr.z, (__bf16)yr.w};
                    *reinterpret_cast<u32x2e*>(tbuf + slot * 64 + 16 * (q ^ sw) + 8 * half) = __builtin_bit_cast(u32x2e, ob);
                }
            }
        }
    }
    // ================= conv2 over [m0, m0 + BM2): t from the same buffers (chunk wn was written by the waves wn) =================
    {
        f32x16 acc2[FM2][1];
#pragma unroll
        for (int i = 0; i < FM2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc2[i][0][e] = 0.f;
        // (the step's own wait + barrier orders the ds_writes of t before the first read)
        RPG_BLK_CHUNK(FM2, false, acc2, a2, 18, false, false, false, 1);
#pragma unroll
        for (int i = 0; i < FM2; ++i)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) { a2[i][kw][0] += off_b1; a2[i][kw][1] += off_b1; }
        const int m0_ep = m0;                                 // the epilogue's tile (the geometry variables move on to the next tile now)
        if (PS) {
            // from here on the patch slot and the last weight slots load the NEXT tile's first operands (buffer 0 is dead: conv2's
            // chunk 0 has been read); without a next tile every offset is out of range (zero pieces, same instruction count)
            vb += nwg;
            has_next = vb < a.n_tiles;
            geometry(tile_of(has_next ? vb : bid), has_next);
            RPG_BLK_CHUNK(FM2, false, acc2, a2, 27, false, true, true, 0);
        } else {
            RPG_BLK_CHUNK(FM2, false, acc2, a2, 27, false, true, false, 1);
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // BN2 + identity (x re-read from global memory: it was this tile's own patch a moment ago) + ReLU, bf16 stores
#if defined(RPG_BLOCK_ABL) && (RPG_BLOCK_ABL & 1)      // diagnostic builds (timing only, wrong results): no epilogue -- what do its stores and residual reads cost?
        float sacc = 0.f;
#pragma unroll
        for (int i = 0; i < FM2; ++i) sacc += acc2[i][0][0] + acc2[i][0][9];
        if (sacc == 123.456f) reinterpret_cast<__bf16*>(ep.out)[tid] = (__bf16)sacc;
#else
        // (PS: the slabs lie over buffer 1 -- buffer 0 and the weight stages are being filled for the next tile)
        unsigned char* const slab_base = lds_raw + (PS ? off_b1 : 0u);
        if (a.S == 1) bf16_tile_epilogue_lean_body<FM2, 1, NW, true>(acc2, slab_base, ep, m0_ep, 0, a.M, C, wm, wn, lane, wave);
        else block64_strip_epilogue<FM2, NW>(acc2, slab_base, ep, a, m0_ep, wm, wn, lane, wave);
#endif
    }
    if (!PS || !has_next) break;
    first_tile = false;
    }
#undef RPG_BLK_ATABLE
#undef RPG_BLK_CHUNK
#undef RPG_BLK_STEP
#undef RPG_PP_CHUNK
#undef RPG_PP_STEP
#undef RPG_PP_SYNC
}

// x [n][h][w][64] -> y [n][h][w][64] = relu(bn2(conv2(relu(bn1(conv1(x))))) + x); false if the shape is not eligible (the caller
// then launches the two convolutions)
bool launch_block64_fused(const void* x, const void* w1, const float* scale1, const float* shift1, const void* w2, const float* scale2,
                          const float* shift2, void* y, int n, int h, int w, hipStream_t s) {
    constexpr int BM2 = 512, BM1 = BM2 + 128, NS = 4, C = 64;
    constexpr int slab_bytes = 8 * 32 * (32 + 4) * 4;         // the epilogue's staging slabs (8 waves)
    route_begin();
    if (!x || !w1 || !w2 || !scale1 || !shift1 || !scale2 || !shift2 || !y || n <= 0 || w < 4 || h < 1 ||
        !rpg::aligned16(scale1) || !rpg::aligned16(shift1) || !rpg::aligned16(scale2) || !rpg::aligned16(shift2))
        return false;
    // maps up to 62 pixels wide as they are; up to 120 as two column strips of ceil(w / 2) + 2 columns or a few more (see BlockArgs):
    // narrow views put more patch rows under a tile, the first view width whose patch fits the LDS is taken (64 wide: 36 columns)
    const int wfull = w, nreal = n;
    const int ws = (wfull + 1) / 2;
    BlockArgs a{};
    int lds = 0;
    bool fits = false;
    // candidates: the whole map (wv = wfull, one strip) if it is narrow enough, then two strips with views of ws + 2, ws + 3, ... columns
    for (int wv = (wfull + 1 > 64) ? ws + 2 : wfull, first = 1; wv + 1 <= 64 && !fits; wv = first && wfull + 1 <= 64 ? ws + 2 : wv + 1, first = 0) {
        const bool two = !(first && wfull + 1 <= 64);
        if (two && wv >= wfull) break;                        // (a view as wide as the map: nothing to split)
        w = wv; n = two ? 2 * nreal : nreal;
        const long M = (long)n * h * w;
        if (M >= (1L << 30)) return false;
        const int HW = h * w;
        a = BlockArgs{};
        a.S = two ? 2 : 1; a.Wfull = wfull; a.x01 = two ? wfull - wv : 0; a.st0_hi = two ? ws : wfull; a.st1_lo = two ? ws - (wfull - wv) : 0;
        a.x = reinterpret_cast<const __bf16*>(x); a.H = h; a.W = w; a.Nimg = n; a.M = (int)M;
        a.n_tiles = (int)((M + BM2 - 1) / BM2);
        a.P = (w + 2 + 15) / 16 * 16;
        const int rows = (BM1 - 1) / w + 2, imgs = (BM1 - 1) / HW + 2;
        a.PR = rows + 2 * (imgs - 1) + 2;
        a.patch_bytes = (a.PR * a.P * 64 + 1023) / 1024 * 1024;
        a.n_pieces = a.patch_bytes / 1024;
        auto magic = [](int d) { return d <= 1 ? 0u : (unsigned)((1ULL << 32) / (unsigned)d) + 1u; };
        a.mg_hv = magic(h + 2); a.mg_hw = magic(HW); a.mg_w = magic(w); a.mg_p16 = magic(a.P / 16);
        a.scale1 = scale1; a.shift1 = shift1;
        if ((long)(HW + BM1) * HW >= (1L << 32) || (long)(a.PR + h + 2 + 2) * (h + 2) >= (1L << 32)) return false;
        lds = 2 * a.patch_bytes + NS * C * 64 + 1024;
        fits = a.n_pieces <= 72 && lds <= 160 * 1024 && lds >= slab_bytes;
        if ((long)(imgs + 1) * h * wfull * C * 2 >= (1L << 31)) return false;
    }
    if (!fits) return false;
    // 32-bit byte offsets: the patch loads' (relative to a tile's first real image) and, for two strips, the epilogue's (from the tensors' bases)
    if ((long)((BM1 - 1) / (h * w) + 3) * h * wfull * C * 2 >= (1L << 31)) return false;
    if (a.S == 2 && (long)nreal * h * wfull * C * 2 >= (1L << 31)) return false;
    EpiB ep{scale2, shift2, reinterpret_cast<const __bf16*>(x), y, C, 1, 0};
    ep.lean = 1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    static bool once[64] = {};
    if (!once[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(block64_bf16_fused_kernel<BM2, NS, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(block64_bf16_fused_kernel<BM2, NS, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        once[dev] = true;
    }
    // two-group schedule (RPG_TUNE_BF16_FUSE_BLOCK bit 2, experiment): one tile per workgroup, five weight stages
    if ((rpg::tuning().bf16.fuse_block & 4) && lds + C * 64 <= 160 * 1024) {
        static bool once_pp[64] = {};
        if (!once_pp[dev]) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(block64_bf16_fused_kernel<BM2, 5, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            once_pp[dev] = true;
        }
        route_note(ROUTE_BLOCK_TWO_GROUP, BM2, C, 5);
        hipLaunchKernelGGL((block64_bf16_fused_kernel<BM2, 5, false, true>), dim3(a.n_tiles), dim3(512), lds + C * 64, s, a, reinterpret_cast<const __bf16*>(w1),
                           reinterpret_cast<const __bf16*>(w2), ep);
        return true;
    }
    // persistent form (RPG_TUNE_BF16_FUSE_BLOCK bit 1): more than one round of tiles, a grid of whole octets of CUs (the XCD-wise tile
    // order needs blockIdx & 7 to be the XCD of every tile a workgroup walks); the epilogue slabs must fit buffer 1
    const int pgrid = rpg::num_cus() & ~7;
    if ((rpg::tuning().bf16.fuse_block & 2) && pgrid >= 8 && a.n_tiles > pgrid && a.patch_bytes >= slab_bytes) {
        route_note(ROUTE_BLOCK_PERSIST, BM2, C, NS);
        hipLaunchKernelGGL((block64_bf16_fused_kernel<BM2, NS, true>), dim3(pgrid), dim3(512), lds, s, a, reinterpret_cast<const __bf16*>(w1),
                           reinterpret_cast<const __bf16*>(w2), ep);
        return true;
    }
    auto kern = block64_bf16_fused_kernel<BM2, NS, false>;
    route_note(ROUTE_BLOCK, BM2, C, NS);
    hipLaunchKernelGGL(kern, dim3(a.n_tiles), dim3(512), lds, s, a, reinterpret_cast<const __bf16*>(w1), reinterpret_cast<const __bf16*>(w2), ep);
    return true;
}
