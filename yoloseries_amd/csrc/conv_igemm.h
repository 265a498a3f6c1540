// What the translation units of the implicit-GEMM convolution share: the planner (conv_igemm.hip) and one file per kernel
// family (conv_generic.hip, conv_v2.hip, conv_v3.hip, conv_halo.hip, conv_halo160.hip, conv_stem.hip).  Included by those only.
// The types that cross from the planner to a family's launcher live in namespace yh_conv; the kernels themselves stay in the
// anonymous namespace of their file (profilers and the tools recognise the library's kernels by that).
#pragma once
#include "common.h"

#ifndef YH_CONV_ABLATE
#define YH_CONV_ABLATE 0      // timing builds only (make ablate ABL=mask): compile parts of the main loop out
#endif
#ifndef YH_H160_STG
#define YH_H160_STG 3          // weight-ring stages of conv_halo160_kernel (A/B builds: -DYH_H160_STG=4 -DYH_H160_ROWS=304)
#endif
#ifndef YH_H160_ROWS
#define YH_H160_ROWS 328       // rows of one patch buffer
#endif

namespace yh_conv {

constexpr int BM = 128;
constexpr int BK = 32;
constexpr int STEM_BAND = 8;          // image rows per XCD band of the XCD-aware strip order
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

struct ConvK {
    yh_conv_desc d;
    int M, Ctot, Ktot, nkt, mtiles;
    int sa, sb, sc, sdshift;
    // stride-2 data gradient: the output pixels are processed in 4 parity classes (blockIdx.z); a class only
    // touches the taps whose parity matches, so no MFMA work is spent on structurally-zero taps
    int cls, Hc, Wc;
    int fast;      // every input segment has a multiple of 32 channels: tap-major incremental loader
    int v2;        // lean buffer-load kernel eligible
    unsigned segbytes[2], wbytes;   // addressable bytes from seg[i].ptr / w (hardware range check zero-fills beyond)
    unsigned long segbytes64[2];    // the same, unclamped: conv_v3_kernel re-bases its input descriptors at every tile
    int pointwise; // 1x1 / stride 1 / no upsample: input pixel == output pixel
    int xgx, xgy;  // conv_v3_kernel launched as ONE row of xgx * xgy workgroups in XCD-major (m-tile slot, n-tile) order (0: 2-D grid)
    int dbg;       // YH_CONV_DBG kernel-selection switches for A/B timing: 16 generic kernel instead of v2, 64 32-channel
                   // k-steps only, 256 no stem kernel (the ablation masks are compile-time: make ablate ABL=mask)
};

// Per-block partial sums leave the kernel as one fp32 slab row per block (deterministic fixed-order reduction by
// yh_bn_finalize / yh_bn_bwd_finalize).
__device__ __forceinline__ void put_stat(const yh_conv_desc& d, size_t blk, int which, int n, float v)
{
    d.stats[(blk * 2 + which) * d.Npad + n] = v;
}
__device__ __forceinline__ void put_bnr(const yh_conv_desc& d, size_t row, int which, int n, float v)
{
    d.bnr_part[(row * 2 + which) * d.N + n] = v;
}

// Stride-2 data gradients run as four parity classes of output pixels (2i+ph, 2j+pw) that touch only their structurally
// non-zero taps: 1, 2, 2 and 4 taps for a 3x3 kernel.  blockIdx.z enumerates (class, slot): a class owns as many slots as it
// has taps (KH*KW slots in all) and its m-tiles are dealt over slots x gridDim.x blocks, so every block of the launch carries
// the same work (one z per class left the one-tap class idle 3/4 of the time).
__device__ __forceinline__ void cls_slot(const yh_conv_desc& d, int z, int& ph, int& pw, int& slot, int& nslots)
{
    int acc = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int cph = c >> 1, cpw = c & 1;
        const int kh0 = (cph + d.pad) & 1, kw0 = (cpw + d.pad) & 1;
        const int n = ((d.KH - kh0 + 1) / 2) * ((d.KW - kw0 + 1) / 2);
        if (z < acc + n || c == 3) { ph = cph; pw = cpw; slot = z - acc; nslots = n; return; }
        acc += n;
    }
}

// chunk swizzle of the LDS-DMA kernels (conv_v3.hip: "XOR swizzle of the 16-byte chunks")
template <int CHR> __device__ __forceinline__ int swz_f(int row) { return CHR == 8 ? ((row >> 1) & 7) : ((row >> 2) & 3); }

// tile geometry of the halo kernels (conv_halo.hip, conv_halo160.hip), made by conv_halo_geom in conv_igemm.hip
struct HaloGeom { int TH, TW, PW, NP, tiles_x, tiles_y, gx, gy, rowmajor;
                  unsigned long long* stamps; };   // diagnostics (yh_halo_set_stamps): [workgroup][wave][8] cycle sums of the workgroup's 2nd tile

// Block -> (persistent tile slot bx, output-channel tile by) of the halo kernels, launched as ONE row of gx * gy workgroups.  The gy
// channel tiles of a pixel tile stage the SAME input patch: as grid rows (by = blockIdx.y) their linear ids are gx apart, i.e. they
// land on different XCDs at different times and every one fetches the patch again (PMC, YOLOv5x at 1280^2: 2.78x the algorithmic
// bytes on the 320-channel layers).  Workgroups are dealt round-robin to the 8 XCDs by linear id: XCD x takes a contiguous range of
// the order (slot, channel tile), so the gy readers of a patch sit on one XCD, dispatched back to back, and share its L2.
__device__ __forceinline__ void halo_block_map(const HaloGeom& hg, int& bx, int& by)
{
    if (hg.rowmajor) { by = blockIdx.x / hg.gx; bx = blockIdx.x - by * hg.gx; return; }     // YH_HALO_MAP=0: the round-3 order (A/B)
    const int nb = hg.gx * hg.gy, lin = blockIdx.x, x = lin & 7, q = nb >> 3, r = nb & 7;
    const int vid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (lin >> 3);
    bx = vid / hg.gy;
    by = vid - bx * hg.gy;
}

// ---- tile tables: the numbers of an instantiation are spelled here and nowhere else
// register-staged kernels by output-channel tile (a 96-wide tile for the v5m / v5x widths was measured: +2 % on v5m training,
// -3 % on v5x inference): waves and minimum waves per SIMD of conv_v2_kernel (wm2, wn2, minw2) and of conv_igemm_kernel (wm, wn, minw),
// occ = resident blocks per CU of either
struct ConvTile { int bn, wm2, wn2, minw2, wm, wn, minw, occ; };
constexpr ConvTile CONV_TILES[3] = {
    {32, 4, 1, 4, 4, 1, 4, 4},
    {64, 4, 1, 3, 4, 1, 3, 3},           // (8 waves of 32 x 32 measured equal: LDS reads per MFMA double)
    {128, 4, 2, 4, 2, 2, 2, 2},          // conv_v2_kernel: 8 waves: 4 per SIMD with two resident blocks, wave tile 32 x 64
};
constexpr ConvTile conv_tile(int bn) { return CONV_TILES[bn == 32 ? 0 : (bn == 64 ? 1 : 2)]; }

// LDS-DMA kernel (conv_v3_kernel) by variant: 1 = 256 x 128 tile (8 waves), 2 = 128 x 128 (4 waves), 3 = 128 x 64 (4 waves),
// 4 = 256 x 256 (8 waves of 128 x 64: half the LDS-DMA bytes per MFMA of variant 1, whose 48 KB per k-step need 48 B/clk of the
// CU's 64 B/clk intake at the full MFMA rate; 64-channel k-steps only).  stg / occ: ring stages and resident blocks per CU with
// 64- / 32-channel k-steps
struct V3Tile { int bmt, bn, wm, wn, stg64, stg32, occ64, occ32; };
constexpr V3Tile V3_TILES[5] = {
    {},
    {256, 128, 4, 2, 3, 4, 1, 1},
    {128, 128, 2, 2, 2, 4, 2, 2},
    {128, 64, 2, 2, 3, 4, 2, 3},
    {256, 256, 2, 4, 2, 0, 1, 1},
};

// dynamic LDS of conv_igemm_kernel / conv_v2_kernel
template <int BN, int WM, int WN, int BKT = 32>
constexpr size_t conv_smem_bytes() {
    size_t a = 2 * (BM + BN) * (BKT + 8) * 2;
    size_t c = BM * (BN + 8) * 2;
    return (a > c ? a : c) + WM * 2 * BN * 4 + BM * 4;
}

// ---- the plan: which instantiation runs for a descriptor, on what grid, writing how many partial-sum rows.  Made once per call
// and read by the launcher and by the queries (yh_conv_info and the three older ones, through conv_choose), so they cannot drift apart.
enum ConvFamily { FAM_STEM, FAM_HALO160, FAM_HALO, FAM_V3, FAM_V2, FAM_GENERIC };
struct ConvPlan {
    ConvFamily family;
    int v3;                                          // FAM_V3: index into V3_TILES
    int bmt, bn, wm, wn, minw, bkt, stg, epi, ntl;   // template arguments of the instantiation (those its family has)
    bool tl;                                         // ragged last 64-channel block ("tail" forms of the halo / v3 kernels)
    int gx, gy;                                      // persistent blocks over the pixel tiles x output-channel tiles
    dim3 grid, block;                                // the launch made of them (parity-class slots in z, flattened rows)
    int stat_rows, bnr_rows;                         // rows of the BatchNorm partial-sum slab / of the fused-reduction slab
    HaloGeom geo;
    ConvK k;
};

// the launch of a plan of the family: every template argument dispatched from the plan, in the family's file
void conv_launch_stem(const ConvPlan& pl, hipStream_t st);
void conv_launch_halo160(const ConvPlan& pl, hipStream_t st);
void conv_launch_halo(const ConvPlan& pl, hipStream_t st);
void conv_launch_v3(const ConvPlan& pl, hipStream_t st);
void conv_launch_v2(const ConvPlan& pl, hipStream_t st);
void conv_launch_generic(const ConvPlan& pl, hipStream_t st);

}  // namespace yh_conv
