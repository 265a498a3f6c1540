// Implicit-GEMM convolution for gfx950: NHWC bf16 activations, packed bf16 weights
// [Npad][taps*Ctot], fp32 accumulate on v_mfma_f32_32x32x16_bf16.
//
//   out[m][n] = sum_{tap,c} X[src(m,tap)][c] * W[n][tap*Ctot + c]      m = (img,ho,wo)
//
// One kernel serves the forward conv (ConvBnAct / Detect, utils/layer_tools.py:82-94,
// :454-470) and the data gradient (transposed gather, YH_CONV_DGRAD); the input may be
// a virtual channel-concat of two buffers, one of them read through a nearest-2x
// upsample (the neck joins of models/normal/yolov5s.py:101-114 are never materialised).
//
// This file is host code only: it plans a launch (conv_plan: family, instantiation, grid, slab rows) and answers the queries from
// the same plan.  The kernels and the template dispatch of each family are in conv_generic.hip, conv_v2.hip, conv_v3.hip,
// conv_halo.hip, conv_halo160.hip and conv_stem.hip; conv_igemm.h is what they share with this file.  The sibling families behind
// d->algo 7..13 plan in their own files (common.h); conv_choose decides once per call between them and the chain, for the launcher
// and every query alike.
#include "conv_igemm.h"
#include <stdlib.h>

using namespace yh_conv;

namespace {

static unsigned long long* g_halo_stamps = nullptr;

// tile geometry of the halo kernel for an H x W map: TH x TW output pixels (<= 256) whose (TH+2) x (TW+2) patch fits 352 rows,
// chosen to waste the fewest MFMA rows (ragged tiles and TH*TW < 256)
bool conv_halo_geom_search(int H, int W, int max_rows, HaloGeom* g);
// the search below is ~200 divisions: its result per map size is kept (the planner runs for every launch).
// max_rows: patch rows one buffer holds (352 with the 64- / 128-channel weight ring, 324 next to the 160-channel one)
bool conv_halo_geom(int H, int W, HaloGeom* g, int max_rows = 352)
{
    struct Memo { int H, W, R; bool ok; HaloGeom g; };
    static thread_local Memo memo[8];
    static thread_local int next = 0;
    for (int i = 0; i < 8; ++i)
        if (memo[i].H == H && memo[i].W == W && memo[i].R == max_rows && H > 0) { *g = memo[i].g; return memo[i].ok; }
    Memo& m = memo[next];
    next = (next + 1) & 7;
    m.H = H; m.W = W; m.R = max_rows;
    m.ok = conv_halo_geom_search(H, W, max_rows, &m.g);
    *g = m.g;
    return m.ok;
}
bool conv_halo_geom_search(int H, int W, int max_rows, HaloGeom* g)
{
    double best = 0.0;
    bool found = false;
    for (int tw = 4; tw <= 64; ++tw) {
        if (tw > W + 3) break;
        const int th = 256 / tw;
        if (th < 1) continue;
        for (int th2 = th; th2 >= (th > 2 ? th - 2 : 1); --th2) {
            const int pw = tw + 2, ph = th2 + 2;
            if (pw * ph > max_rows) continue;
            const int tx = (W + tw - 1) / tw, ty = (H + th2 - 1) / th2;
            const double eff = (double)H * W / ((double)tx * ty * 256.0);
            if (eff > best + 1e-9) {
                best = eff; found = true;
                g->TH = th2; g->TW = tw; g->PW = pw; g->NP = (pw * ph + 7) / 8; g->tiles_x = tx; g->tiles_y = ty;
            }
        }
    }
    return found && best >= 0.6;
}

// YH_CONV_DBG (kernel-selection switches for A/B timing) is read once per process: the planner runs for every launch
int conv_dbg_mask() {
    static const int mask = [] { const char* e = getenv("YH_CONV_DBG"); return e ? atoi(e) : 0; }();
    return mask;
}
// YH_HALO_MAP (block order of the halo / LDS-DMA kernels), read once: -1 unset
int conv_halo_map() {
    static const int v = [] { const char* e = getenv("YH_HALO_MAP"); return e ? atoi(e) : -1; }();
    return v;
}

// epilogue of the v2 / v3 / halo kernels: 3 fused BatchNorm-backward reduction, 2 generic (conv_generic, common.h), 1 BatchNorm partial sums, 0 plain store
inline int conv_epi(const yh_conv_desc* d) { return d->bnr_part ? 3 : (conv_generic(d) ? 2 : (d->stats ? 1 : 0)); }
// stride-2 data gradient processed as four parity classes of output pixels (cls_slot)
inline bool conv_cls(const yh_conv_desc* d) {
    return d->mode == YH_CONV_DGRAD && d->stride == 2 && d->Ho % 2 == 0 && d->Wo % 2 == 0 && d->KH >= 2 && d->KW >= 2 && !d->stats;
}
// bytes a buffer descriptor of segment s / of the weights has to address (< 2 GiB for the buffer-load kernels)
inline unsigned long conv_seg_bytes(const yh_conv_desc* d, int s) {
    const yh_seg& g = d->seg[s];
    const unsigned long npix = (unsigned long)d->B * (d->Hi >> g.ups) * (d->Wi >> g.ups);
    return ((npix - 1) * g.ld + g.C) * 2;
}
inline int conv_ctot(const yh_conv_desc* d) { int c = 0; for (int s = 0; s < d->nseg; ++s) c += d->seg[s].C; return c; }
inline unsigned long conv_w_bytes(const yh_conv_desc* d) { return (unsigned long)d->Npad * d->KH * d->KW * conv_ctot(d) * 2; }
constexpr unsigned long GiB2 = 1ul << 31;

bool stem_eligible(const yh_conv_desc* d)
{
    if (d->mode != YH_CONV_FWD || d->nseg != 1 || d->seg[0].C != 16 || d->seg[0].ups) return false;
    if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != 1) return false;
    if (d->N < 32 || d->N > 96 || d->N % 16 || d->Npad < ((d->N + 31) / 32) * 32) return false;     // 1..3 channel tiles of 32
    if (d->stats && d->N > 64) return false;                                                        // statistics: at most two tiles
    if (d->Wo % 32 || d->bias || d->res || d->accumulate || d->nsplit < d->N) return false;
    if ((d->scale == nullptr) != (d->shift == nullptr)) return false;
    if (d->stats && d->scale) return false;
    if (!d->scale && d->act != YH_ACT_NONE) return false;
    const unsigned long npix = (unsigned long)d->B * d->Hi * d->Wi;
    if (((npix - 1) * d->seg[0].ld + 16) * 2 >= (1ul << 31) || (long)d->B * d->Ho * d->Wo >= (1L << 31) - 64) return false;
    if (conv_dbg_mask() & 256) return false;
    return true;
}
constexpr int STEM_BLOCKS = 256 * 2;

// can this descriptor run on the buffer-load kernel (conv_v2_kernel)?
// `rebased`: the caller re-bases its input descriptors at every tile of <= 256 output rows (conv_v3_kernel), so only the images
// one tile spans have to fit the 2 GiB a descriptor addresses; otherwise the whole segment has to.
static bool conv_buf_ok(const yh_conv_desc* d, bool rebased)
{
    if (d->nseg < 1 || d->nseg > 2) return false;
    if (conv_dbg_mask() & 16) return false;
    if ((long)d->B * d->Hi * d->Wi >= (1L << 31) || (long)d->B * d->Ho * d->Wo >= (1L << 31)) return false;
    for (int s2 = 0; s2 < d->nseg; ++s2) {
        const yh_seg& g = d->seg[s2];
        if (!rebased) {
            if (conv_seg_bytes(d, s2) >= GiB2) return false;  // buffer descriptors address < 2 GiB
        } else {
            // a tile of 256 rows starts in image im0 and ends at most 256 / (rows per image) + 1 images later; the rows per
            // image are Ho*Wo, or a quarter of that for the parity classes of a stride-2 data gradient
            const unsigned long rows_img = (unsigned long)(d->Ho / 2 > 0 ? d->Ho / 2 : 1) * (d->Wo / 2 > 0 ? d->Wo / 2 : 1);
            const unsigned long span = 256 / rows_img + 2;
            const unsigned long pimg = (unsigned long)(d->Hi >> g.ups) * (d->Wi >> g.ups) * g.ld * 2;
            if (span * pimg + 256ul * g.ld * 2 >= GiB2) return false;
        }
    }
    if (conv_w_bytes(d) >= GiB2) return false;
    if (conv_generic(d) && d->stats) return false;                        // statistics of an affine / activated output: generic kernel only
    return true;
}
bool conv_v2_ok(const yh_conv_desc* d) { return conv_buf_ok(d, false); }

int pick_bn(int N) { return N <= 32 ? 32 : (N <= 64 ? 64 : 128); }

// channels per k-step: 64 (128-byte tile rows: whole cache lines per row, half the barriers) when every input
// segment has a multiple of 64 channels (128-wide output tiles only), else 32
int pick_bkt(const yh_conv_desc* d, int bn) {
    if (bn != 128) return 32;              // measured: the narrower tiles lose more from the lower residency than they gain
    if (d->nseg < 1 || d->nseg > 2) return 32;
    for (int s = 0; s < d->nseg; ++s) if (d->seg[s].C % 64) return 32;
    if (d->tile_k == 32) return 32;
    if (conv_dbg_mask() & 64) return 32;
    return 64;
}

int conv_v3_bkt(const yh_conv_desc* d);
// ---- eligibility of the families, asked in the order of conv_plan's chain (each assumes the earlier ones declined)
// LDS-DMA kernel (conv_v3_kernel) variant for this descriptor (V3_TILES): 0 = none (v2 / generic kernel).
// d->algo: 0 library default, 1 force v2, 2..4 = variant 1..3 when eligible, 14 = variant 4 when eligible.
int conv_v3_variant(const yh_conv_desc* d)
{
    if (d->algo == 1 || d->algo == 5 || d->algo == 6 || !conv_buf_ok(d, true)) return 0;
    if (conv_dbg_mask() & 512) return 0;
    const int bkt = conv_v3_bkt(d);
    if (bkt == 0) return 0;
    if (d->N <= 32) return 0;
    if (d->tile_n == 32) return 0;
    if (d->algo >= 2 && d->algo <= 4) return d->algo - 1;
    if (d->algo == 14) {
        // 256 x 256 tile (variant 4): whole 64-channel blocks in every segment, N a multiple of 256, 64-channel k-steps; else the default
        bool ok = bkt == 64 && d->tile_k != 32 && d->N % 256 == 0;
        for (int s = 0; s < d->nseg; ++s) ok = ok && d->seg[s].C % 64 == 0;
        if (ok) return 4;
    }
    // default: the big tile for K-heavy layers with enough pixel tiles to fill the chip, else v2
    const long M = (long)d->B * d->Ho * d->Wo;
    const long K = (long)d->KH * d->KW * conv_ctot(d);
    if (d->N > 64 && K >= 512 && M >= 256L * 192) return 1;
    return 0;
}
// what the two halo kernels share: 3x3 / stride 1 / pad 1 on one input segment that is not upsampled, on the buffer-load path
bool conv_halo_shape_ok(const yh_conv_desc* d)
{
    if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != 1 || d->nseg != 1 || d->seg[0].ups) return false;
    return d->Ho == d->Hi && d->Wo == d->Wi && conv_v2_ok(d);
}
// halo kernel (conv_halo_kernel): >= 64 input channels in a multiple of 16, N > 32.
// d->algo: 5 forces it when eligible; 0 (library default) takes it when the tile geometry wastes < 25 % of the MFMA rows
bool conv_halo_ok(const yh_conv_desc* d, HaloGeom* g)
{
    if (d->algo != 0 && d->algo != 5) return false;
    if (conv_dbg_mask() & 1024) return false;
    if (d->seg[0].C % 16 || d->seg[0].C < 64 || d->N <= 32 || d->tile_n == 32) return false;
    if (!conv_halo_shape_ok(d) || !conv_halo_geom(d->Ho, d->Wo, g)) return false;
    if (d->algo == 0) {
        const double eff = (double)d->Ho * d->Wo / ((double)g->tiles_x * g->tiles_y * 256.0);
        if (eff < 0.75 || (long)d->B * g->tiles_x * g->tiles_y < 128) return false;
    }
    return true;
}
// 160-wide halo kernel (conv_halo160_kernel): only on request (d->algo == 6; the engine times it where it is eligible):
// >= 64 input channels in a multiple of 32, N a multiple of 160, inference epilogues
bool conv_halo160_ok(const yh_conv_desc* d, HaloGeom* g)
{
    if (d->algo != 6) return false;
    if (d->seg[0].C % 32 || d->seg[0].C < 64 || d->N % 160 || d->stats || d->bnr_part) return false;
    return conv_halo_shape_ok(d) && conv_halo_geom(d->Ho, d->Wo, g, YH_H160_ROWS == 328 ? 324 : YH_H160_ROWS);
}

// channels per k-step of the LDS-DMA kernel: 0 = not eligible.  64 needs whole 64-channel blocks in every segment but the
// last, whose channel count may be any multiple of 16 (the "tail" variant of the kernel); 32 needs multiples of 32 everywhere.
// Where both work, 64 is the default (half the barriers) and d->tile_k == 32 selects the short steps.
int conv_v3_bkt(const yh_conv_desc* d) {
    bool ok64 = true, ok32 = true;
    int Ctot = 0;
    for (int s = 0; s < d->nseg; ++s) {
        const int C = d->seg[s].C;
        Ctot += C;
        if (C % 32) ok32 = false;
        if (s + 1 < d->nseg ? (C % 64 != 0) : (C % 16 != 0)) ok64 = false;
    }
    if (Ctot < 64) ok64 = false;
    if (ok64 && !(ok32 && d->tile_k == 32)) return 64;
    return ok32 ? 32 : 0;
}

// Blocks per (parity class, slot) of a stride-2 data gradient on the register-staged / generic kernels.  The nine (class, slot)
// blocks with the same blockIdx.x walk the same pixel regions at the same pace and read the same gy rows (each gy pixel feeds
// nine taps spread over the four classes): with a multiple of 8 blocks per slot they share an XCD (workgroups go round-robin
// to the 8 XCDs by linear id) and the rows are fetched from HBM once per XCD-L2 instead of once per class (measured on the
// YOLOv5s stage-1 / stage-2 layers: +10 % / +7 %).  Rounded DOWN so that the launch still fits one resident wave of blocks.
int cls_inner_blocks(int gx) { return gx >= 32 ? gx / 32 * 32 : gx; }          // whole groups of 4 blocks x 8 XCDs (conv_v2_kernel)
constexpr int CLS_INNER_MIN_TILES = 256;          // conv_v2_kernel: regions per class from which a block walks the four classes itself
int cls_blocks_per_slot(int gx_total, int zslots, long mtiles_cls)
{
    int g = (gx_total + zslots - 1) / zslots;
    if ((g % 8) * 8 <= g) g = (g / 8) * 8;          // at most an eighth of the blocks given up for it
    if (g > mtiles_cls) g = (int)mtiles_cls;
    return g < 1 ? 1 : g;
}

// the planning helpers are called on half-filled descriptors (sizing, tuning): answer 0 instead of dividing by a zero dimension
bool conv_desc_plannable(const yh_conv_desc* d) {
    return d && (d->nseg == 1 || d->nseg == 2) && d->B > 0 && d->Ho > 0 && d->Wo > 0 && d->Hi > 0 && d->Wi > 0 && d->KH > 0 && d->KW > 0 &&
           (d->stride == 1 || d->stride == 2) && d->N > 0 && d->seg[0].C > 0;
}

bool conv_plan(const yh_conv_desc* d, ConvPlan* pl)
{
    if (!conv_desc_plannable(d)) return false;
    const long M = (long)d->B * d->Ho * d->Wo;
    const bool cls = conv_cls(d), generic = conv_generic(d);
    const long mtiles = ((cls ? M / 4 : M) + BM - 1) / BM;
    ConvK& k = pl->k;
    k.d = *d;
    k.M = (int)(cls ? M / 4 : M);
    k.Ctot = conv_ctot(d);
    k.Ktot = d->KH * d->KW * k.Ctot;
    k.nkt = (k.Ktot + BK - 1) / BK;
    k.mtiles = (int)mtiles;
    if (d->mode == YH_CONV_FWD) { k.sa = d->stride; k.sb = 1; k.sc = -d->pad; k.sdshift = 0; }
    else { k.sa = 1; k.sb = -1; k.sc = d->pad; k.sdshift = d->stride == 2 ? 1 : 0; }
    if (k.d.nsplit > k.d.N) k.d.nsplit = k.d.N + 8;   // everything goes to out0
    if (d->nseg == 1) k.d.seg[1] = k.d.seg[0];
    k.dbg = conv_dbg_mask();
    k.cls = cls; k.Hc = cls ? d->Ho / 2 : d->Ho; k.Wc = cls ? d->Wo / 2 : d->Wo;
    k.xgx = k.xgy = 0;
    k.v2 = conv_v2_ok(d) ? 1 : 0;
    k.pointwise = (d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0 && !cls) ? 1 : 0;
    bool addressable = (unsigned long)M < GiB2 - BM && conv_w_bytes(d) < GiB2;        // by one descriptor per operand, not re-based
    for (int s2 = 0; s2 < 2; ++s2) {
        k.segbytes[s2] = 0; k.segbytes64[s2] = 0;
        if (s2 < d->nseg) {
            if (d->seg[s2].ups) k.pointwise = 0;
            const unsigned long bytes = conv_seg_bytes(d, s2);
            if (bytes >= GiB2) addressable = false;
            k.segbytes[s2] = bytes >= GiB2 ? 0x7fffffffu : (unsigned)bytes;          // only read where k.v2 / halo hold
            k.segbytes64[s2] = bytes;
        }
    }
    if (d->nseg == 1) k.segbytes64[1] = k.segbytes64[0];
    k.wbytes = (unsigned)conv_w_bytes(d);
    // the buffer-load kernel walks 32-channel blocks: a first segment must end on a block boundary, the last may be ragged;
    // the generic kernel's fast loader needs whole 32-channel blocks
    k.fast = 1;
    if (d->nseg > 1 && d->seg[0].C % 32) k.fast = 0;
    if ((long)d->B * d->Hi * d->Wi >= (1L << 31)) k.fast = 0;
    if (d->seg[d->nseg - 1].C % 32 && !k.v2) k.fast = 0;

    // ---- family (one ordered chain), tile and persistent blocks gx x gy: exactly one resident wave of blocks (256 CUs x blocks/CU
    // of the instantiation), so there is no partially filled second round; d->grid_cap overrides the cap on gx
    pl->block = dim3(256);
    pl->tl = false;
    pl->v3 = 0;
    long xtiles = mtiles;          // pixel tiles (halo: patches, stem: groups of four strips) the gx blocks walk
    int cap, cap_min = 1;          // most blocks along x, the least the cap goes down to
    if (stem_eligible(d)) {
        pl->family = FAM_STEM;
        pl->epi = d->scale ? 2 : (d->stats ? 1 : 0);
        pl->ntl = (d->N + 31) / 32;
        pl->bn = 32; pl->gy = 1;
        xtiles = (M / 32 + 3) / 4;
        cap = STEM_BLOCKS;
    } else if (conv_halo160_ok(d, &pl->geo) || conv_halo_ok(d, &pl->geo)) {
        pl->family = d->algo == 6 ? FAM_HALO160 : FAM_HALO;
        pl->epi = pl->family == FAM_HALO160 ? (generic ? 2 : 0) : conv_epi(d);
        pl->tl = (k.Ctot % 64) != 0;
        pl->bn = pl->family == FAM_HALO160 ? 160 : (d->N <= 64 ? 64 : 128);
        pl->gy = (d->N + pl->bn - 1) / pl->bn;
        pl->block = dim3(512);
        xtiles = (long)d->B * pl->geo.tiles_x * pl->geo.tiles_y;
        cap = 256 / pl->gy;
    } else if ((pl->v3 = conv_v3_variant(d)) != 0) {
        const V3Tile& t = V3_TILES[pl->v3];
        pl->family = FAM_V3;
        pl->bkt = conv_v3_bkt(d);          // conv_v3_variant already checked the addressing (conv_buf_ok, re-based)
        pl->bmt = t.bmt; pl->bn = t.bn; pl->wm = t.wm; pl->wn = t.wn;
        pl->stg = pl->bkt == 64 ? t.stg64 : t.stg32;
        pl->tl = pl->bkt == 64 && (k.Ctot % 64) != 0;
        pl->epi = conv_epi(d);
        pl->gy = (d->N + t.bn - 1) / t.bn;
        pl->block = dim3(t.wm * t.wn * 64);
        xtiles = ((cls ? M / 4 : M) + t.bmt - 1) / t.bmt;
        cap = (256 * (pl->bkt == 64 ? t.occ64 : t.occ32)) / (pl->gy * (cls ? d->KH * d->KW : 1));
    } else {
        const ConvTile t = conv_tile((d->tile_n == 32 || d->tile_n == 64 || d->tile_n == 128) ? d->tile_n : pick_bn(d->N));
        pl->family = k.v2 ? FAM_V2 : FAM_GENERIC;
        pl->bn = t.bn;
        pl->wm = k.v2 ? t.wm2 : t.wm; pl->wn = k.v2 ? t.wn2 : t.wn; pl->minw = k.v2 ? t.minw2 : t.minw;
        pl->bkt = pick_bkt(d, t.bn);
        pl->epi = conv_epi(d);
        pl->gy = (d->N + t.bn - 1) / t.bn;
        pl->block = dim3(pl->wm * pl->wn * 64);
        xtiles = (M + BM - 1) / BM;          // (not per class: the cap below is what bounds a class launch)
        // also bounds the BatchNorm partial-sum rows the finalize kernel reduces
        cap = (256 * t.occ) / pl->gy / 8 * 8;
        cap_min = 8;
    }
    if (cap < cap_min) cap = cap_min;
    if (d->grid_cap > 0 && pl->family != FAM_STEM) cap = d->grid_cap;
    const int gx = pl->gx = (int)(xtiles < cap ? xtiles : cap), gy = pl->gy;
    pl->stat_rows = gx;          // (statistics exclude the parity classes: one row per gx block in every family)

    // ---- the launch made of gx x gy, and the rows of the fused BatchNorm-backward reduction (one per block along x and z)
    int rows = gx;
    pl->grid = dim3(gx, gy, 1);
    if (pl->family == FAM_STEM) {
        // XCD-aware strip order (see the kernel): whole bands per XCD and whole workgroup octets; YH_STEM_MAP=0: strips in order
        static const int smap = getenv("YH_STEM_MAP") ? atoi(getenv("YH_STEM_MAP")) : 1;
        k.xgx = (smap && gx % 8 == 0 && ((long)d->B * d->Ho) % (8 * STEM_BAND) == 0) ? 1 : 0;
        pl->grid = dim3(gx);
    } else if (pl->family == FAM_HALO160 || pl->family == FAM_HALO) {
        // conv_halo_kernel, measured (profiles/r04_step_experiments.txt j): +0.5 % on YOLOv5x inference, -1 % on the YOLOv5l train step
        // (forward with statistics / data gradients) -> the XCD-major order only under the inference epilogue; YH_HALO_MAP=0: never
        const bool xcd_major = pl->family == FAM_HALO160 || pl->epi == 2;
        pl->geo.gx = gx; pl->geo.gy = gy; pl->geo.rowmajor = (conv_halo_map() == 0 || gy == 1 || !xcd_major) ? 1 : 0;
        pl->geo.stamps = pl->family == FAM_HALO160 ? g_halo_stamps : nullptr;
        pl->grid = dim3(gx * gy);              // one row of workgroups: halo_block_map
    } else if (pl->family == FAM_V3) {
        const int zslots = cls ? d->KH * d->KW : 1;      // (parity class, slot) pairs: see cls_slot
        rows = gx * zslots;
        pl->grid = dim3(gx, gy, zslots);
        // one row of workgroups in XCD-major order, measured: no gain on YOLOv5x inference (707 / 712 -> 691 / 717 img/s), -2 % on the
        // YOLOv5l train step: off (YH_HALO_MAP=2 enables it)
        if (!cls && gy > 1 && conv_halo_map() == 2) { k.xgx = gx; k.xgy = gy; pl->grid = dim3(gx * gy, 1, 1); }
    } else if (cls) {
        // conv_v2_kernel walks the classes of a region inside the block where a class has enough regions: no z dimension.  The rows
        // are conv_v2_kernel's, the only one of the two with the fused reduction (the generic kernel's launch refuses it)
        const int zslots = d->KH * d->KW;
        const int inner = cls_inner_blocks(gx < mtiles ? gx : (int)mtiles), per_slot = cls_blocks_per_slot(gx, zslots, mtiles);
        const bool walk = mtiles >= CLS_INNER_MIN_TILES;
        rows = walk ? inner : per_slot * zslots;
        pl->grid = (walk && k.v2) ? dim3(inner, gy, 1) : dim3(per_slot, gy, zslots);
    }
    // 0: the descriptor cannot take the fused reduction here (the caller keeps the separate yh_bn_silu_bwd_reduce pass)
    pl->bnr_rows = addressable ? rows : 0;
    return true;
}

/* name of the instantiation, as profilers print it */
void conv_plan_name(const ConvPlan& pl, char* out, int len)
{
    const char* tl = pl.tl ? "true" : "false";
    switch (pl.family) {
    case FAM_STEM: snprintf(out, len, "conv_stem_kernel<%d, %d>", pl.epi, pl.ntl); break;
    case FAM_HALO160: snprintf(out, len, "conv_halo160_kernel<%d, %s>", pl.epi, tl); break;
    case FAM_HALO: snprintf(out, len, "conv_halo_kernel<%d, %d, %s>", pl.bn, pl.epi, tl); break;
    case FAM_V3: snprintf(out, len, "conv_v3_kernel<%d, %d, %d, %d, %d, %d, %d, %s>", pl.bmt, pl.bn, pl.wm, pl.wn, pl.bkt, pl.stg, pl.epi, tl); break;
    case FAM_V2: snprintf(out, len, "conv_v2_kernel<%d, %d, %d, %d, %d, %d>", pl.bn, pl.wm, pl.wn, pl.minw, pl.epi, pl.bkt); break;
    case FAM_GENERIC: snprintf(out, len, "conv_igemm_kernel<%d, %d, %d, %s, %d>", pl.bn, pl.wm, pl.wn, pl.k.fast ? "true" : "false", pl.minw); break;
    }
}

int conv_launch(const ConvPlan& pl, hipStream_t st)
{
    static const char* const what[] = {"yh_conv_igemm(stem)", "yh_conv_igemm(halo160)", "yh_conv_igemm(halo)", "yh_conv_igemm(v3)", "yh_conv_igemm(v2)", "yh_conv_igemm"};
    switch (pl.family) {
    case FAM_STEM: conv_launch_stem(pl, st); break;
    case FAM_HALO160: conv_launch_halo160(pl, st); break;
    case FAM_HALO: conv_launch_halo(pl, st); break;
    case FAM_V3: conv_launch_v3(pl, st); break;
    case FAM_V2: conv_launch_v2(pl, st); break;
    case FAM_GENERIC: conv_launch_generic(pl, st); break;
    }
    YH_CHECK_LAUNCH(what[pl.family]);
    return YH_OK;
}

// ---- sibling families (own files, each with its own *_plan) behind d->algo: stride-2 data-gradient kernel (conv_dg2.hip), 3x3 patch
// kernel (conv_p3.hip), 80-channel halo kernel (conv_h80.hip), pointwise kernels (conv_pw.hip, conv_pt.hip), 80 -> 160 kernel
// (conv_c80.hip); 11 is unassigned and so always declines.  `slabs`: the partial-sum slabs the family's kernels write, which are as many
// rows as its grid; a slab it does not write has the rows the chain plans for the descriptor (no launch of the family writes them)
enum ConvSlabs { SLABS_NONE, SLABS_BNR, SLABS_BOTH };          // none / fused reduction / statistics and fused reduction
struct ConvSibling { int algo, family; ConvSlabs slabs; int (*info)(const yh_conv_desc*, ConvSibInfo*); int (*launch)(const yh_conv_desc*, yh_stream); };
const ConvSibling CONV_SIBLINGS[] = {
    {7, YH_CONV_FAM_DG2, SLABS_BNR, yh_dg2_info, yh_dg2_launch},    {8, YH_CONV_FAM_P3, SLABS_BOTH, yh_p3_info, yh_p3_launch},
    {9, YH_CONV_FAM_H80, SLABS_NONE, yh_h80_info, yh_h80_launch},   {10, YH_CONV_FAM_PW, SLABS_NONE, yh_pw_info, yh_pw_launch},
    {11, 0, SLABS_NONE, nullptr, nullptr},                          {12, YH_CONV_FAM_C80, SLABS_NONE, yh_c80_info, yh_c80_launch},
    {13, YH_CONV_FAM_PT, SLABS_BOTH, yh_pt_info, yh_pt_launch},
};

// The one choice behind the launcher and all four queries, made once per call for a plannable d:
//   - the sibling row of d->algo takes d: `sib` (`rc`: its answer), and the chain does not plan;
//   - the row declines, or is unassigned: the chain plans (`pl`) the algo-0 copy of d in `d0`;
//   - there is no such row: the chain plans d as it stands.
// `ask(row)`: how the caller puts d to the sibling, which plans once either way: the launcher by its launch (which, where the
// sibling takes d, is the launch), yh_conv_info by its info.  One sibling plan and one chain plan at the most.
struct ConvChoice { const ConvSibling* sib; int rc; const yh_conv_desc* d; yh_conv_desc d0; ConvPlan pl; };
template <class Ask> void conv_choose(const yh_conv_desc* d, ConvChoice* c, Ask ask)
{
    c->sib = nullptr; c->d = d;
    for (const ConvSibling& s : CONV_SIBLINGS)
        if (s.algo == d->algo) {
            c->rc = s.info ? ask(s) : YH_CONV_DECLINED;
            if (c->rc != YH_CONV_DECLINED) { c->sib = &s; return; }
            c->d0 = *d; c->d0.algo = 0; c->d = &c->d0;
            break;
        }
    conv_plan(c->d, &c->pl);
}
// yh_conv_bnr_rows' own preconditions, which need no plan
bool conv_bnr_possible(const yh_conv_desc* d)
{
    if (d->mode != YH_CONV_DGRAD || d->nseg != 1 || d->seg[0].C % 8 || d->seg[0].ups || d->N % 8) return false;
    return !(conv_generic_na(d) || d->stats || (conv_dbg_mask() & 16));
}

// the argument checks of yh_conv_igemm that need no plan (a descriptor that passes is plannable)
int conv_check_args(const yh_conv_desc* d)
{
    YH_CHECK_ARG(d != nullptr, "yh_conv_igemm: null desc");
    YH_CHECK_ARG(d->nseg == 1 || d->nseg == 2, "yh_conv_igemm: nseg must be 1 or 2 (got %d)", d->nseg);
    YH_CHECK_ARG(d->mode == YH_CONV_FWD || d->mode == YH_CONV_DGRAD, "yh_conv_igemm: bad mode");
    YH_CHECK_ARG(d->stride == 1 || d->stride == 2, "yh_conv_igemm: stride must be 1 or 2");
    YH_CHECK_ARG(d->B > 0 && d->Ho > 0 && d->Wo > 0 && d->Hi > 0 && d->Wi > 0, "yh_conv_igemm: bad dims");
    YH_CHECK_ARG(d->KH > 0 && d->KW > 0 && d->KH <= 7 && d->KW <= 7, "yh_conv_igemm: bad kernel size");
    for (int s = 0; s < d->nseg; ++s) {
        const yh_seg& g = d->seg[s];
        YH_CHECK_ARG(g.ptr && yh_aligned16(g.ptr), "yh_conv_igemm: seg %d pointer null/unaligned", s);
        YH_CHECK_ARG(g.C > 0 && g.C % 8 == 0 && g.ld % 8 == 0 && g.ld >= g.C, "yh_conv_igemm: seg %d C=%d ld=%d must be multiples of 8", s, g.C, g.ld);
        YH_CHECK_ARG(g.ups == 0 || g.ups == 1, "yh_conv_igemm: seg %d bad ups", s);
        if (g.ups) YH_CHECK_ARG(d->Hi % 2 == 0 && d->Wi % 2 == 0, "yh_conv_igemm: upsampled segment needs even Hi/Wi");
    }
    YH_CHECK_ARG(d->w && yh_aligned16(d->w), "yh_conv_igemm: weights null/unaligned");
    YH_CHECK_ARG(d->N > 0 && d->Npad >= d->N && d->Npad % 128 == 0, "yh_conv_igemm: N=%d Npad=%d (Npad must be a multiple of 128)", d->N, d->Npad);
    YH_CHECK_ARG(d->out0 && yh_aligned16(d->out0) && d->ld0 % 8 == 0, "yh_conv_igemm: out0 null/unaligned");
    YH_CHECK_ARG(d->nsplit > 0 && d->nsplit % 8 == 0 || d->nsplit >= d->N, "yh_conv_igemm: nsplit must be a multiple of 8");
    if (d->nsplit < d->N) YH_CHECK_ARG(d->out1 && yh_aligned16(d->out1) && d->ld1 % 8 == 0, "yh_conv_igemm: out1 null/unaligned");
    if (d->res) YH_CHECK_ARG(yh_aligned16(d->res) && d->ldr % 8 == 0, "yh_conv_igemm: res unaligned");
    if (d->mode == YH_CONV_FWD) {
        YH_CHECK_ARG((d->Hi + 2 * d->pad - d->KH) / d->stride + 1 == d->Ho && (d->Wi + 2 * d->pad - d->KW) / d->stride + 1 == d->Wo,
                     "yh_conv_igemm: fwd geometry mismatch Hi=%d Ho=%d k=%d s=%d p=%d", d->Hi, d->Ho, d->KH, d->stride, d->pad);
    } else {
        YH_CHECK_ARG((d->Ho + 2 * d->pad - d->KH) / d->stride + 1 == d->Hi && (d->Wo + 2 * d->pad - d->KW) / d->stride + 1 == d->Wi,
                     "yh_conv_igemm: dgrad geometry mismatch Ho=%d Hi=%d k=%d s=%d p=%d", d->Ho, d->Hi, d->KH, d->stride, d->pad);
    }
    YH_CHECK_ARG((long)d->B * d->Ho * d->Wo < (1L << 31) - BM, "yh_conv_igemm: too many output pixels");
    return YH_OK;
}
// ... and those that read the plan
int conv_check_plan(const yh_conv_desc* d, const ConvPlan& pl)
{
    YH_CHECK_ARG(pl.gy * pl.bn <= d->Npad, "yh_conv_igemm: Npad too small for tile");
    if (d->bnr_part && pl.family != FAM_STEM) {
        YH_CHECK_ARG((pl.k.v2 || pl.family == FAM_V3) && !conv_generic_na(d) && !d->stats && d->mode == YH_CONV_DGRAD,
                     "yh_conv_igemm: the fused BatchNorm-backward reduction needs the plain buffer-load data-gradient path");
        YH_CHECK_ARG(conv_bnr_operands(d) && d->N % 8 == 0, "yh_conv_igemm: bad fused-reduction operands");
    }
    if (pl.family == FAM_HALO160 || pl.family == FAM_HALO) YH_CHECK_ARG(pl.k.v2 && !pl.k.cls, "yh_conv_igemm: the halo kernel needs the buffer-load path");
    return YH_OK;
}
int conv_public_family(ConvFamily f)
{
    static const int pub[] = {YH_CONV_FAM_STEM, YH_CONV_FAM_HALO160, YH_CONV_FAM_HALO, YH_CONV_FAM_V3, YH_CONV_FAM_V2, YH_CONV_FAM_GENERIC};
    return pub[f];
}
}  // namespace

extern "C" int yh_conv_igemm(const yh_conv_desc* d, yh_stream stream)
{
    if (const int rc = conv_check_args(d)) return rc;
    ConvChoice c;
    conv_choose(d, &c, [&](const ConvSibling& s) { return s.launch(d, stream); });
    if (c.sib) return c.rc;
    if (const int rc = conv_check_plan(c.d, c.pl)) return rc;
    return conv_launch(c.pl, (hipStream_t)stream);
}

/* what yh_conv_igemm(d) will launch (include/yolohip.h): the rc of the launch's checks; `out` is filled from the dims alone
 * whenever the descriptor is plannable.  (A sibling checks its fused-reduction operands before it names its kernel: without them
 * the name stays empty.) */
extern "C" int yh_conv_info(const yh_conv_desc* d, yh_conv_plan_info* out)
{
    YH_CHECK_ARG(out != nullptr, "yh_conv_info: null out");
    memset(out, 0, sizeof(*out));
    int rc = conv_check_args(d);
    if (!conv_desc_plannable(d)) return rc;
    ConvChoice c;
    ConvSibInfo si = {};
    conv_choose(d, &c, [&](const ConvSibling& s) { return s.info(d, &si); });
    if (c.sib) {
        out->family = c.sib->family;
        snprintf(out->name, sizeof(out->name), "%s", si.name);
        if (rc == YH_OK) rc = c.rc;
        if (c.sib->slabs != SLABS_BOTH) conv_plan(d, &c.pl);          // a slab the family does not write: the chain's rows for d as it stands
    } else {
        out->family = conv_public_family(c.pl.family);
        out->variant = c.pl.v3;
        out->tail = c.pl.tl ? 1 : 0;
        conv_plan_name(c.pl, out->name, (int)sizeof(out->name));
        if (rc == YH_OK) rc = conv_check_plan(c.d, c.pl);
    }
    // the slabs: the sibling's grid rows where its family writes that slab, else what the chain planned
    out->stat_rows = c.sib && c.sib->slabs == SLABS_BOTH ? si.rows : c.pl.stat_rows;
    if (conv_bnr_possible(d)) out->bnr_rows = c.sib && c.sib->slabs != SLABS_NONE ? si.rows : c.pl.bnr_rows;
    return rc;
}

/* name of the kernel instantiation yh_conv_igemm launches for this descriptor, as profilers print it */
extern "C" int yh_conv_kernel_name(const yh_conv_desc* d, char* buf, int buflen)
{
    YH_CHECK_ARG(buf && buflen >= 64, "yh_conv_kernel_name: buffer too small");
    yh_conv_plan_info o;
    const int rc = yh_conv_info(d, &o);
    if (rc == YH_OK) snprintf(buf, buflen, "%s", o.name);
    return rc;
}

/* rows of the BatchNorm partial-sum slab (d->stats) the launch for this descriptor writes (0 while the descriptor is not plannable) */
extern "C" int yh_conv_stat_blocks(const yh_conv_desc* d) { yh_conv_plan_info o = {}; yh_conv_info(d, &o); return o.stat_rows; }

/* rows of the partial-sum slab a data-gradient launch with the fused BatchNorm-backward reduction (bnr_*) writes:
 * [rows][2][N] floats (sum dz | sum dz*z), consumed by yh_bn_bwd_finalize(part, rows, ...).  0: this descriptor
 * cannot take the fused path (the caller keeps the separate yh_bn_silu_bwd_reduce pass). */
extern "C" int yh_conv_bnr_rows(const yh_conv_desc* d) { yh_conv_plan_info o = {}; yh_conv_info(d, &o); return o.bnr_rows; }

/* diagnostics: a device buffer of grid x 8 x 8 uint64 that receives cycle sums of every workgroup's 2nd tile in conv_halo160_kernel (NULL: off) */
extern "C" void yh_halo_set_stamps(void* p) { g_halo_stamps = (unsigned long long*)p; }
