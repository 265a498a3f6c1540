// Halo kernel of the implicit-GEMM convolution (conv_igemm.hip plans it: FAM_HALO, geometry from conv_halo_geom).
// halo kernel: 3x3 / stride 1 / pad 1 convolutions (forward and data gradient) without the im2col redundancy on the
// global -> LDS path.  The CU's intake (LDS-DMA through the texture path, ~35-45 B/clk in practice) is what bounds the
// tiles of conv_v3: a 256 x 128 tile needs 48 KB per 64-channel k-step.  Here a block owns a 2-D tile of TH x TW output
// pixels (TH*TW <= 256) of ONE image and stages, per 64-channel block, the (TH+2) x (TW+2) input patch ONCE; the nine taps
// are nine k-steps that read their A fragments from the same patch at a shifted pixel (patch row + dy*(TW+2) + dx), so only
// the weight tile (16 KB) is streamed per k-step: ~22 KB per k-step instead of 48.  Patch rows are 128 bytes, chunk-swizzled
// by the patch row index on the source side of the DMA (as in conv_v3); the patch of the next channel block is prefetched
// in six parts behind the taps 0..5 of the current one; weight tiles go through a 3-stage ring.  MFMA rows that are not an
// output pixel of the tile (ragged tiles) read a zero line, so their accumulators are exact zeros for the statistics.
// (HaloGeom, halo_block_map: conv_igemm.h)
#include "conv_igemm.h"

using namespace yh_conv;

namespace {

// TL (tail): the channel count is a multiple of 16 but not of 64 (YOLOv5m / v5x widths: 96, 80, 160): the last channel block
// runs only (C % 64) / 16 of its four 16-channel sub-steps.  Its DMA still fetches whole 128-byte rows (the bytes behind the
// last channel belong to the next pixel / the next tap's weights, or are zero-filled past the end of the buffer): they are
// never read as fragments.
template <int BN, int EPI, bool TL>
__global__ __launch_bounds__(512, 2) void conv_halo_kernel(const ConvK p, const HaloGeom hg)
{
    constexpr int BMT = 256, WM = 4, WN = 2, BKT = 64, STG = 4;
    constexpr int NWV = WM * WN, NT = NWV * 64;
    constexpr int TM = 2, TN = BN / (WN * 32);
    constexpr int ROWB = BKT * 2, CHR = 8, RPI = 8;
    constexpr int NB = BN / (RPI * NWV);             // weight-tile DMA instructions per wave and k-step (2 | 1)
    constexpr int NPW = 6;                           // patch DMA instructions per wave and channel block (<= 6*8*8 = 384 patch rows)
    constexpr int PATCH_ROWS = 352;                  // >= NP*8, see conv_halo_geom
    constexpr int PATCH_BYTES = PATCH_ROWS * ROWB;   // 45056
    constexpr int BST_BYTES = BN * ROWB;
    constexpr int ZERO_OFF = 2 * PATCH_BYTES + STG * BST_BYTES;       // 128 zero bytes
    constexpr int MAIN_BYTES = ZERO_OFF + 128;
    constexpr int CP = BN + 8;                       // epilogue buffer: 128 rows x CP bf16 inside the idle patch buffer
    static_assert(128 * CP * 2 <= PATCH_BYTES, "epilogue half tile must fit a patch buffer");
    constexpr unsigned OOB = 0x80000000u;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* sConst = reinterpret_cast<float*>(smem + MAIN_BYTES);            // [3][BN]: bias | scale | shift (EPI 2), scale | shift (EPI 3)
    int* sPix = reinterpret_cast<int*>(smem + MAIN_BYTES + 3 * BN * 4);     // [BMT] output pixel of each tile row, -1 = none

    const yh_conv_desc& d = p.d;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN, wn = wave % WN;
    int bx, by;
    halo_block_map(hg, bx, by);
    const int n0 = by * BN;
    const int ncb = (p.Ctot + BKT - 1) / BKT;
    const int tailn = TL ? (p.Ctot % BKT) / 16 : BKT / 16;   // 16-channel sub-steps of the last channel block
    const int H = d.Ho, W = d.Wo;                    // stride 1, pad 1: input grid == output grid
    const int TH = hg.TH, TW = hg.TW, PW = hg.PW, NP = hg.NP;
    const int tiles_per_img = hg.tiles_x * hg.tiles_y;
    const int ntiles = d.B * tiles_per_img;
    const int ldx2 = d.seg[0].ld * 2;
    const bool dgrad = d.mode == YH_CONV_DGRAD;
#if YH_CONV_ABLATE & 1
    const bool mtile_never = d.B < 0;               // timing build: DMA issue compiled in but never taken
#endif

    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)d.seg[0].ptr, 0, p.segbytes[0], 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)d.w, 0, p.wbytes, 0x00020000);

    const int lrow = lane >> 3, lq = lane & 7;
    unsigned voffB[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int row = (j * NWV + wave) * RPI + lrow;
        voffB[j] = (unsigned)(((n0 + row) * p.Ktot + ((lq ^ swz_f<CHR>(row)) * 8)) * 2);
    }
    const int hsel = lane >> 5;
    int rdBk[BKT / 16];                               // weight fragment offsets inside a ring slot, per 16-channel sub-step
#pragma unroll
    for (int ks = 0; ks < BKT / 16; ++ks)
        rdBk[ks] = 2 * PATCH_BYTES + (wn * (TN * 32) + (lane & 31)) * ROWB + (((ks * 2 + hsel) ^ swz_f<CHR>(lane & 31)) << 4);

    if (t < 32) reinterpret_cast<unsigned*>(smem + ZERO_OFF)[t] = 0u;
    if (EPI == 2) {
        for (int i = t; i < 3 * BN; i += NT) {
            const int which = i / BN, c = i - which * BN;
            const float* src = which == 0 ? d.bias : (which == 1 ? d.scale : d.shift);
            sConst[i] = (src && n0 + c < d.N) ? src[n0 + c] : (which == 1 ? 1.f : 0.f);
        }
    }
    if (EPI == 3) {
        for (int i = t; i < 2 * BN; i += NT) {
            const int which = i / BN, c = i - which * BN;
            sConst[i] = (n0 + c < d.N) ? d.bnr_ws[(size_t)which * d.bnr_C + n0 + c] : 0.f;
        }
    }
    // per-thread running sums over the 8 channels of the chunk this thread stores (EPI 1: sum, sum of squares of the stored
    // bf16 values; EPI 3: sum dz, sum dz*z): a thread always handles the same channel chunk (NT % (BN/8) == 0)
    float bs_[8], bq_[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { bs_[e] = 0.f; bq_[e] = 0.f; }
    __syncthreads();

    // tile -> origin, patch-loader offsets (instruction i of this wave fills patch rows (i*8 + wave)*8 .. +8)
    auto patch_offsets = [&](int tile, unsigned (&vo)[NPW]) {
        const int img = tile / tiles_per_img;
        const int trem = tile - img * tiles_per_img;
        const int tyi = trem / hg.tiles_x;
        const int y0 = tyi * TH, x0 = (trem - tyi * hg.tiles_x) * TW;
#pragma unroll
        for (int i = 0; i < NPW; ++i) {
            const int pr = (i * NWV + wave) * RPI + lrow;
            const int py = pr / PW, px = pr - py * PW;
            const int y = y0 - 1 + py, x = x0 - 1 + px;
            const bool ok = pr < (TH + 2) * PW && y >= 0 && y < H && x >= 0 && x < W;
            vo[i] = ok ? (unsigned)((img * H + y) * W + x) * (unsigned)ldx2 + (unsigned)((lq ^ swz_f<CHR>(pr)) * 16) : OOB;
        }
    };
    auto issue_patch_part = [&](const unsigned (&vo)[NPW], int part, int cblk, int pbuf) -> int {   // one instruction of this wave
        const int inst = part * NWV + wave;
        if (inst >= NP) return 0;
        unsigned char* dst = smem + pbuf * PATCH_BYTES + inst * (RPI * ROWB);
#pragma unroll
        for (int i = 0; i < NPW; ++i)
            if (i == part) lds_dma16(rs0, dst, vo[i], cblk * (BKT * 2));
        return 1;
    };
    auto issue_B = [&](int kt2, int slot) {           // weight tile of k-step kt2 (the stream repeats every nkt steps: tile independent)
        const int cblk = kt2 / 9, tap = kt2 - cblk * 9;
        const int sw = (tap * p.Ctot + cblk * BKT) * 2;
        unsigned char* sb = smem + 2 * PATCH_BYTES + slot * BST_BYTES + wave * (RPI * ROWB);
#pragma unroll
        for (int j = 0; j < NB; ++j) lds_dma16(rsw, sb + j * (NWV * RPI * ROWB), voffB[j], sw);
    };

    int tile = bx;
    unsigned voffP[NPW], voffN[NPW];
    int slot = 0, islot = STG - 1, pb = 0;
    if (tile < ntiles) {
        patch_offsets(tile, voffP);
#pragma unroll
        for (int part = 0; part < NPW; ++part) issue_patch_part(voffP, part, 0, 0);
        issue_B(0, 0);
        issue_B(1, 1);                               // nkt >= 9
        issue_B(2, 2);
        YH_VMCNT(NB);                                // patch and the weight tiles of steps 0, 1 have landed; the third stays in flight
    }
    for (; tile < ntiles; tile += hg.gx) {
        const bool has_next = tile + hg.gx < ntiles;
        const int img = tile / tiles_per_img;
        const int trem = tile - img * tiles_per_img;
        const int tyi = trem / hg.tiles_x;
        const int y0 = tyi * TH, x0 = (trem - tyi * hg.tiles_x) * TW;
        // fragment rows of this lane: MFMA row -> tile pixel -> patch row of the tap (dy, dx) = (0, 0)
        int pr0[TM];
        bool inv[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int r = wm * (TM * 32) + i * 32 + (lane & 31);
            const int ty = r / TW, tx = r - ty * TW;
            inv[i] = !(ty < TH && y0 + ty < H && x0 + tx < W);
            pr0[i] = ty * PW + tx;
        }
        for (int r = t; r < BMT; r += NT) {
            const int ty = r / TW, tx = r - ty * TW;
            sPix[r] = (ty < TH && y0 + ty < H && x0 + tx < W) ? ((img * H + y0 + ty) * W + x0 + tx) : -1;
        }

        f32x16_t acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

        // k loop: channel blocks outside, the nine taps fully unrolled inside (tap, its (dy, dx), the patch part and the weight
        // column of the step two ahead are compile-time: the per-step scalar / vector overhead is what bounds this loop, not MFMA)
        int prev_group = 0;
        bf16x8_t afN[TM], bfN[TN];
        for (int cblk = 0; cblk < ncb; ++cblk) {
            const bool last_blk = cblk + 1 == ncb;
            const int ksn = (TL && last_blk) ? tailn : BKT / 16;      // wave-uniform
            if (last_blk && has_next) patch_offsets(tile + hg.gx, voffN);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int kt = cblk * 9 + tap;
                // all DMA groups except the one issued at the previous step must have landed (step 0: waited before the tile)
#if YH_CONV_ABLATE & 1
                YH_VMCNT(0);
#else
                if (kt > 0) YH_VMCNT_SW(prev_group);
#endif
#if !(YH_CONV_ABLATE & 256)
                __builtin_amdgcn_s_barrier();
#endif
                prev_group = 0;
#if YH_CONV_ABLATE & 1
                if (mtile_never)
#endif
                {
                    // weight tile of step kt + 2 (wrapping into the next tile's stream)
                    const int tapB = (tap + STG - 1) % 9;
                    const int cblkB = cblk + ((tap + STG - 1) >= 9 ? 1 : 0);
                    if (cblkB < ncb || has_next) {
                        const int cb2 = cblkB < ncb ? cblkB : 0;
                        const int sw = (tapB * p.Ctot + cb2 * BKT) * 2;
                        unsigned char* sb = smem + 2 * PATCH_BYTES + islot * BST_BYTES + wave * (RPI * ROWB);
#pragma unroll
                        for (int j = 0; j < NB; ++j) lds_dma16(rsw, sb + j * (NWV * RPI * ROWB), voffB[j], sw);
                        prev_group = NB;
                    }
                    if (tap < NPW && !(YH_CONV_ABLATE & 512)) {
                        if (!last_blk) prev_group += issue_patch_part(voffP, tap, cblk + 1, pb ^ 1);
                        else if (has_next) prev_group += issue_patch_part(voffN, tap, 0, pb ^ 1);
                    }
                }
                // fragments of this step: sub-step 0 was requested during the previous step (A from the resident patch, B from a ring
                // slot that had landed one barrier earlier: the ring is one stage deeper than the steps in flight need), so the
                // MFMAs start right behind the barrier; only the first step of a tile loads them here
                bf16x8_t af[TM], bfr[TN];
                if (tap == 0 && cblk == 0) {
                    int tapoff0 = dgrad ? 2 * PW + 2 : 0;
                    asm volatile("" : "+s"(tapoff0));
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        const int pr = pr0[i] + tapoff0;
                        const int fx = swz_f<CHR>(pr);
                        const int ab = inv[i] ? ZERO_OFF : pb * PATCH_BYTES + pr * ROWB + (((fx & 1) ^ hsel) << 4);
                        afN[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(smem + ab + ((inv[i] ? 0 : (fx >> 1)) << 5)));
                    }
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        bfN[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(smem + slot * BST_BYTES + rdBk[0] + j * (32 * ROWB)));
                }
                const int kh = tap / 3, kw = tap % 3;
                int tapoff = dgrad ? (2 - kh) * PW + (2 - kw) : kh * PW + kw;            // scalar
                // keep this step's address arithmetic inside the step: hoisted to the top of the unrolled block it costs 36 live VGPRs
                asm volatile("" : "+s"(tapoff));
                const int sbase = slot * BST_BYTES;
                // A: patch row of this lane's pixel for this tap; rows outside the tile read the 128-byte zero line.  The chunk
                // swizzle (kc ^ f(row)) << 4 with kc = 2 ks + h splits into a per-step term (h ^ f0) << 4 and ((ks ^ f12) << 5)
                int abase[TM], af12[TM];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int pr = pr0[i] + tapoff;
                    const int fx = swz_f<CHR>(pr);
                    abase[i] = inv[i] ? ZERO_OFF : pb * PATCH_BYTES + pr * ROWB + (((fx & 1) ^ hsel) << 4);
                    af12[i] = inv[i] ? 0 : (fx >> 1);
                }
#pragma unroll
                for (int ks = 0; ks < BKT / 16; ++ks) {
                    if (TL && ks >= ksn) continue;
                    if (ks == 0) {
#pragma unroll
                        for (int i = 0; i < TM; ++i) af[i] = afN[i];
#pragma unroll
                        for (int j = 0; j < TN; ++j) bfr[j] = bfN[j];
                    } else {
#pragma unroll
                        for (int i = 0; i < TM; ++i)
                            af[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(smem + abase[i] + ((ks ^ af12[i]) << 5)));
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            bfr[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(smem + sbase + rdBk[ks] + j * (32 * ROWB)));
                    }
                    if (ks == (TL ? 0 : BKT / 16 - 2) && !(tap == 8 && last_blk)) {
                        // request sub-step 0 of the NEXT step (next tap of this channel block, or tap 0 of the next block in the other
                        // patch buffer, whose parts landed before this step's barrier)
                        const int ntap = tap == 8 ? 0 : tap + 1;
                        const int nkh = ntap / 3, nkw = ntap % 3;
                        int ntapoff = dgrad ? (2 - nkh) * PW + (2 - nkw) : nkh * PW + nkw;
                        asm volatile("" : "+s"(ntapoff));
                        const int npb = tap == 8 ? (pb ^ 1) : pb;
                        const int nslot = slot + 1 == STG ? 0 : slot + 1;
#pragma unroll
                        for (int i = 0; i < TM; ++i) {
                            const int pr = pr0[i] + ntapoff;
                            const int fx = swz_f<CHR>(pr);
                            const int ab = inv[i] ? ZERO_OFF : npb * PATCH_BYTES + pr * ROWB + (((fx & 1) ^ hsel) << 4);
                            afN[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(smem + ab + ((inv[i] ? 0 : (fx >> 1)) << 5)));
                        }
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            bfN[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(smem + nslot * BST_BYTES + rdBk[0] + j * (32 * ROWB)));
                    }
                    // operands swapped (D = W x X^T): a lane then holds ONE pixel (lane & 31) and, per register group, four
                    // consecutive channels: the accumulators pack to 8-byte LDS stores in the epilogue
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
                }
                slot = slot + 1 == STG ? 0 : slot + 1;
                islot = islot + 1 == STG ? 0 : islot + 1;
            }
            pb ^= 1;
        }
        // the next tile's patch and first weight tile must have landed before its step 0 (its second weight tile stays in flight);
        // the epilogue works in the patch buffer the next tile does NOT use
        if (has_next) { YH_VMCNT(NB); } else { YH_VMCNT(0); }
        uint16_t* sC = reinterpret_cast<uint16_t*>(smem + (pb ^ 1) * PATCH_BYTES);
        constexpr int CPR = BN / 8;
        constexpr int NCH = 128 * CPR / NT;
        static_assert((128 * CPR) % NT == 0, "chunks must divide over the threads");
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
            YH_LDS_BARRIER();                         // previous phase's readers done (ph 0: every wave is out of the k loop)
            if ((wm >> 1) == ph) {
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int cc = wn * (TN * 32) + j * 32 + 8 * g + 4 * hsel;
                        float4 cb = make_float4(0.f, 0.f, 0.f, 0.f), cs = make_float4(1.f, 1.f, 1.f, 1.f), ct = cb;
                        if (EPI == 2) {
                            cb = *reinterpret_cast<const float4*>(sConst + cc);
                            cs = *reinterpret_cast<const float4*>(sConst + BN + cc);
                            ct = *reinterpret_cast<const float4*>(sConst + 2 * BN + cc);
                        }
#pragma unroll
                        for (int i = 0; i < TM; ++i) {
                            float v0 = acc[i][j][4 * g], v1 = acc[i][j][4 * g + 1], v2 = acc[i][j][4 * g + 2], v3 = acc[i][j][4 * g + 3];
                            if (EPI == 2) {
                                v0 = (v0 + cb.x) * cs.x + ct.x; v1 = (v1 + cb.y) * cs.y + ct.y;
                                v2 = (v2 + cb.z) * cs.z + ct.z; v3 = (v3 + cb.w) * cs.w + ct.w;
                                if (d.act == YH_ACT_SILU) { v0 = silu_fast(v0); v1 = silu_fast(v1); v2 = silu_fast(v2); v3 = silu_fast(v3); }
                            }
                            const int row = (wm & 1) * (TM * 32) + i * 32 + (lane & 31);
                            *reinterpret_cast<uint2*>(sC + row * CP + cc) = make_uint2(pack2(v0, v1), pack2(v2, v3));
                        }
                    }
            }
            YH_LDS_BARRIER();
            uint4 zpre[EPI == 3 ? NCH : 1];
            if (EPI == 3) {
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    const int id = t + i * NT;
                    const int row = id / CPR;
                    const int n = n0 + (id - row * CPR) * 8;
                    const int orow = sPix[ph * 128 + row];
                    zpre[i] = make_uint4(0, 0, 0, 0);
                    if (orow >= 0 && n < d.N) zpre[i] = *reinterpret_cast<const uint4*>(d.bnr_z + (size_t)orow * d.bnr_ldz + n);
                }
            }
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int id = t + i * NT;
                const int row = id / CPR;
                const int cch = id - row * CPR;
                const int n = n0 + cch * 8;
                const int orow_i = sPix[ph * 128 + row];
                if (orow_i >= 0 && n < d.N) {
                    const size_t orow = (size_t)orow_i;
                    uint4 v = *reinterpret_cast<const uint4*>(sC + row * CP + cch * 8);
                    if (EPI == 2) {
                        uint16_t* dst;
                        const bool first = n < d.nsplit;
                        if (first) dst = d.out0 + orow * d.ld0 + n;
                        else       dst = d.out1 + orow * d.ld1 + (n - d.nsplit);
                        const bool addres = (d.res != nullptr) && first;
                        if (addres || d.accumulate) {
                            float f[8];
                            unpack8(v, f);
                            if (addres) {
                                uint4 rv = *reinterpret_cast<const uint4*>(d.res + orow * d.ldr + n);
                                float g2[8]; unpack8(rv, g2);
#pragma unroll
                                for (int e = 0; e < 8; ++e) f[e] += g2[e];
                            }
                            if (d.accumulate) {
                                uint4 ov = *reinterpret_cast<const uint4*>(dst);
                                float g2[8]; unpack8(ov, g2);
#pragma unroll
                                for (int e = 0; e < 8; ++e) f[e] += g2[e];
                            }
                            v = pack8(f);
                        }
                        *reinterpret_cast<uint4*>(dst) = v;
                    } else {
                        if (EPI == 3 && d.accumulate) {
                            const uint4 ov = *reinterpret_cast<const uint4*>(d.out0 + orow * d.ld0 + n);
                            float f[8], g0[8];
                            unpack8(v, f);
                            unpack8(ov, g0);
#pragma unroll
                            for (int e = 0; e < 8; ++e) f[e] += g0[e];
                            v = pack8(f);
                        }
                            *reinterpret_cast<uint4*>(d.out0 + orow * d.ld0 + n) = v;
                        if (EPI == 1) {
                            float f[8];
                            unpack8(v, f);
#pragma unroll
                            for (int e = 0; e < 8; ++e) { bs_[e] += f[e]; bq_[e] += f[e] * f[e]; }
                        }
                        if (EPI == 3) {
                            const uint4 zv = zpre[i];
                            float g2[8], z[8];
                            unpack8(v, g2);
                            unpack8(zv, z);
                            const float4 s0 = *reinterpret_cast<const float4*>(sConst + cch * 8);
                            const float4 s1 = *reinterpret_cast<const float4*>(sConst + cch * 8 + 4);
                            const float4 h0 = *reinterpret_cast<const float4*>(sConst + BN + cch * 8);
                            const float4 h1 = *reinterpret_cast<const float4*>(sConst + BN + cch * 8 + 4);
                            const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                            const float sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                const float a = z[e] * sc[e] + sh[e];
                                const float sg = sigmoid_fast(a);
                                const float dz = g2[e] * (sg * (1.f + a * (1.f - sg)));
                                bs_[e] += dz; bq_[e] += dz * z[e];
                            }
                        }
                    }
                }
            }
        }
        YH_LDS_BARRIER();                             // epilogue buffer and pixel table free for the next tile
#pragma unroll
        for (int i = 0; i < NPW; ++i) voffP[i] = voffN[i];
    }

    // per-block partial sums (EPI 1: statistics row of this block; EPI 3: BatchNorm-backward slab row)
    if (EPI == 1 || EPI == 3) {
        constexpr int CPR2 = BN / 8;
        YH_VMCNT(0);
        float* sRed = reinterpret_cast<float*>(smem);          // [NT][16]
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) { sRed[t * 16 + e] = bs_[e]; sRed[t * 16 + 8 + e] = bq_[e]; }
        __syncthreads();
        for (int i = t; i < 2 * BN; i += NT) {
            const int which = i / BN, c = i - which * BN;
            float v = 0.f;
            for (int j = c / 8; j < NT; j += CPR2) v += sRed[j * 16 + which * 8 + (c & 7)];
            if (EPI == 1) put_stat(d, bx, which, n0 + c, v);
            else if (n0 + c < d.N) put_bnr(d, bx, which, n0 + c, v);
        }
    }
}

template <int BN>
constexpr size_t conv_halo_smem_bytes() {
    return 2 * 352 * 128 + 4 * (size_t)BN * 128 + 128 + 3 * BN * 4 + 256 * 4;
}

template <int BN, bool TL> void halo_launch(const ConvPlan& pl, hipStream_t st)
{
    const size_t sm = conv_halo_smem_bytes<BN>();
    static YhDevOnce attr_set;
    yh_lds_limit(attr_set, {{(const void*)conv_halo_kernel<BN, 0, TL>, (int)sm}, {(const void*)conv_halo_kernel<BN, 1, TL>, (int)sm},
                            {(const void*)conv_halo_kernel<BN, 2, TL>, (int)sm}, {(const void*)conv_halo_kernel<BN, 3, TL>, (int)sm}});
    if (pl.epi == 3)      conv_halo_kernel<BN, 3, TL><<<pl.grid, pl.block, sm, st>>>(pl.k, pl.geo);
    else if (pl.epi == 2) conv_halo_kernel<BN, 2, TL><<<pl.grid, pl.block, sm, st>>>(pl.k, pl.geo);
    else if (pl.epi == 1) conv_halo_kernel<BN, 1, TL><<<pl.grid, pl.block, sm, st>>>(pl.k, pl.geo);
    else                  conv_halo_kernel<BN, 0, TL><<<pl.grid, pl.block, sm, st>>>(pl.k, pl.geo);
}

}  // namespace

void yh_conv::conv_launch_halo(const ConvPlan& pl, hipStream_t st)
{
    if (pl.tl) { if (pl.bn == 64) halo_launch<64, true>(pl, st); else halo_launch<128, true>(pl, st); }
    else       { if (pl.bn == 64) halo_launch<64, false>(pl, st); else halo_launch<128, false>(pl, st); }
}
