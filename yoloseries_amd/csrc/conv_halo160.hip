// 160-wide halo kernel of the implicit-GEMM convolution (conv_igemm.hip plans it: FAM_HALO160; YH_H160_STG / YH_H160_ROWS: conv_igemm.h).
// 160-wide variant of the halo kernel for the YOLOv5x widths (N = 160, 320, ...): the 128-wide tiles of conv_halo_kernel compute 256
// channels for 160.  Same structure (2-D pixel tile, patch staged once per 64-channel block and double buffered, nine taps =
// nine k-steps, 4-stage weight ring fed by LDS-DMA), but the wave tile is 64 pixels x 80 channels on
// v_mfma_f32_16x16x32_bf16 (4 x 5 tiles of 16 x 16, nine 16-byte fragment reads per twenty MFMAs) so that 4 x 2 waves cover
// 256 x 160 exactly.  A THREE-stage weight ring (60 KB) leaves 2 x 328 patch rows: the 18 x 18 patch of a 16 x 16 pixel tile fits,
// which tiles the 160 x 160 / 80 x 80 maps of YOLOv5x at 1280^2 without a ragged edge (round 5; the four-stage ring left
// 304 rows -> 23 x 10 tiles, 0.89 / 0.83 of the MFMA rows useful).
// Inference epilogues only (EPI 0 plain, EPI 2 bias / folded BN + SiLU / residual / split destination): YOLOv5x is
// not a training configuration of this build.  Operands swapped as in conv_halo_kernel (D = W x X^T): a lane holds one pixel and four
// consecutive channels per accumulator.
#include "conv_igemm.h"

#ifndef YH_H160_SPLIT_ISSUE
#define YH_H160_SPLIT_ISSUE 1
#endif

using namespace yh_conv;

namespace {

struct H160True { static constexpr bool value = true; };
struct H160False { static constexpr bool value = false; };
typedef unsigned int h160_u32x4 __attribute__((ext_vector_type(4)));
// a 16-byte LDS read the CALLER waits for (h160_wait_frags) before the first use
template <int OFF> __device__ __forceinline__ h160_u32x4 h160_lds16(unsigned addr) {
    h160_u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
// s_waitcnt lgkmcnt(0) tied to the nine fragment registers it makes valid: their uses cannot be scheduled ahead of it
__device__ __forceinline__ void h160_wait_frags(h160_u32x4 (&xf)[4], h160_u32x4 (&wf)[5]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xf[0]), "+v"(xf[1]), "+v"(xf[2]), "+v"(xf[3]), "+v"(wf[0]), "+v"(wf[1]), "+v"(wf[2]), "+v"(wf[3]), "+v"(wf[4]) :: "memory");
}
__device__ __forceinline__ void h160_wait_frags2(h160_u32x4 (&xf)[4], h160_u32x4 (&wf)[5], f32x4_t& last) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xf[0]), "+v"(xf[1]), "+v"(xf[2]), "+v"(xf[3]), "+v"(wf[0]), "+v"(wf[1]), "+v"(wf[2]), "+v"(wf[3]), "+v"(wf[4]), "+v"(last) :: "memory");
}
template <int EPI, bool TL>
__global__ __launch_bounds__(512, 1) void conv_halo160_kernel(const ConvK p, const HaloGeom hg)
{
    constexpr int BN = 160, BMT = 256, WN = 2, BKT = 64, STG = YH_H160_STG;
    constexpr int NWV = 8, NT = 512;
    constexpr int TMR = 4, TNC = 5;                  // 16-pixel / 16-channel tiles per wave (64 x 80)
    constexpr int ROWB = BKT * 2, CHR = 8, RPI = 8;
    // BN / RPI = 20 weight-tile DMA instructions per k-step: 3 for waves 0..3, 2 for waves 4..7
    constexpr int PATCH_ROWS = YH_H160_ROWS;          // multiple of 8: a DMA instruction writes 8 rows
    constexpr int NPW = (PATCH_ROWS / 8 + NWV - 1) / NWV;   // patch DMA instructions per wave and channel block (one per tap step: <= 9)
    static_assert(PATCH_ROWS % 8 == 0 && NPW <= 9 && STG >= 3 && STG <= 4, "patch parts ride on the tap steps");
    constexpr int PATCH_BYTES = PATCH_ROWS * ROWB;   // 38912
    constexpr int BST_BYTES = BN * ROWB;             // 20480
    constexpr int ZERO_OFF = 2 * PATCH_BYTES + STG * BST_BYTES;
    constexpr int MAIN_BYTES = ZERO_OFF + 128;
    constexpr int CP = BN + 8;                       // epilogue buffer: 64 rows x CP bf16 inside the idle patch buffer
    static_assert(64 * CP * 2 <= PATCH_BYTES, "epilogue quarter tile must fit a patch buffer");
    static_assert(EPI == 0 || EPI == 2, "inference epilogues only");
    constexpr unsigned OOB = 0x80000000u;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) unsigned char*)smem);
    float* sConst = reinterpret_cast<float*>(smem + MAIN_BYTES);            // [3][BN]: bias | scale | shift
    int* sPix = reinterpret_cast<int*>(smem + MAIN_BYTES + 3 * BN * 4);     // [BMT] output pixel of each tile row, -1 = none

    const yh_conv_desc& d = p.d;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN, wn = wave % WN;
    int bx, by;
    halo_block_map(hg, bx, by);
    const int n0 = by * BN;
    const int ncb = TL ? (p.Ctot + BKT - 1) / BKT : p.Ctot / BKT;
    const int H = d.Ho, W = d.Wo;
    const int TH = hg.TH, TW = hg.TW, PW = hg.PW, NP = hg.NP;
    const int tiles_per_img = hg.tiles_x * hg.tiles_y;
    const int ntiles = d.B * tiles_per_img;
    const int ldx2 = d.seg[0].ld * 2;
    const bool dgrad = d.mode == YH_CONV_DGRAD;
    const int nbw = wave < 4 ? 3 : 2;                // weight DMA instructions of this wave per k-step

    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)d.seg[0].ptr, 0, p.segbytes[0], 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)d.w, 0, p.wbytes, 0x00020000);

    const int lrow = lane >> 3, lq = lane & 7;
    unsigned voffB[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int row = (j * NWV + wave) * RPI + lrow;             // j = 2: rows 128 .. 159 (waves 0..3 only)
        voffB[j] = (unsigned)(((n0 + row) * p.Ktot + ((lq ^ swz_f<CHR>(row)) * 8)) * 2);
    }
    // fragment geometry of v_mfma_f32_16x16x32_bf16: lane l supplies row / column (l & 15), k = 8 (l >> 4) .. +8
    const int l15 = lane & 15, kq = lane >> 4;
    int rdW[2];                                       // weight fragment offset inside a ring slot per 32-channel sub-step (+ j * 16 rows)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
        rdW[ks] = 2 * PATCH_BYTES + (wn * 80 + l15) * ROWB + (((ks * 4 + kq) ^ swz_f<CHR>(l15)) << 4);
    // rows of a wave's channel tiles differ by multiples of 16: swz_f(row) = (row >> 1) & 7 then differs by 8 j mod 8 = 0, so the
    // lane's swizzle term is the same for every tile j

    if (t < 32) reinterpret_cast<unsigned*>(smem + ZERO_OFF)[t] = 0u;
    if (EPI == 2) {
        for (int i = t; i < 3 * BN; i += NT) {
            const int which = i / BN, c = i - which * BN;
            const float* src = which == 0 ? d.bias : (which == 1 ? d.scale : d.shift);
            sConst[i] = (src && n0 + c < d.N) ? src[n0 + c] : (which == 1 ? 1.f : 0.f);
        }
    }
    __syncthreads();

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
    auto issue_patch_part = [&](const unsigned (&vo)[NPW], int part, int cblk, int pbuf) -> int {
        const int inst = part * NWV + wave;
        if (inst >= NP) return 0;
        unsigned char* dst = smem + pbuf * PATCH_BYTES + inst * (RPI * ROWB);
#pragma unroll
        for (int i = 0; i < NPW; ++i)
            if (i == part) lds_dma16(rs0, dst, vo[i], cblk * (BKT * 2));
        return 1;
    };
    auto issue_W = [&](int tap, int cblk, int slot) {
        const int sw = (tap * p.Ctot + cblk * BKT) * 2;
        unsigned char* sb = smem + 2 * PATCH_BYTES + slot * BST_BYTES + wave * (RPI * ROWB);
        lds_dma16(rsw, sb, voffB[0], sw);
        lds_dma16(rsw, sb + NWV * RPI * ROWB, voffB[1], sw);
        if (wave < 4) lds_dma16(rsw, sb + 2 * NWV * RPI * ROWB, voffB[2], sw);
    };

    int tile = bx;
    unsigned voffP[NPW];             // patch offsets of the tile whose patch parts are being requested: this tile's; from its last
                                     // channel block on, the next tile's (the current ones are dead by then)
    int slot = 0, islot = STG - 1, pb = 0;
    if (tile < ntiles) {
        patch_offsets(tile, voffP);
#pragma unroll
        for (int part = 0; part < NPW; ++part) issue_patch_part(voffP, part, 0, 0);
        issue_W(0, 0, 0);
        issue_W(1, 0, 1);                             // nine taps per channel block: steps 0..STG-2 are taps 0.. of block 0
        if (STG == 4) issue_W(2, 0, 2);
        if (wave < 4) { YH_VMCNT(3); } else { YH_VMCNT(2); }   // patch + all weight tiles but the last one issued have landed
    }
    for (; tile < ntiles; tile += hg.gx) {
        const bool has_next = tile + hg.gx < ntiles;
        const int img = tile / tiles_per_img;
        const int trem = tile - img * tiles_per_img;
        const int tyi = trem / hg.tiles_x;
        const int y0 = tyi * TH, x0 = (trem - tyi * hg.tiles_x) * TW;
        int pr0[TMR];
        bool inv[TMR];
#pragma unroll
        for (int i = 0; i < TMR; ++i) {
            const int r = wm * 64 + i * 16 + l15;
            const int ty = r / TW, tx = r - ty * TW;
            inv[i] = !(ty < TH && y0 + ty < H && x0 + tx < W);
            pr0[i] = ty * PW + tx;
        }
        for (int r = t; r < BMT; r += NT) {
            const int ty = r / TW, tx = r - ty * TW;
            sPix[r] = (ty < TH && y0 + ty < H && x0 + tx < W) ? ((img * H + y0 + ty) * W + x0 + tx) : -1;
        }

        f32x4_t acc[TMR][TNC];
#pragma unroll
        for (int i = 0; i < TMR; ++i)
#pragma unroll
            for (int j = 0; j < TNC; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

        int prev_group = 0;
        h160_u32x4 xfA[TMR], wfA[TNC], xfB[TMR], wfB[TNC];
        bool pendB = false;                           // wave-uniform: a second sub-step waits in xfB / wfB
        const bool stamp = hg.stamps != nullptr && tile == bx + hg.gx;        // wave-uniform
        unsigned long long tq0 = 0, tq1, tq2, s_wait = 0, s_issue = 0, s_mfma = 0, t_begin = 0;
        if (stamp) t_begin = __builtin_amdgcn_s_memtime();
        // one 64-channel block = nine tap steps.  TWO: the block has both 32-channel sub-steps (all but the tail block of a TL
        // kernel, whose channel count ends in a half block) — a compile-time property of the step's code: with the pipeline
        // state in run-time flags the compiler fenced every step's reads and MFMAs into separate regions
        auto do_block = [&](auto two_tag, const int cblk) {
            constexpr bool TWO = decltype(two_tag)::value;
            const bool last_blk = cblk + 1 == ncb;
            if (last_blk && has_next) patch_offsets(tile + hg.gx, voffP);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int kt = cblk * 9 + tap;
                // all DMA groups except the one issued at the previous step must have landed (step 0: waited before the tile)
                if (stamp) tq0 = __builtin_amdgcn_s_memtime();
                if (kt > 0) YH_VMCNT_SW(prev_group);
                __builtin_amdgcn_s_barrier();
                if (stamp) { tq1 = __builtin_amdgcn_s_memtime(); s_wait += tq1 - tq0; }
                prev_group = 0;
                auto issue_step = [&]() {
                    // weight tile of step kt + STG - 1 (wrapping into the next tile's stream)
                    const int tapB = (tap + STG - 1) % 9;
                    const int cblkB = cblk + ((tap + STG - 1) >= 9 ? 1 : 0);
                    if (cblkB < ncb || has_next) {
                        issue_W(tapB, cblkB < ncb ? cblkB : 0, islot);
                        prev_group = nbw;
                    }
                    if (tap < NPW && !(YH_CONV_ABLATE & 512)) {
                        if (!last_blk) prev_group += issue_patch_part(voffP, tap, cblk + 1, pb ^ 1);
                        else if (has_next) prev_group += issue_patch_part(voffP, tap, 0, pb ^ 1);
                    }
                };
                // The two waves of a SIMD (w and w + 4) come out of the barrier together: waves 0..3 request the step's transfers
                // first, waves 4..7 after their first sub-step, so one of the pair issues MFMAs while the other one issues transfers
                // (stamps: the transfers of a step cost ~390 cycles of issue during which the SIMD ran no MFMA)
                const bool issue_first = !YH_H160_SPLIT_ISSUE || wave < 4;
                if (issue_first) issue_step();
                if (stamp) { tq2 = __builtin_amdgcn_s_memtime(); s_issue += tq2 - tq1; }
                const int kh = tap / 3, kw = tap % 3;
                int tapoff = dgrad ? (2 - kh) * PW + (2 - kw) : kh * PW + kw;            // scalar
                asm volatile("" : "+s"(tapoff));
                const int sbase = slot * BST_BYTES;
                int abase[TMR], afx[TMR];
#pragma unroll
                for (int i = 0; i < TMR; ++i) {
                    const int pr = pr0[i] + tapoff;
                    abase[i] = inv[i] ? ZERO_OFF : pb * PATCH_BYTES + pr * ROWB;
                    afx[i] = inv[i] ? -1 : swz_f<CHR>(pr);
                }
                // Software pipeline over the sub-steps (round 5; stamps showed two exposed LDS round trips per step — both waves of a
                // SIMD leave the barrier together and waited for their fragments at the same time): the fragments of this step's
                // FIRST sub-step are requested, the MFMAs of the PREVIOUS step's second sub-step (fragments already in registers: its
                // ring slot may be refilled by now) run while they arrive, then the second sub-step's fragments are requested behind
                // the first sub-step's MFMAs and wait in registers for the next step.
                // The fragment reads are inline asm, invisible to the compiler's s_waitcnt bookkeeping (it answered every read that
                // crosses a loop iteration with lgkmcnt(0) right behind it); the waits are the explicit ones below, tied to the
                // registers they make valid.
                auto read_frags = [&](int ks, h160_u32x4 (&xf)[TMR], h160_u32x4 (&wf)[TNC]) {
                    const unsigned wb = lds0 + (unsigned)(sbase + rdW[ks]);
                    wf[0] = h160_lds16<0>(wb); wf[1] = h160_lds16<16 * ROWB>(wb); wf[2] = h160_lds16<32 * ROWB>(wb);
                    wf[3] = h160_lds16<48 * ROWB>(wb); wf[4] = h160_lds16<64 * ROWB>(wb);
#pragma unroll
                    for (int i = 0; i < TMR; ++i) {
                        const int off = afx[i] < 0 ? (kq << 4) : (((ks * 4 + kq) ^ afx[i]) << 4);
                        xf[i] = h160_lds16<0>(lds0 + (unsigned)(abase[i] + off));
                    }
                };
                auto mfma_row = [&](int i, const h160_u32x4 (&xf)[TMR], const h160_u32x4 (&wf)[TNC]) {
#pragma unroll
                    for (int j = 0; j < TNC; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wf[j]), __builtin_bit_cast(bf16x8_t, xf[i]), acc[i][j], 0, 0, 0);
                };
                read_frags(0, xfA, wfA);
                // a pending second sub-step: inside a block the previous step's (TWO), at a block's first step what the flag says
                if (tap == 0 ? pendB : TWO) {
#pragma unroll
                    for (int i = 0; i < TMR; ++i) mfma_row(i, xfB, wfB);
                }
                if (!issue_first) issue_step();
                h160_wait_frags2(xfA, wfA, acc[TMR - 1][TNC - 1]);            // arrived during the MFMAs above (a tile's first step: exposed once)
                mfma_row(0, xfA, wfA);
                if (TWO) read_frags(1, xfB, wfB);
#pragma unroll
                for (int i = 1; i < TMR; ++i) mfma_row(i, xfA, wfA);
                // the second sub-step's fragments land behind those 15 MFMAs, before the next barrier lets the slot be refilled
                if (TWO) h160_wait_frags2(xfB, wfB, acc[TMR - 1][TNC - 1]);
                if (tap == 8) pendB = TWO;
                // the second sub-step's fragments have landed (behind 20 MFMAs) before the next barrier lets the slot be refilled
                if (stamp) s_mfma += __builtin_amdgcn_s_memtime() - tq2;
                slot = slot + 1 == STG ? 0 : slot + 1;
                islot = islot + 1 == STG ? 0 : islot + 1;
            }
            pb ^= 1;
        };
        const int nfull = TL ? ncb - 1 : ncb;         // TL: the channel count ends in a half block (C % 64 == 32)
        for (int cblk = 0; cblk < nfull; ++cblk) do_block(H160True{}, cblk);
        if (TL) do_block(H160False{}, ncb - 1);
        if (pendB) {
#pragma unroll
            for (int i = 0; i < TMR; ++i)
#pragma unroll
                for (int j = 0; j < TNC; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wfB[j]), __builtin_bit_cast(bf16x8_t, xfB[i]), acc[i][j], 0, 0, 0);
        }
        unsigned long long t_loop = 0, t_act = 0;
        if (stamp) t_loop = __builtin_amdgcn_s_memtime();
        // the next tile's patch and all its weight tiles issued so far but the last must have landed before its step 0;
        // the epilogue works in the patch buffer the next tile does NOT use
        if (has_next) { if (wave < 4) { YH_VMCNT(3); } else { YH_VMCNT(2); } } else { YH_VMCNT(0); }
        uint16_t* sC = reinterpret_cast<uint16_t*>(smem + (pb ^ 1) * PATCH_BYTES);
        constexpr int CPR = BN / 8;                   // 20 chunks of 8 channels per row
        // bias / folded BatchNorm / SiLU of the whole tile first, by all eight waves at once: inside the phases below only the two
        // waves of one pixel row-group are active, and the activation (80 values per lane, two quarter-rate transcendentals each)
        // would run on two of the four SIMDs at a time
        if (EPI == 2) {
#pragma unroll
            for (int j = 0; j < TNC; ++j) {
                const int cc = wn * 80 + j * 16 + 4 * kq;
                const float4 cb = *reinterpret_cast<const float4*>(sConst + cc);
                const float4 cs = *reinterpret_cast<const float4*>(sConst + BN + cc);
                const float4 ct = *reinterpret_cast<const float4*>(sConst + 2 * BN + cc);
#pragma unroll
                for (int i = 0; i < TMR; ++i) {
                    float v0 = (acc[i][j][0] + cb.x) * cs.x + ct.x, v1 = (acc[i][j][1] + cb.y) * cs.y + ct.y;
                    float v2 = (acc[i][j][2] + cb.z) * cs.z + ct.z, v3 = (acc[i][j][3] + cb.w) * cs.w + ct.w;
                    if (d.act == YH_ACT_SILU) { v0 = silu_fast(v0); v1 = silu_fast(v1); v2 = silu_fast(v2); v3 = silu_fast(v3); }
                    acc[i][j][0] = v0; acc[i][j][1] = v1; acc[i][j][2] = v2; acc[i][j][3] = v3;
                }
            }
        }
        if (stamp) t_act = __builtin_amdgcn_s_memtime();
#pragma unroll 1
        for (int ph = 0; ph < 4; ++ph) {
            YH_LDS_BARRIER();                         // previous phase's readers done (ph 0: every wave is out of the k loop)
            if (wm == ph) {
#pragma unroll
                for (int j = 0; j < TNC; ++j) {
                    const int cc = wn * 80 + j * 16 + 4 * kq;
#pragma unroll
                    for (int i = 0; i < TMR; ++i)
                        *reinterpret_cast<uint2*>(sC + (i * 16 + l15) * CP + cc) =
                            make_uint2(pack2(acc[i][j][0], acc[i][j][1]), pack2(acc[i][j][2], acc[i][j][3]));
                }
            }
            YH_LDS_BARRIER();
            for (int id = t; id < 64 * CPR; id += NT) {
                const int row = id / CPR;
                const int cch = id - row * CPR;
                const int n = n0 + cch * 8;
                const int orow_i = sPix[ph * 64 + row];
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
                        *reinterpret_cast<uint4*>(d.out0 + orow * d.ld0 + n) = v;
                    }
                }
            }
        }
        YH_LDS_BARRIER();                             // epilogue buffer and pixel table free for the next tile
        if (stamp && lane == 0) {
            unsigned long long* o = hg.stamps + ((size_t)blockIdx.x * NWV + wave) * 8;
            const unsigned long long t_end = __builtin_amdgcn_s_memtime();
            o[0] = s_wait; o[1] = s_issue; o[2] = s_mfma; o[3] = t_loop - t_begin; o[4] = t_act - t_loop; o[5] = t_end - t_act; o[6] = t_end - t_begin; o[7] = 1;
        }
    }
}

constexpr size_t conv_halo160_smem_bytes() { return 2 * YH_H160_ROWS * 128 + YH_H160_STG * 160 * 128 + 128 + 3 * 160 * 4 + 256 * 4; }
static_assert(conv_halo160_smem_bytes() <= 160 * 1024, "LDS budget of conv_halo160_kernel");

}  // namespace

void yh_conv::conv_launch_halo160(const ConvPlan& pl, hipStream_t st)
{
    const size_t sm = conv_halo160_smem_bytes();
    static YhDevOnce attr_set;
    yh_lds_limit(attr_set, {{(const void*)conv_halo160_kernel<0, false>, (int)sm}, {(const void*)conv_halo160_kernel<0, true>, (int)sm},
                            {(const void*)conv_halo160_kernel<2, false>, (int)sm}, {(const void*)conv_halo160_kernel<2, true>, (int)sm}});
    if (pl.epi == 2) { if (pl.tl) conv_halo160_kernel<2, true><<<pl.grid, pl.block, sm, st>>>(pl.k, pl.geo); else conv_halo160_kernel<2, false><<<pl.grid, pl.block, sm, st>>>(pl.k, pl.geo); }
    else             { if (pl.tl) conv_halo160_kernel<0, true><<<pl.grid, pl.block, sm, st>>>(pl.k, pl.geo); else conv_halo160_kernel<0, false><<<pl.grid, pl.block, sm, st>>>(pl.k, pl.geo); }
}
