// LDS-DMA kernel of the implicit-GEMM convolution (conv_igemm.hip plans it: FAM_V3, tiles in V3_TILES).
// v3: the main loop restructured around LDS-DMA.  A/B tiles go global -> LDS directly (buffer_load ... lds, 1 KiB per
// wave instruction, no VGPR staging and no ds_write phase) into a ring of STG stages; a wave waits only for ITS OWN
// transfers of the stage it is about to read (counted s_waitcnt vmcnt(N): the younger stages stay in flight across the
// barrier), then ONE raw s_barrier per k-step both publishes that stage and frees the stage consumed one step earlier,
// which is refilled at once.  Wave tile 64 x 64 (four MFMAs per four fragment reads: half the LDS read traffic per
// MFMA of the 32 x 64 wave tile of v2), block tile BMT x BN = 256 x 128 (8 waves) or 128 x 128 / 128 x 64 (4 waves).
// LDS rows are unpadded (an LDS-DMA instruction writes 1 KiB contiguously: lane l -> base + 16 l); bank conflicts are
// avoided by an XOR swizzle of the 16-byte chunks applied on the SOURCE side (the lane that fills LDS chunk position q
// of row r fetches global chunk q ^ f(r)) and again on the fragment reads.  Padding taps / rows past M carry an
// out-of-range offset: the range check of the buffer descriptor makes the DMA write zeros.
// Eligible when every segment has a multiple of BKT channels (host check); everything else runs on v2.
// (swz_f: conv_igemm.h)
#include "conv_igemm.h"

using namespace yh_conv;

namespace {

// TL (tail, BKT 64 only): the channel count is a multiple of 16 but not of 64 (YOLOv5m / v5x widths: 96, 80, 160, 320 + 160 ...):
// the last channel block of every tap runs (C % 64) / 16 of its four 16-channel sub-steps.  Its rows are still fetched whole
// (128 bytes: the bytes behind the last channel are the next pixel's / the next tap's, zeros past the end of the buffer)
// and never read as fragments.
template <int BMT, int BN, int WM, int WN, int BKT, int STG, int EPI, bool TL = false>
__global__ __launch_bounds__(WM * WN * 64, 2) void conv_v3_kernel(const ConvK p)
{
    static_assert(!TL || BKT == 64, "tail blocks: 64-channel k-steps only");
    constexpr int NWV = WM * WN;
    constexpr int NT = NWV * 64;
    constexpr int TM = BMT / (WM * 32);
    constexpr int TN = BN / (WN * 32);
    constexpr int ROWB = BKT * 2;                   // bytes per tile row
    constexpr int CHR = BKT / 8;                    // 16-byte chunks per tile row
    constexpr int RPI = 1024 / ROWB;                // tile rows one LDS-DMA wave instruction fills
    constexpr int NA = BMT / (RPI * NWV);           // A instructions per wave and stage
    constexpr int NB = BN / (RPI * NWV);            // B instructions per wave and stage
    constexpr int LPS = NA + NB;                    // LDS-DMA instructions per wave and stage
    constexpr int STAGE_BYTES = (BMT + BN) * ROWB;
    constexpr int CP = BN + 8;
    constexpr int RING_BYTES = STG * STAGE_BYTES;
    constexpr int MAIN_BYTES = RING_BYTES > (BMT * CP * 2) ? RING_BYTES : (BMT * CP * 2);
    constexpr unsigned OOB = 0x80000000u;
    static_assert(NA >= 1 && NB >= 1 && BMT % (RPI * NWV) == 0 && BN % (RPI * NWV) == 0, "tile / wave count mismatch");
    static_assert(STG >= 2 && STG <= 4, "2..4 stages");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* sC = reinterpret_cast<uint16_t*>(smem);
    float* sStat = reinterpret_cast<float*>(smem + MAIN_BYTES);
    int* sPix = reinterpret_cast<int*>(smem + MAIN_BYTES + WM * 2 * BN * 4);

    const yh_conv_desc& d = p.d;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN;
    const int wn = wave % WN;
    // the gy output-channel tiles of an m-tile read the same input rows: as grid rows they are gx workgroups apart (other XCDs, other
    // times: every one fetches the rows again — PMC on YOLOv5x stage-2 conv, 3x3 / s2, 3 channel tiles: 30 GB fetched for a 4.2 GB
    // input); launched as one row in XCD-major (slot, channel tile) order they share an XCD's L2 (halo_block_map)
    int bx = blockIdx.x, by = blockIdx.y, gdx = gridDim.x;
    if (p.xgx > 0) {
        const int nb = p.xgx * p.xgy, lin = blockIdx.x, x = lin & 7, q = nb >> 3, r = nb & 7;
        const int vid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (lin >> 3);
        bx = vid / p.xgy; by = vid - bx * p.xgy; gdx = p.xgx;
    }
    const int n0 = by * BN;
    const int HoWo = d.Ho * d.Wo;
    const int sdmask = (1 << p.sdshift) - 1;
    int ph = 0, pw = 0, zslot = 0, zslots = 1;
    if (p.cls) cls_slot(d, blockIdx.z, ph, pw, zslot, zslots);
    const int kh0 = (ph + d.pad) & 1, kw0 = (pw + d.pad) & 1;
    const int nkw = p.cls ? (d.KW - kw0 + 1) / 2 : d.KW;
    const int nkh = p.cls ? (d.KH - kh0 + 1) / 2 : d.KH;
    const int ncb = TL ? (p.Ctot + BKT - 1) / BKT : p.Ctot / BKT;
    const int tailn = TL ? (p.Ctot % BKT) / 16 : BKT / 16;
    const int nkt = nkh * nkw * ncb;
    const int HcWc = p.Hc * p.Wc;
    const int C0 = d.seg[0].C;
    const int mtiles = (p.M + BMT - 1) / BMT;

    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)d.w, 0, p.wbytes, 0x00020000);
    // Input descriptors are re-based at every tile (to the first pixel row of a pointwise tile, else to the first image the
    // tile touches), so the 32-bit lane offsets stay tile-relative and an input tensor may be larger than the 2 GiB one
    // descriptor can address (the host checks that the images one tile spans fit: conv_v3_span_ok).
    const unsigned long pimg0 = (unsigned long)(d.Hi >> d.seg[0].ups) * (d.Wi >> d.seg[0].ups) * (unsigned long)(d.seg[0].ld * 2);
    const unsigned long pimg1 = (unsigned long)(d.Hi >> d.seg[1].ups) * (d.Wi >> d.seg[1].ups) * (unsigned long)(d.seg[1].ld * 2);
    auto rebased = [](const void* ptr, unsigned long off, unsigned long total) {
        const unsigned long rem = total - off;
        return __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const char*>(ptr) + off), 0,
                                                 rem > 0x7fffffffUL ? 0x7fffffffu : (unsigned)rem, 0x00020000);
    };

    // loader geometry: instruction i of this wave fills tile rows (i*NWV + wave)*RPI .. +RPI; this lane's row / chunk
    const int lrow = lane / CHR, lq = lane % CHR;
    unsigned voffB[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int row = (j * NWV + wave) * RPI + lrow;
        voffB[j] = (unsigned)(((n0 + row) * p.Ktot + ((lq ^ swz_f<CHR>(row)) * 8)) * 2);
    }
    unsigned chA[NA];                                // byte offset of this lane's (swizzled) source chunk inside the k-block
#pragma unroll
    for (int i = 0; i < NA; ++i) chA[i] = (unsigned)((lq ^ swz_f<CHR>((i * NWV + wave) * RPI + lrow)) * 16);

    // fragment reads: rows of a wave tile differ by multiples of 32, so the swizzle term depends on the lane only
    const int fx = swz_f<CHR>(lane & 31);
    int koff[BKT / 16];
#pragma unroll
    for (int ks = 0; ks < BKT / 16; ++ks) koff[ks] = ((ks * 2 + (lane >> 5)) ^ fx) * 16;
    const int rdA0 = (wm * (TM * 32) + (lane & 31)) * ROWB;                 // + i*32*ROWB
    const int rdB0 = BMT * ROWB + (wn * (TN * 32) + (lane & 31)) * ROWB;    // + j*32*ROWB

    float run_s = 0.f, run_q = 0.f;
    float bs_[8], bq_[8];
    if (EPI == 3) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { bs_[e] = 0.f; bq_[e] = 0.f; }
        for (int i = t; i < 2 * BN; i += NT) {
            const int which = i / BN, c = i - which * BN;
            sStat[i] = (n0 + c < d.N) ? d.bnr_ws[(size_t)which * d.bnr_C + n0 + c] : 0.f;
        }
        __syncthreads();
    }

    for (int mt = bx + gdx * zslot; mt < mtiles; mt += gdx * zslots) {
        const int m0 = mt * BMT;
        const int im0 = p.pointwise ? 0 : m0 / (p.cls ? HcWc : HoWo);          // first image of the tile
        const unsigned long off0 = p.pointwise ? (unsigned long)m0 * (unsigned long)(d.seg[0].ld * 2) : (unsigned long)im0 * pimg0;
        const unsigned long off1 = p.pointwise ? (unsigned long)m0 * (unsigned long)(d.seg[1].ld * 2) : (unsigned long)im0 * pimg1;
        const __amdgpu_buffer_rsrc_t rs0 = rebased(d.seg[0].ptr, off0, p.segbytes64[0]);
        const __amdgpu_buffer_rsrc_t rs1 = rebased(d.seg[1].ptr, off1, p.segbytes64[1]);
        int hb[NA], wb[NA], img[NA];          // img: relative to im0
        unsigned voff0[NA], voff1[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int row = (i * NWV + wave) * RPI + lrow;
            const int m = m0 + row;
            voff0[i] = OOB; voff1[i] = OOB;
            img[i] = 0; hb[i] = -(1 << 28); wb[i] = -(1 << 28);
            if (m < p.M) {
                if (p.pointwise) {
                    voff0[i] = (unsigned)row * (unsigned)(d.seg[0].ld * 2) + chA[i];
                    voff1[i] = (unsigned)row * (unsigned)(d.seg[1].ld * 2) + chA[i];
                } else {
                    int im, ho, wo;
                    if (p.cls) {
                        im = m / HcWc;
                        const int rem = m - im * HcWc;
                        const int ii = rem / p.Wc;
                        ho = 2 * ii + ph; wo = 2 * (rem - ii * p.Wc) + pw;
                    } else {
                        im = m / HoWo;
                        const int rem = m - im * HoWo;
                        ho = rem / d.Wo;
                        wo = rem - ho * d.Wo;
                    }
                    img[i] = im - im0; hb[i] = ho * p.sa + p.sc; wb[i] = wo * p.sa + p.sc;
                    if (p.cls && lq == 0) sPix[row] = (im * d.Ho + ho) * d.Wo + wo;
                }
            }
        }

        f32x16_t acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

        int ld_tap = 0, ld_cb = 0, kcol_base = 0;
        auto tap_setup = [&](int tapl) {
            int kh = tapl / nkw;
            int kw = tapl - kh * nkw;
            if (p.cls) { kh = kh0 + 2 * kh; kw = kw0 + 2 * kw; }
            kcol_base = (kh * d.KW + kw) * p.Ctot;
            if (p.pointwise) return;
            const int u0 = d.seg[0].ups, u1 = d.seg[1].ups;
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int hn = hb[i] + kh * p.sb;
                const int wn_ = wb[i] + kw * p.sb;
                bool ok = hn >= 0 && wn_ >= 0 && (((hn | wn_) & sdmask) == 0);
                const int hs = hn >> p.sdshift, ws = wn_ >> p.sdshift;
                ok = ok && hs < d.Hi && ws < d.Wi;
                const unsigned pix0 = (unsigned)((img[i] * (d.Hi >> u0) + (hs >> u0)) * (d.Wi >> u0) + (ws >> u0));
                const unsigned pix1 = (unsigned)((img[i] * (d.Hi >> u1) + (hs >> u1)) * (d.Wi >> u1) + (ws >> u1));
                voff0[i] = ok ? pix0 * (unsigned)(d.seg[0].ld * 2) + chA[i] : OOB;
                voff1[i] = ok ? pix1 * (unsigned)(d.seg[1].ld * 2) + chA[i] : OOB;
            }
        };
        // one stage = NA + NB LDS-DMA instructions of this wave
        auto issue = [&](int slot) {
            if (ld_cb == 0) tap_setup(ld_tap);
            const int c = ld_cb * BKT;
            const bool s1 = d.nseg > 1 && c >= C0;           // wave-uniform
            unsigned char* sa = smem + slot * STAGE_BYTES + wave * (RPI * ROWB);
            if (s1) {
                const int so = (c - C0) * 2;
#pragma unroll
                for (int i = 0; i < NA; ++i)
                    lds_dma16(rs1, sa + i * (NWV * RPI * ROWB), voff1[i], so);
            } else {
                const int so = c * 2;
#pragma unroll
                for (int i = 0; i < NA; ++i)
                    lds_dma16(rs0, sa + i * (NWV * RPI * ROWB), voff0[i], so);
            }
            const int sw = (kcol_base + c) * 2;
            unsigned char* sb = sa + BMT * ROWB;
#pragma unroll
            for (int j = 0; j < NB; ++j)
                lds_dma16(rsw, sb + j * (NWV * RPI * ROWB), voffB[j], sw);
            if (++ld_cb == ncb) { ld_cb = 0; ++ld_tap; }
        };

#pragma unroll
        for (int s = 0; s < STG - 1; ++s)
            if (s < nkt) issue(s);
        int slot = 0, islot = STG - 1, rd_cb = 0;
        for (int kt = 0; kt < nkt; ++kt) {
            // this wave's transfers of stage kt have landed when at most the younger stages are outstanding
            const int younger = nkt - 1 - kt;
            if (STG == 2 || younger == 0) YH_VMCNT(0);
            else if (STG == 3 || younger == 1) YH_VMCNT(LPS);
            else YH_VMCNT(2 * LPS);
            __builtin_amdgcn_s_barrier();          // stage kt complete for every wave; stage kt-1 no longer read by anyone
            // The 8-wave tiles: a wave issues 6-8 transfers per step (~100 cycles of issue each, no MFMA of that wave meanwhile).  Both
            // waves of a SIMD (w and w + 4) doing so right behind the barrier leaves the matrix pipe idle for that long: waves 4-7
            // issue theirs behind their first sub-step — which every channel block has, also a tail block — beside their partners'
            // MFMAs (the slot they fill was freed by the barrier; a wave still issues once per step, in order: the counted waits
            // hold).  Isolated +3...+11 % on both 8-wave tiles (profiles/r06_step_experiments.txt j).
            constexpr bool W8 = NWV == 8;
            const bool more = kt + STG - 1 < nkt;
            if (more && (!W8 || wave < NWV / 2)) issue(islot);
            const unsigned char* sbase = smem + slot * STAGE_BYTES;
            int ksn = BKT / 16;                    // wave-uniform: sub-steps of this channel block
            if (TL) {
                if (rd_cb + 1 == ncb) { ksn = tailn; rd_cb = 0; } else ++rd_cb;
            }
#pragma unroll
            for (int ks = 0; ks < BKT / 16; ++ks) {
                if (TL && ks >= ksn) continue;
                bf16x8_t af[TM], bfr[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    af[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(sbase + rdA0 + i * (32 * ROWB) + koff[ks]));
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    bfr[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(sbase + rdB0 + j * (32 * ROWB) + koff[ks]));
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
                if (W8 && ks == 0 && more && wave >= NWV / 2) issue(islot);
            }
            slot = slot + 1 == STG ? 0 : slot + 1;
            islot = islot + 1 == STG ? 0 : islot + 1;
        }
        __syncthreads();                           // nothing in flight (last wait was vmcnt(0)); ring -> epilogue buffer

        // ---- epilogue (as v2): accumulators -> LDS (bf16, row-major) -> 16-byte global stores
        // EPI 3 reads the producer's raw output z of every output chunk: requested ahead of the accumulator conversion — except on the
        // 256 x 256 tile (16 chunks per thread: 64 registers beside 128 accumulators spill), which loads z where it is used
        constexpr int CPRz = BN / 8;
        constexpr int NCHz = BMT * CPRz / NT;
        constexpr bool ZPRE = NCHz <= 8;
        uint4 zpre[(EPI == 3 && ZPRE) ? NCHz : 1];
        if (EPI == 3 && ZPRE) {
#pragma unroll
            for (int i = 0; i < NCHz; ++i) {
                const int id = t + i * NT;
                const int row = id / CPRz;
                const int m = m0 + row;
                const int n = n0 + (id - row * CPRz) * 8;
                zpre[i] = make_uint4(0, 0, 0, 0);
                if (m < p.M && n < d.N) {
                    const size_t orow = p.cls ? (size_t)sPix[row] : (size_t)m;
                    zpre[i] = *reinterpret_cast<const uint4*>(d.bnr_z + orow * d.bnr_ldz + n);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int c = wn * (TN * 32) + j * 32 + (lane & 31);
            float bs = 0.f, scl = 1.f, sft = 0.f;
            if (EPI == 2) {
                const int n = n0 + c;
                const bool nv = n < d.N;
                bs = (d.bias && nv) ? d.bias[n] : 0.f;
                scl = (d.scale && nv) ? d.scale[n] : 1.f;
                sft = (d.shift && nv) ? d.shift[n] : 0.f;
            }
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                uint16_t* dst = sC + (wm * (TM * 32) + i * 32 + 4 * (lane >> 5)) * CP + c;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc[i][j][r];
                    if (EPI == 2) {
                        v = (v + bs) * scl + sft;
                        if (d.act == YH_ACT_SILU) v = silu_fast(v);
                    }
                    dst[((r & 3) + 8 * (r >> 2)) * CP] = f2bf(v);
                    if (EPI == 1) { s += v; q += v * v; }
                }
            }
            if (EPI == 1) {
                s += __shfl_xor(s, 32, 64);
                q += __shfl_xor(q, 32, 64);
                if (lane < 32) {
                    sStat[(wm * 2 + 0) * BN + c] = s;
                    sStat[(wm * 2 + 1) * BN + c] = q;
                }
            }
        }
        __syncthreads();

        constexpr int CPR = BN / 8;
        constexpr int NCH = BMT * CPR / NT;
        uint4 zq[(EPI == 3 && !ZPRE) ? 4 : 1];       // the 256 x 256 tile: z of the next four chunks, requested together
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            if (EPI == 3 && !ZPRE && (i & 3) == 0) {
                // (the stores of the previous chunks may alias z for all the compiler knows: loads left inside the chunk's own
                // iteration were issued one by one behind them — sixteen dependent round trips per tile)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int id2 = t + (i + g) * NT;
                    const int row2 = id2 / CPR;
                    const int m2 = m0 + row2;
                    const int n2 = n0 + (id2 - row2 * CPR) * 8;
                    zq[g] = make_uint4(0, 0, 0, 0);
                    if (m2 < p.M && n2 < d.N) {
                        const size_t orow2 = p.cls ? (size_t)sPix[row2] : (size_t)m2;
                        zq[g] = *reinterpret_cast<const uint4*>(d.bnr_z + orow2 * d.bnr_ldz + n2);
                    }
                }
            }
            const int id = t + i * NT;
            const int row = id / CPR;
            const int cch = id - row * CPR;
            const int m = m0 + row;
            const int n = n0 + cch * 8;
            if (m < p.M && n < d.N) {
                uint4 v = *reinterpret_cast<const uint4*>(sC + row * CP + cch * 8);
                const size_t orow = p.cls ? (size_t)sPix[row] : (size_t)m;
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
                            float g[8]; unpack8(rv, g);
#pragma unroll
                            for (int e = 0; e < 8; ++e) f[e] += g[e];
                        }
                        if (d.accumulate) {
                            uint4 ov = *reinterpret_cast<const uint4*>(dst);
                            float g[8]; unpack8(ov, g);
#pragma unroll
                            for (int e = 0; e < 8; ++e) f[e] += g[e];
                        }
                        v = pack8(f);
                    }
                    *reinterpret_cast<uint4*>(dst) = v;
                } else {
                    if (EPI == 3 && d.accumulate) {
                        // last writer of a gradient with several contributions: add the earlier ones (bf16, as the generic
                        // epilogue does) and take the BatchNorm-backward sums over the rounded total
                        const uint4 ov = *reinterpret_cast<const uint4*>(d.out0 + orow * d.ld0 + n);
                        float f[8], g0[8];
                        unpack8(v, f);
                        unpack8(ov, g0);
#pragma unroll
                        for (int e = 0; e < 8; ++e) f[e] += g0[e];
                        v = pack8(f);
                    }
                    *reinterpret_cast<uint4*>(d.out0 + orow * d.ld0 + n) = v;
                    if (EPI == 3) {
                        const uint4 zv = ZPRE ? zpre[ZPRE ? i : 0] : zq[ZPRE ? 0 : (i & 3)];
                        float g[8], z[8];
                        unpack8(v, g);
                        unpack8(zv, z);
                        const float4 s0 = *reinterpret_cast<const float4*>(sStat + cch * 8);
                        const float4 s1 = *reinterpret_cast<const float4*>(sStat + cch * 8 + 4);
                        const float4 h0 = *reinterpret_cast<const float4*>(sStat + BN + cch * 8);
                        const float4 h1 = *reinterpret_cast<const float4*>(sStat + BN + cch * 8 + 4);
                        const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                        const float sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const float a = z[e] * sc[e] + sh[e];
                            const float sg = sigmoid_fast(a);
                            const float dz = g[e] * (sg * (1.f + a * (1.f - sg)));
                            bs_[e] += dz; bq_[e] += dz * z[e];
                        }
                    }
                }
            }
        }
        if (EPI == 1 && t < BN) {
#pragma unroll
            for (int w = 0; w < WM; ++w) {
                run_s += sStat[(w * 2 + 0) * BN + t];
                run_q += sStat[(w * 2 + 1) * BN + t];
            }
        }
        __syncthreads();
    }

    if (EPI == 1 && t < BN) {
        put_stat(d, bx, 0, n0 + t, run_s);
        put_stat(d, bx, 1, n0 + t, run_q);
    }
    if (EPI == 3) {
        constexpr int CPR2 = BN / 8;
        float* sRed = reinterpret_cast<float*>(smem);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) { sRed[t * 16 + e] = bs_[e]; sRed[t * 16 + 8 + e] = bq_[e]; }
        __syncthreads();
        const size_t rowi = (size_t)blockIdx.z * gdx + bx;
        for (int i = t; i < 2 * BN; i += NT) {
            const int which = i / BN, c = i - which * BN;
            float v = 0.f;
            for (int j = c / 8; j < NT; j += CPR2) v += sRed[j * 16 + which * 8 + (c & 7)];
            if (n0 + c < d.N) put_bnr(d, rowi, which, n0 + c, v);
        }
    }
}

template <int BMT, int BN, int WM, int BKT, int STG>
constexpr size_t conv3_smem_bytes() {
    size_t a = (size_t)STG * (BMT + BN) * BKT * 2;
    size_t c = (size_t)BMT * (BN + 8) * 2;
    return (a > c ? a : c) + WM * 2 * BN * 4 + BMT * 4;
}

template <int V, int BKT, bool TL> void v3_launch(const ConvPlan& pl, hipStream_t st)
{
    constexpr V3Tile T = V3_TILES[V];
    constexpr int STG = BKT == 64 ? T.stg64 : T.stg32;
    const size_t sm = conv3_smem_bytes<T.bmt, T.bn, T.wm, BKT, STG>();
    static YhDevOnce attr_set;
    yh_lds_limit(attr_set, {{(const void*)conv_v3_kernel<T.bmt, T.bn, T.wm, T.wn, BKT, STG, 0, TL>, (int)sm}, {(const void*)conv_v3_kernel<T.bmt, T.bn, T.wm, T.wn, BKT, STG, 1, TL>, (int)sm},
                            {(const void*)conv_v3_kernel<T.bmt, T.bn, T.wm, T.wn, BKT, STG, 2, TL>, (int)sm}, {(const void*)conv_v3_kernel<T.bmt, T.bn, T.wm, T.wn, BKT, STG, 3, TL>, (int)sm}});
    if (pl.epi == 3)      conv_v3_kernel<T.bmt, T.bn, T.wm, T.wn, BKT, STG, 3, TL><<<pl.grid, pl.block, sm, st>>>(pl.k);
    else if (pl.epi == 2) conv_v3_kernel<T.bmt, T.bn, T.wm, T.wn, BKT, STG, 2, TL><<<pl.grid, pl.block, sm, st>>>(pl.k);
    else if (pl.epi == 1) conv_v3_kernel<T.bmt, T.bn, T.wm, T.wn, BKT, STG, 1, TL><<<pl.grid, pl.block, sm, st>>>(pl.k);
    else                  conv_v3_kernel<T.bmt, T.bn, T.wm, T.wn, BKT, STG, 0, TL><<<pl.grid, pl.block, sm, st>>>(pl.k);
}

}  // namespace

void yh_conv::conv_launch_v3(const ConvPlan& pl, hipStream_t st)
{
#define YH_V3_STEPS(V_) (pl.tl ? v3_launch<V_, 64, true>(pl, st) : (pl.bkt == 64 ? v3_launch<V_, 64, false>(pl, st) : v3_launch<V_, 32, false>(pl, st)))
    if (pl.v3 == 4) v3_launch<4, 64, false>(pl, st); else if (pl.v3 == 1) YH_V3_STEPS(1); else if (pl.v3 == 2) YH_V3_STEPS(2); else YH_V3_STEPS(3);
#undef YH_V3_STEPS
}
