// Register-staged buffer-load kernel of the implicit-GEMM convolution (conv_igemm.hip plans it: FAM_V2).
// v2: the tiling of conv_igemm_kernel (conv_generic.hip), written for a minimal instruction count per k-tile.  Operands are fetched with raw
// buffer loads: the per-lane byte offset of a tile row is computed once per TAP (not per k-tile), padding taps
// and rows past M simply carry an out-of-range offset (the hardware range check returns zeros, no branches),
// and the walk along the channels / along K is a SCALAR offset.  Eligible when every segment has a multiple
// of 32 channels and every operand is smaller than 2 GiB (host check).
#include "conv_igemm.h"

using namespace yh_conv;

namespace {

typedef unsigned int u32x4_nt __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld_nt16(const uint16_t* p) {
    u32x4_nt v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_nt*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_nt16(uint16_t* p, uint4 v) {
    u32x4_nt w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<u32x4_nt*>(p));
}

#ifdef YH_CONV_STAMPS
// timing build only (make stamps): per-phase s_memtime totals of block 0's four waves
__device__ long long g_stamps[32];
#endif

template <int BN, int WM, int WN, int MINW, int EPI, int BKT>     // block = WM x WN waves   // BKT: channels per k-step (32 | 64); EPI 0: plain store, 1: + BatchNorm partial sums, 2: generic epilogue
__global__ __launch_bounds__(WM * WN * 64, MINW) void conv_v2_kernel(const ConvK p)
{
    constexpr int NT = WM * WN * 64;                // threads per block
    constexpr int TM = BM / (WM * 32);
    constexpr int TN = BN / (WN * 32);
    constexpr int LDSPX = BKT + 8;                  // LDS row pitch in elements: 80 B / 144 B rows, conflict-free ds_read_b128
    constexpr int CHR = BKT / 8;                    // 16-byte chunks per tile row
    constexpr int RPP = NT / CHR;                   // tile rows covered by one pass of the block's threads
    constexpr int NA = BM / RPP;                    // A chunks per thread
    constexpr int NBL = (BN * CHR + NT - 1) / NT;   // B chunks per thread
    constexpr int CP = BN + 8;
    constexpr int MAIN_BYTES = (2 * (BM + BN) * LDSPX * 2) > (BM * CP * 2) ? (2 * (BM + BN) * LDSPX * 2) : (BM * CP * 2);
    constexpr unsigned OOB = 0x80000000u;

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* sA = reinterpret_cast<uint16_t*>(smem);
    uint16_t* sB = sA + 2 * BM * LDSPX;
    uint16_t* sC = reinterpret_cast<uint16_t*>(smem);
    float* sStat = reinterpret_cast<float*>(smem + MAIN_BYTES);
    int* sPix = reinterpret_cast<int*>(smem + MAIN_BYTES + WM * 2 * BN * 4);

    const yh_conv_desc& d = p.d;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    const int wm = wave / WN;
    const int wn = wave % WN;
    const int kc = t % CHR;
    const int rowA = t / CHR;
    const int n0 = blockIdx.y * BN;
    const int HoWo = d.Ho * d.Wo;
    const int sdmask = (1 << p.sdshift) - 1;
    // channel blocks are walked per segment: a segment's ragged last block (channel count not a multiple of the k-step) is masked
    // to zero on the activation side, and the next segment starts a block of its own at its first channel (80 + 80: 3 + 3 blocks)
    const int C0 = d.seg[0].C;
    const int ncb0 = d.nseg > 1 ? (C0 + BKT - 1) / BKT : 0;
    const int ncb = d.nseg > 1 ? ncb0 + (p.Ctot - C0 + BKT - 1) / BKT : (p.Ctot + BKT - 1) / BKT;
    const int HcWc = p.Hc * p.Wc;

    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)d.seg[0].ptr, 0, p.segbytes[0], 0x00020000);
    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc((void*)(d.nseg > 1 ? d.seg[1].ptr : d.seg[0].ptr), 0,
                                                                          d.nseg > 1 ? p.segbytes[1] : p.segbytes[0], 0x00020000);
    const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc((void*)d.w, 0, p.wbytes, 0x00020000);

    // per-thread constants: weight row offsets, LDS addresses
    unsigned voffB[NBL];
#pragma unroll
    for (int j = 0; j < NBL; ++j) {
        const int id = t + j * NT;
        voffB[j] = id < BN * CHR ? (unsigned)(((n0 + id / CHR) * p.Ktot + kc * 8) * 2) : OOB;
    }
    const int ldsA0 = rowA * LDSPX + kc * 8;         // + RPP*LDSPX per further row of this thread
    const int ldsB0 = rowA * LDSPX + kc * 8;         // row (t + j*NT)/CHR == rowA + j*RPP

    float run_s = 0.f, run_q = 0.f;
    // EPI 3 (data gradient that is the ONLY writer of a ConvBnAct output's gradient): the BatchNorm+SiLU backward
    // reduction of that producer is taken here, from the tile that is being stored anyway: dz = g * silu'(bn(z)),
    // partial sums of dz and dz*z per channel.  A thread always handles the same 8-channel chunk (NT % (BN/8) == 0).
    float bs_[8], bq_[8];
    if (EPI == 3) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { bs_[e] = 0.f; bq_[e] = 0.f; }
        for (int i = t; i < 2 * BN; i += NT) {          // scale | shift of the block's channels -> LDS (sStat is free in this mode)
            const int which = i / BN, c = i - which * BN;
            sStat[i] = (n0 + c < d.N) ? d.bnr_ws[(size_t)which * d.bnr_C + n0 + c] : 0.f;
        }
        __syncthreads();
    }
#ifdef YH_CONV_STAMPS
    long long st_load = 0, st_mma = 0, st_store = 0, st_bar = 0, st_pro = 0, st_epi = 0, st_n = 0;
    const long long st_begin = __builtin_amdgcn_s_memtime();
#define STAMP(var) do { const long long now_ = __builtin_amdgcn_s_memtime(); var += now_ - st_t; st_t = now_; } while (0)
#else
#define STAMP(var) do { } while (0)
#endif

    // Stride-2 data gradient: a block takes the four parity classes of a pixel region one after the other (1, 2, 2 and 4 taps for
    // a 3x3 kernel), so the gy rows the classes share come out of its XCD's L2 after the first fetch and the two 64-byte halves
    // of the 128-byte lines that neighbouring classes write (a class owns every other pixel) meet in L2 before they are evicted.
    // Layers with fewer regions than CUs keep the classes in blockIdx.z instead ((class, slot) pairs, see cls_slot): more blocks.
    const bool zcls = p.cls && gridDim.z > 1;
    int zph = 0, zpw = 0, zslot = 0, zslots = 1;
    if (zcls) cls_slot(d, blockIdx.z, zph, zpw, zslot, zslots);
    const int csh = (p.cls && !zcls) ? 2 : 0;
    // With a multiple of 32 blocks the four classes of a region go to four blocks of ONE XCD at the same time instead (blocks b,
    // b+8, b+16, b+24 form a group; the class rotates per step so that every block carries the same work): the shared gy rows are
    // still in that XCD's L2 when the other three classes ask for them (a lone block comes back to them after ~8 MB of other
    // blocks' traffic: PMC showed gy fetched 4.6 times).  +3 / +7 / +21 % on the YOLOv5s stage-1 / 2 / 3 layers.
    const bool grp = p.cls && !zcls && (gridDim.x % 32 == 0);
    const int g_q = (blockIdx.x >> 3) & 3;
    const int g_idx = (blockIdx.x & 7) + 8 * (blockIdx.x >> 5);
    const int g_n = gridDim.x >> 2;
    for (int it = 0;; ++it) {
        const int mt = grp ? g_idx + g_n * it : blockIdx.x + gridDim.x * (zcls ? zslot + zslots * it : (it >> csh));
        if (mt >= p.mtiles) break;
#ifdef YH_CONV_STAMPS
        long long st_t = __builtin_amdgcn_s_memtime();
#endif
        const int gc = (g_q + it) & 3;
        const int ph = zcls ? zph : (p.cls ? ((grp ? gc >> 1 : it >> 1) & 1) : 0), pw = zcls ? zpw : (p.cls ? ((grp ? gc : it) & 1) : 0);
        const int kh0 = (ph + d.pad) & 1, kw0 = (pw + d.pad) & 1;
        const int nkw = p.cls ? (d.KW - kw0 + 1) / 2 : d.KW;
        const int nkh = p.cls ? (d.KH - kh0 + 1) / 2 : d.KH;
        const int nkt = nkh * nkw * ncb;
        const int m0 = mt * BM;
        int hb[NA], wb[NA], img[NA];
        unsigned voff0[NA], voff1[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int m = m0 + rowA + RPP * i;
            voff0[i] = OOB; voff1[i] = OOB;
            img[i] = 0; hb[i] = -(1 << 28); wb[i] = -(1 << 28);
            if (m < p.M) {
                if (p.pointwise) {
                    voff0[i] = (unsigned)m * (unsigned)(d.seg[0].ld * 2) + kc * 16;
                    voff1[i] = (unsigned)m * (unsigned)(d.seg[1].ld * 2) + kc * 16;
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
                    img[i] = im; hb[i] = ho * p.sa + p.sc; wb[i] = wo * p.sa + p.sc;
                    if (p.cls && kc == 0) sPix[rowA + RPP * i] = (im * d.Ho + ho) * d.Wo + wo;
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

        u32x4_t ra[NA], rb[NBL];
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
                voff0[i] = ok ? pix0 * (unsigned)(d.seg[0].ld * 2) + kc * 16 : OOB;
                voff1[i] = ok ? pix1 * (unsigned)(d.seg[1].ld * 2) + kc * 16 : OOB;
            }
        };
        auto load_tile = [&]() {
            if (ld_cb == 0) tap_setup(ld_tap);
            const bool s1 = d.nseg > 1 && ld_cb >= ncb0;     // wave-uniform
            const int c = s1 ? C0 + (ld_cb - ncb0) * BKT : ld_cb * BKT;      // channel of the concatenated input the block starts at
            // channels of this thread's chunk that lie past the segment (last block of a channel count that is not a
            // multiple of the k-step) read as zero; the weight columns they meet are finite, so they add nothing
            const bool cok = c + kc * 8 < (s1 || d.nseg == 1 ? p.Ctot : C0);
#if YH_CONV_ABLATE
            if (YH_CONV_ABLATE & 1) {
#pragma unroll
                for (int i = 0; i < NA; ++i) ra[i] = u32x4_t{0, 0, 0, 0};
            } else
#endif
            if (s1) {
                const int so = (c - C0) * 2;
#pragma unroll
                for (int i = 0; i < NA; ++i) ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rs1, cok ? voff1[i] : OOB, so, 0);
            } else {
                const int so = c * 2;
#pragma unroll
                for (int i = 0; i < NA; ++i) ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rs0, cok ? voff0[i] : OOB, so, 0);
            }
            const int sw = (kcol_base + c) * 2;
#if YH_CONV_ABLATE
            if (YH_CONV_ABLATE & 8) {
#pragma unroll
                for (int j = 0; j < NBL; ++j) rb[j] = u32x4_t{0, 0, 0, 0};
            } else
#endif
#pragma unroll
            for (int j = 0; j < NBL; ++j) rb[j] = __builtin_amdgcn_raw_buffer_load_b128(rsw, voffB[j], sw, 0);
            if (++ld_cb == ncb) { ld_cb = 0; ++ld_tap; }
        };
        auto store_tile = [&](int buf) {
            uint16_t* a = sA + buf * BM * LDSPX + ldsA0;
            uint16_t* b = sB + buf * BN * LDSPX + ldsB0;
#pragma unroll
            for (int i = 0; i < NA; ++i) *reinterpret_cast<u32x4_t*>(a + i * RPP * LDSPX) = ra[i];
#pragma unroll
            for (int j = 0; j < NBL; ++j)
                if (t + j * NT < BN * CHR) *reinterpret_cast<u32x4_t*>(b + j * RPP * LDSPX) = rb[j];
        };

        load_tile();
        store_tile(0);
        __syncthreads();
        STAMP(st_pro);
        for (int kt = 0; kt < nkt; ++kt) {
            const int buf = kt & 1;
            const bool more = (kt + 1) < nkt;
            if (more) load_tile();
            STAMP(st_load);
            const uint16_t* a = sA + buf * BM * LDSPX;
            const uint16_t* b = sB + buf * BN * LDSPX;
#pragma unroll
            for (int ks = 0; ks < BKT / 16; ++ks) {
                bf16x8_t af[TM], bfr[TN];
                const int koff = (ks * 2 + (lane >> 5)) * 8;
#if YH_CONV_ABLATE
                if (YH_CONV_ABLATE & 64) {
#pragma unroll
                    for (int i = 0; i < TM; ++i) af[i] = __builtin_bit_cast(bf16x8_t, ra[0]);
#pragma unroll
                    for (int j = 0; j < TN; ++j) bfr[j] = __builtin_bit_cast(bf16x8_t, rb[0]);
                } else {
#endif
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    af[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(a + (wm * (TM * 32) + i * 32 + (lane & 31)) * LDSPX + koff));
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    bfr[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(b + (wn * (TN * 32) + j * 32 + (lane & 31)) * LDSPX + koff));
#if YH_CONV_ABLATE
                }
#endif
#if YH_CONV_ABLATE
                if (YH_CONV_ABLATE & 4) {
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) acc[i][j][0] += (float)af[i][0] * (float)bfr[j][0];
                } else
#endif
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            }
            STAMP(st_mma);
#if YH_CONV_ABLATE
            if (more && !(YH_CONV_ABLATE & 128)) store_tile(buf ^ 1);
            STAMP(st_store);
            if (!(YH_CONV_ABLATE & 256)) __syncthreads();
#else
            if (more) store_tile(buf ^ 1);
            STAMP(st_store);
            __syncthreads();
#endif
            STAMP(st_bar);
#ifdef YH_CONV_STAMPS
            ++st_n;
#endif
        }

        // ---- epilogue
#if YH_CONV_ABLATE
        if (YH_CONV_ABLATE & 2) {
            float sink = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sink += acc[i][j][r];
            if (sink == 12345.678f) d.out0[0] = 1;
            continue;
        }
#endif
        // EPI 3: the producer's z chunks this thread will need in the read-out are requested now, so that their latency
        // hides behind the accumulator -> LDS transposition and its barrier
        constexpr int CPRz = BN / 8;
        constexpr int NCHz = BM * CPRz / NT;
        uint4 zpre[EPI == 3 ? NCHz : 1];
        if (EPI == 3) {
#pragma unroll
            for (int i = 0; i < NCHz; ++i) {
                const int id = t + i * NT;
                const int row = id / CPRz;
                const int m = m0 + row;
                const int n = n0 + (id - row * CPRz) * 8;
                zpre[i] = make_uint4(0, 0, 0, 0);
                if (m < p.M && n < d.N) {
                    const size_t orow = p.cls ? (size_t)sPix[row] : (size_t)m;
                    zpre[i] = ld_nt16(d.bnr_z + orow * d.bnr_ldz + n);          // last reader of z
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
                    if (EPI == 1) { s += v; q += v * v; }      // rows past M and padded channels are exact zeros
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
        constexpr int NCH = BM * CPR / NT;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
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
                    // EPI 3 streams its output (non-temporal): the gradient is read next by a whole-tensor pass, and the stride-2
                    // classes write 64-byte halves of lines — kept in L2 they cost a line fill each and push out the gy rows the
                    // classes share (PMC on the YOLOv5s stage-1 layer: 1.99 -> 1.39 GB fetched; +1.5 % on the train step)
                    if (EPI == 3) st_nt16(d.out0 + orow * d.ld0 + n, v);
                    else *reinterpret_cast<uint4*>(d.out0 + orow * d.ld0 + n) = v;
                    if (EPI == 3) {
                        const uint4 zv = zpre[i];
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
        STAMP(st_epi);
    }
#ifdef YH_CONV_STAMPS
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && lane == 0) {
        long long* o = g_stamps + wave * 8;
        o[0] = st_load; o[1] = st_mma; o[2] = st_store; o[3] = st_bar; o[4] = st_pro; o[5] = st_epi; o[6] = st_n;
        o[7] = __builtin_amdgcn_s_memtime() - st_begin;
    }
#endif
#undef STAMP

    if (EPI == 1 && t < BN) {
        put_stat(d, blockIdx.x, 0, n0 + t, run_s);
        put_stat(d, blockIdx.x, 1, n0 + t, run_q);
    }
    if (EPI == 3) {
        constexpr int CPR2 = BN / 8;
        float* sRed = reinterpret_cast<float*>(smem);          // [NT][16], aliases the (now idle) tile buffers
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) { sRed[t * 16 + e] = bs_[e]; sRed[t * 16 + 8 + e] = bq_[e]; }
        __syncthreads();
        const size_t rowi = (size_t)blockIdx.z * gridDim.x + blockIdx.x;
        for (int i = t; i < 2 * BN; i += NT) {
            const int which = i / BN, c = i - which * BN;
            float v = 0.f;
            for (int j = c / 8; j < NT; j += CPR2) v += sRed[j * 16 + which * 8 + (c & 7)];
            if (n0 + c < d.N) put_bnr(d, rowi, which, n0 + c, v);
        }
    }
}

template <int BN, int BKT> void v2_launch(const ConvPlan& pl, hipStream_t st)
{
    constexpr ConvTile T = conv_tile(BN);
    const size_t sm = conv_smem_bytes<BN, T.wm2, T.wn2, BKT>();
    if (pl.epi == 3)      conv_v2_kernel<BN, T.wm2, T.wn2, T.minw2, 3, BKT><<<pl.grid, pl.block, sm, st>>>(pl.k);
    else if (pl.epi == 2) conv_v2_kernel<BN, T.wm2, T.wn2, T.minw2, 2, BKT><<<pl.grid, pl.block, sm, st>>>(pl.k);
    else if (pl.epi == 1) conv_v2_kernel<BN, T.wm2, T.wn2, T.minw2, 1, BKT><<<pl.grid, pl.block, sm, st>>>(pl.k);
    else                  conv_v2_kernel<BN, T.wm2, T.wn2, T.minw2, 0, BKT><<<pl.grid, pl.block, sm, st>>>(pl.k);
}

}  // namespace

void yh_conv::conv_launch_v2(const ConvPlan& pl, hipStream_t st)
{
    if (pl.bn == 128) { if (pl.bkt == 64) v2_launch<128, 64>(pl, st); else v2_launch<128, 32>(pl, st); }
    else if (pl.bn == 64) v2_launch<64, 32>(pl, st);
    else v2_launch<32, 32>(pl, st);
}

#ifdef YH_CONV_STAMPS
extern "C" int yh_debug_read_stamps(long long* host_out32)
{
    return hipMemcpyFromSymbol(host_out32, HIP_SYMBOL(g_stamps), sizeof(long long) * 32) == hipSuccess ? 0 : -1;
}
#endif
