// Generic kernel of the implicit-GEMM convolution (conv_igemm.hip plans it: FAM_GENERIC): any channel count, any epilogue.
//
// Tile: BM=128 pixels x BN in {32,64,128} channels x BK=32, 256 threads = 4 waves.
// A/B tiles are register-staged (global_load_dwordx4 -> ds_write_b128) so that padding
// taps can be zero-filled; LDS rows are padded to 80 B which makes the ds_read_b128
// fragment reads conflict-free.  Double-buffered LDS, next tile's global loads are
// issued before the MFMAs of the current one.  The epilogue transposes through LDS
// so every global store is a 16-byte row chunk, and optionally emits per-channel
// sum / sum-of-squares partials (training-mode BatchNorm statistics) per block.
#include "conv_igemm.h"

using namespace yh_conv;

namespace {

constexpr int LDSP = 40;   // bf16 elements per LDS row (32 + 8 pad = 80 bytes)

template <int BN, int WM, int WN, bool FAST, int MINW>
__global__ __launch_bounds__(256, MINW) void conv_igemm_kernel(const ConvK p)
{
    constexpr int TM = BM / (WM * 32);
    constexpr int TN = BN / (WN * 32);
    constexpr int NBL = (BN * 4 + 255) / 256;       // B chunks per thread
    constexpr int CP = BN + 8;                      // sC row pitch (elements)
    constexpr int MAIN_BYTES = (2 * (BM + BN) * LDSP * 2) > (BM * CP * 2) ? (2 * (BM + BN) * LDSP * 2) : (BM * CP * 2);

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint16_t* sA = reinterpret_cast<uint16_t*>(smem);            // [2][BM][LDSP]
    uint16_t* sB = sA + 2 * BM * LDSP;                            // [2][BN][LDSP]
    uint16_t* sC = reinterpret_cast<uint16_t*>(smem);            // [BM][CP] (aliases sA/sB)
    float* sStat = reinterpret_cast<float*>(smem + MAIN_BYTES);  // [WM][2][BN]
    int* sPix = reinterpret_cast<int*>(smem + MAIN_BYTES + WM * 2 * BN * 4);   // [BM] output pixel of each tile row (cls mode)

    const yh_conv_desc& d = p.d;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    const int wm = wave / WN;
    const int wn = wave % WN;
    const int kc = t & 3;
    const int rowA = t >> 2;
    const int n0 = blockIdx.y * BN;
    const int HoWo = d.Ho * d.Wo;
    const int sdmask = (1 << p.sdshift) - 1;
    // parity class of this block (cls mode): output pixels (2i+ph, 2j+pw); taps kh = kh0 + 2a, kw = kw0 + 2b
    int ph = 0, pw = 0, zslot = 0, zslots = 1;
    if (p.cls) cls_slot(d, blockIdx.z, ph, pw, zslot, zslots);
    const int kh0 = (ph + d.pad) & 1, kw0 = (pw + d.pad) & 1;
    const int nkw = p.cls ? (d.KW - kw0 + 1) / 2 : d.KW;
    const int nkh = p.cls ? (d.KH - kh0 + 1) / 2 : d.KH;
    const int Keff = nkh * nkw * p.Ctot;
    const int nkt = p.cls ? (Keff + BK - 1) / BK : p.nkt;
    const int HcWc = p.Hc * p.Wc;

    float run_s = 0.f, run_q = 0.f;

    for (int mt = blockIdx.x + gridDim.x * zslot; mt < p.mtiles; mt += gridDim.x * zslots) {
        const int m0 = mt * BM;
        int hb[2], wb[2], img[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int m = m0 + rowA + 64 * i;
            if (m < p.M) {
                int im, ho, wo;
                if (p.cls) {
                    im = m / HcWc;
                    int rem = m - im * HcWc;
                    int ii = rem / p.Wc;
                    ho = 2 * ii + ph; wo = 2 * (rem - ii * p.Wc) + pw;
                } else {
                    im = m / HoWo;
                    int rem = m - im * HoWo;
                    ho = rem / d.Wo;
                    wo = rem - ho * d.Wo;
                }
                img[i] = im; hb[i] = ho * p.sa + p.sc; wb[i] = wo * p.sa + p.sc;
                if (p.cls && kc == 0) sPix[rowA + 64 * i] = (im * d.Ho + ho) * d.Wo + wo;
            } else {
                img[i] = 0; hb[i] = -(1 << 28); wb[i] = -(1 << 28);
            }
        }

        f32x16_t acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

        uint4 ra[2], rb[NBL];

        // ---- loader state: k-tiles are walked tap-major.  On the fast path (every segment a multiple of 32
        // channels) a k-tile never straddles a tap or a segment, so the per-row pixel offsets and validity are
        // recomputed only when the tap changes and a k-tile costs a pointer increment.
        int ld_tap = 0, ld_cb = 0;
        int pix0[2] = {0, 0}, pix1[2] = {0, 0};
        bool okr[2] = {false, false};
        int kcol_base = 0;
        const int ncb = p.Ctot >> 5;
        auto tap_setup = [&](int tapl) {
            int kh = tapl / nkw;
            int kw = tapl - kh * nkw;
            if (p.cls) { kh = kh0 + 2 * kh; kw = kw0 + 2 * kw; }
            kcol_base = (kh * d.KW + kw) * p.Ctot;
            const int u0 = d.seg[0].ups, u1 = d.seg[1].ups;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int hn = hb[i] + kh * p.sb;
                const int wn_ = wb[i] + kw * p.sb;
                bool ok = hn >= 0 && wn_ >= 0 && (((hn | wn_) & sdmask) == 0);
                const int hs = hn >> p.sdshift, ws = wn_ >> p.sdshift;
                ok = ok && hs < d.Hi && ws < d.Wi;
                okr[i] = ok;
                pix0[i] = (img[i] * (d.Hi >> u0) + (hs >> u0)) * (d.Wi >> u0) + (ws >> u0);
                pix1[i] = (img[i] * (d.Hi >> u1) + (hs >> u1)) * (d.Wi >> u1) + (ws >> u1);
            }
        };
        auto load_fast = [&]() {
            if (ld_cb == 0) tap_setup(ld_tap);
            const int c = ld_cb * 32 + kc * 8;
            const bool s1 = d.nseg > 1 && c >= d.seg[0].C;
            const uint16_t* sp = s1 ? d.seg[1].ptr : d.seg[0].ptr;
            const int sld = s1 ? d.seg[1].ld : d.seg[0].ld;
            const int cc = s1 ? c - d.seg[0].C : c;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                uint4 v = make_uint4(0, 0, 0, 0);
                if (okr[i] && !(YH_CONV_ABLATE & 1)) v = *reinterpret_cast<const uint4*>(sp + (size_t)(s1 ? pix1[i] : pix0[i]) * sld + cc);
                ra[i] = v;
            }
            const uint16_t* wp = d.w + (size_t)n0 * p.Ktot + kcol_base + c;
#pragma unroll
            for (int i = 0; i < NBL; ++i) {
                const int id = t + i * 256;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (id < BN * 4 && !(YH_CONV_ABLATE & 8)) v = *reinterpret_cast<const uint4*>(wp + (size_t)(id >> 2) * p.Ktot);
                rb[i] = v;
            }
            if (++ld_cb == ncb) { ld_cb = 0; ++ld_tap; }
        };
        auto load_generic = [&](int kt) {
            const int k = kt * BK + kc * 8;
            const bool kvalid = k < Keff;
            int tap = 0, c = 0;
            if (kvalid) { tap = k / p.Ctot; c = k - tap * p.Ctot; }
            int kh = tap / nkw;
            int kw = tap - kh * nkw;
            if (p.cls) { kh = kh0 + 2 * kh; kw = kw0 + 2 * kw; }
            const int kcol = (kh * d.KW + kw) * p.Ctot + c;      // column in the packed weight rows
            const int sidx = (d.nseg > 1 && c >= d.seg[0].C) ? 1 : 0;
            const yh_seg& sg = d.seg[sidx];
            const int cc = c - (sidx ? d.seg[0].C : 0);
            const int ups = sg.ups;
            const int Hs = d.Hi >> ups, Ws = d.Wi >> ups;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int hn = hb[i] + kh * p.sb;
                int wn_ = wb[i] + kw * p.sb;
                bool ok = kvalid && hn >= 0 && wn_ >= 0 && (((hn | wn_) & sdmask) == 0);
                int hs = hn >> p.sdshift, ws = wn_ >> p.sdshift;
                ok = ok && hs < d.Hi && ws < d.Wi;
                hs >>= ups; ws >>= ups;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (ok) {
                    size_t pix = ((size_t)img[i] * Hs + hs) * Ws + ws;
                    v = *reinterpret_cast<const uint4*>(sg.ptr + pix * sg.ld + cc);
                }
                ra[i] = v;
            }
#pragma unroll
            for (int i = 0; i < NBL; ++i) {
                int id = t + i * 256;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (id < BN * 4 && kvalid) {
                    int n = id >> 2;
                    v = *reinterpret_cast<const uint4*>(d.w + (size_t)(n0 + n) * p.Ktot + kcol);
                }
                rb[i] = v;
            }
        };
        auto load_tile = [&](int kt) {
            if constexpr (FAST) load_fast(); else load_generic(kt);
        };
        auto store_tile = [&](int buf) {
            uint16_t* a = sA + buf * BM * LDSP;
            uint16_t* b = sB + buf * BN * LDSP;
#pragma unroll
            for (int i = 0; i < 2; ++i)
                *reinterpret_cast<uint4*>(a + (rowA + 64 * i) * LDSP + kc * 8) = ra[i];
#pragma unroll
            for (int i = 0; i < NBL; ++i) {
                int id = t + i * 256;
                if (id < BN * 4) *reinterpret_cast<uint4*>(b + (id >> 2) * LDSP + kc * 8) = rb[i];
            }
        };

        load_tile(0);
        store_tile(0);
        __syncthreads();

        for (int kt = 0; kt < nkt; ++kt) {
            const int buf = kt & 1;
            const bool more = (kt + 1) < nkt;
            if (more) load_tile(kt + 1);
            const uint16_t* a = sA + buf * BM * LDSP;
            const uint16_t* b = sB + buf * BN * LDSP;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8_t af[TM], bfr[TN];
                const int koff = (ks * 2 + (lane >> 5)) * 8;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    int r = wm * (TM * 32) + i * 32 + (lane & 31);
                    uint4 v = *reinterpret_cast<const uint4*>(a + r * LDSP + koff);
                    af[i] = __builtin_bit_cast(bf16x8_t, v);
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    int r = wn * (TN * 32) + j * 32 + (lane & 31);
                    uint4 v = *reinterpret_cast<const uint4*>(b + r * LDSP + koff);
                    bfr[j] = __builtin_bit_cast(bf16x8_t, v);
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        if (!(YH_CONV_ABLATE & 4)) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            }
            if (more) store_tile(buf ^ 1);
            __syncthreads();
        }

        // ---- epilogue: registers -> LDS (bf16, transposed to row-major) ----
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int c = wn * (TN * 32) + j * 32 + (lane & 31);
            const int n = n0 + c;
            const bool nv = n < d.N;
            const float bs = (d.bias && nv) ? d.bias[n] : 0.f;
            const float scl = (d.scale && nv) ? d.scale[n] : 1.f;
            const float sft = (d.shift && nv) ? d.shift[n] : 0.f;
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    int row = wm * (TM * 32) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    float v = acc[i][j][r] + bs;
                    v = v * scl + sft;
                    if (d.act == YH_ACT_SILU) v = silu_fast(v);
                    uint16_t hb16 = f2bf(v);
                    if (!(YH_CONV_ABLATE & 2)) sC[row * CP + c] = hb16;
                    float vr = (m0 + row < p.M) ? bf2f(hb16) : 0.f;   // rows past M carry only the bias
                    s += vr; q += vr * vr;
                }
            }
            if (d.stats) {
                s += __shfl_xor(s, 32, 64);
                q += __shfl_xor(q, 32, 64);
                if (lane < 32) {
                    sStat[(wm * 2 + 0) * BN + c] = s;
                    sStat[(wm * 2 + 1) * BN + c] = q;
                }
            }
        }
        __syncthreads();

        constexpr int CPR = BN / 8;                 // chunks per row
        constexpr int NCH = BM * CPR / 256;         // chunks per thread
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            int id = t + i * 256;
            int row = id / CPR;
            int cch = id - row * CPR;
            int m = m0 + row;
            int n = n0 + cch * 8;
            if (m < p.M && n < d.N) {
                uint4 v = *reinterpret_cast<const uint4*>(sC + row * CP + cch * 8);
                uint16_t* dst;
                bool first = n < d.nsplit;
                const size_t orow = p.cls ? (size_t)sPix[row] : (size_t)m;
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
            }
        }
        if (d.stats && t < BN) {
#pragma unroll
            for (int w = 0; w < WM; ++w) {
                run_s += sStat[(w * 2 + 0) * BN + t];
                run_q += sStat[(w * 2 + 1) * BN + t];
            }
        }
        __syncthreads();
    }

    if (d.stats && t < BN) {
        put_stat(d, blockIdx.x, 0, n0 + t, run_s);
        put_stat(d, blockIdx.x, 1, n0 + t, run_q);
    }
}

template <int BN> void generic_launch(const ConvPlan& pl, hipStream_t st)
{
    constexpr ConvTile T = conv_tile(BN);
    const size_t sm = conv_smem_bytes<BN, T.wm, T.wn>();
    if (pl.k.fast) conv_igemm_kernel<BN, T.wm, T.wn, true, T.minw><<<pl.grid, pl.block, sm, st>>>(pl.k);
    else           conv_igemm_kernel<BN, T.wm, T.wn, false, T.minw><<<pl.grid, pl.block, sm, st>>>(pl.k);
}

}  // namespace

void yh_conv::conv_launch_generic(const ConvPlan& pl, hipStream_t st)
{
    if (pl.bn == 32) generic_launch<32>(pl, st); else if (pl.bn == 64) generic_launch<64>(pl, st); else generic_launch<128>(pl, st);
}

// diagnostics: resident blocks per CU the runtime predicts for each instantiation (bn = 32/64/128)
template <int BN> static hipError_t conv_generic_occupancy(int* nb)
{
    constexpr ConvTile T = conv_tile(BN);
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(nb, conv_igemm_kernel<BN, T.wm, T.wn, true, T.minw>, 256, conv_smem_bytes<BN, T.wm, T.wn>());
}
extern "C" int yh_debug_conv_occupancy(int bn)
{
    int nb = -1;
    const hipError_t e = bn == 32 ? conv_generic_occupancy<32>(&nb) : (bn == 64 ? conv_generic_occupancy<64>(&nb) : conv_generic_occupancy<128>(&nb));
    return e == hipSuccess ? nb : -(int)e;
}
