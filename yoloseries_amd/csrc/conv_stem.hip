// Stem kernel of the implicit-GEMM convolution (conv_igemm.hip plans it: FAM_STEM, eligibility in stem_eligible).
// Stem ("focus") kernel: 3x3 / stride 1 / pad 1 on the 16-channel space-to-depth image, 32 output channels
// (utils/layer_tools.py:82-94 applied to models/normal/yolov5s.py's 6x6/s2 stem).  K per tap is exactly one
// v_mfma_f32_32x32x16_bf16, the whole weight matrix (9 fragments) lives in registers, and a WAVE works alone on strips
// of 32 consecutive output pixels of one image row: 9 coalesced 1-KB loads (one per tap, fragments straight from
// global memory in MFMA layout, hardware zero fill at the borders), 9 MFMAs, no LDS staging, no barriers.
// The MFMA runs with swapped operands (D = W x X^T): a lane then holds 4 consecutive CHANNELS of one pixel per
// accumulator group, lanes l and l+32 exchange halves with v_permlane32_swap into 16-byte chunks, and the strip leaves
// through a wave-private LDS strip in memory order (1 KiB of consecutive chunks per store instruction).  BatchNorm statistics are per-lane running sums over all strips of the wave, reduced once at the end.
// The layer moves 630 MB for 0.6 GFLOP/MB: it is HBM bound.
// (STEM_BAND: conv_igemm.h)
#include "conv_igemm.h"

using namespace yh_conv;

namespace {

struct StemTag {};

// NTL = output-channel tiles of 32 (v5s 32 -> 1; v5m 48 / v5l 64 -> 2; v5x 80 -> 3, inference only: the running sums of
// three tiles do not fit the register file): the nine fragments of every tile stay in registers, a strip's nine input
// fragments are loaded once and multiplied with each tile in turn.
template <int EPI, int NTL>    // 0 plain, 1 + BatchNorm partial sums, 2 folded BN (scale, shift) + SiLU
__global__ __launch_bounds__(256, NTL == 3 ? 1 : 2) void conv_stem_kernel(const ConvK p)
{
    constexpr unsigned OOB = 0x80000000u;
    static_assert(EPI != 1 || NTL <= 2, "statistics: at most two channel tiles");
    __shared__ float sRed[EPI == 1 ? 4 : 1][2][32 * NTL];
    __shared__ __attribute__((aligned(16))) float sConst[2][32 * NTL];           // EPI 2: scale | shift
    // the two-tile training form (64 channels: whole 128-byte rows, 254 registers) keeps its direct stores: staged it spills and gains nothing
    constexpr bool STAGED = !(EPI == 1 && NTL == 2);
    constexpr int STEM_SP = 32 * NTL + 8;                                        // pitch (elements) of a staged output row
    __shared__ __attribute__((aligned(16))) uint16_t sOut[STAGED ? 4 * 32 * STEM_SP : 8];      // [wave][32 pixels][STEM_SP]
    const yh_conv_desc& d = p.d;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int W = d.Wo, H = d.Ho;
    const int ldx = d.seg[0].ld * 2;                  // bytes per input pixel
    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc((void*)d.seg[0].ptr, 0, p.segbytes[0], 0x00020000);

    // weights: fragment of tap t for this lane = W[n = 32 nt + r][t*16 + 8h .. +8] (rows past N are zero in the packed image)
    bf16x8_t wf[NTL][9];
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
        for (int tp = 0; tp < 9; ++tp)
            wf[nt][tp] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(d.w + (size_t)(nt * 32 + r) * p.Ktot + tp * 16 + 8 * h));

    if (EPI == 2) {
        for (int i = t; i < 2 * 32 * NTL; i += 256) {
            const int which = i / (32 * NTL), c = i - which * (32 * NTL);
            sConst[which][c] = c < d.N ? (which == 0 ? d.scale[c] : d.shift[c]) : 0.f;
        }
        __syncthreads();
    }
    // channels of this lane after the MFMA: tile nt, group g (0..3) -> 32 nt + 8g + 4h + (0..3)
    float ssum[EPI == 1 ? NTL : 1][16], ssq[EPI == 1 ? NTL : 1][16];
    if (EPI == 1) {
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt)
#pragma unroll
            for (int e = 0; e < 16; ++e) { ssum[nt][e] = 0.f; ssq[nt][e] = 0.f; }
    }

    const int nstrip = p.M >> 5;                      // W % 32 == 0: strips never cross an image row
    const int wstride = gridDim.x * 4;
    const int spr = W >> 5;                           // strips per row

    u32x4_t xa[2][9];
    auto issue = [&](int s, int set) __attribute__((always_inline)) {
        const int rowid = s / spr;                    // img*H + ho
        const int wo0 = (s - rowid * spr) << 5;
        const int ho = rowid % H;
        const unsigned base = (unsigned)((rowid * W + wo0 + r) * ldx + h * 16);
        const bool lok = (wo0 + r) > 0, rok = (wo0 + r) < W - 1;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const bool row_ok = (ho + kh - 1) >= 0 && (ho + kh - 1) < H;        // wave-uniform
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const bool ok = row_ok && (kw == 0 ? lok : (kw == 2 ? rok : true));
                const unsigned vo = base + (unsigned)(((kh - 1) * W + (kw - 1)) * ldx);
                if (set == 0) xa[0][kh * 3 + kw] = __builtin_amdgcn_raw_buffer_load_b128(rsx, ok ? vo : OOB, 0, 0);
                else          xa[1][kh * 3 + kw] = __builtin_amdgcn_raw_buffer_load_b128(rsx, ok ? vo : OOB, 0, 0);
            }
        }
    };
    auto compute = [&](int s, int set) __attribute__((always_inline)) {
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) {
            f32x16_t acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
            for (int tp = 0; tp < 9; ++tp)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[nt][tp], __builtin_bit_cast(bf16x8_t, set == 0 ? xa[0][tp] : xa[1][tp]), acc, 0, 0, 0);
            // acc[g*4 + e]: pixel r, channel 32 nt + 8g + 4h + e
            uint32_t pk[4][2];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[g * 4 + e];
                if (EPI == 2) {
                    const float4 sc = *reinterpret_cast<const float4*>(&sConst[0][nt * 32 + 8 * g + 4 * h]);
                    const float4 sh = *reinterpret_cast<const float4*>(&sConst[1][nt * 32 + 8 * g + 4 * h]);
                    v[0] = v[0] * sc.x + sh.x; v[1] = v[1] * sc.y + sh.y; v[2] = v[2] * sc.z + sh.z; v[3] = v[3] * sc.w + sh.w;
                    if (d.act == YH_ACT_SILU) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = silu_fast(v[e]);
                    }
                }
                pk[g][0] = pack2(v[0], v[1]);
                pk[g][1] = pack2(v[2], v[3]);
                if (EPI == 1) {                           // statistics of the stored (bf16-rounded) values
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float q = __uint_as_float(e & 1 ? (pk[g][e >> 1] & 0xffff0000u) : (pk[g][e >> 1] << 16));
                        ssum[EPI == 1 ? nt : 0][g * 4 + e] += q; ssq[EPI == 1 ? nt : 0][g * 4 + e] += q * q;
                    }
                }
            }
            // lanes l / l+32: lower half keeps its channels 8g..8g+3 of g = 0, 2 and receives 8g+4..8g+7 from the upper
            // half; the upper half ends up with the 16-byte chunks of g = 1, 3
            uint4 c01, c23;
            {
                auto a0 = __builtin_amdgcn_permlane32_swap(pk[0][0], pk[1][0], false, false);
                auto a1 = __builtin_amdgcn_permlane32_swap(pk[0][1], pk[1][1], false, false);
                auto b0 = __builtin_amdgcn_permlane32_swap(pk[2][0], pk[3][0], false, false);
                auto b1 = __builtin_amdgcn_permlane32_swap(pk[2][1], pk[3][1], false, false);
                c01 = make_uint4(a0[0], a1[0], a0[1], a1[1]);
                c23 = make_uint4(b0[0], b1[0], b0[1], b1[1]);
            }
            // through a wave-private LDS strip [32 pixels][N channels]: stored from the registers, an instruction writes 32 bytes of
            // every pixel row (2.3 TB/s of writes measured: the layer is all writes); read back in memory order, an instruction
            // writes 1 KiB of consecutive 16-byte chunks
            if constexpr (STAGED) {
                uint16_t* srow = sOut + (wave * 32 + r) * STEM_SP + nt * 32 + 8 * h;
                *reinterpret_cast<uint4*>(srow) = c01;                             // channels 32nt +  0..7  (h = 0) /  8..15 (h = 1)
                *reinterpret_cast<uint4*>(srow + 16) = c23;                        // channels 32nt + 16..23 (h = 0) / 24..31 (h = 1)
            } else {
                uint16_t* dst = d.out0 + ((size_t)s * 32 + r) * d.ld0 + nt * 32 + 8 * h;
                *reinterpret_cast<uint4*>(dst) = c01;
                if (nt * 32 + 16 < d.N) *reinterpret_cast<uint4*>(dst + 16) = c23;
            }
        }
        if constexpr (!STAGED) return;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                         // LDS executes a wave's accesses in order
        const int cpp = d.N >> 3;                                                  // 16-byte chunks per pixel
        const size_t m0 = (size_t)s * 32;
#pragma unroll
        for (int it = 0; it < (32 * 32 * NTL / 8 + 63) / 64; ++it) {
            const int q = it * 64 + lane;
            const int px = q / cpp, ck = q - px * cpp;
            if (px < 32)
                *reinterpret_cast<uint4*>(d.out0 + (m0 + px) * d.ld0 + ck * 8) = *reinterpret_cast<const uint4*>(sOut + (wave * 32 + px) * STEM_SP + ck * 8);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                         // read before the next strip overwrites it
    };

    // Strip order.  Workgroups are dealt round-robin to the 8 XCDs by id, and a strip needs the input rows above and below its
    // own: with strips simply dealt to waves in order, vertically adjacent strips land on different XCDs and every XCD fetches
    // every input row (PMC: 3.2 - 4.2x the input).  With p.xgx set (whole bands of STEM_BAND rows per XCD: host check) XCD x works
    // through the bands x, x + 8, ... — its waves walk a band row by row together, so the halo rows are L2 hits.
    auto strip_of = [&](int u) __attribute__((always_inline)) {      // u: position in this wave's XCD-local (or global) order
        if (!p.xgx) return u;
        const int per_band = STEM_BAND * spr;
        const int bl = u / per_band, within = u - bl * per_band;
        return ((bl << 3) + ((int)blockIdx.x & 7)) * per_band + within;
    };
    const int ustride = p.xgx ? (int)(gridDim.x >> 3) * 4 : wstride;
    const int ulim = p.xgx ? nstrip >> 3 : nstrip;
    int u = p.xgx ? (int)(blockIdx.x >> 3) * 4 + wave : (int)blockIdx.x * 4 + wave;
    if (u < ulim) issue(strip_of(u), 0);
    for (; u < ulim; u += 2 * ustride) {
        const int u1 = u + ustride, u2 = u + 2 * ustride;
        if (u1 < ulim) issue(strip_of(u1), 1);
        compute(strip_of(u), 0);
        if (u1 < ulim) {
            if (u2 < ulim) issue(strip_of(u2), 0);
            compute(strip_of(u1), 1);
        }
    }

    if (EPI == 1) {
        // lane holds 16 channels x its pixel column per tile: sum over the 32 pixel lanes of each half, then over the waves
#pragma unroll
        for (int nt = 0; nt < (EPI == 1 ? NTL : 1); ++nt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float a = ssum[nt][e], q = ssq[nt][e];
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); q += __shfl_xor(q, o, 64); }
                if (r == 0) { const int ch = nt * 32 + 8 * (e >> 2) + 4 * h + (e & 3); sRed[wave][0][ch] = a; sRed[wave][1][ch] = q; }
            }
        __syncthreads();
        if (t < 64 * NTL) {
            const int which = t / (32 * NTL), ch = t - which * (32 * NTL);
            const float v = sRed[0][which][ch] + sRed[1][which][ch] + sRed[2][which][ch] + sRed[3][which][ch];
            if (ch < d.Npad) put_stat(d, blockIdx.x, which, ch, v);
        }
    }
}

template <int NTL> void stem_launch(const ConvPlan& pl, hipStream_t st)
{
    if (pl.epi == 2)      conv_stem_kernel<2, NTL><<<pl.grid, pl.block, 0, st>>>(pl.k);
    else if (pl.epi == 1) conv_stem_kernel<1, (NTL <= 2 ? NTL : 2)><<<pl.grid, pl.block, 0, st>>>(pl.k);
    else                  conv_stem_kernel<0, NTL><<<pl.grid, pl.block, 0, st>>>(pl.k);
}

}  // namespace

void yh_conv::conv_launch_stem(const ConvPlan& pl, hipStream_t st)
{
    if (pl.ntl == 1) stem_launch<1>(pl, st); else if (pl.ntl == 2) stem_launch<2>(pl, st); else stem_launch<3>(pl, st);
}
