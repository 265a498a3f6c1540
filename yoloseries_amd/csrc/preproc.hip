// Input pre-processing on the device: a batch of raw uint8 HWC images -> the letterboxed (B, 3, H, W) fp32 network input,
// bit-identical to utils/letterbox.py letter_resize_img + dataset/data_collater.py normal_normalization on the host.
//
// The geometry arrives as per-image index tables (source row of every output row, source column of every output column, -1 on the
// border): the host builds them with the float64 expression of resize_nearest, which integer arithmetic in a kernel does not
// reproduce.  The scale is the correctly rounded fp32 quotient v / 255.0f (== float32(v / 255.0) for all 256 bytes; v * (1 / 255.0f)
// differs for 126 of them): one true division per table entry, 256 entries in LDS per workgroup.  This file compiles with the exact
// flags (Makefile: not in CONTRACT_FAST).
//
// One workgroup owns an output row (b, y) of all three planes, so the source row is fetched from memory once: the three bytes of a
// pixel are read by the same lane, neighbouring lanes read neighbouring pixels, and L1 / L2 serve the repeats of an up-scale.  The
// bytes are read one (or two) at a time, so an image that starts at any byte offset needs no special case.  Each lane stores 16
// contiguous bytes per plane.  Measured ("Ingest"): about half the rate of its stores alone -- the byte loads
// set the time, not a chain of latencies (four rows in flight per workgroup measured the same); staging the row in LDS by 16-byte
// loads is the open step.
#include "common.h"

#define LB_MAX_THREADS 512
#define LB_GRID_CAP 2048                    // workgroups per launch: (b, y) rows past it are taken by the grid-stride loop

__global__ __launch_bounds__(LB_MAX_THREADS) void letterbox_batch_kernel(
    const uint8_t* __restrict__ raw, const int64_t* __restrict__ img_off, const int32_t* __restrict__ src_hw,
    const int32_t* __restrict__ rows, const int32_t* __restrict__ cols, unsigned nrows, unsigned H, int W, int fill_value, float* __restrict__ out)
{
    __shared__ float lut[256];
    for (int v = threadIdx.x; v < 256; v += blockDim.x) lut[v] = (float)v / 255.0f;
    __syncthreads();
    const float fill = lut[fill_value];
    const int nthreads = blockDim.x;
    const int W4 = W >> 2;
    const long plane = (long)H * W;
    for (unsigned row = blockIdx.x; row < nrows; row += gridDim.x) {
        const unsigned b = row / H;
        const unsigned y = row - b * H;
        const int r = rows[row];                                      // rows is [B][H]: row == b * H + y
        const int32_t* crow = cols + (long)b * W;
        float* o = out + ((long)b * 3 * H + y) * W;
        if (r < 0) {                                                  // border row: nothing is read from raw
            const float4 f = make_float4(fill, fill, fill, fill);
            for (int x4 = threadIdx.x; x4 < W4; x4 += nthreads) {
                *reinterpret_cast<float4*>(o + x4 * 4) = f;
                *reinterpret_cast<float4*>(o + plane + x4 * 4) = f;
                *reinterpret_cast<float4*>(o + 2 * plane + x4 * 4) = f;
            }
            continue;
        }
        const uint8_t* src = raw + img_off[b] + (long)r * src_hw[2 * b + 1] * 3;
        for (int x4 = threadIdx.x; x4 < W4; x4 += nthreads) {
            const int4 c4 = *reinterpret_cast<const int4*>(crow + x4 * 4);
            const int c[4] = {c4.x, c4.y, c4.z, c4.w};
            // no branch around the loads, so all twelve are in flight together: a border column reads column 0 of the row (which
            // exists: r >= 0) and drops it
            int v[3][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint8_t* s = src + (c[e] < 0 ? 0 : c[e]) * 3;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch][e] = s[ch];
            }
            float p[3][4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) p[ch][e] = lut[c[e] < 0 ? fill_value : v[ch][e]];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                *reinterpret_cast<float4*>(o + ch * plane + x4 * 4) = make_float4(p[ch][0], p[ch][1], p[ch][2], p[ch][3]);
        }
    }
}

extern "C" int yh_letterbox_batch(const uint8_t* raw, const int64_t* img_off, const int32_t* src_hw, const int32_t* rows, const int32_t* cols,
                                  int B, int H, int W, int fill_value, float* out, yh_stream stream)
{
    YH_CHECK_ARG(raw && img_off && src_hw && rows && cols && out, "yh_letterbox_batch: null pointer");
    YH_CHECK_ARG(B > 0 && H > 0 && W > 0, "yh_letterbox_batch: B, H, W must be positive (B=%d H=%d W=%d)", B, H, W);
    YH_CHECK_ARG(W % 4 == 0, "yh_letterbox_batch: W=%d is not a multiple of 4 (16-byte stores)", W);
    YH_CHECK_ARG(yh_aligned16(out) && yh_aligned16(cols), "yh_letterbox_batch: out / cols not 16-byte aligned");
    YH_CHECK_ARG((((uintptr_t)img_off) & 7) == 0 && ((((uintptr_t)src_hw) | ((uintptr_t)rows)) & 3) == 0, "yh_letterbox_batch: index tables unaligned");
    YH_CHECK_ARG(fill_value >= 0 && fill_value <= 255, "yh_letterbox_batch: fill_value %d is not a byte", fill_value);
    YH_CHECK_ARG((long)B * H <= 0x7fffffffL, "yh_letterbox_batch: B * H = %ld output rows do not fit 31 bits", (long)B * H);
    const unsigned nrows = (unsigned)B * (unsigned)H;
    int threads = ((W / 4 + YH_WAVE - 1) / YH_WAVE) * YH_WAVE;       // one lane per 4 output columns, whole waves
    if (threads > LB_MAX_THREADS) threads = LB_MAX_THREADS;
    const int grid = (int)(nrows < LB_GRID_CAP ? nrows : LB_GRID_CAP);
    hipLaunchKernelGGL(letterbox_batch_kernel, dim3(grid), dim3(threads), 0, (hipStream_t)stream,
                       raw, img_off, src_hw, rows, cols, nrows, (unsigned)H, W, fill_value, out);
    YH_CHECK_LAUNCH("yh_letterbox_batch");
    return YH_OK;
}

// ---------------------------------------------------------------- bilinear resize (multi-scale training)
// torch's F.interpolate(mode='bilinear', align_corners=False) on the CPU, bit for bit: per axis
//   scale = float(n_in) / float(n_out)  (divided on the host),  src = max(fma(scale, d + 0.5, -0.5), 0),
//   i0 = min(int(src), n_in - 1),  i1 = min(i0 + 1, n_in - 1),  l1 = src - i0,  l0 = 1 - l1
// and per pixel, with a the row and b the column weights and A B | C D the taps of rows y0 | y1, one of torch's two forms: its
// general kernel's  out = fma(a0, fma(A, b0, B * b1), a1 * fma(C, b0, D * b1)),  or, where torch runs its small-output kernel
// (Ho + Wo <= 128: _use_vectorized_kernel_cond_2d of ATen's UpSampleKernel.cpp), the four products
//   out = fma(a1*b1, D, fma(a1*b0, C, fma(a0*b0, A, (a0*b1) * B)))  with each weight product rounded first.
// Every operation is pinned by an intrinsic; other orders of the same expressions differ from torch in the last place or two at
// small sizes and by up to 3e-5 at 640-wide inputs.
// The indices come out of the clamps, so no argument can make the kernel read outside x.
//
// One workgroup owns RS_ROWS consecutive output rows of every plane of one image, one lane four consecutive output columns of all of
// them: the column taps and weights live in registers for the whole tile, neighbouring lanes read neighbouring source pixels, and the
// source rows that the tile's output rows share are meant to be fetched from memory once, L1 / L2 serving the repeats (by design:
// the traffic has not been measured; staging the rows in LDS by 16-byte loads is the alternative).  Stores are 16 bytes per
// lane.  The s2d form writes the stem's input (yh_input_s2d's layout and fp32 -> bf16 conversion) straight from the samples: one lane
// owns one output pixel, i.e. a 2 x 2 block of resized positions of every channel, 32 contiguous bytes.
#define RS_MAX_THREADS 512
#define RS_GRID_CAP 2048                    // workgroups per launch: tiles past it are taken by the grid-stride loop
#define RS_ROWS 4                           // output rows per tile (2 rows of the s2d form)
#define RS_SMALL_SUM 128                    // Ho + Wo up to which torch's CPU build takes its four-product kernel

struct RsAxis { int i0, i1; float l0, l1; };

__device__ __forceinline__ RsAxis rs_axis(float scale, int d, int n_in)
{
    RsAxis a;
    const float src = fmaxf(__fmaf_rn(scale, __fadd_rn((float)d, 0.5f), -0.5f), 0.f);
    a.i0 = min((int)src, n_in - 1);
    a.i1 = min(a.i0 + 1, n_in - 1);
    a.l1 = __fsub_rn(src, (float)a.i0);
    a.l0 = __fsub_rn(1.0f, a.l1);
    return a;
}

__device__ __forceinline__ float rs_sample(const float* __restrict__ p0, const float* __restrict__ p1, const RsAxis& cx, const RsAxis& cy,
                                           bool small)
{
    if (small) {                            // wave-uniform: a property of the launch
        float acc = __fmul_rn(__fmul_rn(cy.l0, cx.l1), p0[cx.i1]);
        acc = __fmaf_rn(__fmul_rn(cy.l0, cx.l0), p0[cx.i0], acc);
        acc = __fmaf_rn(__fmul_rn(cy.l1, cx.l0), p1[cx.i0], acc);
        return __fmaf_rn(__fmul_rn(cy.l1, cx.l1), p1[cx.i1], acc);
    }
    const float r0 = __fmaf_rn(p0[cx.i0], cx.l0, __fmul_rn(p0[cx.i1], cx.l1));
    const float r1 = __fmaf_rn(p1[cx.i0], cx.l0, __fmul_rn(p1[cx.i1], cx.l1));
    return __fmaf_rn(cy.l0, r0, __fmul_rn(cy.l1, r1));
}

template <bool VEC>
__global__ __launch_bounds__(RS_MAX_THREADS) void resize_bilinear_kernel(
    const float* __restrict__ x, unsigned ntiles, int C, int H, int W, int Ho, int Wo, float sy, float sx, int small, float* __restrict__ out)
{
    const unsigned tiles_per_img = (unsigned)((Ho + RS_ROWS - 1) / RS_ROWS);
    const int ngroups = (Wo + 3) >> 2;
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned b = tile / tiles_per_img;
        const int y_base = (int)(tile - b * tiles_per_img) * RS_ROWS;
        for (int g = threadIdx.x; g < ngroups; g += blockDim.x) {
            RsAxis cx[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) cx[e] = rs_axis(sx, min(g * 4 + e, Wo - 1), W);
            for (int r = 0; r < RS_ROWS && y_base + r < Ho; ++r) {
                const int y = y_base + r;
                const RsAxis cy = rs_axis(sy, y, H);
                for (int c = 0; c < C; ++c) {
                    const long plane = (long)b * C + c;
                    const float* p0 = x + (plane * H + cy.i0) * (long)W;
                    const float* p1 = x + (plane * H + cy.i1) * (long)W;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = rs_sample(p0, p1, cx[e], cy, small != 0);
                    float* o = out + (plane * Ho + y) * (long)Wo + g * 4;
                    if (VEC) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                    else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (g * 4 + e < Wo) o[e] = v[e];
                    }
                }
            }
        }
    }
}

template <int CIN>
__global__ __launch_bounds__(RS_MAX_THREADS) void resize_bilinear_s2d_kernel(
    const float* __restrict__ x, unsigned ntiles, int H, int W, int Ho, int Wo, float sy, float sx, int small, uint16_t* __restrict__ out)
{
    const int H2 = Ho >> 1, W2 = Wo >> 1;
    const unsigned tiles_per_img = (unsigned)((H2 + RS_ROWS / 2 - 1) / (RS_ROWS / 2));
    for (unsigned tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const unsigned b = tile / tiles_per_img;
        const int h2_base = (int)(tile - b * tiles_per_img) * (RS_ROWS / 2);
        for (int g = threadIdx.x; g < W2; g += blockDim.x) {
            const RsAxis cx[2] = {rs_axis(sx, 2 * g, W), rs_axis(sx, 2 * g + 1, W)};
            for (int r = 0; r < RS_ROWS / 2 && h2_base + r < H2; ++r) {
                const int h2 = h2_base + r;
                float f[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) f[e] = 0.f;
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    const RsAxis cy = rs_axis(sy, 2 * h2 + dy, H);
#pragma unroll
                    for (int c = 0; c < CIN; ++c) {
                        const long plane = (long)b * CIN + c;
                        const float* p0 = x + (plane * H + cy.i0) * (long)W;
                        const float* p1 = x + (plane * H + cy.i1) * (long)W;
                        f[(dy * 2 + 0) * CIN + c] = rs_sample(p0, p1, cx[0], cy, small != 0);
                        f[(dy * 2 + 1) * CIN + c] = rs_sample(p0, p1, cx[1], cy, small != 0);
                    }
                }
                uint4* o = reinterpret_cast<uint4*>(out + (((long)b * H2 + h2) * W2 + g) * 16);
                o[0] = pack8(f);
                o[1] = pack8(f + 8);
            }
        }
    }
}

static int rs_threads(int lanes)
{
    const int t = ((lanes + YH_WAVE - 1) / YH_WAVE) * YH_WAVE;       // whole waves
    return t > RS_MAX_THREADS ? RS_MAX_THREADS : t;
}

extern "C" int yh_resize_bilinear(const float* x, int B, int C, int H, int W, int Ho, int Wo, float* out, yh_stream stream)
{
    YH_CHECK_ARG(x && out, "yh_resize_bilinear: null pointer (x=%p out=%p)", (const void*)x, (void*)out);
    YH_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0,
                 "yh_resize_bilinear: sizes must be positive (B=%d C=%d H=%d W=%d Ho=%d Wo=%d)", B, C, H, W, Ho, Wo);
    YH_CHECK_ARG((((uintptr_t)x) & 3) == 0, "yh_resize_bilinear: x is not 4-byte aligned");
    YH_CHECK_ARG(yh_aligned16(out), "yh_resize_bilinear: out is not 16-byte aligned");
    YH_CHECK_ARG((long)B * C * Ho <= 0x7fffffffL && (long)B * C * H <= 0x7fffffffL,
                 "yh_resize_bilinear: B * C * max(H, Ho) = %ld rows do not fit 31 bits", (long)B * C * (H > Ho ? H : Ho));
    const unsigned ntiles = (unsigned)B * (unsigned)((Ho + RS_ROWS - 1) / RS_ROWS);
    const int grid = (int)(ntiles < RS_GRID_CAP ? ntiles : RS_GRID_CAP);
    const int threads = rs_threads((Wo + 3) / 4);
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const int small = Ho + Wo <= RS_SMALL_SUM;
    if (Wo % 4 == 0)
        hipLaunchKernelGGL(resize_bilinear_kernel<true>, dim3(grid), dim3(threads), 0, (hipStream_t)stream, x, ntiles, C, H, W, Ho, Wo, sy, sx, small, out);
    else
        hipLaunchKernelGGL(resize_bilinear_kernel<false>, dim3(grid), dim3(threads), 0, (hipStream_t)stream, x, ntiles, C, H, W, Ho, Wo, sy, sx, small, out);
    YH_CHECK_LAUNCH("yh_resize_bilinear");
    return YH_OK;
}

extern "C" int yh_resize_bilinear_s2d(const float* x, int B, int Cin, int H, int W, int Ho, int Wo, yh_bf16* out, yh_stream stream)
{
    YH_CHECK_ARG(x && out, "yh_resize_bilinear_s2d: null pointer (x=%p out=%p)", (const void*)x, (void*)out);
    YH_CHECK_ARG(B > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0,
                 "yh_resize_bilinear_s2d: sizes must be positive (B=%d H=%d W=%d Ho=%d Wo=%d)", B, H, W, Ho, Wo);
    YH_CHECK_ARG(Cin >= 1 && Cin <= 4, "yh_resize_bilinear_s2d: Cin=%d is not in 1..4 (16 output channels = 4 * Cin + padding)", Cin);
    YH_CHECK_ARG(Ho % 2 == 0 && Wo % 2 == 0, "yh_resize_bilinear_s2d: output size %dx%d is not even (space-to-depth by 2)", Ho, Wo);
    YH_CHECK_ARG((((uintptr_t)x) & 3) == 0, "yh_resize_bilinear_s2d: x is not 4-byte aligned");
    YH_CHECK_ARG(yh_aligned16(out), "yh_resize_bilinear_s2d: out is not 16-byte aligned");
    YH_CHECK_ARG((long)B * Cin * H <= 0x7fffffffL && (long)B * Ho <= 0x7fffffffL,
                 "yh_resize_bilinear_s2d: B * max(Cin * H, Ho) = %ld rows do not fit 31 bits", (long)B * (Cin * H > Ho ? Cin * H : Ho));
    const unsigned ntiles = (unsigned)B * (unsigned)((Ho / 2 + RS_ROWS / 2 - 1) / (RS_ROWS / 2));
    const dim3 grid(ntiles < RS_GRID_CAP ? ntiles : RS_GRID_CAP), threads(rs_threads(Wo / 2));
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const int small = Ho + Wo <= RS_SMALL_SUM;
    uint16_t* o = reinterpret_cast<uint16_t*>(out);
    const hipStream_t st = (hipStream_t)stream;
    switch (Cin) {
        case 1: hipLaunchKernelGGL(resize_bilinear_s2d_kernel<1>, grid, threads, 0, st, x, ntiles, H, W, Ho, Wo, sy, sx, small, o); break;
        case 2: hipLaunchKernelGGL(resize_bilinear_s2d_kernel<2>, grid, threads, 0, st, x, ntiles, H, W, Ho, Wo, sy, sx, small, o); break;
        case 3: hipLaunchKernelGGL(resize_bilinear_s2d_kernel<3>, grid, threads, 0, st, x, ntiles, H, W, Ho, Wo, sy, sx, small, o); break;
        default: hipLaunchKernelGGL(resize_bilinear_s2d_kernel<4>, grid, threads, 0, st, x, ntiles, H, W, Ho, Wo, sy, sx, small, o); break;
    }
    YH_CHECK_LAUNCH("yh_resize_bilinear_s2d");
    return YH_OK;
}
