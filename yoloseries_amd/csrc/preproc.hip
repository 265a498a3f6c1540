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
