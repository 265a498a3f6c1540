// Train-time augmentation on the device: mosaic + random perspective + flips + HSV jitter of a batch of raw uint8 HWC images as one
// gather per output pixel, written as the letterbox's output, (B, 3, H, W) fp32 in [0, 1].  The mosaic canvas is never built: it is
// described by up to four paste rectangles ("tiles") per image, and the warp, the flips and the crop are one 3 x 3 matrix (output
// pixel -> canvas).  utils/augment.py augment_batch_host states the same computation in NumPy float32; the two agree bit for bit.
//
// Operation order, every operation a correctly rounded fp32 operation (this file compiles with the exact flags: no contraction):
//   xf = float(x), yf = float(y)
//   nu = (m0*xf + m1*yf) + m2      nv = (m3*xf + m4*yf) + m5      w = (m6*xf + m7*yf) + m8
//   u = nu / w,  v = nv / w                                  (skipped where the last row is 0 0 1: dividing by 1.0f is exact)
//   fu = min(max(floor(u), -2), 2^30),  fv likewise          (fmax / fmin: a NaN coordinate becomes -2, i.e. outside)
//   ax = u - fu,  ay = v - fv,  bx = 1 - ax,  by = 1 - ay
//   taps p00 p01 | p10 p11 at (fu + {0, 1}, fv + {0, 1}): the byte of the highest tile whose rectangle holds the tap, else fill_value
//   top = p00*bx + p01*ax,  bot = p10*bx + p11*ax,  val = top*by + bot*ay        (0..255 scale, no rounding to uint8)
//   HSV gains g, if given, on (r, g, b) = val of the three planes:
//     V = max(r, max(g, b)),  m = min(r, min(g, b)),  d = V - m,  S = V > 0 ? (255*d) / V : 0
//     H = d == 0 ? 0 : V == r ? (30*(g - b)) / d : V == g ? 60 + (30*(b - r)) / d : 120 + (30*(r - g)) / d;  H < 0: H += 180
//     H' = fmod(H*g0, 180),  S' = min(S*g1, 255),  V' = min(V*g2, 255),  s = S' / 255,  h6 = H' / 30
//     i = min(max(int(floor(h6)), 0), 5),  f = h6 - i,  p = V'*(1 - s),  q = V'*(1 - s*f),  t = V'*(1 - s*(1 - f))
//     (r, g, b) = (V',t,p) (q,V',p) (p,V',t) (p,q,V') (t,p,V') (V',p,q) for i = 0..5
//   out = val / 255
//
// One workgroup owns an output row (b, y) of all three planes, one lane four consecutive columns: the matrix, the tiles and the gains
// of the row are wave-uniform (scalar registers), the tile test is selects, and a tap that hits no tile reads byte 0..2 of raw and
// drops it, so the 48 byte loads of a lane (4 pixels x 4 taps x 3 channels) are issued without a branch between them.  Source
// indices are clamped into their image, so a wrong table reads a wrong pixel of raw, never an address outside the image it names
// (an image of 2^31 pixels or more is the collate's to refuse).  Each lane stores 16 contiguous bytes per plane.
// Measured ("Ingest"): several times the letterbox kernel's time at the same output size; the integer work of
// the tile test and the byte loads set the time, not the stores.  Staging the source rows in LDS by 16-byte loads is the open step.
#include "common.h"

#define AUG_MAX_THREADS 512
#define AUG_GRID_CAP 2048                   // workgroups per launch: (b, y) rows past it are taken by the grid-stride loop

// offsets into raw of the bytes shown at the canvas pixels (tx + {0, 1}, ty + {0, 1}) (order: 00 01 | 10 11, x fastest), or -1 where
// the canvas shows the fill value.  Per tile: one range test per axis and tap position (unsigned: tx - ox0 < ox1 - ox0), the clamped
// source column / row of both positions, and the four offsets relative to the image, selected where the tile is hit; 32-bit
// arithmetic on unsigned values (wrapping is defined, and a wrapped offset of a clamped index is smaller than the true one: still
// inside the image), the 64-bit image offset added at the end.  The tile fields are wave-uniform (scalar registers).
__device__ __forceinline__ void aug_tap_offsets(const yh_aug_tile* __restrict__ t, int ch, int cw, int tx, int ty, long off[4])
{
    unsigned rel[4] = {0u, 0u, 0u, 0u};
    long base[4] = {0L, 0L, 0L, 0L};
    bool hit[4] = {false, false, false, false};
    const unsigned ux = (unsigned)tx, uy = (unsigned)ty;
#pragma unroll
    for (int k = 0; k < 4; ++k) {           // later tiles are pasted over earlier ones
        const bool live = t[k].src_h > 0 && t[k].src_w > 0 && t[k].ox1 > t[k].ox0 && t[k].oy1 > t[k].oy0;
        const unsigned rw = (unsigned)t[k].ox1 - (unsigned)t[k].ox0, rh = (unsigned)t[k].oy1 - (unsigned)t[k].oy0;
        const bool inx[2] = {ux - (unsigned)t[k].ox0 < rw, ux + 1u - (unsigned)t[k].ox0 < rw};
        const bool iny[2] = {live && uy - (unsigned)t[k].oy0 < rh, live && uy + 1u - (unsigned)t[k].oy0 < rh};
        const int dx = (int)((unsigned)t[k].sx0 - (unsigned)t[k].ox0 + ux), dy = (int)((unsigned)t[k].sy0 - (unsigned)t[k].oy0 + uy);
        const int wm = t[k].src_w - 1, hm = t[k].src_h - 1;
        const unsigned sx[2] = {(unsigned)min(max(dx, 0), wm), (unsigned)min(max((int)((unsigned)dx + 1u), 0), wm)};
        const unsigned sy[2] = {(unsigned)min(max(dy, 0), hm) * (unsigned)t[k].src_w,
                                (unsigned)min(max((int)((unsigned)dy + 1u), 0), hm) * (unsigned)t[k].src_w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = inx[j & 1] && iny[j >> 1];
            rel[j] = in ? sy[j >> 1] + sx[j & 1] : rel[j];
            base[j] = in ? t[k].off : base[j];
            hit[j] = hit[j] || in;
        }
    }
    const bool cx[2] = {ux < (unsigned)cw, ux + 1u < (unsigned)cw};
    const bool cy[2] = {uy < (unsigned)ch, uy + 1u < (unsigned)ch};
#pragma unroll
    for (int j = 0; j < 4; ++j) off[j] = hit[j] && cx[j & 1] && cy[j >> 1] ? base[j] + (long)rel[j] * 3 : -1L;
}

__device__ __forceinline__ void aug_hsv(float& r, float& g, float& b, float g0, float g1, float g2)
{
    const float V = fmaxf(r, fmaxf(g, b));
    const float m = fminf(r, fminf(g, b));
    const float d = __fsub_rn(V, m);
    const float S = V > 0.f ? __fdiv_rn(__fmul_rn(255.f, d), V) : 0.f;
    float H;
    if (d == 0.f) H = 0.f;
    else if (V == r) H = __fdiv_rn(__fmul_rn(30.f, __fsub_rn(g, b)), d);
    else if (V == g) H = __fadd_rn(60.f, __fdiv_rn(__fmul_rn(30.f, __fsub_rn(b, r)), d));
    else H = __fadd_rn(120.f, __fdiv_rn(__fmul_rn(30.f, __fsub_rn(r, g)), d));
    if (H < 0.f) H = __fadd_rn(H, 180.f);
    const float H2 = fmodf(__fmul_rn(H, g0), 180.f);
    const float S2 = fminf(__fmul_rn(S, g1), 255.f);
    const float V2 = fminf(__fmul_rn(V, g2), 255.f);
    const float s = __fdiv_rn(S2, 255.f);
    const float h6 = __fdiv_rn(H2, 30.f);
    const float fi = fminf(fmaxf(floorf(h6), 0.f), 5.f);
    const int i = (int)fi;
    const float f = __fsub_rn(h6, fi);
    const float p = __fmul_rn(V2, __fsub_rn(1.f, s));
    const float q = __fmul_rn(V2, __fsub_rn(1.f, __fmul_rn(s, f)));
    const float t = __fmul_rn(V2, __fsub_rn(1.f, __fmul_rn(s, __fsub_rn(1.f, f))));
    r = i == 0 || i == 5 ? V2 : i == 1 ? q : i == 4 ? t : p;
    g = i == 1 || i == 2 ? V2 : i == 0 ? t : i == 3 ? q : p;
    b = i == 3 || i == 4 ? V2 : i == 2 ? t : i == 5 ? q : p;
}

__global__ __launch_bounds__(AUG_MAX_THREADS) void augment_batch_kernel(
    const uint8_t* __restrict__ raw, const yh_aug_tile* __restrict__ tiles, const int32_t* __restrict__ canvas_hw,
    const float* __restrict__ minv, const float* __restrict__ hsv_gain, unsigned nrows, unsigned H, int W, int fill_value,
    float* __restrict__ out)
{
    const int nthreads = blockDim.x;
    const int W4 = W >> 2;
    const long plane = (long)H * W;
    const float fill = (float)fill_value;
    for (unsigned row = blockIdx.x; row < nrows; row += gridDim.x) {
        const unsigned b = row / H;
        const unsigned y = row - b * H;
        const yh_aug_tile* t = tiles + (long)b * 4;
        const int ch = canvas_hw[2 * b], cw = canvas_hw[2 * b + 1];
        const float* m = minv + (long)b * 9;
        const float m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5], m6 = m[6], m7 = m[7], m8 = m[8];
        const bool affine = m6 == 0.f && m7 == 0.f && m8 == 1.f;      // per image: w == 1.0f for every pixel
        const float yf = (float)y;
        float* o = out + ((long)b * 3 * H + y) * W;
        for (int x4 = threadIdx.x; x4 < W4; x4 += nthreads) {
            long off[4][4];
            float ax[4], ay[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xf = (float)(x4 * 4 + e);
                float u = __fadd_rn(__fadd_rn(__fmul_rn(m0, xf), __fmul_rn(m1, yf)), m2);
                float v = __fadd_rn(__fadd_rn(__fmul_rn(m3, xf), __fmul_rn(m4, yf)), m5);
                if (!affine) {
                    const float w = __fadd_rn(__fadd_rn(__fmul_rn(m6, xf), __fmul_rn(m7, yf)), m8);
                    u = __fdiv_rn(u, w);
                    v = __fdiv_rn(v, w);
                }
                const float fu = fminf(fmaxf(floorf(u), -2.f), 1073741824.f);
                const float fv = fminf(fmaxf(floorf(v), -2.f), 1073741824.f);
                ax[e] = __fsub_rn(u, fu);
                ay[e] = __fsub_rn(v, fv);
                aug_tap_offsets(t, ch, cw, (int)fu, (int)fv, off[e]);
            }
            // no branch around the loads: a tap that shows the fill value reads bytes 0..2 of raw and drops them
            int px[4][4][3];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint8_t* s = raw + (off[e][k] < 0 ? 0L : off[e][k]);
#pragma unroll
                    for (int c = 0; c < 3; ++c) px[e][k][c] = s[c];
                }
            float val[3][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float bx = __fsub_rn(1.f, ax[e]), by = __fsub_rn(1.f, ay[e]);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float p00 = off[e][0] < 0 ? fill : (float)px[e][0][c];
                    const float p01 = off[e][1] < 0 ? fill : (float)px[e][1][c];
                    const float p10 = off[e][2] < 0 ? fill : (float)px[e][2][c];
                    const float p11 = off[e][3] < 0 ? fill : (float)px[e][3][c];
                    const float top = __fadd_rn(__fmul_rn(p00, bx), __fmul_rn(p01, ax[e]));
                    const float bot = __fadd_rn(__fmul_rn(p10, bx), __fmul_rn(p11, ax[e]));
                    val[c][e] = __fadd_rn(__fmul_rn(top, by), __fmul_rn(bot, ay[e]));
                }
            }
            if (hsv_gain) {                                           // per launch
                const float g0 = hsv_gain[3 * b], g1 = hsv_gain[3 * b + 1], g2 = hsv_gain[3 * b + 2];
#pragma unroll
                for (int e = 0; e < 4; ++e) aug_hsv(val[0][e], val[1][e], val[2][e], g0, g1, g2);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<float4*>(o + c * plane + x4 * 4) = make_float4(
                    __fdiv_rn(val[c][0], 255.f), __fdiv_rn(val[c][1], 255.f), __fdiv_rn(val[c][2], 255.f), __fdiv_rn(val[c][3], 255.f));
        }
    }
}

extern "C" int yh_augment_batch(const uint8_t* raw, const yh_aug_tile* tiles, const int32_t* canvas_hw, const float* minv,
                                const float* hsv_gain, int B, int H, int W, int fill_value, float* out, yh_stream stream)
{
    YH_CHECK_ARG(raw && tiles && canvas_hw && minv && out, "yh_augment_batch: null pointer");
    YH_CHECK_ARG(B > 0 && H > 0 && W > 0, "yh_augment_batch: B, H, W must be positive (B=%d H=%d W=%d)", B, H, W);
    YH_CHECK_ARG(W % 4 == 0, "yh_augment_batch: W=%d is not a multiple of 4 (16-byte stores)", W);
    YH_CHECK_ARG(yh_aligned16(out), "yh_augment_batch: out is not 16-byte aligned");
    YH_CHECK_ARG((((uintptr_t)tiles) & 7) == 0 && ((((uintptr_t)canvas_hw) | ((uintptr_t)minv) | ((uintptr_t)hsv_gain)) & 3) == 0,
                 "yh_augment_batch: tables unaligned (tiles 8 bytes, canvas_hw / minv / hsv_gain 4 bytes)");
    YH_CHECK_ARG(fill_value >= 0 && fill_value <= 255, "yh_augment_batch: fill_value %d is not a byte", fill_value);
    YH_CHECK_ARG((long)B * H <= 0x7fffffffL, "yh_augment_batch: B * H = %ld output rows do not fit 31 bits", (long)B * H);
    const unsigned nrows = (unsigned)B * (unsigned)H;
    int threads = ((W / 4 + YH_WAVE - 1) / YH_WAVE) * YH_WAVE;       // one lane per 4 output columns, whole waves
    if (threads > AUG_MAX_THREADS) threads = AUG_MAX_THREADS;
    const int grid = (int)(nrows < AUG_GRID_CAP ? nrows : AUG_GRID_CAP);
    hipLaunchKernelGGL(augment_batch_kernel, dim3(grid), dim3(threads), 0, (hipStream_t)stream,
                       raw, tiles, canvas_hw, minv, hsv_gain, nrows, (unsigned)H, W, fill_value, out);
    YH_CHECK_LAUNCH("yh_augment_batch");
    return YH_OK;
}
