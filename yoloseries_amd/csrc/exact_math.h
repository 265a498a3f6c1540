// Device math shared by the files whose results must match the oracle's fp32 operation order bit for bit: the three losses,
// the box utilities and the post-processing (loss_v5.hip, loss_yolox.hip, loss_v8.hip, bbox.hip, postproc.hip).
// ONLY files built with the Makefile's EXACT flags (-ffp-contract=off, no SLP / loop vectorizer) may include this header: under
// contraction the same text would round differently in each includer.  Everything here is inlined into its caller, so one
// definition gives every caller the same operations in the same order.
#pragma once
#include "common.h"

// IEEE division and libm expf (common.h's sigmoidf_ / sigmoid_fast are the approximate forms of the bf16 activation path)
__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// one element of a head tensor, fp32 or bf16 (uint16_t), as float
template <typename T> __device__ __forceinline__ float ldf(const T* p);
template <> __device__ __forceinline__ float ldf<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ldf<uint16_t>(const uint16_t* p) { return bf2f(*p); }
template <typename T> __device__ __forceinline__ void stf(T* p, float v);
template <> __device__ __forceinline__ void stf<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void stf<uint16_t>(uint16_t* p, float v) { *p = f2bf(v); }

// BCEWithLogits(x, t, pos_weight) as torch computes it; dx = d/dx, dt = d/dt (either may be null)
__device__ __forceinline__ float bce_logits(float x, float t, float pw, float* dx, float* dt) {
    const float lw = 1.0f + (pw - 1.0f) * t;
    const float sp = log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.0f);      // softplus(-x) = -log(sigmoid(x))
    const float sg = sigm(x);
    if (dx) *dx = (1.0f - t) - lw * (1.0f - sg);
    if (dt) *dt = -x + (pw - 1.0f) * sp;                              // d/dt [(1-t)x + (1+(pw-1)t) sp]
    return (1.0f - t) * x + lw * sp;
}
// focal factor (1 - acc)^gamma * alpha_t with acc = t p + (1-t)(1-p), and its derivatives (either may be null).
// d(1-acc)/dx = -(2t-1) p (1-p).  Where om <= 0 (the sigmoid rounded to t exactly) the power's derivative is taken as 0 and
// dx is formed as (0 * d(1-acc)/dx) * alpha_t: a zero whose sign follows the operands, never 0 * alpha_t alone.
__device__ __forceinline__ float focal_factor(float x, float t, float gamma, float alpha, float* dx, float* dt) {
    const float pr = sigm(x);
    const float acc = t * pr + (1.0f - t) * (1.0f - pr);
    const float om = 1.0f - acc;
    const float gf = powf(om, gamma);
    const float af = t * alpha + (1.0f - t) * (1.0f - alpha);
    const float dgf_dom = om > 0.f ? gamma * powf(om, gamma - 1.0f) : 0.f;
    if (dx) *dx = dgf_dom * (-(2.0f * t - 1.0f) * pr * (1.0f - pr)) * af;
    if (dt) *dt = dgf_dom * (-(2.0f * pr - 1.0f)) * af + gf * (2.0f * alpha - 1.0f);
    return gf * af;
}

// gpu_CIoU of xyxy boxes (utils/bbox_tools.py:286-339 of the reference, eps 1e-9) + gradient w.r.t. b1, alpha constant:
// the YOLOv5 and YOLOv8 box terms and yh_iou_pairwise kind 2
static __device__ float ciou_fwd_bwd(const float* b1, const float* b2, float* g /*4 or null*/)
{
    const float eps = 1e-9f;
    const float x1 = b1[0], y1 = b1[1], x2 = b1[2], y2 = b1[3];
    const float X1 = b2[0], Y1 = b2[1], X2 = b2[2], Y2 = b2[3];
    const float w1 = x2 - x1, h1 = y2 - y1, w2 = X2 - X1, h2 = Y2 - Y1;
    const float ixmax = fminf(x2, X2), ixmin = fmaxf(x1, X1);
    const float iymax = fminf(y2, Y2), iymin = fmaxf(y1, Y1);
    const float iwr = ixmax - ixmin, ihr = iymax - iymin;
    const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
    const float inter = iw * ih;
    const float union_raw = w1 * h1 + w2 * h2 - inter;
    const float uni = fmaxf(union_raw, eps);
    const float iou = inter / uni;
    const float cxmin = fminf(x1, X1), cxmax = fmaxf(x2, X2);
    const float cymin = fminf(y1, Y1), cymax = fmaxf(y2, Y2);
    const float c_hs = cymax - cymin, c_ws = cxmax - cxmin;
    const float cd_raw = c_ws * c_ws + c_hs * c_hs;
    const float c1x = (x1 + x2) / 2.f, c1y = (y1 + y2) / 2.f;
    const float c2x = (X1 + X2) / 2.f, c2y = (Y1 + Y2) / 2.f;
    const float ctr_ws = c1x - c2x, ctr_hs = c1y - c2y;
    const float ctr = ctr_hs * ctr_hs + ctr_ws * ctr_ws;
    const float kk = (float)(4.0 / (3.14159265358979323846 * 3.14159265358979323846));
    const float h1c = fmaxf(h1, eps), h2c = fmaxf(h2, eps);
    const float u1 = w1 / h1c;
    const float dA = atanf(u1) - atanf(w2 / h2c);
    const float v = kk * dA * dA;
    const float alpha = v / fmaxf(1.f - iou + v, eps);
    const float cd = fmaxf(cd_raw, eps);
    const float ciou = iou - (ctr / cd + v * alpha);
    if (g) {
        // order of unknowns: x1, y1, x2, y2
        // torch.min/max split the gradient evenly on ties (minimum/maximum backward); clamp(min=0) passes at >= 0
        auto lt = [](float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); };
        const float pw_ = (iwr >= 0.f) ? 1.f : 0.f, ph_ = (ihr >= 0.f) ? 1.f : 0.f;
        const float diw[4] = {-pw_ * lt(X1, x1), 0.f, pw_ * lt(x2, X2), 0.f};
        const float dih[4] = {0.f, -ph_ * lt(Y1, y1), 0.f, ph_ * lt(y2, Y2)};
        const float dw1[4] = {-1.f, 0.f, 1.f, 0.f};
        const float dh1[4] = {0.f, -1.f, 0.f, 1.f};
        const float dcw[4] = {-lt(x1, X1), 0.f, lt(X2, x2), 0.f};
        const float dch[4] = {0.f, -lt(y1, Y1), 0.f, lt(Y2, y2)};
        const float dcx[4] = {0.5f, 0.f, 0.5f, 0.f};
        const float dcy[4] = {0.f, 0.5f, 0.f, 0.5f};
        const float du_dw = 1.f / h1c;
        const float du_dh = (h1 >= eps) ? -w1 / (h1c * h1c) : 0.f;
        const float datan = 1.f / (1.f + u1 * u1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float dinter = ih * diw[i] + iw * dih[i];
            const float dunion = (union_raw >= eps) ? (dw1[i] * h1 + w1 * dh1[i] - dinter) : 0.f;
            const float diou = (dinter * uni - inter * dunion) / (uni * uni);
            const float dcd = (cd_raw >= eps) ? (2.f * c_ws * dcw[i] + 2.f * c_hs * dch[i]) : 0.f;
            const float dctr = 2.f * ctr_ws * dcx[i] + 2.f * ctr_hs * dcy[i];
            const float dterm = (dctr * cd - ctr * dcd) / (cd * cd);
            const float dv = 2.f * kk * dA * datan * (du_dw * dw1[i] + du_dh * dh1[i]);
            g[i] = diou - dterm - alpha * dv;
        }
    }
    return ciou;
}

// K fp64 accumulators of a 256-thread block (four waves) -> sred[k][wave]; after the barrier block_total(sred[k]) is the block's
// sum of accumulator k, the four wave slots added in index order 0+1+2+3: that fixed order makes the losses deterministic
template <int K>
__device__ __forceinline__ void block_partials(const double (&acc)[K], double (&sred)[K][4]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double a = wave_sum_d(acc[k]);
        if ((threadIdx.x & 63) == 0) sred[k][threadIdx.x >> 6] = a;
    }
    __syncthreads();
}
__device__ __forceinline__ double block_total(const double (&s)[4]) { return s[0] + s[1] + s[2] + s[3]; }
