// Flat parameter-arena kernels: index-map gather between the fp32 master parameters
// (PyTorch OIHW layout, state_dict compatible) and the packed bf16 weight images read
// by the convolution kernels (conv_igemm.hip plans them), plus the optimizer-side streaming kernels (SGD-nesterov and Adam with
// per-element parameter groups, grad-norm, EMA) of train_yolov5.py:258-280,342-350 and
// trainer/ema_model.py:20-28.  All HBM-bound, one launch per step each.
#include "common.h"
#include <stdarg.h>

namespace {
constexpr int TH = 256;
inline int grid_for(long n) {
    long g = (n + TH - 1) / TH;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (int)g;
}

// eight elements per thread: two 16-byte index loads, eight gathered floats in flight, ONE 16-byte store (a 2-byte store per lane
// wrote 128 bytes per wave instruction: 77 us per step for the 18 MB of YOLOv5s' packed weights); the tail and unaligned
// destinations take the scalar path
__global__ void pack_bf16_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx, long n, uint16_t* __restrict__ dst)
{
    const long n8 = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(idx)) & 15) ? 0 : n >> 3;
    for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < n8; c += (long)gridDim.x * blockDim.x) {
        const int4 j0 = *reinterpret_cast<const int4*>(idx + c * 8), j1 = *reinterpret_cast<const int4*>(idx + c * 8 + 4);
        const int j[8] = {j0.x, j0.y, j0.z, j0.w, j1.x, j1.y, j1.z, j1.w};
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = j[e] >= 0 ? src[j[e]] : 0.f;
        uint4 v;
        v.x = (uint32_t)f2bf(f[0]) | ((uint32_t)f2bf(f[1]) << 16);
        v.y = (uint32_t)f2bf(f[2]) | ((uint32_t)f2bf(f[3]) << 16);
        v.z = (uint32_t)f2bf(f[4]) | ((uint32_t)f2bf(f[5]) << 16);
        v.w = (uint32_t)f2bf(f[6]) | ((uint32_t)f2bf(f[7]) << 16);
        *reinterpret_cast<uint4*>(dst + c * 8) = v;
    }
    for (long i = n8 * 8 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int32_t j = idx[i];
        dst[i] = j >= 0 ? f2bf(src[j]) : (uint16_t)0;
    }
}
__global__ void gather_f32_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx, long n, float* __restrict__ dst)
{
    const long n4 = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(idx)) & 15) ? 0 : n >> 2;      // four per thread: 16-byte stores
    for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < n4; c += (long)gridDim.x * blockDim.x) {
        const int4 j = *reinterpret_cast<const int4*>(idx + c * 4);
        float4 v;
        v.x = j.x >= 0 ? src[j.x] : 0.f; v.y = j.y >= 0 ? src[j.y] : 0.f; v.z = j.z >= 0 ? src[j.z] : 0.f; v.w = j.w >= 0 ? src[j.w] : 0.f;
        *reinterpret_cast<float4*>(dst + c * 4) = v;
    }
    for (long i = n4 * 4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int32_t j = idx[i];
        dst[i] = j >= 0 ? src[j] : 0.f;
    }
}
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                           const uint8_t* __restrict__ group, long n, const float* __restrict__ lr,
                           const float* __restrict__ wd, float momentum, int nesterov, int first,
                           const float* __restrict__ grad_scale)
{
    const float gs = grad_scale ? *grad_scale : 1.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int gi = group ? group[i] : 0;
        float pv = p[i];
        float gv = g[i] * gs + wd[gi] * pv;
        float b = first ? gv : momentum * buf[i] + gv;
        buf[i] = b;
        float upd = nesterov ? gv + momentum * b : b;
        p[i] = pv - lr[gi] * upd;
    }
}
// same update with the per-step scalars read from device memory (scal = lr[0..2] | wd[0..2] | momentum | first-step flag):
// nothing about the step is baked into the launch arguments, so a captured hipGraph replays with the values the host wrote
// into `scal` before the replay (warm-up of lr / momentum, train_yolov5.py:437-456)
__global__ void sgd_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                               const uint8_t* __restrict__ group, long n, const float* __restrict__ scal, int nesterov,
                               const float* __restrict__ grad_scale)
{
    const float gs = grad_scale ? *grad_scale : 1.f;
    const float lr[3] = {scal[0], scal[1], scal[2]}, wd[3] = {scal[3], scal[4], scal[5]};
    const float momentum = scal[6];
    const bool first = scal[7] != 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int gi = group ? group[i] : 0;
        gi = gi > 2 ? 2 : gi;
        float pv = p[i];
        float gv = g[i] * gs + (gi == 0 ? wd[0] : (gi == 1 ? wd[1] : wd[2])) * pv;
        float b = first ? gv : momentum * buf[i] + gv;
        buf[i] = b;
        float upd = nesterov ? gv + momentum * b : b;
        p[i] = pv - (gi == 0 ? lr[0] : (gi == 1 ? lr[1] : lr[2])) * upd;
    }
}
// ---- Adam (torch.optim.Adam: no amsgrad, L2 weight decay folded into the gradient) ------------------------------------------
// device block of yh_adam_step_dev / yh_adam_advance, 16 floats (include/yolohip.h):
//   [0..2] lr | [3..5] wd | [6] beta1 | [7] beta2 | [8] eps | [9] bc1 = 1 - beta1^t | [10] sqrt(1 - beta2^t) | [11] reserved |
//   [12..13] int64 step count t | [14..15] reserved
constexpr int ADAM_LR = 0, ADAM_WD = 3, ADAM_B1 = 6, ADAM_B2 = 7, ADAM_EPS = 8, ADAM_BC1 = 9, ADAM_SBC2 = 10, ADAM_T = 12;
constexpr int ADAM_UNROLL = 2;       // 16-byte chunks per thread and iteration: 8 loads of 16 bytes in flight per lane (88 VGPRs)
constexpr int ADAM_BLOCKS = 1280;    // 5 workgroups of 4 waves per CU, the resident set at that register count; caps from 768 to none
                                     // measured inside the process-to-process spread at 7.2 M and 46.6 M elements
struct AdamConst {
    float gs, wd[3], step[3], b2, omb1, omb2, sbc2, eps;
};
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, int gi, const AdamConst& c)
{
    gi = gi > 2 ? 2 : gi;
    const float gv = g * c.gs + (gi == 0 ? c.wd[0] : (gi == 1 ? c.wd[1] : c.wd[2])) * p;
    m = m + c.omb1 * (gv - m);                               // torch's lerp_(grad, 1 - beta1)
    v = c.b2 * v + c.omb2 * gv * gv;
    const float denom = sqrtf(v) / c.sbc2 + c.eps;
    p = p - (gi == 0 ? c.step[0] : (gi == 1 ? c.step[1] : c.step[2])) * (m / denom);
}
__device__ __forceinline__ void adam_chunk(float4& P, const float4& G, float4& M, float4& V, uint32_t gw, const AdamConst& c)
{
    adam_elem(P.x, G.x, M.x, V.x, gw & 255, c);
    adam_elem(P.y, G.y, M.y, V.y, (gw >> 8) & 255, c);
    adam_elem(P.z, G.z, M.z, V.z, (gw >> 16) & 255, c);
    adam_elem(P.w, G.w, M.w, V.w, gw >> 24, c);
}
// the four group bytes of elements i..i+3 as one word (byte e = element i + e)
__device__ __forceinline__ uint32_t adam_groups(const uint8_t* __restrict__ group, long i, bool word_ok)
{
    if (!group) return 0u;
    if (word_ok) return *reinterpret_cast<const uint32_t*>(group + i);
    return (uint32_t)group[i] | ((uint32_t)group[i + 1] << 8) | ((uint32_t)group[i + 2] << 16) | ((uint32_t)group[i + 3] << 24);
}
// One streaming pass, 16 B read and 12 B written per element plus the group byte.  Every per-step scalar comes from `blk` (and
// grad_scale), none from the launch arguments, for the reason given above sgd_dev_kernel.  Layout of the pass: a scalar head up to
// the first 16-byte boundary of p, 16-byte loads / stores of p, g, m, v from there (ADAM_UNROLL chunks per thread issued before the
// first use), a scalar tail.  The body needs g, m and v at p's phase within 16 bytes; any other combination runs the scalar loop
// over all n.  The arithmetic stays scalar fp32 (no packed forms: Makefile, EXACT).
__global__ __launch_bounds__(TH) void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, const uint8_t* __restrict__ group, long n,
                                                      const float* __restrict__ blk, const float* __restrict__ grad_scale)
{
    AdamConst c;
    c.gs = grad_scale ? *grad_scale : 1.f;
    const float b1 = blk[ADAM_B1], bc1 = blk[ADAM_BC1];
    c.b2 = blk[ADAM_B2];
    c.omb1 = (float)(1.0 - (double)b1);                      // torch rounds the Python double 1 - beta once
    c.omb2 = (float)(1.0 - (double)c.b2);
    c.sbc2 = blk[ADAM_SBC2];
    c.eps = blk[ADAM_EPS];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c.wd[k] = blk[ADAM_WD + k];
        c.step[k] = blk[ADAM_LR + k] / bc1;
    }
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    const uintptr_t ap = reinterpret_cast<uintptr_t>(p);
    const bool same = ((ap & 3) | (((reinterpret_cast<uintptr_t>(g) ^ ap) | (reinterpret_cast<uintptr_t>(m) ^ ap) |
                                    (reinterpret_cast<uintptr_t>(v) ^ ap)) & 15)) == 0;
    long head = same ? (long)(((16 - (ap & 15)) & 15) >> 2) : n;
    head = head < n ? head : n;
    for (long i = tid; i < head; i += nth) {
        float pv = p[i], mv = m[i], vv = v[i];
        adam_elem(pv, g[i], mv, vv, group ? group[i] : 0, c);
        p[i] = pv; m[i] = mv; v[i] = vv;
    }
    if (!same) return;
    const long n4 = (n - head) >> 2;
    float4* p4 = reinterpret_cast<float4*>(p + head);
    const float4* g4 = reinterpret_cast<const float4*>(g + head);
    float4* m4 = reinterpret_cast<float4*>(m + head);
    float4* v4 = reinterpret_cast<float4*>(v + head);
    const uint8_t* gr = group ? group + head : nullptr;
    const bool word_ok = (reinterpret_cast<uintptr_t>(gr) & 3) == 0;
    long ch = tid;
    for (; ch + (ADAM_UNROLL - 1) * nth < n4; ch += ADAM_UNROLL * nth) {
        float4 P[ADAM_UNROLL], G[ADAM_UNROLL], M[ADAM_UNROLL], V[ADAM_UNROLL];
        uint32_t gw[ADAM_UNROLL];
#pragma unroll
        for (int u = 0; u < ADAM_UNROLL; ++u) {
            const long cu = ch + u * nth;
            P[u] = p4[cu]; G[u] = g4[cu]; M[u] = m4[cu]; V[u] = v4[cu];
            gw[u] = adam_groups(gr, cu * 4, word_ok);
        }
#pragma unroll
        for (int u = 0; u < ADAM_UNROLL; ++u) {
            const long cu = ch + u * nth;
            adam_chunk(P[u], G[u], M[u], V[u], gw[u], c);
            p4[cu] = P[u]; m4[cu] = M[u]; v4[cu] = V[u];
        }
    }
    for (; ch < n4; ch += nth) {
        float4 P = p4[ch], M = m4[ch], V = v4[ch];
        adam_chunk(P, g4[ch], M, V, adam_groups(gr, ch * 4, word_ok), c);
        p4[ch] = P; m4[ch] = M; v4[ch] = V;
    }
    for (long i = head + n4 * 4 + tid; i < n; i += nth) {
        float pv = p[i], mv = m[i], vv = v[i];
        adam_elem(pv, g[i], mv, vv, group ? group[i] : 0, c);
        p[i] = pv; m[i] = mv; v[i] = vv;
    }
}
// the step count of Adam kept on the device, like the EMA's below: one thread advances t and writes the two bias corrections of
// THIS step, evaluated in double from the betas the block holds (torch: 1 - beta1 ** step, (1 - beta2 ** step) ** 0.5 in Python floats)
__global__ void adam_advance_kernel(float* __restrict__ blk)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        long long* cnt = reinterpret_cast<long long*>(blk + ADAM_T);
        const long long t = cnt[0] + 1;
        cnt[0] = t;
        const double b1 = (double)blk[ADAM_B1], b2 = (double)blk[ADAM_B2];
        blk[ADAM_BC1] = (float)(1.0 - pow(b1, (double)t));
        blk[ADAM_SBC2] = (float)sqrt(1.0 - pow(b2, (double)t));
    }
}
__global__ void ema_dev_kernel(float* __restrict__ e, const float* __restrict__ p, long n, const float* __restrict__ decay_dev)
{
    const float decay = *decay_dev;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        e[i] = decay * e[i] + (1.f - decay) * p[i];
}
// EMA decay schedule kept on the device (trainer/ema_model.py:12: decay = ratio * (1 - exp(-n / tau)), n = update count):
// one thread advances the counter and writes the decay of THIS update, evaluated in double like the reference's Python float
__global__ void ema_advance_kernel(long long* __restrict__ counter, float* __restrict__ decay, double ratio, double tau)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const long long n = counter[0] + 1;
        counter[0] = n;
        decay[0] = (float)(ratio * (1.0 - exp(-(double)n / tau)));
    }
}
__global__ __launch_bounds__(TH) void sumsq_part_kernel(const float* __restrict__ x, long n, float* __restrict__ part)
{
    __shared__ double sw[TH / 64];
    double s = 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float v = x[i];
        s += (double)v * (double)v;
    }
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tsum = 0.0;
        for (int w = 0; w < TH / 64; ++w) tsum += sw[w];
        part[blockIdx.x] = (float)tsum;
    }
}
__global__ __launch_bounds__(256) void sum_final_kernel(const float* __restrict__ part, int nb, float* out)
{
    __shared__ double sw[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) s += (double)part[i];
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = (float)(sw[0] + sw[1] + sw[2] + sw[3]);
}
__global__ void clip_scale_kernel(const float* sumsq, float max_norm, float* out)
{
    // torch.nn.utils.clip_grad_norm_: coef = max_norm / (total_norm + 1e-6), clamped to 1
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float c = max_norm / (sqrtf(*sumsq) + 1e-6f);
        *out = c < 1.f ? c : 1.f;
    }
}
__global__ void ema_kernel(float* __restrict__ e, const float* __restrict__ p, long n, float decay)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        e[i] = decay * e[i] + (1.f - decay) * p[i];
}
}  // namespace

// ---- error plumbing shared by every translation unit ------------------------
static thread_local char g_err[512] = "";
void yh_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* yh_last_error(void) { return g_err; }
extern "C" int yh_version(void) { return 100; }
extern "C" int yh_device_cus(void) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
    return prop.multiProcessorCount;
}

extern "C" int yh_pack_bf16(const float* src, const int32_t* idx, int64_t n, yh_bf16* dst, yh_stream stream)
{
    YH_CHECK_ARG(src && idx && dst && n >= 0, "yh_pack_bf16: bad args");
    if (n == 0) return YH_OK;
    hipLaunchKernelGGL(pack_bf16_kernel, dim3(grid_for(n)), dim3(TH), 0, (hipStream_t)stream, src, idx, (long)n, dst);
    YH_CHECK_LAUNCH("yh_pack_bf16");
    return YH_OK;
}
extern "C" int yh_gather_f32(const float* src, const int32_t* idx, int64_t n, float* dst, yh_stream stream)
{
    YH_CHECK_ARG(src && idx && dst && n >= 0, "yh_gather_f32: bad args");
    if (n == 0) return YH_OK;
    hipLaunchKernelGGL(gather_f32_kernel, dim3(grid_for(n)), dim3(TH), 0, (hipStream_t)stream, src, idx, (long)n, dst);
    YH_CHECK_LAUNCH("yh_gather_f32");
    return YH_OK;
}
extern "C" int yh_sgd_step(float* p, const float* g, float* buf, const uint8_t* group, int64_t n,
                           const float* lr, const float* wd, int ngroups, float momentum, int nesterov,
                           int first_step, const float* grad_scale, yh_stream stream)
{
    YH_CHECK_ARG(p && g && buf && lr && wd && n >= 0 && ngroups >= 1 && ngroups <= 256, "yh_sgd_step: bad args");
    if (n == 0) return YH_OK;
    hipLaunchKernelGGL(sgd_kernel, dim3(grid_for(n)), dim3(TH), 0, (hipStream_t)stream,
                       p, g, buf, group, (long)n, lr, wd, momentum, nesterov, first_step, grad_scale);
    YH_CHECK_LAUNCH("yh_sgd_step");
    return YH_OK;
}
extern "C" int yh_sgd_step_dev(float* p, const float* g, float* buf, const uint8_t* group, int64_t n,
                               const float* scal, int nesterov, const float* grad_scale, yh_stream stream)
{
    YH_CHECK_ARG(p && g && buf && scal && n >= 0, "yh_sgd_step_dev: bad args");
    if (n == 0) return YH_OK;
    hipLaunchKernelGGL(sgd_dev_kernel, dim3(grid_for(n)), dim3(TH), 0, (hipStream_t)stream, p, g, buf, group, (long)n, scal, nesterov, grad_scale);
    YH_CHECK_LAUNCH("yh_sgd_step_dev");
    return YH_OK;
}
extern "C" int yh_adam_advance(float* blk, yh_stream stream)
{
    YH_CHECK_ARG(blk && (reinterpret_cast<uintptr_t>(blk) & 7) == 0, "yh_adam_advance: bad args (the block is 16 floats, 8-byte aligned)");
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, blk);
    YH_CHECK_LAUNCH("yh_adam_advance");
    return YH_OK;
}
extern "C" int yh_adam_step_dev(float* p, const float* g, float* m, float* v, const uint8_t* group, int64_t n,
                                const float* blk, const float* grad_scale, yh_stream stream)
{
    YH_CHECK_ARG(p && g && m && v && blk && n >= 0, "yh_adam_step_dev: bad args");
    if (n == 0) return YH_OK;
    // one workgroup per TH * ADAM_UNROLL chunks of 16 bytes, capped: a full grid pass is ADAM_BLOCKS * TH * 4 * ADAM_UNROLL elements
    long blocks = ((long)n / 4 + (long)TH * ADAM_UNROLL - 1) / ((long)TH * ADAM_UNROLL);
    blocks = blocks > ADAM_BLOCKS ? ADAM_BLOCKS : (blocks < 1 ? 1 : blocks);
    hipLaunchKernelGGL(adam_dev_kernel, dim3((int)blocks), dim3(TH), 0, (hipStream_t)stream, p, g, m, v, group, (long)n, blk, grad_scale);
    YH_CHECK_LAUNCH("yh_adam_step_dev");
    return YH_OK;
}
extern "C" int yh_ema_update_dev(float* ema, const float* p, int64_t n, const float* decay_dev, yh_stream stream)
{
    YH_CHECK_ARG(ema && p && decay_dev && n >= 0, "yh_ema_update_dev: bad args");
    if (n == 0) return YH_OK;
    hipLaunchKernelGGL(ema_dev_kernel, dim3(grid_for(n)), dim3(TH), 0, (hipStream_t)stream, ema, p, (long)n, decay_dev);
    YH_CHECK_LAUNCH("yh_ema_update_dev");
    return YH_OK;
}
extern "C" int yh_ema_advance(int64_t* counter, float* decay, double ratio, double tau, yh_stream stream)
{
    YH_CHECK_ARG(counter && decay && tau > 0.0, "yh_ema_advance: bad args");
    hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)counter, decay, ratio, tau);
    YH_CHECK_LAUNCH("yh_ema_advance");
    return YH_OK;
}
extern "C" int yh_sumsq(const float* x, int64_t n, float* part, float* out, yh_stream stream)
{
    YH_CHECK_ARG(x && part && out && n > 0, "yh_sumsq: bad args (part needs 4096 floats)");
    int nb = grid_for(n);
    hipLaunchKernelGGL(sumsq_part_kernel, dim3(nb), dim3(TH), 0, (hipStream_t)stream, x, (long)n, part);
    hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, nb, out);
    YH_CHECK_LAUNCH("yh_sumsq");
    return YH_OK;
}
extern "C" int yh_ema_update(float* ema, const float* p, int64_t n, float decay, yh_stream stream)
{
    YH_CHECK_ARG(ema && p && n >= 0, "yh_ema_update: bad args");
    if (n == 0) return YH_OK;
    hipLaunchKernelGGL(ema_kernel, dim3(grid_for(n)), dim3(TH), 0, (hipStream_t)stream, ema, p, (long)n, decay);
    YH_CHECK_LAUNCH("yh_ema_update");
    return YH_OK;
}

extern "C" int yh_clip_scale(const float* sumsq, float max_norm, float* out, yh_stream stream)
{
    YH_CHECK_ARG(sumsq && out && max_norm > 0.f, "yh_clip_scale: bad args");
    hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sumsq, max_norm, out);
    YH_CHECK_LAUNCH("yh_clip_scale");
    return YH_OK;
}
