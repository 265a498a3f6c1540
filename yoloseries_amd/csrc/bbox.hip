// Box utilities on gfx950 behind the evaluators and the YOLOX path: yh_iou_matrix (gpu_iou / numba_iou / the evaluators' bbox_iou of
// every pair) and yh_iou_pairwise (GIoU / DIoU / CIoU of matching rows, CIoU with the gradient w.r.t. the first box).
#include "exact_math.h"

namespace {
__global__ void iou_matrix_kernel(const float* __restrict__ b1, int n1, const float* __restrict__ b2, int n2,
                                  float eps_clamp, float* __restrict__ out)
{
    long tot = (long)n1 * n2;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < tot; id += (long)gridDim.x * blockDim.x) {
        int i = (int)(id / n2), j = (int)(id - (long)i * n2);
        const float* a = b1 + (size_t)i * 4;
        const float* b = b2 + (size_t)j * 4;
        const float a1 = (a[2] - a[0]) * (a[3] - a[1]);
        const float a2 = (b[2] - b[0]) * (b[3] - b[1]);
        float w = fminf(a[2], b[2]) - fmaxf(a[0], b[0]);
        float h = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
        if (eps_clamp >= 0.f) { w = fmaxf(w, 0.f); h = fmaxf(h, 0.f); }      // < 0: the evaluators' bbox_iou (trainer/eval_yolov5.py:237-258) clamps nothing
        const float inter = w * h;
        float den = a1 + a2 - inter;
        if (eps_clamp > 0.f) den = fmaxf(den, eps_clamp);      // gpu_iou; 0 -> numba_iou (no clamp, 0/0 = NaN)
        out[id] = inter / den;
    }
}

__global__ void iou_pairwise_kernel(int kind, const float* __restrict__ b1, const float* __restrict__ b2, int n,
                                    float* __restrict__ out, float* __restrict__ grad)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* a = b1 + (size_t)i * 4;
    const float* b = b2 + (size_t)i * 4;
    if (kind == 2) {
        float g[4];
        out[i] = ciou_fwd_bwd(a, b, grad ? g : nullptr);
        if (grad) { grad[i * 4 + 0] = g[0]; grad[i * 4 + 1] = g[1]; grad[i * 4 + 2] = g[2]; grad[i * 4 + 3] = g[3]; }
        return;
    }
    const float eps = 1e-6f;
    const float a1 = (a[2] - a[0]) * (a[3] - a[1]);
    const float a2 = (b[2] - b[0]) * (b[3] - b[1]);
    const float w = fmaxf(fminf(a[2], b[2]) - fmaxf(a[0], b[0]), 0.f);
    const float h = fmaxf(fminf(a[3], b[3]) - fmaxf(a[1], b[1]), 0.f);
    const float inter = w * h;
    const float uni = a1 + a2 - inter;
    const float iou = inter / fmaxf(uni, eps);
    const float cw = fmaxf(a[2], b[2]) - fminf(a[0], b[0]);
    const float chh = fmaxf(a[3], b[3]) - fminf(a[1], b[1]);
    if (kind == 0) {            // GIoU utils/bbox_tools.py:193-230
        const float ca = cw * chh;
        out[i] = iou - fabsf(ca - uni) / fabsf(fmaxf(ca, eps));
    } else {                    // DIoU :233-283
        const float cd = cw * cw + chh * chh;
        const float dx = (a[2] + a[0]) / 2.f - (b[2] + b[0]) / 2.f;
        const float dy = (a[3] + a[1]) / 2.f - (b[3] + b[1]) / 2.f;
        float v = iou - (dx * dx + dy * dy) / fmaxf(cd, eps);
        out[i] = fminf(fmaxf(v, -1.f), 1.f);
    }
}
}  // namespace

extern "C" int yh_iou_matrix(const float* b1, int n1, const float* b2, int n2, float eps_clamp, float* out, yh_stream stream)
{
    YH_CHECK_ARG(b1 && b2 && out && n1 >= 0 && n2 >= 0, "yh_iou_matrix: bad args");
    long tot = (long)n1 * n2;
    if (tot == 0) return YH_OK;
    int g = (int)((tot + 255) / 256 > 4096 ? 4096 : (tot + 255) / 256);
    hipLaunchKernelGGL(iou_matrix_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, b1, n1, b2, n2, eps_clamp, out);
    YH_CHECK_LAUNCH("yh_iou_matrix");
    return YH_OK;
}

extern "C" int yh_iou_pairwise(int kind, const float* b1, const float* b2, int n, float* out, float* grad_b1, yh_stream stream)
{
    YH_CHECK_ARG(b1 && b2 && out && n >= 0 && kind >= 0 && kind <= 2, "yh_iou_pairwise: bad args");
    YH_CHECK_ARG(grad_b1 == nullptr || kind == 2, "yh_iou_pairwise: gradient only for CIoU");
    if (n == 0) return YH_OK;
    hipLaunchKernelGGL(iou_pairwise_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, kind, b1, b2, n, out, grad_b1);
    YH_CHECK_LAUNCH("yh_iou_pairwise");
    return YH_OK;
}
