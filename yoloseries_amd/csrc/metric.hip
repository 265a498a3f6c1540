// Validation metric on the device: the NMS table of a batch (yh_nms_batched's out / nkeep) and the collate's ground truth, both in
// the letterboxed frame, to the per-detection match table that mAP_v2 consumes — the un-letterbox of val_yolov5.py
// (preds_postprocess / gt_bbox_postprocess) and the true-positive matching of utils/mAP.py compute_tp in one launch, so that a
// validation pass copies one compact table to the host at its end instead of every image's rows.
//
// Operation order, every operation a correctly rounded fp32 operation (this file compiles with the exact flags: no contraction):
//   detection     x' = min(max((x - pad_left) / scale, 1), org_w - 1)      y' = min(max((y - pad_top) / scale, 1), org_h - 1)
//   ground truth  x' = (x - pad_left) / scale                               y' = (y - pad_top) / scale             (no clamp)
//   IoU (iou_np)  a_gt = (x2 - x1) * (y2 - y1),  a_det likewise,  w = max(0, min(x2, X2) - max(x1, X1)),  h likewise,
//                 inter = w * h,  iou = inter / min(max((a_gt + a_det) - inter, 1e-6f), 1e7f)
//   class match   gt_cls == det_cls as floats; a ground-truth row with cls < 0 (or NaN) is padding, wherever it sits
// Matching, compute_tp in closed form: g*(p) is the valid ground truth of p's class with the largest IoU among those with
// (double)iou >= thr[0]; ground truth g is kept by the LOWEST p with g*(p) == g (after the first np.unique of compute_tp the rows
// are ordered by prediction index, so the second keeps the first of them, not the one with the highest IoU); every other detection
// is unmatched.  Exact IoU ties between two ground truths of one detection go through an unstable sort on the host and are outside
// its contract: this kernel takes the lowest ground-truth index.  NaN coordinates are outside the contract too (fmaxf / fminf drop
// a NaN where NumPy propagates it).
//
// One workgroup of four waves per image.  The un-letterboxed ground truth is staged in LDS VM_CHUNK rows at a time (any maxbox runs;
// the collate's lists fit one chunk); one detection per thread, strided over nkeep, loops over the staged rows for g*(p); the
// winner per ground truth is an LDS atomicMin on the detection index; after the barrier behind it the rows are written.  Between
// chunks a detection's best pair lives in its own iou / gt_idx row, which only its thread touches.  Bound by latency, not
// bandwidth: a batch is B workgroups of a few microseconds.
#include "common.h"
#include <limits.h>

#define VM_THREADS 256
#define VM_CHUNK 512                        // ground-truth rows staged per pass: 512 * (16 + 4 + 4) bytes = 12 KiB of LDS
#define VM_MAX_THR 16

struct vm_thr { double v[VM_MAX_THR]; };

__device__ __forceinline__ float vm_unbox(float v, float pad, float scale) { return __fdiv_rn(__fsub_rn(v, pad), scale); }
__device__ __forceinline__ float vm_clamp(float v, float hi) { return fminf(fmaxf(v, 1.f), hi); }

__global__ __launch_bounds__(VM_THREADS) void val_match_kernel(
    const float* __restrict__ det, const int32_t* __restrict__ nkeep, const float* __restrict__ gt, const float* __restrict__ info,
    int max_keep, int maxbox, int gt_ld, int num_class, vm_thr thr, int n_thr,
    float* __restrict__ box, float* __restrict__ conf, int32_t* __restrict__ cls, float* iou, int32_t* gt_idx,
    uint16_t* __restrict__ tp, int32_t* __restrict__ nrow, int32_t* __restrict__ gt_hist)
{
    __shared__ float4 s_box[VM_CHUNK];
    __shared__ float s_cls[VM_CHUNK];
    __shared__ int s_win[VM_CHUNK];
    const int b = blockIdx.x, t = threadIdx.x;
    const int nk = min(max(nkeep[b], 0), max_keep);
    const float* gtb = gt + (long)b * maxbox * gt_ld;
    // an image counts iff it has a detection and a valid ground truth; the classes of a counting image's ground truth are counted
    int any = 0;
    if (nk > 0)
        for (int g = t; g < maxbox; g += VM_THREADS) {
            const float c = gtb[(long)g * gt_ld + 4];
            if (c >= 0.f) {
                any = 1;
                if (c < (float)num_class) atomicAdd(gt_hist + (int)c, 1);
            }
        }
    any = __syncthreads_or(any);
    if (t == 0) nrow[b] = any ? nk : 0;
    if (!any) return;                                                 // uniform: nk and any are the workgroup's

    const float scale = info[b * 5], pad_top = info[b * 5 + 1], pad_left = info[b * 5 + 2];
    const float hi_y = __fsub_rn(info[b * 5 + 3], 1.f), hi_x = __fsub_rn(info[b * 5 + 4], 1.f);
    const long row0 = (long)b * max_keep;

    // ---- g*(p): the best ground truth of every detection, chunk by chunk
    for (int base = 0; base < maxbox; base += VM_CHUNK) {
        const int n = min(VM_CHUNK, maxbox - base);
        if (base) __syncthreads();                                    // the previous chunk has been read
        for (int g = t; g < n; g += VM_THREADS) {
            const float* r = gtb + (long)(base + g) * gt_ld;
            s_box[g] = make_float4(vm_unbox(r[0], pad_left, scale), vm_unbox(r[1], pad_top, scale),
                                   vm_unbox(r[2], pad_left, scale), vm_unbox(r[3], pad_top, scale));
            s_cls[g] = r[4];
        }
        __syncthreads();
        for (int p = t; p < nk; p += VM_THREADS) {
            const float* d = det + (row0 + p) * 6;
            const float x1 = vm_clamp(vm_unbox(d[0], pad_left, scale), hi_x), y1 = vm_clamp(vm_unbox(d[1], pad_top, scale), hi_y);
            const float x2 = vm_clamp(vm_unbox(d[2], pad_left, scale), hi_x), y2 = vm_clamp(vm_unbox(d[3], pad_top, scale), hi_y);
            const float dc = d[5];
            float best = 0.f;
            int bg = -1;
            if (base == 0) {
                float* o = box + (row0 + p) * 4;
                o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2;
                conf[row0 + p] = d[4];
                cls[row0 + p] = (int)dc;
            } else {
                best = iou[row0 + p];
                bg = gt_idx[row0 + p];
            }
            const float a_det = __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));
            for (int g = 0; g < n; ++g) {
                const float gc = s_cls[g];
                if (!(gc >= 0.f) || gc != dc) continue;
                const float4 q = s_box[g];
                const float a_gt = __fmul_rn(__fsub_rn(q.z, q.x), __fsub_rn(q.w, q.y));
                const float w = fmaxf(0.f, __fsub_rn(fminf(q.z, x2), fmaxf(q.x, x1)));
                const float h = fmaxf(0.f, __fsub_rn(fminf(q.w, y2), fmaxf(q.y, y1)));
                const float inter = __fmul_rn(w, h);
                const float uni = fminf(fmaxf(__fsub_rn(__fadd_rn(a_gt, a_det), inter), 1e-6f), 1e7f);
                const float v = __fdiv_rn(inter, uni);
                if ((double)v >= thr.v[0] && v > best) { best = v; bg = base + g; }      // strict: ties keep the lowest index
            }
            iou[row0 + p] = best;
            gt_idx[row0 + p] = bg;
        }
    }

    // ---- one detection per ground truth: the lowest p with g*(p) == g
    for (int base = 0; base < maxbox; base += VM_CHUNK) {
        const int n = min(VM_CHUNK, maxbox - base);
        if (base) __syncthreads();                                    // the previous chunk's winners have been read
        for (int g = t; g < n; g += VM_THREADS) s_win[g] = INT_MAX;
        __syncthreads();
        for (int p = t; p < nk; p += VM_THREADS) {
            const int bg = gt_idx[row0 + p];
            if (bg >= base && bg < base + n) atomicMin(&s_win[bg - base], p);
        }
        __syncthreads();
        for (int p = t; p < nk; p += VM_THREADS) {
            const int bg = gt_idx[row0 + p];
            if (bg < 0) {
                if (base == 0) tp[row0 + p] = 0;                      // unmatched from the start: iou 0, gt_idx -1 are written
                continue;
            }
            if (bg < base || bg >= base + n) continue;
            if (s_win[bg - base] != p) {                              // a lower detection keeps this ground truth
                iou[row0 + p] = 0.f;
                gt_idx[row0 + p] = -1;
                tp[row0 + p] = 0;
                continue;
            }
            const double v = (double)iou[row0 + p];
            unsigned m = 0;
#pragma unroll
            for (int k = 0; k < VM_MAX_THR; ++k) m |= (k < n_thr && v >= thr.v[k] ? 1u : 0u) << k;
            tp[row0 + p] = (uint16_t)m;
        }
    }
}

extern "C" int yh_val_match(const float* det, const int32_t* nkeep, const float* gt, const float* info, int B, int max_keep, int maxbox,
                            int gt_ld, int num_class, const double* thr, int n_thr, float* box, float* conf, int32_t* cls, float* iou,
                            int32_t* gt_idx, uint16_t* tp, int32_t* nrow, int32_t* gt_hist, yh_stream stream)
{
    YH_CHECK_ARG(det && nkeep && gt && info && thr, "yh_val_match: null input pointer");
    YH_CHECK_ARG(box && conf && cls && iou && gt_idx && tp && nrow && gt_hist, "yh_val_match: null output pointer");
    YH_CHECK_ARG(B > 0 && max_keep > 0 && maxbox > 0 && num_class > 0,
                 "yh_val_match: B, max_keep, maxbox, num_class must be positive (B=%d max_keep=%d maxbox=%d num_class=%d)", B, max_keep, maxbox, num_class);
    YH_CHECK_ARG(gt_ld >= 5, "yh_val_match: gt_ld=%d, a ground-truth row is xmin, ymin, xmax, ymax, cls (gt_ld >= 5)", gt_ld);
    YH_CHECK_ARG(n_thr >= 1 && n_thr <= VM_MAX_THR, "yh_val_match: n_thr=%d is outside 1..%d", n_thr, VM_MAX_THR);
    YH_CHECK_ARG((long)B * max_keep <= 0x7fffffffL / 6 && (long)maxbox * gt_ld <= 0x7fffffffL,
                 "yh_val_match: tables too large (B * max_keep = %ld, maxbox * gt_ld = %ld)", (long)B * max_keep, (long)maxbox * gt_ld);
    YH_CHECK_ARG(((((uintptr_t)det) | ((uintptr_t)nkeep) | ((uintptr_t)gt) | ((uintptr_t)info) | ((uintptr_t)box) | ((uintptr_t)conf) |
                   ((uintptr_t)cls) | ((uintptr_t)iou) | ((uintptr_t)gt_idx) | ((uintptr_t)nrow) | ((uintptr_t)gt_hist)) & 3) == 0 &&
                 (((uintptr_t)tp) & 1) == 0, "yh_val_match: unaligned table (4 bytes; tp 2 bytes)");
    vm_thr th;
    for (int k = 0; k < VM_MAX_THR; ++k) th.v[k] = k < n_thr ? thr[k] : 2.0;
    hipLaunchKernelGGL(val_match_kernel, dim3(B), dim3(VM_THREADS), 0, (hipStream_t)stream,
                       det, nkeep, gt, info, max_keep, maxbox, gt_ld, num_class, th, n_thr, box, conf, cls, iou, gt_idx, tp, nrow, gt_hist);
    YH_CHECK_LAUNCH("yh_val_match");
    return YH_OK;
}
