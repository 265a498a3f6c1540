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

// ---------------------------------------------------------------------------------------------------------------- yh_val_ap
// The rest of the metric: the match table of a whole pass (conf, cls, tp as MatchAccumulator holds them) to the per-class AP and the
// precision / recall curves of utils/mAP.py compute_ap_per_class / compute_ap, so that a pass returns num_class * (n_thr + 2 * n_pr)
// doubles instead of the table.  The rows come ordered (`order`: class ascending, then conf descending; the caller sorts).
//
// Operation order, every operation a correctly rounded fp64 operation, once.  Class c with T = gt_hist[c] > 0 and n > 0 rows, row i
// of its segment (0-based), threshold k:
//   ctp_i = rows <= i with bit k set (integer)      rec_i = (double)ctp_i / ((double)T + 1e-16)
//   pre_i = (double)ctp_i / ((double)(i + 1) + 1e-16)                          (ctp_i + cfp_i is the integer i + 1)
//   AP      rec' = [0, rec.., 1], pre' = [1, pre.., 0], env_j = max over m >= j of pre'_m, ys_q = interp(xs_ap[q]; rec', env),
//           ap = sum over q of ((ys_{q+1} + ys_q) / 2) * (xs_ap[q+1] - xs_ap[q]), added left to right from q = 0
//   curves  (threshold 0)  recall[q] = interp(-xs_pr[q]; -(double)conf, rec, left = 0), precision[q] likewise with pre, left = 1
//   interp  NumPy's: x < xp[0] -> left (default fp[0]); x > xp[last] -> fp[last]; else j = the last index with xp[j] <= x and the
//           result is fp[j] if x == xp[j], else ((fp[j+1] - fp[j]) / (xp[j+1] - xp[j])) * (x - xp[j]) + fp[j]
// Outside the contract: two rows of one class with equal conf and different tp masks (the host's order there comes from an unstable
// sort; with the stable sort of MatchAccumulator.finish_ap the lower original row comes first), NaN or negative conf, a grid that is
// not ascending, a class with more true positives than ground truth (rec' would not be sorted).  None of them can make the kernel
// read or write out of bounds: every index into a table is bounded by construction and an entry of `order` is clamped to [0, N).
//
// One workgroup of four waves per (class, threshold).  Two lanes find the class's segment by binary search in cls[order[.]].  The
// segment is walked forward VA_CHUNK rows at a time: a ballot and a popcount are the wave's inclusive scan of bit k, the waves'
// totals and the chunks' carry go through LDS, ctp goes to the workspace ([n_thr][N] int32).  rec' / pre' are then walked backward
// in chunks for the envelope (a shuffle suffix-max per wave, the carry from the chunks behind); rec' is non-decreasing, so index j
// answers exactly the grid points in [rec'_j, rec'_{j+1}): the lane that holds j looks them up in the grid (LDS) and writes their
// ys, no envelope is stored.  The k = 0 workgroup also writes the two curves, a binary search in the segment's conf per grid point.
#define VA_THREADS 256
#define VA_CHUNK 256                        // rows per step of either walk: one per thread
#define VA_MAX_AP 1024                      // n_ap at most: the grid and its ys live in LDS (16 KiB)

__device__ __forceinline__ int va_row(const int32_t* __restrict__ order, int i, int N) { return min(max(order[i], 0), N - 1); }

// the inner branch of NumPy's interp: (slope) * (x - x0) + f0, three roundings and a division, never fused
__device__ __forceinline__ double va_lerp(double f0, double f1, double x0, double x1, double x)
{
    return __dadd_rn(__dmul_rn(__ddiv_rn(__dsub_rn(f1, f0), __dsub_rn(x1, x0)), __dsub_rn(x, x0)), f0);
}

__global__ __launch_bounds__(VA_THREADS) void val_ap_kernel(
    const float* __restrict__ conf, const int32_t* __restrict__ cls, const uint16_t* __restrict__ tp, const int32_t* __restrict__ order,
    int N, const int32_t* __restrict__ gt_hist, int n_thr, const double* __restrict__ xs_ap, int n_ap, const double* __restrict__ xs_pr,
    int n_pr, int32_t* ctp_ws, double* __restrict__ ap, double* __restrict__ precision, double* __restrict__ recall,
    int32_t* __restrict__ npred)
{
    __shared__ double s_xs[VA_MAX_AP], s_ys[VA_MAX_AP];
    __shared__ double s_env[VA_CHUNK + 1], s_rec[VA_CHUNK + 1];       // [VA_CHUNK]: the first element of the chunk behind
    __shared__ double s_wmax[VA_THREADS / 64];
    __shared__ int s_wsum[VA_THREADS / 64];
    __shared__ int s_seg[2];
    const int c = blockIdx.x, k = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;

    if (t < 2) {                                                      // the first row of class c (t = 0) and of class c + 1 (t = 1)
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (cls[va_row(order, mid, N)] < c + t) lo = mid + 1; else hi = mid;
        }
        s_seg[t] = lo;
    }
    __syncthreads();
    const int s = s_seg[0], n = s_seg[1] - s_seg[0];
    const int T = gt_hist[c];
    if (k == 0 && t == 0) npred[c] = max(n, 0);
    if (n <= 0 || T <= 0) {                                           // uniform: nothing to rank, or nothing to find
        if (t == 0) ap[(long)c * n_thr + k] = 0.0;
        if (k == 0)
            for (int q = t; q < n_pr; q += VA_THREADS) precision[(long)c * n_pr + q] = recall[(long)c * n_pr + q] = 0.0;
        return;
    }
    const double t_den = __dadd_rn((double)T, 1e-16);

    // ---- forward: ctp of every row of the segment
    int32_t* ctp = ctp_ws + (long)k * N + s;
    int carry = 0;
    for (int base = 0; base < n; base += VA_CHUNK) {
        const int i = base + t;
        const int bit = i < n ? (tp[va_row(order, s + i, N)] >> k) & 1 : 0;
        const unsigned long long m = __ballot(bit);
        const int incl = __popcll(m & (~0ull >> (63 - lane)));
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        int before = carry;
        for (int w = 0; w < VA_THREADS / 64; ++w) {
            if (w < wave) before += s_wsum[w];
            carry += s_wsum[w];
        }
        if (i < n) ctp[i] = before + incl;
        __syncthreads();                                              // the totals have been read; after the last chunk: ctp is written
    }

    // ---- the curves, threshold 0: one grid point per thread, a binary search in the segment's conf
    if (k == 0)
        for (int q = t; q < n_pr; q += VA_THREADS) {
            const double x = -xs_pr[q];
            const double x_first = -(double)conf[va_row(order, s, N)], x_last = -(double)conf[va_row(order, s + n - 1, N)];
            double r, p;
            if (x < x_first) {
                r = 0.0; p = 1.0;
            } else {
                int j = n - 1;
                if (!(x > x_last)) {                                  // the last j with xp[j] <= x
                    int lo = 0, hi = n;
                    while (lo < hi) {
                        const int mid = lo + ((hi - lo) >> 1);
                        if (-(double)conf[va_row(order, s + mid, N)] <= x) lo = mid + 1; else hi = mid;
                    }
                    j = max(lo - 1, 0);
                }
                const double xj = -(double)conf[va_row(order, s + j, N)];
                const double cj = (double)ctp[j];
                r = __ddiv_rn(cj, t_den);
                p = __ddiv_rn(cj, __dadd_rn((double)(j + 1), 1e-16));
                if (j < n - 1 && xj != x) {
                    const double xn = -(double)conf[va_row(order, s + j + 1, N)], cn = (double)ctp[j + 1];
                    r = va_lerp(r, __ddiv_rn(cn, t_den), xj, xn, x);
                    p = va_lerp(p, __ddiv_rn(cn, __dadd_rn((double)(j + 2), 1e-16)), xj, xn, x);
                }
            }
            recall[(long)c * n_pr + q] = r;
            precision[(long)c * n_pr + q] = p;
        }

    // ---- backward over rec' / pre' (L = n + 2 elements): the envelope, and the ys of the grid points each index answers
    for (int q = t; q < n_ap; q += VA_THREADS) {
        s_xs[q] = xs_ap[q];
        s_ys[q] = 0.0;                                                // x >= 1 = rec'[L - 1]: env[L - 1] = 0
    }
    __syncthreads();
    const int L = n + 2;
    double env_behind = 0.0, rec_behind = 1.0;                        // pre' >= 0 and ends in 0: 0 is the neutral element here
    for (int base = (L - 1) / VA_CHUNK * VA_CHUNK; base >= 0; base -= VA_CHUNK) {
        const int j = base + t;
        double r = 1.0, v = 0.0;                                      // j == L - 1, and the idle lanes behind it
        if (j == 0) {
            r = 0.0; v = 1.0;
        } else if (j < L - 1) {
            const double cj = (double)ctp[j - 1];
            r = __ddiv_rn(cj, t_den);
            v = __ddiv_rn(cj, __dadd_rn((double)j, 1e-16));
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double o = __shfl_down(v, off);
            if (lane + off < 64) v = fmax(v, o);
        }
        if (lane == 0) s_wmax[wave] = v;
        __syncthreads();
        double behind = env_behind;
        for (int w = VA_THREADS / 64 - 1; w > wave; --w) behind = fmax(behind, s_wmax[w]);
        v = fmax(v, behind);
        s_env[t] = v;
        s_rec[t] = r;
        if (t == 0) { s_env[VA_CHUNK] = env_behind; s_rec[VA_CHUNK] = rec_behind; }
        __syncthreads();
        const double r1 = s_rec[t + 1];
        if (j < L - 1 && r < r1) {                                    // grid points in [rec'_j, rec'_{j+1}): j is their last index
            const double v1 = s_env[t + 1];
            int lo = 0, hi = n_ap;
            while (lo < hi) {                                         // the first grid point >= rec'_j
                const int mid = (lo + hi) >> 1;
                if (s_xs[mid] < r) lo = mid + 1; else hi = mid;
            }
            for (int q = lo; q < n_ap && s_xs[q] < r1; ++q) s_ys[q] = s_xs[q] == r ? v : va_lerp(v, v1, r, r1, s_xs[q]);
        }
        env_behind = s_env[0];
        rec_behind = s_rec[0];
        __syncthreads();                                              // the chunk has been read (and, at the end, ys is written)
    }
    for (int q = t; q < n_ap && s_xs[q] < 0.0; q += VA_THREADS) s_ys[q] = env_behind;      // below rec'[0] = 0: left = env[0]
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int q = 0; q + 1 < n_ap; ++q)
            sum = __dadd_rn(sum, __dmul_rn(__ddiv_rn(__dadd_rn(s_ys[q + 1], s_ys[q]), 2.0), __dsub_rn(s_xs[q + 1], s_xs[q])));
        ap[(long)c * n_thr + k] = sum;
    }
}

extern "C" size_t yh_val_ap_ws_bytes(int N, int n_thr) { return N > 0 && n_thr > 0 ? (size_t)N * (size_t)n_thr * sizeof(int32_t) : 0; }

extern "C" int yh_val_ap(const float* conf, const int32_t* cls, const uint16_t* tp, const int32_t* order, int N, const int32_t* gt_hist,
                         int num_class, int n_thr, const double* xs_ap, int n_ap, const double* xs_pr, int n_pr, double* ap,
                         double* precision, double* recall, int32_t* npred, void* ws, yh_stream stream)
{
    YH_CHECK_ARG(conf && cls && tp && order && gt_hist && xs_ap && xs_pr, "yh_val_ap: null input pointer");
    YH_CHECK_ARG(ap && precision && recall && npred && ws, "yh_val_ap: null output or ws pointer");
    YH_CHECK_ARG(N > 0 && num_class > 0, "yh_val_ap: N and num_class must be positive (N=%d num_class=%d)", N, num_class);
    YH_CHECK_ARG(n_thr >= 1 && n_thr <= VM_MAX_THR, "yh_val_ap: n_thr=%d is outside 1..%d", n_thr, VM_MAX_THR);
    YH_CHECK_ARG(n_ap >= 2 && n_ap <= VA_MAX_AP, "yh_val_ap: n_ap=%d is outside 2..%d", n_ap, VA_MAX_AP);
    YH_CHECK_ARG(n_pr >= 1, "yh_val_ap: n_pr=%d must be positive", n_pr);
    YH_CHECK_ARG(((((uintptr_t)conf) | ((uintptr_t)cls) | ((uintptr_t)order) | ((uintptr_t)gt_hist) | ((uintptr_t)npred) | ((uintptr_t)ws)) & 3) == 0 &&
                 (((uintptr_t)tp) & 1) == 0 &&
                 ((((uintptr_t)xs_ap) | ((uintptr_t)xs_pr) | ((uintptr_t)ap) | ((uintptr_t)precision) | ((uintptr_t)recall)) & 7) == 0,
                 "yh_val_ap: unaligned table (conf, cls, order, gt_hist, npred, ws 4 bytes; tp 2 bytes; the double tables 8 bytes)");
    hipLaunchKernelGGL(val_ap_kernel, dim3(num_class, n_thr), dim3(VA_THREADS), 0, (hipStream_t)stream,
                       conf, cls, tp, order, N, gt_hist, n_thr, xs_ap, n_ap, xs_pr, n_pr, (int32_t*)ws, ap, precision, recall, npred);
    YH_CHECK_LAUNCH("yh_val_ap");
    return YH_OK;
}
