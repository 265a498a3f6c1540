// YOLOv8 loss on gfx950: task-aligned assignment, CIoU and distribution focal loss (loss/yolov8_loss.py:12-411 of the
// reference, tblr2xyxy / xyxy2tblr of utils/bbox_tools.py:392-426).  Everything here is HBM- or latency-bound; no MFMA.
//
//   pre       per (cell, side): softmax over the side's `reg` logits, expectation with the projection 1..reg (:30,:119),
//             box (gx-l, gy-t, gx+r, gy+b) in grid units with the grid (col+0.5, row+0.5); clears the per-cell claim
//             counters and the per-ground-truth maxima.
//   assign    one workgroup per (image, ground-truth row): walks only the cells whose centre lies inside the box, stage by
//             stage; metric = ciou^beta * sigmoid(class logit)^alpha (:146-177); every thread keeps the `topk` best of its
//             own cells as sorted 64-bit keys (metric bits, inverted cell index) in LDS, the workgroup merges the lists in
//             `topk` rounds of a block arg-max and claims the winners (integer atomics on the per-cell counters).
//   resolve   per claimed cell: a cell claimed more than once goes to the arg-max of the IoU over ALL valid ground truths of
//             the image, also one that did not claim it (:200-220, kept); then metric and IoU of (owner, cell) and their
//             maxima per ground truth (max by bits on non-negative floats).
//   loss_fwd  16-byte chunks of every cell row: class BCE-with-logits (pos_weight) times the focal factor against
//             onehot * norm, norm = metric * max iou / (max metric + 1e-9) (:277); the chunk-0 thread of an assigned cell adds
//             (1 - CIoU) * norm (gpu_CIoU, eps 1e-9, alpha constant) and the DFL cross-entropies * norm (:311-324).
//             Block partials in double, summed in a fixed order by `finalize`: no float atomics anywhere.
//   loss_bwd  the same chunks: writes the whole gradient tensor; class logits everywhere (the focal factor is differentiated
//             through, :56-61), box logits on assigned cells through CIoU -> xyxy -> expectation -> softmax plus the DFL terms.
//
// Nothing scales with B*M*N: the workspace holds 28 bytes per cell and 8 per ground-truth row, `saved` 8 bytes per cell.
//
// Three deliberate departures from the reference:
//   1. Fewer than `topk` positive metrics.  torch.topk fills a ground truth's list up with zero-metric cells in whatever
//      order it leaves ties (also cells outside the box); they get target 0 and weight 0 and change only tar_nums and,
//      rarely, a conflict.  Here only strictly positive metrics are picked: such a ground truth gets fewer cells.  Ties
//      between equal positive metrics go to the lower cell index, stages in the order given.
//   2. Rectangular maps.  make_grid (:327-346) swaps the mesh and views (w, h, 2) as (h, w, 2): right for square maps,
//      scrambled otherwise.  Here x = col + 0.5, y = row + 0.5, stride = img_size0 / H.
//   3. The NaN branch (print and input(), :68-91) is dropped: NaNs propagate into the result.
#include "exact_math.h"

namespace {

constexpr int MAXS = 4;
constexpr int KMAX = 24;           // topk: the per-thread lists of the assignment take topk * 2 KiB of LDS
constexpr int MAXREG = 32;
constexpr int NB = 512;            // blocks along x of the loss kernels, per stage
constexpr int NKIND = 5;           // partial sums: class, iou, dfl, sum of class targets, assigned cells

struct V8Layout {
    size_t owner, norm, den, total;                                    // saved
    size_t w_pbox, w_cnt, w_met, w_iou, w_gmax, w_part, w_total;       // workspace
    int cell_off[MAXS];            // first cell of stage s inside an image's N cells
    int N;
};

V8Layout make_v8layout(const yh_v8loss_desc& d) {
    V8Layout L;
    int n = 0;
    for (int s = 0; s < MAXS; ++s) {
        L.cell_off[s] = n;
        if (s < d.num_stage) n += d.H[s] * d.W[s];
    }
    L.N = n;
    const size_t cells = (size_t)d.B * n, rows = (size_t)d.B * d.maxbox;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    L.owner = take(sizeof(int32_t) * cells);
    L.norm = take(sizeof(float) * cells);
    L.den = take(64);
    L.total = o;
    o = 0;
    L.w_pbox = take(sizeof(float) * 4 * cells);
    L.w_cnt = take(sizeof(int32_t) * cells);
    L.w_met = take(sizeof(float) * cells);
    L.w_iou = take(sizeof(float) * cells);
    L.w_gmax = take(sizeof(uint32_t) * 2 * rows);
    L.w_part = take(sizeof(double) * NKIND * MAXS * NB);
    L.w_total = o;
    return L;
}

struct V8K {
    yh_v8loss_desc d;
    V8Layout L;
};
struct StageV { const void* pred; void* gpred; int H, W, ld, off; float stride; };
struct StagesV { StageV s[MAXS]; };

template <typename T> __device__ __forceinline__ void load8(const T* p, float* f);
template <> __device__ __forceinline__ void load8<float>(const float* p, float* f) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
template <> __device__ __forceinline__ void load8<uint16_t>(const uint16_t* p, float* f) { unpack8(*reinterpret_cast<const uint4*>(p), f); }
template <typename T> __device__ __forceinline__ void store8(T* p, const float* f);
template <> __device__ __forceinline__ void store8<float>(float* p, const float* f) {
    reinterpret_cast<float4*>(p)[0] = make_float4(f[0], f[1], f[2], f[3]);
    reinterpret_cast<float4*>(p)[1] = make_float4(f[4], f[5], f[6], f[7]);
}
template <> __device__ __forceinline__ void store8<uint16_t>(uint16_t* p, const float* f) { *reinterpret_cast<uint4*>(p) = pack8(f); }

// softmax statistics of one side's `reg` logits z[0..reg): mx = max, se = sum exp(z - mx), ex = sum exp(z - mx) * (k + 1).
// vec: reg % 8 == 0, so that every side starts on a 16-byte boundary of the (16-byte aligned, ld % 8 == 0) cell row
template <typename T>
__device__ __forceinline__ void side_stats(const T* z, int reg, bool vec, float& mx, float& se, float& ex)
{
    mx = -INFINITY; se = 0.f; ex = 0.f;
    if (vec) {
        float f[8];
        for (int k0 = 0; k0 < reg; k0 += 8) {
            load8<T>(z + k0, f);
#pragma unroll
            for (int j = 0; j < 8; ++j) mx = fmaxf(mx, f[j]);
        }
        for (int k0 = 0; k0 < reg; k0 += 8) {
            load8<T>(z + k0, f);
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float e = expf(f[j] - mx); se += e; ex += e * (float)(k0 + j + 1); }
        }
    } else {
        for (int k = 0; k < reg; ++k) mx = fmaxf(mx, ldf<T>(z + k));
        for (int k = 0; k < reg; ++k) { const float e = expf(ldf<T>(z + k) - mx); se += e; ex += e * (float)(k + 1); }
    }
}

// sides are [t, b, l, r]; the box slots are [xmin, ymin, xmax, ymax] (tblr2xyxy)
__device__ __forceinline__ float side_coord(int side, float dist, float gx, float gy) {
    return side == 0 ? gy - dist : side == 1 ? gy + dist : side == 2 ? gx - dist : gx + dist;
}
__device__ __forceinline__ int side_slot(int side) { return side == 0 ? 1 : side == 1 ? 3 : side == 2 ? 0 : 2; }

// YOLOV8Loss.ciou (:370-411), eps 1e-6: a = ground truth, b = prediction, both xyxy in pixels.  Assignment only: no gradient.
__device__ __forceinline__ float ciou_assign(const float* a, const float* b)
{
    const float eps = 1e-6f;
    const float w1 = a[2] - a[0], h1 = a[3] - a[1], w2 = b[2] - b[0], h2 = b[3] - b[1];
    const float inter = fmaxf(fminf(a[2], b[2]) - fmaxf(a[0], b[0]), 0.f) * fmaxf(fminf(a[3], b[3]) - fmaxf(a[1], b[1]), 0.f);
    const float uni = fmaxf(fmaxf(w1 * h1, 0.f) + fmaxf(w2 * h2, 0.f) - inter, eps);
    const float iou = inter / uni;
    const float cw = fmaxf(a[2], b[2]) - fminf(a[0], b[0]), ch = fmaxf(a[3], b[3]) - fminf(a[1], b[1]);
    const float diag = fmaxf(ch * ch + cw * cw, eps);
    const float dx = a[2] + a[0] - (b[2] + b[0]), dy = a[3] + a[1] - (b[1] + b[3]);
    const float cd = (dx * dx + dy * dy) / 4.f;
    const float da = atanf(w1 / h1) - atanf(w2 / h2);
    const float v = (float)(4.0 / (3.14159265358979323846 * 3.14159265358979323846)) * (da * da);
    const float alpha = v / fmaxf(1.f - iou + v, eps);
    return iou - (cd / diag + v * alpha);
}

// The class term of one logit: BCE-with-logits with pos_weight times the focal factor of focal_loss_factor (:348-368), and
// (dx) its derivative with the factor differentiated through.  One sigmoid and one power serve both: the derivative of
// om^gamma is gamma * om^gamma / om.
__device__ __forceinline__ float cls_term(const yh_v8loss_desc& d, float x, float t, float* dx) {
    const float pr = sigm(x);
    const float lw = 1.0f + (d.cls_pos_weight - 1.0f) * t;
    const float sp = log1pf(expf(-fabsf(x))) + fmaxf(-x, 0.0f);      // softplus(-x) = -log(sigmoid(x))
    const float l = (1.0f - t) * x + lw * sp;
    const float om = 1.0f - (t * pr + (1.0f - t) * (1.0f - pr));
    // om^gamma for om in [0, 1] as exp2(gamma * log2(om)): about 1e-6 relative where the general powf pays for a range and
    // sign analysis this operand never needs; om == 0 is taken apart so that gamma == 0 still gives 1
    const float gf = om > 0.f ? exp2f(d.focal_gamma * log2f(om)) : (d.focal_gamma == 0.f ? 1.f : 0.f);
    const float af = t * d.focal_alpha + (1.0f - t) * (1.0f - d.focal_alpha);
    const float ff = gf * af;
    if (dx) {
        const float dl = (1.0f - t) - lw * (1.0f - pr);
        const float dff = (om > 0.f ? d.focal_gamma * gf / om : 0.f) * (-(2.0f * t - 1.0f) * pr * (1.0f - pr)) * af;
        *dx = dl * ff + l * dff;
    }
    return l * ff;
}

// One (ground truth, cell) pair of the assignment: is the cell's centre inside the box (:124-144), and if so the clamped CIoU
// of the box with the cell's prediction in pixels and the metric (:164-177).  The assignment and the conflict pass both come
// through here, so they see the same bits.
template <typename T>
__device__ __forceinline__ bool pair_eval(const yh_v8loss_desc& d, const float* tb, int cls, float cx, float cy, float stride,
                                          const float* pbox, const T* row, float& iou, float& metric)
{
    iou = 0.f; metric = 0.f;
    const float l = cx - tb[0], t = cy - tb[1], r = tb[2] - cx, b = tb[3] - cy;
    if (!(fminf(fminf(t, b), fminf(l, r)) > 1e-9f)) return false;
    const float4 q = *reinterpret_cast<const float4*>(pbox);
    const float pb[4] = {q.x * stride, q.y * stride, q.z * stride, q.w * stride};
    iou = fmaxf(ciou_assign(tb, pb), 0.f);
    metric = powf(iou, d.beta) * powf(sigm(ldf<T>(row + 4 * d.reg + cls)), d.alpha);
    return true;
}

__device__ __forceinline__ bool valid_row(const yh_v8loss_desc& d, const float* tg) { return tg[4] >= 0.f && (int)tg[4] < d.num_class; }

// ------------------------------------------------------------------------------------------------
// grid (blocks, stages); one thread per (cell, side)
template <typename T>
__global__ __launch_bounds__(256) void v8_pre_kernel(const V8K p, const StagesV sts, unsigned char* __restrict__ wsb,
                                                     unsigned char* __restrict__ svb)
{
    const StageV st = sts.s[blockIdx.y];
    const yh_v8loss_desc& d = p.d;
    const int n = st.H * st.W;
    const bool vec = d.reg % 8 == 0;
    float* pbox = reinterpret_cast<float*>(wsb + p.L.w_pbox);
    int32_t* cnt = reinterpret_cast<int32_t*>(wsb + p.L.w_cnt);
    int32_t* owner = reinterpret_cast<int32_t*>(svb + p.L.owner);
    const T* pred = reinterpret_cast<const T*>(st.pred);
    const long tot = (long)d.B * n * 4;
    const long step = (long)gridDim.x * 256;
    const long gtid = (long)blockIdx.x * 256 + threadIdx.x;
    for (long i = gtid; i < tot; i += step) {
        const long cell = i >> 2;
        const int side = (int)(i & 3);
        const int b = (int)(cell / n), loc = (int)(cell - (long)b * n);
        float mx, se, ex;
        side_stats<T>(pred + (size_t)cell * st.ld + side * d.reg, d.reg, vec, mx, se, ex);
        const size_t gc = (size_t)b * p.L.N + st.off + loc;
        const float gx = (float)(loc % st.W) + 0.5f, gy = (float)(loc / st.W) + 0.5f;
        pbox[gc * 4 + side_slot(side)] = side_coord(side, ex / se, gx, gy);
        if (side == 0) { cnt[gc] = 0; owner[gc] = -1; }
    }
    if (blockIdx.y == 0) {
        uint32_t* gmax = reinterpret_cast<uint32_t*>(wsb + p.L.w_gmax);
        for (long i = gtid; i < 2l * d.B * d.maxbox; i += step) gmax[i] = 0u;
    }
}

// grid (maxbox, B); dynamic LDS: topk * 256 keys of 8 bytes
template <typename T>
__global__ __launch_bounds__(256) void v8_assign_kernel(const V8K p, const StagesV sts, const float* __restrict__ targets,
                                                        unsigned char* __restrict__ wsb, unsigned char* __restrict__ svb)
{
    extern __shared__ unsigned long long s_list[];          // [k][thread], descending in k; 0 = empty
    __shared__ unsigned long long s_w[2][4];
    const yh_v8loss_desc& d = p.d;
    const int m = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const float* tg = targets + ((size_t)b * d.maxbox + m) * 6;
    if (!valid_row(d, tg)) return;                          // block-uniform
    const float tb[4] = {tg[0], tg[1], tg[2], tg[3]};
    const int cls = (int)tg[4];
    const int K = d.topk;
    const float* pbox = reinterpret_cast<const float*>(wsb + p.L.w_pbox) + (size_t)b * p.L.N * 4;
    int32_t* cnt = reinterpret_cast<int32_t*>(wsb + p.L.w_cnt) + (size_t)b * p.L.N;
    int32_t* owner = reinterpret_cast<int32_t*>(svb + p.L.owner) + (size_t)b * p.L.N;
    for (int k = 0; k < K; ++k) s_list[k * 256 + t] = 0ull;
    for (int s = 0; s < d.num_stage; ++s) {
        const StageV st = sts.s[s];
        const T* pred = reinterpret_cast<const T*>(st.pred) + (size_t)b * st.H * st.W * st.ld;
        // a rectangle of cells that contains every centre inside the box (one cell of margin); the exact test is pair_eval's.
        // fmaxf / fminf drop a NaN operand, so the bounds are integers inside the map whatever the box holds
        const int c_lo = (int)fminf(fmaxf(floorf(tb[0] / st.stride - 0.5f) - 1.f, 0.f), (float)st.W);
        const int c_hi = (int)fminf(fmaxf(ceilf(tb[2] / st.stride - 0.5f) + 1.f, -1.f), (float)(st.W - 1));
        const int r_lo = (int)fminf(fmaxf(floorf(tb[1] / st.stride - 0.5f) - 1.f, 0.f), (float)st.H);
        const int r_hi = (int)fminf(fmaxf(ceilf(tb[3] / st.stride - 0.5f) + 1.f, -1.f), (float)(st.H - 1));
        const int nw = c_hi - c_lo + 1, nh = r_hi - r_lo + 1;
        if (nw <= 0 || nh <= 0) continue;
        for (int i = t; i < nw * nh; i += 256) {
            const int row = r_lo + i / nw, col = c_lo + i % nw;
            const int loc = row * st.W + col;
            const float cx = ((float)col + 0.5f) * st.stride, cy = ((float)row + 0.5f) * st.stride;
            float iou, metric;
            pair_eval<T>(d, tb, cls, cx, cy, st.stride, pbox + (size_t)(st.off + loc) * 4, pred + (size_t)loc * st.ld, iou, metric);
            if (!(metric > 0.f)) continue;                  // departure 1: strictly positive metrics only (NaN falls out too)
            const unsigned long long key = ((unsigned long long)__float_as_uint(metric) << 32) | (0xffffffffu - (unsigned)(st.off + loc));
            if (key > s_list[(K - 1) * 256 + t]) {
                int j = K - 1;
                while (j > 0 && s_list[(j - 1) * 256 + t] < key) { s_list[j * 256 + t] = s_list[(j - 1) * 256 + t]; --j; }
                s_list[j * 256 + t] = key;
            }
        }
    }
    // merge: the largest head of the 256 sorted lists, `topk` times.  Keys are unique (they hold the cell), larger key =
    // larger metric, then lower cell index
    int head = 0;
    for (int k = 0; k < K; ++k) {
        const unsigned long long mine = head < K ? s_list[head * 256 + t] : 0ull;
        unsigned long long v = mine;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned hi = __shfl_xor((unsigned)(v >> 32), o, 64), lo = __shfl_xor((unsigned)v, o, 64);
            const unsigned long long ov = ((unsigned long long)hi << 32) | lo;
            v = ov > v ? ov : v;
        }
        if (lane == 0) s_w[k & 1][wv] = v;
        __syncthreads();
        unsigned long long win = s_w[k & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) win = s_w[k & 1][w] > win ? s_w[k & 1][w] : win;
        if (win == 0ull) break;                             // block-uniform: fewer than topk positive metrics
        if (mine == win) ++head;
        if (t == 0) {
            const unsigned cell = 0xffffffffu - (unsigned)win;
            atomicAdd(&cnt[cell], 1);
            owner[cell] = m;                                // racy only where cnt ends > 1: the resolve pass decides those
        }
    }
}

// one thread per cell of the batch
template <typename T>
__global__ __launch_bounds__(256) void v8_resolve_kernel(const V8K p, const StagesV sts, const float* __restrict__ targets,
                                                         unsigned char* __restrict__ wsb, unsigned char* __restrict__ svb)
{
    const yh_v8loss_desc& d = p.d;
    const int N = p.L.N;
    const float* pbox = reinterpret_cast<const float*>(wsb + p.L.w_pbox);
    const int32_t* cnt = reinterpret_cast<const int32_t*>(wsb + p.L.w_cnt);
    float* c_met = reinterpret_cast<float*>(wsb + p.L.w_met);
    float* c_iou = reinterpret_cast<float*>(wsb + p.L.w_iou);
    uint32_t* gmax = reinterpret_cast<uint32_t*>(wsb + p.L.w_gmax);
    int32_t* owner = reinterpret_cast<int32_t*>(svb + p.L.owner);
    const long tot = (long)d.B * N;
    for (long gc = (long)blockIdx.x * 256 + threadIdx.x; gc < tot; gc += (long)gridDim.x * 256) {
        const int c = cnt[gc];
        if (c == 0) continue;
        const int b = (int)(gc / N), nn = (int)(gc - (long)b * N);
        int s = 0;
        for (int q = 1; q < d.num_stage; ++q) if (nn >= sts.s[q].off) s = q;
        const StageV st = sts.s[s];
        const int loc = nn - st.off;
        const float cx = ((float)(loc % st.W) + 0.5f) * st.stride, cy = ((float)(loc / st.W) + 0.5f) * st.stride;
        const T* row = reinterpret_cast<const T*>(st.pred) + ((size_t)b * st.H * st.W + loc) * st.ld;
        int g = owner[gc];
        float iou, metric;
        if (c > 1) {
            // arg-max of the IoU over all valid ground truths of the image, the first of equal ones (:215)
            float bv = -1.f; g = 0;
            for (int m = 0; m < d.maxbox; ++m) {
                const float* tg = targets + ((size_t)b * d.maxbox + m) * 6;
                if (!valid_row(d, tg)) continue;
                const float tb[4] = {tg[0], tg[1], tg[2], tg[3]};
                pair_eval<T>(d, tb, (int)tg[4], cx, cy, st.stride, pbox + (size_t)gc * 4, row, iou, metric);
                if (iou > bv) { bv = iou; g = m; }
            }
            owner[gc] = g;
        }
        const float* tg = targets + ((size_t)b * d.maxbox + g) * 6;
        const float tb[4] = {tg[0], tg[1], tg[2], tg[3]};
        pair_eval<T>(d, tb, (int)tg[4], cx, cy, st.stride, pbox + (size_t)gc * 4, row, iou, metric);
        c_met[gc] = metric; c_iou[gc] = iou;
        // non-negative floats order like their bits
        atomicMax(&gmax[((size_t)b * d.maxbox + g) * 2 + 0], __float_as_uint(metric));
        atomicMax(&gmax[((size_t)b * d.maxbox + g) * 2 + 1], __float_as_uint(iou));
    }
}

// the target distances [t, b, l, r] of an assigned cell in grid units, clamped to [0, reg - 1 - 0.01] (:312-313)
__device__ __forceinline__ void dfl_target(const float* tbs, float gx, float gy, int reg, float* tt) {
    const float hi = (float)((double)(reg - 1) - 0.01);
    tt[0] = fminf(fmaxf(gy - tbs[1], 0.f), hi); tt[1] = fminf(fmaxf(tbs[3] - gy, 0.f), hi);
    tt[2] = fminf(fmaxf(gx - tbs[0], 0.f), hi); tt[3] = fminf(fmaxf(tbs[2] - gx, 0.f), hi);
}

// grid (NB, stages); one thread per 8-element chunk of a cell row
template <typename T>
__global__ __launch_bounds__(256) void v8_loss_fwd_kernel(const V8K p, const StagesV sts, const float* __restrict__ targets,
                                                          const unsigned char* __restrict__ wsb, unsigned char* __restrict__ svb,
                                                          double* __restrict__ part)
{
    __shared__ double sred[NKIND][4];
    const StageV st = sts.s[blockIdx.y];
    const yh_v8loss_desc& d = p.d;
    const int n = st.H * st.W, cpr = st.ld / 8, nc = d.num_class, c_first = 4 * d.reg;
    const bool vec = d.reg % 8 == 0;
    const float* pbox = reinterpret_cast<const float*>(wsb + p.L.w_pbox);
    const float* c_met = reinterpret_cast<const float*>(wsb + p.L.w_met);
    const uint32_t* gmax = reinterpret_cast<const uint32_t*>(wsb + p.L.w_gmax);
    const int32_t* owner = reinterpret_cast<const int32_t*>(svb + p.L.owner);
    float* norm_out = reinterpret_cast<float*>(svb + p.L.norm);
    const T* pred = reinterpret_cast<const T*>(st.pred);
    const long nchunk = (long)d.B * n * cpr;
    double acc[NKIND] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nchunk; i += (long)gridDim.x * 256) {
        const long cell = i / cpr;
        const int c0 = (int)(i - cell * cpr) * 8;
        const int b = (int)(cell / n), loc = (int)(cell - (long)b * n);
        const size_t gc = (size_t)b * p.L.N + st.off + loc;
        const T* row = pred + (size_t)cell * st.ld;
        float f[8];
        load8<T>(row + c0, f);
        const int g = owner[gc];
        float norm = 0.f; int tcls = -1;
        const float* tg = nullptr;
        if (g >= 0) {
            const size_t r = (size_t)b * d.maxbox + g;
            tg = targets + r * 6;
            norm = (c_met[gc] * __uint_as_float(gmax[r * 2 + 1])) / (__uint_as_float(gmax[r * 2 + 0]) + 1e-9f);
            tcls = (int)tg[4];
        }
        float lc = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = c0 + j - c_first;
            if (c >= 0 && c < nc) {
                const float tt = c == tcls ? norm : 0.f;
                lc += cls_term(d, f[j], tt, nullptr);
            }
        }
        acc[0] += (double)lc;
        if (c0 == 0) {
            norm_out[gc] = norm;
            if (g >= 0) {
                const float gx = (float)(loc % st.W) + 0.5f, gy = (float)(loc / st.W) + 0.5f;
                const float4 q = *reinterpret_cast<const float4*>(pbox + gc * 4);
                const float pb[4] = {q.x, q.y, q.z, q.w};
                const float tbs[4] = {tg[0] / st.stride, tg[1] / st.stride, tg[2] / st.stride, tg[3] / st.stride};
                const float ci = ciou_fwd_bwd(pb, tbs, nullptr);
                float tt[4], dfl = 0.f;
                dfl_target(tbs, gx, gy, d.reg, tt);
#pragma unroll
                for (int side = 0; side < 4; ++side) {
                    const T* z = row + side * d.reg;
                    float mx, se, ex;
                    side_stats<T>(z, d.reg, vec, mx, se, ex);
                    const float lse = mx + logf(se);
                    const int tl = (int)tt[side];
                    const float wl = (float)(tl + 1) - tt[side], wr = 1.f - wl;
                    dfl += (lse - ldf<T>(z + tl)) * wl + (lse - ldf<T>(z + tl + 1)) * wr;
                }
                acc[1] += (double)((1.f - ci) * norm);
                acc[2] += (double)(dfl / 4.f * norm);
                acc[3] += (double)norm;
                acc[4] += 1.0;
            }
        }
    }
    block_partials(acc, sred);
    if (threadIdx.x < NKIND) part[((size_t)threadIdx.x * MAXS + blockIdx.y) * NB + blockIdx.x] = block_total(sred[threadIdx.x]);
}

// one block of NKIND waves: wave k sums kind k over the stages' partials in a fixed order
__global__ __launch_bounds__(64 * NKIND) void v8_finalize_kernel(const V8K p, const double* __restrict__ part, unsigned char* __restrict__ svb,
                                                                 float* __restrict__ result)
{
    __shared__ double ssum[NKIND];
    const yh_v8loss_desc& d = p.d;
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double a = 0.0;
    for (int s = 0; s < d.num_stage; ++s)
        for (int i = lane; i < NB; i += 64) a += part[((size_t)k * MAXS + s) * NB + i];
    a = wave_sum_d(a);
    if (lane == 0) ssum[k] = a;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float den = fmaxf((float)ssum[3], 1.f);            // max(cls_score.sum(), 1) (:61,:308)
    *reinterpret_cast<float*>(svb + p.L.den) = den;
    const float cls = (float)ssum[0] / den * d.cls_scale * (float)d.B;
    const float iou = (float)ssum[1] / den * d.iou_scale * (float)d.B;
    const float dfl = (float)ssum[2] / den * d.dfl_scale * (float)d.B;
    result[0] = cls + iou + dfl; result[1] = cls; result[2] = iou; result[3] = dfl;
    result[4] = (float)ssum[4]; result[5] = (float)ssum[3]; result[6] = 0.f; result[7] = 0.f;
}

// grid (blocks, stages); one thread per 8-element chunk of a cell row, which it writes whole
template <typename T>
__global__ __launch_bounds__(256) void v8_loss_bwd_kernel(const V8K p, const StagesV sts, const float* __restrict__ targets,
                                                          const unsigned char* __restrict__ svb, const float* __restrict__ gout)
{
    const StageV st = sts.s[blockIdx.y];
    const yh_v8loss_desc& d = p.d;
    const int n = st.H * st.W, cpr = st.ld / 8, nc = d.num_class, reg = d.reg, c_first = 4 * reg;
    const bool vec = reg % 8 == 0;
    const int32_t* owner = reinterpret_cast<const int32_t*>(svb + p.L.owner);
    const float* norm_in = reinterpret_cast<const float*>(svb + p.L.norm);
    const float den = *reinterpret_cast<const float*>(svb + p.L.den);
    const T* pred = reinterpret_cast<const T*>(st.pred);
    T* gp = reinterpret_cast<T*>(st.gpred);
    const float go = *gout * (float)d.B / den;
    const float kc = go * d.cls_scale, ki = go * d.iou_scale, kd = go * d.dfl_scale;
    const long nchunk = (long)d.B * n * cpr;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nchunk; i += (long)gridDim.x * 256) {
        const long cell = i / cpr;
        const int c0 = (int)(i - cell * cpr) * 8;
        const int b = (int)(cell / n), loc = (int)(cell - (long)b * n);
        const size_t gc = (size_t)b * p.L.N + st.off + loc;
        const T* row = pred + (size_t)cell * st.ld;
        float f[8], gr[8];
        load8<T>(row + c0, f);
        const int g = owner[gc];
        float norm = 0.f; int tcls = -1;
        if (g >= 0) { norm = norm_in[gc]; tcls = (int)targets[((size_t)b * d.maxbox + g) * 6 + 4]; }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = c0 + j - c_first;
            gr[j] = 0.f;
            if (c >= 0 && c < nc) {
                const float tt = c == tcls ? norm : 0.f;
                float dx;
                cls_term(d, f[j], tt, &dx);
                gr[j] = kc * dx;
            }
        }
        if (g >= 0 && c0 < c_first) {
            const float* tg = targets + ((size_t)b * d.maxbox + g) * 6;
            const float gx = (float)(loc % st.W) + 0.5f, gy = (float)(loc / st.W) + 0.5f;
            float mx[4], se[4], ee[4], pb[4];
#pragma unroll
            for (int side = 0; side < 4; ++side) {
                float ex;
                side_stats<T>(row + side * reg, reg, vec, mx[side], se[side], ex);
                ee[side] = ex / se[side];
                pb[side_slot(side)] = side_coord(side, ee[side], gx, gy);
            }
            const float tbs[4] = {tg[0] / st.stride, tg[1] / st.stride, tg[2] / st.stride, tg[3] / st.stride};
            float gci[4], tt[4];
            ciou_fwd_bwd(pb, tbs, gci);
            dfl_target(tbs, gx, gy, reg, tt);
            // d(iou term) / d(expected distance) per side: the box moves against t and l, with b and r
            const float kin = -ki * norm;
            const float de[4] = {-kin * gci[1], kin * gci[3], -kin * gci[0], kin * gci[2]};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = c0 + j;
                if (e < c_first) {
                    const int side = e / reg, k = e - side * reg;
                    const float smx = side == 0 ? mx[0] : side == 1 ? mx[1] : side == 2 ? mx[2] : mx[3];
                    const float sse = side == 0 ? se[0] : side == 1 ? se[1] : side == 2 ? se[2] : se[3];
                    const float see = side == 0 ? ee[0] : side == 1 ? ee[1] : side == 2 ? ee[2] : ee[3];
                    const float sde = side == 0 ? de[0] : side == 1 ? de[1] : side == 2 ? de[2] : de[3];
                    const float stt = side == 0 ? tt[0] : side == 1 ? tt[1] : side == 2 ? tt[2] : tt[3];
                    const float pk = expf(f[j] - smx) / sse;
                    const int tl = (int)stt;
                    const float wl = (float)(tl + 1) - stt, wr = 1.f - wl;
                    const float hit = k == tl ? wl : (k == tl + 1 ? wr : 0.f);
                    gr[j] = sde * (pk * ((float)(k + 1) - see)) + kd * norm * ((pk - hit) / 4.f);
                }
            }
        }
        store8<T>(gp + (size_t)cell * st.ld + c0, gr);
    }
}

int check_v8desc(const yh_v8loss_desc* d, const char* who) {
    YH_CHECK_ARG(d != nullptr, "%s: null desc", who);
    YH_CHECK_ARG(d->B > 0 && d->maxbox > 0 && d->num_class >= 1, "%s: bad B/maxbox/classes", who);
    YH_CHECK_ARG(d->num_stage >= 1 && d->num_stage <= MAXS, "%s: bad num_stage", who);
    YH_CHECK_ARG(d->reg >= 2 && d->reg <= MAXREG, "%s: reg must be 2..%d", who, MAXREG);
    YH_CHECK_ARG(d->topk >= 1 && d->topk <= KMAX, "%s: topk must be 1..%d", who, KMAX);
    YH_CHECK_ARG(d->img_size0 > 0.f, "%s: bad img_size0", who);
    long cells = 0;
    for (int s = 0; s < d->num_stage; ++s) {
        YH_CHECK_ARG(d->H[s] > 0 && d->W[s] > 0 && d->ldp[s] % 8 == 0 && d->ldp[s] >= 4 * d->reg + d->num_class && (long)d->H[s] * d->W[s] <= (1 << 20),
                     "%s: stage %d dims / ld invalid", who, s);
        cells += (long)d->H[s] * d->W[s];
    }
    YH_CHECK_ARG(cells * d->B < (1l << 31) && (long)d->B * d->maxbox < (1l << 28), "%s: too many cells or target rows", who);
    return YH_OK;
}

void fill_stages(const yh_v8loss_desc* d, const V8Layout& L, const void* const* preds, void* const* gpreds, StagesV& all) {
    for (int s = 0; s < MAXS; ++s) {
        const int q = s < d->num_stage ? s : 0;
        StageV& sg = all.s[s];
        sg.pred = preds[q]; sg.gpred = gpreds ? gpreds[q] : nullptr;
        sg.H = d->H[q]; sg.W = d->W[q]; sg.ld = d->ldp[q]; sg.off = L.cell_off[q];
        sg.stride = d->img_size0 / (float)d->H[q];
    }
}

int blocks_for(long threads, int cap) {
    const long nb = (threads + 255) / 256;
    return (int)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}

}  // namespace

extern "C" size_t yh_v8loss_saved_bytes(const yh_v8loss_desc* d) { return d ? make_v8layout(*d).total : 0; }
extern "C" size_t yh_v8loss_ws_bytes(const yh_v8loss_desc* d) { return d ? make_v8layout(*d).w_total : 0; }
/* byte offsets inside `saved`: out[0] = owner [B][N] i32 (matched target row per cell, -1 none), out[1] = norm [B][N] f32,
 * out[2] = N (cells per image), out[3] = 0, out[4..7] = first cell of each stage inside an image's N cells */
extern "C" int yh_v8loss_layout(const yh_v8loss_desc* d, int64_t* out) {
    YH_CHECK_ARG(d && out, "yh_v8loss_layout: null");
    const V8Layout L = make_v8layout(*d);
    out[0] = (int64_t)L.owner; out[1] = (int64_t)L.norm; out[2] = L.N; out[3] = 0;
    for (int s = 0; s < MAXS; ++s) out[4 + s] = L.cell_off[s];
    return YH_OK;
}

extern "C" int yh_v8_loss_fwd(const yh_v8loss_desc* d, const void* const* preds, const float* targets, float* result,
                              void* saved, void* ws, yh_stream stream)
{
    int rc = check_v8desc(d, "yh_v8_loss_fwd");
    if (rc) return rc;
    YH_CHECK_ARG(preds && targets && result && saved && ws, "yh_v8_loss_fwd: null pointer");
    YH_CHECK_ARG(yh_aligned16(saved) && yh_aligned16(ws), "yh_v8_loss_fwd: saved / ws must be 16-byte aligned");
    for (int s = 0; s < d->num_stage; ++s) YH_CHECK_ARG(preds[s] && yh_aligned16(preds[s]), "yh_v8_loss_fwd: preds[%d] null/unaligned", s);
    hipStream_t st = (hipStream_t)stream;
    V8K k; k.d = *d; k.L = make_v8layout(*d);
    unsigned char* sv = (unsigned char*)saved;
    unsigned char* wsb = (unsigned char*)ws;
    double* part = reinterpret_cast<double*>(wsb + k.L.w_part);
    StagesV all;
    fill_stages(d, k.L, preds, nullptr, all);
    long cmax = 1;
    for (int s = 0; s < d->num_stage; ++s) { const long c = (long)d->B * d->H[s] * d->W[s]; if (c > cmax) cmax = c; }
    const dim3 g_pre(blocks_for(cmax * 4, 8192), d->num_stage), g_asg(d->maxbox, d->B), g_loss(NB, d->num_stage);
    const int g_res = blocks_for((long)d->B * k.L.N, 8192);
    const size_t lds = (size_t)d->topk * 256 * sizeof(unsigned long long);
    yh_pred_type(d->pred_is_f32, [&](auto e) {
        using T = decltype(e);
        hipLaunchKernelGGL((v8_pre_kernel<T>), g_pre, dim3(256), 0, st, k, all, wsb, sv);
        hipLaunchKernelGGL((v8_assign_kernel<T>), g_asg, dim3(256), lds, st, k, all, targets, wsb, sv);
        hipLaunchKernelGGL((v8_resolve_kernel<T>), dim3(g_res), dim3(256), 0, st, k, all, targets, wsb, sv);
        hipLaunchKernelGGL((v8_loss_fwd_kernel<T>), g_loss, dim3(256), 0, st, k, all, targets, wsb, sv, part);
    });
    hipLaunchKernelGGL(v8_finalize_kernel, dim3(1), dim3(64 * NKIND), 0, st, k, part, sv, result);
    YH_CHECK_LAUNCH("yh_v8_loss_fwd");
    return YH_OK;
}

extern "C" int yh_v8_loss_bwd(const yh_v8loss_desc* d, const void* const* preds, const float* targets, const float* gout,
                              const void* saved, void* const* gpreds, void* ws, yh_stream stream)
{
    int rc = check_v8desc(d, "yh_v8_loss_bwd");
    if (rc) return rc;
    (void)ws;                      // the backward recomputes what it needs from preds and `saved`
    YH_CHECK_ARG(preds && targets && gout && saved && gpreds, "yh_v8_loss_bwd: null pointer");
    YH_CHECK_ARG(yh_aligned16(saved), "yh_v8_loss_bwd: saved must be 16-byte aligned");
    for (int s = 0; s < d->num_stage; ++s)
        YH_CHECK_ARG(preds[s] && gpreds[s] && yh_aligned16(preds[s]) && yh_aligned16(gpreds[s]), "yh_v8_loss_bwd: stage %d pointers null/unaligned", s);
    hipStream_t st = (hipStream_t)stream;
    V8K k; k.d = *d; k.L = make_v8layout(*d);
    StagesV all;
    fill_stages(d, k.L, preds, gpreds, all);
    long chmax = 1;
    for (int s = 0; s < d->num_stage; ++s) { const long c = (long)d->B * d->H[s] * d->W[s] * (d->ldp[s] / 8); if (c > chmax) chmax = c; }
    const dim3 grid(blocks_for(chmax, 8192), d->num_stage);
    yh_pred_type(d->pred_is_f32, [&](auto e) {
        hipLaunchKernelGGL((v8_loss_bwd_kernel<decltype(e)>), grid, dim3(256), 0, st, k, all, targets, (const unsigned char*)saved, gout);
    });
    YH_CHECK_LAUNCH("yh_v8_loss_bwd");
    return YH_OK;
}
