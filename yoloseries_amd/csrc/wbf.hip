// Weighted box fusion on the device (utils/weighted_fusion_bbox.py, trainer/eval_yolov5.py:44-92 do_wfb): the candidate rows of the
// three test-time-augmentation passes of an image are merged by clustering instead of suppression.
//
// Per (image, class), rows by score descending (ties: table row ascending; the caller sorts), starting from NO cluster:
//   a row joins EVERY cluster whose fused box has IoU >= iou_thr with it; a row that joins none founds a new cluster; the fused box
//   of every cluster that changed is refreshed before the next row is taken.
// Operation order, every operation a correctly rounded fp64 operation, once (this file compiles with the exact flags):
//   IoU (cpu_iou)  a_row = (x2 - x1) * (y2 - y1),  a_clu likewise,  w = max(0, min(x2, X2) - max(x1, X1)),  h likewise,
//                  inter = w * h,  iou = inter / max((a_row + a_clu) - inter, 1e-6)
//   cluster sums   A_k += (double)b_k * (double)s  (k = 0..3, arrival order),  S += s,  SW += s * w,  W += w,  N += 1
//   fused box      box_mean 0 (the reference: np.mean over the members of b * s / sum(s)):  (A_k / S) / N
//                  box_mean 1 (the usual weighted box):                                     A_k / S
//   fused score    SW / W, taken once when the segment is done
// Outside the contract: NaN coordinates or scores, non-positive scores (S could be 0), rows of `order` below nvalid that are not
// sorted by (class ascending, score descending).  None of them can make a kernel read or write out of bounds: an entry of `order` is
// clamped to [0, cap), nvalid to [0, cap], a segment's clusters are at most its rows, and every slot index derives from those.
//
// wbf_fuse_kernel: one workgroup of four waves per (class, image).  Two lanes find the segment by binary search in the sorted rows'
// class.  The rows are staged WBF_CHUNK at a time in LDS and taken one by one; thread t owns the clusters j with j % WBF_THREADS == t,
// for the IoU test, the update and the creation alike, so a cluster's state is only ever touched by one thread: no atomics and no
// barrier for the state.  The one thing the threads share per row is "did any cluster take it": __syncthreads_or (a ballot per
// wave, one LDS word).  The state of the first L clusters of a segment lives in LDS ([12][L] doubles, L = min(cap,
// WBF_LDS_CLUSTERS)), that of the others in the workspace ([B][12][cap] doubles: cluster j of the segment that starts at sorted row s
// is column s + j, and j < the segment's rows, so segments never meet).  A cluster's output row goes to the staging table at the
// SORTED position of its founding row; wbf_compact_kernel (a workgroup per image) closes the holes, which leaves the rows class
// ascending, then in creation order, without a segment knowing another's count.
// Cost: a row costs one pass of the workgroup over the segment's clusters, so a segment of n rows in m clusters costs
// n * ceil(m / 256) steps of an fp64 IoU; every row its own cluster in one class is the O(n^2 / 256) worst case.
#include "common.h"

#define WBF_THREADS 256
#define WBF_CHUNK 256                       // rows staged per pass: one per thread
#define WBF_FIELDS 12                       // doubles per cluster
#define WBF_LDS_CLUSTERS 1024               // clusters of a segment whose state lives in LDS: 12 * 8 * 1024 = 96 KiB

namespace {

enum { WF_A = 0, WF_S = 4, WF_SW = 5, WF_W = 6, WF_BOX = 7, WF_NF = 11 };      // WF_NF: founder's row within the segment << 32 | N

__device__ __forceinline__ int wbf_row(const int32_t* __restrict__ order, long i, int cap) { return min(max(order[i], 0), cap - 1); }

// one row as every thread sees it: the box, its area, its contribution to A (box * score), score, score * weight, weight
struct WbfRow { double x1, y1, x2, y2, area, ax, ay, az, aw, sc, sw, w; };

// The three things done to a cluster's state, on `p` with field stride `ld`: s_state / L for a cluster in LDS, the workspace columns
// / cap for one past it.  Each call site names one of the two, so every access is an LDS or a global access, never a flat one.
// the IoU test of cluster j against the row and, on a hit, the update of its sums and its fused box -> 1 on a hit
__device__ __forceinline__ int wbf_take(double* __restrict__ p, long ld, int j, const WbfRow& r, double iou_thr, int box_mean)
{
    const double X1 = p[WF_BOX * ld + j], Y1 = p[(WF_BOX + 1) * ld + j], X2 = p[(WF_BOX + 2) * ld + j], Y2 = p[(WF_BOX + 3) * ld + j];
    const double a_clu = (X2 - X1) * (Y2 - Y1);
    const double iw = fmax(0.0, fmin(r.x2, X2) - fmax(r.x1, X1));
    const double ih = fmax(0.0, fmin(r.y2, Y2) - fmax(r.y1, Y1));
    const double inter = iw * ih;
    const double iou = inter / fmax((r.area + a_clu) - inter, 1e-6);
    if (!(iou >= iou_thr)) return 0;
    const double A0 = p[WF_A * ld + j] + r.ax, A1 = p[(WF_A + 1) * ld + j] + r.ay, A2 = p[(WF_A + 2) * ld + j] + r.az, A3 = p[(WF_A + 3) * ld + j] + r.aw;
    const double S = p[WF_S * ld + j] + r.sc;
    const long long nf = __double_as_longlong(p[WF_NF * ld + j]) + 1;
    p[WF_A * ld + j] = A0; p[(WF_A + 1) * ld + j] = A1; p[(WF_A + 2) * ld + j] = A2; p[(WF_A + 3) * ld + j] = A3;
    p[WF_S * ld + j] = S;
    p[WF_SW * ld + j] = p[WF_SW * ld + j] + r.sw;
    p[WF_W * ld + j] = p[WF_W * ld + j] + r.w;
    p[WF_NF * ld + j] = __longlong_as_double(nf);
    double B0 = A0 / S, B1 = A1 / S, B2 = A2 / S, B3 = A3 / S;
    if (box_mean == 0) {
        const double N = (double)(int)(nf & 0xffffffffLL);
        B0 = B0 / N; B1 = B1 / N; B2 = B2 / N; B3 = B3 / N;
    }
    p[WF_BOX * ld + j] = B0; p[(WF_BOX + 1) * ld + j] = B1; p[(WF_BOX + 2) * ld + j] = B2; p[(WF_BOX + 3) * ld + j] = B3;
    return 1;
}

// cluster j founded by the row at position `pos` of the segment (N = 1: both box means are A / S)
__device__ __forceinline__ void wbf_found(double* __restrict__ p, long ld, int j, const WbfRow& r, int pos)
{
    p[WF_A * ld + j] = r.ax; p[(WF_A + 1) * ld + j] = r.ay; p[(WF_A + 2) * ld + j] = r.az; p[(WF_A + 3) * ld + j] = r.aw;
    p[WF_S * ld + j] = r.sc; p[WF_SW * ld + j] = r.sw; p[WF_W * ld + j] = r.w;
    p[WF_NF * ld + j] = __longlong_as_double(((long long)pos << 32) | 1LL);
    p[WF_BOX * ld + j] = r.ax / r.sc; p[(WF_BOX + 1) * ld + j] = r.ay / r.sc;
    p[(WF_BOX + 2) * ld + j] = r.az / r.sc; p[(WF_BOX + 3) * ld + j] = r.aw / r.sc;
}

// cluster j's output row, at the staging slot of its founding row
__device__ __forceinline__ void wbf_emit(const double* __restrict__ p, long ld, int j, int n, int c, float* __restrict__ so, int32_t* __restrict__ sm)
{
    const long long nf = __double_as_longlong(p[WF_NF * ld + j]);
    const int pos = min(max((int)(nf >> 32), 0), n - 1);
    float* o = so + (long)pos * 6;
    o[0] = (float)p[WF_BOX * ld + j]; o[1] = (float)p[(WF_BOX + 1) * ld + j];
    o[2] = (float)p[(WF_BOX + 2) * ld + j]; o[3] = (float)p[(WF_BOX + 3) * ld + j];
    o[4] = (float)(p[WF_SW * ld + j] / p[WF_W * ld + j]);
    o[5] = (float)c;
    sm[pos] = (int)(nf & 0xffffffffLL);
}

__global__ __launch_bounds__(WBF_THREADS) void wbf_fuse_kernel(
    const float* __restrict__ cand, const float* __restrict__ weight, const int32_t* __restrict__ order,
    const int32_t* __restrict__ nvalid, int cap, int L, double iou_thr, int box_mean,
    double* __restrict__ state, float* __restrict__ st_out, int32_t* __restrict__ st_mem)
{
    extern __shared__ double s_state[];                               // [WBF_FIELDS][L]
    __shared__ float4 s_box[WBF_CHUNK];
    __shared__ float s_sc[WBF_CHUNK], s_wt[WBF_CHUNK];
    __shared__ int s_seg[2];
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int nv = min(max(nvalid[b], 0), cap);
    const float* cb = cand + (long)b * cap * 6;
    const float* wb = weight + (long)b * cap;
    const int32_t* ord = order + (long)b * cap;

    if (t < 2) {                                                      // the first sorted row of class c (t = 0) and of class c + 1 (t = 1)
        int lo = 0, hi = nv;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((int)cb[(long)wbf_row(ord, mid, cap) * 6 + 5] < c + t) lo = mid + 1; else hi = mid;
        }
        s_seg[t] = lo;
    }
    __syncthreads();
    const int s = s_seg[0], n = s_seg[1] - s_seg[0];
    if (n <= 0) return;                                               // uniform

    double* gs = state + (long)b * WBF_FIELDS * cap + s;              // field f of cluster j >= L: gs[f * cap + j]
    float* so = st_out + ((long)b * cap + s) * 6;
    int32_t* sm = st_mem + (long)b * cap + s;
    int nclu = 0;                                                     // the same in every thread
    for (int base = 0; base < n; base += WBF_CHUNK) {
        const int m = min(WBF_CHUNK, n - base);
        if (base) __syncthreads();                                    // the previous chunk has been read
        if (t < m) {
            const int r = wbf_row(ord, s + base + t, cap);
            const float* q = cb + (long)r * 6;
            s_box[t] = make_float4(q[0], q[1], q[2], q[3]);
            s_sc[t] = q[4];
            s_wt[t] = wb[r];
            sm[base + t] = 0;                                         // no cluster founded here, unless its owner says so at the end
        }
        __syncthreads();
        for (int i = 0; i < m; ++i) {
            const float4 q = s_box[i];
            const double x1 = (double)q.x, y1 = (double)q.y, x2 = (double)q.z, y2 = (double)q.w;
            const double sc = (double)s_sc[i], w = (double)s_wt[i];
            const double a_row = (x2 - x1) * (y2 - y1);
            const double ax = x1 * sc, ay = y1 * sc, az = x2 * sc, aw = y2 * sc, sw = sc * w;
            const WbfRow row = {x1, y1, x2, y2, a_row, ax, ay, az, aw, sc, sw, w};
            int hit = 0;
            const int n_lds = min(nclu, L);
            int j = t;
            for (; j < n_lds; j += WBF_THREADS) hit |= wbf_take(s_state, L, j, row, iou_thr, box_mean);
            for (; j < nclu; j += WBF_THREADS) hit |= wbf_take(gs, cap, j, row, iou_thr, box_mean);
            const int any = __syncthreads_or(hit);
            if (!any) {                                               // uniform: the row founds cluster nclu, written by its owner
                if (t == nclu % WBF_THREADS) {
                    if (nclu < L) wbf_found(s_state, L, nclu, row, base + i);
                    else          wbf_found(gs, cap, nclu, row, base + i);
                }
                ++nclu;
            }
        }
    }
    __syncthreads();                                                  // the zeros of the last chunk's sm are behind us
    const int n_lds = min(nclu, L);                                   // nclu <= n: a row founds at most one cluster
    int j = t;
    for (; j < n_lds; j += WBF_THREADS) wbf_emit(s_state, L, j, n, c, so, sm);
    for (; j < nclu; j += WBF_THREADS) wbf_emit(gs, cap, j, n, c, so, sm);
}

// closes the holes of the staging table: the rows with members > 0 among the first nvalid[b], in order
__global__ __launch_bounds__(WBF_THREADS) void wbf_compact_kernel(
    const float* __restrict__ st_out, const int32_t* __restrict__ st_mem, const int32_t* __restrict__ nvalid, int cap,
    float* __restrict__ out, int32_t* __restrict__ nout, int32_t* __restrict__ members)
{
    __shared__ int wave_cnt[WBF_THREADS / 64];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int nv = min(max(nvalid[b], 0), cap);
    const long row0 = (long)b * cap;
    int base = 0;                                                     // the same in every thread
    for (int p0 = 0; p0 < nv; p0 += WBF_THREADS) {
        const int p = p0 + t;
        const int mem = p < nv ? st_mem[row0 + p] : 0;
        const bool flag = mem > 0;
        const unsigned long long bal = __ballot(flag);
        const int within = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wv] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < WBF_THREADS / 64; ++w) { const int k = wave_cnt[w]; if (w < wv) before += k; total += k; }
        if (flag) {
            const long dst = row0 + base + before + within;           // <= row0 + p: never past the image's rows
            const float* q = st_out + (row0 + p) * 6;
            float* o = out + dst * 6;
            o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3]; o[4] = q[4]; o[5] = q[5];
            if (members) members[dst] = mem;
        }
        base += total;
        __syncthreads();                                              // the counts have been read
    }
    if (t == 0) nout[b] = base;
}

inline size_t wbf_rows(int B, int cap) { return (size_t)B * (size_t)cap; }

}  // namespace

extern "C" int yh_wbf_lds_clusters(void) { return WBF_LDS_CLUSTERS; }

extern "C" size_t yh_wbf_ws_bytes(int B, int cap)
{
    if (B <= 0 || cap <= 0) return 0;
    return wbf_rows(B, cap) * (WBF_FIELDS * sizeof(double) + 6 * sizeof(float) + sizeof(int32_t));
}

extern "C" int yh_wbf_batched(const float* cand, const float* weight, const int32_t* order, const int32_t* nvalid, int B, int cap,
                              int num_class, double iou_thr, int box_mean, float* out, int32_t* nout, int32_t* members, void* ws,
                              yh_stream stream)
{
    YH_CHECK_ARG(cand && weight && order && nvalid, "yh_wbf_batched: null input pointer");
    YH_CHECK_ARG(out && nout && ws, "yh_wbf_batched: null output or ws pointer");
    YH_CHECK_ARG(B > 0 && cap > 0 && num_class > 0, "yh_wbf_batched: B, cap, num_class must be positive (B=%d cap=%d num_class=%d)", B, cap, num_class);
    YH_CHECK_ARG(B <= 65535 && num_class <= 0x7fffffff / 2 && (long)B * cap <= 0x7fffffffL / WBF_FIELDS,
                 "yh_wbf_batched: tables too large (B=%d, B * cap = %ld)", B, (long)B * cap);
    YH_CHECK_ARG(box_mean == 0 || box_mean == 1, "yh_wbf_batched: box_mean=%d must be 0 (reference) or 1 (weighted)", box_mean);
    YH_CHECK_ARG(iou_thr == iou_thr, "yh_wbf_batched: iou_thr is NaN");
    YH_CHECK_ARG(((((uintptr_t)cand) | ((uintptr_t)weight) | ((uintptr_t)order) | ((uintptr_t)nvalid) | ((uintptr_t)out) | ((uintptr_t)nout) |
                   ((uintptr_t)members)) & 3) == 0 && (((uintptr_t)ws) & 7) == 0, "yh_wbf_batched: unaligned table (4 bytes; ws 8 bytes)");
    const int L = cap < WBF_LDS_CLUSTERS ? cap : WBF_LDS_CLUSTERS;
    static YhDevOnce attr;
    yh_lds_limit(attr, {{(const void*)wbf_fuse_kernel, WBF_LDS_CLUSTERS * WBF_FIELDS * (int)sizeof(double)}});
    double* state = (double*)ws;
    float* st_out = (float*)(state + wbf_rows(B, cap) * WBF_FIELDS);
    int32_t* st_mem = (int32_t*)(st_out + wbf_rows(B, cap) * 6);
    hipLaunchKernelGGL(wbf_fuse_kernel, dim3(num_class, B), dim3(WBF_THREADS), (size_t)L * WBF_FIELDS * sizeof(double), (hipStream_t)stream,
                       cand, weight, order, nvalid, cap, L, iou_thr, box_mean, state, st_out, st_mem);
    YH_CHECK_LAUNCH("yh_wbf_batched (fuse)");
    hipLaunchKernelGGL(wbf_compact_kernel, dim3(B), dim3(WBF_THREADS), 0, (hipStream_t)stream, st_out, st_mem, nvalid, cap, out, nout, members);
    YH_CHECK_LAUNCH("yh_wbf_batched (compact)");
    return YH_OK;
}
