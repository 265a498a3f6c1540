// YOLOv8 inference post-processing on gfx950 (trainer/eval_yolov8.py:76-102 and :168-196 of the reference): distribution-focal
// decode of the anchor-free head, class sigmoid, candidate filter.  The head of one cell is [4*reg box logits | num_class class
// logits]; the box sides come in the order [t, b, l, r], each the expectation of softmax(reg logits) over the 1-BASED bins
// 1..reg (loss/yolov8_loss.py:30), and the box is (gx - l, gy - t, gx + r, gy + b) * stride (utils/bbox_tools.py:392-407) with
// stride = img_h / H.  There is no objectness and there are no anchors: nothing in postproc.hip decodes this head.
//
//   v8_decode_full      one thread per output element of the (B, N, 4+nc) tensor do_inference returns.
//   v8_filter_kernel    fused decode + filter, one workgroup per image, one thread per cell (ws == NULL): small heads, and the
//                       cross-check of the two-pass form.
//   v8_scan_kernel      two-pass form, pass 1: a block owns 64 consecutive cells of one stage, brings their rows to LDS with
//                       coalesced 16-byte loads (scalar where the row start or ldp is not 16-byte aligned) — every head byte is
//                       read once — and evaluates a cell with FOUR lanes: each takes every fourth class, then one box side.
//                       Wave ballots and a four-entry block prefix order the candidates of the chunk; they go to the staging
//                       area [B][nchunk][64][6] with their counts.
//   v8_gather_kernel    pass 2, one block per image: counts -> offsets in prediction order, staged rows -> final rows.
//   v8_filter_decoded   the candidate rule on an already decoded tensor, single label or one row per (cell, class).
// The table is the [B][cap][6] table yh_nms_batched consumes.  Order is decided by ballots and prefix sums alone: no atomics.
//
// Candidate rule (:175-196): score = max_c sigmoid(x_c), compared ON THE fp32 SIGMOID VALUES (logits 17 and 25 both give
// 1.0f), class = the first index that reaches it, candidate iff score >= cls_thr.  Before the nc sigmoids a cell is dropped if
// sigm(max logit) * 1.0001f < cls_thr: expf and the division are accurate to a few ulp, so no class of such a cell can reach
// the threshold (about 99 % of the cells of a trained head leave here); every surviving cell is evaluated in full, so the
// shortcut never decides a row.  Both fused forms, and yh_v8_decode_full followed by yh_v8_filter_decoded, give the same table
// bit for bit: they share side_dist / box_slot and the tie rule.
//
// Departure from the reference: make_grid (:133-137) views a (w, h, 2) mesh as (h, w, 2), which is the grid (col + 0.5,
// row + 0.5) for square maps and a scramble for rectangular ones; here x = col + 0.5, y = row + 0.5 always (as loss_v8.hip).
// NaN logits are outside the contract: a NaN class logit is never a maximum, a NaN box logit gives a NaN box.
#include <float.h>
#include "exact_math.h"

namespace {

constexpr int MAXS = 4;
constexpr int DPIX = 64;          // cells per block of the two-pass form = rows per key of the staging area

// one pass of test-time augmentation (:59-69): xyxy * (1 / scale), then the flipped axis' corner pair is mirrored and swapped
struct View8 {
    float inv;                    // 1.0f / scale, taken once on the host
    int flip;                     // 0 none, 2 rows, 3 columns
    float img_h, img_w;
    int append;                   // first row of image b: ncand[b] on entry instead of 0
};

struct Dec8 {
    yh_v8dec_desc d;
    const void* pred[MAXS];
    float stride[MAXS];           // img_h / H
    int start[MAXS + 1];          // first cell of each stage inside an image's N cells
    int cstart[MAXS + 1];         // first 64-cell chunk of each stage: the chunk index is the key, in prediction order
    int ntot;
};

// softmax expectation of one side: sum_k exp(z_k - max) * (k + 1) / sum_k exp(z_k - max)
template <typename T>
__device__ __forceinline__ float side_dist(const T* z, int reg)
{
    float mx = -INFINITY, se = 0.f, ex = 0.f;
    for (int k = 0; k < reg; ++k) mx = fmaxf(mx, ldf<T>(z + k));
    for (int k = 0; k < reg; ++k) { const float e = expf(ldf<T>(z + k) - mx); se += e; ex += e * (float)(k + 1); }
    return ex / se;
}
// box slot [xmin, ymin, xmax, ymax] -> the side [t, b, l, r] it is made from
__device__ __forceinline__ int slot_side(int slot) { return slot == 0 ? 2 : slot == 1 ? 0 : slot == 2 ? 3 : 1; }
__device__ __forceinline__ float box_slot(int slot, float dist, float gx, float gy, float st) {
    return (slot == 0 ? gx - dist : slot == 1 ? gy - dist : slot == 2 ? gx + dist : gy + dist) * st;
}

// cell index (within an image) -> stage, index inside the stage
__device__ __forceinline__ void locate(const Dec8& k, int pi, int& s, int& r) {
    s = 0;
#pragma unroll
    for (int i = 1; i < MAXS; ++i) if (i < k.d.num_stage && pi >= k.start[i]) s = i;
    r = pi - k.start[s];
}
template <typename T>
__device__ __forceinline__ const T* cell_ptr(const Dec8& k, int b, int s, int r) {
    return reinterpret_cast<const T*>(k.pred[s]) + ((size_t)b * k.d.H[s] * k.d.W[s] + r) * k.d.ldp[s];
}

template <typename T>
__global__ void v8_decode_full_kernel(const Dec8 k, float* __restrict__ out)
{
    const int E = 4 + k.d.num_class, reg = k.d.reg;
    const long tot = (long)k.d.B * k.ntot * E;
    for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < tot; id += (long)gridDim.x * blockDim.x) {
        const int e = (int)(id % E);
        const long q = id / E;
        const int pi = (int)(q % k.ntot), b = (int)(q / k.ntot);
        int s, r;
        locate(k, pi, s, r);
        const T* row = cell_ptr<T>(k, b, s, r);
        float v;
        if (e < 4) {
            const int y = r / k.d.W[s], x = r - y * k.d.W[s];
            v = box_slot(e, side_dist<T>(row + slot_side(e) * reg, reg), (float)x + 0.5f, (float)y + 0.5f, k.stride[s]);
        } else {
            v = sigm(ldf<T>(row + 4 * reg + (e - 4)));
        }
        out[id] = v;
    }
}

// One cell by P lanes (P = 1: the calling thread alone; P = 4: the four lanes lane & ~3 .. + 3 of a wave, which must all call with the
// same cell and j = lane & 3).  true = candidate; box / score / cls are then valid in every one of the P lanes.
template <typename T, int P>
__device__ __forceinline__ bool eval_cell(const Dec8& k, const View8& v, const T* row, int s, int y, int x, int lane, float cls_thr,
                                          float* box, float& score, int& cls)
{
    const int nc = k.d.num_class, reg = k.d.reg;
    const int j = P == 1 ? 0 : (lane & 3);
    const T* cl = row + 4 * reg;
    float m = -INFINITY;
    for (int c = j; c < nc; c += P) m = fmaxf(m, ldf<T>(cl + c));
    if (P == 4) { m = fmaxf(m, __shfl_xor(m, 1, 64)); m = fmaxf(m, __shfl_xor(m, 2, 64)); }
    if (sigm(m) * 1.0001f < cls_thr) return false;                // no class can reach the threshold (header comment)
    float best = -INFINITY;
    int bc = 0;
    for (int c = j; c < nc; c += P) {
        const float pc = sigm(ldf<T>(cl + c));
        if (pc > best) { best = pc; bc = c; }                     // first maximum of this lane's classes
    }
    if (P == 4) {
#pragma unroll
        for (int o = 1; o <= 2; o <<= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oc = __shfl_xor(bc, o, 64);
            if (ob > best || (ob == best && oc < bc)) { best = ob; bc = oc; }      // equal values: the lower class index
        }
    }
    if (!(best >= cls_thr)) return false;                         // :175, inclusive
    float dist[4];
    if (P == 4) {
        const float mine = side_dist<T>(row + j * reg, reg);
#pragma unroll
        for (int i = 0; i < 4; ++i) dist[i] = __shfl(mine, (lane & ~3) + i, 64);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) dist[i] = side_dist<T>(row + i * reg, reg);
    }
    const float gx = (float)x + 0.5f, gy = (float)y + 0.5f, st = k.stride[s];
#pragma unroll
    for (int i = 0; i < 4; ++i) box[i] = box_slot(i, dist[slot_side(i)], gx, gy, st) * v.inv;      // ripe[..., :4] /= s (:59)
    if (v.flip == 2) { const float lo = v.img_h - box[3], hi = v.img_h - box[1]; box[1] = lo; box[3] = hi; }       // :60-64
    if (v.flip == 3) { const float lo = v.img_w - box[2], hi = v.img_w - box[0]; box[0] = lo; box[2] = hi; }       // :65-69
    score = best;
    cls = bc;
    return true;
}

template <typename T>
__global__ __launch_bounds__(1024) void v8_filter_kernel(const Dec8 k, const View8 v, float cls_thr, float* __restrict__ cand,
                                                         int32_t* __restrict__ ncand, int cap)
{
    __shared__ int wave_cnt[16];
    __shared__ int base_s;
    const int b = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t == 0) base_s = v.append ? max(ncand[b], 0) : 0;
    __syncthreads();
    float* out = cand + (size_t)b * cap * 6;
    for (int p0 = 0; p0 < k.ntot; p0 += 1024) {
        const int pi = p0 + t;
        bool flag = false;
        float box[4] = {0, 0, 0, 0}, score = 0.f;
        int cls = 0;
        if (pi < k.ntot) {
            int s, r;
            locate(k, pi, s, r);
            const int y = r / k.d.W[s], x = r - y * k.d.W[s];
            flag = eval_cell<T, 1>(k, v, cell_ptr<T>(k, b, s, r), s, y, x, lane, cls_thr, box, score, cls);
        }
        const unsigned long long bal = __ballot(flag);
        const int within = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wv] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int c = wave_cnt[w]; if (w < wv) before += c; total += c; }
        const int base = base_s;
        if (flag) {
            const int pos = base + before + within;
            if ((unsigned)pos < (unsigned)cap) {                  // unsigned: a base near INT_MAX that wraps must not store either
                float* o = out + (size_t)pos * 6;
                o[0] = box[0]; o[1] = box[1]; o[2] = box[2]; o[3] = box[3]; o[4] = score; o[5] = (float)cls;
            }
        }
        __syncthreads();
        if (t == 0) base_s = base + total;
        __syncthreads();
    }
    if (t == 0) ncand[b] = base_s;
}

template <typename T>
__global__ __launch_bounds__(256) void v8_scan_kernel(const Dec8 k, const View8 v, float cls_thr, float* __restrict__ stage,
                                                      int32_t* __restrict__ counts, int nkeys)
{
    // all LDS is dynamic (the limit raised for this kernel is the whole 160 KB): the four wave counts sit in front of the tile
    extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
    int* wave_cnt = reinterpret_cast<int*>(dsm);
    T* tile = reinterpret_cast<T*>(dsm + 16);
    const int b = blockIdx.y;
    int s = 0;
#pragma unroll
    for (int i = 1; i < MAXS; ++i) if (i < k.d.num_stage && (int)blockIdx.x >= k.cstart[i]) s = i;
    const int c = blockIdx.x - k.cstart[s];
    const int hw = k.d.H[s] * k.d.W[s];
    const int p0 = c * DPIX;
    const int npix = min(DPIX, hw - p0);
    const int ldp = k.d.ldp[s];
    // LDS rows are 16 bytes longer than the head rows, so that the 16 cells of a wave do not start on the same banks
    constexpr int LPAD = 16 / (int)sizeof(T);
    const int lds_ld = ldp + LPAD;
    const T* src = reinterpret_cast<const T*>(k.pred[s]) + ((size_t)b * hw + p0) * ldp;
    const int t = threadIdx.x;
    // only the 4*reg + nc leading elements of a row are read (a head may be a channel slice of a wider tensor: ldp is then longer, and
    // what follows the last cell's elements need not exist), rounded up to whole 16-byte pieces where rows are 16-byte aligned
    const int cols = 4 * k.d.reg + k.d.num_class;
    if (((size_t)src & 15) == 0 && (ldp * (int)sizeof(T)) % 16 == 0) {
        const int rowp = ldp * (int)sizeof(T) / 16;           // 16-byte pieces between rows
        const int cpr = (cols * (int)sizeof(T) + 15) / 16;    // pieces read per row
        const int nv = npix * cpr;
        constexpr int NLD = 8;                                // all loads of a round are requested before the first LDS store
        for (int i0 = 0; i0 < nv; i0 += 256 * NLD) {
            uint4 q[NLD];
            int at[NLD];
#pragma unroll
            for (int u = 0; u < NLD; ++u) {
                const int i = i0 + u * 256 + t;
                const int r = i / cpr, c16 = i - r * cpr;
                at[u] = r * lds_ld + c16 * LPAD;
                q[u] = make_uint4(0, 0, 0, 0);
                if (i < nv) q[u] = reinterpret_cast<const uint4*>(src)[r * rowp + c16];
            }
#pragma unroll
            for (int u = 0; u < NLD; ++u)
                if (i0 + u * 256 + t < nv) *reinterpret_cast<uint4*>(tile + at[u]) = q[u];
        }
    } else {
        const int nelem = npix * cols;
        for (int i = t; i < nelem; i += 256) { const int r = i / cols, e = i - r * cols; tile[r * lds_ld + e] = src[(size_t)r * ldp + e]; }
    }
    __syncthreads();
    const int lane = t & 63, wv = t >> 6, cell = t >> 2;
    bool flag = false;
    float box[4] = {0, 0, 0, 0}, score = 0.f;
    int cls = 0;
    if (cell < npix) {                                        // the four lanes of a cell take this branch together
        const int pidx = p0 + cell;
        const int y = pidx / k.d.W[s], x = pidx - y * k.d.W[s];
        flag = eval_cell<T, 4>(k, v, tile + cell * lds_ld, s, y, x, lane, cls_thr, box, score, cls);
    }
    const bool lead = flag && (lane & 3) == 0;                // one row per cell: its first lane writes it
    const unsigned long long bal = __ballot(lead);
    if (lane == 0) wave_cnt[wv] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int n = wave_cnt[w]; if (w < wv) before += n; total += n; }
    const size_t key = (size_t)b * nkeys + blockIdx.x;
    if (t == 0) counts[key] = total;
    if (lead) {
        float* o = stage + (key * DPIX + before + __popcll(bal & ((1ull << lane) - 1ull))) * 6;
        o[0] = box[0]; o[1] = box[1]; o[2] = box[2]; o[3] = box[3]; o[4] = score; o[5] = (float)cls;
    }
}

// the gather of postproc.hip's two-pass filter, restated here because that one is local to its file
__global__ __launch_bounds__(1024) void v8_gather_kernel(const float* __restrict__ stage, const int32_t* __restrict__ counts, int nkeys,
                                                         float* __restrict__ cand, int32_t* __restrict__ ncand, int cap, int append)
{
    __shared__ int wsum[16];
    __shared__ int base_s;
    const int b = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t == 0) base_s = append ? max(ncand[b], 0) : 0;
    __syncthreads();
    float* out = cand + (size_t)b * cap * 6;
    for (int k0 = 0; k0 < nkeys; k0 += 1024) {
        const int key = k0 + t;
        const int cnt = key < nkeys ? counts[(size_t)b * nkeys + key] : 0;
        int incl = cnt;                                  // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int u = wsum[w]; if (w < wv) before += u; total += u; }
        const int base = base_s;
        int pos = base + before + incl - cnt;
        const float* src = stage + ((size_t)b * nkeys + (key < nkeys ? key : 0)) * DPIX * 6;
        for (int i = 0; i < cnt && (unsigned)pos < (unsigned)cap; ++i, ++pos) {
#pragma unroll
            for (int e = 0; e < 6; ++e) out[(size_t)pos * 6 + e] = src[i * 6 + e];
        }
        __syncthreads();
        if (t == 0) base_s = base + total;
        __syncthreads();
    }
    if (t == 0) ncand[b] = base_s;
}

// Candidate rule on a decoded (B, N, 4+nc) tensor (the argument of numba_nms, :168-196).  multi: one row per (cell, class) with
// value >= cls_thr in (cell, class) order (:186-189); else the first maximum, inclusive threshold.  A thread counts its cell's rows,
// a wave / block prefix sum places them.
__global__ __launch_bounds__(1024) void v8_filter_decoded_kernel(const float* __restrict__ dec, int N, int nc, float cls_thr, int multi,
                                                                 float* __restrict__ cand, int32_t* __restrict__ ncand, int cap)
{
    __shared__ int wave_cnt[16];
    __shared__ int base_s;
    const int b = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int E = 4 + nc;
    if (t == 0) base_s = 0;
    __syncthreads();
    float* out = cand + (size_t)b * cap * 6;
    for (int p0 = 0; p0 < N; p0 += 1024) {
        const int pi = p0 + t;
        const float* row = dec + ((size_t)b * N + (pi < N ? pi : 0)) * E;
        int cnt = 0, cls = 0;
        float best = -INFINITY;
        if (pi < N) {
            if (multi) {
                for (int c = 0; c < nc; ++c) cnt += (row[4 + c] >= cls_thr) ? 1 : 0;
            } else {
                for (int c = 0; c < nc; ++c) { const float pc = row[4 + c]; if (pc > best) { best = pc; cls = c; } }
                cnt = (best >= cls_thr) ? 1 : 0;
            }
        }
        int incl = cnt;                                   // inclusive prefix sum over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
        if (lane == 63) wave_cnt[wv] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int c = wave_cnt[w]; if (w < wv) before += c; total += c; }
        int pos = base_s + before + incl - cnt;
        if (cnt > 0) {
            const float x0 = row[0], y0 = row[1], x1 = row[2], y1 = row[3];
            for (int c = multi ? 0 : cls; c < (multi ? nc : cls + 1); ++c) {
                const float sc = row[4 + c];
                if (multi && !(sc >= cls_thr)) continue;
                if ((unsigned)pos < (unsigned)cap) {
                    float* o = out + (size_t)pos * 6;
                    o[0] = x0; o[1] = y0; o[2] = x1; o[3] = y1; o[4] = sc; o[5] = (float)c;
                }
                ++pos;
            }
        }
        __syncthreads();
        if (t == 0) base_s += total;
        __syncthreads();
    }
    if (t == 0) ncand[b] = base_s;
}

int fill_dec8(const yh_v8dec_desc* d, const void* const* preds, Dec8* k, const char* who) {
    YH_CHECK_ARG(d && preds, "%s: null desc", who);
    YH_CHECK_ARG(d->B > 0 && d->num_class >= 1, "%s: bad dims (B %d, num_class %d)", who, d->B, d->num_class);
    YH_CHECK_ARG(d->num_stage >= 1 && d->num_stage <= MAXS, "%s: num_stage %d is outside 1..4", who, d->num_stage);
    YH_CHECK_ARG(d->reg >= 2 && d->reg <= 32, "%s: reg %d is outside 2..32", who, d->reg);
    YH_CHECK_ARG(d->img_h > 0.f && d->img_h <= FLT_MAX, "%s: img_h must be positive and finite", who);
    k->d = *d;
    int acc = 0, cacc = 0;
    for (int s = 0; s <= MAXS; ++s) {
        k->start[s] = acc;
        k->cstart[s] = cacc;
        if (s == MAXS) break;
        k->pred[s] = nullptr;
        k->stride[s] = 0.f;
        if (s < d->num_stage) {
            YH_CHECK_ARG(preds[s] != nullptr && d->H[s] > 0 && d->W[s] > 0, "%s: stage %d: null tensor or empty map", who, s);
            YH_CHECK_ARG(d->ldp[s] >= 4 * d->reg + d->num_class, "%s: stage %d: ldp %d < 4*reg + num_class = %d", who, s, d->ldp[s],
                         4 * d->reg + d->num_class);
            k->pred[s] = preds[s];
            k->stride[s] = d->img_h / (float)d->H[s];
            acc += d->H[s] * d->W[s];
            cacc += (d->H[s] * d->W[s] + DPIX - 1) / DPIX;
        }
    }
    k->ntot = acc;
    return YH_OK;
}

}  // namespace

extern "C" int yh_v8_decode_full(const yh_v8dec_desc* d, const void* const* preds, float* out, yh_stream stream)
{
    Dec8 k;
    const int rc = fill_dec8(d, preds, &k, "yh_v8_decode_full");
    if (rc) return rc;
    YH_CHECK_ARG(out != nullptr, "yh_v8_decode_full: null output");
    const long tot = (long)d->B * k.ntot * (4 + d->num_class);
    const int g = (int)((tot + 255) / 256 > 8192 ? 8192 : (tot + 255) / 256);
    yh_pred_type(d->pred_is_f32, [&](auto e) {
        hipLaunchKernelGGL((v8_decode_full_kernel<decltype(e)>), dim3(g), dim3(256), 0, (hipStream_t)stream, k, out);
    });
    YH_CHECK_LAUNCH("yh_v8_decode_full");
    return YH_OK;
}

/* staging area [B][nchunk][64][6] fp32 + counts [B][nchunk] int32 of the two-pass filter */
extern "C" size_t yh_v8_decode_filter_ws_bytes(const yh_v8dec_desc* d)
{
    if (!d || d->B <= 0 || d->num_stage < 1 || d->num_stage > MAXS) return 0;
    size_t nkeys = 0;
    for (int s = 0; s < d->num_stage; ++s) {
        if (d->H[s] <= 0 || d->W[s] <= 0) return 0;
        nkeys += (size_t)((d->H[s] * d->W[s] + DPIX - 1) / DPIX);
    }
    return (size_t)d->B * nkeys * (DPIX * 6 * 4 + 4);
}

extern "C" int yh_v8_decode_filter(const yh_v8dec_desc* d, const void* const* preds, const yh_view_xform* xf, float cls_thr,
                                   float* cand, int32_t* ncand, int cap, void* ws, yh_stream stream)
{
    const char* who = "yh_v8_decode_filter";
    Dec8 k;
    const int rc = fill_dec8(d, preds, &k, who);
    if (rc) return rc;
    View8 v = {1.0f, 0, 0.f, 0.f, 0};
    if (xf) {
        YH_CHECK_ARG(xf->flip_axis == 0 || xf->flip_axis == 2 || xf->flip_axis == 3, "%s: flip_axis %d is not 0, 2 or 3", who, xf->flip_axis);
        YH_CHECK_ARG(xf->scale > 0.f && xf->scale <= FLT_MAX, "%s: scale must be positive and finite", who);
        v = View8{1.0f / xf->scale, xf->flip_axis, xf->img_h, xf->img_w, 1};
    }
    YH_CHECK_ARG(cand && ncand && cap > 0 && cap % 4 == 0, "%s: cand/ncand null or cap not a positive multiple of 4", who);
    if (!ws) {
        yh_pred_type(d->pred_is_f32, [&](auto e) {
            hipLaunchKernelGGL((v8_filter_kernel<decltype(e)>), dim3(d->B), dim3(1024), 0, (hipStream_t)stream, k, v, cls_thr, cand, ncand, cap);
        });
        YH_CHECK_LAUNCH(who);
        return YH_OK;
    }
    YH_CHECK_ARG(yh_aligned16(ws), "%s: workspace unaligned", who);
    const int nkeys = k.cstart[MAXS];
    float* stage = reinterpret_cast<float*>(ws);
    int32_t* counts = reinterpret_cast<int32_t*>(stage + (size_t)d->B * nkeys * DPIX * 6);
    int ldmax = 0;
    for (int s = 0; s < d->num_stage; ++s) ldmax = d->ldp[s] > ldmax ? d->ldp[s] : ldmax;
    const size_t sm = 16 + (size_t)DPIX * ((size_t)ldmax * (d->pred_is_f32 ? 4 : 2) + 16);      // wave counts, then rows padded by 16 bytes
    YH_CHECK_ARG(sm <= 160 * 1024, "%s: head rows of %d elements do not fit the LDS tile", who, ldmax);
    YH_CHECK_ARG(d->B <= 65535, "%s: B %d exceeds the grid's y extent", who, d->B);
    char label[64];
    yh_pred_type(d->pred_is_f32, [&](auto e) {
        using T = decltype(e);
        static YhDevOnce attr;          // one per element type: the attribute belongs to the instantiation
        yh_lds_limit(attr, {{(const void*)v8_scan_kernel<T>, 160 * 1024}});
        hipLaunchKernelGGL((v8_scan_kernel<T>), dim3(nkeys, d->B), dim3(256), sm, (hipStream_t)stream, k, v, cls_thr, stage, counts, nkeys);
    });
    snprintf(label, sizeof(label), "%s(scan)", who);
    YH_CHECK_LAUNCH(label);
    hipLaunchKernelGGL(v8_gather_kernel, dim3(d->B), dim3(1024), 0, (hipStream_t)stream, stage, counts, nkeys, cand, ncand, cap, v.append);
    snprintf(label, sizeof(label), "%s(gather)", who);
    YH_CHECK_LAUNCH(label);
    return YH_OK;
}

extern "C" int yh_v8_filter_decoded(const float* dec, int B, int N, int num_class, float cls_thr, int multi_label,
                                    float* cand, int32_t* ncand, int cap, yh_stream stream)
{
    YH_CHECK_ARG(dec && cand && ncand, "yh_v8_filter_decoded: null pointer");
    YH_CHECK_ARG(B > 0 && N > 0 && num_class >= 1 && cap > 0 && cap % 4 == 0, "yh_v8_filter_decoded: bad dims or cap not a positive multiple of 4");
    YH_CHECK_ARG(multi_label == 0 || multi_label == 1, "yh_v8_filter_decoded: multi_label must be 0 or 1");
    hipLaunchKernelGGL(v8_filter_decoded_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, dec, N, num_class, cls_thr, multi_label, cand, ncand, cap);
    YH_CHECK_LAUNCH("yh_v8_filter_decoded");
    return YH_OK;
}
