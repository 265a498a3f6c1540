// YOLOv7 loss on gfx950 (loss/yolov7_loss.py:17-402 of the reference), on the same anchor heads as the YOLOv5 loss:
//   candidates — yh_v5_assign (loss_v5.hip) on the embedded v5 descriptor: YOLOV7Loss.match (:166-242) is YOLOV5Loss.match.  The
//                result is a LIST per stage: a cell may appear more than once and every copy is a candidate of its own.
//   cand       — per candidate: decode the box to pixels (:283-289), sigmoid(obj) and the class cost against an all-zero target,
//                sum_c BCE(z_c, 0) with z_c = logit(sqrt(sigmoid(cls_c) * sigmoid(obj))) (:325-331).
//   runs       — the starts of the runs of equal image id in each stage's list: the list is ordered (neighbour, anchor, image,
//                row), so an image's candidates are at most 5 * A runs of consecutive entries.
//   simota     — one workgroup per (image, stage) (simple_ota, :293-372): the image's candidates (the index ranges of its runs)
//                and valid rows are gathered in order; one wave per target row forms the row of -log(iou + 1e-9) in LDS, takes dynamic_k from its min(topk, Xp)
//                LARGEST entries (:315-316), turns the row into costs in place and claims its dynamic_k smallest.  A pair's class
//                cost is the candidate's all-zero sum with the target's class switched to 1: O(1) per pair.  A candidate claimed
//                once goes to its claimant; one claimed more than once goes to the arg-min of its cost over ALL valid rows (:346).
//                No cost matrix is stored: LDS holds one row per wave.
//   compact    — order-preserving ballot compaction of the kept candidates into the matched list, with the target box in stage
//                units relative to the candidate's cell (:359-363).
//   pos_fwd / obj_fwd / finalize / obj_bwd / pos_bwd — the scheme of loss_v5.hip over the matched list; what differs from v5: class
//                targets 0.95 / 0.05, the objectness sum is divided by max(N, 1) instead of the cell count, the objectness target
//                may be the constant 1, and a stage without a matched row adds no class term.
// Ties (the reference leaves them to torch.topk / torch.min): equal costs go to the lower candidate index, equal costs between
// targets to the lower target row.  Out of contract: where sqrt(sigmoid(cls) * sigmoid(obj)) rounds to 1 the reference's logit is
// infinite and its cost inf or NaN; a NaN cost is never selected here.
// Every index is bounded by a capacity from the descriptor (cap rows per stage, MAXC candidates and MAXG valid rows per
// (image, stage)), never by a count read from memory alone.
#include "exact_math.h"

namespace {

constexpr int MAXS = 4;
constexpr int MAXG = 128;               // valid rows of an image (include/yolohip.h)
constexpr int MAXC = 5 * 3 * MAXG;      // candidates of one (image, stage): 5 neighbours x 3 anchors x MAXG rows
constexpr int PART_BLOCKS = 1024;       // partial-sum slots per (stage, kind)
constexpr int RUNS_AT = 8;               // ccount[RUNS_AT + s]: runs of stage s (ccount[s]: its candidates)
constexpr float CLS_POS = 0.95f, CLS_NEG = 0.05f;     // smooth_bce() with its default eps (:11-13, :38)

struct Cand {                           // 32 bytes per candidate, written by cand, read by simota
    float box[4];                       // xyxy pixels
    float clsbase, sobj;                // sum_c BCE(z_c, 0); sigmoid(obj)
    int32_t pix, anc;                   // (img * H + gy) * W + gx, -1: not a candidate of any image; anchor
};

struct Layout {                         // byte offsets inside `saved` (s_*) and `ws` (w_*)
    size_t s_count, s_bal_used, s_tbox, s_tidx, s_ciou, s_next, s_head, s_total;
    size_t w_part, w_ccount, w_ctbox, w_ctidx, w_cand, w_mt, w_runs, w_total;
    size_t head_off[MAXS];              // element offsets of each stage inside head
    int cap;                            // rows per stage of every list
    int ncell[MAXS];
};

Layout make_layout(const yh_v5loss_desc& d) {
    Layout L;
    L.cap = 5 * d.num_anchor * d.B * d.maxbox;
    const size_t rows = (size_t)d.num_stage * L.cap;
    size_t o = 0;
    L.s_count = o; o += 64;
    L.s_bal_used = o; o += 64;
    L.s_tbox = o; o += rows * 4 * sizeof(float);
    L.s_tidx = o; o += rows * 6 * sizeof(int32_t);          // (cls, img, anchor, gy, gx, target row)
    L.s_ciou = o; o += rows * sizeof(float);
    L.s_next = o; o += rows * sizeof(int32_t);
    o = (o + 255) & ~(size_t)255;
    L.s_head = o;
    size_t e = 0;
    for (int s = 0; s < d.num_stage; ++s) {
        L.head_off[s] = e;
        L.ncell[s] = d.B * d.num_anchor * d.H[s] * d.W[s];
        e += L.ncell[s];
    }
    o += e * sizeof(int32_t);
    L.s_total = (o + 255) & ~(size_t)255;
    o = 0;
    L.w_part = o; o += sizeof(double) * MAXS * 3 * PART_BLOCKS;
    L.w_ccount = o; o += 64;
    L.w_ctbox = o; o += rows * 4 * sizeof(float);
    L.w_ctidx = o; o += rows * 5 * sizeof(int32_t);
    o = (o + 31) & ~(size_t)31;
    L.w_cand = o; o += rows * sizeof(Cand);
    L.w_mt = o; o += rows * sizeof(int32_t);
    L.w_runs = o; o += rows * sizeof(int32_t);
    L.w_total = (o + 255) & ~(size_t)255;
    return L;
}

struct LossK {
    yh_v5loss_desc d;
    Layout L;
    int topk, iou_cof;
};

struct Stage {
    const void* pred;
    void* gpred;
    int s, H, W, ld;
};
struct Stages { Stage s[4]; };

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }

// ---------------------------------------------------------------- per candidate: pixel box, sigmoid(obj), all-zero class cost
template <typename T>
__global__ __launch_bounds__(256) void v7_cand_kernel(const LossK p, const Stages sts, const int32_t* __restrict__ ccount,
                                                      const int32_t* __restrict__ ctidx, Cand* __restrict__ cand)
{
    const Stage st = sts.s[blockIdx.y];
    const yh_v5loss_desc& d = p.d;
    const int s = st.s, E = 5 + d.num_class;
    const int NC = imin(ccount[s], p.L.cap);
    const T* pred = reinterpret_cast<const T*>(st.pred);
    const float ds = d.img_size1 / (float)st.W;                  // :78 ds_scale, used for x and y alike
    for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < NC; n += gridDim.x * blockDim.x) {
        const int32_t* ii = ctidx + ((size_t)s * p.L.cap + n) * 5;
        const int img = ii[1], anc = ii[2], gy = ii[3], gx = ii[4];
        Cand c;
        c.box[0] = c.box[1] = c.box[2] = c.box[3] = 0.f; c.clsbase = 0.f; c.sobj = 0.f; c.pix = -1; c.anc = 0;
        if (img >= 0 && img < d.B && anc >= 0 && anc < d.num_anchor && gy >= 0 && gy < st.H && gx >= 0 && gx < st.W) {
            c.pix = (img * st.H + gy) * st.W + gx;
            c.anc = anc;
            const T* row = pred + (size_t)c.pix * st.ld + anc * E;
            const float aw = d.anchors[s][anc][0] / ds, ah = d.anchors[s][anc][1] / ds;      // :81 anchor_stage
            const float px = ((sigm(ldf<T>(row + 0)) * 2.f - 0.5f) + (float)gx) * ds;            // :283
            const float py = ((sigm(ldf<T>(row + 1)) * 2.f - 0.5f) + (float)gy) * ds;
            const float t2 = sigm(ldf<T>(row + 2)) * 2.f, t3 = sigm(ldf<T>(row + 3)) * 2.f;
            const float pw = t2 * t2 * aw * ds, ph = t3 * t3 * ah * ds;                         // :285
            c.box[0] = px - pw / 2.f; c.box[1] = py - ph / 2.f; c.box[2] = px + pw / 2.f; c.box[3] = py + ph / 2.f;
            c.sobj = sigm(ldf<T>(row + 4));
            float acc = 0.f;
            for (int e = 5; e < E; ++e) {
                const float pr = sqrtf(sigm(ldf<T>(row + e)) * c.sobj);
                acc += bce_logits(logf(pr / (1.f - pr)), 0.f, 1.f, nullptr, nullptr);
            }
            c.clsbase = acc;
        }
        cand[(size_t)s * p.L.cap + n] = c;
    }
}

// -log(gpu_iou + 1e-9) of a target and a candidate box, xyxy pixels (utils/bbox_tools.py:164-190: the union is clamped at 1e-9)
__device__ __forceinline__ float pair_neg(const float* tb, const Cand& c) {
    const float a1 = (tb[2] - tb[0]) * (tb[3] - tb[1]);
    const float a2 = (c.box[2] - c.box[0]) * (c.box[3] - c.box[1]);
    const float iw = fmaxf(fminf(tb[2], c.box[2]) - fmaxf(tb[0], c.box[0]), 0.f);
    const float ih = fmaxf(fminf(tb[3], c.box[3]) - fmaxf(tb[1], c.box[1]), 0.f);
    const float inter = iw * ih;
    const float iou = inter / fmaxf(a1 + a2 - inter, 1e-9f);
    return -logf(iou + 1e-9f);
}
// sum_c BCE(z_c, onehot(cls)_c): the candidate's all-zero sum with the target's class switched from 0 to 1
template <typename T>
__device__ __forceinline__ float pair_cls(const T* pred, int ld, int E, const Cand& c, int cls) {
    if (cls < 0 || cls >= E - 5 || c.pix < 0) return c.clsbase;
    const float x = ldf<T>(pred + (size_t)c.pix * ld + c.anc * E + 5 + cls);
    const float pr = sqrtf(sigm(x) * c.sobj);
    const float z = logf(pr / (1.f - pr));
    return c.clsbase - bce_logits(z, 0.f, 1.f, nullptr, nullptr) + bce_logits(z, 1.f, 1.f, nullptr, nullptr);
}
template <typename T>
__device__ __forceinline__ float pair_cost(const T* pred, int ld, int E, const float* tb, int cls, const Cand& c) {
    return 3.f * pair_neg(tb, c) + pair_cls<T>(pred, ld, E, c, cls);                  // :335
}

// the wave's entry that comes first: LARGEST (value, then lower index) or smallest (value, then lower index); index -1: none
template <bool LARGEST>
__device__ __forceinline__ bool comes_first(float v, int i, float bv, int bi) {
    if (i < 0) return false;
    if (bi < 0) return true;
    return (LARGEST ? v > bv : v < bv) || (v == bv && i < bi);
}
template <bool LARGEST>
__device__ __forceinline__ void wave_first(float& bv, int& bi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (comes_first<LARGEST>(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
}
// the next entry of row[0..n) in the order (LARGEST: descending value | else ascending value, then ascending index) after
// (pv, pi); pi < 0: the first.  NaN entries are never returned.  All lanes of the wave get the same answer.
template <bool LARGEST>
__device__ __forceinline__ void row_next(const float* row, int n, int lane, float pv, int pi, float& bv, int& bi) {
    bv = 0.f; bi = -1;
    for (int c = lane; c < n; c += 64) {
        const float v = row[c];
        if (v != v) continue;
        const bool after = pi < 0 || (LARGEST ? v < pv : v > pv) || (v == pv && c > pi);
        if (after && comes_first<LARGEST>(v, c, bv, bi)) { bv = v; bi = c; }
    }
    wave_first<LARGEST>(bv, bi);
}

// ---------------------------------------------------------------- runs of equal image id in a stage's candidate list
// runs[s][r] = index of the first entry of run r (order-preserving ballot compaction of the run starts), ccount[RUNS_AT + s] = runs
__global__ __launch_bounds__(1024) void v7_runs_kernel(const LossK p, const int32_t* __restrict__ ctidx, int32_t* __restrict__ ccount,
                                                       int32_t* __restrict__ runs)
{
    __shared__ int wave_cnt[16];
    __shared__ int base_s;
    const int s = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int NC = imin(ccount[s], p.L.cap);
    const int32_t* ci = ctidx + (size_t)s * p.L.cap * 5;
    int32_t* out = runs + (size_t)s * p.L.cap;
    if (t == 0) base_s = 0;
    __syncthreads();
    for (int q0 = 0; q0 < NC; q0 += 1024) {
        const int q = q0 + t;
        const bool flag = q < NC && (q == 0 || ci[(size_t)q * 5 + 1] != ci[(size_t)(q - 1) * 5 + 1]);
        const unsigned long long bal = __ballot(flag);
        const int within = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wv] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int c = wave_cnt[w];
            if (w < wv) before += c;
            total += c;
        }
        const int base = base_s;
        if (flag) out[base + before + within] = q;           // position <= q < cap
        __syncthreads();
        if (t == 0) base_s = base + total;
        __syncthreads();
    }
    if (t == 0) ccount[RUNS_AT + s] = base_s;
}

// ---------------------------------------------------------------- SimOTA over the candidates of one (image, stage)
template <typename T>
__global__ __launch_bounds__(256) void v7_simota_kernel(const LossK p, const Stages sts, const float* __restrict__ targets,
                                                        const int32_t* __restrict__ ccount, const int32_t* __restrict__ ctidx,
                                                        const Cand* __restrict__ cand, const int32_t* __restrict__ runs,
                                                        int32_t* __restrict__ mt)
{
    __shared__ int lidx[MAXC];              // the image's candidates, in order: index into the stage's list
    __shared__ int claim[MAXC], who[MAXC];  // how many targets took the candidate, and one of them
    __shared__ float rows[4][MAXC];         // one row of the (target, candidate) matrix per wave
    __shared__ float tbx[MAXG][4];
    __shared__ int tcl[MAXG], trw[MAXG];
    __shared__ int wave_cnt[4];
    __shared__ int run_q[256], run_n[256];  // the runs of this image found in one step over the run list
    __shared__ int base_s, nt_s;
    const Stage st = sts.s[blockIdx.y];
    const yh_v5loss_desc& d = p.d;
    const int b = blockIdx.x, s = st.s, E = 5 + d.num_class, MB = d.maxbox;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int NC = imin(ccount[s], p.L.cap);
    const int CI = imin(5 * d.num_anchor * imin(MB, MAXG), MAXC);
    const T* pred = reinterpret_cast<const T*>(st.pred);
    const int32_t* ci = ctidx + (size_t)s * p.L.cap * 5;
    const Cand* cd = cand + (size_t)s * p.L.cap;
    const int NR = imin(ccount[RUNS_AT + s], p.L.cap);
    const int32_t* rl = runs + (size_t)s * p.L.cap;
    if (t == 0) base_s = 0;
    // valid rows of the image (:294), in order
    if (wv == 0) {
        int base = 0;
        for (int j0 = 0; j0 < MB; j0 += 64) {
            const int j = j0 + lane;
            const float* tg = targets + ((size_t)b * MB + (j < MB ? j : 0)) * 6;
            const bool ok = j < MB && tg[4] >= 0.f;
            const unsigned long long bal = __ballot(ok);
            const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
            if (ok && pos < MAXG) {
                tbx[pos][0] = tg[0]; tbx[pos][1] = tg[1]; tbx[pos][2] = tg[2]; tbx[pos][3] = tg[3];
                tcl[pos] = (int)tg[4]; trw[pos] = j;
            }
            base += __popcll(bal);
        }
        if (lane == 0) nt_s = imin(base, MAXG);
    }
    __syncthreads();
    // candidates of the image (:295), in order.  The stage's list is ordered (neighbour, anchor, image, row), so an image's
    // candidates are a few runs of consecutive entries (v7_runs_kernel lists every run's start): the block reads the run
    // list, 5 * A * B entries at most for well-formed image ids, and copies the index ranges of its own runs
    for (int r0 = 0; r0 < NR; r0 += 256) {
        const int r = r0 + t;
        int q = 0, n = 0;
        bool flag = false;
        if (r < NR) {
            q = rl[r];
            const int e = r + 1 < NR ? rl[r + 1] : NC;
            if (q >= 0 && q < e && e <= NC) { flag = ci[(size_t)q * 5 + 1] == b; n = e - q; }
        }
        const unsigned long long bal = __ballot(flag);
        const int within = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wv] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c = wave_cnt[w];
            if (w < wv) before += c;
            total += c;
        }
        if (flag) { run_q[before + within] = q; run_n[before + within] = n; }
        __syncthreads();
        int base = base_s;
        for (int i = 0; i < total; ++i) {                     // uniform over the block
            const int rq = run_q[i], rn = run_n[i];
            for (int c = t; c < rn && base + c < CI; c += 256) { lidx[base + c] = rq + c; claim[base + c] = 0; who[base + c] = -1; }
            base = imin(base + rn, CI);
        }
        __syncthreads();
        if (t == 0) base_s = base;
        __syncthreads();
    }
    const int Xp = imin(base_s, CI), Xt = nt_s;
    if (Xp == 0 || Xt == 0) return;                          // the reference reaches k = 0 and matches nothing
    const int kk = imin(p.topk, Xp);
    float* row = rows[wv];
    for (int t0 = 0; t0 < Xt; t0 += 4) {                      // uniform over the block: the barriers below are reached by all
        const int ti = t0 + wv;
        const bool act = ti < Xt;
        if (act) for (int c = lane; c < Xp; c += 64) row[c] = pair_neg(tbx[ti], cd[lidx[c]]);
        __syncthreads();
        int dynk = 0;
        if (act) {
            // :315-316 sum of the kk LARGEST -log(iou) values, truncated, clamped to [1, kk]
            float sum = 0.f, pv = 0.f;
            int pi = -1;
            for (int r = 0; r < kk; ++r) {
                float bv; int bi;
                row_next<true>(row, Xp, lane, pv, pi, bv, bi);
                if (bi < 0) break;
                sum += bv; pv = bv; pi = bi;
            }
            const float cl = fminf(fmaxf(sum, -1.0e9f), 1.0e9f);
            dynk = sum != sum ? 1 : (int)cl;
            dynk = dynk < 1 ? 1 : (dynk > kk ? kk : dynk);
        }
        __syncthreads();
        if (act) for (int c = lane; c < Xp; c += 64) row[c] = 3.f * row[c] + pair_cls<T>(pred, st.ld, E, cd[lidx[c]], tcl[ti]);
        __syncthreads();
        if (act) {
            float pv = 0.f;
            int pi = -1;
            for (int r = 0; r < dynk; ++r) {                  // :339 the dynk smallest costs
                float bv; int bi;
                row_next<false>(row, Xp, lane, pv, pi, bv, bi);
                if (bi < 0) break;
                if (lane == 0) { atomicAdd(&claim[bi], 1); who[bi] = ti; }
                pv = bv; pi = bi;
            }
        }
        __syncthreads();
    }
    // :344-351 one target per claimed candidate
    for (int c = t; c < Xp; c += 256) {
        const int n = claim[c];
        if (n == 0) continue;
        int m = who[c];
        if (n > 1) {
            const Cand cc = cd[lidx[c]];
            float bv = 0.f;
            m = -1;
            for (int ti = 0; ti < Xt; ++ti) {
                const float v = pair_cost<T>(pred, st.ld, E, tbx[ti], tcl[ti], cc);
                if (v == v && (m < 0 || v < bv)) { bv = v; m = ti; }
            }
        }
        if (m >= 0 && m < Xt) mt[(size_t)s * p.L.cap + lidx[c]] = trw[m];
    }
}

// ---------------------------------------------------------------- matched list, in candidate order
__global__ __launch_bounds__(1024) void v7_compact_kernel(const LossK p, const float* __restrict__ targets,
                                                          const int32_t* __restrict__ ccount, const int32_t* __restrict__ ctidx,
                                                          const int32_t* __restrict__ mt, int32_t* __restrict__ count,
                                                          float* __restrict__ tbox, int32_t* __restrict__ tidx)
{
    __shared__ int wave_cnt[16];
    __shared__ int base_s;
    const yh_v5loss_desc& d = p.d;
    const int s = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int NC = imin(ccount[s], p.L.cap);
    const float fw = (float)d.W[s], fh = (float)d.H[s];
    const int32_t* ci = ctidx + (size_t)s * p.L.cap * 5;
    const int32_t* ms = mt + (size_t)s * p.L.cap;
    float* ob = tbox + (size_t)s * p.L.cap * 4;
    int32_t* oi = tidx + (size_t)s * p.L.cap * 6;
    if (t == 0) base_s = 0;
    __syncthreads();
    for (int q0 = 0; q0 < NC; q0 += 1024) {
        const int q = q0 + t;
        int m = -1, img = 0;
        if (q < NC) {
            m = ms[q];
            img = ci[(size_t)q * 5 + 1];
            if (m >= d.maxbox || img < 0 || img >= d.B) m = -1;
        }
        const bool flag = m >= 0;
        const unsigned long long bal = __ballot(flag);
        const int within = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wv] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int c = wave_cnt[w];
            if (w < wv) before += c;
            total += c;
        }
        const int base = base_s;
        if (flag) {
            const int pos = base + before + within;          // <= q < cap
            const int32_t* ii = ci + (size_t)q * 5;
            const int gy = ii[3], gx = ii[4];
            const float* tg = targets + ((size_t)img * d.maxbox + m) * 6;
            const float x1 = tg[0], y1 = tg[1], x2 = tg[2], y2 = tg[3];
            // :361-363 xyxy2xywhn (utils/bbox_tools.py:103-119), * fm size, minus the cell
            const float gxf = (((x1 + x2) / 2.0f) / d.img_size0) * fw, gyf = (((y1 + y2) / 2.0f) / d.img_size1) * fh;
            float* bb = ob + (size_t)pos * 4;
            bb[0] = gxf - (float)gx; bb[1] = gyf - (float)gy;
            bb[2] = ((x2 - x1) / d.img_size0) * fw; bb[3] = ((y2 - y1) / d.img_size1) * fh;
            int32_t* oo = oi + (size_t)pos * 6;
            oo[0] = (int)tg[4]; oo[1] = img; oo[2] = ii[2]; oo[3] = gy; oo[4] = gx; oo[5] = m;
        }
        __syncthreads();
        if (t == 0) base_s = base + total;
        __syncthreads();
    }
    if (t == 0) count[s] = base_s;
}

// Decode the predicted box of one matched row in stage units and evaluate CIoU (+ grads w.r.t. the 4 logits) (:122-130)
__device__ __forceinline__ float pos_box(const yh_v5loss_desc& d, int s, int anc, const float* lg, const float* tb,
                                         float* dlogit /*4 or null*/)
{
    const float ds = d.img_size1 / (float)d.W[s];
    const float aw = d.anchors[s][anc][0] / ds, ah = d.anchors[s][anc][1] / ds;
    const float s0 = sigm(lg[0]), s1 = sigm(lg[1]), s2 = sigm(lg[2]), s3 = sigm(lg[3]);
    const float px = s0 * 2.f - 0.5f, py = s1 * 2.f - 0.5f;
    const float t2 = s2 * 2.f, t3 = s3 * 2.f;
    const float pw = t2 * t2 * aw, ph = t3 * t3 * ah;
    const float b1[4] = {px - pw / 2.f, py - ph / 2.f, px + pw / 2.f, py + ph / 2.f};
    const float b2[4] = {tb[0] - tb[2] / 2.f, tb[1] - tb[3] / 2.f, tb[0] + tb[2] / 2.f, tb[1] + tb[3] / 2.f};
    float g[4];
    const float c = ciou_fwd_bwd(b1, b2, dlogit ? g : nullptr);
    if (dlogit) {
        const float dpx = g[0] + g[2], dpy = g[1] + g[3];
        const float dpw = (g[2] - g[0]) / 2.f, dph = (g[3] - g[1]) / 2.f;
        dlogit[0] = dpx * 2.f * s0 * (1.f - s0);
        dlogit[1] = dpy * 2.f * s1 * (1.f - s1);
        dlogit[2] = dpw * (2.f * t2 * aw) * (2.f * s2 * (1.f - s2));
        dlogit[3] = dph * (2.f * t3 * ah) * (2.f * s3 * (1.f - s3));
    }
    return c;
}

// ---------------------------------------------------------------- matched rows, forward (16 lanes per row)
template <typename T>
__global__ __launch_bounds__(256) void v7_pos_fwd_kernel(const LossK p, const Stages sts, const int32_t* __restrict__ count,
                                                         const float* __restrict__ tbox, const int32_t* __restrict__ tidx,
                                                         float* __restrict__ ciou_out, int32_t* __restrict__ next,
                                                         int32_t* __restrict__ head, double* __restrict__ part)
{
    const Stage st = sts.s[blockIdx.y];
    __shared__ double sred[2][4];
    const yh_v5loss_desc& d = p.d;
    const int s = st.s;
    const int N = imin(count[s], p.L.cap);
    const int E = 5 + d.num_class;
    const int t = threadIdx.x, sub = t & 15, grp = t >> 4;
    const T* pred = reinterpret_cast<const T*>(st.pred);
    double acc[2] = {0.0, 0.0};          // iou, class
    for (int n = blockIdx.x * 16 + grp; n < N; n += gridDim.x * 16) {
        const int32_t* ii = tidx + ((size_t)s * p.L.cap + n) * 6;
        const float* tb = tbox + ((size_t)s * p.L.cap + n) * 4;
        const int cls = ii[0], img = ii[1], anc = ii[2], gy = ii[3], gx = ii[4];
        const T* row = pred + (((size_t)img * st.H + gy) * st.W + gx) * st.ld + anc * E;
        float lg[4];
        {
            float mine = (sub < 4) ? ldf<T>(row + sub) : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) lg[i] = __shfl(mine, i, 16);
        }
        const float c = pos_box(d, s, anc, lg, tb, nullptr);
        float cls_sum = 0.f;
        for (int e = 5 + sub; e < E; e += 16) {                // :104-114
            const float x = ldf<T>(row + e);
            const float tt = (e - 5 == cls) ? CLS_POS : CLS_NEG;
            float l = bce_logits(x, tt, d.cls_pos_weight, nullptr, nullptr);
            if (d.use_focal) l *= focal_factor(x, tt, d.focal_gamma, d.focal_alpha, nullptr, nullptr);
            cls_sum += l;
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) cls_sum += __shfl_xor(cls_sum, o, 16);
        if (sub == 0) {
            ciou_out[(size_t)s * p.L.cap + n] = c;
            acc[0] += (double)(1.0f - c);
            acc[1] += (double)cls_sum;
            const int cell = ((img * d.num_anchor + anc) * st.H + gy) * st.W + gx;
            const int prev = atomicExch(head + p.L.head_off[s] + cell, n);
            next[(size_t)s * p.L.cap + n] = prev;
        }
    }
    block_partials(acc, sred);
    if (t == 0) {
        part[((size_t)s * 3 + 0) * PART_BLOCKS + blockIdx.x] = block_total(sred[0]);
        part[((size_t)s * 3 + 1) * PART_BLOCKS + blockIdx.x] = block_total(sred[1]);
    }
}

// largest row index in a cell's list == the last writer of t_cof[...] (:134-136); bounded by the list capacity
__device__ __forceinline__ int list_max(const int32_t* next, int h, int cap) {
    int m = h;
    for (int it = 0; h >= 0 && h < cap && it < cap; ++it) { m = h > m ? h : m; h = next[h]; }
    return m;
}
// objectness target of a cell whose list starts at h (:133-136)
__device__ __forceinline__ float cof_target(const LossK& p, const float* ci, const int32_t* nx, int h) {
    if (h < 0 || h >= p.L.cap) return 0.f;
    return p.iou_cof ? fmaxf(ci[list_max(nx, h, p.L.cap)], 0.f) : 1.0f;
}

// ---------------------------------------------------------------- objectness, forward
template <typename T>
__global__ __launch_bounds__(256) void v7_obj_fwd_kernel(const LossK p, const Stages sts, const float* __restrict__ ciou,
                                                         const int32_t* __restrict__ next, const int32_t* __restrict__ head,
                                                         double* __restrict__ part)
{
    const Stage st = sts.s[blockIdx.y];
    __shared__ double sred[1][4];
    const yh_v5loss_desc& d = p.d;
    const int s = st.s, A = d.num_anchor, E = 5 + d.num_class;
    const int ncell = p.L.ncell[s];
    const T* pred = reinterpret_cast<const T*>(st.pred);
    const int32_t* hd = head + p.L.head_off[s];
    const int32_t* nx = next + (size_t)s * p.L.cap;
    const float* ci = ciou + (size_t)s * p.L.cap;
    double acc[1] = {0.0};
    // thread index enumerates (img, y, x, a) with a fastest so that neighbouring lanes share cache lines
    for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < ncell; id += gridDim.x * blockDim.x) {
        const int a = id % A;
        const int pix = id / A;                               // (img*H + y)*W + x
        const int x = pix % st.W;
        const int r2 = pix / st.W;
        const int y = r2 % st.H;
        const int img = r2 / st.H;
        const float lg = ldf<T>(pred + (size_t)pix * st.ld + a * E + 4);
        const float tt = cof_target(p, ci, nx, hd[((img * A + a) * st.H + y) * st.W + x]);
        float l = bce_logits(lg, tt, d.cof_pos_weight, nullptr, nullptr);
        if (d.use_focal) l *= focal_factor(lg, tt, d.focal_gamma, d.focal_alpha, nullptr, nullptr);
        acc[0] += (double)l;
    }
    block_partials(acc, sred);
    if (threadIdx.x == 0) part[((size_t)s * 3 + 2) * PART_BLOCKS + blockIdx.x] = block_total(sred[0]);
}

// ---------------------------------------------------------------- finalize (:145-154)
__global__ __launch_bounds__(1024) void v7_finalize_kernel(const LossK p, const int32_t* __restrict__ count, const double* __restrict__ part,
                                                           int nb_pos, int nb_obj, double* balances, double* bal_used, float* result)
{
    // deterministic tree: wave w sums the strided partials of (stage, kind) = w; lanes combine in fixed order
    __shared__ double ssum[MAXS * 3];
    const yh_v5loss_desc& d = p.d;
    const int S = d.num_stage;
    {
        const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
        if (wv < S * 3) {
            const int kind = wv % 3;
            const int n = kind == 2 ? nb_obj : nb_pos;
            double a = 0.0;
            for (int i = lane; i < n; i += 64) a += part[(size_t)wv * PART_BLOCKS + i];
            a = wave_sum_d(a);
            if (lane == 0) ssum[wv] = a;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double s3 = 3.0 / S;
    double iou_loss = 0.0, cof_loss = 0.0, cls_loss = 0.0;
    long tar = 0;
    for (int s = 0; s < S; ++s) {
        const double a = ssum[s * 3 + 0], b = ssum[s * 3 + 1], c = ssum[s * 3 + 2];
        const int N = imin(count[s], p.L.cap);
        tar += N;
        if (N > 0) {
            cls_loss += (double)(float)(b / ((double)N * d.num_class));
            iou_loss += (double)(float)(a / N);
        }
        const double cof_sum = (double)(float)(c / (double)(N > 1 ? N : 1));
        const double bal = balances[s];
        bal_used[s] = bal;
        const double cof_tmp = (double)(float)(cof_sum * bal);
        balances[s] = bal * 0.9999 + 0.0001 / cof_tmp;        // :147
        cof_loss += cof_tmp;
    }
    const double b1 = balances[1];
    for (int s = 0; s < S; ++s) balances[s] /= b1;            // :150
    iou_loss *= d.iou_scale * s3;
    cof_loss *= d.cof_scale * s3 * (S == 3 ? 1.0 : 1.4);
    cls_loss *= d.cls_scale * s3;
    result[0] = (float)((iou_loss + cof_loss + cls_loss) * d.B);
    result[1] = (float)(iou_loss * d.B);
    result[2] = (float)(cof_loss * d.B);
    result[3] = (float)(cls_loss * d.B);
    result[4] = (float)tar;
    result[5] = result[6] = result[7] = 0.f;
}

// ---------------------------------------------------------------- backward
// Whole gradient tensor = zeros + objectness gradients, streamed once: a block walks tiles of 64 pixels, one thread per
// (pixel, anchor) evaluates the objectness gradient into LDS, then all threads write the tile's 16-byte chunks.
template <typename T>
__global__ __launch_bounds__(256) void v7_obj_bwd_kernel(const LossK p, const Stages sts, const float* __restrict__ gout,
                                                         const int32_t* __restrict__ count, const double* __restrict__ bal_used,
                                                         const float* __restrict__ ciou, const int32_t* __restrict__ next,
                                                         const int32_t* __restrict__ head)
{
    const Stage st = sts.s[blockIdx.y];
    constexpr int TP = 64;                 // pixels per tile
    __shared__ float sG[TP * 4];
    const yh_v5loss_desc& d = p.d;
    const int s = st.s, A = d.num_anchor, E = 5 + d.num_class;
    const int cpr = st.ld / 8;
    const int npix = d.B * st.H * st.W;
    const int t = threadIdx.x;
    const T* pred = reinterpret_cast<const T*>(st.pred);
    T* gp = reinterpret_cast<T*>(st.gpred);
    const int32_t* hd = head + p.L.head_off[s];
    const int32_t* nx = next + (size_t)s * p.L.cap;
    const float* ci = ciou + (size_t)s * p.L.cap;
    const double s3 = 3.0 / d.num_stage;
    const int N = imin(count[s], p.L.cap);
    const float coef = (float)((double)(*gout) * d.B * d.cof_scale * s3 * (d.num_stage == 3 ? 1.0 : 1.4) * bal_used[s] / (double)(N > 1 ? N : 1));
    const int ntile = (npix + TP - 1) / TP;
    for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int pix0 = tile * TP;
        if (t < TP * A) {
            const int pl = t / A, a = t - pl * A;
            const int pix = pix0 + pl;
            float gv = 0.f;
            if (pix < npix) {
                const int x = pix % st.W;
                const int r2 = pix / st.W;
                const int y = r2 % st.H;
                const int img = r2 / st.H;
                const float lg = ldf<T>(pred + (size_t)pix * st.ld + a * E + 4);
                const float tt = cof_target(p, ci, nx, hd[((img * A + a) * st.H + y) * st.W + x]);
                float dl, df = 0.f, f = 1.f;
                const float l = bce_logits(lg, tt, d.cof_pos_weight, &dl, nullptr);
                if (d.use_focal) f = focal_factor(lg, tt, d.focal_gamma, d.focal_alpha, &df, nullptr);
                gv = coef * (dl * f + l * df);
            }
            sG[pl * 4 + a] = gv;
        }
        __syncthreads();
        for (int i = t; i < TP * cpr; i += 256) {
            const int pl = i / cpr;
            const int c0 = (i - pl * cpr) * 8;
            const int pix = pix0 + pl;
            if (pix >= npix) break;
            float g[8];
#pragma unroll
            for (int e2 = 0; e2 < 8; ++e2) g[e2] = 0.f;
            for (int a = 0; a < A; ++a) {                       // objectness channels are a*E+4
                const int ch = a * E + 4;
                if (ch >= c0 && ch < c0 + 8) g[ch - c0] = sG[pl * 4 + a];
            }
            T* dst = gp + (size_t)pix * st.ld + c0;
            if (sizeof(T) == 2) {
                *reinterpret_cast<uint4*>(dst) = pack8(g);
            } else {
                float4* d4 = reinterpret_cast<float4*>(dst);
                d4[0] = make_float4(g[0], g[1], g[2], g[3]);
                d4[1] = make_float4(g[4], g[5], g[6], g[7]);
            }
        }
        __syncthreads();
    }
}

// The member with the largest row index of each cell list sums the gradients of all members (ascending row order: the copies of
// a duplicated cell each contribute) and writes the cell's non-objectness channels.
template <typename T>
__global__ __launch_bounds__(256) void v7_pos_bwd_kernel(const LossK p, const Stages sts, const float* __restrict__ gout,
                                                         const int32_t* __restrict__ count, const float* __restrict__ tbox,
                                                         const int32_t* __restrict__ tidx, const int32_t* __restrict__ next,
                                                         const int32_t* __restrict__ head)
{
    const Stage st = sts.s[blockIdx.y];
    const yh_v5loss_desc& d = p.d;
    const int s = st.s;
    const int N = imin(count[s], p.L.cap);
    const int E = 5 + d.num_class;
    const int cap = p.L.cap;
    const int t = threadIdx.x, sub = t & 15, grp = t >> 4;
    const T* pred = reinterpret_cast<const T*>(st.pred);
    T* gp = reinterpret_cast<T*>(st.gpred);
    const int32_t* nx = next + (size_t)s * cap;
    const double s3 = 3.0 / d.num_stage;
    const float go = *gout;
    const float kbox = (float)(-(double)go * d.B * d.iou_scale * s3 / (double)N);
    const float kcls = (float)((double)go * d.B * d.cls_scale * s3 / ((double)N * d.num_class));
    for (int n = blockIdx.x * 16 + grp; n < N; n += gridDim.x * 16) {
        const int32_t* ii = tidx + ((size_t)s * cap + n) * 6;
        const int img = ii[1], anc = ii[2], gy = ii[3], gx = ii[4];
        const int cell = ((img * d.num_anchor + anc) * st.H + gy) * st.W + gx;
        const int h = head[p.L.head_off[s] + cell];
        if (list_max(nx, h, cap) != n) continue;              // not this cell's writer
        const size_t roff = (((size_t)img * st.H + gy) * st.W + gx) * st.ld + anc * E;
        const T* row = pred + roff;
        float lg[4];
        {
            float mine = (sub < 4) ? ldf<T>(row + sub) : 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) lg[i] = __shfl(mine, i, 16);
        }
        // per-lane accumulators for channels e = sub, sub+16, ...
        float gacc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) gacc[i] = 0.f;
        // visit members in ascending row index: repeatedly pick the smallest index > last
        int last = -1;
        for (int guard = 0; guard < cap; ++guard) {
            int m = 0x7fffffff;
            int q = h;
            for (int it = 0; q >= 0 && q < cap && it < cap; ++it) { if (q > last && q < m) m = q; q = nx[q]; }
            if (m == 0x7fffffff) break;
            last = m;
            const int32_t* mi = tidx + ((size_t)s * cap + m) * 6;
            const float* tb = tbox + ((size_t)s * cap + m) * 4;
            const int cls = mi[0];
            float dl4[4];
            pos_box(d, s, anc, lg, tb, dl4);
            int slot = 0;
            for (int e = sub; e < E; e += 16, ++slot) {
                float gv = 0.f;
                if (e < 4) gv = kbox * dl4[e];
                else if (e >= 5) {
                    const float x = ldf<T>(row + e);
                    const float tt = (e - 5 == cls) ? CLS_POS : CLS_NEG;
                    float dl, df = 0.f, f = 1.f;
                    const float l = bce_logits(x, tt, d.cls_pos_weight, &dl, nullptr);
                    if (d.use_focal) f = focal_factor(x, tt, d.focal_gamma, d.focal_alpha, &df, nullptr);
                    gv = kcls * (dl * f + l * df);
                }
                if (slot < 8) gacc[slot] += gv;
            }
        }
        int slot = 0;
        for (int e = sub; e < E; e += 16, ++slot)
            if (e != 4 && slot < 8) stf<T>(gp + roff + e, gacc[slot]);
    }
}

// ---------------------------------------------------------------- debug reader
__global__ __launch_bounds__(256) void v7_matches_kernel(const LossK p, const int32_t* __restrict__ count, const int32_t* __restrict__ tidx,
                                                         int32_t* __restrict__ count_out, int32_t* __restrict__ rows)
{
    const int s = blockIdx.y;
    const int N = imin(count[s], p.L.cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) count_out[s] = N;
    if (blockIdx.x == 0 && threadIdx.x < MAXS && s == 0 && (int)threadIdx.x >= p.d.num_stage) count_out[threadIdx.x] = 0;
    for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < p.L.cap; n += gridDim.x * blockDim.x) {
        const int32_t* ii = tidx + ((size_t)s * p.L.cap + n) * 6;
        int32_t* oo = rows + ((size_t)s * p.L.cap + n) * 5;
#pragma unroll
        for (int k = 0; k < 5; ++k) oo[k] = n < N ? ii[1 + k] : -1;
    }
}

int check_desc(const yh_v7loss_desc* v, const char* who) {
    YH_CHECK_ARG(v != nullptr, "%s: null desc", who);
    const yh_v5loss_desc* d = &v->v5;
    YH_CHECK_ARG(d->B > 0 && d->maxbox > 0 && d->num_class >= 1 && d->num_anchor >= 1 && d->num_anchor <= 3, "%s: bad B/maxbox/classes/anchors", who);
    YH_CHECK_ARG(d->num_stage == 3 || d->num_stage == 4, "%s: num_stage must be 3 or 4", who);
    YH_CHECK_ARG(5 + d->num_class <= 128, "%s: at most 123 classes supported", who);
    YH_CHECK_ARG(v->topk >= 1 && v->topk <= 24, "%s: topk=%d must be 1..24", who, v->topk);
    YH_CHECK_ARG(d->targets_xywhn == 0, "%s: targets are xyxy pixels (targets_xywhn must be 0)", who);
    for (int s = 0; s < d->num_stage; ++s) {
        YH_CHECK_ARG(d->H[s] > 0 && d->W[s] > 0, "%s: bad stage dims", who);
        YH_CHECK_ARG(d->ldp[s] % 8 == 0 && d->ldp[s] >= d->num_anchor * (5 + d->num_class), "%s: ldp[%d]=%d must be a multiple of 8 and >= A*(5+nc)", who, s, d->ldp[s]);
        YH_CHECK_ARG((long)d->B * d->num_anchor * d->H[s] * d->W[s] < (1L << 31), "%s: too many cells", who);
    }
    YH_CHECK_ARG((long)5 * d->num_anchor * d->B * d->maxbox < (1L << 26), "%s: too many targets", who);
    return YH_OK;
}

// the four stage slots of a launch; slots past num_stage repeat stage 0 and are never indexed (gridDim.y = num_stage)
void fill_stages(const yh_v5loss_desc* d, const void* const* preds, void* const* gpreds, Stages& all) {
    for (int s = 0; s < 4; ++s) {
        const int q = s < d->num_stage ? s : 0;
        Stage& sg = all.s[s];
        sg.pred = preds[q]; sg.gpred = gpreds ? gpreds[q] : nullptr; sg.s = q; sg.H = d->H[q]; sg.W = d->W[q]; sg.ld = d->ldp[q];
    }
}

LossK make_k(const yh_v7loss_desc* v) {
    LossK k;
    k.d = v->v5; k.L = make_layout(v->v5); k.topk = v->topk; k.iou_cof = v->use_iou_as_tar_cof != 0;
    return k;
}
int pos_blocks(const Layout& L) {
    const int nb = (L.cap + 15) / 16;
    return nb > PART_BLOCKS ? PART_BLOCKS : nb;
}

}  // namespace

extern "C" size_t yh_v7loss_ws_bytes(const yh_v7loss_desc* d) { return d ? make_layout(d->v5).w_total : 0; }
extern "C" size_t yh_v7loss_saved_bytes(const yh_v7loss_desc* d) { return d ? make_layout(d->v5).s_total : 0; }

extern "C" int yh_v7_loss_fwd(const yh_v7loss_desc* v, const void* const* preds, const float* targets,
                              double* balances, float* result, void* saved, void* ws, yh_stream stream)
{
    int rc = check_desc(v, "yh_v7_loss_fwd");
    if (rc) return rc;
    const yh_v5loss_desc* d = &v->v5;
    YH_CHECK_ARG(preds && targets && balances && result && saved && ws, "yh_v7_loss_fwd: null pointer");
    YH_CHECK_ARG(yh_aligned16(saved) && yh_aligned16(ws), "yh_v7_loss_fwd: saved / ws unaligned");
    for (int s = 0; s < d->num_stage; ++s) YH_CHECK_ARG(preds[s] && yh_aligned16(preds[s]), "yh_v7_loss_fwd: preds[%d] null/unaligned", s);
    hipStream_t st = (hipStream_t)stream;
    const LossK k = make_k(v);
    const Layout& L = k.L;
    char* sv = (char*)saved;
    char* w = (char*)ws;
    int32_t* count = (int32_t*)(sv + L.s_count);
    double* bal_used = (double*)(sv + L.s_bal_used);
    float* tbox = (float*)(sv + L.s_tbox);
    int32_t* tidx = (int32_t*)(sv + L.s_tidx);
    float* ciou = (float*)(sv + L.s_ciou);
    int32_t* next = (int32_t*)(sv + L.s_next);
    int32_t* head = (int32_t*)(sv + L.s_head);
    double* part = (double*)(w + L.w_part);
    int32_t* ccount = (int32_t*)(w + L.w_ccount);
    float* ctbox = (float*)(w + L.w_ctbox);
    int32_t* ctidx = (int32_t*)(w + L.w_ctidx);
    Cand* cand = (Cand*)(w + L.w_cand);
    int32_t* mt = (int32_t*)(w + L.w_mt);
    int32_t* runs = (int32_t*)(w + L.w_runs);
    // cell lists empty, no candidate matched
    rc = yh_fill_u32(head, 0xffffffffu, (int64_t)((L.s_total - L.s_head) / 4), stream);
    if (rc) return rc;
    rc = yh_fill_u32(mt, 0xffffffffu, (int64_t)d->num_stage * L.cap, stream);
    if (rc) return rc;
    // 1. candidates: the YOLOv5 match, into this call's own buffers
    rc = yh_v5_assign(d, targets, ccount, ctbox, ctidx, nullptr, stream);
    if (rc) return rc;
    const int nb_pos = pos_blocks(L);
    const int nb_obj = PART_BLOCKS;
    int nb_cand = (L.cap + 255) / 256;
    if (nb_cand > 1024) nb_cand = 1024;
    Stages all;
    fill_stages(d, preds, nullptr, all);
    hipLaunchKernelGGL(v7_runs_kernel, dim3(d->num_stage), dim3(1024), 0, st, k, ctidx, ccount, runs);
    yh_pred_type(d->pred_is_f32, [&](auto e) {
        using T = decltype(e);
        // 2. SimOTA over the candidates of every (image, stage), then the matched list in candidate order
        hipLaunchKernelGGL((v7_cand_kernel<T>), dim3(nb_cand, d->num_stage), dim3(256), 0, st, k, all, ccount, ctidx, cand);
        hipLaunchKernelGGL((v7_simota_kernel<T>), dim3(d->B, d->num_stage), dim3(256), 0, st, k, all, targets, ccount, ctidx, cand, runs, mt);
        hipLaunchKernelGGL(v7_compact_kernel, dim3(d->num_stage), dim3(1024), 0, st, k, targets, ccount, ctidx, mt, count, tbox, tidx);
        // 3. / 4. matched rows of every stage, then the objectness pass of every stage (it reads the stage's CIoU values)
        hipLaunchKernelGGL((v7_pos_fwd_kernel<T>), dim3(nb_pos, d->num_stage), dim3(256), 0, st, k, all, count, tbox, tidx, ciou, next, head, part);
        hipLaunchKernelGGL((v7_obj_fwd_kernel<T>), dim3(nb_obj, d->num_stage), dim3(256), 0, st, k, all, ciou, next, head, part);
    });
    hipLaunchKernelGGL(v7_finalize_kernel, dim3(1), dim3(1024), 0, st, k, count, part, nb_pos, nb_obj, balances, bal_used, result);
    YH_CHECK_LAUNCH("yh_v7_loss_fwd");
    return YH_OK;
}

extern "C" int yh_v7_loss_bwd(const yh_v7loss_desc* v, const void* const* preds, const float* gout,
                              const void* saved, void* const* gpreds, void* ws, yh_stream stream)
{
    (void)ws;
    int rc = check_desc(v, "yh_v7_loss_bwd");
    if (rc) return rc;
    const yh_v5loss_desc* d = &v->v5;
    YH_CHECK_ARG(preds && gout && saved && gpreds, "yh_v7_loss_bwd: null pointer");
    for (int s = 0; s < d->num_stage; ++s) YH_CHECK_ARG(preds[s] && gpreds[s] && yh_aligned16(gpreds[s]), "yh_v7_loss_bwd: stage %d pointers null/unaligned", s);
    hipStream_t st = (hipStream_t)stream;
    const LossK k = make_k(v);
    const Layout& L = k.L;
    const char* sv = (const char*)saved;
    const int32_t* count = (const int32_t*)(sv + L.s_count);
    const double* bal_used = (const double*)(sv + L.s_bal_used);
    const float* tbox = (const float*)(sv + L.s_tbox);
    const int32_t* tidx = (const int32_t*)(sv + L.s_tidx);
    const float* ciou = (const float*)(sv + L.s_ciou);
    const int32_t* next = (const int32_t*)(sv + L.s_next);
    const int32_t* head = (const int32_t*)(sv + L.s_head);
    const int nb_pos = pos_blocks(L);
    Stages all;
    fill_stages(d, preds, gpreds, all);
    long ntile_max = 1;
    for (int s = 0; s < d->num_stage; ++s) {
        const long ntile = ((long)d->B * d->H[s] * d->W[s] + 63) / 64;
        if (ntile > ntile_max) ntile_max = ntile;
    }
    const int gb = (int)(ntile_max > 4096 ? 4096 : ntile_max);
    // the objectness pass writes every stage's whole gradient tensor, then the matched rows fill their channels: two launches
    yh_pred_type(d->pred_is_f32, [&](auto e) {
        using T = decltype(e);
        hipLaunchKernelGGL((v7_obj_bwd_kernel<T>), dim3(gb, d->num_stage), dim3(256), 0, st, k, all, gout, count, bal_used, ciou, next, head);
        hipLaunchKernelGGL((v7_pos_bwd_kernel<T>), dim3(nb_pos, d->num_stage), dim3(256), 0, st, k, all, gout, count, tbox, tidx, next, head);
    });
    YH_CHECK_LAUNCH("yh_v7_loss_bwd");
    return YH_OK;
}

extern "C" int yh_v7_matches(const yh_v7loss_desc* v, const void* saved, int32_t* count, int32_t* rows, yh_stream stream)
{
    int rc = check_desc(v, "yh_v7_matches");
    if (rc) return rc;
    YH_CHECK_ARG(saved && count && rows, "yh_v7_matches: null pointer");
    const LossK k = make_k(v);
    const char* sv = (const char*)saved;
    int nb = (k.L.cap + 255) / 256;
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(v7_matches_kernel, dim3(nb, v->v5.num_stage), dim3(256), 0, (hipStream_t)stream, k,
                       (const int32_t*)(sv + k.L.s_count), (const int32_t*)(sv + k.L.s_tidx), count, rows);
    YH_CHECK_LAUNCH("yh_v7_matches");
    return YH_OK;
}
