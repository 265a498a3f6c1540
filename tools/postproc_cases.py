"""Inputs for the post-processing parity tests (tests/test_postproc_cases_host.py, tests/test_gpu_postproc_edges.py).

Plain NumPy, no GPU, no torch.  Every generator is deterministic in its arguments; the host test proves from the oracle alone that the
inputs reach what they claim (chunks the NMS kernel has to skip, max_keep reached inside a 64-chunk, ties across a chunk edge, rows
exactly on a threshold, ...), so a generator that drifts fails there and not silently on the GPU.

  nms_table / DESIGNED      candidate tables (n, 6) [x0, y0, x1, y1, score, cls] for yh_nms_batched
  decoded_rows              decoded tensors (B, N, 5+nc) for yh_filter_decoded, values on a 1/16 grid so products hit thresholds exactly
  HEAD_CASES                head tensors for yh_decode_full / yh_decode_filter(_view): the array the oracle reads and the buffer the
                            kernel reads, with NaN in every element the kernel has no business reading"""
import numpy as np

F32 = np.float32

# ---------------------------------------------------------------------------------------------------------------- NMS
IOU_THR = 0.45
NMS_SIZES = (0, 1, 2, 63, 64, 65, 128, 129, 1023, 1024, 1025, 2048, 2049, 2999, 3000, 4096, 4097, 8191, 8192, 8193)
# (class_aware, inclusive, max_keep, merge_filter)
NMS_CONFIGS = ((1, 1, 300, 1), (0, 0, 300, 0), (1, 1, 7, 1), (1, 1, 1000, 0))
ZERO_AREA = (100.0, 100.0, 100.0, 140.0)
NUM_ZERO_AREA = 8
_NMS_SEED = {2999: 29992}       # n -> seed where the default (n itself) misses a property the host test asks for


def _quarter(x):
    return (np.round(np.asarray(x, dtype=np.float64) * 4) / 4).astype(F32)


def _cluster_boxes(r, n, nclust):
    """n boxes around nclust centres on a 640 canvas: centres jittered +-6 px, sizes x [0.75, 1.3], quarter-pixel corners"""
    ctr = r.uniform(40, 600, (nclust, 2))
    wh = r.uniform(10, 100, (nclust, 2))             # small enough that the jitter splits a cluster into several picks
    k = r.randint(0, nclust, n)
    c = ctr[k] + r.uniform(-6, 6, (n, 2))
    s = wh[k] * r.uniform(0.75, 1.3, (n, 2))
    return _quarter(np.concatenate((c - s / 2, c + s / 2), axis=1)), k


def nms_table(n, seed=None):
    """(n, 6) float32.  About n/12 clusters, 4 classes, scores k/64 (many exact ties), 10 % of the scores exactly 0, 90 % of the
    rows in their cluster's class; for n >= 32 eight rows with a positive score become the zero-area box ZERO_AREA of class 1"""
    seed = _NMS_SEED.get(n, n) if seed is None else seed
    r = np.random.RandomState(seed)
    t = np.zeros((n, 6), F32)
    if n == 0:
        return t
    nclust = max(1, n // 12)
    ccls = r.randint(0, 4, nclust)
    t[:, :4], k = _cluster_boxes(r, n, nclust)
    t[:, 4] = r.randint(1, 64, n).astype(F32) / F32(64)
    t[r.uniform(size=n) < 0.1, 4] = 0
    own = r.uniform(size=n) < 0.9
    t[:, 5] = np.where(own, ccls[k], r.randint(0, 4, n))
    if n >= 32:
        rows = r.choice(np.flatnonzero(t[:, 4] > 0), NUM_ZERO_AREA, replace=False)
        t[rows, :4] = ZERO_AREA
        t[rows, 5] = 1
    return t


def stack_table(n=1500):
    """1200 rows are +-2 px copies of three boxes of one class with scores in [32/64, 63/64]: after the first chunk of the sorted list
    every chunk of copies is struck out as a whole.  The other 300 rows are spread, with scores below 32/64.  Rows permuted."""
    r = np.random.RandomState(1500)
    ncopy = n - 300
    base = np.array([[60, 60, 260, 260], [330, 80, 560, 300], [120, 350, 420, 600]], np.float64)
    t = np.zeros((n, 6), F32)
    t[:ncopy, :4] = _quarter(base[r.randint(0, 3, ncopy)] + r.uniform(-2, 2, (ncopy, 4)))
    t[:ncopy, 4] = r.randint(32, 64, ncopy).astype(F32) / F32(64)
    t[:ncopy, 5] = 0
    c = r.uniform(20, 620, (300, 2))
    s = r.uniform(8, 40, (300, 2))
    t[ncopy:, :4] = _quarter(np.concatenate((c - s / 2, c + s / 2), axis=1))
    t[ncopy:, 4] = r.randint(1, 32, 300).astype(F32) / F32(64)
    t[ncopy:, 5] = r.randint(0, 4, 300)
    return t[r.permutation(n)]


def alltie_table(n=200):
    t = nms_table(n, seed=7200)
    t[:, 4] = 0.5
    return t


def allzero_table(n=130):
    t = nms_table(n, seed=7130)
    t[:, 4] = 0
    return t


def one_positive_table():
    return np.array([[10.25, 20.5, 110.75, 90.0, 0.5, 2.0]], F32)


NUM_TRIPLES = 64


def on_threshold_table():
    """64 triples A, B, C of one class on an 8 x 8 grid of cells that do not touch.  A and B are 29 wide and overlap by 18:
    IoU = 18h / 40h, which fp32 rounds to exactly float32(0.45) — the inclusive rule suppresses B, the exclusive rule keeps it.
    C is A moved one pixel towards B with the lowest score: A suppresses it under both rules, and it gives A (and a B that wrongly
    survived) a second overlapping candidate for the merge filter.  Rows 3i, 3i+1, 3i+2 are A, B, C of triple i.  The first 32
    triples have adjacent scores (B is met in A's 64-chunk), the others have B 24/64 below A (B is struck out from a later chunk)."""
    t = np.zeros((3 * NUM_TRIPLES, 6), F32)
    for i in range(NUM_TRIPLES):
        x, y, h = 5.0 + 80 * (i % 8), 5.25 + 80 * (i // 8), 20.0 + 4 * (i % 7)
        for j, dx in enumerate((0.0, 11.0, 1.0)):
            t[3 * i + j, :4] = (x + dx, y, x + dx + 29, y + h)
        sa = 60 - (i % 16) * 3 if i < 32 else 63 - i % 16
        sb = sa - 1 if i < 32 else sa - 24
        sc = sb - 1 if i < 32 else sb - 8
        t[3 * i:3 * i + 3, 4] = np.array((sa, sb, sc), F32) / F32(64)
        t[3 * i:3 * i + 3, 5] = i % 4
    return t


DESIGNED = {"stack": stack_table, "alltie": alltie_table, "allzero": allzero_table, "one_positive": one_positive_table,
            "on_threshold": on_threshold_table}
DESIGNED_CONFIGS = NMS_CONFIGS[:2]


def sorted_positions(table):
    """candidate indices with a positive score in the kernel's order: score descending, index ascending"""
    idx = np.flatnonzero(table[:, 4] > 0)
    return idx[np.lexsort((idx, -table[idx, 4].astype(np.float64)))]


# ---------------------------------------------------------------------------------------------------------------- filter
FILTER_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
FILTER_NC = (1, 3, 80)
FILTER_B = 3
FILTER_THR = (0.25, 0.25)        # conf, cls
# with equal thresholds a single-label YOLOv5 row with obj == conf_thr can never pass (obj * cls <= obj): the second pair makes the
# `obj >= conf_thr` rule of that mode decide rows
FILTER_THRS = (FILTER_THR, (0.25, 0.125))


def decoded_rows(B, N, nc, seed):
    """(B, N, 5+nc) float32.  obj and class values are multiples of 1/16, so obj == 0.25 and obj * cls == 0.25 occur and are exact.
    One class per row is 'hot' (any multiple of 1/16), the others stay at or below 3/16 (never a candidate of their own); about 8 % of
    the rows (nc > 1) carry their largest value twice — the first must win.  The last image has obj = 0 everywhere."""
    r = np.random.RandomState(seed)
    E = 5 + nc
    d = np.zeros((B, N, E), F32)
    d[..., 0:2] = _quarter(r.uniform(20, 620, (B, N, 2)))
    d[..., 2:4] = _quarter(r.uniform(4, 200, (B, N, 2)))
    d[..., 4] = r.randint(0, 17, (B, N)).astype(F32) / F32(16)
    d[..., 5:] = r.randint(0, 4, (B, N, nc)).astype(F32) / F32(16)
    hot = r.randint(0, nc, (B, N))
    bi, ni = np.meshgrid(np.arange(B), np.arange(N), indexing="ij")
    d[bi, ni, 5 + hot] = r.randint(0, 17, (B, N)).astype(F32) / F32(16)
    if nc > 1:
        tie = r.uniform(size=(B, N)) < 0.08
        tie[:, :4] = False
        second = (hot + 1 + r.randint(0, nc - 1, (B, N))) % nc
        v = r.randint(4, 17, (B, N)).astype(F32) / F32(16)
        for b, i in zip(*np.nonzero(tie)):
            d[b, i, 5 + hot[b, i]] = d[b, i, 5 + second[b, i]] = v[b, i]
    for b in range(B):                      # rows exactly on the thresholds, and one tie between two classes that decides cls
        d[b, 0, 4], d[b, 0, 5:] = 0.25, 0
        d[b, 0, 5 + hot[b, 0]] = 1.0
        if N >= 2:
            d[b, 1, 4], d[b, 1, 5:] = 0.5, 0
            d[b, 1, 5 + hot[b, 1]] = 0.5
        if N >= 3 and nc > 1:
            d[b, 2, 4], d[b, 2, 5:] = 1.0, 0
            d[b, 2, 5 + nc - 1] = d[b, 2, 5 + nc // 2 - 1] = 0.5
        if N >= 4:                          # obj * cls == 0.125: on the class threshold of FILTER_THRS[1]
            d[b, 3, 4], d[b, 3, 5:] = 0.5, 0
            d[b, 3, 5 + hot[b, 3]] = 0.25
    d[B - 1, :, 4] = 0
    return d


# ---------------------------------------------------------------------------------------------------------------- heads
ANCHORS = np.array([[[10, 13], [16, 30], [33, 23]], [[30, 61], [62, 45], [59, 119]], [[116, 90], [156, 198], [373, 326]],
                    [[436, 615], [739, 380], [925, 792]]], F32)
STRIDES = (8.0, 16.0, 32.0, 64.0)
HEAD_THR = (0.3, 0.3)


def bf16_round(x):
    """float32 -> nearest-even bfloat16, returned as float32"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    u = (u + (((u >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return u.view(F32)


def bf16_bits(x):
    """bf16-representable float32 -> its 16 bits (what the kernel's buffer holds)"""
    return (np.ascontiguousarray(x, dtype=F32).view(np.uint32) >> 16).astype(np.uint16)


BF16_NAN = np.uint16(0x7FC0)


class HeadCase:
    """One head descriptor.  stages: ((H, W), ...); ldp: row length of the kernel buffer in elements; shift: elements between a
    16-byte boundary and the first element of every stage buffer."""

    def __init__(self, id, yolox, A, nc, stages, B, ldp=None, shift=0, seed=0, img_h=None):
        self.id, self.yolox, self.A, self.nc, self.stages, self.B = id, int(yolox), A, nc, tuple(stages), B
        self.E = 5 + nc
        self.ldp = ldp if ldp is not None else ((A * self.E + 7) // 8) * 8
        self.shift, self.seed, self.img_h = shift, seed, img_h
        self.npred = sum(A * h * w for h, w in self.stages)

    def strides(self):
        if self.yolox:
            return tuple(float(self.img_h) / h for h, _ in self.stages)
        return STRIDES[:len(self.stages)]

    def anchors(self):
        return ANCHORS[:len(self.stages), :self.A]

    def raw(self, bf16):
        """per stage (B, A, 5+nc, h, w) float32: N(0, 1), objectness N(0, 1.5); rounded to bf16 values when bf16"""
        r = np.random.RandomState(self.seed)
        out = []
        for h, w in self.stages:
            x = r.standard_normal((self.B, self.A, self.E, h, w)).astype(F32)
            x[:, :, 4] *= F32(1.5)
            out.append(bf16_round(x) if bf16 else x)
        return out

    def build(self, bf16):
        """-> (oracle inputs, kernel buffers).  Oracle inputs: per stage (B, A*(5+nc), h, w) for the v5 decode, (B, A, 5+nc, h, w)
        for YOLOX.  Kernel buffers: per stage (flat, offset): flat is a 1-D float32 (or uint16 holding bf16 bits) array, the
        [B][h][w][ldp] tensor starts `offset` elements in; everything outside the A*(5+nc) leading columns of a row is NaN."""
        raws = self.raw(bf16)
        oracle = [x if self.yolox else x.reshape(self.B, self.A * self.E, *x.shape[3:]) for x in raws]
        bufs = []
        for x, (h, w) in zip(raws, self.stages):
            cells = x.transpose(0, 3, 4, 1, 2).reshape(self.B, h, w, self.A * self.E)
            body = np.full((self.B, h, w, self.ldp), np.nan, F32)
            body[..., :self.A * self.E] = cells
            flat = np.full(self.shift + body.size + 64, np.nan, F32)
            flat[self.shift:self.shift + body.size] = body.ravel()
            if bf16:
                bits = np.full(flat.shape, BF16_NAN, np.uint16)
                bits[self.shift:self.shift + body.size] = np.where(np.isnan(body.ravel()), BF16_NAN, bf16_bits(np.nan_to_num(body.ravel())))
                flat = bits
            bufs.append((flat, self.shift))
        return oracle, bufs


HEAD_CASES = (
    HeadCase("unpadded_nc1", 0, 3, 1, ((5, 7), (3, 4), (1, 2)), B=2, ldp=18, seed=11),           # rows of 72 / 36 bytes
    HeadCase("shifted_base", 0, 3, 1, ((5, 7), (3, 4), (1, 2)), B=2, ldp=24, shift=1, seed=12),    # aligned rows, unaligned tile
    HeadCase("four_stages", 0, 2, 3, ((8, 8), (5, 13), (7, 9), (1, 1)), B=2, seed=13),             # 64, 65, 63, 1 cells
    HeadCase("long_row", 0, 3, 1, ((3, 7301),), B=1, seed=14),                                     # 1029 chunk keys, 65 709 predictions
    HeadCase("yolox_rect", 1, 1, 3, ((12, 20), (6, 10), (3, 5)), B=2, seed=15, img_h=96),
    HeadCase("wide_row_tiny_map", 0, 3, 80, ((2, 2), (1, 1)), B=3, ldp=256, seed=16),              # 66 KB fp32 tile, 4 of 64 lanes live
)
