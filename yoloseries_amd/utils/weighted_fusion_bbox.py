"""Weighted box fusion on the host, in NumPy fp64: the mirror of csrc/wbf.hip and the reference's public function.

Per class ascending, rows by score descending (a STABLE sort: equal scores in table order), starting from no cluster: a row joins
every cluster whose fused box has IoU >= iou_thr with it (intersection sides clamped at 0, union clipped below at 1e-6), or founds a
new cluster when it joins none; the fused boxes are refreshed before the next row.  Fused score = sum(s w) / sum(w); fused box =
sum(s b) / sum(s) / N ('reference': the reference's np.mean divides by the member count once more) or sum(s b) / sum(s)
('weighted').  DESIGN.md section 4 lists where this differs from the reference's text (seeding, ties, the return type).
"""
import numpy as np

__all__ = ['weighted_fusion_bbox', 'fuse_table', 'BOX_MEANS']

BOX_MEANS = ('reference', 'weighted')


def _iou_one_to_many(box, boxes):
    """fp64 IoU of one xyxy box with (M, 4) boxes, in the kernel's operation order"""
    a_row = (box[2] - box[0]) * (box[3] - box[1])
    a_clu = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    w = np.maximum(0.0, np.minimum(box[2], boxes[:, 2]) - np.maximum(box[0], boxes[:, 0]))
    h = np.maximum(0.0, np.minimum(box[3], boxes[:, 3]) - np.maximum(box[1], boxes[:, 1]))
    inter = w * h
    return inter / np.maximum((a_row + a_clu) - inter, 1e-6)


def fuse_table(rows7, iou_thr, box_mean='reference'):
    """One image's rows (n, 7) [xmin, ymin, xmax, ymax, score, class, weight] -> (out (m, 6) float64 [box, score, class], members
    (m,) int64): class ascending, then the order the clusters were founded.  Rows with weight <= 0 or score <= 0 are not
    candidates.  Running sums in arrival order, vectorised over the clusters of a class: the arithmetic of csrc/wbf.hip."""
    if box_mean not in BOX_MEANS:
        raise ValueError(f"fuse_table: box_mean {box_mean!r} is not one of {BOX_MEANS}")
    rows = np.asarray(rows7, dtype=np.float64).reshape(-1, 7)
    rows = rows[(rows[:, 6] > 0) & (rows[:, 4] > 0)]
    outs, mems = [], []
    for lab in np.unique(rows[:, 5]):
        seg = rows[rows[:, 5] == lab]
        seg = seg[np.argsort(-seg[:, 4], kind='stable')]
        n = len(seg)
        A, S, SW, W = np.zeros((n, 4)), np.zeros(n), np.zeros(n), np.zeros(n)
        N = np.zeros(n, dtype=np.int64)
        box = np.zeros((n, 4))
        m = 0
        for r in seg:
            b, s, w = r[:4], r[4], r[6]
            hit = np.nonzero(_iou_one_to_many(b, box[:m]) >= iou_thr)[0] if m else np.zeros(0, dtype=np.int64)
            if hit.size == 0:
                hit = np.array([m])
                m += 1
            A[hit] += b * s
            S[hit] += s
            SW[hit] += s * w
            W[hit] += w
            N[hit] += 1
            fused = A[hit] / S[hit, None]
            box[hit] = fused / N[hit, None] if box_mean == 'reference' else fused
        outs.append(np.concatenate((box[:m], (SW[:m] / W[:m])[:, None], np.full((m, 1), lab)), axis=1))
        mems.append(N[:m])
    if not outs:
        return np.zeros((0, 6)), np.zeros(0, dtype=np.int64)
    return np.concatenate(outs, axis=0), np.concatenate(mems)


def weighted_fusion_bbox(bbox_list, iou_thr=0.5):
    """:param bbox_list: (N, 7) [xmin, ymin, xmax, ymax, score, class, weight]
    :return: (Cluster, Fusion), one entry per class ascending: Cluster[c] is the list of clusters, each the list of its member rows
             (7 floats) in arrival order; Fusion[c] the list of their fused rows, arrays [xmin, ymin, xmax, ymax, score, class].
    The box is spelled as the reference spells it, the mean over the members of b * s / sum(s)."""
    rows = np.asarray(bbox_list, dtype=np.float64).reshape(-1, 7)
    Cluster, Fusion = [], []
    for lab in np.unique(rows[:, 5]):
        seg = rows[rows[:, 5] == lab]
        seg = seg[np.argsort(-seg[:, 4], kind='stable')]
        clusters, fusion = [], []
        for r in seg:
            hit = []
            if fusion:
                hit = np.nonzero(_iou_one_to_many(r[:4], np.asarray(fusion)[:, :4]) >= iou_thr)[0].tolist()
            if not hit:
                clusters.append([])
                fusion.append(None)
                hit = [len(clusters) - 1]
            for j in hit:
                clusters[j].append(r.tolist())
                mem = np.asarray(clusters[j])
                box = np.mean(mem[:, :4] * mem[:, 4:5] / np.sum(mem[:, 4]), axis=0)
                score = np.sum(mem[:, 4] * mem[:, 6]) / np.sum(mem[:, 6])
                fusion[j] = np.append(box, [score, lab])
        Cluster.append(clusters)
        Fusion.append(fusion)
    return Cluster, Fusion
