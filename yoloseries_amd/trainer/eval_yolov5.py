"""YOLOV5Evaluator — host-side mirror of trainer/eval_yolov5.py:10-317 over csrc/postproc.hip.

forward -> decode -> candidate filter -> class-aware greedy NMS -> merge filter all run on
the GPU; only the final (n,6) rows per image cross PCIe (the reference copies the whole
decoded (B, 25200, 85) tensor to the host, :265).  With use_tta each of the three passes is
decoded and filtered straight from its head tensors into one candidate table
(_tta_from_heads): no decoded tensor, no concatenation.  With use_tta and hyp['wfb'] the table is merged by weighted box fusion
(csrc/wbf.hip) instead of NMS, where it lies.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib
from .._lib import DecodeDesc, ViewXform, check, lib
from ..layout import to_cell_major

__all__ = ['YOLOV5Evaluator', 'MatchAccumulator', 'info_tensor']



def _decode_ws(owner, d, dev):
    """workspace of the two-pass decode + filter (yh_decode_filter_ws_bytes), kept on the evaluator between calls"""
    need = int(lib().yh_decode_filter_ws_bytes(C.byref(d)))
    ws = getattr(owner, "_decode_ws_buf", None)
    if ws is None or ws.numel() < need or ws.device != torch.device(dev):
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        owner._decode_ws_buf = ws
    return ws.data_ptr()

IOU_THRESHOLDS = tuple(np.linspace(0.5, 0.95, 10).tolist())        # mAP_v2.iou_thr
AP_GRID, PR_GRID = 101, 1000                                        # compute_ap's recall grid, compute_ap_per_class's confidence grid


def info_tensor(info):
    """the batch's resize_info dicts (dataset/data_collater.py) -> (B, 5) float32 [scale, pad_top, pad_left, org_h, org_w], built
    once per batch on the host; a tensor passes through"""
    if torch.is_tensor(info):
        return info.to(torch.float32).contiguous()
    rows = [[r['scale'], r['pad_top'], r['pad_left'], r['org_shape'][0], r['org_shape'][1]] for r in info]
    return torch.from_numpy(np.asarray(rows, dtype=np.float32).reshape(len(rows), 5))


class MatchAccumulator:
    """The match tables of a validation pass, kept on the device: append(evaluate_matches(...)) per batch, finish() or finish_ap() once.  Owns the
    gt_hist buffer that yh_val_match accumulates into (pass acc.gt_hist to evaluate_matches)."""

    def __init__(self, num_class, device):
        self.num_class = int(num_class)
        self.gt_hist = torch.zeros(self.num_class, dtype=torch.int32, device=device)
        self._parts = []
        self.images = 0

    def append(self, m):
        if m['gt_hist'] is not self.gt_hist:
            raise ValueError("MatchAccumulator.append: evaluate_matches was not given this accumulator's gt_hist")
        self._parts.append((m['conf'], m['cls'], m['tp'], m['nrow']))
        self.images += m['nrow'].numel()

    def _compact(self):
        """-> (conf, cls int32, tp int16) of the rows that count, on the device; None without a batch"""
        if not self._parts:
            return None
        keep = torch.cat([(torch.arange(c.shape[1], device=c.device)[None, :] < n[:, None]).reshape(-1) for c, _, _, n in self._parts])
        conf = torch.cat([c.reshape(-1) for c, _, _, _ in self._parts])[keep]
        cls = torch.cat([c.reshape(-1) for _, c, _, _ in self._parts])[keep]
        tp = torch.cat([t.reshape(-1) for _, _, t, _ in self._parts])[keep]
        return conf, cls, tp

    def finish(self):
        """-> (conf (N,) float32, cls (N,) int32, tp (N, 10) bool, gt_hist (num_class,) int64) as NumPy, the padded rows compacted
        away on the device and everything brought over in ONE device-to-host copy (the only point the host waits)"""
        rows = self._compact()
        if rows is not None:
            conf, cls, tp = rows
            flat = torch.cat([conf.view(torch.int32), cls, tp.to(torch.int32) & 0xffff, self.gt_hist])
        else:
            flat = self.gt_hist
        h = flat.cpu().numpy()
        n = (h.size - self.num_class) // 3
        conf, cls, bits, hist = h[:n].view(np.float32), h[n:2 * n], h[2 * n:3 * n], h[3 * n:]
        tp = ((bits[:, None] >> np.arange(len(IOU_THRESHOLDS))[None, :]) & 1).astype(bool)
        return conf.copy(), cls.copy(), tp, hist.astype(np.int64)

    def finish_ap(self):
        """The AP and the precision / recall curves of the pass, computed on the device (yh_val_ap) -> (ap (num_class, 10),
        precision (num_class, 1000), recall (num_class, 1000), npred (num_class,) int64, gt_hist (num_class,) int64) as NumPy, for
        mAP_v2.from_curves: what compute_ap_per_class makes of finish()'s table, with a row per class id (zeros where the class has
        no ground truth or no detection).  The rows are compacted as in finish(), ordered by one stable sort of an int64 key (class
        in the high word, the complement of conf's bits in the low one: class ascending, conf descending, ties in table order) and
        ONE copy brings the five results over.  Without any detection nothing is launched: ap, precision and recall have no rows."""
        nc, nt = self.num_class, len(IOU_THRESHOLDS)
        rows = self._compact()
        if rows is None or rows[0].numel() == 0:
            return (np.zeros((0, nt)), np.zeros((0, PR_GRID)), np.zeros((0, PR_GRID)), np.zeros(nc, np.int64),
                    self.gt_hist.cpu().numpy().astype(np.int64))
        conf, cls, tp = (t.contiguous() for t in rows)
        n, dev = conf.numel(), conf.device
        key = (cls.to(torch.int64) << 32) | (0xFFFFFFFF - (conf.view(torch.int32).to(torch.int64) & 0xFFFFFFFF))
        order = torch.sort(key, stable=True)[1].to(torch.int32)
        xs = torch.from_numpy(np.concatenate((np.linspace(0, 1, AP_GRID), np.linspace(0, 1, PR_GRID)))).to(dev)
        nd = nc * (nt + 2 * PR_GRID)
        out = torch.empty(nd + nc, dtype=torch.float64, device=dev)           # the doubles, then npred and gt_hist as int32 pairs
        tail = out[nd:].view(torch.int32)
        ws = torch.empty(max(int(lib().yh_val_ap_ws_bytes(n, nt)), 16), dtype=torch.uint8, device=dev)
        o_ap, o_pre, o_rec = out[:nc * nt], out[nc * nt:nc * (nt + PR_GRID)], out[nc * (nt + PR_GRID):nd]
        check(lib().yh_val_ap(conf.data_ptr(), cls.data_ptr(), tp.data_ptr(), order.data_ptr(), n, self.gt_hist.data_ptr(), nc, nt,
                              xs.data_ptr(), AP_GRID, xs[AP_GRID:].data_ptr(), PR_GRID, o_ap.data_ptr(), o_pre.data_ptr(),
                              o_rec.data_ptr(), tail.data_ptr(), ws.data_ptr(), _lib.stream_ptr()), "yh_val_ap")
        tail[nc:] = self.gt_hist
        h = out.cpu().numpy()
        ints = h[nd:].view(np.int32).astype(np.int64)
        return (h[:nc * nt].reshape(nc, nt).copy(), h[nc * nt:nc * (nt + PR_GRID)].reshape(nc, PR_GRID).copy(),
                h[nc * (nt + PR_GRID):nd].reshape(nc, PR_GRID).copy(), ints[:nc], ints[nc:])


class YOLOV5Evaluator:

    def __init__(self, yolo, anchors, hyp, compute_metric=False):
        self.yolo = yolo
        self.hyp = hyp
        self.device = hyp['device']
        self.num_class = hyp['num_class']
        self.anchor_num = anchors.size(1)
        self.anchors = anchors
        self.num_stage = len(anchors)
        self.ds_scales = [8, 16, 32]
        self.inp_h, self.inp_w = hyp['input_img_size']
        self.use_tta = hyp['use_tta']
        self.iou_threshold = hyp['compute_metric_iou_threshold'] if compute_metric else hyp['iou_threshold']
        self.cls_threshold = hyp['compute_metric_cls_threshold'] if compute_metric else hyp['cls_threshold']
        self.conf_threshold = hyp['compute_metric_conf_threshold'] if compute_metric else hyp['conf_threshold']
        self._anchors_host = anchors.detach().cpu().tolist()
        self._init_wfb()

    def _init_wfb(self):
        """hyp['wfb'] (with use_tta only, as in the reference: without it the key is ignored) and its keys, checked once"""
        from ..hipk import WBF_BOX_MEANS
        hyp = self.hyp
        self.wfb = bool(self.use_tta and hyp.get('wfb', False))
        weights = hyp.get('wfb_weights', None)
        weights = [1., 1., 1.] if weights is None else list(weights)
        if len(weights) < len(self._TTA_PASSES):
            raise ValueError(f"wfb_weights {weights}: test-time augmentation has {len(self._TTA_PASSES)} passes, one weight each")
        if any(not float(w) > 0 for w in weights):
            raise ValueError(f"wfb_weights {weights}: every weight must be > 0 (a row with weight <= 0 is no candidate)")
        self.wfb_weights = [float(w) for w in weights[:len(self._TTA_PASSES)]]
        if self.wfb and not float(hyp['wfb_skip_box_threshold']) >= 0:          # a fused score divides by the sum of the scores
            raise ValueError(f"wfb_skip_box_threshold {hyp['wfb_skip_box_threshold']}: must be >= 0 (candidates need a score > 0)")
        self.wfb_box_mean = hyp.get('wfb_box_mean', 'reference')
        if self.wfb_box_mean not in WBF_BOX_MEANS:
            raise ValueError(f"wfb_box_mean {self.wfb_box_mean!r} is not one of {sorted(WBF_BOX_MEANS)}")

    # ------------------------------------------------------------------ reference API
    @torch.no_grad()
    def __call__(self, inputs):
        """:param inputs: (b, 3, h, w) -> list (len b) of FloatTensor (n, 6) [xmin, ymin, xmax, ymax, conf, cls] on CPU, or None"""
        if self.wfb:
            return self._fusion_rows(*self._wfb_candidates(inputs))
        outs = self._run_nms(*self._candidates(inputs))
        return [torch.from_numpy(x) if x is not None else None for x in outs]

    def _candidates(self, inputs):
        """forward + decode + filter of a batch by the configured path -> candidate table (cand, ncand, B, cap) on the device, for
        NMS; the table that weighted box fusion merges is _wfb_candidates'"""
        if self.use_tta and self.hyp.get('mutil_label', False):       # through the decoded tensor, like _cand_from_heads
            merge_preds_out, _ = self.test_time_augmentation(inputs)
            return self._filter_decoded(merge_preds_out)
        if self.use_tta:
            return self._tta_cand(inputs)
        return self._cand_from_heads(self.yolo(inputs))

    # ------------------------------------------------------------------ weighted box fusion (hyp['wfb'] with use_tta)
    def _wfb_thresholds(self, from_heads):
        """(conf, cls) thresholds that make the candidate kernels apply do_wfb's rule (eval_yolov5.py:57-74): obj > t, then
        cls * obj > t, both STRICT, t = wfb_skip_box_threshold as fp32.  The kernels compare in fp32, where v > t is
        v >= nextafter(t, +inf): the v5 rules test obj >= conf and, single label, best > cls (strict already) or, multi label,
        cls * obj >= cls."""
        t = np.float32(self.hyp['wfb_skip_box_threshold'])
        up = np.nextafter(t, np.float32(np.inf))
        return float(up), float(up if self.hyp.get('mutil_label', False) else t)

    _WFB_FILTER_MODES = (0, 2)    # do_wfb is the same text in both reference evaluators: the v5 rule of yh_filter_decoded

    def _wfb_decoded(self, preds_out):
        """per-pass decoded tensors -> (cand (B, cap, 6), weight (B, cap)): each pass filtered by do_wfb's rule (yh_filter_decoded),
        the tables side by side, weight 0 on the unused tail of each"""
        if len(preds_out) > len(self.wfb_weights):
            raise ValueError(f"do_wfb: {len(preds_out)} passes, {len(self.wfb_weights)} weights")
        mode = self._WFB_FILTER_MODES[1 if self.hyp.get('mutil_label', False) else 0]
        cands, weights = [], []
        for p, w in zip(preds_out, self.wfb_weights):
            cand, ncand, B, cap = self._filter_decoded(p, self._wfb_thresholds(False), mode)
            cands.append(cand)
            weights.append((torch.arange(cap, device=cand.device)[None, :] < ncand[:, None]).to(torch.float32) * w)
        return torch.cat(cands, dim=1), torch.cat(weights, dim=1)

    def _wfb_candidates(self, inputs):
        """forward + decode + do_wfb's filter of the three passes -> (cand (B, cap, 6), weight (B, cap)) on the device"""
        if self.hyp.get('mutil_label', False):                        # one row per (prediction, class): through the decoded tensors
            return self._wfb_decoded(self.test_time_augmentation(inputs)[1])
        cand, _ncand, _B, _cap, weight = self._tta_table(inputs, self._wfb_thresholds(True), self.wfb_weights)
        return cand, weight

    def _fuse_device(self, cand, weight):
        """yh_wbf_batched on a candidate table -> (out (B, cap, 6), nout (B,)) on the device; nothing is copied or awaited"""
        from ..hipk import wbf
        out, nout, _members = wbf(cand, weight, float(self.hyp['wfb_iou_threshold']), self.wfb_box_mean, num_class=self.num_class)
        return out, nout

    def _fusion_rows(self, cand, weight):
        """_fuse_device + the copy of its table to the host -> list (len B) of FloatTensor (n, 6), class ascending then in the order
        the clusters were founded, or None"""
        out, nout = self._fuse_device(cand, weight)
        self.last_ncand = (weight > 0).sum(dim=1).cpu().tolist()
        n_h = nout.cpu().tolist()
        out_h = out.cpu()
        return [None if n_h[b] == 0 else out_h[b, :n_h[b]].clone() for b in range(len(n_h))]

    @torch.no_grad()
    def do_wfb(self, preds_out):
        """"weighted fusion bbox" (trainer/eval_yolov5.py:44-92): the decoded tensors of the passes [(bs, X, 5+nc), ...] -> per
        image None, or the reference's nesting: one list per class present (ascending) of that class's fused rows, arrays
        [xmin, ymin, xmax, ymax, score, class] — the rows __call__ returns, from the same kernel"""
        rows = self._fusion_rows(*self._wfb_decoded(list(preds_out)))
        nested = []
        for r in rows:
            if r is None:
                nested.append(None)
                continue
            r = r.numpy()
            nested.append([[x for x in r[r[:, 5] == c]] for c in np.unique(r[:, 5])])
        return nested

    def _detections_device(self, inputs):
        """the forward and the merge of a batch by the configured path -> (det (B, K, 6), n (B,)) on the device: the NMS table, or
        with use_tta and hyp['wfb'] the fusion table"""
        if self.wfb:
            return self._fuse_device(*self._wfb_candidates(inputs))
        return self._nms_device(*self._candidates(inputs))

    def _desc(self, stage_preds):
        d = DecodeDesc()
        d.B = stage_preds[0].shape[0]
        d.num_class, d.num_anchor, d.num_stage = self.num_class, self.anchor_num, len(stage_preds)
        canon = []
        for s, p in enumerate(stage_preds):
            c, ld = to_cell_major(p)
            canon.append(c)
            d.H[s], d.W[s], d.ldp[s] = p.shape[2], p.shape[3], ld
            d.stride[s] = float(self.ds_scales[s])
            for a in range(self.anchor_num):
                d.anchors[(s * 3 + a) * 2], d.anchors[(s * 3 + a) * 2 + 1] = self._anchors_host[s][a]
        if len({c.dtype for c in canon}) != 1:
            canon = [to_cell_major(c.float())[0] for c in canon]
        d.pred_is_f32 = int(canon[0].dtype == torch.float32)
        d.yolox = 0
        ptrs = (C.c_void_p * 4)(*[c.data_ptr() for c in canon], *([None] * (4 - len(canon))))
        return d, canon, ptrs

    @torch.no_grad()
    def do_inference(self, inputs):
        """forward + decode: (bs, sum_s A*h*w, 5+nc) float32 in the reference's order
        (stage small->large, anchor, y, x) (:182-209)"""
        stage_preds = self.yolo(inputs)
        return self.decode(stage_preds)

    def decode(self, stage_preds):
        if not stage_preds[0].is_cuda:
            raise _lib.YoloHipError("YOLOV5Evaluator: tensors must live on an MI355X device")
        d, canon, ptrs = self._desc(stage_preds)
        n = sum(self.anchor_num * p.shape[2] * p.shape[3] for p in stage_preds)
        out = torch.empty(d.B, n, 5 + self.num_class, dtype=torch.float32, device=stage_preds[0].device)
        check(lib().yh_decode_full(C.byref(d), ptrs, out.data_ptr(), _lib.stream_ptr()), "yh_decode_full")
        return out

    def _nms_device(self, cand, ncand, B, cap):
        """yh_nms_batched on a candidate table -> (out (B, max_keep, 6), nkeep (B,)) on the device; nothing is copied or awaited"""
        dev = cand.device
        L = lib()
        max_keep = int(self.hyp['max_predictions_per_img'])
        out = torch.empty(B, max_keep, 6, dtype=torch.float32, device=dev)
        nkeep = torch.zeros(B, dtype=torch.int32, device=dev)
        keep = torch.empty(B, max_keep, dtype=torch.int32, device=dev)
        ws = torch.empty(L.yh_nms_ws_bytes(B, cap), dtype=torch.uint8, device=dev)
        check(L.yh_nms_batched(cand.data_ptr(), ncand.data_ptr(), B, cap, float(self.iou_threshold),
                               int(bool(self.hyp['agnostic'])), 1, max_keep, int(bool(self.hyp['postprocess_bbox'])),
                               out.data_ptr(), nkeep.data_ptr(), keep.data_ptr(), ws.data_ptr(), _lib.stream_ptr()), "yh_nms_batched")
        return out, nkeep

    def _run_nms(self, cand, ncand, B, cap):
        """_nms_device + the copy of its table to the host -> list (len B) of np.ndarray (n, 6) or None"""
        out, nkeep = self._nms_device(cand, ncand, B, cap)
        nc_h = ncand.cpu().tolist()
        nk_h = nkeep.cpu().tolist()
        self.last_ncand = nc_h                 # candidates that entered NMS per image (bench.py reports boxes/s from it)
        out_h = out.cpu().numpy()
        return [None if nc_h[b] == 0 else out_h[b, :nk_h[b]].copy() for b in range(B)]

    # ------------------------------------------------------------------ metric on the device
    @torch.no_grad()
    def evaluate_matches(self, inputs, ann, info, gt_hist=None):
        """The forward, filter and NMS (or fusion) of __call__, then yh_val_match on that table where it lies: the detections in the ORIGINAL
        frame and their true-positive matches against `ann`, as device tensors — nothing is copied to the host or awaited.
        :param ann: (B, maxbox, >= 5) [xmin, ymin, xmax, ymax, cls, ...] in the letterboxed frame, cls < 0 = padding (the collate format)
        :param info: (B, 5) float32 [scale, pad_top, pad_left, org_h, org_w], or the batch's list of resize_info dicts
        :param gt_hist: (num_class,) int32 device tensor to accumulate the ground-truth classes into (MatchAccumulator.gt_hist)
        :return: dict of box (B, K, 4), conf (B, K), cls (B, K) int32, iou (B, K), gt_idx (B, K) int32, tp (B, K) int16 (bit k: IoU
                 threshold k of mAP_v2, read it as uint16), nrow (B,) int32, gt_hist; rows at or past nrow[b] are undefined"""
        det, nkeep = self._detections_device(inputs)
        dev = det.device
        B, K = det.shape[0], det.shape[1]
        info = info_tensor(info).to(dev, non_blocking=True)
        ann = ann.to(device=dev, dtype=torch.float32)
        if ann.dim() != 3 or ann.shape[0] != B or ann.shape[2] < 5 or tuple(info.shape) != (B, 5):
            raise ValueError(f"evaluate_matches: ann {tuple(ann.shape)} / info {tuple(info.shape)} do not describe a batch of {B} images")
        if ann.shape[1] == 0:                                          # no ground truth at all: one padding row per image
            ann = torch.full((B, 1, 5), -1.0, dtype=torch.float32, device=dev)
        ann = ann.contiguous()
        if gt_hist is None:
            gt_hist = torch.zeros(self.num_class, dtype=torch.int32, device=dev)
        o = dict(box=torch.empty(B, K, 4, dtype=torch.float32, device=dev), conf=torch.empty(B, K, dtype=torch.float32, device=dev),
                 cls=torch.empty(B, K, dtype=torch.int32, device=dev), iou=torch.empty(B, K, dtype=torch.float32, device=dev),
                 gt_idx=torch.empty(B, K, dtype=torch.int32, device=dev), tp=torch.empty(B, K, dtype=torch.int16, device=dev),
                 nrow=torch.empty(B, dtype=torch.int32, device=dev), gt_hist=gt_hist)
        thr = (C.c_double * len(IOU_THRESHOLDS))(*IOU_THRESHOLDS)
        check(lib().yh_val_match(det.data_ptr(), nkeep.data_ptr(), ann.data_ptr(), info.data_ptr(), B, K, ann.shape[1], ann.shape[2],
                                 self.num_class, thr, len(IOU_THRESHOLDS), o['box'].data_ptr(), o['conf'].data_ptr(), o['cls'].data_ptr(),
                                 o['iou'].data_ptr(), o['gt_idx'].data_ptr(), o['tp'].data_ptr(), o['nrow'].data_ptr(),
                                 gt_hist.data_ptr(), _lib.stream_ptr()), "yh_val_match")
        return o

    def _nms_from_heads(self, stage_preds):
        """fused decode + filter + NMS straight from the head tensors (no decoded tensor is materialised)"""
        return self._run_nms(*self._cand_from_heads(stage_preds))

    def _cand_from_heads(self, stage_preds):
        if self.hyp.get('mutil_label', False):          # one candidate per (prediction, class): through the decoded tensor (:276-279)
            return self._filter_decoded(self.decode(stage_preds))
        d, canon, ptrs = self._desc(stage_preds)
        dev = stage_preds[0].device
        B = d.B
        n = sum(self.anchor_num * p.shape[2] * p.shape[3] for p in stage_preds)
        cap = min(((n + 3) // 4) * 4, 16384)
        while True:
            cand = torch.empty(B, cap, 6, dtype=torch.float32, device=dev)
            ncand = torch.zeros(B, dtype=torch.int32, device=dev)
            check(lib().yh_decode_filter(C.byref(d), ptrs, float(self.conf_threshold), float(self.cls_threshold),
                                         cand.data_ptr(), ncand.data_ptr(), cap, _decode_ws(self, d, dev), _lib.stream_ptr()), "yh_decode_filter")
            if cap >= n or int(ncand.max().item()) <= cap:
                break
            cap = ((n + 3) // 4) * 4
        return cand, ncand, B, cap

    _TTA_PASSES = ((1, None), (0.83, 2), (0.67, 3))       # (scale, flipped axis) of test_time_augmentation (:159-160)
    _TTA_FIRST_CAP = 3 * 16384                            # rows per image of the first try: _nms_from_heads' figure per pass

    def _view_desc(self, stage_preds, img):
        """descriptor of the heads one TTA pass returned for the network input `img`; `img` is unused here — the YOLOX override
        takes its strides from it"""
        return self._desc(stage_preds)

    @torch.no_grad()
    def _tta_from_heads(self, inputs):
        return self._run_nms(*self._tta_cand(inputs))

    @torch.no_grad()
    def _tta_cand(self, inputs):
        """test_time_augmentation + numba_nms without the decoded tensors: each pass is decoded, filtered, un-scaled and
        un-flipped straight from its heads (yh_decode_filter_view) and appended to one candidate table, in the order of the
        concatenation, before the next forward overwrites the engine's head buffers; one NMS over the table.  Same rows as
        numba_nms(test_time_augmentation(inputs)[0]), bit for bit."""
        return self._tta_table(inputs, (self.conf_threshold, self.cls_threshold))[:4]

    def _tta_table(self, inputs, thresholds, pass_weights=None):
        """_tta_cand's table under the given (conf, cls) thresholds -> (cand, ncand, B, cap, weight); with pass_weights, weight
        (B, cap) holds the weight of the pass that wrote each row (0 on the unused tail), set on the device from the counts before
        and after the pass"""
        conf_thr, cls_thr = thresholds
        img_h, img_w = inputs.size(2), inputs.size(3)
        cap = None
        while True:
            cand, n_all, weight = None, 0, None
            for k, (s, f) in enumerate(self._TTA_PASSES):
                img = inputs.flip(dims=(f,)) if f else inputs
                img = self.scale_img(img, s)
                d, canon, ptrs = self._view_desc(self.yolo(img), img)
                n = sum(d.num_anchor * d.H[i] * d.W[i] for i in range(d.num_stage))
                n_all += n
                if cand is None:
                    dev, B = canon[0].device, d.B
                    if cap is None:
                        cap = min(((3 * n + 3) // 4) * 4, self._TTA_FIRST_CAP)
                    cand = torch.empty(B, cap, 6, dtype=torch.float32, device=dev)
                    ncand = torch.zeros(B, dtype=torch.int32, device=dev)
                    if pass_weights is not None:
                        weight = torch.zeros(B, cap, dtype=torch.float32, device=dev)
                        col = torch.arange(cap, device=dev)[None, :]
                if weight is not None:
                    before = ncand.clone()
                xf = ViewXform(s, f or 0, img_h, img_w)
                check(lib().yh_decode_filter_view(C.byref(d), ptrs, C.byref(xf), float(conf_thr), float(cls_thr),
                                                  cand.data_ptr(), ncand.data_ptr(), cap, _decode_ws(self, d, dev), _lib.stream_ptr()),
                      "yh_decode_filter_view")
                if weight is not None:
                    weight.masked_fill_((col >= before[:, None]) & (col < ncand[:, None]), float(pass_weights[k]))
            if cap >= n_all or int(ncand.max().item()) <= cap:
                break
            cap = ((n_all + 3) // 4) * 4                  # one row per prediction of the three passes: cannot overflow
        return cand, ncand, B, cap, weight

    _FILTER_MODES = (0, 2)        # yh_filter_decoded mode of the single-label / hyp['mutil_label'] candidate rule (:266-286)

    def _filter_decoded(self, preds_out, thresholds=None, mode=None):
        """decoded (bs, N, 5+nc) -> candidate tables (bs, cap, 6) [xmin, ymin, xmax, ymax, conf, cls] + counts, on the device:
        obj >= conf threshold, cls * obj, arg-max > cls threshold or — hyp['mutil_label'] — one candidate per (prediction, class)
        in np.nonzero order (:266-286; yh_filter_decoded).  thresholds / mode: (conf, cls) and the yh_filter_decoded mode in place
        of the evaluator's own (the fusion path)"""
        conf_thr, cls_thr = thresholds or (self.conf_threshold, self.cls_threshold)
        p = preds_out.detach().to(torch.float32).contiguous()
        if not p.is_cuda:
            p = p.to(self.device if str(self.device).startswith("cuda") else "cuda:0")
        B, n, E = p.shape
        assert E == 5 + self.num_class
        cap = ((n + 3) // 4) * 4
        multi = bool(self.hyp.get('mutil_label', False))
        if mode is None:
            mode = self._FILTER_MODES[1 if multi else 0]
        while True:
            cand = torch.empty(B, cap, 6, dtype=torch.float32, device=p.device)
            ncand = torch.zeros(B, dtype=torch.int32, device=p.device)
            check(lib().yh_filter_decoded(p.data_ptr(), B, n, self.num_class, float(conf_thr), float(cls_thr), mode,
                                          cand.data_ptr(), ncand.data_ptr(), cap, _lib.stream_ptr()), "yh_filter_decoded")
            most = int(ncand.max().item()) if multi else 0          # multi-label: up to num_class candidates per prediction
            if most <= cap:
                break
            cap = ((most + 3) // 4) * 4
        return cand, ncand, B, cap

    def do_nms(self, preds_out):
        """"Do NMS with torch" (trainer/eval_yolov5.py:94-150): decoded (bs, X, 5+nc) -> list of (n, 6) device tensors or None.
        Candidate rule as numba_nms (yh_filter_decoded); suppression by utils.gpu_nms — hyp['iou_type'] one of iou / giou /
        diou / ciou, EXCLUSIVE threshold — on boxes offset by cls * 4096 when hyp['agnostic'] is set; at most
        max_predictions_per_img rows; with hyp['postprocess_bbox'] a kept box survives only if MORE than one candidate
        overlaps it by > threshold under `bbox_iou` (the unclamped IoU below; the box merge the reference computes there is
        written to a temporary it never returns, :143, so the rows are the candidates' own).  The reference's gpu_nms raises
        IndexError for more than one candidate (utils/nms.py:62-63 indexes a 1-D score tensor with a (1, M) mask); this follows
        the semantics its loop spells — the single-candidate and empty cases agree with it literally."""
        from ..utils.nms import gpu_nms
        cand, ncand, B, _cap = self._filter_decoded(preds_out)
        outputs = []
        for i, bbox_num in enumerate(ncand.cpu().tolist()):
            if not bbox_num:
                outputs.append(None)
                continue
            x = cand[i, :bbox_num]
            box_offset = x[:, 5] * 4096 if self.hyp['agnostic'] else x[:, 5] * 0.
            bboxes_offseted = x[:, :4] + box_offset[:, None]
            keep_index = gpu_nms(bboxes_offseted, x[:, 4].contiguous(), self.hyp['iou_type'], self.iou_threshold)
            if len(keep_index) > self.hyp['max_predictions_per_img']:
                keep_index = keep_index[:self.hyp['max_predictions_per_img']]
            if self.hyp['postprocess_bbox'] and 1 < bbox_num < 3000:
                iou = self.bbox_iou(bboxes_offseted[keep_index], bboxes_offseted)      # (N, M)
                keep_index = torch.tensor(keep_index)[((iou > self.iou_threshold).float().sum(dim=1) > 1).cpu()]
            outputs.append(x[keep_index])
        return outputs

    @staticmethod
    def bbox_iou(bbox1, bbox2):
        """(N, 4), (M, 4) xyxy -> (N, M) IoU exactly as trainer/eval_yolov5.py:237-258 spells it: NO clamp on the intersection
        sides (two boxes apart on BOTH axes get a positive "intersection", the product of two negative sides) and none on the
        union (0 / 0 = NaN).  yh_iou_matrix with a negative clamp."""
        assert bbox1.ndim == 2
        assert bbox2.ndim == 2
        from ..utils.bbox_tools import _iou_matrix
        return _iou_matrix(bbox1, bbox2, -1.0)

    def numba_nms(self, preds_out):
        """:param preds_out: decoded (bs, N, 5+nc) tensor -> list of np.ndarray (n,6) or None (:261-317)"""
        return self._run_nms(*self._filter_decoded(preds_out))

    def test_time_augmentation(self, inputs):
        """3 passes (1.0/none, 0.83/flip-y, 0.67/flip-x), un-scaled / un-flipped, concatenated (:152-179)"""
        img_h, img_w = inputs.size(2), inputs.size(3)
        aug_preds = []
        for s, f in zip([1, 0.83, 0.67], [None, 2, 3]):
            img = inputs.flip(dims=(f,)) if f else inputs
            img = self.scale_img(img, s)
            ripe = self.do_inference(img)
            ripe[..., :4] /= s
            if f == 2:
                ripe[..., 1] = img_h - ripe[..., 1]
            if f == 3:
                ripe[..., 0] = img_w - ripe[..., 0]
            aug_preds.append(ripe)
        return torch.cat(aug_preds, dim=1).contiguous(), aug_preds

    @staticmethod
    def scale_img(img, scale_factor):
        """:160-227 bilinear down-scale then pad to a multiple of 32 with 0.447"""
        if scale_factor == 1.0:
            return img
        h, w = img.shape[2], img.shape[3]
        new_h, new_w = int(scale_factor * h), int(scale_factor * w)
        img = F.interpolate(img, size=(new_h, new_w), align_corners=False, mode='bilinear')
        out_h, out_w = int(np.ceil(h / 32) * 32), int(np.ceil(w / 32) * 32)
        return F.pad(img, [0, out_w - new_w, 0, out_h - new_h], value=0.447)

    def make_grid(self, row_num, col_num):
        y, x = torch.meshgrid([torch.arange(row_num, device=self.device), torch.arange(col_num, device=self.device)], indexing='ij')
        return torch.stack((x, y), dim=2).reshape(row_num, col_num, 2)[None, None, ...].contiguous()
