"""YOLOV5Loss — host-side mirror of the reference class (loss/yolov5_loss.py:8-235)
over the HIP kernels of csrc/loss_v5.hip.  Same constructor, call signature, returned
dict and stateful ``balances``; the arithmetic runs on the GPU only.

Prediction tensors are consumed in place when they are the cell-major ("NHWC") views
the yoloseries_amd models return (shape (B, A*(5+nc), h, w), strides (h*w*ld, 1, w*ld, ld));
any other tensor is first copied into that layout (torch copy, off the fast path).
"""
import ctypes as C

import torch

from .. import _lib
from .._lib import V5LossDesc, check, lib
from ._base import BalancedLossBase, canon_heads

__all__ = ["YOLOV5Loss"]


class YOLOV5Loss(BalancedLossBase):
    _SAVED_BYTES, _WS_BYTES = "yh_v5loss_saved_bytes", "yh_v5loss_ws_bytes"
    _SIZE_ATTR = "input_img_size"
    _KEEP_LAST = False          # no debug reader of the last call's state: nothing keeps its `saved` buffer alive
    _MAX_GT = None

    def __init__(self, anchors, hyp, stage_num=3):
        """:param anchors: tensor (3, 3, 2) in pixels; :param hyp: flat config dict (config/config.py:14-20)"""
        super().__init__(stage_num)
        self.anchors = anchors
        self.hyp = hyp
        self.device = hyp['device']
        self.input_img_size = hyp['input_img_size']
        self.stage_num = stage_num
        self._anchors_host = [[[float(v) for v in a] for a in st] for st in anchors.detach().cpu().tolist()]

    def _make_desc(self, preds, targets):
        hyp = self.hyp
        d = V5LossDesc()
        d.B, d.maxbox = targets.shape[0], targets.shape[1]
        d.num_class = hyp['num_class']
        d.num_anchor = len(self._anchors_host[0])
        d.num_stage = len(preds)
        d.img_size0, d.img_size1 = float(self.input_img_size[0]), float(self.input_img_size[1])
        for s in range(d.num_stage):
            for a in range(d.num_anchor):
                d.anchors[(s * 3 + a) * 2 + 0] = self._anchors_host[s][a][0]
                d.anchors[(s * 3 + a) * 2 + 1] = self._anchors_host[s][a][1]
        d.anchor_thr = float(hyp['anchor_match_thr'])
        d.cls_smooth = float(hyp['class_smooth_factor'])
        d.cls_pos_weight = float(hyp['cls_pos_weight'])
        d.cof_pos_weight = float(hyp['cof_pos_weight'])
        d.use_focal = int(bool(hyp['use_focal_loss']))
        d.focal_gamma = float(hyp.get('focal_loss_gamma', 1.5))
        d.focal_alpha = float(hyp.get('focal_loss_alpha', 0.25))
        d.iou_scale, d.cof_scale, d.cls_scale = float(hyp['iou_loss_scale']), float(hyp['cof_loss_scale']), float(hyp['cls_loss_scale'])
        canon = canon_heads(preds)
        for s, c in enumerate(canon):
            d.H[s], d.W[s], d.ldp[s] = c.shape[2], c.shape[3], c.stride(3)
            assert c.shape[1] == d.num_anchor * (5 + d.num_class)
        d.pred_is_f32 = int(canon[0].dtype == torch.float32)
        d.targets_xywhn = 0
        return d, canon

    def _fwd(self, L, desc, ptrs, targets, result, saved, ws):
        check(L.yh_v5_loss_fwd(C.byref(desc), ptrs, targets.data_ptr(), self._balances.data_ptr(), result.data_ptr(),
                               saved.data_ptr(), ws.data_ptr(), _lib.stream_ptr()), "yh_v5_loss_fwd")

    def _bwd(self, L, desc, ptrs, targets, gout, saved, gptrs, ws):
        check(L.yh_v5_loss_bwd(C.byref(desc), ptrs, gout.data_ptr(), saved.data_ptr(), gptrs, ws.data_ptr(),
                               _lib.stream_ptr()), "yh_v5_loss_bwd")

    # ---- reference API ---------------------------------------------------------------------
    def __call__(self, stage_preds, targets_batch):
        """:param stage_preds: (small, mid, large) each (bn, A*(5+nc), h, w)
        :param targets_batch: (bn, bbox_num, 6) [xmin, ymin, xmax, ymax, cls, img_id], padding rows -1"""
        assert isinstance(stage_preds, (list, tuple))
        assert isinstance(targets_batch, torch.Tensor), f"targets's type should be torch.Tensor but we got {type(targets_batch)}"
        assert stage_preds[0].size(0) == targets_batch.size(0), "the length of predictions and targets should be the same"
        self._guard(stage_preds, targets_batch)
        tot, result = self._apply(stage_preds, targets_batch)
        return self._items(tot, result, ('iou_loss', 'cof_loss', 'cls_loss', 'tar_nums'))

    def match(self, targets, anchor_stage, fm_shape):
        """Reference signature (loss/yolov5_loss.py:142): targets (A, bn, bbox_num, 7) normalised
        [x, y, w, h, cls, img_id, anchor_id]; anchor_stage (A,2) in grid units; fm_shape [w, h].
        Returns tar_box (N,4), cls, img_idx, anc_idx, gy, gx (int64)."""
        L = lib()
        t = targets[0][..., :6].detach().to(torch.float32).contiguous()
        if not t.is_cuda:
            raise _lib.YoloHipError("YOLOV5Loss.match: tensors must live on an MI355X device")
        fw, fh = int(fm_shape[0]), int(fm_shape[1])
        d = V5LossDesc()
        d.B, d.maxbox, d.num_class, d.num_anchor, d.num_stage = t.shape[0], t.shape[1], self.hyp['num_class'], anchor_stage.shape[0], 1
        d.H[0], d.W[0], d.ldp[0] = fh, fw, ((anchor_stage.shape[0] * (5 + self.hyp['num_class']) + 7) // 8) * 8
        d.img_size0, d.img_size1 = float(fw), float(fw)      # ds = img_size1 / fw = 1: anchors are already in grid units
        av = anchor_stage.detach().cpu().tolist()
        for a in range(d.num_anchor):
            d.anchors[a * 2], d.anchors[a * 2 + 1] = float(av[a][0]), float(av[a][1])
        d.anchor_thr = float(self.hyp['anchor_match_thr'])
        d.targets_xywhn = 1
        cap = 5 * d.num_anchor * d.B * d.maxbox
        count = torch.zeros(1, dtype=torch.int32, device=t.device)
        tbox = torch.empty(cap, 4, dtype=torch.float32, device=t.device)
        tidx = torch.empty(cap, 5, dtype=torch.int32, device=t.device)
        check(L.yh_v5_assign(C.byref(d), t.data_ptr(), count.data_ptr(), tbox.data_ptr(), tidx.data_ptr(), None,
                             _lib.stream_ptr()), "yh_v5_assign")
        n = int(count.item())
        ti = tidx[:n].long()
        return tbox[:n], ti[:, 0], ti[:, 1], ti[:, 2], ti[:, 3], ti[:, 4]

    def assign(self, targets_batch, fm_sizes):
        """All stages at once from the raw batch targets (xyxy pixels): list of match() tuples."""
        L = lib()
        t = targets_batch.detach().to(torch.float32).contiguous()
        d = V5LossDesc()
        d.B, d.maxbox, d.num_class, d.num_anchor, d.num_stage = t.shape[0], t.shape[1], self.hyp['num_class'], len(self._anchors_host[0]), len(fm_sizes)
        d.img_size0, d.img_size1 = float(self.input_img_size[0]), float(self.input_img_size[1])
        ld = ((d.num_anchor * (5 + d.num_class) + 7) // 8) * 8      # no prediction is read here; the descriptor check wants ld >= A*(5+nc)
        for s, (fh, fw) in enumerate(fm_sizes):
            d.H[s], d.W[s], d.ldp[s] = fh, fw, ld
            for a in range(d.num_anchor):
                d.anchors[(s * 3 + a) * 2], d.anchors[(s * 3 + a) * 2 + 1] = self._anchors_host[s][a]
        d.anchor_thr = float(self.hyp['anchor_match_thr'])
        cap = 5 * d.num_anchor * d.B * d.maxbox
        S = d.num_stage
        count = torch.zeros(S, dtype=torch.int32, device=t.device)
        tbox = torch.empty(S, cap, 4, dtype=torch.float32, device=t.device)
        tidx = torch.empty(S, cap, 5, dtype=torch.int32, device=t.device)
        check(L.yh_v5_assign(C.byref(d), t.data_ptr(), count.data_ptr(), tbox.data_ptr(), tidx.data_ptr(), None,
                             _lib.stream_ptr()), "yh_v5_assign")
        outs = []
        for s, n in enumerate(count.tolist()):
            ti = tidx[s, :n].long()
            outs.append((tbox[s, :n], ti[:, 0], ti[:, 1], ti[:, 2], ti[:, 3], ti[:, 4]))
        return outs

    def focal_loss_factor(self, pred, target):
        """loss/yolov5_loss.py:216-235 (kept for API completeness; the kernels fuse it)."""
        prob = torch.sigmoid(pred)
        acc_scale = target * prob + (1.0 - target) * (1.0 - prob)
        gamma = self.hyp.get('focal_loss_gamma', 1.5)
        alpha = self.hyp.get('focal_loss_alpha', 0.25)
        return (1.0 - acc_scale) ** gamma * (target * alpha + (1.0 - target) * (1.0 - alpha))
