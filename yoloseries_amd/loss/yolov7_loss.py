"""YOLOV7Loss — host-side mirror of the reference class (loss/yolov7_loss.py:17-402) over the HIP kernels of
csrc/loss_v7.hip.  Same constructor, call signature, returned dict and stateful ``balances``; the YOLOv5 anchor match, the
SimOTA refinement over its candidates and every loss term run on the GPU without host synchronisation (the reference loops
over stages, images and targets in Python).  It takes the anchor heads of the YOLOv5 models: a drop-in alternative to
YOLOV5Loss.

A head is (B, A*(5+nc), h, w), consumed in place when it is the cell-major view the models return, or the reference's
(B, A, h, w, 5+nc), which is copied into that layout.  The tie rules (equal costs: lower candidate, then lower target row)
and the out-of-contract region are described in csrc/loss_v7.hip and DESIGN.md §4."""
import ctypes as C

import torch

from .. import _lib
from .._lib import V7LossDesc, check, lib
from ._base import BalancedLossBase, canon_heads

__all__ = ["YOLOV7Loss"]

MAX_TOPK = 24            # include/yolohip.h: the limit the YOLOv8 loss has


def _ref_layout_to_cell_major(p):
    """the reference's (bn, A, h, w, E) head -> the cell-major (bn, A*E, h, w) view of a new [bn][h][w][ld] buffer: ONE copy, made
    with differentiable torch ops so that the autograd graph carries the gradient back to `p`"""
    B, A, h, w, E = p.shape
    if p.dtype not in (torch.bfloat16, torch.float32):
        p = p.float()
    C_, ld = A * E, ((A * E + 7) // 8) * 8
    buf = p.new_zeros(B, h, w, ld)
    buf[..., :C_].view(B, h, w, A, E).copy_(p.permute(0, 2, 3, 1, 4))
    return buf[..., :C_].permute(0, 3, 1, 2)                 # strides (h*w*ld, 1, w*ld, ld): consumed in place


class YOLOV7Loss(BalancedLossBase):
    _SAVED_BYTES, _WS_BYTES = "yh_v7loss_saved_bytes", "yh_v7loss_ws_bytes"
    _SIZE_ATTR = "input_img_size"

    def __init__(self, anchors, hyp, stage_num=3):
        """:param anchors: tensor (stage_num, 3, 2) in pixels; :param hyp: flat config dict with the YOLOv5 loss's keys plus
        'topk' and 'use_iou_as_tar_cof'"""
        super().__init__(stage_num)
        self.anchors = anchors
        self.hyp = hyp
        self.device = hyp['device']
        self.input_img_size = hyp['input_img_size']
        self.stage_num = stage_num
        self.positive_smooth_cls, self.negative_smooth_cls = 0.95, 0.05        # smooth_bce() with its default (:11-13)
        self.use_iou_as_tar_cof = hyp["use_iou_as_tar_cof"]
        self._anchors_host = [[[float(v) for v in a] for a in st] for st in anchors.detach().cpu().tolist()]
        self._check_topk()

    def _check_topk(self):
        topk = self.hyp['topk']
        if int(topk) != topk or not 1 <= int(topk) <= MAX_TOPK:
            raise _lib.YoloHipError(f"YOLOV7Loss: topk={topk!r}; 1..{MAX_TOPK} are supported (include/yolohip.h)")

    def _make_desc(self, preds, targets):
        hyp = self.hyp
        self._check_topk()
        v = V7LossDesc()
        d = v.v5
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
        d.cls_smooth = self.positive_smooth_cls          # not read by the kernels: the class targets are fixed
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
        v.topk = int(hyp['topk'])
        v.use_iou_as_tar_cof = int(bool(self.use_iou_as_tar_cof))
        return v, canon

    def _fwd(self, L, desc, ptrs, targets, result, saved, ws):
        check(L.yh_v7_loss_fwd(C.byref(desc), ptrs, targets.data_ptr(), self._balances.data_ptr(), result.data_ptr(),
                               saved.data_ptr(), ws.data_ptr(), _lib.stream_ptr()), "yh_v7_loss_fwd")

    def _bwd(self, L, desc, ptrs, targets, gout, saved, gptrs, ws):
        check(L.yh_v7_loss_bwd(C.byref(desc), ptrs, gout.data_ptr(), saved.data_ptr(), gptrs, ws.data_ptr(),
                               _lib.stream_ptr()), "yh_v7_loss_bwd")

    # ---- reference API ---------------------------------------------------------------------
    def __call__(self, stage_preds, targets_batch):
        """:param stage_preds: dict (as in the reference) or list / tuple of the stage heads, small stride first, each
        (bn, A*(5+nc), h, w) or the reference's (bn, A, h, w, 5+nc)
        :param targets_batch: (bn, bbox_num, 6) [xmin, ymin, xmax, ymax, cls, img_id], padding rows -1"""
        heads = list(stage_preds.values()) if isinstance(stage_preds, dict) else list(stage_preds)
        assert isinstance(targets_batch, torch.Tensor), f"targets's type should be torch.Tensor but we got {type(targets_batch)}"
        assert heads[0].size(0) == targets_batch.size(0), "the length of predictions and targets should be the same"
        if len(heads) not in (3, 4):
            raise _lib.YoloHipError(f"YOLOV7Loss: {len(heads)} stages; 3 or 4 are supported")
        self._guard(heads, targets_batch)
        heads = [_ref_layout_to_cell_major(p) if p.dim() == 5 else p for p in heads]
        tot, result = self._apply(heads, targets_batch)
        return self._items(tot, result, ('iou_loss', 'cof_loss', 'cls_loss', 'tar_nums'))

    def matches(self):
        """(debug / tests) per stage an int32 array (n, 5) of the rows the last call matched, in candidate order:
        (img, anchor, gy, gx, target row inside the image's rows of the target tensor)"""
        desc, saved = self._last
        S, cap = desc.v5.num_stage, 5 * desc.v5.num_anchor * desc.v5.B * desc.v5.maxbox
        count = torch.zeros(4, dtype=torch.int32, device=saved.device)
        rows = torch.empty(S, cap, 5, dtype=torch.int32, device=saved.device)
        check(lib().yh_v7_matches(C.byref(desc), saved.data_ptr(), count.data_ptr(), rows.data_ptr(), _lib.stream_ptr()),
              "yh_v7_matches")
        return [rows[s, :n].cpu().numpy() for s, n in enumerate(count.tolist()[:S])]

    def focal_loss_factor(self, pred, target):
        """loss/yolov7_loss.py:383-402 (kept for API completeness; the kernels fuse it)."""
        prob = torch.sigmoid(pred)
        acc_scale = target * prob + (1.0 - target) * (1.0 - prob)
        gamma = self.hyp.get('focal_loss_gamma', 1.5)
        alpha = self.hyp.get('focal_loss_alpha', 0.25)
        return (1.0 - acc_scale) ** gamma * (target * alpha + (1.0 - target) * (1.0 - alpha))
