"""YOLOXLoss — host-side mirror of the reference class (loss/yolox_loss.py:11-458) over csrc/loss_yolox.hip.
Same constructor / call signature / returned dict / stateful ``balances``; like the reference it converts the
caller's target tensor from xyxy to xywh IN PLACE (:42).  SimOTA assignment and every loss term run on the GPU
without host synchronisation (the reference loops over images and ground truths in Python)."""
import ctypes as C

import torch

from .. import _lib
from .._lib import YoloxDesc, check, lib
from ._base import BalancedLossBase, canon_heads

__all__ = ["YOLOXLoss"]

_IOU_TYPES = {"iou": 0, "giou": 1, "ciou": 2}


class YOLOXLoss(BalancedLossBase):
    _SAVED_BYTES, _WS_BYTES = "yh_yolox_saved_bytes", "yh_yolox_ws_bytes"

    def __init__(self, hyp) -> None:
        super().__init__(hyp.get('num_stage', 3))
        self.hyp = hyp
        self.num_anchors = hyp['num_anchors']
        self.num_stage = hyp.get('num_stage', 3)
        self.img_sz = hyp['input_img_size']
        self.num_class = hyp['num_class']
        self.use_l1 = hyp.get('use_l1', True)
        self.iou_loss_scale = hyp.get('iou_loss_scale', 0.5)
        self.cls_loss_scale = hyp.get('cls_loss_scale', 1.0)
        self.l1_loss_scale = hyp.get('l1_loss_scale', 1.0)
        self.cof_loss_scale = hyp.get('cof_loss_scale', 1.0)
        self.device = hyp['device']
        self.cls_smoothness = hyp['class_smooth_factor']
        if self.num_anchors != 1:
            raise NotImplementedError("YOLOXLoss on the HIP path supports num_anchors=1 (the shipped configuration)")
        # class part of the SimOTA cost: the reference evaluates it on zero logits (label_assign :111-147), so it is one
        # constant; computed here with the reference's own fp32 expression
        t = torch.zeros(self.num_class); t[0] = float(self.cls_smoothness)
        pc = torch.sqrt(torch.sigmoid(torch.zeros(self.num_class)) * torch.sigmoid(torch.zeros(1)))
        self._cls_cost_const = float((-(t * torch.log(pc) + (1 - t) * torch.log(1 - pc))).sum(-1))

    def _make_desc(self, preds, targets):
        hyp = self.hyp
        d = YoloxDesc()
        d.B, d.maxbox, d.num_class, d.num_stage = targets.shape[0], targets.shape[1], self.num_class, len(preds)
        if any(p.dim() == 5 and p.shape[1] != 1 for p in preds):
            raise NotImplementedError("YOLOXLoss on the HIP path supports num_anchors=1")
        canon = canon_heads([p[:, 0] if p.dim() == 5 else p for p in preds])          # (B, 1, E, h, w) or (B, E, h, w)
        for s, c in enumerate(canon):
            d.H[s], d.W[s], d.ldp[s] = c.shape[2], c.shape[3], c.stride(3)
            assert c.shape[1] == 5 + self.num_class
        d.pred_is_f32 = int(canon[0].dtype == torch.float32)
        d.img_size0 = float(self.img_sz[0])
        d.use_focal = int(bool(hyp['use_focal_loss']))
        d.focal_gamma, d.focal_alpha = float(hyp.get('focal_loss_gamma', 1.5)), float(hyp.get('focal_loss_alpha', 0.25))
        d.use_l1 = int(bool(self.use_l1))
        d.iou_scale, d.cls_scale, d.cof_scale, d.l1_scale = (float(self.iou_loss_scale), float(self.cls_loss_scale),
                                                           float(self.cof_loss_scale), float(self.l1_loss_scale))
        d.cls_smooth = float(self.cls_smoothness)
        d.cls_pos_weight, d.cof_pos_weight = float(hyp.get("cls_pos_weight", 1.)), float(hyp.get("cof_pos_weight", 1.))
        d.iou_type = _IOU_TYPES[hyp['iou_type']]
        d.topk, d.center_radius = int(hyp['topk']), float(hyp['center_radius'])
        d.cls_cost_const = self._cls_cost_const
        return d, canon

    def _fwd(self, L, desc, ptrs, targets, result, saved, ws):
        check(L.yh_yolox_loss_fwd(C.byref(desc), ptrs, targets.data_ptr(), self._balances.data_ptr(), result.data_ptr(),
                                  saved.data_ptr(), ws.data_ptr(), _lib.stream_ptr()), "yh_yolox_loss_fwd")

    def _bwd(self, L, desc, ptrs, targets, gout, saved, gptrs, ws):
        check(L.yh_yolox_loss_bwd(C.byref(desc), ptrs, targets.data_ptr(), gout.data_ptr(), saved.data_ptr(), gptrs,
                                  _lib.stream_ptr()), "yh_yolox_loss_bwd")

    def __call__(self, preds, tars):
        """preds: dict {'pred_s','pred_m','pred_l'} of (N, num_anchors, 5+nc, h, w); tars: (N, bbox_num, 6)
        [xmin, ymin, xmax, ymax, class_id, img_id] — converted to [x_ctr, y_ctr, w, h, ...] in place."""
        plist = list(preds.values())
        self._guard(plist, tars)
        b = tars[..., :4].clone()
        tars[..., 0:2] = (b[..., 0:2] + b[..., 2:4]) / 2
        tars[..., 2:4] = b[..., 2:4] - b[..., 0:2]
        tot, result = self._apply(plist, tars)
        return self._items(tot, result, ('iou_loss', 'l1_loss', 'cls_loss', 'cof_loss', 'fg_nums', 'tar_nums'), counts=('fg_nums', 'tar_nums'))

    def foreground_masks(self):
        """(debug / tests) per-stage bool masks (N*h*w,) of the cells SimOTA selected in the last call."""
        desc, saved = self._last
        lay = torch.zeros(8, dtype=torch.int64)
        check(lib().yh_yolox_layout(C.byref(desc), lay.data_ptr()), "yh_yolox_layout")
        lay = lay.tolist()
        raw = saved.cpu().numpy()
        import numpy as np
        outs = []
        for s in range(desc.num_stage):
            n = desc.H[s] * desc.W[s]
            cnt = np.frombuffer(raw[lay[0]:lay[0] + 4 * 4 * desc.B].tobytes(), dtype=np.int32)[s * desc.B:(s + 1) * desc.B]
            cells = np.frombuffer(raw[lay[1]:].tobytes(), dtype=np.int32, count=lay[4 + s] + desc.B * n)[lay[4 + s]:]
            m = np.zeros(desc.B * n, dtype=bool)
            for b in range(desc.B):
                m[b * n + cells[b * n:b * n + cnt[b]]] = True
            outs.append(m)
        return outs
