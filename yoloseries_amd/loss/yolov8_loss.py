"""YOLOV8Loss — host-side mirror of the reference class (loss/yolov8_loss.py:12-411) over csrc/loss_v8.hip.
Same constructor keys / call signature / returned dict.  Task-aligned assignment, the class, CIoU and DFL terms and the whole
backward run on the GPU without host synchronisation and without any (B, M, N) matrix (the reference materialises several and
repeats the targets to (B, M, N, 4)).  The three deliberate departures from the reference (fewer than topk positive metrics,
rectangular maps, the NaN prompt) are described in csrc/loss_v8.hip and DESIGN.md §4."""
import ctypes as C

import torch

from .. import _lib
from .._lib import V8LossDesc, check, lib
from ._base import LossBase, canon_heads

__all__ = ["YOLOV8Loss"]


class YOLOV8Loss(LossBase):
    _SAVED_BYTES, _WS_BYTES = "yh_v8loss_saved_bytes", "yh_v8loss_ws_bytes"

    def __init__(self, hyp) -> None:
        super().__init__()
        self.hyp = hyp
        self.alpha = hyp['alpha']
        self.beta = hyp['beta']
        self.topk = hyp['topk']
        self.reg = hyp['reg']
        self.img_sz = hyp['input_img_size']
        self.num_class = hyp['num_class']
        self.iou_loss_scale = hyp.get('iou_loss_scale', 7.5)
        self.cls_loss_scale = hyp.get('cls_loss_scale', 0.5)
        self.dfl_loss_scale = hyp.get('dfl_loss_scale', 1.5)
        self.device = hyp['device']

    def _make_desc(self, preds, targets):
        hyp = self.hyp
        d = V8LossDesc()
        d.B, d.maxbox, d.num_class, d.num_stage = targets.shape[0], targets.shape[1], self.num_class, len(preds)
        d.reg, d.topk = int(self.reg), int(self.topk)
        for s, p in enumerate(preds):
            if p.dim() != 4 or p.shape[1] != 4 * self.reg + self.num_class or p.shape[0] != d.B:
                raise _lib.YoloHipError(f"YOLOV8Loss: head {s} has shape {tuple(p.shape)}; expected "
                                        f"({d.B}, {4 * self.reg + self.num_class}, h, w)")
        canon = canon_heads(preds)
        for s, c in enumerate(canon):
            d.H[s], d.W[s], d.ldp[s] = c.shape[2], c.shape[3], c.stride(3)
        d.pred_is_f32 = int(canon[0].dtype == torch.float32)
        d.img_size0 = float(self.img_sz[0])
        d.alpha, d.beta = float(self.alpha), float(self.beta)
        d.focal_gamma, d.focal_alpha = float(hyp.get('focal_loss_gamma', 1.5)), float(hyp.get('focal_loss_alpha', 0.25))
        d.cls_pos_weight = float(hyp.get("cls_pos_weight", 1.))
        d.iou_scale, d.cls_scale, d.dfl_scale = float(self.iou_loss_scale), float(self.cls_loss_scale), float(self.dfl_loss_scale)
        return d, canon

    def _fwd(self, L, desc, ptrs, targets, result, saved, ws):
        check(L.yh_v8_loss_fwd(C.byref(desc), ptrs, targets.data_ptr(), result.data_ptr(), saved.data_ptr(), ws.data_ptr(),
                               _lib.stream_ptr()), "yh_v8_loss_fwd")

    def _bwd(self, L, desc, ptrs, targets, gout, saved, gptrs, ws):
        check(L.yh_v8_loss_bwd(C.byref(desc), ptrs, targets.data_ptr(), gout.data_ptr(), saved.data_ptr(), gptrs,
                               ws.data_ptr(), _lib.stream_ptr()), "yh_v8_loss_bwd")

    def __call__(self, preds, tars):
        """preds: dict of (b, 4*reg + num_class, h, w) head tensors, stages in the dict's order; tars: (b, M, 6)
        [xmin, ymin, xmax, ymax, class_id, img_id], padding rows class_id < 0."""
        plist = list(preds.values())
        if not 1 <= len(plist) <= 4:
            raise _lib.YoloHipError(f"YOLOV8Loss: {len(plist)} stages; 1..4 are supported")
        self._guard(plist, tars)
        tot, result = self._apply(plist, tars)
        return self._items(tot, result, ('cls_loss', 'iou_loss', 'dfl_loss', 'tar_nums'))

    def assignment(self):
        """(debug / tests) per stage an int32 array (b, h*w): the target row matched to each cell in the last call, -1 where none."""
        desc, saved = self._last
        lay = torch.zeros(8, dtype=torch.int64)
        check(lib().yh_v8loss_layout(C.byref(desc), lay.data_ptr()), "yh_v8loss_layout")
        lay = lay.tolist()
        n_all = lay[2]
        own = saved[lay[0]:lay[0] + 4 * desc.B * n_all].cpu().numpy().view("int32").reshape(desc.B, n_all)
        return [own[:, lay[4 + s]:lay[4 + s] + desc.H[s] * desc.W[s]].copy() for s in range(desc.num_stage)]
