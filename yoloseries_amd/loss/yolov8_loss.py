"""YOLOV8Loss — host-side mirror of the reference class (loss/yolov8_loss.py:12-411) over csrc/loss_v8.hip.
Same constructor keys / call signature / returned dict.  Task-aligned assignment, the class, CIoU and DFL terms and the whole
backward run on the GPU without host synchronisation and without any (B, M, N) matrix (the reference materialises several and
repeats the targets to (B, M, N, 4)).  The three deliberate departures from the reference (fewer than topk positive metrics,
rectangular maps, the NaN prompt) are described in csrc/loss_v8.hip and DESIGN.md §4."""
import ctypes as C

import torch

from .. import _lib
from .._lib import V8LossDesc, check, lib
from ..layout import to_cell_major

__all__ = ["YOLOV8Loss"]

MAX_GT = 128          # valid ground truths per image (include/yolohip.h)


class _V8LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, targets, *preds):
        desc, canon = owner._make_desc(preds, targets)
        L = lib()
        dev = targets.device
        saved = torch.empty(L.yh_v8loss_saved_bytes(C.byref(desc)), dtype=torch.uint8, device=dev)
        ws = owner._workspace(L.yh_v8loss_ws_bytes(C.byref(desc)), dev)
        result = torch.empty(8, dtype=torch.float32, device=dev)
        ptrs = (C.c_void_p * 4)(*[c.data_ptr() for c in canon], *([None] * (4 - len(canon))))
        check(L.yh_v8_loss_fwd(C.byref(desc), ptrs, targets.data_ptr(), result.data_ptr(), saved.data_ptr(), ws.data_ptr(),
                               _lib.stream_ptr()), "yh_v8_loss_fwd")
        ctx.owner, ctx.desc, ctx.canon, ctx.saved, ctx.targets = owner, desc, canon, saved, targets
        ctx.in_meta = [p.dtype for p in preds]
        owner._last = (desc, saved)
        ctx.mark_non_differentiable(result)
        return result[0:1].clone(), result

    @staticmethod
    def backward(ctx, gtot, _gres):
        L = lib()
        desc, canon = ctx.desc, ctx.canon
        gout = gtot.to(torch.float32).contiguous()
        gbufs = [torch.empty(c.shape[0], c.shape[2], c.shape[3], c.stride(3), dtype=c.dtype, device=c.device) for c in canon]
        ws = ctx.owner._workspace(L.yh_v8loss_ws_bytes(C.byref(desc)), gout.device)
        ptrs = (C.c_void_p * 4)(*[c.data_ptr() for c in canon], *([None] * (4 - len(canon))))
        gptrs = (C.c_void_p * 4)(*[g.data_ptr() for g in gbufs], *([None] * (4 - len(canon))))
        check(L.yh_v8_loss_bwd(C.byref(desc), ptrs, ctx.targets.data_ptr(), gout.data_ptr(), ctx.saved.data_ptr(), gptrs,
                               ws.data_ptr(), _lib.stream_ptr()), "yh_v8_loss_bwd")
        outs = []
        for g, c, dtype in zip(gbufs, canon, ctx.in_meta):
            Bn, Ct, h, w = c.shape
            ld = c.stride(3)
            v = g.as_strided((Bn, Ct, h, w), (h * w * ld, 1, w * ld, ld))
            outs.append(v if v.dtype == dtype else v.to(dtype))
        return (None, None, *outs)


class YOLOV8Loss:

    def __init__(self, hyp) -> None:
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
        self._ws = None
        self._last = None

    def set_input_img_size(self, hw):
        """The size [h, w] of the images behind the next predictions (multi-scale training: the size of the step).  The stage
        strides are img_sz[0] / h of each head, taken from this attribute at every call; a NEW list is stored, so
        `hyp['input_img_size']` keeps the configured value."""
        self.img_sz = [int(hw[0]), int(hw[1])]

    def _workspace(self, nbytes, dev):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self._ws

    def _make_desc(self, preds, targets):
        hyp = self.hyp
        d = V8LossDesc()
        d.B, d.maxbox, d.num_class, d.num_stage = targets.shape[0], targets.shape[1], self.num_class, len(preds)
        d.reg, d.topk = int(self.reg), int(self.topk)
        canon = []
        for s, p in enumerate(preds):
            if p.dim() != 4 or p.shape[1] != 4 * self.reg + self.num_class or p.shape[0] != d.B:
                raise _lib.YoloHipError(f"YOLOV8Loss: head {s} has shape {tuple(p.shape)}; expected "
                                        f"({d.B}, {4 * self.reg + self.num_class}, h, w)")
            c, ld = to_cell_major(p)
            canon.append(c)
            d.H[s], d.W[s], d.ldp[s] = c.shape[2], c.shape[3], ld
        if len({c.dtype for c in canon}) != 1:
            canon = [to_cell_major(c.float())[0] for c in canon]
        d.pred_is_f32 = int(canon[0].dtype == torch.float32)
        d.img_size0 = float(self.img_sz[0])
        d.alpha, d.beta = float(self.alpha), float(self.beta)
        d.focal_gamma, d.focal_alpha = float(hyp.get('focal_loss_gamma', 1.5)), float(hyp.get('focal_loss_alpha', 0.25))
        d.cls_pos_weight = float(hyp.get("cls_pos_weight", 1.))
        d.iou_scale, d.cls_scale, d.dfl_scale = float(self.iou_loss_scale), float(self.cls_loss_scale), float(self.dfl_loss_scale)
        return d, canon

    def __call__(self, preds, tars):
        """preds: dict of (b, 4*reg + num_class, h, w) head tensors, stages in the dict's order; tars: (b, M, 6)
        [xmin, ymin, xmax, ymax, class_id, img_id], padding rows class_id < 0."""
        plist = list(preds.values())
        if not 1 <= len(plist) <= 4:
            raise _lib.YoloHipError(f"YOLOV8Loss: {len(plist)} stages; 1..4 are supported")
        if not plist[0].is_cuda:
            raise _lib.YoloHipError("YOLOV8Loss: predictions must live on an MI355X device (no CPU path in the product)")
        dev = plist[0].device
        # a target tensor with more than MAX_GT rows may hold more valid boxes in one image than the library accepts: refused here,
        # before any launch (tensors of up to MAX_GT rows cannot, and pay no host synchronisation for the check)
        if tars.shape[1] > MAX_GT:
            most = int((tars[..., 4] >= 0).sum(dim=1).max().item()) if tars.shape[0] else 0
            if most > MAX_GT:
                raise _lib.YoloHipError(f"YOLOV8Loss: an image has {most} ground-truth boxes; at most {MAX_GT} per image are "
                                        f"supported (include/yolohip.h)")
        targets = tars.detach().to(device=dev, dtype=torch.float32).contiguous()
        tot, result = _V8LossFn.apply(self, targets, *plist)
        if self.hyp.get('loss_items_on_device', False):
            return {'tot_loss': tot, 'cls_loss': result[1], 'iou_loss': result[2], 'dfl_loss': result[3], 'tar_nums': result[4]}
        r = result.tolist()
        return {'tot_loss': tot, 'cls_loss': r[1], 'iou_loss': r[2], 'dfl_loss': r[3], 'tar_nums': int(r[4])}

    def assignment(self):
        """(debug / tests) per stage an int32 array (b, h*w): the target row matched to each cell in the last call, -1 where none."""
        desc, saved = self._last
        lay = torch.zeros(8, dtype=torch.int64)
        check(lib().yh_v8loss_layout(C.byref(desc), lay.data_ptr()), "yh_v8loss_layout")
        lay = lay.tolist()
        n_all = lay[2]
        own = saved[lay[0]:lay[0] + 4 * desc.B * n_all].cpu().numpy().view("int32").reshape(desc.B, n_all)
        return [own[:, lay[4 + s]:lay[4 + s] + desc.H[s] * desc.W[s]].copy() for s in range(desc.num_stage)]
