"""YOLOV8Evaluator — host-side mirror of trainer/eval_yolov8.py:11-227 over csrc/postproc_v8.hip and the NMS of csrc/postproc.hip.

forward -> DFL decode -> class sigmoid -> candidate filter -> class-aware greedy NMS -> merge filter all run on the GPU; only the
final (n, 6) rows per image cross PCIe.  The reference moves the whole head to the host for the softmax (:84) and runs the filter and
the NMS in NumPy.  `yolo` is any callable that returns the dict of head tensors (pred_xs, pred_s, pred_m, pred_l or the last 1-3
of them), each (b, 4*reg + num_class, h, w).  With use_tta each of the three passes is decoded, filtered, un-scaled and un-flipped
straight from its heads into one candidate table.  Rectangular maps use the grid (col + 0.5, row + 0.5), where the reference's
make_grid scrambles them.  hyp['wfb'] is not consulted, as in the reference.
"""
import ctypes as C

import torch

from .. import _lib
from .._lib import V8DecDesc, ViewXform, check, lib
from ..loss._base import canon_heads, stage_ptrs
from .eval_yolov5 import YOLOV5Evaluator

__all__ = ['YOLOV8Evaluator']


class YOLOV8Evaluator:

    def __init__(self, yolo, hyp, compute_metric=False):
        self.yolo = yolo
        self.hyp = hyp
        self.device = hyp['device']
        self.num_class = hyp['num_class']
        self.inp_h, self.inp_w = hyp['input_img_size']
        self.use_tta = hyp['use_tta']
        self.grids = None
        self.iou_threshold = hyp['compute_metric_iou_threshold'] if compute_metric else hyp['iou_threshold']
        self.cls_threshold = hyp['compute_metric_cls_threshold'] if compute_metric else hyp['cls_threshold']
        self.reg = hyp['reg']
        self.last_ncand = None

    # ------------------------------------------------------------------ reference API
    @torch.no_grad()
    def __call__(self, inputs):
        """:param inputs: (b, 3, h, w) -> list (len b) of FloatTensor (n, 6) [xmin, ymin, xmax, ymax, score, cls] on CPU, or None"""
        outs = self._run_nms(*self._candidates(inputs))
        return [torch.from_numpy(x) if x is not None else None for x in outs]

    def _candidates(self, inputs):
        """forward + decode + filter of a batch by the configured path -> candidate table (cand, ncand, B, cap) on the device"""
        if self.use_tta and self.hyp.get('mutil_label', False):       # through the decoded tensor, like _cand_from_heads
            return self._filter_decoded(self.test_time_augmentation(inputs)[0])
        if self.use_tta:
            return self._tta_cand(inputs)
        return self._cand_from_heads(self.yolo(inputs), inputs.size(2))

    def _desc(self, preds, img_h):
        """descriptor of the heads `preds` (dict or sequence) a forward of an input of height img_h returned"""
        plist = list(preds.values()) if isinstance(preds, dict) else list(preds)
        if not 1 <= len(plist) <= 4:
            raise _lib.YoloHipError(f"YOLOV8Evaluator: {len(plist)} stages; 1..4 are supported")
        E = 4 * int(self.reg) + int(self.num_class)
        for s, p in enumerate(plist):
            if not torch.is_tensor(p) or not p.is_cuda:
                raise _lib.YoloHipError("YOLOV8Evaluator: tensors must live on an MI355X device")
            if p.dim() != 4 or p.shape[1] != E or p.shape[0] != plist[0].shape[0]:
                raise _lib.YoloHipError(f"YOLOV8Evaluator: head {s} has shape {tuple(p.shape)}; expected ({plist[0].shape[0]}, {E}, h, w)")
        canon = canon_heads(plist)
        d = V8DecDesc()
        d.B, d.num_class, d.num_stage, d.reg = canon[0].shape[0], int(self.num_class), len(canon), int(self.reg)
        for s, c in enumerate(canon):
            d.H[s], d.W[s], d.ldp[s] = c.shape[2], c.shape[3], c.stride(3)
        d.pred_is_f32 = int(canon[0].dtype == torch.float32)
        d.img_h = float(img_h)
        return d, canon, stage_ptrs(canon)

    @staticmethod
    def _ncell(d):
        return sum(d.H[s] * d.W[s] for s in range(d.num_stage))

    @torch.no_grad()
    def do_inference(self, inputs):
        """forward + decode: (bs, N, 4 + nc) float32 [xmin, ymin, xmax, ymax, sigmoid(cls)...], stages in the dict's order, cells
        row-major (:88-102)"""
        return self.decode(self.yolo(inputs), inputs.size(2))

    def decode(self, preds, img_h):
        d, canon, ptrs = self._desc(preds, img_h)
        out = torch.empty(d.B, self._ncell(d), 4 + self.num_class, dtype=torch.float32, device=canon[0].device)
        check(lib().yh_v8_decode_full(C.byref(d), ptrs, out.data_ptr(), _lib.stream_ptr()), "yh_v8_decode_full")
        return out

    def post_processing(self, pred_reg):
        """(b, N, 4*reg) box logits -> (b, N, 4) distances [t, b, l, r] in grid units: softmax over each side's reg logits, expectation
        over the bins 1..reg (:76-85).  Through yh_v8_decode_full with every cell a 1 x 1 map of its own, img_h = 1 (stride 1,
        gx = gy = 0.5) and one dummy class: the box is (0.5 - l, 0.5 - t, 0.5 + r, 0.5 + b)."""
        if not pred_reg.is_cuda:
            raise _lib.YoloHipError("YOLOV8Evaluator: tensors must live on an MI355X device")
        b, n, c = pred_reg.shape
        buf = torch.zeros(b * n, ((c + 1 + 7) // 8) * 8, dtype=torch.float32, device=pred_reg.device)
        buf[:, :c] = pred_reg.detach().float().reshape(b * n, c)
        d = V8DecDesc()
        d.B, d.num_class, d.num_stage, d.reg = b * n, 1, 1, c // 4
        d.H[0], d.W[0], d.ldp[0], d.pred_is_f32, d.img_h = 1, 1, buf.shape[1], 1, 1.0
        out = torch.empty(b, n, 5, dtype=torch.float32, device=buf.device)
        check(lib().yh_v8_decode_full(C.byref(d), stage_ptrs([buf]), out.data_ptr(), _lib.stream_ptr()), "yh_v8_decode_full")
        return torch.stack((0.5 - out[..., 1], out[..., 3] - 0.5, 0.5 - out[..., 0], out[..., 2] - 0.5), dim=-1)

    # the NMS stage and the image scaling are the YOLOv5 evaluator's, unchanged: they read only hyp, iou_threshold and the table.
    # _nms_device -> (out (B, max_keep, 6), nkeep (B,)) on the device, the table yh_val_match consumes; _run_nms copies it to the
    # host and keeps last_ncand; scale_img is :104-120; bbox_iou :144-166 (no clamp on the intersection sides or the union)
    _nms_device = YOLOV5Evaluator._nms_device
    _run_nms = YOLOV5Evaluator._run_nms
    scale_img = staticmethod(YOLOV5Evaluator.scale_img)
    bbox_iou = staticmethod(YOLOV5Evaluator.bbox_iou)

    def _ws(self, d, dev):
        """workspace of the two-pass decode + filter, kept on the evaluator between calls"""
        need = int(lib().yh_v8_decode_filter_ws_bytes(C.byref(d)))
        ws = getattr(self, "_decode_ws_buf", None)
        if ws is None or ws.numel() < need or ws.device != torch.device(dev):
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
            self._decode_ws_buf = ws
        return ws.data_ptr()

    _FIRST_CAP = 16384                                    # rows per image and pass of the first try

    def _cand_from_heads(self, preds, img_h):
        """fused decode + filter straight from the head tensors (no decoded tensor is materialised)"""
        if self.hyp.get('mutil_label', False):          # one candidate per (cell, class): through the decoded tensor (:186-189)
            return self._filter_decoded(self.decode(preds, img_h))
        d, canon, ptrs = self._desc(preds, img_h)
        dev, B, n = canon[0].device, d.B, self._ncell(d)
        cap = min(((n + 3) // 4) * 4, self._FIRST_CAP)
        while True:
            cand = torch.empty(B, cap, 6, dtype=torch.float32, device=dev)
            ncand = torch.zeros(B, dtype=torch.int32, device=dev)
            check(lib().yh_v8_decode_filter(C.byref(d), ptrs, None, float(self.cls_threshold), cand.data_ptr(), ncand.data_ptr(), cap,
                                            self._ws(d, dev), _lib.stream_ptr()), "yh_v8_decode_filter")
            if cap >= n or int(ncand.max().item()) <= cap:
                break
            cap = ((n + 3) // 4) * 4                      # one row per cell: cannot overflow
        return cand, ncand, B, cap

    _TTA_PASSES = ((1, None), (0.83, 2), (0.67, 3))       # (scale, flipped axis) of test_time_augmentation (:47-48)

    @torch.no_grad()
    def _tta_cand(self, inputs):
        """test_time_augmentation + numba_nms' filter without the decoded tensors: the candidates of the three passes are appended to one
        table in pass order (the order of the concatenation, :73) — the same rows as the filter applied to the concatenated tensor"""
        img_h, img_w = inputs.size(2), inputs.size(3)
        cap = None
        while True:
            cand, n_all = None, 0
            for s, f in self._TTA_PASSES:
                img = inputs.flip(dims=(f,)) if f else inputs
                img = self.scale_img(img, s)
                d, canon, ptrs = self._desc(self.yolo(img), img.size(2))
                n_all += self._ncell(d)
                if cand is None:
                    dev, B = canon[0].device, d.B
                    if cap is None:
                        cap = min(((3 * self._ncell(d) + 3) // 4) * 4, 3 * self._FIRST_CAP)
                    cand = torch.empty(B, cap, 6, dtype=torch.float32, device=dev)
                    ncand = torch.zeros(B, dtype=torch.int32, device=dev)
                xf = ViewXform(s, f or 0, img_h, img_w)
                check(lib().yh_v8_decode_filter(C.byref(d), ptrs, C.byref(xf), float(self.cls_threshold), cand.data_ptr(),
                                                ncand.data_ptr(), cap, self._ws(d, dev), _lib.stream_ptr()), "yh_v8_decode_filter")
            if cap >= n_all or int(ncand.max().item()) <= cap:
                break
            cap = ((n_all + 3) // 4) * 4
        return cand, ncand, B, cap

    def _filter_decoded(self, preds_out):
        """decoded (bs, N, 4+nc) -> candidate tables (bs, cap, 6) + counts on the device (:175-196; yh_v8_filter_decoded)"""
        if not torch.is_tensor(preds_out) or not preds_out.is_cuda:
            raise _lib.YoloHipError("YOLOV8Evaluator: tensors must live on an MI355X device")
        p = preds_out.detach().to(torch.float32).contiguous()
        B, n, E = p.shape
        if E != 4 + self.num_class:
            raise _lib.YoloHipError(f"YOLOV8Evaluator: decoded tensor has {E} columns; expected {4 + self.num_class}")
        cap = ((n + 3) // 4) * 4
        multi = bool(self.hyp.get('mutil_label', False))
        while True:
            cand = torch.empty(B, cap, 6, dtype=torch.float32, device=p.device)
            ncand = torch.zeros(B, dtype=torch.int32, device=p.device)
            check(lib().yh_v8_filter_decoded(p.data_ptr(), B, n, self.num_class, float(self.cls_threshold), int(multi),
                                             cand.data_ptr(), ncand.data_ptr(), cap, _lib.stream_ptr()), "yh_v8_filter_decoded")
            most = int(ncand.max().item()) if multi else 0          # multi-label: up to num_class rows per cell
            if most <= cap:
                break
            cap = ((most + 3) // 4) * 4
        return cand, ncand, B, cap

    def numba_nms(self, preds_out):
        """:param preds_out: decoded (bs, N, 4+nc) device tensor -> list of np.ndarray (n, 6) or None (:168-227)"""
        return self._run_nms(*self._filter_decoded(preds_out))

    def test_time_augmentation(self, inputs):
        """3 passes (1.0 / none, 0.83 / flipped rows, 0.67 / flipped columns), un-scaled, un-flipped, concatenated (:40-73)"""
        img_h, img_w = inputs.size(2), inputs.size(3)
        aug_preds = []
        for s, f in self._TTA_PASSES:
            img = inputs.flip(dims=(f,)) if f else inputs
            img = self.scale_img(img, s)
            ripe = self.do_inference(img)
            ripe[..., :4] /= s
            if f == 2:
                ymin, ymax = img_h - ripe[..., 3], img_h - ripe[..., 1]
                ripe[..., 1], ripe[..., 3] = ymin, ymax
            if f == 3:
                xmin, xmax = img_w - ripe[..., 2], img_w - ripe[..., 0]
                ripe[..., 0], ripe[..., 2] = xmin, xmax
            aug_preds.append(ripe)
        return torch.cat(aug_preds, dim=1).contiguous(), aug_preds

    def make_grid(self, shape_list, strides, device):
        """[[h, w], ...], strides -> grid (N, 2) [x, y] = (col + 0.5, row + 0.5), stride (N, 1) (:122-141; the reference's own mesh is
        this grid for square maps only)"""
        g, s = [], []
        for stride, (h, w) in zip(strides, shape_list):
            y, x = torch.meshgrid(torch.arange(h, device=device) + 0.5, torch.arange(w, device=device) + 0.5, indexing='ij')
            g.append(torch.stack((x, y), dim=2).reshape(-1, 2))
            s.append(torch.ones((h * w, 1), device=device) * stride)
        return torch.cat(g, 0), torch.cat(s, 0)
