"""What the three loss classes share on the host: the head tensors in cell-major layout, the workspace cache, the stage pointer
arrays, the gradient buffers and their views, the ground-truth-count guard, the ``balances`` state and ONE autograd Function
that calls the owner's forward and backward entry points.  A loss class adds its constructor, its descriptor (``_make_desc``),
the two library calls (``_fwd`` / ``_bwd``) and its result dictionary."""
import ctypes as C

import torch

from .. import _lib
from ..layout import cell_major_view, to_cell_major

MAX_GT = 128          # valid ground truths per image (include/yolohip.h; MAXG in csrc/loss_yolox.hip holds them in LDS)


def canon_heads(heads):
    """(B, C, h, w) head tensors -> cell-major views of one dtype (fp32 where the heads' dtypes differ); ld = c.stride(3)"""
    canon = [to_cell_major(p)[0] for p in heads]
    if len({c.dtype for c in canon}) != 1:
        canon = [to_cell_major(c.float())[0] for c in canon]
    return canon


def stage_ptrs(tensors):
    """the 4-slot pointer array of the C entry points"""
    return (C.c_void_p * 4)(*[t.data_ptr() for t in tensors], *([None] * (4 - len(tensors))))


class LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, targets, *preds):
        desc, canon = owner._make_desc(preds, targets)
        L = _lib.lib()
        dev = targets.device
        saved = torch.empty(getattr(L, owner._SAVED_BYTES)(C.byref(desc)), dtype=torch.uint8, device=dev)
        ws = owner._workspace(getattr(L, owner._WS_BYTES)(C.byref(desc)), dev)
        result = torch.empty(8, dtype=torch.float32, device=dev)
        owner._fwd(L, desc, stage_ptrs(canon), targets, result, saved, ws)
        ctx.owner, ctx.desc, ctx.canon, ctx.saved, ctx.targets = owner, desc, canon, saved, targets
        ctx.in_meta = [(p.dim(), p.dtype) for p in preds]
        if owner._KEEP_LAST:
            owner._last = (desc, saved)
        ctx.mark_non_differentiable(result)
        return result[0:1].clone(), result

    @staticmethod
    def backward(ctx, gtot, _gres):
        L = _lib.lib()
        owner, desc, canon = ctx.owner, ctx.desc, ctx.canon
        gout = gtot.to(torch.float32).contiguous()
        gbufs = [torch.empty(c.shape[0], c.shape[2], c.shape[3], c.stride(3), dtype=c.dtype, device=c.device) for c in canon]
        ws = owner._workspace(getattr(L, owner._WS_BYTES)(C.byref(desc)), gout.device)
        owner._bwd(L, desc, stage_ptrs(canon), ctx.targets, gout, ctx.saved, stage_ptrs(gbufs), ws)
        outs = []
        for g, c, (ndim, dtype) in zip(gbufs, canon, ctx.in_meta):
            v = cell_major_view(g, c.shape[1])
            if ndim == 5:          # YOLOX heads given as (B, 1, E, h, w)
                v = v.unsqueeze(1)
            outs.append(v if v.dtype == dtype else v.to(dtype))
        return (None, None, *outs)


class LossBase:
    _SAVED_BYTES = _WS_BYTES = None          # names of the library's size queries
    _SIZE_ATTR = "img_sz"                    # the public attribute that holds the input size [h, w]
    _KEEP_LAST = True                        # keep (desc, saved) of the last call for the debug readers
    _MAX_GT = MAX_GT                         # None: any number of valid ground truths per image

    def __init__(self):
        self._ws = None
        self._last = None

    def set_input_img_size(self, hw):
        """The size [h, w] of the images behind the next predictions (multi-scale training: the size of the step).  Everything a
        call derives from the size -- target normalisation, the anchors' grid scale, the stage strides -- goes into a descriptor
        built from this attribute when the call runs (nothing of an earlier size is kept); a NEW list is stored, so
        `hyp['input_img_size']`, which the evaluators share, keeps the configured value.  (The reference normalises by the
        configured size whatever the step's: DESIGN.md section 4.)"""
        setattr(self, self._SIZE_ATTR, [int(hw[0]), int(hw[1])])

    def _workspace(self, nbytes, dev):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self._ws

    def _guard(self, heads, tars):
        """refuses, before any launch, heads off the device and more valid ground truths in one image than the library accepts"""
        name = type(self).__name__
        if not heads[0].is_cuda:
            raise _lib.YoloHipError(f"{name}: predictions must live on an MI355X device (no CPU path in the product)")
        # only a target tensor with more than MAX_GT rows can hold too many valid boxes: smaller ones pay no host synchronisation
        if self._MAX_GT is not None and tars.shape[1] > self._MAX_GT:
            most = int((tars[..., 4] >= 0).sum(dim=1).max().item()) if tars.shape[0] else 0
            if most > self._MAX_GT:
                raise _lib.YoloHipError(f"{name}: an image has {most} ground-truth boxes; at most {self._MAX_GT} per image are "
                                        f"supported (include/yolohip.h)")

    def _apply(self, heads, tars):
        """-> (tot_loss with the autograd graph behind it, the 8 result floats on the device)"""
        dev = heads[0].device
        targets = tars.detach().to(device=dev, dtype=torch.float32).contiguous()
        return LossFn.apply(self, targets, *heads)

    def _items(self, tot, result, names, counts=("tar_nums",)):
        """the returned dictionary: names[i] = result[1 + i]; `counts` are ints where the scalars are read back"""
        if self.hyp.get('loss_items_on_device', False):
            # no host sync: the scalars stay on the device (bench / graph-captured training loops)
            return {'tot_loss': tot, **{k: result[1 + i] for i, k in enumerate(names)}}
        r = result.tolist()
        return {'tot_loss': tot, **{k: int(r[1 + i]) if k in counts else r[1 + i] for i, k in enumerate(names)}}


class BalancedLossBase(LossBase):
    """a loss with the stateful per-stage objectness `balances` (an fp64 device vector the forward kernel reads and updates)"""

    def __init__(self, num_stage):
        super().__init__()
        self._num_stage = num_stage
        self._init_balances = [4., 1., 0.4] if num_stage == 3 else [4., 1., 0.4, 0.1]
        self._balances = None

    @property
    def balances(self):
        if self._balances is None:
            return list(self._init_balances)
        return self._balances.cpu().tolist()[:self._num_stage]

    @balances.setter
    def balances(self, v):
        self._init_balances = [float(x) for x in v]
        if self._balances is not None:
            self._balances[:len(v)] = torch.tensor(self._init_balances, dtype=torch.float64, device=self._balances.device)

    def _apply(self, heads, tars):
        dev = heads[0].device
        if self._balances is None or self._balances.device != dev:
            self._balances = torch.zeros(4, dtype=torch.float64, device=dev)
            self._balances[:len(self._init_balances)] = torch.tensor(self._init_balances, dtype=torch.float64)
        return super()._apply(heads, tars)
