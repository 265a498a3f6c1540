"""Flat-arena optimizers for the HIP models: the three parameter groups of the reference's ``_init_optimizer``
(train_yolov5.py:258-280 — BN weights | conv weights + weight decay | biases) with either of its two branches,
torch.optim.SGD(nesterov) (FlatSGD) or torch.optim.Adam (FlatAdam), clip_grad_norm_(10) (:344) and zero_grad in three launches
over the model's flat parameter arena instead of ~3x177 per-tensor kernels.

``param_groups`` is a list of dicts with 'lr' / 'initial_lr' / 'weight_decay' and 'momentum' (SGD) or 'betas' / 'eps' (Adam), so
the reference's warm-up code (train_yolov5.py:437-456) can mutate it unchanged: it moves 'momentum' only where a group has one."""
import torch
from torch import nn

from .. import hipk
from .._lib import YoloHipError

__all__ = ['FlatSGD', 'FlatAdam']


class _FlatOptimizer:
    """what the two optimizers share: the lazily built group map over the parameter arena, the flat gradient hand-off
    (accumulation, data-parallel exchange), gradient clipping through a device scalar and the host bookkeeping around a captured
    step.  A subclass keeps its state tensors (_build_state), its device scalars (_sync_scalars) and its kernels (_launch)."""

    def __init__(self, model):
        self.model = model
        model.flat_grads_only = True
        self._built_for = None
        self.steps = 0
        self._gacc = None
        self._nacc = 0
        model._yh_grad_hook_opt = self._on_grad

    @property
    def _who(self):
        return type(self).__name__

    def _build(self, pack):
        gid = {}
        for m in self.model.modules():
            if hasattr(m, "bias") and isinstance(m.bias, nn.Parameter):
                gid[id(m.bias)] = 2
            if isinstance(m, nn.BatchNorm2d):
                gid[id(m.weight)] = 0
            elif hasattr(m, 'weight') and isinstance(m.weight, nn.Parameter):
                gid[id(m.weight)] = 1
        dev = pack.device
        group = torch.empty(pack.n, dtype=torch.uint8, device=dev)
        o = 0
        for p in pack.params:
            group[o:o + p.numel()] = gid.get(id(p), 1)
            o += p.numel()
        self.group = group
        self._build_state(pack.n, dev)
        self.part = torch.zeros(4096, dtype=torch.float32, device=dev)
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.scale = torch.ones(1, dtype=torch.float32, device=dev)
        self._lr_host = None
        self._built_for = pack
        self._use_scale = False

    def _state_from_pending(self, pending, n, dev, what):
        """a zeroed state tensor of the arena's size, or the one a checkpoint brought before the arena existed (resume)"""
        t = torch.zeros(n, dtype=torch.float32, device=dev)
        if pending is not None:
            if pending.numel() != n:
                raise YoloHipError(f"{self._who}: checkpointed {what} has {pending.numel()} elements, the model {n}")
            t.copy_(pending.to(dev))
        return t

    def _pack(self):
        st = self.model.__dict__.get('_yh')
        if not st or st['pack'] is None:
            raise YoloHipError(f"{self._who}: run a forward pass first (the parameter arena is created lazily)")
        if self._built_for is not st['pack']:
            self._build(st['pack'])
        return st['pack']

    def _on_grad(self, flat_g):
        # gradient accumulation over several backward() calls (train_yolov5.py:327-337)
        if self._nacc == 0:
            self._gacc = flat_g
        else:
            self._gacc = self._gacc + flat_g
        self._nacc += 1

    def replace_accumulated(self):
        """the data-parallel exchange averaged the ACCUMULATED gradient at an accumulation boundary and hands it over as
        the next flat gradient: drop the local sum so that _on_grad() takes the average as is (utils/dist.py)"""
        self._gacc, self._nacc = None, 0

    def _grad(self):
        g = self._gacc if self._gacc is not None else getattr(self.model, "_yh_last_flat_grad", None)
        if g is None:
            raise YoloHipError(f"{self._who}.step(): no gradient (call backward() first)")
        return g

    def clip_grad_norm_(self, max_norm):
        self._pack()
        g = self._grad()
        hipk.sumsq(g, self.part, self.sumsq)
        hipk.clip_scale(self.sumsq, max_norm, self.scale)
        self._use_scale = True
        return self.sumsq          # device scalar: total_norm ** 2 (no host sync)

    def _push(self, dst, vals, what):
        """`vals` into the device tensor `dst`.  The copy is an ordinary stream-ordered H2D from pageable memory: staged when it is
        issued, so the host may run ahead; it must be issued outside a graph capture (GraphedStep calls this before each replay)."""
        if torch.cuda.is_current_stream_capturing():
            raise YoloHipError(f"{self._who}: {what} changed inside a graph capture; call graph_pre_replay() "
                               "(or step once eagerly) before capturing")
        dst.copy_(torch.tensor(vals, dtype=dst.dtype))

    def step(self):
        pack = self._pack()
        g = self._grad()
        self._sync_scalars()
        self._launch(pack, g, self.scale if self._use_scale else None)
        self.steps += 1
        self._use_scale = False

    def graph_pre_replay(self):
        """host-side bookkeeping of one step that runs as a graph replay: refresh the device scalars if the schedule moved
        them, count the step"""
        self._pack()
        self._sync_scalars()
        self.steps += 1

    def graph_pre_capture(self):
        """push the device scalars outside the capture that is about to start"""
        self._pack()
        self._sync_scalars()

    def graph_snapshot(self):
        return (self.steps, self._use_scale)

    def graph_restore(self, snap):
        """a capture failed after step() had advanced the host counters without running a kernel"""
        self.steps, self._use_scale = snap
        self._lr_host = None                      # rewrite the device scalars at the next step

    def zero_grad(self, set_to_none=True):
        self._gacc, self._nacc = None, 0
        self.model._yh_last_flat_grad = None


class FlatSGD(_FlatOptimizer):

    def __init__(self, model, lr, momentum=0.937, weight_decay=1e-4, nesterov=True):
        super().__init__(model)
        self.nesterov = nesterov
        self.param_groups = [
            {"name": "bn_weight", "lr": lr, "initial_lr": lr, "momentum": momentum, "weight_decay": 0.0},
            {"name": "weight", "lr": lr, "initial_lr": lr, "momentum": momentum, "weight_decay": weight_decay},
            {"name": "bias", "lr": lr, "initial_lr": lr, "momentum": momentum, "weight_decay": 0.0},
        ]
        self._pending_buf = None        # momentum buffer loaded before the parameter arena exists (resume)

    def _build_state(self, n, dev):
        self.buf = self._state_from_pending(self._pending_buf, n, dev, "momentum buffer")
        self._pending_buf = None
        # per-step scalars live in device memory (lr[3] | wd[3] | momentum | first-step flag): the step kernel takes no
        # host value as a launch argument, so a captured hipGraph of the step replays correctly (utils/graph.py)
        self.scal = torch.zeros(8, dtype=torch.float32, device=dev)

    def _sync_scalars(self):
        """device copy of lr / weight decay / momentum / first-step flag, rewritten only when a value changed (warm-up,
        per-epoch schedule)"""
        vals = tuple(float(pg["lr"]) for pg in self.param_groups) + tuple(float(pg["weight_decay"]) for pg in self.param_groups) + \
            (float(self.param_groups[0]["momentum"]), 1.0 if self.steps == 0 else 0.0)
        if vals != self._lr_host:
            self._push(self.scal, vals, "learning-rate / momentum")
            self._lr_host = vals

    def _launch(self, pack, g, scale):
        hipk.sgd_step_dev(pack.flat, g, self.buf, self.group, self.scal, self.nesterov, scale)

    def state_dict(self):
        buf = self.buf if self._built_for is not None else self._pending_buf
        return {"momentum_buffer": buf, "steps": self.steps, "param_groups": [dict(g) for g in self.param_groups]}

    def load_state_dict(self, sd):
        """Training.load_model() runs before the first forward, i.e. before the flat parameter arena (and with it the
        momentum buffer) exists: the loaded buffer is kept and copied in when the arena is built."""
        self.param_groups = [dict(g) for g in sd["param_groups"]]
        self.steps = sd["steps"]
        mb = sd.get("momentum_buffer")
        if mb is None:
            if self.steps > 0:
                raise YoloHipError("FlatSGD.load_state_dict: steps > 0 but the checkpoint holds no momentum buffer")
            return
        if self._built_for is not None:
            if mb.numel() != self.buf.numel():
                raise YoloHipError(f"FlatSGD: checkpointed momentum buffer has {mb.numel()} elements, the model {self.buf.numel()}")
            self.buf.copy_(mb)
        else:
            self._pending_buf = mb.detach().clone()


class FlatAdam(_FlatOptimizer):
    """torch.optim.Adam (no amsgrad, L2 weight decay) on the arena: the reference's optim.Adam(params, lr, betas=(momentum, 0.999))
    branch.  The groups carry no 'momentum' key, which is what makes the reference's warm-up leave the betas alone.  One beta pair
    and one eps serve the whole arena (group 0's, as FlatSGD reads group 0's momentum); lr and weight decay are per group."""

    def __init__(self, model, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(model)
        betas = (float(betas[0]), float(betas[1]))
        self.param_groups = [
            {"name": "bn_weight", "lr": lr, "initial_lr": lr, "betas": betas, "eps": eps, "weight_decay": 0.0},
            {"name": "weight", "lr": lr, "initial_lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay},
            {"name": "bias", "lr": lr, "initial_lr": lr, "betas": betas, "eps": eps, "weight_decay": 0.0},
        ]
        self._pending_m = self._pending_v = None     # moments loaded before the parameter arena exists (resume)

    def _build_state(self, n, dev):
        self.m = self._state_from_pending(self._pending_m, n, dev, "exp_avg")
        self.v = self._state_from_pending(self._pending_v, n, dev, "exp_avg_sq")
        self._pending_m = self._pending_v = None
        # the device block of yh_adam_step_dev (include/yolohip.h): lr[3] | wd[3] | beta1 | beta2 | eps written from here, the bias
        # corrections and the int64 step count behind them advanced by yh_adam_advance inside the step
        self.blk = torch.zeros(hipk.ADAM_BLK_FLOATS, dtype=torch.float32, device=dev)
        self._dev_steps = None          # the count the device block holds; None: unknown, write it

    def _sync_scalars(self):
        """device copy of lr / weight decay / betas / eps, rewritten only when a value changed (warm-up, per-epoch schedule); the
        device step count is rewritten only when it cannot be the host's `steps` (first use, a loaded checkpoint, a failed
        capture) — otherwise it follows on its own, one yh_adam_advance per step"""
        g0 = self.param_groups[0]
        vals = tuple(float(pg["lr"]) for pg in self.param_groups) + tuple(float(pg["weight_decay"]) for pg in self.param_groups) + \
            (float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"]))
        if vals != self._lr_host:
            self._push(self.blk[:hipk.ADAM_BLK_HOST], vals, "learning-rate / betas")
            self._lr_host = vals
        if self._dev_steps != self.steps:
            self._push(self.blk[hipk.ADAM_BLK_T:hipk.ADAM_BLK_T + 2].view(torch.int64), [int(self.steps)], "the step count")
            self._dev_steps = self.steps

    def _launch(self, pack, g, scale):
        hipk.adam_advance(self.blk)
        hipk.adam_step_dev(pack.flat, g, self.m, self.v, self.group, self.blk, scale)
        self._dev_steps = self.steps + 1

    def graph_pre_replay(self):
        super().graph_pre_replay()
        self._dev_steps = self.steps              # the replay's yh_adam_advance brings the device count there

    def graph_restore(self, snap):
        super().graph_restore(snap)
        self._dev_steps = None

    def state_dict(self):
        m, v = (self.m, self.v) if self._built_for is not None else (self._pending_m, self._pending_v)
        return {"exp_avg": m, "exp_avg_sq": v, "steps": self.steps, "param_groups": [dict(g) for g in self.param_groups]}

    def load_state_dict(self, sd):
        """like FlatSGD.load_state_dict: before the first forward the moments are kept and copied in when the arena is built"""
        m, v = sd.get("exp_avg"), sd.get("exp_avg_sq")
        if (m is None) != (v is None):
            raise YoloHipError("FlatAdam.load_state_dict: the checkpoint holds one of exp_avg / exp_avg_sq without the other")
        if m is None and sd["steps"] > 0:
            raise YoloHipError("FlatAdam.load_state_dict: steps > 0 but the checkpoint holds no moments (exp_avg, exp_avg_sq)")
        if m is not None and self._built_for is not None:
            for t, what in ((m, "exp_avg"), (v, "exp_avg_sq")):
                if t.numel() != self.m.numel():
                    raise YoloHipError(f"FlatAdam: checkpointed {what} has {t.numel()} elements, the model {self.m.numel()}")
        self.param_groups = [dict(g) for g in sd["param_groups"]]
        self.steps = sd["steps"]
        if m is None:
            return
        if self._built_for is not None:
            self.m.copy_(m)
            self.v.copy_(v)
        else:
            self._pending_m, self._pending_v = m.detach().clone(), v.detach().clone()
