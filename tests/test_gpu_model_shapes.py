"""The whole network OFF THE SQUARE: H != W, a deepest map that is odd or smaller than the 5 x 5 pool window, batch 1 and an odd
batch — through Builder, Program and the backward engine — against the reference's own classes (fp32 on the CPU, recorded by
tools/gen_golden.py::gen_g18 into g18_shapes.npz / g18_shapes_b.npz).  Every other whole-network test runs a square input, where a
swapped (H, W) pair in a descriptor, a join or a head view is invisible, and where the kernel choices that follow the map — halo
tile geometry, the parity-class data gradient (even Ho, Wo), the stem's Wo % 32, the pixel-count conditions of the weight-gradient
forms, the fused SPPF kernel — never flip.

  key            model     B x H x W      maps at stride 8 / 16 / 32
  v5s_96x160     YOLOv5s   3 x  96 x 160  12 x 20,  6 x 10, 3 x 5    odd batch, deepest map smaller than the pool window, H != W
  v5s_224x288    YOLOv5s   1 x 224 x 288  28 x 36, 14 x 18, 7 x 9    batch 1, odd deepest map
  v5s_416        YOLOv5s   2 x 416 x 416  52, 26, 13                 the classic 416 size
  v5m_96x160     YOLOv5m   3 x  96 x 160                             48 / 96 / 192-channel layers
  v5x_224x288    YOLOv5x   1 x 224 x 288                             80 / 160 / 320 / 640-channel kernel families
  yolox_96x160   YOLOXs    3 x  96 x 160                             stacked head GEMM on non-square maps

Each case runs on fresh models (a program is built at first use) under three plans: as this box tunes it; with YH_CONV_TUNE=0 /
YH_WGRAD_TUNE=0 — the library-default plan, identical on every box; and with the last candidate of the tuner's own list for
every launch (`_plan`) — the specialised families, identical on every box too.  The kernels each program resolved to are printed,
not asserted.  The bars are those of tests/test_gpu_model.py (test_full_graph_gradients_eval_mode_bn, test_model_mlx_forward_golden);
the generator asserted that the reference's own bf16-autocast run stays inside them at these shapes.
"""
import collections
import os

import numpy as np
import pytest
import torch

from test_gpu_model import G, _close, _frozen_bn_gradients, fill_state

pytestmark = pytest.mark.gpu

_V5 = lambda o: list(o)                         # noqa: E731
_X = lambda o: list(o.values())                 # noqa: E731
CASES = {  # key: (fixture, model class, constructor arguments, heads of the model's output, (batch, H, W))
    "v5s_96x160": ("g18_shapes.npz", "YOLOV5Small", (3, 80), _V5, (3, 96, 160)),
    "v5s_224x288": ("g18_shapes.npz", "YOLOV5Small", (3, 80), _V5, (1, 224, 288)),
    "v5s_416": ("g18_shapes.npz", "YOLOV5Small", (3, 80), _V5, (2, 416, 416)),
    "v5m_96x160": ("g18_shapes_b.npz", "YOLOV5Middle", (3, 80), _V5, (3, 96, 160)),
    "v5x_224x288": ("g18_shapes_b.npz", "YOLOV5XLarge", (3, 80), _V5, (1, 224, 288)),
    "yolox_96x160": ("g18_shapes_b.npz", "YOLOXSmall", (1, 3, 80, 0.01), _X, (3, 96, 160)),
}
KEYS = list(CASES)
PLANS = ["tuned", "default", "last"]
NC, ANCHORS_V5 = 80, 3
# Norm bars wider than the rule (max(2e-2, 1.5 cal_n)), per key and NAMED parameter, after the v5l line of _frozen_bn_gradients.
# v5s_96x160, first conv of the bottleneck on the 3 x 5 map (256 -> 256, 1x1: 45 pixels per weight-gradient sum, the smallest
# gradient norm of the net, 0.10).  This gradient is ill-conditioned in bf16 whoever computes it:
#   * the reference's OWN bf16-autocast gradient is, against its fp32 one, a projection of 0.9845 plus a residual of 15.7 % of
#     the norm — -1.55 % and +1.2 % on the norm, which happen to cancel to the recorded cal_n = 0.31 %; its cal_e, 5.2 %, is the
#     largest of any conv weight in the fixture;
#   * the HIP path measures projection 0.972 / residual 14.2 % / norm -1.77 % under the default and the tuned plan and
#     0.968 / 15.3 % / -2.01 % under the last-candidate plan, and the whole difference between the plans comes from twelve forward
#     layers on conv_p3_kernel instead of conv_v2_kernel: 25 of their ~700 000 output values differ, by one bf16 step, both kernels
#     within 0.5 steps of an fp64 convolution of the same operands — and that moves this gradient by 6.7 % of its norm.
# Which kernels the tuned plan takes is decided by timing on each box, so the bar has to hold for every candidate: 2.5e-2, the
# floor of the v5l line.
NORM_BAR = {"v5s_96x160": {"backbone_stage4_bscp.blocks.0.conv_bn_act_1.conv.weight": 2.5e-2}}


def _case(key):
    """(fixture arrays, make, outs_of, input seed, input shape): seed and shape as the fixture recorded them"""
    from yoloseries_amd import models
    fixture, cls, args, outs_of, bhw = CASES[key]
    g = np.load(os.path.join(G, fixture))
    xshape = tuple(int(v) for v in g[f"{key}_xshape"])
    assert xshape == (bhw[0], 3, bhw[1], bhw[2])
    return g, fixture, (lambda: getattr(models, cls)(*args)), outs_of, int(g[f"{key}_xseed"][0]), xshape


def _plan(monkeypatch, plan):
    """How the programs built in this test choose their kernels (decided when a program is built).
    'tuned': as this box times them.  'default': no timing, the library's own choice for every launch.  'last': no timing either —
    every conv, data-gradient and weight-gradient launch takes the LAST of the candidates the tuner would have timed for it
    (_conv_candidates / _wgrad_candidates list the generic kernel first and the families added later — the specialised ones —
    last).  Any candidate can win the timing on some box, so each must be right; this plan runs the same ones on every box."""
    if plan == "default":
        monkeypatch.setenv("YH_CONV_TUNE", "0")
        monkeypatch.setenv("YH_WGRAD_TUNE", "0")
    elif plan == "last":
        import ctypes as C
        from yoloseries_amd.engine.tune import TunerMixin

        def last_conv(self, d, kind, name, stats_ok=False):
            d.algo, d.tile_k, d.grid_cap = self._conv_candidates(self.L, d, kind)[-1]

        def last_wgrad(self, wd, M, ntile, op):
            for tk, sps in reversed(self._wgrad_candidates(self.L, wd, M, ntile)):
                for sp in sps:
                    wd.tile_k, wd.splits = tk, sp
                    if not wd.partial or self.L.yh_conv_wgrad_ws_bytes(C.byref(wd)) <= wd.partial_bytes:
                        return sp
            raise AssertionError(f"no weight-gradient candidate for {op.name}")
        monkeypatch.setattr(TunerMixin, "_tune_conv", last_conv)
        monkeypatch.setattr(TunerMixin, "_tune_wgrad_splits", last_wgrad)


def _head_shapes(key, xshape):
    B, _, H, W = xshape
    if key.startswith("yolox"):
        return [(B, 1, 5 + NC, H // s, W // s) for s in (8, 16, 32)]
    return [(B, ANCHORS_V5 * (5 + NC), H // s, W // s) for s in (8, 16, 32)]


def _print_kernels(model, key, plan):
    """the kernels every command list of the model's programs resolved to: makes a failing log show what ran"""
    def walk(cmds, into):
        for c in cmds or ():
            if c[-1][0] != 'sync':
                into[c[-1][0].split('<')[0]] += 1
    for shape, prog in model._yh_state()['progs'].items():
        for what in ("cmd_eval", "cmd_train", "cmd_frozen", "cmd_bwd"):
            names = collections.Counter()
            walk(getattr(prog, what, None), names)
            if names:
                print(f"{key} [{plan}] {shape} {what}: " + ", ".join(f"{n} x{c}" for n, c in sorted(names.items())))


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("key", KEYS)
def test_frozen_bn_gradients_off_square(dev, monkeypatch, key, plan):
    """test_full_graph_gradients_eval_mode_bn's check, unchanged, at the g18 shapes: output samples within 3e-2; every parameter's
    64 sampled gradient elements and its gradient norm within the project's bars (conv weights max(3e-2, 1.5 cal) / max(2e-2,
    1.5 cal), BatchNorm affine max(8e-2, 2 cal) / max(5e-2, 2 cal); one named exception: NORM_BAR); both backward schedules;
    running statistics bit-unchanged"""
    _plan(monkeypatch, plan)
    g, fixture, make, outs_of, xseed, xshape = _case(key)
    assert [tuple(g[f"{key}_out_shape{i}"]) for i in range(3)] == _head_shapes(key, xshape)
    made = []
    try:
        _frozen_bn_gradients(dev, fixture, key, lambda: made.append(make()) or made[-1], xseed, xshape, outs_of,
                             norm_bar=NORM_BAR.get(key))
    finally:
        for model in made:
            _print_kernels(model, key, plan)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("key", KEYS)
def test_inference_program_off_square(dev, monkeypatch, key, plan):
    """eval() under torch.no_grad(): the inference program (BatchNorm folded into the conv epilogue, the in-place concat plan, the
    inference-only kernels where the tuner takes them) gives heads of the right shapes and the same output samples within 3e-2"""
    _plan(monkeypatch, plan)
    g, _, make, outs_of, xseed, xshape = _case(key)
    model = make()
    fill_state(model, int(g[f"{key}_seed"][0]))
    model = model.to(dev).eval()
    x = torch.from_numpy(np.random.RandomState(xseed).rand(*xshape).astype(np.float32)).to(dev)
    with torch.no_grad():
        outs = outs_of(model(x))
    prog = model._yh_program(xshape[0], xshape[2], xshape[3])
    assert prog.cmd_train is None, "torch.no_grad() in eval() must run the inference program"
    _print_kernels(model, key, plan)
    assert [tuple(o.shape) for o in outs] == _head_shapes(key, xshape)
    for i, o in enumerate(outs):
        flat = o.float().contiguous().cpu().numpy().reshape(-1)
        _close(flat[g[f"{key}_out_idx{i}"]], g[f"{key}_out_val{i}"], 3e-2, f"{key} [{plan}] inference out{i}")


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("key", [k for k in KEYS if k.startswith("v5s_")])
def test_training_forward_off_square(dev, monkeypatch, key, plan):
    """one train() forward on the seeded default init: running statistics of four layers (stem to the last C3 of the head) at the
    bars of test_model_mlx_forward_golden, exactly one more batch tracked, finite heads of the right shapes"""
    _plan(monkeypatch, plan)
    g, _, make, outs_of, xseed, xshape = _case(key)
    torch.manual_seed(0)
    model = make().to(dev).train()
    x = torch.from_numpy(np.random.RandomState(xseed).rand(*xshape).astype(np.float32)).to(dev)
    probes = (("focus", 2e-2), ("backbone_stage2_conv", 2e-2), ("backbone_stage4_conv", 3e-2), ("head_stage4_bscp.cba3", 6e-2))
    mods = dict(model.named_modules())
    # (the constructor leaves every BatchNorm at one tracked batch, as the reference's does with its dummy forward: _init_bias)
    assert all(int(mods[pn].bn.num_batches_tracked) == 1 for pn, _ in probes)
    outs = [o.detach() for o in outs_of(model(x))]
    _print_kernels(model, key, plan)
    assert [tuple(o.shape) for o in outs] == _head_shapes(key, xshape) == [tuple(g[f"{key}_train_shape{i}"]) for i in range(3)]
    for o in outs:
        assert torch.isfinite(o.float()).all()
    for pn, tol in probes:
        bn = mods[pn].bn
        assert int(bn.num_batches_tracked) == 1 + 1 == int(g[f"{key}_nbt_{pn}"][0]), pn      # exactly one more batch, as the reference counts
        _close(bn.running_mean.cpu().numpy(), g[f"{key}_rm_{pn}"], tol, f"{key} [{plan}] {pn} running_mean", outlier_frac=0.01)
        _close(bn.running_var.cpu().numpy(), g[f"{key}_rv_{pn}"], tol, f"{key} [{plan}] {pn} running_var", outlier_frac=0.01)
