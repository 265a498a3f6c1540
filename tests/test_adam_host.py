"""Adam on the flat parameter arena, the parts that need no GPU: the two entry points (yh_adam_advance, yh_adam_step_dev) are
declared, exported and bound; FlatAdam's groups and state dict on a CPU-constructed model; and the inputs, the float64 oracle
(torch.optim.Adam on the CPU) and the tolerance that tests/test_gpu_adam.py holds the kernel to.

The tolerance.  The project's bar for the SGD step is rtol 1e-5, atol 1e-6 on every output.  Adam adds a square root and a division,
so before that bar was taken over, adam_restate_f32() below — the kernel's arithmetic restated in NumPy float32, operation by
operation — was run against the float64 oracle on every input of the GPU tests (step parity at n = 1, 255, 4099 and one grid pass
+ 4099, the edge values with and without a group map, the clipped tail).  Its largest error, as a fraction of the bar
atol + rtol * |ref|, was 0.053 (on m, at the largest size; p 0.028, v 0.014): float32 arithmetic in this order sits about twenty
times inside the bar, and four times that error (the allowance for an operation order that differs between restatement and kernel)
is still inside it.  So the bar stays rtol 1e-5, atol 1e-6 on p, m and v.  test_float32_restatement_is_inside_the_bar repeats the
measurement (without the largest size: 0.024 on m) and asserts that four times the restatement's error stays inside the bar."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-5, 1e-6
LR, WD, BETAS, EPS = [0.01, 0.002, 0.05], [1e-3, 5e-4, 1e-2], (0.9, 0.999), 1e-8


def _f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------- inputs shared with the GPU tests
def parity_case(n, steps=3):
    """three steps from zero moments, three groups interleaved"""
    g = torch.Generator().manual_seed(100 + n % 1000)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(steps)]
    return dict(p=p, grads=grads, group=(torch.arange(n) % 3).to(torch.uint8), lr=LR, wd=WD, betas=BETAS, eps=EPS, max_norm=None)


ZERO, DECAY, TINY, HUGE = slice(0, 256), slice(256, 512), slice(512, 768), slice(768, 1024)


def edge_case(with_group):
    """two steps over: ZERO — gradient 0 on p = 0 (m = v = 0, no update, no NaN); DECAY — gradient 0 on p != 0 (weight decay is
    the whole gradient); TINY / HUGE — gradients of 1e-20 (on p = 0) and 1e4 in the same launch; group bytes 3 and 255 (read group 2)"""
    n = 4099
    g = torch.Generator().manual_seed(7)
    p = torch.randn(n, generator=g) + 0.5
    p[ZERO] = 0.0
    p[TINY] = 0.0                                    # no weight-decay term on top of the 1e-20
    grads = []
    for _ in range(2):
        gr = torch.randn(n, generator=g)
        sign = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0)
        gr[ZERO] = 0.0
        gr[DECAY] = 0.0
        gr[TINY] = 1e-20 * sign[TINY]
        gr[HUGE] = 1e4 * sign[HUGE]
        grads.append(gr)
    group = torch.tensor([0, 1, 2, 3, 255], dtype=torch.uint8).repeat(n // 5 + 1)[:n] if with_group else None
    return dict(p=p, grads=grads, group=group, lr=LR, wd=WD, betas=BETAS, eps=EPS, max_norm=None)


def clip_case():
    """two steps: a gradient norm of about 64, clipped to 10, then one of about 0.6, left alone"""
    n = 4099
    g = torch.Generator().manual_seed(6)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * mag for mag in (1.0, 0.01)]
    return dict(p=p, grads=grads, group=(torch.arange(n) % 3).to(torch.uint8), lr=LR, wd=WD, betas=BETAS, eps=EPS, max_norm=10.0)


def group_index(case):
    """the group each element reads: NULL map = group 0, bytes above 2 = group 2"""
    n = case["p"].numel()
    return torch.zeros(n, dtype=torch.long) if case["group"] is None else case["group"].long().clamp(max=2)


def adam_oracle(case):
    """torch.optim.Adam (and clip_grad_norm_) on the CPU in float64, fed the float32-rounded hyper-parameters and the three groups;
    returns (p, exp_avg, exp_avg_sq) after every step and the total norms clip_grad_norm_ saw"""
    gi, n = group_index(case), case["p"].numel()
    idx = {k: torch.nonzero(gi == k).reshape(-1) for k in range(3)}
    idx = {k: i for k, i in idx.items() if i.numel()}
    ref = {k: case["p"][i].double().clone().requires_grad_(True) for k, i in idx.items()}
    opt = torch.optim.Adam([{"params": [ref[k]], "lr": _f32(case["lr"][k]), "weight_decay": _f32(case["wd"][k])} for k in ref],
                           lr=1e-3, betas=(_f32(case["betas"][0]), _f32(case["betas"][1])), eps=_f32(case["eps"]))
    out, norms = [], []
    for g in case["grads"]:
        for k, i in idx.items():
            ref[k].grad = g[i].double()
        if case["max_norm"] is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(list(ref.values()), case["max_norm"])))
        opt.step()
        P, M, V = (torch.empty(n, dtype=torch.float64) for _ in range(3))
        for k, i in idx.items():
            P[i], M[i], V[i] = ref[k].detach(), opt.state[ref[k]]["exp_avg"], opt.state[ref[k]]["exp_avg_sq"]
        out.append((P, M, V))
    return out, norms


def adam_restate_f32(case):
    """the arithmetic of adam_dev_kernel / adam_advance_kernel (csrc/arena.hip) in NumPy float32, in the kernel's operation order"""
    f = np.float32
    gi = group_index(case).numpy()
    p = case["p"].numpy().astype(f)
    m, v = np.zeros_like(p), np.zeros_like(p)
    lr, wd = np.array(case["lr"], f), np.array(case["wd"], f)
    b1, b2, eps = f(case["betas"][0]), f(case["betas"][1]), f(case["eps"])
    omb1, omb2 = f(1.0 - float(b1)), f(1.0 - float(b2))
    out = []
    for t, g in enumerate(case["grads"], 1):
        g = g.numpy().astype(f)
        gs = f(1.0)
        if case["max_norm"] is not None:
            ss = f((g.astype(np.float64) ** 2).sum())
            gs = min(f(case["max_norm"]) / (np.sqrt(ss) + f(1e-6)), f(1.0))
        bc1, sbc2 = f(1.0 - float(b1) ** t), f(math.sqrt(1.0 - float(b2) ** t))
        step = (lr / bc1)[gi]
        gv = g * gs + wd[gi] * p
        m = m + omb1 * (gv - m)
        v = b2 * v + omb2 * gv * gv
        denom = np.sqrt(v) / sbc2 + eps
        p = p - step * (m / denom)
        assert p.dtype == m.dtype == v.dtype == f
        out.append((torch.from_numpy(p.copy()), torch.from_numpy(m.copy()), torch.from_numpy(v.copy())))
    return out


def bar_fraction(got, ref):
    """largest error of `got` as a fraction of the bar ATOL + RTOL * |ref| (<= 1: inside); inf for a NaN"""
    got, ref = got.double().cpu(), ref.double().cpu()
    frac = (got - ref).abs() / (ATOL + RTOL * ref.abs())
    return float(frac.nan_to_num(nan=float("inf")).max())


# ------------------------------------------------------------------------------------------------------------------ the bar
def test_float32_restatement_is_inside_the_bar():
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for case in [parity_case(n) for n in (1, 255, 4099)] + [edge_case(True), edge_case(False), clip_case()]:
        ref, _ = adam_oracle(case)
        for got_t, ref_t in zip(adam_restate_f32(case), ref):
            for name, a, b in zip("pmv", got_t, ref_t):
                worst[name] = max(worst[name], bar_fraction(a, b))
    print("float32 restatement, largest error / (atol + rtol |ref|):", worst)
    assert 4 * max(worst.values()) <= 1.0, worst      # measured: p 0.018, m 0.024, v 0.014


# ------------------------------------------------------------------------------------------------------- the entry points
@pytest.mark.parametrize("name,nargs", [("yh_adam_advance", 2), ("yh_adam_step_dev", 9)])
def test_adam_entry_points_are_declared_exported_and_bound(name, nargs):
    import ctypes as C
    from yoloseries_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "yolohip.h")).read()
    proto = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert proto, f"include/yolohip.h does not declare {name}"
    assert name in _lib.EXPORTED_SYMBOLS
    res, args = _lib._SIGS[name]
    assert res is C.c_int32 and len(args) == len(re.sub(r"/\*.*?\*/", "", proto.group(1)).split(",")) == nargs
    assert hasattr(C.CDLL(_lib.LIB_PATH), name), f"{name} is not exported by the built library"
    assert getattr(_lib.lib(), name).argtypes == args


def test_grid_pass_constant_follows_the_launch_code():
    """hipk.ADAM_GRID_PASS (the size the GPU parity test goes past) is what yh_adam_step_dev launches"""
    from yoloseries_amd import hipk
    src = open(os.path.join(ROOT, "yoloseries_amd", "csrc", "arena.hip")).read()
    th, blocks, unroll = (int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("TH", "ADAM_BLOCKS", "ADAM_UNROLL"))
    assert hipk.ADAM_GRID_PASS == blocks * th * 4 * unroll
    assert hipk.ADAM_BLK_FLOATS == 16 and hipk.ADAM_BLK_T % 2 == 0 and hipk.ADAM_BLK_HOST <= hipk.ADAM_BLK_BC1 < hipk.ADAM_BLK_SBC2 < hipk.ADAM_BLK_T


# -------------------------------------------------------------------------------------------------------------- FlatAdam
@pytest.fixture(scope="module")
def small():
    from yoloseries_amd import models
    torch.manual_seed(0)
    return models.YOLOV5Small(3, 80)


def test_flat_adam_groups(small):
    from yoloseries_amd.utils import FlatAdam
    opt = FlatAdam(small, lr=1e-3, betas=(0.937, 0.999), weight_decay=5e-4)
    assert [g["name"] for g in opt.param_groups] == ["bn_weight", "weight", "bias"]
    for g in opt.param_groups:
        assert "momentum" not in g                   # what makes the reference's warm-up leave Adam's groups alone
        assert g["lr"] == g["initial_lr"] == 1e-3 and g["betas"] == (0.937, 0.999) and g["eps"] == 1e-8
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 5e-4, 0.0]
    assert small.flat_grads_only and small._yh_grad_hook_opt == opt._on_grad
    d = FlatAdam(small, lr=1e-3).param_groups[1]
    assert d["betas"] == (0.9, 0.999) and d["weight_decay"] == 0.0


def test_flat_adam_state_dict_before_the_first_forward(small):
    from yoloseries_amd._lib import YoloHipError
    from yoloseries_amd.utils import FlatAdam
    n = sum(p.numel() for p in small.parameters())
    opt = FlatAdam(small, lr=1e-3)
    sd = opt.state_dict()
    assert set(sd) == {"exp_avg", "exp_avg_sq", "steps", "param_groups"}
    assert sd["exp_avg"] is None and sd["exp_avg_sq"] is None and sd["steps"] == 0
    g = torch.Generator().manual_seed(1)
    m, v = torch.randn(n, generator=g), torch.rand(n, generator=g)
    groups = [dict(pg, lr=3e-4) for pg in sd["param_groups"]]
    opt.load_state_dict({"exp_avg": m, "exp_avg_sq": v, "steps": 17, "param_groups": groups})
    m_in, v_in = m.clone(), v.clone()
    m.zero_()                                        # the pending copies are the optimizer's own
    back = opt.state_dict()
    assert back["steps"] == opt.steps == 17 and back["param_groups"][0]["lr"] == 3e-4
    assert torch.equal(back["exp_avg"], m_in) and torch.equal(back["exp_avg_sq"], v_in)
    fresh = FlatAdam(small, lr=1e-3)
    fresh.load_state_dict(back)                      # round trip
    assert torch.equal(fresh.state_dict()["exp_avg"], m_in) and fresh.steps == 17
    with pytest.raises(YoloHipError, match="steps > 0"):
        FlatAdam(small, lr=1e-3).load_state_dict({"exp_avg": None, "exp_avg_sq": None, "steps": 3, "param_groups": groups})
    with pytest.raises(YoloHipError):
        FlatAdam(small, lr=1e-3).load_state_dict({"exp_avg": m_in, "exp_avg_sq": None, "steps": 3, "param_groups": groups})
    zero = FlatAdam(small, lr=1e-3)
    zero.load_state_dict({"exp_avg": None, "exp_avg_sq": None, "steps": 0, "param_groups": groups})
    assert zero.steps == 0 and zero.state_dict()["exp_avg"] is None
    with pytest.raises(YoloHipError, match="forward pass first"):
        opt.step()


def test_flat_sgd_keeps_its_surface(small):
    """the shared base moved no name FlatSGD's users read"""
    from yoloseries_amd.utils import FlatSGD
    opt = FlatSGD(small, lr=0.01)
    assert all("momentum" in g for g in opt.param_groups)
    assert set(opt.state_dict()) == {"momentum_buffer", "steps", "param_groups"}
    for name in ("_pack", "_on_grad", "replace_accumulated", "clip_grad_norm_", "step", "zero_grad", "graph_pre_replay", "graph_pre_capture",
                 "graph_snapshot", "graph_restore", "load_state_dict"):
        assert callable(getattr(opt, name))


def test_driver_rejects_an_unknown_optimizer():
    """_init_optimizer names the two choices (the reference's RuntimeError there is a bare expression and raises nothing)"""
    import train_yolov5

    class T(train_yolov5.Training):
        def __init__(self, hyp):
            self.hyp, self.model = hyp, None
    with pytest.raises(ValueError, match="'sgd' and 'adam'"):
        T({"optimizer": "rmsprop", "lr": 0.01, "momentum": 0.9, "weight_decay": 0.0})._init_optimizer()
