"""Adam on the flat parameter arena (yh_adam_advance + yh_adam_step_dev, FlatAdam, optimizer: adam in the drivers) on the GPU.

The oracle throughout is torch.optim.Adam on the CPU in float64, fed the float32-rounded hyper-parameters and the same three
groups (tests/test_adam_host.py: adam_oracle).  The bar is the project's own for the SGD step, rtol 1e-5, atol 1e-6 on p, m and v:
a NumPy float32 restatement of the kernel's arithmetic, run against that oracle on every input used here, stayed at 0.053 of the
bar or below (p 0.028, m 0.053, v 0.014), so four times its error is still inside the bar and the bar was not widened
(the measurement and its test are in tests/test_adam_host.py)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from test_adam_host import (ATOL, DECAY, EPS, HUGE, LR, RTOL, TINY, WD, ZERO, _f32, adam_oracle, bar_fraction, clip_case, edge_case,
                            parity_case)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _close(got, ref, what):
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape
    err = (got - ref).abs()
    bad = ~(err <= ATOL + RTOL * ref.abs())
    print(f"{what}: largest error {bar_fraction(got, ref):.3f} of the bar")
    assert not bad.any(), f"{what}: max err {err.nan_to_num(nan=float('inf')).max().item():.4g}, {bad.sum().item()} of {err.numel()} out of tolerance"


def _block(dev, case, t=0):
    """the device block of yh_adam_step_dev as the host writes it: lr[3] | wd[3] | beta1 | beta2 | eps, and the step count"""
    from yoloseries_amd import hipk
    blk = torch.zeros(hipk.ADAM_BLK_FLOATS, device=dev)
    blk[:hipk.ADAM_BLK_HOST] = torch.tensor(list(case["lr"]) + list(case["wd"]) + [case["betas"][0], case["betas"][1], case["eps"]])
    blk[hipk.ADAM_BLK_T:hipk.ADAM_BLK_T + 2].view(torch.int64).fill_(t)
    return blk


def _views(dev, n, off, fill):
    """p, g, m, v as slices starting `off` elements into 16-byte aligned buffers whose margins hold `fill`"""
    full = [torch.full((n + 16,), fill, device=dev) for _ in range(4)]
    views = [f[4 + off:4 + off + n] for f in full]
    assert all(f.data_ptr() % 16 == 0 for f in full) and all(v.data_ptr() % 16 == 4 * (off % 4) for v in views)
    return full, views


def _run(dev, case, off=0, fill=1e6, check_every_step=None):
    """the case's steps through yh_adam_advance + yh_adam_step_dev (+ yh_sumsq / yh_clip_scale where it clips); compares p, m, v
    with the oracle after every step through `check_every_step(step, p, m, v, ref)`; returns the buffers and the clip scales"""
    from yoloseries_amd import hipk
    n = case["p"].numel()
    ref, norms = adam_oracle(case)
    full, (p, g, m, v) = _views(dev, n, off, fill)
    p.copy_(case["p"])
    m.zero_()
    v.zero_()
    group = None if case["group"] is None else case["group"].to(dev)
    blk = _block(dev, case)
    part, ss, gs = torch.zeros(4096, device=dev), torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    scales = []
    for step, grad in enumerate(case["grads"]):
        g.copy_(grad)
        if case["max_norm"] is not None:
            hipk.sumsq(g, part, ss)
            hipk.clip_scale(ss, case["max_norm"], gs)
            scales.append(gs.item())
        hipk.adam_advance(blk)
        hipk.adam_step_dev(p, g, m, v, group, blk, gs if case["max_norm"] is not None else None)
        check_every_step(step, p, m, v, ref[step])
    assert int(blk[hipk.ADAM_BLK_T:hipk.ADAM_BLK_T + 2].view(torch.int64).item()) == len(case["grads"])
    return full, (p, g, m, v), scales, norms


def _margins_hold(full, views, off, fill):
    n = views[0].numel()
    for f in full:
        for edge in (f[:4 + off], f[4 + off + n:]):
            assert bool(edge.isnan().all()) if math.isnan(fill) else bool((edge == fill).all()), "a margin element changed"


# ------------------------------------------------------------------------------------------------------------ 1. step parity
def _sizes():
    from yoloseries_amd import hipk
    return (1, 255, 4099, hipk.ADAM_GRID_PASS + 4099)


@pytest.mark.parametrize("which", range(4))
def test_step_parity(dev, which):
    """three steps, three groups with their own lr and weight decay, from zero moments; the largest size is one full grid pass of
    the launch plus 4099 elements, its first and second pass judged separately"""
    from yoloseries_amd import hipk
    n = _sizes()[which]
    case = parity_case(n)
    PASS = hipk.ADAM_GRID_PASS

    def check(step, p, m, v, ref):
        for name, got, want in zip(("p", "exp_avg", "exp_avg_sq"), (p, m, v), ref):
            _close(got[:PASS], want[:PASS], f"n={n} step {step + 1} {name} (first grid pass)")
            if n > PASS:
                _close(got[PASS:], want[PASS:], f"n={n} step {step + 1} {name} (elements of the second grid pass)")
    full, views, _, _ = _run(dev, case, check_every_step=check)
    _margins_hold(full, views, 0, 1e6)


# --------------------------------------------------------------------------------------------------------- 2. unaligned views
@pytest.mark.parametrize("fill", (1e6, NAN))
@pytest.mark.parametrize("off", (1, 2, 3))
def test_unaligned_views(dev, off, fill):
    """p, g, m and v each start `off` elements past a 16-byte boundary: the scalar head brings the 16-byte body into phase; the
    result matches the oracle and nothing in front of or behind any of the four views changed"""
    case = parity_case(4099, steps=2)

    def check(step, p, m, v, ref):
        for name, got, want in zip(("p", "exp_avg", "exp_avg_sq"), (p, m, v), ref):
            _close(got, want, f"offset {off} step {step + 1} {name}")
    full, views, _, _ = _run(dev, case, off=off, fill=fill, check_every_step=check)
    _margins_hold(full, views, off, fill)


def test_views_out_of_phase_take_the_scalar_loop(dev):
    """p, g, m, v at four different phases (0, 1, 2, 3 elements past a 16-byte boundary): no 16-byte access fits all four"""
    from yoloseries_amd import hipk
    case = parity_case(4099, steps=1)
    n = 4099
    ref, _ = adam_oracle(case)
    full = [torch.full((n + 16,), 1e6, device=dev) for _ in range(4)]
    p, g, m, v = (f[4 + k:4 + k + n] for k, f in enumerate(full))
    p.copy_(case["p"])
    g.copy_(case["grads"][0])
    m.zero_()
    v.zero_()
    blk = _block(dev, case)
    hipk.adam_advance(blk)
    hipk.adam_step_dev(p, g, m, v, case["group"].to(dev), blk)
    for name, got, want in zip(("p", "exp_avg", "exp_avg_sq"), (p, m, v), ref[0]):
        _close(got, want, f"out of phase {name}")
    for k, f in enumerate(full):
        assert bool((f[:4 + k] == 1e6).all()) and bool((f[4 + k + n:] == 1e6).all())


# -------------------------------------------------------------------------------------------------------------- 3. edge values
@pytest.mark.parametrize("with_group", (True, False))
def test_edge_values(dev, with_group):
    """zero gradients on p = 0 (everything stays exactly 0), weight decay alone on p != 0, gradients of 1e-20 and 1e4 in one
    launch, group bytes 3 and 255 reading group 2, and group == NULL reading group 0"""
    case = edge_case(with_group)
    p0 = case["p"]

    def check(step, p, m, v, ref):
        for name, got, want in zip(("p", "exp_avg", "exp_avg_sq"), (p, m, v), ref):
            assert not bool(got.isnan().any()), name
            _close(got, want, f"edge values step {step + 1} {name}")
        for t in (p, m, v):
            assert bool((t[ZERO] == 0).all()), "a zero gradient on a zero parameter must change nothing"
        assert bool((m[DECAY] != 0).all()) and bool((p[DECAY].cpu() != p0[DECAY]).all()), "weight decay on a non-zero parameter"
        assert bool((v[HUGE] > 1e4).all()) and bool((v[TINY] < 1e-30).all())
    _run(dev, case, check_every_step=check)
    if with_group:
        # bytes 3 and 255 did read group 2: the same elements with group 0's constants are out of tolerance
        other = dict(case, group=torch.where(case["group"] > 2, torch.zeros_like(case["group"]), case["group"]))
        a, b = adam_oracle(case)[0][0][0], adam_oracle(other)[0][0][0]
        assert bar_fraction(a, b) > 100


# ------------------------------------------------------------------------------------------------------------ 4. clipped tail
def test_clipped_adam_tail(dev):
    """yh_sumsq -> yh_clip_scale -> Adam with grad_scale against clip_grad_norm_ + torch.optim.Adam (float64): two steps, the first
    with a gradient norm of about 64 (clipped to 10), the second of about 0.6 (left alone)"""
    case = clip_case()

    def check(step, p, m, v, ref):
        for name, got, want in zip(("p", "exp_avg", "exp_avg_sq"), (p, m, v), ref):
            _close(got, want, f"clipped tail step {step + 1} {name}")
    _, _, scales, norms = _run(dev, case, check_every_step=check)
    assert 60 < norms[0] < 70 and 0.5 < norms[1] < 0.7, norms
    for s, total in zip(scales, norms):
        want = min(1.0, case["max_norm"] / (total + 1e-6))
        assert abs(s - want) <= 1e-6 * want
    assert scales[0] < 0.2 and scales[1] == 1.0, scales


# ---------------------------------------------------------------------------------------------------------- 5. device counter
def test_device_counter(dev):
    """yh_adam_advance from a count of 41 gives 42 and the bias corrections of step 42, evaluated in double from the float32 betas
    in the block; betas written to the block afterwards are what the next advance reads; nothing else in the block moves"""
    from yoloseries_amd import hipk
    case = dict(lr=LR, wd=WD, betas=(0.937, 0.999), eps=EPS)
    blk = _block(dev, case, t=41)
    before = blk.clone()
    hipk.adam_advance(blk)
    cnt = blk[hipk.ADAM_BLK_T:hipk.ADAM_BLK_T + 2].view(torch.int64)
    b1, b2 = _f32(0.937), _f32(0.999)
    assert int(cnt.item()) == 42
    assert abs(float(blk[hipk.ADAM_BLK_BC1]) - (1.0 - b1 ** 42)) <= 1e-7
    assert abs(float(blk[hipk.ADAM_BLK_SBC2]) - math.sqrt(1.0 - b2 ** 42)) <= 1e-7
    keep = [i for i in range(hipk.ADAM_BLK_FLOATS) if i not in (hipk.ADAM_BLK_BC1, hipk.ADAM_BLK_SBC2, hipk.ADAM_BLK_T, hipk.ADAM_BLK_T + 1)]
    assert torch.equal(blk[keep], before[keep])
    blk[6:8] = torch.tensor([0.8, 0.99], device=dev)
    hipk.adam_advance(blk)
    b1, b2 = _f32(0.8), _f32(0.99)
    assert int(cnt.item()) == 43
    assert abs(float(blk[hipk.ADAM_BLK_BC1]) - (1.0 - b1 ** 43)) <= 1e-7
    assert abs(float(blk[hipk.ADAM_BLK_SBC2]) - math.sqrt(1.0 - b2 ** 43)) <= 1e-7
    # n == 0 is a no-op (a zero-element torch view has no pointer to pass: the entry point is called as C sees it)
    from yoloseries_amd import _lib
    x = torch.full((8,), 3.0, device=dev)
    assert _lib.lib().yh_adam_step_dev(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 0, blk.data_ptr(), None, hipk._st()) == 0
    assert bool((x == 3.0).all())
    assert _lib.lib().yh_adam_step_dev(None, x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 8, blk.data_ptr(), None, hipk._st()) != 0


# ------------------------------------------------------------------------------------------------------------ 6. graph replay
def _setup(dev, graph):
    """the set-up of tests/test_gpu_graph.py::_setup (YOLOv5s, B = 4, 128 x 128) with FlatAdam(lr = 1e-3)"""
    import bench
    from yoloseries_amd import models
    from yoloseries_amd.loss import YOLOV5Loss
    from yoloseries_amd.trainer import ExponentialMovingAverageModel
    from yoloseries_amd.utils import FlatAdam, GraphedStep
    from yoloseries_amd.utils.synth import COCO_ANCHORS, synth_targets
    torch.manual_seed(0)
    B, img = 4, 128
    model = models.YOLOV5Small(3, 80).to(dev).train()
    lossf = YOLOV5Loss(torch.from_numpy(COCO_ANCHORS).to(dev), bench.make_hyp(dev, img, B))
    opt = FlatAdam(model, lr=1e-3)
    ema = ExponentialMovingAverageModel(model)
    x = torch.rand(B, 3, img, img, generator=torch.Generator().manual_seed(1)).to(dev)
    t = torch.from_numpy(synth_targets(B, img, 80, 12, seed=4, min_boxes=6)).to(dev)

    def step():
        out = lossf(model(x), t)
        out["tot_loss"].backward()
        opt.clip_grad_norm_(10.0)
        opt.step()
        opt.zero_grad()
        ema.update(model)
        return out
    stepper = GraphedStep(step, pre_replay=[opt.graph_pre_replay, ema.graph_pre_replay], warmup=2, enabled=graph)
    return model, opt, ema, stepper


def test_graph_replay_matches_eager_deterministic(dev, monkeypatch):
    """eight steps, the learning rate changed at step 5, eager against GraphedStep, with deterministic weight gradients (the
    workspace form, as in tests/test_gpu_graph.py): Adam divides by sqrt(v) and turns last-bit gradient noise into full-size steps
    where gradients are near zero, so the atomic form cannot be held to any useful bar.  Same mode, step counts and device blocks
    bit for bit; losses within 1e-3; parameters and EMA within the bars of the SGD test"""
    from yoloseries_amd import engine, hipk
    monkeypatch.setattr(engine.flags, "WG_WS_BYTES", 256 << 20)
    runs = {}
    for graph in (False, True):
        model, opt, ema, stepper = _setup(dev, graph)
        losses = []
        for it in range(8):
            if it == 5:
                for g in opt.param_groups:
                    g["lr"] = 5e-4
            losses.append(float(stepper()["tot_loss"].item()))
        torch.cuda.synchronize()
        assert stepper.mode == ("hipGraph replay" if graph else "eager"), stepper.failed
        flat = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu().numpy()
        eflat = torch.cat([p.detach().reshape(-1) for p in ema.ema.parameters()]).cpu().numpy()
        blk = opt.blk.cpu()
        assert int(blk[hipk.ADAM_BLK_T:hipk.ADAM_BLK_T + 2].view(torch.int64).item()) == opt.steps       # the host mirror follows the device
        np.testing.assert_allclose(blk[:3].numpy(), 5e-4, rtol=1e-6)                                      # the schedule change arrived
        assert abs(float(blk[hipk.ADAM_BLK_BC1]) - (1.0 - _f32(0.9) ** 8)) <= 1e-7
        assert float(opt.m.abs().sum()) > 0 and float(opt.v.sum()) > 0
        runs[graph] = (np.array(losses), flat, eflat, opt.steps, ema.update_num, blk.view(torch.int32).numpy())
    (l0, p0, e0, s0, u0, c0), (l1, p1, e1, s1, u1, c1) = runs[False], runs[True]
    assert s0 == s1 == 8 and u0 == u1 == 8
    np.testing.assert_array_equal(c0, c1)                       # device blocks, bit for bit
    assert np.isfinite(l0).all() and np.isfinite(l1).all()
    print("losses eager", l0, "replay", l1, "param diff", np.abs(p1 - p0).max() / np.abs(p0).max(), "ema diff", np.abs(e1 - e0).max() / np.abs(e0).max())
    np.testing.assert_allclose(l1, l0, rtol=1e-3)
    assert np.abs(p1 - p0).max() <= 1e-3 * np.abs(p0).max()
    assert np.abs(e1 - e0).max() <= 1e-4 * np.abs(e0).max() + 1e-7


def test_scalars_changed_inside_a_capture_raise(dev, monkeypatch):
    """like FlatSGD: a learning rate (or a step count) that the device block does not hold yet cannot be pushed while the stream
    is capturing (the capture is simulated: what matters is that nothing is copied and the block stays as it was)"""
    from yoloseries_amd._lib import YoloHipError
    model, opt, ema, stepper = _setup(dev, False)
    stepper()
    torch.cuda.synchronize()
    before = opt.blk.clone()
    opt.param_groups[0]["lr"] = 7e-4
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(YoloHipError, match="learning-rate / betas changed inside a graph capture"):
            opt._sync_scalars()
        opt.param_groups[0]["lr"] = 1e-3
        opt.steps += 1
        with pytest.raises(YoloHipError, match="step count changed inside a graph capture"):
            opt._sync_scalars()
        opt.steps -= 1
    assert torch.equal(opt.blk, before)
    opt.param_groups[0]["lr"] = 7e-4
    opt._sync_scalars()                             # outside a capture it goes through
    assert abs(float(opt.blk[0]) - 7e-4) <= 1e-9 and torch.equal(opt.blk[1:], before[1:])


# ------------------------------------------------------------------------------------------------------------------ 7. driver
def test_training_driver_with_adam(dev, tmp_path, monkeypatch):
    """train_yolov5.py --optimizer adam: warm-up (lr only, the betas stay), Adam, EMA, checkpoint with optim_type 'adam', resume into
    Adam (state restored) and into SGD (weights only, as the reference does when the types differ)"""
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    import train_yolov5
    from yoloseries_amd.utils import FlatAdam, FlatSGD
    seen = []
    warmup = train_yolov5.Training.warmup

    def recording_warmup(self, step_in_total):
        warmup(self, step_in_total)
        seen.append((step_in_total, [dict(g) for g in self.optimizer.param_groups]))
    monkeypatch.setattr(train_yolov5.Training, "warmup", recording_warmup)
    t = train_yolov5.main(["--epochs", "2", "--img", "128", "--batch", "4", "--steps-per-epoch", "4", "--optimizer", "adam"])
    monkeypatch.setattr(train_yolov5.Training, "warmup", warmup)
    assert isinstance(t.optimizer, FlatAdam) and t.hyp["optimizer"] == "adam"
    losses = [h["tot_loss"] for h in t.history]
    assert len(losses) == 8 and all(np.isfinite(losses)), losses
    # the warm-up moved the learning rates and nothing else
    hyp = t.hyp
    W = hyp["warmup_steps"]
    assert len(seen) == 8 and [s for s, _ in seen] == list(range(1, 9)) and 2 <= W <= 8
    for step, groups in seen:
        for j, g in enumerate(groups):
            assert "momentum" not in g and g["betas"] == (hyp["momentum"], 0.999) and g["eps"] == 1e-8
            if step < W:                             # group 2 (biases) comes down from warmup_bias_max_lr, the others up from 0
                lo = hyp["warmup_bias_max_lr"] if j == 2 else 0.0
                assert g["lr"] == pytest.approx(np.interp(step, [0., W], [lo, g["initial_lr"]]))
    first = seen[0][1]
    assert hyp["warmup_bias_max_lr"] > first[2]["lr"] > first[2]["initial_lr"] > first[0]["lr"] == first[1]["lr"] > 0
    ck = torch.load(t.last_ckpt, map_location="cpu", weights_only=False)
    assert ck["optim_type"] == "adam"
    sd = ck["optim_state_dict"]
    assert set(sd) == {"exp_avg", "exp_avg_sq", "steps", "param_groups"} and sd["steps"] == 8
    assert float(sd["exp_avg"].abs().sum()) > 0 and float(sd["exp_avg_sq"].sum()) > 0 and bool((sd["exp_avg_sq"] >= 0).all())
    # resume with Adam: step count at once, both moments once the first forward has built the arena
    t2 = train_yolov5.Training(t.anchors, dict(t.hyp, pretrained_model_path=t.last_ckpt, total_epoch=2))
    assert isinstance(t2.optimizer, FlatAdam) and t2.start_epoch == 2 and t2.optimizer.steps == 8
    for (k, a), (_, b) in zip(t.model.state_dict().items(), t2.model.state_dict().items()):
        assert torch.equal(a.cpu(), b.cpu()), k
    t2.model.train()
    t2.model(torch.rand(4, 3, 128, 128, device=dev))
    t2.optimizer._pack()
    assert torch.equal(t2.optimizer.m.cpu(), sd["exp_avg"]) and torch.equal(t2.optimizer.v.cpu(), sd["exp_avg_sq"])
    # resume with SGD: the weights, and a fresh optimizer
    t3 = train_yolov5.Training(t.anchors, dict(t.hyp, optimizer="sgd", pretrained_model_path=t.last_ckpt, total_epoch=2))
    assert isinstance(t3.optimizer, FlatSGD) and t3.optimizer.steps == 0 and t3.optimizer._pending_buf is None
    for (k, a), (_, b) in zip(t.model.state_dict().items(), t3.model.state_dict().items()):
        assert torch.equal(a.cpu(), b.cpu()), k
    t3.model.train()
    t3.model(torch.rand(4, 3, 128, 128, device=dev))
    t3.optimizer._pack()
    assert not bool(t3.optimizer.buf.any())
    # ... and the other way round: an SGD checkpoint resumed with Adam
    t3.save_model(2, filename="from_sgd")
    t4 = train_yolov5.Training(t.anchors, dict(t.hyp, optimizer="adam", pretrained_model_path=t3.last_ckpt, total_epoch=2))
    assert isinstance(t4.optimizer, FlatAdam) and t4.optimizer.steps == 0 and t4.optimizer._pending_m is None
    for (k, a), (_, b) in zip(t3.model.state_dict().items(), t4.model.state_dict().items()):      # t3's forward moved its BN statistics
        assert torch.equal(a.cpu(), b.cpu()), k


def test_yolox_training_driver_with_adam(dev, tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    monkeypatch.chdir(tmp_path)
    import train_yolox
    from yoloseries_amd.utils import FlatAdam
    t = train_yolox.main(["--epochs", "2", "--img", "128", "--batch", "4", "--steps-per-epoch", "4", "--optimizer", "adam"])
    assert isinstance(t.optimizer, FlatAdam)
    losses = [h["tot_loss"] for h in t.history]
    assert len(losses) == 8 and all(np.isfinite(losses)), losses
