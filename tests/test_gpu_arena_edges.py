"""Edges of the kernels in csrc/arena.hip: launches past one grid pass (4096 blocks of 256 threads), the scalar paths of the
vectorised gathers, bf16 rounding of yh_pack_bf16, and the gradient-clipping tail of the train step
(yh_sumsq -> yh_clip_scale -> yh_sgd_step / yh_sgd_step_dev with grad_scale).

References are plain torch in float64 on the same fp32 inputs; the optimizer bar is the project's (rtol 1e-5, atol 1e-6)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PASS = 4096 * 256                # threads of one grid pass
NAN = float("nan")
_RAN = set()


def _close(got, ref, rtol, atol, what):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape
    err = (got - ref).abs()
    bad = ~(err <= atol + rtol * ref.abs())
    assert not bad.any(), f"{what}: max err {err.nan_to_num(nan=float('inf')).max().item():.4g}, {bad.sum().item()} of {err.numel()} out of tolerance"


def _close_passes(got, ref, rtol, atol, what):
    _close(got[:PASS], ref[:PASS], rtol, atol, what + " (first grid pass)")
    _close(got[PASS:], ref[PASS:], rtol, atol, what + " (elements of the second grid pass)")


def _gather_ref(src, idx):
    return torch.where(idx >= 0, src[idx.clamp(min=0).long()], torch.zeros((), device=src.device))


# ---------------------------------------------------------------- gathers
def test_pack_and_gather_beyond_one_grid_pass(dev):
    """the second iteration of the 8-wide / 4-wide loops and the scalar tail behind it; guard elements on both sides stay"""
    from yoloseries_amd import hipk
    _RAN.add("gather_pass")
    g = torch.Generator(device=dev).manual_seed(1)
    src = torch.randn(1 << 20, generator=g, device=dev)
    n = 8 * PASS + 8 * 5 + 3
    idx = torch.randint(-1, src.numel(), (n,), generator=g, dtype=torch.int32, device=dev)
    full = torch.full((n + 16,), 7.0, dtype=torch.bfloat16, device=dev)
    hipk.pack_bf16(src, idx, full[8:8 + n])
    ref = _gather_ref(src, idx).to(torch.bfloat16)
    dst = full[8:8 + n]
    assert torch.equal(dst[:8 * PASS], ref[:8 * PASS]), "pack_bf16 (first grid pass)"
    assert torch.equal(dst[8 * PASS:8 * PASS + 40], ref[8 * PASS:8 * PASS + 40]), "pack_bf16 (second pass of the 8-wide loop)"
    assert torch.equal(dst[8 * PASS + 40:], ref[8 * PASS + 40:]), "pack_bf16 (scalar tail)"
    assert (full[:8] == 7.0).all() and (full[8 + n:] == 7.0).all()
    n = 4 * PASS + 4 * 3 + 1
    idx = idx[:n]
    full = torch.full((n + 8,), 7.0, device=dev)
    hipk.gather_f32(src, idx, full[4:4 + n])
    ref = _gather_ref(src, idx)
    dst = full[4:4 + n]
    assert torch.equal(dst[:4 * PASS], ref[:4 * PASS]), "gather_f32 (first grid pass)"
    assert torch.equal(dst[4 * PASS:4 * PASS + 12], ref[4 * PASS:4 * PASS + 12]), "gather_f32 (second pass of the 4-wide loop)"
    assert torch.equal(dst[4 * PASS + 12:], ref[4 * PASS + 12:]), "gather_f32 (scalar tail)"
    assert (full[:4] == 7.0).all() and (full[4 + n:] == 7.0).all()


@pytest.mark.parametrize("kernel", ("pack_bf16", "gather_f32"))
def test_unaligned_operands_take_the_scalar_path(dev, kernel):
    """dst[1:], idx[1:] and both: equal to the aligned (vectorised) result, nothing written in front of or behind dst"""
    from yoloseries_amd import hipk
    _RAN.add("unaligned_" + kernel)
    n = 100003
    g = torch.Generator(device=dev).manual_seed(2)
    src = torch.randn(n, generator=g, device=dev)
    idx_al = torch.randint(-1, n, (n,), generator=g, dtype=torch.int32, device=dev)
    idx_off = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), idx_al])[1:]
    assert idx_al.data_ptr() % 16 == 0 and idx_off.data_ptr() % 16 == 4 and torch.equal(idx_al, idx_off)
    dt = torch.bfloat16 if kernel == "pack_bf16" else torch.float32
    run = getattr(hipk, kernel)
    ref = _gather_ref(src, idx_al).to(dt)
    for d_off, idx in ((0, idx_al), (1, idx_al), (0, idx_off), (1, idx_off)):
        full = torch.full((n + 32,), 7.0, dtype=dt, device=dev)
        dst = full[16 + d_off:16 + d_off + n]
        assert dst.data_ptr() % 16 == d_off * full.element_size()
        run(src, idx, dst)
        assert torch.equal(dst, ref), (kernel, d_off, idx is idx_off)
        assert (full[:16 + d_off] == 7.0).all() and (full[16 + d_off + n:] == 7.0).all()


def test_pack_bf16_rounds_to_nearest_even(dev):
    """ties both ways, one fp32 ulp either side of a tie, +-0, subnormals, the largest finite values, +-inf, NaN: bit-equal to
    torch's fp32 -> bf16 conversion on the vector path and on the scalar path"""
    from yoloseries_amd import hipk
    _RAN.add("rounding")
    f = np.float32
    ties = [f(1 + 2.0 ** -8), f(1 + 3 * 2.0 ** -8), f(-(1 + 2.0 ** -8)), f(-(1 + 3 * 2.0 ** -8)), f(2.0 ** -126 * (1 + 2.0 ** -8))]
    vals = list(ties)
    for t in ties:
        vals += [np.nextafter(t, f(np.inf)), np.nextafter(t, f(-np.inf))]
    fmax = np.finfo(np.float32).max
    vals += [f(0.0), f(-0.0), f(1e-40), f(-1e-40), f(2.0 ** -133), f(2.0 ** -134), f(3 * 2.0 ** -134), f(2.0 ** -149), f(2.0 ** -126),
             f(3.39e38), f(-3.39e38), f(3.3961e38), fmax, -fmax, f(np.inf), f(-np.inf), f(np.nan), f(1.0), f(-2.5)]
    src = torch.from_numpy(np.array(vals, dtype=np.float32)).to(dev)
    k = src.numel()
    ref = src.to(torch.bfloat16)
    assert ref[0].item() == 1.0 and ref[1].item() == 1 + 2.0 ** -6          # the ties go to the even mantissa
    idx = torch.arange(k, dtype=torch.int32, device=dev).repeat(8)          # 8 * k elements: every one on the 8-wide path
    for off in (0, 1):                                                       # off = 1: unaligned dst, scalar path
        full = torch.zeros(8 * k + 16, dtype=torch.bfloat16, device=dev)
        dst = full[8 + off:8 + off + 8 * k]
        hipk.pack_bf16(src, idx, dst)
        want = ref.repeat(8)
        nan = want.isnan()
        assert torch.equal(dst.isnan(), nan) and nan.sum().item() == 8
        assert torch.equal(dst.view(torch.int16)[~nan], want.view(torch.int16)[~nan]), f"bits differ (dst offset {off})"


# ---------------------------------------------------------------- optimizer-side kernels
def _sgd_ref(p, g, buf, gi, lr, wd, mom, nesterov, first, gs=1.0):
    """one step in float64; lr / wd / mom / gs are the fp32 values the kernel reads"""
    p, g, buf = p.double(), g.double(), buf.double()
    lr_e, wd_e = lr.double()[gi], wd.double()[gi]
    gv = g * gs + wd_e * p
    b = gv if first else mom * buf + gv
    upd = gv + mom * b if nesterov else b
    return p - lr_e * upd, b


def _f32(x):
    return float(np.float32(x))


def test_streaming_kernels_beyond_one_grid_pass(dev):
    """yh_sgd_step, yh_ema_update, yh_ema_update_dev, yh_sumsq with n = 4096 * 256 + 4099"""
    from yoloseries_amd import hipk
    _RAN.add("stream_pass")
    n = PASS + 4099
    g = torch.Generator(device=dev).manual_seed(3)
    p, grad, buf = (torch.randn(n, generator=g, device=dev) for _ in range(3))
    group = (torch.arange(n, device=dev) % 3).to(torch.uint8)
    lr, wd = torch.tensor([0.1, 0.01, 0.05], device=dev), torch.tensor([0.0, 5e-4, 1e-2], device=dev)
    p_ref, b_ref = _sgd_ref(p, grad, buf, group.long(), lr, wd, _f32(0.937), True, False)
    hipk.sgd_step(p, grad, buf, group, lr, wd, 0.937, True, False)
    _close_passes(p, p_ref, 1e-5, 1e-6, "sgd_step p")
    _close_passes(buf, b_ref, 1e-5, 1e-6, "sgd_step momentum buffer")
    for how in ("host", "dev"):
        e = torch.randn(n, generator=g, device=dev)
        e_ref = _f32(0.99) * e.double() + (1 - _f32(0.99)) * p.double()
        if how == "host":
            hipk.ema_update(e, p, 0.99)
        else:
            hipk.ema_update_dev(e, p, torch.tensor([0.99], device=dev))
        _close_passes(e, e_ref, 1e-5, 1e-6, f"ema_update ({how} decay)")
    part, out = torch.full((4096,), NAN, device=dev), torch.full((1,), NAN, device=dev)
    hipk.sumsq(grad, part, out)
    _close(out, (grad.double() ** 2).sum().reshape(1), 1e-6, 0.0, "sumsq")
    tail = torch.zeros_like(grad)
    tail[PASS:] = grad[PASS:]
    hipk.sumsq(tail, part, out)
    _close(out, (tail.double() ** 2).sum().reshape(1), 1e-6, 0.0, "sumsq of the elements of the second grid pass")


@pytest.mark.parametrize("n", (1, 255))
def test_sumsq_small(dev, n):
    from yoloseries_amd import hipk
    _RAN.add(("sumsq", n))
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(dev)
    full = torch.cat([torch.full((4,), 1e6, device=dev), x, torch.full((4,), 1e6, device=dev)])          # nothing is read past the ends
    part, out = torch.full((4096,), NAN, device=dev), torch.full((1,), NAN, device=dev)
    hipk.sumsq(full[4:4 + n], part, out)
    _close(out, (x.double() ** 2).sum().reshape(1), 1e-6, 0.0, "sumsq")


@pytest.mark.parametrize("case", ("plain", "no_momentum", "no_group", "three_groups"))
def test_sgd_step_variants(dev, case):
    """no nesterov, momentum 0, group == NULL, three groups — each as a continuing step (first_step = 0) on a non-zero buffer"""
    from yoloseries_amd import hipk
    _RAN.add(("sgd", case))
    n = 4099
    g = torch.Generator().manual_seed(4)
    p, grad, buf = (torch.randn(n, generator=g).to(dev) for _ in range(3))
    lr, wd = torch.tensor([0.1, 0.01, 0.05], device=dev), torch.tensor([1e-3, 5e-4, 0.0], device=dev)
    mom = 0.0 if case == "no_momentum" else 0.9
    nesterov = case == "three_groups"
    group = None if case == "no_group" else (torch.arange(n) % (3 if case == "three_groups" else 2)).to(torch.uint8).to(dev)
    gi = torch.zeros(n, dtype=torch.long, device=dev) if group is None else group.long()
    p0, b0 = p.clone(), buf.clone()
    p_ref, b_ref = _sgd_ref(p0, grad, b0, gi, lr, wd, _f32(mom), nesterov, False)
    hipk.sgd_step(p, grad, buf, group, lr, wd, mom, nesterov, False)
    _close(p, p_ref, 1e-5, 1e-6, "p")
    _close(buf, b_ref, 1e-5, 1e-6, "momentum buffer")
    assert not torch.equal(buf, grad), "first_step = 0 must use the buffer"
    # the first step ignores what the buffer holds
    p, buf = p0.clone(), b0.clone()
    p_ref, b_ref = _sgd_ref(p0, grad, b0, gi, lr, wd, _f32(mom), nesterov, True)
    hipk.sgd_step(p, grad, buf, group, lr, wd, mom, nesterov, True)
    _close(p, p_ref, 1e-5, 1e-6, "p (first step)")
    _close(buf, b_ref, 1e-5, 1e-6, "momentum buffer (first step)")


def test_sgd_step_dev_group_cap(dev):
    """group bytes above 2 read the constants of group 2"""
    from yoloseries_amd import hipk
    _RAN.add("group_cap")
    n = 4099
    g = torch.Generator().manual_seed(5)
    p, grad, buf = (torch.randn(n, generator=g).to(dev) for _ in range(3))
    group = torch.tensor([0, 1, 2, 3, 255], dtype=torch.uint8).repeat(n // 5 + 1)[:n].to(dev)
    scal = torch.tensor([0.1, 0.05, 0.2, 0.0, 1e-2, 1e-3, 0.9, 0.0], device=dev)
    p_ref, b_ref = _sgd_ref(p, grad, buf, group.long().clamp(max=2), scal[:3], scal[3:6], _f32(0.9), True, False)
    hipk.sgd_step_dev(p, grad, buf, group, scal, True)
    _close(p, p_ref, 1e-5, 1e-6, "p")
    _close(buf, b_ref, 1e-5, 1e-6, "momentum buffer")


@pytest.mark.parametrize("s,max_norm", [(0.25, 1.0), (1.0, 1.0), (100.0, 1.0), (0.0, 1.0), (3.0, 10.0), (4e4, 10.0)])
def test_clip_scale(dev, s, max_norm):
    """norm below, equal to, above max_norm and zero: min(1, max_norm / (sqrt(s) + 1e-6))"""
    from yoloseries_amd import hipk
    _RAN.add(("clip", s, max_norm))
    out = torch.full((3,), NAN, device=dev)
    hipk.clip_scale(torch.tensor([s], device=dev), max_norm, out[1:2])
    want = min(1.0, max_norm / (s ** 0.5 + 1e-6))
    got = out[1].item()
    assert abs(got - want) <= 1e-6 * want and got <= 1.0
    assert got == 1.0 if s ** 0.5 < max_norm else got < 1.0
    assert out[0].isnan() and out[2].isnan()


@pytest.mark.parametrize("entry", ("sgd_step", "sgd_step_dev"))
def test_clipped_sgd_tail(dev, entry):
    """yh_sumsq -> yh_clip_scale -> SGD with grad_scale against torch.nn.utils.clip_grad_norm_ + torch.optim.SGD (float64): two
    steps, the first with a gradient norm of about 64 (clipped to 10), the second of about 0.6 (left alone)"""
    from yoloseries_amd import hipk
    _RAN.add(("tail", entry))
    n, half, max_norm, mom = 4099, 2049, 10.0, 0.937
    g = torch.Generator().manual_seed(6)
    p = torch.randn(n, generator=g).to(dev)
    lrs, wds = [0.1, 0.01], [0.0, 5e-4]
    ref = [p[:half].double().clone().requires_grad_(True), p[half:].double().clone().requires_grad_(True)]
    opt = torch.optim.SGD([{"params": [ref[i]], "lr": _f32(lrs[i]), "weight_decay": _f32(wds[i])} for i in range(2)], lr=0.1, momentum=_f32(mom), nesterov=True)
    group = torch.zeros(n, dtype=torch.uint8, device=dev)
    group[half:] = 1
    lr, wd = torch.tensor(lrs, device=dev), torch.tensor(wds, device=dev)
    scal = torch.tensor(lrs + [0.0] + wds + [0.0, mom, 1.0], device=dev)
    buf = torch.zeros(n, device=dev)
    part, ss, gs = torch.zeros(4096, device=dev), torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    scales = []
    for step, mag in enumerate((1.0, 0.01)):
        grad = (torch.randn(n, generator=g) * mag).to(dev)
        ref[0].grad, ref[1].grad = grad[:half].double(), grad[half:].double()
        total = torch.nn.utils.clip_grad_norm_(ref, max_norm)
        opt.step()
        hipk.sumsq(grad, part, ss)
        hipk.clip_scale(ss, max_norm, gs)
        if entry == "sgd_step":
            hipk.sgd_step(p, grad, buf, group, lr, wd, mom, True, step == 0, gs)
        else:
            scal[7] = 1.0 if step == 0 else 0.0
            hipk.sgd_step_dev(p, grad, buf, group, scal, True, gs)
        scales.append(gs.item())
        want = min(1.0, max_norm / (total.item() + 1e-6))
        assert abs(gs.item() - want) <= 1e-6 * want
    assert scales[0] < 0.2 and scales[1] == 1.0, scales
    _close(p, torch.cat(ref).detach(), 1e-5, 1e-6, "parameters after two clipped steps")


def test_zz_every_case_ran():
    want = {"gather_pass", "unaligned_pack_bf16", "unaligned_gather_f32", "rounding", "stream_pass", "group_cap", ("sumsq", 1), ("sumsq", 255),
            ("tail", "sgd_step"), ("tail", "sgd_step_dev")} | {("sgd", c) for c in ("plain", "no_momentum", "no_group", "three_groups")}
    assert want <= _RAN and sum(1 for k in _RAN if isinstance(k, tuple) and k[0] == "clip") == 6
