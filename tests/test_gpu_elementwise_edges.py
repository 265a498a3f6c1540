"""Edges of the kernels in csrc/elementwise.hip: ragged channel counts (C/8 that does not divide the thread counts), launches
that leave the first grid pass, the slab walk of the finalize kernels, saturated SiLU, and the entry points that had no test.

References are plain torch in float64 on the same bf16-representable inputs.  Every bf16 operand is the channel slice
[8, 8 + C) of a buffer with C + 16 channels: inputs are NaN outside the slice, outputs hold a sentinel outside it.

Bars (tests/test_gpu_elementwise.py): bf16 outputs rtol 8e-3 / atol 2e-2; gy 1e-2 and 1e-2 * max|ref|; dgamma / dbeta / coef
2e-3 and 2e-3 * max|ref|; an overwritten gres is bit-exact.  The finalize kernels are compared with the same expressions in
float64 on the same slab values: rtol 1e-6, and atol 2^-22 * (largest term) where fp32 products are subtracted.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = 7.0                      # sentinel of output buffers (exact in bf16)
NAN = float("nan")
BF = torch.bfloat16
EPS = float(np.float32(1e-3))   # the value the kernels receive
MOM = float(np.float32(0.03))
U22 = 2.0 ** -22
U40 = 2.0 ** -40

RAGGED_C = (8, 24, 48, 80, 96, 160, 192, 320, 2048)
RAGGED_M = (1, 7, 257, 1000)
PARTS = ((80, 80), (24, 40, 8), (48, 96, 48, 8))
GRID_APPLY = ((80, 60000), (24, 180000))
GRID_REDUCE = ((24, 140000), (1024, 20000))
FIN_NBLK = (1, 31, 32, 33, 255, 256, 257, 600)
FIN_C = (8, 24, 80, 264)
_RAN = {"ragged": set(), "parts": set(), "grid_apply": set(), "grid_reduce": set(), "grid_misc": set(), "fin": set(), "fin_parts": set()}


# ---------------------------------------------------------------- helpers
def _nan_slice(lead, C, dev, seed, scale=1.0):
    """random bf16 values in channels [8, 8 + C) of a NaN buffer -> (buffer, Slice, float64 values)"""
    from yoloseries_amd import hipk
    g = torch.Generator(device=dev).manual_seed(seed)
    buf = torch.full((*lead, C + 16), NAN, dtype=BF, device=dev)
    buf[..., 8:8 + C] = (torch.randn(*lead, C, generator=g, device=dev) * scale).to(BF)
    return buf, hipk.Slice(buf, 8, C), buf[..., 8:8 + C].double()


def _sent_slice(lead, C, dev):
    from yoloseries_amd import hipk
    buf = torch.full((*lead, C + 16), SENT, dtype=BF, device=dev)
    return buf, hipk.Slice(buf, 8, C)


def _guard_ok(buf, C):
    assert (buf[..., :8] == SENT).all() and (buf[..., 8 + C:] == SENT).all(), "written outside the channel slice"


def _close(got, ref, rtol, atol, what=""):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    lim = atol + rtol * ref.abs()
    bad = ~(err <= lim)          # a NaN on either side is bad
    assert not bad.any(), f"{what}: max err {err.nan_to_num(nan=math.inf).max().item():.4g}, {bad.sum().item()} of {err.numel()} out of tolerance"


def _close_passes(got, ref, rtol, atol, what, tail=1000):
    """rows that only a later grid pass reaches are reported on their own"""
    n = got.shape[0]
    got, ref = got.reshape(n, -1), ref.reshape(n, -1)
    _close(got[:n - tail], ref[:n - tail], rtol, atol, what + " (first rows)")
    _close(got[n - tail:], ref[n - tail:], rtol, atol, what + f" (last {tail} rows: a later grid pass)")


def _params(C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.5).to(dev)


def _ws_of(yv, gamma, beta, dev):
    """ws = scale | shift | mean | invstd from yh_bn_finalize on the float64 sums of the slice (one slab row)"""
    from yoloseries_amd import hipk
    M, C = yv.shape
    stats = torch.stack([yv.sum(0), (yv * yv).sum(0)]).float().reshape(1, 2, C).contiguous()
    ws = torch.full((4 * C,), NAN, device=dev)
    hipk.bn_finalize(stats, 1, C, C, M, gamma, beta, None, None, None, EPS, MOM, ws)
    return ws


class _Ref:
    """training-mode BatchNorm + SiLU and its backward in float64"""

    def __init__(self, yv, gamma, beta):
        self.M = yv.shape[0]
        self.gamma = gamma.double()
        self.mean = yv.mean(0)
        self.invstd = ((yv - self.mean) ** 2).mean(0).add(EPS).rsqrt()
        self.xhat = (yv - self.mean) * self.invstd
        self.z = self.xhat * self.gamma + beta.double()
        self.sg = torch.sigmoid(self.z)
        self.act = self.z * self.sg

    def backward(self, gv):
        self.dz = gv * self.sg * (1 + self.z * (1 - self.sg))
        self.dbeta = self.dz.sum(0)
        self.dgamma = (self.dz * self.xhat).sum(0)
        self.coef = torch.cat([self.dbeta, self.dgamma]) / self.M
        self.gy = self.gamma * self.invstd * (self.dz - self.dbeta / self.M - self.xhat * self.dgamma / self.M)
        return self


def _mx(t):
    return t.abs().max().item()


# ---------------------------------------------------------------- 1. ragged widths
@pytest.mark.parametrize("M", RAGGED_M)
@pytest.mark.parametrize("C", RAGGED_C)
def test_bn_silu_passes_at_ragged_widths(dev, C, M):
    """yh_bn_silu_apply (with / without residual), yh_bn_silu_bwd_reduce + yh_bn_bwd_finalize, yh_bn_silu_bwd_apply (gres absent,
    overwritten, accumulated) against float64 at chunk counts that do not divide 256 / 512 threads and at fewer rows than one
    reduce block has row groups.

    M = 1: xhat, dgamma and gy are identically zero in exact arithmetic, so "x * max|ref|" asks for exact zeros, which differences
    of fp32 products cannot give.  There the absolute bar is 2^-22 * (largest term of the difference), the rule of the finalize
    tests: dgamma = invstd * (sum(dz*y) - mean*sum(dz)), gy = gamma*invstd*dz - (...)."""
    from yoloseries_amd import hipk
    _RAN["ragged"].add((C, M))
    ybuf, y, yv = _nan_slice((M,), C, dev, 1, 2.0)
    gamma, beta = _params(C, dev, 100 + C)
    ws = _ws_of(yv, gamma, beta, dev)
    r = _Ref(yv, gamma, beta)
    # forward
    obuf, o = _sent_slice((M,), C, dev)
    hipk.bn_silu_apply(y, ws, M, o)
    _close(obuf[:, 8:8 + C], r.act, 8e-3, 2e-2, "apply")
    _guard_ok(obuf, C)
    rbuf, res, resv = _nan_slice((M,), C, dev, 2)
    obuf, o = _sent_slice((M,), C, dev)
    hipk.bn_silu_apply(y, ws, M, o, res)
    # |bf16(act) - act| + |bf16(sum) - sum| <= 2^-9 (|act| + |sum|): inside atol + rtol * |sum| for |act| <= 10
    _close(obuf[:, 8:8 + C], r.act + resv, 8e-3, 2e-2, "apply + residual")
    _guard_ok(obuf, C)
    # backward
    gbuf, ga, gv = _nan_slice((M,), C, dev, 3)
    r.backward(gv)
    nblk = hipk.ew_blocks(M)
    assert nblk == (M + 255) // 256
    part = torch.full((nblk, 2, C), NAN, device=dev)
    hipk.bn_silu_bwd_reduce(ga, y, ws, M, part)
    dgamma, dbeta, coef = (torch.full((n,), NAN, device=dev) for n in (C, C, 2 * C))
    hipk.bn_bwd_finalize(part, nblk, C, M, ws, dgamma, dbeta, coef)
    fl_dg = fl_gy = 0.0
    if M == 1:
        fl_dg = U22 * _mx(r.invstd * (r.dz * yv).abs().sum(0))
        fl_gy = U22 * _mx(r.gamma * r.invstd * r.dz)
    _close(dbeta, r.dbeta, 2e-3, 2e-3 * _mx(r.dbeta), "dbeta")
    _close(dgamma, r.dgamma, 2e-3, 2e-3 * _mx(r.dgamma) + fl_dg, "dgamma")
    _close(coef[:C], r.coef[:C], 2e-3, 2e-3 * _mx(r.coef[:C]), "coef[0]")
    _close(coef[C:], r.coef[C:], 2e-3, 2e-3 * _mx(r.coef[C:]) + fl_dg / M, "coef[1]")
    gres0buf, _, gres0 = _nan_slice((M,), C, dev, 4)
    for mode in ("none", "overwrite", "accumulate"):
        gybuf, gy = _sent_slice((M,), C, dev)
        grbuf = gres0buf.clone()
        grbuf[:, :8] = SENT
        grbuf[:, 8 + C:] = SENT
        gres = None if mode == "none" else hipk.Slice(grbuf, 8, C)
        hipk.bn_silu_bwd_apply(ga, y, ws, gamma, coef, M, gy, gres, int(mode == "accumulate"))
        _close(gybuf[:, 8:8 + C], r.gy, 1e-2, 1e-2 * _mx(r.gy) + fl_gy, f"gy ({mode})")
        _guard_ok(gybuf, C)
        _guard_ok(grbuf, C)
        if mode == "none":
            assert torch.equal(grbuf[:, 8:8 + C].view(torch.int16), gres0buf[:, 8:8 + C].view(torch.int16))
        elif mode == "overwrite":
            assert torch.equal(grbuf[:, 8:8 + C].view(torch.int16), gbuf[:, 8:8 + C].view(torch.int16)), "gres overwrite is a copy"
        else:
            _close(grbuf[:, 8:8 + C], gres0 + gv, 8e-3, 2e-2, "gres accumulate")


def _stacked(dev, Cs, M, seed):
    """operands of a stacked layer: y over all channels, per part constants (from the float64 reference sums), destinations,
    incoming gradients; coef comes from the reference so that the apply passes are tested on their own"""
    from yoloseries_amd import hipk
    Ct = sum(Cs)
    ybuf, y, yv = _nan_slice((M,), Ct, dev, seed, 2.0)
    parts, c0 = [], 0
    for i, C in enumerate(Cs):
        gamma, beta = _params(C, dev, seed + 10 + i)
        yp = yv[:, c0:c0 + C]
        ws = _ws_of(yp, gamma, beta, dev)
        gbuf, ga, gv = _nan_slice((M,), C, dev, seed + 20 + i)
        r = _Ref(yp, gamma, beta).backward(gv)
        parts.append(dict(C=C, c0=c0, y=hipk.Slice(ybuf, 8 + c0, C), gamma=gamma, ws=ws, ga=ga, gbuf=gbuf, ref=r, coef=r.coef.float().contiguous()))
        c0 += C
    return ybuf, y, parts


def _run_parts(dev, Cs, M, seed, close):
    """both _parts passes: bit-identical to the per-part launches, within the bars of float64, nothing outside the slices"""
    from yoloseries_amd import hipk
    Ct = sum(Cs)
    ybuf, y, parts = _stacked(dev, Cs, M, seed)
    outs = []
    gy1buf, gy1 = _sent_slice((M,), Ct, dev)          # per-part launches
    gyPbuf, gyP = _sent_slice((M,), Ct, dev)          # one launch
    for q in parts:
        C = q["C"]
        o1buf, o1 = _sent_slice((M,), C, dev)
        hipk.bn_silu_apply(q["y"], q["ws"], M, o1)
        hipk.bn_silu_bwd_apply(q["ga"], q["y"], q["ws"], q["gamma"], q["coef"], M, hipk.Slice(gy1buf, 8 + q["c0"], C))
        oPbuf, oP = _sent_slice((M,), C, dev)
        outs.append((o1buf, oPbuf))
        q["out"] = oP
    hipk.bn_silu_apply_parts(y, M, [dict(ws=q["ws"], C=q["C"], out=q["out"]) for q in parts])
    hipk.bn_silu_bwd_apply_parts(y, M, [dict(ws=q["ws"], C=q["C"], ga=q["ga"], gamma=q["gamma"], coef=q["coef"]) for q in parts], gyP)
    torch.cuda.synchronize()
    for q, (o1buf, oPbuf) in zip(parts, outs):
        C, r = q["C"], q["ref"]
        assert torch.equal(oPbuf.view(torch.int16), o1buf.view(torch.int16)), f"apply_parts differs from the per-part launch (C={C})"
        _guard_ok(oPbuf, C)
        close(oPbuf[:, 8:8 + C], r.act, 8e-3, 2e-2, f"apply_parts C={C}")
        close(gyPbuf[:, 8 + q["c0"]:8 + q["c0"] + C], r.gy, 1e-2, 1e-2 * _mx(r.gy), f"bwd_apply_parts C={C}")
    assert torch.equal(gyPbuf.view(torch.int16), gy1buf.view(torch.int16)), "bwd_apply_parts differs from the per-part launches"
    _guard_ok(gyPbuf, Ct)


@pytest.mark.parametrize("M", (7, 1000))
@pytest.mark.parametrize("Cs", PARTS)
def test_stacked_passes_at_ragged_widths(dev, Cs, M):
    _RAN["parts"].add((Cs, M))
    _run_parts(dev, Cs, M, 40, _close)


def test_bad_slices_are_refused(dev):
    """C > 2048, ld < C and a pointer that is not 16-byte aligned return an error before anything is launched"""
    from yoloseries_amd import hipk
    from yoloseries_amd._lib import YoloHipError
    M = 4

    def calls(C, mk):
        ws, gamma, coef = torch.zeros(4 * C, device=dev), torch.ones(C, device=dev), torch.zeros(2 * C, device=dev)
        part, out = torch.zeros(1, 2, C, device=dev), torch.zeros(C, device=dev)
        return [lambda: hipk.bn_silu_apply(mk(), ws, M, mk()),
                lambda: hipk.bn_silu_bwd_reduce(mk(), mk(), ws, M, part),
                lambda: hipk.bn_silu_bwd_apply(mk(), mk(), ws, gamma, coef, M, mk()),
                lambda: hipk.colsum(mk(), M, part, out)]

    wide = lambda C: torch.zeros(2 * M, C + 16, dtype=BF, device=dev)      # noqa: E731  (room for whatever a launch would touch)
    for f in calls(2056, lambda: hipk.Slice(wide(2056), 8, 2056)):
        with pytest.raises(YoloHipError):
            f()
    for f in calls(80, lambda: hipk.Slice(torch.zeros(4 * M, 72, dtype=BF, device=dev), 0, 80)):          # ld = C - 8
        with pytest.raises(YoloHipError):
            f()
    for f in calls(80, lambda: hipk.Slice(wide(80), 4, 80)):                                                # 8 bytes off
        with pytest.raises(YoloHipError):
            f()
    y80 = hipk.Slice(wide(80), 8, 80)
    ws = torch.zeros(4 * 40, device=dev)
    for bad in (hipk.Slice(wide(40), 4, 40), hipk.Slice(torch.zeros(4 * M, 32, dtype=BF, device=dev), 0, 40)):
        ok = hipk.Slice(wide(40), 8, 40)
        with pytest.raises(YoloHipError):
            hipk.bn_silu_apply_parts(y80, M, [dict(ws=ws, C=40, out=ok), dict(ws=ws, C=40, out=bad)])
        with pytest.raises(YoloHipError):
            hipk.bn_silu_bwd_apply_parts(y80, M, [dict(ws=ws, C=40, ga=ok, gamma=ws, coef=ws), dict(ws=ws, C=40, ga=bad, gamma=ws, coef=ws)], y80)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. past one grid pass
@pytest.mark.parametrize("C,M", GRID_APPLY)
def test_apply_passes_beyond_one_grid_pass(dev, C, M):
    """more than 2048 * 256 chunks: the `m += rstep` loops run; the rows of the later pass are asserted on their own"""
    from yoloseries_amd import hipk
    _RAN["grid_apply"].add((C, M))
    assert M * (C // 8) > 2048 * 256
    ybuf, y, yv = _nan_slice((M,), C, dev, 5, 2.0)
    gamma, beta = _params(C, dev, 6)
    ws = _ws_of(yv, gamma, beta, dev)
    gbuf, ga, gv = _nan_slice((M,), C, dev, 7)
    r = _Ref(yv, gamma, beta).backward(gv)
    coef = r.coef.float().contiguous()
    rbuf, res, resv = _nan_slice((M,), C, dev, 8)
    obuf, o = _sent_slice((M,), C, dev)
    hipk.bn_silu_apply(y, ws, M, o, res)
    _close_passes(obuf[:, 8:8 + C], r.act + resv, 8e-3, 2e-2, "apply + residual")
    _guard_ok(obuf, C)
    gybuf, gy = _sent_slice((M,), C, dev)
    grbuf, gres, gres0 = _nan_slice((M,), C, dev, 9)
    hipk.bn_silu_bwd_apply(ga, y, ws, gamma, coef, M, gy, gres, 1)
    _close_passes(gybuf[:, 8:8 + C], r.gy, 1e-2, 1e-2 * _mx(r.gy), "gy")
    _close_passes(grbuf[:, 8:8 + C], gres0 + gv, 8e-3, 2e-2, "gres accumulate")
    _guard_ok(gybuf, C)
    assert grbuf[:, :8].isnan().all() and grbuf[:, 8 + C:].isnan().all()
    # the stacked passes stride, their per-part launches (half the chunks) do not
    Cs = (C // 2, C // 2) if C % 16 == 0 else (8, C - 8)
    _run_parts(dev, Cs, M, 60, _close_passes)


@pytest.mark.parametrize("C,M", GRID_REDUCE)
def test_reductions_beyond_one_grid_pass(dev, C, M):
    """yh_bn_silu_bwd_reduce + finalize and yh_colsum where a block takes many row groups (C = 1024: the 4-deep main loop) and
    where yh_ew_blocks is capped (M = 140 000).  The project's 2e-3 * max bar holds with room: a float32 torch evaluation of the
    same sums is within 1e-6 * max of float64 at these sizes."""
    from yoloseries_amd import hipk
    _RAN["grid_reduce"].add((C, M))
    nblk = hipk.ew_blocks(M)
    assert nblk == min(512, (M + 255) // 256)
    if M == 140000:
        assert nblk == 512
    ybuf, y, yv = _nan_slice((M,), C, dev, 11, 2.0)
    gamma, beta = _params(C, dev, 12)
    ws = _ws_of(yv, gamma, beta, dev)
    gbuf, ga, gv = _nan_slice((M,), C, dev, 13)
    r = _Ref(yv, gamma, beta)
    tail = torch.zeros(M, 1, dtype=torch.float64, device=dev)
    tail[M - 1000:] = 1.0
    for what, mask in (("all rows", None), ("only the last 1000 rows (a later row group of every block)", tail)):
        if mask is not None:
            gbuf[:, 8:8 + C] = (gv * mask).to(BF)
        g64 = gbuf[:, 8:8 + C].double()
        r.backward(g64)
        part = torch.full((nblk, 2, C), NAN, device=dev)
        hipk.bn_silu_bwd_reduce(ga, y, ws, M, part)
        dgamma, dbeta, coef = (torch.full((n,), NAN, device=dev) for n in (C, C, 2 * C))
        hipk.bn_bwd_finalize(part, nblk, C, M, ws, dgamma, dbeta, coef)
        _close(dbeta, r.dbeta, 2e-3, 2e-3 * _mx(r.dbeta), "dbeta, " + what)
        _close(dgamma, r.dgamma, 2e-3, 2e-3 * _mx(r.dgamma), "dgamma, " + what)
        _close(coef, r.coef, 2e-3, 2e-3 * _mx(r.coef), "coef, " + what)
        part = torch.full((nblk, 2, C), NAN, device=dev)
        out = torch.full((C,), NAN, device=dev)
        hipk.colsum(ga, M, part, out)
        ref = g64.sum(0)
        _close(out, ref, 2e-3, 2e-3 * _mx(ref), "colsum, " + what)


def test_pool_and_upsample_beyond_one_grid_pass(dev):
    """yh_maxpool5_fwd / _bwd and yh_upsample2_bwd on 552 960 chunks (> 2048 * 256): `id += gridDim * blockDim` runs"""
    from yoloseries_amd import hipk
    _RAN["grid_misc"].add("pool")
    B, H, W, C = 6, 96, 96, 80
    assert B * H * W * (C // 8) > 2048 * 256
    xbuf, x, xv = _nan_slice((B, H, W), C, dev, 21)
    obuf, o = _sent_slice((B, H, W), C, dev)
    idx = torch.full((B, H, W, C), 99, dtype=torch.int8, device=dev)
    hipk.maxpool5_fwd(x, B, H, W, o, idx)
    xn = xv.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ref = F.max_pool2d(xn, 5, 1, 2)
    refl = ref.detach().permute(0, 2, 3, 1)
    got = obuf[..., 8:8 + C].double()
    assert torch.equal(got[:5], refl[:5]), "maxpool5_fwd (first images)"
    assert torch.equal(got[5], refl[5]), "maxpool5_fwd (last image: the second grid pass)"
    _guard_ok(obuf, C)
    gbuf, go, gov = _nan_slice((B, H, W), C, dev, 22)
    (gref,) = torch.autograd.grad(ref, xn, gov.permute(0, 3, 1, 2))
    gref = gref.permute(0, 2, 3, 1)
    gibuf, gi = _sent_slice((B, H, W), C, dev)
    hipk.maxpool5_bwd(go, idx, B, H, W, gi, 0)
    _close(gibuf[:5, ..., 8:8 + C], gref[:5], 8e-3, 2e-2, "maxpool5_bwd (first images)")
    _close(gibuf[5, ..., 8:8 + C], gref[5], 8e-3, 2e-2, "maxpool5_bwd (last image: the second grid pass)")
    _guard_ok(gibuf, C)
    # upsample gradient
    _RAN["grid_misc"].add("upsample")
    hbuf, ghi, hv = _nan_slice((B, 2 * H, 2 * W), C, dev, 23)
    lbuf, glo = _sent_slice((B, H, W), C, dev)
    hipk.upsample2_bwd(ghi, B, H, W, glo, 0)
    uref = hv.reshape(B, H, 2, W, 2, C).sum((2, 4))
    _close(lbuf[:5, ..., 8:8 + C], uref[:5], 8e-3, 2e-2, "upsample2_bwd (first images)")
    _close(lbuf[5, ..., 8:8 + C], uref[5], 8e-3, 2e-2, "upsample2_bwd (last image: the second grid pass)")
    _guard_ok(lbuf, C)


def _s2d_ref(x):
    B, Cin, H, W = x.shape
    return x.reshape(B, Cin, H // 2, 2, W // 2, 2).permute(0, 2, 4, 3, 5, 1).reshape(B, H // 2, W // 2, 4 * Cin).to(BF)


def test_s2d_and_fill_beyond_one_grid_pass(dev):
    from yoloseries_amd import hipk
    _RAN["grid_misc"].add("s2d")
    B, H, W = 3, 896, 896
    assert B * (H // 2) * (W // 2) > 2048 * 256
    x = torch.rand(B, 3, H, W, device=dev)
    out = torch.full((B, H // 2, W // 2, 16), SENT, dtype=BF, device=dev)
    hipk.input_s2d(x, out)
    ref = _s2d_ref(x)
    for b, what in ((slice(0, 2), "first images"), (slice(2, 3), "last image: the second grid pass")):
        assert torch.equal(out[b, ..., :12], ref[b]) and (out[b, ..., 12:] == 0).all(), f"input_s2d ({what})"
    _RAN["grid_misc"].add("fill")
    n = 2048 * 256 + 3
    t = torch.full((n + 8,), 0x11111111, dtype=torch.int32, device=dev)
    hipk.fill_u32(t, 0xDEADBEEF, n, word_off=4)
    v = 0xDEADBEEF - (1 << 32)
    assert (t[4:4 + 2048 * 256] == v).all(), "fill_u32 (first pass)"
    assert (t[4 + 2048 * 256:4 + n] == v).all(), "fill_u32 (second pass)"
    assert (t[:4] == 0x11111111).all() and (t[4 + n:] == 0x11111111).all()


# ---------------------------------------------------------------- 3. the slab walk of the finalize kernels
def _fwd_slab(nblk, C, ld, dev, seed):
    """[nblk][2][ld] forward statistics, 64 samples per row; NaN in the padding columns.
    channel 0: constant 3.0 (variance exactly 0); channel 1: sum(x^2)/count one fp32 ulp below mean^2; the others: mean 50, std 0.05"""
    g = torch.Generator().manual_seed(seed)
    x = 50.0 + 0.05 * torch.randn(nblk, 64, C, generator=g, dtype=torch.float64)
    slab = torch.full((nblk, 2, ld), NAN, dtype=torch.float32)
    slab[:, 0, :C] = x.sum(1).float()
    slab[:, 1, :C] = (x * x).sum(1).float()
    count = nblk * 64
    slab[:, 0, 0], slab[:, 1, 0] = 192.0, 576.0
    slab[:, :, 1] = 0.0
    slab[0, 0, 1] = 3.0 * count
    slab[0, 1, 1] = float(np.nextafter(np.float32(9.0 * count), np.float32(0.0)))
    assert float(slab[0, 0, 1]) == 3.0 * count and float(slab[0, 1, 1]) < 9.0 * count
    return slab.to(dev), count


def _fin_ref(slab, C, count, gamma, beta, rm, rv):
    """the finalize in float64, from the slab values"""
    s = slab[:, :, :C].double().sum(0)
    mean = s[0] / count
    var = (s[1] / count - mean * mean).clamp(min=0.0)
    invstd = (var + EPS).rsqrt()
    scale = gamma.double() * invstd
    unbiased = var * count / (count - 1) if count > 1 else var
    d = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=beta.double() - mean * scale,
             shift_term=torch.maximum(beta.double().abs(), (mean * scale).abs()))
    if rm is not None:
        d.update(rm=(1 - MOM) * rm.double() + MOM * mean, rm_term=torch.maximum(((1 - MOM) * rm.double()).abs(), (MOM * mean).abs()),
                 rv=(1 - MOM) * rv.double() + MOM * unbiased)
    return d


def _check_fin(ws, C, ref, rm=None, rv=None, what=""):
    _close(ws[:C], ref["scale"], 1e-6, 0.0, what + " scale")
    _close(ws[C:2 * C], ref["shift"], 0.0, U22 * ref["shift_term"], what + " shift")
    _close(ws[2 * C:3 * C], ref["mean"], 1e-6, 0.0, what + " mean")
    _close(ws[3 * C:], ref["invstd"], 1e-6, 0.0, what + " invstd")
    if rm is not None:
        _close(rm, ref["rm"], 0.0, U22 * ref["rm_term"], what + " running_mean")
        _close(rv, ref["rv"], 1e-6, 0.0, what + " running_var")


@pytest.mark.parametrize("pad", (False, True))
@pytest.mark.parametrize("C", FIN_C)
@pytest.mark.parametrize("nblk", FIN_NBLK)
def test_finalize_kernels_walk_the_slab(dev, nblk, C, pad):
    """yh_bn_finalize, yh_bn_bwd_finalize and yh_colsum's finalize on slabs of 1 .. 600 rows (clamped and masked rows, eight loads in
    flight, the 256-row stride), ldstat = C and ldstat = C rounded up to 128 with NaN padding.  yh_bn_bwd_finalize and the
    column-sum finalize take no leading dimension (the slab is dense) and run in the ldstat = C cases; yh_colsum has no entry point
    for a slab of its own and at most 512 blocks, so its 600-row case runs with the 512 rows of M = 131 072."""
    from yoloseries_amd import hipk
    _RAN["fin"].add((nblk, C, pad))
    ld = (C + 127) // 128 * 128 if pad else C
    slab, count = _fwd_slab(nblk, C, ld, dev, 7 * nblk + C)
    g = torch.Generator().manual_seed(nblk + C)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
    rm, rv = (50 + torch.randn(C, generator=g)).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev)
    nbt = torch.tensor([41], dtype=torch.int64, device=dev)
    rm0, rv0 = rm.clone(), rv.clone()
    ws = torch.full((4 * C,), NAN, device=dev)
    hipk.bn_finalize(slab, nblk, ld, C, count, gamma, beta, rm, rv, nbt, EPS, MOM, ws)
    ref = _fin_ref(slab, C, count, gamma, beta, rm0, rv0)
    _check_fin(ws, C, ref, rm, rv, "first call:")
    assert nbt.item() == 42
    assert not ws.isnan().any()
    e = np.float32(1.0 / math.sqrt(float(np.float32(1e-3))))
    assert ws[2 * C].item() == 3.0 and ws[3 * C].item() == e, "constant channel: mean exact, invstd = eps ** -0.5"
    assert ws[2 * C + 1].item() == 3.0 and ws[3 * C + 1].item() == e, "variance one ulp below zero is clamped"
    # second call: same constants bit for bit, the running statistics move on from the first call's
    rm1, rv1, ws1 = rm.clone(), rv.clone(), ws.clone()
    ws.fill_(NAN)
    hipk.bn_finalize(slab, nblk, ld, C, count, gamma, beta, rm, rv, nbt, EPS, MOM, ws)
    assert torch.equal(ws, ws1) and nbt.item() == 43
    _check_fin(ws, C, _fin_ref(slab, C, count, gamma, beta, rm1, rv1), rm, rv, "second call:")
    # no running statistics
    ws.fill_(NAN)
    hipk.bn_finalize(slab, nblk, ld, C, count, gamma, beta, None, None, None, EPS, MOM, ws)
    assert torch.equal(ws, ws1)
    # one sample: the unbiased variance is the biased one (no division by count - 1 = 0)
    one = torch.full((nblk, 2, ld), NAN, device=dev)
    one[:, :, :C] = 0.0
    xs = torch.where(torch.arange(C) % 2 == 0, torch.tensor(1.5), torch.randn(C, generator=g)).to(dev)
    one[nblk - 1, 0, :C], one[nblk - 1, 1, :C] = xs, xs * xs
    rm, rv = rm0.clone(), rv0.clone()
    ws.fill_(NAN)
    hipk.bn_finalize(one, nblk, ld, C, 1, gamma, beta, rm, rv, None, EPS, MOM, ws)
    _check_fin(ws, C, _fin_ref(one, C, 1, gamma, beta, rm0, rv0), rm, rv, "count = 1:")
    assert not rv.isnan().any() and ws[3 * C].item() == e
    if pad:
        return
    # backward finalize on a dense slab
    part = torch.randn(nblk, 2, C, generator=g).to(dev)
    wsb = torch.cat([torch.zeros(2 * C), torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5]).to(dev)
    Mrows = 1000
    outs = []
    for _ in range(2):
        dgamma, dbeta, coef = (torch.full((n,), NAN, device=dev) for n in (C, C, 2 * C))
        hipk.bn_bwd_finalize(part, nblk, C, Mrows, wsb, dgamma, dbeta, coef)
        outs.append(torch.cat([dgamma, dbeta, coef]))
    assert torch.equal(outs[0], outs[1])
    s = part.double().sum(0)
    dg = wsb[3 * C:].double() * (s[1] - wsb[2 * C:3 * C].double() * s[0])
    # the sums and the difference are taken in fp64 on both sides, in different orders: up to 600 additions, each within 2^-53 of
    # the running sum, i.e. within 2^-43 of sum|x|; 2^-40 leaves a factor of 8
    a = part.double().abs().sum(0)
    dg_a = wsb[3 * C:].double() * (a[1] + wsb[2 * C:3 * C].double().abs() * a[0])
    _close(dbeta, s[0], 1e-6, U40 * a[0], "dbeta")
    _close(dgamma, dg, 1e-6, U40 * dg_a, "dgamma")
    _close(coef, torch.cat([s[0], dg]) / Mrows, 1e-6, U40 * torch.cat([a[0], dg_a]) / Mrows, "coef")
    # column sums: the finalize of a real launch against the float64 sum of that launch's partial slab
    nb = min(nblk, 512)
    M = nb * 256
    assert hipk.ew_blocks(M) == nb
    gbuf, ga, _ = _nan_slice((M,), C, dev, 31)
    cpart = torch.full((nb, 2, C), NAN, device=dev)
    out = torch.full((C,), NAN, device=dev)
    hipk.colsum(ga, M, cpart, out)
    out1 = out.clone()
    _close(out, cpart[:, 0, :].double().sum(0), 1e-6, U40 * cpart[:, 0, :].double().abs().sum(0), "colsum finalize")
    hipk.colsum(ga, M, cpart, out)
    assert torch.equal(out, out1)


@pytest.mark.parametrize("Cs,nblks,pad", [((80, 24, 8, 264), (33, 600, 1, 257), True), ((264, 8), (256, 31), False), ((24, 80, 24), (255, 32, 600), True)])
def test_parts_finalizes_match_single_layer_calls(dev, Cs, nblks, pad):
    """yh_bn_finalize_parts / yh_bn_bwd_finalize_parts with a different slab height per part: bit-identical to the single-layer calls"""
    from yoloseries_amd import hipk
    _RAN["fin_parts"].add((Cs, nblks, pad))
    g = torch.Generator().manual_seed(5)
    count = 4096
    fwd, bwd, keep = [], [], []
    for C, nblk in zip(Cs, nblks):
        ld = (C + 127) // 128 * 128 if pad else C
        slab, _ = _fwd_slab(nblk, C, ld, dev, C + nblk)
        gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
        rm0, rv0 = torch.randn(C, generator=g).to(dev), (torch.rand(C, generator=g) + 0.5).to(dev)
        a = dict(ws=torch.full((4 * C,), NAN, device=dev), rm=rm0.clone(), rv=rv0.clone(), nbt=torch.tensor([41], dtype=torch.int64, device=dev))
        b = dict(ws=torch.full((4 * C,), NAN, device=dev), rm=rm0.clone(), rv=rv0.clone(), nbt=torch.tensor([41], dtype=torch.int64, device=dev))
        hipk.bn_finalize(slab, nblk, ld, C, count, gamma, beta, a["rm"], a["rv"], a["nbt"], EPS, MOM, a["ws"])
        fwd.append(dict(ws=b["ws"], C=C, slab=slab.data_ptr(), nblk=nblk, ldslab=ld, gamma=gamma, beta=beta, running_mean=b["rm"],
                        running_var=b["rv"], num_batches=b["nbt"], eps=EPS, momentum=MOM))
        part = torch.randn(nblk, 2, C, generator=g).to(dev)
        for d in (a, b):
            d.update(dgamma=torch.full((C,), NAN, device=dev), dbeta=torch.full((C,), NAN, device=dev), coef=torch.full((2 * C,), NAN, device=dev))
        hipk.bn_bwd_finalize(part, nblk, C, count, a["ws"], a["dgamma"], a["dbeta"], a["coef"])
        bwd.append(dict(ws=a["ws"], C=C, slab=part.data_ptr(), nblk=nblk, dgamma=b["dgamma"], dbeta=b["dbeta"], coef=b["coef"]))
        keep.append((slab, part, a, b))
    hipk.bn_finalize_parts(fwd, count)
    hipk.bn_bwd_finalize_parts(bwd, count)
    torch.cuda.synchronize()
    for C, (slab, part, a, b) in zip(Cs, keep):
        for k in ("ws", "rm", "rv", "nbt", "dgamma", "dbeta", "coef"):
            assert not a[k].double().isnan().any(), (C, k)
            assert torch.equal(a[k], b[k]), f"part with C={C}: {k} differs from the single-layer call"


# ---------------------------------------------------------------- 4. saturation and special values
ZS = [s * v for v in (0.0, 1e-3, 1.0, 20.0, 87.0, 88.0, 89.0, 100.0, 1e4) for s in (1.0, -1.0)]


@pytest.mark.parametrize("how", ("scale", "shift"))
def test_saturated_silu_and_its_derivative(dev, how):
    """z = y * scale + shift takes every value of ZS in every lane of an 8-channel chunk (channel 8k + e holds ZS[(k + e) % 18]),
    either as y = 1, scale = z or as scale = 0, shift = z.  With gamma = invstd = 1, mean = 0, coef = 0 and g = 1 the backward apply
    writes the derivative factor sg * (1 + z * (1 - sg)) itself and the reduce sums it over the rows."""
    from yoloseries_amd import hipk
    C, M = 8 * len(ZS), 5
    z32 = torch.tensor([ZS[(c // 8 + c % 8) % len(ZS)] for c in range(C)], dtype=torch.float32)
    zero, one = torch.zeros(C), torch.ones(C)
    ws = (torch.cat([z32, zero, zero, one]) if how == "scale" else torch.cat([zero, z32, zero, one])).to(dev)
    ybuf, y, yv = _nan_slice((M,), C, dev, 1)
    if how == "scale":
        ybuf[:, 8:8 + C] = 1.0
        yv = ybuf[:, 8:8 + C].double()
    z = z32.double().to(dev).expand(M, C)
    sg = torch.sigmoid(z)
    act, der = z * sg, sg * (1 + z * (1 - sg))
    lo, hi = (z32 <= -100).to(dev), (z32 >= 100).to(dev)
    obuf, o = _sent_slice((M,), C, dev)
    hipk.bn_silu_apply(y, ws, M, o)
    out = obuf[:, 8:8 + C]
    assert torch.isfinite(out.float()).all()
    _close(out, act, 8e-3, 2e-2, "silu")
    assert (out[:, lo] == 0).all(), "silu(z <= -100) is +-0"
    assert torch.equal(out[:, hi], z32.to(dev).to(BF).expand(M, C)[:, hi]), "silu(z >= 100) is bf16(z)"
    gbuf, ga, _ = _nan_slice((M,), C, dev, 2)
    gbuf[:, 8:8 + C] = 1.0
    gamma = torch.ones(C, device=dev)
    coef = torch.full((2 * C,), NAN, device=dev)
    hipk.fill_u32(coef, 0, 2 * C)
    gybuf, gy = _sent_slice((M,), C, dev)
    hipk.bn_silu_bwd_apply(ga, y, ws, gamma, coef, M, gy)
    d = gybuf[:, 8:8 + C]
    assert torch.isfinite(d.float()).all()
    assert (d[:, lo] == 0).all() and (d[:, hi] == 1).all(), "derivative factor at |z| >= 100"
    _close(d, der, 8e-3, 2e-2, "derivative factor")
    _guard_ok(gybuf, C)
    part = torch.full((1, 2, C), NAN, device=dev)
    hipk.bn_silu_bwd_reduce(ga, y, ws, M, part)
    assert torch.isfinite(part).all()
    assert (part[0, 0, lo] == 0).all() and (part[0, 0, hi] == M).all()
    _close(part[0, 0], der.sum(0), 2e-3, 2e-3 * M, "sum of the derivative factor")
    _close(part[0, 1], (der * yv).sum(0), 2e-3, 2e-3 * M * max(1.0, _mx(yv)), "sum of derivative * y")


def test_one_nan_stays_where_it_is(dev):
    """a NaN in y: exactly one NaN element after the apply passes, exactly its channel's sums after the reduce"""
    from yoloseries_amd import hipk
    C, M, rr, cc = 80, 300, 123, 37
    ybuf, y, yv = _nan_slice((M,), C, dev, 1, 2.0)
    gamma, beta = _params(C, dev, 2)
    ws = _ws_of(yv, gamma, beta, dev)
    ybuf[rr, 8 + cc] = NAN
    gbuf, ga, gv = _nan_slice((M,), C, dev, 3)
    want = torch.zeros(M, C, dtype=torch.bool, device=dev)
    want[rr, cc] = True
    obuf, o = _sent_slice((M,), C, dev)
    hipk.bn_silu_apply(y, ws, M, o)
    assert torch.equal(obuf[:, 8:8 + C].isnan(), want)
    coef = torch.zeros(2 * C, device=dev)
    gybuf, gy = _sent_slice((M,), C, dev)
    hipk.bn_silu_bwd_apply(ga, y, ws, gamma, coef, M, gy)
    assert torch.equal(gybuf[:, 8:8 + C].isnan(), want)
    nblk = hipk.ew_blocks(M)
    part = torch.zeros(nblk, 2, C, device=dev)
    hipk.bn_silu_bwd_reduce(ga, y, ws, M, part)
    dgamma, dbeta, coef = torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(2 * C, device=dev)
    hipk.bn_bwd_finalize(part, nblk, C, M, ws, dgamma, dbeta, coef)
    wc = torch.zeros(C, dtype=torch.bool, device=dev)
    wc[cc] = True
    assert torch.equal(dgamma.isnan(), wc) and torch.equal(dbeta.isnan(), wc) and torch.equal(coef.isnan(), torch.cat([wc, wc]))


# ---------------------------------------------------------------- 5. entry points without a test
@pytest.mark.parametrize("C", (8, 80, 300))
def test_bn_frozen(dev, C):
    """constants from the running statistics against float64; then (C % 8 == 0) the chain of eval-mode training — frozen ws, coef
    zeroed by yh_fill_u32, yh_bn_silu_bwd_apply — against autograd through F.batch_norm(training=False) + F.silu in float64"""
    from yoloseries_amd import hipk
    g = torch.Generator().manual_seed(C)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
    rm, rv = torch.randn(C, generator=g).to(dev), (torch.rand(C, generator=g) + 0.1).to(dev)
    ws = torch.full((4 * C,), NAN, device=dev)
    hipk.bn_frozen(gamma, beta, rm, rv, EPS, C, ws)
    invstd = (rv.double() + EPS).rsqrt()
    scale = gamma.double() * invstd
    _close(ws[:C], scale, 1e-6, 0.0, "scale")
    _close(ws[C:2 * C], beta.double() - rm.double() * scale, 0.0, U22 * torch.maximum(beta.double().abs(), (rm.double() * scale).abs()), "shift")
    assert torch.equal(ws[2 * C:3 * C], rm)
    _close(ws[3 * C:], invstd, 1e-6, 0.0, "invstd")
    if C % 8:
        return
    M = 257
    ybuf, y, yv = _nan_slice((M,), C, dev, 1, 2.0)
    gbuf, ga, gv = _nan_slice((M,), C, dev, 2)
    x = yv.clone().requires_grad_(True)
    a = F.silu(F.batch_norm(x, rm.double(), rv.double(), gamma.double(), beta.double(), False, MOM, EPS))
    (gx,) = torch.autograd.grad(a, x, gv)
    obuf, o = _sent_slice((M,), C, dev)
    hipk.bn_silu_apply(y, ws, M, o)
    _close(obuf[:, 8:8 + C], a.detach(), 8e-3, 2e-2, "eval-mode forward")
    coef = torch.full((2 * C,), NAN, device=dev)
    hipk.fill_u32(coef, 0, 2 * C)
    gybuf, gy = _sent_slice((M,), C, dev)
    hipk.bn_silu_bwd_apply(ga, y, ws, gamma, coef, M, gy)
    _close(gybuf[:, 8:8 + C], gx, 1e-2, 1e-2 * _mx(gx), "eval-mode gy")
    _guard_ok(gybuf, C)


def test_bn_fold_batch(dev):
    """four items (300 and 1024 channels exceed the block's 256 threads), an eps each: bit-identical to four yh_bn_fold calls and
    within rtol 1e-6 of float64.  beta > 0 > running_mean and gamma > 0, so that the shift is a sum of positive terms: a relative
    bar means nothing on a cancelling difference."""
    from yoloseries_amd import hipk
    g = torch.Generator().manual_seed(9)
    items, singles = [], []
    for C, eps in ((8, 1e-3), (80, 1e-5), (300, 1e-4), (1024, 1e-2)):
        eps = float(np.float32(eps))
        q = dict(gamma=(torch.rand(C, generator=g) + 0.5).to(dev), beta=(torch.rand(C, generator=g) + 0.1).to(dev),
                 rm=(-torch.rand(C, generator=g) - 0.1).to(dev), rv=(torch.rand(C, generator=g) + 0.1).to(dev),
                 scale=torch.full((C + 2,), NAN, device=dev)[1:C + 1], shift=torch.full((C + 2,), NAN, device=dev)[1:C + 1], eps=eps)
        items.append(q)
        s1, h1 = torch.full((C,), NAN, device=dev), torch.full((C,), NAN, device=dev)
        hipk.bn_fold(q["gamma"], q["beta"], q["rm"], q["rv"], eps, C, s1, h1)
        singles.append((s1, h1))
    table = hipk.bn_fold_batch(items)
    torch.cuda.synchronize()
    del table
    for q, (s1, h1) in zip(items, singles):
        assert torch.equal(q["scale"], s1) and torch.equal(q["shift"], h1)
        s = q["gamma"].double() / (q["rv"].double() + q["eps"]).sqrt()
        _close(q["scale"], s, 1e-6, 0.0, "scale")
        _close(q["shift"], q["beta"].double() - q["rm"].double() * s, 1e-6, 0.0, "shift")


@pytest.mark.parametrize("n", (0, 1, 255, 257))
def test_fill_u32_value_and_guards(dev, n):
    from yoloseries_amd import hipk
    t = torch.full((n + 8,), 0x11111111, dtype=torch.int32, device=dev)
    hipk.fill_u32(t, 0xDEADBEEF, n, word_off=4)
    assert (t[4:4 + n] == 0xDEADBEEF - (1 << 32)).all()
    assert (t[:4] == 0x11111111).all() and (t[4 + n:] == 0x11111111).all()


# ---------------------------------------------------------------- 7. small companions
@pytest.mark.parametrize("H,W", [(1, 1), (2, 9), (4, 1)])
def test_maxpool5_tiny_maps_and_slices(dev, H, W):
    from yoloseries_amd import hipk
    B, C = 2, 24
    xbuf, x, xv = _nan_slice((B, H, W), C, dev, 3)
    xbuf[..., 8:8 + C] = (xv * 2).round().div(2).to(BF)          # ties: the first maximum in window order wins
    xv = xbuf[..., 8:8 + C].double()
    obuf, o = _sent_slice((B, H, W), C, dev)
    idx = torch.full((B, H, W, C), 99, dtype=torch.int8, device=dev)
    hipk.maxpool5_fwd(x, B, H, W, o, idx)
    xn = xv.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ref = F.max_pool2d(xn, 5, 1, 2)
    assert torch.equal(obuf[..., 8:8 + C].double(), ref.detach().permute(0, 2, 3, 1))
    _guard_ok(obuf, C)
    o2buf, o2 = _sent_slice((B, H, W), C, dev)
    hipk.maxpool5_fwd(x, B, H, W, o2, None)                         # no arg-max wanted
    assert torch.equal(o2buf.view(torch.int16), obuf.view(torch.int16))
    gbuf, go, gov = _nan_slice((B, H, W), C, dev, 4)
    (gref,) = torch.autograd.grad(ref, xn, gov.permute(0, 3, 1, 2))
    gibuf, gi = _sent_slice((B, H, W), C, dev)
    hipk.maxpool5_bwd(go, idx, B, H, W, gi, 0)
    _close(gibuf[..., 8:8 + C], gref.permute(0, 2, 3, 1), 8e-3, 2e-2, "maxpool5_bwd")
    _guard_ok(gibuf, C)


def test_maxpool5_all_minus_inf(dev):
    """as torch does it: output -inf, the arg-max stays at the first window position inside the image — position 0 wherever the
    window's corner (h - 2, w - 2) lies inside — and the backward routes each gradient there"""
    from yoloseries_amd import hipk
    B, H, W, C = 1, 6, 7, 8
    xbuf = torch.full((B, H, W, C + 16), NAN, dtype=BF, device=dev)
    xbuf[..., 8:8 + C] = float("-inf")
    obuf, o = _sent_slice((B, H, W), C, dev)
    idx = torch.full((B, H, W, C), 99, dtype=torch.int8, device=dev)
    hipk.maxpool5_fwd(hipk.Slice(xbuf, 8, C), B, H, W, o, idx)
    assert (obuf[..., 8:8 + C] == float("-inf")).all()
    _guard_ok(obuf, C)
    first = (2 - torch.arange(H).view(H, 1)).clamp(min=0) * 5 + (2 - torch.arange(W).view(1, W)).clamp(min=0)
    assert torch.equal(idx, first.to(torch.int8).view(1, H, W, 1).expand(B, H, W, C).to(dev))
    assert (idx[:, 2:, 2:] == 0).all()
    gbuf, go, gov = _nan_slice((B, H, W), C, dev, 4)
    gibuf, gi = _sent_slice((B, H, W), C, dev)
    hipk.maxpool5_bwd(go, idx, B, H, W, gi, 0)
    xn = xbuf[..., 8:8 + C].double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    (gref,) = torch.autograd.grad(F.max_pool2d(xn, 5, 1, 2), xn, gov.permute(0, 3, 1, 2))
    gref = gref.permute(0, 2, 3, 1)
    _close(gibuf[..., 8:8 + C], gref, 8e-3, 2e-2, "maxpool5_bwd")
    assert torch.equal(gibuf[:, :H - 2, :W - 2, 8:8 + C][:, 1:, 1:].double(), gov[:, 3:, 3:]), "interior: out(h, w) -> in(h - 2, w - 2) only"
    _guard_ok(gibuf, C)


@pytest.mark.parametrize("C", (8, 24))
@pytest.mark.parametrize("Hlo,Wlo", [(1, 1), (3, 5)])
def test_upsample2_bwd_overwrite_and_slices(dev, Hlo, Wlo, C):
    from yoloseries_amd import hipk
    B = 2
    hbuf, ghi, hv = _nan_slice((B, 2 * Hlo, 2 * Wlo), C, dev, 5)
    ref = hv.reshape(B, Hlo, 2, Wlo, 2, C).sum((2, 4))
    lbuf, glo = _sent_slice((B, Hlo, Wlo), C, dev)
    hipk.upsample2_bwd(ghi, B, Hlo, Wlo, glo, 0)
    _close(lbuf[..., 8:8 + C], ref, 8e-3, 2e-2, "overwrite")
    _guard_ok(lbuf, C)
    abuf, acc, av = _nan_slice((B, Hlo, Wlo), C, dev, 6)
    hipk.upsample2_bwd(ghi, B, Hlo, Wlo, acc, 1)
    _close(abuf[..., 8:8 + C], ref + av, 8e-3, 2e-2, "accumulate")
    assert abuf[..., :8].isnan().all() and abuf[..., 8 + C:].isnan().all()


@pytest.mark.parametrize("Cin,H,W", [(1, 6, 10), (4, 6, 10), (3, 2, 2)])
def test_input_s2d_channel_counts(dev, Cin, H, W):
    from yoloseries_amd import hipk
    B = 2
    x = torch.rand(B, Cin, H, W, device=dev)
    out = torch.full((B, H // 2, W // 2, 16), SENT, dtype=BF, device=dev)
    hipk.input_s2d(x, out)
    assert torch.equal(out[..., :4 * Cin], _s2d_ref(x)) and (out[..., 4 * Cin:] == 0).all()


def test_zz_every_case_ran():
    """no case of the ragged-width, grid-pass and slab-walk sections hides behind a skip or a typo in a parameter list"""
    assert _RAN["ragged"] == {(C, M) for C in RAGGED_C for M in RAGGED_M} and len(_RAN["ragged"]) == 36
    assert _RAN["parts"] == {(Cs, M) for Cs in PARTS for M in (7, 1000)}
    assert _RAN["grid_apply"] == set(GRID_APPLY) and _RAN["grid_reduce"] == set(GRID_REDUCE)
    assert _RAN["grid_misc"] == {"pool", "upsample", "s2d", "fill"}
    assert _RAN["fin"] == {(n, C, p) for n in FIN_NBLK for C in FIN_C for p in (False, True)} and len(_RAN["fin"]) == 64
    assert len(_RAN["fin_parts"]) == 3
