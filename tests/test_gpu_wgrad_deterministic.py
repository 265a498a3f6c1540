"""The workspace form of conv_wgs_kernel (yh_wgrad_desc.partial with tile_k 129): the stream-K weight gradient leaves its kernel by
plain stores into slot v + t of a workspace (v: virtual workgroup, t: tile) and wgs_reduce_kernel adds the slots of every tile to
dw in ascending v — bit-reproducible, on the kernel family the default mode uses.

Shapes: B = 2 on a 16 x 16 output map (M = 512 pixels = 16 units of 32), the smallest at which every path of the form runs: one
tile / many ragged tiles, workgroups that span several tiles, exact grids, several workgroups per tile, segments that straddle tile
boundaries, more workgroups than units (the clamp).  Reference: the fp32 torch weight gradient of the same bf16 values, held to the
bar tests/test_gpu_conv.py::test_conv_wgrad_wave_private_tiles holds the atomic form to (2e-3 relative + 2e-3 of the largest
element).  Bit identity: 20 launches into a re-initialised dw beside a busy second stream, every result equal to the first."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SLOT = 128 * 128 * 4
GUARD = 256          # floats behind the advertised workspace size that must stay untouched

# name: (B, H, W, Cin, Cout, k, stride, coff, Ctot, ups), workgroup counts
CASES = {
    "one_tile_pw": ((2, 16, 16, 128, 128, 1, 1, 0, 128, 0), (1, 3, 16)),
    # 2 n-tiles x 7 column tiles = 14 tiles; rows 200..255 of the second n-tile and columns 864..895 of the last column tile are dead
    "ragged_3x3": ((2, 16, 16, 96, 200, 3, 1, 0, 96, 0), (5, 14, 28, 37, 4096)),
    "stride2": ((2, 32, 32, 64, 128, 3, 2, 0, 64, 0), (7,)),
    "upsampled": ((2, 16, 16, 64, 128, 3, 1, 0, 64, 1), (5,)),
    "segment_of_concat": ((2, 16, 16, 64, 128, 1, 1, 64, 192, 0), (3,)),
}
PARAMS = [(n, g) for n, (_, gs) in CASES.items() for g in gs]


def _nhwc(shape, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).to(dev)


def _nchw(x):
    return x.float().permute(0, 3, 1, 2).contiguous()


def _close(got, ref, rtol, atol, what=""):
    err = (got.float() - ref).abs()
    bad = err > atol + rtol * ref.abs()
    print(f"{what}: max err {err.max().item():.4g}, ref max {ref.abs().max().item():.4g}, bar {atol:.4g} + {rtol:g} |ref|")
    assert not bad.any(), f"{what}: max err {err.max().item():.4g} (ref max {ref.abs().max().item():.4g}), {bad.sum().item()} / {bad.numel()} out of tol"


def _pattern(rows, cols, dev):
    """the nonzero content dw holds before a launch"""
    i = torch.arange(rows * cols, device=dev, dtype=torch.float32).reshape(rows, cols)
    return 0.25 + (i % 13) * 0.03125 - (i % 7) * 0.0625


class _Layer:
    """operands of one case (computed once per module), its descriptor and the fp32 reference [Cout][k][k][Cin]"""

    def __init__(self, dev, case, seed):
        from yoloseries_amd import hipk
        B, H, W, Cin, Cout, k, s, coff, Ctot, ups = case
        p = k // 2
        self.case, self.p = case, p
        self.Ho, self.Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        ldg = (Cout + 7) // 8 * 8
        self.gy = torch.zeros(B, self.Ho, self.Wo, ldg, dtype=torch.bfloat16, device=dev)
        self.gy[..., :Cout] = _nhwc((B, self.Ho, self.Wo, Cout), dev, seed)
        self.x = _nhwc((B, H >> ups, W >> ups, Cin), dev, seed + 1)
        xin = _nchw(self.x)
        if ups:
            xin = F.interpolate(xin, scale_factor=2, mode="nearest")
        w = torch.zeros(Cout, Cin, k, k, device=dev, requires_grad=True)
        (ref,) = torch.autograd.grad(F.conv2d(xin, w, stride=s, padding=p), w, _nchw(self.gy[..., :Cout]))
        self.ref = ref.permute(0, 2, 3, 1).contiguous()
        self.pat = _pattern(Cout, k * k * Ctot, dev)
        self.hipk = hipk

    def desc(self, dw, G, coff=None):
        B, H, W, Cin, Cout, k, s, coff0, Ctot, ups = self.case
        hipk = self.hipk
        d = hipk.wgrad_desc(hipk.full(self.gy), Cout, hipk.Slice(self.x, 0, Cin, ups=ups), coff0 if coff is None else coff, Ctot,
                            B, self.Ho, self.Wo, H, W, k, s, self.p, dw, G)
        d.tile_k = 129
        return d


@pytest.fixture(scope="module")
def layers(dev):
    return {n: _Layer(dev, c, 100 + 10 * i) for i, (n, (c, _)) in enumerate(CASES.items())}


@pytest.fixture(scope="module")
def busy(dev):
    """copies and matmuls on a second stream next to every launch (tools/race_screen.py: the conditions of the two-stream step)"""
    side = torch.cuda.Stream(device=dev)
    big = torch.empty(1 << 27, dtype=torch.uint8, device=dev)
    mm = (torch.randn(1024, 1024, device=dev), torch.randn(1024, 1024, device=dev))

    def run():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                big[:1 << 26].copy_(big[1 << 26:])
                mm[0] @ mm[1]
    yield run
    torch.cuda.synchronize()


def _plan(L, d, G):
    """tiles, effective workgroups and slot bytes of a launch, restated from the kernel's header"""
    B, Ho, Wo = d.B, d.Ho, d.Wo
    T = ((d.N + 127) // 128) * ((d.KH * d.KW * d.seg.C + 127) // 128)
    U = T * (B * Ho * Wo // 32)
    Ge = min(max(G, 1), 4096, U)
    return T, Ge, (Ge + T - 1) * SLOT


def _ws(dev, need):
    ws = torch.full((need // 4 + GUARD,), float("nan"), device=dev)
    return ws


def _nan_bits_intact(t):
    return bool((t.view(torch.int32) == torch.full((1,), float("nan"), device=t.device).view(torch.int32)).all())


@pytest.mark.parametrize("name,G", PARAMS)
def test_workspace_form_values_bounds_and_bit_identity(dev, layers, busy, name, G):
    from yoloseries_amd import hipk
    from yoloseries_amd._lib import lib
    L = lib()
    ly = layers[name]
    B, H, W, Cin, Cout, k, s, coff, Ctot, ups = ly.case
    dw = ly.pat.clone()
    d = ly.desc(dw, G)
    T, Ge, need = _plan(L, d, G)
    d.partial, d.partial_bytes = 16, 1 << 40                       # the queries look at the form, not at the pointer
    # (these three fail without the workspace form: the descriptor was ineligible, the name empty, the size the split-M formula)
    assert L.yh_conv_wgrad_wave_tiles(C.byref(d)) == T
    nm = L.yh_conv_wgrad_wave_name(C.byref(d)).decode()
    assert nm == ("conv_wgs_kernel<true, true>" if (k == 1 and s == 1 and not ups) else "conv_wgs_kernel<false, true>"), nm
    assert L.yh_conv_wgrad_ws_bytes(C.byref(d)) == need, (L.yh_conv_wgrad_ws_bytes(C.byref(d)), need, T, Ge)
    ws = _ws(dev, need)
    d.partial, d.partial_bytes = ws.data_ptr(), need
    first = None
    for rep in range(20):
        dw.copy_(ly.pat)
        ws.fill_(float("nan"))                                      # a slot that is read but was never written shows as NaN
        busy()
        hipk.wgrad_launch(d)
        torch.cuda.synchronize()
        if first is None:
            first = dw.clone()
            assert not torch.isnan(dw).any()
            got = dw.reshape(Cout, k, k, Ctot)
            _close(got[..., coff:coff + Cin] - ly.pat.reshape(Cout, k, k, Ctot)[..., coff:coff + Cin], ly.ref, 2e-3,
                   2e-3 * ly.ref.abs().max().item(), f"{name} G={G}")
            mask = torch.ones(Ctot, dtype=torch.bool, device=dev)
            mask[coff:coff + Cin] = False
            assert torch.equal(got[..., mask], ly.pat.reshape(Cout, k, k, Ctot)[..., mask])    # the other segments' columns: untouched
        else:
            assert torch.equal(dw, first), f"{name} G={G}: launch {rep} differs from the first in {(dw != first).sum().item()} elements"
        assert _nan_bits_intact(ws[need // 4:])                     # nothing written behind the advertised size
    # slot v + t of every (workgroup, tile) pair whose unit range intersects was written whole; the other slots of the G + T - 1
    # (an exact grid uses T of them: no workgroup straddles a tile boundary) were not touched
    nk = B * ly.Ho * ly.Wo // 32
    used = {v + u // nk for v in range(Ge) for u in range(T * nk * v // Ge, T * nk * (v + 1) // Ge)}
    assert max(used) <= Ge + T - 2
    slots = ws[:need // 4].reshape(Ge + T - 1, SLOT // 4)
    for sl in range(Ge + T - 1):
        if sl in used:
            assert not torch.isnan(slots[sl]).any(), f"slot {sl} has unwritten elements"
        else:
            assert _nan_bits_intact(slots[sl]), f"slot {sl} belongs to no (workgroup, tile) pair but was written"


def test_workspace_too_small_or_unaligned_is_refused_and_launches_nothing(dev, layers):
    from yoloseries_amd._lib import lib
    L = lib()
    ly = layers["ragged_3x3"]
    dw = ly.pat.clone()
    d = ly.desc(dw, 28)
    _, _, need = _plan(L, d, 28)
    ws = _ws(dev, need)
    for ptr, nbytes in ((ws.data_ptr(), need - 4), (ws.data_ptr() + 4, need)):
        d.partial, d.partial_bytes = ptr, nbytes
        assert L.yh_conv_wgrad(C.byref(d), None) == -1              # YH_EINVAL
        torch.cuda.synchronize()
        assert torch.equal(dw, ly.pat) and _nan_bits_intact(ws)


def test_two_segments_share_dw_and_workspace(dev, busy):
    """a layer over a two-segment concat: two launches (coff_k 0 and C) into one dw, stream-ordered, sharing one workspace"""
    from yoloseries_amd import hipk
    from yoloseries_amd._lib import lib
    L = lib()
    Cin, Cout, k = 64, 128, 3
    segs = [_Layer(dev, (2, 16, 16, Cin, Cout, k, 1, c, 2 * Cin, 0), 300 + c) for c in (0, Cin)]
    segs[1].gy = segs[0].gy                                          # one output gradient, two input segments
    xin = _nchw(torch.cat([segs[0].x, segs[1].x], dim=-1))
    w = torch.zeros(Cout, 2 * Cin, k, k, device=dev, requires_grad=True)
    (ref,) = torch.autograd.grad(F.conv2d(xin, w, padding=1), w, _nchw(segs[0].gy[..., :Cout]))
    ref = ref.permute(0, 2, 3, 1).reshape(Cout, -1)
    pat = segs[0].pat
    dw = pat.clone()
    ds = [sg.desc(dw, G) for sg, G in zip(segs, (6, 11))]
    need = max(_plan(L, d, G)[2] for d, G in zip(ds, (6, 11)))
    ws = _ws(dev, need)
    for d in ds:
        d.partial, d.partial_bytes = ws.data_ptr(), need
    first = None
    for rep in range(20):
        dw.copy_(pat)
        ws.fill_(float("nan"))
        busy()
        for d in ds:
            hipk.wgrad_launch(d)
        torch.cuda.synchronize()
        if first is None:
            first = dw.clone()
            _close(dw - pat, ref, 2e-3, 2e-3 * ref.abs().max().item(), "two segments")
        else:
            assert torch.equal(dw, first), rep
        assert _nan_bits_intact(ws[need // 4:])


# ---- engine -----------------------------------------------------------------------------------------------------------------------

def _passes(m, x, n):
    """n forward + backward passes on fixed inputs: the flat gradient of every parameter after each"""
    out = []
    for _ in range(n):
        for p_ in m.parameters():
            p_.grad = None
        sum((o.float() ** 2).mean() for o in m(x)).backward()
        torch.cuda.synchronize()
        out.append(m._yh_last_flat_grad.clone())
    return out


def _wgrad_launches(m):
    (prog,) = m._yh_state()['progs'].values()
    return prog, [(c[1].name, c[3][0], int(c[2].splits), int(c[2].tile_k)) for c in prog.cmd_bwd if c[0] == 'wgrad']


def _v5s(dev):
    from yoloseries_amd import models
    torch.manual_seed(0)
    m = models.YOLOV5Small(3, 80).to(dev).train()
    x = torch.rand(4, 3, 128, 128, generator=torch.Generator().manual_seed(5)).to(dev)
    return m, x


def test_engine_keeps_the_wave_tile_kernel_in_deterministic_mode(dev, monkeypatch):
    """YOLOv5s at 4 x 128^2 with set_deterministic(True) and the launch-parameter timing replaced by a fixed rule — tile_k 129 on 48
    workgroups wherever the form is eligible — so that the check does not depend on which candidate a box times fastest: those
    launches carry the workspace form's names, and every parameter gradient is bit-identical over five passes"""
    import yoloseries_amd
    from yoloseries_amd import engine
    from yoloseries_amd._lib import lib
    L = lib()
    orig = engine.Program._tune_wgrad_splits
    forced = []

    def rule(self, wd, M, ntile, op):
        wd.tile_k, wd.splits = 129, 48
        if wd.partial and not wd.bn_z and L.yh_conv_wgrad_wave_tiles(C.byref(wd)) > 0 and \
                L.yh_conv_wgrad_ws_bytes(C.byref(wd)) <= wd.partial_bytes:
            forced.append((op.name, wd.coff_k))
            return 48
        wd.tile_k = 0
        return orig(self, wd, M, ntile, op)
    monkeypatch.setattr(engine.Program, "_tune_wgrad_splits", rule)
    yoloseries_amd.set_deterministic(True)
    try:
        m, x = _v5s(dev)
        grads = _passes(m, x, 5)
        prog, launches = _wgrad_launches(m)
        assert prog.bwd_deterministic and prog.wg_ws is not None
        wave = [ln for ln in launches if ln[3] == 129]
        assert len(wave) == len(forced) >= 20, (len(wave), len(forced))
        assert all(ln[1] in ("conv_wgs_kernel<true, true>", "conv_wgs_kernel<false, true>") for ln in wave), wave[:4]
        # the shared workspace is what the largest launch needs, not the cap
        assert prog.wg_ws.numel() * 4 < engine.flags.WG_WS_CAP
        assert all(torch.isfinite(g).all() for g in grads) and grads[0].abs().max() > 0
        for i, g in enumerate(grads[1:]):
            assert torch.equal(g, grads[0]), f"pass {i + 1}: {(g != grads[0]).sum().item()} gradient elements differ"
    finally:
        yoloseries_amd.set_deterministic(False)


def test_engine_set_deterministic_rebuilds_and_restores_the_default_launch_list(dev):
    """as a user gets it (timed launch parameters): a model whose backward was built in the default mode rebuilds it after
    set_deterministic(True) — bit-identical gradients over five passes, close to the default mode's — and after
    set_deterministic(False) launches exactly what it launched before"""
    import yoloseries_amd
    from yoloseries_amd import engine
    m, x = _v5s(dev)
    try:
        g_def = _passes(m, x, 1)[0]
        prog, before = _wgrad_launches(m)
        assert not prog.bwd_deterministic and prog.wg_ws is None
        assert not any(ln[1].endswith(", true>") and ln[1].startswith("conv_wgs") for ln in before)
        yoloseries_amd.set_deterministic(True)
        assert engine.flags.WG_WS_BYTES == engine.flags.WG_WS_CAP and not prog.bwd_ready
        grads = _passes(m, x, 5)
        prog2, det = _wgrad_launches(m)
        assert prog2 is prog and prog.bwd_deterministic and prog.wg_ws is not None
        assert [ln[0] for ln in det] == [ln[0] for ln in before]
        for i, g in enumerate(grads[1:]):
            assert torch.equal(g, grads[0]), f"pass {i + 1}: {(g != grads[0]).sum().item()} gradient elements differ"
        # the two modes differ by fp32 summation order only (the bar tests/test_gpu_dist.py holds two default runs to)
        assert (grads[0] - g_def).abs().max() <= 1e-3 * g_def.abs().max()
    finally:
        yoloseries_amd.set_deterministic(False)
    assert engine.flags.WG_WS_BYTES == 0 and not prog.bwd_ready
    _passes(m, x, 1)
    assert _wgrad_launches(m)[1] == before
