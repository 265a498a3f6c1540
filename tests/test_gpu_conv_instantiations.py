"""Every kernel instantiation yh_conv_igemm can launch, run once against float64 torch.

One case per row of tools/conv_rows.py (tests/test_host_logic.py checks on the host that the rows cover every name the planner
emits): the smallest descriptor whose plan names the instantiation — B >= 2, an image boundary inside a pixel tile, M no multiple of
the tile, ragged N, the fewest input channels.  Before every launch yh_conv_info must name the row's instantiation.

Operands are built so that a defect shows as a wrong value: inputs are channel slices of wider NaN-filled buffers with 256 NaN rows
before and after them; outputs are channel slices of wider sentinel-filled buffers followed by 64 sentinel rows; both slabs have
sentinel rows past the rows the plan announces.  Nothing outside the advertised extent may change.

Reference: the same operation in float64 (F.conv2d, torch.autograd.grad for the data gradient) on the identical bf16-representable
operands, the epilogue of include/yolohip.h on top.  Bars, those of tests/test_gpu_conv.py: forward 8e-3 relative + 2e-2; with a
residual or accumulation 1e-2 + 3e-2; data gradient 1e-2 + 4e-2.  Partial sums against float64 sums of the STORED values:
statistics within the rounding noise of the stored tensor (the bounds of tests/test_gpu_tune_table.py), the fused reduction within
2e-3 (conv_rows.silu_bwd_sums_close, shared with test_gpu_conv.py::_dgrad_check).

Persistent walk: every row whose family honours grid_cap runs again with grid_cap 1 and 2 (one block walks all pixel tiles / half
of them): outputs bit-identical to the uncapped launch (include/yolohip.h, at tile_n / grid_cap), exactly the announced slab rows."""
import ctypes as C
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conv_rows():
    spec = importlib.util.spec_from_file_location("conv_rows", os.path.join(ROOT, "tools", "conv_rows.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _conv_rows()
PAD = R.PAD
GUARD = 256            # NaN rows before and after every input: one pixel tile of the widest kernel
TAIL = 64              # sentinel rows after every output
SENT = 7.0             # sentinel of the bf16 outputs
SLAB_SENT = -777.0     # sentinel of the fp32 slabs
_RAN = set()
BF16 = torch.bfloat16


def _info(d):
    from yoloseries_amd._lib import ConvInfo, lib
    o = ConvInfo()
    rc = lib().yh_conv_info(C.byref(d), C.byref(o))
    return rc, o.name.decode(), o.stat_rows, o.bnr_rows


def _close(got, ref, rtol, atol, what):
    err = (got.double() - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: max err {err.max().item():.4g} (ref max {ref.abs().max().item():.4g}), {int(bad.sum())} of {bad.numel()} out of tolerance"


class _Operands:
    """inputs, weights, epilogue operands and the float64 result of a row: made once per test, shared by all its launches"""

    def __init__(self, r, dev, seed):
        from yoloseries_amd import hipk
        self.r, self.dev = r, dev
        g = self.g = torch.Generator(device=dev).manual_seed(seed)
        Hi, Wi = r.in_hw
        self.M = M = r.B * r.H * r.W
        N = r.N
        self.segs, self.keep, xs = [], [], []
        for Cs, ld, ups in r.seg_list:
            h, w = Hi >> ups, Wi >> ups
            flat = torch.full((GUARD + r.B * h * w + GUARD, ld), float("nan"), dtype=BF16, device=dev)
            x = torch.randn(r.B, h, w, Cs, generator=g, device=dev).to(BF16)
            view = flat[GUARD:GUARD + r.B * h * w].view(r.B, h, w, ld)
            view[..., PAD:PAD + Cs] = x
            self.segs.append(hipk.Slice(view, PAD, Cs, ups))
            self.keep.append(flat)
            xs.append(x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if ups else x)
        xin = torch.cat(xs, 3).double().permute(0, 3, 1, 2)
        Ctot = xin.shape[1]
        if r.mode == R.F:
            w = (torch.randn(N, Ctot, r.k, r.k, generator=g, device=dev) / (Ctot * r.k * r.k) ** 0.5).to(BF16).float()
            self.wp = hipk.pack_weight_fwd(w)
            acc = F.conv2d(xin, w.double(), stride=r.stride, padding=r.pad)
        else:
            w = (torch.randn(Ctot, N, r.k, r.k, generator=g, device=dev) / (Ctot * r.k * r.k) ** 0.5).to(BF16).float()
            self.wp = hipk.pack_weight_dgrad(w)
            x0 = torch.zeros(r.B, N, r.H, r.W, dtype=torch.float64, device=dev, requires_grad=True)
            (acc,) = torch.autograd.grad(F.conv2d(x0, w.double(), stride=r.stride, padding=r.pad), x0, xin)
        assert tuple(acc.shape) == (r.B, N, r.H, r.W)
        v = acc.permute(0, 2, 3, 1).reshape(M, N)
        c = r.case()
        self.n0 = n0 = r.nsplit
        self.bias = torch.randn(N, generator=g, device=dev) if c["bias"] else None
        self.scale = torch.rand(N, generator=g, device=dev) + 0.5 if c["scale"] else None
        self.shift = torch.randn(N, generator=g, device=dev) * 0.5 if c["shift"] else None
        self.res = None
        if self.bias is not None:
            v = v + self.bias.double()
        if self.scale is not None:
            v = v * self.scale.double() + self.shift.double()
        if c["act"]:
            v = v * torch.sigmoid(v)
        if c["res"]:
            self.res = torch.zeros(M, c["ldr"], dtype=BF16, device=dev)
            self.res[:, :n0] = torch.randn(M, n0, generator=g, device=dev).to(BF16)
            v = v.clone()
            v[:, :n0] += self.res[:, :n0].double()
        self.ref = v                                              # [M][N] float64: what a launch without accumulation stores
        self.prior = torch.randn(M, N, generator=g, device=dev).to(BF16)          # what an accumulating launch finds in the destination
        if r.epi == "bnr":
            self.z = torch.randn(M, c["bnr_ldz"], generator=g, device=dev).to(BF16)
            self.ws = torch.zeros(2 * c["bnr_C"], device=dev)
            self.ws[:N] = torch.rand(N, generator=g, device=dev) + 0.5
            self.ws[c["bnr_C"]:c["bnr_C"] + N] = torch.randn(N, generator=g, device=dev)

    def launch(self, grid_cap=0, accumulate=None, bnr=None, must_be_row=True):
        """one launch of the row's descriptor into fresh sentinel-filled destinations -> (both destination buffers, stored [M][N],
        slab or None, instantiation name); accumulate / bnr override the row's epilogue"""
        from yoloseries_amd import hipk
        from yoloseries_amd._lib import YH_ACT_NONE, YH_ACT_SILU
        r, dev, M, N, n0 = self.r, self.dev, self.M, self.r.N, self.n0
        c = r.case()
        accumulate = bool(c["accumulate"]) if accumulate is None else accumulate
        bnr = bool(c["bnr"]) if bnr is None else bnr
        Hi, Wi = r.in_hw
        bufs = [torch.full((M + TAIL, n0 + 2 * PAD), SENT, dtype=BF16, device=dev)]
        if n0 < N:
            bufs.append(torch.full((M + TAIL, N - n0 + 2 * PAD), SENT, dtype=BF16, device=dev))
        widths = [n0, N - n0][:len(bufs)]
        if accumulate:
            bufs[0][:M, PAD:PAD + n0] = self.prior[:, :n0]
            if n0 < N:
                bufs[1][:M, PAD:PAD + N - n0] = self.prior[:, n0:]
        init = [b.clone() for b in bufs]
        d = hipk.conv_desc(self.segs, r.mode, r.B, r.H, r.W, Hi, Wi, r.k, r.stride, r.pad, self.wp, N, hipk.Slice(bufs[0], PAD, n0), nsplit=n0,
                           out1=hipk.Slice(bufs[1], PAD, N - n0) if n0 < N else None, bias=self.bias, scale=self.scale, shift=self.shift,
                           act=YH_ACT_SILU if c["act"] else YH_ACT_NONE, accumulate=int(accumulate),
                           res=hipk.Slice(self.res, 0, n0) if self.res is not None else None)
        d.tile_n, d.tile_k, d.algo, d.grid_cap = r.tile_n, r.tile_k, r.algo, grid_cap
        slab = None
        if c["stats"]:
            d.stats = self.wp.data_ptr()                    # placeholder: the plan only looks at null / non-null
            rows = _info(d)[2]
            assert rows > 0
            slab = torch.full((rows + 2, 2, self.wp.shape[0]), SLAB_SENT, device=dev)
            d.stats = slab.data_ptr()
        if bnr:
            d.bnr_z, d.bnr_ldz, d.bnr_C, d.bnr_ws = self.z.data_ptr(), c["bnr_ldz"], c["bnr_C"], self.ws.data_ptr()
            d.bnr_part = self.ws.data_ptr()                 # placeholder: the row count only looks at null / non-null
            rows = _info(d)[3]
            assert rows > 0
            slab = torch.full((rows + 2, 2, N), SLAB_SENT, device=dev)
            d.bnr_part = slab.data_ptr()
        rc, name, stat_rows, bnr_rows = _info(d)
        assert rc == 0 and name, (r.id, rc, name)
        if must_be_row:
            assert name == r.name, f"{r.id}: planned to {name}"          # a row never silently falls through to another kernel
        if slab is not None:
            assert slab.shape[0] - 2 == (stat_rows if c["stats"] else bnr_rows)
        hipk.conv_launch(d)
        torch.cuda.synchronize()
        # nothing outside the advertised extent changed: channels beside the slice, rows after it, slab rows past the announced ones
        for b, b0, wdt in zip(bufs, init, widths):
            rest = b.clone()
            rest[:M, PAD:PAD + wdt] = b0[:M, PAD:PAD + wdt]
            assert torch.equal(rest, b0), f"{r.id}: wrote outside its destination slice"
        if slab is not None:
            assert (slab[-2:] == SLAB_SENT).all(), f"{r.id}: wrote past the {slab.shape[0] - 2} slab rows the plan announces"
            assert not (slab[:-2, :, :N] == SLAB_SENT).any(), f"{r.id}: a slab row of the {slab.shape[0] - 2} announced was not written"
            slab = slab[:-2, :, :N]
        stored = torch.cat([b[:M, PAD:PAD + wdt] for b, wdt in zip(bufs, widths)], 1)
        return bufs, stored, slab, name

    def check_output(self, stored, accumulate, what):
        r, n0 = self.r, self.n0
        ref = self.ref + self.prior.double() if accumulate else self.ref
        if r.mode == R.D:
            _close(stored, ref, 1e-2, 4e-2, what)
        elif accumulate:
            _close(stored, ref, 1e-2, 3e-2, what)
        else:
            loose = self.res is not None          # the residual's columns (the first destination) carry a second rounding
            _close(stored[:, :n0], ref[:, :n0], *((1e-2, 3e-2) if loose else (8e-3, 2e-2)), what)
            _close(stored[:, n0:], ref[:, n0:], 8e-3, 2e-2, what + " (second destination)")

    def check_stats(self, slab, stored, what):
        """BatchNorm partial sums against float64 sums of the stored values: some families sum the fp32 accumulators, others the stored
        values — both within the rounding noise of the stored tensor (per element <= 2^-9 |v|, random sign: a random walk of
        2^-9 sqrt(sum v^2), 3.5 sigma; the sum of squares carries 2 v e), the bounds of tests/test_gpu_tune_table.py"""
        o = stored.double()
        o2 = o * o
        so, so2 = o.sum(0), o2.sum(0)
        s1, s2 = slab[:, 0].double().sum(0), slab[:, 1].double().sum(0)
        n1 = 2.0 ** -9 * so2.sqrt() * 3.5 + 1e-2
        n2 = 2.0 ** -8 * (o2 * o2).sum(0).sqrt() * 3.5 + 1e-2
        assert ((s1 - so).abs() <= n1 + 1e-5 * o.abs().sum(0)).all(), f"{what}: sum {(s1 - so).abs().max().item():.4g} vs noise bound {n1.max().item():.4g}"
        assert ((s2 - so2).abs() <= n2 + 1e-5 * so2).all(), f"{what}: sum of squares {(s2 - so2).abs().max().item():.4g} vs {n2.max().item():.4g}"

    def check_bnr(self, slab, stored, what):
        N, bC = self.r.N, self.ws.numel() // 2
        assert R.silu_bwd_sums_close(slab, stored, self.z[:, :N], self.ws[:N], self.ws[bC:bC + N]), what

    def check_slab(self, slab, stored, what):
        if self.r.epi in ("stats", "gstats"):
            self.check_stats(slab, stored, what)
        elif slab is not None:
            self.check_bnr(slab, stored, what)


@pytest.mark.parametrize("row", R.ROWS, ids=[r.id for r in R.ROWS])
def test_conv_instantiation(dev, row):
    r = row
    ops = _Operands(r, dev, 4000 + R.ROWS.index(r))
    own_acc = r.epi == "acc"
    bufs, stored, slab, _ = ops.launch()
    ops.check_output(stored, own_acc, r.id)
    ops.check_slab(slab, stored, r.id)
    if r.epi == "bnr":
        # the fused reduction as the LAST of several writers: what is already in the buffer is added, bit-identical to the accumulating
        # generic epilogue of the family, and the sums are taken over the rounded total
        _, acc_only, _, acc_name = ops.launch(accumulate=True, bnr=False, must_be_row=False)
        assert acc_name.split("<")[0] == r.name.split("<")[0], (r.id, acc_name)
        _, last, slab2, _ = ops.launch(accumulate=True)
        assert torch.equal(last, acc_only), f"{r.id}: last-writer form differs from the accumulating epilogue ({acc_name})"
        ops.check_output(last, True, r.id + " accumulating")
        ops.check_bnr(slab2, last, r.id + " accumulating")
    elif r.mode == R.F and r.epi in ("full", "one", "nores", "bn"):
        # the generic epilogue accumulating on top of what the destination holds, where that is still this instantiation
        probe = r.case(accumulate=1)
        if R.plan(_lib(), probe)[:2] == (0, r.name):
            _, acc2, _, _ = ops.launch(accumulate=True)
            ops.check_output(acc2, True, r.id + " accumulating")
    if r.cap:
        # persistent walk: one block walks every pixel tile (grid_cap 1) / half of them (2); the sums regroup, the output does not change
        for cap in (1, 2):
            cbufs, cstored, cslab, _ = ops.launch(grid_cap=cap)
            for a, b in zip(cbufs, bufs):
                assert torch.equal(a, b), f"{r.id}: grid_cap {cap} changes the output"
            ops.check_slab(cslab, cstored, f"{r.id} grid_cap {cap}")
    _RAN.add(r.id)


def _lib():
    from yoloseries_amd._lib import lib
    return lib()


def test_zz_every_row_ran():
    """no row hides behind a deselection, a skip or a typo: every row of tools/conv_rows.py ran to its end"""
    missing = [r.id for r in R.ROWS if r.id not in _RAN]
    assert not missing, missing
