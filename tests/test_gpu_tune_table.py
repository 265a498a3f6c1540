"""GPU parity of the kernels AT THE JUDGED SHAPES WITH THE SHIPPED LAUNCH TABLE: every training entry of
yoloseries_amd/tune_defaults.json — the (algo, tile_k, grid_cap) of the forward convolutions / data gradients and the
(splits, tile_k) of the weight gradients that `bench.py` actually executes for YOLOv5s / YOLOv5l / YOLOXs at batch 64, 640 x 640 —
is rebuilt from its key as a descriptor at the REAL shape (B = 64, 160^2 ... 20^2 maps, M up to 1.6 M pixels, stream-K over
192 / 256 workgroups), launched through the C ABI with the shipped parameters and compared with fp32 torch
(`F.conv2d`, its autograd data / weight gradient) on identical bf16-representable inputs.  Bars as in tests/test_gpu_conv.py:
bf16 outputs 1e-2 relative + 4e-2 of the scale, fp32 weight gradients 1e-2 of the largest element; BatchNorm partial sums and
the fused BatchNorm-backward reduction against fp64 sums of the stored values.

All entries run by default (a few minutes); YH_TUNE_TEST_PARTS=n YH_TUNE_TEST_PART=i runs the i-th of n seeded shares."""
import ctypes as C
import json
import os
import random

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table():
    with open(os.path.join(ROOT, "yoloseries_amd", "tune_defaults.json")) as f:
        t = json.load(f)
    from yoloseries_amd.engine import KEY_CONV, KEY_CONV_P3, KEY_CONV_PT, KEY_CONV_S2D, KEY_WGRAD
    conv, wgrad = [], []
    for k, v in sorted(t.items()):
        parts = k.split(":")
        f = [int(x) for x in parts[-1].split(",")]
        if parts[0] in (KEY_CONV, KEY_CONV_S2D, KEY_CONV_P3, KEY_CONV_PT) and parts[1] in ("fwd", "dgrad"):
            conv.append((k, f, v))
        elif parts[0] in (KEY_WGRAD, KEY_WGRAD + "f"):
            wgrad.append((k, f, v, parts[0].endswith("f")))
    return conv, wgrad


def _share(items):
    n = int(os.environ.get("YH_TUNE_TEST_PARTS", "1"))
    if n <= 1:
        return items
    i = int(os.environ.get("YH_TUNE_TEST_PART", "0")) % n
    order = list(range(len(items)))
    random.Random(20260504).shuffle(order)
    return [items[j] for j in sorted(order[i::n])]


def _rand_bf16(shape, dev, seed, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=dev) * scale).to(torch.bfloat16)


def _tap_views(x_nhwc, k, stride, pad, Ho, Wo):
    """[(kh, kw, X_tap)]: X_tap [B * Ho * Wo][C] = the input pixel every output pixel reads through tap (kh, kw) (zero outside the map):
    a k x k convolution / its weight gradient as k * k fp32 matmuls — the same contraction as torch's convolution, without its
    per-shape algorithm search (the reference of a 3 x 3 weight gradient took 2-3 s that way)"""
    B, H, W, Cc = x_nhwc.shape
    xp = F.pad(x_nhwc, (0, 0, pad, pad, pad, pad))
    for kh in range(k):
        for kw in range(k):
            yield kh, kw, xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride, :].reshape(-1, Cc)


def _close(got, ref, rtol, atol, what):
    err = (got.float() - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: max err {err.max().item():.4g} (ref max {ref.abs().max().item():.4g}), {int(bad.sum())} of {bad.numel()} out of tolerance"


def test_shipped_table_covers_the_training_workloads():
    conv, wgrad = _table()
    assert len(conv) >= 200 and len(wgrad) >= 100
    assert all(f[1] == 64 for _, f, _ in conv) and all(f[6] == 64 for _, f, _, _ in wgrad)


NCHUNK = 8          # the walk is cut into chunks: a chunk is a test of its own (progress on the console, bounded time per test)


@pytest.mark.parametrize("chunk", range(NCHUNK))
def test_conv_entries_at_judged_shapes(dev, chunk):
    from yoloseries_amd import hipk
    from yoloseries_amd._lib import ConvDesc, YH_CONV_DGRAD, check, lib
    L = lib()
    conv, _ = _table()
    fams = {}
    items = list(enumerate(_share(conv)))
    for ki, (key, f, (tile_k, grid_cap, algo)) in items[chunk::NCHUNK]:
        (mode, B, Ho, Wo, Hi, Wi, k, stride, pad, N, nseg, C0, ld0s, ups0, C1, ups1, ldo, nsplit, accumulate, stats, res, act, bias, scale,
         bnr, acc_rows) = f
        assert not res and not act and not bias and not scale and not acc_rows and nsplit == N, key
        seed = 1000 + 7 * ki
        segC = [C0, C1][:nseg]
        segups = [ups0, ups1][:nseg]
        segs, xs = [], []
        for si in range(nseg):
            h, w = Hi >> segups[si], Wi >> segups[si]
            ld = ld0s if si == 0 else segC[si]
            buf = _rand_bf16((B, h, w, ld), dev, seed + si)
            segs.append(hipk.Slice(buf, 0, segC[si], segups[si]))
            xs.append(buf)
        Ctot = sum(segC)
        out = torch.full((B, Ho, Wo, ldo), 3.0, dtype=torch.bfloat16, device=dev)
        out0 = out.clone()
        if mode == YH_CONV_DGRAD:
            # the GEMM's "input" is gy [B][Hi][Wi][Nk] (Nk = forward output channels rounded to 8), its N the forward layer's input channels
            assert nseg == 1 and not ups0
            Nk, Cin = C0, N
            w = (torch.randn(Nk, Cin, k, k, device=dev, generator=torch.Generator(device=dev).manual_seed(seed + 5)) / (Nk * k * k) ** 0.5)
            w = w.to(torch.bfloat16).float()
            wp = hipk.pack_weight_dgrad(w)
            d = hipk.conv_desc(segs, mode, B, Ho, Wo, Hi, Wi, k, stride, pad, wp, N, hipk.Slice(out, 0, N), accumulate=accumulate)
        else:
            w = (torch.randn(N, Ctot, k, k, device=dev, generator=torch.Generator(device=dev).manual_seed(seed + 5)) / (Ctot * k * k) ** 0.5)
            w = w.to(torch.bfloat16).float()
            wp = hipk.pack_weight_fwd(w)
            d = hipk.conv_desc(segs, mode, B, Ho, Wo, Hi, Wi, k, stride, pad, wp, N, hipk.Slice(out, 0, N), accumulate=accumulate)
        d.tile_k, d.grid_cap, d.algo = tile_k, grid_cap, algo
        st = slab = z = ws = None
        if stats:
            st = torch.zeros(L.yh_conv_stat_blocks(C.byref(d)), 2, wp.shape[0], device=dev)
            d.stats = st.data_ptr()
        if bnr:
            z = _rand_bf16((B, Ho, Wo, N), dev, seed + 8)
            g = torch.Generator(device=dev).manual_seed(seed + 9)
            ws = torch.cat([torch.rand(N, generator=g, device=dev) + 0.5, torch.randn(N, generator=g, device=dev)])
            d.bnr_z, d.bnr_ldz, d.bnr_C, d.bnr_ws = z.data_ptr(), N, N, ws.data_ptr()
            d.bnr_part = out.data_ptr()                     # placeholder: the row count only looks at null / non-null
            rows = L.yh_conv_bnr_rows(C.byref(d))
            assert rows > 0, f"{key}: the shipped entry asks for the fused reduction but the kernel family cannot take it"
            slab = torch.zeros(rows, 2, N, device=dev)
            d.bnr_part = slab.data_ptr()
        name = C.create_string_buffer(96)
        check(L.yh_conv_kernel_name(C.byref(d), name, 96), "yh_conv_kernel_name")
        fams[name.value.decode().split("<")[0]] = fams.get(name.value.decode().split("<")[0], 0) + 1
        check(L.yh_conv_igemm(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), f"yh_conv_igemm [{key}]")
        # fp32 torch reference of the same op (1x1 layers: the same contraction as one fp32 matmul — no per-shape convolution search)
        if mode == YH_CONV_DGRAD and k == 1 and stride == 1 and pad == 0:
            ref = (xs[0][..., :C0].float().reshape(-1, C0) @ w.reshape(C0, N)).reshape(B, Ho, Wo, N)
        elif mode == YH_CONV_DGRAD:
            gy = xs[0][..., :C0].float().permute(0, 3, 1, 2)
            ref = torch.nn.grad.conv2d_input((B, N, Ho, Wo), w, gy, stride=stride, padding=pad).permute(0, 2, 3, 1)
        elif k == 1 and stride == 1 and pad == 0:
            parts = []
            for si in range(nseg):
                x = xs[si][..., :segC[si]].float()
                parts.append(x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if segups[si] else x)
            ref = (torch.cat(parts, 3).reshape(-1, Ctot) @ w.reshape(N, Ctot).t()).reshape(B, Ho, Wo, N)
        else:
            parts = []
            for si in range(nseg):
                x = xs[si][..., :segC[si]].float()
                parts.append(x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if segups[si] else x)
            ref = torch.zeros(B * Ho * Wo, N, device=dev)
            for kh, kw, xt in _tap_views(torch.cat(parts, 3), k, stride, pad, Ho, Wo):
                ref.addmm_(xt, w[:, :, kh, kw].t())
            ref = ref.reshape(B, Ho, Wo, N)
        if accumulate:
            ref = ref.to(torch.bfloat16).float() + out0[..., :N].float()
        torch.cuda.synchronize()
        _close(out[..., :N], ref, 1e-2, 4e-2, key)
        assert torch.equal(out[..., N:], out0[..., N:]), f"{key}: wrote outside its channel slice"
        o = out[..., :N].float().reshape(-1, N)
        S = lambda v: v.sum(0, dtype=torch.float64)          # noqa: E731  column sums accumulated in fp64
        if stats:
            # BatchNorm partial sums: some families sum the fp32 accumulators, others the stored (bf16-rounded) values — both are within
            # the rounding noise of the stored tensor: per element <= 2^-9 |v|, random sign, i.e. a random walk of 2^-9 sqrt(sum v^2)
            # (six sigma allowed); the sum of squares carries 2 v e
            s1, s2 = st[:, 0, :N].double().sum(0), st[:, 1, :N].double().sum(0)
            o2 = o * o
            so, so2 = S(o), S(o2)
            n1 = 2.0 ** -9 * so2.sqrt() * 3.5 + 1e-2
            n2 = 2.0 ** -8 * S(o2 * o2).sqrt() * 3.5 + 1e-2
            assert ((s1 - so).abs() <= n1 + 1e-5 * S(o.abs())).all(), f"{key}: sum {(s1 - so).abs().max().item():.4g} vs noise bound {n1.max().item():.4g}"
            assert ((s2 - so2).abs() <= n2 + 1e-5 * so2).all(), f"{key}: sum of squares {(s2 - so2).abs().max().item():.4g} vs {n2.max().item():.4g}"
            del o2
        if bnr:
            zz = z.float().reshape(-1, N)
            a = zz * ws[:N] + ws[N:]
            sg = torch.sigmoid(a)
            dz = o * (sg * (1 + a * (1 - sg)))
            got = slab.double().sum(0)
            assert torch.allclose(got[0], S(dz), rtol=2e-3, atol=2e-3 * S(dz.abs()).max().item()), key
            assert torch.allclose(got[1], S(dz * zz), rtol=2e-3, atol=2e-3 * S((dz * zz).abs()).max().item()), key
            del zz, a, sg, dz
        del out, out0, ref, xs, segs, w, wp, st, slab, z, ws
    print("kernel families exercised:", dict(sorted(fams.items())))
    assert len(fams) >= 4


def test_conv_entries_launch_to_launch_bit_identical(dev):
    """every conv entry of the shipped table (forward, data gradient, inference; 530 shapes) launched six times — FORTY times for the
    families with hand-counted waits (conv_pt_kernel, conv_halo160_kernel, conv_wgs_kernel: round 5's errors showed in 1 launch of 60) —
    into NaN-filled outputs, every launch NEXT TO A BUSY SECOND STREAM (copies and matmuls: the conditions of the two-stream step):
    outputs, statistics and fused-reduction slabs of every launch bit-identical to the first
    (the kernels are deterministic: a difference is a missing wait or a hazard; the weight-gradient entries — fp32 atomics — within 1e-3 of
    the largest element — the screen that reproduces round 5's store hazard
    of conv_pt_kernel on every box, tools/race_screen.py) and no NaN left in a first launch's output"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("race_screen", os.path.join(ROOT, "tools", "race_screen.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n, bad, fams = mod.screen(6, "", verbose=False, beside=True)
    assert n >= 600 and len(fams) >= 12
    assert not bad, bad[:5]


def _eval_entries():
    with open(os.path.join(ROOT, "yoloseries_amd", "tune_defaults.json")) as f:
        t = json.load(f)
    ev = []
    for k, v in sorted(t.items()):
        parts = k.split(":")
        if len(parts) == 3 and parts[1] == "eval":
            ev.append((k, [int(x) for x in parts[2].split(",")], v))
    # every entry of the judged inference configuration (YOLOv5x at 1280 x 1280, batch 128), a quarter of the others (batch 32 / 64)
    big = [e for e in ev if e[1][1] == 128]
    rest = [e for e in ev if e[1][1] != 128]
    random.Random(20261005).shuffle(rest)
    return big + rest[:len(rest) // 4]


NCHUNK_EVAL = 6


@pytest.mark.parametrize("chunk", range(NCHUNK_EVAL))
def test_eval_entries_at_judged_shapes(dev, chunk):
    """the INFERENCE entries of the shipped table (folded BatchNorm + SiLU epilogue, residual, split destination, outputs as channel
    slices of wider buffers, two-segment / upsampled inputs) at their own shapes with the kernel family / tile the table names —
    all of YOLOv5x at 1280 x 1280, batch 128 (conv_halo160 / h80 / c80 / pw / pt / stem kernels), a quarter of the rest — against
    fp32 torch, the reference taken 16 images at a time"""
    from yoloseries_amd import hipk
    from yoloseries_amd._lib import YH_ACT_SILU, check, lib
    L = lib()
    fams = {}
    for ki, (key, f, (tile_k, grid_cap, algo)) in list(enumerate(_eval_entries()))[chunk::NCHUNK_EVAL]:
        (mode, B, Ho, Wo, Hi, Wi, k, stride, pad, N, nseg, C0, ld0s, ups0, C1, ups1, ldo, nsplit, accumulate, stats, res, act, bias, scale,
         bnr, _z) = f
        assert mode == 0 and not stats and not bnr and not accumulate and not bias and act == 1 and scale == 1, key
        seed = 9000 + 13 * ki
        g = torch.Generator(device=dev).manual_seed(seed)
        segC, segups = [C0, C1][:nseg], [ups0, ups1][:nseg]
        segs, xs = [], []
        for si in range(nseg):
            h, w_ = Hi >> segups[si], Wi >> segups[si]
            ld = ld0s if si == 0 else segC[si]
            buf = torch.randn(B, h, w_, ld, generator=g, device=dev).to(torch.bfloat16)
            segs.append(hipk.Slice(buf, 0, segC[si], segups[si]))
            xs.append(buf)
        Ctot = sum(segC)
        w = (torch.randn(N, Ctot, k, k, device=dev, generator=g) / (Ctot * k * k) ** 0.5).to(torch.bfloat16).float()
        wp = hipk.pack_weight_fwd(w)
        sc = torch.rand(N, generator=g, device=dev) + 0.5
        sh = torch.randn(N, generator=g, device=dev) * 0.5
        n0 = min(nsplit, N)
        out0 = torch.full((B, Ho, Wo, ldo), 3.0, dtype=torch.bfloat16, device=dev)
        out1 = torch.full((B, Ho, Wo, N - n0 + 8), 3.0, dtype=torch.bfloat16, device=dev) if n0 < N else None
        rs = torch.randn(B, Ho, Wo, n0, generator=g, device=dev).to(torch.bfloat16) if res else None
        d = hipk.conv_desc(segs, 0, B, Ho, Wo, Hi, Wi, k, stride, pad, wp, N, hipk.Slice(out0, 0, n0), nsplit=n0,
                           out1=hipk.Slice(out1, 0, N - n0) if out1 is not None else None, scale=sc, shift=sh, act=YH_ACT_SILU,
                           res=hipk.full(rs) if rs is not None else None)
        d.tile_k, d.grid_cap, d.algo = tile_k, grid_cap, algo
        name = C.create_string_buffer(96)
        check(L.yh_conv_kernel_name(C.byref(d), name, 96), "yh_conv_kernel_name")
        fams[name.value.decode().split("<")[0]] = fams.get(name.value.decode().split("<")[0], 0) + 1
        check(L.yh_conv_igemm(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), f"yh_conv_igemm [{key}]")
        torch.cuda.synchronize()
        for b0 in range(0, B, 16):
            b1 = min(B, b0 + 16)
            if k == 1 and stride == 1 and pad == 0:
                parts = []
                for si in range(nseg):
                    x = xs[si][b0:b1, ..., :segC[si]].float()
                    parts.append(x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if segups[si] else x)
                ref = (torch.cat(parts, 3).reshape(-1, Ctot) @ w.reshape(N, Ctot).t()).reshape(b1 - b0, Ho, Wo, N)
            else:
                parts = []
                for si in range(nseg):
                    x = xs[si][b0:b1, ..., :segC[si]].float()
                    parts.append(x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if segups[si] else x)
                ref = torch.zeros((b1 - b0) * Ho * Wo, N, device=dev)
                for kh, kw, xt in _tap_views(torch.cat(parts, 3), k, stride, pad, Ho, Wo):
                    ref.addmm_(xt, w[:, :, kh, kw].t())
                ref = ref.reshape(b1 - b0, Ho, Wo, N)
            ref = F.silu(ref * sc + sh)
            if rs is not None:
                ref[..., :n0] += rs[b0:b1].float()
            _close(out0[b0:b1, ..., :n0], ref[..., :n0], 1e-2, 4e-2, key)
            if out1 is not None:
                _close(out1[b0:b1, ..., :N - n0], ref[..., n0:], 1e-2, 4e-2, key + " (second destination)")
            del ref, parts
        assert (out0[..., n0:] == 3.0).all(), f"{key}: wrote outside its channel slice"
        assert out1 is None or (out1[..., N - n0:] == 3.0).all(), f"{key}: wrote outside the second destination's slice"
        del out0, out1, rs, xs, segs, w, wp
    print("kernel families exercised:", dict(sorted(fams.items())))


@pytest.mark.parametrize("chunk", range(2))
def test_wgrad_entries_at_judged_shapes(dev, chunk):
    from yoloseries_amd import hipk
    from yoloseries_amd._lib import check, lib
    L = lib()
    _, wgrad = _table()
    fams = {}
    for ki, (key, f, (splits, tile_k), fused) in list(enumerate(_share(wgrad)))[chunk::2]:
        N, ldg, C0, ld0, ups, Ctot, B, Ho, Wo, Hi, Wi, k, stride, pad = f
        seed = 5000 + 11 * ki
        M = B * Ho * Wo
        coff = Ctot - C0                                     # place the segment at the END of the layer's input channels
        x = _rand_bf16((B, Hi >> ups, Wi >> ups, ld0), dev, seed)
        gy = _rand_bf16((B, Ho, Wo, ldg), dev, seed + 1, 0.25)
        dw = torch.zeros(N, k * k * Ctot, device=dev)
        d = hipk.wgrad_desc(hipk.Slice(gy, 0, N), N, hipk.Slice(x, 0, C0, ups), coff, Ctot, B, Ho, Wo, Hi, Wi, k, stride, pad, dw, splits)
        d.tile_k = tile_k
        gz_ref = gy[..., :N].float()
        if fused:
            # the stem: gz is formed from (ga, z) where the gy tile is staged (yh_wgrad_desc.bn_*), bit for bit the apply pass's gz
            g = torch.Generator(device=dev).manual_seed(seed + 2)
            z = _rand_bf16((B, Ho, Wo, N), dev, seed + 3)
            mean, invstd = torch.randn(N, generator=g, device=dev) * 0.3, torch.rand(N, generator=g, device=dev) + 0.5
            gamma = torch.rand(N, generator=g, device=dev) + 0.5
            beta = torch.randn(N, generator=g, device=dev) * 0.2
            scale = gamma * invstd
            ws = torch.cat([scale, beta - mean * scale, mean, invstd])
            coef = torch.cat([torch.randn(N, generator=g, device=dev) * 0.05, torch.randn(N, generator=g, device=dev) * 0.05])
            gz = torch.zeros(B, Ho, Wo, N, dtype=torch.bfloat16, device=dev)
            hipk.bn_silu_bwd_apply(hipk.Slice(gy, 0, N), hipk.full(z), ws, gamma, coef, M, hipk.full(gz))
            gz_ref = gz.float()
            d.bn_z, d.bn_ldz = z.data_ptr(), N
            d.bn_ws, d.bn_gamma, d.bn_coef = ws.data_ptr(), gamma.data_ptr(), coef.data_ptr()
        name = Program_wgrad_name(L, d)
        fams[name.split("<")[0]] = fams.get(name.split("<")[0], 0) + 1
        check(L.yh_conv_wgrad(C.byref(d), C.c_void_p(torch.cuda.current_stream().cuda_stream)), f"yh_conv_wgrad [{key}]")
        if k == 1 and stride == 1 and pad == 0:
            xf = x[..., :C0].float()
            if ups:
                xf = xf.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
            rw = (gz_ref.reshape(-1, N).t() @ xf.reshape(-1, C0)).reshape(N, 1, 1, C0)
            xin = xf
        else:
            xin = x[..., :C0].float()
            if ups:
                xin = xin.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
            rw = torch.empty(N, k, k, C0, device=dev)            # [N][kh][kw][C0]
            gz2 = gz_ref.reshape(-1, N).t().contiguous()
            for kh, kw, xt in _tap_views(xin, k, stride, pad, Ho, Wo):
                rw[:, kh, kw, :] = gz2 @ xt
            del gz2
        torch.cuda.synchronize()
        got = dw.view(N, k, k, Ctot)
        _close(got[..., coff:], rw, 1e-2, 1e-2 * rw.abs().max().item(), key)
        assert not got[..., :coff].any(), f"{key}: wrote outside its column slice"
        del x, gy, dw, rw, got, xin
    print("kernel families exercised:", dict(sorted(fams.items())))
    assert "conv_wgs_kernel" in fams


def Program_wgrad_name(L, d):
    from yoloseries_amd.engine import Program
    return Program._wgrad_name(L, d)


def test_engine_tunes_the_recorded_keys_from_its_candidates(dev, monkeypatch, tmp_path):
    """the tuner on real engine descriptors (data gradients with the fused reduction, two-segment and upsampled layers, accumulation):
    YOLOv5s at 2 x 128 x 128 with the shipped table off and an empty local one times every layer of a training forward, a backward
    and an inference forward.  The keys it stores are those of tests/golden/tune_keys_v5s_2x128.json (recorded with this body on
    the commit before the tuner read yh_conv_info; keys do not depend on timing, the stored choices do and are not compared), and
    every stored conv choice is one of the candidates TunerMixin._conv_candidates listed for its key"""
    import bench
    from yoloseries_amd import models
    from yoloseries_amd.engine import flags, tune
    from yoloseries_amd.loss import YOLOV5Loss
    from yoloseries_amd.utils.synth import COCO_ANCHORS, synth_targets
    cache = tmp_path / "tune_cache.json"
    monkeypatch.setenv("YH_TUNE_DEFAULTS", "0")
    monkeypatch.setenv("YH_TUNE_CACHE", str(cache))
    monkeypatch.setattr(tune._tune_cache, "data", None)
    monkeypatch.setattr(flags, "TUNE_ITERS", 1)
    lists, enumerate_ = {}, tune.TunerMixin._conv_candidates

    def spy(L, d, kind):
        cands = lists[tune.TunerMixin._conv_tune_key(d, kind, kind == "fwd")] = enumerate_(L, d, kind)
        return cands
    monkeypatch.setattr(tune.TunerMixin, "_conv_candidates", staticmethod(spy))
    x = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(5)).to(dev)
    t = torch.from_numpy(synth_targets(2, 128, 80, 8, seed=6, min_boxes=4)).to(dev)
    torch.manual_seed(0)
    m = models.YOLOV5Small(3, 80).to(dev).train()
    YOLOV5Loss(torch.from_numpy(COCO_ANCHORS).to(dev), bench.make_hyp(dev, 128, 2))(m(x), t)["tot_loss"].backward()
    m.eval()
    with torch.no_grad():
        m(x)
    torch.cuda.synchronize()
    stored = json.load(open(cache))
    assert sorted(stored) == json.load(open(os.path.join(ROOT, "tests", "golden", "tune_keys_v5s_2x128.json")))
    conv = {k: v for k, v in stored.items() if k.startswith("conv")}
    assert len(conv) >= 100 and set(conv) == set(lists)
    for k, (tile_k, grid_cap, algo) in conv.items():
        assert (algo, tile_k, grid_cap) in lists[k], (k, conv[k], lists[k])
