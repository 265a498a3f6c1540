"""Thin tensor-level wrappers over the C ABI (include/yolohip.h).

torch is used here only for device memory and the current stream; all arithmetic is
done by the HIP kernels.  Activations are NHWC bf16 tensors (rows = B*H*W pixels); a
"slice" is (tensor, channel offset, channels) and maps to (ptr + coff, ld).
"""
import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import ConvDesc, Seg, WgradDesc, YH_ACT_NONE, YH_ACT_SILU, YH_CONV_DGRAD, YH_CONV_FWD, check, lib


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, elem_off=0):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr() + elem_off * t.element_size())


@dataclass
class Slice:
    """A channel slice [coff, coff+C) of an NHWC bf16 buffer of shape (B,H,W,Ctot)."""
    buf: torch.Tensor
    coff: int
    C: int
    ups: int = 0

    @property
    def ld(self):
        return self.buf.shape[-1]

    def ptr(self):
        return self.buf.data_ptr() + 2 * self.coff


def full(buf):
    return Slice(buf, 0, buf.shape[-1])


def make_seg(s: Slice) -> Seg:
    return Seg(C.c_void_p(s.ptr()), s.ld, s.C, s.ups, 0)


def pack_weight_fwd(w_oihw: torch.Tensor, npad=None) -> torch.Tensor:
    """OIHW fp32 -> [Npad][KH*KW*C] bf16 (k = tap*C + c). Test/helper path (torch ops)."""
    n, c, kh, kw = w_oihw.shape
    npad = npad or ((n + 127) // 128) * 128
    out = torch.zeros(npad, kh * kw * c, dtype=torch.bfloat16, device=w_oihw.device)
    out[:n] = w_oihw.permute(0, 2, 3, 1).reshape(n, -1).to(torch.bfloat16)
    return out


def pack_weight_dgrad(w_oihw: torch.Tensor, cpad=None) -> torch.Tensor:
    """OIHW fp32 -> [Cpad][KH*KW*N] bf16 (k = tap*N + n): the dgrad GEMM's B operand."""
    n, c, kh, kw = w_oihw.shape
    cpad = cpad or ((c + 127) // 128) * 128
    out = torch.zeros(cpad, kh * kw * n, dtype=torch.bfloat16, device=w_oihw.device)
    out[:c] = w_oihw.permute(1, 2, 3, 0).reshape(c, -1).to(torch.bfloat16)
    return out


def conv_desc(segs, mode, B, Ho, Wo, Hi, Wi, k, stride, pad, w, N, out0, nsplit=None, out1=None,
              bias=None, scale=None, shift=None, act=YH_ACT_NONE, accumulate=0, res=None, stats=None):
    d = ConvDesc()
    for i, s in enumerate(segs):
        d.seg[i] = make_seg(s)
    d.nseg = len(segs)
    d.mode = mode
    d.B, d.Ho, d.Wo, d.Hi, d.Wi = B, Ho, Wo, Hi, Wi
    d.KH = d.KW = k
    d.stride, d.pad = stride, pad
    d.w = w.data_ptr()
    d.N, d.Npad = N, w.shape[0]
    d.bias = bias.data_ptr() if bias is not None else None
    d.scale = scale.data_ptr() if scale is not None else None
    d.shift = shift.data_ptr() if shift is not None else None
    d.act, d.accumulate = act, accumulate
    d.out0, d.ld0 = out0.ptr(), out0.ld
    d.nsplit = nsplit if nsplit is not None else N
    if out1 is not None:
        d.out1, d.ld1 = out1.ptr(), out1.ld
    if res is not None:
        d.res, d.ldr = res.ptr(), res.ld
    d.stats = stats.data_ptr() if stats is not None else None
    return d


def conv_stat_blocks(d: ConvDesc) -> int:
    return lib().yh_conv_stat_blocks(C.byref(d))


def conv_kernel_name(d: ConvDesc, honoured=False):
    """instantiation yh_conv_igemm launches for d, profiler spelling (yh_conv_info: no device needed).  honoured=True: None where
    the layer is not eligible for the kernel d.algo asks for (the library would run its default instead)"""
    o = _lib.ConvInfo()
    lib().yh_conv_info(C.byref(d), C.byref(o))             # (the rc speaks of operands: the callers want the plan)
    if honoured and _lib.CONV_ALGO_FAMILY.get(d.algo, (o.family, o.variant)) != (o.family, o.variant):
        return None
    return o.name.decode()


def conv_launch(d: ConvDesc):
    check(lib().yh_conv_igemm(C.byref(d), _st()), "yh_conv_igemm")


def wgrad_desc(gy: Slice, N, seg: Slice, coff_k, Ctot, B, Ho, Wo, Hi, Wi, k, stride, pad, dw, splits):
    d = WgradDesc()
    d.gy, d.ldg, d.N = gy.ptr(), gy.ld, N
    d.seg = make_seg(seg)
    d.coff_k, d.Ctot = coff_k, Ctot
    d.B, d.Ho, d.Wo, d.Hi, d.Wi = B, Ho, Wo, Hi, Wi
    d.KH = d.KW = k
    d.stride, d.pad = stride, pad
    d.dw = dw.data_ptr()
    d.splits = splits
    return d


def wgrad_launch(d: WgradDesc):
    check(lib().yh_conv_wgrad(C.byref(d), _st()), "yh_conv_wgrad")


def bn_finalize(stats, nblk, ldstat, Cn, count, gamma, beta, rm, rv, nbt, eps, momentum, ws):
    check(lib().yh_bn_finalize(_p(stats), nblk, ldstat, Cn, count, _p(gamma), _p(beta), _p(rm), _p(rv), _p(nbt),
                               eps, momentum, _p(ws), _st()), "yh_bn_finalize")


def bn_fold(gamma, beta, rm, rv, eps, Cn, scale, shift):
    check(lib().yh_bn_fold(_p(gamma), _p(beta), _p(rm), _p(rv), eps, Cn, _p(scale), _p(shift), _st()), "yh_bn_fold")


def bn_frozen(gamma, beta, rm, rv, eps, Cn, ws):
    """evaluation-mode BatchNorm constants from the running statistics: ws = scale | shift | mean | invstd"""
    check(lib().yh_bn_frozen(_p(gamma), _p(beta), _p(rm), _p(rv), eps, Cn, _p(ws), _st()), "yh_bn_frozen")


def bn_fold_batch(items):
    """items: dicts with gamma, beta, rm, rv, scale, shift (tensors) and eps; returns the device table (keep it alive until the launch ran)"""
    from ._lib import BnFoldItem
    arr = (BnFoldItem * len(items))()
    for a, q in zip(arr, items):
        for k in ("gamma", "beta", "rm", "rv", "scale", "shift"):
            setattr(a, k, q[k].data_ptr())
        a.eps, a.C = q["eps"], q["gamma"].numel()
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(items[0]["gamma"].device)
    check(lib().yh_bn_fold_batch(_p(table), len(items), _st()), "yh_bn_fold_batch")
    return table


def bn_silu_apply(y: Slice, ws, M, out: Slice, res: Slice = None):
    check(lib().yh_bn_silu_apply(y.ptr(), y.ld, _p(ws), y.C, M, out.ptr(), out.ld,
                                 res.ptr() if res else None, res.ld if res else 0, _st()), "yh_bn_silu_apply")


def ew_blocks(M):
    return lib().yh_ew_blocks(M)


def bn_silu_bwd_reduce(ga: Slice, y: Slice, ws, M, part):
    check(lib().yh_bn_silu_bwd_reduce(ga.ptr(), ga.ld, y.ptr(), y.ld, _p(ws), y.C, M, _p(part), _st()),
          "yh_bn_silu_bwd_reduce")


def bn_bwd_finalize(part, nblk, Cn, M, ws, dgamma, dbeta, coef):
    check(lib().yh_bn_bwd_finalize(_p(part), nblk, Cn, M, _p(ws), _p(dgamma), _p(dbeta), _p(coef), _st()), "yh_bn_bwd_finalize")


def bn_silu_bwd_apply(ga: Slice, y: Slice, ws, gamma, coef, M, gy: Slice, gres: Slice = None, gres_acc=0):
    check(lib().yh_bn_silu_bwd_apply(ga.ptr(), ga.ld, y.ptr(), y.ld, _p(ws), _p(gamma), _p(coef), y.C, M,
                                     gy.ptr(), gy.ld, gres.ptr() if gres else None, gres.ld if gres else 0,
                                     gres_acc, _st()), "yh_bn_silu_bwd_apply")


def _bn_parts(parts):
    """parts: dicts with ws, C and (forward) out: Slice or (backward) ga: Slice, gamma, coef"""
    from ._lib import BnPart
    arr = (BnPart * len(parts))()
    for a, q in zip(arr, parts):
        a.ws, a.C = q["ws"].data_ptr(), q["C"]
        if "out" in q:
            a.out, a.ldo = q["out"].ptr(), q["out"].ld
        if "ga" in q:
            a.ga, a.ldga = q["ga"].ptr(), q["ga"].ld
            a.gamma, a.coef = q["gamma"].data_ptr(), q["coef"].data_ptr()
        if "slab" in q:          # finalize: forward (gamma, beta, rm, rv, nbt, eps, momentum, ldslab) or backward (dgamma, dbeta, coef)
            a.slab, a.nblk, a.ldslab = q["slab"], q["nblk"], q.get("ldslab", q["C"])
            for k in ("gamma", "beta", "running_mean", "running_var", "num_batches", "dgamma", "dbeta", "coef"):
                if k in q:
                    setattr(a, k, q[k].data_ptr())
            a.eps, a.momentum = q.get("eps", 0.0), q.get("momentum", 0.0)
    return arr


def bn_finalize_parts(parts, count):
    arr = _bn_parts(parts)
    check(lib().yh_bn_finalize_parts(arr, len(parts), count, _st()), "yh_bn_finalize_parts")


def bn_bwd_finalize_parts(parts, M):
    arr = _bn_parts(parts)
    check(lib().yh_bn_bwd_finalize_parts(arr, len(parts), M, _st()), "yh_bn_bwd_finalize_parts")


def bn_silu_apply_parts(y: Slice, M, parts):
    arr = _bn_parts(parts)
    check(lib().yh_bn_silu_apply_parts(y.ptr(), y.ld, M, arr, len(parts), _st()), "yh_bn_silu_apply_parts")


def bn_silu_bwd_apply_parts(y: Slice, M, parts, gy: Slice):
    arr = _bn_parts(parts)
    check(lib().yh_bn_silu_bwd_apply_parts(y.ptr(), y.ld, M, arr, len(parts), gy.ptr(), gy.ld, _st()), "yh_bn_silu_bwd_apply_parts")


def colsum(g: Slice, M, part, out):
    check(lib().yh_colsum(g.ptr(), g.ld, g.C, M, _p(part), _p(out), _st()), "yh_colsum")


def maxpool5_fwd(x: Slice, B, H, W, out: Slice, idx):
    check(lib().yh_maxpool5_fwd(x.ptr(), x.ld, B, H, W, x.C, out.ptr(), out.ld, _p(idx), _st()), "yh_maxpool5_fwd")


def maxpool5_bwd(gout: Slice, idx, B, H, W, gin: Slice, accumulate):
    check(lib().yh_maxpool5_bwd(gout.ptr(), gout.ld, _p(idx), B, H, W, gout.C, gin.ptr(), gin.ld, accumulate, _st()),
          "yh_maxpool5_bwd")


def upsample2_bwd(ghi: Slice, B, Hlo, Wlo, glo: Slice, accumulate):
    check(lib().yh_upsample2_bwd(ghi.ptr(), ghi.ld, B, Hlo, Wlo, ghi.C, glo.ptr(), glo.ld, accumulate, _st()),
          "yh_upsample2_bwd")


def input_s2d(x, out):
    B, Cin, H, W = x.shape
    check(lib().yh_input_s2d(_p(x), B, Cin, H, W, _p(out), _st()), "yh_input_s2d")


def letterbox_batch(raw, img_off, src_hw, rows, cols, out, fill_value=128):
    """raw uint8 images (concatenated HWC) + index tables (utils/letterbox.py pack_raw_batch) -> out (B, 3, H, W) float32, on the
    current stream.  The tables' contents are the caller's: the kernel reads raw wherever they point."""
    B, _, H, W = out.shape
    want = ((raw, torch.uint8, None), (img_off, torch.int64, (B,)), (src_hw, torch.int32, (B, 2)), (rows, torch.int32, (B, H)),
            (cols, torch.int32, (B, W)), (out, torch.float32, (B, 3, H, W)))
    for t, dtype, shape in want:
        if t.dtype != dtype or not t.is_cuda or t.device != out.device or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
            raise ValueError(f"letterbox_batch: expected a contiguous {dtype} tensor of shape {shape or '(n,)'} on {out.device}, "
                             f"got {t.dtype} {tuple(t.shape)} on {t.device}")
    check(lib().yh_letterbox_batch(_p(raw), _p(img_off), _p(src_hw), _p(rows), _p(cols), B, H, W, int(fill_value), _p(out), _st()),
          "yh_letterbox_batch")


def augment_batch(raw, tiles, canvas_hw, minv, hsv_gain, out, fill_value=128):
    """raw uint8 images (concatenated HWC) + the plan tables of dataset/data_collater.py augment_collate_fn -> out (B, 3, H, W) float32
    on the current stream: mosaic, warp, flips and HSV jitter in one launch (utils/augment.py augment_batch_host is the definition).
    tiles: (B, 4, 40) uint8, the bytes of yh_aug_tile records; hsv_gain: (B, 3) float32 or None.  The tables' contents are the
    caller's: the kernel reads raw wherever they point (inside the image they name)."""
    B, _, H, W = out.shape
    want = [(raw, torch.uint8, None), (tiles, torch.uint8, (B, 4, 40)), (canvas_hw, torch.int32, (B, 2)), (minv, torch.float32, (B, 9)),
            (out, torch.float32, (B, 3, H, W))]
    if hsv_gain is not None:
        want.append((hsv_gain, torch.float32, (B, 3)))
    for t, dtype, shape in want:
        if t.dtype != dtype or not t.is_cuda or t.device != out.device or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
            raise ValueError(f"augment_batch: expected a contiguous {dtype} tensor of shape {shape or '(n,)'} on {out.device}, "
                             f"got {t.dtype} {tuple(t.shape)} on {t.device}")
    if raw.numel() < 3:
        raise ValueError(f"augment_batch: raw holds {raw.numel()} bytes, less than one pixel")
    check(lib().yh_augment_batch(_p(raw), _p(tiles), _p(canvas_hw), _p(minv), _p(hsv_gain), B, H, W, int(fill_value), _p(out), _st()),
          "yh_augment_batch")


def _resize_src(x, who):
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
        raise ValueError(f"{who}: expected a contiguous (B, C, H, W) float32 tensor on the GPU, got {x.dtype} {tuple(x.shape)} on {x.device}")
    return x.shape


def resize_bilinear(x, out):
    """x (B, C, H, W) float32 -> out (B, C, Ho, Wo) float32 on the current stream: F.interpolate(bilinear, align_corners=False) of
    torch's CPU build, bit for bit (utils/multiscale.py resize_bilinear_host states the arithmetic)"""
    B, Ch, H, W = _resize_src(x, "resize_bilinear")
    if (out.dim() != 4 or tuple(out.shape[:2]) != (B, Ch) or out.dtype != torch.float32 or out.device != x.device
            or not out.is_contiguous()):
        raise ValueError(f"resize_bilinear: expected a contiguous float32 output ({B}, {Ch}, Ho, Wo) on {x.device}, "
                         f"got {out.dtype} {tuple(out.shape)} on {out.device}")
    check(lib().yh_resize_bilinear(_p(x), B, Ch, H, W, out.shape[2], out.shape[3], _p(out), _st()), "yh_resize_bilinear")


def resize_bilinear_s2d(x, out):
    """x (B, Cin <= 4, H, W) float32 -> out (B, Ho/2, Wo/2, 16) bfloat16, the stem's input at the size (Ho, Wo): the bits of
    input_s2d(resize_bilinear(x)) without the float32 intermediate"""
    B, Cin, H, W = _resize_src(x, "resize_bilinear_s2d")
    if (out.dim() != 4 or out.shape[0] != B or out.shape[3] != 16 or out.dtype != torch.bfloat16 or out.device != x.device
            or not out.is_contiguous()):
        raise ValueError(f"resize_bilinear_s2d: expected a contiguous bfloat16 output ({B}, Ho/2, Wo/2, 16) on {x.device}, "
                         f"got {out.dtype} {tuple(out.shape)} on {out.device}")
    check(lib().yh_resize_bilinear_s2d(_p(x), B, Cin, H, W, 2 * out.shape[1], 2 * out.shape[2], _p(out), _st()), "yh_resize_bilinear_s2d")


def fill_zero(t):
    nbytes = t.numel() * t.element_size()
    assert nbytes % 4 == 0
    check(lib().yh_fill_u32(_p(t), 0, nbytes // 4, _st()), "yh_fill_u32")


def fill_u32(t, value, n_words, word_off=0):
    """n_words 32-bit words of t, from word `word_off` on, set to `value`"""
    check(lib().yh_fill_u32(C.c_void_p(t.data_ptr() + 4 * word_off), value, n_words, _st()), "yh_fill_u32")


def pack_bf16(src, idx, dst):
    check(lib().yh_pack_bf16(_p(src), _p(idx), idx.numel(), _p(dst), _st()), "yh_pack_bf16")


def gather_f32(src, idx, dst):
    check(lib().yh_gather_f32(_p(src), _p(idx), idx.numel(), _p(dst), _st()), "yh_gather_f32")


def sgd_step(p, g, buf, group, lr, wd, momentum, nesterov, first, grad_scale=None):
    check(lib().yh_sgd_step(_p(p), _p(g), _p(buf), _p(group), p.numel(), _p(lr), _p(wd), lr.numel(), momentum,
                            int(nesterov), int(first), _p(grad_scale), _st()), "yh_sgd_step")


def sumsq(x, part, out):
    check(lib().yh_sumsq(_p(x), x.numel(), _p(part), _p(out), _st()), "yh_sumsq")


def ema_update(ema, p, decay):
    check(lib().yh_ema_update(_p(ema), _p(p), p.numel(), decay, _st()), "yh_ema_update")


def clip_scale(sumsq_t, max_norm, out):
    check(lib().yh_clip_scale(_p(sumsq_t), float(max_norm), _p(out), _st()), "yh_clip_scale")


def sgd_step_dev(p, g, buf, group, scal, nesterov, grad_scale=None):
    """SGD step with lr | wd | momentum | first-step flag read from the device tensor `scal` (8 floats): graph-replay safe"""
    check(lib().yh_sgd_step_dev(_p(p), _p(g), _p(buf), _p(group), p.numel(), _p(scal), int(nesterov), _p(grad_scale), _st()), "yh_sgd_step_dev")


# layout of Adam's device block (include/yolohip.h, yh_adam_step_dev): 16 floats, the step count one int64 at floats 12..13
ADAM_BLK_FLOATS, ADAM_BLK_HOST, ADAM_BLK_BC1, ADAM_BLK_SBC2, ADAM_BLK_T = 16, 9, 9, 10, 12
ADAM_GRID_PASS = 1280 * 256 * 4 * 2      # elements of one full grid pass of the step kernel (csrc/arena.hip: ADAM_BLOCKS x TH x 4 x ADAM_UNROLL)


def adam_advance(blk):
    """step count of the device block += 1, bias corrections of that step written into the block"""
    check(lib().yh_adam_advance(_p(blk), _st()), "yh_adam_advance")


def adam_step_dev(p, g, m, v, group, blk, grad_scale=None):
    """Adam step with lr | wd | betas | eps | bias corrections read from the device block `blk` (16 floats): graph-replay safe"""
    check(lib().yh_adam_step_dev(_p(p), _p(g), _p(m), _p(v), _p(group), p.numel(), _p(blk), _p(grad_scale), _st()), "yh_adam_step_dev")


def ema_update_dev(ema, p, decay_dev):
    check(lib().yh_ema_update_dev(_p(ema), _p(p), p.numel(), _p(decay_dev), _st()), "yh_ema_update_dev")


def ema_advance(counter, decay, ratio, tau):
    check(lib().yh_ema_advance(_p(counter), _p(decay), float(ratio), float(tau), _st()), "yh_ema_advance")


WBF_BOX_MEANS = {'reference': 0, 'weighted': 1}


def wbf_lds_clusters():
    """clusters of one (image, class) whose state yh_wbf_batched keeps in LDS; the ones past it live in its workspace"""
    return int(lib().yh_wbf_lds_clusters())


def wbf_order(cand, weight, num_class):
    """The row order yh_wbf_batched consumes -> (order (B, cap) int32, nvalid (B,) int32): one stable sort of an int64 key per image —
    non-candidates last, class ascending, the complement of the score's bits (score descending), ties in table order.  A row is a
    candidate iff weight > 0, score > 0 and 0 <= cls < num_class."""
    score, cls = cand[:, :, 4], cand[:, :, 5]
    valid = (weight > 0) & (score > 0) & (cls >= 0) & (cls < num_class)
    ci = torch.where(valid, cls, torch.zeros_like(cls)).to(torch.int64)
    bits = score.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = torch.where(valid, (ci << 32) | (0xFFFFFFFF - bits), torch.full_like(ci, 1 << 62))
    return torch.sort(key, dim=1, stable=True)[1].to(torch.int32).contiguous(), valid.sum(dim=1).to(torch.int32)


def wbf(cand, weight, iou_thr, box_mean='reference', num_class=None):
    """Weighted box fusion of candidate tables on the device: wbf_order, the workspace, yh_wbf_batched.
    cand (B, cap, 6) float32 [xmin, ymin, xmax, ymax, score, cls], weight (B, cap) float32: a row is a candidate iff weight > 0,
    score > 0 and 0 <= cls < num_class.  num_class None: taken from the table (the one host wait of this function; pass it to stay
    asynchronous).
    -> out (B, cap, 6) float32, nout (B,) int32, members (B, cap) int32; rows at or past nout[b] are undefined."""
    if box_mean not in WBF_BOX_MEANS:
        raise ValueError(f"wbf: box_mean {box_mean!r} is not one of {sorted(WBF_BOX_MEANS)}")
    if not cand.is_cuda:
        raise _lib.YoloHipError("wbf: tensors must live on an MI355X device")
    cand = cand.to(torch.float32).contiguous()
    weight = weight.to(device=cand.device, dtype=torch.float32).contiguous()
    if cand.dim() != 3 or cand.shape[2] != 6 or tuple(weight.shape) != tuple(cand.shape[:2]):
        raise ValueError(f"wbf: cand {tuple(cand.shape)} / weight {tuple(weight.shape)} are not (B, cap, 6) / (B, cap)")
    B, cap = cand.shape[0], cand.shape[1]
    dev = cand.device
    out = torch.empty(B, max(cap, 1), 6, dtype=torch.float32, device=dev)
    nout = torch.zeros(B, dtype=torch.int32, device=dev)
    members = torch.zeros(B, max(cap, 1), dtype=torch.int32, device=dev)
    if B == 0 or cap == 0:
        return out, nout, members
    if num_class is None:
        cls = cand[:, :, 5]
        num_class = int(torch.where(weight > 0, cls, torch.zeros_like(cls)).nan_to_num(0.0).clamp(0, 2 ** 20).max().item()) + 1
    order, nvalid = wbf_order(cand, weight, num_class)
    ws = torch.empty(max(int(lib().yh_wbf_ws_bytes(B, cap)), 16), dtype=torch.uint8, device=dev)
    check(lib().yh_wbf_batched(_p(cand), _p(weight), _p(order), _p(nvalid), B, cap, int(num_class), float(iou_thr),
                               WBF_BOX_MEANS[box_mean], _p(out), _p(nout), _p(members), _p(ws), _st()), "yh_wbf_batched")
    return out, nout, members
