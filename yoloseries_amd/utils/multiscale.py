"""Multi-scale training: the reference's `Training.mutil_scale_training` (train_yolov5.py:526-544, train_yolox.py:511-) with the
bilinear resize on the GPU.

With `hyp['mutil_scale_training']` set the reference draws, per step, a side length in [0.5 S, 1.5 S] rounded down to a multiple
of 32, resizes the collated batch with `F.interpolate(mode='bilinear', align_corners=False)` and multiplies the box columns of the
targets by the scale.  Here the resize is one HIP kernel (csrc/preproc.hip) whose arithmetic reproduces torch's
CPU result bit for bit; `resize_bilinear_host` states that arithmetic in NumPy and is what the GPU tests compare to.  The models
take the drawn size as `forward(x, input_size=...)` and resize while they write the stem's input, so the training drivers never
materialise the resized fp32 batch."""
import math
import random

import numpy as np

__all__ = ['bilinear_tables', 'resize_bilinear_host', 'resize_bilinear', 'draw_multiscale_shape', 'mutil_scale_training']

_F32 = np.float32


def bilinear_tables(n_in, n_out):
    """One axis of the resize: (i0, i1) int32 and (l0, l1) float32, each (n_out,): output position d reads the taps i0[d], i1[d]
    with the weights l0[d], l1[d].  scale = float32(n_in) / float32(n_out); src = max(fma(scale, d + 0.5, -0.5), 0) -- the float64
    expression below is exact before its one rounding to float32, which is what the fused multiply-add computes."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"bilinear_tables: sizes must be positive, got {n_in} -> {n_out}")
    scale = _F32(n_in) / _F32(n_out)
    src = (np.float64(scale) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5).astype(_F32)
    src = np.maximum(src, _F32(0))
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(_F32)).astype(_F32)
    l0 = (_F32(1) - l1).astype(_F32)
    return i0, i1, l0, l1


def _fma32(a, b, c):
    """float32 fma(a, b, c) = a * b + c rounded once.  The product of two float32 is exact in float64; its sum with c is rounded to
    odd there (the rounding error of the float64 sum is recovered exactly and turned into a sticky last bit), after which the
    rounding to float32 is the correct one: no double rounding."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    with np.errstate(invalid='ignore'):
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                                   # TwoSum: p + c == s + err exactly
        even = (s.view(np.int64) & 1) == 0
        fix = even & (err != 0) & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(_F32)


SMALL_OUTPUT_SUM = 128      # Ho + Wo up to which torch's CPU build runs its small-output kernel (RS_SMALL_SUM in csrc/preproc.hip)


def resize_bilinear_host(x, size):
    """(B, C, H, W) float32 array -> (B, C, Ho, Wo) float32: torch's CPU `F.interpolate(x, size, mode='bilinear',
    align_corners=False)` bit for bit, and the arithmetic of yh_resize_bilinear.  With a / b the row / column weights, A B the taps
    of row y0 at x0, x1 and C D those of row y1:  out = fma(a0, fma(A, b0, B * b1), a1 * fma(C, b0, D * b1)),  torch's general
    kernel.  Where Ho + Wo <= 128 torch dispatches to another kernel (ATen UpSampleKernel.cpp, _use_vectorized_kernel_cond_2d)
    that sums four products, each weight product rounded first:  out = fma(a1*b1, D, fma(a1*b0, C, fma(a0*b0, A, (a0*b1) * B)));
    the same switch is made here and in the kernels.  Caveat: torch's general kernel is not unique in the last place -- the same
    2x3x64x64 -> 96x96 input gives it two results with 1 and with 8 threads (torch 2.10) -- so above the switch "bit for bit" means
    its result with the default thread count, as recorded in tests/golden/g16_multiscale.npz; the small-output form has shown no
    such dependence and is also compared with live torch."""
    x = np.ascontiguousarray(x, dtype=_F32)
    if x.ndim != 4:
        raise ValueError(f"resize_bilinear_host: expected (B, C, H, W), got {x.shape}")
    Ho, Wo = int(size[0]), int(size[1])
    y0, y1, a0, a1 = bilinear_tables(x.shape[2], Ho)
    x0, x1, b0, b1 = bilinear_tables(x.shape[3], Wo)
    a0, a1 = a0[:, None], a1[:, None]
    top, bot = x[:, :, y0], x[:, :, y1]
    A, B, C, D = top[..., x0], top[..., x1], bot[..., x0], bot[..., x1]
    if Ho + Wo <= SMALL_OUTPUT_SUM:
        w = [np.broadcast_to((a * b).astype(_F32), A.shape) for a in (a0, a1) for b in (b0, b1)]       # a0b0, a0b1, a1b0, a1b1
        return _fma32(w[3], D, _fma32(w[2], C, _fma32(w[0], A, (w[1] * B).astype(_F32))))
    r0 = _fma32(A, b0, (B * b1).astype(_F32))
    r1 = _fma32(C, b0, (D * b1).astype(_F32))
    return _fma32(np.broadcast_to(a0, r0.shape), r0, (a1 * r1).astype(_F32))


def resize_bilinear(x, size):
    """(B, C, H, W) float32 tensor on the GPU -> a new (B, C, size[0], size[1]) float32 tensor, on the current stream."""
    import torch
    from .. import hipk
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    out = torch.empty(x.shape[0], x.shape[1], int(size[0]), int(size[1]), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        hipk.resize_bilinear(x, out)
    return out


def draw_multiscale_shape(input_img_size, hw):
    """The draw of train_yolov5.py:537-541 for a batch of size `hw` = (h, w): returns (scale, new_shape).  The side length comes
    from the `random` module's global generator, as in the reference; its float arguments to `randrange` are spelled as the integers
    they stand for (current Python rejects floats; the draws are the same).  A configured size below 64 could draw 0: it draws 32."""
    s = int(max(input_img_size))
    random_shape = max(random.randrange(int(s * 0.5), int(s * 1.5) + 32) // 32 * 32, 32)
    scale = random_shape / max(hw)
    if scale != 1.:
        new_shape = [math.ceil(v * scale / 32) * 32 for v in hw]
    else:
        new_shape = [int(v) for v in hw]
    return scale, new_shape


def mutil_scale_training(imgs, targets, shape=None, input_img_size=None):
    """train_yolov5.py:526-544 on device tensors: `imgs` (bn, 3, h, w) float32 resized to the drawn shape, the box columns of
    `targets` (bn, bbox_num, 6) multiplied by the scale IN PLACE over all rows, padding included (:543); returns (imgs, targets).
    `shape` = [h', w'] forces the shape (the scale is then max(shape) / max(h, w), which is how the reference's shape follows from
    its scale); otherwise it is drawn around `input_img_size` (default: the batch's own size).  The models' `forward(x,
    input_size=shape)` is the fused form of the image half: same numbers, no resized fp32 batch in memory."""
    hw = [int(v) for v in imgs.shape[2:]]
    if shape is None:
        scale, new_shape = draw_multiscale_shape(hw if input_img_size is None else input_img_size, hw)
    else:
        new_shape = [int(shape[0]), int(shape[1])]
        scale = max(new_shape) / max(hw)
    if new_shape != hw:
        imgs = resize_bilinear(imgs, new_shape)
    if scale != 1.:
        targets[:, :, :4] *= scale
    return imgs, targets
