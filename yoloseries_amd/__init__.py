"""yoloseries_amd — MI355X (gfx950) native hot path of yl-jiang/YOLOSeries.

Layout:  csrc/ (HIP kernels + C ABI, include/yolohip.h)  ·  _lib.py / hipk.py (ctypes binding)
         models/ loss/ trainer/ utils/ (host-side mirror of the reference's Python surface)
"""
__version__ = "0.1.0"

__all__ = ["set_deterministic"]


def set_deterministic(enabled):
    """Bit-reproducible training on / off (default off).  Everything of the step but the weight gradients is reproducible already;
    with ``enabled`` those leave their kernels through a workspace and a fixed-order sum instead of fp32 atomics, on the same kernel
    families (engine/flags.py).  Holds for every training program built afterwards; a model whose backward was already built with
    the other setting rebuilds it on its next backward pass (a captured hipGraph keeps what it recorded: call this first).
    ``utils.gpu.init_seed`` seeds the generators as in the reference and does not touch this switch."""
    from .engine import flags
    flags.set_deterministic(enabled)
