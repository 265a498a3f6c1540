#!/usr/bin/env python3
"""Generate tests/golden/g16_multiscale.npz: inputs (uint8; the tests divide by 255) and what torch's CPU build returns for
F.interpolate(x, size, mode='bilinear', align_corners=False) on them.  Needs torch only; run it where the golden vectors are made.

torch's CPU build has two bilinear kernels: outputs with Ho + Wo <= 128 take one that sums four weighted taps (cases `small*`),
larger ones the general kernel (cases `general*`); utils/multiscale.py states both.  The general kernel's result can also depend on
torch's thread count (2x3x64x64 -> 96x96 differs in the last place between 1 and 8 threads on torch 2.10): the recorded outputs are
those of the default count, and the file keeps the torch version and that count."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g16_multiscale.npz")
# name -> (input shape, seed of the input, output size)
CASES = {
    "small_up": ((2, 3, 24, 40), 161, (40, 72)),
    "small_down": ((2, 3, 24, 40), 161, (16, 24)),
    "small_identity": ((2, 3, 24, 40), 161, (24, 40)),
    "small_odd": ((1, 3, 37, 53), 162, (45, 71)),
    "general_up": ((1, 3, 64, 96), 163, (96, 160)),
    "general_down": ((1, 3, 96, 128), 164, (64, 96)),
}


def main():
    g = {"torch_version": np.array(torch.__version__), "num_threads": np.array(torch.get_num_threads())}
    for name, (shape, seed, size) in CASES.items():
        u8 = np.random.RandomState(seed).randint(0, 256, size=shape, dtype=np.uint8)
        x = torch.from_numpy(u8.astype(np.float32) / np.float32(255))
        g[f"{name}_x"] = u8
        g[f"{name}_out"] = F.interpolate(x, size=size, mode='bilinear', align_corners=False).numpy()
    np.savez_compressed(OUT, **g)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    sys.exit(main())
