"""One row per kernel instantiation yh_conv_igemm can launch: the smallest descriptor whose plan names it.

tests/test_gpu_conv_instantiations.py runs every row on the GPU against float64 torch; tests/test_host_logic.py checks, without a
device, that every row is planned to its name and that the rows cover every name the planner emits (conv_plan_table.py's corpora
and tests/golden/conv_plan_digest.json).  A new instantiation needs a row here before either passes.

A row:  (name, tag, mode, B, H, W, segments, N, k, stride, pad, epilogue, algo, tile_k, tile_n)
  name      what yh_conv_info answers for the descriptor (the instantiation as profilers print it)
  tag       tells rows of one instantiation apart (a launch-shape branch of the plan: see the end of ROWS)
  mode      F forward, D data gradient.  H x W is the grid of the pixels written (D: the gradient's grid, the forward layer's input)
  segments  input channels per segment, "32+64"; "^" marks a segment read through the nearest-2x upsample.  Every segment is a
            channel slice [8, 8 + C) of a buffer C + 16 wide
  N         output channels (D: the forward layer's input channels)
  epilogue  plain | stats | full (bias, folded BN, SiLU, residual, split destination) | one (the same into one destination) |
            nores (bias, folded BN, SiLU) | bn (folded BN, SiLU) | gstats (bias beside statistics: the generic kernel) |
            acc (accumulate) | bnr (fused BatchNorm-backward reduction)
Shapes: B >= 2, an image boundary inside a pixel tile, M no multiple of the tile and at least two tiles (3 x 17 x 13 = 663 pixels);
stride-2 data gradients on an even grid (3 x 18 x 14) where they run as parity classes; the fewest input channels the instantiation
takes (tails: 80 = 64 + 16, and 112 = 64 + 48 in the tail-48 rows; 32-channel k-steps: 96, or 32 + 64 in two segments); N ragged
against the channel tile (24 of 32, 48 of 64, 160 of 128; the 256-wide tile takes multiples of 256 only).

Every family's plan honours grid_cap — conv_plan and each sibling's *_plan — except the stem's (`pl->family != FAM_STEM`): Row.cap.

Compiled but reached by no valid descriptor (no row): conv_pt_kernel<64, 64, 3> and <128, 128, 3> — the fused reduction on a
two-segment data gradient, for which yh_conv_bnr_rows answers 0 (conv_bnr_possible: one segment)."""
import collections
import ctypes as C
import importlib.util
import os

_HERE = os.path.dirname(os.path.abspath(__file__))


def _plan_table():
    spec = importlib.util.spec_from_file_location("conv_plan_table", os.path.join(_HERE, "conv_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _plan_table()
F, D = 0, 1
PAD = 8           # channel offset of every operand slice inside its buffer (which is 2 * PAD channels wider)
IGNORES_GRID_CAP = ("conv_stem_kernel",)

_ROWS = [
    ("conv_c80_kernel", "", F, 3, 17, 13, "80", 160, 3, 1, 1, "nores", 12, 0, 0),
    ("conv_c80_kernel", "stride-2", F, 3, 17, 13, "80", 160, 3, 2, 1, "nores", 12, 0, 0),
    ("conv_dg2_kernel<1, 32, 0, 1>", "", D, 3, 18, 14, "32", 24, 3, 2, 1, "acc", 7, 0, 0),
    ("conv_dg2_kernel<1, 32, 3, 1>", "", D, 3, 18, 14, "32", 24, 3, 2, 1, "bnr", 7, 0, 0),
    ("conv_dg2_kernel<1, 64, 0, 1>", "", D, 3, 18, 14, "64", 24, 3, 2, 1, "plain", 7, 0, 0),
    ("conv_dg2_kernel<1, 64, 3, 1>", "", D, 3, 18, 14, "64", 24, 3, 2, 1, "bnr", 7, 0, 0),
    ("conv_dg2_kernel<2, 32, 0, 1>", "", D, 3, 18, 14, "32", 48, 3, 2, 1, "plain", 7, 0, 0),
    ("conv_dg2_kernel<2, 32, 3, 1>", "", D, 3, 18, 14, "32", 48, 3, 2, 1, "bnr", 7, 0, 0),
    ("conv_dg2_kernel<2, 64, 0, 1>", "", D, 3, 18, 14, "64", 48, 3, 2, 1, "acc", 7, 0, 0),
    ("conv_dg2_kernel<2, 64, 3, 1>", "", D, 3, 18, 14, "64", 48, 3, 2, 1, "bnr", 7, 0, 0),
    ("conv_h80_kernel<80, 5, 0>", "", F, 3, 17, 13, "80", 80, 3, 1, 1, "plain", 9, 0, 0),
    ("conv_h80_kernel<80, 5, 2>", "", F, 3, 17, 13, "80", 80, 3, 1, 1, "full", 9, 0, 0),
    ("conv_halo160_kernel<0, false>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "plain", 6, 0, 0),
    ("conv_halo160_kernel<0, true>", "", F, 3, 17, 13, "96", 160, 3, 1, 1, "plain", 6, 0, 0),
    ("conv_halo160_kernel<2, false>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "full", 6, 0, 0),
    ("conv_halo160_kernel<2, true>", "", F, 3, 17, 13, "96", 160, 3, 1, 1, "full", 6, 0, 0),
    # halo kernel: N = 160 is two channel tiles (EPI 2: the XCD-major block order), N = 48 one (row-major)
    ("conv_halo_kernel<128, 0, false>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "plain", 5, 0, 0),
    ("conv_halo_kernel<128, 0, true>", "", F, 3, 17, 13, "80", 160, 3, 1, 1, "plain", 5, 0, 0),
    ("conv_halo_kernel<128, 1, false>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "stats", 5, 0, 0),
    ("conv_halo_kernel<128, 1, true>", "", F, 3, 17, 13, "80", 160, 3, 1, 1, "stats", 5, 0, 0),
    ("conv_halo_kernel<128, 2, false>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "full", 5, 0, 0),
    ("conv_halo_kernel<128, 2, true>", "", F, 3, 17, 13, "80", 160, 3, 1, 1, "full", 5, 0, 0),
    ("conv_halo_kernel<128, 3, false>", "", D, 3, 17, 13, "64", 160, 3, 1, 1, "bnr", 5, 0, 0),
    ("conv_halo_kernel<128, 3, true>", "", D, 3, 17, 13, "80", 160, 3, 1, 1, "bnr", 5, 0, 0),
    ("conv_halo_kernel<64, 0, false>", "", F, 3, 17, 13, "64", 48, 3, 1, 1, "plain", 5, 0, 0),
    ("conv_halo_kernel<64, 0, true>", "", F, 3, 17, 13, "80", 48, 3, 1, 1, "plain", 5, 0, 0),
    ("conv_halo_kernel<64, 1, false>", "", F, 3, 17, 13, "64", 48, 3, 1, 1, "stats", 5, 0, 0),
    ("conv_halo_kernel<64, 1, true>", "", F, 3, 17, 13, "80", 48, 3, 1, 1, "stats", 5, 0, 0),
    ("conv_halo_kernel<64, 2, false>", "", F, 3, 17, 13, "64", 48, 3, 1, 1, "full", 5, 0, 0),
    ("conv_halo_kernel<64, 2, true>", "", F, 3, 17, 13, "80", 48, 3, 1, 1, "full", 5, 0, 0),
    ("conv_halo_kernel<64, 3, false>", "", D, 3, 17, 13, "64", 48, 3, 1, 1, "bnr", 5, 0, 0),
    ("conv_halo_kernel<64, 3, true>", "", D, 3, 17, 13, "80", 48, 3, 1, 1, "bnr", 5, 0, 0),
    # generic kernel: statistics of an affine output (conv_buf_ok declines them); 16 channels: no whole 32-channel block
    ("conv_igemm_kernel<128, 2, 2, false, 2>", "", F, 3, 17, 13, "16", 160, 3, 1, 1, "gstats", 0, 0, 0),
    ("conv_igemm_kernel<128, 2, 2, true, 2>", "", F, 3, 17, 13, "32", 160, 3, 1, 1, "gstats", 0, 0, 0),
    ("conv_igemm_kernel<32, 4, 1, false, 4>", "", F, 3, 17, 13, "16", 24, 3, 1, 1, "gstats", 0, 0, 0),
    ("conv_igemm_kernel<32, 4, 1, true, 4>", "", F, 3, 17, 13, "32", 24, 3, 1, 1, "gstats", 0, 0, 0),
    ("conv_igemm_kernel<64, 4, 1, false, 3>", "", F, 3, 17, 13, "16", 48, 3, 1, 1, "gstats", 0, 0, 0),
    ("conv_igemm_kernel<64, 4, 1, true, 3>", "", F, 3, 17, 13, "32", 48, 3, 1, 1, "gstats", 0, 0, 0),
    # patch kernel <channel tiles, k-step, EPI, pixel tiles per wave (tile_n 32: one), stride>
    ("conv_p3_kernel<1, 32, 0, 1, 1>", "", F, 3, 17, 13, "32", 24, 3, 1, 1, "plain", 8, 0, 32),
    ("conv_p3_kernel<1, 32, 0, 1, 2>", "", F, 3, 17, 13, "32", 24, 3, 2, 1, "plain", 8, 0, 32),
    ("conv_p3_kernel<1, 32, 0, 2, 1>", "", F, 3, 17, 13, "32", 24, 3, 1, 1, "plain", 8, 0, 0),
    ("conv_p3_kernel<1, 32, 0, 2, 2>", "", F, 3, 17, 13, "32", 24, 3, 2, 1, "plain", 8, 0, 0),
    ("conv_p3_kernel<1, 32, 1, 1, 1>", "", F, 3, 17, 13, "32", 24, 3, 1, 1, "stats", 8, 0, 32),
    ("conv_p3_kernel<1, 32, 1, 1, 2>", "", F, 3, 17, 13, "32", 24, 3, 2, 1, "stats", 8, 0, 32),
    ("conv_p3_kernel<1, 32, 1, 2, 1>", "", F, 3, 17, 13, "32", 24, 3, 1, 1, "stats", 8, 0, 0),
    ("conv_p3_kernel<1, 32, 1, 2, 2>", "", F, 3, 17, 13, "32", 24, 3, 2, 1, "stats", 8, 0, 0),
    ("conv_p3_kernel<1, 32, 3, 1, 1>", "", D, 3, 17, 13, "32", 24, 3, 1, 1, "bnr", 8, 0, 32),
    ("conv_p3_kernel<1, 32, 3, 2, 1>", "", D, 3, 17, 13, "32", 24, 3, 1, 1, "bnr", 8, 0, 0),
    ("conv_p3_kernel<1, 64, 0, 1, 1>", "", F, 3, 17, 13, "64", 24, 3, 1, 1, "plain", 8, 0, 32),
    ("conv_p3_kernel<1, 64, 0, 2, 1>", "", D, 3, 17, 13, "64", 24, 3, 1, 1, "acc", 8, 0, 0),
    ("conv_p3_kernel<1, 64, 1, 1, 1>", "", F, 3, 17, 13, "64", 24, 3, 1, 1, "stats", 8, 0, 32),
    ("conv_p3_kernel<1, 64, 1, 2, 1>", "", F, 3, 17, 13, "64", 24, 3, 1, 1, "stats", 8, 0, 0),
    ("conv_p3_kernel<1, 64, 3, 1, 1>", "", D, 3, 17, 13, "64", 24, 3, 1, 1, "bnr", 8, 0, 32),
    ("conv_p3_kernel<1, 64, 3, 2, 1>", "", D, 3, 17, 13, "64", 24, 3, 1, 1, "bnr", 8, 0, 0),
    ("conv_p3_kernel<2, 32, 0, 1, 1>", "", D, 3, 17, 13, "32", 48, 3, 1, 1, "acc", 8, 0, 32),
    ("conv_p3_kernel<2, 32, 0, 1, 2>", "", F, 3, 17, 13, "32", 48, 3, 2, 1, "plain", 8, 0, 32),
    ("conv_p3_kernel<2, 32, 0, 2, 1>", "", F, 3, 17, 13, "32", 48, 3, 1, 1, "plain", 8, 0, 0),
    ("conv_p3_kernel<2, 32, 0, 2, 2>", "", F, 3, 17, 13, "32", 48, 3, 2, 1, "plain", 8, 0, 0),
    ("conv_p3_kernel<2, 32, 1, 1, 1>", "", F, 3, 17, 13, "32", 48, 3, 1, 1, "stats", 8, 0, 32),
    ("conv_p3_kernel<2, 32, 1, 1, 2>", "", F, 3, 17, 13, "32", 48, 3, 2, 1, "stats", 8, 0, 32),
    ("conv_p3_kernel<2, 32, 1, 2, 1>", "", F, 3, 17, 13, "32", 48, 3, 1, 1, "stats", 8, 0, 0),
    ("conv_p3_kernel<2, 32, 1, 2, 2>", "", F, 3, 17, 13, "32", 48, 3, 2, 1, "stats", 8, 0, 0),
    ("conv_p3_kernel<2, 32, 3, 1, 1>", "", D, 3, 17, 13, "32", 48, 3, 1, 1, "bnr", 8, 0, 32),
    ("conv_p3_kernel<2, 32, 3, 2, 1>", "", D, 3, 17, 13, "32", 48, 3, 1, 1, "bnr", 8, 0, 0),
    ("conv_p3_kernel<2, 64, 0, 1, 1>", "", F, 3, 17, 13, "64", 48, 3, 1, 1, "plain", 8, 0, 32),
    ("conv_p3_kernel<2, 64, 0, 2, 1>", "", F, 3, 17, 13, "64", 48, 3, 1, 1, "plain", 8, 0, 0),
    ("conv_p3_kernel<2, 64, 1, 1, 1>", "", F, 3, 17, 13, "64", 48, 3, 1, 1, "stats", 8, 0, 32),
    ("conv_p3_kernel<2, 64, 1, 2, 1>", "", F, 3, 17, 13, "64", 48, 3, 1, 1, "stats", 8, 0, 0),
    ("conv_p3_kernel<2, 64, 3, 1, 1>", "", D, 3, 17, 13, "64", 48, 3, 1, 1, "bnr", 8, 0, 32),
    ("conv_p3_kernel<2, 64, 3, 2, 1>", "", D, 3, 17, 13, "64", 48, 3, 1, 1, "bnr", 8, 0, 0),
    # training pointwise kernel <C0, C1, EPI>: EPI 4 = the generic epilogue with a memory operand (residual / accumulate)
    ("conv_pt_kernel<128, 0, 0>", "", F, 3, 17, 13, "128", 24, 1, 1, 0, "plain", 13, 0, 0),
    ("conv_pt_kernel<128, 0, 1>", "", F, 3, 17, 13, "128", 24, 1, 1, 0, "stats", 13, 0, 0),
    ("conv_pt_kernel<128, 0, 2>", "", F, 3, 17, 13, "128", 24, 1, 1, 0, "nores", 13, 0, 0),
    ("conv_pt_kernel<128, 0, 3>", "", D, 3, 17, 13, "128", 24, 1, 1, 0, "bnr", 13, 0, 0),
    ("conv_pt_kernel<128, 0, 4>", "", D, 3, 17, 13, "128", 24, 1, 1, 0, "acc", 13, 0, 0),
    ("conv_pt_kernel<128, 128, 0>", "", F, 3, 17, 13, "128+128", 24, 1, 1, 0, "plain", 13, 0, 0),
    ("conv_pt_kernel<128, 128, 1>", "", F, 3, 17, 13, "128+128", 24, 1, 1, 0, "stats", 13, 0, 0),
    ("conv_pt_kernel<128, 128, 2>", "", F, 3, 17, 13, "128+128", 24, 1, 1, 0, "nores", 13, 0, 0),
    ("conv_pt_kernel<128, 128, 2>", "upsampled-second", F, 3, 18, 14, "128+128^", 24, 1, 1, 0, "nores", 13, 0, 0),
    ("conv_pt_kernel<128, 128, 4>", "", F, 3, 17, 13, "128+128", 24, 1, 1, 0, "one", 13, 0, 0),
    ("conv_pt_kernel<256, 0, 0>", "", F, 3, 17, 13, "256", 24, 1, 1, 0, "plain", 13, 0, 0),
    ("conv_pt_kernel<256, 0, 1>", "", F, 3, 17, 13, "256", 24, 1, 1, 0, "stats", 13, 0, 0),
    ("conv_pt_kernel<256, 0, 2>", "", F, 3, 17, 13, "256", 24, 1, 1, 0, "nores", 13, 0, 0),
    ("conv_pt_kernel<256, 0, 3>", "", D, 3, 17, 13, "256", 24, 1, 1, 0, "bnr", 13, 0, 0),
    ("conv_pt_kernel<256, 0, 4>", "", F, 3, 17, 13, "256", 24, 1, 1, 0, "one", 13, 0, 0),
    ("conv_pt_kernel<256, 256, 0>", "", F, 3, 17, 13, "256+256", 24, 1, 1, 0, "plain", 13, 0, 0),
    ("conv_pt_kernel<256, 256, 1>", "", F, 3, 17, 13, "256+256", 24, 1, 1, 0, "stats", 13, 0, 0),
    ("conv_pt_kernel<256, 256, 2>", "", F, 3, 17, 13, "256+256", 24, 1, 1, 0, "nores", 13, 0, 0),
    ("conv_pt_kernel<320, 0, 0>", "", F, 3, 17, 13, "320", 24, 1, 1, 0, "plain", 13, 0, 0),
    ("conv_pt_kernel<320, 0, 2>", "", F, 3, 17, 13, "320", 24, 1, 1, 0, "nores", 13, 0, 0),
    ("conv_pt_kernel<512, 0, 0>", "", F, 3, 17, 13, "512", 24, 1, 1, 0, "plain", 13, 0, 0),
    ("conv_pt_kernel<512, 0, 1>", "", F, 3, 17, 13, "512", 24, 1, 1, 0, "stats", 13, 0, 0),
    ("conv_pt_kernel<512, 0, 2>", "", F, 3, 17, 13, "512", 24, 1, 1, 0, "nores", 13, 0, 0),
    ("conv_pt_kernel<64, 64, 0>", "", F, 3, 17, 13, "64+64", 24, 1, 1, 0, "plain", 13, 0, 0),
    ("conv_pt_kernel<64, 64, 1>", "", F, 3, 17, 13, "64+64", 24, 1, 1, 0, "stats", 13, 0, 0),
    ("conv_pt_kernel<64, 64, 1>", "upsampled-first", F, 3, 18, 14, "64^+64", 24, 1, 1, 0, "stats", 13, 0, 0),
    ("conv_pt_kernel<64, 64, 2>", "", F, 3, 17, 13, "64+64", 24, 1, 1, 0, "nores", 13, 0, 0),
    ("conv_pt_kernel<64, 64, 4>", "", F, 3, 17, 13, "64+64", 24, 1, 1, 0, "one", 13, 0, 0),
    ("conv_pw_kernel<160, 5, 1, 0>", "", F, 3, 17, 13, "160", 80, 1, 1, 0, "plain", 10, 0, 0),
    ("conv_pw_kernel<160, 5, 1, 2>", "", F, 3, 17, 13, "160", 80, 1, 1, 0, "full", 10, 0, 0),
    ("conv_pw_kernel<320, 5, 1, 0>", "", F, 3, 17, 13, "320", 80, 1, 1, 0, "plain", 10, 0, 0),
    ("conv_pw_kernel<320, 5, 1, 2>", "", F, 3, 17, 13, "320", 80, 1, 1, 0, "full", 10, 0, 0),
    ("conv_pw_kernel<80, 5, 2, 0>", "", F, 3, 17, 13, "80", 80, 1, 1, 0, "plain", 10, 0, 0),
    ("conv_pw_kernel<80, 5, 2, 2>", "", F, 3, 17, 13, "80", 80, 1, 1, 0, "full", 10, 0, 0),
    # stem <EPI, channel tiles of 32>: 32-pixel strips (Wo a multiple of 32), four to a block; 3 x 5 rows: the strip map is off
    ("conv_stem_kernel<0, 1>", "", F, 3, 5, 32, "16", 32, 3, 1, 1, "plain", 0, 0, 0),
    ("conv_stem_kernel<0, 2>", "", F, 3, 5, 32, "16", 48, 3, 1, 1, "plain", 0, 0, 0),
    ("conv_stem_kernel<0, 3>", "", F, 3, 5, 32, "16", 80, 3, 1, 1, "plain", 0, 0, 0),
    ("conv_stem_kernel<1, 1>", "", F, 3, 5, 32, "16", 32, 3, 1, 1, "stats", 0, 0, 0),
    ("conv_stem_kernel<1, 2>", "", F, 3, 5, 32, "16", 48, 3, 1, 1, "stats", 0, 0, 0),
    ("conv_stem_kernel<2, 1>", "", F, 3, 5, 32, "16", 32, 3, 1, 1, "bn", 0, 0, 0),
    ("conv_stem_kernel<2, 2>", "", F, 3, 5, 32, "16", 48, 3, 1, 1, "bn", 0, 0, 0),
    ("conv_stem_kernel<2, 3>", "", F, 3, 5, 32, "16", 80, 3, 1, 1, "bn", 0, 0, 0),
    # register-staged kernel <BN, waves, waves, min waves, EPI, k-step>
    ("conv_v2_kernel<128, 4, 2, 4, 0, 32>", "", F, 3, 17, 13, "16", 160, 3, 1, 1, "plain", 0, 0, 0),
    ("conv_v2_kernel<128, 4, 2, 4, 0, 64>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "plain", 0, 0, 0),
    ("conv_v2_kernel<128, 4, 2, 4, 1, 32>", "", F, 3, 17, 13, "16", 160, 3, 1, 1, "stats", 0, 0, 0),
    ("conv_v2_kernel<128, 4, 2, 4, 1, 64>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "stats", 0, 0, 0),
    ("conv_v2_kernel<128, 4, 2, 4, 2, 32>", "", F, 3, 17, 13, "16", 160, 3, 1, 1, "full", 0, 0, 0),
    ("conv_v2_kernel<128, 4, 2, 4, 2, 64>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "full", 0, 0, 0),
    ("conv_v2_kernel<128, 4, 2, 4, 3, 32>", "", D, 3, 17, 13, "16", 160, 3, 1, 1, "bnr", 0, 0, 0),
    ("conv_v2_kernel<128, 4, 2, 4, 3, 64>", "", D, 3, 17, 13, "64", 160, 3, 1, 1, "bnr", 0, 0, 0),
    ("conv_v2_kernel<32, 4, 1, 4, 0, 32>", "", F, 3, 17, 13, "16", 24, 3, 1, 1, "plain", 0, 0, 0),
    ("conv_v2_kernel<32, 4, 1, 4, 1, 32>", "", F, 3, 17, 13, "16", 24, 3, 1, 1, "stats", 0, 0, 0),
    ("conv_v2_kernel<32, 4, 1, 4, 2, 32>", "", F, 3, 17, 13, "16", 24, 3, 1, 1, "full", 0, 0, 0),
    ("conv_v2_kernel<32, 4, 1, 4, 3, 32>", "", D, 3, 17, 13, "16", 24, 3, 1, 1, "bnr", 0, 0, 0),
    ("conv_v2_kernel<64, 4, 1, 3, 0, 32>", "", F, 3, 17, 13, "16", 48, 3, 1, 1, "plain", 0, 0, 0),
    ("conv_v2_kernel<64, 4, 1, 3, 1, 32>", "", F, 3, 17, 13, "16", 48, 3, 1, 1, "stats", 0, 0, 0),
    ("conv_v2_kernel<64, 4, 1, 3, 2, 32>", "", F, 3, 17, 13, "16", 48, 3, 1, 1, "full", 0, 0, 0),
    ("conv_v2_kernel<64, 4, 1, 3, 3, 32>", "", D, 3, 17, 13, "16", 48, 3, 1, 1, "bnr", 0, 0, 0),
    # LDS-DMA ring kernel <BM, BN, waves, waves, k-step, stages, EPI, tail>
    ("conv_v3_kernel<128, 128, 2, 2, 32, 4, 0, false>", "", F, 3, 17, 13, "96", 160, 3, 1, 1, "plain", 3, 32, 0),
    ("conv_v3_kernel<128, 128, 2, 2, 32, 4, 1, false>", "", F, 3, 17, 13, "32+64", 160, 3, 1, 1, "stats", 3, 0, 0),
    ("conv_v3_kernel<128, 128, 2, 2, 32, 4, 2, false>", "", F, 3, 17, 13, "96", 160, 3, 1, 1, "full", 3, 32, 0),
    ("conv_v3_kernel<128, 128, 2, 2, 32, 4, 3, false>", "", D, 3, 17, 13, "96", 160, 3, 1, 1, "bnr", 3, 32, 0),
    ("conv_v3_kernel<128, 128, 2, 2, 64, 2, 0, false>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "plain", 3, 0, 0),
    ("conv_v3_kernel<128, 128, 2, 2, 64, 2, 0, true>", "", F, 3, 17, 13, "80", 160, 3, 1, 1, "plain", 3, 0, 0),
    ("conv_v3_kernel<128, 128, 2, 2, 64, 2, 1, false>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "stats", 3, 0, 0),
    ("conv_v3_kernel<128, 128, 2, 2, 64, 2, 1, true>", "", F, 3, 17, 13, "80", 160, 3, 1, 1, "stats", 3, 0, 0),
    ("conv_v3_kernel<128, 128, 2, 2, 64, 2, 2, false>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "full", 3, 0, 0),
    ("conv_v3_kernel<128, 128, 2, 2, 64, 2, 2, true>", "", F, 3, 17, 13, "80", 160, 3, 1, 1, "full", 3, 0, 0),
    ("conv_v3_kernel<128, 128, 2, 2, 64, 2, 3, false>", "", D, 3, 17, 13, "64", 160, 3, 1, 1, "bnr", 3, 0, 0),
    ("conv_v3_kernel<128, 128, 2, 2, 64, 2, 3, true>", "", D, 3, 17, 13, "80", 160, 3, 1, 1, "bnr", 3, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 32, 4, 0, false>", "", F, 3, 17, 13, "96", 48, 3, 1, 1, "plain", 4, 32, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 32, 4, 1, false>", "", F, 3, 17, 13, "32+64", 48, 3, 1, 1, "stats", 4, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 32, 4, 2, false>", "", F, 3, 17, 13, "96", 48, 3, 1, 1, "full", 4, 32, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 32, 4, 3, false>", "", D, 3, 17, 13, "96", 48, 3, 1, 1, "bnr", 4, 32, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 64, 3, 0, false>", "", F, 3, 17, 13, "64", 48, 3, 1, 1, "plain", 4, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 64, 3, 0, true>", "", F, 3, 17, 13, "80", 48, 3, 1, 1, "plain", 4, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 64, 3, 1, false>", "", F, 3, 17, 13, "64", 48, 3, 1, 1, "stats", 4, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 64, 3, 1, true>", "", F, 3, 17, 13, "80", 48, 3, 1, 1, "stats", 4, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 64, 3, 2, false>", "", F, 3, 17, 13, "64", 48, 3, 1, 1, "full", 4, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 64, 3, 2, true>", "", F, 3, 17, 13, "80", 48, 3, 1, 1, "full", 4, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 64, 3, 3, false>", "", D, 3, 17, 13, "64", 48, 3, 1, 1, "bnr", 4, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 64, 3, 3, true>", "", D, 3, 17, 13, "80", 48, 3, 1, 1, "bnr", 4, 0, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 32, 4, 0, false>", "", F, 3, 17, 13, "96", 160, 3, 1, 1, "plain", 2, 32, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 32, 4, 1, false>", "", F, 3, 17, 13, "32+64", 160, 3, 1, 1, "stats", 2, 0, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 32, 4, 2, false>", "", F, 3, 17, 13, "96", 160, 3, 1, 1, "full", 2, 32, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 32, 4, 3, false>", "", D, 3, 17, 13, "96", 160, 3, 1, 1, "bnr", 2, 32, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 64, 3, 0, false>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "plain", 2, 0, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 64, 3, 0, true>", "", F, 3, 17, 13, "80", 160, 3, 1, 1, "plain", 2, 0, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 64, 3, 1, false>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "stats", 2, 0, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 64, 3, 1, true>", "", F, 3, 17, 13, "80", 160, 3, 1, 1, "stats", 2, 0, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 64, 3, 2, false>", "", F, 3, 17, 13, "64", 160, 3, 1, 1, "full", 2, 0, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 64, 3, 2, true>", "", F, 3, 17, 13, "80", 160, 3, 1, 1, "full", 2, 0, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 64, 3, 3, false>", "", D, 3, 17, 13, "64", 160, 3, 1, 1, "bnr", 2, 0, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 64, 3, 3, true>", "", D, 3, 17, 13, "80", 160, 3, 1, 1, "bnr", 2, 0, 0),
    ("conv_v3_kernel<256, 256, 2, 4, 64, 2, 0, false>", "", F, 3, 17, 13, "64", 256, 3, 1, 1, "plain", 14, 0, 0),
    ("conv_v3_kernel<256, 256, 2, 4, 64, 2, 1, false>", "", F, 3, 17, 13, "64", 256, 3, 1, 1, "stats", 14, 0, 0),
    ("conv_v3_kernel<256, 256, 2, 4, 64, 2, 2, false>", "", F, 3, 17, 13, "64", 256, 3, 1, 1, "full", 14, 0, 0),
    ("conv_v3_kernel<256, 256, 2, 4, 64, 2, 3, false>", "", D, 3, 17, 13, "64", 256, 3, 1, 1, "bnr", 14, 0, 0),
    # ---- launch-shape branches of conv_plan: which block handles which pixel
    # stride-2 data gradient on conv_v2_kernel: a block walks the four parity classes of its regions itself from 256 regions per
    # class on (CLS_INNER_MIN_TILES: 2 x 256 x 256 pixels), below that one grid slot per (class, tap slot)
    ("conv_v2_kernel<32, 4, 1, 4, 3, 32>", "class-walk", D, 2, 256, 256, "64", 32, 3, 2, 1, "bnr", 1, 0, 0),
    ("conv_v2_kernel<32, 4, 1, 4, 3, 32>", "class-slots", D, 2, 32, 32, "64", 32, 3, 2, 1, "bnr", 1, 0, 0),
    ("conv_v2_kernel<32, 4, 1, 4, 2, 32>", "class-slots-acc", D, 3, 18, 14, "64", 24, 3, 2, 1, "acc", 1, 0, 0),
    # ... and on an odd grid, where the plan leaves the parity-class form
    ("conv_v2_kernel<64, 4, 1, 3, 3, 32>", "odd-grid", D, 3, 17, 13, "64", 48, 3, 2, 1, "bnr", 1, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 64, 3, 3, false>", "classes", D, 3, 18, 14, "64", 48, 3, 2, 1, "bnr", 4, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 64, 3, 3, false>", "odd-grid", D, 3, 17, 13, "64", 48, 3, 2, 1, "bnr", 4, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 64, 3, 2, true>", "classes-acc", D, 3, 18, 14, "80", 48, 3, 2, 1, "acc", 4, 0, 0),
    # the stem's XCD-aware strip map (ConvK.xgx): a multiple of 8 blocks and B * Ho a multiple of 8 * STEM_BAND
    ("conv_stem_kernel<1, 2>", "strip-map", F, 2, 32, 32, "16", 48, 3, 1, 1, "stats", 0, 0, 0),
    ("conv_stem_kernel<2, 3>", "strip-map", F, 2, 32, 32, "16", 80, 3, 1, 1, "bn", 0, 0, 0),
    # the halo kernel's XCD-major block order over more workgroups than XCDs (5 patches x 2 channel tiles: 8 XCD ranges of 2 and 1)
    ("conv_halo_kernel<128, 2, false>", "xcd-major", F, 5, 17, 13, "64", 160, 3, 1, 1, "full", 5, 0, 0),
    # ---- the other tail: a last block of 48 channels (112 = 64 + 48) where the rows above take 16
    ("conv_halo_kernel<128, 1, true>", "tail-48", F, 3, 17, 13, "112", 160, 3, 1, 1, "stats", 5, 0, 0),
    ("conv_halo_kernel<64, 3, true>", "tail-48", D, 3, 17, 13, "112", 48, 3, 1, 1, "bnr", 5, 0, 0),
    ("conv_v3_kernel<256, 128, 4, 2, 64, 3, 1, true>", "tail-48", F, 3, 17, 13, "112", 160, 3, 1, 1, "stats", 2, 0, 0),
    ("conv_v3_kernel<128, 128, 2, 2, 64, 2, 2, true>", "tail-48", F, 3, 17, 13, "64+48", 160, 3, 1, 1, "full", 3, 0, 0),
    ("conv_v3_kernel<128, 64, 2, 2, 64, 3, 3, true>", "tail-48", D, 3, 17, 13, "112", 48, 3, 1, 1, "bnr", 4, 0, 0),
]


class Row(collections.namedtuple("Row", "name tag mode B H W segs N k stride pad epi algo tile_k tile_n")):
    __slots__ = ()

    @property
    def id(self):
        return self.name + ("/" + self.tag if self.tag else "")

    @property
    def cap(self):
        """the family's plan honours grid_cap (the persistent-walk repeat of the GPU test)"""
        return not self.name.startswith(IGNORES_GRID_CAP)

    @property
    def seg_list(self):
        """[(C, ld, ups)]"""
        return [(int(s.rstrip("^")), int(s.rstrip("^")) + 2 * PAD, int(s.endswith("^"))) for s in self.segs.split("+")]

    @property
    def in_hw(self):
        """the map the segments are read from (D: the output gradient's)"""
        if self.mode == F:
            return (self.H - 1) * self.stride + self.k - 2 * self.pad, (self.W - 1) * self.stride + self.k - 2 * self.pad
        return (self.H + 2 * self.pad - self.k) // self.stride + 1, (self.W + 2 * self.pad - self.k) // self.stride + 1

    @property
    def nsplit(self):
        """columns of the first destination: half of N in whole groups of 8 under the split epilogue"""
        return self.N // 16 * 8 if self.epi == "full" else self.N

    def case(self, **over):
        """the row as a case of conv_plan_table.py (make_desc(case): the descriptor with fake operands)"""
        segs = self.seg_list
        Hi, Wi = self.in_hw
        N, n0 = self.N, self.nsplit
        e = self.epi
        c = dict(mode=self.mode, B=self.B, Ho=self.H, Wo=self.W, Hi=Hi, Wi=Wi, KH=self.k, KW=self.k, stride=self.stride, pad=self.pad,
                 N=N, Npad=(N + 127) // 128 * 128, nseg=len(segs), C0=segs[0][0], lds0=segs[0][1], ups0=segs[0][2], C1=0, lds1=0, ups1=0,
                 ld0=n0 + 2 * PAD, nsplit=n0, ld1=N - n0 + 2 * PAD if n0 < N else 0, ldr=n0 + PAD if e in ("full", "one") else 0,
                 accumulate=int(e == "acc"), stats=int(e in ("stats", "gstats")), res=int(e in ("full", "one")),
                 act=int(e in ("full", "one", "nores", "bn")), bias=int(e in ("full", "one", "nores", "gstats")),
                 scale=int(e in ("full", "one", "nores", "bn")), shift=int(e in ("full", "one", "nores", "bn")), bnr=int(e == "bnr"),
                 bnr_ldz=N + PAD if e == "bnr" else 0, bnr_C=N + PAD if e == "bnr" else 0, tile_k=self.tile_k, tile_n=self.tile_n,
                 grid_cap=0, algo=self.algo, ptrs=0)
        if len(segs) == 2:
            c.update(C1=segs[1][0], lds1=segs[1][1], ups1=segs[1][2])
        c.update(over)
        return c


ROWS = [Row(*r) for r in _ROWS]


def plan(L, case):
    """(rc, name, stat_rows, bnr_rows) of yh_conv_info for a case: no device needed"""
    from yoloseries_amd._lib import ConvInfo
    o = ConvInfo()
    rc = L.yh_conv_info(C.byref(T.make_desc(case)), C.byref(o))
    return rc, o.name.decode(), o.stat_rows, o.bnr_rows


def silu_bwd_sums(g, z, scale, shift):
    """what the fused BatchNorm-backward reduction sums per channel over the stored gradient g [M][C]: dz = g * silu'(z * scale + shift);
    returns (sum dz, sum dz * z, sum |dz|, sum |dz * z|) in float64 (the last two scale the comparison's absolute bar)"""
    g, z = g.double(), z.double()
    a = z * scale.double() + shift.double()
    sg = a.sigmoid()
    dz = g * (sg * (1 + a * (1 - sg)))
    return dz.sum(0), (dz * z).sum(0), dz.abs().sum(0), (dz * z).abs().sum(0)


def silu_bwd_sums_close(slab, g, z, scale, shift):
    """the slab [rows][2][C] of a fused reduction against silu_bwd_sums of the stored gradient: 2e-3 relative + 2e-3 of the largest
    column's sum of magnitudes (the bar of tests/test_gpu_conv.py::_dgrad_check)"""
    import torch
    s0, s1, a0, a1 = silu_bwd_sums(g, z, scale, shift)
    got = slab.double().sum(0)
    return (torch.allclose(got[0], s0, rtol=2e-3, atol=2e-3 * a0.max().item()) and
            torch.allclose(got[1], s1, rtol=2e-3, atol=2e-3 * a1.max().item()))
