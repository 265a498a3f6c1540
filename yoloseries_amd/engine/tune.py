"""Tuner: the launch-parameter tables (shipped + per-machine) and the per-layer timing of the eligible kernel families
(Program._tune_conv / _tune_wgrad_splits), as a mixin of engine.program.Program."""
import ctypes as C
import json
import os

import torch

from .._lib import CONV_ALGO_FAMILY, YH_CONV_DGRAD, YH_WGRAD_PATCH, YH_WGRAD_WAVE, ConvInfo, WgradInfo, check
from . import flags as _flags

# the table shipped with the package lives beside the package modules
TUNE_DEFAULTS_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tune_defaults.json")


def _tune_cache_path():
    """per-machine timings live in the user's cache directory, not in the package (YH_TUNE_CACHE overrides)"""
    base = os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache")
    return os.environ.get("YH_TUNE_CACHE", os.path.join(base, "yoloseries_amd", "tune_cache.json"))


class _TuneTable:
    """launch parameters per layer shape.  Two layers, never mixed: the shipped table for the BASELINE configurations
    (tune_defaults.json, timed on an MI355X with tools/make_tune_defaults.sh: the same choices on every box, no tuning launches in
    the first steps; read-only) and what THIS machine timed itself for other shapes (a small JSON file, kept across processes).
    A lookup asks the local layer first, then the shipped one; only locally timed keys are ever written back, so a later
    release of tune_defaults.json is not shadowed by a frozen copy of the old one.  YH_TUNE_DEFAULTS=0 ignores the shipped table."""

    def __init__(self):
        self.shipped, self.local, self.dirty = {}, {}, False
        if os.environ.get("YH_TUNE_DEFAULTS", "1") != "0":
            self.shipped = self._read(TUNE_DEFAULTS_PATH)
        self.local = self._read(_tune_cache_path())
        self.hits_shipped = self.hits_local = self.timed = 0

    @staticmethod
    def _read(path):
        try:
            with open(path) as f:
                return dict(json.load(f))
        except (OSError, ValueError):
            return {}

    def __contains__(self, key):
        return key in self.local or key in self.shipped

    def __getitem__(self, key):
        if key in self.local:
            self.hits_local += 1
            return self.local[key]
        self.hits_shipped += 1
        return self.shipped[key]

    def __setitem__(self, key, value):
        self.local[key] = value
        self.timed += 1
        self.dirty = True

    def save(self):
        if not self.dirty:
            return
        self.dirty = False
        path = _tune_cache_path()
        try:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            tmp = f"{path}.{os.getpid()}.tmp"
            with open(tmp, "w") as f:
                json.dump(self.local, f, indent=0, sort_keys=True)
            os.replace(tmp, path)
        except OSError:
            pass                               # read-only install: tune again next time


def _tune_cache():
    if _tune_cache.data is None:
        _tune_cache.data = _TuneTable()
    return _tune_cache.data


_tune_cache.data = None


def _tune_cache_save():
    if _tune_cache.data is not None:
        _tune_cache.data.save()


def tuning_source():
    """where the launch parameters of this process came from (reported by bench.py)"""
    t = _tune_cache()
    return {"shipped_table": t.hits_shipped, "local_cache": t.hits_local, "timed_now": t.timed}

# version prefixes of the tuning-table keys: bumped when the candidates or the meaning of a tuned value change, so that stale
# entries of a shipped / cached table are not applied.  Stride-2 data gradients carry their own version (conv_dg2_kernel, algo 7,
# joined their candidates in round 3), and so do weight gradients that leave through the partial-tile workspace.
KEY_CONV, KEY_CONV_S2D, KEY_CONV_P3, KEY_CONV_EVAL, KEY_WGRAD, KEY_WGRAD_WS = "conv6", "conv7", "conv8", "conv9", "wgrad10", "wgrad11"   # wgrad11: conv_wgs_kernel's workspace form joined the workspace candidates (wgrad8 entries never saw it)
KEY_CONV_C80 = "conv10"        # inference 3x3 layers with 80 -> 160 channels: conv_c80_kernel (algo 12) joined their candidates in round 4
KEY_CONV_PT = "conv11"         # 1x1 layers conv_pt_kernel (algo 13) takes: training with 128 / 256 / 512 input channels, inference with 320 (round 5)
KEY_CONV_H160 = "conv14"       # inference 3x3 / stride-1 layers with N a multiple of 160: re-timed against the FINAL conv_halo160_kernel of round 5 (16 x 16 tiles, pipelined sub-steps): it now takes every one of them, also the 640-channel layers the conv12 entries had left on conv_halo_kernel
TUNE_KEY_VERSIONS = frozenset((KEY_CONV, KEY_CONV_S2D, KEY_CONV_P3, KEY_CONV_EVAL, KEY_CONV_C80, KEY_CONV_PT, KEY_CONV_H160, KEY_WGRAD, KEY_WGRAD_WS, KEY_WGRAD + "f", KEY_WGRAD_WS + "f"))


class TunerMixin:
    """timed choice of kernel family / launch parameters per layer shape (mixed into Program)"""

    def _tune_conv(self, d, kind, name, stats_ok=False):
        """Launch parameters of one conv / dgrad launch — kernel family (register-staged conv_v2 or LDS-DMA conv_v3 with one
        of its tiles), k-step width, cap on persistent blocks — timed once when the program is built: the best setting
        differs per layer shape by 5-40 % (YH_CONV_TUNE=0: library defaults).  Results never change (identical math);
        only the number of BatchNorm partial-sum rows follows the grid."""
        if os.environ.get("YH_CONV_TUNE", "1") == "0":
            return
        key = self._conv_tune_key(d, kind, stats_ok)
        cache = _tune_cache()
        if key in cache:
            d.tile_k, d.grid_cap, d.algo = (int(v) for v in cache[key])
            return
        L = self.L
        cands = self._conv_candidates(L, d, kind)
        # scratch operands big enough for every grid tried below (the head gradient pointer is filled in at run time)
        infos = [self._conv_info(L, d, *c) for c in cands]
        rows_max = max([1] + [o.stat_rows for o in infos])
        bnr_max = max([1] + [o.bnr_rows for o in infos]) if d.bnr_part else 1
        saved = (d.seg[0].ptr, d.stats, d.bnr_part)
        if not d.seg[0].ptr:
            d.seg[0].ptr = self.gy_scratch.data_ptr()
        if stats_ok:
            tmp_stats = torch.zeros(rows_max + 8, 2, d.Npad, dtype=torch.float32, device=self.dev)
            d.stats = tmp_stats.data_ptr()
        if d.bnr_part:
            tmp_part = torch.zeros((bnr_max + 8) * 2 * d.N, dtype=torch.float32, device=self.dev)
            d.bnr_part = tmp_part.data_ptr()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        best, best_ms = (0, 0, 1), None
        for algo, tk, cap in cands:
            d.algo, d.tile_k, d.grid_cap = algo, tk, cap
            check(L.yh_conv_igemm(C.byref(d), st), f"yh_conv_igemm tune [{name}]")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(_flags.TUNE_ITERS):
                L.yh_conv_igemm(C.byref(d), st)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if best_ms is None or ms < best_ms * (0.97 if _flags.TUNE_ITERS < 8 else 0.99):   # keep the earlier candidate unless clearly better
                best, best_ms = (tk, cap, algo), ms
        d.tile_k, d.grid_cap, d.algo = best
        d.seg[0].ptr, d.stats, d.bnr_part = saved
        cache[key] = [int(best[0]), int(best[1]), int(best[2])]

    @staticmethod
    def _conv_info(L, d, algo=None, tile_k=None, grid_cap=None):
        """the library's plan for this descriptor (yh_conv_info), optionally with other launch parameters asked; no device needed"""
        o, saved = ConvInfo(), (d.algo, d.tile_k, d.grid_cap)
        d.algo, d.tile_k, d.grid_cap = (s if v is None else v for v, s in zip((algo, tile_k, grid_cap), saved))
        L.yh_conv_info(C.byref(d), C.byref(o))             # (the rc speaks of operands: the callers want the plan)
        d.algo, d.tile_k, d.grid_cap = saved
        return o

    @staticmethod
    def _conv_tune_key(d, kind, stats_ok):
        """key of this launch in the tuning tables: a version prefix by the candidates the layer has (TUNE_KEY_VERSIONS), the kind
        of launch, and every descriptor field a timing depends on"""
        one = d.nseg == 1
        c0 = d.seg[0].C
        ctot = c0 + (d.seg[1].C if d.nseg > 1 else 0)
        pointwise = d.KH == 1 and d.stride == 1
        if d.mode == YH_CONV_DGRAD and d.stride == 2:
            prefix = KEY_CONV_S2D
        elif kind != 'eval':
            small3 = d.KH == 3 and d.stride == 1 and one and c0 <= 128 and d.N <= 128
            pt = pointwise and ctot in (128, 256, 512) and (one or c0 == d.seg[1].C)
            prefix = KEY_CONV_P3 if small3 else (KEY_CONV_PT if pt else KEY_CONV)
        else:
            c80 = d.KH == 3 and one and c0 == 80 and d.N == 160
            h160 = d.KH == 3 and d.stride == 1 and one and d.N % 160 == 0 and c0 >= 64 and c0 % 32 == 0
            pte = pointwise and one and ctot == 320 and d.nsplit >= d.N     # conv_pt_kernel's inference form
            prefix = KEY_CONV_C80 if c80 else (KEY_CONV_H160 if h160 else (KEY_CONV_PT if pte else KEY_CONV_EVAL))
        return f"{prefix}:{kind}:" + ",".join(str(int(v)) for v in (
            d.mode, d.B, d.Ho, d.Wo, d.Hi, d.Wi, d.KH, d.stride, d.pad, d.N, d.nseg, d.seg[0].C, d.seg[0].ld, d.seg[0].ups,
            d.seg[1].C if d.nseg > 1 else 0, d.seg[1].ups if d.nseg > 1 else 0, d.ld0, d.nsplit, d.accumulate, int(bool(d.stats or stats_ok)),
            int(bool(d.res)), d.act, int(bool(d.bias)), int(bool(d.scale)), int(bool(d.bnr_part)), 0))

    @staticmethod
    def _conv_candidates(L, d, kind):
        """[(algo, tile_k, grid_cap)] _tune_conv times for this descriptor, in that order.  Which requests the library would honour
        is read from its plan (CONV_ALGO_FAMILY); which of them are worth timing is decided here.  Needs no device, leaves d alone."""
        info = lambda algo, tk=0, cap=0: TunerMixin._conv_info(L, d, algo, tk, cap)     # noqa: E731
        whole = lambda n: all(d.seg[i].C % n == 0 for i in range(d.nseg))               # noqa: E731
        base = info(1).stat_rows
        cands = []
        for tk in ((0, 32) if whole(64) and d.N > 64 else (0,)):
            for cap in (0, 2 * base):
                if cap and info(1, tk, cap).stat_rows == base:
                    continue                       # fewer tiles than blocks: the cap changes nothing
                cands.append((1, tk, cap))
        if os.environ.get("YH_CONV_V3", "1") == "0":
            return cands
        for algo in (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14):
            if str(algo) in _flags.SKIP_ALGOS:
                continue
            o = info(algo)
            if (o.family, o.variant) != CONV_ALGO_FAMILY[algo]:
                continue                           # not eligible: the library would run its default
            cands.append((algo, 0, 0))
            if algo < 5 and o.tail and whole(32):
                cands.append((algo, 32, 0))        # ragged last channel block: 32-channel steps instead of 64 + tail
        return cands

    def _kernel_name(self, d):
        """instantiation yh_conv_igemm launches for descriptor d, spelled as rocprofv3 prints it"""
        return self._conv_info(self.L, d).name.decode()

    def _tune_wgrad_splits(self, wd, M, ntile, op):
        """Split-M factor (and, for the wide 64-row tilings, the pixels per k-step) of one weight-gradient launch.  The best
        total block count depends on the tile configuration's residency and on how the atomics of the epilogue amortise
        (measured 256..1024 blocks, up to 1.6x apart), so it is timed once per layer when the backward program is built
        (YH_WGRAD_TUNE=0: fixed 512-block rule).  Sets wd.tile_k, returns the split factor."""
        if os.environ.get("YH_WGRAD_TUNE", "1") == "0":
            return self._wgrad_splits_for(self.L, wd, M, ntile, 512)
        key = f"{KEY_WGRAD_WS if wd.partial else KEY_WGRAD}{'f' if wd.bn_z else ''}:" + ",".join(str(int(v)) for v in (wd.N, wd.ldg, wd.seg.C, wd.seg.ld, wd.seg.ups, wd.Ctot, wd.B, wd.Ho, wd.Wo,
                                                          wd.Hi, wd.Wi, wd.KH, wd.stride, wd.pad))
        cache = _tune_cache()
        if key in cache:
            sp, tk = (int(v) for v in cache[key])
            wd.splits, wd.tile_k = sp, tk
            if not wd.partial or self.L.yh_conv_wgrad_ws_bytes(C.byref(wd)) <= wd.partial_bytes:
                return sp                  # (a choice timed with a larger workspace than this program's is timed again)
        gy_saved = wd.gy
        if not wd.gy:                      # head gradient arrives at run time: time against the scratch buffer
            if self.gy_scratch.numel() < M * wd.ldg:
                return self._wgrad_splits_for(self.L, wd, M, ntile, 512)
            wd.gy = self.gy_scratch.data_ptr()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        best, best_ms = None, None
        for tk, sps in self._wgrad_candidates(self.L, wd, M, ntile):
            wd.tile_k = tk
            for sp in sps:
                wd.splits = sp
                if wd.partial and self.L.yh_conv_wgrad_ws_bytes(C.byref(wd)) > wd.partial_bytes:
                    continue                   # more partial tiles than the workspace holds
                check(self.L.yh_conv_wgrad(C.byref(wd), st), f"yh_conv_wgrad tune [{op.name}]")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(_flags.TUNE_ITERS):
                    self.L.yh_conv_wgrad(C.byref(wd), st)
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                if best_ms is None or ms < best_ms:
                    best, best_ms = (sp, tk), ms
        wd.gy = gy_saved
        wd.tile_k = best[1]
        self.wgrad_tuned[(op.name, wd.coff_k)] = (best[0], best_ms / _flags.TUNE_ITERS)
        cache[key] = [int(best[0]), int(best[1])]
        return best[0]

    @staticmethod
    def _wgrad_info(L, wd, tile_k=None):
        """the library's plan for this descriptor (yh_conv_wgrad_info), optionally with another tile_k asked; no device needed"""
        o, saved = WgradInfo(), wd.tile_k
        if tile_k is not None:
            wd.tile_k = tile_k
        L.yh_conv_wgrad_info(C.byref(wd), C.byref(o))      # (the rc speaks of operands and workspace: the callers want the plan)
        wd.tile_k = saved
        return o

    @staticmethod
    def _wgrad_splits_for(L, wd, M, ntile, total, tk=0):
        nt = L.yh_conv_wgrad_tiles2(wd.N, wd.KH * wd.KW * wd.seg.C, tk) if tk == 128 else ntile
        return max(1, min((M + 255) // 256, (total + nt - 1) // nt))

    @staticmethod
    def _wgrad_candidates(L, wd, M, ntile):
        """[(tile_k, [splits ...])] _tune_wgrad_splits times for this descriptor, in that order.  Which requests the library would
        honour is read from its plan; which of them are worth timing is decided here.  Needs no device."""
        honoured = lambda tk: TunerMixin._wgrad_info(L, wd, tk).tile_k == tk     # noqa: E731
        tks = (0, 64) if honoured(64) else (0,)
        if honoured(32):
            tks = tks + (32, 35)            # the general tiling with 32-pixel k-steps (two blocks per CU): 8 waves of 32 x 64 / 4 of 64 x 64
        if honoured(128) and wd.N > 32 and not wd.bn_z:
            tks = tks + (128,)              # the general 128-column tiling on a layer that defaults to a wide one
        if not wd.partial and TunerMixin._wgrad_info(L, wd, 40).form == YH_WGRAD_PATCH:
            tks = tks + (40,)               # patch form (conv_wgp_kernel): the input patch of a pixel region staged once in LDS
        wave = TunerMixin._wgrad_info(L, wd, 129)
        wtiles = wave.tiles if wave.form == YH_WGRAD_WAVE and not wd.bn_z and os.environ.get("YH_WGRAD_WAVE", "1") != "0" else 0
        if wtiles > 0:
            tks = tks + (129,)              # wave-private 128 x 128 tiles + stream-K (conv_wgs_kernel): `splits` = workgroups, one per CU;
                                            # with a workspace its slot form (same workgroup counts: G + tiles - 1 slots of 64 KB)
        cands = []
        for tk in tks:
            if tk == 129:                   # an exact tiles x splits grid where it fills the chip, else 256 workgroups dealt (tile, 32 pixels) units
                # Workgroups (= CUs: the form holds a whole CU) a weight gradient may take.  Alone on the chip 256 is fastest; in the
                # two-stream backward the main chain runs beside it, and its short latency-bound kernels (finalize launches, small
                # layers) wait for a CU while a weight gradient holds all of them: the YOLOv5s step is shortest when the weight
                # gradients leave a quarter of the CUs alone (12.00 -> 11.90 ms), the YOLOv5l step — long kernels on both streams —
                # when its big layers take the whole chip (43.36 -> 42.82 ms): layers under 60 GFLOP get 192, the others 256
                # (profiles/r04_step_experiments.txt d).  Half of the budget is timed too: on the small layers the atomics (one
                # partial tile per workgroup) dominate.
                wflops = 2.0 * M * wd.N * wd.KH * wd.KW * wd.seg.C
                gmax = int(os.environ.get("YH_WGS_G", "256" if wflops >= 60e9 else "192"))
                sps = set()
                for g in (gmax, gmax // 2):
                    sps |= {g} | ({wtiles * (g // wtiles)} if wtiles <= g else set())
                sps = sorted(sps)
            else:
                sps = [1024] if tk == 40 else sorted({TunerMixin._wgrad_splits_for(L, wd, M, ntile, t, tk) for t in (256, 512, 768, 1024, 1536)})
            cands.append((tk, sps))
        return cands

    @staticmethod
    def _wgrad_name(L, wd):
        """instantiation yh_conv_wgrad launches for this descriptor, profiler spelling"""
        return TunerMixin._wgrad_info(L, wd).name.decode()
