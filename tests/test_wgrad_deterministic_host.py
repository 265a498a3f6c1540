"""Host side of the deterministic weight gradients (no device needed): the workspace size of conv_wgs_kernel's slot form against a
restatement over the layer corpus of tools/conv_plan_table.py, the resource usage of the new instantiations, the public switch."""
import ctypes as C
import importlib.util
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 128 * 128 * 4


def _corpus():
    """weight-gradient descriptors (one per input segment) of every layer the shipped table knows: the forward entries
    tools/conv_plan_table.py walks and the table's own weight-gradient keys"""
    from yoloseries_amd._lib import WgradDesc
    spec = importlib.util.spec_from_file_location("conv_plan_table", os.path.join(ROOT, "tools", "conv_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def desc(N, ldg, Cseg, ld, ups, Ctot, coff, B, Ho, Wo, Hi, Wi, k, stride, pad):
        d = WgradDesc()
        d.N, d.ldg = N, ldg
        d.seg.C, d.seg.ld, d.seg.ups = Cseg, ld, ups
        d.coff_k, d.Ctot = coff, Ctot
        d.B, d.Ho, d.Wo, d.Hi, d.Wi = B, Ho, Wo, Hi, Wi
        d.KH = d.KW = k
        d.stride, d.pad = stride, pad
        return d
    out = []
    for _, f, _v in mod.table_keys():
        c = mod.case_of_key(f)
        if c["mode"] != 0:
            continue
        ctot = c["C0"] + (c["C1"] if c["nseg"] > 1 else 0)
        ldg = (c["N"] + 7) // 8 * 8
        out.append(desc(c["N"], ldg, c["C0"], c["lds0"], c["ups0"], ctot, 0, c["B"], c["Ho"], c["Wo"], c["Hi"], c["Wi"], c["KH"], c["stride"], c["pad"]))
        if c["nseg"] > 1:
            out.append(desc(c["N"], ldg, c["C1"], c["lds1"], c["ups1"], ctot, c["C0"], c["B"], c["Ho"], c["Wo"], c["Hi"], c["Wi"], c["KH"], c["stride"], c["pad"]))
    with open(os.path.join(ROOT, "yoloseries_amd", "tune_defaults.json")) as fh:
        for key in sorted(json.load(fh)):
            if key.startswith("wgrad10:"):
                N, ldg, Cs, ld, ups, Ctot, B, Ho, Wo, Hi, Wi, k, stride, pad = (int(v) for v in key.split(":")[1].split(","))
                out.append(desc(N, ldg, Cs, ld, ups, Ctot, 0, B, Ho, Wo, Hi, Wi, k, stride, pad))
    return out


def _eligible(d):
    """conv_wgs_kernel's layer rules (csrc/conv_wgs.hip, wgs_plan), restated for well-formed layers"""
    M = d.B * d.Ho * d.Wo
    return (d.N >= 64 and d.seg.C % 32 == 0 and d.seg.ld % 8 == 0 and d.coff_k % 8 == 0 and M % 32 == 0 and d.Ho * d.Wo >= 16 and
            d.stride in (1, 2) and not (d.seg.ups and (d.Hi % 2 or d.Wi % 2)) and
            (M - 1) * d.ldg * 2 < (1 << 31) - 8192 and d.B * (d.Hi >> d.seg.ups) * (d.Wi >> d.seg.ups) * d.seg.ld * 2 < (1 << 31) - 8192)


def test_slot_workspace_bytes_match_the_restated_formula_over_the_layer_corpus():
    from yoloseries_amd._lib import lib
    L = lib()
    corpus = _corpus()
    assert len(corpus) >= 300
    n_el = 0
    for d in corpus:
        d.partial, d.partial_bytes = 16, 1 << 40          # the queries look at the form, never at the memory
        d.tile_k, d.splits = 0, 8
        split_m = L.yh_conv_wgrad_ws_bytes(C.byref(d))     # the split-M formula of conv_wgrad_kernel's form
        d.tile_k = 129
        T = L.yh_conv_wgrad_wave_tiles(C.byref(d))
        assert (T > 0) == _eligible(d), (T, [getattr(d, f) for f, _ in d._fields_[1:18] if f != "seg"], d.seg.C, d.seg.ld)
        if T == 0:
            assert L.yh_conv_wgrad_wave_name(C.byref(d)) == b""
            assert L.yh_conv_wgrad_ws_bytes(C.byref(d)) == split_m
            continue
        n_el += 1
        pw = d.KH == 1 and d.stride == 1 and d.pad == 0 and not d.seg.ups
        assert L.yh_conv_wgrad_wave_name(C.byref(d)).decode() == f"conv_wgs_kernel<{'true' if pw else 'false'}, true>"
        assert T == ((d.N + 127) // 128) * ((d.KH * d.KW * d.seg.C + 127) // 128)
        U = T * (d.B * d.Ho * d.Wo // 32)
        for G in (0, 1, 7, 96, 192, 256, 4096, 100000):
            d.splits = G
            Ge = min(max(G, 1), 4096, U)
            assert L.yh_conv_wgrad_ws_bytes(C.byref(d)) == (Ge + T - 1) * SLOT, (G, Ge, T)
        # the atomic form of the same layer keeps its name; a fused stem backward has no form here
        d.partial = None
        assert L.yh_conv_wgrad_wave_name(C.byref(d)).decode() == f"conv_wgs_kernel<{'true' if pw else 'false'}>"
        d.partial, d.bn_z = 16, 16
        assert L.yh_conv_wgrad_wave_tiles(C.byref(d)) == 0
        d.bn_z = None
    assert n_el >= 100, n_el


def test_workspace_instantiations_use_no_scratch_and_no_more_registers(tmp_path):
    """the accumulators of conv_wgs_kernel fill the AGPRs: an epilogue that copied them to arch VGPRs, or spilled, would change
    the static allocation that decides the kernel's residency.  Resource metadata of the generated code, per instantiation."""
    import subprocess
    src = os.path.join(ROOT, "yoloseries_amd", "csrc", "conv_wgs.hip")
    out = tmp_path / "wgs.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "--cuda-device-only", "-S",
                    "-o", str(out), src], check=True, capture_output=True)
    text = out.read_text()
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        vals = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", blk)}
        vals["agpr_count"] = int(re.match(r"\s+(\d+)", blk).group(1))
        meta[name] = vals
    for pw in ("Lb1E", "Lb0E"):
        atomic = next(v for k, v in meta.items() if f"conv_wgs_kernelI{pw}EEv" in k)
        wsf = next(v for k, v in meta.items() if f"conv_wgs_kernelI{pw}Lb1EEEv" in k)
        assert wsf["private_segment_fixed_size"] == 0 and wsf["vgpr_spill_count"] == 0, wsf
        assert wsf["vgpr_count"] <= atomic["vgpr_count"] and wsf["agpr_count"] <= atomic["agpr_count"], (wsf, atomic)
        assert atomic["private_segment_fixed_size"] == 0 and atomic["vgpr_spill_count"] == 0, atomic
    red = next(v for k, v in meta.items() if "wgs_reduce_kernel" in k)
    assert red["private_segment_fixed_size"] == 0 and red["vgpr_spill_count"] == 0, red


def test_set_deterministic_switches_the_engine_flag_and_the_key_version():
    import yoloseries_amd
    from yoloseries_amd import engine
    assert "set_deterministic" in yoloseries_amd.__all__
    assert engine.KEY_WGRAD_WS == "wgrad11" and {"wgrad11", "wgrad11f"} <= engine.TUNE_KEY_VERSIONS and "wgrad8" not in engine.TUNE_KEY_VERSIONS
    old = engine.flags.WG_WS_BYTES
    try:
        yoloseries_amd.set_deterministic(True)
        assert engine.flags.WG_WS_BYTES == engine.flags.WG_WS_CAP == 256 << 20
        yoloseries_amd.set_deterministic(False)
        assert engine.flags.WG_WS_BYTES == 0
    finally:
        engine.flags.WG_WS_BYTES = old


def test_training_drivers_take_the_deterministic_flag():
    for drv in ("train_yolov5.py",):
        text = open(os.path.join(ROOT, drv)).read()
        assert '"--deterministic"' in text and text.index("set_deterministic(True)") < text.index("Config().get_config")
    assert "train_yolov5.main(argv" in open(os.path.join(ROOT, "train_yolox.py")).read()      # the YOLOX driver parses through it
