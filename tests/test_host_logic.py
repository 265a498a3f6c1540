"""CPU tests of the host side: the C-ABI library loads and exports every symbol the header declares, the
engine's graph builder and weight-packing index maps are correct (checked by emulating the packed GEMMs in
NumPy against torch convolutions), and the synthetic-data generators are deterministic."""
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from yoloseries_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "yolohip.h")).read()
    declared = set(re.findall(r"\b(yh_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"yh_stream", "yh_bf16"}
    L = _lib.lib()                       # raises if any symbol bound in _lib.py is missing
    assert L.yh_version() >= 100
    import ctypes
    raw = ctypes.CDLL(_lib.LIB_PATH)
    missing = [s for s in sorted(declared) if not hasattr(raw, s)]
    assert not missing, f"declared in include/yolohip.h but not exported: {missing}"
    unbound = [s for s in sorted(declared) if s not in _lib.EXPORTED_SYMBOLS]
    assert not unbound, f"declared but not bound in yoloseries_amd/_lib.py: {unbound}"


def test_ctypes_struct_sizes_match_header_layout(tmp_path):
    """the ctypes mirrors (yoloseries_amd/_lib.py) against the C compiler's view of include/yolohip.h: size of every struct and the
    offset of every field, from a probe compiled with gcc"""
    import ctypes as C
    import subprocess
    from yoloseries_amd import _lib
    pairs = [("yh_seg", _lib.Seg), ("yh_conv_desc", _lib.ConvDesc), ("yh_conv_plan_info", _lib.ConvInfo), ("yh_wgrad_desc", _lib.WgradDesc),
             ("yh_wgrad_info", _lib.WgradInfo),
             ("yh_v5loss_desc", _lib.V5LossDesc),
             ("yh_yolox_desc", _lib.YoloxDesc), ("yh_decode_desc", _lib.DecodeDesc), ("yh_bn_fold_item", _lib.BnFoldItem),
             ("yh_bn_part", _lib.BnPart), ("yh_cmd", _lib.Cmd)]
    hdr = open(os.path.join(ROOT, "include", "yolohip.h")).read()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "yolohip.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        body = hdr[hdr.index(f"typedef struct {cname} {{"):hdr.index(f"}} {cname};")]
        for fname, _ in cls._fields_:
            if fname.startswith("reserved") and not re.search(rf"\b{fname}\b", body):
                continue
            assert re.search(rf"\b{fname}\b", body), f"{cname}.{fname} is in the ctypes mirror but not in the header"
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("  return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs:
        assert C.sizeof(cls) == int(want[cname]), f"{cname}: ctypes {C.sizeof(cls)} bytes, C {want[cname]}"
        for fname, _ in cls._fields_:
            key = f"{cname}.{fname}"
            if key in want:
                assert getattr(cls, fname).offset == int(want[key]), f"{key}: ctypes offset {getattr(cls, fname).offset}, C {want[key]}"


def _builder_for(model, B, H, W):
    from yoloseries_amd.engine import Builder
    b = Builder()
    outs = model._yh_build(b, B, H, W)
    return b, outs


def test_v5s_graph_structure():
    from yoloseries_amd import models
    from yoloseries_amd.engine import ConvOp, PoolOp
    m = models.YOLOV5Small(3, 80)
    b, outs = _builder_for(m, 2, 640, 640)
    convs = [o for o in b.ops if isinstance(o, ConvOp)]
    pools = [o for o in b.ops if isinstance(o, PoolOp)]
    # 60 nn.Conv2d in the reference model; the 8 C3 blocks fuse cba1+cba2 into one GEMM -> 52 conv ops
    assert sum(len(o.parts) for o in convs) == 60 and len(convs) == 52 and len(pools) == 3
    macs = sum(2 * o.Ho * o.Wo * o.N * o.k * o.k * (12 if o.focus else o.Ctot) for o in convs) / 2
    assert abs(macs / 1e9 - 8.217) < 0.01, macs            # 8.217 GMAC / image at 640x640
    assert [(o.Ho, o.N) for o in outs] == [(80, 255), (40, 255), (20, 255)]
    # the neck joins read the low-resolution map through the upsampling addressing mode
    ups = [o.name for o in convs if any(s.ups for s in o.segs)]
    assert ups == ["head_stage1_bscp.cba12", "head_stage2_bscp.cba12"]


def _emulate_conv(pk, op, x_nhwc):
    """NumPy emulation of conv_igemm.hip's math from the packed weight image (fp32, no rounding)"""
    off, npad, K = pk.wloc[(op.name, 'fwd')]
    idx = pk.pack_idx_np[off:off + npad * K].reshape(npad, K)
    flat = np.concatenate([p.detach().numpy().reshape(-1) for p in pk.params])
    Wp = np.where(idx >= 0, flat[np.clip(idx, 0, None)], 0.0)[:op.N]
    Bn, H, W, Cn = x_nhwc.shape
    k, s, p = op.k, op.stride, op.pad
    xp = np.pad(x_nhwc, ((0, 0), (p, p), (p, p), (0, 0)))
    cols = []
    for kh in range(k):
        for kw in range(k):
            cols.append(xp[:, kh:kh + s * op.Ho:s, kw:kw + s * op.Wo:s, :])
    A = np.concatenate(cols, axis=-1).reshape(-1, K)
    return (A @ Wp.T).reshape(Bn, op.Ho, op.Wo, op.N)


def test_weight_packing_maps_cpu():
    """fused C3 dual conv, the space-to-depth stem and a 3x3 conv: packed-image GEMM == torch conv"""
    from yoloseries_amd import models
    from yoloseries_amd.engine import ConvOp, ParamPack
    torch.manual_seed(0)
    m = models.YOLOV5Small(3, 80)
    b, _ = _builder_for(m, 1, 64, 64)
    pk = ParamPack(m, b.ops, host_only=True)
    ops = {o.name: o for o in b.ops if isinstance(o, ConvOp)}
    rs = np.random.RandomState(0)
    # stem: 6x6/s2/p2 on (1,3,64,64) == 3x3/s1/p1 on the space-to-depth tensor
    x = rs.randn(1, 3, 64, 64).astype(np.float32)
    ref = F.conv2d(torch.from_numpy(x), m.focus.conv.weight, None, 2, 2).permute(0, 2, 3, 1).detach().numpy()
    s2d = np.zeros((1, 32, 32, 16), np.float32)
    s2d[..., :12] = x.reshape(1, 3, 32, 2, 32, 2).transpose(0, 2, 4, 3, 5, 1).reshape(1, 32, 32, 12)
    np.testing.assert_allclose(_emulate_conv(pk, ops["focus"], s2d), ref, rtol=1e-4, atol=1e-4)
    # fused cba1|cba2 of the first C3
    op = ops["backbone_stage1_bscp.cba12"]
    xin = rs.randn(1, 16, 16, 64).astype(np.float32)
    xt = torch.from_numpy(xin).permute(0, 3, 1, 2)
    c3 = m.backbone_stage1_bscp
    ref = torch.cat([F.conv2d(xt, c3.cba1.conv.weight), F.conv2d(xt, c3.cba2.conv.weight)], 1).permute(0, 2, 3, 1).detach().numpy()
    np.testing.assert_allclose(_emulate_conv(pk, op, xin), ref, rtol=1e-4, atol=1e-4)
    # stride-2 3x3
    op = ops["backbone_stage2_conv"]
    xin = rs.randn(1, 16, 16, 64).astype(np.float32)
    ref = F.conv2d(torch.from_numpy(xin).permute(0, 3, 1, 2), m.backbone_stage2_conv.conv.weight, None, 2, 1).permute(0, 2, 3, 1).detach().numpy()
    np.testing.assert_allclose(_emulate_conv(pk, op, xin), ref, rtol=1e-4, atol=1e-4)
    # gradient un-packing: every parameter element is produced exactly once
    un = pk.unpack_idx_np
    assert (un >= 0).all() and len(np.unique(un)) == len(un) and un.max() < pk.gsize


def test_yolox_block_diagonal_head_packing_cpu():
    from yoloseries_amd import models
    from yoloseries_amd.engine import ConvOp, ParamPack
    torch.manual_seed(0)
    m = models.YOLOXSmall(1, 3, 80, 0.01)
    b, outs = _builder_for(m, 1, 64, 64)
    pk = ParamPack(m, b.ops, host_only=True)
    op = outs[0]
    assert op.N == 85 and op.Ctot == 256 and op.part_seg == [0, 0, 1]
    rs = np.random.RandomState(1)
    freg, fcls = rs.randn(1, 8, 8, 128).astype(np.float32), rs.randn(1, 8, 8, 128).astype(np.float32)
    lay = m.detect.pred_small
    tr, tc = torch.from_numpy(freg).permute(0, 3, 1, 2), torch.from_numpy(fcls).permute(0, 3, 1, 2)
    ref = torch.cat([F.conv2d(tr, lay['reg'].weight), F.conv2d(tr, lay['cof'].weight), F.conv2d(tc, lay['cls'][1].weight)], 1)
    got = _emulate_conv(pk, op, np.concatenate([freg, fcls], -1))
    np.testing.assert_allclose(got, ref.permute(0, 2, 3, 1).detach().numpy(), rtol=1e-4, atol=1e-4)
    # bias gather follows the output-column order reg | cof | cls
    flat = np.concatenate([p.detach().numpy().reshape(-1) for p in pk.params])
    o = pk.bias_loc[op.name]
    bias = flat[pk.fpack_idx_np[o:o + 85]]
    np.testing.assert_array_equal(bias, np.concatenate([lay['reg'].bias.detach().numpy(), lay['cof'].bias.detach().numpy(), lay['cls'][1].bias.detach().numpy()]))
    assert len(m.state_dict()) == 414


def test_synth_generators_are_deterministic():
    from yoloseries_amd.utils.synth import synth_head_outputs, synth_targets
    a, b2 = synth_targets(4, 640, 80, 20, seed=1), synth_targets(4, 640, 80, 20, seed=1)
    np.testing.assert_array_equal(a, b2)
    assert a.shape[2] == 6 and (a[..., 4].max() < 80) and ((a[..., 5] == -1) | (a[..., 5] >= 0)).all()
    pad = a[..., 4] < 0
    assert (a[pad] == -1).all()
    h = synth_head_outputs(1, 64, 80, 3, seed=3)
    assert [x.shape for x in h] == [(1, 255, 8, 8), (1, 255, 4, 4), (1, 255, 2, 2)]


def test_product_refuses_cpu_tensors():
    """no CPU fallback: the product path fails loudly instead of computing on the host"""
    import pytest
    from yoloseries_amd import models
    from yoloseries_amd._lib import YoloHipError
    m = models.YOLOV5Small(3, 80)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 64, 64))
    from yoloseries_amd.loss import YOLOV5Loss
    from yoloseries_amd.utils.synth import COCO_ANCHORS
    lf = YOLOV5Loss(torch.from_numpy(COCO_ANCHORS), dict(device="cpu", input_img_size=[64, 64], num_class=80))
    with pytest.raises(YoloHipError):
        lf([torch.zeros(1, 255, 8, 8)], torch.zeros(1, 2, 6))


def test_product_never_imports_the_oracle():
    """the oracle is test infrastructure: nothing under yoloseries_amd/ (nor the drivers) may import or call it"""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    offenders = []
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(os.path.join(root, "yoloseries_amd")) for f in fs if f.endswith(".py")]
    files += [os.path.join(root, f) for f in ("train_yolov5.py", "val_yolov5.py")]
    for path in files:
        src = open(path).read()
        if re.search(r"^\s*(from|import)\s+oracle\b", src, re.M):
            offenders.append(path)
    assert not offenders, offenders


# names the reference's drivers import (train_yolov5.py:28-44, val_yolov5.py:20-33; SURVEY.md §8b "Runtime helpers the
# drivers import"): with `utils`, `trainer`, `loss`, `models`, `dataset`, `config` aliased to this package every one of them
# must resolve, so the driver scripts only change their import roots
DRIVER_IMPORTS = {
    "config": ["Config"],
    "loss": ["YOLOV5Loss", "YOLOXLoss"],
    "trainer": ["YOLOV5Evaluator", "YOLOXEvaluator", "ExponentialMovingAverageModel"],
    "dataset": ["build_dataloader", "build_test_dataloader", "build_val_dataloader"],
    "models": ["YOLOV5Small", "YOLOV5Middle", "YOLOV5Large", "YOLOV5XLarge", "YOLOXSmall"],
    "utils": ["cv2_save_img", "cv2_save_img_plot_pred_gt", "maybe_mkdir", "clear_dir", "time_synchronize", "summary_model", "mAP_v2", "configure_nccl",
              "configure_omp", "get_local_rank", "print_config", "get_rank", "get_world_size", "occupy_mem", "padding",
              "MeterBuffer", "all_reduce_norm", "is_parallel", "adjust_status", "synchronize", "configure_module", "launch",
              "get_num_devices", "gpu_nms", "gpu_linear_soft_nms", "gpu_exponential_soft_nms", "numba_nms", "gpu_iou",
              "gpu_CIoU", "gpu_DIoU", "gpu_Giou", "xyxy2xywh", "xyxy2xywhn", "xywh2xyxy", "numba_iou", "numba_xywh2xyxy",
              "numba_xyxy2xywh", "letter_resize_img", "letter_resize_bbox"],
}


def _alias_modules():
    import importlib
    import sys
    import yoloseries_amd.dataset, yoloseries_amd.loss, yoloseries_amd.models, yoloseries_amd.trainer, yoloseries_amd.utils  # noqa: F401,E401
    saved = {k: sys.modules.get(k) for k in DRIVER_IMPORTS}
    for k in ("utils", "trainer", "loss", "models", "dataset"):
        sys.modules[k] = importlib.import_module("yoloseries_amd." + k)
    sys.modules["config"] = importlib.import_module("config")
    return saved


def _restore_modules(saved):
    import sys
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def test_driver_import_surface_resolves():
    saved = _alias_modules()
    try:
        ns = {}
        for mod, names in DRIVER_IMPORTS.items():
            exec(f"from {mod} import {', '.join(names)}", ns)
        exec("from models import *", ns)
        assert callable(ns["launch"]) and callable(ns["YOLOV5Small"])
        # the names each of the reference's four drivers imports from these roots, as recorded from their own
        # `from <root> import ...` statements (tests/golden/driver_imports.json), resolved against the aliases
        import json
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "driver_imports.json")) as f:
            recorded = json.load(f)
        assert sorted(recorded) == ["train_yolov5.py", "train_yolox.py", "val_yolov5.py", "val_yolox.py"]
        for driver, roots in recorded.items():
            assert roots and set(roots) <= set(DRIVER_IMPORTS), (driver, sorted(roots))
            for mod, names in roots.items():
                exec(f"from {mod} import {', '.join(names)}", {})   # raises ImportError if a name the driver needs is missing
    finally:
        _restore_modules(saved)


def test_runtime_helpers_behaviour(tmp_path):
    """host helpers mirrored from utils/common.py, utils/meter.py, utils/model_utils.py, utils/logger.py, utils/setup_env.py"""
    import torch
    from yoloseries_amd import models, utils as U
    assert U.padding(640) == (640, 640) and U.padding(641) == (672, 672) and U.padding((100, 33), 32) == (128, 64)
    d = tmp_path / "a" / "b"
    U.maybe_mkdir(str(d)); U.maybe_mkdir(d)
    (d / "f.txt").write_text("x")
    U.clear_dir(str(d))
    assert d.exists() and not list(d.iterdir())
    assert not U.is_parallel(torch.nn.Linear(2, 2))
    assert isinstance(U.time_synchronize(), float)
    mb = U.MeterBuffer(window_size=3)
    for v in (1.0, 2.0, 3.0, 4.0):
        mb.update(tot_loss=torch.tensor(v), iter_time=v * 2)
    assert mb["tot_loss"].latest == 4.0 and abs(mb["tot_loss"].avg - 3.0) < 1e-9 and abs(mb["tot_loss"].global_avg - 2.5) < 1e-9
    assert list(mb.get_filtered_meter("time")) == ["iter_time"] and mb["iter_time"].median == 6.0
    mb.clear_meters(); assert mb["tot_loss"].latest is None and mb["tot_loss"].total == 10.0
    m = models.YOLOV5Small(3, 80).train()
    with U.adjust_status(m, training=False) as mm:
        assert not any(x.training for x in mm.modules())
    assert all(x.training for x in m.modules())
    sm = U.summary_model(m, [640, 640])
    assert sm["number_params"] == 7235389 and abs(sm["flops"] * 2 - 8.217) < 0.01      # MACs / 2e9 like the reference's thop line
    # drawing helpers of the val driver (val_yolov5.py:21-22): files are written, boxes change pixels, the blend keeps the size
    import numpy as np
    from PIL import Image
    pic = np.full((64, 96, 3), 90, dtype=np.uint8)
    U.cv2_save_img(pic, [[10, 20, 50, 60]], [3], [0.9], str(tmp_path / "v" / "p.png"))
    U.cv2_save_img_plot_pred_gt(pic, [[10, 20, 50, 60]], [3], [0.9], [[30, 25, 80, 50]], [1], str(tmp_path / "v" / "pg.png"))
    U.cv2_save_img_plot_pred_gt(pic, [], [], [], [], [], str(tmp_path / "v" / "none.png"))
    a, b, c0 = (np.asarray(Image.open(tmp_path / "v" / n)) for n in ("p.png", "pg.png", "none.png"))
    assert a.shape == b.shape == c0.shape == pic.shape and (a != pic).any() and (b != a).any() and (c0 == pic).all()
    assert tuple(a[40, 10]) == (0, 238, 238)                     # left edge of the predicted box
    table = U.print_config({"lr": 0.01, "_hidden": 1, "name": "x"})
    assert "lr" in table and "_hidden" not in table
    import os as _os
    env = dict(_os.environ)
    try:
        U.configure_nccl(); U.configure_omp(); U.configure_module()
        assert _os.environ["NCCL_IB_DISABLE"] == "1" and _os.environ["NCCL_SOCKET_IFNAME"] == "lo"
    finally:
        _os.environ.clear(); _os.environ.update(env)
    import numpy as _np
    U.cv2_save_img(_np.zeros((64, 64, 3), _np.uint8), [[4, 4, 40, 40]], [3], [0.9], str(tmp_path / "o" / "x.png"))
    assert (tmp_path / "o" / "x.png").stat().st_size > 0
    called = []
    U.launch(lambda a: called.append(a), 1, args=(5,))
    assert called == [5]


def _launch_main(tag):
    import torch.distributed as dist
    from yoloseries_amd.utils import get_local_rank, get_rank, get_world_size
    t = __import__("torch").tensor([float(get_rank() + 1)])
    dist.all_reduce(t)
    assert get_world_size() == 2 and t.item() == 3.0 and get_local_rank() == get_rank()
    open(f"{tag}.{get_rank()}", "w").write("ok")


def test_launch_two_ranks_gloo(tmp_path):
    """utils.launch (utils/launch.py:39-139): spawns one process per rank, initialises the process group and the local group"""
    from yoloseries_amd.utils import launch
    tag = str(tmp_path / "done")
    launch(_launch_main, 2, backend="gloo", dist_url="auto", args=(tag,))
    assert os.path.exists(tag + ".0") and os.path.exists(tag + ".1")


def test_shipped_tuning_table_matches_the_engine_key_versions():
    """yoloseries_amd/tune_defaults.json (tools/make_tune_defaults.sh) must be regenerated whenever the meaning of a tuned value
    changes: its keys carry the same version prefixes the engine asks for"""
    import json
    from yoloseries_amd import engine
    path = engine.TUNE_DEFAULTS_PATH
    assert os.path.dirname(path) == os.path.dirname(os.path.dirname(os.path.abspath(engine.__file__)))
    table = json.load(open(path))
    prefixes = {k.split(":", 1)[0] for k in table}
    assert prefixes <= engine.TUNE_KEY_VERSIONS and engine.KEY_CONV in prefixes, (prefixes, engine.TUNE_KEY_VERSIONS)
    assert len(table) > 300
    assert all(isinstance(v, list) and all(isinstance(x, int) for x in v) for v in table.values())


def test_planning_helpers_tolerate_empty_descriptors():
    """yh_conv_stat_blocks / yh_conv_bnr_rows are called while a descriptor is being filled in: a zero dimension answers 0"""
    import ctypes as C
    from yoloseries_amd._lib import ConvDesc, lib
    d = ConvDesc()
    assert lib().yh_conv_stat_blocks(C.byref(d)) == 0
    assert lib().yh_conv_bnr_rows(C.byref(d)) == 0


def test_conv_plan_table_is_stable():
    """what yh_conv_igemm decides — kernel instantiation, BatchNorm partial-sum rows, fused-reduction rows — for every shipped entry of
    the tuning table and 2 000 seeded random descriptors (invalid ones and their return codes included), through the C ABI alone,
    against the record tests/golden/conv_plan_digest.json: one sha256 per 100 lines of the table and the set of kernel
    instantiations (`tools/conv_plan_table.py --digest`; lines and names as before the planner was consolidated into conv_plan, the
    rows of declined sibling requests — six chunks — as they are since those answer like algo 0).  Planning is host code: no device needed.  A deliberate change of a plan — a new family, another tile —
    regenerates the record; `tools/conv_plan_table.py --reduced` prints the lines of a chunk that differs"""
    import json
    from yoloseries_amd._lib import lib
    mod = _conv_plan_table()
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_plan_digest.json")))
    got = mod.digest(mod.reduced(lib()), want["chunk"])
    assert want["lines"] >= 2500 and got["lines"] == want["lines"]
    assert got["names"] == want["names"], (sorted(set(got["names"]) - set(want["names"])), sorted(set(want["names"]) - set(got["names"])))
    bad = [i for i, (g, w) in enumerate(zip(got["sha256"], want["sha256"])) if g != w]
    assert not bad and len(got["sha256"]) == len(want["sha256"]), f"plans differ from the record in chunks {bad} (of {want['chunk']} lines each)"
    fams = {n.split("<")[0] for n in want["names"]}
    assert {"conv_stem_kernel", "conv_halo160_kernel", "conv_halo_kernel", "conv_v3_kernel", "conv_v2_kernel", "conv_igemm_kernel",
            "conv_dg2_kernel", "conv_p3_kernel", "conv_pt_kernel"} <= fams, fams


def _conv_plan_table():
    import importlib.util
    spec = importlib.util.spec_from_file_location("conv_plan_table", os.path.join(ROOT, "tools", "conv_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _conv_rows():
    import importlib.util
    spec = importlib.util.spec_from_file_location("conv_rows", os.path.join(ROOT, "tools", "conv_rows.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_conv_rows_name_every_instantiation_the_planner_emits():
    """tools/conv_rows.py, the table tests/test_gpu_conv_instantiations.py runs on the GPU: every row's descriptor is planned to the
    row's name (rc 0, slab rows where its epilogue writes a slab), its grid_cap column is what the plan does (at batch 64, where the
    uncapped grid has more than one block), and the rows' names are a superset of every name the planner emits — over the keys of
    the shipped table with every algo x tile_k x tile_n x grid_cap of conv_plan_table.table_lines, the reduced corpus (shipped
    choices, 2 000 seeded random descriptors) and the names of tests/golden/conv_plan_digest.json.  An instantiation added without
    a row fails here, on a machine without a GPU"""
    import json
    from yoloseries_amd._lib import lib
    R, L = _conv_rows(), lib()
    ids = [r.id for r in R.ROWS]
    assert len(set(ids)) == len(ids) >= 160
    for r in R.ROWS:
        rc, name, stat_rows, bnr_rows = R.plan(L, r.case())
        assert (rc, name) == (0, r.name), (r.id, rc, name)
        assert r.B >= 2 and r.N % 8 == 0
        assert (stat_rows > 0 if r.epi in ("stats", "gstats") else True) and (bnr_rows > 0 if r.epi == "bnr" else True), (r.id, stat_rows, bnr_rows)
        for cap in (1, 2):
            assert R.plan(L, r.case(grid_cap=cap))[:2] == (0, r.name), (r.id, cap)          # the cap never changes the instantiation
        big = [R.plan(L, r.case(B=64, grid_cap=cap))[2] for cap in (0, 1, 2)]
        assert (big[1] < big[0]) == r.cap, (r.id, big)
        if r.cap:          # one slab row per block along x: the cap itself (conv_pt_kernel: whole octets of pixel slots)
            assert big[1:] == ([8, 8] if r.name.startswith("conv_pt_kernel") else [1, 2]), (r.id, big)
    mod = R.T
    emitted = set(json.load(open(os.path.join(ROOT, "tests", "golden", "conv_plan_digest.json")))["names"])
    for lines in (mod.table_lines(L), mod.reduced(L)):
        emitted |= set(mod.digest(lines)["names"])
    assert len(emitted) >= 120
    assert not emitted - {r.name for r in R.ROWS}, sorted(emitted - {r.name for r in R.ROWS})


def test_conv_info_agrees_with_the_three_queries():
    """yh_conv_info against yh_conv_kernel_name / yh_conv_stat_blocks / yh_conv_bnr_rows over the reduced corpus of
    tools/conv_plan_table.py (the 530 shipped entries and 2 000 seeded random descriptors, invalid ones included): the same rc, the
    same name where a name is given, the same rows always; a descriptor without operand pointers is refused and planned alike"""
    import ctypes as C
    import random
    from yoloseries_amd import _lib
    mod, L = _conv_plan_table(), _lib.lib()
    cases = []
    for _, f, (tile_k, grid_cap, algo) in mod.table_keys():
        cases.append(dict(mod.case_of_key(f), tile_k=tile_k, grid_cap=grid_cap, algo=algo))
    r = random.Random(20261016)
    cases += [mod.random_case(r) for _ in range(2000)]
    assert len(cases) == 2530
    fams, refused = set(), 0
    for c in cases:
        d, o, buf = mod.make_desc(c), _lib.ConvInfo(), C.create_string_buffer(96)
        rc = L.yh_conv_info(C.byref(d), C.byref(o))
        assert rc == L.yh_conv_kernel_name(C.byref(d), buf, 96), c
        assert rc != 0 or (o.name == buf.value and o.name), c
        assert o.stat_rows == L.yh_conv_stat_blocks(C.byref(d)) and o.bnr_rows == L.yh_conv_bnr_rows(C.byref(d)), c
        refused += rc != 0
        if rc == 0:
            fams.add(o.family)
    assert fams == set(range(12)) and 300 < refused < 1000, (fams, refused)
    # valid but for its operands (the engine fills in a head gradient's address at run time): refused, and planned like the same
    # layer with them.  A ring-kernel layer with a tail and a conv_pt_kernel data gradient with the fused reduction
    for f, algo, want in (([0, 64, 80, 80, 80, 80, 1, 1, 0, 96, 1, 96, 96, 0, 0, 0, 96, 96, 0, 1, 0, 0, 0, 0, 0, 0], 3,
                           (_lib.YH_CONV_FAM_V3, 2, 1, b"conv_v3_kernel<128, 128, 2, 2, 64, 2, 1, true>")),
                          ([1, 64, 80, 80, 80, 80, 1, 1, 0, 64, 1, 128, 128, 0, 0, 0, 64, 64, 0, 0, 0, 0, 0, 0, 1, 0], 13,
                           (_lib.YH_CONV_FAM_PT, 0, 0, b"conv_pt_kernel<128, 0, 3>"))):
        c = dict(mod.case_of_key(f), algo=algo)
        d, o, bare, ob = mod.make_desc(c), _lib.ConvInfo(), mod.make_desc(c), _lib.ConvInfo()
        bare.seg[0].ptr = bare.w = bare.out0 = None
        assert L.yh_conv_info(C.byref(d), C.byref(o)) == 0 and L.yh_conv_info(C.byref(bare), C.byref(ob)) != 0
        assert (o.family, o.variant, o.tail, o.name) == want and o.stat_rows > 0
        assert all(getattr(o, n) == getattr(ob, n) for n, _ in _lib.ConvInfo._fields_)


def test_declined_sibling_request_answers_as_algo_0():
    """A descriptor whose algo names a sibling family (7 .. 13) that does not take it — 11, unassigned, never does — runs the plan of
    the same descriptor with algo 0, so every query answers as that one: all fields of yh_conv_info and its rc, yh_conv_stat_blocks
    and yh_conv_bnr_rows.  Over the reduced corpus of tools/conv_plan_table.py (530 shipped entries, 2 000 seeded random descriptors)
    x the seven algos; the counts are a property of tune_defaults.json and the seed"""
    import ctypes as C
    import random
    from yoloseries_amd import _lib
    mod, L = _conv_plan_table(), _lib.lib()
    cases = [mod.case_of_key(f) for _, f, _ in mod.table_keys()]
    r = random.Random(20261016)
    cases += [mod.random_case(r) for _ in range(2000)]

    def ask(c, algo):
        d, o = mod.make_desc(dict(c, algo=algo)), _lib.ConvInfo()
        rc = L.yh_conv_info(C.byref(d), C.byref(o))
        return (rc,) + tuple(getattr(o, n) for n, _ in _lib.ConvInfo._fields_), (L.yh_conv_stat_blocks(C.byref(d)), L.yh_conv_bnr_rows(C.byref(d)))

    fields = [n for n, _ in _lib.ConvInfo._fields_]
    i_fam, i_stat, i_bnr = (1 + fields.index(n) for n in ("family", "stat_rows", "bnr_rows"))
    declined, honoured, bad = 0, 0, []
    for c in cases:
        info0, rows0 = ask(c, 0)
        for algo in (7, 8, 9, 10, 11, 12, 13):
            info, rows = ask(c, algo)
            assert rows == (info[i_stat], info[i_bnr]), (c, algo)
            if algo != 11 and info[i_fam] == _lib.CONV_ALGO_FAMILY[algo][0]:
                honoured += 1
                continue
            declined += 1
            if (info, rows) != (info0, rows0):
                bad.append((algo, c, info, info0))
    assert (declined, honoured) == (17371, 339), (declined, honoured)
    assert not bad, (len(bad), bad[:3])


CONV_PREFIX_GROUPS = {("conv6", "conv11", "dgrad"): 50, ("conv6", "conv11", "fwd"): 24, ("conv9", "conv11", "eval"): 6, ("conv9", "conv10", "eval"): 2}


def test_conv_tune_keys_round_trip():
    """TunerMixin._conv_tune_key rebuilds the conv keys of the shipped table from the descriptors they describe: 448 of the 530
    exactly; the other 82 carry a version prefix the engine no longer asks for (entries from before conv_pt_kernel / conv_c80_kernel
    joined their layers' candidates) beside a live twin under the new one.  The numbers are a property of tune_defaults.json"""
    from yoloseries_amd.engine.tune import TunerMixin
    mod = _conv_plan_table()
    keys = {k: f for k, f, _ in mod.table_keys()}
    assert len(keys) == 530
    same, groups = 0, {}
    for key, f in keys.items():
        kind = key.split(":")[1]
        got = TunerMixin._conv_tune_key(mod.make_desc(mod.case_of_key(f)), kind, False)
        if got == key:
            same += 1
            continue
        assert got.split(":")[1:] == key.split(":")[1:] and got in keys, (key, got)
        g = (key.split(":")[0], got.split(":")[0], kind)
        groups[g] = groups.get(g, 0) + 1
    assert same == 448 and groups == CONV_PREFIX_GROUPS, (same, groups)


def _conv_enum_desc(mod, f, kind, stats=False):
    """the descriptor of a table key as the engine holds it when it enumerates candidates: the statistics pointer of a training
    forward is attached only afterwards, for the timing"""
    c = mod.case_of_key(f)
    if kind == "fwd":
        c["stats"] = int(stats)
    return mod.make_desc(c)


def test_conv_tuner_candidates():
    """the (algo, tile_k, grid_cap) candidates the engine times per conv launch (TunerMixin._conv_candidates: the library's plan says
    which requests it would honour) for every conv key of the shipped table, against tests/golden/conv_tune_candidates.json.  The record
    was taken on the commit before this function existed, by running the enumeration loop _tune_conv had then — it asked
    yh_conv_kernel_name per algo and matched substrings of the profiler spelling — over the same descriptors on the CPU; one line
    per key, "<key> -> algo,tile_k,grid_cap;...", in the order of conv_plan_table.table_keys().  Every shipped choice is one of
    its key's candidates; the list does not depend on the input address being known; a training forward gives the same list with
    the statistics pointer attached, and its shipped choice the same statistics rows"""
    import ctypes as C
    import hashlib
    import json
    from yoloseries_amd._lib import lib
    from yoloseries_amd.engine.tune import TunerMixin
    mod, L = _conv_plan_table(), lib()
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_tune_candidates.json")))
    assert hashlib.sha256("\n".join(want).encode()).hexdigest() == "267a49d88aca1d279f2eaa3c7e6aa9f06a7f370cf1afc2ab057c5168c8725891"
    got, total, nfwd = [], 0, 0
    for key, f, (tile_k, grid_cap, algo) in mod.table_keys():
        kind = key.split(":")[1]
        d = _conv_enum_desc(mod, f, kind)
        d.algo, d.tile_k, d.grid_cap = 3, 32, 24
        cands = TunerMixin._conv_candidates(L, d, kind)
        assert (d.algo, d.tile_k, d.grid_cap) == (3, 32, 24)          # the enumeration leaves the descriptor as it was
        assert (algo, tile_k, grid_cap) in cands, (key, cands)
        bare = _conv_enum_desc(mod, f, kind)
        bare.seg[0].ptr = None          # (a head layer's data gradient: its input address arrives at run time)
        assert TunerMixin._conv_candidates(L, bare, kind) == cands, key
        if kind == "fwd":
            ds = _conv_enum_desc(mod, f, kind, stats=True)
            assert TunerMixin._conv_candidates(L, ds, kind) == cands, key
            assert TunerMixin._conv_info(L, ds, algo, tile_k, grid_cap).stat_rows == TunerMixin._conv_info(L, d, algo, tile_k, grid_cap).stat_rows
            nfwd += 1
        total += len(cands)
        got.append(f"{key} -> " + ";".join(f"{a},{tk},{cap}" for a, tk, cap in cands))
    assert (len(got), total, nfwd) == (530, 3960, 118)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:3]


#   kind, key fields (conv_plan_table.case_of_key) | candidates
CONV_CANDIDATE_ROWS = [
    ("fwd", (0, 64, 320, 320, 320, 320, 3, 1, 1, 32, 1, 16, 16, 0, 0, 0, 32, 32, 0, 1, 0, 0, 0, 0, 0, 0), "1,0,0"),                                      # stem: nothing else
    ("fwd", (0, 64, 80, 80, 80, 80, 1, 1, 0, 64, 1, 64, 64, 0, 0, 0, 64, 64, 0, 1, 0, 0, 0, 0, 0, 0), "1,0,0;1,0,1536;2,0,0;3,0,0;4,0,0"),               # v3, whole 64-channel blocks
    ("fwd", (0, 64, 80, 80, 80, 80, 1, 1, 0, 96, 1, 96, 96, 0, 0, 0, 96, 96, 0, 1, 0, 0, 0, 0, 0, 0), "1,0,0;1,0,1024;2,0,0;2,32,0;3,0,0;3,32,0;4,0,0;4,32,0"),   # v3 with a tail
    ("fwd", (0, 64, 20, 20, 20, 20, 3, 1, 1, 128, 1, 512, 512, 0, 0, 0, 128, 128, 0, 1, 0, 0, 0, 0, 0, 0), "1,0,0;1,32,0;2,0,0;3,0,0;4,0,0;5,0,0"),      # halo, both k-steps of v2
    ("eval", (0, 32, 40, 40, 40, 40, 3, 1, 1, 640, 1, 640, 640, 0, 0, 0, 640, 640, 0, 0, 0, 1, 0, 1, 0, 0), "1,0,0;1,0,192;1,32,0;1,32,192;2,0,0;3,0,0;4,0,0;5,0,0;6,0,0"),   # halo160
    ("dgrad", (1, 64, 320, 320, 160, 160, 3, 2, 1, 32, 1, 64, 64, 0, 0, 0, 32, 32, 0, 0, 0, 0, 0, 0, 1, 0), "1,0,0;1,0,2048;7,0,0"),                     # dg2
    ("fwd", (0, 64, 160, 160, 160, 160, 3, 1, 1, 32, 1, 32, 32, 0, 0, 0, 32, 32, 0, 1, 0, 0, 0, 0, 0, 0), "1,0,0;1,0,2048;8,0,0"),                       # p3
    ("eval", (0, 32, 320, 320, 320, 320, 3, 1, 1, 80, 1, 80, 80, 0, 0, 0, 80, 80, 0, 0, 1, 1, 0, 1, 0, 0), "1,0,0;1,0,1024;2,0,0;3,0,0;4,0,0;5,0,0;9,0,0"),      # h80
    ("eval", (0, 32, 320, 320, 320, 320, 1, 1, 0, 80, 1, 80, 80, 0, 0, 0, 80, 80, 0, 0, 0, 1, 0, 1, 0, 0), "1,0,0;1,0,1024;2,0,0;3,0,0;4,0,0;10,0,0"),   # pw
    ("eval", (0, 32, 320, 320, 640, 640, 3, 2, 1, 160, 1, 80, 80, 0, 0, 0, 160, 160, 0, 0, 0, 1, 0, 1, 0, 0), "1,0,0;1,0,512;2,0,0;3,0,0;4,0,0;12,0,0"), # c80
    ("dgrad", (1, 64, 80, 80, 80, 80, 1, 1, 0, 64, 1, 128, 128, 0, 0, 0, 64, 64, 0, 0, 0, 0, 0, 0, 1, 0), "1,0,0;1,0,1536;2,0,0;3,0,0;4,0,0;13,0,0"),    # pt
    ("fwd", (0, 64, 20, 20, 40, 40, 3, 2, 1, 256, 1, 256, 256, 0, 0, 0, 256, 256, 0, 1, 0, 0, 0, 0, 0, 0), "1,0,0;1,32,0;2,0,0;3,0,0;4,0,0;14,0,0"),     # the 256 x 256 tile
]


def test_conv_tuner_candidates_per_family(monkeypatch):
    """one layer per kernel family: the candidate lists the tuner produced when it matched kernel names, and what the two switches
    take out of them — YH_CONV_V3=0 everything but the register-staged kernel, flags.SKIP_ALGOS exactly the algos it names"""
    from yoloseries_amd._lib import lib
    from yoloseries_amd.engine import flags
    from yoloseries_amd.engine.tune import TunerMixin
    mod, L = _conv_plan_table(), lib()
    monkeypatch.delenv("YH_CONV_V3", raising=False)
    monkeypatch.setattr(flags, "SKIP_ALGOS", frozenset())
    lists = []
    for kind, f, want in CONV_CANDIDATE_ROWS:
        cands = TunerMixin._conv_candidates(L, _conv_enum_desc(mod, f, kind), kind)
        assert ";".join(f"{a},{tk},{cap}" for a, tk, cap in cands) == want, (kind, f)
        lists.append(cands)
    assert {a for cands in lists for a, _, _ in cands} == {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14}
    monkeypatch.setattr(flags, "SKIP_ALGOS", frozenset(("3", "13", "14")))
    for (kind, f, _), cands in zip(CONV_CANDIDATE_ROWS, lists):
        assert TunerMixin._conv_candidates(L, _conv_enum_desc(mod, f, kind), kind) == [c for c in cands if c[0] not in (3, 13, 14)]
    monkeypatch.setattr(flags, "SKIP_ALGOS", frozenset())
    monkeypatch.setenv("YH_CONV_V3", "0")
    for (kind, f, _), cands in zip(CONV_CANDIDATE_ROWS, lists):
        assert TunerMixin._conv_candidates(L, _conv_enum_desc(mod, f, kind), kind) == [c for c in cands if c[0] == 1]


def _wgrad_plan_table():
    import importlib.util
    import sys
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)          # (the module imports conv_plan_table.digest)
    spec = importlib.util.spec_from_file_location("wgrad_plan_table", os.path.join(tools, "wgrad_plan_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_wgrad_plan_table_is_stable():
    """what yh_conv_wgrad decides — form, kernel instantiation, tiles, effective splits, honoured tile_k, workspace bytes — for every
    shipped weight-gradient entry of the tuning table and 2 000 seeded random descriptors, through yh_conv_wgrad_info alone, against
    the record tests/golden/wgrad_plan_digest.json (`tools/wgrad_plan_table.py --digest`, taken from the library as it was before the
    decisions were consolidated into wg_plan, its columns composed from the queries of that time).  No device needed.  A deliberate
    change of a plan regenerates the record; `tools/wgrad_plan_table.py --reduced` prints the lines of a chunk that differs"""
    import json
    from yoloseries_amd._lib import lib
    mod = _wgrad_plan_table()
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "wgrad_plan_digest.json")))
    got = mod.digest(mod.reduced(lib()), want["chunk"])
    assert want["lines"] >= 2100 and got["lines"] == want["lines"]
    assert got["names"] == want["names"], (sorted(set(got["names"]) - set(want["names"])), sorted(set(want["names"]) - set(got["names"])))
    bad = [i for i, (g, w) in enumerate(zip(got["sha256"], want["sha256"])) if g != w]
    assert not bad and len(got["sha256"]) == len(want["sha256"]), f"plans differ from the record in chunks {bad} (of {want['chunk']} lines each)"
    assert {"conv_wgrad_kernel", "conv_wgp_kernel", "conv_wgpf_kernel", "conv_wgs_kernel"} <= {n.split("<")[0] for n in want["names"]}


# the conv_wgrad_kernel instantiations of the library: <WN, WC, TNW, TCW, TK, MINW, PF2> and whether the row also exists fused
WGRAD_ROWS = [("1, 5, 1, 1, 32, 3, true", True), ("1, 5, 1, 1, 64, 3, true", True), ("1, 4, 1, 2, 32, 3, true", True), ("1, 4, 1, 2, 64, 2, true", True),
              ("1, 4, 1, 3, 32, 3, false", False), ("1, 4, 1, 3, 64, 2, false", False), ("1, 4, 2, 1, 32, 4, false", False),
              ("1, 4, 2, 1, 64, 2, false", False), ("1, 4, 2, 2, 32, 3, false", True), ("1, 4, 2, 2, 64, 2, false", True),
              ("1, 4, 2, 3, 32, 2, false", False), ("2, 2, 1, 2, 64, 3, true", False), ("4, 2, 1, 2, 64, 4, true", False),
              ("4, 2, 1, 2, 32, 2, true", False), ("2, 2, 2, 2, 32, 2, false", False)]


def test_wgrad_plan_names_are_the_compiled_kernels(tmp_path):
    """every kernel name yh_conv_wgrad_info reports for a descriptor it accepts (the reduced corpus of tools/wgrad_plan_table.py) is a
    kernel symbol of the built library, every conv_wgrad_kernel instantiation in the code object of conv_wgrad.hip is reported for
    some descriptor (no dead instantiation), and that code object holds exactly the known instantiations and wgrad_reduce_kernel.
    Symbols are listed (llvm-objdump -t), nothing is disassembled."""
    import subprocess
    from test_isa_packed_forms import OBJDUMP, _code_objects
    from yoloseries_amd import _lib
    if not os.path.exists(OBJDUMP):
        import pytest
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    mod = _wgrad_plan_table()
    L = _lib.lib()
    reported = set()
    for _, c in mod.reduced_cases():
        rc, _, name = mod.info(L, mod.make_desc(L, c))[:3]
        if rc == 0:
            reported.add(name)
    kernels, own = set(), None
    for i, blob in enumerate(_code_objects(_lib.LIB_PATH)):
        f = tmp_path / f"co_{i}.elf"
        f.write_bytes(blob)
        syms = subprocess.run([OBJDUMP, "-t", "-C", str(f)], stdout=subprocess.PIPE, text=True, check=True).stdout
        names = {m.group(1) for m in re.finditer(r" F \.text\s+\S+\s+(?:\.protected )?(?:void )?(?:\(anonymous namespace\)::)?(\w+(?:<[^>]*>)?)\(", syms)}
        kernels |= names
        if "wgrad_reduce_kernel" in names:
            own = names
    assert own is not None, "no code object with wgrad_reduce_kernel"
    assert reported and reported <= kernels, sorted(reported - kernels)
    want = {f"conv_wgrad_kernel<{a}, false>" for a, _ in WGRAD_ROWS} | {f"conv_wgrad_kernel<{a}, true>" for a, fused in WGRAD_ROWS if fused}
    assert own == want | {"wgrad_reduce_kernel"}, (sorted(own - want), sorted(want - own))
    assert want <= reported, sorted(want - reported)


def test_wgrad_tuner_candidates():
    """the (tile_k, splits) candidates the engine times for a weight gradient (Program._wgrad_candidates: the library's plan says
    which requests it would honour) for one layer per tiling, patch- and wave-eligible layers and the fused stem, without / with a
    workspace: the lists the tuner produced when it matched kernel names instead"""
    from yoloseries_amd._lib import lib
    from yoloseries_amd.engine.tune import TunerMixin
    mod = _wgrad_plan_table()
    L = lib()
    #        N, ldg, C, ld, ups, Ctot, B, Ho, Wo, Hi, Wi, k, stride, pad | bn_z | tile_k candidates without, with a workspace
    layers = [((32, 32, 32, 64, 0, 32, 64, 160, 160, 160, 160, 1, 1, 0), 0, (0, 64, 40), (0, 64)),               # <1, 5, 1, 1>, patch-eligible
              ((32, 32, 192, 192, 0, 192, 64, 80, 80, 80, 80, 1, 1, 0), 0, (0, 64), (0, 64)),                    # <1, 4, 1, 2>
              ((32, 32, 32, 32, 0, 32, 64, 160, 160, 160, 160, 3, 1, 1), 0, (0, 64, 40), (0, 64)),               # <1, 4, 1, 3>
              ((128, 128, 128, 128, 0, 128, 64, 160, 160, 160, 160, 1, 1, 0), 0, (0, 64, 128, 129), (0, 64, 128, 129)),     # <1, 4, 2, 1>, wave-eligible
              ((128, 128, 256, 256, 0, 256, 64, 40, 40, 40, 40, 1, 1, 0), 0, (0, 64, 128, 129), (0, 64, 128, 129)),         # <1, 4, 2, 2>
              ((192, 192, 384, 384, 0, 384, 64, 40, 40, 40, 40, 1, 1, 0), 0, (0, 128, 129), (0, 128, 129)),      # <1, 4, 2, 3>
              ((64, 64, 64, 64, 0, 64, 64, 160, 160, 160, 160, 3, 1, 1), 0, (0, 40, 129), (0, 129)),             # <2, 2, 1, 2>
              ((1024, 1024, 1024, 1024, 0, 1024, 64, 20, 20, 20, 20, 1, 1, 0), 0, (0, 32, 35, 129), (0, 32, 35, 129)),      # <4, 2, 1, 2>
              ((96, 96, 48, 48, 0, 48, 64, 160, 160, 320, 320, 3, 2, 1), 0, (0, 32, 35), (0, 32, 35)),           # ... 48 channels: no wave form
              ((32, 32, 16, 16, 0, 16, 64, 320, 320, 320, 320, 3, 1, 1), 1, (0, 64, 40), (0, 64)),               # fused stem, N <= 32
              ((48, 48, 16, 16, 0, 16, 64, 320, 320, 320, 320, 3, 1, 1), 1, (0, 64, 40), (0, 64))]               # fused stem, N > 32
    got = {}
    for f, bn, without, with_ws in layers:
        for ws, want in ((0, without), (1, with_ws)):
            c = mod.case_of_key("wgrad11f" if bn else "wgrad11", f)
            c["ws"] = ws
            wd = mod.make_desc(L, c)
            M, ntile = wd.B * wd.Ho * wd.Wo, L.yh_conv_wgrad_tiles(wd.N, wd.KH * wd.KW * wd.seg.C)
            wd.tile_k, wd.splits = 7, 11
            cands = TunerMixin._wgrad_candidates(L, wd, M, ntile)
            assert (wd.tile_k, wd.splits) == (7, 11)          # the enumeration leaves the descriptor as it was
            assert tuple(tk for tk, _ in cands) == want, (f, ws, cands)
            got[f[0], f[11], ws] = dict(cands)
    assert got[1024, 1, 0] == {0: [4, 8, 12, 16, 24], 32: [4, 8, 12, 16, 24], 35: [4, 8, 12, 16, 24], 129: [64, 96, 192]}
    assert got[192, 1, 1] == {0: [86, 171, 256, 342, 400], 128: [43, 86, 128, 171, 256], 129: [96, 192]}
    assert got[64, 3, 0] == {0: [52, 103, 154, 205, 308], 40: [1024], 129: [125, 128, 255, 256]}


def test_wgrad_refusals_agree_between_plan_query_and_launcher():
    """every argument check of yh_conv_wgrad, one descriptor each with exactly that field broken: yh_conv_wgrad_info and
    yh_conv_wgrad return the same non-zero rc and name the same check.  The operands are fake addresses — the launcher is called
    only after the query has refused the descriptor (both read one plan: it refuses before anything is launched)"""
    import ctypes as C
    from yoloseries_amd import _lib
    mod = _wgrad_plan_table()
    L = _lib.lib()
    base = dict(N=32, ldg=32, C=16, ld=16, ups=0, coff_k=0, Ctot=16, B=2, Ho=12, Wo=20, Hi=12, Wi=20, KH=3, stride=1, pad=1, splits=3,
                tile_k=0, bn=0, ws=0)

    def desc(**kw):
        ptrs = {k: kw.pop(k) for k in list(kw) if k in ("gy", "ptr", "dw", "partial", "partial_bytes", "bn_ldz", "bn_ws")}
        d = mod.make_desc(L, dict(base, **kw))
        for k, v in ptrs.items():
            setattr(d.seg if k == "ptr" else d, k, v)
        return d
    o = _lib.WgradInfo()
    ok = desc()
    assert L.yh_conv_wgrad_info(C.byref(ok), C.byref(o)) == 0 and o.name == b"conv_wgrad_kernel<1, 5, 1, 1, 32, 3, true, false>"
    assert L.yh_conv_wgrad_info(C.byref(desc(tile_k=40)), C.byref(o)) == 0 and o.form == _lib.YH_WGRAD_PATCH
    one_pixel = dict(KH=1, pad=0, C=8, ld=8, Ctot=8, N=8)
    broken = [
        ("null desc / bad dims", None),
        ("null desc / bad dims", desc(B=0)),
        ("null desc / bad dims", desc(Wi=0)),
        ("workspace too small / unaligned", desc(ws=3)),                      # 4 bytes short
        ("workspace too small / unaligned", desc(ws=1, partial=8 * mod.P + 4)),
        ("workspace too small / unaligned", desc(ws=3, tile_k=129, N=64, C=32, ld=32, Ctot=32, ldg=64, Ho=16, Hi=16)),     # the wave form's slots
        ("bad operands", desc(tile_k=40, gy=mod.P + 2)),                      # patch form
        ("bad operands", desc(tile_k=40, dw=None)),
        ("a single image needs a 2 GiB operand", desc(**one_pixel, B=1, Ho=4096, Wo=4096, Hi=4096, Wi=4096, ldg=64)),
        ("gy null/unaligned", desc(gy=None)),
        ("gy null/unaligned", desc(ldg=36)),
        ("needs ldg padded to 8", desc(N=28, ldg=24)),
        ("segment misaligned", desc(C=12, Ctot=12)),
        ("segment misaligned", desc(ptr=None)),
        ("bad channel offset", desc(coff_k=8)),
        ("bad stride", desc(stride=3)),
        ("bad kernel size", desc(KH=9, pad=4)),
        ("geometry mismatch", desc(Hi=13)),
        ("dw null / bad splits", desc(dw=None)),
        ("dw null / bad splits", desc(splits=0)),
        ("upsampled segment needs even dims", desc(ups=1, Ho=13, Hi=13)),
        ("too many pixels", desc(**dict(one_pixel, ld=0), ldg=0, B=1 << 15, Ho=256, Wo=256, Hi=256, Wi=256)),
        ("operands of 2 GiB or more", desc(N=1 << 30, ldg=0)),
        ("too many splits", desc(B=64, Ho=184, Wo=184, Hi=184, Wi=184, splits=70000)),       # 67 712 splits of 32 pixels hold pixels
        ("fused BatchNorm backward (bn_z) needs a wide tiling", desc(bn=1, C=32, ld=32, Ctot=32)),          # <1, 4, 1, 3>: not fused
        ("fused BatchNorm backward (bn_z) needs a wide tiling", desc(bn=1, N=64, ldg=64, C=8, ld=8, Ctot=8)),      # <1, 4, 2, 1>
        ("bad fused-BatchNorm operands", desc(bn=1, bn_ldz=24)),
        ("bad fused-BatchNorm operands", desc(bn=1, bn_ws=None)),
        ("bn_z of 2 GiB or more", desc(bn=1, bn_ldz=1 << 22)),
    ]
    for what, d in broken:
        ref = C.byref(d) if d is not None else None
        rc = L.yh_conv_wgrad_info(ref, C.byref(o))
        msg = L.yh_last_error().decode()
        assert rc != 0 and what in msg, (what, rc, msg)
        assert L.yh_conv_wgrad(ref, None) == rc and L.yh_last_error().decode() == msg, (what, L.yh_last_error())


def test_executor_knows_every_program_entry_point():
    """yh_exec (csrc/exec.hip) replays the engine's command lists: every entry point a Program emits must be in its table, with
    the argument count the ctypes signature declares (stream included)"""
    import ctypes as C
    from yoloseries_amd import _lib
    L = _lib.lib()
    for name in ("yh_conv_igemm", "yh_conv_wgrad", "yh_bn_finalize", "yh_bn_fold_batch", "yh_bn_silu_apply", "yh_bn_silu_bwd_reduce",
                 "yh_bn_bwd_finalize", "yh_bn_silu_bwd_apply", "yh_colsum", "yh_maxpool5_fwd", "yh_maxpool5_bwd", "yh_upsample2_bwd",
                 "yh_fill_u32"):
        n = C.c_int32(0)
        assert L.yh_exec_op(name.encode(), C.byref(n)) >= 0, name
        assert n.value == len(_lib._SIGS[name][1]) <= _lib.YH_CMD_SLOTS, (name, n.value)
    assert L.yh_exec_op(b"yh_nms_batched", None) == -1
    assert C.sizeof(_lib.Cmd) == 16 + 8 * _lib.YH_CMD_SLOTS


def test_fuse_conv_bn_matches_reference_fixture():
    """fuse_conv_bn (utils/layer_tools.py:26-53): weight and bias of the fused conv against the reference's (g6 `fuse_w`, `fuse_b`)
    — host-side parameter algebra, CPU"""
    import torch
    from test_gpu_model import fill_state
    from yoloseries_amd.utils.layer_tools import ConvBnAct, fuse_conv_bn
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "g6_blocks.npz"))
    cb = ConvBnAct(16, 32, 3, 1, 1)
    fill_state(cb, int(g["fuse_args"][0]))
    with torch.no_grad():
        fused = fuse_conv_bn(cb.conv, cb.bn)
    assert not fused.weight.requires_grad and not fused.bias.requires_grad
    np.testing.assert_allclose(fused.weight.numpy(), g["fuse_w"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(fused.bias.numpy(), g["fuse_b"], rtol=1e-6, atol=1e-7)


def _asm_pending_reads(text):
    """compiler-generated instructions that read a register an inline-asm load (ds_read / buffer_load into registers) has written,
    in front of the next inline-asm s_waitcnt of the load's counter: [(kernel, line, instruction)]"""
    def regs(tok):
        out = set()
        for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", tok):
            out |= set(range(int(m.group(1)), int(m.group(2)) + 1)) if m.group(1) else {int(m.group(3))}
        return out
    hits, in_asm, pend, kern = [], False, {}, ""
    for i, ln in enumerate(text.split("\n")):
        t = ln.strip()
        if re.match(r"^_Z\w+:", ln):
            kern, pend = ln.split(":")[0], {}
        if t.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if t.startswith(";;#ASMEND"):
            in_asm = False
            continue
        if not ln.startswith("\t") or t.startswith((".", ";")):
            continue
        if in_asm:
            m = re.match(r"(ds_read\w*|buffer_load_dword\w*)\s+(\S+),", t)
            if m and not t.endswith(" lds"):
                for r in regs(m[2]):
                    pend[r] = "lgkm" if m[1].startswith("ds_") else "vm"
            if t.startswith("s_waitcnt"):
                pend = {r: c for r, c in pend.items() if not ((c == "lgkm" and "lgkmcnt" in t) or (c == "vm" and "vmcnt" in t))}
        elif pend:
            parts = t.split(None, 1)
            if len(parts) == 2 and parts[0].startswith(("v_", "ds_", "buffer_", "global_")):
                ops = parts[1].split(",")
                srcs = parts[1] if parts[0].startswith(("buffer_store", "global_store", "ds_write", "v_cmp")) else ",".join(ops[1:])
                if regs(srcs) & set(pend):
                    hits.append((kern, i, t))
    return hits


def test_inline_asm_loads_are_not_read_before_their_wait(tmp_path):
    """conv_halo160_kernel requests its fragments by inline-asm ds_read and waits for them by an inline-asm s_waitcnt tied to the
    destination registers.  The compiler believes those registers defined at the ds_read: should it ever copy or use one in front
    of the wait (it did exactly that to conv_pt_kernel's operand loads in round 5), the copy holds stale bytes.  The generated
    code of every kernel of the generic conv (one file per kernel family beside the planner, conv_igemm.hip) is scanned: no
    compiler-generated instruction reads such a register before the wait."""
    import subprocess
    text = ""
    for family in ("conv_generic", "conv_v2", "conv_v3", "conv_halo", "conv_halo160", "conv_stem"):
        src = os.path.join(ROOT, "yoloseries_amd", "csrc", family + ".hip")
        out = tmp_path / (family + ".s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "--cuda-device-only", "-S",
                        "-o", str(out), src], check=True, capture_output=True)
        text += out.read_text()
    assert "conv_halo160_kernel" in text and len(re.findall(r";;#ASMSTART\n\s*ds_read_b128", text)) >= 10
    hits = _asm_pending_reads(text)
    assert not hits, hits[:5]


def test_conv_pt_kernel_has_no_register_spills(tmp_path):
    """conv_pt_kernel counts its vector-memory instructions by hand (s_waitcnt vmcnt(N) with compile-time N): a register spill would add
    scratch loads / stores the counts do not know about.  Every instantiation the library launches must compile without scratch."""
    import subprocess
    src = os.path.join(ROOT, "yoloseries_amd", "csrc", "conv_pt.hip")
    out = tmp_path / "pt.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "--cuda-device-only", "-S",
                    "-o", str(out), src], check=True, capture_output=True)
    text = out.read_text()
    kernels = re.findall(r"^(_ZN\S*conv_pt_kernel\S*):.*?; ScratchSize: (\d+)", text, flags=re.S | re.M)
    assert len(kernels) >= 20, len(kernels)
    bad = [(k, n) for k, n in kernels if int(n) != 0]
    assert not bad, bad
    # nothing in flight may be held in a register the compiler knows as a C value: every inline-asm load of this file is an LDS-DMA
    # transfer (round 5: operands loaded into registers by asm and "tied" to their wait were copied by the compiler in front of it)
    asm_loads = re.findall(r";;#ASMSTART\n((?:(?!;;#ASMEND).)*?buffer_load_dword\S*[^\n]*)", text, flags=re.S)
    assert asm_loads and all(ln.strip().endswith(" lds") for blk in asm_loads for ln in blk.split("\n") if "buffer_load" in ln), \
        [ln for blk in asm_loads for ln in blk.split("\n") if "buffer_load" in ln and not ln.strip().endswith(" lds")][:3]
