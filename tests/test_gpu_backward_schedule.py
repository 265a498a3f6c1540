"""The backward schedule on the GPU: the two runners of a compiled pass (yh_exec replay / one call per launch) against each other on
one deterministic program, and the compiled arrays against the recorded schedule (tools/bwd_schedule.py)."""
import importlib.util
import itertools
import json
import os
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bwd_schedule_v5s_2x128.json")


def _tool():
    spec = importlib.util.spec_from_file_location("bwd_schedule", os.path.join(ROOT, "tools", "bwd_schedule.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_compiled_schedules_match_the_record(dev, monkeypatch):
    """every compiled backward array of YOLOv5s (all eight combinations), of YOLOXSmall and of YOLOv5s in deterministic mode, rendered by
    tools/bwd_schedule.py, against tests/golden/bwd_schedule_v5s_2x128.json — recorded from the two-interpreter code (`produced_by`
    in the file).  On a mismatch the current rendering is printed."""
    monkeypatch.setenv("YH_CONV_TUNE", "0")
    monkeypatch.setenv("YH_WGRAD_TUNE", "0")
    from yoloseries_amd import engine
    assert engine.flags.WG_WS_BYTES == 0, "the record was taken in the default mode: this test runs ahead of the module's deterministic-mode fixture"
    T = _tool()
    with open(GOLDEN) as f:
        want = json.load(f)
    assert want.pop("produced_by") and want.pop("shape") == list(T.SHAPE)
    scheds = T.schedules(dev)
    got = T.document(scheds)
    got.pop("shape")

    def flat(doc):
        return {(name, k): v for name, by_combo in doc.items() for k, v in by_combo.items()}
    want, got = flat(want), flat(got)
    assert len(got) == 8 + 1 + 1 and sorted(got) == sorted(want)
    bad = [nk for nk in got if got[nk] != want[nk]]
    for name, k in bad:
        print(f"--- {name} {k}: recorded {want[(name, k)] if name != 'v5s_full' else '(the full rendering)'}, now:")
        print("\n".join(scheds["v5s" if name == "v5s_full" else name][k]))
    assert not bad, f"compiled backward schedules differ from the record: {bad}"


@pytest.fixture(scope="module")
def det_v5s(dev):
    """YOLOv5s at 2 x 3 x 128 x 128 whose program was built in deterministic mode (no atomics anywhere in the backward), without
    launch-parameter timing; the mode stays on while the module's cases run, since switching it off marks the program stale"""
    import yoloseries_amd
    from yoloseries_amd import models
    mp = pytest.MonkeyPatch()
    mp.setenv("YH_CONV_TUNE", "0")
    mp.setenv("YH_WGRAD_TUNE", "0")
    yoloseries_amd.set_deterministic(True)
    try:
        torch.manual_seed(0)
        m = models.YOLOV5Small(3, 80).to(dev).train()
        x = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(5)).to(dev)
        _pass(m, x)
        prog = m._yh_program(2, 128, 128)
        assert prog.bwd_deterministic
        yield m, x, prog
    finally:
        yoloseries_amd.set_deterministic(False)
        mp.undo()


def _pass(m, x):
    for p_ in m.parameters():
        p_.grad = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # eval() under autograd warns once per model
        sum((o.float() ** 2).mean() for o in m(x)).backward()
    torch.cuda.synchronize()
    return m._yh_last_flat_grad.clone()


@pytest.mark.parametrize("two,frozen,hooked", list(itertools.product((True, False), repeat=3)))
def test_runners_agree_bit_for_bit(det_v5s, two, frozen, hooked):
    """forward + backward of one deterministic program on the same weights and input, once through each runner (flags.USE_EXEC
    flipped in between): the bucket hook gets the same slices in the same order (at least 3), every finisher runs once, and
    the flat gradient is EQUAL — both runners issue the same launches on the same descriptors, and nothing in this mode sums
    with atomics.  Measured at the commit before the per-launch runner read the compiled array: equal in all eight cases."""
    from yoloseries_amd import engine
    m, x, prog = det_v5s
    old_exec, old_two = engine.flags.USE_EXEC, prog.two_streams
    res = {}
    try:
        prog.two_streams = two
        m.train(not frozen)
        for use in (False, True):
            engine.flags.USE_EXEC = use
            slices, done = [], []

            def hook(part):
                slices.append((part.storage_offset(), part.numel()))
                k = len(slices) - 1
                return lambda: done.append(k)
            if hooked:
                m._yh_bucket_hook = hook
            g = _pass(m, x)
            m.__dict__.pop("_yh_bucket_hook", None)
            res[use] = (slices, sorted(done), g)
    finally:
        engine.flags.USE_EXEC, prog.two_streams = old_exec, old_two
        m.__dict__.pop("_yh_bucket_hook", None)
        m.train()
    (s0, d0, g0), (s1, d1, g1) = res[False], res[True]
    print(f"two={two} frozen={frozen} hooked={hooked}: buckets {s1}, max |g| {g0.abs().max().item():.4g}, "
          f"differing elements {(g0 != g1).sum().item()}, max diff {(g0 - g1).abs().max().item():.4g}")
    assert torch.isfinite(g0).all() and g0.abs().max() > 0
    assert s0 == s1
    if hooked:
        assert len(s1) >= 3 and len(set(s1)) == len(s1)
        assert d0 == d1 == list(range(len(s1)))
    else:
        assert not s1 and not d1
    assert torch.equal(g0, g1)
