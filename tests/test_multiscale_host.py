"""Host side of multi-scale training (utils/multiscale.py, engine/module.py): the NumPy statement of the bilinear resize against
torch's CPU F.interpolate (live and recorded in tests/golden/g16_multiscale.npz by tools/gen_golden_multiscale.py), the draw of the
step's shape, and the program cache's eviction order.

torch's CPU build has two bilinear kernels and picks by the output size (Ho + Wo <= 128: four weighted taps summed; larger: rows
then columns); resize_bilinear_host makes the same switch.  The `small_*` cases take the first, `general_*` on the other."""
import math
import os
import random

import numpy as np
import pytest

from yoloseries_amd.utils.multiscale import bilinear_tables, draw_multiscale_shape, resize_bilinear_host

G = os.path.join(os.path.dirname(__file__), "golden", "g16_multiscale.npz")
SIZES = {"small_up": (40, 72), "small_down": (16, 24), "small_identity": (24, 40), "small_odd": (45, 71),
         "general_up": (96, 160), "general_down": (64, 96)}
SMALL_CASES = ["small_up", "small_down", "small_identity", "small_odd"]


def load_case(name):
    """(input float32 = uint8 / 255, output size, torch's recorded output)"""
    g = np.load(G)
    return g[f"{name}_x"].astype(np.float32) / np.float32(255), SIZES[name], g[f"{name}_out"]


@pytest.mark.parametrize("name", SMALL_CASES)
def test_host_equals_live_interpolate(name):
    import torch
    import torch.nn.functional as F
    x, size, _ = load_case(name)
    got = resize_bilinear_host(x, size)
    ref = F.interpolate(torch.from_numpy(x), size=size, mode='bilinear', align_corners=False).numpy()
    diff = got != ref
    print(f"{name}: {diff.mean():.3f} of the elements differ, max |diff| {np.abs(got - ref).max():.3g}")
    np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("name", SMALL_CASES + ["general_up", "general_down"])
def test_host_equals_fixture(name):
    x, size, ref = load_case(name)
    got = resize_bilinear_host(x, size)
    assert got.dtype == np.float32 and got.shape == ref.shape == x.shape[:2] + size
    print(f"{name}: {(got != ref).mean():.3f} of the elements differ, max |diff| {np.abs(got - ref).max():.3g}")
    np.testing.assert_array_equal(got, ref)


def test_identity_is_a_copy():
    x, size, _ = load_case("small_identity")
    assert tuple(x.shape[2:]) == size
    np.testing.assert_array_equal(resize_bilinear_host(x, size), x)


def test_nothing_clamps_values():
    x = (np.random.RandomState(5).randn(1, 2, 9, 11) * 3).astype(np.float32)
    out = resize_bilinear_host(x, (9, 11))
    np.testing.assert_array_equal(out, x)
    up = resize_bilinear_host(x, (20, 30))
    assert up.min() < -1 and up.max() > 1 and up.min() >= x.min() and up.max() <= x.max()


@pytest.mark.parametrize("n_in,n_out", [(24, 40), (40, 24), (37, 45), (640, 960), (640, 320), (8, 8200), (5, 5), (1, 7)])
def test_tables(n_in, n_out):
    i0, i1, l0, l1 = bilinear_tables(n_in, n_out)
    assert i0.dtype == i1.dtype == np.int32 and l0.dtype == l1.dtype == np.float32 and len(i0) == len(l1) == n_out
    assert i0.min() >= 0 and i1.max() <= n_in - 1 and ((i1 == i0 + 1) | (i1 == n_in - 1)).all()
    assert (l1 >= 0).all() and (l1 <= 1).all() and np.array_equal(l0, np.float32(1) - l1)
    # fma(scale, d + 0.5, -0.5) in float32, element by element
    scale = np.float32(n_in) / np.float32(n_out)
    for d in (0, 1, n_out // 2, n_out - 1):
        src = max(np.float32(float(scale) * (d + 0.5) - 0.5), np.float32(0))      # exact in float64 before its one rounding
        assert i0[d] == min(int(src), n_in - 1) and l1[d] == np.float32(src - np.float32(i0[d]))


def test_draw_square():
    random.seed(1234)
    seen = set()
    for _ in range(2000):
        scale, shape = draw_multiscale_shape([640, 640], (640, 640))
        assert shape[0] == shape[1] and shape[0] % 32 == 0 and 320 <= shape[0] <= 960
        assert scale == shape[0] / 640
        seen.add(shape[0])
    assert min(seen) == 320 and max(seen) == 960 and seen == set(range(320, 961, 32))


def test_draw_non_square_follows_the_reference_lines():
    """train_yolov5.py:537-541 literally, on the same generator state"""
    hw, size = (480, 640), [512, 640]
    for seed in range(50):
        random.seed(seed)
        scale, shape = draw_multiscale_shape(size, hw)
        random.seed(seed)
        input_img_size = max(size)
        random_shape = random.randrange(int(input_img_size * 0.5), int(input_img_size * 1.5 + 32)) // 32 * 32
        want_scale = random_shape / max(hw)
        want = [math.ceil(x * want_scale / 32) * 32 for x in hw] if want_scale != 1. else list(hw)
        assert scale == want_scale and shape == want and max(shape) == random_shape


def test_draw_uses_the_global_generator():
    random.seed(7)
    a = [draw_multiscale_shape([128, 128], (128, 128))[1] for _ in range(20)]
    random.seed(7)
    b = [draw_multiscale_shape([128, 128], (128, 128))[1] for _ in range(20)]
    assert a == b and len({tuple(s) for s in a}) > 1 and all(64 <= s[0] <= 192 for s in a)


# ---------------------------------------------------------------- program cache
class StubProgram:
    def __init__(self, nbytes):
        self.nbytes = nbytes

    def owned_bytes(self):
        return self.nbytes


def _visit(progs, key, nbytes, budget):
    """what HipModuleMixin._yh_program does around a look-up"""
    from yoloseries_amd.engine.module import _evict_programs
    if key not in progs:
        progs[key] = StubProgram(nbytes)
    prog = progs[key]
    _evict_programs(progs, key, budget)
    assert key in progs and progs[key] is prog
    return prog


def test_cache_without_budget_is_first_in_first_out():
    progs = {}
    for k in "abcd":
        _visit(progs, k, 10, None)
    _visit(progs, "a", 10, None)                       # a hit does not refresh an entry ...
    assert list(progs) == list("abcd")
    _visit(progs, "e", 10, None)                       # ... so the oldest INSERTED goes, used last or not
    assert list(progs) == list("bcde")
    _visit(progs, "a", 10 ** 12, None)                 # bytes play no part
    assert list(progs) == list("cdea")


def test_cache_with_budget_is_least_recently_used():
    progs = {}
    for k in "abc":
        _visit(progs, k, 10, 30)
    assert list(progs) == list("abc")
    _visit(progs, "a", 10, 30)                         # refreshed: b is now the coldest
    assert list(progs) == list("bca")
    _visit(progs, "d", 10, 30)
    assert list(progs) == list("cad")
    _visit(progs, "e", 25, 30)                         # makes room for 25: everything else goes
    assert list(progs) == ["e"]
    for k in "fghijk":                                 # the count is not bounded: six small programs fit
        _visit(progs, k, 1, 31)
    assert list(progs) == list("efghijk")
    _visit(progs, "big", 100, 30)                      # larger than the budget on its own: it alone stays (the one in use is never dropped)
    assert list(progs) == ["big"]
    _visit(progs, "l", 1, 30)
    assert list(progs) == ["l"]


def test_cache_budget_follows_programs_that_grow():
    progs = {}
    a = _visit(progs, "a", 10, 30)
    _visit(progs, "b", 10, 30)
    a.nbytes = 25                                      # a built its training buffers after it was inserted
    _visit(progs, "b", 10, 30)
    assert list(progs) == ["b"]
