"""Plan table of yh_conv_wgrad: what the library decides for a weight-gradient descriptor, without a device.

One line per descriptor:  key -> form, kernel name, tiles / effective splits / honoured tile_k, ws_bytes  — the fields of
yh_conv_wgrad_info.  Planning is host code: the query makes no HIP call and dereferences no operand, so the operands are fake
16-byte-aligned addresses and the table is the same on a machine without a GPU.  This tool never calls yh_conv_wgrad: with fake
operands that would be a real launch.  Two builds of the library plan alike exactly when their tables are byte-identical:

    YH_LIBRARY=/path/to/old/libyolohip.so python tools/wgrad_plan_table.py --all > old.txt
    python tools/wgrad_plan_table.py --all > new.txt && cmp old.txt new.txt

A library from before yh_conv_wgrad_info lacks the symbol; for it the columns are composed the way the engine used to
(compose_legacy: the name queries patched up as Program._wgrad_name did, yh_conv_wgrad_tiles2, yh_conv_wgrad_ws_bytes).  Two columns
had no query at all — the effective splits and whether tile_k was honoured: there compose_legacy RESTATES the rounding of the old
wg_split_plan (on the k-step of the reported name) and the wg_wide / tk64 rules of csrc/conv_wgrad.hip.  compose_legacy goes with the next pull request.

Corpus (--all):
  table    every weight-gradient key of yoloseries_amd/tune_defaults.json (wgrad10 / wgrad11: without / with a workspace, an `f`
           suffix: fused BatchNorm backward) with its shipped (splits, tile_k), and with tile_k {0, 32, 35, 40, 64, 128, 129} x
           splits {1, 5, 192, 1024} x workspace absent / present;
  random   a seeded sweep (--random N, default 20000): N = 8 .. 1280, Kseg on both sides of 128 / 160 / 256 / 384, N on both sides of
           32 / 64, maps whose pixel count is no multiple of 32 or 64, upsampled segments, bn_z, coff_k / Ctot segments, a workspace that
           is large, exact or 4 bytes short, and sizes on both sides of the 2 GiB limits.

tests/test_host_logic.py::test_wgrad_plan_table_is_stable compares digest(reduced()) — the shipped entries and 2 000 random cases,
one sha256 per 100 lines plus the set of kernel names (conv_plan_table.digest) — with tests/golden/wgrad_plan_digest.json (--digest
writes it; --reduced prints the lines themselves)."""
import argparse
import ctypes as C
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
from conv_plan_table import digest  # noqa: E402

P = 0x10000          # fake operand addresses: P * k (16-byte aligned, never dereferenced)
BIG = 1 << 40        # a workspace that holds anything
FIELDS = ("N", "ldg", "C", "ld", "ups", "coff_k", "Ctot", "B", "Ho", "Wo", "Hi", "Wi", "KH", "stride", "pad", "splits", "tile_k", "bn",
          "ws")          # ws: 0 no workspace, 1 large, 2 exactly yh_conv_wgrad_ws_bytes, 3 four bytes short
FORMS = ("im2col", "patch", "wave")


def make_desc(L, c):
    from yoloseries_amd._lib import WgradDesc
    d = WgradDesc()
    d.gy, d.ldg, d.N = P, c["ldg"], c["N"]
    d.seg.ptr, d.seg.C, d.seg.ld, d.seg.ups = 2 * P, c["C"], c["ld"], c["ups"]
    d.coff_k, d.Ctot = c["coff_k"], c["Ctot"]
    d.B, d.Ho, d.Wo, d.Hi, d.Wi = c["B"], c["Ho"], c["Wo"], c["Hi"], c["Wi"]
    d.KH = d.KW = c["KH"]
    d.stride, d.pad, d.dw = c["stride"], c["pad"], 3 * P
    d.splits, d.tile_k = c["splits"], c["tile_k"]
    if c["bn"]:
        d.bn_z, d.bn_ldz, d.bn_ws, d.bn_gamma, d.bn_coef = 4 * P, c["N"], 5 * P, 6 * P, 7 * P
    if c["ws"]:
        d.partial, d.partial_bytes = 8 * P, BIG
        if c["ws"] > 1:
            d.partial_bytes = max(0, L.yh_conv_wgrad_ws_bytes(C.byref(d)) - (4 if c["ws"] == 3 else 0))
    return d


_TK64 = {"1, 5, 1, 1, 32, 3, true": "1, 5, 1, 1, 64, 3, true", "1, 4, 1, 2, 32, 3, true": "1, 4, 1, 2, 64, 2, true",
         "1, 4, 1, 3, 32, 3, false": "1, 4, 1, 3, 64, 2, false", "1, 4, 2, 1, 32, 4, false": "1, 4, 2, 1, 64, 2, false",
         "1, 4, 2, 2, 32, 3, false": "1, 4, 2, 2, 64, 2, false"}


def compose_legacy(L, d):
    """(form, name, tiles, effective splits, honoured tile_k, ws_bytes) from the queries of a library without yh_conv_wgrad_info.
    DELETE with the next pull request: every library then has the query."""
    N, Kseg, tk = d.N, d.KH * d.KW * d.seg.C, d.tile_k
    args = L.yh_conv_wgrad_kernel_name2(N, Kseg, tk).decode()[len("conv_wgrad_kernel<"):-len(", false>")]
    wide = Kseg <= 384 and not (tk == 128 and Kseg >= 128)
    tk64 = tk == 64 and args in _TK64
    if tk64:
        args = _TK64[args]
    form, name, tiles = 0, f"conv_wgrad_kernel<{args}, {'true' if d.bn_z else 'false'}>", L.yh_conv_wgrad_tiles2(N, Kseg, tk)
    step = int(args.split(", ")[4])
    rps = (-(-d.B * d.Ho * d.Wo // max(d.splits, 1)) + step - 1) // step * step
    splits = -(-d.B * d.Ho * d.Wo // rps)
    ok = tk64 or (tk == 128 and not wide and Kseg <= 384) or (tk in (32, 35) and args.startswith(("4, 2, 1, 2, 32", "2, 2, 2, 2, 32")))
    if tk == 129 and L.yh_conv_wgrad_wave_tiles(C.byref(d)) > 0:
        form, name, tiles, splits, ok = 2, L.yh_conv_wgrad_wave_name(C.byref(d)).decode(), L.yh_conv_wgrad_wave_tiles(C.byref(d)), d.splits, True
    elif tk == 40 and L.yh_conv_wgrad_patch_ok(C.byref(d)):
        buf = C.create_string_buffer(96)
        L.yh_conv_wgrad_patch_name(C.byref(d), buf, 96)
        form, name, splits, ok = 1, buf.value.decode(), d.splits, True
    return form, name, tiles, splits, tk if ok else 0, L.yh_conv_wgrad_ws_bytes(C.byref(d))


def info(L, d):
    """(rc, form, name, tiles, effective splits, honoured tile_k, ws_bytes) of one descriptor; rc None from compose_legacy"""
    if not hasattr(L, "yh_conv_wgrad_info"):
        return (None,) + compose_legacy(L, d)
    from yoloseries_amd._lib import WgradInfo
    o = WgradInfo()
    rc = L.yh_conv_wgrad_info(C.byref(d), C.byref(o))
    return rc, o.form, o.name.decode(), o.tiles, o.splits, o.tile_k, o.ws_bytes


def answer(L, d):
    _, form, name, tiles, splits, tk, ws = info(L, d)
    return f"{FORMS[form]}, {name}, tiles {tiles} splits {splits} tile_k {tk}, ws_bytes {ws}"


def case_of_key(prefix, f):
    """the case a tuning-table key describes (engine/tune.py builds the key from the descriptor)"""
    N, ldg, Cs, ld, ups, Ctot, B, Ho, Wo, Hi, Wi, k, stride, pad = f
    return dict(N=N, ldg=ldg, C=Cs, ld=ld, ups=ups, coff_k=0, Ctot=Ctot, B=B, Ho=Ho, Wo=Wo, Hi=Hi, Wi=Wi, KH=k, stride=stride, pad=pad,
                splits=1, tile_k=0, bn=int(prefix.endswith("f")), ws=int(prefix.startswith("wgrad11")))


def table_keys():
    with open(os.path.join(ROOT, "yoloseries_amd", "tune_defaults.json")) as f:
        t = json.load(f)
    for k, v in sorted(t.items()):
        prefix, _, rest = k.partition(":")
        if prefix in ("wgrad10", "wgrad10f", "wgrad11", "wgrad11f"):
            yield k, prefix, [int(x) for x in rest.split(",")], v


def table_cases(shipped_only=False):
    """(label, case) of the tuning-table part"""
    for key, prefix, f, (splits, tile_k) in table_keys():
        c = case_of_key(prefix, f)
        c.update(splits=splits, tile_k=tile_k)
        yield f"{key} shipped {splits},{tile_k}", dict(c)
        if shipped_only:
            continue
        for tk in (0, 32, 35, 40, 64, 128, 129):
            for sp in (1, 5, 192, 1024):
                for ws in (0, 1):
                    c.update(splits=sp, tile_k=tk, ws=ws)
                    yield f"{key} k{tk} s{sp} w{ws}", dict(c)


def random_case(r):
    """one case of the seeded sweep: a plausible layer of one of several kinds"""
    kind = r.choice(("any", "any", "pointwise", "edge", "edge", "stem", "patch", "wave", "big", "big"))
    k, stride = r.choice(((1, 1), (1, 1), (3, 1), (3, 1), (3, 2), (5, 1), (6, 2), (7, 1)))
    pad = r.choice((k // 2, k // 2, 0))
    B = r.choice((1, 2, 3, 8, 16, 64, 128))
    Ho = r.choice((1, 3, 7, 13, 20, 33, 40, 64, 80, 81, 160))
    Wo = r.choice((Ho, Ho, Ho + 1, 32, 96))
    N = 8 * r.randint(1, 160)
    Cs = 8 * r.randint(1, 80)
    ups, bn = 0, 0
    if kind == "pointwise":
        k, stride, pad = 1, 1, 0
        Cs = r.choice((64, 120, 128, 136, 160, 168, 256, 264, 320, 384, 392, 512))
    elif kind == "edge":           # Kseg and N around the thresholds of the tilings
        k, stride, pad = r.choice(((1, 1, 0), (1, 1, 0), (3, 1, 1)))
        Kseg = r.choice((128, 160, 256, 384)) + r.choice((-72, -8, 0, 0, 8, 72))
        Cs = max(8, (Kseg // (k * k)) // 8 * 8)
        N = r.choice((8, 24, 32, 40, 56, 64, 72, 128, 136, 256))
    elif kind == "stem":
        k, stride, pad, Cs = 3, 1, 1, r.choice((16, 16, 24, 32))
        N = r.choice((16, 32, 48, 64, 80))
        bn = r.choice((0, 1, 1))
        Wo, Ho = r.choice((32, 64, 160, 320, 100)), r.choice((8, 64, 320, 33))
    elif kind == "patch":
        k, stride, pad = r.choice(((3, 1, 1), (3, 2, 1), (1, 1, 0)))
        Cs, N = r.choice((16, 32, 64)), r.choice((8, 16, 32, 48, 64, 72))
        bn = r.choice((0, 0, 1))
    elif kind == "wave":
        k, stride, pad = r.choice(((1, 1, 0), (3, 1, 1), (3, 2, 1)))
        Cs, N = 32 * r.randint(1, 20), r.choice((56, 64, 128, 160, 256, 320, 640))
        Ho = Wo = r.choice((20, 40, 80, 13, 16))
        B = r.choice((2, 16, 32, 64))
    elif kind == "big":            # around 2 GiB of gy / input per launch and per image
        B = r.choice((1, 2, 64, 128, 256))          # (B * Ho * Wo stays below 2^31: the old workspace query divides by zero beyond)
        Ho = Wo = r.choice((160, 320, 640, 1280, 2048))
        Cs, N = r.choice((8, 32, 64, 256)), r.choice((8, 32, 64, 256))
    if r.random() < 0.15 and stride == 1:
        ups = 1
        Ho, Wo = 2 * ((Ho + 1) // 2), 2 * ((Wo + 1) // 2)
    Hi, Wi = (Ho - 1) * stride + k - 2 * pad, (Wo - 1) * stride + k - 2 * pad
    if stride == 2 and r.random() < 0.7:
        Hi, Wi = Hi + 1, Wi + 1               # the even map a stride-2 layer usually reads
    if ups and (Hi % 2 or Wi % 2) and r.random() < 0.8:
        ups = 0
    Ctot = Cs + r.choice((0, 0, 0, 8, 64, Cs))
    coff_k = r.choice((0, 8 * r.randint(0, (Ctot - Cs) // 8)))
    bn = bn or int(r.random() < 0.05)
    return dict(N=N, ldg=(N + 7) // 8 * 8 + r.choice((0, 0, 0, 8, 256)), C=Cs, ld=Cs + r.choice((0, 0, 0, 8, 64, Cs, 4096)), ups=ups,
                coff_k=coff_k, Ctot=Ctot, B=B, Ho=Ho, Wo=Wo, Hi=Hi, Wi=Wi, KH=k, stride=stride, pad=pad,
                splits=r.choice((1, 2, 5, 37, 192, 256, 1024, 4096, 70000, 200000)), tile_k=r.choice((0, 0, 0, 32, 35, 40, 64, 128, 129, 129, 7)),
                bn=bn, ws=r.choice((0, 0, 1, 1, 2, 3)))


def random_cases(n, seed=20261018):
    r = random.Random(seed)
    for i in range(n):
        c = random_case(r)
        yield f"r{i}:" + ",".join(str(c[f]) for f in FIELDS), c


def reduced_cases():
    """the slice the CPU tests use: the shipped entries and 2 000 random cases"""
    yield from table_cases(shipped_only=True)
    yield from random_cases(2000)


def lines(L, cases):
    for label, c in cases:
        yield f"{label} -> {answer(L, make_desc(L, c))}"


def reduced(L):
    return lines(L, reduced_cases())


def load_library():
    """the library as it is — not through _lib.lib(), which insists on every symbol of today's header (YH_LIBRARY may be older)"""
    import torch  # noqa: F401  (binds the HIP runtime the library wants, as _lib.lib() does)
    from yoloseries_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for name, (res, args) in _lib._SIGS.items():
        if name.startswith("yh_conv_wgrad") and name != "yh_conv_wgrad" and hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, args
    if not hasattr(L, "yh_conv_wgrad_info"):
        L.yh_conv_wgrad_kernel_name2.restype, L.yh_conv_wgrad_kernel_name2.argtypes = C.c_char_p, [C.c_int32] * 3
    return L


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--all", action="store_true", help="table + random parts")
    ap.add_argument("--reduced", action="store_true", help="the slice tests/golden/wgrad_plan_digest.json records, line by line")
    ap.add_argument("--digest", action="store_true", help="that slice as tests/golden/wgrad_plan_digest.json holds it")
    ap.add_argument("--random", type=int, default=20000)
    a = ap.parse_args()
    L = load_library()
    out = sys.stdout
    if a.reduced:
        out.writelines(ln + "\n" for ln in reduced(L))
    if a.digest:
        json.dump(digest(reduced(L)), out, indent=0)
        out.write("\n")
    if a.all:
        out.writelines(ln + "\n" for ln in lines(L, table_cases()))
        out.writelines(ln + "\n" for ln in lines(L, random_cases(a.random)))


if __name__ == "__main__":
    main()
