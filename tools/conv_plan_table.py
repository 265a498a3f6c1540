"""Plan table of yh_conv_igemm: what the library decides for a descriptor, without a device.

One line per descriptor:  key -> rc, kernel name, yh_conv_stat_blocks, yh_conv_bnr_rows  — obtained only through the C ABI
(yh_conv_info, which answers what the three older queries answer).  Planning and naming are host code: the query makes
no HIP call and dereferences no operand pointer, so the operands are fake 16-byte-aligned addresses and the table is the same on
a machine without a GPU.  Two builds of the library plan alike exactly when their tables are byte-identical:

    YH_LIBRARY=/path/to/old/libyolohip.so python tools/conv_plan_table.py --all > old.txt
    python tools/conv_plan_table.py --all > new.txt && cmp old.txt new.txt

Corpus (--all):
  table    every conv key of yoloseries_amd/tune_defaults.json with its shipped (tile_k, grid_cap, algo) and with every
           algo x tile_k {0, 32} x tile_n {0, 32, 64, 128} x grid_cap {0, 2 * base} (base as the tuner takes it);
  random   a seeded sweep (--random N, default 24000) over the same fields and what the table lacks: odd maps, N = 8 .. 1280, ragged
           last segments, two segments with upsampling, stride-2 data gradients, split destinations, sizes on both sides of the
           2 GiB descriptor limits and invalid descriptors (their rc is part of the record);
  env      the table part again under each planning switch — YH_CONV_DBG = 16, 64, 256, 512, 1024, YH_HALO_MAP = 0, 2,
           YH_STEM_MAP = 0 — each in a fresh child process (the library reads them once).  YH_STEM_MAP / YH_HALO_MAP only steer the
           block order inside a launch (ConvK.xgx / HaloGeom.rowmajor): names and rows do not show them.

tests/test_host_logic.py::test_conv_plan_table_is_stable compares digest(reduced()) — the shipped entries and 2 000 random cases,
as one sha256 per 100 lines plus the set of kernel names — with tests/golden/conv_plan_digest.json (--digest writes it;
--reduced prints the lines themselves, to find what changed inside a chunk)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ALGOS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 14)
ENVS = [("YH_CONV_DBG", v) for v in ("16", "64", "256", "512", "1024")] + [("YH_HALO_MAP", "0"), ("YH_HALO_MAP", "2"), ("YH_STEM_MAP", "0")]
P = 0x10000          # fake operand addresses: P * k (16-byte aligned, never dereferenced)

# every field a case carries (the key of a random case is these values in this order)
FIELDS = ("mode", "B", "Ho", "Wo", "Hi", "Wi", "KH", "KW", "stride", "pad", "N", "Npad", "nseg", "C0", "lds0", "ups0", "C1", "lds1", "ups1",
          "ld0", "nsplit", "ld1", "ldr", "accumulate", "stats", "res", "act", "bias", "scale", "shift", "bnr", "bnr_ldz", "bnr_C",
          "tile_k", "tile_n", "grid_cap", "algo", "ptrs")


def make_desc(c):
    """ConvDesc of a case (dict over FIELDS).  ptrs: 0 all operands present; 1 seg[0].ptr null, 2 weights unaligned, 3 out0 null,
    4 out1 missing, 5 fused-reduction operands missing"""
    from yoloseries_amd._lib import ConvDesc
    d = ConvDesc()
    ptrs = c["ptrs"]
    d.seg[0].ptr, d.seg[0].C, d.seg[0].ld, d.seg[0].ups = (None if ptrs == 1 else P), c["C0"], c["lds0"], c["ups0"]
    if c["nseg"] >= 2:
        d.seg[1].ptr, d.seg[1].C, d.seg[1].ld, d.seg[1].ups = 2 * P, c["C1"], c["lds1"], c["ups1"]
    d.nseg, d.mode = c["nseg"], c["mode"]
    d.B, d.Ho, d.Wo, d.Hi, d.Wi = c["B"], c["Ho"], c["Wo"], c["Hi"], c["Wi"]
    d.KH, d.KW, d.stride, d.pad = c["KH"], c["KW"], c["stride"], c["pad"]
    d.w = 3 * P + 8 if ptrs == 2 else 3 * P
    d.N, d.Npad = c["N"], c["Npad"]
    d.bias = 4 * P if c["bias"] else None
    d.scale = 5 * P if c["scale"] else None
    d.shift = 6 * P if c["shift"] else None
    d.act, d.accumulate = c["act"], c["accumulate"]
    d.out0, d.ld0, d.nsplit = (None if ptrs == 3 else 7 * P), c["ld0"], c["nsplit"]
    if c["nsplit"] < c["N"] and ptrs != 4:
        d.out1 = 8 * P
    d.ld1, d.ldr = c["ld1"], c["ldr"]
    d.res = 9 * P if c["res"] else None
    d.stats = 10 * P if c["stats"] else None
    d.tile_n, d.grid_cap, d.tile_k, d.algo = c["tile_n"], c["grid_cap"], c["tile_k"], c["algo"]
    if c["bnr"]:
        d.bnr_part = 13 * P
        if ptrs != 5:
            d.bnr_z, d.bnr_ws = 11 * P, 12 * P
        d.bnr_ldz, d.bnr_C = c["bnr_ldz"], c["bnr_C"]
    return d


def answer(L, d):
    """'rc, kernel name, stat blocks, bnr rows' of one descriptor"""
    from yoloseries_amd._lib import ConvInfo
    o = ConvInfo()
    rc = L.yh_conv_info(C.byref(d), C.byref(o))
    return f"{rc}, {o.name.decode() if rc == 0 else '-'}, {o.stat_rows}, {o.bnr_rows}"


def case_of_key(f):
    """the case a tuning-table key describes (engine/tune.py builds the key from the descriptor)"""
    (mode, B, Ho, Wo, Hi, Wi, k, stride, pad, N, nseg, C0, lds0, ups0, C1, ups1, ld0, nsplit, accumulate, stats, res, act, bias, scale,
     bnr, _) = f
    n0 = min(nsplit, N)
    return dict(mode=mode, B=B, Ho=Ho, Wo=Wo, Hi=Hi, Wi=Wi, KH=k, KW=k, stride=stride, pad=pad, N=N, Npad=(N + 127) // 128 * 128,
                nseg=nseg, C0=C0, lds0=lds0, ups0=ups0, C1=C1, lds1=C1, ups1=ups1, ld0=ld0, nsplit=nsplit, ld1=(N - n0 + 8 + 7) // 8 * 8,
                ldr=(n0 + 7) // 8 * 8, accumulate=accumulate, stats=stats, res=res, act=act, bias=bias, scale=scale, shift=scale, bnr=bnr,
                bnr_ldz=N, bnr_C=N, tile_k=0, tile_n=0, grid_cap=0, algo=0, ptrs=0)


def table_keys():
    with open(os.path.join(ROOT, "yoloseries_amd", "tune_defaults.json")) as f:
        t = json.load(f)
    for k, v in sorted(t.items()):
        parts = k.split(":")
        if len(parts) == 3 and parts[1] in ("fwd", "dgrad", "eval"):
            yield k, [int(x) for x in parts[2].split(",")], v


def table_lines(L, shipped_only=False):
    for key, f, (tile_k, grid_cap, algo) in table_keys():
        c = case_of_key(f)
        c.update(tile_k=tile_k, grid_cap=grid_cap, algo=algo)
        yield f"{key} shipped {tile_k},{grid_cap},{algo} -> {answer(L, make_desc(c))}"
        if shipped_only:
            continue
        c.update(tile_k=0, grid_cap=0, algo=1)
        base = L.yh_conv_stat_blocks(C.byref(make_desc(c)))
        for algo in ALGOS:
            for tk in (0, 32):
                for tn in (0, 32, 64, 128):
                    for cap in (0, 2 * base):
                        c.update(tile_k=tk, tile_n=tn, grid_cap=cap, algo=algo)
                        yield f"{key} a{algo} k{tk} n{tn} g{cap} -> {answer(L, make_desc(c))}"


def random_case(r):
    """one case of the seeded sweep: a plausible layer of one of several kinds, then (one time in four) something broken in it"""
    kind = r.choice(("any", "any", "pointwise", "halo", "halo", "stem", "s2dgrad", "s2dgrad", "big", "two"))
    mode = r.choice((0, 1))
    k, stride = r.choice(((1, 1), (3, 1), (3, 2), (5, 1), (2, 2), (6, 2), (7, 1)))
    pad = r.choice((k // 2, k // 2, 0, 1))
    B = r.choice((1, 2, 3, 8, 16, 64, 128))
    Ho = r.choice((1, 3, 7, 13, 20, 33, 40, 64, 80, 81, 160, 320))
    Wo = r.choice((Ho, Ho, Ho + 1, 32, 96, 160))
    N = 8 * r.randint(1, 160)
    nseg = 1
    C0 = r.choice((8, 16, 24, 32, 40, 48, 64, 80, 96, 128, 160, 192, 256, 320, 384, 512, 640, 1024))
    C1, ups0, ups1 = 0, 0, 0
    if kind == "pointwise":
        k, stride, pad = 1, 1, 0
        C0 = r.choice((64, 128, 256, 320, 512))
    elif kind == "halo":
        mode, k, stride, pad = r.choice((0, 0, 1)), 3, 1, 1
        C0 = r.choice((48, 64, 80, 96, 128, 160, 256, 320, 640))
        N = r.choice((N, 64, 128, 160, 256, 320, 640))
    elif kind == "stem":
        mode, k, stride, pad, C0 = 0, 3, 1, 1, 16
        N = r.choice((16, 32, 48, 64, 80, 96, 112))
        Wo = r.choice((32, 64, 160, 320, 640, 100))
        Ho = r.choice((8, 64, 320, 640, 33))
    elif kind == "s2dgrad":
        mode, stride = 1, 2
        k = r.choice((3, 3, 2, 6, 1))
        pad = r.choice((k // 2, 0, 2 if k == 6 else 1))
        Ho, Wo = r.choice((40, 80, 160, 320, 41)), r.choice((40, 80, 160, 320, 43))
        N = r.choice((N, 32, 64, 128, 256, 512))
    elif kind == "big":
        B = r.choice((128, 256, 512, 1024))
        Ho = Wo = r.choice((320, 640, 1280, 2048))
        C0 = r.choice((8, 32, 64, 128, 256))
    elif kind == "two":
        mode, nseg = 0, 2
        C0 = r.choice((32, 64, 96, 128, 256, 48))
        C1 = r.choice((C0, C0, 16, 24, 40, 64, 128))
        ups0, ups1 = r.choice(((0, 0), (1, 0), (0, 1)))
        if ups0 or ups1:
            Ho, Wo = 2 * ((Ho + 1) // 2), 2 * ((Wo + 1) // 2)
    if mode == 0:
        Hi, Wi = (Ho - 1) * stride + k - 2 * pad, (Wo - 1) * stride + k - 2 * pad
        if stride == 2 and r.random() < 0.5:
            Hi, Wi = Hi + 1, Wi + 1               # the even map a stride-2 layer usually reads
    else:
        Hi, Wi = (Ho + 2 * pad - k) // stride + 1, (Wo + 2 * pad - k) // stride + 1
    lds0 = C0 + r.choice((0, 0, 0, 8, 64, C0, 4096, 65536))
    lds1 = C1 + r.choice((0, 0, 8, C1))
    plain = r.random() < 0.5
    stats = int(r.random() < (0.4 if plain else 0.1))
    bnr = int(mode == 1 and r.random() < (0.5 if plain else 0.1))
    scale = 0 if plain else r.choice((0, 1, 1))
    nsplit = N if plain or r.random() < 0.6 else r.choice((8 * r.randint(1, max(1, N // 8)), 8 * r.randint(1, max(1, N // 8)), N // 16 * 8 + 8, N + 8, N + 8, 12))
    c = dict(mode=mode, B=B, Ho=Ho, Wo=Wo, Hi=Hi, Wi=Wi, KH=k, KW=k, stride=stride, pad=pad, N=N, Npad=(N + 127) // 128 * 128 + r.choice((0, 0, 0, 128)),
             nseg=nseg, C0=C0, lds0=lds0, ups0=ups0, C1=C1, lds1=lds1, ups1=ups1, ld0=(N + 7) // 8 * 8 + r.choice((0, 0, 8, 256)), nsplit=nsplit,
             ld1=(max(N - nsplit, 0) + 15) // 8 * 8, ldr=(N + 7) // 8 * 8, accumulate=0 if plain else r.choice((0, 0, 1)), stats=stats,
             res=0 if plain else r.choice((0, 0, 1)), act=0 if plain else r.choice((0, 1)), bias=0 if plain else r.choice((0, 0, 1)),
             scale=scale, shift=scale, bnr=bnr, bnr_ldz=N + r.choice((0, 0, 8)), bnr_C=N + r.choice((0, 0, 8)),
             tile_k=r.choice((0, 0, 32)), tile_n=r.choice((0, 0, 0, 32, 64, 128)), grid_cap=r.choice((0, 0, 0, 8, 24, 100, 1000)),
             algo=r.choice(ALGOS), ptrs=0)
    if r.random() < 0.25:          # invalid descriptors: one field broken
        what = r.randrange(16)
        if what == 0: c["nseg"] = r.choice((0, 3))
        elif what == 1: c["mode"] = 2
        elif what == 2: c["stride"] = r.choice((0, 3))
        elif what == 3: c[r.choice(("B", "Ho", "Wo", "Hi", "Wi"))] = r.choice((0, -1))
        elif what == 4: c["KH"] = r.choice((0, 8, c["KH"] + 1))
        elif what == 5: c["C0"] = c["C0"] + r.choice((4, -8, 1))
        elif what == 6: c["lds0"] = r.choice((c["C0"] - 8, c["C0"] + 4))
        elif what == 7: c["N"] = c["N"] + r.choice((1, 4, -c["N"]))
        elif what == 8: c["Npad"] = r.choice((c["N"], c["Npad"] - 128, c["Npad"] + 64, 0))
        elif what == 9: c["shift"] = 1 - c["shift"]
        elif what == 10: c["ptrs"] = r.randint(1, 5)
        elif what == 11: c["Hi"], c["Wi"] = c["Hi"] + r.choice((1, 2, -1)), c["Wi"] + 1
        elif what == 12: c["ups0"] = r.choice((1, 2))
        elif what == 13: c["ld0"] = c["ld0"] + 4
        elif what == 14: c["bnr_C"] = c["N"] - 8
        else: c["pad"] = r.choice((-1, 3, 5))
    return c


def random_lines(L, n, seed=20261016):
    r = random.Random(seed)
    for i in range(n):
        c = random_case(r)
        yield f"r{i}:" + ",".join(str(c[f]) for f in FIELDS) + f" -> {answer(L, make_desc(c))}"


def reduced(L):
    """the slice the CPU test pins: the shipped entries and 2 000 random cases"""
    yield from table_lines(L, shipped_only=True)
    yield from random_lines(L, 2000)


def digest(lines, chunk=100):
    """a table in a few KB: one sha256 per `chunk` lines and the distinct kernel instantiations"""
    lines = list(lines)
    names = sorted({ln.split(" -> ")[1].split(", ", 1)[1].rsplit(", ", 2)[0] for ln in lines} - {"-"})
    return {"lines": len(lines), "chunk": chunk, "names": names,
            "sha256": [hashlib.sha256("\n".join(lines[i:i + chunk]).encode()).hexdigest() for i in range(0, len(lines), chunk)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--all", action="store_true", help="table + random + env parts")
    ap.add_argument("--table", action="store_true", help="the tuning-table part only (what a child process of --all prints)")
    ap.add_argument("--reduced", action="store_true", help="the slice tests/golden/conv_plan_digest.json records, line by line")
    ap.add_argument("--digest", action="store_true", help="that slice as tests/golden/conv_plan_digest.json holds it")
    ap.add_argument("--random", type=int, default=24000)
    a = ap.parse_args()
    from yoloseries_amd._lib import lib
    L = lib()
    out = sys.stdout
    if a.reduced:
        out.writelines(ln + "\n" for ln in reduced(L))
    if a.digest:
        json.dump(digest(reduced(L)), out, indent=0)
        out.write("\n")
    if a.table or a.all:
        out.writelines(ln + "\n" for ln in table_lines(L))
    if a.all:
        out.writelines(ln + "\n" for ln in random_lines(L, a.random))
        for name, val in ENVS:
            out.write(f"# {name}={val}\n")
            out.flush()
            env = dict(os.environ)
            env[name] = val
            subprocess.run([sys.executable, os.path.abspath(__file__), "--table"], env=env, stdout=out, check=True)


if __name__ == "__main__":
    main()
