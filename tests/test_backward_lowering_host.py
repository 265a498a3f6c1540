"""The backward lowering (engine/backward.py compile_backward) on the host: hand-written command lists in the layout
_build_backward produces, integers in place of the event handles, nothing executed.  What both runners of the compiled array
follow is checked here once: the gz ring's records and waits, the serial schedule, on-main weight gradients, bucket breaks,
frozen-BatchNorm fills and the head-gradient patches."""
import types

import pytest

from yoloseries_amd._lib import BnPart, ConvDesc, WgradDesc, YH_CMD_EVENT_RECORD, YH_CMD_STREAM_WAIT, lib
from yoloseries_amd.engine.backward import compile_backward

EV_GZ, EV_WG = 1000, [2000, 2001, 2002]
SYNC = ('sync', 0, 0.0)


def _op(name, kind='cba'):
    return types.SimpleNamespace(name=name, kind=kind, y=types.SimpleNamespace(C=16), Ho=4, Wo=4)


def _main(L, label):
    """stands in for main-stream work"""
    return (L.yh_fill_u32, (0, 0, 0), label, ('yh_fill_u32', 0, 0.0))


def _layers(L, n, ngz, on_main_layers=()):
    """n consecutive ConvBnAct layers: gz_begin, the pass that WRITES the layer's gz buffer (main), the weight gradient that reads it
    (side, between wg_begin and wg_end — or on the main stream without them), the data gradient that reads it (main)"""
    cmds, on_main = [], set()
    for l in range(n):
        slot = l % ngz
        wd = WgradDesc()
        cmds += [('gz_begin', slot, None, SYNC), _main(L, f"write:{l}")]
        if l in on_main_layers:
            on_main.add(id(wd))
            cmds.append(('wgrad', _op(f"wgrad:{l}"), wd, ('wg', 1.0, 1.0)))
        else:
            cmds += [('wg_begin', None, None, SYNC), ('wgrad', _op(f"wgrad:{l}"), wd, ('wg', 1.0, 1.0)), ('wg_end', [slot], None, SYNC)]
        cmds.append(_main(L, f"read:{l}"))
    return cmds, on_main


def _lower(L, cmds, two=True, buckets=(), frozen=False, on_main=frozenset(), ngz=3):
    return compile_backward(L, cmds, two, list(buckets), frozen, EV_GZ if two else None, EV_WG[:ngz] if two else (), on_main,
                            lambda op: True, lambda op, boff: (0, op.y.C, op.y.C, 2 * op.Ho * op.Wo, 0x7000, 0x8000 + 4 * boff))


def _entries(cc):
    """[(kind 'call' | 'record' | 'wait', stream, label or event handle)]"""
    out = []
    for i in range(cc.n):
        c = cc.arr[i]
        if c.op == YH_CMD_EVENT_RECORD or c.op == YH_CMD_STREAM_WAIT:
            assert cc.py[i] == c.slots[0] and c.nslots == 1
            out.append(('record' if c.op == YH_CMD_EVENT_RECORD else 'wait', c.stream, int(c.slots[0])))
        else:
            assert c.op >= 0 and cc.names[i].endswith(f"[{cc.py[i][2][-1]}]")
            out.append(('call', c.stream, cc.py[i][2][-1]))
    assert len(cc.names) == len(cc.py) == cc.n
    return out


@pytest.mark.parametrize("ngz", [1, 2, 3])
def test_gz_ring_is_safe(ngz):
    """Replay of the emitted entries, 8 layers: what each stream KNOWS to be complete on the other is what the events it waited
    for had seen at their last record.  A side-stream weight gradient of layer l starts only behind a wait for a main-stream record
    that follows the pass writing l's gz; the pass that writes a gz buffer again starts only behind a main-stream wait for a
    side-stream record that follows every earlier weight gradient reading that buffer.  Every wg_begin is a record on stream 0
    directly followed by a wait for the same event on stream 1."""
    L = lib()
    n = 8
    cmds, _ = _layers(L, n, ngz)
    cc, breaks, patches = _lower(L, cmds, ngz=ngz)
    assert not breaks and not patches
    ent = _entries(cc)
    done = {0: set(), 1: set()}             # labels enqueued so far per stream
    seen = {}                               # event -> (stream it was last recorded on, what that stream had enqueued by then)
    knows = {0: set(), 1: set()}            # per stream: labels of the OTHER stream known complete
    wgrads = 0
    for kind, s, what in ent:
        if kind == 'record':
            seen[what] = (s, set(done[s]))
        elif kind == 'wait':
            src, labels = seen[what]        # (a wait for an event never recorded would be a KeyError)
            assert src != s
            knows[s] |= labels
        else:
            what_kind, l = what.split(":")
            l = int(l)
            if what_kind == 'wgrad':
                assert s == 1 and f"write:{l}" in knows[1], f"weight gradient of layer {l} may start before its gz is written"
                wgrads += 1
            else:
                assert s == 0
                if what_kind == 'write':
                    for l2 in range(l % ngz, l, ngz):
                        assert f"wgrad:{l2}" in knows[0], f"layer {l} may overwrite gz buffer {l % ngz} under layer {l2}'s weight gradient"
            done[s].add(what)
    assert wgrads == n
    begins = [i for i, e in enumerate(ent) if e == ('record', 0, EV_GZ)]
    assert len(begins) == n and all(ent[i + 1] == ('wait', 1, EV_GZ) for i in begins)
    # the ring lets the side stream lag: the main stream waits ngz layers late, never for the layer it has just handed over
    waits0 = [e[2] for e in ent if e[:2] == ('wait', 0)]
    assert waits0 == [EV_WG[l % ngz] for l in range(n - ngz)]
    assert [e[2] for e in ent if e[:2] == ('record', 1)] == [EV_WG[l % ngz] for l in range(n)]


def test_serial_schedule_has_no_events():
    L = lib()
    cmds, _ = _layers(L, 7, 3)
    cc, _, _ = _lower(L, cmds, two=False)
    ent = _entries(cc)
    assert all(kind == 'call' and s == 0 for kind, s, _ in ent)
    assert [w for _, _, w in ent] == [c[1].name if c[0] == 'wgrad' else c[2] for c in cmds if c[3] != SYNC]


def test_on_main_weight_gradient_stays_on_stream_0_without_events():
    L = lib()
    cmds, on_main = _layers(L, 7, 3, on_main_layers=(6,))
    ent = _entries(_lower(L, cmds, on_main=on_main)[0])
    i = ent.index(('call', 0, "wgrad:6"))
    assert ent[i - 1] == ('call', 0, "write:6") and ent[i + 1] == ('call', 0, "read:6")
    assert sum(1 for e in ent if e == ('record', 0, EV_GZ)) == 6 and ('call', 1, "wgrad:5") in ent


def test_bucket_breaks_and_frozen_fills():
    """breaks are the array positions of the first entry lowered from the bucket's command (the end for trailing buckets); with
    frozen=True every finalize is directly followed by the fill(s) of its coefficients, inside its command's segment"""
    L = lib()
    parts = (BnPart * 2)()
    parts[0].coef, parts[0].C, parts[1].coef, parts[1].C = 0x5000, 24, 0x6000, 40
    fin = (L.yh_bn_bwd_finalize, (0x100, 3, 32, 64, 0x200, 0x300, 0x400, 0x4000), "bn:0", ('yh_bn_bwd_finalize', 0, 1.0))
    finp = (L.yh_bn_bwd_finalize_parts, (parts, 2, 64), "bn:1", ('yh_bn_bwd_finalize', 0, 1.0))
    cmds = [('gz_begin', 0, None, SYNC), fin, _main(L, "write:0"), ('wg_begin', None, None, SYNC),
            ('wgrad', _op("wgrad:0"), WgradDesc(), ('wg', 1.0, 1.0)), ('wg_end', [0], None, SYNC), _main(L, "read:0"),
            ('gz_begin', 0, None, SYNC), finp, _main(L, "write:1")]
    buckets = [(2, 0, 10), (7, 10, 20), (9, 20, 30), (len(cmds), 30, 40)]
    cc, breaks, _ = _lower(L, cmds, buckets=buckets, ngz=1)
    assert breaks == [1, 7, 9, 10] and cc.n == 10
    cc, breaks, _ = _lower(L, cmds, buckets=buckets, frozen=True, ngz=1)
    assert breaks == [2, 8, 12, 13] and cc.n == 13
    ent = _entries(cc)
    assert [e[2] for e in ent] == ["bn:0", "bn:0", "write:0", EV_GZ, EV_GZ, "wgrad:0", EV_WG[0], "read:0", EV_WG[0],
                                   "bn:1", "bn:1", "bn:1", "write:1"]
    fills = {i: list(cc.arr[i].slots[:3]) for i in range(cc.n) if cc.names[i].startswith("yh_fill_u32 [bn")}
    assert fills == {1: [0x4000, 0, 64], 10: [0x5000, 0, 48], 11: [0x6000, 0, 80]}
    assert all(cc.py[i][2][:3] == ('yh_fill_u32', 0, 0.0) and cc.arr[i].stream == 0 for i in fills)
    for ci, _lo, _hi in buckets:            # the same positions, from the lowering of the commands in front of the bucket
        assert breaks[[b[0] for b in buckets].index(ci)] == _lower(L, cmds[:ci], frozen=True, ngz=1)[0].n
    # serial: the same breaks minus the event entries in front of them
    assert _lower(L, cmds, two=False, buckets=buckets, frozen=True)[1] == [2, 5, 8, 9]


@pytest.mark.parametrize("two", [True, False])
def test_head_patches(two):
    """one patch per launch of a head (plain) layer: the column sum's slot 0, the weight-gradient descriptor's gy, the
    data-gradient descriptor's seg[0].ptr; the setter reaches the array slot and the argument of the per-launch call alike"""
    L = lib()
    cmds, want = [], []
    for h in range(3):
        op, wd, d = _op(f"head{h}", 'plain'), WgradDesc(), ConvDesc()
        cmds += [('head_colsum', op, 64 * h, ('yh_colsum', 0, 1.0)), ('wg_begin', None, None, SYNC), ('wgrad', op, wd, ('wg', 1.0, 1.0)),
                 ('wg_end', None, None, SYNC), ('dgrad', op, d, ('dg', 1.0, 1.0))]
        want += [('colsum', None), ('wgrad', wd), ('dgrad', d)]
    cmds += _layers(L, 2, 3)[0]
    cc, _, patches = _lower(L, cmds, two=two)
    assert len(patches) == len(want) and all(p[0] == k and p[1] is o for p, (k, o) in zip(patches, want))
    assert [n for _k, _o, n, _i in patches] == [f"head{h}" for h in range(3) for _ in range(3)]
    for h, (kind, _obj, name, i) in enumerate(patches[::3]):
        c = cc.arr[i]
        assert cc.names[i] == f"yh_colsum [head{h}]" and c.stream == (1 if two else 0)
        assert list(c.slots[:c.nslots]) == [0, 16, 16, 32, 0x7000, 0x8000 + 256 * h, 0]
        assert cc.py[i][2] == ('yh_colsum', 0, 1.0, f"head{h}")
        cc.set_arg(i, 0, 0xABC000 + h)
        assert c.slots[0] == 0xABC000 + h == cc.py[i][1][0] and cc.py[i][1][1:] == [16, 16, 32, 0x7000, 0x8000 + 256 * h]
    ent = _entries(cc)
    assert ('call', 1 if two else 0, "head1") in ent and sum(1 for e in ent if e[0] != 'call') == (0 if not two else 2 * 3 + 2 * 2 + 2)
