"""Executor: a pass of the engine lowered once to a yh_cmd array (include/yolohip.h) and run either by one yh_exec call per segment
(run) or by one ctypes call per launch from the same array (run_each: YH_EXEC=0, profiling)."""
import ctypes as C
import struct

import torch

from .._lib import Cmd, YH_CMD_EVENT_RECORD, YH_CMD_SLOTS, YoloHipError, check


def _slot(v):
    """a command argument widened to the 8-byte slot yh_exec expects"""
    if v is None:
        return 0
    if isinstance(v, float):
        return struct.unpack("<Q", struct.pack("<d", v))[0]
    if isinstance(v, (C.Structure, C.Array)):
        return C.addressof(v)
    return int(v) & 0xFFFFFFFFFFFFFFFF


class CompiledCmds:
    """a command list as a yh_cmd array (include/yolohip.h): built once per program.  `py` holds, per entry, what a launch from
    Python needs: (ctypes function, argument list, profile key) of a call, the event (a torch.cuda.Event; any token whose integer
    value is the handle will do where nothing is run) of an event entry."""

    def __init__(self, L, capacity):
        self.L = L
        self.arr = (Cmd * max(capacity, 1))()
        self.n = 0
        self.names = []
        self.py = []
        self.source = None              # the Python command list this array was compiled from

    def call(self, fn, args, stream=0, label="", meta=None):
        nargs = C.c_int32(0)
        op = self.L.yh_exec_op(fn.__name__.encode(), C.byref(nargs))
        if op < 0 or nargs.value != len(args) + 1 or nargs.value > YH_CMD_SLOTS:
            raise YoloHipError(f"{fn.__name__} [{label}] cannot be compiled into a program ({len(args)} arguments)")
        c = self.arr[self.n]
        c.op, c.nslots, c.stream = op, nargs.value, stream
        for i, v in enumerate(args):
            c.slots[i] = _slot(v)
        self.names.append(f"{fn.__name__} [{label}]")
        self.py.append((fn, list(args), None if meta is None else tuple(meta) + (label,)))
        self.n += 1
        return self.n - 1

    def event(self, kind, ev, stream):
        c = self.arr[self.n]
        c.op, c.nslots, c.stream = kind, 1, stream
        c.slots[0] = int(getattr(ev, "cuda_event", ev))
        self.names.append("event record" if kind == YH_CMD_EVENT_RECORD else "stream wait")
        self.py.append(ev)
        self.n += 1

    def set_arg(self, i, k, v):
        """argument k of call i, for both runners"""
        self.arr[i].slots[k] = _slot(v)
        self.py[i][1][k] = v

    def run(self, streams, lo=0, hi=None):
        """entries lo..hi by one yh_exec call; streams: raw handles"""
        hi = self.n if hi is None else hi
        if hi <= lo:
            return
        failed = C.c_int32(-1)
        arr = (C.c_void_p * len(streams))(*streams)
        rc = self.L.yh_exec(C.cast(C.byref(self.arr, lo * C.sizeof(Cmd)), C.POINTER(Cmd)), hi - lo, arr, len(streams), C.byref(failed))
        if rc != 0:
            check(rc, self.names[lo + failed.value] if failed.value >= 0 else "yh_exec")

    def run_each(self, streams, lo=0, hi=None, prof=None):
        """entries lo..hi one by one from Python; streams: torch streams.  prof: {profile key: [(start, end)]} gets a timing event
        pair around every call, recorded on the stream the call goes to"""
        raw = [C.c_void_p(s.cuda_stream) for s in streams]
        for i in range(lo, self.n if hi is None else hi):
            c, rec = self.arr[i], self.py[i]
            if c.op < 0:
                if c.op == YH_CMD_EVENT_RECORD:
                    rec.record(streams[c.stream])
                else:
                    streams[c.stream].wait_event(rec)
                continue
            fn, args, key = rec
            if prof is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(streams[c.stream])
            rc = fn(*args, raw[c.stream])
            if rc != 0:
                check(rc, self.names[i])
            if prof is not None:
                e1.record(streams[c.stream])
                prof.setdefault(key, []).append((e0, e1))
