"""Program, backward side: the backward program (BatchNorm+SiLU backward, fused reductions, data / weight gradients, the
gz ring and the weight-gradient stream), its compiled form, gradient buckets for the data-parallel exchange."""
import ctypes as C
import os

import numpy as np
import torch

from .. import hipk
from .._lib import (BnPart, ConvDesc, YH_BN_MAX_PARTS, WgradDesc, YH_CMD_EVENT_RECORD, YH_CMD_STREAM_WAIT, YH_ACT_NONE, YH_CONV_DGRAD,
                    YoloHipError)
from ..hipk import Slice
from ..streams import side_stream
from . import flags as _flags
from .executor import CompiledCmds
from .graph import ConvOp, PoolOp, Ref, _rup, plan_grad_buckets, sppf_chain
from .tune import _tune_cache_save


class BackwardMixin:

    def _head_on_side(self, op, two):
        """does a head layer's bias gradient (column sums of the head gradient) run on the weight-gradient stream?  Only with a
        scratch of its own: `part_scratch` belongs to the main stream's BatchNorm reductions (a layer wider than `head_scratch` was
        sized for — it is sized from the widest plain op of the graph, so none today — falls back to the main stream, never to a
        shared buffer on another stream)"""
        return bool(two and _flags.HEAD_COLSUM_SIDE and op.y.C * 1024 * 2 <= self.head_scratch.numel())

    def _head_scratch(self, op, two):
        """partial-sum scratch of a head layer's bias gradient: its own buffer when the column sums run on the side stream"""
        return self.head_scratch.data_ptr() if self._head_on_side(op, two) else self.part_scratch.data_ptr()

    def _is_fused_stem(self, op):
        """a ConvBnAct without a data gradient (the stem) whose BatchNorm backward apply runs inside its weight gradient (YH_FUSE_STEM_BWD)"""
        if not isinstance(op, ConvOp) or op.kind != 'cba':
            return False
        Kseg0 = op.k * op.k * op.segs[0].C
        return bool(_flags.FUSE_STEM_BWD and len(op.parts) == 1 and len(op.segs) == 1 and op.res is None and
                    not op.segs[0].buf.needs_grad and op.N % 8 == 0 and
                    ((op.N <= 32 and Kseg0 <= 256) or (op.N > 32 and 128 < Kseg0 <= 256)) and
                    (_flags.FUSE_STEM_BWD >= 2 or (self.wg_ws is None and self._stem_patch_ok(op))))

    def _wgrad_desc(self, op, sg, coff_k, gy, ldg, N, bn=None, dw=None):
        """yh_wgrad_desc of input segment sg of op.  bn = (ws, gamma, coef) pointers: gy is the gradient of the activation and the
        BatchNorm backward apply runs inside the launch (the fused stem)"""
        wd = WgradDesc()
        wd.gy, wd.ldg, wd.N = gy, ldg, N
        if bn:
            wd.bn_z, wd.bn_ldz = op.y.t.data_ptr(), op.y.C
            wd.bn_ws, wd.bn_gamma, wd.bn_coef = bn
        wd.seg = hipk.make_seg(sg.sl())
        wd.coff_k, wd.Ctot = coff_k, op.Ctot
        wd.B, wd.Ho, wd.Wo, wd.Hi, wd.Wi = self.B, op.Ho, op.Wo, op.Hi, op.Wi
        wd.KH = wd.KW = op.k
        wd.stride, wd.pad = op.stride, op.pad
        wd.dw = dw
        if self.wg_ws is not None:
            wd.partial, wd.partial_bytes = self.wg_ws.data_ptr(), self.wg_ws.numel() * 4
        return wd

    def _stem_patch_ok(self, op):
        """does the patch form of the weight gradient (conv_wgpf_kernel) take this layer with the fused BatchNorm backward?"""
        z = op.y.t.data_ptr()          # placeholder operands: eligibility only looks at null / alignment
        wd = self._wgrad_desc(op, op.segs[0], 0, z, op.N, op.N, bn=(z, z, z))
        wd.tile_k = 40
        return bool(self.L.yh_conv_wgrad_patch_ok(C.byref(wd)))

    # -- backward --------------------------------------------------------------------------
    def _build_backward(self):
        B, pk, L = self.B, self.pack, self.L
        cmds = []
        self._wgrad_on_main = set()      # ids of the weight-gradient descriptors that stay on the main stream
        max_gy = 0
        for b in self.bufs:
            b.ginit = np.zeros(b.C, dtype=bool)
            if b.needs_grad and b.g is None and not b.name.endswith(".y") and not getattr(b, "is_head", False):
                b.g = torch.zeros(B, b.H, b.W, b.C, dtype=torch.bfloat16, device=self.dev)
        for op in self.ops:
            if isinstance(op, ConvOp) and op.kind == 'cba':
                max_gy = max(max_gy, B * op.Ho * op.Wo * op.N)
        self.gy_scratch = torch.zeros(max(max_gy, 8), dtype=torch.bfloat16, device=self.dev)
        # the weight gradients run on a side stream next to the data-gradient / BatchNorm chain (they only share the
        # layer's gz): consecutive layers alternate between two gz buffers so that a layer's wgrad may still be
        # reading its gz while the next layer's BN backward writes the other one
        self.two_streams = os.environ.get("YH_BWD_STREAMS", "1") != "0"
        NGZ = self.ngz = _flags.NGZ
        self.gy_ring = [self.gy_scratch] + ([torch.zeros(max(max_gy, 8), dtype=torch.bfloat16, device=self.dev) for _ in range(NGZ - 1)] if self.two_streams else [self.gy_scratch] * (NGZ - 1))
        n_cba = 0
        self.part_scratch = torch.zeros(1024 * 2 * 2048, dtype=torch.float32, device=self.dev)
        # partial sums of the head layers' bias gradients (column sums of the head gradients): these run on the SIDE stream (they feed
        # nothing but the packed gradient arena; the largest takes 76 us on YOLOv5s) and may not share a scratch with the main stream
        head_c = max([256] + [op.y.C for op in self.ops if isinstance(op, ConvOp) and op.kind == 'plain'])
        self.head_scratch = torch.zeros(1024 * 2 * head_c, dtype=torch.float32, device=self.dev)
        self.coef_scratch = {}
        self.ups_scratch = {}
        self.wgrad_tuned = {}
        # workspace of the weight gradients' split-M partial tiles (plain stores + a deterministic reduce instead of fp32
        # atomics; set_deterministic(False) / YH_WGRAD_PARTIAL=0: atomics).  One buffer serves every launch: they all run on one
        # stream, in order.  While the program is built the launches are timed against a buffer of the cap's size; the program
        # keeps one of the size its largest launch needs (below).
        self.bwd_deterministic = _flags.WG_WS_BYTES > 0
        self.wg_ws = torch.empty(_flags.WG_WS_BYTES // 4, dtype=torch.float32, device=self.dev) if _flags.WG_WS_BYTES > 0 else None
        wg_descs = []

        writes_seen = {}

        def claim(ref):
            """returns accumulate flag for a write into grad(ref) and marks it written"""
            k3 = (ref.buf.name, ref.coff, ref.C)
            writes_seen[k3] = writes_seen.get(k3, 0) + 1
            flags = ref.buf.ginit[ref.coff:ref.coff + ref.C]
            if flags.all():
                return 1
            if flags.any():
                raise YoloHipError(f"partial gradient overlap on {ref.buf.name}")
            flags[:] = True
            return 0

        def require(ref, who):
            if not ref.buf.ginit[ref.coff:ref.coff + ref.C].all():
                raise YoloHipError(f"{who}: gradient of {ref.buf.name}[{ref.coff}:{ref.coff + ref.C}] is never produced")

        # head outputs receive their gradient from the caller
        for o in self.outputs:
            if isinstance(o, ConvOp):
                o.y.ginit[:] = True
            else:
                o.buf.ginit[o.coff:o.coff + o.C] = True

        # Which ConvBnAct outputs get the LAST contribution to their gradient from a data-gradient launch (a conv reads exactly
        # that slice, not upsampled; residual adds / pools / other convs that read it come later in the forward, so their
        # gradient is already in the buffer)?  For those the BatchNorm-backward reduction is taken in that dgrad's epilogue
        # (yh_conv_desc.bnr_*, accumulating where it is not the only writer) and the separate reduce pass is dropped.
        fuse_ok = os.environ.get("YH_FUSE_BNR", "1") != "0"
        fuse_acc = os.environ.get("YH_FUSE_BNR_ACC", "1") != "0"     # ... also when that launch accumulates onto earlier writers
        uses, producer_of = {}, {}
        for o2 in self.ops:
            if isinstance(o2, PoolOp):
                uses.setdefault((o2.src.buf.name, o2.src.coff, o2.src.C), []).append(('pool',))
                continue
            for sg2 in o2.segs:
                uses.setdefault((sg2.buf.name, sg2.coff, sg2.C), []).append(('seg', sg2.ups))
            if o2.res is not None:
                uses.setdefault((o2.res.buf.name, o2.res.coff, o2.res.C), []).append(('res',))
            if o2.kind == 'cba':
                c0_ = 0
                for pi2, n2 in enumerate(o2.part_N):
                    r2 = o2.outs[pi2]
                    producer_of[(r2.buf.name, r2.coff, r2.C)] = (o2, pi2, c0_)
                    c0_ += n2
        for o2 in self.outputs:
            if not isinstance(o2, ConvOp):
                uses.setdefault((o2.buf.name, o2.coff, o2.C), []).append(('out',))

        def last_writer(key):
            """asked by a data-gradient launch that has just claimed `key` (a non-upsampled conv segment): was that the LAST write
            into this gradient slice — every other consumer (conv segments, residual adds, pools) comes later in the forward
            and so earlier in this program — with no differently-sliced use of the same buffer overlapping it?"""
            u = uses.get(key, [])
            if any(x[0] == 'out' for x in u) or writes_seen.get(key, 0) != len(u):
                return False
            return not any(k2[0] == key[0] and k2 != key and not (k2[1] + k2[2] <= key[1] or k2[1] >= key[1] + key[2]) for k2 in uses)
        self.bnr_fused = {}
        marks = []
        skip_bwd = set()
        nops = len(self.ops)
        for ri, op in enumerate(reversed(self.ops)):
            oi = nops - 1 - ri
            if oi in skip_bwd:
                continue
            if isinstance(op, PoolOp) and oi >= 2 and sppf_chain(self.ops, oi - 2, L):
                # the chain's backward in one launch; needs every pool's input gradient to exist already (cba2's data gradient wrote
                # all four slices of the concat buffer earlier in this program) — else the three single launches below
                p1, p2, p3 = self.ops[oi - 2:oi + 1]
                flags = lambda r: r.buf.ginit[r.coff:r.coff + r.C]        # noqa: E731
                if flags(p3.dst).all() and flags(p3.src).all() and flags(p2.src).all():
                    acc1 = claim(p1.src)
                    claim(p2.src); claim(p3.src)
                    g1, g2, g3, gx_ = p1.dst.sl(True), p2.dst.sl(True), p3.dst.sl(True), p1.src.sl(True)
                    Hs, Ws = p1.src.buf.H, p1.src.buf.W
                    cmds.append((L.yh_sppf_pool3_bwd, (g1.ptr(), g2.ptr(), g3.ptr(), g1.ld, p1.idx.data_ptr(), p2.idx.data_ptr(), p3.idx.data_ptr(),
                                                       B, Hs, Ws, g1.C, gx_.ptr(), gx_.ld, acc1), p1.name,
                                 ('yh_sppf_pool3_bwd', 0, (13.0 if acc1 else 11.0) * B * Hs * Ws * g1.C)))
                    skip_bwd.update((oi - 1, oi - 2))
                    continue
            if isinstance(op, PoolOp):
                require(op.dst, op.name)
                acc = claim(op.src)
                go, gi = op.dst.sl(True), op.src.sl(True)
                cmds.append((L.yh_maxpool5_bwd, (go.ptr(), go.ld, op.idx.data_ptr(), B, op.src.buf.H, op.src.buf.W, go.C,
                                                 gi.ptr(), gi.ld, acc), op.name, ('yh_maxpool5_bwd', 0, (7.0 if acc else 5.0) * B * op.src.buf.H * op.src.buf.W * go.C)))
                continue
            M = B * op.Ho * op.Wo
            st = self.op_state[op.name]
            gdw = pk.gpack.data_ptr() + 4 * pk.gloc[op.name]
            gys = self.gy_scratch
            if op.kind == 'cba':
                gys = self.gy_ring[n_cba % NGZ]
                cmds.append(('gz_begin', n_cba % NGZ, None, ('sync', 0, 0.0)))       # main stream: wait until this gz buffer's last wgrad is done
                n_cba += 1
            if op.kind == 'plain':
                # gradient arrives in op.y.g (set per call); bias grad = column sums
                st['gy_ref'] = 'head'
                gy_ptr_holder = st
                conv = op.parts[0][0]
                cmds.append(('head_colsum', op, pk.bias_g.get((op.name, 0)), ('yh_colsum', 0, 2.0 * M * op.y.C)))
                gy_ld, gyN = op.y.C, op.N
                gy_sl = None
            else:
                c0 = 0
                # a layer without a data gradient (the stem: its input is the image) hands gz to nobody but its own weight
                # gradient: that kernel forms gz from (ga, z) in its operand loader (yh_wgrad_desc.bn_*), the apply pass — the
                # last 0.2 ms of the backward's critical path on YOLOv5s — and the gz round trip through HBM disappear
                fused_stem = self._is_fused_stem(op)
                merged = (_flags.MERGE_PARTS and 2 <= len(op.parts) <= YH_BN_MAX_PARTS and
                          not (op.res is not None and op.res.buf.needs_grad))
                bwd_parts = (BnPart * len(op.parts))() if merged else None
                scratch_off = 0
                for pi, ((conv, bn), n) in enumerate(zip(op.parts, op.part_N)):
                    require(op.outs[pi], op.name)
                    ga = op.outs[pi].sl(True)
                    ws = st['ws'][pi]
                    coef = torch.zeros(2 * n, dtype=torch.float32, device=self.dev)
                    self.coef_scratch[(op.name, pi)] = coef
                    nblk = L.yh_ew_blocks(M)
                    ypart = op.y.t.data_ptr() + 2 * c0
                    part_ptr = self.part_scratch.data_ptr()
                    fused = self.bnr_fused.get((op.name, pi))
                    if fused is not None:          # the consumer's data gradient already left the partial sums in its own slab
                        part_ptr, nblk = fused[0].data_ptr(), fused[1]
                    else:
                        if bwd_parts is not None:  # the merged finalize reads every part's rows: they may not share the scratch slab
                            part_ptr += 4 * scratch_off
                            scratch_off += nblk * 2 * n
                            assert scratch_off <= self.part_scratch.numel()
                        cmds.append((L.yh_bn_silu_bwd_reduce, (ga.ptr(), ga.ld, ypart, op.y.C, ws.data_ptr(), n, M,
                                                               part_ptr), op.name, ('yh_bn_silu_bwd_reduce', 0, 4.0 * M * n)))
                    goff, boff = pk.bn_g[(op.name, pi)]
                    if bwd_parts is not None:
                        pa = bwd_parts[pi]
                        pa.slab, pa.nblk = part_ptr, nblk
                        pa.dgamma, pa.dbeta = pk.gpack.data_ptr() + 4 * goff, pk.gpack.data_ptr() + 4 * boff
                    else:
                        cmds.append((L.yh_bn_bwd_finalize, (part_ptr, nblk, n, M, ws.data_ptr(),
                                                            pk.gpack.data_ptr() + 4 * goff, pk.gpack.data_ptr() + 4 * boff,
                                                            coef.data_ptr()), op.name, ('yh_bn_bwd_finalize', 0, 8.0 * nblk * n)))
                    gres_ptr, gres_ld, gres_acc = None, 0, 0
                    if op.res is not None and pi == 0 and op.res.buf.needs_grad:
                        gres_acc = claim(op.res)
                        gr = op.res.sl(True)
                        gres_ptr, gres_ld = gr.ptr(), gr.ld
                    if bwd_parts is not None:
                        pa = bwd_parts[pi]
                        pa.ws, pa.C, pa.ga, pa.ldga = ws.data_ptr(), n, ga.ptr(), ga.ld
                        pa.gamma, pa.coef = bn.weight.data_ptr(), coef.data_ptr()
                    elif fused_stem:
                        st['fused_bwd'] = (ga, ws, bn, coef)
                    else:
                        cmds.append((L.yh_bn_silu_bwd_apply, (ga.ptr(), ga.ld, ypart, op.y.C, ws.data_ptr(), bn.weight.data_ptr(),
                                                              coef.data_ptr(), n, M, gys.data_ptr() + 2 * c0, op.N,
                                                              gres_ptr, gres_ld, gres_acc), op.name,
                                     ('yh_bn_silu_bwd_apply', 0, (6.0 + (4.0 if gres_acc else 2.0) * (gres_ptr is not None)) * M * n)))
                    c0 += n
                if bwd_parts is not None:          # the parts' reductions are done: one finalize, one pass writes gz of the whole stacked layer
                    self._keep.append(bwd_parts)
                    cmds.append((L.yh_bn_bwd_finalize_parts, (bwd_parts, len(op.parts), M), op.name,
                                 ('yh_bn_bwd_finalize', 0, 8.0 * sum(int(q.nblk) * int(q.C) for q in bwd_parts))))
                    cmds.append((L.yh_bn_silu_bwd_apply_parts, (op.y.t.data_ptr(), op.y.C, M, bwd_parts, len(op.parts), gys.data_ptr(), op.N),
                                 op.name, ('yh_bn_silu_bwd_apply_parts', 0, 6.0 * M * op.N)))
                gy_ld, gyN = op.N, op.N
            # wgrad per segment (side stream: starts when gz is ready).  The fused stem's weight gradient is the LAST link of the backward's
            # critical chain (it waits for the finalize behind the last data gradient): it stays on the main stream, beside the side
            # stream's last weight gradient instead of behind it
            on_main = op.kind == 'cba' and fused_stem
            if on_main:
                ga_, ws_, bn_, coef_ = st['fused_bwd']
                wg_args = (ga_.ptr(), ga_.ld, gyN, (ws_.data_ptr(), bn_.weight.data_ptr(), coef_.data_ptr()), gdw)
            else:
                wg_args = (gys.data_ptr() if op.kind == 'cba' else 0, gy_ld, gyN, None, gdw)
            coff_k = 0
            launches = []
            for si, sg in enumerate(op.segs):
                wd = self._wgrad_desc(op, sg, coff_k, *wg_args)
                ntile = L.yh_conv_wgrad_tiles(gyN, op.k * op.k * sg.C)
                kcols = op.k * op.k * (12 if op.focus else sg.C)
                nbytes_x = 2.0 * B * (op.Hi >> sg.ups) * (op.Wi >> sg.ups) * sg.C
                wd.splits = self._tune_wgrad_splits(wd, M, ntile, op)
                self._keep.append(wd)
                wg_descs.append(wd)
                if on_main:
                    self._wgrad_on_main.add(id(wd))
                launches.append((op, wd, (self._wgrad_name(L, wd), 2.0 * M * op.N * kcols,
                                          2.0 * M * gy_ld * (2 if wd.bn_z else 1) + nbytes_x)))
                coff_k += sg.C
            slot = (n_cba - 1) % NGZ if op.kind == 'cba' else None
            if not on_main:
                cmds.append(('wg_begin', None, None, ('sync', 0, 0.0)))
            for ln in launches:
                cmds.append(('wgrad',) + ln)
            if not on_main:
                cmds.append(('wg_end', [slot] if slot is not None else None, None, ('sync', 0, 0.0)))
            # every gradient of this op's parameters has been enqueued: its slice of the packed arena is final
            marks.append((len(cmds), pk.gloc[op.name]))
            # dgrad per segment
            for si, sg in enumerate(op.segs):
                if not sg.buf.needs_grad:
                    continue
                wp, cpad, Kd = pk.wptr((op.name, 'dgrad', si))
                Nk = _rup(op.N, 8)
                d = ConvDesc()
                d.seg[0].ptr = gys.data_ptr() if op.kind == 'cba' else 0
                d.seg[0].ld, d.seg[0].C, d.seg[0].ups = gy_ld, Nk, 0
                d.nseg, d.mode = 1, YH_CONV_DGRAD
                d.B, d.Ho, d.Wo, d.Hi, d.Wi = B, op.Hi, op.Wi, op.Ho, op.Wo
                d.KH = d.KW = op.k
                d.stride, d.pad = op.stride, op.pad
                d.w, d.N, d.Npad = wp, sg.C, cpad
                d.act = YH_ACT_NONE
                d.nsplit = sg.C
                if sg.ups:
                    tmp = torch.zeros(B, op.Hi, op.Wi, sg.C, dtype=torch.bfloat16, device=self.dev)
                    self.ups_scratch[(op.name, si)] = tmp
                    d.out0, d.ld0, d.accumulate = tmp.data_ptr(), sg.C, 0
                    acc = claim(Ref(sg.buf, sg.coff, sg.C))
                    gl = Slice(sg.buf.g, sg.coff, sg.C)
                    self._keep.append(d)
                    self._tune_conv(d, 'dgrad', op.name)
                    cmds.append(('dgrad', op, d, (self._kernel_name(d), 2.0 * M * op.N * op.k * op.k * sg.C, self._conv_bytes(d))))
                    cmds.append((L.yh_upsample2_bwd, (tmp.data_ptr(), sg.C, B, sg.buf.H, sg.buf.W, sg.C, gl.ptr(), gl.ld, acc), op.name,
                                 ('yh_upsample2_bwd', 0, (2.0 + (1.0 if acc else 0.5)) * B * op.Hi * op.Wi * sg.C)))
                else:
                    acc = claim(Ref(sg.buf, sg.coff, sg.C))
                    gl = Slice(sg.buf.g, sg.coff, sg.C)
                    d.out0, d.ld0, d.accumulate = gl.ptr(), gl.ld, acc
                    self._keep.append(d)
                    key = (sg.buf.name, sg.coff, sg.C)
                    def bnr_slab(po, ppi):
                        """size the fused reduction's slab for the grid d has now; its rows (0: d cannot take the fused reduction)"""
                        rows = self._conv_info(L, d).bnr_rows
                        if rows != self.bnr_fused.get((po.name, ppi), (None, 0))[1]:
                            slab = torch.zeros(rows * 2 * sg.C, dtype=torch.float32, device=self.dev)
                            d.bnr_part = slab.data_ptr()
                            self.bnr_fused[(po.name, ppi)] = (slab, rows)
                        return rows
                    if fuse_ok and key in producer_of and last_writer(key) and (acc == 0 or fuse_acc):
                        po, ppi, pc0 = producer_of[key]
                        if bnr_slab(po, ppi) > 0:
                            d.bnr_z, d.bnr_ldz = po.y.t.data_ptr() + 2 * pc0, po.y.C
                            d.bnr_ws, d.bnr_C = self.op_state[po.name]['ws'][ppi].data_ptr(), sg.C
                    self._tune_conv(d, 'dgrad', op.name)
                    if d.bnr_part:
                        bnr_slab(po, ppi)          # the tuned block cap may have changed the grid
                    cmds.append(('dgrad', op, d, (self._kernel_name(d), 2.0 * M * op.N * op.k * op.k * sg.C, self._conv_bytes(d))))
        if self.wg_ws is not None:       # the shared workspace: what the largest launch of the program needs
            need = max([int(L.yh_conv_wgrad_ws_bytes(C.byref(wd))) for wd in wg_descs] + [16])
            if need > self.wg_ws.numel() * 4:
                raise YoloHipError(f"weight-gradient workspace: a launch needs {need} bytes, the cap is {self.wg_ws.numel() * 4}")
            self.wg_ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=self.dev)
            for wd in wg_descs:
                wd.partial, wd.partial_bytes = self.wg_ws.data_ptr(), self.wg_ws.numel() * 4
        _flags.note_backward_built(self)
        self.cmd_bwd = cmds
        self.bwd_buckets = plan_grad_buckets(marks, pk.gsize, int(os.environ.get("YH_DP_BUCKETS", "4")))
        self.bwd_ready = True
        _tune_cache_save()

    def _bucket_ready(self, bucket_hook, bucket, main, side):
        """hand a finished gradient bucket to the data-parallel hook.  With the side stream, the bucket's weight gradients
        were enqueued THERE and its BatchNorm / bias gradients on the main stream: the hook is called in the side stream's
        context after it has been made to wait for the main stream's position, so the collective is ordered behind both
        without stalling the dgrad / BatchNorm chain."""
        part = self.pack.gpack[bucket[1]:bucket[2]]
        if side is None:
            return bucket_hook(part)
        self._ev_gz.record(main)
        side.wait_event(self._ev_gz)
        with torch.cuda.stream(side):
            return bucket_hook(part)

    def _compile_backward(self, two, buckets, frozen):
        """compile_backward of this program's command list, on its own events and head-gradient scratch"""
        if two:
            for ev in [self._ev_gz] + self._ev_wg:        # materialise the raw event handles
                ev.record(self._side)

        def colsum_args(op, boff):                        # (argument 0, the head gradient, arrives per call)
            return (0, op.y.C, op.y.C, self.B * op.Ho * op.Wo, self._head_scratch(op, two), self.pack.gpack.data_ptr() + 4 * boff)
        return compile_backward(self.L, self.cmd_bwd, two, buckets, frozen, self._ev_gz if two else None, self._ev_wg if two else (),
                                self._wgrad_on_main, lambda op: self._head_on_side(op, two), colsum_args)

    def backward(self, head_grads, bucket_hook=None, frozen=False, param_views=True):
        """head_grads: list of [B,h,w,ld] bf16 gradient buffers matching self.outputs (plain ops).
        bucket_hook(slice of the packed fp32 gradient arena) -> finisher or None: called as soon as a bucket of
        gradients is complete (data-parallel all-reduce overlapped with the remaining backward); finishers run
        before the gradients are scattered to parameter order.
        frozen: the backward of the evaluation-mode-BatchNorm forward.
        param_views=False: only the flat gradient is wanted (the flat-arena optimizer): the 177 per-parameter views — ~0.5 ms of
        host time between the last backward kernel and the optimizer's first — are not built."""
        if not self.bwd_ready:
            self._build_backward()
        buckets = self.bwd_buckets if bucket_hook is not None else []
        pk = self.pack
        hipk.fill_zero(pk.gpack)
        heads = {}
        for o, g in zip(self.outputs, head_grads):
            if isinstance(o, ConvOp):
                heads[o.name] = g
            else:
                o.buf.g[..., o.coff:o.coff + o.C].copy_(g)
        prof, two = self.profile, self.two_streams
        main, side = torch.cuda.current_stream(), None
        if two:
            if getattr(self, "_side", None) is None:
                # a stream PROBED to run beside the compute stream (streams.py: a fresh stream may share its hardware queue)
                self._side = side_stream(self.dev)
                self._ev_gz = torch.cuda.Event()
                self._ev_wg = [torch.cuda.Event() for _ in range(self.ngz)]
                self._ev_all = torch.cuda.Event()
            side = self._side
            self._ev_gz.record(main)               # packed arena zeroed, head gradients in place
            side.wait_event(self._ev_gz)
        key = ('bwd', two, bucket_hook is not None, frozen)
        comp = self._compiled.get(key)
        if comp is None or comp[0].source is not self.cmd_bwd:
            comp = self._compiled[key] = self._compile_backward(two, buckets, frozen)
        cc, breaks, patches = comp
        for kind, obj, opname, i in patches:          # head gradients arrive per call
            ptr = heads[opname].data_ptr()
            if kind == 'wgrad':
                obj.gy = ptr
            elif kind == 'dgrad':
                obj.seg[0].ptr = ptr
            else:
                cc.set_arg(i, 0, ptr)
        streams = [main, side] if two else [main]
        if prof is None and _flags.USE_EXEC:
            # replay the compiled array (yh_exec): one call per bucket segment instead of one ctypes call per launch
            raw = [s.cuda_stream for s in streams]
            run = lambda lo, hi: cc.run(raw, lo, hi)                        # noqa: E731
        else:
            run = lambda lo, hi: cc.run_each(streams, lo, hi, prof)         # noqa: E731
        lo, finishers = 0, []
        for pos, bucket in zip(breaks, buckets):
            run(lo, pos)
            lo = pos
            finishers.append(self._bucket_ready(bucket_hook, bucket, main, side))
        run(lo, cc.n)
        if two:
            self._ev_all.record(side)
            main.wait_event(self._ev_all)
        for f in finishers:
            if f is not None:
                f()
        return pk.grads_to_params(param_views)


def compile_backward(L, cmds, two, buckets, frozen, ev_gz, ev_wg, on_main, head_on_side, colsum_args):
    """The backward command list `cmds` lowered to a yh_cmd array: kernels on stream 0 (main) / 1 (side: weight gradients, head bias
    gradients), the event records and stream waits of the gz ring in between.  The ONE place that decides streams and
    synchronisation; both runners of the array (CompiledCmds.run / run_each) follow it.
    two: the side stream is used (else everything on stream 0, no event entry).  buckets: [(command index, lo, hi)] (plan_grad_buckets).
    frozen: the backward of the evaluation-mode-BatchNorm forward — the same launches, with the batch-mean coefficients every
    yh_bn_bwd_finalize leaves for the apply pass zeroed right behind it (gz = gamma * invstd * dz).
    ev_gz, ev_wg: the event of "gz is ready" and one event per gz buffer (torch.cuda.Events whose handles exist, or bare handles).
    on_main: ids of the weight-gradient descriptors that stay on the main stream.  head_on_side(op): does a head layer's bias
    gradient run on the side stream?  colsum_args(op, offset of the bias gradient): its yh_colsum arguments.
    Returns (array, array positions at which a gradient bucket is complete: the first entry of the bucket's command, per-call
    patches for the head gradients: (kind, descriptor, op name, entry))."""
    cc = CompiledCmds(L, (2 + (YH_BN_MAX_PARTS if frozen else 0)) * len(cmds) + 8)      # at most: two events, or a finalize and its fills
    cc.source = cmds
    breaks, patches = [], []
    pending = {}                      # gz buffer -> index of the event its last weight-gradient launch recorded
    nb = 0
    for ci, cmd in enumerate(cmds):
        while nb < len(buckets) and buckets[nb][0] == ci:
            breaks.append(cc.n)
            nb += 1
        fn, meta = cmd[0], cmd[3]
        if fn == 'gz_begin':          # main stream: wait until this gz buffer's last weight gradient is done
            e = pending.get(cmd[1])
            if two and e is not None:
                cc.event(YH_CMD_STREAM_WAIT, ev_wg[e], 0)
                pending = {s: q for s, q in pending.items() if q != e}
        elif fn == 'wg_begin':
            if two:
                cc.event(YH_CMD_EVENT_RECORD, ev_gz, 0)
                cc.event(YH_CMD_STREAM_WAIT, ev_gz, 1)
        elif fn == 'wg_end':
            if two and cmd[1]:
                cc.event(YH_CMD_EVENT_RECORD, ev_wg[cmd[1][0]], 1)
                for slot in cmd[1]:
                    pending[slot] = cmd[1][0]
        elif fn == 'head_colsum':
            _, op, boff, _m = cmd
            if boff is not None:
                i = cc.call(L.yh_colsum, colsum_args(op, boff), 1 if two and head_on_side(op) else 0, op.name, meta)
                patches.append(('colsum', None, op.name, i))
        elif fn == 'wgrad':
            _, op, wd, _m = cmd
            if "wgrad" in _flags.ABL_SKIP:
                continue
            cc.call(L.yh_conv_wgrad, (wd,), 1 if two and id(wd) not in on_main else 0, op.name, meta)
            if op.kind == 'plain':
                patches.append(('wgrad', wd, op.name, -1))
        elif fn == 'dgrad':
            _, op, d, _m = cmd
            cc.call(L.yh_conv_igemm, (d,), 0, op.name, meta)
            if op.kind == 'plain':
                patches.append(('dgrad', d, op.name, -1))
        else:
            _, args, name, _m = cmd
            if fn.__name__ in _flags.ABL_SKIP:
                continue
            cc.call(fn, args, 0, name, meta)
            if frozen and fn is L.yh_bn_bwd_finalize:
                cc.call(L.yh_fill_u32, (args[7], 0, 2 * args[2]), 0, name, ('yh_fill_u32', 0, 0.0))
            elif frozen and fn is L.yh_bn_bwd_finalize_parts:
                for q in args[0][:args[1]]:
                    cc.call(L.yh_fill_u32, (q.coef, 0, 2 * int(q.C)), 0, name, ('yh_fill_u32', 0, 0.0))
    breaks += [cc.n] * (len(buckets) - nb)
    return cc, breaks, patches
