"""Program: the pre-built kernel launches of one (batch, input shape) — forward (engine.forward), backward (engine.backward), tuning (engine.tune)."""
import torch

from .._lib import lib
from .backward import BackwardMixin
from .forward import ForwardMixin
from .tune import TunerMixin


class Program(ForwardMixin, BackwardMixin, TunerMixin):
    """Pre-built kernel launches for one (batch, input shape)."""

    def __init__(self, builder, pack, B, outputs, bn_eps_of=None):
        self.B, self.pack = B, pack
        self.ops, self.bufs = builder.ops, builder.bufs
        self.outputs = outputs          # list of ConvOp (plain) or Ref whose buffers are returned
        dev = pack.device
        self.dev = dev
        self.L = lib()
        for b in self.bufs:
            # raw conv outputs (".y") are training-only and allocated by _build_train(); head buffers are fresh per forward
            if not b.name.endswith(".y") and not getattr(b, "is_head", False):
                b.t = torch.zeros(B, b.H, b.W, b.C, dtype=torch.bfloat16, device=dev)
        self.generation = 0
        self.profile = None             # {(kernel family, algorithmic flops): [(start_event, end_event)]} when profiling
        # the lowered passes, behind both runners (yh_exec replay / one call per launch):
        # 'train' | 'frozen' | 'eval' -> CompiledCmds;  ('bwd', two_streams, hooked, frozen) -> (CompiledCmds, breaks, patches)
        self._compiled = {}
        self.bwd_ready = False
        self._keep = []                 # keeps ctypes structs / tensors alive
        self._owned = None              # (state the count was taken in, bytes): owned_bytes()
        self._build_forward()

    def owned_bytes(self):
        """Bytes of device memory that live as long as this program does: activation, gradient and workspace buffers of every
        stage built so far (the training program and the backward allocate theirs at first use, so the figure grows until the
        program has run each once).  Not counted: the shared ParamPack and the model's own tensors, which survive the program, and
        the head tensors, which are fresh at every forward and belong to the caller.  Buffers that alias one storage count once."""
        # the walk is repeated when a stage that allocates has run since the last count: the training program (cmd_train), the
        # backward (bwd_ready, and its descriptors in _keep), a compiled command list, the shared weight-gradient workspace (wg_ws,
        # re-allocated when a launch needs more).  A new allocation site must show up in this tuple
        state = (getattr(self, "cmd_train", None) is not None, self.bwd_ready, len(self._keep), len(self._compiled),
                 id(getattr(self, "wg_ws", None)))
        if self._owned is None or self._owned[0] != state:
            self._owned = (state, _tensor_bytes(self, skip=(self.pack,)))
        return self._owned[1]


def _tensor_bytes(root, skip=()):
    """bytes of the distinct CUDA storages reachable from `root` through containers and the engine's own objects"""
    seen_obj, storages = {id(o) for o in skip}, {}
    stack = [root]
    while stack:
        o = stack.pop()
        if id(o) in seen_obj:
            continue
        seen_obj.add(id(o))
        if isinstance(o, torch.Tensor):
            if o.is_cuda and not isinstance(o, torch.nn.Parameter):
                st = o.untyped_storage()
                storages[st.data_ptr()] = st.nbytes()
        elif isinstance(o, dict):
            stack.extend(o.values())
        elif isinstance(o, (list, tuple, set)):
            stack.extend(o)
        elif type(o).__module__.startswith(__package__) and hasattr(o, "__dict__"):
            head = bool(getattr(o, "is_head", False))
            stack.extend(v for k, v in vars(o).items() if not (head and k == "t"))
    return sum(storages.values())
