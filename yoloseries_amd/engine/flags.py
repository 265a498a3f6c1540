"""Environment switches of the engine: read once at import into the attributes of this module; the engine reads every switch as
`flags.X` at the point of use, so a test or tool that patches an attribute here changes the next program that is built."""
import os

BN_EPS_DEFAULT = 1e-3

TUNE_ITERS = max(1, int(os.environ.get("YH_TUNE_ITERS", "3")))   # launches timed per candidate (tools/make_tune_defaults.sh: 12)
MERGE_PARTS = os.environ.get("YH_MERGE_PARTS", "1") != "0"   # stacked ConvBnAct layers: one BN+SiLU pass for all parts
# Deterministic weight gradients (yoloseries_amd.set_deterministic(True), or YH_WGRAD_PARTIAL=1 at import): the weight gradients'
# partial tiles go to a workspace with plain stores and are summed in a fixed order by a second kernel (yh_wgrad_desc.partial)
# instead of fp32 atomics: BIT-REPRODUCIBLE gradients.  Every kernel family but the patch form and the fused stem backward has
# a workspace form: conv_wgs_kernel (tile_k 129) keeps its stream-K schedule and writes one 64 KB slot per (workgroup, tile) pair,
# conv_wgrad_kernel its split-M tiles; the engine times them against each other per layer as in the default mode.  The atomic
# form stays the default.  NOT MEASURED YET on this kernel family (the 4 % / 1.6 % figures earlier revisions quoted here belonged
# to conv_wgrad_kernel's workspace form alone): DESIGN §5 lists the three measurements that are owed.
# WG_WS_BYTES > 0 switches the mode on for the programs built afterwards and caps the ONE workspace every launch of a program
# shares (they run on one stream, in order); the program allocates what its largest launch needs, not the cap.
# YH_FUSE_STEM_BWD: the BatchNorm backward apply of a layer without a data gradient (the stem) runs inside its weight gradient's
# operand staging (yh_wgrad_desc.bn_*; the staged gz is the apply pass's gz bit for bit, tests/test_gpu_conv.py): the last pass of
# the backward's critical path and the gz round trip through HBM disappear.  1 (default): where the patch form of the weight
# gradient takes the layer (conv_wgpf_kernel: <= 64 output channels) — measured on the YOLOv5s step 12.70 -> 12.58..12.64 ms (+0.8 %,
# profiles/r03_step_experiments.txt m); 2: also through the im2col form (conv_wgrad_kernel<..., FBN>: 0.55 ms against 0.22 + 0.25 —
# the sigmoid of 210 M elements is hidden behind HBM time in a streaming pass but not between the barriers of a 15-wave-per-CU GEMM;
# the step gets 1 % slower); 0: never.
FUSE_STEM_BWD = int(os.environ.get("YH_FUSE_STEM_BWD", "1"))
HEAD_COLSUM_SIDE = os.environ.get("YH_HEAD_COLSUM_SIDE", "1") != "0"    # bias gradients of the head layers on the weight-gradient stream
SPPF_FUSE = os.environ.get("YH_SPPF_FUSE", "1") != "0"      # FastSPP's three pools in one launch per direction (csrc/sppf.hip)
WG_WS_CAP = 256 << 20
WG_WS_BYTES = WG_WS_CAP if os.environ.get("YH_WGRAD_PARTIAL", "0") == "1" else 0
NGZ = int(os.environ.get("YH_GZ_RING", "3"))   # gz buffers the side-stream weight gradients may lag behind by
# YH_SKIP_ALGOS=<n>[,<n>]: leave these kernel families (yh_conv_desc.algo) out of the per-layer timing — A/B runs of a new family on
# one box (use a YH_TUNE_CACHE of its own and YH_TUNE_DEFAULTS=0 for the layers concerned)
SKIP_ALGOS = frozenset(x for x in os.environ.get("YH_SKIP_ALGOS", "").split(",") if x)

# YH_ABL_SKIP=<entry point>[,...|wgrad]: TIMING EXPERIMENTS ONLY (results are wrong) — the named launches are left out of the
# compiled programs (and so of both their runners), which gives the wall time a step would have if that family were free
# (profiles/r03_step_ablation.txt)
ABL_SKIP = frozenset(x for x in os.environ.get("YH_ABL_SKIP", "").split(",") if x)

# YH_EXEC=0: launch every entry of the compiled command array from Python (one ctypes call each) instead of replaying the array
# with one yh_exec call (csrc/exec.hip)
USE_EXEC = os.environ.get("YH_EXEC", "1") != "0"


# programs whose backward has been built (weak: a program dies with its model), for set_deterministic
import weakref  # noqa: E402

_BUILT = weakref.WeakSet()


def note_backward_built(prog):
    _BUILT.add(prog)


def set_deterministic(enabled):
    """Deterministic weight gradients on / off for every training program built from now on (see the comment at WG_WS_BYTES).
    A live program whose backward was built with the other setting is NOT left behind: it is marked stale and rebuilds its
    backward (descriptors, workspace, launch parameters) on its next backward pass.  A hipGraph captured from such a program
    keeps replaying the launches it recorded: choose the mode before capturing."""
    global WG_WS_BYTES
    enabled = bool(enabled)
    WG_WS_BYTES = WG_WS_CAP if enabled else 0
    for prog in list(_BUILT):
        if prog.bwd_ready and getattr(prog, "bwd_deterministic", enabled) != enabled:
            prog.bwd_ready = False
            for key in [k for k in prog._compiled if isinstance(k, tuple) and k and k[0] == 'bwd']:
                del prog._compiled[key]
