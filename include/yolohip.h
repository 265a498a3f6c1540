/*
 * yolohip.h — C ABI of libyolohip.so, the MI355X (gfx950) kernels behind the
 * yl-jiang/YOLOSeries detection hot path.
 *
 * The reference has no FFI layer of its own (it is pure PyTorch);
 * every entry point below replaces a Python op sequence of the reference, cited
 * as  file:line  relative to the reference tree.  The Python mirror in
 * yoloseries_amd/ binds these with ctypes.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer owned by the caller unless the name
 *    says host.  Kernels are only enqueued on `stream`; nothing here
 *    allocates, frees, synchronises or copies to the host, so every call is
 *    legal inside hipStreamBeginCapture.
 *  - Activations are NHWC bf16 (raw uint16 storage), `ld` = elements between
 *    consecutive pixels, so a channel slice of a wider buffer is (ptr+coff, ld).
 *    Channel counts and channel offsets of activation operands are multiples of 8
 *    (16-byte vector access).
 *  - Return value: 0 on success, negative yh_status otherwise;
 *    yh_last_error() gives a thread-local message.
 */
#ifndef YOLOHIP_H
#define YOLOHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* yh_stream;          /* hipStream_t */
typedef uint16_t yh_bf16;         /* raw bfloat16 bits */

enum yh_status {
    YH_OK = 0,
    YH_EINVAL = -1,               /* bad shape / alignment / null pointer */
    YH_ELAUNCH = -2,              /* hipLaunch reported an error */
    YH_EUNSUPPORTED = -3
};

const char* yh_last_error(void);
int yh_version(void);
/* number of compute units of the current device (for workspace sizing) */
int yh_device_cus(void);

/* ------------------------------------------------------------------------ *
 * Implicit-GEMM convolution (MFMA 32x32x16 bf16, fp32 accumulate)
 * replaces nn.Conv2d inside ConvBnAct / Detect:
 *   utils/layer_tools.py:82-94 (ConvBnAct), :454-470 (Detect),
 *   torch.cat / nn.Upsample in the neck: models/normal/yolov5s.py:101-114
 * ------------------------------------------------------------------------ */

/* One channel segment of the (virtually concatenated) conv input. */
typedef struct yh_seg {
    const yh_bf16* ptr;   /* first channel of this segment at pixel 0          */
    int32_t ld;           /* elements per pixel of the underlying buffer        */
    int32_t C;            /* channels in this segment (multiple of 8)           */
    int32_t ups;          /* 1: buffer is (H/2,W/2), read with nearest-2x upsample */
    int32_t _pad;
} yh_seg;

#define YH_CONV_FWD   0   /* hi = ho*stride - pad + kh                          */
#define YH_CONV_DGRAD 1   /* hi = (ho + pad - kh)/stride, only when divisible   */

#define YH_ACT_NONE 0
#define YH_ACT_SILU 1

typedef struct yh_conv_desc {
    yh_seg   seg[2];      /* input = concat(seg[0], seg[1]) along channels      */
    int32_t  nseg;
    int32_t  mode;        /* YH_CONV_FWD / YH_CONV_DGRAD                        */
    int32_t  B, Ho, Wo;   /* output pixel grid; rows M = B*Ho*Wo                */
    int32_t  Hi, Wi;      /* logical input grid (of the concatenated input)     */
    int32_t  KH, KW, stride, pad;
    const yh_bf16* w;     /* packed weights [Npad][KH*KW*Ctot], k = tap*Ctot+c  */
    int32_t  N;           /* real output channels                               */
    int32_t  Npad;        /* rows allocated in w (multiple of 128, zero filled) */
    /* epilogue: v = acc (+bias[n]); if scale: v = v*scale[n]+shift[n];
     *           act; out = v (+res) (+out if accumulate)                        */
    const float* bias;    /* [N] or NULL                                         */
    const float* scale;   /* [N] or NULL  (folded BN, inference)                 */
    const float* shift;   /* [N] or NULL                                         */
    int32_t  act;
    int32_t  accumulate;  /* 1: out += result (gradient accumulation)            */
    yh_bf16* out0; int32_t ld0;   /* columns [0,nsplit)  -> out0[m*ld0 + n]          */
    int32_t  nsplit;              /* multiple of 8; == N when a single destination   */
    yh_bf16* out1; int32_t ld1;   /* columns [nsplit,N)  -> out1[m*ld1 + n-nsplit]   */
    const yh_bf16* res; int32_t ldr;  /* residual added after act to out0 columns, or NULL */
    /* per-channel batch statistics of the stored (bf16-rounded) pre-activation,
     * as per-block partial sums: stats[(blk*2+0)*Npad + n] = sum, [(blk*2+1)*Npad+n] = sumsq,
     * blk in [0, yh_conv_stat_blocks()).  NULL: not collected.                   */
    float*   stats;
    /* launch tuning (0 = library default): output-channel tile width 32/64/128, channels per k-step and the cap on
     * persistent blocks along the pixel axis.  Results are identical for every setting except the number (and so the
     * summation grouping) of the statistics rows; yh_conv_stat_blocks() honours both.            */
    int32_t  tile_n;
    int32_t  grid_cap;
    int32_t  tile_k;      /* channels per k-step, 32 or 64 (64 needs whole 64-channel blocks in every segment but the last and the
                           * 128-wide tile on the register-staged kernel)                                               */
    int32_t  algo;        /* kernel family: 0 library default, 1 register-staged (conv_v2_kernel), 2..4 LDS-DMA ring
                           * (conv_v3_kernel) with a 256x128 / 128x128 / 128x64 tile, 5 the 3x3 halo kernel (conv_halo_kernel), 6 its
                           * 160-channel-wide variant (conv_halo160_kernel: N % 160 == 0, no statistics), when the shape is eligible;
                           * 7 the stride-2 data-gradient kernel (conv_dg2_kernel: DGRAD of a 3x3 / s2 / p1 layer with even output
                           * dims and gz channels in a multiple of 32: the four parity classes from one LDS patch of gz);
                           * 8 the 3x3 / stride-1 patch kernel for small channel counts (conv_p3_kernel: <= 128 channels in a multiple
                           * of 32 in, <= 128 out, forward with statistics or data gradient with the fused reduction);
                           * 9 the 80-channel halo kernel (conv_h80_kernel: 3x3 / s1 / p1 with exactly 80 input channels and N % 80 == 0,
                           * no statistics: 256-pixel x 80-channel tiles on 16x16x32 MFMAs, reduction over the flattened (tap, channel)
                           * index — no padding of N or K);
                           * 10 the pointwise kernel (conv_pw_kernel: 1x1 / s1 / p0 forward with exactly 80, 160 or 320 input channels and
                           * N % 80 == 0, no statistics: pixel tiles and the weight tile whole in LDS, no k loop over memory);
                           * (11: retired in round 5 — the wave-private forward kernel lost to tile quantisation on every BASELINE shape,
                           * profiles/r04_step_experiments.txt k);
                           * 12 the 80 -> 160 channel tap kernel (conv_c80_kernel: 3x3 / s1 or s2 / p1 forward with exactly 80 input and 160
                           * output channels, inference epilogue into one destination, no residual: 256 pixels x 160 channels per
                           * workgroup, one tap per stage — no padding of N or K; YOLOv5x's stage-1 downsampling layer);
                           * 13 the training pointwise kernel (conv_pt_kernel: 1x1 / s1 / p0, forward or data gradient, 128 or 256 input
                           * channels in one segment or in two equal halves (either may be upsampled), one destination; plain /
                           * statistics / generic / fused-reduction epilogues: 32-pixel tiles whole in LDS through a four-deep ring with
                           * counted waits, the 128 x C weight tile resident, no k loop over memory);
                           * 14 the LDS-DMA ring kernel with a 256 x 256 tile (8 waves of 128 x 64, two stages of 64 channels: half the
                           * staged bytes per MFMA of the 256 x 128 tile): N a multiple of 256, whole 64-channel blocks in every segment */
    /* DGRAD only — fused BatchNorm+SiLU backward reduction of the layer whose output gradient this launch writes
     * (it must be the LAST writer of that gradient: out0 covers exactly the producer's N channels; with `accumulate` the earlier
     * contributions already in out0 are added first and the sums are taken over the rounded total):
     * bnr_z = the producer's raw conv output (same pixel grid / channels as out0), bnr_ws = its scale | shift (stride bnr_C),
     * bnr_part = slab [yh_conv_bnr_rows()][2][N] receiving sum(dz), sum(dz*z) per block, dz = g * silu'(z*scale+shift).
     * Replaces yh_bn_silu_bwd_reduce for that layer; yh_bn_bwd_finalize consumes the slab.  NULL: off.          */
    const yh_bf16* bnr_z; int32_t bnr_ldz; int32_t bnr_C;
    const float* bnr_ws;
    float*   bnr_part;
} yh_conv_desc;
/* number of partial-sum rows the conv kernel writes for this shape: those of the launch yh_conv_igemm makes for the same
 * descriptor (an algo that is not eligible answers as algo 0 does, which is what then runs) */
int yh_conv_stat_blocks(const yh_conv_desc* d);
int yh_conv_igemm(const yh_conv_desc* d, yh_stream stream);
/* name of the kernel instantiation yh_conv_igemm launches for this descriptor ("conv_v2_kernel<128, 2, 2, 2, 1>"),
 * as rocprofv3 prints it: lets bench.py report per-kernel numbers that line up with the profiler's */
int yh_conv_kernel_name(const yh_conv_desc* d, char* buf, int buflen);
/* rows of the bnr_part slab for this data-gradient descriptor, as the launch yh_conv_igemm makes for the same descriptor writes
 * them; 0 = fused reduction not available for it */
int yh_conv_bnr_rows(const yh_conv_desc* d);
/* What yh_conv_igemm(d) will launch — family, rows of both slabs, instantiation — decided by the same plan: the three queries
 * above in one call, so the rows are those of the launch yh_conv_igemm makes for the same descriptor (where its algo is not
 * eligible: every field as with algo 0).  Needs no device and dereferences no operand.  Returns the rc yh_conv_igemm would return from its own argument
 * checks; `out` is filled from the dims alone whenever they are positive (as yh_conv_stat_blocks answers), also beside a non-zero
 * rc such as a null operand. */
enum { YH_CONV_FAM_GENERIC = 0, YH_CONV_FAM_V2, YH_CONV_FAM_V3, YH_CONV_FAM_HALO, YH_CONV_FAM_HALO160, YH_CONV_FAM_STEM,
       YH_CONV_FAM_DG2, YH_CONV_FAM_P3, YH_CONV_FAM_H80, YH_CONV_FAM_PW, YH_CONV_FAM_C80, YH_CONV_FAM_PT };
typedef struct yh_conv_plan_info {
    int32_t  family;                  /* YH_CONV_FAM_*: the kernel that runs (an algo that is not eligible falls back to the default) */
    int32_t  variant;                 /* conv_v3_kernel: its tile, 1 = 256x128, 2 = 128x128, 3 = 128x64, 4 = 256x256; else 0 */
    int32_t  tail;                    /* 1: the ragged-last-64-channel-block form of conv_v3_kernel / the halo kernels; siblings: 0 */
    int32_t  stat_rows;               /* yh_conv_stat_blocks(d) */
    int32_t  bnr_rows;                /* yh_conv_bnr_rows(d) */
    int32_t  reserved;
    char     name[96];                /* what yh_conv_kernel_name writes */
} yh_conv_plan_info;
int yh_conv_info(const yh_conv_desc* d, yh_conv_plan_info* out);

/* Weight gradient: dW[n][tap*Ctot + coff_k + c] += sum_m gy[m][n] * X[src(m,tap)][c]
 * (fp32 atomics into a zeroed packed buffer).  One launch per input segment.
 * replaces the autograd backward of nn.Conv2d (train_yolov5.py:337). */
typedef struct yh_wgrad_desc {
    const yh_bf16* gy; int32_t ldg;   /* [M][ldg] gradient of the conv output      */
    int32_t  N;                       /* output channels                            */
    yh_seg   seg;                     /* ONE input segment                          */
    int32_t  coff_k;                  /* channel offset of this segment inside Ctot */
    int32_t  Ctot;
    int32_t  B, Ho, Wo, Hi, Wi, KH, KW, stride, pad;
    float*   dw;                      /* [N][KH*KW*Ctot] fp32, accumulated          */
    int32_t  splits;                  /* split of the M (pixel) reduction, >=1      */
    int32_t  tile_k;                  /* launch tuning: 64 = 64-pixel k-steps on the wide 64-row tilings (0 / 32: default);
                                         128 = the general 128-column tiling also where KH*KW*C <= 384 (needs >= 128 columns);
                                         on the general tiling: 32 = 32-pixel k-steps (two blocks per CU), 35 = four waves of
                                         64 x 64 on 32-pixel k-steps; 40 = the patch form (conv_wgp_kernel: 3x3 layers with 16 / 32 /
                                         64 input channels and <= 64 outputs: the input patch of a pixel region staged once in LDS,
                                         persistent blocks, `splits` caps their number) where yh_conv_wgrad_patch_ok();
                                         129 = wave-private 128 x 128 tiles + stream-K (conv_wgs_kernel: input channels a multiple
                                         of 32, >= 64 outputs, B*Ho*Wo a multiple of 32; `splits` = workgroups, one per CU) where
                                         yh_conv_wgrad_wave_tiles() > 0 */
    /* optional workspace of >= yh_conv_wgrad_ws_bytes() bytes (16-byte aligned, caller-owned, may be shared by launches on ONE
     * stream): the split-M partial tiles are written there with plain stores and summed into dw by a second kernel in split
     * order — bit-reproducible, and faster than the fp32 atomics of the default form (NULL), which are bound by the atomic rate
     * of L2.  dw is read-modify-written by that kernel: launches that share dw columns must be stream-ordered.
     * The form of the launch decides the layout and yh_conv_wgrad_ws_bytes() answers for it: with tile_k 129 where
     * yh_conv_wgrad_wave_tiles() > 0, conv_wgs_kernel keeps its stream-K schedule and writes one 128 x 128 fp32 tile (64 KB) per
     * (workgroup, tile) pair into slot v + t (v: virtual workgroup, t: tile), G + T - 1 slots for G = min(splits, T * M / 32)
     * workgroups and T tiles; wgs_reduce_kernel then adds the slots of every tile to dw in ascending v (yh_conv_wgrad_wave_name()
     * reports conv_wgs_kernel<PW, true>).  As above: launches that share one workspace must run on ONE stream, and dw is
     * read-modify-written.  The patch form (tile_k 40) and the fused stem backward (bn_z) have no workspace form of their own:
     * with a workspace such launches go through conv_wgrad_kernel's.  A workspace that is too small or unaligned: YH_EINVAL,
     * nothing is launched. */
    float*   partial;
    uint64_t partial_bytes;
    /* Fused BatchNorm+SiLU backward for a layer WITHOUT a data gradient (the stem: its input is the image): with bn_z != NULL
     * `gy` is not gz but ga, the gradient w.r.t. the layer's ACTIVATION, and the kernel forms gz = gamma*invstd*(dz - c1 - xhat*c2),
     * dz = ga*silu'(z*scale+shift), in its operand loader — the arithmetic of yh_bn_silu_bwd_apply, rounded to bf16 exactly as that
     * pass stores it — so gz is never written or re-read (YOLOv5s stem at batch 64: 420 MB each way) and the pass disappears from
     * the end of the backward's critical path.  bn_z = raw conv output [M][bn_ldz], bn_ws = scale|shift|mean|invstd (stride N),
     * bn_gamma [N], bn_coef = mean(dz)|mean(dz*xhat) (yh_bn_bwd_finalize).  Layers with N <= 64 * ... tilings listed in
     * conv_wgrad.hip (wide tilings of up to 256 im2col columns); others return YH_EINVAL.                                      */
    const yh_bf16* bn_z; int32_t bn_ldz; int32_t reserved0;
    const float* bn_ws; const float* bn_gamma; const float* bn_coef;
} yh_wgrad_desc;
int yh_conv_wgrad(const yh_wgrad_desc* d, yh_stream stream);
size_t yh_conv_wgrad_ws_bytes(const yh_wgrad_desc* d);
int yh_conv_wgrad_patch_ok(const yh_wgrad_desc* d);
int yh_conv_wgrad_patch_name(const yh_wgrad_desc* d, char* buf, int buflen);   /* instantiation of the patch form, profiler spelling */
/* What yh_conv_wgrad(d) will launch, decided by the same plan.  Needs no device and dereferences no operand.  Returns the rc
 * yh_conv_wgrad would return from its own checks (the wave form's launcher adds operand checks of its own); `out` is filled from
 * the dims alone — as yh_conv_wgrad_ws_bytes answers — whenever B, Ho, Wo, N, C, KH, KW are positive, also beside a non-zero rc. */
typedef struct yh_wgrad_info {
    int32_t  form;                    /* 0 im2col (conv_wgrad_kernel), 1 patch (conv_wgp_kernel), 2 wave (conv_wgs_kernel) */
    int32_t  tiles;                   /* tiles of that form: yh_conv_wgrad_tiles2() / yh_conv_wgrad_wave_tiles() */
    int32_t  splits;                  /* im2col: splits that hold pixels after rounding to whole k-steps; else `splits` as given */
    int32_t  tile_k;                  /* the request in tile_k where it changed the launch, 0 where it was ignored */
    uint64_t ws_bytes;                /* yh_conv_wgrad_ws_bytes(d) */
    char     name[96];                /* the kernel instantiation, profiler spelling */
} yh_wgrad_info;
int yh_conv_wgrad_info(const yh_wgrad_desc* d, yh_wgrad_info* out);
/* number of (out-channel x im2col-column) tiles the kernel uses for a layer; callers size `splits` so that
 * tiles*splits is about one resident wave of blocks */
int yh_conv_wgrad_tiles(int N, int Kseg);
int yh_conv_wgrad_tiles2(int N, int Kseg, int tile_k);

/* ------------------------------------------------------------------------ *
 * BatchNorm (training statistics) + SiLU, forward and backward
 * replaces nn.BatchNorm2d(eps=1e-3, momentum=0.03) + nn.SiLU
 *   utils/layer_tools.py:87-91
 * ------------------------------------------------------------------------ */
/* reduce conv partial sums -> mean/invstd/scale/shift, update running stats.
 * ws layout (fp32, 4*C): scale | shift | mean | invstd                        */
int yh_bn_finalize(const float* stats, int nblk, int ldstat, int C, int64_t count,
                   const float* gamma, const float* beta,
                   float* running_mean, float* running_var, int64_t* num_batches,
                   float eps, float momentum, float* ws, yh_stream stream);
/* inference fold: scale = gamma/sqrt(rv+eps), shift = beta - rm*scale         */
int yh_bn_fold(const float* gamma, const float* beta, const float* rm, const float* rv,
               float eps, int C, float* scale, float* shift, yh_stream stream);
/* BatchNorm in evaluation mode inside a differentiable forward (nn.BatchNorm2d.eval() with autograd on): the workspace the
 * BN+SiLU passes read — scale | shift | mean | invstd, 4*C floats like yh_bn_finalize's — from the RUNNING statistics; the running
 * statistics are not updated.  The backward of such a layer is yh_bn_bwd_finalize with its `coef` output zeroed (no batch-mean
 * terms: gz = gamma * invstd * dz).  utils/layer_tools.py:90-91 under model.eval() */
int yh_bn_frozen(const float* gamma, const float* beta, const float* rm, const float* rv, float eps, int C, float* ws, yh_stream stream);
/* the same for every BatchNorm of a network in one launch: `items_dev` is a table of nitems entries in DEVICE memory
 * (the pointers inside it are device pointers; built once per program by the caller)                                 */
typedef struct yh_bn_fold_item {
    const float* gamma; const float* beta; const float* rm; const float* rv;
    float* scale; float* shift;
    float eps; int32_t C;
} yh_bn_fold_item;
int yh_bn_fold_batch(const yh_bn_fold_item* items_dev, int nitems, yh_stream stream);
/* out = silu(y*scale+shift) (+res) ; all bf16 NHWC slices                      */
int yh_bn_silu_apply(const yh_bf16* y, int ldy, const float* ws, int C, int64_t M,
                     yh_bf16* out, int ldo, const yh_bf16* res, int ldr, yh_stream stream);
/* pass 1 of the backward: partial sums of gz and gz*y per channel (gz = ga*silu'(bn(y)))
 * part layout: [nblk][2][C], nblk = yh_ew_blocks(M)                            */
int yh_ew_blocks(int64_t M);
int yh_bn_silu_bwd_reduce(const yh_bf16* ga, int ldga, const yh_bf16* y, int ldy,
                          const float* ws, int C, int64_t M, float* part, yh_stream stream);
/* combine partials (fp64): sum(gz*xhat) = invstd*(sum(gz*y) - mean*sum(gz)) with mean/invstd from ws
 * -> dgamma, dbeta and coefficients; coef layout (fp32, 2*C): mean(gz) | mean(gz*xhat) */
int yh_bn_bwd_finalize(const float* part, int nblk, int C, int64_t M, const float* ws,
                       float* dgamma, float* dbeta, float* coef, yh_stream stream);
/* pass 2: gy = gamma*invstd*(gz - c1 - xhat*c2); optional residual pass-through
 * gres (op)= ga                                                                */
int yh_bn_silu_bwd_apply(const yh_bf16* ga, int ldga, const yh_bf16* y, int ldy,
                         const float* ws, const float* gamma, const float* coef,
                         int C, int64_t M, yh_bf16* gy, int ldgy,
                         yh_bf16* gres, int ldgres, int gres_accumulate, yh_stream stream);
/* Stacked ConvBnAct layers — ONE convolution whose output channels belong to several BatchNorm + SiLU modules (C3 runs
 * cba1 and cba2 on the same input: utils/layer_tools.py:106-114, stacked into one GEMM here): the apply passes of all parts
 * as one launch over whole rows of y.  Part i covers the columns [C_0 + .. + C_{i-1}, + C_i) of y (and of gy in the backward).
 * The passes read: forward ws, C, out, ldo; backward ws, C, ga, ldga, gamma, coef (as in yh_bn_silu_bwd_apply).  No residual. */
#define YH_BN_MAX_PARTS 4
typedef struct yh_bn_part {
    float*         ws;       /* [4*C] scale | shift | mean | invstd of this part (written by the finalize, read by the passes) */
    int32_t        C;        /* channels of the part, multiple of 8                                            */
    int32_t        ldo;      /* forward pass: row pitch of out                                                 */
    yh_bf16*       out;      /* forward pass: activation of this part (its own tensor / slice)                 */
    const yh_bf16* ga;       /* backward pass: gradient w.r.t. this part's activation                          */
    int32_t        ldga;
    int32_t        nblk;     /* finalize: rows of `slab`                                                       */
    const float*   gamma;    /* BatchNorm weight of the part (forward finalize, backward pass)                 */
    float*         coef;     /* [2*C]: written by the backward finalize, read by the backward pass             */
    const float*   slab;     /* finalize: partial sums of THIS part — forward [nblk][2][ldslab] at its first channel
                                (yh_conv_desc.stats + channel offset), backward [nblk][2][C]                   */
    int32_t        ldslab;   /* forward finalize: row pitch of slab (Npad of the convolution)                  */
    float          eps;
    const float*   beta;     /* forward finalize */
    float*         running_mean;
    float*         running_var;
    int64_t*       num_batches;
    float          momentum;
    int32_t        _pad;
    float*         dgamma;   /* backward finalize */
    float*         dbeta;
} yh_bn_part;
/* yh_bn_finalize / yh_bn_bwd_finalize of every part in one launch (the kernels are latency bound: a launch per part costs the
 * same ~6 us as one for all) */
int yh_bn_finalize_parts(const yh_bn_part* parts, int nparts, int64_t count, yh_stream stream);
int yh_bn_bwd_finalize_parts(const yh_bn_part* parts, int nparts, int64_t M, yh_stream stream);
int yh_bn_silu_apply_parts(const yh_bf16* y, int ldy, int64_t M, const yh_bn_part* parts, int nparts, yh_stream stream);
int yh_bn_silu_bwd_apply_parts(const yh_bf16* y, int ldy, int64_t M, const yh_bn_part* parts, int nparts,
                               yh_bf16* gy, int ldgy, yh_stream stream);
/* column sums of a bf16 matrix (bias gradient of Detect): out[c] += sum_m g[m][c] */
int yh_colsum(const yh_bf16* g, int ldg, int C, int64_t M, float* part, float* out, yh_stream stream);

/* ------------------------------------------------------------------------ *
 * SPPF max-pool 5x5 s1 p2 (utils/layer_tools.py:270-288), NHWC bf16
 * idx: int8 per element, window position (0..24) of the first maximum
 * ------------------------------------------------------------------------ */
int yh_maxpool5_fwd(const yh_bf16* x, int ldx, int B, int H, int W, int C,
                    yh_bf16* out, int ldo, int8_t* idx, yh_stream stream);
int yh_maxpool5_bwd(const yh_bf16* gout, int ldgo, const int8_t* idx, int B, int H, int W, int C,
                    yh_bf16* gin, int ldgi, int accumulate, yh_stream stream);
/* FastSPP's chain x2 = mp(x), x3 = mp(x2), x4 = mp(x3) (utils/layer_tools.py:282-288) in one launch per direction for maps of
 * <= 1920 pixels (yh_sppf_pool3_ok; 20 x 20 at 640^2 input, 40 x 40 at 1280^2): the map of one image x 32 / 16 / 8 channels (maps of up to
 * 480 / 960 / 1920 pixels) lives in LDS, the pools run
 * separably.  Bit-identical to three yh_maxpool5_fwd / yh_maxpool5_bwd launches (arg-max rule, summation order, rounding points).
 * Backward: g1..g3 = gradients of x2..x4 as they stand before the pools' backward (ld ldg), gx (+)= the chain's gradient w.r.t. x;
 * the intermediate sums g(x3)', g(x2)' are not written back. */
int yh_sppf_pool3_ok(int H, int W, int C);
int yh_sppf_pool3_fwd(const yh_bf16* x, int ldx, int B, int H, int W, int C, yh_bf16* o1, yh_bf16* o2, yh_bf16* o3, int ldo,
                      int8_t* i1, int8_t* i2, int8_t* i3, yh_stream stream);
int yh_sppf_pool3_bwd(const yh_bf16* g1, const yh_bf16* g2, const yh_bf16* g3, int ldg, const int8_t* i1, const int8_t* i2, const int8_t* i3,
                      int B, int H, int W, int C, yh_bf16* gx, int ldx, int accumulate, yh_stream stream);
/* gradient of nearest-2x upsample: glo (op)= sum of the 2x2 block of ghi        */
int yh_upsample2_bwd(const yh_bf16* ghi, int ldh, int B, int Hlo, int Wlo, int C,
                     yh_bf16* glo, int ldl, int accumulate, yh_stream stream);
/* input image NCHW fp32 (B,3,H,W) -> space-to-depth NHWC bf16 (B,H/2,W/2,16):
 * channel = (dy*2+dx)*3 + c, channels 12..15 zero.  The 6x6/s2/p2 stem conv of
 * models/normal/yolov5s.py:16 becomes a 3x3/s1/p1 conv on this tensor.          */
int yh_input_s2d(const float* x, int B, int Cin, int H, int W, yh_bf16* out, yh_stream stream);
int yh_fill_u32(void* p, uint32_t v, int64_t n_words, yh_stream stream);
/* letterbox + normalisation of a batch of raw images (utils/data_aug.py:21-70 letter_resize_img and
 * dataset/data_collater.py normal_normalization of the reference, per image on the host there):
 *   out[b][c][y][x] = (float)v / 255.0f,  v = raw[img_off[b] + (rows[b][y] * src_w + cols[b][x]) * 3 + c],
 *   or v = fill_value where rows[b][y] or cols[b][x] is -1 (the letterbox border).
 * raw: the images HWC uint8, concatenated without padding (image b starts at byte img_off[b], any alignment);
 * src_hw[b] = {src_h, src_w}; rows [B][H] / cols [B][W] hold the source row / column of every output row / column.
 * The caller owns the validity of the tables (every entry -1 or inside its image).  W % 4 == 0, out and cols 16-byte
 * aligned, 0 <= fill_value <= 255.                                                                                  */
int yh_letterbox_batch(const uint8_t* raw, const int64_t* img_off, const int32_t* src_hw,
                       const int32_t* rows, const int32_t* cols,
                       int B, int H, int W, int fill_value, float* out /* (B,3,H,W) */, yh_stream stream);
/* bilinear resize of a batch, the arithmetic of torch's F.interpolate(mode='bilinear', align_corners=False) on the CPU bit for bit
 * (the multi-scale training of the reference, train_yolov5.py:526-544): per axis scale = float(n_in) / float(n_out),
 * src = max(fma(scale, d + 0.5, -0.5), 0), i0 = min(int(src), n_in-1), i1 = min(i0+1, n_in-1), l1 = src - i0, l0 = 1 - l1;
 * out = fma(a0, fma(A, b0, B*b1), a1 * fma(C, b0, D*b1)), a / b the row / column weights, A B | C D the taps of rows y0 | y1;
 * where Ho + Wo <= 128 torch runs another kernel, and so does this: out = fma(a1*b1, D, fma(a1*b0, C, fma(a0*b0, A, (a0*b1)*B))).
 * (torch's general kernel is itself not unique in the last place: with another thread count its own result can differ; the
 * form above is what it computes with its default threads on large batches, recorded in tests/golden/g16_multiscale.npz)
 * x (B,C,H,W) fp32 -> out (B,C,Ho,Wo) fp32, any sizes; out 16-byte aligned.                                                   */
int yh_resize_bilinear(const float* x, int B, int C, int H, int W, int Ho, int Wo, float* out, yh_stream stream);
/* the same samples written as the stem's input: x (B,Cin<=4,H,W) fp32 -> out (B,Ho/2,Wo/2,16) bf16 in yh_input_s2d's channel
 * order, zero padding and fp32 -> bf16 conversion; equal to yh_input_s2d(yh_resize_bilinear(x)) bit for bit with no fp32
 * intermediate in memory.  Ho and Wo even; out 16-byte aligned.                                                               */
int yh_resize_bilinear_s2d(const float* x, int B, int Cin, int H, int W, int Ho, int Wo, yh_bf16* out, yh_stream stream);
/* train-time augmentation of a batch of raw images (utils/data_aug.py: mosaic :579-671, RandomPerspective :482-576, RandomHSV
 * :363-389, RandomFlipLR/UD :434-478 of the reference, per image on the host there) as one gather per output pixel.  The canvas
 * that the reference pastes (up to) four images into is described, not built: */
typedef struct yh_aug_tile {      /* one pasted image of the (virtual) canvas */
    int64_t off;                  /* byte offset of the image in `raw` (HWC uint8, any alignment) */
    int32_t src_h, src_w;
    int32_t sx0, sy0;             /* source pixel shown at the rectangle's top-left corner */
    int32_t ox0, oy0, ox1, oy1;   /* paste rectangle in canvas pixels, half open; empty = unused tile */
} yh_aug_tile;
/* Output pixel (x, y) of image b samples the canvas at (u, v) = ((m0 x + m1 y + m2) / w, (m3 x + m4 y + m5) / w),
 * w = m6 x + m7 y + m8 (pixel i at coordinate i, OpenCV's convention), bilinearly in fp32 from the taps floor(u) + {0, 1},
 * floor(v) + {0, 1}.  A tap inside the canvas and inside a tile's rectangle is that tile's byte at
 * (sy0 + ty - oy0, sx0 + tx - ox0) (the highest tile index wins where rectangles overlap); every other tap is fill_value.
 * hsv_gain (NULL = off) multiplies hue / saturation / value of the blended pixel (float HSV on OpenCV's 8-bit scales); the
 * result / 255 is stored.  yoloseries_amd/csrc/augment.hip lists the operation order, utils/augment.py augment_batch_host is the
 * same computation in NumPy, bit for bit.
 * tiles [B][4], canvas_hw [B][2] = {h, w}, minv [B][9] row major, hsv_gain [B][3].  The caller owns the validity of the tables
 * (dataset/data_collater.py augment_collate_fn checks them): rectangles inside their canvas, source windows inside their images,
 * images inside raw, raw at least 3 bytes (a tap that shows the fill value reads bytes 0..2 and drops them).  Source indices are
 * clamped into [0, src_h) x [0, src_w) all the same.  W % 4 == 0, out 16-byte aligned, tiles 8-byte aligned,
 * 0 <= fill_value <= 255.                                                                                                  */
int yh_augment_batch(const uint8_t* raw, const yh_aug_tile* tiles /* [B][4] */, const int32_t* canvas_hw /* [B][2] */,
                     const float* minv /* [B][9] output pixel -> canvas, row major */, const float* hsv_gain /* [B][3]; NULL = off */,
                     int B, int H, int W, int fill_value, float* out /* (B,3,H,W) */, yh_stream stream);

/* ------------------------------------------------------------------------ *
 * Parameter arena: gather/scatter between the fp32 master parameters and the
 * packed bf16 weight images the conv kernels read.
 * ------------------------------------------------------------------------ */
/* dst_bf16[i] = idx[i] >= 0 ? bf16(src[idx[i]]) : 0                             */
int yh_pack_bf16(const float* src, const int32_t* idx, int64_t n, yh_bf16* dst, yh_stream stream);
/* dst[i] = idx[i] >= 0 ? src[idx[i]] : 0   (packed fp32 grads -> parameter layout) */
int yh_gather_f32(const float* src, const int32_t* idx, int64_t n, float* dst, yh_stream stream);
/* SGD with momentum/nesterov on a flat arena; group[i] selects lr/wd.
 * torch.optim.SGD semantics (train_yolov5.py:258-280):
 *   g += wd*p ; buf = first ? g : mom*buf + g ; g = nesterov ? g + mom*buf : buf ; p -= lr*g */
int yh_sgd_step(float* p, const float* g, float* buf, const uint8_t* group, int64_t n,
                const float* lr, const float* wd, int ngroups, float momentum, int nesterov,
                int first_step, const float* grad_scale, yh_stream stream);
/* the same step with every per-step scalar in DEVICE memory: scal[8] = lr[3] | wd[3] | momentum | first-step flag (!= 0).
 * No value of the step is a launch argument, so a captured hipGraph replays correctly while the host changes lr / momentum
 * between replays (warm-up, train_yolov5.py:437-456); at most 3 parameter groups. */
int yh_sgd_step_dev(float* p, const float* g, float* buf, const uint8_t* group, int64_t n,
                    const float* scal, int nesterov, const float* grad_scale, yh_stream stream);
/* Adam on a flat arena, torch.optim.Adam semantics (no amsgrad, L2 weight decay folded into the gradient), the second branch of
 * _init_optimizer (train_yolov5.py:258-280: optim.Adam(params, lr, betas=(momentum, 0.999)) on the same three groups):
 *   gv = g*grad_scale + wd[group]*p ; m += (1-beta1)*(gv-m) ; v = beta2*v + (1-beta2)*gv*gv ;
 *   p -= (lr[group]/bc1) * m / (sqrt(v)/sqrt(bc2) + eps),   bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, t = count of THIS step.
 * Every per-step scalar lives in DEVICE memory, in one block of 16 floats (8-byte aligned):
 *   blk[0..2] lr | blk[3..5] wd | blk[6] beta1 | blk[7] beta2 | blk[8] eps | blk[9] bc1 | blk[10] sqrt(bc2) | blk[11] reserved |
 *   blk[12..13] step count t as ONE int64 | blk[14..15] reserved.
 * The host writes blk[0..8] (and t, when it resumes); yh_adam_advance, in front of the step on the same stream, adds one to t and
 * writes blk[9] and blk[10], evaluated in double from the betas in the block.  No value of the step is a launch argument, so a
 * captured hipGraph replays correctly while the host changes lr between replays.  group: one byte per element, NULL = group 0,
 * bytes above 2 read group 2.  p, g, m, v: any float pointers; 16-byte loads / stores are used where all four share their phase
 * within 16 bytes (a scalar head and tail around them), the scalar loop otherwise.  grad_scale: device scalar of yh_clip_scale, or NULL. */
int yh_adam_advance(float* blk, yh_stream stream);
int yh_adam_step_dev(float* p, const float* g, float* m, float* v, const uint8_t* group, int64_t n,
                     const float* blk, const float* grad_scale, yh_stream stream);
/* EMA with the decay read from device memory (trainer/ema_model.py:20-28: the decay ramps with the update count) */
int yh_ema_update_dev(float* ema, const float* p, int64_t n, const float* decay_dev, yh_stream stream);
/* advance the device-resident EMA update counter by one and write the decay of this update,
 * decay = ratio * (1 - exp(-counter / tau)) evaluated in double (trainer/ema_model.py:12); then yh_ema_update_dev(.., decay, ..).
 * Keeps the whole train step free of host-computed scalars (hipGraph replay). */
int yh_ema_advance(int64_t* counter, float* decay, double ratio, double tau, yh_stream stream);
/* sum of squares of a flat fp32 buffer (for clip_grad_norm_, train_yolov5.py:344) */
int yh_sumsq(const float* x, int64_t n, float* part, float* out, yh_stream stream);
/* clip coefficient min(1, max_norm/(sqrt(sumsq)+1e-6)) as a device scalar for yh_sgd_step's grad_scale */
int yh_clip_scale(const float* sumsq, float max_norm, float* out, yh_stream stream);
/* EMA: e = d*e + (1-d)*p over a flat arena (trainer/ema_model.py:20-28)         */
int yh_ema_update(float* ema, const float* p, int64_t n, float decay, yh_stream stream);

/* ------------------------------------------------------------------------ *
 * YOLOv5 loss (loss/yolov5_loss.py:30-235)
 * ------------------------------------------------------------------------ */
typedef struct yh_v5loss_desc {
    int32_t B, maxbox, num_class, num_anchor, num_stage;
    int32_t H[4], W[4];           /* stage feature-map sizes                       */
    float   img_size0, img_size1; /* hyp['input_img_size'][0], [1]                */
    float   anchors[4][3][2];     /* pixels, anchors[stage][a] = (w,h)            */
    float   anchor_thr;           /* hyp['anchor_match_thr']                      */
    float   cls_smooth, cls_pos_weight, cof_pos_weight;
    int32_t use_focal; float focal_gamma, focal_alpha;
    float   iou_scale, cof_scale, cls_scale;
    int32_t pred_is_f32;          /* 0: bf16 predictions, 1: fp32                  */
    int32_t ldp[4];               /* elements per cell of each prediction buffer   */
    int32_t targets_xywhn;        /* 1: targets already hold (cx,cy,w,h)/img size — the argument
                                     convention of YOLOV5Loss.match (loss/yolov5_loss.py:142)   */
} yh_v5loss_desc;

/* workspace sizes in bytes */
size_t yh_v5loss_ws_bytes(const yh_v5loss_desc* d);
/* Target assignment for all stages (YOLOV5Loss.match, loss/yolov5_loss.py:142-214).
 * targets: [B][maxbox][6] fp32 (xmin,ymin,xmax,ymax,cls,img_id), padding rows -1.
 * Per stage s, with cap = 5*A*B*maxbox rows:
 *   count[s]                    int32
 *   tbox  [s][cap][4] fp32      (x-cx, y-cy, w, h) grid units
 *   tidx  [s][cap][5] int32     (cls, img, anchor, gy, gx)                       */
int yh_v5_assign(const yh_v5loss_desc* d, const float* targets,
                 int32_t* count, float* tbox, int32_t* tidx, void* ws, yh_stream stream);
/* Forward loss. preds[s]: [B][H][W][ldp] with channel a*(5+nc)+e.
 * balances: [num_stage] fp64 device state (python floats in the reference), updated in place.
 * result (fp32[8]): tot, iou, cof, cls, tar_nums, 0,0,0  (iou/cof/cls already x B)
 * saved: opaque per-call state for the backward, yh_v5loss_saved_bytes()         */
size_t yh_v5loss_saved_bytes(const yh_v5loss_desc* d);
int yh_v5_loss_fwd(const yh_v5loss_desc* d, const void* const* preds, const float* targets,
                   double* balances, float* result, void* saved, void* ws, yh_stream stream);
/* Backward: gpreds[s] same geometry/dtype as preds[s], fully overwritten.
 * gout: device pointer to d(loss)/d(tot) scalar.                                 */
int yh_v5_loss_bwd(const yh_v5loss_desc* d, const void* const* preds, const float* gout,
                   const void* saved, void* const* gpreds, void* ws, yh_stream stream);

/* ------------------------------------------------------------------------ *
 * YOLOv7 loss (loss/yolov7_loss.py:17-402): the YOLOv5 anchor / neighbour match (yh_v5_assign) yields a candidate LIST per
 * stage, a SimOTA dynamic-k assignment over the candidates of each (image, stage) keeps some of them, and CIoU, class BCE
 * and all-cell objectness BCE run over what is kept.  Same head tensors as the YOLOv5 loss.
 * ------------------------------------------------------------------------ */
typedef struct yh_v7loss_desc {
    yh_v5loss_desc v5;            /* every field as in the YOLOv5 loss, except: cls_smooth is not read (the class targets are
                                     smooth_bce()'s 0.95 / 0.05) and targets_xywhn must be 0                               */
    int32_t topk;                 /* hyp['topk'], 1..24                                                                    */
    int32_t use_iou_as_tar_cof;   /* objectness target of a matched cell: 1 clamp(ciou, 0), 0 the constant 1.0             */
} yh_v7loss_desc;
/* At most 128 valid rows (class id >= 0) per image, the contract of the YOLOX loss: the CALLER guarantees it (YOLOV7Loss counts
 * them whenever maxbox > 128 and raises before any launch); later valid rows of an image would be left out of the SimOTA step.
 * An (image, stage) therefore has at most 5 * num_anchor * min(maxbox, 128) candidates.  With cap = 5 * num_anchor * B * maxbox,
 * ws holds 76 bytes and saved 48 bytes per stage and cap row, plus 4 bytes per cell in saved: nothing grows with
 * maxbox^2 * B or with cells * maxbox.                                                                                   */
size_t yh_v7loss_ws_bytes(const yh_v7loss_desc* d);
size_t yh_v7loss_saved_bytes(const yh_v7loss_desc* d);
/* preds / targets / balances / saved as in yh_v5_loss_fwd.  result fp32[8]: tot, iou, cof, cls, tar_nums, 0, 0, 0     */
int yh_v7_loss_fwd(const yh_v7loss_desc* d, const void* const* preds, const float* targets,
                   double* balances, float* result, void* saved, void* ws, yh_stream stream);
/* gpreds[s]: same geometry/dtype as preds[s], fully overwritten.  gout: device pointer to d(loss)/d(tot).               */
int yh_v7_loss_bwd(const yh_v7loss_desc* d, const void* const* preds, const float* gout,
                   const void* saved, void* const* gpreds, void* ws, yh_stream stream);
/* (debug / tests) the matched rows of the forward call that wrote `saved`, in candidate order:
 * count[4] int32 (matched rows per stage), rows[num_stage][cap][5] int32 (img, anchor, gy, gx, target row inside the image's
 * maxbox rows); rows past a stage's count are -1.  Both are device buffers.                                             */
int yh_v7_matches(const yh_v7loss_desc* d, const void* saved, int32_t* count, int32_t* rows, yh_stream stream);

/* ------------------------------------------------------------------------ *
 * YOLOX loss with SimOTA assignment (loss/yolox_loss.py:11-458)
 * ------------------------------------------------------------------------ */
typedef struct yh_yolox_desc {
    int32_t B, maxbox, num_class, num_stage;
    int32_t H[4], W[4], ldp[4];   /* per stage: feature map size, elements per cell ([x,y,w,h,obj,cls...] order) */
    int32_t pred_is_f32;
    float   img_size0;            /* hyp['input_img_size'][0]; stride = img_size0 / H                          */
    int32_t use_focal; float focal_gamma, focal_alpha;
    int32_t use_l1;
    float   iou_scale, cls_scale, cof_scale, l1_scale;
    float   cls_smooth, cls_pos_weight, cof_pos_weight;
    int32_t iou_type;             /* 0 iou, 1 giou, 2 ciou (YOLOXLoss.iou_loss :378-415)                        */
    int32_t topk; float center_radius;
    float   cls_cost_const;       /* class part of the SimOTA cost: constant in the reference (:111-147)        */
} yh_yolox_desc;
/* Ground truths per image: the assignment keeps at most 128 valid rows (class id >= 0) of an image in LDS.  `maxbox` may be
 * larger (padding rows do not count), but the CALLER guarantees that no image has more than 128 valid rows: the library
 * cannot see device data on the host, and rows beyond the 128th would be left out of the assignment.  YOLOXLoss
 * (loss/yolox_loss.py) counts them whenever maxbox > 128 and raises YoloHipError before any launch. */
size_t yh_yolox_saved_bytes(const yh_yolox_desc* d);
size_t yh_yolox_ws_bytes(const yh_yolox_desc* d);
int yh_yolox_layout(const yh_yolox_desc* d, int64_t* out8);
/* targets_xywh: [B][maxbox][6] (cx,cy,w,h,cls,img) pixels, padding rows cls < 0 (the reference converts the
 * caller's xyxy tensor in place, :42).  result fp32[8]: tot, iou, l1, cls, cof, fg_nums, tar_nums, 0           */
int yh_yolox_loss_fwd(const yh_yolox_desc* d, const void* const* preds, const float* targets_xywh,
                      double* balances, float* result, void* saved, void* ws, yh_stream stream);
int yh_yolox_loss_bwd(const yh_yolox_desc* d, const void* const* preds, const float* targets_xywh, const float* gout,
                      const void* saved, void* const* gpreds, yh_stream stream);

/* ------------------------------------------------------------------------ *
 * YOLOv8 loss: task-aligned assignment, CIoU, DFL (loss/yolov8_loss.py:12-411)
 * ------------------------------------------------------------------------ */
typedef struct yh_v8loss_desc {
    int32_t B, maxbox, num_class, num_stage;
    int32_t reg, topk;            /* logits per box side (2..32); cells per ground truth (1..24)                  */
    int32_t H[4], W[4], ldp[4];   /* per stage: feature map size, elements per cell ([4*reg box, cls...] order)  */
    int32_t pred_is_f32;
    float   img_size0;            /* hyp['input_img_size'][0]; stride = img_size0 / H                            */
    float   alpha, beta;          /* metric = iou^beta * score^alpha                                             */
    float   focal_gamma, focal_alpha, cls_pos_weight;
    float   iou_scale, cls_scale, dfl_scale;
} yh_v8loss_desc;
/* Valid rows are those with 0 <= class id < num_class.  The 128 valid rows per image that YOLOV8Loss (loss/yolov8_loss.py)
 * enforces before any launch (it counts rows with class id >= 0 whenever maxbox > 128 and raises YoloHipError) are the
 * contract it shares with YOLOXLoss, not a capacity of these kernels: there is one workgroup per row, and only the pass that
 * settles multiply-chosen cells walks an image's rows serially, so its time grows with their number.  Neither buffer scales
 * with B * maxbox * cells: ws holds 28 bytes per cell and 8 per target row, saved 8 bytes per cell (both 16-byte aligned). */
size_t yh_v8loss_ws_bytes(const yh_v8loss_desc* d);
size_t yh_v8loss_saved_bytes(const yh_v8loss_desc* d);
/* byte offsets inside `saved`: out8[0] = matched target row per cell [B][N] i32 (-1: none), out8[1] = class-target value per
 * cell [B][N] f32, out8[2] = N, out8[4..7] = first cell of each stage inside an image's N cells */
int yh_v8loss_layout(const yh_v8loss_desc* d, int64_t* out8);
/* targets: [B][maxbox][6] (xmin,ymin,xmax,ymax,cls,img) pixels, padding rows cls < 0.
 * result fp32[8]: tot, cls, iou, dfl, tar_nums (assigned cells), sum of the class targets, 0, 0                       */
int yh_v8_loss_fwd(const yh_v8loss_desc* d, const void* const* preds, const float* targets, float* result,
                   void* saved, void* ws, yh_stream stream);
/* gpreds[s]: same geometry/dtype as preds[s], fully overwritten.  gout: device pointer to d(loss)/d(tot).             */
int yh_v8_loss_bwd(const yh_v8loss_desc* d, const void* const* preds, const float* targets, const float* gout,
                   const void* saved, void* const* gpreds, void* ws, yh_stream stream);

/* Box utilities (utils/bbox_tools.py:164-339) fp32.  yh_iou_matrix: (n1, n2) IoU of xyxy boxes; eps_clamp > 0: union clamped from
 * below (gpu_iou, utils/bbox_tools.py:164-190), 0: no clamp on the union (numba_iou :12-35: 0 / 0 = NaN), < 0: no clamp on the
 * intersection sides either (the evaluators' bbox_iou, trainer/eval_yolov5.py:237-258, trainer/eval_yolox.py) */
int yh_iou_matrix(const float* b1, int n1, const float* b2, int n2, float eps_clamp, float* out, yh_stream stream);
/* kind: 0 giou 1 diou 2 ciou ; pairwise (N,) ; grad (optional) d out/d b1 [N][4] */
int yh_iou_pairwise(int kind, const float* b1, const float* b2, int n, float* out, float* grad_b1, yh_stream stream);

/* ------------------------------------------------------------------------ *
 * Inference post-processing (trainer/eval_yolov5.py:182-317, utils/nms.py:10-27)
 * ------------------------------------------------------------------------ */
typedef struct yh_decode_desc {
    int32_t B, num_class, num_anchor, num_stage;
    int32_t H[4], W[4];
    float   stride[4];
    float   anchors[4][3][2];     /* pixels */
    int32_t pred_is_f32;
    int32_t ldp[4];
    int32_t yolox;                /* 0: v5 decode, 1: YOLOX decode (eval_yolox.py:123-150) */
} yh_decode_desc;
/* Full decode to (B, sum(A*H*W), 5+nc) fp32, the tensor do_inference returns.    */
int yh_decode_full(const yh_decode_desc* d, const void* const* preds, float* out, yh_stream stream);
/* Fused decode + candidate filter, order preserving.
 *  cand: [B][cap][6] fp32 (xmin,ymin,xmax,ymax,conf,cls) ; ncand: [B] int32, written not read: the table starts at row 0 (may
 *  exceed cap: rows past cap are counted, not stored).  yh_decode_filter_view below appends instead.
 *  conf_ge: obj >= conf_thr ; cls_gt: cls_conf > cls_thr (v5) / obj*max>=conf & cls>=thr (yolox) */
int yh_decode_filter(const yh_decode_desc* d, const void* const* preds, float conf_thr, float cls_thr,
                     float* cand, int32_t* ncand, int cap, void* ws, yh_stream stream);
/*  ws: yh_decode_filter_ws_bytes(d) bytes, 16-byte aligned: the image is spread over blocks of 64 pixels (rows staged through LDS
 *  with coalesced loads), their candidates are ordered by a second, per-image pass.  ws == NULL: one workgroup per image walks
 *  the predictions (same result; for small heads).                                                                     */
size_t yh_decode_filter_ws_bytes(const yh_decode_desc* d);
/* One pass of test-time augmentation (trainer/eval_yolov5.py:152-179) through the same filter, both forms.  Between the decode
 * and the xywh -> xyxy step the centre-format box (cx, cy, w, h) is mapped back to the original image, in the evaluator's order:
 * all four values times 1.0f / scale (the reciprocal taken once in fp32 — what torch's device kernel computes for
 * `ripe[..., :4] /= s` with a host scalar — not a division per value), then cy = img_h - cy for flip_axis 2 or cx = img_w - cx
 * for flip_axis 3.  Thresholds, class arg-max and the candidate rule are those of yh_decode_filter.
 * The candidates are APPENDED: on entry ncand[b] is the number of rows image b's table holds already (zero it before the first
 * pass; negative counts as 0); the pass stores its candidates from that row on, in prediction order, and leaves
 * ncand[b] = old + its count.  Rows at or past cap are counted, not stored.  scale 1, flip_axis 0 and ncand == 0 give
 * yh_decode_filter's table bit for bit.  ws as for yh_decode_filter (staging area and counts are per call), or NULL.
 * YH_EINVAL: xf NULL, flip_axis outside {0, 2, 3}, scale not positive and finite.  Enqueues only: no allocation, no sync. */
typedef struct yh_view_xform {
    float   scale;
    int32_t flip_axis;            /* 0 none, 2 rows, 3 columns */
    float   img_h, img_w;         /* of the original image, pixels */
} yh_view_xform;
int yh_decode_filter_view(const yh_decode_desc* d, const void* const* preds, const yh_view_xform* xf,
                          float conf_thr, float cls_thr, float* cand, int32_t* ncand /* in/out */, int cap,
                          void* ws, yh_stream stream);
/* The same filter applied to an already decoded (B, N, 5+nc) fp32 tensor — the argument of
 * YOLOV5Evaluator.numba_nms (trainer/eval_yolov5.py:261-286); used after TTA merging.  `yolox`: 0 YOLOv5 single label,
 * 1 YOLOX, 2 YOLOv5 multi-label (hyp['mutil_label'], :276-279: one candidate per (prediction, class) with cls*obj >= cls_thr,
 * in (prediction, class) order; ncand may exceed cap — rows past cap are counted, not stored: the caller re-runs with more),
 * 3 YOLOX multi-label (trainer/eval_yolox.py:218-221: the same among the predictions with obj * max(cls) >= conf_thr). */
int yh_filter_decoded(const float* dec, int B, int N, int num_class, float conf_thr, float cls_thr, int yolox,
                      float* cand, int32_t* ncand, int cap, yh_stream stream);
/* YOLOv8 post-processing (trainer/eval_yolov8.py:76-102, :168-196; yoloseries_amd/csrc/postproc_v8.hip).  A head holds, per cell,
 * 4*reg box logits — sides [t, b, l, r], each softmax(reg logits) . [1, 2, ..., reg] — then num_class class logits; no
 * objectness, no anchors.  Cells: stages in the order given, row-major inside a stage, N = sum H*W.  Box = (gx - l, gy - t,
 * gx + r, gy + b) * (img_h / H) with gx = col + 0.5, gy = row + 0.5 (rectangular maps too: the reference's make_grid scrambles
 * those); scores = sigmoid(class logit), the exact one.  NaN logits are outside the contract.
 * ldp: elements between consecutive cells of a cell-major view, >= 4*reg + num_class; only the leading 4*reg + num_class
 * elements of a row are read, rounded up to whole 16-byte pieces where the tensor and ldp are 16-byte aligned. */
typedef struct yh_v8dec_desc {
    int32_t B, num_class, num_stage, reg;     /* num_stage 1..4, reg 2..32 */
    int32_t H[4], W[4], ldp[4];
    int32_t pred_is_f32;                      /* 1: fp32 heads, 0: bf16 */
    float   img_h;                            /* height of the network input, pixels */
} yh_v8dec_desc;
/* Full decode to (B, N, 4+nc) fp32 [xmin, ymin, xmax, ymax, sigmoid(cls)...], the tensor do_inference returns. */
int yh_v8_decode_full(const yh_v8dec_desc* d, const void* const* preds, float* out, yh_stream stream);
/* Fused decode + single-label candidate filter, order preserving: score = max_c sigmoid(x_c) compared on the fp32 sigmoid values,
 * class = the first index that reaches it, candidate iff score >= cls_thr.  cand [B][cap][6] (xmin, ymin, xmax, ymax, score,
 * cls), cap a positive multiple of 4: the table yh_nms_batched consumes.  The decoded tensor is never written.
 *  xf == NULL: the table starts at row 0 and ncand is written, not read.
 *  xf != NULL: one pass of test-time augmentation (:40-73), APPENDED as yh_decode_filter_view appends (ncand in/out, negative
 *  counts as 0): every box value times 1.0f / scale (the reciprocal taken once in fp32), then for flip_axis 2
 *  ymin' = img_h - ymax, ymax' = img_h - ymin, for flip_axis 3 xmin' = img_w - xmax, xmax' = img_w - xmin (xf->img_h / img_w:
 *  the original image).  {1, 0} with ncand == 0 gives the xf == NULL table bit for bit.
 *  Rows at or past cap are counted, not stored.
 *  ws: yh_v8_decode_filter_ws_bytes(d) bytes, 16-byte aligned (staging area [B][chunks of 64 cells][64][6] and counts; nothing is
 *  sized B*N*(4+nc)): blocks of 64 cells stage their rows through LDS, a second pass per image orders their candidates.
 *  ws == NULL: one workgroup per image walks the cells (same table bit for bit; for small heads).
 * YH_EINVAL: null pointers, reg outside 2..32, num_stage outside 1..4, ldp < 4*reg + num_class, bad xf, bad cap, unaligned ws.
 * All entry points enqueue only: no allocation, no synchronisation. */
size_t yh_v8_decode_filter_ws_bytes(const yh_v8dec_desc* d);
int yh_v8_decode_filter(const yh_v8dec_desc* d, const void* const* preds, const yh_view_xform* xf, float cls_thr,
                        float* cand, int32_t* ncand /* in/out with xf */, int cap, void* ws, yh_stream stream);
/* The candidate rule on an already decoded (B, N, 4+nc) fp32 tensor, the argument of YOLOV8Evaluator.numba_nms.  multi_label 0: as
 * yh_v8_decode_filter; 1 (hyp['mutil_label'], :186-189): one row per (cell, class) with value >= cls_thr, in (cell, class) order.
 * ncand may exceed cap: rows past cap are counted, not stored. */
int yh_v8_filter_decoded(const float* dec, int B, int N, int num_class, float cls_thr, int multi_label,
                         float* cand, int32_t* ncand, int cap, yh_stream stream);
/* Greedy NMS per image on candidate lists, selection order = reference order.
 *  class_aware: add cls*4096 to the box before IoU (hyp['agnostic'] == True in the reference)
 *  thr_inclusive: 1 -> suppress when iou >= thr (numba_nms), 0 -> iou > thr (gpu_nms)
 *  merge_filter: postprocess_bbox filter (eval_yolov5.py:306-315)
 *  out: [B][max_keep][6] ; nkeep [B] ; keep_idx [B][max_keep] index into the candidate list
 *  ncand[b] > cap (a filter that counted rows it could not store) is read as cap: the first cap rows of image b are its candidates.
 *  Only keep_idx[b][0 .. nkeep[b]) is defined: keep_idx past nkeep[b] is undefined (scratch of the pick list); out past nkeep[b]
 *  is not written.
 *  Candidates are sorted once by (score descending, index ascending) and consumed in chunks of 64 whose mutual suppression is a
 *  64 x 64 bit matrix built with wave shuffles; scores must be non-negative (non-positive scores are never selected).
 *  ws: yh_nms_ws_bytes(B, cap) bytes, 16-byte aligned (sort keys, class-offset boxes in candidate and in sorted order, flags) */
size_t yh_nms_ws_bytes(int B, int cap);
int yh_nms_batched(const float* cand, const int32_t* ncand, int B, int cap,
                   float iou_thr, int class_aware, int thr_inclusive, int max_keep, int merge_filter,
                   float* out, int32_t* nkeep, int32_t* keep_idx, void* ws, yh_stream stream);
/* Validation metric on the device (yoloseries_amd/csrc/metric.hip lists the operation order): the NMS table of a batch and its
 * ground truth, both in the letterboxed frame, to the per-detection match table of utils/mAP.py — the un-letterbox of
 * val_yolov5.py (preds_postprocess: (v - pad) / scale clamped to [1, org - 1]; gt_bbox_postprocess: no clamp; true fp32 divisions)
 * and compute_tp (IoU as iou_np, same class, the 10 COCO thresholds) per image.
 *  det [B][max_keep][6], nkeep [B]: what yh_nms_batched writes.  gt [B][maxbox][gt_ld], gt_ld >= 5: xmin, ymin, xmax, ymax, cls —
 *  the collate format; a row with cls < 0 is padding, anywhere in the list.  info [B][5]: scale, pad_top, pad_left, org_h, org_w.
 *  thr: n_thr <= 16 doubles in HOST memory, ascending (read during the call; thr[0] is the matching threshold).
 * An image counts iff nkeep[b] > 0 and it has a valid ground-truth row (the rule of mAP_v2.__init__).  Per image and row
 * p < nkeep[b] (rows at or past nkeep[b], and every row of an image that does not count, are left untouched):
 *  box [B][max_keep][4] the detection in the original frame; conf; cls (int32); iou: the matched IoU, 0 when unmatched; gt_idx: the
 *  matched row of gt, -1 when unmatched; tp (uint16): bit k set iff matched and (double)iou >= thr[k].
 *  nrow [B]: nkeep[b] if the image counts, else 0.  gt_hist [num_class] int32 is ACCUMULATED (integer atomics; zero it before the
 *  first batch): the classes of the valid ground truth of the images that count.
 * Detection p is matched to the valid ground truth of its class with the largest IoU >= thr[0]; a ground truth claimed by several
 * detections keeps the LOWEST p (compute_tp's second np.unique), the others are unmatched.  Exact IoU ties between two ground
 * truths of one detection are outside the host code's contract (unstable sort); here the lowest ground-truth row wins.
 * YH_EINVAL: a NULL pointer, gt_ld < 5, n_thr outside 1..16, a non-positive size.  Enqueues only: no allocation, no sync. */
int yh_val_match(const float* det, const int32_t* nkeep, const float* gt, const float* info, int B, int max_keep, int maxbox,
                 int gt_ld, int num_class, const double* thr, int n_thr, float* box, float* conf, int32_t* cls, float* iou,
                 int32_t* gt_idx, uint16_t* tp, int32_t* nrow, int32_t* gt_hist, yh_stream stream);
/* The rest of the metric on the device: the match table of a whole pass to the per-class AP and the precision / recall curves of
 * utils/mAP.py compute_ap_per_class / compute_ap (yoloseries_amd/csrc/metric.hip lists the operation order: fp64, each operation once).
 *  conf [N] fp32, cls [N] int32, tp [N] uint16 (bit k: IoU threshold k): the compacted rows of the images that count, as yh_val_match
 *  wrote them.  order [N] int32: a permutation of the rows, class ascending, then conf descending — the library does not sort.
 *  gt_hist [num_class] int32.  xs_ap [n_ap], xs_pr [n_pr] doubles in DEVICE memory, ascending: np.linspace(0, 1, 101) and
 *  np.linspace(0, 1, 1000), made by the caller (i * step and i / n differ in the last bit); 2 <= n_ap <= 1024, n_pr >= 1.
 *  ap [num_class][n_thr], precision [num_class][n_pr], recall [num_class][n_pr] doubles (the curves are threshold 0's);
 *  npred [num_class] int32: the rows of the class, counted or not.  Every element of the four is written on every call; ap,
 *  precision and recall of a class with gt_hist[c] <= 0 or without a row are zeros.  ap is the trapezoid sum over xs_ap added left
 *  to right (np.sum adds pairwise: a few ulp apart).
 *  ws: yh_val_ap_ws_bytes(N, n_thr) bytes, 4-byte aligned (the cumulative true positives per row and threshold).
 * Outside the contract: two rows of one class with equal conf and different tp masks (the host's order there comes from an unstable
 * sort; here `order` decides — with a stable sort the lower original row comes first); NaN or negative conf; a class with more
 * true positives than ground truth.  An entry of order outside [0, N) is clamped, never followed.
 * YH_EINVAL: a NULL pointer, non-positive N or num_class, n_thr outside 1..16, n_ap outside 2..1024, n_pr < 1, an unaligned table.
 * One launch, a workgroup per (class, threshold).  Enqueues only: no allocation, no sync. */
size_t yh_val_ap_ws_bytes(int N, int n_thr);
int yh_val_ap(const float* conf, const int32_t* cls, const uint16_t* tp, const int32_t* order, int N, const int32_t* gt_hist,
              int num_class, int n_thr, const double* xs_ap, int n_ap, const double* xs_pr, int n_pr, double* ap, double* precision,
              double* recall, int32_t* npred, void* ws, yh_stream stream);

/* Weighted box fusion (utils/weighted_fusion_bbox.py, do_wfb of trainer/eval_yolov5.py:44-92) of candidate tables where they lie:
 * per (image, class), rows by score descending, starting from no cluster, a row joins EVERY cluster whose fused box has fp64 IoU
 * (cpu_iou: sides clamped at 0, union clipped below at 1e-6) >= iou_thr with it, or founds a new one; the fused boxes are refreshed
 * after every row (yoloseries_amd/csrc/wbf.hip lists the operation order: fp64 running sums in arrival order, each operation once).
 *  cand [B][cap][6]: xmin, ymin, xmax, ymax, score, cls.  weight [B][cap]: the row's model weight; <= 0: not a candidate (holes
 *  anywhere in a table are fine).
 *  order [B][cap] int32, nvalid [B]: order[b][0 .. nvalid[b]) are the candidate rows of image b — weight > 0, score > 0, 0 <= cls <
 *  num_class — class ascending, then score descending; the library does not sort.  Entries past nvalid[b] are not read.
 *  box_mean 0: the reference's box, sum(s_i b_i) / sum(s_i) / N (its np.mean divides by the member count once more); 1: the usual
 *  weighted box sum(s_i b_i) / sum(s_i).  The fused score is sum(s_i w_i) / sum(w_i) in both.
 *  out [B][cap][6]: float32 of the fp64 box and score, and the class; rows class ascending, then in the order the clusters were
 *  founded; nout [B]; rows at or past nout[b] are undefined.  members [B][cap] (may be NULL): N of each output row.
 *  ws: yh_wbf_ws_bytes(B, cap) bytes, 8-byte aligned.  The state of the first yh_wbf_lds_clusters() clusters of an (image, class)
 *  lives in LDS, that of the others in ws: the number of clusters is bounded by the number of rows only.
 * Outside the contract: NaN coordinates or scores; a row below nvalid with cls outside [0, num_class) (its staging slot is never
 * written).  Neither can make a kernel read or write out of bounds: entries of order and nvalid are clamped.
 * YH_EINVAL: a NULL pointer (members excepted), non-positive B / cap / num_class, B > 65535, box_mean outside {0, 1}, NaN iou_thr,
 * an unaligned table.  Two launches (a workgroup per (class, image), then one per image).  Enqueues only: no allocation, no sync. */
int yh_wbf_lds_clusters(void);
size_t yh_wbf_ws_bytes(int B, int cap);
int yh_wbf_batched(const float* cand, const float* weight, const int32_t* order, const int32_t* nvalid, int B, int cap, int num_class,
                   double iou_thr, int box_mean, float* out, int32_t* nout, int32_t* members, void* ws, yh_stream stream);

/* ------------------------------------------------------------------------
 * Program executor: replay a pre-built list of launches with one call (the engine's forward / backward programs; replaces the
 * host loop over ~700 calls of a train step: train_yolov5.py:327-350 spends that time inside torch's dispatcher instead).
 * A command is an entry point of this library (index from yh_exec_op) with its arguments widened to 8-byte slots — pointers
 * and integers as (u)int64, float / double as the bit pattern of a double — in declaration order, the stream slot last (its
 * value is replaced by streams[cmd.stream]); or YH_CMD_EVENT_RECORD / YH_CMD_STREAM_WAIT with a hipEvent_t in slot 0.
 * Executed in order; on failure returns the callee's status and, in *failed, the index of the command.              */
#define YH_CMD_SLOTS 16
#define YH_CMD_EVENT_RECORD (-1)
#define YH_CMD_STREAM_WAIT  (-2)
typedef struct yh_cmd {
    int32_t  op;            /* yh_exec_op() index, or YH_CMD_EVENT_RECORD / YH_CMD_STREAM_WAIT */
    int32_t  nslots;        /* argument count incl. the stream */
    int32_t  stream;        /* index into yh_exec's streams[] */
    int32_t  reserved;
    uint64_t slots[YH_CMD_SLOTS];
} yh_cmd;
int yh_exec_op(const char* name, int* nargs);
int yh_exec(const yh_cmd* cmds, int n, const yh_stream* streams, int nstreams, int* failed);

#ifdef __cplusplus
}
#endif
#endif /* YOLOHIP_H */
