// Shared device helpers for the gfx950 kernels (wave64, bf16 storage as uint16).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/yolohip.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

#define YH_WAVE 64

__device__ __forceinline__ float bf2f(uint16_t u) { return __uint_as_float(((uint32_t)u) << 16); }
// round-to-nearest-even, NaN preserving (hipcc lowers the cast to v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint16_t f2bf(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(uint16_t, b);
}
__device__ __forceinline__ float bf_round(float f) { return bf2f(f2bf(f)); }

__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
    f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}
// two floats -> packed bf16 pair (lo in bits 0..15), one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) float f32x2_t;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    f32x2_t v = {lo, hi};
    bf16x2_t b = __builtin_convertvector(v, bf16x2_t);
    return __builtin_bit_cast(uint32_t, b);
}
__device__ __forceinline__ uint4 pack8(const float* f) {
    uint4 v;
    v.x = pack2(f[0], f[1]);
    v.y = pack2(f[2], f[3]);
    v.z = pack2(f[4], f[5]);
    v.w = pack2(f[6], f[7]);
    return v;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }
__device__ __forceinline__ float siluf_(float x) { return x * sigmoidf_(x); }
// approximate-reciprocal variants (v_exp_f32 + v_rcp_f32, ~1 ulp each) for the bf16 activation path;
// the loss / assignment kernels keep the IEEE-division forms above
__device__ __forceinline__ float sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float silu_fast(float x) { return x * sigmoid_fast(x); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- LDS-DMA (global -> LDS without VGPR staging) ---------------------------
#define YH_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(n) : "memory")
// counted wait with a wave-uniform run-time count (the instruction takes an immediate)
#define YH_VMCNT_SW(n) do { switch (n) { case 0: YH_VMCNT(0); break; case 1: YH_VMCNT(1); break; case 2: YH_VMCNT(2); break; case 3: YH_VMCNT(3); break; \
    case 4: YH_VMCNT(4); break; case 5: YH_VMCNT(5); break; case 6: YH_VMCNT(6); break; case 7: YH_VMCNT(7); break; case 8: YH_VMCNT(8); break; \
    case 9: YH_VMCNT(9); break; default: YH_VMCNT(10); break; } } while (0)
// workgroup barrier that orders LDS accesses only: unlike __syncthreads() it does not drain LDS-DMA transfers in flight
#define YH_LDS_BARRIER() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); } while (0)

// one LDS-DMA wave instruction: 64 lanes x 16 bytes from (rsrc, per-lane voff + scalar soff) to lds .. lds + 1024
__device__ __forceinline__ void lds_dma16(const __amdgpu_buffer_rsrc_t rs, unsigned char* lds, unsigned voff, int soff)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) void lds_void;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void*)lds, 16, voff, soff, 0, 0);
#endif
}

// ---- host side helpers -----------------------------------------------------
void yh_set_error(const char* fmt, ...);

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: a process that launches on a second GPU must set
// it there too.  One flag per device (bit mask over the first 64 devices, others set the attribute at every launch), written only
// after every hipFuncSetAttribute of the block has succeeded; two threads may both set the attributes (idempotent), none launches
// before they are set.  A failed set leaves the flag clear and the launch behind it reports hipErrorInvalidValue (YH_CHECK_LAUNCH).
// The flags are all the threads share: whether a block succeeded is judged from a local of the thread that ran it.
#include <atomic>
#include <initializer_list>
struct YhDevOnce { std::atomic<uint64_t> mask{0}; };
struct YhLdsLimit { const void* kernel; int bytes; };
// raises the dynamic-LDS limit of every listed kernel on the current device, unless `once` says it has been done there
inline void yh_lds_limit(YhDevOnce& once, std::initializer_list<YhLdsLimit> limits)
{
    int dev = -1;
    const bool flagged = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64;
    if (flagged && ((once.mask.load(std::memory_order_acquire) >> dev) & 1ull)) return;
    bool ok = true;
    for (const YhLdsLimit& l : limits) {
        const hipError_t e = hipFuncSetAttribute(l.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, l.bytes);
        if (e != hipSuccess) { ok = false; yh_set_error("hipFuncSetAttribute(%d bytes of LDS): %s", l.bytes, hipGetErrorString(e)); }
    }
    if (ok && flagged) once.mask.fetch_or(1ull << dev, std::memory_order_release);
}
#define YH_CHECK_ARG(cond, ...) do { if (!(cond)) { yh_set_error(__VA_ARGS__); return YH_EINVAL; } } while (0)
#define YH_CHECK_LAUNCH(name) do { hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) { yh_set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); return YH_ELAUNCH; } } while (0)

static inline bool yh_aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// the element type of the head tensors (desc.pred_is_f32) as a type: f(float()) or f(uint16_t()) (bf16), so that a launch
// of a kernel<T> is written once:  yh_pred_type(d->pred_is_f32, [&](auto e) { using T = decltype(e); ... kernel<T> ... });
template <typename F> inline void yh_pred_type(int is_f32, F&& f) { if (is_f32) f(float()); else f(uint16_t()); }

// an epilogue of a conv beyond the plain store: affine / activation / residual / second destination (_na: accumulation aside)
inline bool conv_generic_na(const yh_conv_desc* d) { return d->bias || d->scale || d->shift || d->act != YH_ACT_NONE || d->res || d->nsplit < d->N; }
inline bool conv_generic(const yh_conv_desc* d) { return conv_generic_na(d) || d->accumulate; }
// the operands of the fused BatchNorm-backward reduction (d->bnr_part) as every kernel with that epilogue reads them
inline bool conv_bnr_operands(const yh_conv_desc* d) { return d->bnr_z && yh_aligned16(d->bnr_z) && d->bnr_ldz % 8 == 0 && d->bnr_ws && d->bnr_C >= d->N; }

// ---- the sibling kernel families behind yh_conv_igemm (d->algo), two functions each, both made from ONE <s>_plan(d) of their file:
//   yh_<s>_info:   what the plan says, without a stream: out->rows = its grid rows along x (the rows of the slabs the family writes)
//                  and out->name = the instantiation as profilers print it; returns the rc of the operand checks that stand before
//                  the launch (the name stays empty where they fail)
//   yh_<s>_launch: plans, checks, launches
// Either answers YH_CONV_DECLINED (info: with rows 0) and sets no error text where the plan does not take the descriptor: the
// dispatcher (conv_choose in conv_igemm.hip) then goes on with the library default.
constexpr int YH_CONV_DECLINED = 1;
struct ConvSibInfo { int rows; char name[96]; };
// conv_dg2.hip: the stride-2 data-gradient kernel (algo 7)
int yh_dg2_info(const yh_conv_desc* d, ConvSibInfo* out);
int yh_dg2_launch(const yh_conv_desc* d, yh_stream stream);
// conv_p3.hip: the 3x3 / stride-1 patch kernel for small channel counts (algo 8)
int yh_p3_info(const yh_conv_desc* d, ConvSibInfo* out);
int yh_p3_launch(const yh_conv_desc* d, yh_stream stream);
// conv_h80.hip: the 80-channel 3x3 halo kernel (YOLOv5x stage 1, inference epilogues; algo 9)
int yh_h80_info(const yh_conv_desc* d, ConvSibInfo* out);
int yh_h80_launch(const yh_conv_desc* d, yh_stream stream);
// conv_pw.hip: the pointwise (1x1) kernel for the 80- / 160- / 320-channel layers of YOLOv5x (inference epilogues; algo 10)
int yh_pw_info(const yh_conv_desc* d, ConvSibInfo* out);
int yh_pw_launch(const yh_conv_desc* d, yh_stream stream);
// conv_c80.hip: the 80 -> 160 channel tap kernel (inference epilogue; algo 12)
int yh_c80_info(const yh_conv_desc* d, ConvSibInfo* out);
int yh_c80_launch(const yh_conv_desc* d, yh_stream stream);
// conv_pt.hip: the pointwise (1x1) kernel of the TRAINING step (all four epilogues; algo 13; rows = pixel slots of its grid)
int yh_pt_info(const yh_conv_desc* d, ConvSibInfo* out);
int yh_pt_launch(const yh_conv_desc* d, yh_stream stream);

// conv_wgp.hip: the patch form of the weight gradient behind yh_conv_wgrad (tile_k 40)
int yh_wgp_ok(const yh_wgrad_desc* d);
int yh_wgp_run(const yh_wgrad_desc* d, yh_stream stream);

// conv_wgs.hip: wave-private 128 x 128 tiles + stream-K for the K-heavy layers behind yh_conv_wgrad (tile_k 129)
int yh_wgs_ok(const yh_wgrad_desc* d);
int yh_wgs_tiles(const yh_wgrad_desc* d);
const char* yh_wgs_name(const yh_wgrad_desc* d);
size_t yh_wgs_ws_bytes(const yh_wgrad_desc* d);
int yh_wgs_run(const yh_wgrad_desc* d, yh_stream stream);
