/*
 * rubiks_hip.h -- C ABI of librubiks_hip.so, the MI355X (gfx950) implementation of
 * the RubiksShift hot path.  This is the drop-in boundary: these entry points are
 * what the reference's extension module `rubiksnet_cuda`
 * (cuda_src/rubiks.cpp:384-396, built by setup.py:41-52) binds, restated as plain C
 * (raw device pointers + sizes, no torch types).  INTEGRATION.md shows the
 * reference-side ctypes binding (`rubiksnet_cuda.py`) a maintainer would add.
 *
 * Conventions (all entry points)
 *   - every pointer is a DEVICE pointer on the device that is current when the call
 *     is made; `stream` is a hipStream_t of that device (NULL = the null stream).
 *     The reference launches on the legacy default stream of whatever device is
 *     current and reads device attributes from device 0 (rubiks3d_kernels.cu:975-998);
 *     here the caller names the stream and the library caches nothing per device.
 *   - tensors are dense/contiguous in the reference's layouts:
 *       3D: x [N,T,C,H,W], y / gy [N,To,C,Ho,Wo], shift / gshift [3,C] rows = (T,H,W)
 *           (rubiks.cpp:197-207, :243-244)
 *       2D: x [N,C,H,W],  y / gy [N,C,Ho,Wo],     shift / gshift [2,C] rows = (H,W)
 *           (rubiks.cpp:61-63)
 *     out = (in + 2*pad - 1) / stride + 1   (rubiks.cpp:166 -- not the conv formula);
 *     rk_out_len() exposes it.
 *   - the caller owns every buffer including outputs and the workspace (the reference
 *     allocates scratch inside, rubiks.cpp:127-132,295-299); nothing is allocated,
 *     freed or synchronised inside the library, so calls are graph-capturable.
 *   - 3D kernels write EVERY element of y / gx / gshift (no pre-zeroing needed).
 *     2D with quantize != 0 reproduces the reference quirk of leaving out-of-range
 *     elements of y / gx untouched (rubiks2d_kernels.cu:116-121, :294-309): pre-zero
 *     those two buffers in that case, as rubiksnet/utils.py:26 does.
 *   - return value: RK_OK (0) or a negative RK_ERR_* code; never exit()s
 *     (the reference's gpuAssert does, rubiks3d_kernels.cu:963-971).  The reference's
 *     Python asserts `ret == 0` (rubiks3d/primitive.py:79,139).
 *   - re-entrant and thread-safe: any thread may call any entry point on any device (autograd worker threads,
 *     nn.DataParallel's one-thread-per-device backward).  The only process-wide mutable state is atomic and
 *     order-independent: the launch-tag counter and poll budget of the in-launch finalizers (rk_dma.hpp), and, PER
 *     DEVICE, the cached CU count, the "dynamic-LDS ceiling already raised" bit of each kernel instantiation
 *     (rk_common.hpp: raise_dynamic_lds -- hipFuncSetAttribute is per device) and the pointer to the caller's give-up
 *     record (rk_fin_status_register below: the library stores the pointer, the memory stays the caller's).  Calls act
 *     on the CURRENT device of the calling thread (hipGetDevice); the Python layer sets it from the tensors' device.
 *   - environment switches, each read once per process:
 *       RK_SHIFT_KERNELS = auto | column | generic selects which kernel families the shift operators may use
 *         (rk_common.hpp; 3-D: rk3d_plan.hpp plan3d::plan, rk_debug_3d_plan shows the choice; 2-D: rk2d_plan.hpp plan2d::plan,
 *         rk_debug_2d_plan, held by tests/test_plan2d.py; every family is bit-identical for y and d(x),
 *         tests/test_fallback_paths_gpu.py);
 *         RK_FORCE_GENERIC=1 is the older spelling of `generic`;
 *       RK_PW2 = 1 | 0 | 2, RK_PW3 = 1 | 0, RK_PW4 = 1 | 0 | 2: the fp32 1x1 kernel generations (rk_pw.hip: plan_gemm;
 *         rk_debug_pw_gemm_plan shows the choice);
 *       RK_SLAB14 = 1 | 0: the slab kernels on 14x14 planes for the backward too / for nothing (unset: forward only;
 *         rk3d_plan.hpp plan3d::plan, rk_debug_3d_plan);
 *       RK_BN_FLAT16 = 0: the 4-element BatchNorm sweep for 16-bit storage too; RK_BN_STATS_FUSED = 0: BatchNorm statistics
 *         as a statistics kernel + a finisher kernel (rk_bn.hip).
 */
#ifndef RUBIKS_HIP_H_
#define RUBIKS_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rk_stream_t; /* hipStream_t */

enum {
    RK_OK = 0,
    RK_ERR_NULL_POINTER = -1,  /* a required pointer is NULL */
    RK_ERR_BAD_DIMS = -2,      /* a dimension is <= 0 or element count overflows int32 */
    RK_ERR_BAD_STRIDE = -3,    /* stride <= 0 or padding < 0 (reference only prints, rubiks.cpp:162-164) */
    RK_ERR_WORKSPACE = -4,     /* workspace NULL or smaller than *_workspace_bytes() */
    RK_ERR_LAUNCH = -5,        /* hipGetLastError() after a launch was not hipSuccess */
    RK_ERR_NO_DEVICE = -6,     /* no usable HIP device */
    RK_ERR_UNSUPPORTED = -7    /* the fused entry point has no kernel for this configuration: nothing was launched, use
                                  the unfused entry points (only the *_bn_* entry points and the planner's test hook return it) */
};

int rk_version(void);                 /* 1000*major + minor */
const char* rk_error_string(int code);
int rk_out_len(int in, int stride, int pad); /* rubiks.cpp:14-30, :161-178 */
int rk_device_count(void);            /* hipGetDeviceCount, 0 when none */
/* test hook (no reference counterpart): the tag the next backward launch with an in-launch row-sum will stamp its
 * workspace granules with; lets the parity tests pre-fill a workspace with adversarial near-miss patterns */
unsigned rk_debug_peek_launch_tag(void);
/* test hooks for the in-launch finalizers' give-up path (tests/test_finalizer_gpu.py): the poll budget after which a
 * finalizer wave stops waiting for partials and writes NaN (default ~2 s; spins <= 0 restores it; returns the previous
 * value), and a launch of ONLY the 3-D finalizer waves over a workspace nothing publishes to. */
int rk_debug_set_finalize_spins(int spins);
int rk3d_debug_finalize_only_f32(void* ws, size_t ws_bytes, int C, int partials, float* gshift, int normalize_grad,
                                 float t_factor, rk_stream_t stream);
/* The give-up record of the in-launch finalizers.  Every streaming backward (and the fused BatchNorm statistics) finishes its
 * per-channel sums inside the producing launch; a finalizer wave that has not seen its partials after the poll budget
 * (~2 s) gives up and its outputs (gshift / gtaps / dgamma / dbeta / k12 / the BatchNorm statistics) are NaN -- long after
 * the entry point returned RK_OK.  A registered record makes that give-up distinguishable from NaN data:
 *   record[0] give-ups (finalizer waves that timed out) since the record was last zeroed
 *   record[1] launch tag of the first of them (0: none)      record[2] launch tag of the most recent one
 *   record[3] reserved, 0
 * (unsigned words; the tag of a launch is what rk_debug_peek_launch_tag returned before it.)  Only a finalizer that gives
 * up writes, with device-scope atomics; the NaN outputs stay as they are.
 * rk_fin_status_register acts on the calling thread's current device: `record` is caller-owned device memory of
 * RK_FIN_STATUS_BYTES, 16-byte aligned and zeroed by the caller, which launches made from then on (any thread, that
 * device) report into; NULL unregisters.  Returns RK_OK, RK_ERR_NO_DEVICE (no current device, or a device index beyond
 * the 64 the library keeps per-device state for) or RK_ERR_BAD_DIMS (misaligned).  No allocation, no copy, no
 * synchronisation, no device call beyond hipGetDevice; the caller reads and re-zeroes the record when it likes (a plain
 * 16-byte copy on a stream).  A caller that never registers gets the behaviour without a record, bit for bit.  The pointer
 * travels as a kernel argument, so a captured hipGraph keeps the one it was captured with: a record must outlive every
 * graph captured while it was registered.
 * rk3d_debug_finalize_only_status_f32 is rk3d_debug_finalize_only_f32 with an explicit record (NULL allowed) in place of
 * the registered one; rk3d_debug_finalize_only_f32 itself never reports (record = NULL). */
#define RK_FIN_STATUS_BYTES 16
int rk_fin_status_register(void* record);
int rk3d_debug_finalize_only_status_f32(void* ws, size_t ws_bytes, int C, int partials, float* gshift, int normalize_grad,
                                        float t_factor, void* record, rk_stream_t stream);
/* the fp32 1x1 GEMM's kernel choice (rk_pw.hip: plan_gemm) with explicit switches RK_PW2 / RK_PW3 / RK_PW4 and CU count, no
 * device call: the status rk_pw_gemm_{f32,fused_f32,stats_f32,bnbwd_f32} would return before launching and, in out[5], the
 * generation (1..4, 0: none), its configuration (1: wm, kc; 2: rb, amode, ct; 3: columns per workgroup, workgroups; 4: row
 * blocks, k-steps) and the statistics tiles of an epilogue call (= rk_pw_gemm_tiles).  aligned: A and X 16-byte aligned;
 * epi 0 / 1 (statistics) / 2 (BatchNorm backward); res, pro, ma: residual, prologue (ka), output affine (ma) present.
 * rk_debug_pw_wgrad_plan: the fp32 d(weight)'s kernel (2: rk_pw2.hip, 1: first generation wide, 0: narrow). */
int rk_debug_pw_gemm_plan(int F, int K, int M, int P, int a_is_mk, int aligned, int epi, int res, int pro, int ma, int pw2,
                          int pw3, int pw4, int cus, int* out);
int rk_debug_pw_wgrad_plan(int F, int K, int M, int P, int pw2);
/* the RubiksShift3D kernel choice (rk3d_plan.hpp: plan3d::plan) with explicit switches and one alignment bit per operand, no
 * device call.  form: 0 forward, 1 backward (want_gx / want_gshift; two_phase: rk3d_backward_partials_f32), 2 rk3d_forward_bn_f32,
 * 3 rk3d_backward_bn_f32; elem_size 4 / 8 / 2 (the 16-bit entry points; forms 2, 3 and two_phase: RK_ERR_UNSUPPORTED); aligned (16 bytes): 1 x / z, 2 y (forward) or gy, 4 gx / dz, 8 the BatchNorm pack;
 * shift_kernels: 0 auto, 1 column, 2 generic (RK_SHIFT_KERNELS); slab14: -1 unset, 0, 1 (RK_SLAB14).  Returns the status the
 * call would have as far as it does not depend on pointers.  out[30]: launches, P (partials per channel and sum: the workspace
 * holds [C][3 or 5][P]), whether a separate finalize launch follows, then per launch (3 x 9): family (the enum of
 * rk3d_plan.hpp), the 5 variant parameters its launcher switches on, grid, block, dynamic LDS bytes. */
int rk_debug_3d_plan(int form, int elem_size, int N, int T, int C, int H, int W, int sT, int sH, int sW, int pT, int pH, int pW,
                     int quantize, int want_gx, int want_gshift, int two_phase, int aligned, int shift_kernels, int slab14,
                     int* out);
/* the RubiksShift2D kernel choice (rk2d_plan.hpp: plan2d::plan) with explicit switches and alignments, no device call.
 * form: 0 forward, 1 backward (want_gshift: enable_shift_grad), 2 rk2d_forward_bn_*, 3 rk2d_backward_bn_*; elem_size 4 / 8 / 2
 * (f16 / bf16 activations, either shift type); aligned: two bits per operand from bit 0 -- x / z, y (forward) or gy, gx / dz, the
 * BatchNorm pack -- 2: a multiple of 16 bytes, 1: of 8, 0: neither; shift_kernels: 0 auto, 1 column, 2 generic
 * (RK_SHIFT_KERNELS); cus: compute units of the device.  Returns the status the call would have as far as it does not depend
 * on pointers.  out[36]: launches, P (partials per channel and sum: the workspace holds [C][2 or 4][P]), whether k2d_finalize /
 * k2d_finalize_bn follows as a launch of its own, then per launch (3 x 11): family (the enum of rk2d_plan.hpp), negate, bn,
 * rounds, M, single, vec, quant, grid, block, dynamic LDS bytes. */
int rk_debug_2d_plan(int form, int elem_size, int N, int C, int H, int W, int sH, int sW, int pH, int pW, int quantize,
                     int want_gshift, int aligned, int shift_kernels, int cus, int* out);

/* ------------------------------------------------------------------------- 3D
 * Replaces rubiks_shift_3d_forward<T>  (cuda_src/rubiks.cpp:181-253) + functor
 * RubiksShift3DForward (cuda_src/rubiks3d.h:13-28) + K1 (rubiks3d_kernels.cu:15-205).
 * pybind names: rubiks_shift_3d_forward_float / _double (rubiks.cpp:392-393). */
int rk3d_forward_f32(const float* x, const float* shift, float* y,
                     int N, int T, int C, int H, int W,
                     int stride_T, int stride_H, int stride_W,
                     int pad_T, int pad_H, int pad_W,
                     int quantize, rk_stream_t stream);
int rk3d_forward_f64(const double* x, const double* shift, double* y,
                     int N, int T, int C, int H, int W,
                     int stride_T, int stride_H, int stride_W,
                     int pad_T, int pad_H, int pad_W,
                     int quantize, rk_stream_t stream);

/* Bytes of scratch rk3d_backward_* needs (elem_size = 4 or 8; 2: the 16-bit entry points, plain fp32 partials).  Replaces the
 * zeros[3C,Ho,Wo] + ones[Ho,Wo] allocations of rubiks.cpp:294-299.  The scratch needs NO initialisation and may be
 * reused by the next call on the same stream: the streaming fp32 kernels keep their partials there as 8-byte
 * {value, launch tag} granules and run the row-sum + K5 inside the backward launch. */
size_t rk3d_backward_workspace_bytes(int N, int T, int C, int H, int W,
                                     int stride_T, int stride_H, int stride_W,
                                     int pad_T, int pad_H, int pad_W, int elem_size);

/* Replaces rubiks_shift_3d_backward<T> (cuda_src/rubiks.cpp:256-379): K2 partials +
 * addmv row-sum (:344-345) + K5 normalise (:352-358) + K3/K4 input grad (:363-376),
 * functors cuda_src/rubiks3d.h:31-81.  pybind names rubiks_shift_3d_backward_float /
 * _double (rubiks.cpp:394-395).  Both gradients are always produced, as in the
 * reference; gx or gshift may be NULL to skip that half (extension).
 * `x` is read only for gshift (the reference passes it to K3/K4 but never reads it). */
int rk3d_backward_f32(const float* x, const float* shift, const float* gy,
                      float* gx, float* gshift,
                      int N, int T, int C, int H, int W,
                      int stride_T, int stride_H, int stride_W,
                      int pad_T, int pad_H, int pad_W,
                      int normalize_grad, float normalize_t_factor, int quantize,
                      void* workspace, size_t workspace_bytes, rk_stream_t stream);
int rk3d_backward_f64(const double* x, const double* shift, const double* gy,
                      double* gx, double* gshift,
                      int N, int T, int C, int H, int W,
                      int stride_T, int stride_H, int stride_W,
                      int pad_T, int pad_H, int pad_W,
                      int normalize_grad, double normalize_t_factor, int quantize,
                      void* workspace, size_t workspace_bytes, rk_stream_t stream);

/* Two-phase form of rk3d_backward_f32, the phases of the reference's own host glue (rubiks.cpp:324-376):
 * _partials = K2 + K3/K4: writes gx (or skips it when NULL) and the per-channel partial sums workspace[C][3][P],
 * P returned through *partials; _finalize = addmv row-sum (:344-345) + K5 normalise (:352-358) into gshift[3][C].
 * rk3d_backward_f32 computes exactly what _partials followed by _finalize compute, bit for bit (same partials,
 * same summation order); on the streaming shapes it does so in ONE launch (bench.py times both forms).          */
int rk3d_backward_partials_f32(const float* x, const float* shift, const float* gy, float* gx,
                               int N, int T, int C, int H, int W,
                               int stride_T, int stride_H, int stride_W, int pad_T, int pad_H, int pad_W,
                               int quantize, void* workspace, size_t workspace_bytes, int* partials,
                               rk_stream_t stream);
int rk3d_backward_finalize_f32(const void* workspace, int C, int partials, float* gshift,
                               int normalize_grad, float normalize_t_factor, rk_stream_t stream);

/* RubiksShift3D on 16-bit activations with the shift table and d(shift) in fp32 -- what torch.autocast hands the operator:
 * bf16 / f16 x, y, gy and gx next to an fp32 parameter.  The shift is never rounded to the storage type; the arithmetic is
 * the fp32 operator's, in fp32 (same expression trees, contraction off), and a result is rounded to the storage type once,
 * on store, round-to-nearest-even.  So y and gx are, bit for bit, what the fp32 entry points give on the widened tensors,
 * narrowed -- quantize included.  gshift is summed in fp32 per partial, then in a fixed order in fp64 per channel, as in
 * the fp32 operator; normalize_grad / normalize_t_factor as there.  gx or gshift may be NULL to skip that half; the
 * workspace (needed for gshift only) is the one for elem_size = 2.  Validation order and error codes as the fp32 entry
 * points.  Pad 0 / quantize off configurations at stride (1,1,1), or at stride (1,2,2) with W % 8 == 0 and even H, whose
 * slabs of G planes are whole 16-byte chunks run on the streaming kernels when every tensor is 16-byte aligned
 * (csrc/rk3d_16.hip); everything else runs on the per-plane kernels at 16-bit storage.  No BatchNorm-fused and no two-phase form exists for these types. */
int rk3d_forward_bf16_sf32(const void* x, const float* shift, void* y,
                           int N, int T, int C, int H, int W,
                           int stride_T, int stride_H, int stride_W,
                           int pad_T, int pad_H, int pad_W,
                           int quantize, rk_stream_t stream);
int rk3d_forward_f16_sf32(const void* x, const float* shift, void* y,
                          int N, int T, int C, int H, int W,
                          int stride_T, int stride_H, int stride_W,
                          int pad_T, int pad_H, int pad_W,
                          int quantize, rk_stream_t stream);
int rk3d_backward_bf16_sf32(const void* x, const float* shift, const void* gy,
                            void* gx, float* gshift,
                            int N, int T, int C, int H, int W,
                            int stride_T, int stride_H, int stride_W,
                            int pad_T, int pad_H, int pad_W,
                            int normalize_grad, float normalize_t_factor, int quantize,
                            void* workspace, size_t workspace_bytes, rk_stream_t stream);
int rk3d_backward_f16_sf32(const void* x, const float* shift, const void* gy,
                           void* gx, float* gshift,
                           int N, int T, int C, int H, int W,
                           int stride_T, int stride_H, int stride_W,
                           int pad_T, int pad_H, int pad_W,
                           int normalize_grad, float normalize_t_factor, int quantize,
                           void* workspace, size_t workspace_bytes, rk_stream_t stream);
/* 1 when the streaming 16-bit kernels (either stride class) take the configuration (elem_size must be 2), pointer alignment aside, else 0.  A
 * pure host predicate, no device call: the Python layer routes autocast activations to the entry points above where it
 * says 1 and keeps the fp32 operator between two casts elsewhere. */
int rk3d_sf32_streams(int N, int T, int C, int H, int W,
                      int stride_T, int stride_H, int stride_W,
                      int pad_T, int pad_H, int pad_W, int quantize, int elem_size);

/* ------------------------------------------------------------------------- 2D
 * Replaces rubiks2d_forward (cuda_src/rubiks.cpp:44-67) + rubiks2d_forward_cuda
 * (rubiks2d_kernels.cu:408-432) + K6 (:94-145).  The reference dispatches
 * float/double/half (AT_DISPATCH_FLOATING_TYPES_AND_HALF); bf16 is an addition.
 * f16/bf16 compute in fp32 and round once on store. */
#define RK_DECL_2D(SFX, TYPE)                                                              \
    int rk2d_forward_##SFX(const TYPE* x, const TYPE* shift, TYPE* y,                      \
                           int N, int C, int H, int W,                                     \
                           int stride_H, int stride_W, int pad_H, int pad_W,               \
                           int quantize, rk_stream_t stream);                              \
    int rk2d_backward_##SFX(const TYPE* gy, const TYPE* x, const TYPE* shift,              \
                            TYPE* gx, TYPE* gshift,                                        \
                            int N, int C, int H, int W,                                    \
                            int stride_H, int stride_W, int pad_H, int pad_W,              \
                            int normalize_grad, int enable_shift_grad, int quantize,       \
                            void* workspace, size_t workspace_bytes, rk_stream_t stream);

/* rk2d_backward_* replaces rubiks2d_backward (cuda_src/rubiks.cpp:94-155): K7 partials
 * (rubiks2d_kernels.cu:147-266) + addmv row-sum (rubiks.cpp:140-143) + K9 normalise
 * (:381-397) when enable_shift_grad, then K8 (:269-379).  With enable_shift_grad == 0
 * gshift is left untouched, as in the reference.  f16 / bf16 pointers are uint16_t
 * bit patterns, passed as void*. */
RK_DECL_2D(f32, float)
RK_DECL_2D(f64, double)
RK_DECL_2D(f16, void)
RK_DECL_2D(bf16, void)
#undef RK_DECL_2D

/* 16-bit activations next to an fp32 shift table (what torch.autocast hands the operator: bf16 / f16 activations,
 * fp32 nn.Parameter).  The reference instantiates K6-K9 at ONE scalar type (rubiks2d_kernels.cu:113-114 reads the
 * shift in the tensor's type), so an autocast caller of it must round the parameter to 16 bits first; these entry
 * points keep the shift, everything derived from it (floor / remainder, the 1e-7 integer test of :189, the quantize
 * positions of :117-118) and d(shift) in fp32, exactly as rk2d_*_f32 evaluate them.  Same workspace as rk2d_backward_*. */
#define RK_DECL_2D_SF32(SFX)                                                                \
    int rk2d_forward_##SFX##_sf32(const void* x, const float* shift, void* y,              \
                                  int N, int C, int H, int W,                              \
                                  int stride_H, int stride_W, int pad_H, int pad_W,        \
                                  int quantize, rk_stream_t stream);                       \
    int rk2d_backward_##SFX##_sf32(const void* gy, const void* x, const float* shift,      \
                                   void* gx, float* gshift,                                \
                                   int N, int C, int H, int W,                             \
                                   int stride_H, int stride_W, int pad_H, int pad_W,       \
                                   int normalize_grad, int enable_shift_grad, int quantize, \
                                   void* workspace, size_t workspace_bytes, rk_stream_t stream);
RK_DECL_2D_SF32(f16)
RK_DECL_2D_SF32(bf16)
#undef RK_DECL_2D_SF32

size_t rk2d_backward_workspace_bytes(int N, int C, int H, int W,
                                     int stride_H, int stride_W, int pad_H, int pad_W,
                                     int elem_size);

/* Training fusion for the 2-D operator (round 5; the -aq blocks of rubiksnet/backbone.py:129-131 with models.py:71-79's
 * RubiksShift2D): the shift applied to relu(bn2(z)) = max(a z + b, 0) without the activation being stored.
 *   forward : y = shift2d(round(max(a z + b, 0))); ab [2][C] = the affine map of bn2's training forward
 *             (rk_bn_stats_finish_* / rk_bn_finish_tiles_f32).
 *   backward: dz = d(bn2's output) = d(x) of the shift masked by the ReLU; gshift [2][C] (K9 applied when normalize_grad);
 *             bn2's backward constants k12 [2][C] = (sum dz, sum dz zhat) / count, d(gamma), d(beta): what
 *             rk_bn_bwd_dx_pre_* needs to finish bn2's d(x) in one pass.  abmi [C][4] = (a, b, mean, invstd).
 * Shift table and d(shift) in fp32 (as rk2d_*_sf32).  RK_ERR_UNSUPPORTED (nothing launched) when no fused kernel takes the
 * configuration: quantize on, or fp32 planes the LDS-DMA kernels stream (stride 1, pad 0, W % 4 == 0 other than 14 x 14 --
 * normalise pass + streaming kernel is the faster pair there), or a shape only the column kernels take with RK_COLUMN=0;
 * the caller then normalises with rk_bn_apply_affine_* and calls the plain entry points.  Fused today: 14 x 14 planes
 * (fp32 / bf16), bf16 56 x 56 / 112 x 112 (raw-plane kernels), bf16 28 x 28 (register-staged), and every other stride /
 * padding / plane through the column kernels (the stride-2 layers, 7 x 7). */
/* 1 when a fused kernel takes this configuration at this storage size (4 = fp32, 2 = bf16), else 0 */
int rk2d_bn_fused_shape(int N, int C, int H, int W, int sH, int sW, int pH, int pW, int elem_size);
size_t rk2d_backward_bn_workspace_bytes(int N, int C, int H, int W, int stride_H, int stride_W, int pad_H, int pad_W);
int rk2d_forward_bn_f32(const float* z, const float* ab, const float* shift, float* y, int N, int C, int H, int W,
                        int stride_H, int stride_W, int pad_H, int pad_W, int quantize, rk_stream_t stream);
int rk2d_forward_bn_bf16_sf32(const void* z, const float* ab, const float* shift, void* y, int N, int C, int H, int W,
                              int stride_H, int stride_W, int pad_H, int pad_W, int quantize, rk_stream_t stream);
int rk2d_backward_bn_f32(const float* gy, const float* z, const float* abmi, const float* shift, float* dz, float* gshift,
                         float* k12, float* dgamma, float* dbeta, int N, int C, int H, int W, int stride_H, int stride_W,
                         int pad_H, int pad_W, int normalize_grad, int quantize, void* workspace, size_t workspace_bytes,
                         rk_stream_t stream);
int rk2d_backward_bn_bf16_sf32(const void* gy, const void* z, const float* abmi, const float* shift, void* dz, float* gshift,
                               float* k12, float* dgamma, float* dbeta, int N, int C, int H, int W, int stride_H,
                               int stride_W, int pad_H, int pad_W, int normalize_grad, int quantize, void* workspace,
                               size_t workspace_bytes, rk_stream_t stream);

/* ------------------------------------------------------------ temporal 3-tap
 * The device half of AttentionShift (rubiksnet/attention_shift.py:32-39): the
 * per-channel 3-tap temporal filter the reference runs as transpose -> grouped
 * conv1d(groups=C*H*W) -> transpose -> contiguous.  `taps` is the [C,3] tensor (fp32;
 * fp64 for the _f64 entry points) of already soft-maxed weights (attention_shift.py:29-30, computed on the host side
 * in PyTorch so autograd owns std/softmax); x, y are [NT, C, H, W] with
 * NT = n_batch * n_segment; zero padding in t.
 *   y[n,t] = taps[c,0]*x[n,t-1] + taps[c,1]*x[n,t] + taps[c,2]*x[n,t+1]
 * backward: gx = adjoint; gtaps[C,3] (same type as taps) = sum over n,t,h,w of gy * x[t-1+k]. */
#define RK_DECL_TAP(SFX, TYPE, TAPT)                                                       \
    int rk_tshift3_forward_##SFX(const TYPE* x, const TAPT* taps, TYPE* y,                 \
                                 int NT, int n_segment, int C, int HW, rk_stream_t stream);\
    int rk_tshift3_backward_##SFX(const TYPE* gy, const TYPE* x, const TAPT* taps,         \
                                  TYPE* gx, TAPT* gtaps,                                   \
                                  int NT, int n_segment, int C, int HW,                    \
                                  void* workspace, size_t workspace_bytes,                 \
                                  rk_stream_t stream);
RK_DECL_TAP(f32, float, float)
RK_DECL_TAP(f64, double, double)
RK_DECL_TAP(f16, void, float)
RK_DECL_TAP(bf16, void, float)
#undef RK_DECL_TAP

size_t rk_tshift3_backward_workspace_bytes(int NT, int n_segment, int C, int HW);
/* The -aq block's training-mode bn1 + ReLU folded into its temporal filter (backbone.py:129 `out = relu(bn1(x))` feeding
 * attention_shift.py:29-39): y = tshift3(relu(a[c] x + b[c])), ab = [2][C] from rk_bn_stats_finish_*; backward: gy -> dz =
 * d(relu(a x + b)) masked by the ReLU (x = the block input BEFORE bn1), gtaps, and bred [C][NT / n_segment] = (sum dz,
 * sum dz xhat) per (channel, clip) for rk_bn_bwd_finish_tiles_f32 (tiles = NT / n_segment) + rk_bn_bwd_dx_pre_*. */
int rk_tshift3_bn_forward_f32(const float* x, const float* taps, const float* ab, float* y, int NT, int S, int C, int HW,
                              rk_stream_t stream);
int rk_tshift3_bn_forward_bf16(const void* x, const float* taps, const float* ab, void* y, int NT, int S, int C, int HW,
                               rk_stream_t stream);
int rk_tshift3_bn_backward_f32(const float* gy, const float* x, const float* taps, const float* ab, const float* save_mean,
                               const float* save_invstd, float* dz, float* gtaps, void* bred, int NT, int S, int C, int HW,
                               void* ws, size_t ws_bytes, rk_stream_t stream);
int rk_tshift3_bn_backward_bf16(const void* gy, const void* x, const float* taps, const float* ab, const float* save_mean,
                                const float* save_invstd, void* dz, float* gtaps, void* bred, int NT, int S, int C, int HW,
                                void* ws, size_t ws_bytes, rk_stream_t stream);

/* The same with BatchNorm's backward constants finished inside the launch (the two sums travel as granules next to the tap
 * sums): k12 [2][C] = (sum dz, sum dz xhat) / (NT HW), dgamma / dbeta [C] -- what rk_bn_bwd_finish_tiles_f32 made of bred. */
size_t rk_tshift3_bn_backward_fin_workspace_bytes(int NT, int n_segment, int C, int HW);
int rk_tshift3_bn_backward_fin_f32(const float* gy, const float* x, const float* taps, const float* ab, const float* save_mean,
                                   const float* save_invstd, float* dz, float* gtaps, float* k12, float* dgamma, float* dbeta,
                                   int NT, int S, int C, int HW, void* ws, size_t ws_bytes, rk_stream_t stream);
int rk_tshift3_bn_backward_fin_bf16(const void* gy, const void* x, const float* taps, const float* ab, const float* save_mean,
                                    const float* save_invstd, void* dz, float* gtaps, float* k12, float* dgamma, float* dbeta,
                                    int NT, int S, int C, int HW, void* ws, size_t ws_bytes, rk_stream_t stream);

/* Downsampling -aq blocks (the activation also feeds the stride-2 projecting shortcut, backbone.py:98-104): the shortcut reads
 * rk_bn_relu_gather2_* (relu(a x + b) at the even pixels, ab = [2][C]); its gradient gsmall [NT, C, H/2, W/2] joins
 * d(activation) inside the temporal filter's backward, before the ReLU mask and BatchNorm's sums. */
int rk_bn_relu_gather2_f32(const float* x, const float* ab, float* xs, int F, int C, int H, int W, rk_stream_t stream);
int rk_bn_relu_gather2_bf16(const void* x, const float* ab, void* xs, int F, int C, int H, int W, rk_stream_t stream);
int rk_tshift3_bn_backward_fork_f32(const float* gy, const float* x, const float* taps, const float* ab, const float* save_mean,
                                    const float* save_invstd, const float* gsmall, float* dz, float* gtaps, float* k12,
                                    float* dgamma, float* dbeta, int NT, int S, int C, int H, int W, void* ws, size_t ws_bytes,
                                    rk_stream_t stream);
int rk_tshift3_bn_backward_fork_bf16(const void* gy, const void* x, const float* taps, const float* ab, const float* save_mean,
                                     const float* save_invstd, const void* gsmall, void* dz, float* gtaps, float* k12,
                                     float* dgamma, float* dbeta, int NT, int S, int C, int H, int W, void* ws, size_t ws_bytes,
                                     rk_stream_t stream);

/* The [C,3] half of AttentionShift (attention_shift.py:29-30): taps = softmax((weight / (std(weight, dim=1) + 1e-6)) / T)
 * over the three taps of a channel (std unbiased), and its backward (gweight from gtaps).  fp32; T is the module's
 * one-element device tensor (no host read); one launch each instead of ~15 + ~25 PyTorch kernels per layer. */
int rk_soft_taps_forward_f32(const float* weight, const float* T, float* taps, int C, rk_stream_t stream);
int rk_soft_taps_backward_f32(const float* weight, const float* T, const float* taps, const float* gtaps, float* gweight,
                              int C, rk_stream_t stream);
/* Every AttentionShift layer of a network in one launch each way.  jobs: device array of n records {const float* weight;
 * const float* T; int64 off; int32 C; int32 pad} (32 bytes); layer i's taps / gtaps / gweight are rows off .. off + C of
 * concatenated [sum C][3] fp32 buffers; max_c = the largest C.  Same arithmetic as the one-layer calls (bit-identical). */
int rk_soft_taps_many_forward_f32(const void* jobs, int n, float* taps, int max_c, rk_stream_t stream);
int rk_soft_taps_many_backward_f32(const void* jobs, int n, const float* taps, const float* gtaps, float* gweight, int max_c,
                                   rk_stream_t stream);

/* ---- BatchNorm2d (+ ReLU) of the backbone blocks -- widening row f3 of SURVEY 8(f) ----------------
 * Replaces the reference's nn.BatchNorm2d followed by nn.ReLU(inplace=True)
 * (rubiksnet/backbone.py:50-53 BN2d; :129 relu(bn1(x)), :131 relu(bn2(conv2(.))), :196 relu(bn_last(x))),
 * i.e. torch.nn.functional.batch_norm + relu on an NCHW tensor.
 *   x, y, dy, dx : [F, C, P] contiguous (F = N*T frames, P = H*W), f32 or bf16; parameters / statistics are f32.
 *   training != 0: batch statistics (biased variance for the normalisation); save_mean / save_invstd [C] are
 *                  written for the backward; running_mean / running_var (both or neither) are updated as
 *                  r = (1 - momentum) r + momentum * stat, with the UNBIASED variance, as torch does.
 *                  Needs ws of rk_bn_workspace_bytes(F, C, P) bytes.
 *   training == 0: y = relu?(gamma (x - running_mean) / sqrt(running_var + eps) + beta); save_*, ws unused.
 *   backward     : gradients of the training-mode forward; the ReLU mask is recomputed from x.  dskip (or NULL): a
 *                  gradient of the same shape added into dx -- the branch of the block's identity shortcut
 *                  (backbone.py:130), which autograd would otherwise sum with a separate elementwise pass.
 *   relu != 0 fuses the ReLU (and its backward).                                                         */
size_t rk_bn_workspace_bytes(int F, int C, int P);
#define RK_DECL_BN(SFX, CTYPE)                                                                                   \
    int rk_bn_relu_forward_##SFX(const CTYPE* x, const float* gamma, const float* beta, float* running_mean,     \
                                 float* running_var, float* save_mean, float* save_invstd, CTYPE* y, int F,      \
                                 int C, int P, float eps, float momentum, int relu, int training, void* ws,     \
                                 size_t ws_bytes, rk_stream_t stream);                                           \
    /* training forward that also does nn.BatchNorm2d's `num_batches_tracked += 1` (int64 device scalar, may be   \
     * NULL) inside the launch instead of a kernel of its own */                                                  \
    int rk_bn_relu_forward_counted_##SFX(const CTYPE* x, const float* gamma, const float* beta,                  \
                                         float* running_mean, float* running_var, float* save_mean,              \
                                         float* save_invstd, CTYPE* y, int F, int C, int P, float eps,           \
                                         float momentum, int relu, long long* num_batches_tracked, void* ws,    \
                                         size_t ws_bytes, rk_stream_t stream);                                   \
    int rk_bn_relu_backward_##SFX(const CTYPE* dy, const CTYPE* x, const float* gamma, const float* beta,        \
                                  const float* save_mean, const float* save_invstd, const CTYPE* dskip,          \
                                  CTYPE* dx, float* dgamma, float* dbeta, int F, int C, int P, int relu,         \
                                  void* ws, size_t ws_bytes, rk_stream_t stream);
RK_DECL_BN(f32, float)
RK_DECL_BN(bf16, void)
#undef RK_DECL_BN

/* ---- 1x1 convolution on NCHW activations -- widening row f1 of SURVEY 8(f), unfused half -----------
 * Replaces torch.nn.functional.conv2d with a 1x1 kernel, stride 1, no bias (rubiksnet/backbone.py:44-45
 * Conv1x1; conv2 / conv3 / stride-1 shortcuts of every block, :87-104) and its two gradients.
 *   rk_pw_gemm_*  : Y[f] = A X[f] (+ R[f]), X [F,K,P], Y / R [F,M,P] fp32 or bf16 storage (fp32 arithmetic),
 *                   A always fp32 (under bf16 autocast the weight is used as it is, no cast), P % 4 == 0.
 *                   forward: A = weight [M=Cout][K=Cin], a_is_mk = 1; R = the block's shortcut
 *                   (backbone.py:134 `out += shortcut`) or NULL;
 *                   d(input): A = weight read as [K=Cout][M=Cin], a_is_mk = 0, X = d(output), R = NULL.
 *   rk_pw_wgrad_* : d(weight)[M][K] (fp32) = sum_f dY[f] X[f]^T, dY [F,M,P], X [F,K,P]; ws of
 *                   rk_pw_wgrad_workspace_bytes() bytes holds per-chunk partials (summed in a fixed order).   */
int rk_pw_gemm_f32(const float* A, const float* X, const float* R, float* Y, int F, int K, int M, int P,
                   int a_is_mk, rk_stream_t stream);
int rk_pw_gemm_bf16(const float* A, const void* X, const void* R, void* Y, int F, int K, int M, int P,
                    int a_is_mk, rk_stream_t stream);
/*   bf16 activations, second generation (rk_pw16.hip): the weight is packed ONCE per version into bf16 MFMA-fragment
 *   order and the GEMM streams X by LDS-DMA, every row of a 128-pixel tile in one workgroup (X crosses HBM once).
 *   rk_pw_packed_bytes(rows, depth): bytes of a packed operand;
 *   rk_pw_pack_bf16: W [Cout][Cin] fp32 -> `fwd` (rows Cout, depth Cin: forward) and / or `bwd` (rows Cin, depth
 *                   Cout: W^T for d(input)); either may be NULL;
 *   rk_pw_gemm_packed_bf16: Y[f] = A X[f] (+ R[f]) with A packed (M rows, depth K); R may be NULL or Y itself.  R [F,M,P]
 *                   is streamed through the same LDS-DMA ring as X (identity-weighted chunks after X's: exact), so both
 *                   F*K*P*2 and F*M*P*2 must stay below 2^31 bytes (RK_ERR_BAD_DIMS otherwise). */
size_t rk_pw_packed_bytes(int rows, int depth);
int rk_pw_pack_bf16(const float* W, int Cout, int Cin, void* fwd, void* bwd, rk_stream_t stream);
/* The same for n weights in one launch (once per train step, pointwise.prepacked): `jobs` = device array of n 40-byte
 * records {const float* W; int64_t fwd_off, bwd_off; int32_t Cout, Cin, nf, nb}: the two images go to base + fwd_off /
 * base + bwd_off (multiples of 16), nf / nb = rk_pw_packed_bytes(..) / 16 of each; max_units = max over jobs of nf + nb. */
int rk_pw_pack_many_bf16(const void* jobs, int n, void* base, int max_units, rk_stream_t stream);
/* bf16 activations on planes without a 16-byte unit in a row (P % 4 != 0, P <= 64: the 7x7 planes of layer4, backbone.py:44-45
 * on [NT, 576, 7, 7]; rk_pw16_odd.hip): a workgroup per frame (a whole frame [K][P] IS contiguous and aligned).
 *   rk_pw_odd16_supported(F, K, M, P): 1 when the GEMM takes [F, K -> M, P] (K % 32 == 0, M % 8 == 0, P <= 64, LDS);
 *   rk_pw_gemm_packed_odd_bf16: Y[f] = A X[f] (+ R[f]), A packed by rk_pw_pack_bf16 (M rows, depth K); tensors 16-byte aligned;
 *   rk_pw_wgrad_odd16_bf16: dW [M][K] fp32 = sum_f dY[f] X[f]^T (K % 8 == M % 8 == 0); ws of .._workspace_bytes(). */
/* The 3x3 / stride-2 / pad-1 stem (backbone.py:154) under bf16 autocast (rk_stem16.hip): fp32 clip X [F, 3, Hin, Win] and fp32
 * weight W [Cout][3][3][3], both rounded to bf16 as autocast rounds them, Y / dY [F, Cout, Hin/2, Win/2] bf16, dW fp32.
 * Win % 32 == 0, Hin % 16 == 0, Cout <= 128 (rk_stem16_supported). */
int rk_stem16_supported(int F, int Cin, int Cout, int Hin, int Win);
/* out [planes][H][W] bf16 = main (NULL: zeros) + small [planes][H/2][W/2] scattered to the even (h, w) -- the gradient of the
 * stride-2 gather in front of a projecting shortcut (backbone.py:98-104) joined to the other consumer's gradient in one pass. */
int rk_scatter2x2_add_bf16(const void* main, const void* small, void* out, long long planes, int H, int W, rk_stream_t stream);
int rk_stem_conv3x3s2_bf16out(const float* W, const float* X, void* Y, int F, int Cin, int Cout, int Hin, int Win, rk_stream_t stream);
size_t rk_stem_wgrad16_workspace_bytes(int F, int Cin, int Cout, int Hin, int Win);
int rk_stem_wgrad3x3s2_bf16(const void* dY, const float* X, float* dW, int F, int Cin, int Cout, int Hin, int Win, void* workspace,
                            size_t workspace_bytes, rk_stream_t stream);
int rk_pw_odd16_supported(int F, int K, int M, int P);
int rk_pw_gemm_packed_odd_bf16(const void* Apk, const void* X, const void* R, void* Y, int F, int K, int M, int P, rk_stream_t stream);
size_t rk_pw_wgrad_odd16_workspace_bytes(int F, int K, int M, int P);
int rk_pw_wgrad_odd16_bf16(const void* dY, const void* X, float* dW, int F, int K, int M, int P, void* workspace,
                           size_t workspace_bytes, rk_stream_t stream);
int rk_pw_gemm_packed_bf16(const void* Apk, const void* X, const void* R, void* Y, int F, int K, int M, int P,
                           rk_stream_t stream);
/* training (round 5): the same GEMM + the tile statistics of Y for the BatchNorm that consumes it (backbone.py:50-53 after
 * :44-45 under autocast): stats float4 [M][tiles] = (pivot, sum(y - pivot), sum((y - pivot)^2), columns) per 64 columns of
 * the values as stored, tiles = rk_pw16_stat_tiles(F, P); finished by rk_bn_finish_tiles_f32. */
int rk_pw16_stat_tiles(int F, int P);
int rk_pw_gemm_packed_stats_bf16(const void* Apk, const void* X, const void* R, void* Y, int F, int K, int M, int P,
                                 void* stats, int tiles, rk_stream_t stream);
/*   rk_pw_wgrad16_bf16: d(weight)[M][K] (fp32) = sum_f dY[f] X[f]^T for bf16 dY [F,M,P], X [F,K,P] (P % 4 == 0, P >= 8):
 *                   both operands DMA'd fragment-wise, output tiles of up to 160 x 160 per workgroup; ws of
 *                   rk_pw_wgrad16_workspace_bytes() bytes (per-split partial matrices, summed in a fixed order). */
size_t rk_pw_wgrad16_workspace_bytes(int F, int K, int M, int P);
int rk_pw_wgrad16_bf16(const void* dY, const void* X, float* dW, int F, int K, int M, int P, void* ws, size_t ws_bytes,
                       rk_stream_t stream);
/*   rk_pw_gemm_fused_f32: inference form, Y[f] = epi(A pro(X[f])) (+ R[f]) with
 *                   pro: x' = relu?(ka[k] x + kb[k]) per input channel  (relu(bn1(x)) feeding conv2, backbone.py:129-131)
 *                   epi: y  = relu?(ma[m] y + mb[m]) per output channel (relu(bn2(conv2(.))), BatchNorm in eval mode:
 *                   a = gamma / sqrt(running_var + eps), b = beta - running_mean * a).  NULL pairs switch a stage off. */
/* eval-mode BatchNorm2d folded to y = a x + b per channel (a = gamma / sqrt(running_var + eps), b = beta -
 * running_mean a): the (ka, kb) / (ma, mb) arrays of the fused entry points below, in one launch. */
int rk_bn_fold_f32(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                   float* a, float* b, int C, rk_stream_t stream);
/* the same fold for n BatchNorm layers in one launch: jobs = device array of {gamma*, beta*, running_mean*, running_var*,
 * int64 off, int32 C, float eps} (48 bytes); ab = [2][total] fp32, layer i's a / b at [off, off + C) of each half */
int rk_bn_fold_many_f32(const void* jobs, int n, float* ab, long long total, int max_c, rk_stream_t stream);
int rk_pw_gemm_fused_f32(const float* A, const float* X, const float* R, float* Y, int F, int K, int M, int P,
                         int a_is_mk, const float* ka, const float* kb, int relu_in, const float* ma,
                         const float* mb, int relu_out, rk_stream_t stream);
/*   rk_stem_conv3x3s2_f32: the backbone's first layer (backbone.py:154, Conv3x3(3, width, stride=2), no bias) on the
 *                   same GEMM with the im2col gathered on the fly: W [Cout][Cin][3][3], X [F,Cin,Hin,Win],
 *                   Y [F,Cout,Hin/2,Win/2]; Hin even, Win % 8 == 0, 9 Cin <= 64.                              */
int rk_stem_conv3x3s2_f32(const float* W, const float* X, float* Y, int F, int Cin, int Cout, int Hin, int Win,
                          rk_stream_t stream);
/* d(weight) of that convolution: dW [Cout][Cin][3][3] (fp32) from dY [F, Cout, Hin/2, Win/2] and X [F, Cin, Hin, Win];
 * workspace of rk_pw_wgrad_workspace_bytes(F, 9 * Cin, Cout, (Hin/2) * (Win/2)) bytes.  Replaces the d(weight) half of
 * conv2d's backward for the stem (backbone.py:154); the stem needs no d(input). */
int rk_stem_wgrad3x3s2_f32(const float* dY, const float* X, float* dW, int F, int Cin, int Cout, int Hin, int Win,
                           void* workspace, size_t workspace_bytes, rk_stream_t stream);
/* 1x1 / stride-2 / no-bias convolution (the projecting shortcut of a downsampling block, backbone.py:98-104) on the
 * same GEMM kernels: forward (the streamed operand read at stride 2), d(input) (results scattered to the even
 * positions, zeros elsewhere: every element of dX is written) and d(weight).  W [Cout][Cin] fp32, X / dX
 * [F, Cin, Hin, Win], Y / dY [F, Cout, Hin/2, Win/2]; Hin even, Win % 8 == 0, Cin and Cout even; the d(weight)
 * workspace is rk_pw_wgrad_workspace_bytes(F, Cin, Cout, (Hin/2) * (Win/2)) bytes. */
int rk_pw_s2_forward_f32(const float* W, const float* X, float* Y, int F, int Cin, int Cout, int Hin, int Win,
                         rk_stream_t stream);
int rk_pw_s2_forward_fused_f32(const float* W, const float* X, float* Y, int F, int Cin, int Cout, int Hin, int Win,
                               const float* ka, const float* kb, int relu_in, rk_stream_t stream);   /* inference: x' =
                               relu?(ka[k] x + kb[k]) on the streamed operand, as rk_pw_gemm_fused_f32's prologue */
int rk_pw_s2_dgrad_f32(const float* W, const float* dY, float* dX, int F, int Cin, int Cout, int Hin, int Win,
                       rk_stream_t stream);
int rk_pw_s2_wgrad_f32(const float* dY, const float* X, float* dW, int F, int Cin, int Cout, int Hin, int Win,
                       void* workspace, size_t workspace_bytes, rk_stream_t stream);
size_t rk_pw_wgrad_workspace_bytes(int F, int K, int M, int P);
int rk_pw_wgrad_f32(const float* dY, const float* X, float* dW, int F, int K, int M, int P, void* ws,
                    size_t ws_bytes, rk_stream_t stream);
int rk_pw_wgrad_bf16(const void* dY, const void* X, float* dW, int F, int K, int M, int P, void* ws,
                     size_t ws_bytes, rk_stream_t stream);

/* 1x1 convolutions on planes with H * W % 4 != 0 -- the 7x7 planes of layer4 (rubiksnet/backbone.py:164), which the
 * kernels above cannot take (a row of 49 floats is not 16-byte aligned): the streamed operand goes through LDS as whole
 * 16-channel frame chunks (contiguous and aligned), see k_pw_gemm_odd.  37 <= P <= 64, K % 4 == 0, fp32.
 *   rk_pw_gemm_odd_f32     : Y[f] = A X[f] (+ R[f]), forward (a_is_mk = 1) / d(input) (a_is_mk = 0)
 *   rk_pw_wgrad_odd_f32    : d(weight); workspace rk_pw_wgrad_odd_workspace_bytes(F, K, M, P)
 *   rk_pw_s2_*_odd_f32     : the 1x1 / stride-2 projecting shortcut onto such planes (14x14 -> 7x7, backbone.py:98-104):
 *                            forward, d(input) (every element of dX written) and d(weight); Hin, Win even. */
int rk_pw_gemm_odd_f32(const float* A, const float* X, const float* R, float* Y, int F, int K, int M, int P,
                       int a_is_mk, rk_stream_t stream);
size_t rk_pw_wgrad_odd_workspace_bytes(int F, int K, int M, int P);
int rk_pw_wgrad_odd_f32(const float* dY, const float* X, float* dW, int F, int K, int M, int P, void* ws,
                        size_t ws_bytes, rk_stream_t stream);
int rk_pw_s2_forward_odd_f32(const float* W, const float* X, float* Y, int F, int Cin, int Cout, int Hin, int Win,
                             rk_stream_t stream);
int rk_pw_s2_dgrad_odd_f32(const float* W, const float* dY, float* dX, int F, int Cin, int Cout, int Hin, int Win,
                           rk_stream_t stream);
int rk_pw_s2_wgrad_odd_f32(const float* dY, const float* X, float* dW, int F, int Cin, int Cout, int Hin, int Win,
                           void* ws, size_t ws_bytes, rk_stream_t stream);

/* ---- training-mode fusion of the block's BatchNorms into the 1x1 GEMMs -- rows f1 / f3 of SURVEY 8(f) ----------
 * The reference block (rubiksnet/backbone.py:123-135) is
 *     a1 = relu(bn1(x)); z = conv2(a1); a2 = relu(bn2(z)); s = as3(a2); out = conv3(s) + shortcut
 * with nn.BatchNorm2d in training mode (:50-53).  Unfused, every BatchNorm is a statistics pass + a normalise pass
 * forward and a reduction pass + a d(x) pass backward.  Here
 *   - the STATISTICS pass rides on the epilogue of the GEMM that produces the tensor (rk_pw_gemm_stats_f32; the stem:
 *     rk_stem_conv3x3s2_stats_f32): one float4 (pivot, sum(y - pivot), sum((y - pivot)^2), -) per (channel, 128-column
 *     wave tile), [M][rk_pw_tiles(F, P)], finished by rk_bn_finish_tiles_f32 into save_mean / save_invstd, the affine map
 *     (a, b) of y = a x + b, and nn.BatchNorm2d's running statistics / num_batches_tracked;
 *   - relu(bn1(x)) is never stored: it is the PROLOGUE (ka, kb, relu_in) of conv2's forward, of the strided shortcut's
 *     forward (rk_pw_s2_forward_fused_f32) and of their d(weight) kernels (rk_pw_wgrad_pro_f32, rk_pw_s2_wgrad_pro_f32);
 *   - the backward REDUCTION pass of bn1 rides on conv2's d(input) GEMM (rk_pw_gemm_bnbwd_f32): the result tile is masked
 *     with [a x + b > 0] and its (sum dz, sum dz xhat) go out as float2 per (channel, tile); rk_bn_bwd_finish_tiles_f32
 *     turns them into k1, k2, d(gamma), d(beta); rk_bn_bwd_dx_pre_f32 is the remaining d(x) pass (+ the identity
 *     shortcut's gradient);
 *   - rk_bn_apply_affine_f32: y = relu?(a x + b) with the finished map (bn2 in front of the shift);
 *   - rk_bn_tile_stats_f32: the same tile statistics for a tensor no GEMM epilogue produced them for.
 * All fp32, P % 4 == 0; results match torch.nn.functional.batch_norm + relu (+ conv2d) and their autograd gradients. */
/*   - relu(bn2(z)) is never stored either (f1 "and/or the preceding ReLU(BN2(.))"): the shift kernels read z and normalise
 *     the landed planes in LDS (rk3d_forward_bn_f32); the backward (rk3d_backward_bn_f32) reads z for the x operand,
 *     masks d(activation) with the ReLU on the way out (dz) and reduces bn2's sum(dz), sum(dz zhat) next to the d(shift)
 *     partials: k12 [2][C], d(gamma), d(beta) come out of the same launch and rk_bn_bwd_dx_pre_f32 finishes d(z).
 *     abmi: [C][4] = (a, b, mean, invstd) as rk_bn_finish_tiles_f32 packs it.  Stride 1 / pad 0 planes with W % 4 == 0
 *     (56x56, 28x28, 112x112); RK_ERR_UNSUPPORTED otherwise (the caller normalises with rk_bn_apply_affine_f32). */
int rk3d_forward_bn_f32(const float* z, const float* abmi, const float* shift, float* y, int N, int T, int C, int H,
                        int W, int stride_T, int stride_H, int stride_W, int pad_T, int pad_H, int pad_W, int quantize,
                        rk_stream_t stream);
size_t rk3d_backward_bn_workspace_bytes(int N, int T, int C, int H, int W, int stride_T, int stride_H, int stride_W,
                                        int pad_T, int pad_H, int pad_W);
int rk3d_backward_bn_f32(const float* z, const float* abmi, const float* shift, const float* gy, float* dz, float* gshift,
                         float* k12, float* dgamma, float* dbeta, int N, int T, int C, int H, int W, int stride_T,
                         int stride_H, int stride_W, int pad_T, int pad_H, int pad_W, int normalize_grad, float t_factor,
                         int quantize, void* workspace, size_t workspace_bytes, rk_stream_t stream);
int rk_pw_tiles(int F, int P);
/* tiles of the training epilogues of ONE rk_pw_gemm_stats_f32 / rk_pw_gemm_bnbwd_f32 call with these arguments: the
 * second-generation fp32 kernels (rk_pw2.hip: v_mfma_f32_16x16x4_f32, no LDS) write one partial per 64 columns, the first
 * generation one per 128; rk_bn_finish_tiles_f32 tells the two apart from (tiles, count). */
int rk_pw_gemm_tiles(const float* A, int F, int K, int M, int P, int a_is_mk);
/* tuning / test hooks of the second-generation fp32 1x1 kernels: the operations of rk_pw_gemm_fused_f32 (prologue only) and
 * rk_pw_wgrad_pro_f32 with the kernel configuration given explicitly (<= 0 / < 0: the planner's choice).  rb: 16-row blocks
 * per wave (3, 4, 5); amode: 0 = A [M][K] by 16-byte loads, 1 = A [K][M] by dword loads, 2 = LDS image; inst: d(weight)
 * tile instance (rk_pw2.hip kWInst), stages: LDS ring depth (2, 3), splits: pixel splits.  RK_ERR_UNSUPPORTED: no instance. */
int rk_pw2_gemm_cfg_f32(const float* A, const float* X, const float* R, float* Y, int F, int K, int M, int P, int a_is_mk,
                        const float* ka, const float* kb, int relu_in, int rb, int amode, int ct, rk_stream_t stream);
/* rk_pw4.hip: the streaming GEMM of the shallow layers (54 -> 54 / 72 -> 72 channels; operand in registers, everything else
 * through a per-wave LDS-DMA record ring) regardless of the size threshold of the dispatch -- test / probe hook.
 * epi 0: Y = A relu?(ka x + kb)(X) (+ R); 1: + statistics tiles (stats [M][tiles] float4, as rk_pw_gemm_stats_f32);
 * 2: the BatchNorm-backward epilogue of rk_pw_gemm_bnbwd_f32 (bx, bpack [M][4], bred [M][tiles] float2); tiles =
 * ceil(F P / 64).  RK_ERR_UNSUPPORTED: no instance for (K, M). */
int rk_pw4_gemm_f32(const float* A, const float* X, const float* R, float* Y, int F, int K, int M, int P, int a_is_mk,
                    const float* ka, const float* kb, int relu_in, int epi, void* stats, const float* bx, const float* bpack,
                    void* bred, int tiles, rk_stream_t stream);
size_t rk_pw2_wgrad_workspace_bytes(int F, int K, int M, int P);
int rk_pw2_wgrad_cfg_f32(const float* dY, const float* X, float* dW, int F, int K, int M, int P, void* ws, size_t ws_bytes,
                         const float* ka, const float* kb, int relu_in, int inst, int stages, int splits, rk_stream_t stream);
/* Operand layout of the two training entry points: rk_pw_gemm_stats_f32 is the FORWARD of conv2 / conv3 and is instantiated
 * for a_is_mk = 1 (A = the weight [M][K]); rk_pw_gemm_bnbwd_f32 is conv2's D(INPUT) and is instantiated for a_is_mk = 0 (A =
 * the weight read as [K][M]).  Those are the layouts rubiksnet_amd/train_block.py uses; the other two combinations have
 * instances only in the first-generation kernel and return RK_ERR_UNSUPPORTED for shapes the later generations take
 * (M <= 224 rows, or the 257..288-row layers): not a layout the training block can produce. */
int rk_pw_gemm_stats_f32(const float* A, const float* X, const float* R, float* Y, int F, int K, int M, int P,
                         int a_is_mk, const float* ka, const float* kb, int relu_in, void* stats, int tiles,
                         rk_stream_t stream);
int rk_stem_conv3x3s2_stats_f32(const float* W, const float* X, float* Y, int F, int Cin, int Cout, int Hin, int Win,
                                void* stats, int tiles, rk_stream_t stream);
int rk_pw_gemm_bnbwd_f32(const float* A, const float* dY, const float* R, float* dZ, int F, int K, int M, int P,
                         int a_is_mk, const float* x, const float* abmi /* [M][4] = (a, b, mean, invstd) */, void* bred,
                         int tiles, rk_stream_t stream);
int rk_pw_wgrad_pro_f32(const float* dY, const float* X, float* dW, int F, int K, int M, int P, const float* ka,
                        const float* kb, int relu_in, void* ws, size_t ws_bytes, rk_stream_t stream);
int rk_pw_s2_wgrad_pro_f32(const float* dY, const float* X, float* dW, int F, int Cin, int Cout, int Hin, int Win,
                           const float* ka, const float* kb, int relu_in, void* ws, size_t ws_bytes, rk_stream_t stream);
int rk_bn_finish_tiles_f32(const void* stats, int tiles, long long count, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float* save_mean, float* save_invstd, float* a,
                           float* b, float* abmi /* [C][4] packed copy, may be NULL */, int C, float eps, float momentum,
                           long long* num_batches_tracked, rk_stream_t stream);
int rk_bn_tile_stats_f32(const float* x, void* stats, int F, int C, int P, rk_stream_t stream);
int rk_bn_apply_affine_bf16(const void* x, const float* a, const float* b, void* y, int F, int C, int P, int relu,
                            rk_stream_t stream);
int rk_bn_apply_affine_f32(const float* x, const float* a, const float* b, float* y, int F, int C, int P, int relu,
                           rk_stream_t stream);
int rk_bn_bwd_finish_tiles_f32(const void* bred, int tiles, long long count, float* k12, float* dgamma, float* dbeta,
                               int C, rk_stream_t stream);
int rk_bn_bwd_dx_pre_f32(const float* dz, const float* x, const float* gamma, const float* save_mean,
                         const float* save_invstd, const float* k12, const float* skip, float* dx, int F, int C, int P,
                         rk_stream_t stream);
int rk_bn_bwd_dx_pre_bf16(const void* dz, const void* x, const float* gamma, const float* save_mean,
                          const float* save_invstd, const float* k12, const void* skip, void* dx, int F, int C, int P,
                          rk_stream_t stream);
/* the statistics half of the training forward alone: save_mean / save_invstd / ab [2][C] (y = a x + b), running statistics
 * and *num_batches_tracked as nn.BatchNorm2d's forward; ws of rk_bn_workspace_bytes() bytes */
int rk_bn_stats_finish_f32(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                           float* save_mean, float* save_invstd, float* ab, int F, int C, int P, float eps, float momentum,
                           long long* num_batches_tracked, void* ws, size_t ws_bytes, rk_stream_t stream);
int rk_bn_stats_finish_bf16(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                            float* save_mean, float* save_invstd, float* ab, int F, int C, int P, float eps, float momentum,
                            long long* num_batches_tracked, void* ws, size_t ws_bytes, rk_stream_t stream);
/* ... also leaving abmi [C][4] = (a, b, mean, invstd), the packed record rk2d_backward_bn_* reads (16-byte aligned) */
int rk_bn_stats_finish_abmi_f32(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                float* save_mean, float* save_invstd, float* ab, float* abmi, int F, int C, int P, float eps,
                                float momentum, long long* num_batches_tracked, void* ws, size_t ws_bytes, rk_stream_t stream);
int rk_bn_stats_finish_abmi_bf16(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                 float* save_mean, float* save_invstd, float* ab, float* abmi, int F, int C, int P, float eps,
                                 float momentum, long long* num_batches_tracked, void* ws, size_t ws_bytes, rk_stream_t stream);

/* ---- input side of the network on the device -- widening row f4 of SURVEY 8(f) ----------------------
 * Replaces, per batch instead of per sample on CPU workers, the reference's transform tail
 * Stack -> ToTorchFormatTensor(div=True) -> GroupNormalize (rubiksnet/transforms.py:329-363, :66-79; wired up
 * in scripts/test_models.py:136-143): hwc [nclips, H, W, CS] uint8 (CS = 3 * frames, channel-interleaved RGB
 * frames as Stack(roll=False) lays them out) -> chw [nclips, CS, H, W],
 * ((v / 255) - mean3[c % 3]) / std3[c % 3], every step rounded in fp32 as the reference's tensor ops round it
 * (the f32 result is bit-identical); H * W * CS % 16 == 0, hwc 16-byte aligned.                              */
int rk_clip_u8_to_chw_f32(const unsigned char* hwc, const float* mean3, const float* std3, float* chw, int nclips,
                          int H, int W, int CS, rk_stream_t stream);
int rk_clip_u8_to_chw_bf16(const unsigned char* hwc, const float* mean3, const float* std3, void* chw, int nclips,
                           int H, int W, int CS, rk_stream_t stream);

/* ---- crop, resize and flip on the device: the head of the reference's transform chain ---------------
 * GroupMultiScaleCrop + GroupRandomHorizontalFlip (training) and GroupScale + GroupCenterCrop / GroupFullResSample /
 * GroupOverSample (evaluation) of rubiksnet/transforms.py, followed by the tail above, in one launch.
 * frames [B, T, Hs, Ws, 3] uint8 RGB as a decoder writes them (any alignment); out [B * V, T, 3, Sh, Sw]; output clip
 * b * V + v is view v of source clip b.  boxes: device int32 [B * V, 9], one record per OUTPUT clip shared by its T
 * frames: (x0, y0, cw, ch, rw, rh, ox, oy, flip).  An output frame is: the crop [y0 : y0 + ch, x0 : x0 + cw] of the
 * source frame, resampled to rw x rh exactly as Pillow's Image.resize((rw, rh), BILINEAR) resamples 8-bit data
 * (horizontal pass to uint8, then vertical; integer weights (int)(w * 2^22 + 0.5) from fp64 triangle-filter
 * coefficients of support max(in / out, 1)), of that the window [oy : oy + Sh, ox : ox + Sw], mirrored left-right when
 * flip != 0, then ((v / 255) - mean3[c]) / std3[c] rounded in fp32 as rk_clip_u8_to_chw does: the f32 result is
 * bit-identical to the reference's chain, the bf16 one is that rounded once to nearest-even.
 * cw / rw and ch / rh may be at most 8 (17 taps).  The boxes are device data: the launcher cannot check them, the
 * kernel clamps every read into `frames`, so a bad box gives a meaningless picture, never an out-of-bounds access
 * (rubiksnet_amd.augment.check_boxes is the host-side check).  Returns RK_ERR_UNSUPPORTED when Sw needs more LDS
 * than a workgroup has (Sw above ~920); no workspace, no allocation, no host synchronisation.                      */
int rk_clip_resample_u8_f32(const unsigned char* frames, const int* boxes, const float* mean3, const float* std3,
                            float* out, int B, int T, int Hs, int Ws, int V, int Sh, int Sw, rk_stream_t stream);
int rk_clip_resample_u8_bf16(const unsigned char* frames, const int* boxes, const float* mean3, const float* std3,
                             void* out, int B, int T, int Hs, int Ws, int V, int Sh, int Sw, rk_stream_t stream);
/* The same pass from a packed arena of B videos of different sizes (rubiksnet/dataset/core.py decodes a list of PIL
 * images per sample; real sets are ragged: one height and many widths, or both).  arena: uint8, arena_bytes long, any
 * alignment.  clips: device int64 [B, 4], one record per video: (byte offset of its first frame in the arena, Hs, Ws, F);
 * its F frames [Hs, Ws, 3] lie back to back from that offset, rows Ws * 3 bytes apart, no padding, and the offset may be
 * any byte.  frame_idx: device int32 [B * V, T]: output frame t of output clip oc shows stored frame
 * clamp(frame_idx[oc, t], 0, F - 1) of video oc / V, so one video can give several temporal clips (the two-clip
 * protocol) and frames may repeat.  boxes [B * V, 9], mean3, std3, out [B * V, T, 3, Sh, Sw] and the arithmetic are those
 * of rk_clip_resample_u8_*: a batch whose videos happen to share one size, with frame_idx[oc, t] = t, gives the same bits.
 * The tables are device data the launcher cannot check; the kernel never reads outside [arena, arena + arena_bytes),
 * whatever they hold.  A record is INVALID when Hs or Ws is outside [1, 16384], F < 1, the offset is negative, or
 * offset + F * Hs * Ws * 3 > arena_bytes: every workgroup of such a video's output clips decides that from the record
 * alone, before its first read of the arena, and writes zeros.  Boxes are clamped as above, into the record's own frame.
 * (rubiksnet_amd.augment.ragged_u8_to_clips checks host tables before they travel.)  B * V and T at most 65535;
 * RK_ERR_UNSUPPORTED when Sw needs more LDS than a workgroup has (the source sizes do not enter); no workspace, no
 * allocation, no host synchronisation.                                                                             */
int rk_clip_resample_ragged_u8_f32(const unsigned char* arena, long long arena_bytes, const long long* clips,
                                   const int* frame_idx, const int* boxes, const float* mean3, const float* std3,
                                   float* out, int B, int V, int T, int Sh, int Sw, rk_stream_t stream);
int rk_clip_resample_ragged_u8_bf16(const unsigned char* arena, long long arena_bytes, const long long* clips,
                                    const int* frame_idx, const int* boxes, const float* mean3, const float* std3,
                                    void* out, int B, int V, int T, int Sh, int Sw, rk_stream_t stream);

/* ---- baseline JPEG frames decoded on the device, bit-exact to libjpeg(-turbo)'s defaults (rk_jpeg.hip) ----
 * What Pillow's Image.open(f).convert("RGB") gives for a baseline file: Huffman decode, jidctint's ISLOW IDCT with its
 * range limit, fancy (triangle) chroma upsampling, jdcolor's 16-bit fixed-point YCbCr -> RGB.  The host parses the
 * headers (rubiksnet_amd.jpeg.parse_jpeg) and hands the device the entropy-coded segments and the tables.
 * Supported: SOF0, 8-bit, one interleaved scan, grayscale or YCbCr at 4:4:4 / 4:2:2 (2x1) / 4:2:0 (2x2), any Huffman
 * tables, DRI / RSTn, width and height in [1, 16384].
 *   streams  device bytes, any alignment: the entropy-coded segments (byte stuffing and RSTn markers included, the
 *            marker that ends the scan excluded) of all frames
 *   frames   device [n] records, below           qtabs  device [nq, 64] in NATURAL (row-major) order
 *   htabs    device [nh] decoding tables, below  rgb    device bytes: frame i's [H, W, 3] at its rgb_off (pack_clips' layout)
 *   status   device int [n + 1]: a RK_JPEG_* code per frame, [n] = the number of frames whose code is not 0
 * Everything but n, nq, nh and the byte counts is device data the launcher cannot check.  The kernels bound every loop
 * by counts from the record, never read outside [streams, streams + stream_bytes), qtabs, htabs or the workspace and
 * never write outside a frame's H * W * 3 bytes or the workspace, whatever the tables and the stream hold; bits wanted
 * past a frame's segment or past a marker read as zero.  A record is checked from its own fields before the first read
 * (RK_JPEG_BAD_RECORD: a size outside [1, 16384], components not 1 or 3, an unknown sampling, a table index >= nq / nh,
 * a negative offset, stream_off + stream_len > stream_bytes, rgb_off + H * W * 3 > rgb_bytes, or a workspace too small
 * for the frames up to and including this one).  A frame with a non-zero code is written as zeros (where its rgb range
 * is valid).  The decoder is stricter than libjpeg, which conceals errors: a code no table holds, a run past
 * coefficient 63 (a ZRL that no coefficient of the block can follow included), a DC difference above 11 bits, an AC value above 10 bits, a DC value outside [-2047, 2047], bits
 * wanted past the end, a missing or out-of-order RSTn, whole bytes left over, or pad bits that are not ones all fail
 * the frame.  Five launches on `stream`, ordered by the stream alone; no allocation, no host synchronisation, no
 * atomics; capturable.  n at most 65535, nq and nh at most 65535.  Returns RK_ERR_NULL_POINTER, RK_ERR_BAD_DIMS (a
 * count out of range, a negative byte count), RK_ERR_WORKSPACE (NULL, not 16-byte aligned, or too small for the offset
 * table of n frames) before anything is launched.                                                                  */
enum {
    RK_JPEG_OK = 0,
    RK_JPEG_BAD_RECORD = 1,   /* decided from the record alone */
    RK_JPEG_BAD_CODE = 2,     /* bits that are no code of the table */
    RK_JPEG_BAD_RUN = 3,      /* a zero run past coefficient 63 */
    RK_JPEG_TRUNCATED = 4,    /* bits wanted past the segment's end or past a marker */
    RK_JPEG_BAD_RESTART = 5,  /* RSTn missing or out of order */
    RK_JPEG_TRAILING = 6,     /* whole bytes left over, or pad bits that are not ones */
    RK_JPEG_BAD_VALUE = 7,    /* a magnitude category or DC value outside what 8-bit baseline can hold */
    RK_JPEG_BAD_INDEX = 8     /* a scan index (below) that does not fit the frame or does not tile its stream */
};
#define RK_JPEG_MAX_SIDE 16384
typedef struct rk_jpeg_frame {
    long long stream_off;           /* the frame's entropy-coded segment: bytes [stream_off, stream_off + stream_len) */
    long long stream_len;
    long long rgb_off;              /* byte offset of its [height, width, 3] output in rgb */
    int width, height;
    int components;                 /* 1 (grayscale: R = G = B = Y) or 3 (YCbCr) */
    int sampling;                   /* 0: 4:4:4, 1: 4:2:2 (luma 2x1), 2: 4:2:0 (luma 2x2); ignored for 1 component */
    int restart_interval;           /* MCUs between RSTn markers, 0: none */
    unsigned short quant[3];        /* per component: row of qtabs */
    unsigned short dc[3], ac[3];    /* per component: element of htabs */
    unsigned short reserved;
} rk_jpeg_frame;                    /* 64 bytes */
typedef struct rk_jpeg_huff {
    unsigned short look[512];       /* the next 9 bits -> (length << 8) | symbol for a code of 1..9 bits, else 0 */
    int maxcode[18];                /* [l], l = 1..16: the largest code of l bits, -1 when there is none */
    int valoff[18];                 /* [l]: index in huffval of the first code of l bits, minus that code */
    unsigned char huffval[256];
} rk_jpeg_huff;                     /* 1424 bytes */
/* Workspace for the n records of a HOST copy of the table (quantised coefficients and component planes of every frame
 * whose sizes are valid, behind an offset table); 0 for n < 1 or a NULL table. */
size_t rk_jpeg_workspace_bytes(const rk_jpeg_frame* frames_host, int n);
int rk_jpeg_decode_u8(const unsigned char* streams, long long stream_bytes, const rk_jpeg_frame* frames,
                      const unsigned short* qtabs, const rk_jpeg_huff* htabs, int nq, int nh, int n, unsigned char* rgb,
                      long long rgb_bytes, void* workspace, size_t workspace_bytes, int* status, rk_stream_t stream);

/* ---- resident JPEG frames decoded by scan index (rk_jpeg.hip) ----
 * A baseline scan can only be entered where the bit position and the DC predictors are known.  A set that stays on the
 * device (streams, records and tables laid out as above; a resident record's rgb_off is not used) is walked ONCE by
 * rk_jpeg_build_index, which remembers that state every seg_mcus[i] MCUs of frame i; every later decode of a frame
 * (rk_jpeg_decode_indexed_u8) then runs one Huffman chain per segment instead of one per frame.
 *   entry      the state at the top of MCU m's iteration, before its restart handling: bit_pos = 8 * (offset in the
 *              frame's segment of the raw byte that holds the next unread bit; FF 00 counts as two raw bytes and the bit
 *              lives in the FF) + (bit in that byte, 0 = most significant) -- the marker's FF, or stream_len, bit 0, when
 *              everything up to a marker or the end is used up -- and the three DC predictors.  The restart state follows
 *              from m and restart_interval and is not stored.
 *   seg_mcus   device int [n]: E_i >= 1; segment s of frame i covers MCUs [s * E_i, min((s + 1) * E_i, nmcu_i))
 *   entry_off  device long long [n + 1]: the exclusive sum of the frames' segment counts ceil(nmcu_i / E_i) (host-made)
 *   entries    device [n_entries]: frame i's entries at [entry_off[i], entry_off[i + 1])
 * rk_jpeg_build_index: one wave per frame, n at most 65535 per call (a larger set is built in chunks: pass the chunk's
 * frames, seg_mcus, entry_off and status; entry_off stays absolute).  A record is checked from its own fields first
 * (RK_JPEG_BAD_RECORD), then its row of the index (E_i < 1, a range that is not ceil(nmcu / E) long or leaves
 * [0, n_entries]: RK_JPEG_BAD_INDEX), before anything of the frame is read; status[i] is otherwise the code
 * rk_jpeg_decode_u8 would give the frame, status[n] the count of non-zero codes.  Entries of a failed frame are undefined.
 * rk_jpeg_decode_indexed_u8: decodes resident frames pick[j] (device int [m]) to rgb + rgb_off[j] (device long long [m]);
 * the same frame may be picked twice.  max_segments: at least the largest segment count among the picked frames (the
 * host knows every geometry; a picked frame with more fails with RK_JPEG_BAD_INDEX).  build_status: the build's
 * status array; a frame whose build code is not 0 is not read and gets that code.  A pick outside [0, n) is
 * RK_JPEG_BAD_RECORD.  Entries are untrusted device data: a segment checks its entry before its first read (bit_pos
 * outside [0, 8 * stream_len], a predictor outside +-2047, a non-zero entry 0) and, after its last MCU, that the reader
 * stands exactly at the next entry's bit_pos with the next entry's predictors (the last segment: at the end of the
 * stream) -- so the segments tile the stream -- and fails with RK_JPEG_BAD_INDEX otherwise.  status [m + 1]: per picked
 * frame the code of its lowest failing segment (a plain pass over a per-segment table in the workspace: no atomics, the
 * same code on every run), [m] the count.  Everything else is as rk_jpeg_decode_u8 documents: failed frames are zeroed
 * where their range is valid, no read outside the arenas, no allocation, no host wait, capturable; seven launches.
 * m and max_segments in [1, 65535].  Each segment is one wave in a workgroup of its own.                            */
typedef struct rk_jpeg_entry {
    long long bit_pos;
    short pred[3];
    short reserved;
} rk_jpeg_entry;                    /* 16 bytes */
int rk_jpeg_build_index(const unsigned char* streams, long long stream_bytes, const rk_jpeg_frame* frames,
                        const rk_jpeg_huff* htabs, int nq, int nh, int n, const int* seg_mcus, const long long* entry_off,
                        rk_jpeg_entry* entries, long long n_entries, int* status, rk_stream_t stream);
/* rk_jpeg_build_index_chunked: the same index -- status and entries identical to rk_jpeg_build_index's for the same
 * arguments, frame by frame, good or corrupt -- without one frame-long chain per frame.  A frame without restart markers
 * is cut into chunks of chunk_bytes raw bytes; a walk of a chunk takes a bit position to be the start of an MCU, decodes
 * whole MCUs to the first MCU boundary at or past the chunk's end, and counts the MCUs and the DC differences.  Rounds in
 * lock-step: first every chunk starts at its own first bit, then at the end the chunk before it reached in the round
 * before (its own first bit again where that walk was refused).  Chunk 0 starts at bit 0, so after round r chunks
 * 0 .. r - 1 hold the sequential walk; Huffman streams fall into step, so the fixed point -- which IS the sequential
 * walk -- comes after a few rounds.  A final pass then walks every chunk from its true start, first MCU number and
 * predictors and writes the entries; the frame has taken the chunked route only if that pass met no refusal, counted
 * exactly nmcu MCUs and found the end of the stream as rk_jpeg_build_index's walk must find it.  Every other frame gets
 * the sequential walk in the same call: restart_interval > 0, no fixed point within max_rounds, any refusal on the way,
 * more than 4096 chunks (the largest chunk count that takes the chunked route), max_rounds == 0.
 *   chunk_bytes  16, 32, 64, 128, 256 or 512        max_rounds  in [0, 64]
 *   workspace    device, 16-byte aligned, rk_jpeg_chunked_workspace_bytes long (an offset table and 32 bytes per chunk);
 *                a frame whose region does not fit takes the sequential walk
 *   route        device int [n]: 0 where the sequential walk produced the frame's result, else the number of rounds
 *                after which the chunked walk had converged
 * One workgroup of 1024 lanes per frame, a lane per chunk (and per 1024th chunk after it); the frame's tables sit in
 * LDS, the chunks' positions and sums in the workspace, the stream is read as aligned 8-byte words (the first and the
 * last word of the arena byte by byte: nothing outside [streams, streams + stream_bytes) is read).  Four launches on `stream`, a linear chain: no allocation, no host wait, no atomics, no
 * hand-off between workgroups; capturable.  Every loop is bounded: the rounds by max_rounds, a walk by its chunk's bits,
 * an MCU by its blocks' 64 symbols each.  Returns as rk_jpeg_build_index, and RK_ERR_BAD_DIMS for a chunk_bytes or
 * max_rounds outside the above, RK_ERR_WORKSPACE (NULL, not 16-byte aligned, shorter than the offset table).
 * rk_jpeg_chunked_workspace_bytes: from a HOST copy of the records; 0 for a NULL table, n < 1 or a chunk_bytes outside
 * the above.                                                                                                          */
size_t rk_jpeg_chunked_workspace_bytes(const rk_jpeg_frame* frames_host, int n, int chunk_bytes);
int rk_jpeg_build_index_chunked(const unsigned char* streams, long long stream_bytes, const rk_jpeg_frame* frames,
                                const rk_jpeg_huff* htabs, int nq, int nh, int n, const int* seg_mcus,
                                const long long* entry_off, rk_jpeg_entry* entries, long long n_entries, int chunk_bytes,
                                int max_rounds, void* workspace, size_t workspace_bytes, int* status, int* route,
                                rk_stream_t stream);
/* Workspace of one indexed decode, from HOST copies of the resident records and of pick: the m gathered records, the
 * per-segment table, then rk_jpeg_workspace_bytes of the picked records.  0 for a NULL table, m < 1 or max_segments < 1;
 * a pick outside [0, n) takes no frame region. */
size_t rk_jpeg_indexed_workspace_bytes(const rk_jpeg_frame* frames_host, int n, const int* pick_host, int m, int max_segments);
int rk_jpeg_decode_indexed_u8(const unsigned char* streams, long long stream_bytes, const rk_jpeg_frame* frames,
                              const unsigned short* qtabs, const rk_jpeg_huff* htabs, int nq, int nh, int n,
                              const rk_jpeg_entry* entries, long long n_entries, const long long* entry_off,
                              const int* seg_mcus, const int* build_status, const int* pick, const long long* rgb_off, int m,
                              int max_segments, unsigned char* rgb, long long rgb_bytes, void* workspace,
                              size_t workspace_bytes, int* status, rk_stream_t stream);

/* ---- resident frames kept as packed DCT coefficients (rk_jpeg.hip) ----
 * A resident set is read again every epoch, but its Huffman code needs undoing once.  What the entropy stage leaves --
 * short[64] per block, natural order, not dequantised -- is kept without its zeros, and a batch is decoded from that:
 * no Huffman stage, the same IDCT on the same coefficients, the same RGB bit for bit.
 * One frame's REGION of the blob (every part on a 2-byte boundary, little endian):
 *   uint32 off[nblocks]   byte offset of block b's record from the region's start; blocks in scan order (MCU by MCU, in
 *                         an MCU the luma blocks row by row, then Cb, then Cr), MCU padding blocks included
 *   the records, back to back in block order: off[0] = 4 * nblocks, record b + 1 starts where record b ends, the last
 *   one ends the region
 *   record: uint64 header   bit 0: the AC values are 16-bit; bit k (1..63): the AC coefficient at zigzag position k is
 *                           not zero
 *           int16  DC
 *           the non-zero AC values in zigzag order, int8 each where all of them fit, else int16 each, padded with a
 *           zero byte to an even count: 10 + n * w rounded up to even, 10 .. 136 bytes
 * Building (a set is processed in slabs of frames, so that the 128-byte-per-block workspace stays bounded):
 * rk_jpeg_coef_sizes runs the entropy stage ONCE over the slab's n records -- entries == NULL: rk_jpeg_decode_u8's one
 * chain per frame; otherwise rk_jpeg_decode_indexed_u8's one chain per segment by the given scan index (entries,
 * n_entries, entry_off, seg_mcus, build_status, max_segments as documented there; rk_jpeg_build_index_chunked makes
 * them) -- and then measures what it left:
 *   workspace    device, 16-byte aligned, rk_jpeg_indexed_workspace_bytes(frames, n, {0 .. n - 1}, n, max_segments)
 *                bytes (max_segments 1 where entries == NULL); it holds the coefficients until rk_jpeg_coef_pack
 *   status       device int [n + 1]: the frame's code as the decoders give it, [n] the count of non-zero codes; a
 *                frame whose blocks do not fit block_cap is RK_JPEG_BAD_RECORD
 *   first_block  device long long [n + 1]: the exclusive sum of the frames' block counts (written)
 *   block_off    device unsigned [block_cap]: at first_block[i] + b the offset of block b's record in frame i's region
 *   region_off   device long long [n + 1]: the exclusive sum of the frames' region lengths, [n] the total; a frame
 *                with a non-zero code has a region of length 0
 * rk_jpeg_coef_pack then writes the offset table and the records of every frame with code 0 to blob + region_off[i]
 * (the caller allocates region_off[n] bytes -- or more and shifts region_off -- between the two calls, which is why
 * they are two); the same frames, workspace, max_segments, status, block_off and first_block.  A region that does not
 * lie inside [0, blob_bytes) on a 2-byte boundary with exactly the measured length is not written.
 * rk_jpeg_decode_coef_u8 decodes frames pick[j] (device int [m]) of a set of n packed frames to rgb + rgb_off[j]:
 *   blob         device bytes, 2-byte aligned      region_off   device long long [n + 1], absolute in blob
 *   frames       device [n] records; stream_off, stream_len, rgb_off and the Huffman indices are not used
 *   build_status device int [n]: the codes rk_jpeg_coef_sizes gave; a frame with a non-zero code is not read, gets
 *                that code and goes out as a zero frame
 *   workspace    device, 16-byte aligned, rk_jpeg_coef_workspace_bytes(frames, n, pick, m): the m gathered records, a
 *                flag per picked frame, an offset table and the component planes -- no coefficient is stored: a lane
 *                expands one block's record straight into the IDCT
 * The blob and the tables are untrusted device data.  RK_JPEG_BAD_RECORD as for rk_jpeg_decode_indexed_u8 (a pick
 * outside [0, n), sizes, the output range, a quantisation index >= nq, the workspace).  RK_JPEG_BAD_INDEX, and a zero
 * frame, before anything outside the frame's region is read: a region that is not inside the blob, not on a 2-byte
 * boundary or not between 14 and 140 bytes per block long; an offset that is odd, inside the table or less than 10
 * bytes from the region's end; off[0] != 4 * nblocks; a header that says 16-bit values and no value; a record whose
 * length, from its header, does not end exactly where the next record starts (the region, for the last).  Every loop
 * is bounded by the block count and the 63 positions of a header.  Six launches on `stream`, a linear chain: no
 * allocation, no host wait, no atomics (lanes that refuse a block store the same flag); capturable.  m in [1, 65535].
 * rk_jpeg_coef_sizes and rk_jpeg_coef_pack: n, nq, nh, max_segments in [1, 65535]; they enqueue only.  Return codes as
 * rk_jpeg_decode_indexed_u8.  rk_jpeg_coef_workspace_bytes: from HOST copies; 0 for a NULL table, n < 1 or m < 1; a pick
 * outside [0, n) takes no planes.                                                                                     */
int rk_jpeg_coef_sizes(const unsigned char* streams, long long stream_bytes, const rk_jpeg_frame* frames,
                       const rk_jpeg_huff* htabs, int nq, int nh, int n, const rk_jpeg_entry* entries, long long n_entries,
                       const long long* entry_off, const int* seg_mcus, const int* build_status, int max_segments,
                       void* workspace, size_t workspace_bytes, int* status, unsigned* block_off, long long block_cap,
                       long long* first_block, long long* region_off, rk_stream_t stream);
int rk_jpeg_coef_pack(const rk_jpeg_frame* frames, int n, int max_segments, const void* workspace, size_t workspace_bytes,
                      const int* status, const unsigned* block_off, long long block_cap, const long long* first_block,
                      const long long* region_off, unsigned char* blob, long long blob_bytes, rk_stream_t stream);
size_t rk_jpeg_coef_workspace_bytes(const rk_jpeg_frame* frames_host, int n, const int* pick_host, int m);
int rk_jpeg_decode_coef_u8(const unsigned char* blob, long long blob_bytes, const rk_jpeg_frame* frames,
                           const unsigned short* qtabs, int nq, int n, const long long* region_off, const int* build_status,
                           const int* pick, const long long* rgb_off, int m, unsigned char* rgb, long long rgb_bytes,
                           void* workspace, size_t workspace_bytes, int* status, rk_stream_t stream);

/* ---- a second, denser record format for the same packed set (rk_jpeg.hip) ----
 * The three entry points above with a trailing record_format: RK_JPEG_COEF_WIDE is the format above, and the functions
 * above ARE these with it; RK_JPEG_COEF_DENSE chooses the value class per coefficient, not per block -- video frames
 * have one to three large values a block and some 25 within +-7 -- and a table of half the size.  Every other argument,
 * the workspace, block_off (the absolute offset of a block's record in its region), the launches and the return codes
 * are as above; any other record_format returns RK_ERR_BAD_DIMS.  A blob is decoded with the format it was packed in.
 * One frame's DENSE region (little endian, every record on a 2-byte boundary, no padding between regions):
 *   uint32 base[G], G = ceil(nblocks / 64), then uint16 rel[nblocks]: block b's record starts base[b / 64] + rel[b]
 *   bytes from the region's start (the packer writes base[g] = the start of record 64 g); the table is 4 G + 2 nblocks
 *   bytes, the first record starts there, record b + 1 starts where record b ends, the last one ends the region
 *   ordinary record: uint8 tag (bits 0-5 `last`, the zigzag position of the last non-zero AC, 0: none; bits 6-7 the
 *           class), int16 DC, ceil(last / 8) mask bytes (bit j: the AC at zigzag position j + 1 is not zero), ceil(n / 2)
 *           bytes of nibbles, one per non-zero AC in zigzag order, low nibble first (the value in 4-bit two's complement
 *           where it lies in -7 .. 7, 0x8: escaped), the e escaped values in order (int8 each in class 0; int16 each in
 *           class 1, used when one leaves int8), a zero byte to an even length:
 *           roundup2(3 + ceil(last / 8) + ceil(n / 2) + e w), 4 .. 130 bytes
 *   raw record (class 2), where the ordinary one would exceed 130 bytes: tag 0x80, a zero byte, int16[64] in natural order
 * RK_JPEG_BAD_INDEX and a zero frame, before anything outside the frame's region is read: a region not inside the blob,
 * odd at either end, or not between the table plus 4 and the table plus 130 bytes per block; a record start inside the
 * table, odd or less than 4 bytes from the region's end; a first record not at the table's end; a span [start, next
 * start) outside 4 .. 130 bytes; a record whose length, from its own tag, mask, nibbles and class, is not its span;
 * class 3; raw with last != 0; a mask whose bit `last` is clear or that has a bit above it; a nibble of 0 for a
 * coefficient the mask names.  The span comes from the table alone and every read of a record is checked against it
 * first.  What the format cannot see: a change that keeps every one of these true, such as a class bit flipped on a
 * record with a single escaped value whose padding absorbs the difference.
 * rk_jpeg_coef_region_bounds: the least and the most bytes a frame of nblocks blocks takes in `format` (table
 * included); host only; RK_ERR_BAD_DIMS for another format or nblocks < 1.                                             */
#define RK_JPEG_COEF_WIDE 0
#define RK_JPEG_COEF_DENSE 1
int rk_jpeg_coef_sizes_as(const unsigned char* streams, long long stream_bytes, const rk_jpeg_frame* frames,
                          const rk_jpeg_huff* htabs, int nq, int nh, int n, const rk_jpeg_entry* entries, long long n_entries,
                          const long long* entry_off, const int* seg_mcus, const int* build_status, int max_segments,
                          void* workspace, size_t workspace_bytes, int* status, unsigned* block_off, long long block_cap,
                          long long* first_block, long long* region_off, rk_stream_t stream, int record_format);
int rk_jpeg_coef_pack_as(const rk_jpeg_frame* frames, int n, int max_segments, const void* workspace, size_t workspace_bytes,
                         const int* status, const unsigned* block_off, long long block_cap, const long long* first_block,
                         const long long* region_off, unsigned char* blob, long long blob_bytes, rk_stream_t stream,
                         int record_format);
int rk_jpeg_decode_coef_as_u8(const unsigned char* blob, long long blob_bytes, const rk_jpeg_frame* frames,
                              const unsigned short* qtabs, int nq, int n, const long long* region_off, const int* build_status,
                              const int* pick, const long long* rgb_off, int m, unsigned char* rgb, long long rgb_bytes,
                              void* workspace, size_t workspace_bytes, int* status, rk_stream_t stream, int record_format);
int rk_jpeg_coef_region_bounds(int record_format, long long nblocks, long long* min_bytes, long long* max_bytes);

/* ---- squeeze-and-excitation gate of RubiksNet-Small -- widening row f3 of SURVEY 8(f) --------------
 * SELayer (rubiksnet/backbone.py:56-71): y = x * sigmoid(W2 relu(W1 mean_hw(x))).  x, y, dy, dx [F, C, P];
 * mean / gate / dgate [F, C] f32.  squeeze: mean over P; scale: y = x * gate; scale_backward: dx = dy * gate and
 * dgate = sum_p dy * x in one pass (the caller adds the squeeze's share dmean / P to dx through autograd).      */
#define RK_DECL_SE(SFX)                                                                                       \
    int rk_se_squeeze_##SFX(const void* x, float* mean, int F, int C, int P, rk_stream_t stream);             \
    int rk_se_scale_##SFX(const void* x, const float* gate, void* y, int F, int C, int P, rk_stream_t stream); \
    int rk_se_scale_backward_##SFX(const void* dy, const void* x, const float* gate, void* dx, float* dgate,  \
                                   int F, int C, int P, rk_stream_t stream);
RK_DECL_SE(f32)
RK_DECL_SE(bf16)
#undef RK_DECL_SE
/* The SE backward of the fused training block in 4 tensor passes instead of 5: dgate[f, c] = sum_p dy * x alone, and -- once
 * the two Linear layers' backward produced d(mean) [F, C] -- dx = dy * gate[f, c] + add[f, c] * add_scale (add_scale = 1 / P
 * is the squeeze's share, SELayer backward of rubiksnet/backbone.py:56-71).  fp32. */
/* The gate's two bias-free Linear layers on the squeezed vector, fused (one workgroup per frame): q [F, C], W1 [Cr, C], W2 [C, Cr]
 * (nn.Linear layout) -> h = relu(q W1^T) [F, Cr], g = sigmoid(h W2^T) [F, C]; backward: dgate [F, C] -> dq [F, C], dW1, dW2
 * (dpre2 [F, C], dpre1 [F, Cr]: caller-owned scratch).  RK_ERR_UNSUPPORTED for C > 2048 or Cr > 128. */
int rk_se_mlp_forward_f32(const float* q, const float* W1, const float* W2, float* h, float* g, int F, int C, int Cr,
                          rk_stream_t stream);
int rk_se_mlp_backward_f32(const float* dgate, const float* g, const float* h, const float* q, const float* W1, const float* W2,
                           float* dpre2, float* dpre1, float* dq, float* dW1, float* dW2, int F, int C, int Cr,
                           rk_stream_t stream);
int rk_se_dgate_f32(const float* dy, const float* x, float* dgate, int F, int C, int P, rk_stream_t stream);
int rk_se_scale_add_f32(const float* x, const float* gate, const float* add, float add_scale, float* y, int F, int C, int P,
                        rk_stream_t stream);

/* ---- the optimizer step of a whole network in one launch (rk_optim.hip; rubiksnet_amd/optim.py) ----------------
 * fp32 parameters, gradients and state.  jobs: device array of n 48-byte records, 8-byte aligned,
 *   {float* p; const float* g (float* with zero_grads); float* s0; float* s1; int64 numel; int32 chunk0; int32 group_flags}
 * one per tensor.  s0 = momentum buffer (SGD; NULL when the group's momentum is 0) or exp_avg (Adam), s1 = exp_avg_sq (Adam).
 * A tensor is cut into chunks of RK_OPTIM_CHUNK elements, the last one short; chunk0 = the chunks of all tensors before
 * it (rk_debug_optim_chunks computes the partition: no device call); `chunks` = the total.  group_flags: bits 0..2 the
 * hyper-parameter group, bit 8 (SGD) this tensor's momentum buffer is uninitialised: it receives g' instead of
 * momentum buf + (1 - dampening) g', torch's first step.  A workgroup owns one chunk and finds its record by binary search over
 * chunk0.  16-byte accesses where p, g and the state are all 16-byte aligned, dword accesses for the tail and for any
 * other tensor; numel 0 is allowed (no chunk).  The table is device data the launcher cannot check.
 * hyper: HOST array of ngroups records; it travels by value in the kernel arguments (an lr schedule needs no upload);
 * more than RK_OPTIM_MAX_GROUPS: RK_ERR_UNSUPPORTED, nothing launched.  Every product and sum rounds separately in fp32:
 *   SGD (torch.optim.SGD):    g' = coef g + wd p;  buf = g' (first) or momentum buf + (1 - dampening) g';
 *                             p -= lr buf, nesterov: p -= lr (g' + momentum buf);  momentum 0: p -= lr g'
 *   Adam (torch.optim.Adam, L2 decay): g' = coef g + wd p;  m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g' g';
 *                             p -= (lr / bc1) m / (sqrt(v) / bc2_sqrt + eps)     bc1 = 1 - beta1^t, bc2_sqrt = sqrt(1 - beta2^t)
 * Clipping by the global L2 norm (torch.nn.utils.clip_grad_norm_): rk_optim_sqnorm_many_f32 writes one fp64 sum of g^2 per
 * chunk into `partials` (rk_optim_sqnorm_workspace_bytes of it); the step launch given partials != NULL has EVERY
 * workgroup add the npartials values up in one fixed order (fp64), coef = min(1, max_norm / (norm + 1e-6)), and workgroup 0
 * stores the norm to norm_out (fp32, may be NULL).  Two plain launches on one stream: no hand-off inside a launch, no
 * atomics; bitwise reproducible.  partials == NULL: coef = 1.  zero_grads != 0: g is overwritten with 0 once read.
 * No allocation, no synchronisation, no device call besides the launch. */
#define RK_OPTIM_CHUNK 4096
#define RK_OPTIM_MAX_GROUPS 8
typedef struct { float lr, weight_decay, momentum, one_minus_dampening; int nesterov; } rk_optim_sgd_hyper;
typedef struct { float step_size, weight_decay, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, bc2_sqrt; } rk_optim_adam_hyper;
/* out[0] = RK_OPTIM_CHUNK, out[1] = chunks in all, out[2 + i] = chunk0 of tensor i (n + 2 ints).  RK_ERR_BAD_DIMS for a
 * negative numel or more than 2^31 - 1 chunks. */
int rk_debug_optim_chunks(const long long* numels, int n, int* out);
size_t rk_optim_sqnorm_workspace_bytes(int chunks);
int rk_optim_sqnorm_many_f32(const void* jobs, int n, int chunks, double* partials, rk_stream_t stream);
int rk_optim_sgd_many_f32(const void* jobs, int n, int chunks, const rk_optim_sgd_hyper* hyper, int ngroups,
                          const double* partials, int npartials, float max_norm, float* norm_out, int zero_grads,
                          rk_stream_t stream);
int rk_optim_adam_many_f32(const void* jobs, int n, int chunks, const rk_optim_adam_hyper* hyper, int ngroups,
                           const double* partials, int npartials, float max_norm, float* norm_out, int zero_grads,
                           rk_stream_t stream);
/* The extended step: the same table, partials, norm_out and zero_grads as above, and opt-in
 *   rule: RK_OPTIM_RULE_SGD / _ADAM (hyper: HOST array of rk_optim_sgd_hyper / rk_optim_adam_hyper, the rules above) or
 *     RK_OPTIM_RULE_ADAMW (torch.optim.AdamW; rk_optim_adamw_hyper): p1 = decay_factor p with decay_factor = 1 - lr wd formed
 *     by the caller in double and rounded once; g' = coef g (no L2 term); m, v as Adam;
 *     p = p1 - (lr / bc1) m / (sqrt(v) / bc2_sqrt + eps).  Another rule: RK_ERR_UNSUPPORTED.
 *   ema: NULL, or a device array of n pointers (8-byte aligned) parallel to the table: the fp32 EMA shadow of tensor i, of
 *     numel elements, or NULL for a tensor without one.  After the rule has produced the new p:
 *     e = ema_decay e + ema_one_minus_decay p_new (two products, one sum, each rounded).  The two factors apply to the whole
 *     launch and travel by value: a warm-up schedule uploads nothing.  16-byte accesses where p, g, the states AND e are
 *     16-byte aligned, dword accesses otherwise.
 *   guard != 0: needs partials (RK_ERR_WORKSPACE without, nothing launched) and skipped, an 8-byte aligned device int64.
 *     When the fp64 sum of the partials is NaN or an infinity, NO workgroup writes p, a state or a shadow (every workgroup
 *     forms the same sum bit for bit: no hand-off, no polling, no atomics); zero_grads still zeroes the gradients; thread 0
 *     of workgroup 0 stores the non-finite norm to norm_out and adds 1 to *skipped with a plain load and store (one writer
 *     per launch, launches ordered by the stream).  A finite sum -- gradients of 1e25 included, whose squares overflow fp32
 *     only -- is an ordinary step.  Guarding without clipping: max_norm = +inf gives coef = 1.
 * Everything is validated before the launch; no allocation, no synchronisation, no device call besides the launch. */
#define RK_OPTIM_RULE_SGD 0
#define RK_OPTIM_RULE_ADAM 1
#define RK_OPTIM_RULE_ADAMW 2
typedef struct { float step_size, decay_factor, beta1, one_minus_beta1, beta2, one_minus_beta2, eps, bc2_sqrt; } rk_optim_adamw_hyper;
int rk_optim_step_ext_f32(int rule, const void* jobs, int n, int chunks, const void* hyper, int ngroups, const double* partials,
                          int npartials, float max_norm, float* norm_out, int zero_grads, const void* ema, float ema_decay,
                          float ema_one_minus_decay, int guard, long long* skipped, rk_stream_t stream);

/* ---- streaming metrics: loss, top-k and per-class accuracy accumulated on the device (rk_metrics.hip; ---------------
 * rubiksnet_amd/metrics.py).  One launch scores `videos` videos: logits [videos * views, classes] row-major contiguous
 * (row b * views + v = view v of video b), labels [videos] int64.  In fp32:
 *   z[k] = (sum over v ascending of x[b, v, k]) / views;   pred = the lowest index among the maxima of z;
 *   rank = #{j : z[j] > z[y]} + #{j < y : z[j] == z[y]}    (a hit at k when rank < k; rank 0 <=> pred == y);
 *   loss = (max + logf(sum expf(z - max))) - z[y], clamped to [0, 2^20].
 * A label outside [0, classes) adds 1 to bad_labels and nothing else (it is checked before it indexes anything).  A video
 * with a NaN or an infinity in z adds 1 to videos, nonfinite and its label's count: a miss at every k, nothing to the loss
 * sum or the confusion matrix.  state: int64 words, 8-byte aligned, rk_metrics_state_bytes of them, zeroed by the caller:
 *   [0] videos  [1] loss sum in units of 2^-32 (llrint(loss * 2^32) per video)  [2] nonfinite  [3] bad_labels
 *   [4..8) hits per top-k slot   [8..8+K) videos per label   [8+K..8+2K) top-1 hits per label
 *   [8+2K..8+2K+K*K) confusion[label][pred], only when confusion != 0
 * Words are added with 64-bit integer atomics only: the state is bit-identical from run to run, and the states of several
 * ranks merge with one integer sum.  No workgroup waits on another.  ntopk values of k (k0.. in slot order, each >= 1; the
 * rest ignored) travel by value.  Per-video outputs, each may be NULL: consensus f32 [videos, classes], pred int32, rank
 * int32, loss f32 [videos]; a bad label or a non-finite video stores rank -1 and loss NaN, a non-finite one pred -1.
 * Returns RK_ERR_NULL_POINTER (logits, labels, state), RK_ERR_BAD_DIMS (a dimension <= 0, videos * views * classes >= 2^31,
 * a k < 1, ntopk < 0, misaligned state), RK_ERR_UNSUPPORTED (views > 64, classes > 65536, ntopk > 4) before anything
 * touches a device.  No allocation, no synchronisation, no device call besides the launch. */
#define RK_METRICS_MAX_TOPK 4
#define RK_METRICS_MAX_VIEWS 64
#define RK_METRICS_MAX_CLASSES 65536
#define RK_METRICS_HEAD_WORDS 8
size_t rk_metrics_state_bytes(int classes, int confusion); /* 0 for classes outside [1, 65536] */
int rk_metrics_update_f32(const float* logits, const long long* labels, long long* state, int videos, int views, int classes,
                          int confusion, int ntopk, int k0, int k1, int k2, int k3, float* consensus, int* pred, int* rank,
                          float* loss, rk_stream_t stream);
int rk_metrics_update_bf16(const void* logits, const long long* labels, long long* state, int videos, int views, int classes,
                           int confusion, int ntopk, int k0, int k1, int k2, int k3, float* consensus, int* pred, int* rank,
                           float* loss, rk_stream_t stream);
int rk_metrics_update_f16(const void* logits, const long long* labels, long long* state, int videos, int views, int classes,
                          int confusion, int ntopk, int k0, int k1, int k2, int k3, float* consensus, int* pred, int* rank,
                          float* loss, rk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RUBIKS_HIP_H_ */
