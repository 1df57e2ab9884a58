// rk_pw_plan.hpp -- which of the four fp32 1x1 GEMM generations runs a call, and the entry points of their launchers:
//   rk_pw.hip   first generation (k_pw_gemm, 128-column tiles): everything the others do not take
//   rk_pw2.hip  barrier-free GEMM (64-column tiles) and d(weight)
//   rk_pw3.hip  per-CU LDS-tiled GEMM of the 257..288-row layers
//   rk_pw4.hip  streaming GEMM of the 54- / 72-channel layers (64-column tiles)
// plan_gemm (rk_pw.hip) holds every eligibility rule and makes no HIP call; the launchers run the configuration they get.
#pragma once
#include "rk_common.hpp"

namespace rk {

struct GFuse {               // per-channel affine (+ReLU) stages: prologue on X rows (ka, kb), epilogue on Y rows (ma, mb)
    const float* ka; const float* kb; const float* ma; const float* mb;
    int relu_in, relu_out;
};
struct GTrain {              // training epilogues, one record per (row, column tile)
    float4* stats;           // EPI 1: [M][J] (pivot, sum(y - pivot), sum((y - pivot)^2), n)
    float2* bred;            // EPI 2: [M][J] (sum dz, sum dz xhat)
    const float* bx;         // EPI 2: the BatchNorm's input, [F, M, P]
    const float4* bpack;     // EPI 2: [M] (a, b, mean, invstd)
    int J;
};

namespace pw {

struct Modes { int pw2, pw3, pw4; };     // RK_PW2 (0 off, 1 where ahead, 2 wherever it can), RK_PW3 (0 off), RK_PW4 (0 off, 2 any size)
Modes env_modes();                       // the process's switches, read once

// one call of the fp32 GEMM: Y[f] = epi(A pro(X[f])) (+ R[f]); aligned: A and X 16-byte aligned
struct GemmCall { int F, K, M, P, a_is_mk, aligned, epi, res, pro, ma; };
// gen 1..4 with its configuration (1: wm, kc; 2: rb, amode, ct; 3: columns per workgroup, workgroups; 4: rb, k-steps),
// or gen 0 and the error code; tiles: the statistics tiles of an epilogue call (= rk_pw_gemm_tiles), else 0
struct GemmPlan { int rc, gen, c0, c1, c2, tiles; };
GemmPlan plan_gemm(const GemmCall& c, const Modes& m, int cus);
int gemm_tiles(int F, int K, int M, int P, int a_is_mk, int aligned, const Modes& m, int cus);
// d(weight): 2 = rk_pw2.hip, 1 = the first generation's wide kernel, 0 = its narrow one
int plan_wgrad(int F, int K, int M, int P, const Modes& m);
// the streaming kernel's row blocks (4, 5) for the call, 0: not taken; any_size: without the size / epilogue policy
int pw4_rb(const GemmCall& c, const Modes& m, bool any_size);
bool pw4_takes(const GemmCall& c);       // ... and has an instance for its flags

}  // namespace pw

namespace pw2 {
struct GCfg { int rb, amode, ct; };
struct WCfg { int id; int ns; int splits; };
bool gemm_cfg(GCfg& c, int K, int M, int a_is_mk, int aligned);
bool gemm_instance(const GCfg& c, int a_is_mk, int aligned, int K, int M, int epi, int pro, int ma);
int gemm(const float* A, const float* X, const float* R, float* Y, int F, int K, int M, int P, int a_is_mk, const GFuse& fz,
         const GTrain& tr, int epi, hipStream_t stream, const GCfg& c);
size_t wgrad_workspace_bytes(int F, int K, int M, int P);
int wgrad(const float* dY, const float* X, float* dW, int F, int K, int M, int P, void* ws, size_t ws_bytes, const float* ka,
          const float* kb, int relu_in, hipStream_t stream, const WCfg* cfg_override);
}  // namespace pw2

namespace pw3 {
int plan(int F, int K, int M, int P, int cus, int* cw);    // workgroups of cw columns, 0: not this kernel's shape
int gemm(const float* A, const float* X, const float* R, float* Y, int F, int K, int M, int P, int a_is_mk, const GFuse& fz,
         const GTrain& tr, int epi, hipStream_t stream, int cw, int nwg);
}  // namespace pw3

namespace pw4 {
int gemm(const float* A, const float* X, const float* R, float* Y, int F, int K, int M, int P, int a_is_mk, const GFuse& fz,
         const GTrain& tr, int epi, hipStream_t stream, int rb);
}  // namespace pw4

}  // namespace rk
