// rk_metrics.hip -- loss, top-k and per-class accuracy of one batch, accumulated on the device in ONE launch
// (include/rubiks_hip.h "streaming metrics"; rubiksnet_amd/metrics.py).
//
// A workgroup owns one video.  Lane <-> class: a thread walks k = tid, tid + 256, ... and reads the `views` rows of its
// column (coalesced along classes), so every pass is `views` row segments per wave-instruction.
//   pass 1   z[k] = (sum over views, ascending) / views; the consensus output; max, lowest argmax, "any non-finite"
//   pass 2   #{z > z[y]} + #{j < y : z == z[y]} and sum expf(z - max); z comes from LDS when classes <= kZLds and is
//            formed again from the logits otherwise (the same operations in the same order: the same bits)
// Thread 0 then adds the video's words to the state with 64-bit INTEGER atomics (no return value used).  Integer adds
// commute: the state is bit-identical from run to run whatever the order workgroups finish in.  No workgroup waits on, or
// reads anything written by, another.  The label is range-checked before it forms any address.
#include "rk_common.hpp"

#include <math.h>

namespace rk {

constexpr int kZLds = 4096;                  // classes whose consensus stays in LDS (16 KB)
constexpr int kWaves = kBlock / kWave;
constexpr int kMaxTopk = RK_METRICS_MAX_TOPK;

struct TopK { int n; int k[kMaxTopk]; };

template <typename T>
__device__ __forceinline__ float consensus_at(const T* __restrict__ row0, int k, int V, int K) {
    float s = ld(row0 + k);
    for (int v = 1; v < V; ++v) s += ld(row0 + (size_t)v * K + k);
    return s / (float)V;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_metrics_update(const T* __restrict__ logits, const long long* __restrict__ labels,
                                                           unsigned long long* __restrict__ state, int V, int K,
                                                           int confusion, TopK topk, float* __restrict__ consensus,
                                                           int* __restrict__ pred_out, int* __restrict__ rank_out,
                                                           float* __restrict__ loss_out) {
    __shared__ float zs[kZLds];
    __shared__ float s_max[kWaves];
    __shared__ int s_arg[kWaves];
    __shared__ int s_bad[kWaves];
    __shared__ float s_sum[kWaves];
    __shared__ int s_cnt[kWaves];

    const int b = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const T* row0 = logits + (size_t)b * V * K;
    const bool in_lds = K <= kZLds;
    const long long label = labels[b];
    const bool label_ok = label >= 0 && label < (long long)K;
    const int y = label_ok ? (int)label : 0;          // (never an address unless label_ok)

    // ---- pass 1 ----
    float m = -INFINITY;
    int arg = 0x7fffffff, bad = 0;
    for (int k = tid; k < K; k += kBlock) {
        const float z = consensus_at(row0, k, V, K);
        if (in_lds) zs[k] = z;
        if (consensus) consensus[(size_t)b * K + k] = z;
        bad |= !(fabsf(z) <= 3.402823466e+38f);       // NaN and +-inf
        if (z > m) { m = z; arg = k; }                 // k ascends: the first of equal maxima stays
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, kWave);
        const int oa = __shfl_xor(arg, o, kWave);
        if (om > m || (om == m && oa < arg)) { m = om; arg = oa; }
    }
    bad = __ballot(bad) != 0ull;
    if (lane == 0) { s_max[wave] = m; s_arg[wave] = arg; s_bad[wave] = bad; }
    __syncthreads();
    m = s_max[0]; arg = s_arg[0]; bad = s_bad[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        const float om = s_max[w];
        const int oa = s_arg[w];
        if (om > m || (om == m && oa < arg)) { m = om; arg = oa; }
        bad |= s_bad[w];
    }

    if (!label_ok || bad) {                            // uniform over the workgroup
        if (tid == 0) {
            if (pred_out) pred_out[b] = bad ? -1 : arg;
            if (rank_out) rank_out[b] = -1;
            if (loss_out) loss_out[b] = __builtin_nanf("");
            if (!label_ok) {
                atomicAdd(state + 3, 1ull);
            } else {
                atomicAdd(state + 0, 1ull);
                atomicAdd(state + 2, 1ull);
                atomicAdd(state + 8 + y, 1ull);
            }
        }
        return;
    }

    // ---- pass 2 ----
    const float zy = in_lds ? zs[y] : consensus_at(row0, y, V, K);
    float sum = 0.f;
    int cnt = 0;
    for (int k = tid; k < K; k += kBlock) {
        const float z = in_lds ? zs[k] : consensus_at(row0, k, V, K);
        cnt += (z > zy) || (z == zy && k < y);
        sum += expf(z - m);
    }
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    if (lane == 0) { s_sum[wave] = sum; s_cnt[wave] = cnt; }
    __syncthreads();
    if (tid != 0) return;
    sum = s_sum[0]; cnt = s_cnt[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) { sum += s_sum[w]; cnt += s_cnt[w]; }

    float loss = (m + logf(sum)) - zy;
    loss = fminf(fmaxf(loss, 0.f), 1048576.f);
    if (pred_out) pred_out[b] = arg;
    if (rank_out) rank_out[b] = cnt;
    if (loss_out) loss_out[b] = loss;
    atomicAdd(state + 0, 1ull);
    atomicAdd(state + 1, (unsigned long long)llrint((double)loss * 4294967296.0));
    for (int i = 0; i < topk.n; ++i)
        if (cnt < topk.k[i]) atomicAdd(state + 4 + i, 1ull);
    atomicAdd(state + 8 + y, 1ull);
    if (cnt == 0) atomicAdd(state + 8 + K + y, 1ull);
    if (confusion) atomicAdd(state + 8 + 2 * (size_t)K + (size_t)y * K + arg, 1ull);
}

template <typename T>
static int metrics_update(const T* logits, const long long* labels, long long* state, int videos, int views, int classes,
                          int confusion, int ntopk, int k0, int k1, int k2, int k3, float* consensus, int* pred, int* rank,
                          float* loss, rk_stream_t stream) {
    if (!logits || !labels || !state) return RK_ERR_NULL_POINTER;
    if (videos <= 0 || views <= 0 || classes <= 0 || ntopk < 0) return RK_ERR_BAD_DIMS;
    if (views > RK_METRICS_MAX_VIEWS || classes > RK_METRICS_MAX_CLASSES || ntopk > kMaxTopk) return RK_ERR_UNSUPPORTED;
    if ((long long)videos * views * classes >= (1ll << 31)) return RK_ERR_BAD_DIMS;
    TopK topk = {ntopk, {k0, k1, k2, k3}};
    for (int i = 0; i < ntopk; ++i)
        if (topk.k[i] < 1) return RK_ERR_BAD_DIMS;
    if ((uintptr_t)state & 7) return RK_ERR_BAD_DIMS;
    hipLaunchKernelGGL(k_metrics_update<T>, dim3(videos), dim3(kBlock), 0, (hipStream_t)stream, logits, labels,
                       (unsigned long long*)state, views, classes, confusion != 0, topk, consensus, pred, rank, loss);
    return launch_status();
}

}  // namespace rk

using namespace rk;

extern "C" {

size_t rk_metrics_state_bytes(int classes, int confusion) {
    if (classes <= 0 || classes > RK_METRICS_MAX_CLASSES) return 0;
    const size_t K = (size_t)classes;
    return (8 + 2 * K + (confusion ? K * K : 0)) * sizeof(long long);
}

int rk_metrics_update_f32(const float* logits, const long long* labels, long long* state, int videos, int views, int classes,
                          int confusion, int ntopk, int k0, int k1, int k2, int k3, float* consensus, int* pred, int* rank,
                          float* loss, rk_stream_t stream) {
    return metrics_update(logits, labels, state, videos, views, classes, confusion, ntopk, k0, k1, k2, k3, consensus, pred,
                          rank, loss, stream);
}

int rk_metrics_update_bf16(const void* logits, const long long* labels, long long* state, int videos, int views, int classes,
                           int confusion, int ntopk, int k0, int k1, int k2, int k3, float* consensus, int* pred, int* rank,
                           float* loss, rk_stream_t stream) {
    return metrics_update((const __hip_bfloat16*)logits, labels, state, videos, views, classes, confusion, ntopk, k0, k1, k2,
                          k3, consensus, pred, rank, loss, stream);
}

int rk_metrics_update_f16(const void* logits, const long long* labels, long long* state, int videos, int views, int classes,
                          int confusion, int ntopk, int k0, int k1, int k2, int k3, float* consensus, int* pred, int* rank,
                          float* loss, rk_stream_t stream) {
    return metrics_update((const __half*)logits, labels, state, videos, views, classes, confusion, ntopk, k0, k1, k2, k3,
                          consensus, pred, rank, loss, stream);
}

}  // extern "C"
