// rk_optim.hip -- the optimizer step of a whole network in ONE launch (SGD with momentum / Adam, fp32), with optional
// clipping by the global gradient norm (one more launch) and optional zeroing of the gradients it consumed.
//
// The "many" idiom of rk_soft_taps_many_* / rk_pw_pack_many_bf16 / rk_bn_fold_many_f32: a device-resident table with one
// record per tensor, built once by the caller (rubiksnet_amd/optim.py).  Tensors differ in size by four orders of magnitude
// (a [3, C] shift table next to a 576 x 576 weight), so the grid is not (tensor, block) but a flat list of fixed-size chunks:
// a workgroup owns chunk blockIdx.x of RK_OPTIM_CHUNK elements and finds the tensor it belongs to by binary search over the
// records' running chunk offsets (block-uniform: scalar loads that hit the constant cache after the first workgroups).
// What changes every step -- lr under a schedule, Adam's bias corrections -- travels by value in the kernel arguments, so
// the table is uploaded only when a pointer moves.
//
// Arithmetic: torch's rules in torch's order, every product and sum rounded separately in fp32 (-ffp-contract=off); the
// layout of the comment in include/rubiks_hip.h.  The op is a pure stream (SGD 5, Adam 7 dwords per element): 16-byte
// accesses, the whole chunk's loads issued before the first use.
//
// Clipping is two plain launches on one stream: k_optim_sqnorm leaves one fp64 sum of squares per chunk, and every
// workgroup of the step launch adds those few thousand L2-resident doubles up itself, all in the same fixed order, so
// all agree on the norm bit for bit: no hand-off inside a launch, no polling, no atomics.
//
// rk_optim_step_ext_f32 is the same step over the same table with three opt-in additions: the AdamW rule (decoupled decay:
// p is scaled by a host-formed 1 - lr wd before Adam's update, the gradient sees no L2 term); an EMA shadow of the new
// parameter as a third state (e = decay e + (1 - decay) p_new, two more dwords per element in the same launch; the shadows'
// addresses come in a device array parallel to the table, NULL = none); and a guard: when the fp64 sum of the partials is
// not finite, no workgroup writes p, a state or a shadow -- every workgroup holds the same sum, so the decision needs no
// hand-off either -- and thread 0 of workgroup 0 counts the skipped step in a caller's int64.
#include "rk_common.hpp"

namespace rk {
namespace optim {

constexpr int kChunk = RK_OPTIM_CHUNK;
constexpr int kVecIter = kChunk / (4 * kBlock);          // 16-byte accesses per thread and tensor of a full chunk
static_assert(kChunk % (4 * kBlock) == 0, "a full chunk is whole 16-byte accesses of the whole workgroup");
constexpr int kFirstStep = 1 << 8;                       // Job::group_flags

struct Job { float* p; float* g; float* s0; float* s1; long long numel; int chunk0; int group_flags; };
static_assert(sizeof(Job) == 48, "the record layout rubiksnet_amd/optim.py writes");
struct SgdArgs { rk_optim_sgd_hyper g[RK_OPTIM_MAX_GROUPS]; };
struct AdamArgs { rk_optim_adam_hyper g[RK_OPTIM_MAX_GROUPS]; };

// the record of chunk b: the LAST one with chunk0 <= b (a tensor of 0 elements shares its chunk0 with its successor and
// is never chosen; records behind the last chunk are never reached).  jobs[0].chunk0 == 0 <= b.
__device__ __forceinline__ int find_job(const Job* __restrict__ jobs, int n, int b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].chunk0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the elements [start, start + cnt) of record j that chunk b covers; cnt <= 0: nothing (a table / `chunks` mismatch cannot
// push an access past numel)
__device__ __forceinline__ int chunk_range(const Job& j, int b, long long* start) {
    *start = (long long)(b - j.chunk0) * kChunk;
    const long long left = j.numel - *start;
    return left >= kChunk ? kChunk : (int)(left > 0 ? left : 0);
}

// The tensors' addresses come out of the table, so the compiler knows no address space for them and would use flat
// accesses; they are global memory.
typedef __attribute__((address_space(1))) float gfloat;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f32x4 gfloat4;

__device__ __forceinline__ bool aligned16(const void* a, const void* b, const void* c, const void* d) {
    return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;       // (NULL counts as aligned)
}

// sum of the workgroup's values, the same in every thread; fixed tree.  Whole workgroup, converged.
__device__ __forceinline__ double block_sum(double v, double* smem) {
    v = wave_sum(v);
    if ((threadIdx.x & (kWave - 1)) == 0) smem[threadIdx.x / kWave] = v;
    __syncthreads();
    static_assert(kBlock / kWave == 4, "four waves");
    return ((smem[0] + smem[1]) + smem[2]) + smem[3];
}

// ---- sum of squares per chunk -----------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_optim_sqnorm(const Job* __restrict__ jobs, int n, double* __restrict__ partials) {
    __shared__ double smem[kBlock / kWave];
    const int b = blockIdx.x;
    const Job j = jobs[find_job(jobs, n, b)];
    long long start;
    const int cnt = chunk_range(j, b, &start);
    const gfloat* __restrict__ g = (const gfloat*)(j.g + start);
    const int nvec = aligned16(j.g, nullptr, nullptr, nullptr) ? cnt >> 2 : 0;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nvec; i += kBlock) {
        const f32x4 v = ((const gfloat4*)g)[i];
        acc += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
    }
    for (int i = nvec * 4 + threadIdx.x; i < cnt; i += kBlock) acc += (double)g[i] * g[i];
    acc = block_sum(acc, smem);
    if (threadIdx.x == 0) partials[b] = acc;
}

// ---- the update rules: one element ------------------------------------------------------------------------------
template <bool BUF> struct SgdRule {
    static constexpr int kStates = BUF ? 1 : 0;
    float coef, lr, wd, mu, omd;
    bool nesterov, first;
    __device__ __forceinline__ void apply(float& p, float g, float& buf, float&) const {
        const float gp = coef * g + wd * p;
        if (!BUF) { p = p - lr * gp; return; }
        buf = first ? gp : mu * buf + omd * gp;
        p = p - lr * (nesterov ? gp + mu * buf : buf);
    }
};
struct AdamRule {
    static constexpr int kStates = 2;
    float coef, step_size, wd, b1, omb1, b2, omb2, eps, bc2s;
    __device__ __forceinline__ void apply(float& p, float g, float& m, float& v) const {
        const float gp = coef * g + wd * p;
        m = b1 * m + omb1 * gp;
        v = b2 * v + omb2 * (gp * gp);
        p = p - step_size * (m / (sqrtf(v) / bc2s + eps));
    }
};

// torch.optim.AdamW: the decay is decoupled (p1 = decay_factor p, decay_factor = 1 - lr wd formed on the host), g' has no L2 term
struct AdamWRule {
    static constexpr int kStates = 2;
    float coef, step_size, decay_factor, b1, omb1, b2, omb2, eps, bc2s;
    __device__ __forceinline__ void apply(float& p, float g, float& m, float& v) const {
        const float p1 = decay_factor * p;
        const float gp = coef * g;
        m = b1 * m + omb1 * gp;
        v = b2 * v + omb2 * (gp * gp);
        p = p1 - step_size * (m / (sqrtf(v) / bc2s + eps));
    }
};
// the EMA shadow of the parameter the rule has just produced
struct Ema {
    float decay, omd;
    __device__ __forceinline__ float apply(float e, float p_new) const { return decay * e + omd * p_new; }
};

template <class Rule> __device__ __forceinline__ void apply4(const Rule& r, f32x4& p, const f32x4& g, f32x4& a, f32x4& b) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = p[e], ae = a[e], be = b[e];
        r.apply(pe, g[e], ae, be);
        p[e] = pe;
        a[e] = ae;
        b[e] = be;
    }
}

// one chunk: elements [0, cnt) behind p / g / s0 / s1 (already offset to the chunk; a chunk starts a multiple of 4 elements
// into its tensor, so the tensor's alignment is the chunk's).  EMA: e_ is the chunk of the parameter's shadow, updated from
// the new p (16-byte accesses only where it is aligned too).
template <class Rule, bool EMA = false>
__device__ __forceinline__ void run_chunk(const Rule& r, float* p_, float* g_, float* s0_, float* s1_, int cnt, bool zero_grads,
                                          float* e_ = nullptr, const Ema ema = Ema{0.f, 0.f}) {
    constexpr int S = Rule::kStates;
    const int nvec = aligned16(p_, g_, S > 0 ? s0_ : nullptr, S > 1 ? s1_ : nullptr) && (!EMA || (((uintptr_t)e_) & 15) == 0)
                         ? cnt >> 2 : 0;
    gfloat* __restrict__ p = (gfloat*)p_;
    gfloat* __restrict__ g = (gfloat*)g_;
    gfloat* __restrict__ s0 = (gfloat*)s0_;
    gfloat* __restrict__ s1 = (gfloat*)s1_;
    gfloat* __restrict__ e = (gfloat*)e_;
    gfloat4* __restrict__ p4 = (gfloat4*)p_;
    gfloat4* __restrict__ g4 = (gfloat4*)g_;
    gfloat4* __restrict__ a4 = (gfloat4*)s0_;
    gfloat4* __restrict__ b4 = (gfloat4*)s1_;
    gfloat4* __restrict__ e4 = (gfloat4*)e_;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    if (nvec == kChunk / 4) {             // a full aligned chunk (nearly all of the bytes): every load before the first use
        f32x4 P[kVecIter], G[kVecIter], A[kVecIter], B[kVecIter], E[kVecIter];
#pragma unroll
        for (int k = 0; k < kVecIter; ++k) {
            const int i = threadIdx.x + k * kBlock;
            P[k] = p4[i];
            G[k] = g4[i];
            A[k] = zero4;
            B[k] = zero4;
            E[k] = zero4;
            if (S > 0) A[k] = a4[i];
            if (S > 1) B[k] = b4[i];
            if (EMA) E[k] = e4[i];
        }
#pragma unroll
        for (int k = 0; k < kVecIter; ++k) {
            const int i = threadIdx.x + k * kBlock;
            apply4(r, P[k], G[k], A[k], B[k]);
            p4[i] = P[k];
            if (S > 0) a4[i] = A[k];
            if (S > 1) b4[i] = B[k];
            if (EMA) {
#pragma unroll
                for (int c = 0; c < 4; ++c) E[k][c] = ema.apply(E[k][c], P[k][c]);
                e4[i] = E[k];
            }
            if (zero_grads) g4[i] = zero4;
        }
        return;
    }
    for (int i = threadIdx.x; i < nvec; i += kBlock) {
        f32x4 P = p4[i], A = zero4, B = zero4, E = zero4;
        if (S > 0) A = a4[i];
        if (S > 1) B = b4[i];
        if (EMA) E = e4[i];
        const f32x4 G = g4[i];
        apply4(r, P, G, A, B);
        p4[i] = P;
        if (S > 0) a4[i] = A;
        if (S > 1) b4[i] = B;
        if (EMA) {
#pragma unroll
            for (int c = 0; c < 4; ++c) E[c] = ema.apply(E[c], P[c]);
            e4[i] = E;
        }
        if (zero_grads) g4[i] = zero4;
    }
    for (int i = nvec * 4 + threadIdx.x; i < cnt; i += kBlock) {       // the tail, and every element of a misaligned tensor
        float P = p[i], A = S > 0 ? s0[i] : 0.f, B = S > 1 ? s1[i] : 0.f;
        const float G = g[i];
        r.apply(P, G, A, B);
        p[i] = P;
        if (S > 0) s0[i] = A;
        if (S > 1) s1[i] = B;
        if (EMA) e[i] = ema.apply(e[i], P);
        if (zero_grads) g[i] = 0.f;
    }
}

// a skipped step's share of zero_grads: the chunk's gradient alone
__device__ __forceinline__ void zero_chunk(float* g_, int cnt) {
    const int nvec = aligned16(g_, nullptr, nullptr, nullptr) ? cnt >> 2 : 0;
    gfloat* __restrict__ g = (gfloat*)g_;
    gfloat4* __restrict__ g4 = (gfloat4*)g_;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < nvec; i += kBlock) g4[i] = zero4;
    for (int i = nvec * 4 + threadIdx.x; i < cnt; i += kBlock) g[i] = 0.f;
}

// coef = min(1, max_norm / (norm + 1e-6)) as torch.nn.utils.clip_grad_norm_ forms it (a NaN norm gives a NaN coef, as there);
// partials == NULL: no clipping.  Whole workgroup, converged.
__device__ __forceinline__ float clip_coef(const double* __restrict__ partials, int npartials, float max_norm,
                                           float* __restrict__ norm_out, double* smem) {
    if (!partials) return 1.0f;
    double acc = 0.0;
    for (int i = threadIdx.x; i < npartials; i += kBlock) acc += partials[i];
    const double norm = sqrt(block_sum(acc, smem));
    if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *(gfloat*)norm_out = (float)norm;
    const double c = (double)max_norm / (norm + 1e-6);
    return !(c >= 1.0) ? (float)c : 1.0f;
}

__global__ __launch_bounds__(kBlock) void k_optim_sgd(const Job* __restrict__ jobs, int n, SgdArgs args,
                                                      const double* __restrict__ partials, int npartials, float max_norm,
                                                      float* __restrict__ norm_out, int zero_grads) {
    __shared__ double smem[kBlock / kWave];
    const float coef = clip_coef(partials, npartials, max_norm, norm_out, smem);
    const int b = blockIdx.x;
    const Job j = jobs[find_job(jobs, n, b)];
    long long start;
    const int cnt = chunk_range(j, b, &start);
    if (cnt <= 0) return;
    const rk_optim_sgd_hyper h = args.g[j.group_flags & (RK_OPTIM_MAX_GROUPS - 1)];
    if (h.momentum != 0.f && j.s0) {
        const SgdRule<true> r{coef, h.lr, h.weight_decay, h.momentum, h.one_minus_dampening, h.nesterov != 0,
                              (j.group_flags & kFirstStep) != 0};
        run_chunk(r, j.p + start, j.g + start, j.s0 + start, nullptr, cnt, zero_grads != 0);
    } else {
        const SgdRule<false> r{coef, h.lr, h.weight_decay, 0.f, 0.f, false, false};
        run_chunk(r, j.p + start, j.g + start, nullptr, nullptr, cnt, zero_grads != 0);
    }
}

__global__ __launch_bounds__(kBlock) void k_optim_adam(const Job* __restrict__ jobs, int n, AdamArgs args,
                                                       const double* __restrict__ partials, int npartials, float max_norm,
                                                       float* __restrict__ norm_out, int zero_grads) {
    __shared__ double smem[kBlock / kWave];
    const float coef = clip_coef(partials, npartials, max_norm, norm_out, smem);
    const int b = blockIdx.x;
    const Job j = jobs[find_job(jobs, n, b)];
    long long start;
    const int cnt = chunk_range(j, b, &start);
    if (cnt <= 0) return;
    const rk_optim_adam_hyper h = args.g[j.group_flags & (RK_OPTIM_MAX_GROUPS - 1)];
    const AdamRule r{coef, h.step_size, h.weight_decay, h.beta1, h.one_minus_beta1, h.beta2, h.one_minus_beta2, h.eps, h.bc2_sqrt};
    run_chunk(r, j.p + start, j.g + start, j.s0 + start, j.s1 + start, cnt, zero_grads != 0);
}

// ---- the extended step: rule by template, EMA shadows, the non-finite guard ----------------------------------------------
struct AdamWArgs { rk_optim_adamw_hyper g[RK_OPTIM_MAX_GROUPS]; };
struct Ext { float* const* ema; float decay, omd; int guard; long long* skipped; };
typedef __attribute__((address_space(1))) long long gint64;

// clip_coef with the guard's verdict: *skip = the sum of the partials is not finite (the same bits in every workgroup, so
// the same verdict).  Thread 0 of workgroup 0 then adds 1 to *skipped: one writer per launch, launches ordered by the
// stream, so a plain load and store.  Whole workgroup, converged.
__device__ __forceinline__ float clip_coef_guarded(const double* __restrict__ partials, int npartials, float max_norm,
                                                   float* __restrict__ norm_out, int guard, long long* skipped, double* smem,
                                                   bool* skip) {
    *skip = false;
    if (!partials) return 1.0f;
    double acc = 0.0;
    for (int i = threadIdx.x; i < npartials; i += kBlock) acc += partials[i];
    const double sum = block_sum(acc, smem);
    const double norm = sqrt(sum);
    if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) *(gfloat*)norm_out = (float)norm;
    if (guard && !(fabs(sum) < __builtin_inf())) {              // NaN or an infinity
        *skip = true;
        if (blockIdx.x == 0 && threadIdx.x == 0) *(gint64*)skipped = *(gint64*)skipped + 1;
        return 1.0f;
    }
    const double c = (double)max_norm / (norm + 1e-6);
    return !(c >= 1.0) ? (float)c : 1.0f;
}

template <int RULE, bool EMA, class Args>
__global__ __launch_bounds__(kBlock) void k_optim_ext(const Job* __restrict__ jobs, int n, Args args,
                                                      const double* __restrict__ partials, int npartials, float max_norm,
                                                      float* __restrict__ norm_out, int zero_grads, Ext x) {
    __shared__ double smem[kBlock / kWave];
    bool skip;
    const float coef = clip_coef_guarded(partials, npartials, max_norm, norm_out, x.guard, x.skipped, smem, &skip);
    const int b = blockIdx.x;
    const int idx = find_job(jobs, n, b);
    const Job j = jobs[idx];
    long long start;
    const int cnt = chunk_range(j, b, &start);
    if (cnt <= 0) return;
    float* const g = j.g + start;
    if (skip) {                                         // nothing but the gradients is written
        if (zero_grads) zero_chunk(g, cnt);
        return;
    }
    const bool zg = zero_grads != 0;
    float* e = nullptr;
    if (EMA) {
        e = x.ema[idx];                                 // (block-uniform; NULL: this tensor has no shadow)
        if (e) e += start;
    }
    const Ema ema{x.decay, x.omd};
    const auto h = args.g[j.group_flags & (RK_OPTIM_MAX_GROUPS - 1)];
    if constexpr (RULE == RK_OPTIM_RULE_SGD) {
        if (h.momentum != 0.f && j.s0) {
            const SgdRule<true> r{coef, h.lr, h.weight_decay, h.momentum, h.one_minus_dampening, h.nesterov != 0,
                                  (j.group_flags & kFirstStep) != 0};
            if (EMA && e) run_chunk<SgdRule<true>, true>(r, j.p + start, g, j.s0 + start, nullptr, cnt, zg, e, ema);
            else run_chunk(r, j.p + start, g, j.s0 + start, nullptr, cnt, zg);
        } else {
            const SgdRule<false> r{coef, h.lr, h.weight_decay, 0.f, 0.f, false, false};
            if (EMA && e) run_chunk<SgdRule<false>, true>(r, j.p + start, g, nullptr, nullptr, cnt, zg, e, ema);
            else run_chunk(r, j.p + start, g, nullptr, nullptr, cnt, zg);
        }
    } else if constexpr (RULE == RK_OPTIM_RULE_ADAM) {
        const AdamRule r{coef, h.step_size, h.weight_decay, h.beta1, h.one_minus_beta1, h.beta2, h.one_minus_beta2, h.eps, h.bc2_sqrt};
        if (EMA && e) run_chunk<AdamRule, true>(r, j.p + start, g, j.s0 + start, j.s1 + start, cnt, zg, e, ema);
        else run_chunk(r, j.p + start, g, j.s0 + start, j.s1 + start, cnt, zg);
    } else {
        const AdamWRule r{coef, h.step_size, h.decay_factor, h.beta1, h.one_minus_beta1, h.beta2, h.one_minus_beta2, h.eps, h.bc2_sqrt};
        if (EMA && e) run_chunk<AdamWRule, true>(r, j.p + start, g, j.s0 + start, j.s1 + start, cnt, zg, e, ema);
        else run_chunk(r, j.p + start, g, j.s0 + start, j.s1 + start, cnt, zg);
    }
}

static int check_table(const void* jobs, int n, int chunks) {
    if (!jobs) return RK_ERR_NULL_POINTER;
    if (n <= 0 || chunks < 0 || ((uintptr_t)jobs & 7)) return RK_ERR_BAD_DIMS;
    return RK_OK;
}

template <class Args, class Hyper, class Kernel>
static int step(Kernel kernel, const void* jobs, int n, int chunks, const Hyper* hyper, int ngroups, const double* partials,
                int npartials, float max_norm, float* norm_out, int zero_grads, rk_stream_t stream) {
    if (!hyper) return RK_ERR_NULL_POINTER;
    if (const int rc = check_table(jobs, n, chunks)) return rc;
    if (ngroups <= 0 || (partials && (npartials <= 0 || ((uintptr_t)partials & 7)))) return RK_ERR_BAD_DIMS;
    if (ngroups > RK_OPTIM_MAX_GROUPS) return RK_ERR_UNSUPPORTED;
    if (chunks == 0) return RK_OK;                      // every tensor is empty
    Args args;
    memset(&args, 0, sizeof(args));
    for (int i = 0; i < ngroups; ++i) args.g[i] = hyper[i];
    hipLaunchKernelGGL(kernel, dim3(chunks), dim3(kBlock), 0, (hipStream_t)stream, (const Job*)jobs, n, args, partials,
                       npartials, max_norm, norm_out, zero_grads);
    return launch_status();
}

template <int RULE, class Args, class Hyper>
static int launch_ext(const void* jobs, int n, int chunks, const void* hyper, int ngroups, const double* partials, int npartials,
                      float max_norm, float* norm_out, int zero_grads, const Ext& x, rk_stream_t stream) {
    Args args;
    memset(&args, 0, sizeof(args));
    for (int i = 0; i < ngroups; ++i) args.g[i] = ((const Hyper*)hyper)[i];
    if (x.ema)
        hipLaunchKernelGGL((k_optim_ext<RULE, true, Args>), dim3(chunks), dim3(kBlock), 0, (hipStream_t)stream, (const Job*)jobs, n,
                           args, partials, npartials, max_norm, norm_out, zero_grads, x);
    else
        hipLaunchKernelGGL((k_optim_ext<RULE, false, Args>), dim3(chunks), dim3(kBlock), 0, (hipStream_t)stream, (const Job*)jobs, n,
                           args, partials, npartials, max_norm, norm_out, zero_grads, x);
    return launch_status();
}

}  // namespace optim
}  // namespace rk

using namespace rk;
using namespace rk::optim;

extern "C" {

int rk_debug_optim_chunks(const long long* numels, int n, int* out) {
    if (!numels || !out) return RK_ERR_NULL_POINTER;
    if (n <= 0) return RK_ERR_BAD_DIMS;
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        if (numels[i] < 0) return RK_ERR_BAD_DIMS;
        out[2 + i] = (int)total;
        total += (numels[i] + kChunk - 1) / kChunk;
        if (total > 0x7fffffffLL) return RK_ERR_BAD_DIMS;
    }
    out[0] = kChunk;
    out[1] = (int)total;
    return RK_OK;
}

size_t rk_optim_sqnorm_workspace_bytes(int chunks) { return chunks > 0 ? (size_t)chunks * sizeof(double) : 0; }

int rk_optim_sqnorm_many_f32(const void* jobs, int n, int chunks, double* partials, rk_stream_t stream) {
    if (!partials) return RK_ERR_WORKSPACE;
    if (const int rc = check_table(jobs, n, chunks)) return rc;
    if ((uintptr_t)partials & 7) return RK_ERR_BAD_DIMS;
    if (chunks == 0) return RK_OK;
    hipLaunchKernelGGL(k_optim_sqnorm, dim3(chunks), dim3(kBlock), 0, (hipStream_t)stream, (const Job*)jobs, n, partials);
    return launch_status();
}

int rk_optim_sgd_many_f32(const void* jobs, int n, int chunks, const rk_optim_sgd_hyper* hyper, int ngroups,
                          const double* partials, int npartials, float max_norm, float* norm_out, int zero_grads,
                          rk_stream_t stream) {
    return step<SgdArgs>(k_optim_sgd, jobs, n, chunks, hyper, ngroups, partials, npartials, max_norm, norm_out, zero_grads, stream);
}

int rk_optim_adam_many_f32(const void* jobs, int n, int chunks, const rk_optim_adam_hyper* hyper, int ngroups,
                           const double* partials, int npartials, float max_norm, float* norm_out, int zero_grads,
                           rk_stream_t stream) {
    return step<AdamArgs>(k_optim_adam, jobs, n, chunks, hyper, ngroups, partials, npartials, max_norm, norm_out, zero_grads, stream);
}

int rk_optim_step_ext_f32(int rule, const void* jobs, int n, int chunks, const void* hyper, int ngroups, const double* partials,
                          int npartials, float max_norm, float* norm_out, int zero_grads, const void* ema, float ema_decay,
                          float ema_one_minus_decay, int guard, long long* skipped, rk_stream_t stream) {
    if (!hyper) return RK_ERR_NULL_POINTER;
    if (const int rc = check_table(jobs, n, chunks)) return rc;
    if (rule != RK_OPTIM_RULE_SGD && rule != RK_OPTIM_RULE_ADAM && rule != RK_OPTIM_RULE_ADAMW) return RK_ERR_UNSUPPORTED;
    if (ngroups <= 0 || (partials && (npartials <= 0 || ((uintptr_t)partials & 7)))) return RK_ERR_BAD_DIMS;
    if (guard && !partials) return RK_ERR_WORKSPACE;
    if (guard && !skipped) return RK_ERR_NULL_POINTER;
    if (((uintptr_t)ema & 7) || (guard && ((uintptr_t)skipped & 7))) return RK_ERR_BAD_DIMS;
    if (ngroups > RK_OPTIM_MAX_GROUPS) return RK_ERR_UNSUPPORTED;
    if (chunks == 0) return RK_OK;                      // every tensor is empty
    const Ext x{(float* const*)ema, ema_decay, ema_one_minus_decay, guard != 0, guard ? skipped : nullptr};
    if (rule == RK_OPTIM_RULE_SGD)
        return launch_ext<RK_OPTIM_RULE_SGD, SgdArgs, rk_optim_sgd_hyper>(jobs, n, chunks, hyper, ngroups, partials, npartials,
                                                                          max_norm, norm_out, zero_grads, x, stream);
    if (rule == RK_OPTIM_RULE_ADAM)
        return launch_ext<RK_OPTIM_RULE_ADAM, AdamArgs, rk_optim_adam_hyper>(jobs, n, chunks, hyper, ngroups, partials, npartials,
                                                                             max_norm, norm_out, zero_grads, x, stream);
    return launch_ext<RK_OPTIM_RULE_ADAMW, AdamWArgs, rk_optim_adamw_hyper>(jobs, n, chunks, hyper, ngroups, partials, npartials,
                                                                            max_norm, norm_out, zero_grads, x, stream);
}

}  // extern "C"
