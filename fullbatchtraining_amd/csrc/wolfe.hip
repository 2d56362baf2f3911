// Strong-Wolfe line search for full-batch gradient descent (hyp.optim.line_search=wolfe, reference additional_optimizers/sgd_linesearch.py:183-381):
// the arithmetic of one search on the flat arena, three HBM-streaming passes.  The search logic itself (trial steps, zoom, cubic interpolation)
// is host code on three scalars per evaluation (training.WolfeSearch).
//
//   fb_mt_wolfe_direction   (theta, grad, mom) -> (mom', p, theta0), out[0] = sum d p          _save_initial_state + _find_descent_direction
//       d    = fma(wd, theta, grad)                                    grad.add(param, alpha=wd)
//       mom' = first ? d : fma(1 - damp, d, rounded(mu mom))           buf.mul_(mu).add_(grad, alpha=1 - damp)
//       p    = -(nesterov ? fma(mu, mom', d) : mom')   (mu = 0: -d)    -grad.add(buf, alpha=mu) / -buf / -grad
//       theta0 = theta                                                 (the value is in a register anyway: the snapshot costs no read)
//   fb_mt_wolfe_trial       theta = fma(step, p, theta0)               _load_initial_state + _foreach_add_(params, p_k, alpha=lr alpha)
//   fb_mt_wolfe_phi_grad    out[0] = sum fma(wd, theta, grad) p        _get_phi_grad
//
// Every product-and-sum is ONE fused multiply-add, written out (__builtin_fmaf) so that the form does not hang on the compiler's contraction:
// it is the form of torch's `add(other, alpha=)` on a CPU with FMA units (recorded in tests/golden/wolfe_optimizer.npz), and instruction by
// instruction the form fb_mt_clip_sgd compiles to -- d, mom' and the Nesterov sum have the bits of that kernel without a clip, so the momentum
// arena and checkpoints are interchangeable between line_search none and wolfe.  mu mom is rounded on its own (mul_ is an operation of its own).
//
// The two reductions follow fb_mt_norms2: float partials per workgroup into ws, finished by a second kernel in double in a fixed order.  No
// atomics; the order of the additions depends on n alone, so every launch gives the same bits.  Per lane: one fma chain over the lane's
// elements (4 per 16-byte vector and pass of the grid-stride loop), then the 6-level shuffle tree of the wave, 3 additions across the waves.
// All pointers 16-byte aligned (whole arenas); n % 4 trailing elements are taken by the first lanes of workgroup 0 after their vectors.
#include "common.h"

namespace {

struct DirHyp { float wd, mu, omd; int nesterov, first; };

// a product that has been rounded (see csrc/fista.hip): no later fma may swallow the multiplication
__device__ __forceinline__ float rounded(float x) {
    asm("" : "+v"(x));
    return x;
}

__device__ __forceinline__ float decayed(float wd, float t, float g) { return __builtin_fmaf(wd, t, g); }

// -> d; p_out, m_out (m_out only meaningful for mu != 0)
__device__ __forceinline__ float direction(const DirHyp& h, float t, float g, float m, float& p_out, float& m_out) {
    const float d = decayed(h.wd, t, g);
    if (h.mu != 0.f) {
        const float buf = h.first ? d : __builtin_fmaf(h.omd, d, rounded(h.mu * m));
        m_out = buf;
        p_out = -(h.nesterov ? __builtin_fmaf(h.mu, buf, d) : buf);
    } else {
        m_out = m;
        p_out = -d;
    }
    return d;
}

__global__ __launch_bounds__(FB_WOLFE_BLOCK) void wolfe_direction_kernel(const float* __restrict__ theta, const float* __restrict__ grad,
                                                                         float* __restrict__ mom, float* __restrict__ p, float* __restrict__ theta0,
                                                                         long long n, DirHyp h, float* __restrict__ ws) {
    __shared__ float sm[8];
    const bool has_mom = h.mu != 0.f, read_mom = has_mom && !h.first;
    const long long n4 = n / 4, gtid = (long long)blockIdx.x * FB_WOLFE_BLOCK + threadIdx.x, gsize = (long long)gridDim.x * FB_WOLFE_BLOCK;
    float acc[1] = {0.f};
    for (long long i = gtid; i < n4; i += gsize) {
        const float4 t = ((const float4*)theta)[i], g = ((const float4*)grad)[i];
        const float4 m = read_mom ? ((const float4*)mom)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 po, mo;
        const float dx = direction(h, t.x, g.x, m.x, po.x, mo.x), dy = direction(h, t.y, g.y, m.y, po.y, mo.y);
        const float dz = direction(h, t.z, g.z, m.z, po.z, mo.z), dw = direction(h, t.w, g.w, m.w, po.w, mo.w);
        acc[0] = __builtin_fmaf(dx, po.x, acc[0]); acc[0] = __builtin_fmaf(dy, po.y, acc[0]);
        acc[0] = __builtin_fmaf(dz, po.z, acc[0]); acc[0] = __builtin_fmaf(dw, po.w, acc[0]);
        ((float4*)p)[i] = po; ((float4*)theta0)[i] = t;
        if (has_mom) ((float4*)mom)[i] = mo;
    }
    const long long e = n4 * 4 + gtid;                  // the n % 4 trailing elements: lanes 0..2 of workgroup 0
    if (e < n) {
        float po, mo;
        const float t = theta[e], d = direction(h, t, grad[e], read_mom ? mom[e] : 0.f, po, mo);
        acc[0] = __builtin_fmaf(d, po, acc[0]);
        p[e] = po; theta0[e] = t;
        if (has_mom) mom[e] = mo;
    }
    block_reduce_sum<1>(acc, sm);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(FB_WOLFE_BLOCK) void wolfe_trial_kernel(float* __restrict__ theta, const float* __restrict__ theta0,
                                                                     const float* __restrict__ p, long long n, float step) {
    const long long n4 = n / 4, gtid = (long long)blockIdx.x * FB_WOLFE_BLOCK + threadIdx.x, gsize = (long long)gridDim.x * FB_WOLFE_BLOCK;
    for (long long i = gtid; i < n4; i += gsize) {
        const float4 t = ((const float4*)theta0)[i], d = ((const float4*)p)[i];
        ((float4*)theta)[i] = make_float4(__builtin_fmaf(step, d.x, t.x), __builtin_fmaf(step, d.y, t.y), __builtin_fmaf(step, d.z, t.z),
                                          __builtin_fmaf(step, d.w, t.w));
    }
    const long long e = n4 * 4 + gtid;
    if (e < n) theta[e] = __builtin_fmaf(step, p[e], theta0[e]);
}

__global__ __launch_bounds__(FB_WOLFE_BLOCK) void wolfe_phi_grad_kernel(const float* __restrict__ theta, const float* __restrict__ grad,
                                                                        const float* __restrict__ p, long long n, float wd, float* __restrict__ ws) {
    __shared__ float sm[8];
    const long long n4 = n / 4, gtid = (long long)blockIdx.x * FB_WOLFE_BLOCK + threadIdx.x, gsize = (long long)gridDim.x * FB_WOLFE_BLOCK;
    float acc[1] = {0.f};
    for (long long i = gtid; i < n4; i += gsize) {
        const float4 t = ((const float4*)theta)[i], g = ((const float4*)grad)[i], d = ((const float4*)p)[i];
        acc[0] = __builtin_fmaf(decayed(wd, t.x, g.x), d.x, acc[0]); acc[0] = __builtin_fmaf(decayed(wd, t.y, g.y), d.y, acc[0]);
        acc[0] = __builtin_fmaf(decayed(wd, t.z, g.z), d.z, acc[0]); acc[0] = __builtin_fmaf(decayed(wd, t.w, g.w), d.w, acc[0]);
    }
    const long long e = n4 * 4 + gtid;
    if (e < n) acc[0] = __builtin_fmaf(decayed(wd, theta[e], grad[e]), p[e], acc[0]);
    block_reduce_sum<1>(acc, sm);
    if (threadIdx.x == 0) ws[blockIdx.x] = acc[0];
}

// second stage: out[0] = sum_b ws[b] in double; thread t adds partials t, t + 256, ..., then a fixed binary tree (as mt_finalize_kernel)
__global__ __launch_bounds__(256) void wolfe_finalize_kernel(const float* __restrict__ ws, float* __restrict__ out, int nblocks) {
    __shared__ double sm[256];
    double s = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) s += (double)ws[b];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)sm[0];
}

inline bool finite_f(float x) { return x - x == 0.f; }

inline unsigned wolfe_blocks(int64_t n) {
    const int64_t want = (n / FB_WOLFE_VEC + FB_WOLFE_BLOCK - 1) / FB_WOLFE_BLOCK;
    return (unsigned)(want < 1 ? 1 : (want > FB_MT_BLOCKS ? FB_MT_BLOCKS : want));
}

inline bool aligned16(const void* a, const void* b, const void* c, const void* d = nullptr, const void* e = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) == 0;
}

}  // namespace

extern "C" int fb_mt_wolfe_direction(const float* theta, const float* grad, float* mom, float* p, float* theta0, int64_t n, float weight_decay,
                                     float momentum, float dampening, int32_t nesterov, int32_t first_step, float* out, float* ws, void* stream) {
    if (!theta || !grad || !p || !theta0 || !out || !ws || (!mom && momentum != 0.f)) FB_FAIL(FB_ERR_ARG, "fb_mt_wolfe_direction: null pointer");
    if (n < 0) FB_FAIL(FB_ERR_ARG, "fb_mt_wolfe_direction: n=%lld", (long long)n);
    if (!finite_f(weight_decay) || !finite_f(momentum) || !finite_f(dampening))
        FB_FAIL(FB_ERR_ARG, "fb_mt_wolfe_direction: weight_decay=%g / momentum=%g / dampening=%g must be finite", (double)weight_decay, (double)momentum,
                (double)dampening);
    if (!aligned16(theta, grad, mom, p, theta0)) FB_FAIL(FB_ERR_ARG, "fb_mt_wolfe_direction: 16-byte alignment required");
    const DirHyp h{weight_decay, momentum, 1.f - dampening, nesterov ? 1 : 0, first_step ? 1 : 0};
    const unsigned nb = wolfe_blocks(n);
    hipLaunchKernelGGL(wolfe_direction_kernel, dim3(nb), dim3(FB_WOLFE_BLOCK), 0, (hipStream_t)stream, theta, grad, mom, p, theta0, (long long)n, h, ws);
    hipLaunchKernelGGL(wolfe_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, out, (int)nb);
    FB_CHECK_LAUNCH("fb_mt_wolfe_direction");
    return FB_OK;
}

extern "C" int fb_mt_wolfe_trial(float* theta, const float* theta0, const float* p, int64_t n, float step, void* stream) {
    if (!theta || !theta0 || !p) FB_FAIL(FB_ERR_ARG, "fb_mt_wolfe_trial: null pointer");
    if (n < 0) FB_FAIL(FB_ERR_ARG, "fb_mt_wolfe_trial: n=%lld", (long long)n);
    if (!finite_f(step)) FB_FAIL(FB_ERR_ARG, "fb_mt_wolfe_trial: step=%g must be finite", (double)step);
    if (!aligned16(theta, theta0, p)) FB_FAIL(FB_ERR_ARG, "fb_mt_wolfe_trial: 16-byte alignment required");
    if (n == 0) return FB_OK;
    hipLaunchKernelGGL(wolfe_trial_kernel, dim3(wolfe_blocks(n)), dim3(FB_WOLFE_BLOCK), 0, (hipStream_t)stream, theta, theta0, p, (long long)n, step);
    FB_CHECK_LAUNCH("fb_mt_wolfe_trial");
    return FB_OK;
}

extern "C" int fb_mt_wolfe_phi_grad(const float* theta, const float* grad, const float* p, int64_t n, float weight_decay, float* out, float* ws,
                                    void* stream) {
    if (!theta || !grad || !p || !out || !ws) FB_FAIL(FB_ERR_ARG, "fb_mt_wolfe_phi_grad: null pointer");
    if (n < 0) FB_FAIL(FB_ERR_ARG, "fb_mt_wolfe_phi_grad: n=%lld", (long long)n);
    if (!finite_f(weight_decay)) FB_FAIL(FB_ERR_ARG, "fb_mt_wolfe_phi_grad: weight_decay=%g must be finite", (double)weight_decay);
    if (!aligned16(theta, grad, p)) FB_FAIL(FB_ERR_ARG, "fb_mt_wolfe_phi_grad: 16-byte alignment required");
    const unsigned nb = wolfe_blocks(n);
    hipLaunchKernelGGL(wolfe_phi_grad_kernel, dim3(nb), dim3(FB_WOLFE_BLOCK), 0, (hipStream_t)stream, theta, grad, p, (long long)n, weight_decay, ws);
    hipLaunchKernelGGL(wolfe_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, out, (int)nb);
    FB_CHECK_LAUNCH("fb_mt_wolfe_phi_grad");
    return FB_OK;
}
