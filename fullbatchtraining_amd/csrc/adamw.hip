// AdamW (hyp/optim=adam, reference optimizers.py:39-40 -> torch.optim.AdamW, single-tensor form, amsgrad=False, maximize=False) as ONE pass over
// the arena: (theta, grad, exp_avg, exp_avg_sq) -> (theta', exp_avg', exp_avg_sq') with the global-norm clip of the consumer fused like in
// fb_mt_clip_sgd / fb_mt_sgd_torch.  Per element, every contraction written out so that the rounding is the same in the vector body and the
// scalar edges (and does not depend on what the compiler fuses):
//   g  = coef != 1 ? coef * grad : grad
//   p1 = p * fma(-lr, wd, 1)                                   param.mul_(1 - lr * weight_decay)
//   m' = fma(1 - beta1, g, beta1 * m)                          exp_avg
//   v' = fma((1 - beta2) * g, g, beta2 * v)                    exp_avg_sq
//   p' = fma(-step_size, m' / (sqrtf(v') / bc2_sqrt + eps), p1)     IEEE division and square root
// step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) come from the host (formed in double from the step count t).  step_size == 0
// (lr 0: step 0 of a warm-up) leaves p' = p1 = p bit for bit while m, v advance.  g = m = v = p = 0 (alignment padding of the arena) stays 0.
// HBM-bound: 16 B read and 12 B written per element without a clip.  One owner per element, no atomics: the result does not depend on the grid.
// 16-byte loads / stores on the body that is aligned in all four operands, scalar head and tail: any offset into the arena and any n work.
#include "common.h"

namespace {

struct AdamHyp { float coef, decay, b1, omb1, b2, omb2, eps, step_size, bc2s; };

__device__ __forceinline__ void adamw_update(const AdamHyp& h, float p, float g, float m, float v, float& p_out, float& g_out, float& m_out, float& v_out) {
#pragma clang fp contract(off)     // (__fmul_rn / __fadd_rn are plain operators to hipcc: nothing below may be fused beyond the fmas written out)
    g_out = h.coef != 1.f ? __fmul_rn(h.coef, g) : g;
    const float p1 = __fmul_rn(p, h.decay);
    m_out = __fmaf_rn(h.omb1, g_out, __fmul_rn(h.b1, m));
    v_out = __fmaf_rn(__fmul_rn(h.omb2, g_out), g_out, __fmul_rn(h.b2, v));
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v_out), h.bc2s), h.eps);
    p_out = h.step_size != 0.f ? __fmaf_rn(-h.step_size, __fdiv_rn(m_out, denom), p1) : p1;
}

__global__ __launch_bounds__(256) void mt_adamw_kernel(float* __restrict__ theta, float* __restrict__ grad, float* __restrict__ exp_avg,
                                                       float* __restrict__ exp_avg_sq, long long n, long long head, long long n4,
                                                       const float* __restrict__ gnorm2, float grad_clip, int torch_clip, float lr, float wd,
                                                       float b1, float b2, float eps, float step_size, float bc2s) {
    AdamHyp h;
    h.coef = 1.f;
    if (grad_clip >= 0.f) {
        const float norm = sqrtf(gnorm2[0]);
        const float c = grad_clip / (norm + 1e-6f);
        if (torch_clip) h.coef = c < 1.f ? c : 1.f;            // clip_grad_norm_: min(1, clip / (norm + 1e-6))
        else if (norm > grad_clip) h.coef = c;                 // _modify_gradient_params: if norm > clip
    }
    const bool write_grad = !torch_clip && h.coef != 1.f;      // (the full-batch closure clips p.grad in place; clip_grad_norm_'s consumer reads only)
    h.decay = __fmaf_rn(-lr, wd, 1.f);
    h.b1 = b1; h.omb1 = 1.f - b1; h.b2 = b2; h.omb2 = 1.f - b2; h.eps = eps; h.step_size = step_size; h.bc2s = bc2s;
    const long long gtid = (long long)blockIdx.x * 256 + threadIdx.x, gsize = (long long)gridDim.x * 256;
    // ---- the body: elements [head, head + 4 n4), 16-byte aligned in every operand
    float4* t4 = (float4*)(theta + head); float4* g4 = (float4*)(grad + head);
    float4* m4 = (float4*)(exp_avg + head); float4* v4 = (float4*)(exp_avg_sq + head);
    for (long long i = gtid; i < n4; i += gsize) {
        const float4 p = t4[i], g = g4[i], m = m4[i], v = v4[i];
        float4 po, go, mo, vo;
        adamw_update(h, p.x, g.x, m.x, v.x, po.x, go.x, mo.x, vo.x); adamw_update(h, p.y, g.y, m.y, v.y, po.y, go.y, mo.y, vo.y);
        adamw_update(h, p.z, g.z, m.z, v.z, po.z, go.z, mo.z, vo.z); adamw_update(h, p.w, g.w, m.w, v.w, po.w, go.w, mo.w, vo.w);
        t4[i] = po; m4[i] = mo; v4[i] = vo;
        if (write_grad) g4[i] = go;
    }
    // ---- the edges: [0, head) and [head + 4 n4, n), one element per thread
    const long long tail0 = head + 4 * n4, edges = head + (n - tail0);
    for (long long e = gtid; e < edges; e += gsize) {
        const long long i = e < head ? e : tail0 + (e - head);
        float po, go, mo, vo;
        adamw_update(h, theta[i], grad[i], exp_avg[i], exp_avg_sq[i], po, go, mo, vo);
        theta[i] = po; exp_avg[i] = mo; exp_avg_sq[i] = vo;
        if (write_grad) grad[i] = go;
    }
}

}  // namespace

extern "C" int fb_mt_adamw(float* theta, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* gnorm2, float grad_clip,
                           int32_t torch_clip, float lr, float weight_decay, float beta1, float beta2, float eps, float step_size,
                           float bc2_sqrt, void* stream) {
    if (!theta || !grad || !exp_avg || !exp_avg_sq) FB_FAIL(FB_ERR_ARG, "fb_mt_adamw: null pointer");
    if (grad_clip >= 0.f && !gnorm2) FB_FAIL(FB_ERR_ARG, "fb_mt_adamw: clipping needs the device norm");
    if (n < 0) FB_FAIL(FB_ERR_ARG, "fb_mt_adamw: n=%lld", (long long)n);
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) FB_FAIL(FB_ERR_ARG, "fb_mt_adamw: betas (%g, %g) outside [0, 1)", (double)beta1, (double)beta2);
    if (!(eps > 0.f)) FB_FAIL(FB_ERR_ARG, "fb_mt_adamw: eps=%g must be positive", (double)eps);
    if (!(bc2_sqrt > 0.f)) FB_FAIL(FB_ERR_ARG, "fb_mt_adamw: bc2_sqrt=%g must be positive (sqrt(1 - beta2^t), t >= 1)", (double)bc2_sqrt);
    if (((uintptr_t)theta | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 3) FB_FAIL(FB_ERR_ARG, "fb_mt_adamw: 4-byte alignment required");
    if (n == 0) return FB_OK;
    // the vector body needs one misalignment shared by the four operands (ranges of the arenas at one offset have it); otherwise all scalar
    const unsigned mis = (unsigned)((uintptr_t)theta & 15);
    const bool same = ((uintptr_t)grad & 15) == mis && ((uintptr_t)exp_avg & 15) == mis && ((uintptr_t)exp_avg_sq & 15) == mis;
    long long head = same ? ((16 - mis) & 15) / 4 : (long long)n;
    if (head > n) head = n;
    const long long n4 = (n - head) / 4;
    const long long work = n4 > 0 ? n4 : n, want = (work + 255) / 256;
    const unsigned nb = (unsigned)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
    hipLaunchKernelGGL(mt_adamw_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, theta, grad, exp_avg, exp_avg_sq, (long long)n, head, n4, gnorm2,
                       grad_clip, (int)torch_clip, lr, weight_decay, beta1, beta2, eps, step_size, bc2_sqrt);
    FB_CHECK_LAUNCH("fb_mt_adamw");
    return FB_OK;
}
