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
// 16-byte loads / stores on the body that is aligned in all four operands, scalar head and tail (arena_pass): any offset into the arena and any n work.
#include "arena_update.h"

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
    h.coef = fb_clip_coef(gnorm2, grad_clip, torch_clip);
    h.decay = __fmaf_rn(-lr, wd, 1.f);
    h.b1 = b1; h.omb1 = 1.f - b1; h.b2 = b2; h.omb2 = 1.f - b2; h.eps = eps; h.step_size = step_size; h.bc2s = bc2s;
    float* const op[4] = {theta, grad, exp_avg, exp_avg_sq};
    arena_pass(op, n, head, n4, !torch_clip && h.coef != 1.f, [&h](float (&x)[4]) { adamw_update(h, x[0], x[1], x[2], x[3], x[0], x[1], x[2], x[3]); });
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
    const ArenaSplit s = arena_split({theta, grad, exp_avg, exp_avg_sq}, n);
    hipLaunchKernelGGL(mt_adamw_kernel, dim3(s.blocks), dim3(256), 0, (hipStream_t)stream, theta, grad, exp_avg, exp_avg_sq, (long long)n, s.head, s.n4,
                       gnorm2, grad_clip, (int)torch_clip, lr, weight_decay, beta1, beta2, eps, step_size, bc2_sqrt);
    FB_CHECK_LAUNCH("fb_mt_adamw");
    return FB_OK;
}
