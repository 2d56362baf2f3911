// FISTA (hyp/optim=fista, reference additional_optimizers/fista.py:44-82: Nesterov-accelerated deterministic gradient descent with the explicit
// t_k sequence, FISTA-MOD / lazy FISTA included; projection None) as ONE pass over the arena: (theta, grad, x_minus) -> (theta', x_minus') with the
// global-norm clip of the consumer fused like in fb_mt_clip_sgd / fb_mt_adamw.  Per element, every operation written out and rounded on its own,
// as the reference's tensor operations round (no fma anywhere), identically in the vector body and the scalar edges:
//   g  = coef != 1 ? coef * grad : grad
//   xp = theta - g * lr                                        x+ = param - grad * lr
//   theta'   = xp * one_plus_ak - x_minus * ak                 param = x+ * (1 + ak) - x- * ak
//   x_minus' = xp
// ak = (tk - 1) / tk' and one_plus_ak = 1 + ak come from the host (float32, the same for every tensor).  The first step has ak = 0, so theta' =
// xp * 1 - x_minus * 0 = xp as long as x_minus is finite (the engine clones theta into it).  theta = g = x_minus = 0 (alignment padding of the
// arena) stays 0.  HBM-bound: 12 B read and 8 B written per element without a clip, as fb_mt_clip_sgd with momentum.  One owner per element, no
// atomics: the result does not depend on the grid.  16-byte loads / stores on the body that is aligned in all three operands, scalar head and
// tail (arena_pass): any offset into the arena and any n work.
#include "arena_update.h"

namespace {

struct FistaHyp { float coef, lr, ak, opak; };

// A product that has been rounded: the value passes through an empty asm statement, so that no later subtraction can be contracted with the
// multiplication into an fma.  (hipcc builds with -ffp-contract=fast, under which the backend fuses across statements whatever the pragma below
// says, and __fmul_rn / __fsub_rn are plain operators to it: without this the body computed fma(-lr, g, theta).)  It emits no instruction.
__device__ __forceinline__ float rounded(float x) {
    asm("" : "+v"(x));
    return x;
}

__device__ __forceinline__ void fista_update(const FistaHyp& h, float p, float g, float xm, float& p_out, float& g_out, float& xm_out) {
#pragma clang fp contract(off)
    g_out = h.coef != 1.f ? __fmul_rn(h.coef, g) : g;
    xm_out = __fsub_rn(p, rounded(__fmul_rn(g_out, h.lr)));
    p_out = __fsub_rn(rounded(__fmul_rn(xm_out, h.opak)), rounded(__fmul_rn(xm, h.ak)));
}

__global__ __launch_bounds__(256) void mt_fista_kernel(float* __restrict__ theta, float* __restrict__ grad, float* __restrict__ x_minus, long long n,
                                                       long long head, long long n4, const float* __restrict__ gnorm2, float grad_clip,
                                                       int torch_clip, float lr, float ak, float one_plus_ak) {
    FistaHyp h;
    h.coef = fb_clip_coef(gnorm2, grad_clip, torch_clip);
    h.lr = lr; h.ak = ak; h.opak = one_plus_ak;
    float* const op[3] = {theta, grad, x_minus};
    arena_pass(op, n, head, n4, !torch_clip && h.coef != 1.f, [&h](float (&x)[3]) { fista_update(h, x[0], x[1], x[2], x[0], x[1], x[2]); });
}

inline bool finite_f(float x) { return x - x == 0.f; }     // (false for inf and NaN; <cmath>'s isfinite is a device overload here)

}  // namespace

extern "C" int fb_mt_fista(float* theta, float* grad, float* x_minus, int64_t n, const float* gnorm2, float grad_clip, int32_t torch_clip, float lr,
                           float ak, float one_plus_ak, void* stream) {
    if (!theta || !grad || !x_minus) FB_FAIL(FB_ERR_ARG, "fb_mt_fista: null pointer");
    if (grad_clip >= 0.f && !gnorm2) FB_FAIL(FB_ERR_ARG, "fb_mt_fista: clipping needs the device norm");
    if (n < 0) FB_FAIL(FB_ERR_ARG, "fb_mt_fista: n=%lld", (long long)n);
    if (!(lr >= 0.f) || !finite_f(lr)) FB_FAIL(FB_ERR_ARG, "fb_mt_fista: lr=%g must be finite and not negative", (double)lr);
    if (!finite_f(ak) || !finite_f(one_plus_ak)) FB_FAIL(FB_ERR_ARG, "fb_mt_fista: ak=%g / one_plus_ak=%g must be finite", (double)ak, (double)one_plus_ak);
    if (((uintptr_t)theta | (uintptr_t)grad | (uintptr_t)x_minus) & 3) FB_FAIL(FB_ERR_ARG, "fb_mt_fista: 4-byte alignment required");
    if (n == 0) return FB_OK;
    const ArenaSplit s = arena_split({theta, grad, x_minus}, n);
    hipLaunchKernelGGL(mt_fista_kernel, dim3(s.blocks), dim3(256), 0, (hipStream_t)stream, theta, grad, x_minus, (long long)n, s.head, s.n4, gnorm2,
                       grad_clip, (int)torch_clip, lr, ak, one_plus_ak);
    FB_CHECK_LAUNCH("fb_mt_fista");
    return FB_OK;
}
