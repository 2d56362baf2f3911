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
// tail: any offset into the arena and any n work.
#include "common.h"

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
    h.coef = 1.f;
    if (grad_clip >= 0.f) {
        const float norm = sqrtf(gnorm2[0]);
        const float c = grad_clip / (norm + 1e-6f);
        if (torch_clip) h.coef = c < 1.f ? c : 1.f;            // clip_grad_norm_: min(1, clip / (norm + 1e-6))
        else if (norm > grad_clip) h.coef = c;                 // _modify_gradient_params: if norm > clip
    }
    const bool write_grad = !torch_clip && h.coef != 1.f;      // (the full-batch closure clips p.grad in place; clip_grad_norm_'s consumer reads only)
    h.lr = lr; h.ak = ak; h.opak = one_plus_ak;
    const long long gtid = (long long)blockIdx.x * 256 + threadIdx.x, gsize = (long long)gridDim.x * 256;
    // ---- the body: elements [head, head + 4 n4), 16-byte aligned in every operand
    float4* t4 = (float4*)(theta + head); float4* g4 = (float4*)(grad + head); float4* x4 = (float4*)(x_minus + head);
    for (long long i = gtid; i < n4; i += gsize) {
        const float4 p = t4[i], g = g4[i], x = x4[i];
        float4 po, go, xo;
        fista_update(h, p.x, g.x, x.x, po.x, go.x, xo.x); fista_update(h, p.y, g.y, x.y, po.y, go.y, xo.y);
        fista_update(h, p.z, g.z, x.z, po.z, go.z, xo.z); fista_update(h, p.w, g.w, x.w, po.w, go.w, xo.w);
        t4[i] = po; x4[i] = xo;
        if (write_grad) g4[i] = go;
    }
    // ---- the edges: [0, head) and [head + 4 n4, n), one element per thread
    const long long tail0 = head + 4 * n4, edges = head + (n - tail0);
    for (long long e = gtid; e < edges; e += gsize) {
        const long long i = e < head ? e : tail0 + (e - head);
        float po, go, xo;
        fista_update(h, theta[i], grad[i], x_minus[i], po, go, xo);
        theta[i] = po; x_minus[i] = xo;
        if (write_grad) grad[i] = go;
    }
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
    // the vector body needs one misalignment shared by the three operands (ranges of the arenas at one offset have it); otherwise all scalar
    const unsigned mis = (unsigned)((uintptr_t)theta & 15);
    const bool same = ((uintptr_t)grad & 15) == mis && ((uintptr_t)x_minus & 15) == mis;
    long long head = same ? ((16 - mis) & 15) / 4 : (long long)n;
    if (head > n) head = n;
    const long long n4 = (n - head) / 4;
    const long long work = n4 > 0 ? n4 : n, want = (work + 255) / 256;
    const unsigned nb = (unsigned)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
    hipLaunchKernelGGL(mt_fista_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, theta, grad, x_minus, (long long)n, head, n4, gnorm2, grad_clip,
                       (int)torch_clip, lr, ak, one_plus_ak);
    FB_CHECK_LAUNCH("fb_mt_fista");
    return FB_OK;
}
