// What the fused update kernels on the arena share: the clip coefficient (every update kernel) and the elementwise pass (fb_mt_adamw, fb_mt_fista).
#pragma once
#include <initializer_list>
#include "common.h"

// The factor of the global-norm clip on the gradient, from the device norm gnorm2[0] = |g|^2; 1 without a clip (grad_clip < 0: gnorm2 is not read).
//   torch_clip = 0: the full-batch closure's form (_modify_gradient_params, reference training.py:198-204): norm > clip ? clip / (norm + 1e-6) : 1
//   torch_clip = 1: torch.nn.utils.clip_grad_norm_'s form: min(1, clip / (norm + 1e-6))
// IEEE square root and division and nothing a contraction could fuse: the same bits in every kernel that calls it.
__device__ __forceinline__ float fb_clip_coef(const float* __restrict__ gnorm2, float grad_clip, int torch_clip) {
    if (!(grad_clip >= 0.f)) return 1.f;
    const float norm = sqrtf(gnorm2[0]);
    const float c = grad_clip / (norm + 1e-6f);
    if (torch_clip) return c < 1.f ? c : 1.f;
    return norm > grad_clip ? c : 1.f;
}

// How arena_pass covers n elements at these addresses: [head, head + 4 n4) as 16-byte accesses, the edges one element per thread.  The body needs
// one misalignment shared by all operands (ranges of the arenas at one offset have it); otherwise all is edge.  At most 2048 workgroups of 256.
struct ArenaSplit { long long head, n4; unsigned blocks; };
inline ArenaSplit arena_split(std::initializer_list<const void*> operands, long long n) {
    const unsigned mis = (unsigned)((uintptr_t)*operands.begin() & 15);
    bool same = true;
    for (const void* p : operands) same = same && ((uintptr_t)p & 15) == mis;
    long long head = same ? ((16 - mis) & 15) / 4 : n;
    if (head > n) head = n;
    const long long n4 = (n - head) / 4;
    const long long work = n4 > 0 ? n4 : n, want = (work + 255) / 256;
    return {head, n4, (unsigned)(want < 1 ? 1 : (want > 2048 ? 2048 : want))};
}

// One pass over N operands of n floats: op[0] is theta, op[1] the gradient, the rest the optimizer's state; update(x) takes element i of every
// operand in x[0..N) and leaves the new values there.  All are written back but the gradient, which is written only with write_grad (the
// full-batch closure clips p.grad in place; clip_grad_norm_'s consumer reads only).  Body and edges call the same update, one owner per element,
// no atomics: its bits depend neither on the split nor on the grid.  (op[] carries no __restrict__; an iteration loads all before it stores any.)
template <int N, typename Update>
__device__ __forceinline__ void arena_pass(float* const (&op)[N], long long n, long long head, long long n4, bool write_grad, const Update& update) {
    const long long gtid = (long long)blockIdx.x * 256 + threadIdx.x, gsize = (long long)gridDim.x * 256;
    for (long long i = gtid; i < n4; i += gsize) {             // ---- the body, 16-byte aligned in every operand
        f32x4_t v[N];
        for (int k = 0; k < N; ++k) v[k] = ((const f32x4_t*)(op[k] + head))[i];
        for (int c = 0; c < 4; ++c) {
            float x[N];
            for (int k = 0; k < N; ++k) x[k] = v[k][c];
            update(x);
            for (int k = 0; k < N; ++k) v[k][c] = x[k];
        }
        for (int k = 0; k < N; ++k)
            if (k != 1 || write_grad) ((f32x4_t*)(op[k] + head))[i] = v[k];
    }
    const long long tail0 = head + 4 * n4, edges = head + (n - tail0);
    for (long long e = gtid; e < edges; e += gsize) {          // ---- the edges, one element per thread
        const long long i = e < head ? e : tail0 + (e - head);
        float x[N];
        for (int k = 0; k < N; ++k) x[k] = op[k][i];
        update(x);
        for (int k = 0; k < N; ++k)
            if (k != 1 || write_grad) op[k][i] = x[k];
    }
}
