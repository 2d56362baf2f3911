// Mini-batch SGD mode (hyp.train_stochastic): the weights change after every block of the loader, so the update and the compute-dtype
// weight copies are wanted once per 128 images instead of once per 50 000.  fb_mt_sgd_prep does both in ONE pass over the arena:
//   (theta, grad, mom) -> (theta', mom')   torch.nn.utils.clip_grad_norm_ + torch.optim.SGD (reference training.py:274-281)
//   theta'             -> forward copy [co][tap][ci_pad] and transposed input-gradient copy [ci][tap][co] of every convolution layer
// instead of fb_mt_clip_sgd + one fb_weight_prep launch per layer, whose transposed copy leaves as 2-byte stores taps*Cout elements apart.
//
// Work items ("tiles"), one workgroup of 256 threads each, enumerated from the device-resident layer table:
//   * a layer tile = 64 output channels x 32 input channels of ONE tap: every thread updates 8 consecutive input channels of one output
//     channel (two 16-byte loads per operand where Cin_real and the offset allow it), writes theta' / mom' / the forward copy from its
//     registers, and parks theta' in LDS as [ci][co]; after the barrier every thread writes 16 contiguous bytes along Cout of the
//     transposed copy (8 bf16 or 4 fp32 values).  One owner per output element, no atomics: the result does not depend on the grid.
//   * a plain tile = 1024 consecutive elements outside every layer (BatchNorm affine parameters, the classifier, alignment gaps): update only.
// Padding columns Cin_real <= ci < Cin_pad of the copies are neither read nor written (the first fb_weight_prep of a run wrote their zeros).
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "arena_update.h"

namespace {

constexpr int SP_TCO = 64, SP_TCI = 32, SP_PLAIN = 1024, SP_MAX_LAYERS = 512, SP_COLS = 8;
enum { T_WOFF = 0, T_COUT = 1, T_TAPS = 2, T_CIN = 3, T_CINP = 4, T_WCOFF = 5, T_DGRAD = 6 };

struct SgdHyp { float coef, lr, wd, mu, one_minus_damp; int nesterov, first; };

// The arithmetic of mt_clip_sgd_kernel (multi_tensor.hip) with the contractions the compiler chose there written out, so that every
// kernel that calls it rounds alike: gr = coef g; d = fma(wd, p, gr); buf = fma(1 - damp, d, mu m); d' = fma(mu, buf, d); p' = fma(-lr, d', p)
__device__ __forceinline__ void sgd_update(const SgdHyp& h, float p, float g, float m, float& p_out, float& m_out) {
    const float gr = h.coef != 1.f ? __fmul_rn(h.coef, g) : g;
    float d = __fmaf_rn(h.wd, p, gr);
    m_out = m;
    if (h.mu != 0.f) {
        const float buf = h.first ? d : __fmaf_rn(h.one_minus_damp, d, __fmul_rn(h.mu, m));
        m_out = buf;
        d = h.nesterov ? __fmaf_rn(h.mu, buf, d) : buf;
    }
    p_out = __fmaf_rn(-h.lr, d, p);
}

struct SpArgs {
    float* theta; const float* grad; float* mom; long long n; const float* gnorm2;
    float grad_clip, lr, wd, mu, damp; int nesterov, first;
    const int* tab; int n_layers; void* w_fwd; void* w_dgrad;
};

__device__ __forceinline__ int sp_layer_tiles(const int* __restrict__ r) {
    return r[T_TAPS] * ((r[T_COUT] + SP_TCO - 1) / SP_TCO) * ((r[T_CIN] + SP_TCI - 1) / SP_TCI);
}

template <typename T> __device__ __forceinline__ T sp_cast(float v) {
    if constexpr (sizeof(T) == 4) return v; else return f32_to_bf16(v);
}

template <typename T>
__global__ __launch_bounds__(256) void mt_sgd_prep_kernel(const SpArgs a) {
    // items 0 .. 2L: item 2k = the gap in front of layer k (item 2L: behind the last layer), item 2k+1 = layer k; pre[i] = tiles of items < i
    __shared__ int pre[2 * SP_MAX_LAYERS + 2];
    __shared__ int bad;
    __shared__ float tile[SP_TCI][SP_TCO + 1];
    const int tid = threadIdx.x, L = a.n_layers, items = 2 * L + 1;
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int i = tid; i < items; i += 256) {
        const int k = i >> 1;
        int cnt;
        if (i & 1) {
            cnt = sp_layer_tiles(a.tab + 8 * k);
        } else {
            long long start = 0, stop = a.n;
            if (k > 0) { const int* r = a.tab + 8 * (k - 1); start = (long long)r[T_WOFF] + (long long)r[T_COUT] * r[T_TAPS] * r[T_CIN]; }
            if (k < L) stop = a.tab[8 * k + T_WOFF];
            if (stop < start || start < 0 || stop > a.n) { bad = 1; stop = start; }      // (the host has refused such a table: never write through it)
            cnt = (int)((stop - start + SP_PLAIN - 1) / SP_PLAIN);
        }
        pre[i + 1] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        pre[0] = 0;
        for (int i = 0; i < items; ++i) pre[i + 1] += pre[i];
    }
    __syncthreads();
    if (bad) return;
    const int total = pre[items];
    SgdHyp h;
    h.coef = fb_clip_coef(a.gnorm2, a.grad_clip, 1);            // (the mini-batch branch clips with clip_grad_norm_)
    h.lr = a.lr; h.wd = a.wd; h.mu = a.mu; h.one_minus_damp = 1.f - a.damp; h.nesterov = a.nesterov; h.first = a.first;
    const bool use_mom = a.mu != 0.f;

    for (int tile_id = blockIdx.x; tile_id < total; tile_id += gridDim.x) {
        int lo = 0, hi = items - 1;                  // the item with pre[item] <= tile_id < pre[item + 1]
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pre[mid] <= tile_id) lo = mid; else hi = mid - 1;
        }
        const int item = lo, local = tile_id - pre[item], k = item >> 1;
        if (!(item & 1)) {
            // ---- plain range: update only ------------------------------------------------------------------------------------------
            long long start = 0, stop = a.n;
            if (k > 0) { const int* r = a.tab + 8 * (k - 1); start = (long long)r[T_WOFF] + (long long)r[T_COUT] * r[T_TAPS] * r[T_CIN]; }
            if (k < L) stop = a.tab[8 * k + T_WOFF];
            const long long base = start + (long long)local * SP_PLAIN + 4 * tid;
            if ((base & 3) == 0 && base + 4 <= stop) {
                const float4 p = *(const float4*)(a.theta + base), g = *(const float4*)(a.grad + base);
                float4 m = make_float4(0.f, 0.f, 0.f, 0.f), po, mo;
                if (use_mom && !a.first) m = *(const float4*)(a.mom + base);
                sgd_update(h, p.x, g.x, m.x, po.x, mo.x); sgd_update(h, p.y, g.y, m.y, po.y, mo.y);
                sgd_update(h, p.z, g.z, m.z, po.z, mo.z); sgd_update(h, p.w, g.w, m.w, po.w, mo.w);
                *(float4*)(a.theta + base) = po;
                if (use_mom) *(float4*)(a.mom + base) = mo;
            } else {
                for (int j = 0; j < 4; ++j) {
                    const long long e = base + j;
                    if (e >= stop) break;
                    float po, mo;
                    sgd_update(h, a.theta[e], a.grad[e], (use_mom && !a.first) ? a.mom[e] : 0.f, po, mo);
                    a.theta[e] = po;
                    if (use_mom) a.mom[e] = mo;
                }
            }
            continue;
        }
        // ---- layer tile ------------------------------------------------------------------------------------------------------------
        const int* r = a.tab + 8 * k;
        const long long w_off = r[T_WOFF], wc_off = r[T_WCOFF];
        const int Cout = r[T_COUT], taps = r[T_TAPS], Cin = r[T_CIN], Cin_pad = r[T_CINP];
        const bool dgrad = r[T_DGRAD] != 0;
        const int n_ci_t = (Cin + SP_TCI - 1) / SP_TCI;
        int tl = local;
        const int ci_t = tl % n_ci_t; tl /= n_ci_t;
        const int t = tl % taps, co_t = tl / taps;
        const int row = tid >> 2, c8 = (tid & 3) * SP_COLS;
        const int co = co_t * SP_TCO + row, ci = ci_t * SP_TCI + c8;
        float v[SP_COLS];
        int n_valid = 0;                             // this thread's columns ci .. ci + n_valid - 1 exist
        if (co < Cout && ci < Cin) {
            n_valid = Cin - ci < SP_COLS ? Cin - ci : SP_COLS;
            const long long e0 = w_off + ((long long)co * taps + t) * Cin + ci;
            const bool vec_in = ((w_off | Cin) & 3) == 0;
#pragma unroll
            for (int hlf = 0; hlf < 2; ++hlf) {
                const long long e = e0 + 4 * hlf;
                float mo[4];
                if (vec_in && 4 * hlf + 4 <= n_valid) {
                    const float4 p = *(const float4*)(a.theta + e), g = *(const float4*)(a.grad + e);
                    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (use_mom && !a.first) m = *(const float4*)(a.mom + e);
                    sgd_update(h, p.x, g.x, m.x, v[4 * hlf + 0], mo[0]); sgd_update(h, p.y, g.y, m.y, v[4 * hlf + 1], mo[1]);
                    sgd_update(h, p.z, g.z, m.z, v[4 * hlf + 2], mo[2]); sgd_update(h, p.w, g.w, m.w, v[4 * hlf + 3], mo[3]);
                    *(float4*)(a.theta + e) = make_float4(v[4 * hlf + 0], v[4 * hlf + 1], v[4 * hlf + 2], v[4 * hlf + 3]);
                    if (use_mom) *(float4*)(a.mom + e) = make_float4(mo[0], mo[1], mo[2], mo[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[4 * hlf + j] = 0.f;
                        if (4 * hlf + j < n_valid) {
                            sgd_update(h, a.theta[e + j], a.grad[e + j], (use_mom && !a.first) ? a.mom[e + j] : 0.f, v[4 * hlf + j], mo[j]);
                            a.theta[e + j] = v[4 * hlf + j];
                            if (use_mom) a.mom[e + j] = mo[j];
                        }
                    }
                }
            }
            // forward copy [co][tap][ci_pad]: 16 bytes per store where the row allows it
            T* wf = (T*)a.w_fwd + wc_off + ((long long)co * taps + t) * Cin_pad + ci;
            const bool vec_out = ((wc_off | Cin_pad) & 7) == 0;
            if constexpr (sizeof(T) == 4) {
#pragma unroll
                for (int hlf = 0; hlf < 2; ++hlf) {
                    if (vec_out && 4 * hlf + 4 <= n_valid) *(float4*)(wf + 4 * hlf) = make_float4(v[4 * hlf + 0], v[4 * hlf + 1], v[4 * hlf + 2], v[4 * hlf + 3]);
                    else
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (4 * hlf + j < n_valid) wf[4 * hlf + j] = v[4 * hlf + j];
                }
            } else {
                if (vec_out && n_valid == SP_COLS) {
                    uint4 o;
                    o.x = (unsigned)f32_to_bf16(v[0]) | ((unsigned)f32_to_bf16(v[1]) << 16); o.y = (unsigned)f32_to_bf16(v[2]) | ((unsigned)f32_to_bf16(v[3]) << 16);
                    o.z = (unsigned)f32_to_bf16(v[4]) | ((unsigned)f32_to_bf16(v[5]) << 16); o.w = (unsigned)f32_to_bf16(v[6]) | ((unsigned)f32_to_bf16(v[7]) << 16);
                    *(uint4*)wf = o;
                } else {
#pragma unroll
                    for (int j = 0; j < SP_COLS; ++j)
                        if (j < n_valid) wf[j] = f32_to_bf16(v[j]);
                }
            }
        }
        if (!dgrad) continue;                        // (uniform over the workgroup: a property of the tile's layer)
#pragma unroll
        for (int j = 0; j < SP_COLS; ++j)
            if (j < n_valid) tile[c8 + j][row] = v[j];
        __syncthreads();
        // transposed copy [ci][tap][co]: runs of 16 bytes along Cout
        constexpr int RUN = 16 / sizeof(T), RUNS_PER_ROW = SP_TCO / RUN;
        const bool vec_t = ((wc_off | Cout) & 7) == 0;
#pragma unroll
        for (int q = tid; q < SP_TCI * RUNS_PER_ROW; q += 256) {
            const int ci_l = q / RUNS_PER_ROW, co_l = (q % RUNS_PER_ROW) * RUN;
            const int cj = ci_t * SP_TCI + ci_l, cb = co_t * SP_TCO + co_l;
            if (cj >= Cin || cb >= Cout) continue;
            T* wd = (T*)a.w_dgrad + wc_off + ((long long)cj * taps + t) * Cout + cb;
            if (vec_t && cb + RUN <= Cout) {
                if constexpr (sizeof(T) == 4) {
                    *(float4*)wd = make_float4(tile[ci_l][co_l], tile[ci_l][co_l + 1], tile[ci_l][co_l + 2], tile[ci_l][co_l + 3]);
                } else {
                    uint4 o;
                    o.x = (unsigned)f32_to_bf16(tile[ci_l][co_l + 0]) | ((unsigned)f32_to_bf16(tile[ci_l][co_l + 1]) << 16);
                    o.y = (unsigned)f32_to_bf16(tile[ci_l][co_l + 2]) | ((unsigned)f32_to_bf16(tile[ci_l][co_l + 3]) << 16);
                    o.z = (unsigned)f32_to_bf16(tile[ci_l][co_l + 4]) | ((unsigned)f32_to_bf16(tile[ci_l][co_l + 5]) << 16);
                    o.w = (unsigned)f32_to_bf16(tile[ci_l][co_l + 6]) | ((unsigned)f32_to_bf16(tile[ci_l][co_l + 7]) << 16);
                    *(uint4*)wd = o;
                }
            } else {
                for (int j = 0; j < RUN && cb + j < Cout; ++j) wd[j] = sp_cast<T>(tile[ci_l][co_l + j]);
            }
        }
        __syncthreads();                             // (the next tile of this workgroup parks its values in the same LDS)
    }
}

// the update alone, torch clip form, gradient read only: the update step of the composition the fused pass is measured against
__global__ __launch_bounds__(256) void mt_sgd_torch_kernel(float* __restrict__ theta, const float* __restrict__ grad, float* __restrict__ mom,
                                                           long long n, const float* __restrict__ gnorm2, float grad_clip, float lr, float wd,
                                                           float mu, float damp, int nesterov, int first) {
    SgdHyp h;
    h.coef = fb_clip_coef(gnorm2, grad_clip, 1);
    h.lr = lr; h.wd = wd; h.mu = mu; h.one_minus_damp = 1.f - damp; h.nesterov = nesterov; h.first = first;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float po, mo;
        sgd_update(h, theta[i], grad[i], (mu != 0.f && !first) ? mom[i] : 0.f, po, mo);
        theta[i] = po;
        if (mu != 0.f) mom[i] = mo;
    }
}

// Host copies of the layer tables seen so far, by (address, rows): the table lives on the device, its checks and the grid size are the
// host's.  The first call with a table reads it back (one blocking copy); later calls do not touch the stream.  The kernel enumerates
// its tiles from the DEVICE table and walks them grid-stride, so a host copy that went stale (another table at a recycled address) costs
// a re-check at most, never a stray write.
struct TabInfo { int rc; long long tiles; bool dgrad; };
std::map<std::pair<const void*, int>, TabInfo> g_tabs;
std::mutex g_tabs_mutex;

int check_table(const std::vector<int32_t>& tab, int n_layers, int64_t n, long long* tiles) {
    long long end = 0, total = 0;
    for (int k = 0; k < n_layers; ++k) {
        const int32_t* r = tab.data() + 8 * k;
        if (r[T_COUT] < 1 || r[T_TAPS] < 1 || r[T_CIN] < 1 || r[T_CINP] < r[T_CIN] || r[T_WCOFF] < 0) return FB_ERR_ARG;
        if (r[T_WOFF] < end) return FB_ERR_ARG;                                       // unsorted or overlapping
        total += (r[T_WOFF] - end + SP_PLAIN - 1) / SP_PLAIN;
        end = (long long)r[T_WOFF] + (long long)r[T_COUT] * r[T_TAPS] * r[T_CIN];
        if (end > n) return FB_ERR_ARG;
        total += (long long)r[T_TAPS] * ((r[T_COUT] + SP_TCO - 1) / SP_TCO) * ((r[T_CIN] + SP_TCI - 1) / SP_TCI);
    }
    total += (n - end + SP_PLAIN - 1) / SP_PLAIN;
    if (total >= (1LL << 31)) return FB_ERR_ARG;
    *tiles = total;
    return FB_OK;
}

}  // namespace

extern "C" int32_t fb_mt_sgd_prep_supported(int32_t dtype, int32_t f16x2_planes) {
    return (dtype == FB_F32 || dtype == FB_BF16) && !f16x2_planes ? 1 : 0;
}

extern "C" int fb_mt_sgd_prep(float* theta, const float* grad, float* mom, int64_t n, const float* gnorm2, float grad_clip, float lr,
                              float weight_decay, float momentum, float dampening, int32_t nesterov, int32_t first_step,
                              const int32_t* layer_tab, int32_t n_layers, void* w_fwd, void* w_dgrad, int32_t dtype, void* stream) {
    if (!theta || !grad || (!mom && momentum != 0.f)) FB_FAIL(FB_ERR_ARG, "fb_mt_sgd_prep: null pointer");
    if (grad_clip >= 0.f && !gnorm2) FB_FAIL(FB_ERR_ARG, "fb_mt_sgd_prep: clipping needs the device norm");
    if (n < 0 || n_layers < 0 || n_layers > SP_MAX_LAYERS) FB_FAIL(FB_ERR_ARG, "fb_mt_sgd_prep: n=%lld, n_layers=%d (at most %d)", (long long)n, n_layers, SP_MAX_LAYERS);
    if (n_layers > 0 && (!layer_tab || !w_fwd)) FB_FAIL(FB_ERR_ARG, "fb_mt_sgd_prep: null layer table or weight copy");
    if (!fb_mt_sgd_prep_supported(dtype, 0)) FB_FAIL(FB_ERR_ARG, "fb_mt_sgd_prep: dtype %d", dtype);
    if (((uintptr_t)theta | (uintptr_t)grad | (uintptr_t)mom | (uintptr_t)w_fwd | (uintptr_t)w_dgrad) & 15)
        FB_FAIL(FB_ERR_ARG, "fb_mt_sgd_prep: 16-byte alignment required");
    TabInfo info{FB_OK, (long long)((n + SP_PLAIN - 1) / SP_PLAIN), false};
    if (n_layers > 0) {
        std::lock_guard<std::mutex> lock(g_tabs_mutex);
        const auto key = std::make_pair((const void*)layer_tab, (int)n_layers);
        auto it = g_tabs.find(key);
        if (it == g_tabs.end() || it->second.rc != FB_OK) {
            std::vector<int32_t> host((size_t)8 * n_layers);
            if (hipMemcpy(host.data(), layer_tab, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
                FB_FAIL(FB_ERR_LAUNCH, "fb_mt_sgd_prep: reading the layer table failed");
            info.rc = check_table(host, n_layers, n, &info.tiles);
            for (int k = 0; k < n_layers; ++k) info.dgrad = info.dgrad || host[8 * k + T_DGRAD] != 0;
            if (info.rc == FB_OK) g_tabs[key] = info;
        } else {
            info = it->second;
        }
    }
    if (info.rc != FB_OK) FB_FAIL(FB_ERR_ARG, "fb_mt_sgd_prep: layer table must be sorted by w_off, non-overlapping, inside [0, n) and have Cin_real <= Cin_pad");
    if (info.dgrad && !w_dgrad) FB_FAIL(FB_ERR_ARG, "fb_mt_sgd_prep: the table has layers with a transposed copy, w_dgrad is null");
    if (info.tiles == 0) return FB_OK;
    const SpArgs a{theta, grad, mom, (long long)n, gnorm2, grad_clip, lr, weight_decay, momentum, dampening, nesterov, first_step,
                   layer_tab, n_layers, w_fwd, w_dgrad};
    if (dtype == FB_F32) hipLaunchKernelGGL((mt_sgd_prep_kernel<float>), dim3((unsigned)info.tiles), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((mt_sgd_prep_kernel<unsigned short>), dim3((unsigned)info.tiles), dim3(256), 0, (hipStream_t)stream, a);
    FB_CHECK_LAUNCH("fb_mt_sgd_prep");
    return FB_OK;
}

extern "C" int fb_mt_sgd_torch(float* theta, const float* grad, float* mom, int64_t n, const float* gnorm2, float grad_clip, float lr,
                               float weight_decay, float momentum, float dampening, int32_t nesterov, int32_t first_step, void* stream) {
    if (!theta || !grad || (!mom && momentum != 0.f)) FB_FAIL(FB_ERR_ARG, "fb_mt_sgd_torch: null pointer");
    if (grad_clip >= 0.f && !gnorm2) FB_FAIL(FB_ERR_ARG, "fb_mt_sgd_torch: clipping needs the device norm");
    const int64_t nb = (n + 255) / 256;
    hipLaunchKernelGGL(mt_sgd_torch_kernel, dim3((unsigned)(nb < 4096 ? (nb < 1 ? 1 : nb) : 4096)), dim3(256), 0, (hipStream_t)stream, theta, grad, mom,
                       (long long)n, gnorm2, grad_clip, lr, weight_decay, momentum, dampening, nesterov, first_step);
    FB_CHECK_LAUNCH("fb_mt_sgd_torch");
    return FB_OK;
}
