// Loss-landscape cruncher (cfg.viz, reference fullbatch/visualization/crunch.py:72-77, _set_parameter_offset): one grid point
//   theta = base + (dx x + dy y)
// on the flat arena AND the forward compute-dtype weight copies of the new point, in ONE pass -- instead of three torch operators and one
// fb_weight_prep launch per layer, 2 601 times for the 51 x 51 preset.  Per element, every operation rounded on its own as the reference's tensor
// operations round (recorded in tests/golden/landscape.npz, offset_form "mul_mul_add_add"; no fma anywhere), identically in body and edges:
//   px = dx[i] * x;  py = dy[i] * y;  d = px + py;  theta[i] = base[i] + d
// (x, y) = (0, 0) therefore returns base (d = +-0).  x and y are read from DEVICE memory: a recorded command list holds the pointer, the host
// writes two floats and replays the list for every point.
//
// The arena stores convolution weights KRSC, [Cout][taps][Cin_real], the order of the forward copy [co][tap][ci_pad]: the copy is a cast and the
// padding stride away, written from the registers that hold theta.  Every thread owns 8 consecutive arena elements (two 16-byte accesses per
// operand); it finds their layer by a binary search over the layer table parked in LDS, and where all 8 lie in one row of one layer and the
// destination is 16-byte aligned the copy leaves as ONE 16-byte (bf16) or two 16-byte (fp32) stores, otherwise element by element.  Elements
// outside every layer (BatchNorm affine parameters, the classifier, alignment gaps) get the offset only; padding columns Cin_real <= ci < Cin_pad
// are neither read nor written (the first fb_weight_prep of a run wrote their zeros).  One owner per element, no atomics: the result does not
// depend on the grid.  The layer table is fb_mt_sgd_prep's, has_dgrad ignored (a landscape has no backward pass).
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "common.h"

namespace {

constexpr int LP_MAX_LAYERS = 512, LP_VEC = FB_LANDSCAPE_VEC, LP_BLOCK = FB_LANDSCAPE_BLOCK, LP_MAX_BLOCKS = FB_LANDSCAPE_BLOCKS;
static_assert(LP_VEC == 8, "the body moves two float4 per operand and one 16-byte bf16 store");
enum { T_WOFF = 0, T_COUT = 1, T_TAPS = 2, T_CIN = 3, T_CINP = 4, T_WCOFF = 5 };

// a value that has been rounded (see csrc/fista.hip): no later addition may swallow the multiplication into an fma
__device__ __forceinline__ float rounded(float x) {
    asm("" : "+v"(x));
    return x;
}

__device__ __forceinline__ float offset_point(float w, float d0, float d1, float x, float y) {
#pragma clang fp contract(off)
    const float px = rounded(__fmul_rn(d0, x)), py = rounded(__fmul_rn(d1, y));
    return __fadd_rn(w, rounded(__fadd_rn(px, py)));
}

struct LpArgs {
    float* theta; const float* base; const float* dx; const float* dy; long long n, head, n8;
    const float* xy; const int* tab; int n_layers; void* w_fwd;
};

template <typename T> __device__ __forceinline__ void lp_store(T* p, float v) {
    if constexpr (sizeof(T) == 4) *p = v; else *p = f32_to_bf16(v);
}

// the copy of ONE element e (value v), searching on from layer k (the last layer that starts at or before some e' <= e, or -1)
template <typename T>
__device__ __forceinline__ void lp_copy_one(const LpArgs& a, const int* s_off, const int* s_end, int k, long long e, float v) {
    while (k + 1 < a.n_layers && s_off[k + 1] <= e) ++k;
    if (k < 0 || e >= s_end[k]) return;
    const int* r = a.tab + 8 * k;
    const unsigned local = (unsigned)(e - s_off[k]), cin = (unsigned)r[T_CIN];
    const unsigned row = local / cin, ci = local - row * cin;
    lp_store<T>((T*)a.w_fwd + (long long)r[T_WCOFF] + (long long)row * r[T_CINP] + ci, v);
}

template <typename T>
__global__ __launch_bounds__(LP_BLOCK) void mt_landscape_point_kernel(const LpArgs a) {
    __shared__ int s_off[LP_MAX_LAYERS], s_end[LP_MAX_LAYERS];
    const int L = a.n_layers;
    for (int k = threadIdx.x; k < L; k += LP_BLOCK) {
        const int* r = a.tab + 8 * k;
        s_off[k] = r[T_WOFF];
        s_end[k] = r[T_WOFF] + r[T_COUT] * r[T_TAPS] * r[T_CIN];
    }
    if (L > 0) __syncthreads();
    const float x = a.xy[0], y = a.xy[1];
    const long long gtid = (long long)blockIdx.x * LP_BLOCK + threadIdx.x, gsize = (long long)gridDim.x * LP_BLOCK;
    // ---- the body: elements [head, head + 8 n8), 16-byte aligned in all four arena operands
    for (long long i = gtid; i < a.n8; i += gsize) {
        const long long e0 = a.head + LP_VEC * i;
        float v[LP_VEC];
#pragma unroll
        for (int hlf = 0; hlf < 2; ++hlf) {
            const long long e = e0 + 4 * hlf;
            const float4 w = *(const float4*)(a.base + e), d0 = *(const float4*)(a.dx + e), d1 = *(const float4*)(a.dy + e);
            v[4 * hlf + 0] = offset_point(w.x, d0.x, d1.x, x, y); v[4 * hlf + 1] = offset_point(w.y, d0.y, d1.y, x, y);
            v[4 * hlf + 2] = offset_point(w.z, d0.z, d1.z, x, y); v[4 * hlf + 3] = offset_point(w.w, d0.w, d1.w, x, y);
            *(float4*)(a.theta + e) = make_float4(v[4 * hlf + 0], v[4 * hlf + 1], v[4 * hlf + 2], v[4 * hlf + 3]);
        }
        if (L == 0) continue;
        int lo = -1, hi = L - 1;                     // the last layer with s_off <= e0 (-1: e0 lies in front of the first layer)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_off[mid] <= e0) lo = mid; else hi = mid - 1;
        }
        const int k = lo;
        const bool in_k = k >= 0 && e0 < s_end[k];
        if (!in_k && (k + 1 >= L || e0 + LP_VEC <= s_off[k + 1])) continue;          // all 8 outside every layer: the offset only
        if (in_k && e0 + LP_VEC <= s_end[k]) {
            const int* r = a.tab + 8 * k;
            const unsigned local = (unsigned)(e0 - s_off[k]), cin = (unsigned)r[T_CIN];
            const unsigned row = local / cin, ci = local - row * cin;
            const long long dst = (long long)r[T_WCOFF] + (long long)row * r[T_CINP] + ci;
            if (ci + LP_VEC <= cin && (dst * sizeof(T)) % 16 == 0) {                  // one row, an aligned destination: 16-byte stores
                T* wf = (T*)a.w_fwd + dst;
                if constexpr (sizeof(T) == 4) {
                    *(float4*)wf = make_float4(v[0], v[1], v[2], v[3]);
                    *(float4*)(wf + 4) = make_float4(v[4], v[5], v[6], v[7]);
                } else {
                    uint4 o;
                    o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], v[3]); o.z = pack_bf16x2(v[4], v[5]); o.w = pack_bf16x2(v[6], v[7]);
                    *(uint4*)wf = o;
                }
                continue;
            }
        }
#pragma unroll
        for (int j = 0; j < LP_VEC; ++j) lp_copy_one<T>(a, s_off, s_end, k, e0 + j, v[j]);
    }
    // ---- the edges: [0, head) and [head + 8 n8, n), one element per thread
    const long long tail0 = a.head + LP_VEC * a.n8, edges = a.head + (a.n - tail0);
    for (long long q = gtid; q < edges; q += gsize) {
        const long long e = q < a.head ? q : tail0 + (q - a.head);
        const float v = offset_point(a.base[e], a.dx[e], a.dy[e], x, y);
        a.theta[e] = v;
        if (L > 0) lp_copy_one<T>(a, s_off, s_end, -1, e, v);
    }
}

// Host copies of the verdicts on the layer tables seen so far, by (address, rows, n) -- as fb_mt_sgd_prep keeps them: the table lives on the
// device, its checks are the host's.  The first call with a table reads it back (one blocking copy); later calls do not touch the stream.
std::map<std::tuple<const void*, int, long long>, int> g_tabs;
std::mutex g_tabs_mutex;

int check_table(const std::vector<int32_t>& tab, int n_layers, int64_t n) {
    long long end = 0;
    for (int k = 0; k < n_layers; ++k) {
        const int32_t* r = tab.data() + 8 * k;
        if (r[T_COUT] < 1 || r[T_TAPS] < 1 || r[T_CIN] < 1 || r[T_CINP] < r[T_CIN] || r[T_WCOFF] < 0) return FB_ERR_ARG;
        if (r[T_WOFF] < end) return FB_ERR_ARG;                                       // unsorted or overlapping
        end = (long long)r[T_WOFF] + (long long)r[T_COUT] * r[T_TAPS] * r[T_CIN];
        if (end > n || end >= (1LL << 31)) return FB_ERR_ARG;
    }
    return FB_OK;
}

}  // namespace

extern "C" int32_t fb_mt_landscape_point_supported(int32_t dtype, int32_t f16x2_planes) {
    return (dtype == FB_F32 || dtype == FB_BF16) && !f16x2_planes ? 1 : 0;
}

extern "C" int fb_mt_landscape_point(float* theta, const float* base, const float* dx, const float* dy, int64_t n, const float* xy,
                                     const int32_t* layer_tab, int32_t n_layers, void* w_fwd, int32_t dtype, void* stream) {
    if (!theta || !base || !dx || !dy || !xy) FB_FAIL(FB_ERR_ARG, "fb_mt_landscape_point: null pointer");
    if (n < 0 || n_layers < 0 || n_layers > LP_MAX_LAYERS)
        FB_FAIL(FB_ERR_ARG, "fb_mt_landscape_point: n=%lld, n_layers=%d (at most %d)", (long long)n, n_layers, LP_MAX_LAYERS);
    if (n_layers > 0 && (!layer_tab || !w_fwd)) FB_FAIL(FB_ERR_ARG, "fb_mt_landscape_point: null layer table or weight copy");
    if (!fb_mt_landscape_point_supported(dtype, 0)) FB_FAIL(FB_ERR_ARG, "fb_mt_landscape_point: dtype %d", dtype);
    if (((uintptr_t)theta | (uintptr_t)base | (uintptr_t)dx | (uintptr_t)dy | (uintptr_t)xy) & 3)
        FB_FAIL(FB_ERR_ARG, "fb_mt_landscape_point: 4-byte alignment required");
    if ((uintptr_t)w_fwd & 15) FB_FAIL(FB_ERR_ARG, "fb_mt_landscape_point: the weight copy must be 16-byte aligned");
    if (layer_tab == nullptr) n_layers = 0;                                           // the offset only
    if (n_layers > 0) {
        std::lock_guard<std::mutex> lock(g_tabs_mutex);
        const auto key = std::make_tuple((const void*)layer_tab, (int)n_layers, (long long)n);
        if (g_tabs.find(key) == g_tabs.end()) {
            std::vector<int32_t> host((size_t)8 * n_layers);
            if (hipMemcpy(host.data(), layer_tab, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
                FB_FAIL(FB_ERR_LAUNCH, "fb_mt_landscape_point: reading the layer table failed");
            if (check_table(host, n_layers, n) != FB_OK)
                FB_FAIL(FB_ERR_ARG, "fb_mt_landscape_point: layer table must be sorted by w_off, non-overlapping, inside [0, n) and have Cin_real <= Cin_pad");
            g_tabs[key] = FB_OK;
        }
    }
    if (n == 0) return FB_OK;
    // the vector body needs one misalignment shared by the four arena operands (whole arenas have it); otherwise all scalar
    const unsigned mis = (unsigned)((uintptr_t)theta & 15);
    const bool same = ((uintptr_t)base & 15) == mis && ((uintptr_t)dx & 15) == mis && ((uintptr_t)dy & 15) == mis;
    long long head = same ? ((16 - mis) & 15) / 4 : (long long)n;
    if (head > n) head = n;
    const long long n8 = (n - head) / LP_VEC;
    const long long work = n8 > 0 ? n8 : n, want = (work + LP_BLOCK - 1) / LP_BLOCK;
    const unsigned nb = (unsigned)(want < 1 ? 1 : (want > LP_MAX_BLOCKS ? LP_MAX_BLOCKS : want));
    const LpArgs a{theta, base, dx, dy, (long long)n, head, n8, xy, layer_tab, n_layers, w_fwd};
    if (dtype == FB_F32) hipLaunchKernelGGL((mt_landscape_point_kernel<float>), dim3(nb), dim3(LP_BLOCK), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((mt_landscape_point_kernel<unsigned short>), dim3(nb), dim3(LP_BLOCK), 0, (hipStream_t)stream, a);
    FB_CHECK_LAUNCH("fb_mt_landscape_point");
    return FB_OK;
}
