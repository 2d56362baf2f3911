// Spatial subsampling of the strided 1x1 shortcut (downsample 'B', reference resnets.py:142-146): a 1x1 convolution with stride 2 and no
// padding reads x[n][2i][2j][:] only, so it runs as the engine's 1x1 stride-1 convolution on a compacted copy of those pixels; its input
// gradient is scattered back onto them.  Both kernels move 16-byte vectors along C, one vector of the half-resolution map per thread and
// grid-stride step (every element of the quarter map is owned by exactly one thread: no atomics, no LDS, no barriers), and index with
// 64 bits throughout -- a chunk group's activation may exceed 2^31 elements.  HBM-bound: a quarter of the full-resolution map is touched.
#include "common.h"

namespace {

// vector index of x[n][2 * oy][2 * ox][cv] for the vector i = ((n * Ho + oy) * Wo + ox) * cvec + cv of the half-resolution map
__device__ __forceinline__ long long subsample_src(long long i, int H, int W, int Ho, int Wo, int cvec) {
    const int cv = (int)(i % cvec);
    long long r = i / cvec;
    const int ox = (int)(r % Wo);
    r /= Wo;
    const int oy = (int)(r % Ho);
    const long long n = r / Ho;
    return ((n * H + 2 * oy) * W + 2 * ox) * cvec + cv;
}

__global__ void subsample2_fwd_kernel(const uint4* __restrict__ x, uint4* __restrict__ y, long long total, int H, int W, int Ho, int Wo, int cvec) {
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) y[i] = x[subsample_src(i, H, W, Ho, Wo, cvec)];
}

template <typename T>
__global__ void subsample2_bwd_add_kernel(uint4* __restrict__ dx, const uint4* __restrict__ dy, long long total, int H, int W, int Ho, int Wo, int cvec) {
    constexpr int V = ET<T>::VEC;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const long long j = subsample_src(i, H, W, Ho, Wo, cvec);
        float a[V], b[V];
        ET<T>::unpack(dx[j], a);
        ET<T>::unpack(dy[i], b);
#pragma unroll
        for (int k = 0; k < V; ++k) a[k] += b[k];      // fp32 sum, rounded once (to nearest even) by pack
        dx[j] = ET<T>::pack(a);
    }
}

// shared argument check; returns the number of 16-byte vectors of the half-resolution map (> 0) or a negative fb_status
long long subsample_check(const char* name, const void* a, const void* b, int32_t n_img, int32_t H, int32_t W, int32_t C, int32_t dtype, int* cvec) {
    if (!a || !b) FB_FAIL(FB_ERR_ARG, "%s: null pointer", name);
    if (dtype != FB_F32 && dtype != FB_BF16) FB_FAIL(FB_ERR_ARG, "%s: dtype %d", name, dtype);
    if (n_img <= 0 || H <= 0 || W <= 0 || C <= 0) FB_FAIL(FB_ERR_ARG, "%s: empty tensor %d x %d x %d x %d", name, n_img, H, W, C);
    const int V = dtype == FB_F32 ? 4 : 8;
    if (C % V != 0) FB_FAIL(FB_ERR_ARG, "%s: %d channels do not form 16-byte vectors", name, C);
    if (((uintptr_t)a | (uintptr_t)b) & 15) FB_FAIL(FB_ERR_ARG, "%s: pointers must be 16-byte aligned", name);
    *cvec = C / V;
    return (long long)n_img * ((H + 1) / 2) * ((W + 1) / 2) * *cvec;
}

inline int subsample_blocks(long long total) { return (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048); }

}  // namespace

extern "C" int fb_subsample2_fwd(const void* x, void* y, int32_t n_img, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream) {
    int cvec = 0;
    const long long total = subsample_check("fb_subsample2_fwd", x, y, n_img, H, W, C, dtype, &cvec);
    if (total < 0) return (int)total;
    hipLaunchKernelGGL(subsample2_fwd_kernel, dim3(subsample_blocks(total)), dim3(256), 0, (hipStream_t)stream, (const uint4*)x, (uint4*)y, total, H, W,
                       (H + 1) / 2, (W + 1) / 2, cvec);
    FB_CHECK_LAUNCH("fb_subsample2_fwd");
    return FB_OK;
}

extern "C" int fb_subsample2_bwd_add(void* dx, const void* dy, int32_t n_img, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream) {
    int cvec = 0;
    const long long total = subsample_check("fb_subsample2_bwd_add", dx, dy, n_img, H, W, C, dtype, &cvec);
    if (total < 0) return (int)total;
    const dim3 grid(subsample_blocks(total));
    if (dtype == FB_F32)
        hipLaunchKernelGGL((subsample2_bwd_add_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, (uint4*)dx, (const uint4*)dy, total, H, W, (H + 1) / 2,
                           (W + 1) / 2, cvec);
    else
        hipLaunchKernelGGL((subsample2_bwd_add_kernel<bf16_tag>), grid, dim3(256), 0, (hipStream_t)stream, (uint4*)dx, (const uint4*)dy, total, H, W,
                           (H + 1) / 2, (W + 1) / 2, cvec);
    FB_CHECK_LAUNCH("fb_subsample2_bwd_add");
    return FB_OK;
}
