// GD-AGC (hyp/optim=gd_agc, reference optimizers.py:45-52 -> additional_optimizers/sgd_agc.py SGD_AGC): Nesterov SGD whose gradient is clipped
// per OUTPUT UNIT against that unit's parameter norm, as ONE pass over the arena with the global-norm clip of the consumer fused like in
// fb_mt_clip_sgd / fb_mt_adamw.  A unit (an output channel of a KRSC convolution weight, a row of fc.weight, a whole 1-D tensor) is one
// contiguous run of floats; the device unit table has one row per tensor, {offset, unit_len, n_units, clip_on} as int64, sorted by offset.
// Per unit u, every contraction written out (the vector and the scalar accesses round alike, whatever the compiler would fuse):
//   g'   = coef != 1 ? coef * g : g                                    the global clip; written back to grad in the full-batch form
//   pn   = max(sqrtf(sum p^2), eps);  gn = sqrtf(sum g'^2);  maxn = pn * clipping          IEEE square roots
//   d    = gn > maxn ? g' * (maxn / max(gn, 1e-6)) : g'                one IEEE division per unit; the strict trigger of the reference
//   d    = fma(wd, p, d); buf = first ? d : fma(1 - damp, d, mu m); d' = nesterov ? fma(mu, buf, d) : buf; p' = fma(-lr, d', p)
// (the last line is sgd_update of sgd_prep.hip = mt_clip_sgd_kernel: with clipping < 0, or in a tensor with clip_on = 0, the result has the bits
// of fb_mt_clip_sgd.)  g = p = m = 0 stays +0: pn = eps, gn = 0, no trigger.
//
// ONE OWNER PER UNIT, from its norms to its update: no atomics, no hand-off between workgroups.  The owner is a team of T threads, and T follows
// from the unit's length alone:
//   * len <= AGC_WAVE_L = 1024 floats: ONE WAVE (T = 64), no LDS, no barrier; a workgroup of four waves takes four consecutive units of a tensor.
//   * len >  AGC_WAVE_L: ONE WORKGROUP (T = 256).
// Thread t of the team takes the 16-byte chunks t, t + T, t + 2T, ... of the unit and adds their squares to ONE accumulator in increasing address
// order (fma(x, x, acc)); a wave's 64 accumulators are folded by a xor butterfly (32, 16, ..., 1: commutative at every level, every lane holds
// the same bits), a workgroup's four wave sums through LDS as ((s0 + s1) + s2) + s3.  That order is a function of the unit's length: not of the
// grid, of the unit's address, of the split of a table over launches, or of the path below.
//   * len <= AGC_L = 5120 floats (5 chunks per thread of a workgroup; every unit of the supported ResNets, whose largest is 4608): theta and grad
//     of the unit stay in REGISTERS between the norms and the update (with mom, fetched in the same phase: at most 3 x 20 VGPRs), so each
//     element of theta, grad and mom is fetched once.  A wave's unit is resident by construction (1 or 4 chunks per lane).
//   * len > AGC_L: the loop path of the workgroup: the same sums in the same order, and theta and grad are read a second time for the update
//     (40 KB+ per workgroup, read back at once: from L2 unless the unit is far larger than the cache).  Tensors without the clip take the update
//     loop alone.
// (A first version gave every unit to one wave, up to 18 chunks per lane in registers: 369 VGPRs, one wave per SIMD, 84 us on ResNet-18's arena
// from HBM where the unfused pair takes 76-81 us.  The workgroup team needs 166 VGPRs, three workgroups per CU overlap their phases; with one
// load phase per unit and a grid of exactly the resident workgroups: 65 us.  profiles/agc.md.)
// A unit whose rows are 16-byte aligned in theta, grad and mom moves as 16-byte accesses; any other (the stem's 27-float rows) as 4-byte ones in
// the same chunk assignment.  Elements outside every unit (the arena's alignment padding) are neither read nor written.
// The smallest units: a 27-float stem row keeps 7 of its wave's 64 lanes busy, a 64-float BatchNorm vector 16; a 1-D tensor, being ONE unit,
// leaves three of its workgroup's four waves idle.  ResNet-18 has 64 stem rows and 41 one-unit tensors (BatchNorm vectors, fc.bias) among
// 4 851 units: 11 338 floats, 0.1 % of the arena, in 57 of its 3 836 work items, which are short and run next to the long ones: packing several
// small units into one wave would buy nothing measurable and cost the one-owner-per-unit simplicity.
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "arena_update.h"

#pragma clang fp contract(off)     // (__fmul_rn / __fadd_rn are plain operators to hipcc: nothing below may be fused beyond the fmas written out)

namespace {

constexpr int AGC_WAVES = 4, AGC_THREADS = 64 * AGC_WAVES;
constexpr int AGC_WAVE_L = 1024;                         // units up to this length are owned by one wave, longer ones by the workgroup
constexpr int AGC_CH = 5;                                // 16-byte chunks per thread of the largest register-resident unit
constexpr long long AGC_L = 4LL * AGC_THREADS * AGC_CH;  // = 5120 floats: the limit of the fast path
constexpr int AGC_MAX_ROWS = 1024, AGC_GRID = 1024;
enum { U_OFF = 0, U_LEN = 1, U_UNITS = 2, U_CLIP = 3 };

struct AgcArgs {
    float* theta; float* grad; float* mom; long long n; const float* gnorm2;
    float grad_clip; int torch_clip; float lr, wd, mu, damp; int nesterov, first; float clipping, eps;
    const long long* tab; int rows;
};
struct AgcHyp { float coef, lr, wd, mu, one_minus_damp, clipping, eps; int nesterov, first; bool write_grad, use_mom, read_mom; };

__device__ __forceinline__ float4 agc_load4(const float* __restrict__ b, long long e, long long len, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e + 4 <= len) {
        if (vec) v = *(const float4*)(b + e);
        else { v.x = b[e]; v.y = b[e + 1]; v.z = b[e + 2]; v.w = b[e + 3]; }
    } else {
        if (e < len) v.x = b[e];
        if (e + 1 < len) v.y = b[e + 1];
        if (e + 2 < len) v.z = b[e + 2];
    }
    return v;
}
__device__ __forceinline__ void agc_store4(float* __restrict__ b, long long e, long long len, bool vec, const float4 v) {
    if (e + 4 <= len) {
        if (vec) *(float4*)(b + e) = v;
        else { b[e] = v.x; b[e + 1] = v.y; b[e + 2] = v.z; b[e + 3] = v.w; }
    } else {
        if (e < len) b[e] = v.x;
        if (e + 1 < len) b[e + 1] = v.y;
        if (e + 2 < len) b[e + 2] = v.z;
    }
}
__device__ __forceinline__ float4 agc_global_clip(const AgcHyp& h, const float4 g) {
    if (h.coef == 1.f) return g;
    return make_float4(__fmul_rn(h.coef, g.x), __fmul_rn(h.coef, g.y), __fmul_rn(h.coef, g.z), __fmul_rn(h.coef, g.w));
}
__device__ __forceinline__ float agc_sumsq(float acc, const float4 v) {      // (a chunk's missing elements are +0: fma(0, 0, acc) = acc)
    acc = __fmaf_rn(v.x, v.x, acc); acc = __fmaf_rn(v.y, v.y, acc); acc = __fmaf_rn(v.z, v.z, acc);
    return __fmaf_rn(v.w, v.w, acc);
}
__device__ __forceinline__ float agc_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = __fadd_rn(v, __shfl_xor(v, off));
    return v;
}
// the team's two sums, in every thread of the team.  T = 256: all four waves of the workgroup call it (two barriers: `sm` is free again after it)
template <int T> __device__ __forceinline__ void agc_team_sums(float& sp, float& sg, float* sm) {
    sp = agc_wave_sum(sp);
    sg = agc_wave_sum(sg);
    if constexpr (T == AGC_THREADS) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) { sm[wave] = sp; sm[AGC_WAVES + wave] = sg; }
        __syncthreads();
        sp = __fadd_rn(__fadd_rn(__fadd_rn(sm[0], sm[1]), sm[2]), sm[3]);
        sg = __fadd_rn(__fadd_rn(__fadd_rn(sm[4], sm[5]), sm[6]), sm[7]);
        __syncthreads();
    }
}
// the unit's factor from its two sums of squares: trig = gn > maxn, f = maxn / max(gn, 1e-6)
__device__ __forceinline__ void agc_factor(const AgcHyp& h, float sp, float sg, bool& trig, float& f) {
    const float pn = fmaxf(__fsqrt_rn(sp), h.eps), gn = __fsqrt_rn(sg);
    const float maxn = __fmul_rn(pn, h.clipping);
    trig = gn > maxn;
    f = trig ? __fdiv_rn(maxn, fmaxf(gn, 1e-6f)) : 1.f;
}
__device__ __forceinline__ void agc_update1(const AgcHyp& h, bool trig, float f, float p, float gc, float m, float& p_out, float& m_out) {
    float d = trig ? __fmul_rn(gc, f) : gc;
    d = __fmaf_rn(h.wd, p, d);
    m_out = m;
    if (h.use_mom) {
        const float buf = h.first ? d : __fmaf_rn(h.one_minus_damp, d, __fmul_rn(h.mu, m));
        m_out = buf;
        d = h.nesterov ? __fmaf_rn(h.mu, buf, d) : buf;
    }
    p_out = __fmaf_rn(-h.lr, d, p);
}
// update of one chunk from registers: p, gc (globally clipped), m (zeros where mom is not read); theta / mom / grad written
__device__ __forceinline__ void agc_update_chunk(const AgcHyp& h, bool trig, float f, const float4 p, const float4 gc, const float4 m,
                                                 float* __restrict__ tp, float* __restrict__ gp, float* __restrict__ mp, long long e, long long len,
                                                 bool vec) {
    float4 po, mo;
    agc_update1(h, trig, f, p.x, gc.x, m.x, po.x, mo.x); agc_update1(h, trig, f, p.y, gc.y, m.y, po.y, mo.y);
    agc_update1(h, trig, f, p.z, gc.z, m.z, po.z, mo.z); agc_update1(h, trig, f, p.w, gc.w, m.w, po.w, mo.w);
    agc_store4(tp, e, len, vec, po);
    if (h.use_mom) agc_store4(mp, e, len, vec, mo);
    if (h.write_grad) agc_store4(gp, e, len, vec, gc);
}

// ---- the fast path: a unit of at most 4 T CH floats owned by T threads (t = the thread's index in its team), theta and grad resident in registers
template <int CH, int T>
__device__ __forceinline__ void agc_unit_resident(const AgcHyp& h, float* __restrict__ tp, float* __restrict__ gp, float* __restrict__ mp, int len,
                                                  bool vec, int t, float* sm) {
    float4 p[CH], g[CH], m[CH];                  // (mom has nothing to do with the norms: it is fetched with the other two so that the unit has ONE load phase)
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int e = 4 * (c * T + t);
        p[c] = agc_load4(tp, e, len, vec);
        g[c] = agc_load4(gp, e, len, vec);
        m[c] = h.read_mom ? agc_load4(mp, e, len, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float sp = 0.f, sg = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        g[c] = agc_global_clip(h, g[c]);
        sp = agc_sumsq(sp, p[c]);
        sg = agc_sumsq(sg, g[c]);
    }
    agc_team_sums<T>(sp, sg, sm);
    bool trig; float f;
    agc_factor(h, sp, sg, trig, f);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int e = 4 * (c * T + t);
        if (e < len) agc_update_chunk(h, trig, f, p[c], g[c], m[c], tp, gp, mp, e, len, vec);
    }
}

// ---- the loop path: any length; with `clip` the sums first (same order as above), then theta and grad are read again for the update
template <int T>
__device__ __forceinline__ void agc_unit_loop(const AgcHyp& h, float* __restrict__ tp, float* __restrict__ gp, float* __restrict__ mp, long long len,
                                              bool vec, int t, bool clip, float* sm) {
    bool trig = false; float f = 1.f;
    if (clip) {
        float sp = 0.f, sg = 0.f;
        for (long long e = 4LL * t; e < len; e += 4 * T) {
            sp = agc_sumsq(sp, agc_load4(tp, e, len, vec));
            sg = agc_sumsq(sg, agc_global_clip(h, agc_load4(gp, e, len, vec)));
        }
        agc_team_sums<T>(sp, sg, sm);
        agc_factor(h, sp, sg, trig, f);
    }
    for (long long e = 4LL * t; e < len; e += 4 * T)
        agc_update_chunk(h, trig, f, agc_load4(tp, e, len, vec), agc_global_clip(h, agc_load4(gp, e, len, vec)),
                         h.read_mom ? agc_load4(mp, e, len, vec) : make_float4(0.f, 0.f, 0.f, 0.f), tp, gp, mp, e, len, vec);
}

// work items of a row, one workgroup each: a long unit, or four consecutive short ones
__device__ __host__ __forceinline__ long long agc_row_items(long long len, long long units) {
    return len > AGC_WAVE_L ? units : (units + AGC_WAVES - 1) / AGC_WAVES;
}

__global__ __launch_bounds__(AGC_THREADS) void mt_agc_sgd_kernel(const AgcArgs a) {
    // pre[r] = items of the rows in front of row r; a row that the host would have refused stops the whole launch before any write
    __shared__ long long pre[AGC_MAX_ROWS + 1];
    __shared__ float sm[2 * AGC_WAVES];
    __shared__ int bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, R = a.rows;
    if (tid == 0) { bad = 0; pre[0] = 0; }
    __syncthreads();
    if (wave == 0) {
        long long carry = 0;
        for (int base = 0; base < R; base += 64) {
            const int r = base + lane;
            long long v = 0;
            if (r < R) {
                const long long* row = a.tab + 4 * r;
                const long long off = row[U_OFF], len = row[U_LEN], units = row[U_UNITS];
                long long prev_end = 0;
                if (r > 0) prev_end = row[U_OFF - 4] + row[U_LEN - 4] * row[U_UNITS - 4];
                if (len < 1 || units < 1 || off < prev_end || off > a.n || units > (a.n - off) / len) bad = 1;
                else v = agc_row_items(len, units);
            }
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const long long up = __shfl_up(v, s);
                if (lane >= s) v += up;
            }
            if (r < R) pre[r + 1] = carry + v;
            carry += __shfl(v, 63);
        }
    }
    __syncthreads();
    if (bad) return;
    const long long total = pre[R];

    AgcHyp h;
    h.coef = fb_clip_coef(a.gnorm2, a.grad_clip, a.torch_clip);
    h.write_grad = !a.torch_clip && h.coef != 1.f;             // (the full-batch closure clips p.grad in place; the AGC-clipped gradient is never written)
    h.lr = a.lr; h.wd = a.wd; h.mu = a.mu; h.one_minus_damp = 1.f - a.damp; h.clipping = a.clipping; h.eps = a.eps;
    h.nesterov = a.nesterov; h.first = a.first; h.use_mom = a.mu != 0.f; h.read_mom = h.use_mom && !a.first;

    // one workgroup per item, the items in DESCENDING order (the arena ends in its longest units: they start first, the short ones fill the tail)
    for (long long w = blockIdx.x; w < total; w += gridDim.x) {
        const long long item = total - 1 - w;
        int lo = 0, hi = R - 1;                                // the row with pre[row] <= item < pre[row + 1]
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pre[mid] <= item) lo = mid; else hi = mid - 1;
        }
        const long long* row = a.tab + 4 * lo;
        const long long len = row[U_LEN], local = item - pre[lo];
        const bool clip = a.clipping >= 0.f && row[U_CLIP] != 0;
        const bool team = len > AGC_WAVE_L;                    // (uniform over the workgroup: every barrier below is reached by all four waves)
        const long long u = team ? local : local * AGC_WAVES + wave;
        if (u >= row[U_UNITS]) continue;                       // (a wave without a unit in the last item of a tensor of short units)
        const long long o = row[U_OFF] + u * len;
        float* tp = a.theta + o; float* gp = a.grad + o; float* mp = h.use_mom ? a.mom + o : nullptr;
        const bool vec = (((uintptr_t)tp | (uintptr_t)gp | (uintptr_t)mp) & 15) == 0;
        if (team) {
            if (!clip || len > AGC_L) agc_unit_loop<AGC_THREADS>(h, tp, gp, mp, len, vec, tid, clip, sm);
            else if (len <= 2 * 4 * AGC_THREADS) agc_unit_resident<2, AGC_THREADS>(h, tp, gp, mp, (int)len, vec, tid, sm);
            else agc_unit_resident<AGC_CH, AGC_THREADS>(h, tp, gp, mp, (int)len, vec, tid, sm);
        } else {
            if (!clip) agc_unit_loop<64>(h, tp, gp, mp, len, vec, lane, false, sm);
            else if (len <= 256) agc_unit_resident<1, 64>(h, tp, gp, mp, (int)len, vec, lane, sm);
            else agc_unit_resident<AGC_WAVE_L / 256, 64>(h, tp, gp, mp, (int)len, vec, lane, sm);
        }
    }
}

// Host copies of the checks of the unit tables seen so far, by (address, rows, n), like the layer tables of fb_mt_sgd_prep: the first call with a
// table reads it back (one blocking copy), later calls do not touch the stream.  The kernel repeats the checks on the DEVICE table, so a host
// copy that went stale (another table at a recycled address) costs a launch that does nothing at most, never a stray write.
struct AgcTabInfo { int rc; long long items; };
std::map<std::tuple<const void*, int, long long>, AgcTabInfo> g_agc_tabs;
std::mutex g_agc_tabs_mutex;

int agc_check_table(const std::vector<long long>& tab, int rows, long long n, long long* items) {
    long long end = 0, total = 0;
    for (int r = 0; r < rows; ++r) {
        const long long* row = tab.data() + 4 * r;
        if (row[U_LEN] < 1 || row[U_UNITS] < 1) return FB_ERR_ARG;
        if (row[U_OFF] < end || row[U_OFF] > n) return FB_ERR_ARG;                     // unsorted, overlapping or outside
        if (row[U_UNITS] > (n - row[U_OFF]) / row[U_LEN]) return FB_ERR_ARG;          // (no product that could overflow)
        end = row[U_OFF] + row[U_LEN] * row[U_UNITS];
        total += agc_row_items(row[U_LEN], row[U_UNITS]);
    }
    *items = total;
    return FB_OK;
}

}  // namespace

extern "C" int fb_mt_agc_sgd(float* theta, float* grad, float* mom, int64_t n, const float* gnorm2, float grad_clip, int32_t torch_clip, float lr,
                             float weight_decay, float momentum, float dampening, int32_t nesterov, int32_t first_step, float clipping,
                             float agc_eps, const int64_t* unit_tab, int32_t n_rows, void* stream) {
    if (!theta || !grad || (!mom && momentum != 0.f)) FB_FAIL(FB_ERR_ARG, "fb_mt_agc_sgd: null pointer");
    if (grad_clip >= 0.f && !gnorm2) FB_FAIL(FB_ERR_ARG, "fb_mt_agc_sgd: clipping needs the device norm");
    if (n < 0 || n_rows < 0 || n_rows > AGC_MAX_ROWS) FB_FAIL(FB_ERR_ARG, "fb_mt_agc_sgd: n=%lld, n_rows=%d (at most %d)", (long long)n, n_rows, AGC_MAX_ROWS);
    if (n_rows > 0 && !unit_tab) FB_FAIL(FB_ERR_ARG, "fb_mt_agc_sgd: null unit table");
    if (clipping >= 0.f && !(agc_eps > 0.f)) FB_FAIL(FB_ERR_ARG, "fb_mt_agc_sgd: agc_eps=%g must be positive", (double)agc_eps);
    if (((uintptr_t)theta | (uintptr_t)grad | (uintptr_t)mom) & 3) FB_FAIL(FB_ERR_ARG, "fb_mt_agc_sgd: 4-byte alignment required");
    if ((uintptr_t)unit_tab & 7) FB_FAIL(FB_ERR_ARG, "fb_mt_agc_sgd: the unit table must be 8-byte aligned");
    if (n_rows == 0) return FB_OK;
    AgcTabInfo info{FB_OK, 0};
    {
        std::lock_guard<std::mutex> lock(g_agc_tabs_mutex);
        const auto key = std::make_tuple((const void*)unit_tab, (int)n_rows, (long long)n);
        auto it = g_agc_tabs.find(key);
        if (it == g_agc_tabs.end()) {
            std::vector<long long> host((size_t)4 * n_rows);
            if (hipMemcpy(host.data(), unit_tab, host.size() * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess)
                FB_FAIL(FB_ERR_LAUNCH, "fb_mt_agc_sgd: reading the unit table failed");
            info.rc = agc_check_table(host, n_rows, n, &info.items);
            if (info.rc == FB_OK) g_agc_tabs[key] = info;
        } else {
            info = it->second;
        }
    }
    if (info.rc != FB_OK) FB_FAIL(FB_ERR_ARG, "fb_mt_agc_sgd: unit table must be sorted by offset, non-overlapping, inside [0, n) and have unit_len, n_units >= 1");
    // a grid of as many workgroups as the device holds at once walks the items: the table prologue is paid once per workgroup, not once per unit,
    // and no second round of workgroups runs on a partly empty device; the items are sorted by size (see the kernel), so the stride hands every
    // workgroup the same mix
    static const int resident = [] {
        int dev = 0, per_cu = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mt_agc_sgd_kernel, AGC_THREADS, 0) != hipSuccess || per_cu < 1)
            return AGC_GRID;
        return prop.multiProcessorCount * per_cu;
    }();
    const unsigned nb = (unsigned)(info.items > resident ? resident : info.items);
    const AgcArgs a{theta, grad, mom, (long long)n, gnorm2, grad_clip, (int)torch_clip, lr, weight_decay, momentum, dampening, (int)nesterov,
                    (int)first_step, clipping, agc_eps, (const long long*)unit_tab, (int)n_rows};
    hipLaunchKernelGGL(mt_agc_sgd_kernel, dim3(nb), dim3(AGC_THREADS), 0, (hipStream_t)stream, a);
    FB_CHECK_LAUNCH("fb_mt_agc_sgd");
    return FB_OK;
}
