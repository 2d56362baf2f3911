/* fb_engine.h -- C ABI of libfbengine.so, the MI355X (gfx950) device side of the full-batch GD hot path.
 *
 * The reference (JonasGeiping/fullbatchtraining) has no FFI: its device work is whatever PyTorch dispatches from
 *   fullbatch/training/training.py:76-83   (_compute_batched_gradient: model fwd, CE, autograd.grad)
 *   fullbatch/models/resnets.py:179-230,296-316 (conv / BN / ReLU / pool / fc graph)
 *   fullbatch/models/modules.py:211-300    (GradRegularizer finite differences: foreach mul/add/sub/div, norms)
 *   fullbatch/training/training.py:45-47   (_stable_mean_accumulation), :162 (per-chunk squared norm)
 *   fullbatch/training/training.py:198-211 (global-norm clip)  +  torch.optim.SGD.step (optimizers.py:28)
 * Each entry point below names the reference call it replaces.  A maintainer binds these with ctypes
 * (see INTEGRATION.md); no torch types cross this boundary.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch caching allocator); nothing here allocates
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), never synchronises
 *   - return 0 on success, a negative fb_status otherwise; fb_last_error_string() describes the last failure of the
 *     calling thread; no other global mutable state, re-entrant, one host thread per GPU
 *   - activations are NHWC ("pixel-major"): [image][y][x][channel], channel counts multiples of 32
 *   - `dtype`: FB_F32 (exact f32 MFMA 16x16x4) or FB_BF16 (bf16 MFMA 16x16x32, fp32 accumulate)
 *   - a launch processes `n_groups` chunks at once ("chunk group"); a chunk is the reference's unit of
 *     BN statistics / loss mean / gradient (training.py:150-168).  Per-chunk quantities are indexed [group][...]
 *   - conv weights live in K-contiguous "KRSC" form: [Cout][R*S][Cin]; per-chunk weight sets (finite-difference
 *     second pass, modules.py:226) are selected by image index / imgs_per_wset
 */
#ifndef FB_ENGINE_H
#define FB_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { FB_OK = 0, FB_ERR_ARG = -1, FB_ERR_SHAPE = -2, FB_ERR_LAUNCH = -3, FB_ERR_UNSUPPORTED = -4 } fb_status;
typedef enum { FB_F32 = 0, FB_BF16 = 1 } fb_dtype;

const char* fb_last_error_string(void);
int fb_abi_version(void);

/* ---------------------------------------------------------------- the ABI, described by the library itself -------- */
/* One table inside the library (csrc/cmdlist.cpp) lists every function declared in this header with its signature as the COMPILER sees
 * it, so a host binding sets its argument types from the table instead of copying them by hand (ABI v15).
 * fb_entry_sig(i): "<return>:<arguments>", one character each: v void, i 32-bit integer, l 64-bit integer, f float, d double, p any
 * pointer, s const char*, C const fb_conv_args*, W const fb_wgrad_args*.  fb_entry_kind(i): 0 a host function (query, profiling, event,
 * command list), 1 an asynchronous launch (returns a status, last argument the stream), 2 a launch that command lists can record
 * (fb_cmd_fn_id).  Name and signature are NULL, the kind -1, for i outside [0, fb_entry_count()). */
int32_t fb_entry_count(void);
const char* fb_entry_name(int32_t i);
const char* fb_entry_sig(int32_t i);
int32_t fb_entry_kind(int32_t i);
/* Layout of the argument structs, `which` 0: fb_conv_args, 1: fb_wgrad_args.  fb_struct_field returns the number of fields (FB_ERR_ARG
 * for another `which`) and, for 0 <= i < that number, field i in declaration order: its name, byte offset, byte size and type code (as above). */
int32_t fb_struct_field(int32_t which, int32_t i, const char** name, int32_t* offset, int32_t* size, char* code);
int32_t fb_struct_size(int32_t which);           /* sizeof, -1 for an unknown struct */
/* value of a constant of this header by name: "FB_MT_BLOCKS", "FB_PROF_CLASSES", "FB_PROF_INFO", "FB_WOLFE_VEC", "FB_WOLFE_BLOCK",
 * "FB_LANDSCAPE_VEC", "FB_LANDSCAPE_BLOCK", "FB_LANDSCAPE_BLOCKS"; -1 for any other name */
int32_t fb_abi_constant(const char* name);

/* Optional measurement aid (the only process-global state in the library, off by default): while enabled every
 * fb_conv2d / fb_conv2d_wgrad launch is bracketed by HIP events recorded on the launch stream.  fb_profile_read waits
 * for the recorded launches and returns, per kernel class {0: igemm fwd, 1: igemm dgrad, 2: wgrad, 3: BN apply, 4: BN backward reduce,
 * 5: BN backward apply}, the summed elapsed milliseconds, the number of launches and the number of launches that
 * were not recorded (pool exhausted): three arrays of FB_PROF_CLASSES elements. */
#define FB_PROF_CLASSES 6
#define FB_PROF_INFO 11   /* shape words filed with a launch (fb_profile_read_launches) */
int fb_profile_enable(int on, int capacity);
int fb_profile_read(double* ms, int64_t* launches, int64_t* dropped);
/* Per-launch records of everything recorded since the last fb_profile_read (which resets: call this one first).  Row i of `info`
 * ([cap][FB_PROF_INFO + 1] int32): {class, FB_PROF_INFO shape words}: convolutions {n_img, Hs, Ws, Cs, Hd, Wd, Cd, R, stride, flags, kernel id}, BatchNorm passes
 * {pixels/128, C, pixels_per_group/128, dtype, residual?, mask?, dy_out?, pooled?, 0, 0, 0}; ms[i] = elapsed milliseconds.
 * Returns the number of rows written (<= cap) or a negative fb_status. */
int64_t fb_profile_read_launches(int32_t* info, float* ms, int64_t cap);

/* ---------------------------------------------------------------- native launch executor -------------------------- */
/* The reference drives its hot loop from the Python interpreter, one dispatch per operator (training.py:144-174).  A chunk group's
 * forward + backward here is a STATIC sequence of 430 (ResNet-18) to 6000 (ResNet-152) launches, so a host binding records it once and
 * replays it with one call: fb_cmdlist_add_call files an entry point (fb_cmd_fn_id(name)) with one 64-bit word per argument except the
 * trailing stream (integers / pointers extended to 64 bits, float / double as bit patterns; `blob`: the argument struct word 0 points
 * to -- copied into the list) and the INDEX of the stream it goes to; fb_cmdlist_add_event files a record (kind 1) or wait (kind 2) of a
 * library event (fb_event_new; fb_event_record / fb_event_wait are the eager forms on the same events, so eager and replayed regions
 * order against each other).  fb_cmdlist_replay issues the list in order on streams[index].  Lists are host objects: created /
 * destroyed by the caller, never shared between threads. */
int32_t fb_cmd_fn_id(const char* name);          /* -1: this entry point cannot be recorded */
int32_t fb_cmd_fn_nargs(int32_t fn);             /* arguments including the stream */
int32_t fb_event_new(void);                      /* -1 on failure */
int32_t fb_event_count(void);                    /* events created so far (they live as long as the process: hosts REUSE the ids of lists they drop) */
int fb_event_record(int32_t ev, void* stream);
int fb_event_wait(int32_t ev, void* stream);
void* fb_cmdlist_create(void);
void fb_cmdlist_destroy(void* list);
int64_t fb_cmdlist_size(const void* list);
int fb_cmdlist_add_call(void* list, int32_t fn, const uint64_t* words, int32_t n_words, int32_t stream_idx, const void* blob, int32_t blob_bytes);
int fb_cmdlist_add_event(void* list, int32_t kind, int32_t ev, int32_t stream_idx);
int fb_cmdlist_replay(const void* list, void* const* streams, int32_t n_streams);

/* ---------------------------------------------------------------- convolution ------------------------------------ */
/* Implicit-GEMM convolution on MFMA.  mode 0: forward  y = conv(x, w)        (ATen convolution, resnets.py:69,206,209,150)
 *                                      mode 1: dgrad    dx = conv_input_grad   (ATen convolution_backward, input part)
 * src  [n_img][Hs][Ws][Cs]   dst [n_img][Hd][Wd][Cd]
 * wgt  [n_wsets][Cd][R*S][Cs] (for mode 1 the caller passes the transposed set produced by fb_weight_prep)
 * addend (optional, mode 1): dst += addend            (addend_mode 1: same shape)
 *                            dst += 0.25*addend[y/2][x/2] (addend_mode 2: gradient of AvgPool2d(2,2), resnets.py:149)
 * stat_partial (optional, mode 0): [2][ceil(M/128)][Cd] per-128-pixel-block channel sums / sums of squares of the fp32
 *   accumulators, consumed by fb_bn_fwd_finalize (training-mode BatchNorm statistics, resnets.py:71).
 * bst_x + bst_mask + stat_partial (optional, mode 1): the reduction pass of the BatchNorm backward that CONSUMES dst (autograd's
 *   native_batch_norm_backward sums behind resnets.py:71,118-121), fused into the epilogue: with g = dst * relu_mask (bst_mask: the bitmask
 *   fb_bn_apply wrote for that BatchNorm's output, 1 byte per 8 channels) and x = bst_x (that BatchNorm's input, shape of dst),
 *   stat_partial receives [2][M/128][Cd] per-128-pixel-block sums of g and of g*x (RAW x: fb_bn_bwd_finalize with raw_x = 1
 *   turns them into dbeta / dgamma).  Ask fb_conv_bwd_stat_supported first; otherwise call fb_bn_bwd_reduce. */
typedef struct {
    const void* src; const void* wgt; void* dst; const void* addend; float* stat_partial;
    int32_t n_img, Hs, Ws, Cs, Hd, Wd, Cd;
    int32_t R, S, stride, pad, mode;
    int32_t imgs_per_wset; int64_t wset_stride;   /* elements between weight sets; 0 = shared */
    int32_t addend_mode; int32_t dtype;
    const void* addend_mask;   /* optional (addend_mode 1): ReLU bitmask of the addend as written by fb_bn_apply (1 byte per 16-byte
                                * vector): dst += addend only where the bit is set, i.e. the masked residual gradient d * (out > 0) of
                                * reference resnets.py:118-121 / autograd's threshold_backward without a materialised copy */
    const void* bst_x; const void* bst_mask;   /* optional (mode 1): fused BatchNorm-backward reduction, see above */
    const float* amax_src; const float* amax_wgt;   /* optional (FB_F32): device arrays holding the largest magnitudes of src and of wgt
                                * (fb_absmax).  Both set: every fp32 operand enters as two scaled fp16 pieces and a product takes three fp16
                                * MFMAs (22 significand bits per operand, fp32 accumulation); src is split inside the kernel, wgt must be the
                                * fp16x2 planes fb_weight_prep(amax) wrote.  amax_src[k] belongs to images [k*amax_imgs, (k+1)*amax_imgs) (one
                                * scale per chunk, so that a chunk's result does not depend on how chunks are batched), amax_wgt[w] to weight
                                * set w.  Unset: three bf16 pieces, six MFMAs (exact fp32 operands), or the exact-f32 MFMA with FB_F32_EXACT=1 */
    int32_t amax_imgs;
} fb_conv_args;
int fb_conv2d(const fb_conv_args* a, void* stream);
/* 1 if fb_conv2d implements addend_mask for these arguments (otherwise it fails with FB_ERR_UNSUPPORTED and the caller masks the
 * addend itself: fb_bn_bwd_apply's dy_out) */
int32_t fb_conv_masked_addend_supported(const fb_conv_args* a);
/* 1 if fb_conv2d implements the fused BatchNorm-backward reduction (bst_x / bst_mask / stat_partial in mode 1) for these arguments */
int32_t fb_conv_bwd_stat_supported(const fb_conv_args* a);
/* Largest magnitudes of n_sets slices of n fp32 values, set_stride floats apart (one streaming pass, atomic maximum of the bit patterns):
 * per_set = 1: out[s] = max |x[s*set_stride + i]| (one scale per chunk: the amax_* arrays above); per_set = 0: out[0] = the maximum
 * over all slices */
int fb_absmax(const float* x, int64_t n, int32_t n_sets, int64_t set_stride, int32_t per_set, float* out, void* stream);

/* wgrad: dw[g][split][Cd][R*S][Cs] (fp32 partial slabs) = sum over the pixels of chunk g (split-K slice `split`) of
 * dy[p][Cd] (x) x[src(p,tap)][Cs]        (ATen convolution_backward, weight part).  Deterministic: no atomics.
 * group_stride (floats): 0 = dense slabs as above; otherwise the slab of (g, split) starts at
 * dw_partial + g*group_stride + split*Cd*R*S*Cs -- with split_k == 1 and unpadded channels that writes the per-chunk
 * gradient straight into the [g][P] gradient arena (group_stride = P) and no fb_wgrad_reduce pass is needed. */
typedef struct {
    const void* x; const void* dy; float* dw_partial;
    int32_t n_img, Hs, Ws, Cs, Hd, Wd, Cd;
    int32_t R, S, stride, pad;
    int32_t imgs_per_group; int32_t split_k; int32_t dtype;
    int64_t group_stride;
    const float* amax_x; const float* amax_dy;   /* optional (FB_F32): largest magnitudes of x and dy PER GROUP of imgs_per_group images
                                                  * (fb_absmax, per_set): fp16x2 split as in fb_conv_args */
    /* optional (1x1, Cs < 64: the stem on its patches; bf16 and fp32 without amax_*; fb_wgrad_bn_fused_supported): the BatchNorm backward apply step INSIDE the
     * operand loader -- `dy` then holds the gradient w.r.t. the BatchNorm + ReLU OUTPUT, and the kernel multiplies by
     *   dy'[p][c] = coef[g][c][0] * (dy[p][c] masked by bn_mask) + coef[g][c][1] * bn_x[p][c] + coef[g][c][2]      (rounded to the storage type)
     * i.e. exactly what fb_bn_bwd_apply would have written to dx with the coefficients of fb_bn_bwd_finalize: a layer whose input gradient
     * nobody needs (the stem) saves writing dx and reading it back.  bn_mask: ReLU bitmask (1 byte per 16-byte vector) or NULL. */
    const void* bn_x; const void* bn_mask; const float* bn_coef;
} fb_wgrad_args;
int32_t fb_wgrad_bn_fused_supported(const fb_wgrad_args* a);
int fb_conv2d_wgrad(const fb_wgrad_args* a, void* stream);

/* Workspace sizes (in floats) of the caller-owned scratch buffers the entry points below take; host-side arithmetic only,
 * no launch.  The library never allocates device memory.
 *   fb_ws_conv_stat_floats   : stat_partial of fb_conv2d(mode 0)  = 2 * ceil(n_img*Hd*Wd / 128) * Cd
 *   fb_ws_wgrad_slab_floats  : dw_partial of fb_conv2d_wgrad      = (n_img/imgs_per_group) * split_k * Cd * R*S * Cs
 *   fb_ws_bn_partial_floats  : partial of fb_bn_bwd_reduce        = 2 * ceil(n_pixels / 128) * C   (upper bound)
 *   fb_ws_mt_floats          : ws of the fb_mt_* reductions       = max(n_groups, 2) * FB_MT_BLOCKS */
int64_t fb_ws_conv_stat_floats(const fb_conv_args* a);
int64_t fb_ws_wgrad_slab_floats(const fb_wgrad_args* a);
int64_t fb_ws_bn_partial_floats(int64_t n_pixels, int32_t C);
int64_t fb_ws_mt_floats(int32_t n_groups);
/* sums the split_k slabs in fixed order, drops channel padding (Cs_pad -> Cs_real), writes [g][Cd][R*S][Cs_real]
 * at out + g*out_group_stride */
int fb_wgrad_reduce(const float* dw_partial, float* out, int64_t out_group_stride, int32_t n_groups, int32_t split_k,
                    int32_t Cd, int32_t taps, int32_t Cs_pad, int32_t Cs_real, void* stream);
/* master fp32 KRSC weights [Cout][taps][Cin_real] of n_wsets sets (wset_stride_in floats apart) ->
 * w_fwd [Cout][taps][Cin_pad] and (optional) w_dgrad [Cin_pad][taps][Cout] in `dtype`, sets wset_stride_out elements apart.
 * amax (optional, FB_F32): device array, amax[s] = largest magnitude of the master weights of set s (fb_absmax, per_set): the copies are
 * written as fp16x2 planes (per 32 values: 32 scaled fp16 high pieces, then 32 low pieces; same size as fp32) -- the weight format fb_conv2d
 * expects whenever fb_conv_args.amax_wgt is set (to this same scalar) */
int fb_weight_prep(const float* master, int64_t wset_stride_in, int64_t wset_stride_out, int32_t n_wsets, int32_t Cout, int32_t taps,
                   int32_t Cin_real, int32_t Cin_pad, void* w_fwd, void* w_dgrad, int32_t dtype, const float* amax, void* stream);

/* ---------------------------------------------------------------- batch norm ------------------------------------- */
/* Per (group, channel): mean, biased var from the partial sums; writes mean/var rows into the [n_groups][ch_total]
 * statistics tables at column ch_off, and scale = gamma*invstd, shift = beta - mean*scale  ([n_groups][C]). */
int fb_bn_fwd_finalize(const float* stat_partial, int32_t n_mblocks, int32_t n_groups, int32_t C, double count,
                       const float* gamma, const float* beta, int64_t param_group_stride, float eps,
                       float* mean_tab, float* var_tab, int32_t ch_total, int32_t ch_off,
                       float* scale, float* shift, float* invstd, void* stream);
/* y = relu?(x*scale[g][c] + shift[g][c] + residual)  residual: none | res | res*rscale[g][c]+rshift[g][c]
 * (BatchNorm2d + ReLU(inplace) + `out += identity`, resnets.py:217-228).
 * amax_out (optional, FB_F32): device array that receives max |y| of every statistics group (fb_absmax per_set semantics, tracked by the
 * same pass): the scale source of the fp16x2 convolutions that read y */
int fb_bn_apply(const void* x, void* y, const float* scale, const float* shift, const void* res, const float* rscale,
                const float* rshift, int64_t n_pixels, int32_t C, int64_t pixels_per_group, int64_t valid_pixels_per_group,
                int32_t relu, void* mask_out, void* pool_out, int32_t pool_W, int32_t dtype, float* amax_out, float* amax_ws, void* stream);
/* floats of scratch (amax_ws) that fb_bn_apply / fb_bn_bwd_apply need when amax_out is set: one per 512-vector run */
int64_t fb_ws_bn_amax_floats(int64_t n_pixels, int32_t C, int64_t pixels_per_group);
/* pool_out (optional): AvgPool2d(2,2) of y, [n_img][H/2][W/2][C] (the 'C' downsample shortcut of the NEXT block, resnets.py:149), written
 * by the same pass -- bit-identical to fb_avgpool2_fwd on y, one read of the activation less.  pool_W = image width of y; only where
 * fb_bn_apply_can_pool() says so (bf16, W*C == 2048 and C <= 256: the 64@32, 128@16, 256@8 maps of ResNet-18/34). */
int32_t fb_bn_apply_can_pool(int32_t C, int32_t W, int64_t pixels_per_group, int32_t dtype);
/* valid_pixels_per_group (0 = all): chunk sizes that do not fill whole 128-pixel statistics blocks (data.batch_size=125, reference
 * data_preparation.py:64-72) are stored padded with zero images; the pixels [valid, pixels_per_group) of every group are written as
 * exact zeros with a clear mask, so they stay out of every later sum (statistics are divided by the REAL count). */
/* mask_out (optional): ReLU mask, one byte per 16-byte vector of y (bit k = element k > 0).  The backward kernels accept it
 * in place of y (1/16 of the bytes).  When both `mask` and `y` are NULL no mask is applied (BN without ReLU). */
/* sequential running-stat EMA for every BN channel of the network in one launch (momentum 0.1, unbiased var,
 * torch BatchNorm2d).  mean_tab/var_tab: [n_passes][n_groups][ch_total] (passes pass_stride floats apart).
 * Update order: for g in groups: for p in passes  -- i.e. chunk g's base pass, then its finite-difference passes,
 * exactly the order in which the reference's sequential loop touches the buffers. */
int fb_bn_running_update(float* running_mean, float* running_var, const float* mean_tab, const float* var_tab, int32_t n_passes,
                         int64_t pass_stride, const float* unbias, int32_t n_groups, int32_t ch_total, float momentum, void* stream);
/* backward: partial sums of dy and dy*xhat with dy = dout * (y > 0) when y != NULL (threshold_backward).  One partial row per
 * workgroup of 128..1024 pixels: fb_bn_bwd_reduce_rows() is the row count to hand to fb_bn_bwd_finalize as n_mblocks. */
int32_t fb_bn_bwd_reduce_rows(int64_t n_pixels, int64_t pixels_per_group);
int fb_bn_bwd_reduce(const void* dout, const void* y, const void* mask, const void* x, const float* mean_tab, const float* invstd,
                     int32_t ch_total, int32_t ch_off, float* partial, int64_t n_pixels, int32_t C,
                     int64_t pixels_per_group, int32_t dtype, void* stream);
/* dgamma/dbeta -> gradient arena (per group), coefficients for fb_bn_bwd_apply.  raw_x = 0: partial holds sums of dy and of dy*xhat
 * (fb_bn_bwd_reduce); raw_x = 1: sums of dy and of dy*x (the fused reduction of fb_conv2d): sum dy*xhat = invstd*(sum dy*x - mean*sum dy),
 * evaluated in double */
int fb_bn_bwd_finalize(const float* partial, int32_t n_mblocks, int32_t n_groups, int32_t C, double count,
                       const float* scale, const float* mean_tab, const float* invstd, int32_t ch_total, int32_t ch_off,
                       float* dgamma, float* dbeta, int64_t grad_group_stride, float* coef, int32_t raw_x, void* stream);
/* dx = c_dy*dy + c_x*x + c_0 ; optionally also stores dy (masked gradient, used by the shortcut branch); amax_out (optional, FB_F32):
 * receives max |dx| as in fb_bn_apply */
int fb_bn_bwd_apply(const void* dout, const void* y, const void* mask, const void* x, const float* coef, void* dx, void* dy_out,
                    int64_t n_pixels, int32_t C, int64_t pixels_per_group, int32_t dtype, float* amax_out, float* amax_ws, void* stream);

/* Two BatchNorms that take the SAME incoming gradient through the SAME ReLU mask (a downsampling block, resnets.py:222-230: out = relu(bn2(conv2) +
 * bn_s(conv_s)): both BatchNorm backward passes start from the gradient of `out`): one read of dout serves both.  fb_bn_bwd_reduce2 writes each
 * BatchNorm's partial rows (sum dy is common) exactly as fb_bn_bwd_reduce would -- finalize each with fb_bn_bwd_finalize -- and fb_bn_bwd_apply2
 * writes both dx tensors.  Bit-identical to the separate calls; the channel vectors of a pixel must divide 256. */
int fb_bn_bwd_reduce2(const void* dout, const void* mask, const void* x_a, const float* invstd_a, int32_t ch_off_a, float* partial_a,
                      const void* x_b, const float* invstd_b, int32_t ch_off_b, float* partial_b, const float* mean_tab, int32_t ch_total,
                      int64_t n_pixels, int32_t C, int64_t pixels_per_group, int32_t dtype, void* stream);
int fb_bn_bwd_apply2(const void* dout, const void* mask, const void* x_a, const float* coef_a, void* dx_a, const void* x_b, const float* coef_b,
                     void* dx_b, int64_t n_pixels, int32_t C, int64_t pixels_per_group, int32_t dtype, void* stream);

/* ---------------------------------------------------------------- data path --------------------------------------- */
/* Stem patch gather: images [n_img][C][H][W] fp32 (device) -> patches [n_img][Ho][Wo][cin_pad] in `dtype`, element tap*C + c
 * (tap-major like the KRSC weights), zero beyond k*k*C and outside the image (the convolution's own zero padding); the stem
 * convolution (resnets.py:150 / :179) then runs as a 1x1 convolution over these rows.
 * Optional on-device augmentation (config/data/CIFAR10.yaml:11-13: RandomCrop(H, crop_pad) then RandomHorizontalFlip):
 * crop_oy/crop_ox [n_img] int8 in [0, 2*crop_pad] (device; both or neither), flip [n_img] int8 0/1 (device, optional);
 * pad_value: HOST array of C floats = value of a black pixel after normalisation (-mean/std), NULL = 0. */
int fb_stem_patches(const float* images, void* patches, int64_t n_img, int32_t C, int32_t H, int32_t W, int32_t k, int32_t stride,
                    int32_t pad, int32_t cin_pad, const int8_t* crop_oy, const int8_t* crop_ox, const int8_t* flip, int32_t crop_pad,
                    const float* pad_value, int32_t dtype, void* stream);

/* ---------------------------------------------------------------- pooling / head --------------------------------- */
int fb_avgpool2_fwd(const void* x, void* y, int32_t n_img, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
/* The spatial sampling of the strided 1x1 shortcut convolution (downsample 'B', resnets.py:142-146: conv1x1(stride 2) -> BN): the convolution
 * itself runs as a 1x1 stride-1 fb_conv2d on the compacted copy.  fwd: y[n][i][j][:] = x[n][2i][2j][:], y is [n_img][(H+1)/2][(W+1)/2][C]
 * (odd H, W allowed; a copy, bit-exact).  bwd_add, in place: dx[n][2i][2j][:] += dy[n][i][j][:], summed in fp32 and rounded once to `dtype`;
 * every other element of dx is neither read nor written; one owner thread per element (deterministic).  16-byte vectors along C: C must be
 * a multiple of 4 (FB_F32) / 8 (FB_BF16) and the pointers 16-byte aligned, FB_ERR_ARG otherwise.  64-bit indexing (ABI v14). */
int fb_subsample2_fwd(const void* x, void* y, int32_t n_img, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
int fb_subsample2_bwd_add(void* dx, const void* dy, int32_t n_img, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
/* MaxPool2d(3,2,1) of the 'standard' stem (resnets.py:78); bwd scatters through recomputed argmax */
int fb_maxpool3s2_fwd(const void* x, void* y, int32_t n_img, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
int fb_maxpool3s2_bwd(const void* x, const void* dy, void* dx, int32_t n_img, int32_t H, int32_t W, int32_t C, int32_t dtype,
                      void* stream);
/* the same pooling with the argmax remembered (what autograd's max_pool2d_with_indices keeps, resnets.py:78): idx [n][Ho][Wo][C] bytes, the window
 * position 0..8 (row-major, first maximum) every output element came from; the backward pass reads it instead of the pre-pool tensor.  Same bits
 * as fb_maxpool3s2_fwd / fb_maxpool3s2_bwd (ABI v13). */
int fb_maxpool3s2_fwd_idx(const void* x, void* y, void* idx, int32_t n_img, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream);
int fb_maxpool3s2_bwd_idx(const void* idx, const void* dy, void* dx, int32_t n_img, int32_t H, int32_t W, int32_t C, int32_t dtype,
                          void* stream);
/* AdaptiveAvgPool2d(1) + flatten (resnets.py:185-186): feat[n][C] fp32 */
int fb_head_pool(const void* a, float* feat, int32_t n_img, int32_t HW, int32_t C, int32_t dtype, void* stream);
/* fc + log_softmax + nll (mean over the chunk) + argmax-correct (training.py:78-80): logits, dlogits [n][classes],
 * loss[g], correct[g].  The loss functions of get_loss_fn (training.py:391-413): label_smoothing s -> LabelSmoothCrossEntropyLoss
 * (modules.py:86-101; s = 0 is CrossEntropyLoss), only_incorrect -> IncorrectCrossEntropyLoss (modules.py:104-119). */
/* Rows with a NEGATIVE label are padding: no loss, no gradient, not counted in the mean or in `correct`. */
int fb_head_loss(const float* feat, const float* fc_w, const float* fc_b, int64_t param_group_stride, const int64_t* labels,
                 float* logits, float* dlogits, float* loss, float* correct, int32_t n_groups, int32_t imgs_per_group,
                 int32_t C, int32_t classes, float label_smoothing, int32_t only_incorrect, void* stream);
/* evaluation helpers (training.py:343-388): BN in eval mode as scale = gamma*rsqrt(running_var+eps), shift = beta - running_mean*scale
 * (torch BatchNorm2d.eval()); and the test-time-flip epilogue (training.py:370-373): outputs = softmax(z_a) + softmax(z_b),
 * loss_sum[0] = sum_n CE(outputs_n, label_n) (cross entropy applied to the summed probabilities, like the reference), correct[0] =
 * #(argmax outputs == label). */
int fb_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, float* scale,
                      float* shift, int32_t C, void* stream);
int fb_head_tta(const float* logits_a, const float* logits_b, const int64_t* labels, int32_t n, int32_t classes, float* ws /* 2n floats */,
                float* loss_sum, float* correct, void* stream);
/* dW_fc[g], db_fc[g] into the gradient arena and d_a = (dlogits @ W)/HW broadcast over the HW pixels */
int fb_head_bwd(const float* feat, const float* dlogits, const float* fc_w, int64_t param_group_stride, float* dfc_w,
                float* dfc_b, int64_t grad_group_stride, void* d_a, int32_t n_groups, int32_t imgs_per_group, int32_t HW,
                int32_t C, int32_t classes, int32_t dtype, void* stream);

/* ---------------------------------------------------------------- multi-tensor (flat fp32 arena) ------------------ */
/* out[g] = sum_i (scale*x[g][i] + add_scale*add[i])^2 (add optional, shared by the groups), deterministic two-stage.
 * ws: n_groups*FB_MT_BLOCKS floats.  (g.pow(2).sum() stack-sum, training.py:162; norm of the finite-difference direction
 * block_strength*g + acc_strength*pre_grads, modules.py:217-223) */
#define FB_MT_BLOCKS 1024
int fb_mt_sqnorm(const float* x, int64_t group_stride, int32_t n_groups, int64_t n, float scale, const float* add, float add_scale,
                 float* out, float* ws, void* stream);
/* running mean over chunks (_stable_mean_accumulation, training.py:45-47): for j: avg += (g[j]-avg)/(counter0+j+1).
 * If sq_out != NULL also writes sq_out[j] = |g[j]|^2 (fused, one pass). */
int fb_mt_accumulate(float* avg, const float* g, int64_t group_stride, int32_t n_groups, int64_t n, int32_t counter0,
                     float* sq_out, float* ws, void* stream);
/* eps_n[g] = eps / sqrt(vnorm2[g]);  theta_out[g] = theta0 + (sign*eps_n[g]) * (s*g[g] + acc*pre)   (modules.py:217-226;
 * pre = the pre-computed full gradient of the acc_strength pre-pass, training.py:128-142, NULL without it) */
int fb_mt_fd_perturb(const float* theta0, const float* g, int64_t group_stride, int32_t n_groups, int64_t n, float s,
                     float eps, float sign, const float* vnorm2, float* eps_n, const float* pre, float acc, float* theta_out,
                     void* stream);
/* vhp = (ga - gb)/eps_n[g]; gt = g + cf*vhp; avg += (gt-avg)/(counter0+j+1)   (modules.py:232-240 + training.py:45-47) */
int fb_mt_fd_combine_accumulate(float* avg, const float* g, const float* ga, const float* gb, int64_t group_stride,
                                int32_t n_groups, int64_t n, const float* eps_n, float cf, int32_t counter0, void* stream);
/* The two halves of fb_mt_fd_combine_accumulate as separate steps, for hyp.batch_clip (training.py:166-167 clips the REGULARISED
 * chunk gradient before it is averaged):  fb_mt_fd_combine: g[j] += cf*(ga[j]-gb[j])/eps_n[j] in place;
 * fb_mt_chunk_clip (_clip_gradient_list, training/utils.py:4-19, p = 2): with norm = sqrt(sq[j]): if norm > clip then
 * g[j] *= clip/(norm + 1e-6) and clipped[j] = 1 else clipped[j] = 0. */
int fb_mt_fd_combine(float* g, const float* ga, const float* gb, int64_t group_stride, int32_t n_groups, int64_t n, const float* eps_n,
                     float cf, void* stream);
int fb_mt_chunk_clip(float* g, int64_t group_stride, int32_t n_groups, int64_t n, const float* sq, float clip, float* clipped, void* stream);
/* out[0] = |a|^2, out[1] = |b|^2 over [0,n) (grad norm for clipping, training.py:202-204; param_norm, :92) */
int fb_mt_norms2(const float* a, const float* b, int64_t n, float* out, float* ws, void* stream);
/* clip (training.py:206-207) + torch.optim.SGD step with weight decay, momentum, dampening, Nesterov.
 * gnorm2: device scalar |grad|^2 (whole vector); grad_clip < 0 disables clipping.  Operates on [0,n) of the
 * pointers given (callers pass shard offsets for the sharded multi-GPU update).  grad is overwritten with the
 * clipped gradient (the closure contract exposes p.grad). */
int fb_mt_clip_sgd(float* theta, float* grad, float* mom, int64_t n, const float* gnorm2, float grad_clip, float lr,
                   float weight_decay, float momentum, float dampening, int32_t nesterov, int32_t first_step, void* stream);
/* y = a*x (+ y*b)  flat helpers used by the sharded path (scale local mean by K_r/K) */
int fb_mt_scale(float* x, int64_t n, float a, void* stream);
/* SAM around the closure (additional_optimizers/sam.py:56-82).  ascent: with g_c = grad * clip coefficient (as
 * fb_mt_clip_sgd, training.py:198-206; grad_clip < 0: none) e_w = g_c * rho / (|g_c| + 1e-12), theta += e_w; restore: theta -= e_w. */
int fb_mt_sam_ascent(float* theta, const float* grad, float* e_w, int64_t n, const float* gnorm2, float grad_clip, float rho, void* stream);
int fb_mt_sam_restore(float* theta, const float* e_w, int64_t n, void* stream);
/* gradient-modification options that are off by default (training.py:187-211):
 *   fb_mt_absmax2  : out[0] = (max|a_i|)^2 -- the L-infinity clip norm (grad_clip_norm=inf, training.py:199-200) in the slot of |a|^2
 *   fb_mt_norm_bias: external norm bias on ONE parameter tensor (training.py:188-196); pnorm2 = device |theta|^2 of all parameters
 * and the model EMA used for evaluation (training/utils.py:22-29): ema = momentum*ema + one_minus*src. */
int fb_mt_absmax2(const float* a, int64_t n, float* out, float* ws, void* stream);
/* out[0] = ((sum |a_i|^p)^(1/p))^2 -- the clip norm for grad_clip_norm = p other than 2 / inf (training.py:201-204) */
int fb_mt_pnorm2(const float* a, int64_t n, float p, float* out, float* ws, void* stream);
int fb_mt_norm_bias(float* grad, const float* theta, int64_t n, const float* pnorm2, float strength, float bias, int32_t norm_type, void* stream);
int fb_mt_ema(float* ema, const float* src, int64_t n, float momentum, float one_minus, void* stream);
/* gradient noise of the closure (training.py:212-215; it acts on the clipped gradient, so the clip is applied in place first):
 *   fb_mt_clip_scale : grad *= grad_clip / (|grad| + 1e-6) if |grad| > grad_clip   (the in-place form of fb_mt_clip_sgd's clip)
 *   fb_mt_grad_noise : mode 0: grad += strength * noise ; mode 1: grad *= 1 + strength * noise   (noise drawn by the caller) */
int fb_mt_clip_scale(float* grad, int64_t n, const float* gnorm2, float grad_clip, void* stream);
int fb_mt_grad_noise(float* grad, const float* noise, int64_t n, float strength, int32_t mode, void* stream);
/* Mini-batch SGD mode (hyp.train_stochastic, reference training.py:241-286; ABI v16).  One pass over the arena [0, n) that turns
 * (theta, grad, mom) into (theta', mom') -- the clip of torch.nn.utils.clip_grad_norm_, coef = min(1, grad_clip / (sqrt(gnorm2[0]) + 1e-6))
 * (grad_clip < 0: none), then the arithmetic of fb_mt_clip_sgd; grad is read only -- AND writes the compute-dtype copies of theta' that
 * fb_weight_prep would: forward [co][tap][ci_pad] into w_fwd, transposed [ci][tap][co] into w_dgrad (element offsets wc_off; padding
 * columns Cin_real <= ci < Cin_pad are neither read nor written).  layer_tab: DEVICE array [n_layers][8] sorted by w_off,
 * {w_off, Cout, taps, Cin_real, Cin_pad, wc_off, has_dgrad, 0}; elements outside every layer get the update only.  dtype FB_F32 / FB_BF16
 * (fb_mt_sgd_prep_supported(dtype, f16x2_planes) == 0: compose fb_mt_sgd_torch + fb_weight_prep instead).  The host checks the table once
 * per (address, n_layers) -- one blocking read-back on first sight -- and refuses an unsorted or out-of-range one without a launch.
 *   fb_mt_sgd_torch: the update alone, same clip form and the same bits for theta' / mom'. */
int fb_mt_sgd_prep(float* theta, const float* grad, float* mom, int64_t n, const float* gnorm2, float grad_clip, float lr,
                   float weight_decay, float momentum, float dampening, int32_t nesterov, int32_t first_step, const int32_t* layer_tab,
                   int32_t n_layers, void* w_fwd, void* w_dgrad, int32_t dtype, void* stream);
int32_t fb_mt_sgd_prep_supported(int32_t dtype, int32_t f16x2_planes);
int fb_mt_sgd_torch(float* theta, const float* grad, float* mom, int64_t n, const float* gnorm2, float grad_clip, float lr,
                    float weight_decay, float momentum, float dampening, int32_t nesterov, int32_t first_step, void* stream);
/* AdamW (hyp/optim=adam: torch.optim.AdamW, single-tensor form, amsgrad=False; additive, ABI v17) on [0, n) of the pointers given, one launch:
 *   g = coef grad;  p *= 1 - lr wd;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g g;
 *   p -= step_size m / (sqrt(v) / bc2_sqrt + eps)
 * step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) are formed by the host in double from the update count t (this one included).
 * The clip reads the device scalar gnorm2[0] (grad_clip < 0: none): torch_clip = 0 is fb_mt_clip_sgd's form (norm > clip: coef = clip / (norm +
 * 1e-6)) and writes the clipped gradient back to grad; torch_clip = 1 is clip_grad_norm_'s, min(1, clip / (norm + 1e-6)), grad read only.
 * step_size = 0 leaves theta bit-identical while exp_avg / exp_avg_sq advance.  Any 4-byte aligned offset and any n; 16-byte accesses where the
 * four operands share their misalignment.  Refused without a launch: null pointers, a clip without gnorm2, a beta outside [0, 1), eps <= 0,
 * bc2_sqrt <= 0. */
int fb_mt_adamw(float* theta, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, const float* gnorm2, float grad_clip,
                int32_t torch_clip, float lr, float weight_decay, float beta1, float beta2, float eps, float step_size, float bc2_sqrt,
                void* stream);
/* GD-AGC (hyp/optim=gd_agc: the reference's SGD_AGC, Nesterov SGD with adaptive gradient clipping per output unit; additive, ABI v17), one
 * launch.  unit_tab: n_rows device rows of four int64 {offset, unit_len, n_units, clip_on}, one per tensor, sorted by offset: the tensor's units
 * are the n_units consecutive runs of unit_len floats from offset (a KRSC convolution weight: Cout units of taps * Cin; a 1-D tensor: 1 unit).
 *   g' = coef grad                                   the global clip of fb_mt_clip_sgd (torch_clip = 0: written back to grad) or of
 *                                                    clip_grad_norm_ (torch_clip = 1: grad read only), as in fb_mt_adamw
 *   per unit: pn = max(|p_u|, agc_eps), gn = |g'_u|, maxn = pn clipping;  d = gn > maxn ? g' (maxn / max(gn, 1e-6)) : g'
 *   then fb_mt_clip_sgd's update on d (weight decay, momentum buffer, dampening, Nesterov, first_step).
 * clipping < 0, or clip_on = 0 in a row: no unit clip, the bits of fb_mt_clip_sgd.  The unit-clipped gradient is never written.  Each unit's
 * two sums of squares are formed by one owner (a wave up to 1024 floats, a workgroup above) in an order that depends on unit_len alone: the
 * result does not depend on the grid or on how a table is split over launches.  Units of at most 5120 floats stay in registers between the
 * norms and the update (every element fetched once); longer ones are read a second time.  Elements of [0, n) in no unit are neither read nor
 * written.  Any 4-byte aligned pointers; rows need not be 16-byte aligned.  The table is checked once per (address, n_rows, n) (one blocking copy) and again by the kernel.  Refused without a launch:
 * null pointers (mom may be null with momentum 0), a clip without gnorm2, agc_eps <= 0 with clipping >= 0, more than 1024 rows, a table that is
 * not sorted, overlaps, leaves [0, n) or has a unit_len or n_units below 1. */
int fb_mt_agc_sgd(float* theta, float* grad, float* mom, int64_t n, const float* gnorm2, float grad_clip, int32_t torch_clip, float lr,
                  float weight_decay, float momentum, float dampening, int32_t nesterov, int32_t first_step, float clipping, float agc_eps,
                  const int64_t* unit_tab, int32_t n_rows, void* stream);
/* FISTA (hyp/optim=fista: the reference's FISTA, Nesterov-accelerated gradient descent with the explicit t_k sequence, projection None;
 * additive, ABI v17) on [0, n) of the pointers given, one launch.  Every operation rounded on its own, as the reference's tensor operations:
 *   g = coef grad;  xp = theta - g lr;  theta = xp one_plus_ak - x_minus ak;  x_minus = xp
 * ak = (tk - 1) / tk' with tk' = (p + sqrt(q + r tk^2)) / 2 and one_plus_ak = 1 + ak are formed by the host in float32 (the same for every
 * tensor); the first step has ak = 0 and leaves theta = xp for a finite x_minus.  The clip reads the device scalar gnorm2[0] (grad_clip < 0:
 * none): torch_clip = 0 is fb_mt_clip_sgd's form (norm > clip: coef = clip / (norm + 1e-6)) and writes the clipped gradient back to grad;
 * torch_clip = 1 is clip_grad_norm_'s, min(1, clip / (norm + 1e-6)), grad read only.  Any 4-byte aligned offset and any n; 16-byte accesses
 * where the three operands share their misalignment.  Refused without a launch: null pointers, n < 0, a clip without gnorm2, lr negative or
 * not finite, ak or one_plus_ak not finite. */
int fb_mt_fista(float* theta, float* grad, float* x_minus, int64_t n, const float* gnorm2, float grad_clip, int32_t torch_clip, float lr, float ak,
                float one_plus_ak, void* stream);
/* Strong-Wolfe line search (hyp.optim.line_search=wolfe: the reference's WolfeGradientDescent; additive, ABI v17): the arithmetic of one search
 * on [0, n) of the pointers given.  Every product-and-sum is one fused multiply-add (torch's add(other, alpha=) on a CPU with FMA units, and the
 * instructions of fb_mt_clip_sgd).  All pointers 16-byte aligned, any n.  The reductions write per-workgroup partials to ws (FB_MT_BLOCKS floats)
 * and finish them in double in a fixed order that depends on n alone: no atomics, the same bits on every launch.
 *   fb_mt_wolfe_direction: d = fma(wd, theta, grad);  mom = first ? d : fma(1 - dampening, d, momentum mom)  (momentum != 0: the bits
 *       fb_mt_clip_sgd writes without a clip; momentum == 0: mom is not touched and may be NULL);  p = -(nesterov ? fma(momentum, mom, d) : mom),
 *       -d for momentum == 0;  theta0 = theta;  out[0] = sum d p.
 *   fb_mt_wolfe_trial:     theta = fma(step, p, theta0)   (step = float(lr alpha), formed by the host in double).
 *   fb_mt_wolfe_phi_grad:  out[0] = sum fma(wd, theta, grad) p; writes nothing else but ws.
 * A launch covers FB_WOLFE_VEC floats per lane, FB_WOLFE_BLOCK lanes per workgroup, at most FB_MT_BLOCKS workgroups per pass of its stride loop.
 * Refused without a launch: null pointers, n < 0, a misaligned pointer, a scalar that is not finite. */
#define FB_WOLFE_VEC 4
#define FB_WOLFE_BLOCK 256
int fb_mt_wolfe_direction(const float* theta, const float* grad, float* mom, float* p, float* theta0, int64_t n, float weight_decay, float momentum,
                          float dampening, int32_t nesterov, int32_t first_step, float* out, float* ws, void* stream);
int fb_mt_wolfe_trial(float* theta, const float* theta0, const float* p, int64_t n, float step, void* stream);
int fb_mt_wolfe_phi_grad(const float* theta, const float* grad, const float* p, int64_t n, float weight_decay, float* out, float* ws, void* stream);
/* Loss-landscape cruncher (cfg.viz: the reference's crunch.py, _set_parameter_offset; additive, ABI v17): one grid point in one launch,
 *   theta = base + (dx x + dy y)       four operations, each rounded on its own as the reference's tensor operations: dx x, dy y, their sum, base + sum
 * on [0, n) of the pointers given, with (x, y) = xy[0], xy[1] read from DEVICE memory -- a recorded command list is replayed for every point after
 * a two-float device write -- AND the forward compute-dtype copy [co][tap][ci_pad] of theta for every convolution layer of layer_tab into w_fwd,
 * written from the same registers (the arena is KRSC: a cast and the padding stride, no transposition).  layer_tab: the DEVICE table of
 * fb_mt_sgd_prep, [n_layers][8] rows {w_off, Cout, taps, Cin_real, Cin_pad, wc_off, has_dgrad (ignored), 0} sorted by w_off; elements outside
 * every layer get the offset only; padding columns Cin_real <= ci < Cin_pad are neither read nor written.  layer_tab = NULL (or n_layers = 0):
 * the offset only -- what a host composes with fb_weight_prep where fb_mt_landscape_point_supported(dtype, f16x2_planes) is 0 (fp16x2 planes).
 * dtype FB_F32 / FB_BF16.  (0, 0) returns base bit for bit (for finite directions).  theta must not overlap the inputs.  Any 4-byte aligned arena
 * pointers and any n; 16-byte accesses where the four arena operands share their misalignment; w_fwd 16-byte aligned.  One owner per element, no
 * atomics: the result does not depend on the grid.  The host checks the table once per (address, n_layers, n) -- one blocking read-back on first
 * sight.  Refused without a launch: null pointers, n < 0, more than 512 layers, a table without w_fwd, a table that is not sorted, overlaps,
 * leaves [0, n) or has Cin_real > Cin_pad, an unknown dtype, a misaligned pointer.
 * A launch covers FB_LANDSCAPE_VEC floats per lane, FB_LANDSCAPE_BLOCK lanes per workgroup, at most FB_LANDSCAPE_BLOCKS workgroups per pass of its stride loop. */
#define FB_LANDSCAPE_VEC 8
#define FB_LANDSCAPE_BLOCK 256
#define FB_LANDSCAPE_BLOCKS 2048
int fb_mt_landscape_point(float* theta, const float* base, const float* dx, const float* dy, int64_t n, const float* xy,
                          const int32_t* layer_tab, int32_t n_layers, void* w_fwd, int32_t dtype, void* stream);
int32_t fb_mt_landscape_point_supported(int32_t dtype, int32_t f16x2_planes);

#ifdef __cplusplus
}
#endif
#endif /* FB_ENGINE_H */
