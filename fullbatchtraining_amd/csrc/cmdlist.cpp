// Native launch executor: command lists of library calls, recorded once and replayed with one host call.
//
// The reference drives its hot loop from Python, one ATen dispatch per operator (fullbatch/training/training.py:144-174: a Python loop
// over chunks around model forward / autograd.grad / foreach ops).  Here one chunk group's forward + backward is ~430 (ResNet-18) to
// ~6000 (ResNet-152) asynchronous launches; through ctypes every launch costs 6-20 us of interpreter time, which the GPU hides for
// ResNet-18 and does not for ResNet-152 (host-bound: 990 ms of enqueue for a 1070 ms step).  The sequence is static -- same entry
// points, same arguments, same buffers every step -- so the host side records it once (every fb_* call with its argument words and
// the index of the stream it went to, every cross-stream event record / wait) and replays it natively: one ctypes call per chunk
// group, ~1-3 us per launch.  Not a hipGraph: the kernels stay ordinary stream launches (events, profiling brackets and rocprofv3
// see them as before), the list just removes the interpreter from the loop.
#include <stdlib.h>

#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.h"

namespace {

template <typename T> inline T word_as(uint64_t w) {
    T v;
    memcpy(&v, &w, sizeof(T));
    return v;
}

using Thunk = int (*)(const uint64_t*, void*);

// Bind<decltype(&f), &f>::call(words, stream): f(words[0] as A0, ..., words[N-2] as A(N-2), stream)
template <typename F, F f> struct Bind;
template <typename... A, int (*f)(A...)> struct Bind<int (*)(A...), f> {
    static constexpr int N = sizeof...(A);
    template <size_t I, typename T> static T arg(const uint64_t* w, void* st) {
        if constexpr (I == N - 1) return (T)st;
        else return word_as<T>(w[I]);
    }
    template <size_t... I> static int run(const uint64_t* w, void* st, std::index_sequence<I...>) { return f(arg<I, A>(w, st)...); }
    static int call(const uint64_t* w, void* st) { return run(w, st, std::index_sequence_for<A...>{}); }
};

// ---- the ABI described by the compiler: one row per function of fb_engine.h, the source of every host binding (fb_entry_*) --------------
template <typename T> constexpr char sig_code() {
    if constexpr (std::is_void_v<T>) return 'v';
    else if constexpr (std::is_same_v<T, int32_t>) return 'i';
    else if constexpr (std::is_same_v<T, int64_t>) return 'l';
    else if constexpr (std::is_same_v<T, float>) return 'f';
    else if constexpr (std::is_same_v<T, double>) return 'd';
    else if constexpr (std::is_same_v<T, const fb_conv_args*>) return 'C';
    else if constexpr (std::is_same_v<T, const fb_wgrad_args*>) return 'W';
    else if constexpr (std::is_same_v<T, const char*>) return 's';
    else if constexpr (std::is_pointer_v<T>) return 'p';
    else static_assert(sizeof(T) == 0, "fb_engine.h uses a type that has no signature code");
}
// Sig<decltype(&f)>::str: "<return>:<arguments>", e.g. fb_conv2d "i:Cp"
template <typename F> struct Sig;
template <typename R, typename... A> struct Sig<R (*)(A...)> {
    static constexpr char str[] = {sig_code<R>(), ':', sig_code<A>()..., '\0'};
};
constexpr bool is_launch_sig(const char* s) {      // int f(..., void* stream)
    int n = 0;
    while (s[n]) ++n;
    return n >= 3 && s[0] == 'i' && s[n - 1] == 'p';
}

enum { HOST = 0, LAUNCH = 1, RECORDABLE = 2 };     // fb_entry_kind
struct Entry { const char* name; int32_t kind; const char* sig; Thunk fn; };
#define FB_ROW(f, kind, thunk) {#f, kind, Sig<decltype(&f)>::str, thunk}
#define FB_HOST(f) FB_ROW(f, HOST, nullptr)
#define FB_LAUNCH(f) FB_ROW(f, LAUNCH, nullptr)
// recordable: an asynchronous entry point whose arguments are scalars, device pointers or ONE leading argument struct (copied into the list)
#define FB_RECORDABLE(f) FB_ROW(f, RECORDABLE, (&Bind<decltype(&f), &f>::call))
constexpr Entry kEntries[] = {
    FB_HOST(fb_last_error_string), FB_HOST(fb_abi_version), FB_HOST(fb_entry_count), FB_HOST(fb_entry_name), FB_HOST(fb_entry_sig),
    FB_HOST(fb_entry_kind), FB_HOST(fb_struct_field), FB_HOST(fb_struct_size), FB_HOST(fb_abi_constant),
    FB_HOST(fb_profile_enable), FB_HOST(fb_profile_read), FB_HOST(fb_profile_read_launches),
    FB_HOST(fb_cmd_fn_id), FB_HOST(fb_cmd_fn_nargs), FB_HOST(fb_event_new), FB_HOST(fb_event_count), FB_HOST(fb_event_record),
    FB_HOST(fb_event_wait), FB_HOST(fb_cmdlist_create), FB_HOST(fb_cmdlist_destroy), FB_HOST(fb_cmdlist_size), FB_HOST(fb_cmdlist_add_call),
    FB_HOST(fb_cmdlist_add_event), FB_HOST(fb_cmdlist_replay),
    // convolution
    FB_RECORDABLE(fb_conv2d), FB_HOST(fb_conv_masked_addend_supported), FB_HOST(fb_conv_bwd_stat_supported), FB_RECORDABLE(fb_absmax),
    FB_HOST(fb_wgrad_bn_fused_supported), FB_RECORDABLE(fb_conv2d_wgrad),
    FB_HOST(fb_ws_conv_stat_floats), FB_HOST(fb_ws_wgrad_slab_floats), FB_HOST(fb_ws_bn_partial_floats), FB_HOST(fb_ws_mt_floats),
    FB_RECORDABLE(fb_wgrad_reduce), FB_RECORDABLE(fb_weight_prep),
    // batch norm
    FB_RECORDABLE(fb_bn_fwd_finalize), FB_RECORDABLE(fb_bn_apply), FB_HOST(fb_ws_bn_amax_floats), FB_HOST(fb_bn_apply_can_pool),
    FB_RECORDABLE(fb_bn_running_update), FB_HOST(fb_bn_bwd_reduce_rows), FB_RECORDABLE(fb_bn_bwd_reduce), FB_RECORDABLE(fb_bn_bwd_finalize),
    FB_RECORDABLE(fb_bn_bwd_apply), FB_RECORDABLE(fb_bn_bwd_reduce2), FB_RECORDABLE(fb_bn_bwd_apply2),
    // data path (fb_stem_patches takes a HOST array), pooling, head
    FB_LAUNCH(fb_stem_patches), FB_RECORDABLE(fb_avgpool2_fwd), FB_RECORDABLE(fb_subsample2_fwd), FB_RECORDABLE(fb_subsample2_bwd_add),
    FB_RECORDABLE(fb_maxpool3s2_fwd), FB_RECORDABLE(fb_maxpool3s2_bwd), FB_RECORDABLE(fb_maxpool3s2_fwd_idx), FB_RECORDABLE(fb_maxpool3s2_bwd_idx),
    FB_RECORDABLE(fb_head_pool), FB_RECORDABLE(fb_head_loss), FB_RECORDABLE(fb_bn_eval_coeffs), FB_LAUNCH(fb_head_tta), FB_RECORDABLE(fb_head_bwd),
    // multi-tensor
    FB_RECORDABLE(fb_mt_sqnorm), FB_RECORDABLE(fb_mt_accumulate), FB_RECORDABLE(fb_mt_fd_perturb), FB_RECORDABLE(fb_mt_fd_combine_accumulate), FB_RECORDABLE(fb_mt_fd_combine), FB_RECORDABLE(fb_mt_chunk_clip),
    FB_RECORDABLE(fb_mt_norms2), FB_RECORDABLE(fb_mt_clip_sgd), FB_RECORDABLE(fb_mt_scale), FB_LAUNCH(fb_mt_sam_ascent), FB_LAUNCH(fb_mt_sam_restore),
    FB_LAUNCH(fb_mt_absmax2), FB_LAUNCH(fb_mt_pnorm2), FB_LAUNCH(fb_mt_norm_bias), FB_LAUNCH(fb_mt_ema), FB_LAUNCH(fb_mt_clip_scale),
    FB_LAUNCH(fb_mt_grad_noise),
    // mini-batch SGD mode
    FB_RECORDABLE(fb_mt_sgd_prep), FB_HOST(fb_mt_sgd_prep_supported), FB_RECORDABLE(fb_mt_sgd_torch),
    // AdamW (hyp/optim=adam)
    FB_RECORDABLE(fb_mt_adamw),
    // GD-AGC (hyp/optim=gd_agc)
    FB_RECORDABLE(fb_mt_agc_sgd),
    // FISTA (hyp/optim=fista)
    FB_RECORDABLE(fb_mt_fista),
    // strong-Wolfe line search (hyp.optim.line_search=wolfe)
    FB_RECORDABLE(fb_mt_wolfe_direction), FB_RECORDABLE(fb_mt_wolfe_trial), FB_RECORDABLE(fb_mt_wolfe_phi_grad),
    // loss-landscape cruncher (cfg.viz)
    FB_RECORDABLE(fb_mt_landscape_point), FB_HOST(fb_mt_landscape_point_supported),
};
constexpr int kNumEntries = sizeof(kEntries) / sizeof(kEntries[0]);
constexpr bool launches_take_a_stream() {
    for (const Entry& e : kEntries)
        if (e.kind != HOST && !is_launch_sig(e.sig)) return false;
    return true;
}
static_assert(launches_take_a_stream(), "a launch row whose function is not int f(..., void* stream)");
inline bool recordable(int32_t fn) { return fn >= 0 && fn < kNumEntries && kEntries[fn].kind == RECORDABLE; }
inline int nargs_of(const Entry& e) { return (int)strlen(e.sig) - 2; }      // (including the stream)

// ---- the argument structs, field by field in header order ----------------------------------------------------------------------------
struct Field { const char* name; int32_t offset, size; char code; };
#define FB_FIELD(S, f) {#f, (int32_t)offsetof(S, f), (int32_t)sizeof(S::f), sig_code<decltype(S::f)>()}
#define F(f) FB_FIELD(fb_conv_args, f)
constexpr Field kConvFields[] = {F(src), F(wgt), F(dst), F(addend), F(stat_partial), F(n_img), F(Hs), F(Ws), F(Cs), F(Hd), F(Wd), F(Cd), F(R), F(S),
                                 F(stride), F(pad), F(mode), F(imgs_per_wset), F(wset_stride), F(addend_mode), F(dtype), F(addend_mask), F(bst_x),
                                 F(bst_mask), F(amax_src), F(amax_wgt), F(amax_imgs)};
#undef F
#define F(f) FB_FIELD(fb_wgrad_args, f)
constexpr Field kWgradFields[] = {F(x), F(dy), F(dw_partial), F(n_img), F(Hs), F(Ws), F(Cs), F(Hd), F(Wd), F(Cd), F(R), F(S), F(stride), F(pad),
                                  F(imgs_per_group), F(split_k), F(dtype), F(group_stride), F(amax_x), F(amax_dy), F(bn_x), F(bn_mask), F(bn_coef)};
#undef F
// a trailing field left out of a table: the last listed field then ends before the struct does
template <size_t N> constexpr bool reaches_end(const Field (&f)[N], size_t align, size_t size) {
    return (f[N - 1].offset + f[N - 1].size + align - 1) / align * align == size;
}
static_assert(reaches_end(kConvFields, alignof(fb_conv_args), sizeof(fb_conv_args)), "kConvFields does not reach the end of fb_conv_args");
static_assert(reaches_end(kWgradFields, alignof(fb_wgrad_args), sizeof(fb_wgrad_args)), "kWgradFields does not reach the end of fb_wgrad_args");
struct StructInfo { const Field* fields; int32_t n, size; };
constexpr StructInfo kStructs[] = {{kConvFields, sizeof(kConvFields) / sizeof(Field), sizeof(fb_conv_args)},
                                   {kWgradFields, sizeof(kWgradFields) / sizeof(Field), sizeof(fb_wgrad_args)}};

enum { CMD_CALL = 0, CMD_EVENT_RECORD = 1, CMD_EVENT_WAIT = 2 };
struct Cmd { int32_t kind, fn, stream, ev; uint32_t off, n; };
struct CmdList {
    std::vector<Cmd> cmds;
    std::vector<uint64_t> words;
    std::vector<std::unique_ptr<uint64_t[]>> blobs;   // copies of argument structs (fb_conv_args / fb_wgrad_args)
};

std::vector<hipEvent_t> g_events;   // process-wide event table: ids are shared by eager calls and by every list

}  // namespace

extern "C" int32_t fb_entry_count(void) { return kNumEntries; }
extern "C" const char* fb_entry_name(int32_t i) { return i >= 0 && i < kNumEntries ? kEntries[i].name : nullptr; }
extern "C" const char* fb_entry_sig(int32_t i) { return i >= 0 && i < kNumEntries ? kEntries[i].sig : nullptr; }
extern "C" int32_t fb_entry_kind(int32_t i) { return i >= 0 && i < kNumEntries ? kEntries[i].kind : -1; }
extern "C" int32_t fb_struct_field(int32_t which, int32_t i, const char** name, int32_t* offset, int32_t* size, char* code) {
    if (which < 0 || which > 1) FB_FAIL(FB_ERR_ARG, "fb_struct_field: unknown struct %d", which);
    const StructInfo& s = kStructs[which];
    if (i >= 0 && i < s.n) {
        *name = s.fields[i].name;
        *offset = s.fields[i].offset;
        *size = s.fields[i].size;
        *code = s.fields[i].code;
    }
    return s.n;
}
extern "C" int32_t fb_struct_size(int32_t which) { return which >= 0 && which <= 1 ? kStructs[which].size : -1; }
extern "C" int32_t fb_abi_constant(const char* name) {
    if (strcmp(name, "FB_MT_BLOCKS") == 0) return FB_MT_BLOCKS;
    if (strcmp(name, "FB_PROF_CLASSES") == 0) return FB_PROF_CLASSES;
    if (strcmp(name, "FB_PROF_INFO") == 0) return FB_PROF_INFO;
    if (strcmp(name, "FB_WOLFE_VEC") == 0) return FB_WOLFE_VEC;
    if (strcmp(name, "FB_WOLFE_BLOCK") == 0) return FB_WOLFE_BLOCK;
    if (strcmp(name, "FB_LANDSCAPE_VEC") == 0) return FB_LANDSCAPE_VEC;
    if (strcmp(name, "FB_LANDSCAPE_BLOCK") == 0) return FB_LANDSCAPE_BLOCK;
    if (strcmp(name, "FB_LANDSCAPE_BLOCKS") == 0) return FB_LANDSCAPE_BLOCKS;
    return -1;
}

// a recordable entry point's id is its row in the table
extern "C" int32_t fb_cmd_fn_id(const char* name) {
    for (int i = 0; i < kNumEntries; ++i)
        if (kEntries[i].kind == RECORDABLE && strcmp(kEntries[i].name, name) == 0) return i;
    return -1;
}
extern "C" int32_t fb_cmd_fn_nargs(int32_t fn) { return recordable(fn) ? nargs_of(kEntries[fn]) : -1; }

// ---- events (timing disabled): cross-stream ordering of eager launches and of recorded lists alike ------------------------------
extern "C" int32_t fb_event_new(void) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
        snprintf(fb_err_buf, sizeof(fb_err_buf), "fb_event_new: hipEventCreateWithFlags failed");
        return -1;
    }
    g_events.push_back(e);
    return (int32_t)g_events.size() - 1;
}
extern "C" int32_t fb_event_count(void) { return (int32_t)g_events.size(); }
extern "C" int fb_event_record(int32_t ev, void* stream) {
    if (ev < 0 || ev >= (int32_t)g_events.size()) FB_FAIL(FB_ERR_ARG, "fb_event_record: unknown event %d", ev);
    if (hipEventRecord(g_events[ev], (hipStream_t)stream) != hipSuccess) FB_FAIL(FB_ERR_LAUNCH, "fb_event_record: hipEventRecord failed");
    return FB_OK;
}
extern "C" int fb_event_wait(int32_t ev, void* stream) {
    if (ev < 0 || ev >= (int32_t)g_events.size()) FB_FAIL(FB_ERR_ARG, "fb_event_wait: unknown event %d", ev);
    if (hipStreamWaitEvent((hipStream_t)stream, g_events[ev], 0) != hipSuccess) FB_FAIL(FB_ERR_LAUNCH, "fb_event_wait: hipStreamWaitEvent failed");
    return FB_OK;
}

// ---- command lists ---------------------------------------------------------------------------------------------------------------
extern "C" void* fb_cmdlist_create(void) { return new CmdList(); }
extern "C" void fb_cmdlist_destroy(void* cl) { delete (CmdList*)cl; }
extern "C" int64_t fb_cmdlist_size(const void* cl) { return cl ? (int64_t)((const CmdList*)cl)->cmds.size() : 0; }

// words: one 64-bit word per argument of the entry point EXCEPT the trailing stream (pointers and integers zero/sign-extended, float
// and double as their bit patterns in the low bytes).  blob (optional): the argument struct words[0] points to; it is copied and
// words[0] redirected to the copy.
extern "C" int fb_cmdlist_add_call(void* handle, int32_t fn, const uint64_t* words, int32_t n_words, int32_t stream_idx, const void* blob,
                                   int32_t blob_bytes) {
    CmdList* cl = (CmdList*)handle;
    if (!cl || !recordable(fn)) FB_FAIL(FB_ERR_ARG, "fb_cmdlist_add_call: bad list or function id %d", fn);
    if (n_words != nargs_of(kEntries[fn]) - 1) FB_FAIL(FB_ERR_ARG, "fb_cmdlist_add_call: %s takes %d words, got %d", kEntries[fn].name, nargs_of(kEntries[fn]) - 1, n_words);
    Cmd c{CMD_CALL, fn, stream_idx, -1, (uint32_t)cl->words.size(), (uint32_t)n_words};
    cl->words.insert(cl->words.end(), words, words + n_words);
    if (blob && blob_bytes > 0) {
        const size_t nw = ((size_t)blob_bytes + 7) / 8;
        cl->blobs.emplace_back(new uint64_t[nw]);
        memcpy(cl->blobs.back().get(), blob, blob_bytes);
        cl->words[c.off] = (uint64_t)(uintptr_t)cl->blobs.back().get();
    }
    cl->cmds.push_back(c);
    return FB_OK;
}
extern "C" int fb_cmdlist_add_event(void* handle, int32_t kind, int32_t ev, int32_t stream_idx) {
    CmdList* cl = (CmdList*)handle;
    if (!cl || (kind != CMD_EVENT_RECORD && kind != CMD_EVENT_WAIT)) FB_FAIL(FB_ERR_ARG, "fb_cmdlist_add_event: bad list or kind %d", kind);
    if (ev < 0 || ev >= (int32_t)g_events.size()) FB_FAIL(FB_ERR_ARG, "fb_cmdlist_add_event: unknown event %d", ev);
    cl->cmds.push_back(Cmd{kind, -1, stream_idx, ev, 0, 0});
    return FB_OK;
}

// Issues every command in recorded order; streams[i] is the hipStream_t behind stream index i of the recording.
extern "C" int fb_cmdlist_replay(const void* handle, void* const* streams, int32_t n_streams) {
    const CmdList* cl = (const CmdList*)handle;
    if (!cl || !streams) FB_FAIL(FB_ERR_ARG, "fb_cmdlist_replay: null list or stream table");
    const size_t n = cl->cmds.size();
    for (size_t i = 0; i < n; ++i) {
        const Cmd& c = cl->cmds[i];
        if (c.stream < 0 || c.stream >= n_streams) FB_FAIL(FB_ERR_ARG, "fb_cmdlist_replay: command %zu wants stream %d of %d", i, c.stream, n_streams);
        void* st = streams[c.stream];
        if (c.kind == CMD_CALL) {
            const int rc = kEntries[c.fn].fn(cl->words.data() + c.off, st);
            if (rc != FB_OK) {
                char inner[400];
                snprintf(inner, sizeof(inner), "%s", fb_err_buf);
                FB_FAIL(rc, "fb_cmdlist_replay: command %zu (%s) failed: %s", i, kEntries[c.fn].name, inner);
            }
        } else if (c.kind == CMD_EVENT_RECORD) {
            if (hipEventRecord(g_events[c.ev], (hipStream_t)st) != hipSuccess) FB_FAIL(FB_ERR_LAUNCH, "fb_cmdlist_replay: hipEventRecord failed at command %zu", i);
        } else {
            if (hipStreamWaitEvent((hipStream_t)st, g_events[c.ev], 0) != hipSuccess) FB_FAIL(FB_ERR_LAUNCH, "fb_cmdlist_replay: hipStreamWaitEvent failed at command %zu", i);
        }
    }
    return FB_OK;
}
