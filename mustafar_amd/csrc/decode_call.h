// decode_call.h -- one fused decode call as the host layers below the C ABI pass it on.  Not part of the public ABI
// (include/mustafar_hip.h): every mustafar_decode_attention* entry point of spmv.hip fills a DecodeCall from its own arguments and
// hands it to one dispatcher there, which routes it by head_dim to decode_attention (spmv.hip) or mustafar_hd64::decode
// (headdim64.hip).  A new argument of the call is a new field here.
#ifndef MUSTAFAR_DECODE_CALL_H
#define MUSTAFAR_DECODE_CALL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mustafar_hip.h"

struct DecodeCall {
    hipStream_t stream = nullptr;
    int head_dim = 128;
    // the compressed cache: the two views (an entry point that takes eight raw arrays passes views without strides), and behind
    // them the DEVICE tables of 256-token extents.  extents_entry: the call came through an entry point that takes base views +
    // tables; the dispatcher checks T_base and clears k_ext / v_ext / T_base when T == T_base (the plain call over the base).
    mustafar_cache_view k{}, v{};
    bool extents_entry = false;
    const mustafar_cache_view* k_ext = nullptr;
    const mustafar_cache_view* v_ext = nullptr;
    int T_base = 0;
    const int32_t* T_device = nullptr;
    const void* q = nullptr;
    void* k_window = nullptr;
    void* v_window = nullptr;
    const void* k_new = nullptr;
    const void* v_new = nullptr;
    void* scores = nullptr;
    int ld_scores = 0;
    void* out = nullptr;
    void* workspace = nullptr;
    int Split_K = 0, T = 0, Batch_Size = 0, groups = 0;
    int window_len = 0, window_capacity = 0;
    float sqrt_d = 0.f;
    const int32_t* window_len_extra = nullptr;
    const void* attention_mask = nullptr;
    int64_t mask_row_stride = 0;
    int heads_per_mask_row = 0;
    uint32_t flags = 0;
    float* lse = nullptr;     // fp32 [Batch_Size] written by the row merge, or nullptr
    bool lse_entry = false;   // the call came through an entry point with an LSE argument, which also accepts a window-less call
};

// The argument checks that head_dim 64 and 128 share word for word; max_window: the file's kMaxWindow.  *no_window: a window-less
// call (the entry points with an LSE only): no window argument at all and at least one compressed token.  Its launch has no window
// workgroups and no window slabs; any other mixture of zero and non-zero window arguments is refused.
inline bool decode_call_ok(const DecodeCall& c, int max_window, bool* no_window)
{
    if (c.attention_mask && (c.heads_per_mask_row < 1 || c.Batch_Size % c.heads_per_mask_row || c.mask_row_stride < 0)) return false;
    *no_window = c.lse_entry && c.window_len == 0 && c.window_capacity == 0 && !c.k_window && !c.v_window && !c.k_new && !c.v_new &&
                 !c.window_len_extra && c.T > 0;
    if (c.T < 0 || (c.T & 63) || c.groups < 1 || c.Batch_Size < 1 || c.Batch_Size % c.groups || (c.window_len < 1 && !*no_window) ||
        c.window_len > c.window_capacity || c.window_capacity > max_window ||
        c.ld_scores < c.T + (c.window_len_extra ? c.window_capacity : c.window_len) || (c.ld_scores & 7) || c.Split_K < 1 ||
        !(c.sqrt_d > 0.f))
        return false;
    return c.q && ((c.k_window && c.v_window) || *no_window) && c.scores && c.out && c.workspace;
}

#endif
