// headdim64.h -- internal interface of headdim64.hip (head_dim 64) to the C ABI entry points of compress.hip and spmv.hip.
// Not part of the public ABI (include/mustafar_hip.h); every function validates its own arguments and returns a hipError_t value.
#ifndef MUSTAFAR_HEADDIM64_H
#define MUSTAFAR_HEADDIM64_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mustafar_hip.h"
#include "decode_call.h"

namespace mustafar_hd64 {

constexpr int kD = 64;

int prune(hipStream_t st, const void* x, void* out, int64_t n_rows, int kth);
// pass 1 of the two-pass conversion: bmp [B', t], accum [B', t + 1], head_off [B' + 1] (halfs); mirror as mustafar_compress_bitmap_mirrored
int bitmap(bool key, hipStream_t st, const void* x, int Bp, int t, int64_t* bmp, int32_t* accum, int64_t* head_off, int64_t* mirror);
// pass 2: the packed streams at nz_flat + head_off[h]
int pack(bool key, hipStream_t st, const void* x, int Bp, int t, const int64_t* bmp, const int32_t* accum, const int64_t* head_off,
         void* nz_flat);

// fused decode of one DecodeCall (decode_call.h; flags already checked by the caller): the plain launch over c.k / c.v, or, with
// c.k_ext set, the one over base views + device tables of 256-token extents.  ev: 4 events (decode launch start / stop, row-merge
// start / stop) or nullptr.  *ran_extents: the EXT instantiation was launched.
int decode(const DecodeCall& c, hipEvent_t* ev, bool* ran_extents);
int64_t workspace_bytes(int T, int Batch_Size, int groups);
// the 256-token trigger: n launches, raw window rows -> one extent per layer and side; the finish lists the views and slides the windows
int trigger_compress_batch(hipStream_t st, int n, const mustafar_trigger_item* items, int64_t head_stride, int Bp, int t, int kth_k, int kth_v,
                           int64_t k_region_halfs, int64_t v_region_halfs);
int trigger_finish_batch(hipStream_t st, int n, const mustafar_trigger_item* items, int64_t head_stride, int Bp, int len, int drop);
// a prefill in 256-token chunks: ONE launch, raw rows -> t / 256 extents per side in a staging of equally spaced extents; and the gather of
// such pieces (behind an optional first cache) into one reference-layout cache: ONE launch, lengths read on the device
int prefill_compress(hipStream_t st, const void* k_x, const void* v_x, int64_t head_stride, int Bp, int t, int kth_k, int kth_v,
                     const mustafar_cache_view* k_stage, const mustafar_cache_view* v_stage, int64_t k_chunk_bytes, int64_t v_chunk_bytes,
                     mustafar_cache_view* k_pieces, mustafar_cache_view* v_pieces, int64_t* k_head_total, int64_t* v_head_total,
                     int64_t k_region_halfs, int64_t v_region_halfs, int32_t* overflow_flag);
int cache_gather(hipStream_t st, const mustafar_cache_view* dst, const mustafar_cache_view* first, int first_tokens,
                 const mustafar_cache_view* pieces, int n_pieces, int Bp);

}  // namespace mustafar_hd64

#endif
