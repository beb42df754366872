/*
 * mustafar_hip.h -- C ABI of libmustafar_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary of the Mustafar sparse-attention decode path.  Every entry point is
 * `extern "C"`, takes plain device pointers / sizes and a `hipStream_t` passed as `void*`,
 * launches asynchronously on that stream and returns a hipError_t value as `int`
 * (0 == hipSuccess; MUSTAFAR_EINVAL for arguments the kernels do not support).
 * No torch types cross this boundary.  Citations are relative to the reference tree.
 *
 * Compressed-cache format (kernel/compression.py:8-247, consumed by kernel/csrc/SpMM_Kernel.cuh):
 *   bmp        u64 [B', tiles]       bit (63-i) set <=> element i of the 64-element tile != 0
 *   idx        u32 [B', tiles+1]     exclusive prefix of ceil8(nnz)/2 per tile (half2 units)
 *   NZ         fp16 stream           per tile ceil8(nnz) halfs: non-zeros in element order, then 0 padding
 *   NZ_offset  u32 [B']              start of each head's stream in uint4 (16-byte) units
 *   K tile id = (token/64)*D + d            -> 64 consecutive tokens of channel d
 *   V tile id = (token/64)*D + (c/64)*64 + token%64 -> 64 consecutive channels of one token
 *   B' = batch * kv_heads, tiles = T*D/64, D = head_dim.
 *
 * Support by head_dim:
 *   D == 128   every entry point.
 *   D == 64    mustafar_prune_magnitude, the two-pass conversion (mustafar_compress_bitmap_{key,value}, _mirrored,
 *              mustafar_compress_pack_{key,value}) and the fused decode through mustafar_decode_attention_hd.  At D = 64 the
 *              K tile id is (token/64)*64 + d and the V tile id (token/64)*64 + token%64 (one tile per token): bmp [B', t],
 *              idx [B', t + 1].  Row pointers (x, out, windows, k_new) must be 16-byte aligned (rows are moved as 16-byte pieces).
 *              Growth by extents (ABI 108): mustafar_trigger_compress_batch_hd, mustafar_trigger_finish_batch_hd and
 *              mustafar_decode_attention_extents_hd.
 *              The prefill from raw rows and the gather of 256-token pieces (ABI 109): mustafar_prefill_compress_hd and
 *              mustafar_cache_gather_hd.
 *              Everything else returns MUSTAFAR_EINVAL for D = 64: the two reference SpMV entry points (D = 128 in the reference),
 *              the one-pass conversion, mustafar_cache_append_*, mustafar_trigger_compress_batch and the D = 128 cache-view /
 *              extent decode forms.
 */
#ifndef MUSTAFAR_HIP_H
#define MUSTAFAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MUSTAFAR_EINVAL 1 /* == hipErrorInvalidValue */

/* Version / build probe: returns MAJOR*100 + MINOR. */
int mustafar_abi_version(void);

/*
 * Key SpMV.  Replaces `Key_SplitK_API` (kernel/build/SpMM_API.cuh:46-64; kernel/csrc/SpMM_API.cu:86-139),
 * the function `mustafar_key_formulation` calls (kernel/kernel_wrapper/mustafar_wrapper.cu:113-130).
 *   C[b, n, m] = fp16( sum_k fp32(Khat_g[m, k]) * fp32(B[b, n, k]) ),  g = b / num_key_value_groups
 *   A           unused (NULL in the reference too)
 *   B           fp16 [Batch_Size, N_Global, K_Global]   (query rows; the reference pads to N_Global = 8)
 *   C           fp16 [Batch_Size, N_Global, M_Global]   every element is written (no pre-zeroing needed)
 *   M_Global    = compressed tokens T (multiple of 64), K_Global = head_dim (128)
 *   N_Global    1 or 8 (the reference supports only 8; 1 is the un-padded fast form)
 *   Reduction_Workspace, Split_K   accepted for signature parity; unused (Split_K must be 1)
 */
int Key_SplitK_API(void* stream, const void* A, const uint64_t* bmp, const void* NZ, const uint32_t* idx,
                   const uint32_t* NZ_offset, const void* B, void* C, int M_Global, int N_Global, int K_Global,
                   void* Reduction_Workspace, int Split_K, int Batch_Size, int num_key_value_groups);

/*
 * Value SpMV.  Replaces `Value_SplitK_API` (kernel/build/SpMM_API.cuh:92-110; SpMM_API.cu:193-254),
 * called by `mustafar_value_formulation` (mustafar_wrapper.cu:242-260).
 *   C[b, n, m] = fp16( sum_k fp32(Vhat_g[k, m]) * fp32(B[b, n, k]) )
 *   B           fp16 [Batch_Size, N_Global, K_Global]   (softmax probabilities, K_Global = T)
 *   C           fp16 [Batch_Size, N_Global, M_Global]   M_Global = head_dim (128)
 *   Split_K     number of token chunks processed by independent workgroups (>= 1).  The reference
 *               carries the parameter but pins it to 1 (mustafar_wrapper.cu:199); here it is live:
 *               use mustafar_value_pick_split_k().  With Split_K > 1, Reduction_Workspace must hold
 *               mustafar_value_workspace_bytes() bytes (fp32 partials + flags; the reference's
 *               SplitK_Reduction, Reduction_Kernel.cuh:26-48, used fp16 partials).
 */
int Value_SplitK_API(void* stream, const void* A, const uint64_t* bmp, const void* NZ, const uint32_t* idx,
                     const uint32_t* NZ_offset, const void* B, void* C, int M_Global, int N_Global, int K_Global,
                     void* Reduction_Workspace, int Split_K, int Batch_Size, int num_key_value_groups);

int     mustafar_value_pick_split_k(int M_Global, int N_Global, int K_Global, int Batch_Size, int num_key_value_groups);
int64_t mustafar_value_workspace_bytes(int M_Global, int N_Global, int K_Global, int Batch_Size,
                                       int num_key_value_groups, int Split_K);

/*
 * Magnitude prune.  Replaces `dh_prune_key` / `dh_prune_value` (models/llama_mustafar_kernel.py:77-153):
 * per row of D halfs, thr = kth smallest |x| (1-indexed), out = |x| >= thr ? x : x*0 (sign-preserving zero).
 * `kth` = max(1, int(target_sparsity * D)) is computed by the caller (model :97).  In-place allowed.
 */
int mustafar_prune_magnitude(void* stream, const void* x, void* out, int64_t n_rows, int D, int kth);

/*
 * Compression.  Replaces `convert_key_batched` / `convert_value_batched` (kernel/compression.py:249-432)
 * as two device passes (each ONE read of x) with one small device->host read between them (the reference needs >= 1 + 2B'):
 *   pass 1  mustafar_compress_bitmap_{key,value}: x fp16 [B', t, D] (already pruned) ->
 *           bmp i64 [B', t*D/64], accum i32 [B', t*D/64 + 1] (accum_counts, compression.py:294-298) and
 *           head_off i64 [B'+1] = exclusive prefix of 2*accum[h][-1] (start of each head in halfs; :302-304).
 *   pass 2  mustafar_compress_pack_{key,value}: writes every half of nz_flat[0 .. head_off[B'])
 *           (non-zeros and zero padding; no pre-zeroing needed); packs x by the bitmaps of pass 1.
 */
int mustafar_compress_bitmap_key(void* stream, const void* x, int Bp, int t, int D, int64_t* bmp, int32_t* accum,
                                 int64_t* head_off);
int mustafar_compress_bitmap_value(void* stream, const void* x, int Bp, int t, int D, int64_t* bmp, int32_t* accum,
                                   int64_t* head_off);
/* Pass 1 with a second copy of head_off for a host that WAITS for it (round 6; kernel/compression.py:308 `total_size = ....item()`: the reference
 * synchronises here too).  host_mirror: B' + 1 int64 of device-visible host memory (hipHostMalloc / a pinned torch tensor) the caller has filled
 * with a negative sentinel; the launch that computes head_off stores every entry there as well, each one aligned 8-byte system-scope store,
 * BEFORE the launch that completes the offsets inside the blocks -- the caller polls until no entry is negative (or the stream has drained)
 * and sizes the packed buffer ~15 us earlier than a device-to-host copy behind the stream would let it.  head_off (device) is written as by
 * the plain calls: pass 2 reads that one.  key != 0: K tile geometry.  host_mirror == NULL: exactly mustafar_compress_bitmap_{key,value}. */
int mustafar_compress_bitmap_mirrored(void* stream, const void* x, int Bp, int t, int D, int key, int64_t* bmp, int32_t* accum,
                                      int64_t* head_off, int64_t* host_mirror);
int mustafar_compress_pack_key(void* stream, const void* x, int Bp, int t, int D, const int64_t* bmp,
                               const int32_t* accum, const int64_t* head_off, void* nz_flat);
int mustafar_compress_pack_value(void* stream, const void* x, int Bp, int t, int D, const int64_t* bmp,
                                 const int32_t* accum, const int64_t* head_off, void* nz_flat);

/*
 * Fused decode attention of one layer (extension).  Replaces the PyTorch glue of the reference hook
 * between the two SpMVs (models/llama_mustafar_kernel.py:270-317): window append, q.K_window^T, concat, / sqrt(d),
 * fp32 softmax, p.V_window, sum.  TWO launches on `stream` by default (T > 0): the one-pass launch -- every 64-token block runs key phase ->
 * softmax step -> value phase, the dense window rides along as a few more workgroups, one slab (max, sum, unnormalised output) per
 * workgroup and head -- and the row kernel that merges the slabs; MUSTAFAR_FLAG_TWO_LAUNCH (and T == 0) select the round-1 structure
 * of four launches: key SpMV (+ window scores) -> softmax -> value SpMV (+ window p.V partials) -> sum of the partials.
 * All operands fp16 unless noted; B' = Batch_Size / num_key_value_groups.
 *   q            [Batch_Size, 128]
 *   k_window     [B', window_capacity, 128]  rows [0, window_len) valid after the call; k_new [B', 128] (or NULL if the
 *   v_window     same                        newest row is already stored) is appended at row window_len - 1
 *   scores       [Batch_Size, ld_scores] scratch (scores, then probabilities); ld_scores >= T + window_len, % 8 == 0
 *   out          [Batch_Size, 128]
 *   workspace    mustafar_decode_workspace_bytes() bytes (fp32 partial slabs); Split_K as for Value_SplitK_API
 *   T            compressed tokens (multiple of 64, 0 allowed: window only; rows longer than 32768 take a streaming
 *                softmax); sqrt_d = sqrt(head_dim)
 *   window_len_extra  NULL, or a device int added to window_len inside the kernels (clamped to the capacity):
 *                lets a captured hipGraph of a whole decode step be replayed while the windows keep growing;
 *                advance it once per step with mustafar_counter_add().  ld_scores must then cover the capacity.
 *   attention_mask    NULL, or the hook's additive fp16 mask (models/llama_mustafar_kernel.py:293-301; the non-flash model
 *                always passes one, :723-728): rows of >= T + window length halfs, `mask_row_stride` halfs apart, one row
 *                per `heads_per_mask_row` consecutive score rows (the reference mask is [bsz, 1, 1, kv_len]: stride kv_len,
 *                heads_per_mask_row = q heads).  Applied exactly as the hook does: fp16(score / sqrt(d)) + mask in fp16,
 *                max with finfo(fp16).min, then the fp32 softmax.  Rows need no alignment.
 *   flags        0, or this call's own choice of FMA engine and launch structure (MUSTAFAR_FLAG_*), which then overrides the
 *                process defaults (environment / mustafar_set_fma_engine / mustafar_set_onepass) for this call only: two hook
 *                instances in one process can run different engines.  Undefined bits are rejected.
 */
#define MUSTAFAR_FLAG_ENGINE_FMA_MIX 1u  /* v_fma_mix_f32 per tile and head (exact products, fp16 subnormals included) */
#define MUSTAFAR_FLAG_ENGINE_MFMA    2u  /* v_mfma_f32_4x4x4_16B_f16 as a 4-wide FMA unit (GQA-4) */
#define MUSTAFAR_FLAG_ENGINE_DOT2    3u  /* v_dot2_f32_f16 on pairs of tiles (GQA-4 one-pass form; the default) */
#define MUSTAFAR_FLAG_TWO_LAUNCH     (1u << 4)  /* key SpMV -> softmax rows -> value SpMV -> sum */
#define MUSTAFAR_FLAG_ONE_PASS       (2u << 4)  /* one launch + slab merge */
int mustafar_decode_attention(void* stream, const uint64_t* k_bmp, const void* k_nz, const uint32_t* k_idx,
                              const uint32_t* k_nz_offset, const uint64_t* v_bmp, const void* v_nz, const uint32_t* v_idx,
                              const uint32_t* v_nz_offset, const void* q, void* k_window, void* v_window, const void* k_new,
                              const void* v_new, int window_len, int window_capacity, void* scores, int ld_scores, void* out,
                              void* workspace, int Split_K, int T, int Batch_Size, int num_key_value_groups, float sqrt_d,
                              const int32_t* window_len_extra, const void* attention_mask, int64_t mask_row_stride,
                              int heads_per_mask_row, uint32_t flags);
int64_t mustafar_decode_workspace_bytes(int T, int Batch_Size, int num_key_value_groups, int Split_K);

/*
 * mustafar_decode_attention for a given head_dim (ABI 107).  Same arguments, same semantics, plus `head_dim`:
 *   128  forwards to mustafar_decode_attention (the same kernels, the same output bit for bit).
 *   64   the D = 64 kernels: q [Batch_Size, 64], windows [B', window_capacity, 64], k_new / v_new [B', 64], out [Batch_Size, 64].
 *        One launch + a row merge: a workgroup serves one kv head and a run of 64-token blocks for all G q heads of it (key phase,
 *        online softmax step, value phase per block), the dense window rides along as 64-row workgroups, each leaves a (max, sum,
 *        output) slab per head and the row kernel merges them.  Group counts 1..8.  Exact fp16 x fp16 products, fp32 sums (the
 *        v_fma_mix engine's arithmetic): every engine flag runs it; MUSTAFAR_FLAG_TWO_LAUNCH is rejected.  `scores` / `ld_scores`
 *        are validated as for D = 128 but not written.  mustafar_last_decode_choice() reports engine 0, structure 1, form 5.
 *        Profile records (mustafar_profile_begin): the one-pass launch as "key", the row merge as "finish".
 *   any other value: MUSTAFAR_EINVAL.
 * mustafar_decode_workspace_bytes_hd: the workspace of that call (0 for an unsupported head_dim).
 */
int mustafar_decode_attention_hd(void* stream, const uint64_t* k_bmp, const void* k_nz, const uint32_t* k_idx,
                                 const uint32_t* k_nz_offset, const uint64_t* v_bmp, const void* v_nz, const uint32_t* v_idx,
                                 const uint32_t* v_nz_offset, const void* q, void* k_window, void* v_window, const void* k_new,
                                 const void* v_new, int window_len, int window_capacity, void* scores, int ld_scores, void* out,
                                 void* workspace, int Split_K, int T, int Batch_Size, int num_key_value_groups, float sqrt_d,
                                 const int32_t* window_len_extra, const void* attention_mask, int64_t mask_row_stride,
                                 int heads_per_mask_row, uint32_t flags, int head_dim);
int64_t mustafar_decode_workspace_bytes_hd(int T, int Batch_Size, int num_key_value_groups, int Split_K, int head_dim);

/*
 * Compressed cache with spare capacity (extension; SURVEY 8f rank 2: the reference re-copies bitmaps, offsets and every
 * head's stream on each 256-token append, models/llama_mustafar_kernel.py:339-390).  Same four arrays as the reference
 * format, but a head's bitmap / offset rows may be longer than the tokens in use, and NZ_offset may leave room behind
 * every head's stream -- so an append writes only the new tokens:
 *   bmp  [B', bmp_head_stride]   tiles [0, 2T) of a row in use        (bmp_head_stride >= 2T;     0 = exactly 2T)
 *   idx  [B', idx_head_stride]   entries [0, 2T] of a row in use      (idx_head_stride >= 2T + 1; 0 = exactly 2T + 1)
 */
typedef struct mustafar_cache_view {
    uint64_t* bmp;
    void*     nz;
    uint32_t* idx;
    uint32_t* nz_offset;
    int64_t   bmp_head_stride;
    int64_t   idx_head_stride;
    int64_t   nz_head_stride;   /* != 0: nz_offset[h] == h * nz_head_stride (uint4 units, < 2^32): the SpMV kernels then compute
                                   the head's stream start instead of loading it (one memory latency less per wave) */
    uint32_t  flags;            /* 0: the tile format above.  MUSTAFAR_VIEW_KEY_ROWS (ABI 113): a KEY cache held as token rows;
                                   MUSTAFAR_VIEW_VALUE_LISTS: a VALUE cache held as sorted channel lists; MUSTAFAR_VIEW_VALUE_PAIR_LISTS:
                                   the same over pairs of blocks, see below */
} mustafar_cache_view;

/*
 * Token-row key blocks (ABI 113): the form the GQA-4 one-pass super-block launch reads a key BASE in.  Made from a
 * tile-format key cache by mustafar_key_rows_plan + mustafar_key_rows_fill and turned back, bit for bit, by mustafar_key_rows_to_tiles.
 * Per kv head and 64-token block:
 *   w            the largest number of channels a token of the block keeps, rounded up to even (2 .. 128; an all-zero block: 2)
 *   ceil(w / 4)  rows of 64 x 4 bytes: the channels of slots 4j .. 4j + 3 of token t in lane t, then
 *   w / 2        rows of 64 half2: the values of slots 2j, 2j + 1 of token t in lane t
 * A token's slots hold its non-zero channels in ascending order; the slots behind them hold value +0 / channel 0.  A row is 256 bytes.
 * A view with MUSTAFAR_VIEW_KEY_ROWS in `flags` names such a cache:
 *   nz               the rows; head h starts at h * nz_head_stride uint4 units (nz_head_stride != 0, a multiple of 16)
 *   idx              u32 [B', idx_head_stride] block table: entry b = (first row of block b, counted from the head's start) << 8 | w
 *   bmp, nz_offset   unused (may be NULL)
 * Only mustafar_decode_attention_view / _extents / _extents_lse_hd read such a view, and only as the key BASE of a launch for which
 * mustafar_decode_reads_key_rows() is 1; every other entry point, and every other use, returns MUSTAFAR_EINVAL.
 */
#define MUSTAFAR_VIEW_KEY_ROWS 1u
/* Pass 1: block widths and the block table.  src: a tile-format KEY view of `tokens` tokens (tokens % 64 == 0) and Bp heads.
 * table u32 [Bp][tokens / 64] and head_rows i64 [Bp] (each head's number of rows) are written; the caller reads head_rows to size `nz`. */
int mustafar_key_rows_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_rows);
/* Pass 2: every row of every block.  dst: a MUSTAFAR_VIEW_KEY_ROWS view whose idx is the table of pass 1 (idx_head_stride == tokens / 64). */
int mustafar_key_rows_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens);
/* Back to tiles: bitmaps, offsets (idx[h][0] = 0 included) and the stream of the first `tokens` tokens of every head of `dst`, a tile-format
 * view with equally spaced stream regions (nz_head_stride != 0) that hold the streams; head_total i64 [Bp]: each head's stream length in halfs.
 * Three launches; nothing is read on the host.  What tiles -> rows -> tiles leaves is what it started from, bit for bit. */
int mustafar_key_rows_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total);
/* Whether the launch that a fused call of this shape runs reads a key base of token rows: 1 for the GQA-4 one-pass super-block launch of four
 * blocks per workgroup on v_fma_mix or v_dot2 (num_key_value_groups % 4 == 0), 0 for its launches of two blocks per workgroup (under 768
 * workgroups: measured slower on rows), for the pair, small and two-launch forms and for the matrix pipe.  T: the
 * compressed tokens the launch is sized for; gy: B' * num_key_value_groups / 4, the head groups of its grid.  Answered from the shape
 * rule of the launch itself, with the largest window standing in for the call's own (as mustafar_decode_reads_extents does). */
int mustafar_decode_reads_key_rows(int num_key_value_groups, int T, int gy, int ld_scores, uint32_t flags);

/*
 * Sorted channel lists: the form the GQA-4 one-pass super-block launch reads a value BASE in.  The ABI version stays 115:
 * callers find these symbols by name.  Made from a tile-format value cache by mustafar_value_lists_plan + mustafar_value_lists_fill and
 * turned back, bit for bit, by mustafar_value_lists_to_tiles.  Per kv head, 64-token block and 64-channel half (channels 0..63, 64..127):
 *   cnt[c]    the number of the block's tokens whose bitmap has channel c set (0..64; a kept +-0 is an entry)
 *   perm[i]   the half's channels sorted by cnt descending, ties by channel ascending: lane i owns channel perm[i]; its list is that
 *             channel's (token in block u8, value fp16) entries, tokens ascending
 *   value row r   slots 2r, 2r + 1 of the first m_r = #{c : cnt[c] > 2r} lanes, one half2 each; the rows end at the first m_r == 0
 *   token row j   slots 4j .. 4j + 3 of the first m_{2j} lanes, four token bytes each
 *   word j        token row j, value row 2j, value row 2j + 1, back to back in dwords; lane i of a row at the row's start + 4 i bytes
 * Slots behind a lane's last entry, inside a row it takes part in, hold value +0 / token 0 (tokens ascend: recognisable on the way back).
 * A block is a 256-byte header, half 0's words, half 1's words, and zeros up to the next multiple of 16 bytes (blocks are 16-byte aligned
 * from the head's start).  Header: bytes 0..127 perm of half 0, of half 1 (channels counted inside the half); bytes 128..191 m_0..m_31 of
 * half 0, of half 1; bytes 192..195 u32, the dword offset of half 1 from the block's start; the rest zero.
 * A view with MUSTAFAR_VIEW_VALUE_LISTS in `flags` names such a cache:
 *   nz               the blocks; head h starts at h * nz_head_stride uint4 units (nz_head_stride != 0)
 *   idx              u32 [B', idx_head_stride] block table: entry b = the dword offset of block b from the head's start, entry
 *                    tokens / 64 the head's dwords (idx_head_stride >= tokens / 64 + 1)
 *   bmp, nz_offset   unused (may be NULL)
 * Only mustafar_decode_attention_view / _extents / _extents_lse_hd read such a view, and only as the value BASE of a launch for which
 * mustafar_decode_reads_value_lists() is 1; every other entry point, and every other use, returns MUSTAFAR_EINVAL.
 */
#define MUSTAFAR_VIEW_VALUE_LISTS 2u
/* Pass 1: block sizes and the block table.  src: a tile-format VALUE view of `tokens` tokens (tokens % 64 == 0) and Bp heads.
 * table u32 [Bp][tokens / 64 + 1] and head_dwords i64 [Bp] (each head's size in dwords) are written; the caller reads head_dwords to size `nz`. */
int mustafar_value_lists_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_dwords);
/* Pass 2: every block.  dst: a MUSTAFAR_VIEW_VALUE_LISTS view whose idx is the table of pass 1 (idx_head_stride == tokens / 64 + 1). */
int mustafar_value_lists_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens);
/* Back to tiles, as mustafar_key_rows_to_tiles: bitmaps, offsets, streams (padding included) and head_total i64 [Bp], bit for bit. */
int mustafar_value_lists_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total);
/* Whether the launch that a fused call of this shape runs reads a value base of lists: the rule of mustafar_decode_reads_key_rows. */
int mustafar_decode_reads_value_lists(int num_key_value_groups, int T, int gy, int ld_scores, uint32_t flags);

/*
 * Sorted channel lists over PAIRS of blocks: the value BASE with one list per channel over the 128 tokens of blocks 2p, 2p + 1 (DESIGN.md
 * 3.3).  The longest list of a half sets the issue time of the value phase, and the longest of 64 lists over 128 tokens is relatively
 * shorter than over 64.  The ABI version stays 115: callers find these symbols by name.  Per kv head, pair p and 64-channel half:
 *   cnt[c]    the number of the pair's tokens whose bitmap has channel c set (0..128; a kept +-0 is an entry)
 *   perm[i]   the half's channels sorted by cnt descending, ties by channel ascending: lane i owns channel perm[i]; its list is that
 *             channel's (token in pair u8: 0..63 block 2p, 64..127 block 2p + 1; value fp16) entries, tokens ascending
 *   rows and words as in MUSTAFAR_VIEW_VALUE_LISTS (m_r = #{c : cnt[c] > 2r}, r = 0..63; up to 32 words); slots behind a list's end inside
 *             a row hold token 0 / value +0
 * A pair is a 256-byte header, half 0's words, half 1's words, and zeros up to the next multiple of 16 bytes.  Header: bytes 0..127 perm
 * of half 0, of half 1; bytes 128..255 m_0..m_63 of half 0, of half 1.  A base of an odd number of blocks ends in a pair of tokens 0..63.
 * A view with MUSTAFAR_VIEW_VALUE_PAIR_LISTS in `flags` names such a cache (P = (tokens / 64 + 1) / 2 pairs):
 *   nz               the pairs; head h starts at h * nz_head_stride uint4 units (nz_head_stride != 0)
 *   idx              u32 [B', idx_head_stride] block table, dword offsets from the head's start: entry 2p = pair p's header, entry
 *                    2p + 1 = its half 1, entry 2P = the head's dwords (idx_head_stride >= 2P + 1)
 *   bmp, nz_offset   unused (may be NULL)
 * Read where MUSTAFAR_VIEW_VALUE_LISTS is, by the same rule (mustafar_decode_reads_value_pair_lists); MUSTAFAR_EINVAL everywhere else.
 */
#define MUSTAFAR_VIEW_VALUE_PAIR_LISTS 4u
/* Pass 1: table u32 [Bp][2P + 1] and head_dwords i64 [Bp].  Pass 2: dst's idx is the table of pass 1 (idx_head_stride == 2P + 1).  Back to
 * tiles bit for bit.  As the three passes of MUSTAFAR_VIEW_VALUE_LISTS. */
int mustafar_value_pair_lists_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_dwords);
int mustafar_value_pair_lists_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens);
int mustafar_value_pair_lists_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total);
int mustafar_decode_reads_value_pair_lists(int num_key_value_groups, int T, int gy, int ld_scores, uint32_t flags);

/*
 * NIBBLE ROWS of a key cache (head_dim 128; arithmetic: mustafar_amd/csrc/key_nibble_rows.h): token rows whose channel
 * numbers are 4-bit steps.  Per kv head and 64-token block, lane = token; a slot is an fp16 value and a step.  A block of width w (even,
 * 2..128) is two shares back to back, one per wave of a pair: the front, slots [0, F), F = ((w / 2 + 1) & ~1), holds a token's first
 * non-zeros as a chain ascending from channel -1; the back, slots [F, w), the rest as a chain descending from channel 128.  A share of n
 * slots is ceil(n / 8) step rows (64 dwords: the steps of slots 8j .. 8j + 7, slot s in bits 4 (s & 7) ..) and n / 2 value rows (64 half2).
 * Step 0: no entry, stay (padding, value +0); 1..14: an entry that many channels on; 15: no entry, 14 channels on (a spacer, value +0).
 * Whether a slot is an entry is told by its step alone: a kept +-0 comes back.  The front takes a token's entries while they fit (greedy);
 * w is the smallest even width at which every token of the block fits.  The view is that of MUSTAFAR_VIEW_KEY_ROWS (table entry b = first
 * row of block b << 8 | w).  Read by the launches for which mustafar_decode_reads_key_nibble_rows() is 1 (the rule of the token rows),
 * and only next to a value base of MUSTAFAR_VIEW_VALUE_PAIR_LISTS; MUSTAFAR_EINVAL everywhere else.  The three passes are those of the
 * token rows; back to tiles bit for bit.
 */
#define MUSTAFAR_VIEW_KEY_NIBBLE_ROWS 8u
int mustafar_key_nibble_rows_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_rows);
int mustafar_key_nibble_rows_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens);
int mustafar_key_nibble_rows_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total);
int mustafar_decode_reads_key_nibble_rows(int num_key_value_groups, int T, int gy, int ld_scores, uint32_t flags);

/*
 * mustafar_decode_attention over a cache that GROWS BY EXTENTS (the 256-token trigger of models/llama_mustafar_kernel.py:324-398
 * without copying or moving what is already compressed): tokens [0, T_base) live in the two base views, tokens
 * [T_base + 256 i, T_base + 256 (i + 1)) in entry i of `k_extents` / `v_extents` -- arrays of mustafar_cache_view in DEVICE memory,
 * each describing a 256-token cache of its own (offsets relative to that extent; nz_head_stride != 0).  An entry is written once,
 * before the first call that names it, and never changed: a captured hipGraph of a call stays valid while the cache grows
 * behind it.  T_base and T - T_base are multiples of 256.  Read by the pair form of the one-pass launch (every group count: GQA-4 on the three engines,
 * GQA-2 and MHA on v_fma_mix; ld_scores % 32 == 0; mustafar_decode_reads_extents() tells); MUSTAFAR_EINVAL otherwise -- consolidate into one view then.
 *   T_device   NULL: T is the number of compressed tokens.  Otherwise a device int holding the compressed tokens IN USE
 *              (T_base <= *T_device <= T, a multiple of 256 beyond T_base), and T is the CAPACITY the launch is sized for: grid,
 *              slabs, score scratch (ld_scores >= T + window capacity), mask columns.  The caller adds 256 to *T_device when a
 *              trigger has listed an extent (and takes 256 off its window_len_extra counter, the windows having slid): ONE
 *              captured graph of the step then serves every cache length up to T (tests/test_gpu_extents.py).
 */
int mustafar_decode_attention_extents(void* stream, const mustafar_cache_view* k_base, const mustafar_cache_view* v_base, int T_base,
                                      const mustafar_cache_view* k_extents, const mustafar_cache_view* v_extents,
                                      const void* q, void* k_window, void* v_window, const void* k_new, const void* v_new,
                                      int window_len, int window_capacity, void* scores, int ld_scores, void* out, void* workspace,
                                      int Split_K, int T, int Batch_Size, int num_key_value_groups, float sqrt_d,
                                      const int32_t* window_len_extra, const void* attention_mask, int64_t mask_row_stride,
                                      int heads_per_mask_row, uint32_t flags, const int32_t* T_device);
int mustafar_decode_reads_extents(int num_key_value_groups, int ld_scores, uint32_t flags);

/* mustafar_decode_attention over two cache views (same semantics, same remaining arguments). */
int mustafar_decode_attention_view(void* stream, const mustafar_cache_view* k_cache, const mustafar_cache_view* v_cache,
                                   const void* q, void* k_window, void* v_window, const void* k_new, const void* v_new,
                                   int window_len, int window_capacity, void* scores, int ld_scores, void* out, void* workspace,
                                   int Split_K, int T, int Batch_Size, int num_key_value_groups, float sqrt_d,
                                   const int32_t* window_len_extra, const void* attention_mask, int64_t mask_row_stride,
                                   int heads_per_mask_row, uint32_t flags);

/*
 * In-place append of t new (already pruned) tokens per head behind the `old_tokens` a view holds: the cache-append
 * logic of the reference hook (models/llama_mustafar_kernel.py:339-390: shift the new offsets by the head's old total,
 * splice bitmaps / offsets, concatenate the streams) as two device passes that touch only the new tokens.
 *   pass 1  mustafar_cache_append_bitmap_{key,value}: bitmaps -> dst.bmp[h][2*old_tokens ...], offsets (continuing from
 *           dst.idx[h][2*old_tokens]; that entry must hold the head's current total, 0 for an empty cache) ->
 *           dst.idx[h][2*old_tokens + 1 ...]; head_total i64 [B'] = each head's NEW stream length in halfs.
 *           The caller checks head_total against the room behind nz_offset[h] before pass 2 (one small device->host read).
 *   pass 2  mustafar_cache_append_pack_{key,value}: the new tiles' non-zeros + padding -> dst.nz at 8*nz_offset[h] halfs.
 * x fp16 [B', t, D], t % 64 == 0, old_tokens % 64 == 0.
 */
/*
 * The two conversion calls of the reference (kernel/compression.py:249-432: bitmaps + offsets, then the packed streams) with ONE read of
 * the rows (round 5): the one-pass compression launch (kth = 0: already pruned) writes bitmaps, offsets and every head's stream -- into a
 * region of worst-case size each --, the caller reads head_off (the sizes of the tensors it returns: the one host read the reference's
 * return type asks for, compression.py:308, now BEHIND the work instead of between two passes over the rows) and
 * mustafar_convert_pack copies the regions head behind head into the exact-size buffer, the reference's layout.
 *   x          fp16 [B', t, 128] contiguous, t % 64 == 0           key        1: K tile geometry, 0: V
 *   bmp / accum   i64 [B', 2t] / i32 [B', 2t + 1] out (compression.py:339)
 *   head_off   i64 [B' + 1] out: exclusive prefix of the heads' stream lengths in halfs, [B'] = the total (compression.py:303-308)
 *   regions    B' * t * 128 halfs of scratch (head h's stream at h * t * 128);  packed  head_off[B'] halfs
 *   overflow_flag  device int, zeroed by the caller: bit 1 = a block gave up waiting for the lengths in front of it (see
 *              mustafar_cache_append_kv): the results are incomplete, repeat through mustafar_compress_bitmap_* / _pack_*
 *   scratch    mustafar_convert_scratch_bytes(B', t) bytes
 */
int64_t mustafar_convert_scratch_bytes(int Bp, int t);
int mustafar_convert_onepass(void* stream, const void* x, int Bp, int t, int D, int key, int64_t* bmp, int32_t* accum, int64_t* head_off,
                             void* regions, int32_t* overflow_flag, void* scratch);
/* The same with a host mirror as mustafar_compress_bitmap_mirrored takes one (round 6), B' + 2 int64 here: [0 .. B'] = head_off,
 * [B' + 1] = the value of *overflow_flag behind the compression launch (zero-extended).  Polled by the caller until no entry is negative. */
int mustafar_convert_onepass_mirrored(void* stream, const void* x, int Bp, int t, int D, int key, int64_t* bmp, int32_t* accum,
                                      int64_t* head_off, void* regions, int32_t* overflow_flag, void* scratch, int64_t* host_mirror);
int mustafar_convert_pack(void* stream, const void* regions, int Bp, int t, int D, const int64_t* head_off, void* packed);
int mustafar_cache_append_bitmap_key(void* stream, const void* x, int Bp, int t, int D, const mustafar_cache_view* dst,
                                     int old_tokens, int64_t* head_total);
int mustafar_cache_append_bitmap_value(void* stream, const void* x, int Bp, int t, int D, const mustafar_cache_view* dst,
                                       int old_tokens, int64_t* head_total);
int mustafar_cache_append_pack_key(void* stream, const void* x, int Bp, int t, int D, const mustafar_cache_view* dst,
                                   int old_tokens);
int mustafar_cache_append_pack_value(void* stream, const void* x, int Bp, int t, int D, const mustafar_cache_view* dst,
                                     int old_tokens);
int mustafar_counter_add(void* stream, int32_t* counter, int delta);

/*
 * The whole 256-token trigger of the hook (models/llama_mustafar_kernel.py:324-398) for K and V together, from the RAW
 * window rows: prune (:325-326, kth = max(1, int(sparsity * D)); 0 = rows already pruned), compress (:328-337) and append
 * (:339-390) in ONE launch behind a memset node: one wave per 64-token block keeps the rows in registers from the load to the
 * packed stream (threshold, bitmaps, counts, pack), and the blocks of a head find their stream positions from each other's
 * published lengths.  No pruned copy is written, nothing is allocated and nothing is read back on the host, so
 * the call can be captured in a hipGraph.  The same call compresses a prefill block (:416-437) into two empty views
 * (old_tokens = 0).  (MUSTAFAR_COMPRESS=twopass in the environment: the two-pass form, three launches.)
 *   k_x / v_x       fp16 rows of 128; head h starts `head_stride` elements after head h - 1 (a window buffer: capacity * 128)
 *   *_head_total    i64 [B'] out: every head's new stream length in halfs (read it whenever convenient, e.g. through an
 *                   asynchronous copy: the next append needs it only to decide about room)
 *   *_region_halfs  room of a head's stream region (0 = unchecked); overflow_flag (device int, REQUIRED; the caller zeroes it):
 *                   bit 0 = a head outgrew its region -- the blocks that would cross the end of the region then write no stream
 *                   bytes (the bitmaps / offsets of the new tokens and *_head_total, the length the head NEEDS, are written):
 *                   re-house at that length and repeat the call with the same old_tokens (it is idempotent);
 *                   bit 1 = a block gave up waiting for the lengths of the blocks in front of it and wrote nothing (the poll is
 *                   bounded so that every wave exits; it relies on workgroups being dispatched in order of their linear id, which
 *                   holds on gfx950; never seen): a hard error, the appended tokens are incomplete -- MUSTAFAR_COMPRESS=twopass in
 *                   the environment selects the three-launch form that has no such wait.
 *                   A caller that cannot read the flag right behind the launch (graph capture) keeps room for one worst-case
 *                   append (t * 128 halfs): bit 0 is then impossible.
 *   scratch         mustafar_compress_scratch_bytes(B', t) bytes
 */
int64_t mustafar_compress_scratch_bytes(int Bp, int t);
int mustafar_cache_append_kv(void* stream, const void* k_x, const void* v_x, int64_t head_stride, int Bp, int t, int D, int kth_k,
                             int kth_v, const mustafar_cache_view* k_dst, const mustafar_cache_view* v_dst, int old_tokens,
                             int64_t* k_head_total, int64_t* v_head_total, int64_t k_region_halfs, int64_t v_region_halfs,
                             int32_t* overflow_flag, void* scratch);
/*
 * Move a cache into another view (larger rows / regions: cache.py re-houses an arena when an append does not fit) -- the bitmaps
 * and offsets of the first `tokens` tokens and the first `stream_halfs` halfs of every head's stream, one launch.  `dst` has
 * equally spaced stream regions (nz_head_stride > 0); its nz_offset array is written.  tokens % 64 == 0, stream_halfs % 8 == 0.
 */
int mustafar_cache_rehouse(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens,
                           int64_t stream_halfs);
/*
 * Form of the fused compression calls (mustafar_cache_append_kv, mustafar_trigger_compress_batch, mustafar_convert_onepass) from the next call
 * on: 0 = the process default (one pass unless MUSTAFAR_COMPRESS=twopass is in the environment), 1 = one pass, 2 = the two-pass form (three
 * launches, no wait between workgroups).  Round 5: a caller whose one-pass launch reported flag bit 1 (a block gave up waiting for the
 * lengths in front of it) repeats the call ONCE in the two-pass form -- the raw rows are still in place, the call is idempotent -- instead
 * of failing (cache.py; counted in cache.compress_fallbacks).  State of the calling host THREAD (round 6; it was process-wide): read the
 * current value (mustafar_compress_get_form), set it, call, set the old value back.
 * mustafar_compress_test_skip_publish (tests only; MUSTAFAR_EINVAL unless the process runs with MUSTAFAR_TEST_HOOKS=1): the block of this
 * index of the calling thread's NEXT one-pass launch does not publish its length, so that every block behind it times out (bit 1); -1 = off.
 */
int mustafar_compress_set_form(int form);
int mustafar_compress_get_form(void);
int mustafar_compress_test_skip_publish(int block);
/*
 * consolidate() on the device (round 5): the `n_extents` appended extents of a cache, read through its DEVICE table of views (the table
 * mustafar_decode_attention_extents reads), are copied behind the `base_tokens` tokens of `dst` -- a view with equally spaced stream regions
 * that mustafar_cache_rehouse has filled with the base in the launch in front of this one.  Offsets are shifted by the head's stream
 * length in front of each extent (model :352-360), read on the device; nothing is read on the host.  `max_extent_halfs`: an upper bound of
 * a head's stream length in any one extent (sizes the grid; the host knows every extent's lengths).  One launch; n_extents <= 21845.
 */
int mustafar_cache_consolidate_extents(void* stream, const mustafar_cache_view* dst, const mustafar_cache_view* extents, int n_extents, int Bp,
                                       int base_tokens, int64_t max_extent_halfs);
/* Window slide of the trigger (model :392-393) in place: rows [drop, len) of every head move to the front
 * (any number of rows may stay: overlapping ranges are moved in ascending pieces). */
int mustafar_window_drop_front(void* stream, void* k_window, void* v_window, int64_t head_stride, int Bp, int len, int drop);

/*
 * The 256-token trigger of ALL layers in two calls (round 4).  The reference runs the trigger layer by layer inside the attention
 * forward (models/llama_mustafar_kernel.py:324-398), each with a dozen host reads; here the layers' window rows are pruned and
 * compressed into one EXTENT each (mustafar_decode_attention_extents) by launches issued back to back from ONE call, the caller reads
 * every layer's flag and lengths with ONE copy, and a second call lists the extents in the device tables and slides the windows.
 * `items`: HOST array, one entry per layer.
 *   k_window / v_window   [B', capacity, 128] window buffers; rows [0, t) of every head are the raw tokens to compress
 *   k_dst / v_dst         views of the layer's new, EMPTY extent (nz_offset written, idx[h][0] == 0; nz_head_stride != 0)
 *   k_table_slot / v_table_slot   device addresses the views are written to by the finish call (the entry of the layer's extent
 *                         tables that the next decode launch will read), or NULL
 *   k_head_total / v_head_total / overflow_flag   as mustafar_cache_append_kv (the flags zeroed by the caller; one per layer)
 * mustafar_trigger_compress_batch: `scratch` = n x mustafar_compress_scratch_bytes(B', t) bytes; region_halfs as mustafar_cache_append_kv.
 * mustafar_trigger_finish_batch: `len` rows of every window are valid, `drop` (= t) leave; the rows that stay (any number) move to the front.
 */
typedef struct mustafar_trigger_item {
    void* k_window;
    void* v_window;
    mustafar_cache_view  k_dst, v_dst;
    mustafar_cache_view* k_table_slot;
    mustafar_cache_view* v_table_slot;
    int64_t* k_head_total;
    int64_t* v_head_total;
    int32_t* overflow_flag;
} mustafar_trigger_item;
int mustafar_trigger_compress_batch(void* stream, int n, const mustafar_trigger_item* items, int64_t head_stride, int Bp, int t, int D,
                                    int kth_k, int kth_v, int64_t k_region_halfs, int64_t v_region_halfs, void* scratch);
int mustafar_trigger_finish_batch(void* stream, int n, const mustafar_trigger_item* items, int64_t head_stride, int Bp, int len, int drop);

/*
 * head_dim 64 grows by extents too (ABI 108).  Format at D = 64: one tile per token and side, so a 256-token extent has 256 bitmaps
 * and 257 offsets per head (bmp_head_stride / idx_head_stride 0 = exactly that).
 *
 * mustafar_trigger_compress_batch_hd: the arguments of mustafar_trigger_compress_batch; D must be 64 and t 256.  n launches back to
 *   back, one per item, no host work in between (n = 1: the layer-by-layer trigger).  A launch takes the RAW rows [0, 256) of both
 *   windows (head h `head_stride` elements behind head h - 1, rows of 64 contiguous halfs, 16-byte aligned, head_stride % 8 == 0) to a
 *   finished extent: prune (kth = max(1, int(sparsity * 64)); 0 = already pruned), bitmaps, offsets, packed stream.  One workgroup owns
 *   one head's extent and knows its whole stream length before it writes a byte: no workgroup waits for another, so overflow_flag bit 1
 *   never occurs and `scratch` is unused (NULL allowed).  Written through k_dst / v_dst (nz_head_stride != 0, nz 16-byte aligned):
 *   bmp[h][0..256), idx[h][0..256], nz_offset[h] = h * nz_head_stride (where nz_offset is not NULL), the stream at the head's region and
 *   *_head_total[h] (halfs).  *_region_halfs: the room of a region, REQUIRED here (0 < region_halfs <= 8 * nz_head_stride).  A head that
 *   needs more sets bit 0 of overflow_flag, still writes its bitmaps, offsets and head_total (the length it needs) and writes NO stream
 *   bytes; the other heads are complete.  Repeat at the measured size: the call is idempotent.
 * mustafar_trigger_finish_batch_hd: mustafar_trigger_finish_batch with the row width as an argument (the D = 128 call moves rows of 128
 *   halfs whatever head_stride says, and so does mustafar_window_drop_front).  D = 128 forwards; D = 64 lists every item's views in its
 *   table slots (NULL: not listed) and slides rows [drop, len) of 64 halfs to the front, in stream order; the buffers keep their addresses.
 * mustafar_decode_attention_extents_hd: mustafar_decode_attention_extents for a given head_dim.  128 forwards.  64: the D = 64 kernel's
 *   EXT instantiation -- same run shape, slabs and sum order as mustafar_decode_attention_hd at the same T, so the same bits.  Block
 *   tb < T_base / 64 comes from the base views (any strides; nz_head_stride 0: nz_offset is loaded), block T_base / 64 + 4 i + j is block
 *   j of table entry i, resolved per block with scalar loads (a workgroup's run may cross base -> extent and extent -> extent).
 *   Validation as mustafar_decode_attention_hd, and T_base > 0, T_base % 256 == 0, (T - T_base) % 256 == 0, (T - T_base) / 256 <= 512,
 *   tables not NULL when T > T_base.  T == T_base without T_device: the plain launch over the base.  With T_device the grid, slabs,
 *   blocks per workgroup and mask columns are sized for the capacity T; blocks at or beyond *T_device / 64 are skipped (a workgroup with
 *   no block in use leaves slabs of weight zero).  Mask columns, the convention of the D = 128 extents launch: compressed token t reads
 *   column t, window row w reads column *T_device + w -- the tokens IN USE, not the capacity -- so a mask row is the model's own
 *   [0, kv_len) row whatever the capacity.  mustafar_last_decode_choice() reports form 6 when the EXT instantiation ran (5: the plain one).
 */
int mustafar_trigger_compress_batch_hd(void* stream, int n, const mustafar_trigger_item* items, int64_t head_stride, int Bp, int t, int D,
                                       int kth_k, int kth_v, int64_t k_region_halfs, int64_t v_region_halfs, void* scratch);
int mustafar_trigger_finish_batch_hd(void* stream, int n, const mustafar_trigger_item* items, int64_t head_stride, int Bp, int len, int drop,
                                     int D);
int mustafar_decode_attention_extents_hd(void* stream, const mustafar_cache_view* k_base, const mustafar_cache_view* v_base, int T_base,
                                         const mustafar_cache_view* k_extents, const mustafar_cache_view* v_extents,
                                         const void* q, void* k_window, void* v_window, const void* k_new, const void* v_new,
                                         int window_len, int window_capacity, void* scores, int ld_scores, void* out, void* workspace,
                                         int Split_K, int T, int Batch_Size, int num_key_value_groups, float sqrt_d,
                                         const int32_t* window_len_extra, const void* attention_mask, int64_t mask_row_stride,
                                         int heads_per_mask_row, uint32_t flags, const int32_t* T_device, int head_dim);

/*
 * Partial attention (ABI 110): the log-sum-exp of a fused decode call, window-less calls, and the merge of partial states.
 *
 * mustafar_decode_attention_lse_hd / mustafar_decode_attention_extents_lse_hd: every argument of mustafar_decode_attention_hd /
 *   mustafar_decode_attention_extents_hd, then `lse`: fp32 [Batch_Size] out, or NULL.
 *     lse[bh] = M + log(sum_t exp(x_t - M)),  M = max_t x_t, over every token the call attends to (compressed and window), x_t being what
 *     the softmax of that call sees: fp16(fp16(score) / sqrt d), with the hook's mask added and clamped where a mask is given.
 *   It is written by the row kernel that merges the slabs, from the (max, sum) pairs it reduces anyway: no further launch, no second
 *   pass.  `out` is what the plain entry point writes, bit for bit.  lse == NULL: the launches and the bits of the plain entry point
 *   (the row kernels' instantiation without an LSE); mustafar_last_decode_choice() is set as there.
 *   The extents form with T == T_base (no T_device) reads the two base views alone, strides included: the form for one
 *   mustafar_cache_view per side (D = 128: any T_base > 0 that is a multiple of 256).
 *   Window-less calls, accepted by these two entry points only: window_len == 0 && window_capacity == 0 with k_window, v_window, k_new,
 *   v_new and window_len_extra all NULL; T > 0 and ld_scores >= T.  No window workgroups and no window slabs are launched; mask
 *   columns are [0, T).  Any other mixture of zero and non-zero window arguments: MUSTAFAR_EINVAL.
 *   D = 128: the LSE (and a window-less call) is served by the one-pass forms -- every group count and engine, extents, T_device, the
 *   small, super-block and lean-pair kernels, all four row-kernel variants.  A call that would run the two-launch form returns
 *   MUSTAFAR_EINVAL before any launch when lse != NULL: T == 0, ld_scores % 32 != 0, MUSTAFAR_FLAG_TWO_LAUNCH, or a process default of
 *   two launches.  D = 64: every shape the kernel takes (T == 0, empty window chunks, slabs of weight zero behind *T_device).
 *
 * mustafar_merge_attention_states: ONE launch.  Part i = attention over a token set of its own: normalised outputs fp16
 *   [Batch_Size, head_dim] at outs + i * out_part_stride (halfs), LSEs fp32 [Batch_Size] at lses + i * lse_part_stride (floats).
 *   Per row, in fp32:  M = max_i lse_i;  w_i = lse_i == -inf ? 0 : exp(lse_i - M);  out = fp16(sum_i w_i out_i / sum_i w_i);
 *   lse_out = M + log(sum_i w_i).  Every part empty: out = 0, lse_out = -inf.  1 <= n_parts <= 64; head_dim 64 or 128; lse_out may be
 *   NULL; strides at least a part's size when n_parts > 1; `out` must not lie inside the parts (nor lse_out inside the LSEs).
 */
int mustafar_decode_attention_lse_hd(void* stream, const uint64_t* k_bmp, const void* k_nz, const uint32_t* k_idx,
                                     const uint32_t* k_nz_offset, const uint64_t* v_bmp, const void* v_nz, const uint32_t* v_idx,
                                     const uint32_t* v_nz_offset, const void* q, void* k_window, void* v_window, const void* k_new,
                                     const void* v_new, int window_len, int window_capacity, void* scores, int ld_scores, void* out,
                                     void* workspace, int Split_K, int T, int Batch_Size, int num_key_value_groups, float sqrt_d,
                                     const int32_t* window_len_extra, const void* attention_mask, int64_t mask_row_stride,
                                     int heads_per_mask_row, uint32_t flags, int head_dim, float* lse);
int mustafar_decode_attention_extents_lse_hd(void* stream, const mustafar_cache_view* k_base, const mustafar_cache_view* v_base, int T_base,
                                             const mustafar_cache_view* k_extents, const mustafar_cache_view* v_extents,
                                             const void* q, void* k_window, void* v_window, const void* k_new, const void* v_new,
                                             int window_len, int window_capacity, void* scores, int ld_scores, void* out, void* workspace,
                                             int Split_K, int T, int Batch_Size, int num_key_value_groups, float sqrt_d,
                                             const int32_t* window_len_extra, const void* attention_mask, int64_t mask_row_stride,
                                             int heads_per_mask_row, uint32_t flags, const int32_t* T_device, int head_dim, float* lse);
int mustafar_merge_attention_states(void* stream, const void* outs, int64_t out_part_stride, const float* lses, int64_t lse_part_stride,
                                    int n_parts, int Batch_Size, int head_dim, void* out, float* lse_out);

/*
 * Shared-prefix segments (ABI 111): ONE compressed copy of a frozen segment decoded for every sequence of a batch (shared_segment.hip).
 *
 * mustafar_decode_shared_segment: attention of n_seqs query tokens over one cache of `kv_heads` heads and T tokens, and nothing else.
 *   Row (s, h) of q attends to kv head h / num_key_value_groups of the one cache.  Two launches: a workgroup of the first serves one kv
 *   head and a run of consecutive 64-token blocks for all R = n_seqs * num_key_value_groups rows of it -- each block expanded once into a
 *   dense fp16 image in LDS, scores and outputs on the matrix pipe (fp16 x fp16 products, fp32 sums), the online softmax of
 *   mustafar_decode_attention_hd -- and leaves one (max, sum, output) slab per row; the row kernel merges a row's slabs.  The stream,
 *   bitmaps and offsets of a block are requested from memory once per launch, whatever n_seqs is.
 *   k_cache / v_cache   HOST views of a cache in the reference format, head_dim 64 or 128 (tiles = T * head_dim / 64 per head):
 *                       bmp / idx strides 0 (exactly tiles / tiles + 1) or larger; nz_head_stride 0: nz_offset is loaded; nz 16-byte aligned
 *   q, out              fp16 [n_seqs, kv_heads * num_key_value_groups, head_dim], contiguous, 16-byte aligned
 *   lse                 fp32 [n_seqs, kv_heads * num_key_value_groups] out, REQUIRED: M + log(sum_t exp(x_t - M)) as the _lse_hd entry points
 *   workspace           mustafar_shared_segment_workspace_bytes() bytes, 16-byte aligned
 *   No window, no new row, no mask, no extents, no device-side T: a frozen segment has none.  MUSTAFAR_EINVAL before any launch for
 *   T <= 0 or T % 64 != 0, n_seqs * num_key_value_groups outside 1..64, num_key_value_groups outside 1..8, head_dim not 64 or 128, null or
 *   misaligned pointers.  Nothing is read back and nothing is allocated: the call can be captured in a hipGraph.
 * mustafar_shared_segment_workspace_bytes: slabs * kv_heads * R * (head_dim + 2) * 4, slabs = ceil(T / 64 / blocks per run); a run holds
 *   ceil(8 R (head_dim + 2) / (88 head_dim)) blocks, so that the slab bytes written and read stay below the stream bytes of the launch
 *   (DESIGN.md 4.10).  0 for the shapes the call refuses.
 */
int64_t mustafar_shared_segment_workspace_bytes(int T, int kv_heads, int num_key_value_groups, int n_seqs, int head_dim);
int mustafar_decode_shared_segment(void* stream, const mustafar_cache_view* k_cache, const mustafar_cache_view* v_cache,
                                   int T, int kv_heads, int num_key_value_groups, int n_seqs,
                                   const void* q, void* out, float* lse, void* workspace, float sqrt_d, int head_dim);

/*
 * Several query tokens per call (ABI 112): n_q consecutive tokens of every sequence decoded by ONE call over the live cache (multi_query.hip).
 *
 * mustafar_decode_multi_query: query token j (0 .. n_q - 1) of sequence b attends to the compressed tokens [0, T) of its own cache and to
 *   window rows [0, window_len - n_q + j] -- its own new row and everything older; the rows of the later tokens are masked (the causal
 *   limit among the new tokens: the only mask).  window_len counts the rows AFTER the append, as in mustafar_decode_attention.  Three
 *   launches (two with k_new == NULL): the n_q new rows are copied into the windows; then a workgroup serves one (sequence, kv head) and
 *   either a run of consecutive 64-token blocks or 64 window rows for all R = n_q * num_key_value_groups rows of it -- each block expanded
 *   once into a dense fp16 image in LDS, scores and outputs on the matrix pipe, the arithmetic of mustafar_decode_shared_segment -- and
 *   leaves one (max, sum, output) slab per row; the row kernel merges a row's slabs.
 *   k_base / v_base     HOST views of tokens [0, T_base) of B' = batch * kv_heads heads, any strides (nz_head_stride 0: nz_offset is
 *                       loaded), as in mustafar_decode_shared_segment; may be NULL when T == 0 (nothing compressed yet: window only)
 *   k_extents / v_extents   DEVICE tables as in mustafar_decode_attention_extents_hd: entry i holds tokens [T_base + 256 i, T_base + 256 (i + 1)),
 *                       offsets relative to the extent, bmp / idx strides 0 = exactly 4 blocks' tiles / + 1, nz_head_stride != 0 or nz_offset
 *                       loaded; resolved per block with scalar loads (a run may cross base -> extent and extent -> extent).  NULL when
 *                       T == T_base.  T > T_base needs T_base % 256 == 0, (T - T_base) % 256 == 0 and at most 512 entries; T == T_base: any
 *                       multiple of 64.  T > 0 needs T_base > 0
 *   q, out              fp16 [B', num_key_value_groups, n_q, head_dim] -- the hook's [bsz, heads, n_q, head_dim] --, contiguous, 16-byte aligned
 *   lse                 fp32 [B', num_key_value_groups, n_q] out, REQUIRED: M + log(sum_t exp(x_t - M)) over what the row saw, x as in the
 *                       _lse_hd entry points
 *   k_window / v_window [B', window_capacity, head_dim]; k_new / v_new [B', n_q, head_dim] are copied to rows [window_len - n_q, window_len)
 *                       (both NULL: the rows are already stored); 16-byte aligned
 *   workspace           mustafar_decode_multi_query_workspace_bytes() bytes, 16-byte aligned
 *   MUSTAFAR_EINVAL before any launch for: n_q < 1, n_q * num_key_value_groups > 64, num_key_value_groups outside 1..8, head_dim not 64 or
 *   128, Bp outside 1..65535, T < 0 or T % 64 != 0, the T_base / extent rules above, window_len < n_q, window_len > window_capacity,
 *   window_capacity > 1024, exactly one of k_new / v_new NULL, NULL or misaligned q / out / windows / new rows / workspace / lse, a base
 *   view mustafar_decode_shared_segment would refuse.  The mask comes with mustafar_decode_multi_query_masked (ABI 114, below), device-side
 *   lengths (window_len_extra, T_device) with mustafar_decode_multi_query_lengths (ABI 115, below); this call is their form with all
 *   three NULL.  Nothing is allocated and nothing is read back: the call can be captured in a hipGraph, which replays these lengths.
 * mustafar_decode_multi_query_workspace_bytes: (ceil(T / 64 / bpw) + ceil(window_capacity / 64)) * Bp * R * (head_dim + 2) * 4, with
 *   bpw = ceil(8 R (head_dim + 2) / (88 head_dim)) blocks per run, the rule of mustafar_shared_segment_workspace_bytes.  0 for the
 *   shapes the call refuses.
 */
int64_t mustafar_decode_multi_query_workspace_bytes(int T, int window_capacity, int Bp, int num_key_value_groups, int n_q, int head_dim);
int mustafar_decode_multi_query(void* stream, const mustafar_cache_view* k_base, const mustafar_cache_view* v_base, int T_base,
                                const mustafar_cache_view* k_extents, const mustafar_cache_view* v_extents,
                                int T, int Bp, int num_key_value_groups, int n_q,
                                const void* q, void* k_window, void* v_window, const void* k_new, const void* v_new,
                                int window_len, int window_capacity, void* out, float* lse, void* workspace, float sqrt_d, int head_dim);

/*
 * Attention masks and draft trees in the several-token call (ABI 114; multi_query.hip).
 *
 * mustafar_decode_multi_query_masked: mustafar_decode_multi_query (its 22 arguments first, in the same order, same workspace) with an additive
 *   fp16 mask.  For head b of B', query token j and column c -- c = t for compressed token t, c = T + w for window row w -- a column the
 *   causal limit lets the token see counts as x' = max(fp16(x + m), finfo(fp16).min), m = mask[(b / heads_per_mask) * mask_batch_stride +
 *   (mask_rows == 1 ? 0 : j) * mask_row_stride + c]: ONE fp16 addition, so m = -inf gives finfo.min -- the hook's rule, as in every fused
 *   entry point.  The causal limit stays on top: a column beyond window_len - n_q + j is not seen whatever the mask says (and its mask value
 *   is not read), so a mask only takes columns away; columns at or beyond T + window_len are never read.  A row whose every visible column
 *   is masked to finfo.min returns what the clamp implies (about the mean of the visible V rows), finite.
 *   mask                fp16, DEVICE, any 2-byte aligned address (a column slice of a wider tensor); strides in halfs.  NULL: exactly the
 *                       launches of mustafar_decode_multi_query (the other mask arguments are not looked at)
 *   mask_rows           1 (one row for all n_q tokens) or n_q
 *   heads_per_mask      consecutive B' heads that share a mask plane (kv_heads for one plane per sequence); 1..Bp, a divisor of Bp
 *   MUSTAFAR_EINVAL before any launch, beyond the cases of mustafar_decode_multi_query: mask at an odd address, mask_rows outside {1, n_q},
 *   heads_per_mask out of range or no divisor of Bp, mask_row_stride < T + window_len with mask_rows > 1, mask_batch_stride < T + window_len
 *   with Bp / heads_per_mask > 1, a negative stride.
 *
 * mustafar_window_keep_rows: for every head and both windows [Bp, window_capacity, head_dim], row row0 + i <- row row0 + keep[seq][i] for
 *   i < n_keep, seq = head / heads_per_seq: the rows of an accepted path of a draft tree moved to the front of the n_rows rows the call
 *   appended.  One launch, one workgroup per (head, window): every source row is read before the first is written, so any index order and
 *   duplicates are safe; an index outside [0, n_rows) is clamped into it (a wrong row, never a wild address).  Rows outside
 *   [row0, row0 + n_keep) are left bit for bit as they are.
 *   keep                int32, DEVICE, [Bp / heads_per_seq][n_keep], 4-byte aligned
 *   MUSTAFAR_EINVAL for: n_keep outside 1..n_rows, n_rows outside 1..64, row0 < 0 or row0 + n_rows > window_capacity, window_capacity > 1024,
 *   head_dim not 64 or 128, NULL or misaligned (16 B) windows, a NULL or misaligned (4 B) keep, Bp outside 1..65535, heads_per_seq < 1 or
 *   no divisor of Bp.
 * Neither call allocates or reads anything back: both can be captured in a hipGraph (these lengths; mustafar_decode_multi_query_lengths
 * below takes them from the device).
 */
int mustafar_decode_multi_query_masked(void* stream, const mustafar_cache_view* k_base, const mustafar_cache_view* v_base, int T_base,
                                       const mustafar_cache_view* k_extents, const mustafar_cache_view* v_extents,
                                       int T, int Bp, int num_key_value_groups, int n_q,
                                       const void* q, void* k_window, void* v_window, const void* k_new, const void* v_new,
                                       int window_len, int window_capacity, void* out, float* lse, void* workspace, float sqrt_d, int head_dim,
                                       const void* mask, int64_t mask_batch_stride, int64_t mask_row_stride, int mask_rows, int heads_per_mask);
int mustafar_window_keep_rows(void* stream, void* k_window, void* v_window, int Bp, int heads_per_seq, int window_capacity, int head_dim,
                              int row0, int n_rows, const int32_t* keep, int n_keep);

/*
 * Device-side lengths in the several-token call (ABI 115; multi_query.hip): ONE captured graph of the call replayed while
 * the window and the compressed cache grow.
 *
 * mustafar_decode_multi_query_lengths: mustafar_decode_multi_query_masked (its 27 arguments first, in the same order, same workspace)
 *   with two DEVICE ints, either of which may be NULL, read once per workgroup when the kernels start -- the conventions of
 *   mustafar_decode_attention_extents_hd.  Both NULL: exactly the launches and bits of mustafar_decode_multi_query_masked, which is this
 *   call with two NULLs.
 *   window_len_extra    the window length in effect is w = window_len + *window_len_extra, clamped by the kernels into
 *                       [n_q, window_capacity] (a bad counter gives a wrong row, never an address outside the window buffers): the new
 *                       rows are copied to rows [w - n_q, w), query token j sees window rows [0, w - n_q + j], image rows at or beyond w
 *                       are zero.  window_len itself keeps the host rules, n_q <= window_len <= window_capacity.  The caller advances
 *                       the int between replays (mustafar_counter_add) by the rows that stayed
 *   T_device            T becomes the CAPACITY the launch is sized for -- grid, slabs, workspace -- and *T_device the compressed tokens IN
 *                       USE: T_base plus a multiple of 256, clamped by the kernels into [T_base, T].  Needs T > T_base and both tables.
 *                       Blocks at or beyond *T_device / 64 are skipped: a run that straddles the limit ends at it, and so does what it
 *                       requests ahead; a run with no block in use touches no byte of the cache (no base loads, no nz_offset load, no
 *                       table entry) and leaves slabs of weight zero.  Table entries at or beyond (*T_device - T_base) / 256 are never
 *                       read, so the caller fills them as the cache grows; it adds 256 to *T_device when a trigger has listed an extent
 *                       and takes 256 off *window_len_extra, the windows having slid
 *   mask columns        compressed token t reads column t, window row w reads column *T_device + w -- the tokens IN USE, not the
 *                       capacity --, so a mask row is the model's own; columns at or beyond *T_device + w are never read.  With either
 *                       pointer not NULL the stride rules of the mask take T + window_capacity in place of T + window_len: a row reaches as
 *                       far as the lengths can
 *   MUSTAFAR_EINVAL before any launch, beyond the cases of mustafar_decode_multi_query_masked: T_device with T == T_base or a NULL table,
 *   either pointer not 4-byte aligned, the mask strides above.  Nothing is allocated and nothing is read back.
 */
int mustafar_decode_multi_query_lengths(void* stream, const mustafar_cache_view* k_base, const mustafar_cache_view* v_base, int T_base,
                                        const mustafar_cache_view* k_extents, const mustafar_cache_view* v_extents,
                                        int T, int Bp, int num_key_value_groups, int n_q,
                                        const void* q, void* k_window, void* v_window, const void* k_new, const void* v_new,
                                        int window_len, int window_capacity, void* out, float* lse, void* workspace, float sqrt_d, int head_dim,
                                        const void* mask, int64_t mask_batch_stride, int64_t mask_row_stride, int mask_rows, int heads_per_mask,
                                        const int32_t* window_len_extra, const int32_t* T_device);

/*
 * Several query tokens per call over frozen and shared segments (shared_segment.hip, multi_query.hip).  These four symbols
 * were added WITHOUT a change of mustafar_abi_version(), which stays 115: nothing that existed changed its behaviour or its bits, and a
 * caller detects the new entry points by symbol (dlsym), not by version.
 *
 * mustafar_decode_shared_segment_multi: mustafar_decode_shared_segment for n_q query tokens of each of n_seqs sequences: one cache of
 *   `kv_heads` heads is read for n_seqs * n_q query tokens, every row sees all T tokens (a frozen segment has no causal limit among them).
 *   q, out              fp16 [n_seqs, kv_heads * num_key_value_groups, n_q, head_dim] -- the hook's [bsz, heads, n_q, head_dim] --, contiguous,
 *                       16-byte aligned;  lse fp32 [n_seqs, kv_heads * num_key_value_groups, n_q], REQUIRED
 *   rows                local row of kv head h: r = s * (groups * n_q) + g * n_q + j for sequence s, q head g of the kv head, query token j;
 *                       R = n_seqs * groups * n_q in 1..1024, groups in 1..8 (groups * n_q is not limited to 8)
 *   launches            two, whatever R: the rows of a kv head are cut into chunks of 64 consecutive local rows (the last one shorter; a
 *                       boundary may fall inside a sequence's rows), the chunks are blockIdx.z of ONE decode launch -- a workgroup serves
 *                       (run, kv head, chunk) and expands its blocks for its own chunk --, and one row-kernel launch merges all rows.  Row
 *                       tiles: those of 64 rows with more than one chunk, else those of R; rows at or beyond R are zero query rows
 *   run length          ceil(8 min(R, 64) (head_dim + 2) / (88 head_dim)) blocks, the rule of mustafar_shared_segment_workspace_bytes
 *   bits                with R <= 64 the launches ARE those of mustafar_decode_shared_segment with groups * n_q in place of groups (the same
 *                       kernel instantiations): bit for bit its result on the same rows.  A chunk of 64 rows gives the bits of a 64-row call
 *                       on those rows
 *   MUSTAFAR_EINVAL before any launch for n_q < 1, R outside 1..1024, and everything mustafar_decode_shared_segment refuses.  Nothing is
 *   read back and nothing is allocated: the call can be captured in a hipGraph.
 * mustafar_shared_segment_multi_workspace_bytes: ceil(T / 64 / run length) * kv_heads * R * (head_dim + 2) * 4; 0 for the shapes the call refuses.
 *
 * mustafar_decode_multi_segment: mustafar_decode_multi_query_masked over compressed tokens ONLY -- the several-token call over a frozen
 *   per-sequence segment: no window, no new rows, no append launch, no window workgroups, no causal limit (query token j sees all T tokens),
 *   no device-side lengths.  Two launches.
 *   k_base .. T         Bp caches as in mustafar_decode_multi_query: base views, T_base, the DEVICE tables of 256-token extents, the same
 *                       T_base / extent rules; T > 0 (and so T_base > 0) is required
 *   q, out, lse         as in mustafar_decode_multi_query: fp16 [B', groups, n_q, head_dim], fp32 [B', groups, n_q]
 *   rows                R = n_q * groups in 1..1024 (a 256-token follow-up turn at GQA-4 is one launch pair), cut into 64-row chunks in
 *                       blockIdx.z exactly as above; run length and workspace by the same rule with Bp for kv_heads
 *   mask                as in mustafar_decode_multi_query_masked with the columns [0, T): mask_rows 1 or n_q, the clamp rule, strides in
 *                       halfs, mask_row_stride >= T with mask_rows > 1, mask_batch_stride >= T with Bp / heads_per_mask > 1.  A row masked
 *                       entirely returns what the clamp implies, finite.  NULL: no mask (the other four arguments are not looked at)
 *   MUSTAFAR_EINVAL before any launch for T <= 0 or T % 64 != 0, n_q < 1, n_q * groups > 1024, groups outside 1..8, head_dim not 64 or 128,
 *   Bp outside 1..65535, the T_base / extent rules, NULL or misaligned q / out / lse / workspace, a base view mustafar_decode_shared_segment
 *   would refuse, the mask rules.  Nothing is allocated and nothing is read back: the call can be captured in a hipGraph.
 * mustafar_decode_multi_segment_workspace_bytes: ceil(T / 64 / run length) * Bp * R * (head_dim + 2) * 4; 0 for the shapes the call refuses.
 */
int64_t mustafar_shared_segment_multi_workspace_bytes(int T, int kv_heads, int num_key_value_groups, int n_seqs, int n_q, int head_dim);
int mustafar_decode_shared_segment_multi(void* stream, const mustafar_cache_view* k_cache, const mustafar_cache_view* v_cache,
                                         int T, int kv_heads, int num_key_value_groups, int n_seqs, int n_q,
                                         const void* q, void* out, float* lse, void* workspace, float sqrt_d, int head_dim);
int64_t mustafar_decode_multi_segment_workspace_bytes(int T, int Bp, int num_key_value_groups, int n_q, int head_dim);
int mustafar_decode_multi_segment(void* stream, const mustafar_cache_view* k_base, const mustafar_cache_view* v_base, int T_base,
                                  const mustafar_cache_view* k_extents, const mustafar_cache_view* v_extents,
                                  int T, int Bp, int num_key_value_groups, int n_q,
                                  const void* q, void* out, float* lse, void* workspace, float sqrt_d, int head_dim,
                                  const void* mask, int64_t mask_batch_stride, int64_t mask_row_stride, int mask_rows, int heads_per_mask);

/*
 * Ragged batches: independent per-sequence caches decoded in one call (ragged_batch.hip).  These three symbols were added
 * WITHOUT a change of mustafar_abi_version(), which stays 115: nothing that existed changed its behaviour or its bits, and a caller
 * detects the new entry points by symbol (dlsym), not by version.
 *
 * mustafar_sequence: one sequence of a ragged batch -- a cache of `kv_heads` heads, its two windows and its lengths --, an entry of a
 *   DEVICE table that mustafar_ragged_set_sequences alone writes (it stores the row strides of the base views resolved; what else it
 *   stores is its business).  176 bytes: k_base at 0, v_base at 64, k_extents at 128, v_extents at 136, k_window at 144, v_window at 152,
 *   T_base at 160, T at 164, window_len at 168, window_capacity at 172.
 *
 * mustafar_ragged_set_sequences: entries [first, first + n) of `table` (DEVICE, 8-byte aligned, the caller's allocation of at least
 *   first + n entries) <- `items` (a HOST array), through small launches that carry the items in their kernel arguments (16 entries per
 *   launch), as mustafar_trigger_finish_batch lists views in table slots: no host-to-device copy, nothing allocated, nothing read back; in
 *   stream order with the decode calls that read the table.  Every item is validated before the first launch, by the rules of
 *   mustafar_decode_multi_query: T % 64 == 0, T > 0 needs T_base > 0, T_base % 64 == 0 and T_base <= T; T > T_base needs both tables,
 *   T_base % 256 == 0, (T - T_base) % 256 == 0 and at most 512 entries; with T_base > 0 both base views are what
 *   mustafar_decode_shared_segment accepts for `kv_heads` heads (flags == 0: tiles); the windows are 16-byte aligned and not NULL;
 *   n_q <= window_len <= window_capacity <= 1024.  window_len == 0 marks an EMPTY slot: nothing else of such an item is looked at, every
 *   pointer may be NULL.  With T == 0 the base views, and with T == T_base the tables, are not looked at.
 *   MUSTAFAR_EINVAL before any launch for an item that breaks a rule, n < 1, first < 0, a NULL or misaligned (8 B) table, NULL items,
 *   kv_heads outside 1..65535, head_dim not 64 or 128, n_q < 1.
 *
 * mustafar_decode_ragged: mustafar_decode_multi_query for n_seqs sequences that share nothing but the head geometry and n_q.  Query token
 *   j of sequence s attends to the compressed tokens [0, T_s) of its own cache and to rows [0, window_len_s - n_q + j] of its own window,
 *   the causal limit of that call; there is no mask (a ragged batch has no padding to hide).  Three launches (two with k_new == NULL):
 *   the n_q new rows of sequence s go to rows [window_len_s - n_q, window_len_s) of its windows; a workgroup of (sequence, kv head) loads
 *   its entry with scalar loads and serves a run of blocks or 64 window rows as in mustafar_decode_multi_query; the row kernel folds the
 *   slabs of a row in the sequence's own numbering.
 *   table               DEVICE, n_seqs entries written by mustafar_ragged_set_sequences with the same kv_heads, n_q and head_dim; read at
 *                       every launch, so one captured graph of this call serves whatever the table holds at replay
 *   q, out              fp16 [n_seqs, kv_heads * num_key_value_groups, n_q, head_dim], contiguous, 16-byte aligned
 *   lse                 fp32 [n_seqs, kv_heads * num_key_value_groups, n_q], REQUIRED
 *   k_new / v_new       [n_seqs, kv_heads, n_q, head_dim], 16-byte aligned, or both NULL: the rows are already stored
 *   T_max, window_capacity_max   size the grid (ceil(T_max / 64 / run length) + ceil(window_capacity_max / 64), n_seqs * kv_heads), the slabs
 *                       and the workspace; run length: the rule of mustafar_decode_multi_query (R = n_q * groups and head_dim alone)
 *   clamps              the kernels clamp every length they load: blocks in use T_s / 64 into [0, T_max / 64]; blocks from the base
 *                       min(T_base_s / 64, blocks in use); the window capacity into [0, min(window_capacity_max, 1024)]; the window length
 *                       into [n_q, capacity]; an entry without both tables reads its base alone.  A stale or wrong entry gives a wrong
 *                       row, never an address outside a window
 *   dead workgroups     a run with no block in use for its sequence, a window chunk at or beyond its sequence's window and every workgroup
 *                       of an empty slot touch no byte of any cache or window and write no slab; table entries of a sequence's extents
 *                       at or beyond (T_s - T_base_s) / 256 are never read
 *   empty slot          reads nothing, appends nothing; out = 0 and lse = -inf, as mustafar_merge_attention_states gives an all-empty row
 *   bits                out and lse of sequence s are bit for bit those of mustafar_decode_multi_query on that sequence alone (Bp = kv_heads,
 *                       its own T, T_base, tables, window length and capacity), whatever else the batch holds and in whatever slot
 *   MUSTAFAR_EINVAL before any launch for: n_seqs < 1, kv_heads < 1, n_seqs * kv_heads > 65535, n_q * num_key_value_groups outside 1..64,
 *   num_key_value_groups outside 1..8, head_dim not 64 or 128, T_max < 0 or T_max % 64 != 0, window_capacity_max outside n_q..1024, exactly
 *   one of k_new / v_new NULL, a NULL or misaligned table (8 B), q / out / workspace / new rows (16 B) or lse (4 B).  Nothing is allocated
 *   and nothing is read back.
 * mustafar_decode_ragged_workspace_bytes: mustafar_decode_multi_query_workspace_bytes(T_max, window_capacity_max, n_seqs * kv_heads,
 *   num_key_value_groups, n_q, head_dim); 0 for the shapes the call refuses.
 */
typedef struct mustafar_sequence {           /* 176 bytes; an entry of a DEVICE table, written by mustafar_ragged_set_sequences only */
    mustafar_cache_view k_base, v_base;      /* tokens [0, T_base) of kv_heads heads, TILE format (flags == 0), any strides */
    const mustafar_cache_view* k_extents;    /* DEVICE tables as in mustafar_decode_multi_query; NULL when T == T_base */
    const mustafar_cache_view* v_extents;
    void* k_window;  void* v_window;         /* [kv_heads, window_capacity, head_dim] fp16, 16-byte aligned */
    int32_t T_base, T, window_len, window_capacity;   /* window_len counts the rows AFTER this call's append; 0 = the slot is empty */
} mustafar_sequence;

int64_t mustafar_decode_ragged_workspace_bytes(int T_max, int window_capacity_max, int n_seqs, int kv_heads,
                                               int num_key_value_groups, int n_q, int head_dim);
int mustafar_ragged_set_sequences(void* stream, mustafar_sequence* table, int first, int n, const mustafar_sequence* items,
                                  int kv_heads, int n_q, int head_dim);
int mustafar_decode_ragged(void* stream, const mustafar_sequence* table, int n_seqs, int kv_heads, int num_key_value_groups, int n_q,
                           int T_max, int window_capacity_max, const void* q, const void* k_new, const void* v_new,
                           void* out, float* lse, void* workspace, float sqrt_d, int head_dim);

/*
 * head_dim 64 (ABI 109): a prefill compressed from the RAW rows, and 256-token pieces gathered into one reference-layout cache.  D must
 * be 64 in both (MUSTAFAR_EINVAL otherwise); both validate before they launch.
 *
 * mustafar_prefill_compress_hd: ONE launch for one layer, grid (kv head, 256-token chunk, K / V): the launch of
 *   mustafar_trigger_compress_batch_hd with a chunk index.  Chunk c of head h reads the raw rows [256 c, 256 c + 256) at
 *   x + h * head_stride + c * 256 * 64 (head_stride: whatever the caller's buffer has -- in a prefill L * 64 with only the first t rows of a
 *   head compressed; rows 16-byte aligned, head_stride % 8 == 0, head_stride >= t * 64) and writes an EXTENT OF ITS OWN exactly as the
 *   trigger writes one: prune (kth = 0: already pruned), 256 bitmaps, 257 offsets starting at 0, nz_offset, the stream in the chunk's
 *   region, the chunk's length.  t % 256 == 0, 0 < t <= 512 * 256.
 *   k_stage / v_stage     HOST views of chunk 0's extent (as k_dst / v_dst of mustafar_trigger_item: nz_head_stride != 0, nz 16-byte
 *                         aligned, bmp / idx strides 0 or >= 256 / 257).  Every array of chunk c lies c * {k,v}_chunk_bytes BYTES behind
 *                         chunk 0's (chunk_bytes > 0, % 16 == 0): t / 256 equally spaced extents per side
 *   k_pieces / v_pieces   DEVICE arrays of t / 256 mustafar_cache_view, or NULL: entry c is written with chunk c's view by this launch --
 *                         the table mustafar_cache_gather_hd (or mustafar_decode_attention_extents_hd) reads
 *   k_head_total / v_head_total   i64 [t / 256][B'] out: chunk c's length of head h in halfs at [c * B' + h]
 *   *_region_halfs        the room of a (head, chunk) region, REQUIRED (0 < region_halfs <= 8 * nz_head_stride).  A (head, chunk) that
 *                         needs more sets bit 0 of overflow_flag (device int, REQUIRED, zeroed by the caller), still writes its bitmaps,
 *                         offsets and length (the length it needs) and writes NO stream bytes; every other (head, chunk) is complete.
 *                         The call is idempotent: repeat it at the measured size.  No workgroup waits for another: bit 1 never occurs.
 * mustafar_cache_gather_hd: ONE launch, grid (piece, kv head), nothing read on the host, no workgroup waits for another.  Gathers, one side
 *   per call, an optional first cache of `first_tokens` tokens and the `n_pieces` 256-token pieces of a DEVICE table (entry i: tokens
 *   [first_tokens + 256 i, first_tokens + 256 (i + 1)), offsets relative to the piece, nz_head_stride != 0 or nz_offset loaded; bmp / idx
 *   strides 0 = 256 / 257) into `dst`, a reference-layout cache of first_tokens + 256 n_pieces tokens: bitmaps copied, offsets shifted by
 *   the head's stream length in front of the piece (model :352-360) -- the first view's last offset and the last offsets of the pieces in
 *   front, summed on the device --, streams copied head behind piece behind piece.
 *   first      HOST view (any strides; nz_head_stride 0: nz_offset is loaded) or NULL with first_tokens == 0; first_tokens % 256 == 0
 *   pieces     DEVICE table; n_pieces <= 512 (NULL with n_pieces == 0); first_tokens / 256 + n_pieces >= 1
 *   dst        HOST view: bmp / idx strides 0 (exactly the tokens / tokens + 1) or larger (columns beyond are not written); the CALLER has
 *              set nz_head_stride (!= 0: head h starts at h * nz_head_stride) or filled nz_offset (uint4 units) from the lengths it knows
 *              on the host, and has sized nz for them; neither is written here.  idx[h][0] is written (0).
 *   Alignment: streams move as 16-byte pieces.  Every tile's stream is padded to 8 halfs, so every length and offset is a multiple of
 *   16 bytes; REQUIRED of the caller: nz of dst, first and every piece 16-byte aligned (head starts are in uint4 units already).
 */
int mustafar_prefill_compress_hd(void* stream, const void* k_x, const void* v_x, int64_t head_stride, int Bp, int t, int D, int kth_k, int kth_v,
                                 const mustafar_cache_view* k_stage, const mustafar_cache_view* v_stage, int64_t k_chunk_bytes,
                                 int64_t v_chunk_bytes, mustafar_cache_view* k_pieces, mustafar_cache_view* v_pieces, int64_t* k_head_total,
                                 int64_t* v_head_total, int64_t k_region_halfs, int64_t v_region_halfs, int32_t* overflow_flag);
int mustafar_cache_gather_hd(void* stream, const mustafar_cache_view* dst, const mustafar_cache_view* first, int first_tokens,
                             const mustafar_cache_view* pieces, int n_pieces, int Bp, int D);

/*
 * FMA engine, process default (a fused call may carry its own in `flags`):
 *   2 = v_dot2_f32_f16 on pairs of tiles (default; GQA-4 one-pass decode launches).  One instruction does two tiles of one head, so
 *       the FMA phase costs 2 + 1.5 cheap instead of 4 vector instructions per tile.  For normal fp16 inputs the instruction is a
 *       two-term dot product with ONE rounding; a product with an fp16-SUBNORMAL input can lose up to its whole value (measured on
 *       gfx950, tools/ubench/dot2_asm_numerics.hip: under 1 % of such products do; never more than the product itself).  So the
 *       softmax weights travel scaled by 2^15 (weights down to 2^-29 stay normal; exactly undone when the slab is written), and a
 *       non-zero K / V / q element below 2^-14 contributes with an absolute error of at most 6.1e-5 x |coefficient| -- inside the
 *       fp16 rounding of the scores and outputs.  Kernels without a dot2 form (the two reference entry points, G < 4) run engine 0.
 *   0 = v_fma_mix_f32 per tile and head (exact fp16 x fp16 products in fp32, subnormals included)
 *   1 = v_mfma_f32_4x4x4_16B_f16 used as a 4-wide FMA unit (opt-in: the north_star leaves MFMA off)
 * Environment: MUSTAFAR_FMA_ENGINE=dot2|valu|mfma.  fp32 accumulation in every engine.
 */
int mustafar_set_fma_engine(int engine);
int mustafar_get_fma_engine(void);

/*
 * Structure of mustafar_decode_attention{,_view}: 1 = one-pass launch -- every wave runs key phase, softmax step and value
 * phase on its 64-token blocks and leaves (max, sum, unnormalised output) slabs that a row kernel merges (flash-decoding over
 * the compressed cache; needs ld_scores % 32 == 0, otherwise the other form runs); 0 = the round-1 form, key SpMV -> softmax
 * rows -> value SpMV -> sum; 2 (default) = the one-pass launch at every size and for every group count
 * (since round 3 it beats two launches at c2 .. c5 on all engines; the two-launch form runs when ld_scores % 32 != 0).  Also MUSTAFAR_ONEPASS=0|1|auto in the environment.  Same inputs, same
 * outputs within fp16 (the one-pass form normalises in fp32 at the end instead of rounding the probabilities to fp16).
 */
int mustafar_set_onepass(int mode);
int mustafar_get_onepass(void);
/* What the last fused call on the calling thread launched: FMA engine that ran (0 v_fma_mix_f32, 1 matrix pipe, 2 v_dot2_f32_f16)
 * | structure << 4 (0 two launches, 1 one-pass) | one-pass form << 8 (0 round-2 forms, 1 lean whole-block: both removed, the codes no longer occur; 2 lean pair grain, 3 super-block pair form: round 5, the default from 768 workgroups on, 4 the small-launch form: round 6, the default below that, 5 the head_dim 64 kernel of mustafar_decode_attention_hd, 6 its extents instantiation: mustafar_decode_attention_extents_hd);
 * -1 before the first call.  For tests and tools: a call's `flags` and the process defaults can be checked against what ran. */
int mustafar_last_decode_choice(void);
/* Tuning knobs for the measurement scripts under tools/ (launch shapes of the one-pass forms); not an operator interface.
 * Round 6: knob 11 = the small-launch kernel (0 never, 1 launches of two blocks per workgroup that put at most one wave on every SIMD -- the
 * default, 2 every launch of two blocks per workgroup); knob 13 = Value_SplitK_API with N_Global = 8 on the lean kernel, the pad rows read by
 * workgroups of their own behind the row-0 workgroups (1, the default) or on round 1's kernel (0).
 * Knob 0 chose among three generations of the one-pass kernel; the two older ones were removed: value 2 is accepted and does nothing,
 * 0 and 1 return MUSTAFAR_EINVAL, and so does knob 12 (the speculative first-chunk request, an experiment that measured slower). */
int mustafar_tune(int knob, int value);

/*
 * Live kernel timing inside mustafar_decode_attention (bench.py roofline leg): HIP events that receive the start and
 * stop timestamps of the key and the value SpMV kernels themselves (hipExtLaunchKernel; the same interval rocprofv3
 * reports) for up to `max_records` calls.  mustafar_profile_end() waits for the recorded events, returns the average
 * durations in microseconds and releases the events.
 */
int mustafar_profile_begin(int max_records);
int mustafar_profile_end(double* key_us_avg, double* value_us_avg, int* records);
/* The same, and the average duration of the row kernel behind a one-pass launch (onepass_finish_kernel; 0 unless every record is one). */
int mustafar_profile_end2(double* key_us_avg, double* value_us_avg, double* finish_us_avg, int* records);

#ifdef __cplusplus
}
#endif
#endif /* MUSTAFAR_HIP_H */
