// multi_query.hip -- several query tokens of every sequence per fused decode call, head_dim 64 and 128, for gfx950.  The C ABI entry points
// mustafar_decode_multi_query, mustafar_decode_multi_query_masked, mustafar_decode_multi_query_lengths,
// mustafar_decode_multi_query_workspace_bytes and mustafar_window_keep_rows (include/mustafar_hip.h, ABI 112, 114 and 115),
// and the call over a frozen per-sequence segment, mustafar_decode_multi_segment with its workspace size.
//
// A caller that verifies n_q drafted tokens, or feeds a short follow-up turn, would issue n_q decode steps, each re-reading the whole
// compressed cache and paying the per-tile cost of the format -- bitmap, rank, address, select -- again.  The n_q tokens of one sequence are
// R = n_q * G query rows over that sequence's own kv head: the arithmetic of shared_segment.hip, whose engine expands a 64-token block once
// into a dense fp16 image in LDS and serves up to 64 rows with v_mfma_f32_16x16x32_f16.  This file adds what a step over the LIVE cache
// needs beyond that: per-sequence caches, the 256-token extents, the dense window and a causal limit among the new tokens.
//
// q, out [B', G, n_q, D] (the hook's [bsz, H, n_q, D]), lse [B', G, n_q]: the R rows of one (sequence, kv head) are consecutive, local row
// r = g * n_q + j for q head g and query token j, padded to row tiles of 16 with zero query rows.
//
// multi_query_append_kernel   copies the n_q new K / V rows of every head to rows [window_len - n_q, window_len) of its window, in a launch
//                             of its own in front: stream order makes them visible to every workgroup of the decode launch
// multi_query_decode_kernel   grid (compressed runs + window chunks, B'), 256 threads; a workgroup serves all R rows of one (sequence, kv head)
//   compressed run   `bpw` consecutive 64-token blocks with the phases and barriers of shared_segment_decode_kernel: stage, K expand, scores,
//                    softmax step, V expand, out.  EXT: block tb < T_base / 64 comes from the base view, block T_base / 64 + 4 i + j is block
//                    j of entry i of a DEVICE table of mustafar_cache_view (offsets relative to the extent), resolved per block with
//                    wave-uniform loads as headdim64.hip's extent_block does: a run may cross base -> extent and extent -> extent, and what
//                    is requested ahead (the next block's metadata and key stream) follows the resolution of the NEXT block
//   window chunk     64 rows of the dense window: the key image [token][channel] is filled straight from the rows of k_window as 16-byte
//                    pieces, the value image [channel][token] is the transpose of the rows of v_window; scores, softmax step and out as for
//                    a compressed block.  The causal limit: window row w is visible to query token j iff
//                    w <= window_len - n_q + j.  An invisible column counts as x = -inf, e = 0; a row that sees no column of its chunk
//                    stays at M = -inf, L = 0 (a slab of weight zero).  Image rows at or beyond window_len are written as zeros
//                    (0 x garbage through the matrix pipe is NaN where the garbage is Inf or NaN).  Chunks at or beyond
//                    ceil(window_len / 64) leave slabs of weight zero
//   MASK             an additive fp16 mask, one row per query token or one for all, one plane per `heads_per_mask` consecutive heads: column
//                    64 tb + t of a compressed block (tb the GLOBAL block number), T + w of window row w.  A softmax thread owns 16
//                    consecutive columns of one row: it asks for their mask values early -- behind the key expand of a compressed block,
//                    ahead of the image fill of a window chunk -- and holds them packed.  x' = max(fp16(x + m), finfo(fp16).min), ONE fp16
//                    addition, the hook's rule; the causal limit stays on top (an invisible column is -inf whatever the mask says, and
//                    its mask value is not read), so a mask only takes columns away.  Columns at or beyond T + window_len are never
//                    read.  The unmasked instantiations take MqArgs alone and are the code they were
//   LEN              the window length and the compressed tokens in use come from two device ints (either may be NULL), read once per
//                    workgroup with scalar loads at the top: w_len = clamp(w_len + *w_extra, n_q, w_cap); EXT: the blocks in use ntb =
//                    clamp(*t_dev / 64, T_base / 64, T / 64), T being the capacity the grid and the slabs are sized for.  A run ends at
//                    ntb, one beyond it reads nothing and leaves slabs of weight zero, and the window's mask columns start at 64 ntb.
//                    The instantiations without LEN are the code they were (multi_query_append_lengths_kernel: the append with the same w_len)
// multi_segment_decode_kernel the compressed runs alone, for up to 1024 rows in chunks of 64 (blockIdx.z): no window, no causal limit, no LEN
// window_keep_kernel          rows row0 + i <- row0 + keep[seq][i] of both windows of every head (accept(keep=) after a draft tree): the source
//                             rows go through LDS and a barrier before the first store, so any order and duplicates are safe
// shared_merge_kernel         (expand_block.h) folds a row's slabs -- compressed runs first, then window chunks -- into out and lse
// Products are fp16 x fp16, exact in fp32; sums are fp32.  No inline assembly.

#include "expand_block.h"

namespace mustafar_shared {
namespace {

typedef const __attribute__((address_space(4))) uint64_t* cu64_p;
constexpr int kMaxExtents = 512;    // entries of the device tables
constexpr int kMaxWindow = 1024;    // rows of a window buffer

// ---- the phases of a block, as shared_segment_decode_kernel runs them.  s_img: halfs of max(64 (D + 8), D kRowPad); s_xe: 16 RT rows of kRowPad halfs; s_alpha: 16 RT floats.

// K expand: lane = token, wave w takes the D / 4 channel tiles [w D / 4, (w + 1) D / 4) -> img[token][channel], rows of D + 8 halfs
template <int D>
__device__ __forceinline__ void expand_keys(const TileMeta& km, uint32_t k0, const uint16_t* sb, h16* s_img, int lane, int wave)
{
    constexpr int KROW = D + 8;
    uint32_t pk[D / 8];   // D / 4 halfs
#pragma unroll
    for (int j = 0; j < D / 4; j += 2) {
        const uint32_t lo = tile_element<D>(km, j, k0, sb, lane);
        const uint32_t hi = tile_element<D>(km, j + 1, k0, sb, lane);
        pk[j >> 1] = lo | (hi << 16);
    }
    uint4* dst = reinterpret_cast<uint4*>(s_img + lane * KROW + wave * (D / 4));
#pragma unroll
    for (int p = 0; p < D / 32; p++) dst[p] = make_uint4(pk[4 * p], pk[4 * p + 1], pk[4 * p + 2], pk[4 * p + 3]);
}

// scores: wave w = tokens [16 w, 16 w + 16) of the key image, every row tile: x -> xe[row][token]
template <int D, int RT>
__device__ __forceinline__ void score_tiles(const h16x8 (&qf)[RT][D / 32], const h16* s_img, h16* s_xe, float inv_sqrt_d, int wave, int l15,
                                            int l4)
{
    constexpr int KS = D / 32, KROW = D + 8;
    h16x8 bf[KS];
#pragma unroll
    for (int s = 0; s < KS; s++) bf[s] = *reinterpret_cast<const h16x8*>(s_img + (wave * 16 + l15) * KROW + 32 * s + 8 * l4);
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; s++) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(qf[rt][s], bf[s], acc, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; i++)   // C: column = token l & 15, row = 4 (l >> 4) + i
            s_xe[(rt * 16 + 4 * l4 + i) * kRowPad + wave * 16 + l15] = scaled(acc[i], inv_sqrt_d);
    }
}

// V expand: lane = channel, wave w takes tokens [16 w, 16 w + 16) (both 64-channel halves at D = 128) -> img[channel][token], rows of kRowPad
template <int D>
__device__ __forceinline__ void expand_values(const TileMeta& vm, uint32_t v0, const uint16_t* sb, h16* s_img, int lane, int wave)
{
#pragma unroll
    for (int hh = 0; hh < D / 64; hh++) {
        uint32_t pk[8];
#pragma unroll
        for (int j = 0; j < 16; j += 2) {
            const uint32_t lo = tile_element<D>(vm, hh * 16 + j, v0, sb, lane);
            const uint32_t hi = tile_element<D>(vm, hh * 16 + j + 1, v0, sb, lane);
            pk[j >> 1] = lo | (hi << 16);
        }
        uint4* dst = reinterpret_cast<uint4*>(s_img + (hh * 64 + lane) * kRowPad + wave * 16);
        dst[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        dst[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
    }
}

// Online softmax step: thread = (row tid >> 2, 16 tokens), four lanes per row: the step of headdim64.hip's softmax_step, the row's max and
// sum folded over the quad.  Rows of zero queries (at or beyond R) go through it like any other: x = 0, finite everywhere.
// LIMIT: columns at or beyond `visible` (0..64, the row's own) count as x = -inf, e = 0; a row that sees no column at all, in this block and
// before it, stays at M = -inf, L = 0 with alpha = 1 (exp(-inf - -inf) would be NaN).
// MASK: x' = max(fp16(x + m), finfo(fp16).min) on the thread's 16 columns first -- packed fp16 additions, each rounded once; m = -inf gives
// finfo.min -- and the limit on top of it.
struct MaskRegs {
    h16x8 a, b;   // the mask values of the thread's 16 columns
};
template <int RT, bool LIMIT, bool MASK = false>
__device__ __forceinline__ void softmax_rows(h16* s_xe, float* s_alpha, float& M, float& L, int srow, int sq, int visible,
                                             const MaskRegs& mk = MaskRegs{})
{
    if (srow < RT * 16) {
        h16x8* px = reinterpret_cast<h16x8*>(s_xe + srow * kRowPad + sq * 16);
        h16x8 xa = px[0], xb = px[1];
        if constexpr (MASK) {
            const h16 lowest = (h16)-65504.f;
            const h16x8 lo = h16x8{lowest, lowest, lowest, lowest, lowest, lowest, lowest, lowest};
            xa = __builtin_elementwise_max(xa + mk.a, lo);
            xb = __builtin_elementwise_max(xb + mk.b, lo);
        }
        float x[16];
#pragma unroll
        for (int j = 0; j < 8; j++) { x[j] = (float)xa[j]; x[8 + j] = (float)xb[j]; }
        if constexpr (LIMIT) {
#pragma unroll
            for (int j = 0; j < 16; j++) x[j] = sq * 16 + j < visible ? x[j] : -INFINITY;
        }
        float mx = x[0];
#pragma unroll
        for (int j = 1; j < 16; j++) mx = fmaxf(mx, x[j]);
        const float mn = fmaxf(M, quad_max(mx));
        float alpha = __expf(M - mn);                 // (exp(-inf) = 0 before the first block)
        float ms = mn;
        if constexpr (LIMIT) {
            if (mn == -INFINITY) { alpha = 1.f; ms = 0.f; }   // nothing seen yet: every e = exp(-inf - 0) = 0
        }
        h16x8 ea, eb;
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const h16 e = (h16)__expf(x[j] - ms);
            sum += (float)e;
            if (j < 8) ea[j] = e; else eb[j - 8] = e;
        }
        L = L * alpha + quad_sum(sum);
        M = mn;
        px[0] = ea;
        px[1] = eb;
        if (sq == 0) s_alpha[srow] = alpha;
    }
}

// out: wave w = channel tiles [w D / 64, (w + 1) D / 64) of the value image, every row tile: o = o * alpha + e . V
template <int D, int RT>
__device__ __forceinline__ void accumulate_out(f32x4 (&o)[RT][D / 64], const h16* s_img, const h16* s_xe, const float* s_alpha, int wave,
                                               int l15, int l4)
{
    constexpr int CT = D / 64;
    h16x8 vf[CT][2];
#pragma unroll
    for (int c = 0; c < CT; c++)
#pragma unroll
        for (int s = 0; s < 2; s++)
            vf[c][s] = *reinterpret_cast<const h16x8*>(s_img + ((wave * CT + c) * 16 + l15) * kRowPad + 32 * s + 8 * l4);
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        const float4 al = *reinterpret_cast<const float4*>(s_alpha + rt * 16 + 4 * l4);
        h16x8 ef[2];
#pragma unroll
        for (int s = 0; s < 2; s++) ef[s] = *reinterpret_cast<const h16x8*>(s_xe + (rt * 16 + l15) * kRowPad + 32 * s + 8 * l4);
#pragma unroll
        for (int c = 0; c < CT; c++) {
            f32x4 acc = o[rt][c];
            acc[0] *= al.x; acc[1] *= al.y; acc[2] *= al.z; acc[3] *= al.w;
#pragma unroll
            for (int s = 0; s < 2; s++) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ef[s], vf[c][s], acc, 0, 0, 0);
            o[rt][c] = acc;
        }
    }
}

// The workgroup's slab of every row: slab = index of the workgroup's first row among all rows of the launch
template <int D, int RT>
__device__ __forceinline__ void write_slabs(const f32x4 (&o)[RT][D / 64], float M, float L, float* ws_o, float* ws_ml, int64_t slab, int R,
                                            int wave, int l15, int l4, int srow, int sq)
{
    constexpr int CT = D / 64;
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int c = 0; c < CT; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int r = rt * 16 + 4 * l4 + i;
                if (r < R) ws_o[(slab + r) * D + (wave * CT + c) * 16 + l15] = o[rt][c][i];
            }
    if (srow < R && sq == 0) { ws_ml[2 * (slab + srow)] = M; ws_ml[2 * (slab + srow) + 1] = L; }
}

// One side of a 64-token block as the phases read it: bitmaps and offsets of its tiles, the head's stream.
struct BlockRef {
    const uint64_t* bmp;
    const uint32_t* idx;
    const uint4* nz;
};
static_assert(sizeof(mustafar_cache_view) == 64, "the first seven 8-byte words of a table entry are read (the eighth holds the flags: extents are tiles)");
// Block j (0..3) of a table entry, head kvh: every field a scalar load (the entry is wave-uniform), offsets relative to the extent.
template <int TILES>
__device__ __forceinline__ BlockRef extent_block(const mustafar_cache_view* entry, int kvh, int j)
{
    const cu64_p f = (cu64_p)reinterpret_cast<const uint64_t*>(entry);   // bmp, nz, idx, nz_offset, bmp stride, idx stride, nz stride
    const int64_t bs = f[4] ? (int64_t)f[4] : 4 * TILES, is = f[5] ? (int64_t)f[5] : 4 * TILES + 1;
    BlockRef r;
    r.bmp = reinterpret_cast<const uint64_t*>(f[0]) + kvh * bs + j * TILES;
    r.idx = reinterpret_cast<const uint32_t*>(f[2]) + kvh * is + j * TILES;
    const int64_t start = f[6] ? (int64_t)kvh * (int64_t)f[6] : (int64_t)((cu32_p)reinterpret_cast<const uint32_t*>(f[3]))[kvh];
    r.nz = reinterpret_cast<const uint4*>(f[1]) + start;
    return r;
}

struct MqArgs {
    SideArgs k, v;                       // the base views (unused when ntb == 0)
    const mustafar_cache_view* k_ext;    // DEVICE tables of the extents (EXT)
    const mustafar_cache_view* v_ext;
    const h16* q;                        // [B', R, D]
    const h16* k_win;                    // [B', w_cap, D]
    const h16* v_win;
    float* ws_o;                         // [runs + chunks, B', R, D]
    float* ws_ml;                        // [runs + chunks, B', R, 2]
    int ntb, ntb_base, bpw, runs, n_q, R, w_len, w_cap;
    float inv_sqrt_d;
};

// MASK: the kernel's argument is MqArgs followed by the mask (the unmasked instantiations keep MqArgs as it is).
struct MqMaskArgs : MqArgs {
    const h16* mask;                     // additive fp16, 2-byte aligned
    int64_t mask_batch_stride;           // halfs between the planes of two groups of `heads_per_mask` heads
    int64_t mask_row_stride;             // halfs between the rows of two query tokens (mask_rows == n_q)
    int mask_rows, heads_per_mask;
};
template <bool MASK>
struct MqKernelArgs { typedef MqArgs type; };
template <>
struct MqKernelArgs<true> { typedef MqMaskArgs type; };
// LEN: the two device lengths follow whatever the instantiation took before (either may be NULL; t_dev is read by EXT alone).
template <bool MASK>
struct MqLenArgs : MqKernelArgs<MASK>::type {
    const int32_t* w_extra;              // added to w_len, the sum clamped into [n_q, w_cap]
    const int32_t* t_dev;                // compressed tokens in use, clamped into [64 ntb_base, 64 ntb]
};
template <bool MASK, bool LEN>
struct MqKernelArgsOf { typedef typename MqKernelArgs<MASK>::type type; };
template <bool MASK>
struct MqKernelArgsOf<MASK, true> { typedef MqLenArgs<MASK> type; };
// w_len + *w_extra in [n_q, w_cap]: a bad counter gives a wrong row, never an address outside the window buffers
__device__ __forceinline__ int device_window_len(int w_len, const int32_t* w_extra, int n_q, int w_cap)
{
    if (!w_extra) return w_len;
    const int extra = min(max((int)*(cu32_p)reinterpret_cast<const uint32_t*>(w_extra), -kMaxWindow), kMaxWindow);   // (no overflow below)
    return min(max(w_len + extra, n_q), w_cap);
}

// The mask values of a thread's 16 columns, packed as they lie in memory.  The base and the strides of a mask are 2-byte aligned only:
// these are loads of 4 and 16 bytes at 2-byte alignment, which global memory serves (no 2-byte loads, which would take a register each
// until they are packed).
struct __attribute__((packed, aligned(2))) MaskPair { uint32_t v; };
struct __attribute__((packed, aligned(2))) MaskOctet { uint32_t v[4]; };
__device__ __forceinline__ MaskRegs load_mask16(const h16* p)
{
    const MaskOctet lo = *reinterpret_cast<const MaskOctet*>(p), hi = *reinterpret_cast<const MaskOctet*>(p + 8);
    MaskRegs mk;
    mk.a = __builtin_bit_cast(h16x8, lo);
    mk.b = __builtin_bit_cast(h16x8, hi);
    return mk;
}
// The first `n` (0..16) of them; the others are 0, belong to columns the row does not see, and are not read: whole pairs as 4 bytes, the
// last value of an odd n as 2 bytes.
__device__ __forceinline__ MaskRegs load_mask(const h16* p, int n)
{
    if (n == 16) return load_mask16(p);
    const uint32_t last = (n & 1) ? (uint32_t)reinterpret_cast<const uint16_t*>(p)[n - 1] : 0u;
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        w[k] = 2 * k == n - 1 ? last : 0u;
        if (2 * k + 1 < n) w[k] = reinterpret_cast<const MaskPair*>(p + 2 * k)->v;
    }
    MaskRegs mk;
    mk.a = __builtin_bit_cast(h16x8, MaskOctet{{w[0], w[1], w[2], w[3]}});
    mk.b = __builtin_bit_cast(h16x8, MaskOctet{{w[4], w[5], w[6], w[7]}});
    return mk;
}

// Block tb of one side: from the head's rows of the base view, or (EXT) from the table behind them.
template <int TILES, bool EXT>
__device__ __forceinline__ BlockRef block_of(const uint64_t* bmp_h, const uint32_t* idx_h, const uint4* nz_h, const mustafar_cache_view* ext,
                                             int ntb_base, int kvh, int tb)
{
    if constexpr (EXT) {
        if (tb >= ntb_base) {
            const int xb = tb - ntb_base;
            return extent_block<TILES>(ext + (xb >> 2), kvh, xb & 3);
        }
    }
    return BlockRef{bmp_h + (int64_t)tb * TILES, idx_h + (int64_t)tb * TILES, nz_h};
}

// A run of compressed blocks [tb0, tb1) of head bkv for the workgroup's row tiles: the compressed branch of multi_query_decode_kernel
// below, statement for statement, as a function for multi_segment_decode_kernel.  (That kernel keeps its own copy: called from there, this
// function changed 64 of its 70 instantiations by a few instructions each -- DESIGN.md 4.14 -- and they are to stay the code they were.)
// mrow (MASK): the mask row of the thread's softmax row at the thread's 16 columns of block 0; m_on: whether the thread has a softmax row.
template <int D, int RT, bool EXT, bool MASK>
__device__ __forceinline__ void compressed_run(const MqArgs& a, int bkv, int tb0, int tb1, const h16x8 (&qf)[RT][D / 32], f32x4 (&o)[RT][D / 64],
                                               float& M, float& L, const h16* mrow, bool m_on, uint4* s_stream, h16* s_img, h16* s_xe,
                                               float* s_alpha, int tid, int lane, int wave, int l15, int l4, int srow, int sq)
{
    constexpr int TILES = D;
    const uint16_t* sb = reinterpret_cast<const uint16_t*>(s_stream);
    const uint4* kz = a.k.nz + (a.k.nz_stride ? (int64_t)bkv * a.k.nz_stride : (int64_t)a.k.nz_offset[bkv]);
    const uint4* vz = a.v.nz + (a.v.nz_stride ? (int64_t)bkv * a.v.nz_stride : (int64_t)a.v.nz_offset[bkv]);
    const uint64_t* kb_h = a.k.bmp + bkv * a.k.bmp_stride;
    const uint32_t* ki_h = a.k.idx + bkv * a.k.idx_stride;
    const uint64_t* vb_h = a.v.bmp + bkv * a.v.bmp_stride;
    const uint32_t* vi_h = a.v.idx + bkv * a.v.idx_stride;

    // the tiles this wave expands: K tile wave D / 4 + lane (lanes below D / 4), V tile 64 (lane >> 4) + 16 wave + (lane & 15) (lanes below D / 4)
    const bool meta_on = lane < D / 4;
    const int k_tile = wave * (D / 4) + lane, v_tile = (lane >> 4) * 64 + wave * 16 + l15;
    BlockRef kc = block_of<TILES, EXT>(kb_h, ki_h, kz, a.k_ext, a.ntb_base, bkv, tb0);
    BlockRef vc = block_of<TILES, EXT>(vb_h, vi_h, vz, a.v_ext, a.ntb_base, bkv, tb0);
    TileMeta km = load_meta(kc.bmp, kc.idx, k_tile, meta_on);
    TileMeta vm = load_meta(vc.bmp, vc.idx, v_tile, meta_on);
    StreamRegs<TILES> kg{}, vg{};
    load_block<TILES>(kc.nz, (cu32_p)kc.idx, tid, kg);
    store_block<TILES>(kg, s_stream, tid);
    uint32_t k0 = kg.i0;
    __syncthreads();
    for (int tb = tb0; tb < tb1; tb++) {
        // requested now, used later: this block's value stream, the next block's bitmaps and offsets -- of the next block as resolved
        MaskRegs mk{};
        load_block<TILES>(vc.nz, (cu32_p)vc.idx, tid, vg);
        const int tn = min(tb + 1, tb1 - 1);
        const BlockRef kn = block_of<TILES, EXT>(kb_h, ki_h, kz, a.k_ext, a.ntb_base, bkv, tn);
        const BlockRef vn = block_of<TILES, EXT>(vb_h, vi_h, vz, a.v_ext, a.ntb_base, bkv, tn);
        const TileMeta km_next = load_meta(kn.bmp, kn.idx, k_tile, meta_on);
        const TileMeta vm_next = load_meta(vn.bmp, vn.idx, v_tile, meta_on);
        expand_keys<D>(km, k0, sb, s_img, lane, wave);
        // MASK: the 16 mask values of the softmax step, requested here: behind them lie two barriers, the scores and the value expand.
        // (Requested in front of the key expand they are live across its 16 packing registers: 7 VGPRs more, and D = 128 at two row
        // tiles drops from three waves per SIMD to two: 104 -> 130 us at n_q = 8)  tb: the global block number
        if constexpr (MASK) { if (m_on) mk = load_mask16(mrow + (int64_t)tb * 64); }
        __syncthreads();   // the key image is whole, the key stream is read
        store_block<TILES>(vg, s_stream, tid);
        score_tiles<D, RT>(qf, s_img, s_xe, a.inv_sqrt_d, wave, l15, l4);
        __syncthreads();   // x is whole, the key image is read, the value stream is staged
        if (tb + 1 < tb1) load_block<TILES>(kn.nz, (cu32_p)kn.idx, tid, kg);   // (requested now, stored behind the softmax)
        expand_values<D>(vm, vg.i0, sb, s_img, lane, wave);
        softmax_rows<RT, false, MASK>(s_xe, s_alpha, M, L, srow, sq, 64, mk);
        __syncthreads();   // e, alpha and the value image are whole, the value stream is read
        if (tb + 1 < tb1) {
            store_block<TILES>(kg, s_stream, tid);
            k0 = kg.i0;
        }
        accumulate_out<D, RT>(o, s_img, s_xe, s_alpha, wave, l15, l4);
        __syncthreads();   // the value image, e and alpha are read; the next key stream is staged
        km = km_next;
        vm = vm_next;
        kc = kn;
        vc = vn;
    }
}

template <int D, int RT, bool EXT, bool MASK, bool LEN>
__global__ __launch_bounds__(kThreads) void multi_query_decode_kernel(typename MqKernelArgsOf<MASK, LEN>::type a)
{
    constexpr int TILES = D;                 // tiles of a 64-token block on either side (D / 64 per token)
    constexpr int KS = D / 32;               // k-steps of the score product
    constexpr int CT = D / 64;               // channel tiles of 16 a wave owns in the output product
    constexpr int KROW = D + 8;              // halfs of a key image row (token-major): 144 / 272 bytes
    constexpr int IMG = (64 * KROW > D * kRowPad) ? 64 * KROW : D * kRowPad;
    __shared__ uint4 s_stream[8 * TILES];    // a block's key or value stream
    __shared__ __attribute__((aligned(16))) h16 s_img[IMG];                 // key image [token][channel], then value image [channel][token]
    __shared__ __attribute__((aligned(16))) h16 s_xe[RT * 16 * kRowPad];    // x, then e: [row][token]
    __shared__ __attribute__((aligned(16))) float s_alpha[RT * 16];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bkv = blockIdx.y, x = blockIdx.x;
    const int R = a.R;
    const int l15 = lane & 15, l4 = lane >> 4;
    const uint16_t* sb = reinterpret_cast<const uint16_t*>(s_stream);

    // LEN: the two device lengths, one wave-uniform load each, asked for here with the q fragments (used behind them: nothing waits for a
    // cold scalar load inside a step).  ntb: the blocks IN USE, which is also the column base of the mask's window part
    int w_len = a.w_len, ntb = a.ntb;
    if constexpr (LEN) {
        w_len = device_window_len(a.w_len, a.w_extra, a.n_q, a.w_cap);
        if constexpr (EXT) {
            if (a.t_dev) ntb = min(max((int)*(cu32_p)reinterpret_cast<const uint32_t*>(a.t_dev) >> 6, a.ntb_base), a.ntb);
        }
    }

    // q fragments (A operand): lane holds q[row 16 rt + (l & 15)][32 s + 8 (l >> 4) ..+8); rows at or beyond R are zero
    h16x8 qf[RT][KS];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        const int r = rt * 16 + l15;
        const bool live = r < R;
        const h16* qrow = a.q + ((int64_t)bkv * R + (live ? r : 0)) * D;
#pragma unroll
        for (int s = 0; s < KS; s++) {
            h16x8 v = *reinterpret_cast<const h16x8*>(qrow + 32 * s + 8 * l4);
            if (!live) v = h16x8{};
            qf[rt][s] = v;
        }
    }
    f32x4 o[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int c = 0; c < CT; c++) o[rt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // softmax state of row tid >> 2 (the four lanes of a quad hold the same values; rows at or beyond 16 RT do not exist)
    const int srow = tid >> 2, sq = tid & 3;
    float M = -INFINITY, L = 0.f;
    // MASK: the row of this thread's softmax row (query token srow % n_q; rows at or beyond R read the row of a token that exists), and
    // whether the thread has a softmax row at all
    const h16* mrow = nullptr;
    const bool m_on = srow < RT * 16;
    if constexpr (MASK)
        mrow = a.mask + (int64_t)(bkv / a.heads_per_mask) * a.mask_batch_stride +
               (a.mask_rows == 1 ? 0 : (int64_t)(srow % a.n_q) * a.mask_row_stride) + sq * 16;

    // LEN: a run with no block in use takes neither branch: it touches no byte of the cache -- no base loads, no nz_offset load, no table
    // resolution -- and leaves slabs of weight zero (M = -inf, L = 0, o = 0).  KEEP the `x * bpw < ntb` test: without it the loop below
    // still does not run and the slabs are the same, so no test on valid tables can tell (the surviving mutant), but the
    // prologue would resolve block tb0 through a table entry beyond the tokens in use -- which callers leave unwritten (the hook's tables
    // are zero there: a NULL view).  Only the hook's graph tests, whose unlisted entries are NULL, stand behind it
    const bool is_run = x < a.runs;
    if (is_run && (!LEN || x * a.bpw < ntb)) {
        // ---- compressed blocks [tb0, tb1) of this head (LEN: a run that straddles the blocks in use ends at them, and so does what it
        // requests ahead: tn below is bounded by tb1)
        const int tb0 = x * a.bpw, tb1 = min(ntb, tb0 + a.bpw);
        const uint4* kz = a.k.nz + (a.k.nz_stride ? (int64_t)bkv * a.k.nz_stride : (int64_t)a.k.nz_offset[bkv]);
        const uint4* vz = a.v.nz + (a.v.nz_stride ? (int64_t)bkv * a.v.nz_stride : (int64_t)a.v.nz_offset[bkv]);
        const uint64_t* kb_h = a.k.bmp + bkv * a.k.bmp_stride;
        const uint32_t* ki_h = a.k.idx + bkv * a.k.idx_stride;
        const uint64_t* vb_h = a.v.bmp + bkv * a.v.bmp_stride;
        const uint32_t* vi_h = a.v.idx + bkv * a.v.idx_stride;

        // the tiles this wave expands: K tile wave D / 4 + lane (lanes below D / 4), V tile 64 (lane >> 4) + 16 wave + (lane & 15) (lanes below D / 4)
        const bool meta_on = lane < D / 4;
        const int k_tile = wave * (D / 4) + lane, v_tile = (lane >> 4) * 64 + wave * 16 + l15;
        BlockRef kc = block_of<TILES, EXT>(kb_h, ki_h, kz, a.k_ext, a.ntb_base, bkv, tb0);
        BlockRef vc = block_of<TILES, EXT>(vb_h, vi_h, vz, a.v_ext, a.ntb_base, bkv, tb0);
        TileMeta km = load_meta(kc.bmp, kc.idx, k_tile, meta_on);
        TileMeta vm = load_meta(vc.bmp, vc.idx, v_tile, meta_on);
        StreamRegs<TILES> kg{}, vg{};
        load_block<TILES>(kc.nz, (cu32_p)kc.idx, tid, kg);
        store_block<TILES>(kg, s_stream, tid);
        uint32_t k0 = kg.i0;
        __syncthreads();
        for (int tb = tb0; tb < tb1; tb++) {
            // requested now, used later: this block's value stream, the next block's bitmaps and offsets -- of the next block as resolved
            MaskRegs mk{};
            load_block<TILES>(vc.nz, (cu32_p)vc.idx, tid, vg);
            const int tn = min(tb + 1, tb1 - 1);
            const BlockRef kn = block_of<TILES, EXT>(kb_h, ki_h, kz, a.k_ext, a.ntb_base, bkv, tn);
            const BlockRef vn = block_of<TILES, EXT>(vb_h, vi_h, vz, a.v_ext, a.ntb_base, bkv, tn);
            const TileMeta km_next = load_meta(kn.bmp, kn.idx, k_tile, meta_on);
            const TileMeta vm_next = load_meta(vn.bmp, vn.idx, v_tile, meta_on);
            expand_keys<D>(km, k0, sb, s_img, lane, wave);
            // MASK: the 16 mask values of the softmax step, requested here: behind them lie two barriers, the scores and the value expand.
            // (Requested in front of the key expand they are live across its 16 packing registers: 7 VGPRs more, and D = 128 at two row
            // tiles drops from three waves per SIMD to two: 104 -> 130 us at n_q = 8)  tb: the global block number
            if constexpr (MASK) { if (m_on) mk = load_mask16(mrow + (int64_t)tb * 64); }
            __syncthreads();   // the key image is whole, the key stream is read
            store_block<TILES>(vg, s_stream, tid);
            score_tiles<D, RT>(qf, s_img, s_xe, a.inv_sqrt_d, wave, l15, l4);
            __syncthreads();   // x is whole, the key image is read, the value stream is staged
            if (tb + 1 < tb1) load_block<TILES>(kn.nz, (cu32_p)kn.idx, tid, kg);   // (requested now, stored behind the softmax)
            expand_values<D>(vm, vg.i0, sb, s_img, lane, wave);
            softmax_rows<RT, false, MASK>(s_xe, s_alpha, M, L, srow, sq, 64, mk);
            __syncthreads();   // e, alpha and the value image are whole, the value stream is read
            if (tb + 1 < tb1) {
                store_block<TILES>(kg, s_stream, tid);
                k0 = kg.i0;
            }
            accumulate_out<D, RT>(o, s_img, s_xe, s_alpha, wave, l15, l4);
            __syncthreads();   // the value image, e and alpha are read; the next key stream is staged
            km = km_next;
            vm = vm_next;
            kc = kn;
            vc = vn;
        }
    } else if (!is_run) {
        // ---- window chunk: rows [w0, w0 + 64) of this head's dense window (a chunk beyond the window leaves its slabs at weight zero)
        const int w0 = (x - a.runs) * 64;
        if (w0 < w_len) {
            MaskRegs mk{};
            if constexpr (MASK)   // the causally visible ones of the thread's 16 columns (below): none at or beyond T + w_len
                mk = load_mask(mrow + (int64_t)ntb * 64 + w0,
                               m_on ? min(16, max(0, w_len - a.n_q + srow % a.n_q + 1 - w0 - sq * 16)) : 0);
            const h16* kw = a.k_win + (int64_t)bkv * a.w_cap * D;
            const h16* vw = a.v_win + (int64_t)bkv * a.w_cap * D;
            // value rows, requested first and held: item = (token pair u, 8-channel piece pc), 32 x D / 8 items over 256 threads
            constexpr int VI = D / 64;
            uint4 va[VI], vb[VI];
#pragma unroll
            for (int k = 0; k < VI; k++) {
                const int it = tid + kThreads * k, w = w0 + 2 * (it & 31), pc = it >> 5;
                va[k] = vb[k] = make_uint4(0u, 0u, 0u, 0u);
                if (w < w_len) va[k] = *reinterpret_cast<const uint4*>(vw + (int64_t)w * D + 8 * pc);
                if (w + 1 < w_len) vb[k] = *reinterpret_cast<const uint4*>(vw + (int64_t)(w + 1) * D + 8 * pc);
            }
            // key image: the rows as they are, 16-byte pieces; rows at or beyond w_len are zeros
#pragma unroll
            for (int k = 0; k < D / 32; k++) {
                const int p = tid + kThreads * k, t = p / (D / 8), pc = p % (D / 8);
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (w0 + t < w_len) v = *reinterpret_cast<const uint4*>(kw + (int64_t)(w0 + t) * D + 8 * pc);
                *reinterpret_cast<uint4*>(s_img + t * KROW + 8 * pc) = v;
            }
            __syncthreads();   // the key image is whole
            score_tiles<D, RT>(qf, s_img, s_xe, a.inv_sqrt_d, wave, l15, l4);
            __syncthreads();   // x is whole, the key image is read
            // value image: the transpose, two tokens of a channel per 4-byte store (the 32 lanes of a half wave: 32 consecutive banks)
#pragma unroll
            for (int k = 0; k < VI; k++) {
                const int it = tid + kThreads * k, u = it & 31, pc = it >> 5;
                uint32_t* dst = reinterpret_cast<uint32_t*>(s_img + 8 * pc * kRowPad + 2 * u);
                const auto put = [&](uint32_t a, uint32_t b, int c) {   // channels c, c + 1 of both tokens
                    dst[c * (kRowPad / 2)] = (a & 0xffffu) | (b << 16);
                    dst[(c + 1) * (kRowPad / 2)] = (a >> 16) | (b & 0xffff0000u);
                };
                put(va[k].x, vb[k].x, 0);
                put(va[k].y, vb[k].y, 2);
                put(va[k].z, vb[k].z, 4);
                put(va[k].w, vb[k].w, 6);
            }
            // the causal limit: query token j = row % n_q sees window rows [0, w_len - n_q + j], `visible` of them in this chunk
            softmax_rows<RT, true, MASK>(s_xe, s_alpha, M, L, srow, sq, w_len - a.n_q + srow % a.n_q + 1 - w0, mk);
            __syncthreads();   // e, alpha and the value image are whole
            accumulate_out<D, RT>(o, s_img, s_xe, s_alpha, wave, l15, l4);
        }
    }
    write_slabs<D, RT>(o, M, L, a.ws_o, a.ws_ml, ((int64_t)x * gridDim.y + bkv) * R, R, wave, l15, l4, srow, sq);
}

// The several-token call over compressed tokens ONLY (mustafar_decode_multi_segment): a frozen per-sequence segment has
// no window, no new rows and no causal limit among the query tokens, and no device-side lengths.  Grid (runs, B', row chunks): a workgroup
// serves local rows [64 z, 64 z + 64) of one (sequence, kv head) -- up to 1024 rows, one expansion of a block per chunk -- over one run
// of blocks.  The window fields of MqArgs are unused; MASK: columns [0, T), the row of query token (row % n_q).
template <int D, int RT, bool EXT, bool MASK>
__global__ __launch_bounds__(kThreads) void multi_segment_decode_kernel(typename MqKernelArgs<MASK>::type a)
{
    constexpr int KS = D / 32, CT = D / 64, KROW = D + 8;
    constexpr int IMG = (64 * KROW > D * kRowPad) ? 64 * KROW : D * kRowPad;
    __shared__ uint4 s_stream[8 * D];        // a block's key or value stream
    __shared__ __attribute__((aligned(16))) h16 s_img[IMG];                 // key image [token][channel], then value image [channel][token]
    __shared__ __attribute__((aligned(16))) h16 s_xe[RT * 16 * kRowPad];    // x, then e: [row][token]
    __shared__ __attribute__((aligned(16))) float s_alpha[RT * 16];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bkv = blockIdx.y, x = blockIdx.x, row0 = 64 * (int)blockIdx.z;
    const int R = a.R;
    const int l15 = lane & 15, l4 = lane >> 4;

    // q fragments (A operand) of the chunk's rows; rows at or beyond R are zero
    h16x8 qf[RT][KS];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        const int r = row0 + rt * 16 + l15;
        const bool live = r < R;
        const h16* qrow = a.q + ((int64_t)bkv * R + (live ? r : 0)) * D;
#pragma unroll
        for (int s = 0; s < KS; s++) {
            h16x8 v = *reinterpret_cast<const h16x8*>(qrow + 32 * s + 8 * l4);
            if (!live) v = h16x8{};
            qf[rt][s] = v;
        }
    }
    f32x4 o[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int c = 0; c < CT; c++) o[rt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int srow = tid >> 2, sq = tid & 3;
    float M = -INFINITY, L = 0.f;
    const h16* mrow = nullptr;
    const bool m_on = srow < RT * 16;
    if constexpr (MASK)
        mrow = a.mask + (int64_t)(bkv / a.heads_per_mask) * a.mask_batch_stride +
               (a.mask_rows == 1 ? 0 : (int64_t)((row0 + srow) % a.n_q) * a.mask_row_stride) + sq * 16;

    compressed_run<D, RT, EXT, MASK>(a, bkv, x * a.bpw, min(a.ntb, x * a.bpw + a.bpw), qf, o, M, L, mrow, m_on, s_stream, s_img, s_xe, s_alpha, tid,
                                     lane, wave, l15, l4, srow, sq);
    // (write_slabs counts rows from the chunk's first: the slab index and the row limit move by row0)
    write_slabs<D, RT>(o, M, L, a.ws_o, a.ws_ml, ((int64_t)x * gridDim.y + bkv) * R + row0, R - row0, wave, l15, l4, srow, sq);
}

// Rows [row0, row0 + n_q) of every head's K and V window <- k_new / v_new [B', n_q, D]; thread = one 16-byte piece, blockIdx.y = side.
__global__ __launch_bounds__(kThreads) void multi_query_append_kernel(const uint4* __restrict__ k_new, const uint4* __restrict__ v_new,
                                                                      uint4* __restrict__ k_win, uint4* __restrict__ v_win, int n_q, int row0,
                                                                      int w_cap, int D8, int total)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int pc = i % D8, j = (i / D8) % n_q, b = i / (D8 * n_q);
    const uint4* src = blockIdx.y ? v_new : k_new;
    uint4* dst = blockIdx.y ? v_win : k_win;
    dst[((int64_t)b * w_cap + row0 + j) * D8 + pc] = src[i];
}

// The same with the window length on the device: row0 = clamp(w_len + *w_extra, n_q, w_cap) - n_q, inside the buffer whatever the counter holds.
__global__ __launch_bounds__(kThreads) void multi_query_append_lengths_kernel(const uint4* __restrict__ k_new, const uint4* __restrict__ v_new,
                                                                              uint4* __restrict__ k_win, uint4* __restrict__ v_win, int n_q,
                                                                              int w_len, const int32_t* __restrict__ w_extra, int w_cap, int D8,
                                                                              int total)
{
    const int row0 = device_window_len(w_len, w_extra, n_q, w_cap) - n_q;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int pc = i % D8, j = (i / D8) % n_q, b = i / (D8 * n_q);
    const uint4* src = blockIdx.y ? v_new : k_new;
    uint4* dst = blockIdx.y ? v_win : k_win;
    dst[((int64_t)b * w_cap + row0 + j) * D8 + pc] = src[i];
}

// Rows [row0, row0 + n_keep) of one head's K or V window <- rows row0 + keep[seq][i], keep clamped to [0, n_rows): grid (B', 2), thread =
// 16-byte pieces.  Every source row is in LDS before the first store (the barrier), so the index order and duplicates do not matter.
template <int D>
__global__ __launch_bounds__(kThreads) void window_keep_kernel(uint4* __restrict__ k_win, uint4* __restrict__ v_win,
                                                               const int32_t* __restrict__ keep, int heads_per_seq, int w_cap, int row0,
                                                               int n_rows, int n_keep)
{
    constexpr int D8 = D / 8;
    __shared__ uint4 s_rows[64 * D8];
    const int b = blockIdx.x;
    uint4* win = (blockIdx.y ? v_win : k_win) + (int64_t)b * w_cap * D8;
    const int32_t* idx = keep + (int64_t)(b / heads_per_seq) * n_keep;
    const int total = n_keep * D8;   // at most 64 D8
    for (int p = threadIdx.x; p < total; p += kThreads) {
        const int i = p / D8, pc = p % D8;
        const int src = min(max(idx[i], 0), n_rows - 1);
        s_rows[p] = win[(int64_t)(row0 + src) * D8 + pc];
    }
    __syncthreads();   // every source row is read
    for (int p = threadIdx.x; p < total; p += kThreads) win[(int64_t)row0 * D8 + p] = s_rows[p];
}

bool mq_shape_ok(int T, int window_capacity, int Bp, int groups, int n_q, int head_dim)
{
    if (n_q < 1 || groups < 1 || groups > 8 || (int64_t)n_q * groups > kMaxRows || Bp < 1 || Bp > 65535 || T < 0 || (T & 63)) return false;
    if (window_capacity < n_q || window_capacity > kMaxWindow) return false;
    return head_dim == 64 || head_dim == 128;
}

template <int D, bool EXT, bool MASK, bool LEN>
void mq_launch(hipStream_t st, const typename MqKernelArgsOf<MASK, LEN>::type& a, const dim3 grid)
{
    switch ((a.R + 15) / 16) {
        case 1: multi_query_decode_kernel<D, 1, EXT, MASK, LEN><<<grid, kThreads, 0, st>>>(a); break;
        case 2: multi_query_decode_kernel<D, 2, EXT, MASK, LEN><<<grid, kThreads, 0, st>>>(a); break;
        case 3: multi_query_decode_kernel<D, 3, EXT, MASK, LEN><<<grid, kThreads, 0, st>>>(a); break;
        default: multi_query_decode_kernel<D, 4, EXT, MASK, LEN><<<grid, kThreads, 0, st>>>(a); break;
    }
}
template <bool MASK, bool LEN>
void mq_launch_any(hipStream_t st, const typename MqKernelArgsOf<MASK, LEN>::type& a, const dim3 grid, int head_dim, bool ext)
{
    if (head_dim == 64) { if (ext) mq_launch<64, true, MASK, LEN>(st, a, grid); else mq_launch<64, false, MASK, LEN>(st, a, grid); }
    else { if (ext) mq_launch<128, true, MASK, LEN>(st, a, grid); else mq_launch<128, false, MASK, LEN>(st, a, grid); }
}
// The instantiation a call takes: MqArgs alone (the launch of ABI 112), + the mask (ABI 114), + the device lengths (ABI 115)
void mq_launch_call(hipStream_t st, const MqLenArgs<true>& a, const dim3 grid, int head_dim, bool ext)
{
    const bool len = a.w_extra || a.t_dev;
    if (a.mask) {
        if (len) mq_launch_any<true, true>(st, a, grid, head_dim, ext);
        else mq_launch_any<true, false>(st, a, grid, head_dim, ext);
    } else if (len) {
        MqLenArgs<false> u{};
        static_cast<MqArgs&>(u) = a;
        u.w_extra = a.w_extra;
        u.t_dev = a.t_dev;
        mq_launch_any<false, true>(st, u, grid, head_dim, ext);
    } else {
        mq_launch_any<false, false>(st, a, grid, head_dim, ext);
    }
}

// ---- the several-token call over a frozen per-sequence segment (mustafar_decode_multi_segment)
bool ms_shape_ok(int T, int Bp, int groups, int n_q, int head_dim)
{
    if (n_q < 1 || n_q > kMaxRowsMulti || groups < 1 || groups > 8 || n_q * groups > kMaxRowsMulti || Bp < 1 || Bp > 65535) return false;
    if (T <= 0 || (T & 63)) return false;
    return head_dim == 64 || head_dim == 128;
}
template <int D, bool EXT, bool MASK>
void ms_launch(hipStream_t st, const typename MqKernelArgs<MASK>::type& a, const dim3 grid)
{
    switch (grid.z > 1 ? 4 : (a.R + 15) / 16) {   // several chunks: every chunk at four row tiles, the last one's spare rows are zero queries
        case 1: multi_segment_decode_kernel<D, 1, EXT, MASK><<<grid, kThreads, 0, st>>>(a); break;
        case 2: multi_segment_decode_kernel<D, 2, EXT, MASK><<<grid, kThreads, 0, st>>>(a); break;
        case 3: multi_segment_decode_kernel<D, 3, EXT, MASK><<<grid, kThreads, 0, st>>>(a); break;
        default: multi_segment_decode_kernel<D, 4, EXT, MASK><<<grid, kThreads, 0, st>>>(a); break;
    }
}
template <bool MASK>
void ms_launch_any(hipStream_t st, const typename MqKernelArgs<MASK>::type& a, const dim3 grid, int head_dim, bool ext)
{
    if (head_dim == 64) { if (ext) ms_launch<64, true, MASK>(st, a, grid); else ms_launch<64, false, MASK>(st, a, grid); }
    else { if (ext) ms_launch<128, true, MASK>(st, a, grid); else ms_launch<128, false, MASK>(st, a, grid); }
}

}  // namespace
}  // namespace mustafar_shared

extern "C" int64_t mustafar_decode_multi_segment_workspace_bytes(int T, int Bp, int num_key_value_groups, int n_q, int head_dim)
{
    using namespace mustafar_shared;
    if (!ms_shape_ok(T, Bp, num_key_value_groups, n_q, head_dim)) return 0;
    const int R = n_q * num_key_value_groups, ntb = T / 64, bpw = blocks_per_run(R < kMaxRows ? R : kMaxRows, head_dim);
    return (int64_t)((ntb + bpw - 1) / bpw) * Bp * R * (head_dim + 2) * (int64_t)sizeof(float);
}

extern "C" int mustafar_decode_multi_segment(void* stream, const mustafar_cache_view* k_base, const mustafar_cache_view* v_base, int T_base,
                                             const mustafar_cache_view* k_extents, const mustafar_cache_view* v_extents, int T, int Bp,
                                             int num_key_value_groups, int n_q, const void* q, void* out, float* lse, void* workspace,
                                             float sqrt_d, int head_dim, const void* mask, int64_t mask_batch_stride, int64_t mask_row_stride,
                                             int mask_rows, int heads_per_mask)
{
    using namespace mustafar_shared;
    if (!ms_shape_ok(T, Bp, num_key_value_groups, n_q, head_dim) || !(sqrt_d > 0.f)) return MUSTAFAR_EINVAL;
    if (T_base <= 0 || T_base > T || (T_base & 63)) return MUSTAFAR_EINVAL;
    if (T > T_base && ((T_base & 255) || ((T - T_base) & 255) || (T - T_base) / 256 > kMaxExtents || !k_extents || !v_extents))
        return MUSTAFAR_EINVAL;
    if (!q || !out || !workspace || !lse || !aligned16(q) || !aligned16(out) || !aligned16(workspace) || ((uintptr_t)lse & 3))
        return MUSTAFAR_EINVAL;
    if (mask) {   // (a NULL mask: the other four arguments are not looked at)
        if (((uintptr_t)mask & 1) || (mask_rows != 1 && mask_rows != n_q) || heads_per_mask < 1 || heads_per_mask > Bp || Bp % heads_per_mask)
            return MUSTAFAR_EINVAL;
        if (mask_batch_stride < 0 || mask_row_stride < 0 || (mask_rows > 1 && mask_row_stride < T) ||
            (Bp / heads_per_mask > 1 && mask_batch_stride < T))
            return MUSTAFAR_EINVAL;
    }
    MqMaskArgs a{};
    if (!side_of(k_base, T_base, Bp, head_dim, &a.k) || !side_of(v_base, T_base, Bp, head_dim, &a.v)) return MUSTAFAR_EINVAL;
    const int R = n_q * num_key_value_groups, ntb = T / 64, bpw = blocks_per_run(R < kMaxRows ? R : kMaxRows, head_dim);
    const int runs = (ntb + bpw - 1) / bpw;
    const bool ext = T > T_base;
    a.k_ext = ext ? k_extents : nullptr;
    a.v_ext = ext ? v_extents : nullptr;
    a.q = static_cast<const h16*>(q);
    a.ws_o = static_cast<float*>(workspace);
    a.ws_ml = a.ws_o + (int64_t)runs * Bp * R * head_dim;
    a.ntb = ntb; a.ntb_base = T_base / 64; a.bpw = bpw; a.runs = runs; a.n_q = n_q; a.R = R;
    a.inv_sqrt_d = (float)(1.0 / (double)sqrt_d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(runs, Bp, (R + kMaxRows - 1) / kMaxRows);
    if (mask) {
        a.mask = static_cast<const h16*>(mask);
        a.mask_batch_stride = mask_batch_stride;
        a.mask_row_stride = mask_row_stride;
        a.mask_rows = mask_rows;
        a.heads_per_mask = heads_per_mask;
        ms_launch_any<true>(st, a, grid, head_dim, ext);
    } else {
        ms_launch_any<false>(st, a, grid, head_dim, ext);
    }
    // the fold of every row's slabs: (kv_heads, G, R) = (B', R, R) addresses row bkv * R + r of out / lse and of every slab
    if (head_dim == 64) shared_merge_kernel<64><<<Bp * R, kThreads, 0, st>>>(a.ws_o, a.ws_ml, runs, Bp, R, R, static_cast<h16*>(out), lse);
    else shared_merge_kernel<128><<<Bp * R, kThreads, 0, st>>>(a.ws_o, a.ws_ml, runs, Bp, R, R, static_cast<h16*>(out), lse);
    return (int)hipGetLastError();
}

extern "C" int64_t mustafar_decode_multi_query_workspace_bytes(int T, int window_capacity, int Bp, int num_key_value_groups, int n_q, int head_dim)
{
    using namespace mustafar_shared;
    if (!mq_shape_ok(T, window_capacity, Bp, num_key_value_groups, n_q, head_dim)) return 0;
    const int R = n_q * num_key_value_groups, ntb = T / 64, bpw = blocks_per_run(R, head_dim);
    return (int64_t)((ntb + bpw - 1) / bpw + (window_capacity + 63) / 64) * Bp * R * (head_dim + 2) * (int64_t)sizeof(float);
}

extern "C" int mustafar_decode_multi_query(void* stream, const mustafar_cache_view* k_base, const mustafar_cache_view* v_base, int T_base,
                                           const mustafar_cache_view* k_extents, const mustafar_cache_view* v_extents, int T, int Bp,
                                           int num_key_value_groups, int n_q, const void* q, void* k_window, void* v_window, const void* k_new,
                                           const void* v_new, int window_len, int window_capacity, void* out, float* lse, void* workspace,
                                           float sqrt_d, int head_dim)
{
    return mustafar_decode_multi_query_masked(stream, k_base, v_base, T_base, k_extents, v_extents, T, Bp, num_key_value_groups, n_q, q, k_window,
                                              v_window, k_new, v_new, window_len, window_capacity, out, lse, workspace, sqrt_d, head_dim, nullptr,
                                              0, 0, 1, 1);
}

extern "C" int mustafar_decode_multi_query_masked(void* stream, const mustafar_cache_view* k_base, const mustafar_cache_view* v_base, int T_base,
                                                  const mustafar_cache_view* k_extents, const mustafar_cache_view* v_extents, int T, int Bp,
                                                  int num_key_value_groups, int n_q, const void* q, void* k_window, void* v_window,
                                                  const void* k_new, const void* v_new, int window_len, int window_capacity, void* out,
                                                  float* lse, void* workspace, float sqrt_d, int head_dim, const void* mask,
                                                  int64_t mask_batch_stride, int64_t mask_row_stride, int mask_rows, int heads_per_mask)
{
    return mustafar_decode_multi_query_lengths(stream, k_base, v_base, T_base, k_extents, v_extents, T, Bp, num_key_value_groups, n_q, q, k_window,
                                               v_window, k_new, v_new, window_len, window_capacity, out, lse, workspace, sqrt_d, head_dim, mask,
                                               mask_batch_stride, mask_row_stride, mask_rows, heads_per_mask, nullptr, nullptr);
}

extern "C" int mustafar_decode_multi_query_lengths(void* stream, const mustafar_cache_view* k_base, const mustafar_cache_view* v_base, int T_base,
                                                   const mustafar_cache_view* k_extents, const mustafar_cache_view* v_extents, int T, int Bp,
                                                   int num_key_value_groups, int n_q, const void* q, void* k_window, void* v_window,
                                                   const void* k_new, const void* v_new, int window_len, int window_capacity, void* out,
                                                   float* lse, void* workspace, float sqrt_d, int head_dim, const void* mask,
                                                   int64_t mask_batch_stride, int64_t mask_row_stride, int mask_rows, int heads_per_mask,
                                                   const int32_t* window_len_extra, const int32_t* T_device)
{
    using namespace mustafar_shared;
    if (!mq_shape_ok(T, window_capacity, Bp, num_key_value_groups, n_q, head_dim) || !(sqrt_d > 0.f)) return MUSTAFAR_EINVAL;
    if (window_len < n_q || window_len > window_capacity || (k_new == nullptr) != (v_new == nullptr)) return MUSTAFAR_EINVAL;
    if (T_base < 0 || T_base > T || (T_base & 63) || (T > 0 && T_base == 0)) return MUSTAFAR_EINVAL;
    if (T > T_base && ((T_base & 255) || ((T - T_base) & 255) || (T - T_base) / 256 > kMaxExtents || !k_extents || !v_extents))
        return MUSTAFAR_EINVAL;
    if (!q || !out || !k_window || !v_window || !workspace || !lse || !aligned16(q) || !aligned16(out) || !aligned16(k_window) ||
        !aligned16(v_window) || !aligned16(workspace) || !aligned16(k_new) || !aligned16(v_new) || ((uintptr_t)lse & 3))
        return MUSTAFAR_EINVAL;
    // device lengths: T is a capacity to grow into (T_device), and a mask row reaches as far as the lengths can (either pointer)
    const bool len = window_len_extra || T_device;
    if (((uintptr_t)window_len_extra & 3) || ((uintptr_t)T_device & 3) || (T_device && (T == T_base || !k_extents || !v_extents)))
        return MUSTAFAR_EINVAL;
    if (mask) {   // (a NULL mask: the other four arguments are not looked at)
        const int64_t columns = (int64_t)T + (len ? window_capacity : window_len);
        if (((uintptr_t)mask & 1) || (mask_rows != 1 && mask_rows != n_q) || heads_per_mask < 1 || heads_per_mask > Bp || Bp % heads_per_mask)
            return MUSTAFAR_EINVAL;
        if (mask_batch_stride < 0 || mask_row_stride < 0 || (mask_rows > 1 && mask_row_stride < columns) ||
            (Bp / heads_per_mask > 1 && mask_batch_stride < columns))
            return MUSTAFAR_EINVAL;
    }
    MqLenArgs<true> a{};
    if (T_base && (!side_of(k_base, T_base, Bp, head_dim, &a.k) || !side_of(v_base, T_base, Bp, head_dim, &a.v))) return MUSTAFAR_EINVAL;
    const int R = n_q * num_key_value_groups, ntb = T / 64, bpw = blocks_per_run(R, head_dim);
    const int runs = (ntb + bpw - 1) / bpw, slabs = runs + (window_capacity + 63) / 64;
    const bool ext = T > T_base;
    a.k_ext = ext ? k_extents : nullptr;
    a.v_ext = ext ? v_extents : nullptr;
    a.q = static_cast<const h16*>(q);
    a.k_win = static_cast<const h16*>(k_window);
    a.v_win = static_cast<const h16*>(v_window);
    a.ws_o = static_cast<float*>(workspace);
    a.ws_ml = a.ws_o + (int64_t)slabs * Bp * R * head_dim;
    a.ntb = ntb; a.ntb_base = T_base / 64; a.bpw = bpw; a.runs = runs; a.n_q = n_q; a.R = R; a.w_len = window_len; a.w_cap = window_capacity;
    a.inv_sqrt_d = (float)(1.0 / (double)sqrt_d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (k_new) {
        const int D8 = head_dim / 8, total = Bp * n_q * D8;
        const dim3 agrid((total + kThreads - 1) / kThreads, 2);
        if (window_len_extra)
            multi_query_append_lengths_kernel<<<agrid, kThreads, 0, st>>>(
                static_cast<const uint4*>(k_new), static_cast<const uint4*>(v_new), static_cast<uint4*>(k_window), static_cast<uint4*>(v_window),
                n_q, window_len, window_len_extra, window_capacity, D8, total);
        else
            multi_query_append_kernel<<<agrid, kThreads, 0, st>>>(
                static_cast<const uint4*>(k_new), static_cast<const uint4*>(v_new), static_cast<uint4*>(k_window), static_cast<uint4*>(v_window),
                n_q, window_len - n_q, window_capacity, D8, total);
    }
    const dim3 grid(slabs, Bp);
    if (mask) {
        a.mask = static_cast<const h16*>(mask);
        a.mask_batch_stride = mask_batch_stride;
        a.mask_row_stride = mask_row_stride;
        a.mask_rows = mask_rows;
        a.heads_per_mask = heads_per_mask;
    }
    a.w_extra = window_len_extra;
    a.t_dev = T_device;
    mq_launch_call(st, a, grid, head_dim, ext);
    // the fold of every row's slabs: (kv_heads, G, R) = (B', R, R) addresses row bkv * R + r of out / lse and of every slab
    if (head_dim == 64) shared_merge_kernel<64><<<Bp * R, kThreads, 0, st>>>(a.ws_o, a.ws_ml, slabs, Bp, R, R, static_cast<h16*>(out), lse);
    else shared_merge_kernel<128><<<Bp * R, kThreads, 0, st>>>(a.ws_o, a.ws_ml, slabs, Bp, R, R, static_cast<h16*>(out), lse);
    return (int)hipGetLastError();
}

extern "C" int mustafar_window_keep_rows(void* stream, void* k_window, void* v_window, int Bp, int heads_per_seq, int window_capacity,
                                         int head_dim, int row0, int n_rows, const int32_t* keep, int n_keep)
{
    using namespace mustafar_shared;
    if ((head_dim != 64 && head_dim != 128) || Bp < 1 || Bp > 65535 || heads_per_seq < 1 || Bp % heads_per_seq) return MUSTAFAR_EINVAL;
    if (n_rows < 1 || n_rows > 64 || n_keep < 1 || n_keep > n_rows || window_capacity > kMaxWindow || row0 < 0 ||
        (int64_t)row0 + n_rows > window_capacity)
        return MUSTAFAR_EINVAL;
    if (!k_window || !v_window || !aligned16(k_window) || !aligned16(v_window) || !keep || ((uintptr_t)keep & 3)) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(Bp, 2);
    if (head_dim == 64)
        window_keep_kernel<64><<<grid, kThreads, 0, st>>>(static_cast<uint4*>(k_window), static_cast<uint4*>(v_window), keep, heads_per_seq,
                                                          window_capacity, row0, n_rows, n_keep);
    else
        window_keep_kernel<128><<<grid, kThreads, 0, st>>>(static_cast<uint4*>(k_window), static_cast<uint4*>(v_window), keep, heads_per_seq,
                                                           window_capacity, row0, n_rows, n_keep);
    return (int)hipGetLastError();
}
