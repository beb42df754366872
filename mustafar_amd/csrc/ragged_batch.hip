// ragged_batch.hip -- one several-token decode call over a RAGGED batch: n_seqs sequences, each with a compressed cache, a dense window and
// lengths of its own, found by the workgroup in a DEVICE table of mustafar_sequence.  The C ABI entry points mustafar_ragged_set_sequences,
// mustafar_decode_ragged and mustafar_decode_ragged_workspace_bytes (include/mustafar_hip.h), for gfx950.
//
// mustafar_decode_multi_query takes one rectangle: every sequence at one compressed length T, one window length, one cache object of
// batch x kv_heads heads.  Here the workgroup of (sequence s, kv head h) loads entry s of the table at its top -- two base views, two extent
// tables, two windows, four ints, all wave-uniform loads -- and from there runs the phases of multi_query_decode_kernel<D, RT, EXT = true>.
// The grid and the slabs are sized for the caller's T_max and window_capacity_max; a workgroup beyond its own sequence's lengths ends at once.
//
// ragged_set_kernel      writes table entries from kernel arguments (up to 16 entries per launch): no host-to-device copy
// ragged_append_kernel   copies the n_q new K / V rows of sequence s to rows [w_len_s - n_q, w_len_s) of its own windows
// ragged_decode_kernel   grid (runs(T_max) + ceil(window_capacity_max / 64), n_seqs * kv_heads), 256 threads.  The phase functions below are
//                        copies of those in multi_query.hip's anonymous namespace (that file stays the code it is; multi_segment_decode_kernel
//                        keeps its own copy of the run for the same reason): the same statements in the same order, hence the same bits
//   lengths              every length is clamped as it is loaded (sequence_lengths): a stale or wrong entry gives a wrong row, never an
//                        address outside a window.  An empty slot (window_len <= 0) has no block and no window row in use
//   dead workgroups      a run with no block in use for its sequence, a window chunk at or beyond its sequence's window and every
//                        workgroup of an empty slot return behind the length loads: no byte of any cache or window is touched, no table
//                        entry of the extents is resolved (the `x * bpw < ntb` guard multi_query.hip documents), no slab is written
// ragged_merge_kernel    shared_merge_kernel's fold in the SEQUENCE'S OWN slab numbering: slab x' of [0, runs_s + chunks_s) is physical slab
//                        x' for a run and runs(T_max) + (x' - runs_s) for a window chunk; dead slabs are neither read nor counted.  The phase
//                        a slab is summed in, and so every fp32 sum, is what mustafar_decode_multi_query on that sequence alone produces:
//                        the result does not depend on the batch.  A row with no slab (an empty slot) gets out = 0, lse = -inf
// Products are fp16 x fp16, exact in fp32; sums are fp32.  No inline assembly.

#include <string.h>

#include "expand_block.h"

namespace mustafar_shared {
namespace {

typedef const __attribute__((address_space(4))) uint64_t* cu64_p;
constexpr int kMaxExtents = 512;    // entries of the device tables
constexpr int kMaxWindow = 1024;    // rows of a window buffer
constexpr int kSeqWords = 22;       // 8-byte words of a table entry
constexpr int kSetItems = 16;       // entries one ragged_set_kernel launch carries in its arguments (2816 of the 4096 bytes a launch may take)
static_assert(sizeof(mustafar_sequence) == 8 * kSeqWords, "a table entry is 176 bytes");
static_assert(sizeof(mustafar_cache_view) == 64, "the first seven 8-byte words of a view are read");

// ---- the phases of a block: copies of multi_query.hip's (see there), without the mask

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

// LIMIT: columns at or beyond `visible` count as x = -inf, e = 0; a row that has seen no column stays at M = -inf, L = 0 with alpha = 1
template <int RT, bool LIMIT>
__device__ __forceinline__ void softmax_rows(h16* s_xe, float* s_alpha, float& M, float& L, int srow, int sq, int visible)
{
    if (srow < RT * 16) {
        h16x8* px = reinterpret_cast<h16x8*>(s_xe + srow * kRowPad + sq * 16);
        h16x8 xa = px[0], xb = px[1];
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

struct BlockRef {
    const uint64_t* bmp;
    const uint32_t* idx;
    const uint4* nz;
};
// Block j (0..3) of an extent table entry, head kvh: every field a scalar load (the entry is wave-uniform), offsets relative to the extent.
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
// Block tb of one side: from the head's rows of the base view, or from the table behind them.
template <int TILES>
__device__ __forceinline__ BlockRef block_of(const uint64_t* bmp_h, const uint32_t* idx_h, const uint4* nz_h, const mustafar_cache_view* ext,
                                             int ntb_base, int kvh, int tb)
{
    if (tb >= ntb_base) {
        const int xb = tb - ntb_base;
        return extent_block<TILES>(ext + (xb >> 2), kvh, xb & 3);
    }
    return BlockRef{bmp_h + (int64_t)tb * TILES, idx_h + (int64_t)tb * TILES, nz_h};
}

// ---- a table entry as the kernels read it.  8-byte words: k_base 0..7, v_base 8..15 (bmp, nz, idx, nz_offset, bmp stride, idx stride, nz
// stride, flags -- mustafar_ragged_set_sequences writes the two row strides RESOLVED, never 0), k_extents 16, v_extents 17, k_window 18,
// v_window 19; 4-byte words 40..43: T_base, T, window_len, window_capacity.

// The lengths of a sequence, clamped: blocks in use into [0, ntb_max], blocks from the base into [0, blocks in use], the capacity into
// [0, min(w_cap_max, 1024)], the window length into [n_q, capacity].  No table of extents: the base alone.  An empty slot
// (window_len <= 0, or no room for n_q rows): ntb = 0 and w_len = 0, nothing in use.  Wave-uniform `e`: four scalar loads.
struct SeqLens {
    int ntb, ntb_base, w_len, w_cap;
};
__device__ __forceinline__ SeqLens sequence_lengths(const mustafar_sequence* e, int ntb_max, int w_cap_max, int n_q)
{
    const cu32_p d = (cu32_p)reinterpret_cast<const uint32_t*>(e);
    const cu64_p f = (cu64_p)reinterpret_cast<const uint64_t*>(e);
    const int t_base = (int)d[40], t = (int)d[41], wl = (int)d[42], wc = (int)d[43];
    const bool tables = f[16] != 0 && f[17] != 0;
    SeqLens n;
    n.w_cap = min(max(wc, 0), min(w_cap_max, kMaxWindow));
    const bool live = wl > 0 && n.w_cap >= n_q;
    n.w_len = live ? min(max(wl, n_q), n.w_cap) : 0;
    n.ntb = live ? min(max(t >> 6, 0), ntb_max) : 0;
    n.ntb_base = min(max(t_base >> 6, 0), n.ntb);
    if (!tables) n.ntb = n.ntb_base;
    return n;
}

struct RgArgs {
    const mustafar_sequence* table;      // DEVICE, n_seqs entries
    const h16* q;                        // [n_seqs * kv_heads, R, D]
    float* ws_o;                         // [runs + chunks, n_seqs * kv_heads, R, D]
    float* ws_ml;                        // [runs + chunks, n_seqs * kv_heads, R, 2]
    int kv_heads, ntb_max, bpw, runs, n_q, R, w_cap_max;   // runs = ceil(ntb_max / bpw): the grid's
    float inv_sqrt_d;
};

template <int D, int RT>
__global__ __launch_bounds__(kThreads) void ragged_decode_kernel(RgArgs a)
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
    const int seq = __builtin_amdgcn_readfirstlane(bkv / a.kv_heads), kvh = bkv - seq * a.kv_heads;
    const int R = a.R;
    const int l15 = lane & 15, l4 = lane >> 4;
    const uint16_t* sb = reinterpret_cast<const uint16_t*>(s_stream);

    // the sequence's entry: its lengths asked for here, with the q fragments (used behind them: nothing waits for a cold scalar load inside a
    // step); the words of the views and the pointers are asked for by the branch that reads them, once, in front of its first block.
    // (Asked for up here as well, the compiler sinks them behind the dead-workgroup test again: the ISA is the same.)
    const mustafar_sequence* e = a.table + seq;
    const cu64_p f = (cu64_p)reinterpret_cast<const uint64_t*>(e);
    const SeqLens n = sequence_lengths(e, a.ntb_max, a.w_cap_max, a.n_q);
    const int ntb = n.ntb, w_len = n.w_len;

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
    // A workgroup with nothing of its sequence to serve: it has read its entry's lengths and (maybe) q, and nothing else.  KEEP the
    // `x * bpw < ntb` test: it is what keeps the prologue below from resolving block tb0 through a table entry beyond the tokens in use,
    // which callers leave unwritten (multi_query.hip documents the same guard)
    const bool is_run = x < a.runs;
    if (is_run ? x * a.bpw >= ntb : (x - a.runs) * 64 >= w_len) return;

    f32x4 o[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int c = 0; c < CT; c++) o[rt][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // softmax state of row tid >> 2 (the four lanes of a quad hold the same values; rows at or beyond 16 RT do not exist)
    const int srow = tid >> 2, sq = tid & 3;
    float M = -INFINITY, L = 0.f;

    if (is_run) {
        // ---- compressed blocks [tb0, tb1) of this head.  The head's row pointers are resolved at once; the view words die here
        const int tb0 = x * a.bpw, tb1 = min(ntb, tb0 + a.bpw);
        const int ntb_base = n.ntb_base;
        const mustafar_cache_view* k_ext = reinterpret_cast<const mustafar_cache_view*>(f[16]);
        const mustafar_cache_view* v_ext = reinterpret_cast<const mustafar_cache_view*>(f[17]);
        const uint4* kz = reinterpret_cast<const uint4*>(f[1]) +
                          (f[6] ? (int64_t)kvh * (int64_t)f[6] : (int64_t)((cu32_p)reinterpret_cast<const uint32_t*>(f[3]))[kvh]);
        const uint4* vz = reinterpret_cast<const uint4*>(f[9]) +
                          (f[14] ? (int64_t)kvh * (int64_t)f[14] : (int64_t)((cu32_p)reinterpret_cast<const uint32_t*>(f[11]))[kvh]);
        const uint64_t* kb_h = reinterpret_cast<const uint64_t*>(f[0]) + kvh * (int64_t)f[4];
        const uint32_t* ki_h = reinterpret_cast<const uint32_t*>(f[2]) + kvh * (int64_t)f[5];
        const uint64_t* vb_h = reinterpret_cast<const uint64_t*>(f[8]) + kvh * (int64_t)f[12];
        const uint32_t* vi_h = reinterpret_cast<const uint32_t*>(f[10]) + kvh * (int64_t)f[13];

        // the tiles this wave expands: K tile wave D / 4 + lane (lanes below D / 4), V tile 64 (lane >> 4) + 16 wave + (lane & 15) (lanes below D / 4)
        const bool meta_on = lane < D / 4;
        const int k_tile = wave * (D / 4) + lane, v_tile = (lane >> 4) * 64 + wave * 16 + l15;
        BlockRef kc = block_of<TILES>(kb_h, ki_h, kz, k_ext, ntb_base, kvh, tb0);
        BlockRef vc = block_of<TILES>(vb_h, vi_h, vz, v_ext, ntb_base, kvh, tb0);
        TileMeta km = load_meta(kc.bmp, kc.idx, k_tile, meta_on);
        TileMeta vm = load_meta(vc.bmp, vc.idx, v_tile, meta_on);
        StreamRegs<TILES> kg{}, vg{};
        load_block<TILES>(kc.nz, (cu32_p)kc.idx, tid, kg);
        store_block<TILES>(kg, s_stream, tid);
        uint32_t k0 = kg.i0;
        __syncthreads();
        for (int tb = tb0; tb < tb1; tb++) {
            // requested now, used later: this block's value stream, the next block's bitmaps and offsets -- of the next block as resolved
            load_block<TILES>(vc.nz, (cu32_p)vc.idx, tid, vg);
            const int tn = min(tb + 1, tb1 - 1);
            const BlockRef kn = block_of<TILES>(kb_h, ki_h, kz, k_ext, ntb_base, kvh, tn);
            const BlockRef vn = block_of<TILES>(vb_h, vi_h, vz, v_ext, ntb_base, kvh, tn);
            const TileMeta km_next = load_meta(kn.bmp, kn.idx, k_tile, meta_on);
            const TileMeta vm_next = load_meta(vn.bmp, vn.idx, v_tile, meta_on);
            expand_keys<D>(km, k0, sb, s_img, lane, wave);
            __syncthreads();   // the key image is whole, the key stream is read
            store_block<TILES>(vg, s_stream, tid);
            score_tiles<D, RT>(qf, s_img, s_xe, a.inv_sqrt_d, wave, l15, l4);
            __syncthreads();   // x is whole, the key image is read, the value stream is staged
            if (tb + 1 < tb1) load_block<TILES>(kn.nz, (cu32_p)kn.idx, tid, kg);   // (requested now, stored behind the softmax)
            expand_values<D>(vm, vg.i0, sb, s_img, lane, wave);
            softmax_rows<RT, false>(s_xe, s_alpha, M, L, srow, sq, 64);
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
    } else {
        // ---- window chunk: rows [w0, w0 + 64) of this head's own dense window, w0 < w_len <= w_cap (the clamped capacity: head kvh of
        // the sequence starts kvh * w_cap rows into its buffers)
        const int w0 = (x - a.runs) * 64;
        const h16* kw = reinterpret_cast<const h16*>(f[18]) + (int64_t)kvh * n.w_cap * D;
        const h16* vw = reinterpret_cast<const h16*>(f[19]) + (int64_t)kvh * n.w_cap * D;
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
        softmax_rows<RT, true>(s_xe, s_alpha, M, L, srow, sq, w_len - a.n_q + srow % a.n_q + 1 - w0);
        __syncthreads();   // e, alpha and the value image are whole
        accumulate_out<D, RT>(o, s_img, s_xe, s_alpha, wave, l15, l4);
    }
    write_slabs<D, RT>(o, M, L, a.ws_o, a.ws_ml, ((int64_t)x * gridDim.y + bkv) * R, R, wave, l15, l4, srow, sq);
}

// Rows [w_len_s - n_q, w_len_s) of every head's K and V window of sequence s <- k_new / v_new [n_seqs * kv_heads, n_q, D]; thread = one
// 16-byte piece, blockIdx.y = side.  The lengths are the decode kernel's (sequence_lengths): the rows lie inside the clamped capacity, and
// an empty slot gets nothing.
__global__ __launch_bounds__(kThreads) void ragged_append_kernel(const mustafar_sequence* __restrict__ table, const uint4* __restrict__ k_new,
                                                                 const uint4* __restrict__ v_new, int kv_heads, int n_q, int ntb_max,
                                                                 int w_cap_max, int D8, int total)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int pc = i % D8, j = (i / D8) % n_q, b = i / (D8 * n_q);
    const int seq = b / kv_heads, kvh = b - seq * kv_heads;
    const mustafar_sequence* e = table + seq;
    const SeqLens n = sequence_lengths(e, ntb_max, w_cap_max, n_q);
    if (n.w_len < n_q) return;   // an empty slot
    const uint4* src = blockIdx.y ? v_new : k_new;
    uint4* dst = static_cast<uint4*>(blockIdx.y ? e->v_window : e->k_window);
    dst[((int64_t)kvh * n.w_cap + n.w_len - n_q + j) * D8 + pc] = src[i];
}

// shared_merge_kernel (expand_block.h) over the sequence's own slabs: one workgroup per row (sequence, head, query token), thread = (slab
// phase, four channels).  Slab x' of [0, runs_s + chunks_s): a run at physical slab x', a window chunk at runs + (x' - runs_s).
template <int D>
__global__ __launch_bounds__(kThreads) void ragged_merge_kernel(const mustafar_sequence* __restrict__ table, const float* __restrict__ ws_o,
                                                                const float* __restrict__ ws_ml, int kv_heads, int ntb_max, int bpw, int runs,
                                                                int n_q, int R, int w_cap_max, h16* __restrict__ out, float* __restrict__ lse)
{
    constexpr int C4 = D / 4, P = kThreads / C4;
    __shared__ float4 part[P][C4];
    __shared__ float dens[P];
    const int seq = __builtin_amdgcn_readfirstlane((int)blockIdx.x / (R * kv_heads));
    const SeqLens n = sequence_lengths(table + seq, ntb_max, w_cap_max, n_q);
    const int runs_s = (n.ntb + bpw - 1) / bpw, S = runs_s + (n.w_len + 63) / 64, skip = runs - runs_s;
    const int lane = threadIdx.x & 63, c4 = threadIdx.x % C4, ph = threadIdx.x / C4;
    const int64_t stride = gridDim.x, first = blockIdx.x;
    float mx = -INFINITY;
    for (int x = lane; x < S; x += 64) mx = fmaxf(mx, ws_ml[2 * ((x < runs_s ? x : x + skip) * stride + first)]);
    const float Mx = wave_max(mx);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float den = 0.f;
#pragma unroll 4
    for (int x = ph; x < S; x += P) {
        const int64_t row = (x < runs_s ? x : x + skip) * stride + first;
        const float2 ml = *reinterpret_cast<const float2*>(ws_ml + 2 * row);
        const float4 o = *reinterpret_cast<const float4*>(ws_o + row * D + 4 * c4);
        const float w = ml.y > 0.f ? __expf(ml.x - Mx) : 0.f;
        den += w * ml.y;
        acc.x += w * o.x; acc.y += w * o.y; acc.z += w * o.z; acc.w += w * o.w;
    }
    part[ph][c4] = acc;
    if (c4 == 0) dens[ph] = den;
    __syncthreads();
    if (ph == 0) {
        float4 ov = make_float4(0.f, 0.f, 0.f, 0.f);
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < P; k++) {
            const float4 p = part[k][c4];
            ov.x += p.x; ov.y += p.y; ov.z += p.z; ov.w += p.w;
            d += dens[k];
        }
        h16* dst = out + (int64_t)blockIdx.x * D + 4 * c4;
        const bool any = d > 0.f;   // (no slab at all: an empty slot, out = 0 and lse = -inf)
        dst[0] = any ? (h16)(ov.x / d) : (h16)0.f;
        dst[1] = any ? (h16)(ov.y / d) : (h16)0.f;
        dst[2] = any ? (h16)(ov.z / d) : (h16)0.f;
        dst[3] = any ? (h16)(ov.w / d) : (h16)0.f;
        if (c4 == 0) lse[blockIdx.x] = any ? Mx + __logf(d) : -INFINITY;
    }
}

// Table entries [first, first + count) <- the entries in the kernel's arguments, 8-byte words, one per thread.
struct SetArgs {
    uint64_t w[kSetItems * kSeqWords];
};
__global__ __launch_bounds__(kThreads) void ragged_set_kernel(uint64_t* __restrict__ table_words, int count_words, SetArgs a)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < count_words) table_words[i] = a.w[i];
}

bool rg_shape_ok(int T_max, int w_cap_max, int n_seqs, int kv_heads, int groups, int n_q, int head_dim)
{
    if (n_seqs < 1 || kv_heads < 1 || kv_heads > 65535 || (int64_t)n_seqs * kv_heads > 65535) return false;
    if (n_q < 1 || groups < 1 || groups > 8 || (int64_t)n_q * groups > kMaxRows || T_max < 0 || (T_max & 63)) return false;
    if (w_cap_max < n_q || w_cap_max > kMaxWindow) return false;
    return head_dim == 64 || head_dim == 128;
}

// An item as the table holds it, or false: the per-sequence rules of mustafar_decode_multi_query.
bool sequence_entry(const mustafar_sequence& it, int kv_heads, int n_q, int head_dim, mustafar_sequence* entry)
{
    *entry = mustafar_sequence{};
    if (it.window_len == 0) return true;   // an empty slot: nothing else is looked at, the entry is all zero
    if (it.window_len < n_q || it.window_len > it.window_capacity || it.window_capacity > kMaxWindow) return false;
    if (!it.k_window || !it.v_window || !aligned16(it.k_window) || !aligned16(it.v_window)) return false;
    const int T = it.T, T_base = it.T_base;
    if (T < 0 || (T & 63) || T_base < 0 || T_base > T || (T_base & 63) || (T > 0 && T_base == 0)) return false;
    if (T > T_base && ((T_base & 255) || ((T - T_base) & 255) || (T - T_base) / 256 > kMaxExtents || !it.k_extents || !it.v_extents))
        return false;
    if (T_base) {
        SideArgs k, v;
        if (!side_of(&it.k_base, T_base, kv_heads, head_dim, &k) || !side_of(&it.v_base, T_base, kv_heads, head_dim, &v)) return false;
        entry->k_base = it.k_base;
        entry->v_base = it.v_base;
        entry->k_base.bmp_head_stride = k.bmp_stride;   // resolved: the kernels multiply, they do not test for 0
        entry->k_base.idx_head_stride = k.idx_stride;
        entry->v_base.bmp_head_stride = v.bmp_stride;
        entry->v_base.idx_head_stride = v.idx_stride;
    }
    if (T > T_base) {
        entry->k_extents = it.k_extents;
        entry->v_extents = it.v_extents;
    }
    entry->k_window = it.k_window;
    entry->v_window = it.v_window;
    entry->T_base = T_base;
    entry->T = T;
    entry->window_len = it.window_len;
    entry->window_capacity = it.window_capacity;
    return true;
}

}  // namespace
}  // namespace mustafar_shared

extern "C" int64_t mustafar_decode_ragged_workspace_bytes(int T_max, int window_capacity_max, int n_seqs, int kv_heads, int num_key_value_groups,
                                                          int n_q, int head_dim)
{
    using namespace mustafar_shared;
    if (!rg_shape_ok(T_max, window_capacity_max, n_seqs, kv_heads, num_key_value_groups, n_q, head_dim)) return 0;
    return mustafar_decode_multi_query_workspace_bytes(T_max, window_capacity_max, n_seqs * kv_heads, num_key_value_groups, n_q, head_dim);
}

extern "C" int mustafar_ragged_set_sequences(void* stream, mustafar_sequence* table, int first, int n, const mustafar_sequence* items,
                                             int kv_heads, int n_q, int head_dim)
{
    using namespace mustafar_shared;
    if (n < 1 || first < 0 || !table || ((uintptr_t)table & 7) || !items || kv_heads < 1 || kv_heads > 65535 ||
        (head_dim != 64 && head_dim != 128) || n_q < 1)
        return MUSTAFAR_EINVAL;
    mustafar_sequence entry;
    for (int i = 0; i < n; i++)   // every item is checked before anything is launched
        if (!sequence_entry(items[i], kv_heads, n_q, head_dim, &entry)) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int i0 = 0; i0 < n; i0 += kSetItems) {
        const int count = n - i0 < kSetItems ? n - i0 : kSetItems;
        SetArgs a{};
        for (int i = 0; i < count; i++) {
            (void)sequence_entry(items[i0 + i], kv_heads, n_q, head_dim, &entry);
            memcpy(a.w + i * kSeqWords, &entry, sizeof(entry));
        }
        const int words = count * kSeqWords;
        ragged_set_kernel<<<(words + kThreads - 1) / kThreads, kThreads, 0, st>>>(
            reinterpret_cast<uint64_t*>(table) + (int64_t)(first + i0) * kSeqWords, words, a);
    }
    return (int)hipGetLastError();
}

extern "C" int mustafar_decode_ragged(void* stream, const mustafar_sequence* table, int n_seqs, int kv_heads, int num_key_value_groups, int n_q,
                                      int T_max, int window_capacity_max, const void* q, const void* k_new, const void* v_new, void* out,
                                      float* lse, void* workspace, float sqrt_d, int head_dim)
{
    using namespace mustafar_shared;
    if (!rg_shape_ok(T_max, window_capacity_max, n_seqs, kv_heads, num_key_value_groups, n_q, head_dim) || !(sqrt_d > 0.f))
        return MUSTAFAR_EINVAL;
    if ((k_new == nullptr) != (v_new == nullptr) || !table || ((uintptr_t)table & 7)) return MUSTAFAR_EINVAL;
    if (!q || !out || !workspace || !lse || !aligned16(q) || !aligned16(out) || !aligned16(workspace) || !aligned16(k_new) || !aligned16(v_new) ||
        ((uintptr_t)lse & 3))
        return MUSTAFAR_EINVAL;
    const int Bp = n_seqs * kv_heads, R = n_q * num_key_value_groups, ntb = T_max / 64, bpw = blocks_per_run(R, head_dim);
    const int runs = (ntb + bpw - 1) / bpw, slabs = runs + (window_capacity_max + 63) / 64;
    RgArgs a{};
    a.table = table;
    a.q = static_cast<const h16*>(q);
    a.ws_o = static_cast<float*>(workspace);
    a.ws_ml = a.ws_o + (int64_t)slabs * Bp * R * head_dim;
    a.kv_heads = kv_heads; a.ntb_max = ntb; a.bpw = bpw; a.runs = runs; a.n_q = n_q; a.R = R; a.w_cap_max = window_capacity_max;
    a.inv_sqrt_d = (float)(1.0 / (double)sqrt_d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (k_new) {
        const int D8 = head_dim / 8, total = Bp * n_q * D8;
        ragged_append_kernel<<<dim3((total + kThreads - 1) / kThreads, 2), kThreads, 0, st>>>(
            table, static_cast<const uint4*>(k_new), static_cast<const uint4*>(v_new), kv_heads, n_q, ntb, window_capacity_max, D8, total);
    }
    const dim3 grid(slabs, Bp);
    const int rt = (R + 15) / 16;
    if (head_dim == 64) {
        switch (rt) {
            case 1: ragged_decode_kernel<64, 1><<<grid, kThreads, 0, st>>>(a); break;
            case 2: ragged_decode_kernel<64, 2><<<grid, kThreads, 0, st>>>(a); break;
            case 3: ragged_decode_kernel<64, 3><<<grid, kThreads, 0, st>>>(a); break;
            default: ragged_decode_kernel<64, 4><<<grid, kThreads, 0, st>>>(a); break;
        }
        ragged_merge_kernel<64><<<Bp * R, kThreads, 0, st>>>(table, a.ws_o, a.ws_ml, kv_heads, ntb, bpw, runs, n_q, R, window_capacity_max,
                                                             static_cast<h16*>(out), lse);
    } else {
        switch (rt) {
            case 1: ragged_decode_kernel<128, 1><<<grid, kThreads, 0, st>>>(a); break;
            case 2: ragged_decode_kernel<128, 2><<<grid, kThreads, 0, st>>>(a); break;
            case 3: ragged_decode_kernel<128, 3><<<grid, kThreads, 0, st>>>(a); break;
            default: ragged_decode_kernel<128, 4><<<grid, kThreads, 0, st>>>(a); break;
        }
        ragged_merge_kernel<128><<<Bp * R, kThreads, 0, st>>>(table, a.ws_o, a.ws_ml, kv_heads, ntb, bpw, runs, n_q, R, window_capacity_max,
                                                              static_cast<h16*>(out), lse);
    }
    return (int)hipGetLastError();
}
