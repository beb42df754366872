// shared_segment.hip -- decode over ONE compressed copy of a segment that every sequence of a batch shares (a system prompt, a document,
// n samples of one prompt), head_dim 64 and 128, for gfx950.  The C ABI entry points mustafar_decode_shared_segment and
// mustafar_shared_segment_workspace_bytes (include/mustafar_hip.h, ABI 111).
//
// The cache holds kv_heads heads in the reference format.  With n_seqs sequences and G q heads per kv head, a kv head serves
// R = n_seqs * G query rows (local row r = s * G + g), and the per-tile cost of this format -- bitmap, rank, address, select -- is paid
// once per tile however many rows then use the value.  So a 64-token block is expanded into a dense fp16 image in LDS and handed to the
// matrix pipe: scores = q [R x D] . K^T [D x 64], out += e [R x 64] . V [64 x D], v_mfma_f32_16x16x32_f16, fp32 accumulators.
//
// Grid (runs, kv heads), 256 threads.  A workgroup serves one kv head and a run of `bpw` consecutive blocks for all R rows (padded to
// row tiles of 16 with zero query rows).  Per block:
//   stage      the block's key stream -- one contiguous 16-byte aligned byte range -- to LDS with coalesced 16-byte loads; the bitmaps and
//              offsets of a wave's tiles with one vector load each, a tile per lane.  Both are requested a phase or a block ahead and
//              held in registers until the LDS buffer is free, so that their latency runs behind the phase in between
//   K expand   lane = token, wave w takes the D / 4 channel tiles [w D / 4, (w + 1) D / 4): the bitmap (v_readlane of the lane that holds
//              it) bit-reversed is the lane mask of a tile and the input of v_mbcnt, which ranks the lane's element in the tile's packed
//              stream (as hd64_decode_kernel); the wave's D / 4 halfs of a token leave as 16-byte LDS stores into img[token][channel]
//   scores     wave w = tokens [16 w, 16 w + 16): the B fragment of k-step s is img[token l & 15][32 s + 8 (l >> 4) ..+8), one 16-byte
//              read; the q fragments stay in registers for the whole run.  x = fp16(fp16(score) * fp32(1 / sqrt d)) -> xe[row][token]
//   softmax    thread = (row, 16 tokens), four lanes per row: the online step of headdim64.hip's softmax_step -- e = fp16(exp(x - m)) back
//              into xe, the running sum adds the rounded e, alpha = exp(m_old - m) per row to LDS; max and sum cross the quad by DPP
//   V expand   lane = channel, wave w takes tokens [16 w, 16 w + 16) (both 64-channel halves at D = 128): 16 halfs of a channel leave
//              as 16-byte stores into img[channel][token] -- the image is the transpose the B operand of e . V wants, no transposing read
//   out        wave w = channel tiles [w D / 64, (w + 1) D / 64): o = o * alpha + e . V
// After the run: one slab (m, l, o[D], fp32) per (workgroup, row); shared_merge_kernel folds a row's slabs into out and lse.
// Products are fp16 x fp16, exact in fp32; sums are fp32.  No inline assembly.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mustafar_hip.h"

namespace mustafar_shared {
namespace {

typedef _Float16 h16;
typedef h16 h16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) uint32_t* cu32_p;   // read-only, wave-uniform: scalar loads

constexpr int kThreads = 256;
constexpr int kMaxRows = 64;     // rows of a kv head per launch
constexpr int kRowPad = 72;      // halfs of a 64-half LDS row: 144 bytes, so the 16 rows of a 16-byte fragment read hit 16 different slots
// Run length.  A workgroup writes one slab of R (D + 2) floats and the row kernel reads it once: 8 R (D + 2) bytes per run.  A block's
// compressed K + V at 70 % sparsity is about 88 D bytes (0.3 x 2 x 64 D halfs of stream, D bitmaps and D offsets per side: 11 KB at
// D = 128).  blocks per run = the smallest count whose stream bytes are at least the slab bytes: ceil(8 R (D + 2) / (88 D)) -- 1 up to
// R = 10, 3 at R = 32, 6 at R = 64.  Depends on R and D alone, so a caller reads the slab count back from the workspace size.
constexpr int kBlockBytesPerD = 88;

inline int blocks_per_run(int R, int D)
{
    return (8 * R * (D + 2) + kBlockBytesPerD * D - 1) / (kBlockBytesPerD * D);
}

__device__ __forceinline__ uint32_t rank_below(uint64_t mr)   // set bits of mr below the lane
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mr >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mr, 0u));
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// max / sum over the four lanes of a quad (v_mov_b32 with a DPP quad permutation: no LDS, no latency to speak of)
template <int ctrl>
__device__ __forceinline__ float quad_xor(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, true));
}
__device__ __forceinline__ float quad_max(float v)
{
    v = fmaxf(v, quad_xor<0xB1>(v));   // lanes 1 0 3 2
    return fmaxf(v, quad_xor<0x4E>(v));                   // lanes 2 3 0 1
}
__device__ __forceinline__ float quad_sum(float v)
{
    v += quad_xor<0xB1>(v);
    return v + quad_xor<0x4E>(v);
}
// x = fp16(fp16(score) * (1/sqrt d)): headdim64.hip's scaled()
__device__ __forceinline__ h16 scaled(float acc, float inv_sqrt_d) { return (h16)((float)(h16)acc * inv_sqrt_d); }

struct SideArgs {
    const uint64_t* bmp;
    const uint32_t* idx;
    const uint4* nz;
    const uint32_t* nz_offset;
    int64_t bmp_stride, idx_stride;
    uint32_t nz_stride;   // != 0: head h starts at h * nz_stride (uint4 units) instead of nz_offset[h]
};
struct SegArgs {
    SideArgs k, v;
    const h16* q;     // [n_seqs, kv_heads * G, D]
    float* ws_o;      // [runs, kv_heads, R, D]
    float* ws_ml;     // [runs, kv_heads, R, 2]
    int ntb, bpw, n_seqs, groups, R;
    float inv_sqrt_d;
};

// A block's packed stream [2 idx[0], 2 idx[tiles]) halfs -> LDS as 16-byte pieces (every tile's stream is padded to 8 halfs, a head's stream
// starts on 16 bytes; at most 8 uint4 per tile), in two halves: the loads are issued early into registers, the LDS stores follow when the
// buffer is free, so that the memory latency runs behind the phase in between.
template <int TILES>
struct StreamRegs {
    uint4 r[8 * TILES / kThreads];
    int n16;
    uint32_t i0;   // the block's first offset (half2 units)
};
template <int TILES>
__device__ __forceinline__ void load_block(const uint4* __restrict__ head_nz, cu32_p idx, int tid, StreamRegs<TILES>& g)
{
    const uint32_t i0 = idx[0], i1 = idx[TILES];
    g.i0 = i0;
    g.n16 = (int)((i1 - i0) >> 2);
    const uint4* src = head_nz + (i0 >> 2);
#pragma unroll
    for (int k = 0; k < 8 * TILES / kThreads; k++) {
        const int i = tid + kThreads * k;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (i < g.n16) v = src[i];
        g.r[k] = v;
    }
}
template <int TILES>
__device__ __forceinline__ void store_block(const StreamRegs<TILES>& g, uint4* s_stream, int tid)
{
#pragma unroll
    for (int k = 0; k < 8 * TILES / kThreads; k++) {
        const int i = tid + kThreads * k;
        if (i < g.n16) s_stream[i] = g.r[k];
    }
}

// Bitmap and offset of the tiles a wave expands in one phase, one tile per lane (a coalesced vector load each); the expand reads tile j's
// through v_readlane, so no memory latency stands between two tiles.
struct TileMeta {
    uint32_t blo, bhi, idx;
};
__device__ __forceinline__ TileMeta load_meta(const uint64_t* __restrict__ bmp, const uint32_t* __restrict__ idx, int tile, bool on)
{
    TileMeta m{0u, 0u, 0u};
    if (on) {
        const uint64_t b = bmp[tile];
        m.blo = (uint32_t)b;
        m.bhi = (uint32_t)(b >> 32);
        m.idx = idx[tile];
    }
    return m;
}
// Element `lane` of the tile that lane j of `m` describes (0 where the bitmap has none), as raw fp16 bits; i0: the staged block's first offset.
template <int TILES>
__device__ __forceinline__ uint32_t tile_element(const TileMeta& m, int j, uint32_t i0, const uint16_t* sb, int lane)
{
    const uint64_t b = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)m.bhi, j) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)m.blo, j);
    const uint64_t mr = __builtin_bitreverse64(b);
    const uint32_t off = 2 * ((uint32_t)__builtin_amdgcn_readlane((int)m.idx, j) - i0) + rank_below(mr);
    const uint32_t raw = sb[off < 64u * TILES ? off : 0];
    return ((mr >> lane) & 1ull) ? raw : 0u;
}

template <int D, int RT>
__global__ __launch_bounds__(kThreads) void shared_segment_decode_kernel(SegArgs a)
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
    const int kvh = blockIdx.y, run = blockIdx.x;
    const int G = a.groups, R = a.R, H = gridDim.y * G;
    const int l15 = lane & 15, l4 = lane >> 4;
    const uint16_t* sb = reinterpret_cast<const uint16_t*>(s_stream);

    // q fragments (A operand): lane holds q[row 16 rt + (l & 15)][32 s + 8 (l >> 4) ..+8); rows at or beyond R are zero
    h16x8 qf[RT][KS];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        const int r = rt * 16 + l15;
        const bool live = r < R;
        const int rr = live ? r : 0;
        const h16* qrow = a.q + ((int64_t)(rr / G) * H + kvh * G + rr % G) * D;
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

    const int tb0 = run * a.bpw, tb1 = min(a.ntb, tb0 + a.bpw);
    const uint4* kz = a.k.nz + (a.k.nz_stride ? (int64_t)kvh * a.k.nz_stride : (int64_t)a.k.nz_offset[kvh]);
    const uint4* vz = a.v.nz + (a.v.nz_stride ? (int64_t)kvh * a.v.nz_stride : (int64_t)a.v.nz_offset[kvh]);
    const uint64_t* kb_h = a.k.bmp + kvh * a.k.bmp_stride;
    const uint32_t* ki_h = a.k.idx + kvh * a.k.idx_stride;
    const uint64_t* vb_h = a.v.bmp + kvh * a.v.bmp_stride;
    const uint32_t* vi_h = a.v.idx + kvh * a.v.idx_stride;

    // the tiles this wave expands: K tile wave D / 4 + lane (lanes below D / 4), V tile 64 (lane >> 4) + 16 wave + (lane & 15) (lanes below D / 4)
    const bool meta_on = lane < D / 4;
    const int k_tile = wave * (D / 4) + lane, v_tile = (lane >> 4) * 64 + wave * 16 + l15;
    TileMeta km = load_meta(kb_h + (int64_t)tb0 * TILES, ki_h + (int64_t)tb0 * TILES, k_tile, meta_on);
    TileMeta vm = load_meta(vb_h + (int64_t)tb0 * TILES, vi_h + (int64_t)tb0 * TILES, v_tile, meta_on);
    StreamRegs<TILES> kg{}, vg{};
    load_block<TILES>(kz, (cu32_p)(ki_h + (int64_t)tb0 * TILES), tid, kg);
    store_block<TILES>(kg, s_stream, tid);
    uint32_t k0 = kg.i0;
    __syncthreads();
    for (int tb = tb0; tb < tb1; tb++) {
        // requested now, used later: this block's value stream, the next block's bitmaps and offsets
        load_block<TILES>(vz, (cu32_p)(vi_h + (int64_t)tb * TILES), tid, vg);
        const int64_t nx = (int64_t)min(tb + 1, tb1 - 1) * TILES;
        const TileMeta km_next = load_meta(kb_h + nx, ki_h + nx, k_tile, meta_on);
        const TileMeta vm_next = load_meta(vb_h + nx, vi_h + nx, v_tile, meta_on);
        // ---- K expand: lane = token, this wave's D / 4 channel tiles -> img[token][channel]
        {
            uint32_t pk[D / 8];   // D / 4 halfs
#pragma unroll
            for (int j = 0; j < D / 4; j += 2) {
                const uint32_t lo = tile_element<TILES>(km, j, k0, sb, lane);
                const uint32_t hi = tile_element<TILES>(km, j + 1, k0, sb, lane);
                pk[j >> 1] = lo | (hi << 16);
            }
            uint4* dst = reinterpret_cast<uint4*>(s_img + lane * KROW + wave * (D / 4));
#pragma unroll
            for (int p = 0; p < D / 32; p++) dst[p] = make_uint4(pk[4 * p], pk[4 * p + 1], pk[4 * p + 2], pk[4 * p + 3]);
        }
        __syncthreads();   // the key image is whole, the key stream is read
        store_block<TILES>(vg, s_stream, tid);
        // ---- scores: this wave's 16 tokens, every row tile
        {
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
                    s_xe[(rt * 16 + 4 * l4 + i) * kRowPad + wave * 16 + l15] = scaled(acc[i], a.inv_sqrt_d);
            }
        }
        __syncthreads();   // x is whole, the key image is read, the value stream is staged
        if (tb + 1 < tb1) load_block<TILES>(kz, (cu32_p)(ki_h + (int64_t)(tb + 1) * TILES), tid, kg);   // (requested now, stored behind the softmax)
        // ---- V expand: lane = channel, this wave's 16 tokens -> img[channel][token]
        {
            const uint32_t v0 = vg.i0;
#pragma unroll
            for (int hh = 0; hh < D / 64; hh++) {
                uint32_t pk[8];
#pragma unroll
                for (int j = 0; j < 16; j += 2) {
                    const uint32_t lo = tile_element<TILES>(vm, hh * 16 + j, v0, sb, lane);
                    const uint32_t hi = tile_element<TILES>(vm, hh * 16 + j + 1, v0, sb, lane);
                    pk[j >> 1] = lo | (hi << 16);
                }
                uint4* dst = reinterpret_cast<uint4*>(s_img + (hh * 64 + lane) * kRowPad + wave * 16);
                dst[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
                dst[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
            }
        }
        // ---- online softmax step: thread = (row tid >> 2, 16 tokens): the step of headdim64.hip's softmax_step, the row's max and sum
        // folded over the quad.  Rows of zero queries (at or beyond R) go through it like any other: x = 0, finite everywhere
        if (srow < RT * 16) {
            h16x8* px = reinterpret_cast<h16x8*>(s_xe + srow * kRowPad + sq * 16);
            const h16x8 xa = px[0], xb = px[1];
            float x[16];
#pragma unroll
            for (int j = 0; j < 8; j++) { x[j] = (float)xa[j]; x[8 + j] = (float)xb[j]; }
            float mx = x[0];
#pragma unroll
            for (int j = 1; j < 16; j++) mx = fmaxf(mx, x[j]);
            const float mn = fmaxf(M, quad_max(mx));
            const float alpha = __expf(M - mn);                 // (exp(-inf) = 0 before the first block)
            h16x8 ea, eb;
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const h16 e = (h16)__expf(x[j] - mn);
                sum += (float)e;
                if (j < 8) ea[j] = e; else eb[j - 8] = e;
            }
            L = L * alpha + quad_sum(sum);
            M = mn;
            px[0] = ea;
            px[1] = eb;
            if (sq == 0) s_alpha[srow] = alpha;
        }
        __syncthreads();   // e, alpha and the value image are whole, the value stream is read
        if (tb + 1 < tb1) {
            store_block<TILES>(kg, s_stream, tid);
            k0 = kg.i0;
        }
        // ---- out: this wave's channel tiles, every row tile
        {
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
        __syncthreads();   // the value image, e and alpha are read; the next key stream is staged
        km = km_next;
        vm = vm_next;
    }
    // ---- the workgroup's slab of every row
    const int64_t slab = ((int64_t)run * gridDim.y + kvh) * R;
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int c = 0; c < CT; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int r = rt * 16 + 4 * l4 + i;
                if (r < R) a.ws_o[(slab + r) * D + (wave * CT + c) * 16 + l15] = o[rt][c][i];
            }
    if (srow < R && sq == 0) { a.ws_ml[2 * (slab + srow)] = M; a.ws_ml[2 * (slab + srow) + 1] = L; }
}

// out[s, h, c] = fp16( sum_x w_x o_x[c] / sum_x w_x l_x ),  w_x = exp(m_x - max m);  lse[s, h] = max m + log(sum_x w_x l_x).  One workgroup
// per row (s, h), thread = (slab phase, four channels): 1024 / D phases over the row's slabs, 16-byte loads that do not depend on each other
// (a row has up to T / 64 slabs and every trip is a memory latency: the phases and the unrolled trips keep many in flight), folded through LDS.
template <int D>
__global__ __launch_bounds__(kThreads) void shared_merge_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml, int S,
                                                                int kv_heads, int G, int R, h16* __restrict__ out, float* __restrict__ lse)
{
    constexpr int C4 = D / 4, P = kThreads / C4;
    __shared__ float4 part[P][C4];
    __shared__ float dens[P];
    const int H = kv_heads * G, s = blockIdx.x / H, h = blockIdx.x % H;
    const int kvh = h / G, r = s * G + h % G;
    const int lane = threadIdx.x & 63, c4 = threadIdx.x % C4, ph = threadIdx.x / C4;
    const int64_t stride = (int64_t)kv_heads * R, first = (int64_t)kvh * R + r;
    float mx = -INFINITY;
    for (int x = lane; x < S; x += 64) mx = fmaxf(mx, ws_ml[2 * (x * stride + first)]);
    const float Mx = wave_max(mx);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float den = 0.f;
#pragma unroll 4
    for (int x = ph; x < S; x += P) {
        const int64_t row = x * stride + first;
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
        dst[0] = (h16)(ov.x / d); dst[1] = (h16)(ov.y / d); dst[2] = (h16)(ov.z / d); dst[3] = (h16)(ov.w / d);
        if (c4 == 0) lse[blockIdx.x] = d > 0.f ? Mx + __logf(d) : -INFINITY;
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool shape_ok(int T, int kv_heads, int groups, int n_seqs, int head_dim)
{
    if (T <= 0 || (T & 63) || kv_heads < 1 || kv_heads > 65535 || groups < 1 || groups > 8 || n_seqs < 1) return false;
    if ((int64_t)n_seqs * groups > kMaxRows) return false;
    return head_dim == 64 || head_dim == 128;
}

// A side's view with its strides resolved, or false: rows shorter than the tokens, a stream the kernel cannot address.
bool side_of(const mustafar_cache_view* v, int T, int kv_heads, int D, SideArgs* s)
{
    if (!v || !v->bmp || !v->idx || !v->nz || !aligned16(v->nz)) return false;
    const int64_t tiles = (int64_t)T * D / 64;
    if ((v->bmp_head_stride && v->bmp_head_stride < tiles) || (v->idx_head_stride && v->idx_head_stride < tiles + 1)) return false;
    if (v->nz_head_stride < 0 || (int64_t)kv_heads * v->nz_head_stride > 0xffffffffll || (!v->nz_head_stride && !v->nz_offset)) return false;
    *s = SideArgs{v->bmp, v->idx, static_cast<const uint4*>(v->nz), v->nz_offset, v->bmp_head_stride ? v->bmp_head_stride : tiles,
                  v->idx_head_stride ? v->idx_head_stride : tiles + 1, (uint32_t)v->nz_head_stride};
    return true;
}

template <int D>
void launch(hipStream_t st, const SegArgs& a, int runs, int kv_heads, h16* out, float* lse)
{
    const dim3 grid(runs, kv_heads);
    switch ((a.R + 15) / 16) {
        case 1: shared_segment_decode_kernel<D, 1><<<grid, kThreads, 0, st>>>(a); break;
        case 2: shared_segment_decode_kernel<D, 2><<<grid, kThreads, 0, st>>>(a); break;
        case 3: shared_segment_decode_kernel<D, 3><<<grid, kThreads, 0, st>>>(a); break;
        default: shared_segment_decode_kernel<D, 4><<<grid, kThreads, 0, st>>>(a); break;
    }
    shared_merge_kernel<D><<<a.n_seqs * kv_heads * a.groups, kThreads, 0, st>>>(a.ws_o, a.ws_ml, runs, kv_heads, a.groups, a.R, out, lse);
}

}  // namespace
}  // namespace mustafar_shared

extern "C" int64_t mustafar_shared_segment_workspace_bytes(int T, int kv_heads, int num_key_value_groups, int n_seqs, int head_dim)
{
    using namespace mustafar_shared;
    if (!shape_ok(T, kv_heads, num_key_value_groups, n_seqs, head_dim)) return 0;
    const int R = n_seqs * num_key_value_groups, ntb = T / 64, bpw = blocks_per_run(R, head_dim);
    return (int64_t)((ntb + bpw - 1) / bpw) * kv_heads * R * (head_dim + 2) * (int64_t)sizeof(float);
}

extern "C" int mustafar_decode_shared_segment(void* stream, const mustafar_cache_view* k_cache, const mustafar_cache_view* v_cache, int T,
                                              int kv_heads, int num_key_value_groups, int n_seqs, const void* q, void* out, float* lse,
                                              void* workspace, float sqrt_d, int head_dim)
{
    using namespace mustafar_shared;
    if (!shape_ok(T, kv_heads, num_key_value_groups, n_seqs, head_dim) || !(sqrt_d > 0.f)) return MUSTAFAR_EINVAL;
    if (!q || !out || !lse || !workspace || !aligned16(q) || !aligned16(out) || ((uintptr_t)lse & 3) || !aligned16(workspace))
        return MUSTAFAR_EINVAL;
    SegArgs a{};
    if (!side_of(k_cache, T, kv_heads, head_dim, &a.k) || !side_of(v_cache, T, kv_heads, head_dim, &a.v)) return MUSTAFAR_EINVAL;
    const int R = n_seqs * num_key_value_groups, ntb = T / 64, bpw = blocks_per_run(R, head_dim);
    const int runs = (ntb + bpw - 1) / bpw;
    a.q = static_cast<const h16*>(q);
    a.ws_o = static_cast<float*>(workspace);
    a.ws_ml = a.ws_o + (int64_t)runs * kv_heads * R * head_dim;
    a.ntb = ntb; a.bpw = bpw; a.n_seqs = n_seqs; a.groups = num_key_value_groups; a.R = R;
    a.inv_sqrt_d = (float)(1.0 / (double)sqrt_d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (head_dim == 64) launch<64>(st, a, runs, kv_heads, static_cast<h16*>(out), lse);
    else launch<128>(st, a, runs, kv_heads, static_cast<h16*>(out), lse);
    return (int)hipGetLastError();
}
