// expand_block.h -- the device side that shared_segment.hip and multi_query.hip have in common: a 64-token block of the compressed format
// expanded once into a dense fp16 image in LDS and served to up to 64 query rows on the matrix pipe (v_mfma_f32_16x16x32_f16), as
// shared_segment.hip's header describes it: the staging of a block's stream and metadata, the expansion of a tile element, the quad
// reductions, the validation of a cache view, and the row kernel that folds a row's (max, sum, output) slabs.  No inline assembly.
#ifndef MUSTAFAR_EXPAND_BLOCK_H
#define MUSTAFAR_EXPAND_BLOCK_H

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
constexpr int kMaxRows = 64;     // rows of a kv head per workgroup (and per launch of the single-token entry points)
constexpr int kMaxRowsMulti = 1024;   // rows of a kv head per launch of the several-token segment forms: up to 16 chunks of kMaxRows in blockIdx.z
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

// out[s, h, c] = fp16( sum_x w_x o_x[c] / sum_x w_x l_x ),  w_x = exp(m_x - max m);  lse[s, h] = max m + log(sum_x w_x l_x).  One workgroup
// per row (s, h), thread = (slab phase, four channels): 1024 / D phases over the row's slabs, 16-byte loads that do not depend on each other
// (a row has up to T / 64 slabs and every trip is a memory latency: the phases and the unrolled trips keep many in flight), folded through LDS.
// multi_query.hip launches it with (kv_heads, G, R) = (B', R, R): H covers the whole grid, so s = 0, kvh = row / R and r = row % R -- the
// rows of one (sequence, kv head) are consecutive in its q / out / lse.
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

// A side's view with its strides resolved, or false: rows shorter than the tokens, a stream the kernel cannot address.
inline bool side_of(const mustafar_cache_view* v, int T, int kv_heads, int D, SideArgs* s)
{
    if (!v || v->flags || !v->bmp || !v->idx || !v->nz || !aligned16(v->nz)) return false;   // (flags: tiles only, not token rows)
    const int64_t tiles = (int64_t)T * D / 64;
    if ((v->bmp_head_stride && v->bmp_head_stride < tiles) || (v->idx_head_stride && v->idx_head_stride < tiles + 1)) return false;
    if (v->nz_head_stride < 0 || (int64_t)kv_heads * v->nz_head_stride > 0xffffffffll || (!v->nz_head_stride && !v->nz_offset)) return false;
    *s = SideArgs{v->bmp, v->idx, static_cast<const uint4*>(v->nz), v->nz_offset, v->bmp_head_stride ? v->bmp_head_stride : tiles,
                  v->idx_head_stride ? v->idx_head_stride : tiles + 1, (uint32_t)v->nz_head_stride};
    return true;
}

}  // namespace
}  // namespace mustafar_shared

#endif /* MUSTAFAR_EXPAND_BLOCK_H */
