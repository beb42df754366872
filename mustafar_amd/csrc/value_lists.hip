// value_lists.hip -- sorted channel lists (include/mustafar_hip.h: MUSTAFAR_VIEW_VALUE_LISTS): the retile passes between
// the tile format of a value cache and the lists the GQA-4 one-pass super-block launch reads its value base in.  head_dim 128 only.
//
//   tiles -> lists   mustafar_value_lists_plan (block sizes, block table) + mustafar_value_lists_fill (one wave per block half)
//   lists -> tiles   mustafar_value_lists_to_tiles: bitmaps and tile lengths per half, the offsets of a head by one scan, the streams per half
//
// A value block in tiles is 128 tiles (tile 64 half + t = channels 64 half .. + 63 of the block's token t; bit 63 - c of its bitmap =
// channel c of the half; its non-zeros in channel order, padded with zeros to a multiple of 8 halfs).  In lists, lane rank(c) of a half
// holds channel c's (token, value) entries in token order.  Both directions walk a channel's tokens in order with one running slot
// counter per lane, so each is the other's inverse element by element.  The index arithmetic is value_lists.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mustafar_hip.h"
#include "value_lists.h"

namespace {

constexpr int kD = 128;   // tiles per 64-token block

__device__ __forceinline__ const uint16_t* head_stream(const mustafar_cache_view& v, int h)
{
    const uint64_t start = v.nz_head_stride ? (uint64_t)h * (uint64_t)v.nz_head_stride : (uint64_t)v.nz_offset[h];   // uint4 units
    return reinterpret_cast<const uint16_t*>(static_cast<const unsigned char*>(v.nz) + 16ull * start);
}
__device__ __forceinline__ int tile_rank(uint64_t m, int c) { return c ? __popcll(m >> (64 - c)) : 0; }
__device__ __forceinline__ const uint64_t* tile_bmp(const mustafar_cache_view& v, int h, int nb)
{
    return v.bmp + (int64_t)h * (v.bmp_head_stride ? v.bmp_head_stride : (int64_t)nb * kD);
}
__device__ __forceinline__ const uint32_t* tile_idx(const mustafar_cache_view& v, int h, int nb)
{
    return v.idx + (int64_t)h * (v.idx_head_stride ? v.idx_head_stride : (int64_t)nb * kD + 1);
}
__device__ __forceinline__ unsigned char* list_block(const mustafar_cache_view& v, int h, int b)
{
    return static_cast<unsigned char*>(v.nz) + 16ull * (uint64_t)h * (uint64_t)v.nz_head_stride + 4ull * v.idx[(int64_t)h * v.idx_head_stride + b];
}

// The lists of one half (64 tiles at bmp), lane = channel c: cnt, the lane the channel's list lives in, and the row widths m[0..31] in LDS.
struct HalfPlan {
    int cnt, rank;
};
__device__ __forceinline__ HalfPlan half_plan(const uint64_t* __restrict__ bmp, int c, unsigned char* m)
{
    HalfPlan p{0, 0};
    for (int t = 0; t < 64; t++) p.cnt += vl_bit(bmp[t], c);
    for (int o = 0; o < 64; o++) {   // rank by comparison: cnt descending, ties by channel ascending
        const int other = __shfl(p.cnt, o, 64);
        p.rank += other > p.cnt || (other == p.cnt && o < c);
    }
    for (int r = 0; r < kVlMaxRows; r++) {
        const int w = __popcll(__ballot(p.cnt > 2 * r));
        if (c == 0) m[r] = (unsigned char)w;
    }
    __syncthreads();
    return p;
}

// One wave per (block, head): the block's size in dwords -> table[h][b] (the scan below turns it into the block's start).
__global__ __launch_bounds__(64) void value_lists_size_kernel(mustafar_cache_view src, int nb, uint32_t* __restrict__ table)
{
    __shared__ unsigned char m[2][kVlMaxRows];
    const int b = blockIdx.x, h = blockIdx.y, c = threadIdx.x;
    const uint64_t* bmp = tile_bmp(src, h, nb) + (int64_t)b * kD;
    half_plan(bmp, c, m[0]);
    half_plan(bmp + 64, c, m[1]);
    if (c == 0) table[(int64_t)h * (nb + 1) + b] = (uint32_t)vl_block_dwords(vl_word_offset(m[0], kVlMaxWords), vl_word_offset(m[1], kVlMaxWords));
}

// One wave per head: sizes -> starts (exclusive prefix; entry nb: the head's dwords).
__global__ __launch_bounds__(64) void value_lists_scan_kernel(int nb, uint32_t* __restrict__ table, int64_t* __restrict__ head_dwords)
{
    const int h = blockIdx.x, l = threadIdx.x;
    uint32_t* tab = table + (int64_t)h * (nb + 1);
    uint32_t run = 0;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int b = b0 + l;
        const uint32_t n = b < nb ? tab[b] : 0u;
        uint32_t inc = n;   // inclusive prefix over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(inc, o, 64);
            if (l >= o) inc += up;
        }
        if (b < nb) tab[b] = run + inc - n;
        run += __shfl(inc, 63, 64);
    }
    if (l == 0) {
        tab[nb] = run;
        head_dwords[h] = (int64_t)run;
    }
}

// One wave per (block half, head), lane = channel: the half's part of the header and its words.
__global__ __launch_bounds__(64) void value_lists_fill_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ unsigned char m_first[kVlMaxRows], m[kVlMaxRows];
    __shared__ int woff[kVlMaxWords + 1];
    const int b = blockIdx.x >> 1, half = blockIdx.x & 1, h = blockIdx.y, c = threadIdx.x;
    const int64_t tile0 = (int64_t)b * kD + half * 64;
    const uint64_t* bmp = tile_bmp(src, h, nb) + tile0;
    const uint32_t* idx = tile_idx(src, h, nb) + tile0;
    const uint16_t* nz = head_stream(src, h);
    unsigned char* blk = list_block(dst, h, b);
    int half0 = 0;
    if (half) {   // (the second half lies behind the first: its size again)
        half_plan(bmp - 64, c, m_first);
        half0 = vl_word_offset(m_first, kVlMaxWords);
    }
    const HalfPlan p = half_plan(bmp, c, m);
    if (c <= kVlMaxWords) woff[c] = vl_word_offset(m, c);
    __syncthreads();
    const int mine = woff[kVlMaxWords];
    // header
    blk[kVlPermByte + half * 64 + p.rank] = (unsigned char)c;
    if (c < kVlMaxRows) blk[kVlWidthByte + half * kVlMaxRows + c] = m[c];
    uint32_t* blk32 = reinterpret_cast<uint32_t*>(blk);
    if (!half) {
        if (c == 0) blk32[kVlHalf1Dword] = (uint32_t)(kVlHeaderDwords + mine);
        if (c > 0 && c < kVlHeaderDwords - kVlHalf1Dword) blk32[kVlHalf1Dword + c] = 0u;
    } else {
        const int used = kVlHeaderDwords + half0 + mine;
        if (used + c < vl_block_dwords(half0, mine)) blk32[used + c] = 0u;   // (at most three dwords of padding)
    }
    // lists
    unsigned char* base = blk + 4 * (kVlHeaderDwords + half0);
    const int i = p.rank;
    int s = 0;
    for (int t = 0; t < 64; t++) {
        const uint64_t bits = bmp[t];
        if (vl_bit(bits, c)) {
            const int w = woff[s >> 2];
            base[vl_token_byte(w, i, s)] = (unsigned char)t;
            *reinterpret_cast<uint16_t*>(base + vl_value_byte(m, w, i, s)) = nz[2ull * idx[t] + tile_rank(bits, c)];
            s++;
        }
    }
    if (s & 1) *reinterpret_cast<uint16_t*>(base + vl_value_byte(m, woff[s >> 2], i, s)) = 0;
    for (int q = s; q < vl_token_slots(s); q++) base[vl_token_byte(woff[q >> 2], i, q)] = 0;
}

// ---- lists -> tiles
// A lane's entries: slot s of lane i is an entry if the lane takes part in its rows and s == 0 or its token is not 0 (tokens ascend).
struct HalfLists {
    const unsigned char* base;   // the half's words
    const unsigned char* m;      // its row widths (header bytes)
    int chan;                    // the channel lane i owns
};
__device__ __forceinline__ HalfLists half_lists(const unsigned char* blk, int half, int i, int* woff)
{
    HalfLists L;
    L.m = blk + kVlWidthByte + half * kVlMaxRows;
    L.base = blk + (half ? 4ull * reinterpret_cast<const uint32_t*>(blk)[kVlHalf1Dword] : 4ull * kVlHeaderDwords);
    L.chan = blk[kVlPermByte + half * 64 + i] & 63;
    if (i <= kVlMaxWords) woff[i] = vl_word_offset(L.m, i);
    __syncthreads();
    return L;
}
// token of slot s of lane i, or -1 behind the lane's last entry
__device__ __forceinline__ int list_token(const HalfLists& L, const int* woff, int i, int s)
{
    if (s >= 2 * kVlMaxRows || i >= L.m[s >> 1]) return -1;
    const int t = L.base[vl_token_byte(woff[s >> 2], i, s)];
    return (s == 0 || t != 0) ? (t & 63) : -1;
}

// One wave per (block half, head): the 64 bitmaps of the half and every tile's length in half2 units -> dst.idx[h][tile + 1].
__global__ __launch_bounds__(64) void value_tiles_bitmap_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ unsigned long long bits[64];
    __shared__ int woff[kVlMaxWords + 1];
    const int b = blockIdx.x >> 1, half = blockIdx.x & 1, h = blockIdx.y, i = threadIdx.x;
    bits[i] = 0ull;
    const HalfLists L = half_lists(list_block(src, h, b), half, i, woff);
    for (int s = 0;; s++) {
        const int t = list_token(L, woff, i, s);
        if (t < 0) break;
        atomicOr(&bits[t], 1ull << (63 - L.chan));
    }
    __syncthreads();
    const int64_t tile0 = (int64_t)b * kD + half * 64;
    uint64_t* bmp = const_cast<uint64_t*>(tile_bmp(dst, h, nb)) + tile0;
    uint32_t* idx = const_cast<uint32_t*>(tile_idx(dst, h, nb)) + tile0;
    const uint64_t mt = bits[i];
    bmp[i] = mt;
    idx[i + 1] = (uint32_t)(((__popcll(mt) + 7) & ~7) >> 1);
}

// One wave per head: the tile lengths -> offsets (exclusive prefix, idx[h][0] = 0), the head's stream length in halfs.
__global__ __launch_bounds__(64) void value_tiles_scan_kernel(mustafar_cache_view dst, int nb, int64_t* __restrict__ head_total)
{
    const int h = blockIdx.x, l = threadIdx.x;
    const int64_t tiles = (int64_t)nb * kD;
    uint32_t* idx = const_cast<uint32_t*>(tile_idx(dst, h, nb));
    uint32_t run = 0;
    if (l == 0) idx[0] = 0u;
    for (int64_t i0 = 0; i0 < tiles; i0 += 64) {   // (tiles % 64 == 0)
        uint32_t inc = idx[i0 + l + 1];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(inc, o, 64);
            if (l >= o) inc += up;
        }
        idx[i0 + l + 1] = run + inc;
        run += __shfl(inc, 63, 64);
    }
    if (l == 0 && head_total) head_total[h] = 2ll * run;
}

// One wave per (block half, head): the streams of the half's 64 tiles, padding included.
__global__ __launch_bounds__(64) void value_tiles_stream_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ int woff[kVlMaxWords + 1];
    const int b = blockIdx.x >> 1, half = blockIdx.x & 1, h = blockIdx.y, i = threadIdx.x;
    const HalfLists L = half_lists(list_block(src, h, b), half, i, woff);
    const int64_t tile0 = (int64_t)b * kD + half * 64;
    const uint64_t* bmp = tile_bmp(dst, h, nb) + tile0;
    const uint32_t* idx = tile_idx(dst, h, nb) + tile0;
    uint16_t* nz = const_cast<uint16_t*>(head_stream(dst, h));
    for (int s = 0;; s++) {
        const int t = list_token(L, woff, i, s);
        if (t < 0) break;
        nz[2ull * idx[t] + tile_rank(bmp[t], L.chan)] = *reinterpret_cast<const uint16_t*>(L.base + vl_value_byte(L.m, woff[s >> 2], i, s));
    }
    const int n = __popcll(bmp[i]), n8 = (n + 7) & ~7;   // lane = token: its tile's padding
    for (int p = n; p < n8; p++) nz[2ull * idx[i] + p] = 0;
}

bool tile_view_ok(const mustafar_cache_view* v, int tokens)
{
    const int64_t tiles = (int64_t)tokens * 2;
    return v && !v->flags && v->bmp && v->idx && v->nz && (v->nz_head_stride || v->nz_offset) && (!v->bmp_head_stride || v->bmp_head_stride >= tiles) &&
           (!v->idx_head_stride || v->idx_head_stride >= tiles + 1);
}
bool lists_view_ok(const mustafar_cache_view* v, int tokens)
{
    return v && v->flags == MUSTAFAR_VIEW_VALUE_LISTS && v->idx && v->nz && v->nz_head_stride > 0 && v->idx_head_stride >= tokens / 64 + 1;
}
bool shape_ok(int Bp, int tokens) { return Bp >= 1 && Bp <= 65535 && tokens > 0 && (tokens & 63) == 0 && tokens / 64 <= 0x3fffffff; }

}  // namespace

extern "C" {

int mustafar_value_lists_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_dwords)
{
    if (!shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !table || !head_dwords) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64;
    value_lists_size_kernel<<<dim3(nb, Bp), 64, 0, st>>>(*src, nb, table);
    value_lists_scan_kernel<<<Bp, 64, 0, st>>>(nb, table, head_dwords);
    return (int)hipGetLastError();
}

int mustafar_value_lists_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens)
{
    if (!shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !lists_view_ok(dst, tokens) || dst->idx_head_stride != tokens / 64 + 1) return MUSTAFAR_EINVAL;
    const int nb = tokens / 64;
    value_lists_fill_kernel<<<dim3(2 * nb, Bp), 64, 0, static_cast<hipStream_t>(stream)>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

int mustafar_value_lists_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total)
{
    if (!shape_ok(Bp, tokens) || !lists_view_ok(src, tokens) || !tile_view_ok(dst, tokens) || !dst->nz_head_stride) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64;
    value_tiles_bitmap_kernel<<<dim3(2 * nb, Bp), 64, 0, st>>>(*src, *dst, nb);
    value_tiles_scan_kernel<<<Bp, 64, 0, st>>>(*dst, nb, head_total);
    value_tiles_stream_kernel<<<dim3(2 * nb, Bp), 64, 0, st>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

}  // extern "C"
