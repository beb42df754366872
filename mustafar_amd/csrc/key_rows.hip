// key_rows.hip -- token-row key blocks (ABI 113; include/mustafar_hip.h): the retile passes between the tile format of a key
// cache and the rows the GQA-4 one-pass super-block launch reads its key base in.  head_dim 128 only.
//
//   tiles -> rows   mustafar_key_rows_plan (block widths, block table) + mustafar_key_rows_fill (one wave per 64-token block, lane = token)
//   rows -> tiles   mustafar_key_rows_to_tiles: bitmaps and tile lengths per block, the offsets of a head by one scan, the streams per block
//
// A key block in tiles is 128 tiles (tile d = channel d of the block's 64 tokens; bit 63 - t of its bitmap = token t; its non-zeros in
// token order, padded with zeros to a multiple of 8 halfs).  In rows, lane t holds token t's non-zero channels in ascending order.  Both
// directions walk the 128 channels in order with one running slot counter per lane, so each is the other's inverse element by element.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mustafar_hip.h"

namespace {

constexpr int kD = 128;   // channels = tiles per 64-token block

__device__ __forceinline__ const uint16_t* head_stream(const mustafar_cache_view& v, int h)
{
    const uint64_t start = v.nz_head_stride ? (uint64_t)h * (uint64_t)v.nz_head_stride : (uint64_t)v.nz_offset[h];   // uint4 units
    return reinterpret_cast<const uint16_t*>(static_cast<const unsigned char*>(v.nz) + 16ull * start);
}
__device__ __forceinline__ int rows_of(int w) { return (w >> 1) + ((w + 3) >> 2); }   // value rows + channel rows of a block of width w
// bit of token t in a tile's bitmap, and the number of the tile's non-zeros in front of it
__device__ __forceinline__ bool tile_bit(uint64_t m, int t) { return (m >> (63 - t)) & 1ull; }
__device__ __forceinline__ int tile_rank(uint64_t m, int t) { return t ? __popcll(m >> (64 - t)) : 0; }

__device__ __forceinline__ int wave_max_i(int v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// One wave per (block, head): the width of the block -> table[h][b] (the scan below turns it into a table entry).
__global__ __launch_bounds__(64) void key_rows_width_kernel(mustafar_cache_view src, int nb, uint32_t* __restrict__ table)
{
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const uint64_t* bmp = src.bmp + (int64_t)h * (src.bmp_head_stride ? src.bmp_head_stride : (int64_t)nb * kD) + (int64_t)b * kD;
    int n = 0;
    for (int d = 0; d < kD; d++) n += tile_bit(bmp[d], t);
    const int w = max(2, (wave_max_i(n) + 1) & ~1);
    if (t == 0) table[(int64_t)h * nb + b] = (uint32_t)w;
}

// One wave per head: widths -> (first row << 8 | w), and the head's number of rows.
__global__ __launch_bounds__(64) void key_rows_scan_kernel(int nb, uint32_t* __restrict__ table, int64_t* __restrict__ head_rows)
{
    const int h = blockIdx.x, l = threadIdx.x;
    uint32_t* tab = table + (int64_t)h * nb;
    uint32_t run = 0;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int b = b0 + l;
        const uint32_t w = b < nb ? tab[b] : 0u;
        const uint32_t r = b < nb ? (uint32_t)rows_of((int)w) : 0u;
        uint32_t inc = r;   // inclusive prefix over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(inc, o, 64);
            if (l >= o) inc += up;
        }
        if (b < nb) tab[b] = ((run + inc - r) << 8) | w;
        run += __shfl(inc, 63, 64);
    }
    if (l == 0) head_rows[h] = (int64_t)run;
}

// One wave per (block, head), lane = token: the rows of the block.
__global__ __launch_bounds__(64) void key_rows_fill_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const int64_t tile0 = (int64_t)b * kD;
    const uint64_t* bmp = src.bmp + (int64_t)h * (src.bmp_head_stride ? src.bmp_head_stride : (int64_t)nb * kD) + tile0;
    const uint32_t* idx = src.idx + (int64_t)h * (src.idx_head_stride ? src.idx_head_stride : (int64_t)nb * kD + 1) + tile0;
    const uint16_t* nz = head_stream(src, h);
    const uint32_t ent = dst.idx[(int64_t)h * dst.idx_head_stride + b];
    const int w = (int)(ent & 0xffu), npair = w >> 1, nword = (w + 3) >> 2;
    unsigned char* blk = static_cast<unsigned char*>(dst.nz) + 16ull * (uint64_t)h * (uint64_t)dst.nz_head_stride + 256ull * (ent >> 8);
    unsigned char* chan = blk + t * 4;                                          // slot c: chan[(c >> 2) * 256 + (c & 3)]
    uint16_t* vals = reinterpret_cast<uint16_t*>(blk + 256 * nword) + t * 2;   // slot c: vals[(c >> 1) * 128 + (c & 1)]
    int c = 0;
    for (int d = 0; d < kD; d++) {
        const uint64_t m = bmp[d];
        if (tile_bit(m, t)) {
            vals[(c >> 1) * 128 + (c & 1)] = nz[2ull * idx[d] + tile_rank(m, t)];
            chan[(c >> 2) * 256 + (c & 3)] = (unsigned char)d;
            c++;
        }
    }
    for (int p = c; p < 2 * npair; p++) vals[(p >> 1) * 128 + (p & 1)] = 0;
    for (int p = c; p < 4 * nword; p++) chan[(p >> 2) * 256 + (p & 3)] = 0;
}

// ---- rows -> tiles
// One wave per (block, head): the 128 bitmaps of the block and every tile's length in half2 units -> dst.idx[h][tile + 1].
__global__ __launch_bounds__(64) void key_tiles_bitmap_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ unsigned long long bits[kD];
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    bits[t] = 0ull;
    bits[t + 64] = 0ull;
    __syncthreads();
    const uint32_t ent = src.idx[(int64_t)h * src.idx_head_stride + b];
    const int w = (int)(ent & 0xffu), nword = (w + 3) >> 2;
    const unsigned char* blk = static_cast<const unsigned char*>(src.nz) + 16ull * (uint64_t)h * (uint64_t)src.nz_head_stride + 256ull * (ent >> 8);
    const unsigned char* chan = blk + t * 4;
    const uint16_t* vals = reinterpret_cast<const uint16_t*>(blk + 256 * nword) + t * 2;
    for (int c = 0; c < w; c++) {
        if ((vals[(c >> 1) * 128 + (c & 1)] & 0x7fffu) == 0) break;   // the slots behind a token's non-zeros hold +0
        atomicOr(&bits[chan[(c >> 2) * 256 + (c & 3)] & (kD - 1)], 1ull << (63 - t));   // (& 127: a channel byte is below 128)
    }
    __syncthreads();
    const int64_t tile0 = (int64_t)b * kD;
    uint64_t* bmp = dst.bmp + (int64_t)h * (dst.bmp_head_stride ? dst.bmp_head_stride : (int64_t)nb * kD) + tile0;
    uint32_t* idx = dst.idx + (int64_t)h * (dst.idx_head_stride ? dst.idx_head_stride : (int64_t)nb * kD + 1) + tile0;
    for (int d = t; d < kD; d += 64) {
        const uint64_t m = bits[d];
        bmp[d] = m;
        idx[d + 1] = (uint32_t)(((__popcll(m) + 7) & ~7) >> 1);
    }
}

// One wave per head: the tile lengths -> offsets (exclusive prefix, idx[h][0] = 0), the head's stream length in halfs.
__global__ __launch_bounds__(64) void key_tiles_scan_kernel(mustafar_cache_view dst, int nb, int64_t* __restrict__ head_total)
{
    const int h = blockIdx.x, l = threadIdx.x;
    const int64_t tiles = (int64_t)nb * kD;
    uint32_t* idx = dst.idx + (int64_t)h * (dst.idx_head_stride ? dst.idx_head_stride : tiles + 1);
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

// One wave per (block, head), lane = token: the streams of the block's 128 tiles, padding included.
__global__ __launch_bounds__(64) void key_tiles_stream_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const uint32_t ent = src.idx[(int64_t)h * src.idx_head_stride + b];
    const unsigned char* blk = static_cast<const unsigned char*>(src.nz) + 16ull * (uint64_t)h * (uint64_t)src.nz_head_stride + 256ull * (ent >> 8);
    const uint16_t* vals = reinterpret_cast<const uint16_t*>(blk + 256 * ((((int)(ent & 0xffu)) + 3) >> 2)) + t * 2;
    const int64_t tile0 = (int64_t)b * kD;
    const uint64_t* bmp = dst.bmp + (int64_t)h * (dst.bmp_head_stride ? dst.bmp_head_stride : (int64_t)nb * kD) + tile0;
    const uint32_t* idx = dst.idx + (int64_t)h * (dst.idx_head_stride ? dst.idx_head_stride : (int64_t)nb * kD + 1) + tile0;
    uint16_t* nz = const_cast<uint16_t*>(head_stream(dst, h));
    int c = 0;
    for (int d = 0; d < kD; d++) {
        const uint64_t m = bmp[d];
        uint16_t* tile = nz + 2ull * idx[d];
        if (tile_bit(m, t)) {
            tile[tile_rank(m, t)] = vals[(c >> 1) * 128 + (c & 1)];
            c++;
        }
        const int n = __popcll(m), n8 = (n + 7) & ~7;
        if (n + t < n8) tile[n + t] = 0;   // (at most 7 halfs of padding)
    }
}

bool tile_view_ok(const mustafar_cache_view* v, int tokens)
{
    const int64_t tiles = (int64_t)tokens * 2;
    return v && !v->flags && v->bmp && v->idx && v->nz && (v->nz_head_stride || v->nz_offset) && (!v->bmp_head_stride || v->bmp_head_stride >= tiles) &&
           (!v->idx_head_stride || v->idx_head_stride >= tiles + 1);
}
bool rows_view_ok(const mustafar_cache_view* v, int tokens)
{
    return v && v->flags == MUSTAFAR_VIEW_KEY_ROWS && v->idx && v->nz && v->nz_head_stride > 0 && (v->nz_head_stride & 15) == 0 &&
           v->idx_head_stride >= tokens / 64;
}
bool shape_ok(int Bp, int tokens) { return Bp >= 1 && Bp <= 65535 && tokens > 0 && (tokens & 63) == 0; }

}  // namespace

extern "C" {

int mustafar_key_rows_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_rows)
{
    if (!shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !table || !head_rows) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64;
    key_rows_width_kernel<<<dim3(nb, Bp), 64, 0, st>>>(*src, nb, table);
    key_rows_scan_kernel<<<Bp, 64, 0, st>>>(nb, table, head_rows);
    return (int)hipGetLastError();
}

int mustafar_key_rows_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens)
{
    if (!shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !rows_view_ok(dst, tokens) || dst->idx_head_stride != tokens / 64) return MUSTAFAR_EINVAL;
    const int nb = tokens / 64;
    key_rows_fill_kernel<<<dim3(nb, Bp), 64, 0, static_cast<hipStream_t>(stream)>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

int mustafar_key_rows_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total)
{
    if (!shape_ok(Bp, tokens) || !rows_view_ok(src, tokens) || !tile_view_ok(dst, tokens) || !dst->nz_head_stride) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64;
    key_tiles_bitmap_kernel<<<dim3(nb, Bp), 64, 0, st>>>(*src, *dst, nb);
    key_tiles_scan_kernel<<<Bp, 64, 0, st>>>(*dst, nb, head_total);
    key_tiles_stream_kernel<<<dim3(nb, Bp), 64, 0, st>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

}  // extern "C"
