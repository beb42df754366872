// tile_view.h -- what a mustafar_cache_view (include/mustafar_hip.h) means, once: where a head's bitmaps, offsets and stream start in a
// tile-format view, the bit and rank of a position in a tile's bitmap, and -- on the host -- which views are well formed: the tile view
// of a retile entry point and the base forms.  Plain inline functions, no kernels; the retile passes
// (base_forms.hip) and decode_attention (spmv.hip) hold their views to these rules.
#pragma once
#include <stdint.h>

#include "../../include/mustafar_hip.h"

#if defined(__HIPCC__)
#define TV_FN __host__ __device__ inline
#else
#define TV_FN inline
#endif

constexpr int kBlockTiles = 128;   // tiles per 64-token block at head_dim 128

// head h's bitmaps / offsets of a view of nb blocks: a head stride of 0 stands for rows of exactly 128 nb tiles / 128 nb + 1 offsets
TV_FN uint64_t* tile_bmp(const mustafar_cache_view& v, int h, int nb)
{
    return v.bmp + (int64_t)h * (v.bmp_head_stride ? v.bmp_head_stride : (int64_t)nb * kBlockTiles);
}
TV_FN uint32_t* tile_idx(const mustafar_cache_view& v, int h, int nb)
{
    return v.idx + (int64_t)h * (v.idx_head_stride ? v.idx_head_stride : (int64_t)nb * kBlockTiles + 1);
}
// head h's stream (tiles), rows or blocks (a base form: nz_head_stride != 0)
TV_FN unsigned char* head_bytes(const mustafar_cache_view& v, int h)
{
    const uint64_t start = v.nz_head_stride ? (uint64_t)h * (uint64_t)v.nz_head_stride : (uint64_t)v.nz_offset[h];   // uint4 units
    return static_cast<unsigned char*>(v.nz) + 16ull * start;
}
TV_FN uint16_t* head_stream(const mustafar_cache_view& v, int h) { return reinterpret_cast<uint16_t*>(head_bytes(v, h)); }
// bit of position p (a key tile: token, a value tile: channel of the half) in a tile's bitmap, and the tile's non-zeros in front of it
TV_FN bool tile_bit(uint64_t m, int p) { return (m >> (63 - p)) & 1ull; }
TV_FN int tile_rank(uint64_t m, int p) { return p ? __builtin_popcountll(m >> (64 - p)) : 0; }

// ---- which views are well formed (host).  Every refusal is MUSTAFAR_EINVAL at the caller.
// what every retile entry point takes: Bp heads (a grid's y), whole 64-token blocks
inline bool retile_shape_ok(int Bp, int tokens) { return Bp >= 1 && Bp <= 65535 && tokens > 0 && (tokens & 63) == 0; }
// a tile-format view a retile pass reads or writes
inline bool tile_view_ok(const mustafar_cache_view* v, int tokens)
{
    const int64_t tiles = (int64_t)tokens * 2;
    return v && !v->flags && v->bmp && v->idx && v->nz && (v->nz_head_stride || v->nz_offset) && (!v->bmp_head_stride || v->bmp_head_stride >= tiles) &&
           (!v->idx_head_stride || v->idx_head_stride >= tiles + 1);
}
// a key base in token rows (flag: MUSTAFAR_VIEW_KEY_ROWS, channel bytes; MUSTAFAR_VIEW_KEY_NIBBLE_ROWS, 4-bit channel steps): rows of 256
// bytes = 16 uint4 from the head's start, a table entry per block
inline bool row_view_ok(const mustafar_cache_view* v, int tokens, uint32_t flag)
{
    return v && v->flags == flag && v->idx && v->nz && v->nz_head_stride > 0 && (v->nz_head_stride & 15) == 0 && v->idx_head_stride >= tokens / 64;
}
// a value base in channel lists (flag: MUSTAFAR_VIEW_VALUE_LISTS, a table entry per block; MUSTAFAR_VIEW_VALUE_PAIR_LISTS, two per pair of
// blocks): `columns` table entries, the closing one among them
inline bool list_view_ok(const mustafar_cache_view* v, uint32_t flag, int columns)
{
    return v && v->flags == flag && v->idx && v->nz && v->nz_head_stride > 0 && v->idx_head_stride >= columns;
}
// the four forms by name (decode_attention)
inline bool key_rows_view_ok(const mustafar_cache_view* v, int tokens) { return row_view_ok(v, tokens, MUSTAFAR_VIEW_KEY_ROWS); }
inline bool key_nibble_rows_view_ok(const mustafar_cache_view* v, int tokens) { return row_view_ok(v, tokens, MUSTAFAR_VIEW_KEY_NIBBLE_ROWS); }
inline bool value_lists_view_ok(const mustafar_cache_view* v, int tokens) { return list_view_ok(v, MUSTAFAR_VIEW_VALUE_LISTS, tokens / 64 + 1); }
inline bool value_pair_lists_view_ok(const mustafar_cache_view* v, int tokens)
{
    return list_view_ok(v, MUSTAFAR_VIEW_VALUE_PAIR_LISTS, 2 * ((tokens / 64 + 1) / 2) + 1);
}
