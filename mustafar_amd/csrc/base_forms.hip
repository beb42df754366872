// base_forms.hip -- the retile passes between the tile format of an arena's base and the forms the GQA-4 one-pass super-block launch
// reads instead (include/mustafar_hip.h): token rows of a KEY base (MUSTAFAR_VIEW_KEY_ROWS, ABI 113; arithmetic: key_rows.h),
// sorted channel lists of a VALUE base per block (MUSTAFAR_VIEW_VALUE_LISTS; arithmetic: value_lists.h) or per pair of blocks
// (MUSTAFAR_VIEW_VALUE_PAIR_LISTS; arithmetic: value_pair_lists.h).  head_dim 128 only.
//
//   tiles -> form   mustafar_<form>_plan (a number per block, then the block table by one scan per head) + mustafar_<form>_fill
//   form -> tiles   mustafar_<form>_to_tiles: bitmaps and tile lengths, the offsets of a head by one scan, the streams
//
// A block in tiles is 128 tiles of 64 bits; a tile's non-zeros follow in bitmap order, padded with zeros to a multiple of 8 halfs.
//   key     tile d = channel d of the block's 64 tokens, bit 63 - t = token t.  In rows, lane t holds token t's non-zero channels in
//           ascending order.  One wave per block, lane = token.
//   value   tile 64 half + t = channels 64 half .. + 63 of token t, bit 63 - c = channel c of the half.  In lists, lane rank(c) of a half
//           holds channel c's (token, value) entries in token order.  One wave per block half, lane = channel.
// Both directions of a form walk a lane's entries in order with one running slot counter per lane, so each is the other's inverse element
// by element.  What a view means and which views are well formed is tile_view.h's; the two scans exist once, for both forms.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mustafar_hip.h"
#include "key_nibble_rows.h"
#include "key_rows.h"
#include "tile_view.h"
#include "value_lists.h"
#include "value_pair_lists.h"

namespace {

constexpr int kD = kBlockTiles;

__device__ __forceinline__ int wave_max_i(int v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
// inclusive prefix of x over the 64 lanes
__device__ __forceinline__ uint32_t wave_scan(uint32_t x, int l)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(x, o, 64);
        if (l >= o) x += up;
    }
    return x;
}

// ---- the two scans, one wave per head
// The block table of a form.  The per-block pass left a number per block (a width, a size); F::units(raw) is what the block takes of the
// head's storage, F::entry(start, raw) its table entry; with F::closing the table has an entry nb, the head's units.
struct RowsTable {   // raw = w; units = rows of 256 bytes
    static constexpr int closing = 0;
    static __device__ uint32_t units(uint32_t w) { return (uint32_t)kr_rows((int)w); }
    static __device__ uint32_t entry(uint32_t first_row, uint32_t w) { return kr_entry(first_row, w); }
};
struct NibbleRowsTable {   // raw = w; units = rows of 256 bytes
    static constexpr int closing = 0;
    static __device__ uint32_t units(uint32_t w) { return (uint32_t)nr_rows((int)w); }
    static __device__ uint32_t entry(uint32_t first_row, uint32_t w) { return nr_entry(first_row, w); }
};
struct ListsTable {   // raw = units = the block's dwords; an entry is the block's start
    static constexpr int closing = 1;
    static __device__ uint32_t units(uint32_t n) { return n; }
    static __device__ uint32_t entry(uint32_t start, uint32_t) { return start; }
};
template <class F>
__global__ __launch_bounds__(64) void block_table_scan_kernel(int nb, uint32_t* __restrict__ table, int64_t* __restrict__ head_units)
{
    const int h = blockIdx.x, l = threadIdx.x;
    uint32_t* tab = table + (int64_t)h * (nb + F::closing);
    uint32_t run = 0;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int b = b0 + l;
        const uint32_t raw = b < nb ? tab[b] : 0u;
        const uint32_t n = b < nb ? F::units(raw) : 0u;
        const uint32_t inc = wave_scan(n, l);
        if (b < nb) tab[b] = F::entry(run + inc - n, raw);
        run += __shfl(inc, 63, 64);
    }
    if (l == 0) {
        if (F::closing) tab[nb] = run;
        head_units[h] = (int64_t)run;
    }
}

// The way back, both forms: the tile lengths in dst.idx[h][tile + 1] -> offsets (exclusive prefix, idx[h][0] = 0), the head's stream
// length in halfs.
__global__ __launch_bounds__(64) void tile_offsets_scan_kernel(mustafar_cache_view dst, int nb, int64_t* __restrict__ head_total)
{
    const int h = blockIdx.x, l = threadIdx.x;
    const int64_t tiles = (int64_t)nb * kD;
    uint32_t* idx = tile_idx(dst, h, nb);
    uint32_t run = 0;
    if (l == 0) idx[0] = 0u;
    for (int64_t i0 = 0; i0 < tiles; i0 += 64) {   // (tiles % 64 == 0)
        const uint32_t inc = wave_scan(idx[i0 + l + 1], l);
        idx[i0 + l + 1] = run + inc;
        run += __shfl(inc, 63, 64);
    }
    if (l == 0 && head_total) head_total[h] = 2ll * run;
}
// a tile of n non-zeros takes n rounded up to 8 halfs of the stream: its length in half2 units
__device__ __forceinline__ uint32_t tile_length(uint64_t m) { return (uint32_t)(((__popcll(m) + 7) & ~7) >> 1); }

__device__ __forceinline__ uint32_t table_entry(const mustafar_cache_view& v, int h, int b) { return v.idx[(int64_t)h * v.idx_head_stride + b]; }

// ================================================================ key: tiles <-> token rows
__device__ __forceinline__ unsigned char* key_block(const mustafar_cache_view& v, int h, uint32_t ent)
{
    return head_bytes(v, h) + (uint64_t)kKrRowBytes * kr_first_row(ent);
}
__device__ __forceinline__ uint16_t& key_value(unsigned char* blk, int w, int t, int c) { return *reinterpret_cast<uint16_t*>(blk + kr_value_byte(w, t, c)); }

// One wave per (block, head): the width of the block -> table[h][b] (the scan turns it into a table entry).
__global__ __launch_bounds__(64) void key_rows_width_kernel(mustafar_cache_view src, int nb, uint32_t* __restrict__ table)
{
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const uint64_t* bmp = tile_bmp(src, h, nb) + (int64_t)b * kD;
    int n = 0;
    for (int d = 0; d < kD; d++) n += tile_bit(bmp[d], t);
    const int w = max(2, (wave_max_i(n) + 1) & ~1);
    if (t == 0) table[(int64_t)h * nb + b] = (uint32_t)w;
}

// One wave per (block, head), lane = token: the rows of the block.
__global__ __launch_bounds__(64) void key_rows_fill_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const int64_t tile0 = (int64_t)b * kD;
    const uint64_t* bmp = tile_bmp(src, h, nb) + tile0;
    const uint32_t* idx = tile_idx(src, h, nb) + tile0;
    const uint16_t* nz = head_stream(src, h);
    const uint32_t ent = table_entry(dst, h, b);
    const int w = kr_width(ent);
    unsigned char* blk = key_block(dst, h, ent);
    int c = 0;
    for (int d = 0; d < kD; d++) {
        const uint64_t m = bmp[d];
        if (tile_bit(m, t)) {
            key_value(blk, w, t, c) = nz[2ull * idx[d] + tile_rank(m, t)];
            blk[kr_chan_byte(t, c)] = (unsigned char)d;
            c++;
        }
    }
    for (int p = c; p < 2 * (w >> 1); p++) key_value(blk, w, t, p) = 0;
    for (int p = c; p < 4 * kr_words(w); p++) blk[kr_chan_byte(t, p)] = 0;
}

// One wave per (block, head): the 128 bitmaps of the block and every tile's length -> dst.idx[h][tile + 1].
__global__ __launch_bounds__(64) void key_tiles_bitmap_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ unsigned long long bits[kD];
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    bits[t] = 0ull;
    bits[t + 64] = 0ull;
    __syncthreads();
    const uint32_t ent = table_entry(src, h, b);
    const int w = kr_width(ent);
    unsigned char* blk = key_block(src, h, ent);
    for (int c = 0; c < w; c++) {
        if ((key_value(blk, w, t, c) & 0x7fffu) == 0) break;   // the slots behind a token's non-zeros hold +0
        atomicOr(&bits[blk[kr_chan_byte(t, c)] & (kD - 1)], 1ull << (63 - t));   // (& 127: a channel byte is below 128)
    }
    __syncthreads();
    const int64_t tile0 = (int64_t)b * kD;
    uint64_t* bmp = tile_bmp(dst, h, nb) + tile0;
    uint32_t* idx = tile_idx(dst, h, nb) + tile0;
    for (int d = t; d < kD; d += 64) {
        const uint64_t m = bits[d];
        bmp[d] = m;
        idx[d + 1] = tile_length(m);
    }
}

// One wave per (block, head), lane = token: the streams of the block's 128 tiles, padding included.
__global__ __launch_bounds__(64) void key_tiles_stream_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const uint32_t ent = table_entry(src, h, b);
    const int w = kr_width(ent);
    unsigned char* blk = key_block(src, h, ent);
    const int64_t tile0 = (int64_t)b * kD;
    const uint64_t* bmp = tile_bmp(dst, h, nb) + tile0;
    const uint32_t* idx = tile_idx(dst, h, nb) + tile0;
    uint16_t* nz = head_stream(dst, h);
    int c = 0;
    for (int d = 0; d < kD; d++) {
        const uint64_t m = bmp[d];
        uint16_t* tile = nz + 2ull * idx[d];
        if (tile_bit(m, t)) {
            tile[tile_rank(m, t)] = key_value(blk, w, t, c);
            c++;
        }
        const int n = __popcll(m), n8 = (n + 7) & ~7;
        if (n + t < n8) tile[n + t] = 0;   // (at most 7 halfs of padding)
    }
}

// ================================================================ key: tiles <-> nibble rows (key_nibble_rows.h)
// lane t's kept channels of a block in tiles
__device__ __forceinline__ NrMask nibble_mask(const uint64_t* __restrict__ bmp, int t)
{
    NrMask m{0ull, 0ull};
    for (int d = 0; d < 64; d++) {
        m.lo |= (uint64_t)tile_bit(bmp[d], t) << d;
        m.hi |= (uint64_t)tile_bit(bmp[64 + d], t) << d;
    }
    return m;
}
// One share of one token, written slot by slot: steps gathered in a dword per step row, values stored as they come.
struct NibbleShareWriter {
    unsigned char* share;   // the share's first row
    int n, t, s;            // its slots, the token, the next slot
    uint32_t word;
    __device__ void put(int step, uint16_t value)
    {
        if (s >= n) return;   // (a chain never outgrows the width the plan pass gave its block)
        word |= (uint32_t)step << nr_step_shift(s);
        *reinterpret_cast<uint16_t*>(share + nr_value_byte(n, t, s)) = value;
        if ((s & 7) == 7) flush();
        s++;
    }
    __device__ void flush()
    {
        *reinterpret_cast<uint32_t*>(share + nr_step_dword_byte(t, s)) = word;
        word = 0u;
    }
    __device__ void gap(int g, uint16_t value)   // the spacers of a gap of g channels, then its entry
    {
        for (; g > kNrSpacerStep; g -= kNrSpacerStep) put(kNrSpacer, 0);
        put(g, value);
    }
    __device__ void pad()   // the slots behind the last entry: step 0, value +0
    {
        while (s < n) put(0, 0);
        if (s & 7) flush();
    }
};

// One wave per (block, head): the width of the block -> table[h][b] (the scan turns it into a table entry).
__global__ __launch_bounds__(64) void key_nibble_rows_width_kernel(mustafar_cache_view src, int nb, uint32_t* __restrict__ table)
{
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const NrMask m = nibble_mask(tile_bmp(src, h, nb) + (int64_t)b * kD, t);
    const int w = wave_max_i(nr_token_width(m, nr_count(m)));
    if (t == 0) table[(int64_t)h * nb + b] = (uint32_t)w;
}

// One wave per (block, head), lane = token: the two shares of the block.
__global__ __launch_bounds__(64) void key_nibble_rows_fill_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const int64_t tile0 = (int64_t)b * kD;
    const uint64_t* bmp = tile_bmp(src, h, nb) + tile0;
    const uint32_t* idx = tile_idx(src, h, nb) + tile0;
    const uint16_t* nz = head_stream(src, h);
    const uint32_t ent = table_entry(dst, h, b);
    const int w = nr_width(ent);
    unsigned char* blk = head_bytes(dst, h) + (uint64_t)kNrRowBytes * nr_first_row(ent);
    const NrMask m = nibble_mask(bmp, t);
    const int last = nr_front_last(m, nr_front(w));
    auto value = [&](int d) { return nz[2ull * idx[d] + tile_rank(bmp[d], t)]; };
    NibbleShareWriter front{blk, nr_front(w), t, 0, 0u};
    for (int d = 0, prev = -1; d <= last; d++) {
        if (nr_kept(m, d)) {
            front.gap(d - prev, value(d));
            prev = d;
        }
    }
    front.pad();
    NibbleShareWriter back{blk + kNrRowBytes * nr_share_first(w, 1), nr_back(w), t, 0, 0u};
    for (int d = 127, prev = 128; d > last; d--) {
        if (nr_kept(m, d)) {
            back.gap(prev - d, value(d));
            prev = d;
        }
    }
    back.pad();
}

// The entries of token t of a block in nibble rows, front chain then back chain: f(channel, value)
template <class F>
__device__ __forceinline__ void nibble_entries(const unsigned char* blk, int w, int t, const F& f)
{
    for (int part = 0; part < 2; part++) {
        const unsigned char* share = blk + kNrRowBytes * nr_share_first(w, part);
        const int n = nr_share_slots(w, part);
        int pos = part ? 128 : -1;
        for (int s = 0; s < n; s++) {
            const int step = (*reinterpret_cast<const uint32_t*>(share + nr_step_dword_byte(t, s)) >> nr_step_shift(s)) & 15;
            if (!step) break;   // (padding: nothing behind it)
            pos += part ? -nr_advance(step) : nr_advance(step);
            if (step != kNrSpacer) f(pos & (kD - 1), *reinterpret_cast<const uint16_t*>(share + nr_value_byte(n, t, s)));   // (& 127: an entry lies in 0 .. 127)
        }
    }
}

// One wave per (block, head): the 128 bitmaps of the block and every tile's length -> dst.idx[h][tile + 1].
__global__ __launch_bounds__(64) void key_nibble_tiles_bitmap_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ unsigned long long bits[kD];
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    bits[t] = 0ull;
    bits[t + 64] = 0ull;
    __syncthreads();
    const uint32_t ent = table_entry(src, h, b);
    const unsigned char* blk = head_bytes(src, h) + (uint64_t)kNrRowBytes * nr_first_row(ent);
    nibble_entries(blk, nr_width(ent), t, [&](int d, uint16_t) { atomicOr(&bits[d], 1ull << (63 - t)); });
    __syncthreads();
    const int64_t tile0 = (int64_t)b * kD;
    uint64_t* bmp = tile_bmp(dst, h, nb) + tile0;
    uint32_t* idx = tile_idx(dst, h, nb) + tile0;
    for (int d = t; d < kD; d += 64) {
        const uint64_t m = bits[d];
        bmp[d] = m;
        idx[d + 1] = tile_length(m);
    }
}

// One wave per (block, head), lane = token: the streams of the block's 128 tiles, padding included.
__global__ __launch_bounds__(64) void key_nibble_tiles_stream_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const uint32_t ent = table_entry(src, h, b);
    const unsigned char* blk = head_bytes(src, h) + (uint64_t)kNrRowBytes * nr_first_row(ent);
    const int64_t tile0 = (int64_t)b * kD;
    const uint64_t* bmp = tile_bmp(dst, h, nb) + tile0;
    const uint32_t* idx = tile_idx(dst, h, nb) + tile0;
    uint16_t* nz = head_stream(dst, h);
    nibble_entries(blk, nr_width(ent), t, [&](int d, uint16_t v) { nz[2ull * idx[d] + tile_rank(bmp[d], t)] = v; });
    for (int d = 0; d < kD; d++) {
        const int n = __popcll(bmp[d]), n8 = (n + 7) & ~7;
        if (n + t < n8) nz[2ull * idx[d] + n + t] = 0;   // (at most 7 halfs of padding)
    }
}

// ================================================================ value: tiles <-> sorted channel lists
__device__ __forceinline__ unsigned char* list_block(const mustafar_cache_view& v, int h, int b) { return head_bytes(v, h) + 4ull * table_entry(v, h, b); }

// The lists of one half (64 tiles at bmp), lane = channel c: cnt, the lane the channel's list lives in, and the row widths m[0..31] in LDS.
struct HalfPlan {
    int cnt, rank;
};
__device__ __forceinline__ HalfPlan half_plan(const uint64_t* __restrict__ bmp, int c, unsigned char* m)
{
    HalfPlan p{0, 0};
    for (int t = 0; t < 64; t++) p.cnt += tile_bit(bmp[t], c);
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

// One wave per (block, head): the block's size in dwords -> table[h][b] (the scan turns it into the block's start).
__global__ __launch_bounds__(64) void value_lists_size_kernel(mustafar_cache_view src, int nb, uint32_t* __restrict__ table)
{
    __shared__ unsigned char m[2][kVlMaxRows];
    const int b = blockIdx.x, h = blockIdx.y, c = threadIdx.x;
    const uint64_t* bmp = tile_bmp(src, h, nb) + (int64_t)b * kD;
    half_plan(bmp, c, m[0]);
    half_plan(bmp + 64, c, m[1]);
    if (c == 0) table[(int64_t)h * (nb + 1) + b] = (uint32_t)vl_block_dwords(vl_word_offset(m[0], kVlMaxWords), vl_word_offset(m[1], kVlMaxWords));
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
        if (tile_bit(bits, c)) {
            const int w = woff[s >> 2];
            base[vl_token_byte(w, i, s)] = (unsigned char)t;
            *reinterpret_cast<uint16_t*>(base + vl_value_byte(m, w, i, s)) = nz[2ull * idx[t] + tile_rank(bits, c)];
            s++;
        }
    }
    if (s & 1) *reinterpret_cast<uint16_t*>(base + vl_value_byte(m, woff[s >> 2], i, s)) = 0;
    for (int q = s; q < vl_token_slots(s); q++) base[vl_token_byte(woff[q >> 2], i, q)] = 0;
}

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

// One wave per (block half, head): the 64 bitmaps of the half and every tile's length -> dst.idx[h][tile + 1].
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
    const uint64_t mt = bits[i];
    tile_bmp(dst, h, nb)[tile0 + i] = mt;
    tile_idx(dst, h, nb)[tile0 + i + 1] = tile_length(mt);
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
    uint16_t* nz = head_stream(dst, h);
    for (int s = 0;; s++) {
        const int t = list_token(L, woff, i, s);
        if (t < 0) break;
        nz[2ull * idx[t] + tile_rank(bmp[t], L.chan)] = *reinterpret_cast<const uint16_t*>(L.base + vl_value_byte(L.m, woff[s >> 2], i, s));
    }
    const int n = __popcll(bmp[i]), n8 = (n + 7) & ~7;   // lane = token: its tile's padding
    for (int p = n; p < n8; p++) nz[2ull * idx[i] + p] = 0;
}

// ================================================================ value: tiles <-> sorted channel lists over pairs of blocks
// Pair p of a head = blocks 2p, 2p + 1 (the last pair of an odd base: block 2p alone); token u of the pair = token u & 63 of block
// 2p + (u >> 6).  The block table has two entries per pair (its header, its half 1) and the closing one: value_pair_lists.h.
__device__ __forceinline__ int pair_tokens(int nb, int p) { return 64 * vpl_pair_blocks(nb, p); }
// tile of token u of a pair, counted from the tile of the pair's token 0 in the same half
__device__ __forceinline__ int pair_tile(int u) { return (u >> 6) * kD + (u & 63); }

// half_plan over a pair's ntok tokens (bmp: the half's tile of the pair's token 0): the row widths m[0..63] in LDS
__device__ __forceinline__ HalfPlan pair_half_plan(const uint64_t* __restrict__ bmp, int ntok, int c, unsigned char* m)
{
    HalfPlan p{0, 0};
    for (int u = 0; u < ntok; u++) p.cnt += tile_bit(bmp[pair_tile(u)], c);
    for (int o = 0; o < 64; o++) {
        const int other = __shfl(p.cnt, o, 64);
        p.rank += other > p.cnt || (other == p.cnt && o < c);
    }
    for (int r = 0; r < kVplMaxRows; r++) {
        const int w = __popcll(__ballot(p.cnt > 2 * r));
        if (c == 0) m[r] = (unsigned char)w;
    }
    __syncthreads();
    return p;
}

// One wave per (pair, head): the dwords of the pair's two table entries -> table[h][2p], [2p + 1] (the scan turns them into starts).
__global__ __launch_bounds__(64) void value_pair_lists_size_kernel(mustafar_cache_view src, int nb, uint32_t* __restrict__ table)
{
    __shared__ unsigned char m[2][kVplMaxRows];
    const int p = blockIdx.x, h = blockIdx.y, c = threadIdx.x;
    const uint64_t* bmp = tile_bmp(src, h, nb) + (int64_t)(2 * p) * kD;
    const int ntok = pair_tokens(nb, p);
    pair_half_plan(bmp, ntok, c, m[0]);
    pair_half_plan(bmp + 64, ntok, c, m[1]);
    if (c == 0) {
        const int half0 = vpl_word_offset(m[0], kVplMaxWords), half1 = vpl_word_offset(m[1], kVplMaxWords);
        uint32_t* tab = table + (int64_t)h * vpl_table_columns(nb) + 2 * p;
        tab[0] = (uint32_t)vpl_front_dwords(half0);
        tab[1] = (uint32_t)vpl_back_dwords(half0, half1);
    }
}

// where a pair's header and the words of one of its halves start
__device__ __forceinline__ unsigned char* pair_header(const mustafar_cache_view& v, int h, int p) { return head_bytes(v, h) + 4ull * table_entry(v, h, 2 * p); }
__device__ __forceinline__ unsigned char* pair_half(const mustafar_cache_view& v, int h, int p, int half)
{
    return head_bytes(v, h) + 4ull * (half ? table_entry(v, h, 2 * p + 1) : table_entry(v, h, 2 * p) + kVplHeaderDwords);
}

// One wave per (pair half, head), lane = channel: the half's part of the header and its words.
__global__ __launch_bounds__(64) void value_pair_lists_fill_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ unsigned char m[kVplMaxRows];
    __shared__ int woff[kVplMaxWords + 1];
    const int p = blockIdx.x >> 1, half = blockIdx.x & 1, h = blockIdx.y, c = threadIdx.x;
    const int64_t tile0 = (int64_t)(2 * p) * kD + half * 64;
    const uint64_t* bmp = tile_bmp(src, h, nb) + tile0;
    const uint32_t* idx = tile_idx(src, h, nb) + tile0;
    const uint16_t* nz = head_stream(src, h);
    const int ntok = pair_tokens(nb, p);
    const HalfPlan pl = pair_half_plan(bmp, ntok, c, m);
    if (c <= kVplMaxWords) woff[c] = vpl_word_offset(m, c);
    __syncthreads();
    unsigned char* hdr = pair_header(dst, h, p);
    hdr[kVplPermByte + half * 64 + pl.rank] = (unsigned char)c;
    hdr[kVplWidthByte + half * kVplMaxRows + c] = m[c];
    unsigned char* base = pair_half(dst, h, p, half);
    if (half) {   // the zeros between this pair and the next (at most three dwords)
        const uint32_t used = table_entry(dst, h, 2 * p + 1) + (uint32_t)woff[kVplMaxWords], end = table_entry(dst, h, 2 * p + 2);
        if (used + c < end) reinterpret_cast<uint32_t*>(head_bytes(dst, h))[used + c] = 0u;
    }
    const int i = pl.rank;
    int s = 0;
    for (int u = 0; u < ntok; u++) {
        const int tl = pair_tile(u);
        const uint64_t bits = bmp[tl];
        if (tile_bit(bits, c)) {
            const int w = woff[s >> 2];
            base[vpl_token_byte(w, i, s)] = (unsigned char)u;
            *reinterpret_cast<uint16_t*>(base + vpl_value_byte(m, w, i, s)) = nz[2ull * idx[tl] + tile_rank(bits, c)];
            s++;
        }
    }
    if (s & 1) *reinterpret_cast<uint16_t*>(base + vpl_value_byte(m, woff[s >> 2], i, s)) = 0;
    for (int q = s; q < vpl_token_slots(s); q++) base[vpl_token_byte(woff[q >> 2], i, q)] = 0;
}

// A lane's entries, as HalfLists: slot s of lane i is an entry if the lane takes part in its rows and s == 0 or its token is not 0.
__device__ __forceinline__ HalfLists pair_half_lists(const mustafar_cache_view& v, int h, int p, int half, int i, int* woff)
{
    const unsigned char* hdr = pair_header(v, h, p);
    HalfLists L;
    L.m = hdr + kVplWidthByte + half * kVplMaxRows;
    L.base = pair_half(v, h, p, half);
    L.chan = hdr[kVplPermByte + half * 64 + i] & 63;
    if (i <= kVplMaxWords) woff[i] = vpl_word_offset(L.m, i);
    __syncthreads();
    return L;
}
// token of slot s of lane i (below ntok, a power of two), or -1 behind the lane's last entry
__device__ __forceinline__ int pair_list_token(const HalfLists& L, const int* woff, int i, int s, int ntok)
{
    if (s >= 2 * kVplMaxRows || i >= L.m[s >> 1]) return -1;
    const int t = L.base[vpl_token_byte(woff[s >> 2], i, s)];
    return (s == 0 || t != 0) ? (t & (ntok - 1)) : -1;
}

// One wave per (pair half, head): the bitmaps of the half's tiles and every tile's length -> dst.idx[h][tile + 1].
__global__ __launch_bounds__(64) void value_pair_tiles_bitmap_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ unsigned long long bits[128];
    __shared__ int woff[kVplMaxWords + 1];
    const int p = blockIdx.x >> 1, half = blockIdx.x & 1, h = blockIdx.y, i = threadIdx.x;
    const int ntok = pair_tokens(nb, p);
    bits[i] = 0ull;
    bits[i + 64] = 0ull;
    const HalfLists L = pair_half_lists(src, h, p, half, i, woff);
    for (int s = 0;; s++) {
        const int t = pair_list_token(L, woff, i, s, ntok);
        if (t < 0) break;
        atomicOr(&bits[t], 1ull << (63 - L.chan));
    }
    __syncthreads();
    const int64_t tile0 = (int64_t)(2 * p) * kD + half * 64;
    for (int u = i; u < ntok; u += 64) {
        const uint64_t mt = bits[u];
        tile_bmp(dst, h, nb)[tile0 + pair_tile(u)] = mt;
        tile_idx(dst, h, nb)[tile0 + pair_tile(u) + 1] = tile_length(mt);
    }
}

// One wave per (pair half, head): the streams of the half's tiles, padding included.
__global__ __launch_bounds__(64) void value_pair_tiles_stream_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ int woff[kVplMaxWords + 1];
    const int p = blockIdx.x >> 1, half = blockIdx.x & 1, h = blockIdx.y, i = threadIdx.x;
    const int ntok = pair_tokens(nb, p);
    const HalfLists L = pair_half_lists(src, h, p, half, i, woff);
    const int64_t tile0 = (int64_t)(2 * p) * kD + half * 64;
    const uint64_t* bmp = tile_bmp(dst, h, nb) + tile0;
    const uint32_t* idx = tile_idx(dst, h, nb) + tile0;
    uint16_t* nz = head_stream(dst, h);
    for (int s = 0;; s++) {
        const int t = pair_list_token(L, woff, i, s, ntok);
        if (t < 0) break;
        const int tl = pair_tile(t);
        nz[2ull * idx[tl] + tile_rank(bmp[tl], L.chan)] = *reinterpret_cast<const uint16_t*>(L.base + vpl_value_byte(L.m, woff[s >> 2], i, s));
    }
    for (int u = i; u < ntok; u += 64) {   // lane = token: its tiles' padding
        const int tl = pair_tile(u);
        const int n = __popcll(bmp[tl]), n8 = (n + 7) & ~7;
        for (int q = n; q < n8; q++) nz[2ull * idx[tl] + q] = 0;
    }
}

}  // namespace

// ================================================================ the entry points (include/mustafar_hip.h); every refusal is tile_view.h's
extern "C" {

int mustafar_key_rows_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_rows)
{
    if (!retile_shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !table || !head_rows) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64;
    key_rows_width_kernel<<<dim3(nb, Bp), 64, 0, st>>>(*src, nb, table);
    block_table_scan_kernel<RowsTable><<<Bp, 64, 0, st>>>(nb, table, head_rows);
    return (int)hipGetLastError();
}

int mustafar_key_rows_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens)
{
    if (!retile_shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !key_rows_view_ok(dst, tokens) || dst->idx_head_stride != tokens / 64) return MUSTAFAR_EINVAL;
    const int nb = tokens / 64;
    key_rows_fill_kernel<<<dim3(nb, Bp), 64, 0, static_cast<hipStream_t>(stream)>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

int mustafar_key_rows_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total)
{
    if (!retile_shape_ok(Bp, tokens) || !key_rows_view_ok(src, tokens) || !tile_view_ok(dst, tokens) || !dst->nz_head_stride) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64;
    key_tiles_bitmap_kernel<<<dim3(nb, Bp), 64, 0, st>>>(*src, *dst, nb);
    tile_offsets_scan_kernel<<<Bp, 64, 0, st>>>(*dst, nb, head_total);
    key_tiles_stream_kernel<<<dim3(nb, Bp), 64, 0, st>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

int mustafar_key_nibble_rows_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_rows)
{
    if (!retile_shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !table || !head_rows) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64;
    key_nibble_rows_width_kernel<<<dim3(nb, Bp), 64, 0, st>>>(*src, nb, table);
    block_table_scan_kernel<NibbleRowsTable><<<Bp, 64, 0, st>>>(nb, table, head_rows);
    return (int)hipGetLastError();
}

int mustafar_key_nibble_rows_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens)
{
    if (!retile_shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !key_nibble_rows_view_ok(dst, tokens) || dst->idx_head_stride != tokens / 64)
        return MUSTAFAR_EINVAL;
    const int nb = tokens / 64;
    key_nibble_rows_fill_kernel<<<dim3(nb, Bp), 64, 0, static_cast<hipStream_t>(stream)>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

int mustafar_key_nibble_rows_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total)
{
    if (!retile_shape_ok(Bp, tokens) || !key_nibble_rows_view_ok(src, tokens) || !tile_view_ok(dst, tokens) || !dst->nz_head_stride) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64;
    key_nibble_tiles_bitmap_kernel<<<dim3(nb, Bp), 64, 0, st>>>(*src, *dst, nb);
    tile_offsets_scan_kernel<<<Bp, 64, 0, st>>>(*dst, nb, head_total);
    key_nibble_tiles_stream_kernel<<<dim3(nb, Bp), 64, 0, st>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

int mustafar_value_lists_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_dwords)
{
    if (!retile_shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !table || !head_dwords) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64;
    value_lists_size_kernel<<<dim3(nb, Bp), 64, 0, st>>>(*src, nb, table);
    block_table_scan_kernel<ListsTable><<<Bp, 64, 0, st>>>(nb, table, head_dwords);
    return (int)hipGetLastError();
}

int mustafar_value_lists_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens)
{
    if (!retile_shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !value_lists_view_ok(dst, tokens) || dst->idx_head_stride != tokens / 64 + 1) return MUSTAFAR_EINVAL;
    const int nb = tokens / 64;
    value_lists_fill_kernel<<<dim3(2 * nb, Bp), 64, 0, static_cast<hipStream_t>(stream)>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

int mustafar_value_lists_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total)
{
    if (!retile_shape_ok(Bp, tokens) || !value_lists_view_ok(src, tokens) || !tile_view_ok(dst, tokens) || !dst->nz_head_stride) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64;
    value_tiles_bitmap_kernel<<<dim3(2 * nb, Bp), 64, 0, st>>>(*src, *dst, nb);
    tile_offsets_scan_kernel<<<Bp, 64, 0, st>>>(*dst, nb, head_total);
    value_tiles_stream_kernel<<<dim3(2 * nb, Bp), 64, 0, st>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

int mustafar_value_pair_lists_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_dwords)
{
    if (!retile_shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !table || !head_dwords) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64, np = vpl_pairs(nb);
    value_pair_lists_size_kernel<<<dim3(np, Bp), 64, 0, st>>>(*src, nb, table);
    block_table_scan_kernel<ListsTable><<<Bp, 64, 0, st>>>(2 * np, table, head_dwords);   // (two entries per pair)
    return (int)hipGetLastError();
}

int mustafar_value_pair_lists_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens)
{
    if (!retile_shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !value_pair_lists_view_ok(dst, tokens) ||
        dst->idx_head_stride != vpl_table_columns(tokens / 64))
        return MUSTAFAR_EINVAL;
    const int nb = tokens / 64;
    value_pair_lists_fill_kernel<<<dim3(2 * vpl_pairs(nb), Bp), 64, 0, static_cast<hipStream_t>(stream)>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

int mustafar_value_pair_lists_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total)
{
    if (!retile_shape_ok(Bp, tokens) || !value_pair_lists_view_ok(src, tokens) || !tile_view_ok(dst, tokens) || !dst->nz_head_stride) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64, np = vpl_pairs(nb);
    value_pair_tiles_bitmap_kernel<<<dim3(2 * np, Bp), 64, 0, st>>>(*src, *dst, nb);
    tile_offsets_scan_kernel<<<Bp, 64, 0, st>>>(*dst, nb, head_total);
    value_pair_tiles_stream_kernel<<<dim3(2 * np, Bp), 64, 0, st>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

}  // extern "C"
