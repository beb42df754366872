// base_forms.hip -- the retile passes between the tile format of an arena's base and the forms the GQA-4 one-pass super-block launch
// reads instead (include/mustafar_hip.h): token rows of a KEY base (MUSTAFAR_VIEW_KEY_ROWS, ABI 113; arithmetic: key_rows.h),
// sorted channel lists of a VALUE base per block (MUSTAFAR_VIEW_VALUE_LISTS; arithmetic: value_lists.h) or per pair of blocks
// (MUSTAFAR_VIEW_VALUE_PAIR_LISTS; arithmetic: value_pair_lists.h); token rows with 4-bit channel steps (MUSTAFAR_VIEW_KEY_NIBBLE_ROWS;
// arithmetic: key_nibble_rows.h).  head_dim 128 only.
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
// by element.  What a view means and which views are well formed is tile_view.h's.  What exists once here: the two scans; the bitmap pass
// of the row forms, over a form's visitor of a token's entries (ByteRows, NibbleRows); all four passes of the list forms, over a form's
// geometry (BlockLists, PairLists); the three entry points, over a form's description (RowForm, ListForm).
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
// head's storage, F::entry(start, raw) its table entry; with F::closing the table has an entry nb, the head's units.  The row forms
// (ByteRows, NibbleRows below) are their own table: raw = w, units = rows of 256 bytes.
struct ListsTable {   // raw = units = the dwords of a table entry; an entry is its start
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
// A row form is the table of its blocks (block_table_scan_kernel: raw = w, units = rows of 256 bytes) and a visitor of the entries token t
// holds in the block of table entry ent, in the form's order: f(channel, value).  The bitmap pass of the way back is written over the
// visitor, once; the width, fill and stream passes are the form's own.
__device__ __forceinline__ unsigned char* key_block(const mustafar_cache_view& v, int h, uint32_t ent)
{
    return head_bytes(v, h) + (uint64_t)kKrRowBytes * kr_first_row(ent);
}
__device__ __forceinline__ uint16_t& key_value(unsigned char* blk, int w, int t, int c) { return *reinterpret_cast<uint16_t*>(blk + kr_value_byte(w, t, c)); }

struct ByteRows {   // key_rows.h
    static constexpr uint32_t flag = MUSTAFAR_VIEW_KEY_ROWS;
    static constexpr int closing = 0;
    static __device__ uint32_t units(uint32_t w) { return (uint32_t)kr_rows((int)w); }
    static __device__ uint32_t entry(uint32_t first_row, uint32_t w) { return kr_entry(first_row, w); }
    template <class F>
    static __device__ __forceinline__ void entries(const mustafar_cache_view& v, int h, uint32_t ent, int t, const F& f)
    {
        const int w = kr_width(ent);
        unsigned char* blk = key_block(v, h, ent);
        for (int c = 0; c < w; c++) {
            const uint16_t value = key_value(blk, w, t, c);
            if ((value & 0x7fffu) == 0) break;              // the slots behind a token's non-zeros hold +0
            f(blk[kr_chan_byte(t, c)] & (kD - 1), value);   // (& 127: a channel byte is below 128)
        }
    }
};
struct NibbleRows {   // key_nibble_rows.h: front chain, then back chain
    static constexpr uint32_t flag = MUSTAFAR_VIEW_KEY_NIBBLE_ROWS;
    static constexpr int closing = 0;
    static __device__ uint32_t units(uint32_t w) { return (uint32_t)nr_rows((int)w); }
    static __device__ uint32_t entry(uint32_t first_row, uint32_t w) { return nr_entry(first_row, w); }
    template <class F>
    static __device__ __forceinline__ void entries(const mustafar_cache_view& v, int h, uint32_t ent, int t, const F& f)
    {
        const int w = nr_width(ent);
        const unsigned char* blk = head_bytes(v, h) + (uint64_t)kNrRowBytes * nr_first_row(ent);
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
};

// One wave per (block, head): the 128 bitmaps of the block and every tile's length -> dst.idx[h][tile + 1].
template <class R>
__global__ __launch_bounds__(64) void key_tiles_bitmap_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ unsigned long long bits[kD];
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    bits[t] = 0ull;
    bits[t + 64] = 0ull;
    __syncthreads();
    R::entries(src, h, table_entry(src, h, b), t, [&](int d, uint16_t) { atomicOr(&bits[d], 1ull << (63 - t)); });
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

// One wave per (block, head), lane = token: the streams of the block's 128 tiles, padding included.  The stream pass is the form's own.
// Nibble rows scatter what the visitor gives.  Rows with channel bytes hold a token's entries in channel order, so slot c belongs to the
// token's c-th tile and the pass walks the tiles instead, with bmp[d] and idx[d] the same for the whole wave: 81 us for a c3 layer, where
// the same pass over the visitor took 140 us (profiles/r13_base_form_templates.txt).
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
__global__ __launch_bounds__(64) void key_nibble_tiles_stream_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const int64_t tile0 = (int64_t)b * kD;
    const uint64_t* bmp = tile_bmp(dst, h, nb) + tile0;
    const uint32_t* idx = tile_idx(dst, h, nb) + tile0;
    uint16_t* nz = head_stream(dst, h);
    NibbleRows::entries(src, h, table_entry(src, h, b), t, [&](int d, uint16_t v) { nz[2ull * idx[d] + tile_rank(bmp[d], t)] = v; });
    for (int d = 0; d < kD; d++) {
        const int n = __popcll(bmp[d]), n8 = (n + 7) & ~7;
        if (n + t < n8) nz[2ull * idx[d] + n + t] = 0;   // (at most 7 halfs of padding)
    }
}

// ---- tiles -> token rows with channel bytes
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

// ---- tiles -> nibble rows (key_nibble_rows.h)
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

// ================================================================ value: tiles <-> sorted channel lists
// A list form holds the lists of a UNIT of tokens -- a block (value_lists.h) or a pair of blocks (value_pair_lists.h) -- as a 256-byte header,
// half 0 and half 1.  The four passes are written over the form's geometry, once: how many tokens a unit has, how many width rows its
// header, where its header, its half 1 and its end lie (dword offsets from the head's start), which tile token u lands in.  One wave per
// unit half, lane = channel; the size pass one wave per unit.
struct HalfPlan {
    int cnt, rank;
};
// The lists of one half of a unit of ntok tokens (bmp: the half's tile of the unit's token 0), lane = channel c: cnt, the lane the
// channel's list lives in, and the row widths m[0 .. G::kRows) in LDS.
template <class G>
__device__ __forceinline__ HalfPlan half_plan(const uint64_t* __restrict__ bmp, int ntok, int c, unsigned char* m)
{
    HalfPlan p{0, 0};
    for (int u = 0; u < ntok; u++) p.cnt += tile_bit(bmp[G::tile(u)], c);
    for (int o = 0; o < 64; o++) {   // rank by comparison: cnt descending, ties by channel ascending
        const int other = __shfl(p.cnt, o, 64);
        p.rank += other > p.cnt || (other == p.cnt && o < c);
    }
    for (int r = 0; r < G::kRows; r++) {
        const int w = __popcll(__ballot(p.cnt > 2 * r));
        if (c == 0) m[r] = (unsigned char)w;
    }
    __syncthreads();
    return p;
}

struct BlockLists {   // unit u = block u; the table has an entry per block, its start, and the closing one
    static constexpr uint32_t flag = MUSTAFAR_VIEW_VALUE_LISTS;
    static constexpr int kTokens = 64, kRows = kVlMaxRows, kWords = kVlMaxWords;
    static __host__ __device__ int count(int nb) { return nb; }
    static __host__ __device__ int columns(int nb) { return nb + 1; }
    static __device__ int tokens(int, int) { return 64; }
    static __device__ int64_t first_tile(int u) { return (int64_t)u * kD; }
    static __device__ int tile(int t) { return t; }   // of token t of the unit, counted from the tile of its token 0 in the same half
    static __device__ uint32_t header(const mustafar_cache_view& v, int h, int u) { return table_entry(v, h, u); }
    static __device__ uint32_t half1(const mustafar_cache_view&, int, int, const uint32_t* head32, uint32_t hdr)   // (the header holds its offset)
    {
        return hdr + head32[hdr + kVlHalf1Dword];
    }
    static __device__ uint32_t end(const mustafar_cache_view& v, int h, int u) { return table_entry(v, h, u + 1); }
    // half 1 while the unit is being filled: the wave of half 0 has yet to write the header, so the size of half 0 again (bmp0: its tiles)
    static __device__ uint32_t fill_half1(const mustafar_cache_view&, int, int, uint32_t hdr, const uint64_t* bmp0, int c)
    {
        __shared__ unsigned char m0[kRows];
        half_plan<BlockLists>(bmp0, 64, c, m0);
        return hdr + (uint32_t)(kVlHeaderDwords + vl_word_offset(m0, kWords));
    }
    // what the wave of half 0 (mine: its dwords) writes behind the perms and the width rows
    static __device__ void header_rest(uint32_t* hdr32, int c, int mine)
    {
        if (c == 0) hdr32[kVlHalf1Dword] = (uint32_t)(kVlHeaderDwords + mine);
        if (c > 0 && c < kVlHeaderDwords - kVlHalf1Dword) hdr32[kVlHalf1Dword + c] = 0u;
    }
    // what the size pass leaves in the head's table (the scan turns it into starts)
    static __device__ void sizes(uint32_t* tab, int u, int half0, int half1) { tab[u] = (uint32_t)vl_block_dwords(half0, half1); }
};
// Unit p = blocks 2p, 2p + 1 (the last pair of an odd base: block 2p alone); token u of the pair = token u & 63 of block 2p + (u >> 6).  The
// table has two entries per pair (its header, its half 1) and the closing one.
struct PairLists {
    static constexpr uint32_t flag = MUSTAFAR_VIEW_VALUE_PAIR_LISTS;
    static constexpr int kTokens = 128, kRows = kVplMaxRows, kWords = kVplMaxWords;
    static __host__ __device__ int count(int nb) { return vpl_pairs(nb); }
    static __host__ __device__ int columns(int nb) { return vpl_table_columns(nb); }
    static __device__ int tokens(int nb, int p) { return 64 * vpl_pair_blocks(nb, p); }
    static __device__ int64_t first_tile(int p) { return (int64_t)(2 * p) * kD; }
    static __device__ int tile(int u) { return (u >> 6) * kD + (u & 63); }
    static __device__ uint32_t header(const mustafar_cache_view& v, int h, int p) { return table_entry(v, h, 2 * p); }
    static __device__ uint32_t half1(const mustafar_cache_view& v, int h, int p, const uint32_t*, uint32_t) { return table_entry(v, h, 2 * p + 1); }
    static __device__ uint32_t end(const mustafar_cache_view& v, int h, int p) { return table_entry(v, h, 2 * p + 2); }
    static __device__ uint32_t fill_half1(const mustafar_cache_view& v, int h, int p, uint32_t hdr, const uint64_t*, int) { return half1(v, h, p, nullptr, hdr); }
    static __device__ void header_rest(uint32_t*, int, int) {}   // (64 width rows per half: the header is full)
    static __device__ void sizes(uint32_t* tab, int p, int half0, int half1)
    {
        tab[2 * p] = (uint32_t)vpl_front_dwords(half0);
        tab[2 * p + 1] = (uint32_t)vpl_back_dwords(half0, half1);
    }
};

// One wave per (unit, head): what the unit takes, in dwords -> the head's table.
template <class G>
__global__ __launch_bounds__(64) void value_lists_size_kernel(mustafar_cache_view src, int nb, uint32_t* __restrict__ table)
{
    __shared__ unsigned char m[2][G::kRows];
    const int u = blockIdx.x, h = blockIdx.y, c = threadIdx.x;
    const uint64_t* bmp = tile_bmp(src, h, nb) + G::first_tile(u);
    const int ntok = G::tokens(nb, u);
    half_plan<G>(bmp, ntok, c, m[0]);
    half_plan<G>(bmp + 64, ntok, c, m[1]);
    if (c == 0) G::sizes(table + (int64_t)h * G::columns(nb), u, vl_word_offset(m[0], G::kWords), vl_word_offset(m[1], G::kWords));
}

// One wave per (unit half, head), lane = channel: the half's part of the header and its words.
template <class G>
__global__ __launch_bounds__(64) void value_lists_fill_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ unsigned char m[G::kRows];
    __shared__ int woff[G::kWords + 1];
    const int u = blockIdx.x >> 1, half = blockIdx.x & 1, h = blockIdx.y, c = threadIdx.x;
    const int64_t tile0 = G::first_tile(u) + half * 64;
    const uint64_t* bmp = tile_bmp(src, h, nb) + tile0;
    const uint32_t* idx = tile_idx(src, h, nb) + tile0;
    const uint16_t* nz = head_stream(src, h);
    const int ntok = G::tokens(nb, u);
    uint32_t* head32 = reinterpret_cast<uint32_t*>(head_bytes(dst, h));
    const uint32_t hdr = G::header(dst, h, u);
    const uint32_t first = half ? G::fill_half1(dst, h, u, hdr, bmp - 64, c) : hdr + kVlHeaderDwords;   // the half's words
    const HalfPlan p = half_plan<G>(bmp, ntok, c, m);
    if (c <= G::kWords) woff[c] = vl_word_offset(m, c);
    __syncthreads();
    const int mine = woff[G::kWords];
    unsigned char* blk = reinterpret_cast<unsigned char*>(head32 + hdr);
    blk[kVlPermByte + half * 64 + p.rank] = (unsigned char)c;
    if (c < G::kRows) blk[kVlWidthByte + half * G::kRows + c] = m[c];
    if (!half) {
        G::header_rest(head32 + hdr, c, mine);
    } else {   // the zeros between this unit and the next (at most three dwords)
        const uint32_t used = first + (uint32_t)mine, end = G::end(dst, h, u);
        if (used + c < end) head32[used + c] = 0u;
    }
    unsigned char* base = reinterpret_cast<unsigned char*>(head32 + first);
    const int i = p.rank;
    int s = 0;
    for (int t = 0; t < ntok; t++) {
        const int tl = G::tile(t);
        const uint64_t bits = bmp[tl];
        if (tile_bit(bits, c)) {
            const int w = woff[s >> 2];
            base[vl_token_byte(w, i, s)] = (unsigned char)t;
            *reinterpret_cast<uint16_t*>(base + vl_value_byte(m, w, i, s)) = nz[2ull * idx[tl] + tile_rank(bits, c)];
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
template <class G>
__device__ __forceinline__ HalfLists half_lists(const mustafar_cache_view& v, int h, int u, int half, int i, int* woff)
{
    const uint32_t* head32 = reinterpret_cast<const uint32_t*>(head_bytes(v, h));
    const uint32_t hdr = G::header(v, h, u);
    const unsigned char* blk = reinterpret_cast<const unsigned char*>(head32 + hdr);
    HalfLists L;
    L.m = blk + kVlWidthByte + half * G::kRows;
    L.base = reinterpret_cast<const unsigned char*>(head32 + (half ? G::half1(v, h, u, head32, hdr) : hdr + kVlHeaderDwords));
    L.chan = blk[kVlPermByte + half * 64 + i] & 63;
    if (i <= G::kWords) woff[i] = vl_word_offset(L.m, i);
    __syncthreads();
    return L;
}
// token of slot s of lane i (below ntok, a power of two), or -1 behind the lane's last entry
template <class G>
__device__ __forceinline__ int list_token(const HalfLists& L, const int* woff, int i, int s, int ntok)
{
    if (s >= 2 * G::kRows || i >= L.m[s >> 1]) return -1;
    const int t = L.base[vl_token_byte(woff[s >> 2], i, s)];
    return (s == 0 || t != 0) ? (t & (ntok - 1)) : -1;
}

// One wave per (unit half, head): the bitmaps of the half's tiles and every tile's length -> dst.idx[h][tile + 1].
template <class G>
__global__ __launch_bounds__(64) void value_tiles_bitmap_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ unsigned long long bits[G::kTokens];
    __shared__ int woff[G::kWords + 1];
    const int u = blockIdx.x >> 1, half = blockIdx.x & 1, h = blockIdx.y, i = threadIdx.x;
    const int ntok = G::tokens(nb, u);
    for (int t = i; t < G::kTokens; t += 64) bits[t] = 0ull;
    const HalfLists L = half_lists<G>(src, h, u, half, i, woff);
    for (int s = 0;; s++) {
        const int t = list_token<G>(L, woff, i, s, ntok);
        if (t < 0) break;
        atomicOr(&bits[t], 1ull << (63 - L.chan));
    }
    __syncthreads();
    const int64_t tile0 = G::first_tile(u) + half * 64;
    for (int t = i; t < ntok; t += 64) {
        const uint64_t mt = bits[t];
        tile_bmp(dst, h, nb)[tile0 + G::tile(t)] = mt;
        tile_idx(dst, h, nb)[tile0 + G::tile(t) + 1] = tile_length(mt);
    }
}

// One wave per (unit half, head): the streams of the half's tiles, padding included.
template <class G>
__global__ __launch_bounds__(64) void value_tiles_stream_kernel(mustafar_cache_view src, mustafar_cache_view dst, int nb)
{
    __shared__ int woff[G::kWords + 1];
    const int u = blockIdx.x >> 1, half = blockIdx.x & 1, h = blockIdx.y, i = threadIdx.x;
    const int ntok = G::tokens(nb, u);
    const HalfLists L = half_lists<G>(src, h, u, half, i, woff);
    const int64_t tile0 = G::first_tile(u) + half * 64;
    const uint64_t* bmp = tile_bmp(dst, h, nb) + tile0;
    const uint32_t* idx = tile_idx(dst, h, nb) + tile0;
    uint16_t* nz = head_stream(dst, h);
    for (int s = 0;; s++) {
        const int t = list_token<G>(L, woff, i, s, ntok);
        if (t < 0) break;
        const int tl = G::tile(t);
        nz[2ull * idx[tl] + tile_rank(bmp[tl], L.chan)] = *reinterpret_cast<const uint16_t*>(L.base + vl_value_byte(L.m, woff[s >> 2], i, s));
    }
    for (int t = i; t < ntok; t += 64) {   // lane = token: its tiles' padding
        const int tl = G::tile(t);
        const int n = __popcll(bmp[tl]), n8 = (n + 7) & ~7;
        for (int q = n; q < n8; q++) nz[2ull * idx[tl] + q] = 0;
    }
}

// ================================================================ the entry points (include/mustafar_hip.h); every refusal is tile_view.h's
// What an entry point needs of a form: its view rule, the columns of its table, the grid's x of its plan pass and of the other passes, the
// table type of the scan and its four kernels.
template <class R, auto WidthKernel, auto FillKernel, auto StreamKernel>
struct RowForm {   // one wave per block in every pass
    using Table = R;
    static bool view_ok(const mustafar_cache_view* v, int tokens) { return row_view_ok(v, tokens, R::flag); }
    static int columns(int nb) { return nb; }
    static int plan_x(int nb) { return nb; }
    static int pass_x(int nb) { return nb; }
    static constexpr auto plan_kernel = WidthKernel, fill_kernel = FillKernel;
    static constexpr auto bitmap_kernel = key_tiles_bitmap_kernel<R>, stream_kernel = StreamKernel;
};
template <class G>
struct ListForm {   // one wave per unit in the plan pass, per unit half in the others
    using Table = ListsTable;
    static bool view_ok(const mustafar_cache_view* v, int tokens) { return list_view_ok(v, G::flag, G::columns(tokens / 64)); }
    static int columns(int nb) { return G::columns(nb); }
    static int plan_x(int nb) { return G::count(nb); }
    static int pass_x(int nb) { return 2 * G::count(nb); }
    static constexpr auto plan_kernel = value_lists_size_kernel<G>, fill_kernel = value_lists_fill_kernel<G>;
    static constexpr auto bitmap_kernel = value_tiles_bitmap_kernel<G>, stream_kernel = value_tiles_stream_kernel<G>;
};
using KeyRows = RowForm<ByteRows, key_rows_width_kernel, key_rows_fill_kernel, key_tiles_stream_kernel>;
using KeyNibbleRows = RowForm<NibbleRows, key_nibble_rows_width_kernel, key_nibble_rows_fill_kernel, key_nibble_tiles_stream_kernel>;
using ValueLists = ListForm<BlockLists>;
using ValuePairLists = ListForm<PairLists>;

// tiles -> the block table (a number per table entry, then the scan) and the heads' units
template <class F>
int plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_units)
{
    if (!retile_shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !table || !head_units) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64;
    F::plan_kernel<<<dim3(F::plan_x(nb), Bp), 64, 0, st>>>(*src, nb, table);
    block_table_scan_kernel<typename F::Table><<<Bp, 64, 0, st>>>(F::columns(nb) - F::Table::closing, table, head_units);
    return (int)hipGetLastError();
}
// tiles -> form; dst.idx is the table of plan()
template <class F>
int fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens)
{
    if (!retile_shape_ok(Bp, tokens) || !tile_view_ok(src, tokens) || !F::view_ok(dst, tokens) || dst->idx_head_stride != F::columns(tokens / 64)) return MUSTAFAR_EINVAL;
    const int nb = tokens / 64;
    F::fill_kernel<<<dim3(F::pass_x(nb), Bp), 64, 0, static_cast<hipStream_t>(stream)>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}
// form -> tiles: bitmaps and tile lengths, the offsets of a head by one scan, the streams
template <class F>
int to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total)
{
    if (!retile_shape_ok(Bp, tokens) || !F::view_ok(src, tokens) || !tile_view_ok(dst, tokens) || !dst->nz_head_stride) return MUSTAFAR_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nb = tokens / 64;
    F::bitmap_kernel<<<dim3(F::pass_x(nb), Bp), 64, 0, st>>>(*src, *dst, nb);
    tile_offsets_scan_kernel<<<Bp, 64, 0, st>>>(*dst, nb, head_total);
    F::stream_kernel<<<dim3(F::pass_x(nb), Bp), 64, 0, st>>>(*src, *dst, nb);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int mustafar_key_rows_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_rows)
{
    return plan<KeyRows>(stream, src, Bp, tokens, table, head_rows);
}
int mustafar_key_rows_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens)
{
    return fill<KeyRows>(stream, src, dst, Bp, tokens);
}
int mustafar_key_rows_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total)
{
    return to_tiles<KeyRows>(stream, src, dst, Bp, tokens, head_total);
}

int mustafar_key_nibble_rows_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_rows)
{
    return plan<KeyNibbleRows>(stream, src, Bp, tokens, table, head_rows);
}
int mustafar_key_nibble_rows_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens)
{
    return fill<KeyNibbleRows>(stream, src, dst, Bp, tokens);
}
int mustafar_key_nibble_rows_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total)
{
    return to_tiles<KeyNibbleRows>(stream, src, dst, Bp, tokens, head_total);
}

int mustafar_value_lists_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_dwords)
{
    return plan<ValueLists>(stream, src, Bp, tokens, table, head_dwords);
}
int mustafar_value_lists_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens)
{
    return fill<ValueLists>(stream, src, dst, Bp, tokens);
}
int mustafar_value_lists_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total)
{
    return to_tiles<ValueLists>(stream, src, dst, Bp, tokens, head_total);
}

int mustafar_value_pair_lists_plan(void* stream, const mustafar_cache_view* src, int Bp, int tokens, uint32_t* table, int64_t* head_dwords)
{
    return plan<ValuePairLists>(stream, src, Bp, tokens, table, head_dwords);
}
int mustafar_value_pair_lists_fill(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens)
{
    return fill<ValuePairLists>(stream, src, dst, Bp, tokens);
}
int mustafar_value_pair_lists_to_tiles(void* stream, const mustafar_cache_view* src, const mustafar_cache_view* dst, int Bp, int tokens, int64_t* head_total)
{
    return to_tiles<ValuePairLists>(stream, src, dst, Bp, tokens, head_total);
}

}  // extern "C"
