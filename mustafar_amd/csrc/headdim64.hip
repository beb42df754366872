// headdim64.hip -- head_dim 64: magnitude prune, the two-pass conversion to the compressed format and the fused decode, for gfx950.
//
// The D = 128 kernels (compress.hip, spmv.hip) are tuned to a 64-token block of 128 tiles; this file is the D = 64 path, written plainly
// (no inline assembly) and reached through the same C ABI entry points (mustafar_prune_magnitude, mustafar_compress_{bitmap,pack}_*,
// mustafar_decode_attention_hd).  Format at D = 64 (kernel/compression.py:32-36, :87-97):
//   K tile id = (token/64)*64 + d          64 consecutive tokens of channel d
//   V tile id = (token/64)*64 + token%64   the 64 channels of one token
//   bmp [B', t], idx [B', t + 1]: one tile per token and head on either side.
//
// Fused decode (mustafar_decode_attention's semantics): grid (x, y) = (S1 compressed workgroups + window chunks, kv head).  A workgroup is
// one wave and serves ALL G q heads of its kv head (q in LDS), so the compressed bytes are read once per kv head.  For every 64-token
// block of its run: the block's key stream -- one contiguous 16-byte aligned byte range -- is copied to LDS with coalesced loads, then
//   key phase    lane = token: for each of the 64 channel tiles the bitmap (a scalar load) bit-reversed is the lane mask of the tile and
//                the input of v_mbcnt, which ranks the lane's element in the tile's packed stream; score[g] += k * q[g][d] in fp32
//   softmax step fp16(score) * (1/sqrt d) -> fp16 (+ mask, clamped), running max / sum per head, e = fp16(exp(x - max)) to LDS
//   value phase  lane = channel: the block's value stream to LDS, one tile per token, o[g] += e[g][token] * v
// Window workgroups do the same over 64 dense window rows each (and store the step's new K / V row).  Each workgroup leaves one
// (max, sum, o[64]) slab per head; hd64_finish_kernel merges a row's slabs.  Products are fp16 x fp16, exact in fp32; sums are fp32.

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mustafar_hip.h"
#include "headdim64.h"

namespace mustafar_hd64 {
namespace {

typedef _Float16 h16;
typedef const __attribute__((address_space(4))) uint64_t* cu64_p;   // read-only, wave-uniform: scalar loads
typedef const __attribute__((address_space(4))) uint32_t* cu32_p;

constexpr int kScanThreads = 256;
constexpr int kWinChunk = 64;       // window rows per window workgroup
constexpr int kMaxWindow = 1024;    // the window capacity the slab count is sized for (as at D = 128)
constexpr int kMaxSlabs = 1024;     // slabs of a row (compressed workgroups + window chunks)
constexpr int kMaxExtents = 512;    // entries of the device tables the EXT decode launch reads
constexpr int kWgTarget = 4096;     // workgroups (= waves) a launch aims for: four per SIMD on 256 CUs

__device__ __forceinline__ bool nonzero_h(uint32_t v) { return (v & 0x7fffu) != 0; }   // -0.0 is zero, NaN is not

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
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------------------------------------------ prune
// Lane = row of 64 halfs (32 words).  thr = k-th smallest magnitude (torch.kthvalue(|x|, k), model :103), found bit by bit from the MSB:
// thr |= b iff fewer than k magnitudes are < (thr | b).  SWAR compare: with the guard bit 0x8000 set in each half, (m | H) - (c | c << 16)
// keeps the guard bit of a half iff that magnitude >= c (no borrow crosses the halves).  out = |x| >= thr ? x : sign-preserving zero.
// row_threshold / prune_row: the search and the rule on a row held in registers (prune64_kernel and the one-launch trigger).
__device__ __forceinline__ uint32_t row_threshold(const uint32_t (&raw)[32], int kth)
{
    const uint32_t H = 0x80008000u, ONES = 0x00010001u;
    uint32_t thr = 0;
#pragma unroll 1
    for (int bit = 14; bit >= 0; bit--) {
        const uint32_t c = thr | (1u << bit);
        const uint32_t cc = c | (c << 16);
        uint32_t ge = 0;
#pragma unroll
        for (int j = 0; j < 32; j++) ge += (((raw[j] | H) - cc) >> 15) & ONES;
        const int below = 64 - (int)((ge & 0xffffu) + (ge >> 16));
        if (below < kth) thr = c;
    }
    return thr;
}
__device__ __forceinline__ void prune_row(uint32_t (&raw)[32], uint32_t thr)
{
    const uint32_t H = 0x80008000u, ONES = 0x00010001u;
    const uint32_t tt = thr | (thr << 16);
#pragma unroll
    for (int j = 0; j < 32; j++) {
        const uint32_t keep = (((raw[j] | H) - tt) >> 15) & ONES;   // bit 0 / bit 16: that half is kept
        raw[j] &= ((keep << 16) - keep) | H;                         // kept halves whole, pruned ones keep their sign bit only
    }
}
__device__ __forceinline__ void load_row(const uint4* __restrict__ src, uint32_t (&raw)[32])
{
#pragma unroll
    for (int p = 0; p < 8; p++) {
        const uint4 v = src[p];
        raw[4 * p] = v.x; raw[4 * p + 1] = v.y; raw[4 * p + 2] = v.z; raw[4 * p + 3] = v.w;
    }
}

__global__ __launch_bounds__(64) void prune64_kernel(const uint4* __restrict__ x, uint4* __restrict__ out, int64_t n_rows, int kth)
{
    const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (row >= n_rows) return;
    uint32_t raw[32];
    load_row(x + row * 8, raw);
    prune_row(raw, row_threshold(raw, kth));
#pragma unroll
    for (int p = 0; p < 8; p++) out[row * 8 + p] = make_uint4(raw[4 * p], raw[4 * p + 1], raw[4 * p + 2], raw[4 * p + 3]);
}

// ------------------------------------------------------------------------------------------------ conversion, pass 1
// grid (block, head), one wave, lane = token row.  Lane l owns tile l of the block: its bitmap (MSB = element 0), its padded count
// ceil8(nnz)/2 (compression.py:46-48) and the inclusive prefix of those counts inside the block; blk[h][tb] = the block's total.
__global__ __launch_bounds__(64) void bitmap64_kernel(const uint16_t* __restrict__ x, int t, int key, int64_t* __restrict__ bmp,
                                                      int32_t* __restrict__ accum, int32_t* __restrict__ blk)
{
    const int lane = threadIdx.x, tb = blockIdx.x, h = blockIdx.y, ntb = gridDim.x;
    const uint4* src = reinterpret_cast<const uint4*>(x + ((int64_t)h * t + (int64_t)tb * 64 + lane) * kD);
    uint32_t w[32];
#pragma unroll
    for (int p = 0; p < 8; p++) {
        const uint4 v = src[p];
        w[4 * p] = v.x; w[4 * p + 1] = v.y; w[4 * p + 2] = v.z; w[4 * p + 3] = v.w;
    }
    uint64_t mine = 0;
    if (key) {   // tile d = channel d of the 64 tokens: the ballot over the lanes (bit l = token l), bit-reversed
#pragma unroll
        for (int d = 0; d < 64; d++) {
            const uint64_t b = __ballot(nonzero_h(w[d >> 1] >> (16 * (d & 1))));
            if (lane == d) mine = __builtin_bitreverse64(b);
        }
    } else {     // tile = this token's row: element c at bit 63 - c
#pragma unroll
        for (int j = 0; j < 32; j++) {
            mine |= (uint64_t)nonzero_h(w[j]) << (63 - 2 * j);
            mine |= (uint64_t)nonzero_h(w[j] >> 16) << (62 - 2 * j);
        }
    }
    int32_t c = ((__popcll(mine) + 7) & ~7) >> 1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t u = __shfl_up(c, o);
        if (lane >= o) c += u;
    }
    const int64_t tile = (int64_t)h * t + (int64_t)tb * 64 + lane;
    bmp[tile] = (int64_t)mine;
    accum[tile + h + 1] = c;   // (row h of accum is t + 1 long)
    if (lane == 63) blk[(int64_t)h * ntb + tb] = c;
}

// One workgroup per head: block totals -> exclusive bases (compression.py:294-298 at block granularity), the head's stream length in
// halfs (:302) -> totals[h], accum[h][0] = 0.
__global__ __launch_bounds__(kScanThreads) void scan64_kernel(int32_t* __restrict__ blk, int ntb, int t, int32_t* __restrict__ accum,
                                                              int64_t* __restrict__ totals)
{
    __shared__ int32_t s_wave[kScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = blockIdx.x;
    int32_t* bt = blk + (int64_t)h * ntb;
    int32_t carry = 0;
    for (int base = 0; base < ntb; base += kScanThreads) {
        const int i = base + threadIdx.x;
        const int32_t own = i < ntb ? bt[i] : 0;
        int32_t v = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t u = __shfl_up(v, o);
            if (lane >= o) v += u;
        }
        if (lane == 63) s_wave[wave] = v;
        __syncthreads();
        int32_t add = carry, tot = 0;
        for (int k = 0; k < kScanThreads / 64; k++) {
            if (k < wave) add += s_wave[k];
            tot += s_wave[k];
        }
        if (i < ntb) bt[i] = v - own + add;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        accum[(int64_t)h * (t + 1)] = 0;
        totals[h] = 2 * (int64_t)carry;
    }
}

// head_off = exclusive prefix of the heads' lengths (compression.py:303-304), [B'] = the total; in place, one workgroup.  mirror: the same
// values stored once more, each an aligned 8-byte system-scope store, into device-visible host memory the caller polls.
__global__ __launch_bounds__(kScanThreads) void head_off64_kernel(int64_t* __restrict__ head_off, int Bp, int64_t* mirror)
{
    __shared__ int64_t s_wave[kScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry = 0;
    for (int base = 0; base < Bp; base += kScanThreads) {
        const int i = base + threadIdx.x;
        const int64_t own = i < Bp ? head_off[i] : 0;
        int64_t v = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t u = __shfl_up(v, o);
            if (lane >= o) v += u;
        }
        if (lane == 63) s_wave[wave] = v;
        __syncthreads();
        int64_t add = carry, tot = 0;
        for (int k = 0; k < kScanThreads / 64; k++) {
            if (k < wave) add += s_wave[k];
            tot += s_wave[k];
        }
        if (i < Bp) {
            head_off[i] = v - own + add;
            if (mirror) __hip_atomic_store(mirror + i, v - own + add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        head_off[Bp] = carry;
        if (mirror) __hip_atomic_store(mirror + Bp, carry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(64) void fixup64_kernel(const int32_t* __restrict__ blk_base, int t, int32_t* __restrict__ accum)
{
    const int tb = blockIdx.x, h = blockIdx.y;
    accum[(int64_t)h * (t + 1) + (int64_t)tb * 64 + threadIdx.x + 1] += blk_base[(int64_t)h * gridDim.x + tb];
}

// ------------------------------------------------------------------------------------------------ conversion, pass 2
// Non-zeros of a tile in ascending element order at its stream offset, then zeros up to ceil8(nnz) (compression.py:164-174, :309).
// m: the tile's bitmap as stored (wave-uniform), v: the lane's element (element index = lane).
__device__ __forceinline__ void pack_tile(uint16_t* __restrict__ dst, uint64_t m, uint16_t v, int lane)
{
    const uint64_t mr = __builtin_bitreverse64(m);
    const int nnz = __popcll(mr);
    if ((mr >> lane) & 1ull) dst[rank_below(mr)] = v;
    if (lane >= nnz && lane < ((nnz + 7) & ~7)) dst[lane] = 0;
}

// grid (block, head), one wave.  K: lane = token (its row in registers), tile d = channel d.  V: lane = channel, tile r = token r.
__global__ __launch_bounds__(64) void pack64_kernel(const uint16_t* __restrict__ x, int t, int key, const int64_t* __restrict__ bmp,
                                                    const int32_t* __restrict__ accum, const int64_t* __restrict__ head_off,
                                                    uint16_t* __restrict__ nz)
{
    const int lane = threadIdx.x, tb = blockIdx.x, h = blockIdx.y;
    const int64_t tile0 = (int64_t)h * t + (int64_t)tb * 64;
    const uint64_t bm = (uint64_t)bmp[tile0 + lane];
    const int32_t st = accum[tile0 + h + lane];   // start of tile `lane` (half2 units)
    uint16_t* nz_h = nz + head_off[h];
    if (key) {
        const uint4* src = reinterpret_cast<const uint4*>(x + (tile0 + lane) * kD);
        uint32_t w[32];
#pragma unroll
        for (int p = 0; p < 8; p++) {
            const uint4 v = src[p];
            w[4 * p] = v.x; w[4 * p + 1] = v.y; w[4 * p + 2] = v.z; w[4 * p + 3] = v.w;
        }
#pragma unroll
        for (int d = 0; d < 64; d++) {
            const uint64_t m = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(bm >> 32), d) << 32) |
                               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bm, d);
            const int32_t s = __builtin_amdgcn_readlane(st, d);
            pack_tile(nz_h + 2 * (int64_t)s, m, (uint16_t)(w[d >> 1] >> (16 * (d & 1))), lane);
        }
    } else {
        const uint16_t* xb = x + tile0 * kD;
#pragma unroll 8
        for (int r = 0; r < 64; r++) {
            const uint64_t m = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(bm >> 32), r) << 32) |
                               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bm, r);
            const int32_t s = __builtin_amdgcn_readlane(st, r);
            pack_tile(nz_h + 2 * (int64_t)s, m, xb[r * kD + lane], lane);
        }
    }
}

// ------------------------------------------------------------------------------------------------ the 256-token trigger in one launch
// RAW window rows -> a finished 256-token extent (mustafar_trigger_compress_batch_hd).  grid (kv head, side: 0 = K, 1 = V), 256 threads:
// wave w = 64-token block w, lane = row; the row's 32 words stay in registers from the load to the packed stream.  Threshold and rule as
// prune64_kernel (kth = 0: the rows are pruned already); K tile d of a block = the ballot of channel d over the lanes, V tile = the
// lane's own row; tile lengths ceil8(nnz); a wave prefix gives the offsets inside the block and the four block totals cross through
// LDS, so the workgroup knows its head's stream length before it writes a byte: no workgroup waits for another one.  A head that needs
// more than region_halfs sets bit 0 of *flag and writes bitmaps, offsets and head_total (the length it needs) but no stream bytes.
struct ExtSide {
    const uint16_t* x;        // window rows: head h at x + h * head_stride, row r 64 halfs behind row r - 1
    uint64_t* bmp;            // [B'][bmp_stride]
    uint32_t* idx;            // [B'][idx_stride]
    uint16_t* nz;             // head h's region at nz + 8 * h * nz_stride halfs
    uint32_t* nz_offset;      // [B'] (or nullptr): h * nz_stride is stored there
    int64_t* head_total;      // [B'] halfs
    int64_t bmp_stride, idx_stride, region_halfs;
    uint32_t nz_stride;       // uint4 units
    int kth;
};

// The body both compression kernels share: 256 raw rows of head h at `rows` -> that head's part of the extent `s` describes.
__device__ __forceinline__ void compress_256_rows(const ExtSide& s, const uint16_t* rows, int h, bool key, int32_t* __restrict__ flag)
{
    __shared__ int32_t s_tot[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t w[32];
    load_row(reinterpret_cast<const uint4*>(rows + (int64_t)(wave * 64 + lane) * kD), w);
    if (s.kth > 0) prune_row(w, row_threshold(w, s.kth));
    uint64_t mine = 0;
    if (key) {
#pragma unroll
        for (int d = 0; d < 64; d++) {
            const uint64_t b = __ballot(nonzero_h(w[d >> 1] >> (16 * (d & 1))));
            if (lane == d) mine = __builtin_bitreverse64(b);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 32; j++) {
            mine |= (uint64_t)nonzero_h(w[j]) << (63 - 2 * j);
            mine |= (uint64_t)nonzero_h(w[j] >> 16) << (62 - 2 * j);
        }
    }
    const int32_t own = ((__popcll(mine) + 7) & ~7) >> 1;   // half2 units
    int32_t c = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t u = __shfl_up(c, o);
        if (lane >= o) c += u;
    }
    if (lane == 63) s_tot[wave] = c;
    __syncthreads();
    int32_t base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < wave) base += s_tot[k];
        total += s_tot[k];
    }
    uint32_t* idx_h = s.idx + (int64_t)h * s.idx_stride;
    s.bmp[(int64_t)h * s.bmp_stride + wave * 64 + lane] = mine;
    idx_h[wave * 64 + lane + 1] = (uint32_t)(base + c);
    if (threadIdx.x == 0) {
        idx_h[0] = 0;
        s.head_total[h] = 2 * (int64_t)total;
        if (s.nz_offset) s.nz_offset[h] = (uint32_t)h * s.nz_stride;
    }
    if (s.region_halfs > 0 && 2 * (int64_t)total > s.region_halfs) {   // (workgroup-uniform)
        if (threadIdx.x == 0) atomicOr(flag, 1);
        return;
    }
    uint16_t* nz_h = s.nz + 8 * (int64_t)h * s.nz_stride;
    const int32_t st = base + c - own;   // start of tile `lane` of this block (half2 units)
    if (key) {
#pragma unroll
        for (int d = 0; d < 64; d++) {
            const uint64_t m = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(mine >> 32), d) << 32) |
                               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, d);
            const int32_t sd = __builtin_amdgcn_readlane(st, d);
            pack_tile(nz_h + 2 * (int64_t)sd, m, (uint16_t)(w[d >> 1] >> (16 * (d & 1))), lane);
        }
    } else {   // the lane's own row: its non-zeros in channel order, then zeros up to ceil8(nnz)
        uint16_t* dst = nz_h + 2 * (int64_t)st;
        int n = 0;
#pragma unroll
        for (int j = 0; j < 64; j++) {
            const uint16_t v = (uint16_t)(w[j >> 1] >> (16 * (j & 1)));
            if (nonzero_h(v)) dst[n++] = v;
        }
        for (; n < 2 * own; n++) dst[n] = 0;
    }
}

__global__ __launch_bounds__(256) void hd64_extent_compress_kernel(ExtSide ks, ExtSide vs, int64_t head_stride, int32_t* __restrict__ flag)
{
    const int h = blockIdx.x;
    const bool key = blockIdx.y == 0;
    const ExtSide& s = key ? ks : vs;
    compress_256_rows(s, s.x + (int64_t)h * head_stride, h, key, flag);
}

// ------------------------------------------------------------------------------------------------ a prefill in 256-token chunks
// RAW rows [0, 256 n) of every head -> n finished extents per side (mustafar_prefill_compress_hd).  grid (kv head, chunk, side): the
// trigger's body on chunk c's rows, x + h * head_stride + c * 256 * 64, into extent c of the staging -- every array of chunk c lies
// c * chunk_bytes behind chunk 0's, its head totals at head_total + c * B'.  Each chunk is an extent of its own (offsets from 0), so
// here too no workgroup waits for another one.  Head 0's workgroup lists the chunk's view in entry c of the side's device table (or
// nullptr), which is what hd64_gather_kernel reads.
__device__ __forceinline__ ExtSide chunk_of(const ExtSide& s, int c, int64_t chunk_bytes, int Bp)
{
    ExtSide r = s;
    const int64_t by = (int64_t)c * chunk_bytes;
    r.bmp = reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(s.bmp) + by);
    r.idx = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(s.idx) + by);
    r.nz = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(s.nz) + by);
    r.nz_offset = s.nz_offset ? reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(s.nz_offset) + by) : nullptr;
    r.head_total = s.head_total + (int64_t)c * Bp;
    return r;
}

__global__ __launch_bounds__(256) void hd64_prefill_compress_kernel(ExtSide ks, ExtSide vs, int64_t head_stride, int64_t k_chunk_bytes,
                                                                    int64_t v_chunk_bytes, mustafar_cache_view* k_pieces,
                                                                    mustafar_cache_view* v_pieces, int32_t* __restrict__ flag)
{
    const int h = blockIdx.x, c = blockIdx.y, Bp = gridDim.x;
    const bool key = blockIdx.z == 0;
    const ExtSide s = chunk_of(key ? ks : vs, c, key ? k_chunk_bytes : v_chunk_bytes, Bp);
    mustafar_cache_view* pieces = key ? k_pieces : v_pieces;
    if (h == 0 && threadIdx.x == 0 && pieces)
        pieces[c] = mustafar_cache_view{s.bmp, s.nz, s.idx, s.nz_offset, s.bmp_stride, s.idx_stride, (int64_t)s.nz_stride};
    compress_256_rows(s, s.x + (int64_t)h * head_stride + (int64_t)c * 256 * kD, h, key, flag);
}

// ------------------------------------------------------------------------------------------------ gather
// 256-token pieces, each with offsets relative to itself, -> ONE reference-layout cache (mustafar_cache_gather_hd): the end of a chunked
// prefill and ExtentCache64.consolidate().  grid (piece, kv head), 256 threads, thread = token.  Pieces [0, n_first) are the 256-token
// slices of the optional first view (a whole cache: its offsets already count from the head's start, shift 0); piece n_first + i is entry
// i of the DEVICE table.  A table piece starts where the stream in front of it ends: the first view's last offset + the last offsets of
// entries [0, i), one or two per thread and a workgroup sum -- read here, nothing on the host, no workgroup waits for another.  Bitmaps
// are copied, offsets are copied + shift (piece 0 writes the head's entry 0), the stream moves as 16-byte pieces: every tile is padded
// to 8 halfs, so every offset is a multiple of 16 bytes behind a head start that is one.
struct GatherArgs {
    mustafar_cache_view dst, first;      // strides resolved by the host (no zeros left in bmp / idx strides)
    const mustafar_cache_view* pieces;
    int first_tokens, n_pieces;
};

__device__ __forceinline__ const uint4* head_stream(const mustafar_cache_view& v, int h)
{
    const int64_t off = v.nz_head_stride ? (int64_t)h * v.nz_head_stride : (int64_t)v.nz_offset[h];
    return static_cast<const uint4*>(v.nz) + off;
}

__global__ __launch_bounds__(256) void hd64_gather_kernel(GatherArgs a)
{
    __shared__ uint32_t s_sum[4];
    const int p = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const int n_first = a.first_tokens >> 8;
    const uint64_t* sb;
    const uint32_t* si;
    const uint4* sz;
    uint32_t shift = 0;
    if (p < n_first) {   // (workgroup-uniform)
        sb = a.first.bmp + (int64_t)h * a.first.bmp_head_stride + p * 256;
        si = a.first.idx + (int64_t)h * a.first.idx_head_stride + p * 256;
        sz = head_stream(a.first, h);
    } else {
        const int i = p - n_first;
        uint32_t part = 0;
        for (int j = t; j < i; j += 256) {
            const mustafar_cache_view e = a.pieces[j];
            part += e.idx[(int64_t)h * (e.idx_head_stride ? e.idx_head_stride : 257) + 256];
        }
        if (t == 0 && n_first) part += a.first.idx[(int64_t)h * a.first.idx_head_stride + a.first_tokens];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
        if ((t & 63) == 0) s_sum[t >> 6] = part;
        __syncthreads();
        shift = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        const mustafar_cache_view e = a.pieces[i];
        sb = e.bmp + (int64_t)h * (e.bmp_head_stride ? e.bmp_head_stride : 256);
        si = e.idx + (int64_t)h * (e.idx_head_stride ? e.idx_head_stride : 257);
        sz = head_stream(e, h);
    }
    const int64_t tok0 = (int64_t)p * 256;
    uint32_t* di = a.dst.idx + (int64_t)h * a.dst.idx_head_stride + tok0;
    a.dst.bmp[(int64_t)h * a.dst.bmp_head_stride + tok0 + t] = sb[t];
    di[t + 1] = si[t + 1] + shift;
    const uint32_t i0 = si[0], i1 = si[256];   // half2 units, multiples of 4
    if (p == 0 && t == 0) di[0] = i0 + shift;   // (0: a cache's and an extent's offsets start there)
    const uint4* src = sz + (i0 >> 2);
    uint4* dst = const_cast<uint4*>(head_stream(a.dst, h)) + ((i0 + shift) >> 2);
    const int n16 = (int)((i1 - i0) >> 2);   // <= 256 tiles x 64 halfs / 8 = 2048
    for (int k = t; k < n16; k += 256) dst[k] = src[k];
}

// The tail of a trigger at D = 64 (mustafar_trigger_finish_batch_hd): one workgroup lists the extent's view in its slot of the device
// table, all slide their head's window rows [drop, len) to the front.  The ranges may overlap: ascending pieces, each read in full
// before it is written.
__global__ __launch_bounds__(256) void hd64_trigger_finish_kernel(uint16_t* k_win, uint16_t* v_win, int64_t head_stride, int len, int drop,
                                                                  mustafar_cache_view k_view, mustafar_cache_view v_view,
                                                                  mustafar_cache_view* k_slot, mustafar_cache_view* v_slot)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        mustafar_cache_view* slot = blockIdx.y ? v_slot : k_slot;
        if (slot) *slot = blockIdx.y ? v_view : k_view;
    }
    if (drop <= 0 || len <= drop) return;
    uint16_t* win = (blockIdx.y ? v_win : k_win) + blockIdx.x * head_stride;
    const int n16 = (len - drop) * (kD / 8);
    const uint4* src = reinterpret_cast<const uint4*>(win + (int64_t)drop * kD);
    uint4* dst = reinterpret_cast<uint4*>(win);
    for (int base = 0; base < n16; base += 4 * 256) {   // (workgroup-uniform trip count)
        uint4 v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int p = base + threadIdx.x + i * 256;
            if (p < n16) v[i] = src[p];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int p = base + threadIdx.x + i * 256;
            if (p < n16) dst[p] = v[i];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ fused decode
struct DecArgs {
    const h16* q;          // [BH, 64]
    float* ws_o;           // [slabs, BH, 64] unnormalised outputs
    float* ws_ml;          // [slabs, BH, 2] (max, sum)
    h16* k_win;            // [B', w_cap, 64]
    h16* v_win;
    const h16* k_new;      // [B', 64] or nullptr
    const h16* v_new;
    const int* w_extra;    // device step counter (graph replay) or nullptr
    const h16* mask;       // additive fp16 mask rows or nullptr
    int64_t mask_stride;
    int mask_heads;
    int T, BH, bpw, S1, w_len, w_cap;
    float inv_sqrt_d;
};

// Operands of the EXT instantiation (mustafar_decode_attention_extents_hd): the base arrays arrive through the kernel's eight pointers,
// the blocks behind T_base through two DEVICE tables of mustafar_cache_view, four blocks per entry.  The plain instantiation carries
// an empty struct in its place and compiles to what it was.
struct ExtArgs {
    const mustafar_cache_view* k_ext;
    const mustafar_cache_view* v_ext;
    const int32_t* t_dev;                // compressed tokens in use (a.T is then the capacity) or nullptr
    int64_t k_bmp_stride, k_idx_stride, v_bmp_stride, v_idx_stride;   // head strides of the base rows
    uint32_t k_nz_stride, v_nz_stride;   // != 0: the base's head h starts at h * stride (uint4 units) instead of k_off[h]
    int T_base;
};
struct NoExt {};
template <bool EXT> struct ExtOf { typedef NoExt type; };
template <> struct ExtOf<true> { typedef ExtArgs type; };
static_assert(sizeof(mustafar_cache_view) == 64, "the EXT kernel reads the first seven 8-byte words of a table entry (the eighth holds the flags: extents are tiles)");
// The row kernel's LSE output, carried the same way: the instantiation without one takes an empty struct and stays what it was.
struct LseArg { float* ptr; };
struct NoLse {};
template <bool LSE> struct LseOf { typedef NoLse type; };
template <> struct LseOf<true> { typedef LseArg type; };

// One side of a 64-token block as the phases read it: bitmaps and offsets of its 64 tiles (scalar loads), the head's stream.
struct BlockRef {
    cu64_p bmp;
    cu32_p idx;
    const uint4* nz;
};
// Block j (0..3) of a table entry, head kvh: every field a scalar load (the entry is wave-uniform), offsets relative to the extent.
__device__ __forceinline__ BlockRef extent_block(const mustafar_cache_view* entry, int kvh, int j)
{
    const cu64_p f = (cu64_p)reinterpret_cast<const uint64_t*>(entry);   // bmp, nz, idx, nz_offset, bmp stride, idx stride, nz stride
    const int64_t bs = f[4] ? (int64_t)f[4] : 256, is = f[5] ? (int64_t)f[5] : 257;
    BlockRef r;
    r.bmp = (cu64_p)(reinterpret_cast<const uint64_t*>(f[0]) + kvh * bs + j * 64);
    r.idx = (cu32_p)(reinterpret_cast<const uint32_t*>(f[2]) + kvh * is + j * 64);
    r.nz = reinterpret_cast<const uint4*>(f[1]) + (int64_t)kvh * (int64_t)f[6];
    return r;
}

// x = fp16(fp16(score) * (1/sqrt d)) (model :284; the product with the fp32 reciprocal, as at D = 128), then the hook's mask: an fp16
// addition clamped at finfo(fp16).min (model :293-301).
__device__ __forceinline__ float scaled(float acc, float inv_sqrt_d) { return (float)(h16)((float)(h16)acc * inv_sqrt_d); }
__device__ __forceinline__ float masked(float x, h16 m) { return fmaxf((float)(h16)(x + (float)m), -65504.f); }

// Online softmax step of one 64-token batch: x (lane = token, -inf beyond the window) -> e in LDS, running (max, sum), o rescaled.
template <int G>
__device__ __forceinline__ void softmax_step(const float (&x)[G], float (&M)[G], float (&L)[G], float (&o)[G], h16* s_e, int lane)
{
#pragma unroll
    for (int g = 0; g < G; g++) {
        const float mn = fmaxf(M[g], wave_max(x[g]));
        const float alpha = __expf(M[g] - mn);                 // (exp(-inf) = 0 before the first batch)
        const float e = (float)(h16)__expf(x[g] - mn);         // e in fp16, as the one-pass forms at D = 128
        L[g] = L[g] * alpha + wave_sum(e);
        o[g] *= alpha;
        M[g] = mn;
        s_e[g * 64 + lane] = (h16)e;
    }
}

// A block's packed stream [2 idx[first tile], 2 idx[first tile + 64]) halfs -> LDS (16-byte pieces: every tile's stream is padded to 8 halfs,
// a head's stream starts on 16 bytes).  Returns the block's first offset (half2 units).
__device__ __forceinline__ uint32_t stage_block(const uint4* __restrict__ head_nz, cu32_p idx, uint4* s_buf, int lane)
{
    const uint32_t i0 = idx[0], i1 = idx[64];
    const int n16 = (int)((i1 - i0) >> 2);   // <= 64 tiles x 64 halfs / 8 = 512
    const uint4* src = head_nz + (i0 >> 2);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int i = lane + 64 * k;
        if (i < n16) s_buf[i] = src[i];
    }
    return i0;
}

template <int G, bool MASK, bool EXT>
__global__ __launch_bounds__(64) void hd64_decode_kernel(const uint64_t* __restrict__ k_bmp, const uint4* __restrict__ k_nz,
                                                         const uint32_t* __restrict__ k_idx, const uint32_t* __restrict__ k_off,
                                                         const uint64_t* __restrict__ v_bmp, const uint4* __restrict__ v_nz,
                                                         const uint32_t* __restrict__ v_idx, const uint32_t* __restrict__ v_off, DecArgs a,
                                                         typename ExtOf<EXT>::type e)
{
    __shared__ uint4 s_buf[512];        // a block's key or value stream (at most 4096 halfs)
    __shared__ h16 s_q[G * 64];
    __shared__ h16 s_e[G * 64];
    const int lane = threadIdx.x, kvh = blockIdx.y, x = blockIdx.x;
    const int bh0 = kvh * G;
    const uint16_t* sb = reinterpret_cast<const uint16_t*>(s_buf);
#pragma unroll
    for (int g = 0; g < G; g++) s_q[g * 64 + lane] = a.q[(int64_t)(bh0 + g) * kD + lane];
    const h16* mrow[G];
#pragma unroll
    for (int g = 0; g < G; g++) mrow[g] = MASK ? a.mask + (int64_t)((bh0 + g) / a.mask_heads) * a.mask_stride : nullptr;
    float M[G], L[G], o[G];
#pragma unroll
    for (int g = 0; g < G; g++) { M[g] = -INFINITY; L[g] = 0.f; o[g] = 0.f; }
    __syncthreads();

    if (x < a.S1) {
        // ---- compressed blocks [tb0, tb1) of kv head kvh
        int ntb = a.T / 64;   // blocks the launch is sized for; EXT with a device-side T: the blocks in use
        if constexpr (EXT) { if (e.t_dev) ntb = min(ntb, __builtin_amdgcn_readfirstlane(*e.t_dev) >> 6); }
        const int tb0 = x * a.bpw, tb1 = min(ntb, tb0 + a.bpw);   // (tb0 >= ntb: no block in use, the slabs keep weight zero)
        const uint4* kz;
        const uint4* vz;
        int ntb_base = 0;
        if constexpr (EXT) {
            ntb_base = e.T_base >> 6;
            kz = k_nz + (e.k_nz_stride ? (int64_t)kvh * e.k_nz_stride : (int64_t)k_off[kvh]);
            vz = v_nz + (e.v_nz_stride ? (int64_t)kvh * e.v_nz_stride : (int64_t)v_off[kvh]);
        } else {
            kz = k_nz + k_off[kvh];
            vz = v_nz + v_off[kvh];
        }
        for (int tb = tb0; tb < tb1; tb++) {
            cu64_p kb, vb;
            cu32_p ki, vi;
            const uint4* kzb = kz;
            const uint4* vzb = vz;
            if constexpr (EXT) {   // resolved per block: a run may cross base -> extent and extent -> extent
                if (tb < ntb_base) {
                    kb = (cu64_p)(k_bmp + kvh * e.k_bmp_stride + (int64_t)tb * 64);
                    ki = (cu32_p)(k_idx + kvh * e.k_idx_stride + (int64_t)tb * 64);
                    vb = (cu64_p)(v_bmp + kvh * e.v_bmp_stride + (int64_t)tb * 64);
                    vi = (cu32_p)(v_idx + kvh * e.v_idx_stride + (int64_t)tb * 64);
                } else {
                    const int xb = tb - ntb_base;
                    const BlockRef kr = extent_block(e.k_ext + (xb >> 2), kvh, xb & 3);
                    const BlockRef vr = extent_block(e.v_ext + (xb >> 2), kvh, xb & 3);
                    kb = kr.bmp; ki = kr.idx; kzb = kr.nz;
                    vb = vr.bmp; vi = vr.idx; vzb = vr.nz;
                }
            } else {
                const int64_t tile0 = (int64_t)kvh * a.T + (int64_t)tb * 64;
                kb = (cu64_p)(k_bmp + tile0);
                ki = (cu32_p)(k_idx + tile0 + kvh);
                vb = (cu64_p)(v_bmp + tile0);
                vi = (cu32_p)(v_idx + tile0 + kvh);
            }
            const uint32_t k0 = stage_block(kzb, ki, s_buf, lane);
            __syncthreads();
            float s[G];
#pragma unroll
            for (int g = 0; g < G; g++) s[g] = 0.f;
#pragma unroll 16
            for (int d = 0; d < 64; d++) {   // key phase: lane = token, tile d = channel d
                const uint64_t mr = __builtin_bitreverse64(kb[d]);
                const uint32_t off = 2 * (ki[d] - k0) + rank_below(mr);
                const uint16_t raw = sb[off < 4096 ? off : 0];
                const float kv = ((mr >> lane) & 1ull) ? (float)__builtin_bit_cast(h16, raw) : 0.f;
#pragma unroll
                for (int g = 0; g < G; g++) s[g] = __builtin_fmaf(kv, (float)s_q[g * 64 + d], s[g]);
            }
            float xs[G];
#pragma unroll
            for (int g = 0; g < G; g++) {
                xs[g] = scaled(s[g], a.inv_sqrt_d);
                if (MASK) xs[g] = masked(xs[g], mrow[g][tb * 64 + lane]);
            }
            __syncthreads();   // (s_buf is read; the value stream goes there next)
            softmax_step<G>(xs, M, L, o, s_e, lane);
            const uint32_t v0 = stage_block(vzb, vi, s_buf, lane);
            __syncthreads();
#pragma unroll 16
            for (int r = 0; r < 64; r++) {   // value phase: lane = channel, tile r = token r
                const uint64_t mr = __builtin_bitreverse64(vb[r]);
                const uint32_t off = 2 * (vi[r] - v0) + rank_below(mr);
                const uint16_t raw = sb[off < 4096 ? off : 0];
                const float vv = ((mr >> lane) & 1ull) ? (float)__builtin_bit_cast(h16, raw) : 0.f;
#pragma unroll
                for (int g = 0; g < G; g++) o[g] = __builtin_fmaf(vv, (float)s_e[g * 64 + r], o[g]);
            }
            __syncthreads();
        }
    } else {
        // ---- window chunk: rows [w0, w0 + 64) of the dense window (the step's new row appended at w_len - 1)
        const int w_len = a.w_extra ? min(a.w_len + *a.w_extra, a.w_cap) : a.w_len;
        const int w0 = (x - a.S1) * kWinChunk;
        int T_used = a.T;   // the window rows' mask columns follow the compressed tokens IN USE (as the D = 128 extents launch)
        if constexpr (EXT) { if (e.t_dev) T_used = __builtin_amdgcn_readfirstlane(*e.t_dev); }
        if (w0 < w_len) {
            const int w = w0 + lane;
            const bool valid = w < w_len;
            const int wr = valid ? w : w0;
            const bool fresh_k = a.k_new && wr == w_len - 1;
            h16* krow = a.k_win + ((int64_t)kvh * a.w_cap + wr) * kD;
            const uint4* ksrc = reinterpret_cast<const uint4*>(fresh_k ? a.k_new + (int64_t)kvh * kD : krow);
            uint4 kr[8];
#pragma unroll
            for (int p = 0; p < 8; p++) kr[p] = ksrc[p];
            if (fresh_k && valid) {   // store the new key row (model :270)
#pragma unroll
                for (int p = 0; p < 8; p++) reinterpret_cast<uint4*>(krow)[p] = kr[p];
            }
            const h16* kh = reinterpret_cast<const h16*>(kr);
            float xs[G];
#pragma unroll
            for (int g = 0; g < G; g++) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < kD; c++) s = __builtin_fmaf((float)kh[c], (float)s_q[g * 64 + c], s);
                float xv = scaled(s, a.inv_sqrt_d);
                if (MASK && valid) xv = masked(xv, mrow[g][T_used + w]);
                xs[g] = valid ? xv : -INFINITY;
            }
            softmax_step<G>(xs, M, L, o, s_e, lane);
            __syncthreads();
            const int n = min(kWinChunk, w_len - w0);
            for (int r = 0; r < n; r++) {   // lane = channel
                const int ww = w0 + r;
                h16* vrow = a.v_win + ((int64_t)kvh * a.w_cap + ww) * kD;
                h16 v;
                if (a.v_new && ww == w_len - 1) {
                    v = a.v_new[(int64_t)kvh * kD + lane];
                    vrow[lane] = v;   // store the new value row (model :309)
                } else {
                    v = vrow[lane];
                }
#pragma unroll
                for (int g = 0; g < G; g++) o[g] = __builtin_fmaf((float)v, (float)s_e[g * 64 + r], o[g]);
            }
        }
    }
    // ---- the workgroup's slab of every head (an empty window chunk: weight zero)
#pragma unroll
    for (int g = 0; g < G; g++) {
        const int64_t row = (int64_t)x * a.BH + bh0 + g;
        a.ws_o[row * kD + lane] = o[g];
        if (lane == 0) { a.ws_ml[2 * row] = M[g]; a.ws_ml[2 * row + 1] = L[g]; }
    }
}

// out[bh, c] = fp16( sum_s w_s o_s[c] / sum_s w_s l_s ),  w_s = exp(m_s - max m) (0 for an empty slab).  One workgroup per row, four waves
// over the slabs (lane = channel), folded through LDS.  LSE: lse[bh] = max m + log(sum_s w_s l_s), the log-sum-exp of the row's scores as the
// softmax saw them, from the (max, sum) pairs reduced here anyway (-inf for a row whose slabs are all empty).
template <bool LSE>
__global__ __launch_bounds__(256) void hd64_finish_kernel(const float* __restrict__ ws_o, const float* __restrict__ ws_ml, int S, int BH,
                                                          h16* __restrict__ out, typename LseOf<LSE>::type lse)
{
    __shared__ float part[4][kD];
    const int bh = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float mx = -INFINITY;
    for (int s = lane; s < S; s += 64) mx = fmaxf(mx, ws_ml[((int64_t)s * BH + bh) * 2]);
    const float Mx = wave_max(mx);
    float acc = 0.f, den = 0.f;
    for (int s = wave; s < S; s += 4) {
        const float m = ws_ml[((int64_t)s * BH + bh) * 2], l = ws_ml[((int64_t)s * BH + bh) * 2 + 1];
        const float w = l > 0.f ? __expf(m - Mx) : 0.f;
        den += w * l;
        acc += w * ws_o[((int64_t)s * BH + bh) * kD + lane];
    }
    part[wave][lane] = acc;
    __shared__ float dens[4];
    if (lane == 0) dens[wave] = den;
    __syncthreads();
    if (wave == 0) {
        const float o = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
        const float d = dens[0] + dens[1] + dens[2] + dens[3];
        out[(int64_t)bh * kD + lane] = (h16)(o / d);
        if constexpr (LSE) { if (lane == 0) lse.ptr[bh] = d > 0.f ? Mx + __logf(d) : -INFINITY; }
    }
}

// blocks per compressed workgroup: ~kWgTarget workgroups over all kv heads, never more slabs per row than the row kernel takes
inline int blocks_per_wg(int ntb, int Bp)
{
    if (ntb <= 0) return 1;
    int bpw = (int)(((int64_t)ntb * Bp + kWgTarget / 2) / kWgTarget);
    if (bpw < 1) bpw = 1;
    while ((ntb + bpw - 1) / bpw > kMaxSlabs - kMaxWindow / kWinChunk) bpw++;
    return bpw;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// ------------------------------------------------------------------------------------------------ host entry points
int prune(hipStream_t st, const void* x, void* out, int64_t n_rows, int kth)
{
    // rows are read and written as 16-byte pieces
    if (kth < 1 || kth > kD || n_rows < 0 || !x || !out || !aligned16(x) || !aligned16(out)) return MUSTAFAR_EINVAL;
    if (n_rows == 0) return 0;
    const int64_t blocks = (n_rows + 63) / 64;
    if (blocks > 0x7fffffff) return MUSTAFAR_EINVAL;
    prune64_kernel<<<(unsigned)blocks, 64, 0, st>>>(static_cast<const uint4*>(x), static_cast<uint4*>(out), n_rows, kth);
    return (int)hipGetLastError();
}

int bitmap(bool key, hipStream_t st, const void* x, int Bp, int t, int64_t* bmp, int32_t* accum, int64_t* head_off, int64_t* mirror)
{
    if (Bp < 1 || t < 64 || (t & 63) || !x || !aligned16(x) || !bmp || !accum || !head_off) return MUSTAFAR_EINVAL;
    const int ntb = t / 64;
    int32_t* blk = nullptr;
    bool pooled = true;
    if (hipMallocAsync(reinterpret_cast<void**>(&blk), sizeof(int32_t) * (size_t)Bp * ntb, st) != hipSuccess) {
        (void)hipGetLastError();
        pooled = false;
        if (hipMalloc(reinterpret_cast<void**>(&blk), sizeof(int32_t) * (size_t)Bp * ntb) != hipSuccess) return (int)hipGetLastError();
    }
    bitmap64_kernel<<<dim3(ntb, Bp), 64, 0, st>>>(static_cast<const uint16_t*>(x), t, key ? 1 : 0, bmp, accum, blk);
    scan64_kernel<<<Bp, kScanThreads, 0, st>>>(blk, ntb, t, accum, head_off);
    head_off64_kernel<<<1, kScanThreads, 0, st>>>(head_off, Bp, mirror);   // (in front of the fix-up: a polling caller has the sizes sooner)
    fixup64_kernel<<<dim3(ntb, Bp), 64, 0, st>>>(blk, t, accum);
    const int err = (int)hipGetLastError();
    if (pooled) {
        (void)hipFreeAsync(blk, st);
    } else {
        (void)hipStreamSynchronize(st);
        (void)hipFree(blk);
    }
    return err;
}

int pack(bool key, hipStream_t st, const void* x, int Bp, int t, const int64_t* bmp, const int32_t* accum, const int64_t* head_off,
         void* nz_flat)
{
    if (Bp < 1 || t < 64 || (t & 63) || !x || !aligned16(x) || !bmp || !accum || !head_off) return MUSTAFAR_EINVAL;
    if (!nz_flat) return 0;   // nothing to write: every tile of every head is empty
    pack64_kernel<<<dim3(t / 64, Bp), 64, 0, st>>>(static_cast<const uint16_t*>(x), t, key ? 1 : 0, bmp, accum, head_off,
                                                   static_cast<uint16_t*>(nz_flat));
    return (int)hipGetLastError();
}

int64_t workspace_bytes(int T, int Batch_Size, int groups)
{
    if (T < 0 || groups < 1 || Batch_Size < groups || Batch_Size % groups) return 0;
    const int ntb = T / 64;
    const int S1 = ntb > 0 ? (ntb + blocks_per_wg(ntb, Batch_Size / groups) - 1) / blocks_per_wg(ntb, Batch_Size / groups) : 0;
    return (int64_t)(S1 + kMaxWindow / kWinChunk) * Batch_Size * (kD + 2) * (int64_t)sizeof(float);
}

namespace {

// Validation and launches of one call.  ext == nullptr: the plain instantiation over one set of arrays.
int launch_decode(const DecodeCall& c, hipEvent_t* ev, const ExtArgs* ext)
{
    bool no_window = false;
    if (!decode_call_ok(c, kMaxWindow, &no_window) || c.groups > 8) return MUSTAFAR_EINVAL;
    const hipStream_t st = c.stream;
    const uint64_t *k_bmp = c.k.bmp, *v_bmp = c.v.bmp;
    const void *k_nz = c.k.nz, *v_nz = c.v.nz;
    const uint32_t *k_idx = c.k.idx, *k_nz_offset = c.k.nz_offset, *v_idx = c.v.idx, *v_nz_offset = c.v.nz_offset;
    const void *q = c.q, *k_new = c.k_new, *v_new = c.v_new, *attention_mask = c.attention_mask;
    void *k_window = c.k_window, *v_window = c.v_window, *out = c.out, *workspace = c.workspace;
    const int window_len = c.window_len, window_capacity = c.window_capacity, T = c.T, Batch_Size = c.Batch_Size, groups = c.groups;
    const int32_t* window_len_extra = c.window_len_extra;
    const int64_t mask_row_stride = c.mask_row_stride;
    const int heads_per_mask_row = c.heads_per_mask_row;
    const float sqrt_d = c.sqrt_d;
    float* lse = c.lse;
    // window rows (and the new rows) are read as 16-byte pieces
    if (!aligned16(k_window) || !aligned16(v_window) || (k_new && !aligned16(k_new))) return MUSTAFAR_EINVAL;
    if (T > 0 && (!k_bmp || !k_nz || !k_idx || !v_bmp || !v_nz || !v_idx)) return MUSTAFAR_EINVAL;
    if (T > 0 && !(ext && ext->k_nz_stride) && !k_nz_offset) return MUSTAFAR_EINVAL;
    if (T > 0 && !(ext && ext->v_nz_stride) && !v_nz_offset) return MUSTAFAR_EINVAL;
    const int Bp = Batch_Size / groups, ntb = T / 64;
    const int bpw = blocks_per_wg(ntb, Bp);
    const int S1 = ntb > 0 ? (ntb + bpw - 1) / bpw : 0;
    const int nchunks = (window_capacity + kWinChunk - 1) / kWinChunk;
    float* ws_o = static_cast<float*>(workspace);
    float* ws_ml = ws_o + (int64_t)(S1 + nchunks) * Batch_Size * kD;
    const DecArgs a{static_cast<const h16*>(q), ws_o, ws_ml, static_cast<h16*>(k_window), static_cast<h16*>(v_window),
                    static_cast<const h16*>(k_new), static_cast<const h16*>(v_new), window_len_extra,
                    static_cast<const h16*>(attention_mask), mask_row_stride, heads_per_mask_row > 0 ? heads_per_mask_row : 1,
                    T, Batch_Size, bpw, S1, window_len, window_capacity, (float)(1.0 / (double)sqrt_d)};
    const dim3 grid(S1 + nchunks, Bp);
    hipEvent_t e0 = ev ? ev[0] : nullptr, e1 = ev ? ev[1] : nullptr, e2 = ev ? ev[2] : nullptr, e3 = ev ? ev[3] : nullptr;
    auto kb = k_bmp, vb = v_bmp;
    auto kz = static_cast<const uint4*>(k_nz), vz = static_cast<const uint4*>(v_nz);
#define MUSTAFAR_HD64_L(GG, MM, EE, TAIL)                                                                                                \
    hipExtLaunchKernelGGL((hd64_decode_kernel<GG, MM, EE>), grid, dim3(64), 0, st, e0, e1, 0, kb, kz, k_idx, k_nz_offset, vb, vz, v_idx, \
                          v_nz_offset, a, TAIL)
#define MUSTAFAR_HD64(GG)                                                                                                              \
    do {                                                                                                                               \
        if (ext) {                                                                                                                     \
            if (attention_mask) MUSTAFAR_HD64_L(GG, true, true, *ext); else MUSTAFAR_HD64_L(GG, false, true, *ext);                     \
        } else {                                                                                                                       \
            if (attention_mask) MUSTAFAR_HD64_L(GG, true, false, NoExt{}); else MUSTAFAR_HD64_L(GG, false, false, NoExt{});             \
        }                                                                                                                              \
    } while (0)
    switch (groups) {
        case 1: MUSTAFAR_HD64(1); break;
        case 2: MUSTAFAR_HD64(2); break;
        case 3: MUSTAFAR_HD64(3); break;
        case 4: MUSTAFAR_HD64(4); break;
        case 5: MUSTAFAR_HD64(5); break;
        case 6: MUSTAFAR_HD64(6); break;
        case 7: MUSTAFAR_HD64(7); break;
        default: MUSTAFAR_HD64(8); break;
    }
#undef MUSTAFAR_HD64
#undef MUSTAFAR_HD64_L
    if (lse)
        hipExtLaunchKernelGGL(hd64_finish_kernel<true>, dim3(Batch_Size), dim3(256), 0, st, e2, e3, 0, ws_o, ws_ml, S1 + nchunks, Batch_Size,
                              static_cast<h16*>(out), LseArg{lse});
    else
        hipExtLaunchKernelGGL(hd64_finish_kernel<false>, dim3(Batch_Size), dim3(256), 0, st, e2, e3, 0, ws_o, ws_ml, S1 + nchunks, Batch_Size,
                              static_cast<h16*>(out), NoLse{});
    return (int)hipGetLastError();
}

// A 256-token extent's view as the trigger writes through it: equally spaced regions, rows of at least 256 / 257 entries.
bool extent_view_ok(const mustafar_cache_view& v, int Bp, int64_t region_halfs)
{
    if (!v.bmp || !v.idx || !v.nz || !aligned16(v.nz) || v.nz_head_stride <= 0 || (int64_t)Bp * v.nz_head_stride > 0xffffffffll) return false;
    if ((v.bmp_head_stride && v.bmp_head_stride < 256) || (v.idx_head_stride && v.idx_head_stride < 257)) return false;
    return region_halfs > 0 && region_halfs <= 8 * v.nz_head_stride;
}

}  // namespace

int decode(const DecodeCall& c, hipEvent_t* ev, bool* ran_extents)
{
    *ran_extents = false;
    const mustafar_cache_view* b[2] = {&c.k, &c.v};
    if (c.k.flags || c.v.flags) return MUSTAFAR_EINVAL;   // (token rows are a head_dim 128 form)
    if (!c.k_ext) {   // the plain launch; base views that carry row strides (T == T_base at an extents entry point) must have rows exactly T long
        for (int i = 0; i < 2; i++)
            if ((b[i]->bmp_head_stride && b[i]->bmp_head_stride != c.T) || (b[i]->idx_head_stride && b[i]->idx_head_stride != c.T + 1))
                return MUSTAFAR_EINVAL;
        return launch_decode(c, ev, nullptr);
    }
    const int T_base = c.T_base;   // (T_base > 0, T > T_base and both in whole extents: checked by the dispatcher)
    if ((c.T - T_base) / 256 > kMaxExtents) return MUSTAFAR_EINVAL;
    for (int i = 0; i < 2; i++)
        if ((b[i]->bmp_head_stride && b[i]->bmp_head_stride < T_base) || (b[i]->idx_head_stride && b[i]->idx_head_stride < T_base + 1) ||
            b[i]->nz_head_stride < 0 || b[i]->nz_head_stride > 0xffffffffll)
            return MUSTAFAR_EINVAL;
    const ExtArgs e{c.k_ext, c.v_ext, c.T_device,
                    c.k.bmp_head_stride ? c.k.bmp_head_stride : T_base, c.k.idx_head_stride ? c.k.idx_head_stride : T_base + 1,
                    c.v.bmp_head_stride ? c.v.bmp_head_stride : T_base, c.v.idx_head_stride ? c.v.idx_head_stride : T_base + 1,
                    (uint32_t)c.k.nz_head_stride, (uint32_t)c.v.nz_head_stride, T_base};
    const int err = launch_decode(c, ev, &e);
    *ran_extents = err == 0;
    return err;
}

int trigger_compress_batch(hipStream_t st, int n, const mustafar_trigger_item* items, int64_t head_stride, int Bp, int t, int kth_k, int kth_v,
                           int64_t k_region_halfs, int64_t v_region_halfs)
{
    if (n < 1 || !items || Bp < 1 || t != 256 || head_stride < (int64_t)t * kD || (head_stride & 7) || kth_k < 0 || kth_k > kD || kth_v < 0 ||
        kth_v > kD)
        return MUSTAFAR_EINVAL;
    for (int i = 0; i < n; i++) {   // every item is checked before anything is launched
        const mustafar_trigger_item& it = items[i];
        if (!it.k_window || !it.v_window || !aligned16(it.k_window) || !aligned16(it.v_window) || !it.k_head_total || !it.v_head_total ||
            !it.overflow_flag || !extent_view_ok(it.k_dst, Bp, k_region_halfs) || !extent_view_ok(it.v_dst, Bp, v_region_halfs))
            return MUSTAFAR_EINVAL;
    }
    for (int i = 0; i < n; i++) {
        const mustafar_trigger_item& it = items[i];
        const ExtSide ks{static_cast<const uint16_t*>(it.k_window), it.k_dst.bmp, it.k_dst.idx, static_cast<uint16_t*>(it.k_dst.nz),
                         it.k_dst.nz_offset, it.k_head_total, it.k_dst.bmp_head_stride ? it.k_dst.bmp_head_stride : 256,
                         it.k_dst.idx_head_stride ? it.k_dst.idx_head_stride : 257, k_region_halfs, (uint32_t)it.k_dst.nz_head_stride, kth_k};
        const ExtSide vs{static_cast<const uint16_t*>(it.v_window), it.v_dst.bmp, it.v_dst.idx, static_cast<uint16_t*>(it.v_dst.nz),
                         it.v_dst.nz_offset, it.v_head_total, it.v_dst.bmp_head_stride ? it.v_dst.bmp_head_stride : 256,
                         it.v_dst.idx_head_stride ? it.v_dst.idx_head_stride : 257, v_region_halfs, (uint32_t)it.v_dst.nz_head_stride, kth_v};
        hd64_extent_compress_kernel<<<dim3(Bp, 2), 256, 0, st>>>(ks, vs, head_stride, it.overflow_flag);
    }
    return (int)hipGetLastError();
}

int prefill_compress(hipStream_t st, const void* k_x, const void* v_x, int64_t head_stride, int Bp, int t, int kth_k, int kth_v,
                     const mustafar_cache_view* k_stage, const mustafar_cache_view* v_stage, int64_t k_chunk_bytes, int64_t v_chunk_bytes,
                     mustafar_cache_view* k_pieces, mustafar_cache_view* v_pieces, int64_t* k_head_total, int64_t* v_head_total,
                     int64_t k_region_halfs, int64_t v_region_halfs, int32_t* overflow_flag)
{
    if (Bp < 1 || t < 256 || (t & 255) || t > kMaxExtents * 256 || head_stride < (int64_t)t * kD || (head_stride & 7) || kth_k < 0 ||
        kth_k > kD || kth_v < 0 || kth_v > kD)
        return MUSTAFAR_EINVAL;
    if (!k_x || !v_x || !aligned16(k_x) || !aligned16(v_x) || !k_stage || !v_stage || !k_head_total || !v_head_total || !overflow_flag)
        return MUSTAFAR_EINVAL;
    // chunk c's arrays lie c * chunk_bytes behind chunk 0's: the stream regions stay 16-byte aligned, the other arrays 8 / 4
    if (k_chunk_bytes <= 0 || (k_chunk_bytes & 15) || v_chunk_bytes <= 0 || (v_chunk_bytes & 15)) return MUSTAFAR_EINVAL;
    if (!extent_view_ok(*k_stage, Bp, k_region_halfs) || !extent_view_ok(*v_stage, Bp, v_region_halfs)) return MUSTAFAR_EINVAL;
    const ExtSide ks{static_cast<const uint16_t*>(k_x), k_stage->bmp, k_stage->idx, static_cast<uint16_t*>(k_stage->nz), k_stage->nz_offset,
                     k_head_total, k_stage->bmp_head_stride ? k_stage->bmp_head_stride : 256,
                     k_stage->idx_head_stride ? k_stage->idx_head_stride : 257, k_region_halfs, (uint32_t)k_stage->nz_head_stride, kth_k};
    const ExtSide vs{static_cast<const uint16_t*>(v_x), v_stage->bmp, v_stage->idx, static_cast<uint16_t*>(v_stage->nz), v_stage->nz_offset,
                     v_head_total, v_stage->bmp_head_stride ? v_stage->bmp_head_stride : 256,
                     v_stage->idx_head_stride ? v_stage->idx_head_stride : 257, v_region_halfs, (uint32_t)v_stage->nz_head_stride, kth_v};
    hd64_prefill_compress_kernel<<<dim3(Bp, t / 256, 2), 256, 0, st>>>(ks, vs, head_stride, k_chunk_bytes, v_chunk_bytes, k_pieces, v_pieces,
                                                                       overflow_flag);
    return (int)hipGetLastError();
}

int cache_gather(hipStream_t st, const mustafar_cache_view* dst, const mustafar_cache_view* first, int first_tokens,
                 const mustafar_cache_view* pieces, int n_pieces, int Bp)
{
    if (!dst || Bp < 1 || first_tokens < 0 || (first_tokens & 255) || n_pieces < 0 || n_pieces > kMaxExtents || (first_tokens > 0) != (first != nullptr) ||
        (n_pieces > 0 && !pieces) || first_tokens / 256 + n_pieces < 1 || first_tokens / 256 + n_pieces > 65535)
        return MUSTAFAR_EINVAL;
    const int64_t tokens = (int64_t)first_tokens + 256 * (int64_t)n_pieces;
    GatherArgs a{*dst, first ? *first : mustafar_cache_view{}, pieces, first_tokens, n_pieces};
    mustafar_cache_view* v[2] = {&a.dst, &a.first};
    const int64_t held[2] = {tokens, first_tokens};
    for (int i = 0; i < (first ? 2 : 1); i++) {
        if (!v[i]->bmp || !v[i]->idx || !v[i]->nz || !aligned16(v[i]->nz) || v[i]->nz_head_stride < 0 ||
            (int64_t)Bp * v[i]->nz_head_stride > 0xffffffffll || (!v[i]->nz_head_stride && !v[i]->nz_offset))
            return MUSTAFAR_EINVAL;
        if (!v[i]->bmp_head_stride) v[i]->bmp_head_stride = held[i];
        if (!v[i]->idx_head_stride) v[i]->idx_head_stride = held[i] + 1;
        if (v[i]->bmp_head_stride < held[i] || v[i]->idx_head_stride < held[i] + 1) return MUSTAFAR_EINVAL;
    }
    hd64_gather_kernel<<<dim3(first_tokens / 256 + n_pieces, Bp), 256, 0, st>>>(a);
    return (int)hipGetLastError();
}

int trigger_finish_batch(hipStream_t st, int n, const mustafar_trigger_item* items, int64_t head_stride, int Bp, int len, int drop)
{
    if (n < 1 || !items || Bp < 1 || drop < 0 || len < drop || head_stride < (int64_t)len * kD || (head_stride & 7)) return MUSTAFAR_EINVAL;
    for (int i = 0; i < n; i++)
        if (!items[i].k_window || !items[i].v_window || !aligned16(items[i].k_window) || !aligned16(items[i].v_window)) return MUSTAFAR_EINVAL;
    for (int i = 0; i < n; i++) {
        const mustafar_trigger_item& it = items[i];
        hd64_trigger_finish_kernel<<<dim3(Bp, 2), 256, 0, st>>>(static_cast<uint16_t*>(it.k_window), static_cast<uint16_t*>(it.v_window),
                                                                head_stride, len, drop, it.k_dst, it.v_dst, it.k_table_slot, it.v_table_slot);
    }
    return (int)hipGetLastError();
}

}  // namespace mustafar_hd64
