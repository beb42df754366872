// shared_segment.hip -- decode over ONE compressed copy of a segment that every sequence of a batch shares (a system prompt, a document,
// n samples of one prompt), head_dim 64 and 128, for gfx950.  The C ABI entry points mustafar_decode_shared_segment and
// mustafar_shared_segment_workspace_bytes (include/mustafar_hip.h, ABI 111), and their several-token forms
// mustafar_decode_shared_segment_multi and mustafar_shared_segment_multi_workspace_bytes.
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

#include "expand_block.h"   // the helpers of a block's expansion and the fold of a row's slabs, shared with multi_query.hip

namespace mustafar_shared {
namespace {

struct SegArgs {
    SideArgs k, v;
    const h16* q;     // [n_seqs, kv_heads * G, D]
    float* ws_o;      // [runs, kv_heads, R, D]
    float* ws_ml;     // [runs, kv_heads, R, 2]
    int ntb, bpw, n_seqs, groups, R;
    float inv_sqrt_d;
};

// CHUNKS (mustafar_decode_shared_segment_multi with more than 64 rows per kv head): grid (runs, kv heads, row chunks), the
// workgroup serves local rows [64 z, 64 z + 64) of its kv head -- the same phases on its own rows, one expansion of the block per chunk.
// Without it row0 is the constant 0 and the instantiations are the code they were.
template <int D, int RT, bool CHUNKS = false>
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
    const int row0 = CHUNKS ? 64 * (int)blockIdx.z : 0;
    const int l15 = lane & 15, l4 = lane >> 4;
    const uint16_t* sb = reinterpret_cast<const uint16_t*>(s_stream);

    // q fragments (A operand): lane holds q[row 16 rt + (l & 15)][32 s + 8 (l >> 4) ..+8); rows at or beyond R are zero
    h16x8 qf[RT][KS];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        const int r = row0 + rt * 16 + l15;
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
                const int r = row0 + rt * 16 + 4 * l4 + i;
                if (r < R) a.ws_o[(slab + r) * D + (wave * CT + c) * 16 + l15] = o[rt][c][i];
            }
    if (row0 + srow < R && sq == 0) { a.ws_ml[2 * (slab + row0 + srow)] = M; a.ws_ml[2 * (slab + row0 + srow) + 1] = L; }
}

bool shape_ok(int T, int kv_heads, int groups, int n_seqs, int head_dim)
{
    if (T <= 0 || (T & 63) || kv_heads < 1 || kv_heads > 65535 || groups < 1 || groups > 8 || n_seqs < 1) return false;
    if ((int64_t)n_seqs * groups > kMaxRows) return false;
    return head_dim == 64 || head_dim == 128;
}

// The several-token form: R = n_seqs * groups * n_q rows per kv head, up to 16 chunks of 64
bool multi_shape_ok(int T, int kv_heads, int groups, int n_seqs, int n_q, int head_dim)
{
    if (T <= 0 || (T & 63) || kv_heads < 1 || kv_heads > 65535 || groups < 1 || groups > 8) return false;
    if (n_seqs < 1 || n_seqs > kMaxRowsMulti || n_q < 1 || n_q > kMaxRowsMulti || (int64_t)n_seqs * groups * n_q > kMaxRowsMulti) return false;
    return head_dim == 64 || head_dim == 128;
}

template <int D>
void launch(hipStream_t st, const SegArgs& a, int runs, int kv_heads, h16* out, float* lse)
{
    const dim3 grid(runs, kv_heads, (a.R + kMaxRows - 1) / kMaxRows);
    if (grid.z > 1) shared_segment_decode_kernel<D, 4, true><<<grid, kThreads, 0, st>>>(a);
    else switch ((a.R + 15) / 16) {
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

// ---- several query tokens of every sequence over the one copy: the rows of a (sequence, kv head) are consecutive in
// [n_seqs, kv_heads * G, n_q, D], so the kernel's row addressing holds with G' = G * n_q q rows per (sequence, kv head)

extern "C" int64_t mustafar_shared_segment_multi_workspace_bytes(int T, int kv_heads, int num_key_value_groups, int n_seqs, int n_q, int head_dim)
{
    using namespace mustafar_shared;
    if (!multi_shape_ok(T, kv_heads, num_key_value_groups, n_seqs, n_q, head_dim)) return 0;
    const int R = n_seqs * num_key_value_groups * n_q, ntb = T / 64, bpw = blocks_per_run(R < kMaxRows ? R : kMaxRows, head_dim);
    return (int64_t)((ntb + bpw - 1) / bpw) * kv_heads * R * (head_dim + 2) * (int64_t)sizeof(float);
}

extern "C" int mustafar_decode_shared_segment_multi(void* stream, const mustafar_cache_view* k_cache, const mustafar_cache_view* v_cache, int T,
                                                    int kv_heads, int num_key_value_groups, int n_seqs, int n_q, const void* q, void* out,
                                                    float* lse, void* workspace, float sqrt_d, int head_dim)
{
    using namespace mustafar_shared;
    if (!multi_shape_ok(T, kv_heads, num_key_value_groups, n_seqs, n_q, head_dim) || !(sqrt_d > 0.f)) return MUSTAFAR_EINVAL;
    if (!q || !out || !lse || !workspace || !aligned16(q) || !aligned16(out) || ((uintptr_t)lse & 3) || !aligned16(workspace))
        return MUSTAFAR_EINVAL;
    SegArgs a{};
    if (!side_of(k_cache, T, kv_heads, head_dim, &a.k) || !side_of(v_cache, T, kv_heads, head_dim, &a.v)) return MUSTAFAR_EINVAL;
    const int Gq = num_key_value_groups * n_q, R = n_seqs * Gq, ntb = T / 64, bpw = blocks_per_run(R < kMaxRows ? R : kMaxRows, head_dim);
    const int runs = (ntb + bpw - 1) / bpw;
    a.q = static_cast<const h16*>(q);
    a.ws_o = static_cast<float*>(workspace);
    a.ws_ml = a.ws_o + (int64_t)runs * kv_heads * R * head_dim;
    a.ntb = ntb; a.bpw = bpw; a.n_seqs = n_seqs; a.groups = Gq; a.R = R;
    a.inv_sqrt_d = (float)(1.0 / (double)sqrt_d);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (head_dim == 64) launch<64>(st, a, runs, kv_heads, static_cast<h16*>(out), lse);
    else launch<128>(st, a, runs, kv_heads, static_cast<h16*>(out), lse);
    return (int)hipGetLastError();
}
