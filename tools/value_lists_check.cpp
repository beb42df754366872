// value_lists_check.cpp -- the index arithmetic of sorted channel lists (mustafar_amd/csrc/value_lists.h) walked on the host: special blocks
// go tiles -> lists -> tiles through the same offset functions the kernels of base_forms.hip use, every access bounds-checked by the
// containers' sizes.  No GPU, no Python:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o value_lists_check tools/value_lists_check.cpp && ./value_lists_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mustafar_amd/csrc/tile_view.h"
#include "../mustafar_amd/csrc/value_lists.h"

namespace {

struct Block {   // 64 tokens x 128 channels: kept flags and fp16 bits
    bool kept[64][128] = {};
    uint16_t val[64][128] = {};
};

struct Half {
    int cnt[64], rank[64];
    unsigned char perm[64], m[kVlMaxRows];
};

Half plan(const uint64_t* bmp)   // as half_plan of base_forms.hip
{
    Half h;
    for (int c = 0; c < 64; c++) {
        h.cnt[c] = 0;
        for (int t = 0; t < 64; t++) h.cnt[c] += tile_bit(bmp[t], c);
    }
    for (int c = 0; c < 64; c++) {
        h.rank[c] = 0;
        for (int o = 0; o < 64; o++) h.rank[c] += h.cnt[o] > h.cnt[c] || (h.cnt[o] == h.cnt[c] && o < c);
        h.perm[h.rank[c]] = (unsigned char)c;
    }
    for (int r = 0; r < kVlMaxRows; r++) {
        int w = 0;
        for (int c = 0; c < 64; c++) w += h.cnt[c] > 2 * r;
        h.m[r] = (unsigned char)w;
    }
    return h;
}

// tiles of one block: 128 bitmaps and one stream per tile (non-zeros in channel order, padded to 8 halfs)
struct Tiles {
    uint64_t bmp[128];
    std::vector<uint16_t> nz[128];
    bool operator==(const Tiles& o) const
    {
        for (int i = 0; i < 128; i++)
            if (bmp[i] != o.bmp[i] || nz[i] != o.nz[i]) return false;
        return true;
    }
};

Tiles to_tiles(const Block& b)
{
    Tiles t;
    for (int half = 0; half < 2; half++)
        for (int tok = 0; tok < 64; tok++) {
            uint64_t m = 0;
            std::vector<uint16_t>& s = t.nz[64 * half + tok];
            for (int c = 0; c < 64; c++)
                if (b.kept[tok][64 * half + c]) {
                    m |= 1ull << (63 - c);
                    s.push_back(b.val[tok][64 * half + c]);
                }
            s.resize((s.size() + 7) & ~size_t(7), 0);
            t.bmp[64 * half + tok] = m;
        }
    return t;
}

std::vector<unsigned char> fill(const Tiles& t)   // as value_lists_fill_kernel, both halves
{
    const Half h0 = plan(t.bmp), h1 = plan(t.bmp + 64);
    const int d0 = vl_word_offset(h0.m, kVlMaxWords), d1 = vl_word_offset(h1.m, kVlMaxWords);
    std::vector<unsigned char> blk(4 * (size_t)vl_block_dwords(d0, d1), 0xee);
    std::fill(blk.begin() + 4 * kVlHalf1Dword, blk.begin() + 4 * kVlHeaderDwords, 0);
    std::fill(blk.begin() + 4 * (kVlHeaderDwords + d0 + d1), blk.end(), 0);
    const uint32_t half1 = (uint32_t)(kVlHeaderDwords + d0);
    std::memcpy(&blk.at(4 * kVlHalf1Dword), &half1, 4);
    for (int half = 0; half < 2; half++) {
        const Half& h = half ? h1 : h0;
        const size_t base = 4 * (size_t)(kVlHeaderDwords + (half ? d0 : 0));
        for (int r = 0; r < kVlMaxRows; r++) blk.at(kVlWidthByte + half * kVlMaxRows + r) = h.m[r];
        for (int c = 0; c < 64; c++) {
            const int i = h.rank[c];
            blk.at(kVlPermByte + half * 64 + i) = (unsigned char)c;
            int s = 0;
            for (int tok = 0; tok < 64; tok++) {
                const uint64_t bits = t.bmp[64 * half + tok];
                if (!tile_bit(bits, c)) continue;
                const int w = vl_word_offset(h.m, s >> 2);
                blk.at(base + vl_token_byte(w, i, s)) = (unsigned char)tok;
                const uint16_t v = t.nz[64 * half + tok].at(tile_rank(bits, c));
                std::memcpy(&blk.at(base + vl_value_byte(h.m, w, i, s)), &v, 2);
                s++;
            }
            if (s & 1) std::memset(&blk.at(base + vl_value_byte(h.m, vl_word_offset(h.m, s >> 2), i, s)), 0, 2);
            for (int q = s; q < vl_token_slots(s); q++) blk.at(base + vl_token_byte(vl_word_offset(h.m, q >> 2), i, q)) = 0;
        }
    }
    return blk;
}

Tiles back(const std::vector<unsigned char>& blk)   // as the three kernels of mustafar_value_lists_to_tiles
{
    Tiles t;
    uint32_t half1;
    std::memcpy(&half1, &blk.at(4 * kVlHalf1Dword), 4);
    for (int i = 0; i < 128; i++) t.bmp[i] = 0;
    for (int pass = 0; pass < 2; pass++)
        for (int half = 0; half < 2; half++) {
            const unsigned char* m = &blk.at(kVlWidthByte + half * kVlMaxRows);
            const size_t base = 4 * (size_t)(half ? half1 : (uint32_t)kVlHeaderDwords);
            if (pass)
                for (int tok = 0; tok < 64; tok++) t.nz[64 * half + tok].assign((__builtin_popcountll(t.bmp[64 * half + tok]) + 7) & ~7, 0);
            for (int i = 0; i < 64; i++) {
                const int c = blk.at(kVlPermByte + half * 64 + i) & 63;
                for (int s = 0; s < 2 * kVlMaxRows && i < m[s >> 1]; s++) {
                    const int w = vl_word_offset(m, s >> 2);
                    const int tok = blk.at(base + vl_token_byte(w, i, s));
                    if (s && !tok) break;
                    if (!pass) t.bmp[64 * half + (tok & 63)] |= 1ull << (63 - c);
                    else {
                        uint16_t v;
                        std::memcpy(&v, &blk.at(base + vl_value_byte(m, w, i, s)), 2);
                        t.nz[64 * half + (tok & 63)].at(tile_rank(t.bmp[64 * half + (tok & 63)], c)) = v;
                    }
                }
            }
        }
    return t;
}

uint32_t rng_state = 12345;
uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

int check(const char* name, const Block& b)
{
    const Tiles t = to_tiles(b);
    const std::vector<unsigned char> blk = fill(t);
    const bool ok = back(blk) == t;
    std::printf("%-28s %5zu bytes  %s\n", name, blk.size(), ok ? "round trip ok" : "MISMATCH");
    return ok ? 0 : 1;
}

}  // namespace

int main()
{
    int bad = 0;
    Block b;
    // random, 30 % kept per token
    for (int t = 0; t < 64; t++)
        for (int c = 0; c < 128; c++)
            if (rnd() % 10 < 3) { b.kept[t][c] = true; b.val[t][c] = (uint16_t)(0x3c00 + rnd() % 512); }
    bad += check("random 30 %", b);
    // a channel kept by all 64 tokens next to a channel kept by none (depth 64, cnt 0)
    Block d = b;
    for (int t = 0; t < 64; t++) { d.kept[t][5] = true; d.val[t][5] = 0x3400; d.kept[t][6] = false; d.kept[t][70] = true; d.val[t][70] = 0xb800; }
    bad += check("depth 64 beside cnt 0", d);
    bad += check("all zero", Block());
    // all lists equal (m_r constant), depth 10 = 2 mod 4: a half word
    Block e;
    for (int t = 0; t < 10; t++)
        for (int c = 0; c < 128; c++) { e.kept[t][c] = true; e.val[t][c] = (uint16_t)(0x3000 + c); }
    bad += check("equal lists, depth 10", e);
    // everything kept: depth 64 in all 128 lanes
    Block f;
    for (int t = 0; t < 64; t++)
        for (int c = 0; c < 128; c++) { f.kept[t][c] = true; f.val[t][c] = (uint16_t)(0x3000 + t); }
    bad += check("dense", f);
    // kept +0 at token 0 and kept -0 at a later token; magnitude ties
    Block z = b;
    z.kept[0][3] = true; z.val[0][3] = 0x0000;
    z.kept[9][3] = true; z.val[9][3] = 0x8000;
    z.kept[0][100] = true; z.val[0][100] = 0x8000;
    for (int c = 0; c < 42; c++) { z.kept[20][c] = true; z.val[20][c] = 0x3e00; }
    bad += check("kept +-0, ties", z);
    // one entry per lane: depth 1, a lone half word
    Block o;
    for (int c = 0; c < 128; c++) { o.kept[c & 63][c] = true; o.val[c & 63][c] = 0x4000; }
    bad += check("depth 1", o);
    return bad ? 1 : 0;
}
