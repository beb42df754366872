// value_pair_lists_check.cpp -- the index arithmetic of sorted channel lists over pairs of blocks (mustafar_amd/csrc/value_pair_lists.h)
// walked on the host: special pairs go tiles -> lists -> tiles through the same offset functions the kernels of base_forms.hip use, every
// access bounds-checked by the containers' sizes.  One line per pair: its name, its size and the CRC-32 of its bytes, which
// tests/test_value_pair_lists_host.py holds to the NumPy reference's.  No GPU, no Python:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o value_pair_lists_check tools/value_pair_lists_check.cpp && ./value_pair_lists_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mustafar_amd/csrc/value_pair_lists.h"

namespace {

struct Pair {   // ntok (64: a trailing half pair, or 128) tokens x 128 channels: kept flags and fp16 bits
    int ntok = 128;
    bool kept[128][128] = {};
    uint16_t val[128][128] = {};
};

bool bit(uint64_t m, int c) { return (m >> (63 - c)) & 1ull; }
int rank_of(uint64_t m, int c) { return c ? __builtin_popcountll(m >> (64 - c)) : 0; }

struct Half {
    int cnt[64], rank[64];
    unsigned char perm[64], m[kVplMaxRows];
};

// tiles of one pair: per half and token a bitmap and a stream (non-zeros in channel order, padded to 8 halfs)
struct Tiles {
    int ntok;
    uint64_t bmp[2][128];
    std::vector<uint16_t> nz[2][128];
    bool operator==(const Tiles& o) const
    {
        if (ntok != o.ntok) return false;
        for (int h = 0; h < 2; h++)
            for (int i = 0; i < ntok; i++)
                if (bmp[h][i] != o.bmp[h][i] || nz[h][i] != o.nz[h][i]) return false;
        return true;
    }
};

Half plan(const uint64_t* bmp, int ntok)   // as half_plan of base_forms.hip
{
    Half h;
    for (int c = 0; c < 64; c++) {
        h.cnt[c] = 0;
        for (int t = 0; t < ntok; t++) h.cnt[c] += bit(bmp[t], c);
    }
    for (int c = 0; c < 64; c++) {
        h.rank[c] = 0;
        for (int o = 0; o < 64; o++) h.rank[c] += h.cnt[o] > h.cnt[c] || (h.cnt[o] == h.cnt[c] && o < c);
        h.perm[h.rank[c]] = (unsigned char)c;
    }
    for (int r = 0; r < kVplMaxRows; r++) {
        int w = 0;
        for (int c = 0; c < 64; c++) w += h.cnt[c] > 2 * r;
        h.m[r] = (unsigned char)w;
    }
    return h;
}

Tiles to_tiles(const Pair& p)
{
    Tiles t;
    t.ntok = p.ntok;
    for (int half = 0; half < 2; half++)
        for (int tok = 0; tok < p.ntok; tok++) {
            uint64_t m = 0;
            std::vector<uint16_t>& s = t.nz[half][tok];
            for (int c = 0; c < 64; c++)
                if (p.kept[tok][64 * half + c]) {
                    m |= 1ull << (63 - c);
                    s.push_back(p.val[tok][64 * half + c]);
                }
            s.resize((s.size() + 7) & ~size_t(7), 0);
            t.bmp[half][tok] = m;
        }
    return t;
}

// a pair's storage and the two numbers the plan pass leaves in the block table for it
struct Stored {
    std::vector<unsigned char> bytes;
    uint32_t front, back;   // header + half 0; half 1 + padding
};

Stored fill(const Tiles& t)   // as value_lists_size_kernel + value_lists_fill_kernel over PairLists, both halves
{
    const Half h0 = plan(t.bmp[0], t.ntok), h1 = plan(t.bmp[1], t.ntok);
    const int d0 = vl_word_offset(h0.m, kVplMaxWords), d1 = vl_word_offset(h1.m, kVplMaxWords);
    Stored s;
    s.front = (uint32_t)vpl_front_dwords(d0);
    s.back = (uint32_t)vpl_back_dwords(d0, d1);
    std::vector<unsigned char>& blk = s.bytes;
    blk.assign(4 * (size_t)(s.front + s.back), 0xee);
    std::fill(blk.begin() + 4 * (size_t)(s.front + d1), blk.end(), 0);
    for (int half = 0; half < 2; half++) {
        const Half& h = half ? h1 : h0;
        const size_t base = 4 * (size_t)(half ? s.front : (uint32_t)kVplHeaderDwords);
        for (int r = 0; r < kVplMaxRows; r++) blk.at(kVplWidthByte + half * kVplMaxRows + r) = h.m[r];
        for (int c = 0; c < 64; c++) {
            const int i = h.rank[c];
            blk.at(kVplPermByte + half * 64 + i) = (unsigned char)c;
            int n = 0;
            for (int tok = 0; tok < t.ntok; tok++) {
                const uint64_t bits = t.bmp[half][tok];
                if (!bit(bits, c)) continue;
                const int w = vl_word_offset(h.m, n >> 2);
                blk.at(base + vl_token_byte(w, i, n)) = (unsigned char)tok;
                const uint16_t v = t.nz[half][tok].at(rank_of(bits, c));
                std::memcpy(&blk.at(base + vl_value_byte(h.m, w, i, n)), &v, 2);
                n++;
            }
            if (n & 1) std::memset(&blk.at(base + vl_value_byte(h.m, vl_word_offset(h.m, n >> 2), i, n)), 0, 2);
            for (int q = n; q < vl_token_slots(n); q++) blk.at(base + vl_token_byte(vl_word_offset(h.m, q >> 2), i, q)) = 0;
        }
    }
    return s;
}

Tiles back(const Stored& st, int ntok)   // as the kernels of mustafar_value_pair_lists_to_tiles
{
    const std::vector<unsigned char>& blk = st.bytes;
    Tiles t;
    t.ntok = ntok;
    for (int h = 0; h < 2; h++)
        for (int i = 0; i < 128; i++) t.bmp[h][i] = 0;
    for (int pass = 0; pass < 2; pass++)
        for (int half = 0; half < 2; half++) {
            const unsigned char* m = &blk.at(kVplWidthByte + half * kVplMaxRows);
            const size_t base = 4 * (size_t)(half ? st.front : (uint32_t)kVplHeaderDwords);
            if (pass)
                for (int tok = 0; tok < ntok; tok++) t.nz[half][tok].assign((__builtin_popcountll(t.bmp[half][tok]) + 7) & ~7, 0);
            for (int i = 0; i < 64; i++) {
                const int c = blk.at(kVplPermByte + half * 64 + i) & 63;
                for (int s = 0; s < 2 * kVplMaxRows && i < m[s >> 1]; s++) {
                    const int w = vl_word_offset(m, s >> 2);
                    int tok = blk.at(base + vl_token_byte(w, i, s));
                    if (s && !tok) break;
                    tok &= ntok - 1;
                    if (!pass) t.bmp[half][tok] |= 1ull << (63 - c);
                    else {
                        uint16_t v;
                        std::memcpy(&v, &blk.at(base + vl_value_byte(m, w, i, s)), 2);
                        t.nz[half][tok].at(rank_of(t.bmp[half][tok], c)) = v;
                    }
                }
            }
        }
    return t;
}

uint32_t crc32(const std::vector<unsigned char>& d)
{
    uint32_t c = 0xffffffffu;
    for (unsigned char b : d) {
        c ^= b;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}

int check(const char* name, const Pair& p)
{
    const Tiles t = to_tiles(p);
    const Stored s = fill(t);
    const bool ok = back(s, p.ntok) == t && s.bytes.size() % 16 == 0;
    std::printf("%-24s %6zu bytes  half1 %5u  crc %08x  %s\n", name, s.bytes.size(), s.front, crc32(s.bytes), ok ? "round trip ok" : "MISMATCH");
    return ok ? 0 : 1;
}

// the pattern the test builds in NumPy too: 30 % kept, values from the position
Pair pattern(int ntok)
{
    Pair p;
    p.ntok = ntok;
    for (int t = 0; t < ntok; t++)
        for (int c = 0; c < 128; c++)
            if ((t * 7 + c * 13 + (t * c) % 11) % 10 < 3) { p.kept[t][c] = true; p.val[t][c] = (uint16_t)(0x3c00 + ((t * 131 + c * 17) & 511)); }
    return p;
}

}  // namespace

int main()
{
    int bad = 0;
    const Pair b = pattern(128);
    bad += check("pattern", b);
    // a channel kept by all 128 tokens next to a channel kept by none (depth 128: 64 value rows, 32 words; cnt 0)
    Pair d = b;
    for (int t = 0; t < 128; t++) { d.kept[t][5] = true; d.val[t][5] = 0x3400; d.kept[t][6] = false; d.kept[t][70] = true; d.val[t][70] = 0xb800; }
    bad += check("depth_128_beside_cnt_0", d);
    bad += check("all_zero", Pair());
    // all lists equal (m_r constant), depth 10 = 2 mod 4 over both blocks: a half word
    Pair e;
    for (int k = 0; k < 10; k++)
        for (int c = 0; c < 128; c++) { const int t = k < 5 ? k : 59 + k; e.kept[t][c] = true; e.val[t][c] = (uint16_t)(0x3000 + c); }
    bad += check("equal_lists_depth_10", e);
    // a trailing half pair: tokens 0..63 only
    bad += check("trailing_half_pair", pattern(64));
    // everything kept: depth 128 in all 128 lanes
    Pair f;
    for (int t = 0; t < 128; t++)
        for (int c = 0; c < 128; c++) { f.kept[t][c] = true; f.val[t][c] = (uint16_t)(0x3000 + t); }
    bad += check("dense", f);
    // kept +0 at token 0 and kept -0 at later tokens
    Pair z = b;
    z.kept[0][3] = true; z.val[0][3] = 0x0000;
    z.kept[9][3] = true; z.val[9][3] = 0x8000;
    z.kept[64][100] = true; z.val[64][100] = 0x8000;
    bad += check("kept_zeros", z);
    // one entry per lane: depth 1, a lone half word
    Pair o;
    for (int c = 0; c < 128; c++) { o.kept[c][c] = true; o.val[c][c] = 0x4000; }
    bad += check("depth_1", o);
    return bad ? 1 : 0;
}
