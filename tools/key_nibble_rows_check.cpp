// key_nibble_rows_check.cpp -- the index arithmetic of nibble-row key blocks (mustafar_amd/csrc/key_nibble_rows.h) walked on the host: the
// special blocks of tests/key_nibble_rows_ref.py go (kept, values) -> nibble rows -> (kept, values) through the same functions the kernels
// of base_forms.hip use, every access bounds-checked by the container's size.  One line per block: its name, its width, its size and the
// CRC-32 of its bytes, which tests/test_key_nibble_rows_host.py holds to the NumPy reference's.  No GPU, no Python:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o key_nibble_rows_check tools/key_nibble_rows_check.cpp && ./key_nibble_rows_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../mustafar_amd/csrc/key_nibble_rows.h"

namespace {

struct Block {   // 64 tokens x 128 channels: kept flags and fp16 bits
    bool kept[64][128] = {};
    uint16_t val[64][128] = {};
    bool operator==(const Block& o) const { return !memcmp(kept, o.kept, sizeof kept) && !memcmp(val, o.val, sizeof val); }
};

uint16_t value_of(int t, int c) { return (uint16_t)(0x3800 + ((37 * t + 11 * c) & 0x3ff)); }

// the patterns of tests/key_nibble_rows_ref.py: special_block()
const char* const kNames[] = {"full_beside_two", "ends", "steps_14_15_28_29", "kept_zeros", "w_mod8_0", "w_mod8_2", "w_mod8_4", "w_mod8_6", "front_alone"};
Block special(int which)
{
    Block b;
    bool zero[64] = {};
    uint16_t zero_bits[64] = {};
    for (int t = 0; t < 64; t++) {
        switch (which) {
        case 0:
            b.kept[t][5] = b.kept[t][100] = true;
            if (t == 7) for (int c = 0; c < 128; c++) b.kept[t][c] = true;
            break;
        case 1:
            if (t % 4 == 0 || t % 4 == 2) b.kept[t][0] = true;
            if (t % 4 == 1 || t % 4 == 2) b.kept[t][127] = true;
            break;
        case 2: {
            static const int gaps[4] = {14, 15, 28, 29};
            const int g = gaps[t % 4];
            if (t == 63) {
                for (int c = 0; c < 32; c++) b.kept[t][c] = b.kept[t][96 + c] = true;
            } else if ((t / 4) % 2 == 0) {
                for (int c = 0; c < 32; c++) b.kept[t][c] = true;
                for (int c = 128 - g; c > 39; c -= g) b.kept[t][c] = true;
            } else {
                for (int c = 96; c < 128; c++) b.kept[t][c] = true;
                for (int c = g - 1; c < 88; c += g) b.kept[t][c] = true;
            }
            break;
        }
        case 3:
            for (int c = 0; c < 128; c++) b.kept[t][c] = (c * 37 + 11 * t) % 128 < 40;
            if (t % 2 == 0) { zero[t] = true; zero_bits[t] = t % 4 == 0 ? 0x0000 : 0x8000; }
            break;
        case 4: case 5: case 6: case 7:
            for (int i = 0; i < 40 + 2 * (which - 4); i++) b.kept[t][(i * 3 + t) % 128] = true;
            break;
        case 8:
            if (t % 2 == 0) b.kept[t][3] = true;
            else b.kept[t][2] = b.kept[t][9] = true;
            break;
        }
        for (int c = 0; c < 128; c++)
            if (b.kept[t][c]) b.val[t][c] = zero[t] ? zero_bits[t] : value_of(t, c);
    }
    return b;
}

NrMask mask_of(const Block& b, int t)
{
    NrMask m{0ull, 0ull};
    for (int c = 0; c < 64; c++) {
        m.lo |= (uint64_t)b.kept[t][c] << c;
        m.hi |= (uint64_t)b.kept[t][64 + c] << c;
    }
    return m;
}

// one share of one token, written slot by slot (as NibbleShareWriter of base_forms.hip)
struct Writer {
    std::vector<unsigned char>& blk;
    int first, n, t, s;
    void put(int step, uint16_t v)
    {
        if (s >= n) { fprintf(stderr, "a chain outgrew its share\n"); exit(1); }
        uint32_t word;
        const int at = first + nr_step_dword_byte(t, s);
        memcpy(&word, &blk.at(at), 4);
        blk.at(at + 3);
        word |= (uint32_t)step << nr_step_shift(s);
        memcpy(&blk.at(at), &word, 4);
        const int av = first + nr_value_byte(n, t, s);
        blk.at(av + 1);
        memcpy(&blk.at(av), &v, 2);
        s++;
    }
    void gap(int g, uint16_t v)
    {
        for (; g > kNrSpacerStep; g -= kNrSpacerStep) put(kNrSpacer, 0);
        put(g, v);
    }
};

std::vector<unsigned char> encode(const Block& b, int* width)
{
    int w = 2;
    for (int t = 0; t < 64; t++) {
        const NrMask m = mask_of(b, t);
        const int wt = nr_token_width(m, nr_count(m));
        if (wt > w) w = wt;
    }
    *width = w;
    std::vector<unsigned char> blk((size_t)kNrRowBytes * nr_rows(w), 0);   // (zeros: steps of 0 and values of +0 behind every chain)
    for (int t = 0; t < 64; t++) {
        const NrMask m = mask_of(b, t);
        const int last = nr_front_last(m, nr_front(w));
        Writer front{blk, 0, nr_front(w), t, 0};
        for (int d = 0, prev = -1; d <= last; d++)
            if (nr_kept(m, d)) { front.gap(d - prev, b.val[t][d]); prev = d; }
        Writer back{blk, kNrRowBytes * nr_share_first(w, 1), nr_back(w), t, 0};
        for (int d = 127, prev = 128; d > last; d--)
            if (nr_kept(m, d)) { back.gap(prev - d, b.val[t][d]); prev = d; }
    }
    return blk;
}

Block decode(const std::vector<unsigned char>& blk, int w)
{
    Block b;
    for (int t = 0; t < 64; t++)
        for (int part = 0; part < 2; part++) {
            const int first = kNrRowBytes * nr_share_first(w, part), n = nr_share_slots(w, part);
            int pos = part ? 128 : -1;
            for (int s = 0; s < n; s++) {
                uint32_t word;
                blk.at(first + nr_step_dword_byte(t, s) + 3);
                memcpy(&word, &blk.at(first + nr_step_dword_byte(t, s)), 4);
                const int step = (word >> nr_step_shift(s)) & 15;
                pos += part ? -nr_advance(step) : nr_advance(step);
                if (pos < -1 || pos > 128) { fprintf(stderr, "a chain left the table: token %d position %d\n", t, pos); exit(1); }
                if (step == 0 || step == kNrSpacer) continue;   // (every slot is walked: padding stays where it is)
                if (pos < 0 || pos > 127) { fprintf(stderr, "an entry outside the channels: token %d position %d\n", t, pos); exit(1); }
                uint16_t v;
                blk.at(first + nr_value_byte(n, t, s) + 1);
                memcpy(&v, &blk.at(first + nr_value_byte(n, t, s)), 2);
                b.kept[t][pos] = true;
                b.val[t][pos] = v;
            }
        }
    return b;
}

uint32_t crc32_of(const std::vector<unsigned char>& d)
{
    uint32_t c = 0xffffffffu;
    for (unsigned char x : d) {
        c ^= x;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}

}  // namespace

int main()
{
    for (int i = 0; i < (int)(sizeof kNames / sizeof kNames[0]); i++) {
        const Block b = special(i);
        int w = 0;
        const std::vector<unsigned char> blk = encode(b, &w);
        if (!(decode(blk, w) == b)) {
            fprintf(stderr, "%s: the round trip is not the identity\n", kNames[i]);
            return 1;
        }
        printf("%s %d %zu %08x\n", kNames[i], w, blk.size(), crc32_of(blk));
    }
    return 0;
}
