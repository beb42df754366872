// value_lists.h -- the index arithmetic of sorted channel lists (include/mustafar_hip.h: MUSTAFAR_VIEW_VALUE_LISTS), shared
// by the retile kernels (base_forms.hip), the decode launch (spmv.hip) and a host program (tools/value_lists_check.cpp): plain C++, no
// device builtins, so that a CPU build under a sanitizer walks the same offsets the kernels do.
//
// A block: a 256-byte header, then half 0 (channels 0..63), then half 1 (channels 64..127), padded with zeros to 16 bytes.
//   header bytes   0..127   perm of half 0, perm of half 1: lane i of a half owns channel perm[i] (counted inside the half)
//                128..191   m_r of half 0, m_r of half 1, r = 0..31: the lanes of value row r (0 from the first absent row on)
//                192..195   u32: the dword offset of half 1 from the block's start (64 + the dwords of half 0)
//                196..255   zero
// A half: words j = 0, 1, ..: token row j (m_{2j} lanes x 4 token bytes), value row 2j (m_{2j} lanes x half2), value row 2j + 1
// (m_{2j+1} lanes x half2; no lanes, no bytes: the half word of a depth of 2 mod 4).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VL_FN __host__ __device__ inline
#else
#define VL_FN inline
#endif

constexpr int kVlHeaderDwords = 64;
constexpr int kVlPermByte = 0, kVlWidthByte = 128, kVlHalf1Dword = 48;
constexpr int kVlMaxRows = 32, kVlMaxWords = 16;
constexpr int kVlBlockAlignDwords = 4;

// A word is the same object in the lists over pairs of blocks (value_pair_lists.h: tokens of 0..127, up to 64 rows): the functions of a
// word exist here, once, for both forms.
// dwords of word j of a half with row widths m[0..]
VL_FN int vl_word_dwords(const unsigned char* m, int j) { return 2 * m[2 * j] + m[2 * j + 1]; }
// dword offset of word j from the half's start (j = the form's MaxWords: the half's size)
VL_FN int vl_word_offset(const unsigned char* m, int j)
{
    int o = 0;
    for (int k = 0; k < j; k++) o += vl_word_dwords(m, k);
    return o;
}
// byte offsets, from the half's start, of slot s of lane i: its token byte and its fp16 value (woff = vl_word_offset(m, s >> 2))
VL_FN int vl_token_byte(int woff, int i, int s) { return 4 * (woff + i) + (s & 3); }
VL_FN int vl_value_byte(const unsigned char* m, int woff, int i, int s)
{
    const int m0 = m[2 * (s >> 2)];
    return 4 * (woff + m0 + ((s & 2) ? m0 : 0) + i) + 2 * (s & 1);
}
// the slots lane i holds, padding included, when its list has cnt entries: whole token rows
VL_FN int vl_token_slots(int cnt) { return (cnt + 3) & ~3; }
VL_FN int vl_block_dwords(int half0, int half1)
{
    return (kVlHeaderDwords + half0 + half1 + kVlBlockAlignDwords - 1) & ~(kVlBlockAlignDwords - 1);
}
