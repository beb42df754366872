// value_pair_lists.h -- the index arithmetic of sorted channel lists over PAIRS of 64-token blocks (include/mustafar_hip.h:
// MUSTAFAR_VIEW_VALUE_PAIR_LISTS), shared by the retile kernels (base_forms.hip), the decode launch (spmv.hip) and a host
// program (tools/value_pair_lists_check.cpp): plain C++, no device builtins, so that a CPU build under a sanitizer walks the same offsets
// the kernels do.
//
// A pair p holds blocks 2p and 2p + 1 of a head: tokens 0..63 are block 2p's, tokens 64..127 block 2p + 1's (a base with an odd number of
// blocks ends in a pair of tokens 0..63 only).  Its storage: a 256-byte header, then half 0 (channels 0..63), then half 1 (channels
// 64..127), padded with zeros to 16 bytes.
//   header bytes   0..127   perm of half 0, perm of half 1: lane i of a half owns channel perm[i] (counted inside the half)
//                128..255   m_r of half 0, m_r of half 1, r = 0..63: the lanes of value row r (0 from the first absent row on)
// A half: words j = 0, 1, ..: token row j (m_{2j} lanes x 4 token bytes), value row 2j (m_{2j} lanes x half2), value row 2j + 1
// (m_{2j+1} lanes x half2; no lanes, no bytes: the half word of a depth of 2 mod 4) -- a word of value_lists.h with tokens of 0..127.
// A channel kept by all 128 tokens fills 64 value rows, so the header has no room for the place of half 1: the block table holds it.
//   table u32 [head][2 pairs + 1], dword offsets from the head's start: entry 2p = the pair's header, entry 2p + 1 = its half 1,
//   entry 2 pairs = the head's dwords.
#pragma once
#include <stdint.h>

#include "value_lists.h"

constexpr int kVplHeaderDwords = kVlHeaderDwords;
constexpr int kVplPermByte = kVlPermByte, kVplWidthByte = kVlWidthByte;
constexpr int kVplMaxRows = 64, kVplMaxWords = 32;
constexpr int kVplAlignDwords = kVlBlockAlignDwords;

VL_FN int vpl_pairs(int blocks) { return (blocks + 1) >> 1; }
VL_FN int vpl_table_columns(int blocks) { return 2 * vpl_pairs(blocks) + 1; }
// the 64-token blocks pair p of a base of `blocks` holds: 2, or 1 for the trailing half pair
VL_FN int vpl_pair_blocks(int blocks, int p) { return 2 * p + 1 < blocks ? 2 : 1; }
// what the two table entries of a pair stand for before the scan: the header with half 0, and half 1 with the padding that keeps the
// next pair 16-byte aligned
VL_FN int vpl_front_dwords(int half0) { return kVplHeaderDwords + half0; }
VL_FN int vpl_back_dwords(int half0, int half1) { return vl_block_dwords(half0, half1) - vpl_front_dwords(half0); }
