// key_nibble_rows.h -- the index arithmetic of nibble-row key blocks (include/mustafar_hip.h: MUSTAFAR_VIEW_KEY_NIBBLE_ROWS),
// the counterpart of key_rows.h: shared by the retile kernels (base_forms.hip), the decode launch (spmv.hip: key_nibble_rows_phase) and the
// stand-alone host check (tools/key_nibble_rows_check.cpp).  Plain C++, no device builtins.
//
// A slot is an fp16 value and a 4-bit STEP; lane t = token t.  A block of width w (even, 2 .. 128) has two SHARES, one per wave of a pair:
//   front  slots [0, F), F = nr_front(w): the token's first non-zeros, a chain of steps ascending from channel -1
//   back   slots [F, w):                  the rest, a chain descending from channel 128
// A share of n slots is nr_share_rows(n) rows of 256 bytes, the block its two shares back to back:
//   ceil(n / 8) step rows   64 x 4 bytes: the steps of slots 8j .. 8j + 7, slot s in bits 4 (s & 7) ..
//   n / 2 value rows        64 x half2:   the values of slots 2j, 2j + 1
// Step code: 0 = no entry, stay (the padding behind a chain's last entry; value +0); 1 .. 14 = an entry that many channels on;
// 15 = no entry, 14 channels on (a spacer; value +0).  Whether a slot is an entry is told by its step alone.  A gap of g channels takes
// nr_gap_slots(g) slots: its spacers, then the entry with step g - 14 x spacers.  A token's chains are greedy: the front takes entries
// while they fit F slots, the back the rest; w is the smallest even width at which every token of the block fits (128 always does).
// Every position a chain visits lies in [-1, 128].  A head's blocks lie back to back; its table entry b = the first row of block b << 8 | w.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NR_FN __host__ __device__ inline
#else
#define NR_FN inline
#endif

constexpr int kNrRowBytes = 256;
constexpr int kNrSpacer = 15, kNrSpacerStep = 14;

NR_FN uint32_t nr_entry(uint32_t first_row, uint32_t w) { return (first_row << 8) | w; }
NR_FN int nr_width(uint32_t ent) { return (int)(ent & 0xffu); }
NR_FN uint32_t nr_first_row(uint32_t ent) { return ent >> 8; }
NR_FN int nr_front(int w) { return ((w >> 1) + 1) & ~1; }   // even, the larger half: the shares differ by at most one value row
NR_FN int nr_back(int w) { return w - nr_front(w); }
NR_FN int nr_step_rows(int n) { return (n + 7) >> 3; }
NR_FN int nr_share_rows(int n) { return nr_step_rows(n) + (n >> 1); }
NR_FN int nr_rows(int w) { return nr_share_rows(nr_front(w)) + nr_share_rows(nr_back(w)); }
// a share: its slots and its first row in the block (part 0: front, 1: back)
NR_FN int nr_share_slots(int w, int part) { return part ? nr_back(w) : nr_front(w); }
NR_FN int nr_share_first(int w, int part) { return part ? nr_share_rows(nr_front(w)) : 0; }
// byte offsets, from the SHARE's start, of slot s of token t in a share of n slots: the dword of its step row, and its fp16 value
NR_FN int nr_step_dword_byte(int t, int s) { return kNrRowBytes * (s >> 3) + 4 * t; }
NR_FN int nr_step_shift(int s) { return 4 * (s & 7); }
NR_FN int nr_value_byte(int n, int t, int s) { return kNrRowBytes * (nr_step_rows(n) + (s >> 1)) + 4 * t + 2 * (s & 1); }
// the slots a gap of g >= 1 channels takes, and how far a step code moves the chain
NR_FN int nr_gap_slots(int g) { return (g + kNrSpacerStep - 1) / kNrSpacerStep; }
NR_FN int nr_advance(int step) { return step == kNrSpacer ? kNrSpacerStep : step; }

// A token's kept channels: bit c of lo = channel c, bit c of hi = channel 64 + c.
struct NrMask {
    uint64_t lo, hi;
};
NR_FN bool nr_kept(const NrMask& m, int c) { return ((c < 64 ? m.lo >> c : m.hi >> (c - 64)) & 1ull) != 0; }
NR_FN int nr_count(const NrMask& m) { return __builtin_popcountll(m.lo) + __builtin_popcountll(m.hi); }
// The greedy split of a token at front size F: the channel of the last entry the front chain holds (-1: none).
NR_FN int nr_front_last(const NrMask& m, int F)
{
    int prev = -1, slots = 0;
    for (int c = 0; c < 128; c++) {
        if (!nr_kept(m, c)) continue;
        slots += nr_gap_slots(c - prev);
        if (slots > F) break;
        prev = c;
    }
    return prev;
}
// the slots the back chain takes for the entries above channel `last`
NR_FN int nr_back_slots(const NrMask& m, int last)
{
    int prev = 128, slots = 0;
    for (int c = 127; c > last; c--) {
        if (!nr_kept(m, c)) continue;
        slots += nr_gap_slots(prev - c);
        prev = c;
    }
    return slots;
}
NR_FN bool nr_fits(const NrMask& m, int w) { return nr_back_slots(m, nr_front_last(m, nr_front(w))) <= nr_back(w); }
// the smallest even width >= from at which the token fits
NR_FN int nr_token_width(const NrMask& m, int from)
{
    int w = from < 2 ? 2 : (from + 1) & ~1;
    while (w < 128 && !nr_fits(m, w)) w += 2;
    return w;
}
