// key_rows.h -- the index arithmetic of token-row key blocks (include/mustafar_hip.h: MUSTAFAR_VIEW_KEY_ROWS), the
// counterpart of value_lists.h: shared by the retile kernels (base_forms.hip) and the decode launch (spmv.hip: key_row_block,
// key_row_share).  Plain C++, no device builtins.
//
// A block of width w (even, 2 .. 128: the most channels a token of the block keeps) is kr_rows(w) rows of 256 bytes, lane t = token t:
//   kr_words(w) = ceil(w / 4) channel rows   64 x 4 bytes: the channels of slots 4j .. 4j + 3
//   w / 2 value rows                         64 x half2: the values of slots 2j, 2j + 1
// A head's blocks lie back to back; its table entry b = the first row of block b << 8 | w.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KR_FN __host__ __device__ inline
#else
#define KR_FN inline
#endif

constexpr int kKrRowBytes = 256;

KR_FN uint32_t kr_entry(uint32_t first_row, uint32_t w) { return (first_row << 8) | w; }
KR_FN int kr_width(uint32_t ent) { return (int)(ent & 0xffu); }
KR_FN uint32_t kr_first_row(uint32_t ent) { return ent >> 8; }
KR_FN int kr_words(int w) { return (w + 3) >> 2; }            // channel rows; a width of 2 mod 4 ends in a half word (one value row)
KR_FN int kr_rows(int w) { return (w >> 1) + kr_words(w); }   // value rows + channel rows
// byte offsets, from the block's start, of slot c of token t: its channel byte and its fp16 value
KR_FN int kr_chan_byte(int t, int c) { return kKrRowBytes * (c >> 2) + 4 * t + (c & 3); }
KR_FN int kr_value_byte(int w, int t, int c) { return kKrRowBytes * (kr_words(w) + (c >> 1)) + 4 * t + 2 * (c & 1); }
