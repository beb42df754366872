// Host build of the DEVICE branch of mustafar_amd/csrc/select_kth.h for tests/test_select_kth.py: the byte-permute stages of
// bit_transpose32 / gather_bytes compiled with g++, __builtin_amdgcn_perm replaced by a model of v_perm_b32 (selector byte i picks
// byte i of the result from the eight bytes {S0, S1}: values 0..3 are bytes of S1, 4..7 bytes of S0; 12 gives 0x00, 13..15 0xff).
#include <stdint.h>
static inline uint32_t emu_perm(uint32_t s0, uint32_t s1, uint32_t sel)
{
    const uint64_t v = ((uint64_t)s0 << 32) | s1;
    uint32_t d = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t s = (sel >> (8 * i)) & 0xffu;
        const uint32_t b = s < 8 ? (uint32_t)(v >> (8 * s)) & 0xffu : s == 12 ? 0u : 0xffu;   // (8..11, sign replication: not used here)
        d |= b << (8 * i);
    }
    return d;
}
#define __HIP_DEVICE_COMPILE__ 1
#define __host__
#define __device__
#define __forceinline__ inline
#define __builtin_amdgcn_perm(a, b, s) emu_perm((a), (b), (s))
#define __builtin_amdgcn_sched_barrier(x) ((void)0)
#include "../../mustafar_amd/csrc/select_kth.h"
extern "C" void kth_rows(const uint32_t* rows, int n_rows, int kth, int serial, uint32_t* out)
{
    for (int r = 0; r < n_rows; r++) {
        uint32_t raw[64];
        for (int j = 0; j < 64; j++) raw[j] = rows[(long)r * 64 + j];
        out[r] = serial ? kth_magnitude128<true>(raw, kth) : kth_magnitude128<false>(raw, kth);
    }
}
