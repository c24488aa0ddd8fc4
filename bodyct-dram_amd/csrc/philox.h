// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), the library's one counter-based generator (gfx950).
// A call maps a 128-bit counter and a 64-bit key to four independent 32-bit words: no state, so any lane can produce the
// words of any position of any stream.  Users: noise_kernel (augment.hip), dropout_kernel (act.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace dram {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// key first, the upper half of the counter zero: the form noise_kernel has always used (same bits)
__device__ __forceinline__ void philox4x32_10(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned out[4]) {
    philox4x32_10(c0, c1, 0u, 0u, k0, k1, out);
}

}  // namespace dram
