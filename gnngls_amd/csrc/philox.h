// philox.h -- the counter-based generator of the kernels that draw on the device (sampling_kernels.hip: the sampled walks;
// oropt_kernels.hip: the cut points of a double-bridge kick).  A draw is a pure function of (seed, counter): it never depends on
// the launch shape or on a neighbour.  Streams are kept apart by counter word 3: 0 = the walks' (b, r, step, 0), 1 = the kicks'
// (b, kick, s, 1), 2 = the ants' of aco_kernels.hip (b, iteration * ants + ant, step, 2).  include/gnngls_hip.h states key, counter and the 53-bit formula; tests/test_sampling_cpu.py restates them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gnngls {

// Philox4x32-10 (Salmon et al., SC'11): counter (c0, c1, c2, c3), key (k0, k1) -> the first two output words
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t &o0, uint32_t &o1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o0 = c0; o1 = c1;
}

// the 53-bit uniform in [0,1) of counter (c0, c1, c2, c3) under key (seed & 0xffffffff, seed >> 32)
__device__ __forceinline__ double philox_uniform53(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t o0, o1;
    philox4x32_10(c0, c1, c2, c3, (uint32_t)seed, (uint32_t)(seed >> 32), o0, o1);
    return (double)((((uint64_t)o0 << 32) | o1) >> 11) * 0x1.0p-53;
}

}  // namespace gnngls
