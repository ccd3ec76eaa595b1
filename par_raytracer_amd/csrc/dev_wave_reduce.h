// dev_wave_reduce.h - a grid-stride kernel's per-lane partial into one word of memory: reduced over the wave with xor-shuffles,
// then one atomic per wave from its lane 0.  Every lane of the wave calls these together; blockDim.x is a multiple of 64.
// (Compiles for the host through the harnesses' one-lane shims of __shfl_xor / atomicMax: tests/*_host_harness.cpp.)
#pragma once

#include "dev_math.h"

namespace prt {

// The largest m of the grid -> *word as the float's bits: non-negative floats order like their bits, and a wave whose m is 0
// (the word's initial value) has nothing to say.
PRT_D void wave_max_to_word(unsigned int * word, float m) {
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63u) == 0u && m > 0.0f) atomicMax(word, __float_as_uint(m));
}

// The grid's sum of n -> *word.
PRT_D void wave_sum_to_word(unsigned int * word, int n) {
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if ((threadIdx.x & 63u) == 0u && n) atomicAdd(word, (unsigned int)n);
}

}  // namespace prt
