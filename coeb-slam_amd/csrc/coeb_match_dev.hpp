// coeb_match_dev.hpp -- device functions the descriptor matchers share (coeb_match.hip: the
// projection searches, coeb_bow.hip: SearchByBoW): the 256-bit Hamming distance and the
// rotation-consistency histogram (ORBmatcher.cc:1602-1638 and its callers).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

constexpr int HISTO_LENGTH = 30;

__device__ __forceinline__ int hamming32(const uint32_t* a, const uint32_t* b)
{
    int d = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d += __popc(a[i] ^ b[i]);
    return d;
}

__device__ __forceinline__ int rot_bin(float a_last, float a_cur)
{
    float rot = a_last - a_cur;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / HISTO_LENGTH));
    if (bin == HISTO_LENGTH) bin = 0;
    return bin;
}

// ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1602-1638) as selects.  max1 >= max2 >= max3
// holds throughout, so s > max1 implies s > max2 implies s > max3, and each branch of the
// reference's if / else-if chain is one combination of the three tests.  (Written as that chain,
// the compiler addressed the index variables through scratch memory -- a dependent scratch
// round trip per bin, ~20 k cycles of k_match's assignment phase per pair.)
__device__ __forceinline__ void three_maxima(const int* hist, int& ind1, int& ind2, int& ind3)
{
    int max1 = 0, max2 = 0, max3 = 0;
    int i1 = -1, i2 = -1, i3 = -1;
#pragma unroll 6
    for (int i = 0; i < HISTO_LENGTH; i++) {
        const int s = hist[i];
        const bool g1 = s > max1, g2 = s > max2, g3 = s > max3;
        max3 = g2 ? max2 : g3 ? s : max3;
        i3 = g2 ? i2 : g3 ? i : i3;
        max2 = g1 ? max1 : g2 ? s : max2;
        i2 = g1 ? i1 : g2 ? i : i2;
        max1 = g1 ? s : max1;
        i1 = g1 ? i : i1;
    }
    ind1 = i1; ind2 = i2; ind3 = i3;
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}
