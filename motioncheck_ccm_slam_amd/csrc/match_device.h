// match_device.h -- helpers that more than one of the matcher's kernel files uses (the files: match_types.h).
#pragma once
#include <hip/hip_runtime.h>

// DescriptorDistance (cslam/src/ORBmatcher.cpp:1653-1669) is popcount(a^b) over 8 dwords: v_xor_b32 + v_bcnt_u32_b32 with accumulate.
__device__ __forceinline__ int ham256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1)
{
    int d = __popc(a0.x ^ b0.x);
    d += __popc(a0.y ^ b0.y); d += __popc(a0.z ^ b0.z); d += __popc(a0.w ^ b0.w);
    d += __popc(a1.x ^ b1.x); d += __popc(a1.y ^ b1.y); d += __popc(a1.z ^ b1.z); d += __popc(a1.w ^ b1.w);
    return d;
}

// The rotation bin of an angle difference in degrees (HISTO_LENGTH 30, factor 1/HISTO_LENGTH as the reference writes it: :191, :260)
__host__ __device__ inline int rot_bin(float r)
{
    if (r < 0.0) r += 360.0f;
    int bin = (int)roundf(r * (1.0f / 30));
    if (bin == 30) bin = 0;
    return bin;
}
