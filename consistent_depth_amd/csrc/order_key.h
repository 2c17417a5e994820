// Order-preserving integer image of a float32: what the exact selections (scale.hip's median, visualize.hip's percentiles) radix-sort on.
#pragma once
#include <hip/hip_runtime.h>

namespace cd {

__device__ __forceinline__ unsigned order_key(float x) {        // monotonic: a < b  <=>  key(a) < key(b)  (-0 < +0: both are the value 0)
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

}  // namespace cd
