// The split-bf16 primitives every matrix-core convolution kernel shares (conv_split, conv1x1_split, wgrad_split, wgrad1x1_split,
// conv_strided): an fp32 operand is split EXACTLY into three bf16 terms and a product is the six significant cross terms,
// accumulated in fp32 (the arithmetic is derived in conv_split.hip's header; tests/test_split_arith_cpu.py restates it in numpy).
// Device-only (inline assembly): not for wgrad_stage_map.h or anything a host compiler sees.
// HAZARD: the compiler does not see cvt_pk_bf16's inline assembly as a vector instruction and pads no wait states behind it.  A
// fragment that goes to LDS first is safe; one that feeds an MFMA straight from registers needs two idle states between the last
// conversion and the matrix instruction (s_nop 1 tied to the fragments, as conv_stem.hip's stem_split8 does) -- without them the MFMA
// can read the registers' previous content, silently.
#pragma once
#include <hip/hip_runtime.h>

namespace cd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// two fp32 -> packed bf16 pair (round to nearest even), low half = a
__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float bf16_lo(unsigned p) { return __uint_as_float(p << 16); }
__device__ __forceinline__ float bf16_hi(unsigned p) { return __uint_as_float(p & 0xffff0000u); }

// (a, b) -> packed pairs of the three split terms
__device__ __forceinline__ void split_pair(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    h = cvt_pk_bf16(a, b);
    const float ra = a - bf16_lo(h), rb = b - bf16_hi(h);
    m = cvt_pk_bf16(ra, rb);
    l = cvt_pk_bf16(ra - bf16_lo(m), rb - bf16_hi(m));
}

// 8 fp32 -> three bf16x8 fragments (hi, mid, lo)
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8 (&f)[3]) {
    u32x4 hh, mm, ll;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        unsigned h, m, l;
        split_pair(v[2 * c], v[2 * c + 1], h, m, l);
        hh[c] = h; mm[c] = m; ll[c] = l;
    }
    f[0] = __builtin_bit_cast(bf16x8, hh); f[1] = __builtin_bit_cast(bf16x8, mm); f[2] = __builtin_bit_cast(bf16x8, ll);
}

// The six products of an accumulator, smallest first: product p multiplies split SPLIT_PA[p] of the A operand with split
// SPLIT_PB[p] of the B operand (0 = hi, 1 = mid, 2 = lo) -- lo x hi, hi x lo, mid x mid, mid x hi, hi x mid, hi x hi.
constexpr int SPLIT_PA[6] = {2, 0, 1, 1, 0, 0}, SPLIT_PB[6] = {0, 2, 1, 0, 1, 0};

}  // namespace cd
