// half_in.h -- real float16 / bfloat16 input read where it lies (xrfthip_dtype XRFTHIP_F16 / XRFTHIP_BF16): the ONE place the float32 families load
// 2-byte samples.  A kernel instantiated with H16 = true reads its input through these loaders and is the float32 kernel from the first register on:
// widening either format to float32 is exact (every float16 / bfloat16 value, subnormals, +-0 and +-inf included, is a float32 value; NaN stays NaN),
// so a half plan's result is the float32 plan's on the widened samples, bit for bit.
//   one loader type per kernel, the format a run-time flag of the parameter block (bf = 0: IEEE float16, 1: bfloat16; wave-uniform) -- two formats
//   do not double the instantiations
//   loads stay vector loads on the float32 kernels' lane <-> sample map: four samples = one 8-byte load where a lane owns four adjacent samples
//   (fasty_cols_kernel), two samples = one 4-byte load where it owns a pair (fasts, fastr, fastg: a wave reads 256 contiguous bytes per instruction)
//   device: v_cvt_f32_f16 for float16, a 16-bit shift for bfloat16; the emulated build decodes float16 in integer arithmetic
#pragma once
#include <cstring>
#include "tile_fft.h"

namespace xrft {

// float32 bits of the float16 value with bits h (h < 65536), integer arithmetic only: exact for every pattern (NaN: payload kept, shifted)
__host__ __device__ __forceinline__ unsigned xrft_f16_bits_to_f32_bits(unsigned h) {
    const unsigned s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 31u) return s | 0x7f800000u | (m << 13);            // inf, NaN
    if (e != 0u) return s | ((e + 112u) << 23) | (m << 13);      // normal: bias 15 -> 127
    if (m == 0u) return s;                                       // +-0
    int p = 9;                                                   // subnormal: m 2^-24, top bit p of m -> exponent p - 24
    while (!((m >> p) & 1u)) --p;
    return s | ((unsigned)(p + 103) << 23) | ((m << (23 - p)) & 0x7fffffu);
}

__device__ __forceinline__ float xrft_bits_as_float(unsigned b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// the two samples of one 32-bit word (little endian: the first sample in the low half)
__device__ __forceinline__ void xrft_widen2(unsigned w, int bf, float& lo, float& hi) {
    if (bf) {
        lo = xrft_bits_as_float(w << 16);
        hi = xrft_bits_as_float(w & 0xffff0000u);
        return;
    }
#ifdef XRFT_EMULATE
    lo = xrft_bits_as_float(xrft_f16_bits_to_f32_bits(w & 0xffffu));
    hi = xrft_bits_as_float(xrft_f16_bits_to_f32_bits(w >> 16));
#else
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 v = __builtin_bit_cast(h2, w);
    lo = (float)v.x;
    hi = (float)v.y;
#endif
}

struct alignas(8) XrftU2 { unsigned x, y; };

// two adjacent samples: one aligned 4-byte load
__device__ __forceinline__ C2<float> xrft_load2_h16(const char* src, int bf) {
    C2<float> r;
    xrft_widen2(*reinterpret_cast<const unsigned*>(src), bf, r.re, r.im);
    return r;
}

// one sample (the unpacked paths of odd row lengths only: the float32 kernels load one sample per lane there, too)
__device__ __forceinline__ float xrft_load1_h16(const char* src, int bf) {
    float lo, hi;
    xrft_widen2((unsigned)*reinterpret_cast<const unsigned short*>(src), bf, lo, hi);
    return lo;
}

}  // namespace xrft
