// 8-bit weights of the few-row weight-streaming projections: OCP e4m3 (`e4m3fn`, NOT the fnuz encoding of gfx942) codes with one
// power-of-two fp32 scale per output row (ops.quantize_w8).  Every finite code is a bf16 AND an fp16 value (4-bit exponent, 3-bit
// mantissa, smallest subnormal 2^-9), so a lane widens its codes in registers to the 16-bit MFMA fragment the 16-bit kernel loads
// from the dequantised weight w16 = code * scale, up to the row's scale - a power of two, which commutes with every fp32 addition of
// the accumulation and is multiplied onto the fp32 sum before the epilogue's first rounding: bit-for-bit the 16-bit kernel on w16.
// Storage order of a row's codes: include/vdd_hip.h ("8-bit weight rows").
#ifndef VDD_W8_H
#define VDD_W8_H

#include "vdd_elem.h"

namespace vdd_elem {

typedef __attribute__((ext_vector_type(4))) uint32_t w8_frag_t;      // 8 x 16 bit: one MFMA A / B operand of a lane

// eight e4m3 codes (byte j = element j of the k-step) -> eight elements of the storage type, exact: v_cvt_scalef32_pk_{bf16,f16}_fp8
// with scale 1.0 widens two codes per instruction (op_sel picks the dword's half)
__device__ __forceinline__ uint32_t w8_pair(uint32_t codes, bool high) {
#if VDD_ELEM_IS_BF16
    return high ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(codes, 1.0f, true))
                : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(codes, 1.0f, false));
#else
    return high ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(codes, 1.0f, true))
                : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(codes, 1.0f, false));
#endif
}
__device__ __forceinline__ w8_frag_t w8_widen(uint2 c) {
    return w8_frag_t{w8_pair(c.x, false), w8_pair(c.x, true), w8_pair(c.y, false), w8_pair(c.y, true)};
}

}  // namespace vdd_elem

#endif /* VDD_W8_H */
