// Device primitives shared by the gfx950 kernel files: vector types, the compile-time loop, the bf16 MFMA wrappers, the bf16 rounding
// every bf16 activation is stored with, ReLU on the bit pattern, 16-byte accesses and the packed fp32 forms.  Each exists once, here.
// Included by the kernels_*.hip files only (tests/test_device_prims.py keeps private copies from coming back).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace ukbb {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>)
template <int N, int I = 0, class F>
__device__ __forceinline__ void unroll(F &&f) {
    if constexpr (I < N) { f(std::integral_constant<int, I>{}); unroll<N, I + 1>(f); }
}

// bf16 inputs, fp32 accumulate: one v_mfma_f32_32x32x16_bf16 covers a whole KC = 16 chunk of a tap.
// Lane (m = lane & 31, h = lane >> 5) supplies A[m][k = 8h..8h+7] and B[k = 8h..8h+7][m] as 8 bf16
// (4 dwords, held as f32x4 or u32x4); the accumulator layout is the same as the f32 32x32 form.
__device__ __forceinline__ f32x16 mfma_bf16(const f32x4 &a, const f32x4 &b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_bf16(const u32x4 &a, const u32x4 &b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// v_mfma_f32_16x16x32_bf16: K = 32 as 8 bf16 per lane
__device__ __forceinline__ f32x4 mfma16(const u32x4 &a, const u32x4 &b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
    const __bf16 l = (__bf16)lo, h = (__bf16)hi;       // RNE; hipcc emits v_cvt_pk_bf16_f32
    return (unsigned)__builtin_bit_cast(unsigned short, l) | ((unsigned)__builtin_bit_cast(unsigned short, h) << 16);
}

// UKBB_PREC_F32X3: the three bf16 pieces of two fp32 values, packed pairwise (low half = x0): x = h + m + l with h = bf16(x), m = bf16(x - h),
// l = bf16(x - h - m), every rounding to nearest even and both residuals exact in fp32 (the library is built with -ffp-contract=off).  What the
// third piece leaves is below 2^-24 |x|.  The FCN head (kernels_head.hip) and the X3 convs (kernels_conv_x3.hip) split their B operands with it.
__device__ __forceinline__ void split_pair(float x0, float x1, unsigned &h, unsigned &m, unsigned &l) {
    h = pack_bf16x2(x0, x1);
    const float r0 = x0 - __builtin_bit_cast(float, h << 16), r1 = x1 - __builtin_bit_cast(float, h & 0xffff0000u);
    m = pack_bf16x2(r0, r1);
    const float q0 = r0 - __builtin_bit_cast(float, m << 16), q1 = r1 - __builtin_bit_cast(float, m & 0xffff0000u);
    l = pack_bf16x2(q0, q1);
}

// ReLU as one integer max: for IEEE floats max_i32(bits(x), 0) is x for x >= +0 and +0 for anything
// with the sign bit set.  fmaxf() on an MFMA result compiles to two instructions (a canonicalising
// max and the max), and on gfx950 every VALU instruction takes issue time away from the fp32 MFMA
// stream (tools/mfma_coissue.hip).  Deliberately not inline asm: the compiler must see a VALU read of
// the accumulator to insert the MFMA -> VALU wait states.
__device__ __forceinline__ float relu_bits(float x) {
    const int b = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(float, b > 0 ? b : 0);
}

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, const f32x4 &v) { *reinterpret_cast<f32x4 *>(p) = v; }

// Packed fp32 add / subtract / fma on register pairs.  hipcc scalarises the subtractions of the Winograd input
// transform into v_sub_f32 (+ moves) when left to itself; every VALU instruction of a producer wave
// costs an MFMA slot, so the packed forms are spelled out.
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) { f32x2 r; asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) { f32x2 r; asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b)); return r; }
// a * b + c (v_pk_fma_f32; a scalar factor is splat into a register pair by the caller)
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { f32x2 r; asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

// One leaf of numpy's pairwise summation tree (loops_utils.h.src, pairwise_sum with PW_BLOCKSIZE = 128): the sum of val(0) .. val(n - 1),
// n <= 128, in numpy's order -- plain for n < 8, else 8 interleaved accumulators, their tree, then the remainder.  A = the type numpy
// accumulates in.  The callers (kernels_prep.hip, kernels_score.hip) run one thread per leaf and combine the leaves up numpy's tree.
template <class A, class V>
__device__ __forceinline__ A pairwise_leaf(int n, V &&val) {
    A res;
    if (n < 8) {
        res = 0;
        for (int i = 0; i < n; ++i) res += val(i);
    } else {
        A r0 = val(0), r1 = val(1), r2 = val(2), r3 = val(3), r4 = val(4), r5 = val(5), r6 = val(6), r7 = val(7);
        int i = 8;
        for (; i < n - (n % 8); i += 8) {
            r0 += val(i); r1 += val(i + 1); r2 += val(i + 2); r3 += val(i + 3);
            r4 += val(i + 4); r5 += val(i + 5); r6 += val(i + 6); r7 += val(i + 7);
        }
        res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (; i < n; ++i) res += val(i);
    }
    return res;
}

// Host side of a kernel templated on the class count: f(integral_constant<int, C>{}) for the counts the launchers instantiate
// (n_class 2, 3, 4: the reference's models); false, and no call, for any other.
template <class F>
inline bool with_classes(int n_class, F &&f) {
    switch (n_class) {
        case 2: f(std::integral_constant<int, 2>{}); return true;
        case 3: f(std::integral_constant<int, 3>{}); return true;
        case 4: f(std::integral_constant<int, 4>{}); return true;
        default: return false;
    }
}

}  // namespace ukbb
