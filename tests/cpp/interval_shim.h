// interval_shim.h -- lets g++ compile the text the code generator emits for the GPU (sample_codegen.h: the prelude, the math and
// volume preludes, struct SdfkK, sdf_eval, sdf_interval) as plain host C++, for tests/test_interval_codegen.py.  Nothing here
// restates a formula of that text: the device qualifiers vanish and three device builtins get host meanings.
#pragma once
#include <cstdint>
#include <cstring>

#define __device__
#define __forceinline__ inline
#define __constant__

static inline float __uint_as_float(unsigned u) { float f; memcpy(&f, &u, 4); return f; }

// clang's IEEE 754:2019 maximum / minimum (g++ has neither builtin): NaN if either operand is NaN, -0 < +0.
static inline float sdfk_shim_maximum(float a, float b)
{
    if (a != a) return a;
    if (b != b) return b;
    if (a == b) return __builtin_signbit(b) ? a : b;
    return b < a ? a : b;
}
static inline float sdfk_shim_minimum(float a, float b)
{
    if (a != a) return a;
    if (b != b) return b;
    if (a == b) return __builtin_signbit(a) ? a : b;
    return a < b ? a : b;
}
#define __builtin_elementwise_maximum(a, b) sdfk_shim_maximum(a, b)
#define __builtin_elementwise_minimum(a, b) sdfk_shim_minimum(a, b)

// One "lane": the ballot of a predicate is that predicate.  In sdfk_sqrt the ballot then selects __builtin_sqrtf exactly when the
// operand is outside the short path (NaN, zero, negative, below 2^-96, +inf), and inside it the shim's reciprocal square root
// feeds one correction step with exact FMA residuals.  Whether the DEVICE's v_rsq_f32 makes that short path correctly rounded is
// the business of tests/test_gpu_sqrt_exhaustive.py; the host build only has to return the correctly rounded root for every
// operand, which tests/test_interval_codegen.py::test_host_sqrt_is_correctly_rounded asserts.
#define __builtin_amdgcn_ballot_w64(p) ((p) ? 1ull : 0ull)
#define __builtin_amdgcn_rsqf(x) (1.0f / __builtin_sqrtf(x))
