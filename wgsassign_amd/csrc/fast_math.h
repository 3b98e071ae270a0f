// The hardware steps of the float32 modes (WGS_MODE_FAST), named once: the scoring kernels (assign_kernels.hip: site_ll_fast), the EM
// kernels (em_kernels.hip: term_fast) and the test hooks (wgs_debug_fast_values, wgs_debug_fast_scan) use these expressions and no
// other.  Everything around them is IEEE float32 arithmetic in a fixed order (the build has -ffp-contract=off), so given the values of
// these two functions the CPU predicts a float32-mode kernel bit for bit (tests/fast_cases.py).
#ifndef WGS_FAST_MATH_H
#define WGS_FAST_MATH_H

// The float32 mode's log of a float32: v_log_f32 (log2) * ln 2.  The instruction flushes a subnormal argument to a zero of its sign
// (assign_kernels.hip: log_special), so every argument below 2^-126 is scaled by 2^32 first -- exact -- and 32 taken off its log2: a
// positive subnormal sum (a likelihood of 1e-40) has its finite log; a negative one, normal or subnormal, stays negative and gives
// NaN; +-0 gives -inf.  A NaN compares false and passes through.  tests/test_gpu_log.py measures the error against log_f32arg over
// every positive float32 (tests/fast_cases.py: FAST_LOG_*).
__device__ __forceinline__ float fast_log(float s)
{
    const bool small = s < 0x1p-126f;
    const float l2 = __builtin_amdgcn_logf(s * (small ? 0x1p32f : 1.0f)) - (small ? 32.0f : 0.0f);
    return l2 * 0.69314718055994530942f;
}

// fast_log for an argument that is NOT below 2^-126 (a positive normal number, +inf or NaN): the same bits without the scaling
// (x * 1 = x and l - 0 = l for every l, NaN included).  The scoring sweep takes it where no lane of a wavefront holds a smaller sum.
__device__ __forceinline__ float fast_log_normal(float s)
{
    return __builtin_amdgcn_logf(s) * 0.69314718055994530942f;
}

// The float32 mode's reciprocal: v_rcp_f32.  It takes a subnormal argument for a zero of its sign and returns a zero where the
// reciprocal is subnormal (tests/test_gpu_log.py counts both over every finite float32), so its callers scale (term_fast).
__device__ __forceinline__ float fast_rcp(float d)
{
    return __builtin_amdgcn_rcpf(d);
}

// g2 = (1 - g0) - g1 as the reference forms it, in double, rounded ONCE to float32: what the float32 modes are handed per (SNP,
// individual).  Formed in float32 it is exactly 0 for the pair (0.001, 0.999), whose double g2 is -1.29e-8: a sum of 0 (-inf) at
// a = 1 where the reference's is negative (NaN), and 12 % off next to it (tests/fast_cases.py).
__device__ __forceinline__ float g2_rounded(float g0, float g1)
{
    return (float)((1.0 - (double)g0) - (double)g1);
}

#endif
