// fold_map.h — the integer-grid algebra of exact FP64 folds, shared by stats.hip (the statistics of the mean qualities) and
// score_phred_long.hip (the two per-read folds of very long reads).
//
// While a running value S stays inside one binade [2^e, 2^(e+1)), adding x is integer addition on that binade's grid
// u = 2^(e-52) apart from ties (x/u ending in exactly .5), which round to even and therefore depend on the parity of the running
// integer.  An element is thus a map  m -> m + a[m & 1]  and such maps compose associatively:
//     (a o b)[p] = a[p] + b[(p + a[p]) & 1].
// Subtracting x is the same map negated: the tie candidates of m - t are m - f and m - f - 1, and the even one is picked by the
// same parity rule as for m + t.
#pragma once

#include <hip/hip_runtime.h>

namespace flx_fold {

constexpr int NO_MAP = -2147483647 - 1;  // "no map" in place of a binade exponent

__device__ __forceinline__ int exponent_of(double v) {  // unbiased exponent of a positive normal double
    return (int)((__double_as_longlong(v) >> 52) & 0x7ff) - 1023;
}

struct Map2 {
    long long a0, a1;
};
__device__ __forceinline__ Map2 compose(const Map2 &a, const Map2 &b) {  // a first, then b
    Map2 c;
    c.a0 = a.a0 + ((a.a0 & 1) ? b.a1 : b.a0);
    c.a1 = a.a1 + (((1 + a.a1) & 1) ? b.a1 : b.a0);
    return c;
}

// integer map of one addend v >= 0 (finite) for a running sum in binade e; ok = false if v cannot be added
// without leaving the binade
__device__ __forceinline__ Map2 elem_map(double v, int e, bool &ok) {
    Map2 m;
    m.a0 = m.a1 = 0;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    if ((bits << 1) == 0) return m;  // +-0
    const int eb = (int)((bits >> 52) & 0x7ff);
    unsigned long long mx = bits & 0x000fffffffffffffull;
    int ex;
    if (eb == 0) ex = -1022;  // subnormal
    else { mx |= 1ull << 52; ex = eb - 1023; }
    const int sh = e - ex;  // v / u = mx >> sh
    if (sh < 0) { ok = false; return m; }
    if (sh == 0) { m.a0 = m.a1 = (long long)mx; return m; }
    if (sh >= 55) return m;
    const unsigned long long f = mx >> sh;
    const unsigned long long rem = mx & ((1ull << sh) - 1ull);
    const unsigned long long half = 1ull << (sh - 1);
    if (rem > half) m.a0 = m.a1 = (long long)(f + 1);
    else if (rem < half) m.a0 = m.a1 = (long long)f;
    else {  // tie: the sum rounds to even
        m.a0 = (long long)(f + (f & 1));
        m.a1 = (long long)(f + ((f + 1) & 1));
    }
    return m;
}

__device__ __forceinline__ double readlane_f64(double v, int src) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), src);
    const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ bool normal_positive(double S) {
    const unsigned long long sb = (unsigned long long)__double_as_longlong(S);
    const int eb = (int)((sb >> 52) & 0x7ff);
    return (sb >> 63) == 0 && eb >= 1 && eb <= 2046;
}

}  // namespace flx_fold
