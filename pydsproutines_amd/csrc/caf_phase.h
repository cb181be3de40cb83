// Exact reduction of a large phase product to a fraction of a turn, shared by caf_propagate.hip and caf_scene.hip.
#pragma once

// No contraction from here on: with it the compiler may fuse the product p of mul_split into p - w, and the residual e is then
// counted twice (an error of an ulp of the product: 1e-8 turn at 1e8 turns).  Both files that include this turn it off anyway.
#pragma clang fp contract(off)

namespace caf {

// a b = whole + rest exactly up to the last rounding of rest: whole the nearest integer of the rounded product, |rest| <= 1/2 + ulp
__device__ __forceinline__ void mul_split(double a, double b, double* whole, double* rest) {
    const double p = a * b;
    const double e = fma(a, b, -p);
    const double w = rint(p);
    *whole = w;
    *rest = (p - w) + e;
}

__device__ __forceinline__ double frac_turn(double t) { return t - rint(t); }

}  // namespace caf
