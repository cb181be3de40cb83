// Exact reduction of a large phase product to a fraction of a turn, shared by caf_propagate.hip, caf_scene.hip and
// caf_cancel.hip, and the float32 unit phasor and complex product of the rotor kernels (caf_propagate.hip, caf_cancel.hip).
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

// exp(j 2 pi t), |t| <= 1/2 turn (+ an ulp): quarter turns in float64, sine and cosine of the rest (<= 1/8 turn) in float32
__device__ __forceinline__ float2 unit_f32(double t) {
    const double q = rint(4.0 * t);
    const float f = (float)(t - 0.25 * q);
    float s, c;
    sincospif(2.0f * f, &s, &c);
    const int qi = (int)q & 3;
    float2 r;
    r.x = qi == 0 ? c : qi == 1 ? -s : qi == 2 ? -c : s;
    r.y = qi == 0 ? s : qi == 1 ? c : qi == 2 ? -s : -c;
    return r;
}

__device__ __forceinline__ float2 cmulf(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}

}  // namespace caf
