// Scalar arithmetic of the float32 / complex64 / complex128 flat table (typed.hip), written so that every
// operation rounds exactly like the reference's compiled kernels (g++ at -O2 on x86-64, std::complex,
// complex division through the compiler runtime's __divsc3 / __divdc3).  This header is the one place
// that knows the complex rules; it compiles for the device (hipcc) and for the host (g++, the CPU test).
//
//   complex * complex   (ac - bd, ad + bc), no contraction (the library builds with -ffp-contract=off)
//   complex * real      component-wise; a real operand is never promoted to a complex one
//   complex / complex   complex128: Smith's method with the runtime's rescaling near the ends of the
//                       exponent range; complex64: the plain formula evaluated in double, rounded once
//   d != 0              a complex value is zero only when both parts are zero
//   conj(a)             (re, -im)
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AMG_HD __host__ __device__ inline
#else
#define AMG_HD inline
#endif

#include <cfloat>
#include <cmath>

namespace amg {
namespace sc {

template <class R>
struct cplx {
    R re, im;
};
using c64 = cplx<float>;
using c128 = cplx<double>;

// the real type F of a value type T (relaxation.h's template parameter F)
template <class T> struct real_of { using type = T; };
template <class R> struct real_of<cplx<R>> { using type = R; };

// T(v) for a real constant v, as `T one = 1.0;` / `T zero = 0.0;` construct it
template <class T> AMG_HD T from_real(double v) { return (T)v; }
template <> AMG_HD c64 from_real<c64>(double v) { return c64{(float)v, 0.0f}; }
template <> AMG_HD c128 from_real<c128>(double v) { return c128{v, 0.0}; }

AMG_HD float add(float a, float b) { return a + b; }
AMG_HD float sub(float a, float b) { return a - b; }
AMG_HD float mul(float a, float b) { return a * b; }
AMG_HD float mulr(float a, float r) { return a * r; }
AMG_HD float div(float a, float b) { return a / b; }
AMG_HD float conj(float a) { return a; }
AMG_HD bool nonzero(float a) { return a != 0.0f; }

template <class R> AMG_HD cplx<R> add(cplx<R> a, cplx<R> b) { return cplx<R>{a.re + b.re, a.im + b.im}; }
template <class R> AMG_HD cplx<R> sub(cplx<R> a, cplx<R> b) { return cplx<R>{a.re - b.re, a.im - b.im}; }
template <class R> AMG_HD cplx<R> mul(cplx<R> a, cplx<R> b)
{
    return cplx<R>{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
template <class R> AMG_HD cplx<R> mulr(cplx<R> a, R r) { return cplx<R>{a.re * r, a.im * r}; }
template <class R> AMG_HD cplx<R> conj(cplx<R> a) { return cplx<R>{a.re, -a.im}; }
template <class R> AMG_HD bool nonzero(cplx<R> a) { return a.re != (R)0 || a.im != (R)0; }

template <class R> AMG_HD R copysign_(R m, R s) { return std::copysign(m, s); }

// The runtime's recovery of infinities and zeros that the formula computed as NaN + i NaN.
template <class R>
AMG_HD void div_recover(R a, R b, R c, R d, R &x, R &y)
{
    if (std::isnan(x) && std::isnan(y)) {
        const R inf = (R)INFINITY;
        if (c == (R)0 && d == (R)0 && (!std::isnan(a) || !std::isnan(b))) {
            x = copysign_(inf, c) * a;
            y = copysign_(inf, c) * b;
        } else if ((std::isinf(a) || std::isinf(b)) && std::isfinite(c) && std::isfinite(d)) {
            a = copysign_(std::isinf(a) ? (R)1 : (R)0, a);
            b = copysign_(std::isinf(b) ? (R)1 : (R)0, b);
            x = inf * (a * c + b * d);
            y = inf * (b * c - a * d);
        } else if ((std::isinf(c) || std::isinf(d)) && std::isfinite(a) && std::isfinite(b)) {
            c = copysign_(std::isinf(c) ? (R)1 : (R)0, c);
            d = copysign_(std::isinf(d) ? (R)1 : (R)0, d);
            x = (R)0 * (a * c + b * d);
            y = (R)0 * (b * c - a * d);
        }
    }
}

// complex128: Smith's method; operands are halved when the larger part of the divisor is at or above
// half the largest double, and scaled up by 2^52 when that part is below 2^-52, or when one part of the
// dividend is subnormal-small while the others are moderate.  A subnormal ratio switches to the
// reassociated form.
AMG_HD c128 div(c128 n, c128 m)
{
    const double RBIG = DBL_MAX / 2, RMIN = DBL_MIN, RMIN2 = DBL_EPSILON, RMINSCAL = 1.0 / DBL_EPSILON;
    const double RMAX2 = RBIG * RMIN2;
    double a = n.re, b = n.im, c = m.re, d = m.im, x, y;
    if (std::fabs(c) < std::fabs(d)) {
        if (std::fabs(d) >= RBIG) { a = a / 2; b = b / 2; c = c / 2; d = d / 2; }
        if (std::fabs(d) < RMIN2) {
            a = a * RMINSCAL; b = b * RMINSCAL; c = c * RMINSCAL; d = d * RMINSCAL;
        } else if ((std::fabs(a) < RMIN && std::fabs(b) < RMAX2 && std::fabs(d) < RMAX2) ||
                   (std::fabs(b) < RMIN && std::fabs(a) < RMAX2 && std::fabs(d) < RMAX2)) {
            a = a * RMINSCAL; b = b * RMINSCAL; c = c * RMINSCAL; d = d * RMINSCAL;
        }
        const double ratio = c / d;
        const double denom = (c * ratio) + d;
        if (std::fabs(ratio) > RMIN) {
            x = ((a * ratio) + b) / denom;
            y = ((b * ratio) - a) / denom;
        } else {
            x = ((c * (a / d)) + b) / denom;
            y = ((c * (b / d)) - a) / denom;
        }
    } else {
        if (std::fabs(c) >= RBIG) { a = a / 2; b = b / 2; c = c / 2; d = d / 2; }
        if (std::fabs(c) < RMIN2) {
            a = a * RMINSCAL; b = b * RMINSCAL; c = c * RMINSCAL; d = d * RMINSCAL;
        } else if ((std::fabs(a) < RMIN && std::fabs(b) < RMAX2 && std::fabs(c) < RMAX2) ||
                   (std::fabs(b) < RMIN && std::fabs(a) < RMAX2 && std::fabs(c) < RMAX2)) {
            a = a * RMINSCAL; b = b * RMINSCAL; c = c * RMINSCAL; d = d * RMINSCAL;
        }
        const double ratio = d / c;
        const double denom = (d * ratio) + c;
        if (std::fabs(ratio) > RMIN) {
            x = ((b * ratio) + a) / denom;
            y = (b - (a * ratio)) / denom;
        } else {
            x = (a + (d * (b / c))) / denom;
            y = (b - (d * (a / c))) / denom;
        }
    }
    div_recover(a, b, c, d, x, y);
    return c128{x, y};
}

// complex64: the plain formula in double (no overflow or underflow is possible there), rounded to float
AMG_HD c64 div(c64 n, c64 m)
{
    const double a = n.re, b = n.im, c = m.re, d = m.im;
    const double denom = (c * c) + (d * d);
    float x = (float)(((a * c) + (b * d)) / denom);
    float y = (float)(((b * c) - (a * d)) / denom);
    div_recover(n.re, n.im, m.re, m.im, x, y);
    return c64{x, y};
}

}  // namespace sc
}  // namespace amg
