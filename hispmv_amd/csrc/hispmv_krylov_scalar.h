// hispmv_krylov_scalar.h -- the scalar rules of the Krylov recurrences (include/hispmv.h: THE UPDATES), written once for
// hispmv_krylov.hip (one scalar block per solve, every thread runs the rule) and hispmv_krylov_multi.hip (one block per column, one
// thread per column runs it).  A rule takes a loaded scalar block S (KrylovScalar) and the fp64 sums its kernel has just finished from
// their partials, moves S on by one step, and returns whether the vector pass behind it acts, with the coefficient of that pass
// rounded ONCE to fp32.  A rule that does not act leaves its coefficient alone.  The caller has seen that S is not frozen (but for
// krylov_rule_init) and puts the answer where its layout wants it.  These lines decide breakdown, freezing and iteration counts: both
// kernel files promise them bit for bit against tests/krylov_model.py.
#pragma once
#include <hip/hip_runtime.h>

#include "hispmv_krylov.h"

namespace hispmv {

// zero, infinite or NaN: no denominator
__device__ __forceinline__ bool bad(double d) { return !(d != 0.0 && fabs(d) <= 1.7976931348623157e308); }
__device__ __forceinline__ bool finite_d(double d) { return fabs(d) <= 1.7976931348623157e308; }
// done or broken down: every later pass leaves the block and its vectors as they are
__device__ __forceinline__ bool frozen(const double* S) { return S[kKsDone] != 0.0 || S[kKsBreakdown] != 0.0; }

// The block from nothing: b2 = (b, b), bb = the reference of the stopping rule ((b, b); CGLS: (A^T b, A^T b)), alpha = omega = 1.
// b = 0: done, and x is to be zeroed (zero_x = 1, otherwise left alone).  A reference that is zero or not finite, or a b2 that is
// not: breakdown.
template <class Flag>
__device__ __forceinline__ void krylov_rule_init(double S[kKrylovState], double b2, double bb, double products, Flag& zero_x) {
#pragma unroll
    for (int i = 0; i < kKrylovState; ++i) S[i] = 0.0;
    S[kKsB2] = b2; S[kKsBb] = bb; S[kKsProducts] = products; S[kKsAlpha] = 1.0; S[kKsOmega] = 1.0;
    if (b2 == 0.0) { S[kKsDone] = 1.0; zero_x = 1; }
    else if (bad(bb) || !finite_d(b2)) S[kKsBreakdown] = 1.0;
}

// The dot pass behind the first product: rr and rho of the initial residual; rr <= rtol^2 * bb: done before any update.
__device__ __forceinline__ void krylov_rule_first(double S[kKrylovState], double rr, double rho, double tol2) {
    S[kKsRr] = rr; S[kKsRho] = rho;
    if (rr <= tol2 * S[kKsBb]) S[kKsDone] = 1.0;
}

// alpha = rho / den.  CG: den = (p, q), CGLS: (q, q); den zero or not finite, or rho not finite: breakdown; counts the update.
// BiCGSTAB: den = (rhat, v); den or rho zero or not finite: breakdown; its update is counted by krylov_rule_bicg_omega.
template <bool kBicg>
__device__ __forceinline__ bool krylov_rule_alpha(double S[kKrylovState], double den, float& a32) {
    S[kKsDen] = den;
    if (bad(den) || (kBicg ? bad(S[kKsRho]) : !finite_d(S[kKsRho]))) { S[kKsBreakdown] = 1.0; return false; }
    const double alpha = S[kKsRho] / den;
    S[kKsAlpha] = alpha;
    if (!kBicg) S[kKsIters] += 1.0;
    a32 = (float)alpha;
    return true;
}

// CG and CGLS: the stopping rule on the new rr, then beta = rho' / rho.  The old rho zero or not finite, or rho' not finite: breakdown.
__device__ __forceinline__ bool krylov_rule_direction(double S[kKrylovState], double rr, double rho, double tol2, float& b32) {
    S[kKsRr] = rr;
    if (rr <= tol2 * S[kKsBb]) { S[kKsDone] = 1.0; S[kKsRho] = rho; return false; }
    if (bad(S[kKsRho]) || !finite_d(rho)) { S[kKsBreakdown] = 1.0; return false; }
    b32 = (float)(rho / S[kKsRho]);
    S[kKsRho] = rho;
    return true;
}

// BiCGSTAB: (s, s) <= rtol^2 * bb: done on the half step x += alpha32 p (returns 1).  Otherwise omega = (t, s) / (t, t) and the whole
// step (returns 2); (t, t) or omega zero or not finite: breakdown (returns 0).  Either step counts the update.
__device__ __forceinline__ int krylov_rule_bicg_omega(double S[kKrylovState], double ss, double ts, double tt, double tol2, float& w32) {
    S[kKsTs] = ts; S[kKsTt] = tt;
    if (ss <= tol2 * S[kKsBb]) { S[kKsRr] = ss; S[kKsDone] = 1.0; S[kKsIters] += 1.0; return 1; }
    if (bad(tt) || bad(ts / tt)) { S[kKsBreakdown] = 1.0; return 0; }
    const double omega = ts / tt;
    S[kKsOmega] = omega; S[kKsIters] += 1.0;
    w32 = (float)omega;
    return 2;
}

// BiCGSTAB: the stopping rule on the new rr, then beta = (rho' / rho) * (alpha / omega); not finite: breakdown.
__device__ __forceinline__ bool krylov_rule_bicg_beta(double S[kKrylovState], double rr, double rho, double tol2, float& b32) {
    S[kKsRr] = rr;
    const double beta = (rho / S[kKsRho]) * (S[kKsAlpha] / S[kKsOmega]);
    if (rr <= tol2 * S[kKsBb]) { S[kKsDone] = 1.0; S[kKsRho] = rho; return false; }
    if (!finite_d(beta)) { S[kKsBreakdown] = 1.0; return false; }
    b32 = (float)beta;
    S[kKsRho] = rho;
    return true;
}

}  // namespace hispmv
