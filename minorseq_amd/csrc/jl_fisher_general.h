// jl_fisher_general.h — FP64 one-sided Fisher's exact test for a 2x2 table whose rows need not sum to the same number
// (docs/SPEC.md §21): a sample's codon count against the count observed in a control at the same position.
//
// The table is [[a, n-a], [c, m-c]] with n = the sample's coverage and m = the control's.  Then
//     X ~ Hypergeometric(M = n + m, K = a + c, n)   and, with p = n/M, q = m/M, L = M - K,
//     P(X = x) = Binom(x; K, p) * Binom(n-x; L, p) / Binom(n; M, p),
// three binomial log-masses in saddle-point (Loader) form folded into one expression: the deviance terms of the third mass are
// exactly zero, the square-root factors take one log.  jl_fisher.h is the p = 1/2 case of this, where the four means K/2, L/2
// are exact; here they are K n / M and the like, rounded, and a deviance bd0(x, mu) moves by (1 - x/mu) d_mu when mu does.
// At 1e7 coverage and p near 1e-300 that is 1e-11 of ln P, so every mean carries its rounding remainder (two fmas: the product
// K n, which rounds above 2^53, as an exact two-product) and the deviance its first-order correction.  Every count is a
// uint32_t, so the bounds hold for every table the ABI can express (tests/fisher_general_domain.py, family `beyond`).  The tail that runs away from the mean is summed by the
// ratio recurrence from the point mass, the other one is its complement.  Written once for device and host.
#pragma once
#include "jl_fisher.h"

// mu = u v / M rounded, *d = the rest of the quotient; u v = uv + uv_lo exactly (uv_lo = 0 below 2^53)
JL_FHD double jl_mean_with_rest(double u, double v, double M, double *d)
{
    const double uv = u * v, uv_lo = fma(u, v, -uv), mu = uv / M;
    *d = (fma(-mu, M, uv) + uv_lo) / M;
    return mu;
}

// bd0(x, mu + d), |d| <= ulp(mu) / 2
JL_FHD double jl_bd0_rest(double x, double mu, double d) { return bd0(x, mu) + (1.0 - x / mu) * d; }

// ln P(X = x) for X ~ Hypergeometric(n + m, K, n), max(0, K - m) <= x <= min(K, n), n > 0, m > 0
JL_FHD double jl_log_pmf_general(double x, double K, double n, double m)
{
    const double TWO_PI = 6.283185307179586477;
    const double M = n + m, L = M - K;
    const double c = K - x, nx = n - x, mc = m - c;
    double s = stirlerr(K) + stirlerr(L) + stirlerr(n) + stirlerr(m) - stirlerr(M);
    s -= stirlerr(x) + stirlerr(c) + stirlerr(nx) + stirlerr(mc);
    // a cell of 0 has the deviance bd0(0, mu) = mu and no square-root factor; the four means sum, in pairs, to K and to L
    double d, mu, r = 1.0;
    mu = jl_mean_with_rest(K, n, M, &d);
    if (x > 0.0) { s -= jl_bd0_rest(x, mu, d); r *= x; } else s -= mu + d;
    mu = jl_mean_with_rest(K, m, M, &d);
    if (c > 0.0) { s -= jl_bd0_rest(c, mu, d); r *= c; } else s -= mu + d;
    mu = jl_mean_with_rest(L, n, M, &d);
    if (nx > 0.0) { s -= jl_bd0_rest(nx, mu, d); r *= nx; } else s -= mu + d;
    mu = jl_mean_with_rest(L, m, M, &d);
    if (mc > 0.0) { s -= jl_bd0_rest(mc, mu, d); r *= mc; } else s -= mu + d;
    // the factors sqrt(2 pi k) of the margins and cells that are not 0 (K = 0 or L = 0: one table only, P = 1)
    double t = n * m / M;
    if (K > 0.0) t *= K; else r *= TWO_PI;
    if (L > 0.0) t *= L; else r *= TWO_PI;
    const int cells = (x > 0.0) + (c > 0.0) + (nx > 0.0) + (mc > 0.0);
    for (int i = cells; i < 4; ++i) t *= TWO_PI;
    return s + 0.5 * log(t / (TWO_PI * r));
}

// P(X = x) for K <= 64 by direct products, as jl_pmf_equal_rows_small:
//   P = C(K, x) * prod_{i<x} (n - i) * prod_{i<K-x} (m - i) / prod_{i<K} (M - i)
// With rows of very different size the value can leave the normal range (the caller then takes the saddle-point form).
JL_FHD double jl_pmf_general_small(double x, double K, double n, double m)
{
    const double c = K - x;
    const double M = n + m;
    double num = 1.0, den = 1.0, p = 1.0;
    int pending = 0;
    for (double i = 0.0; i < K; i += 1.0) {
        num *= i < x ? n - i : m - (i - x);
        den *= M - i;
        if (++pending == 16) { p *= num / den; num = 1.0; den = 1.0; pending = 0; }  // keep both below 1e160
    }
    const double k = x < c ? x : c;
    for (double i = 0.0; i < k; i += 1.0) { num *= K - i; den *= i + 1.0; }
    return p * (num / den);
}

// P(X >= a) for the table [[a, n-a], [c, m-c]]; returns p, *logp = ln p.  GATE: unless the p-value provably cannot lead to
// a call (jl_fisher_greater_equal_rows_or_skip: already the point mass, Bonferroni-adjusted, reaches alpha) — then *skipped
// is set, the tail is not summed and p = 1 comes back.  Every value that IS returned comes from the same expressions either way.
template <bool GATE>
JL_FHD double jl_fisher_greater_general_impl(uint32_t a_, uint32_t n_, uint32_t c_, uint32_t m_, double n_tests, double alpha,
                                             double *logp, bool *skipped)
{
    if (GATE) *skipped = false;
    const double a = a_, c = c_, n = n_, m = m_;
    const double K = a + c, M = n + m, L = M - K;
    const double hi = K < n ? K : n;
    const double lo = K > m ? K - m : 0.0;
    if (a <= lo) { *logp = 0.0; return 1.0; }
    const bool upper = (uint64_t)a_ * m_ >= (uint64_t)n_ * c_;   // a M >= n K, at or above the mean: in integers, both below 2^64
    const double gate = alpha * (1.0 + 1e-6);
    if (upper) {   // sum the decreasing upper tail
        double pm = 0.0, l0 = 0.0;
        const bool direct = K <= 64.0 && (pm = jl_pmf_general_small(a, K, n, m)) > 1e-280;
        if (!direct) l0 = jl_log_pmf_general(a, K, n, m);
        if (GATE && (direct || l0 > -700.0)) {
            double adj = (direct ? pm : exp(l0)) * n_tests;
            if (adj > 1.0) adj = 1.0;
            if (adj >= gate) { *skipped = true; *logp = 0.0; return 1.0; }
        }
        double term = 1.0, sum = 1.0;
        for (double x = a; x < hi; x += 1.0) {
            term *= ((K - x) * (n - x)) / ((x + 1.0) * (L - n + x + 1.0));
            sum += term;
            if (term < sum * 1e-17) break;
        }
        if (direct) {
            double pv = pm * sum;
            if (pv > 1.0) pv = 1.0;
            *logp = log(pv);
            return pv;
        }
        const double lp = l0 + log(sum);
        *logp = lp < 0.0 ? lp : 0.0;
        return lp < -745.0 ? 0.0 : (lp < 0.0 ? exp(lp) : 1.0);
    }
    // below the mean: 1 - P(X <= a-1), the lower tail summed downwards
    const double x0 = a - 1.0;
    double pm = 0.0;
    const bool direct = K <= 64.0 && (pm = jl_pmf_general_small(x0, K, n, m)) > 1e-280;
    if (!direct) pm = exp(jl_log_pmf_general(x0, K, n, m));
    double term = 1.0, sum = 1.0;
    for (double x = x0; x > lo; x -= 1.0) {
        term *= (x * (L - n + x)) / ((K - x + 1.0) * (n - x + 1.0));
        sum += term;
        if (term < sum * 1e-17) break;
    }
    double lower = pm * sum;
    if (lower > 1.0) lower = 1.0;
    *logp = lower < 1.0 ? log1p(-lower) : -HUGE_VAL;
    return 1.0 - lower;
}

JL_FHD double jl_fisher_greater_general(uint32_t a, uint32_t n, uint32_t c, uint32_t m, double *logp)
{
    return jl_fisher_greater_general_impl<false>(a, n, c, m, 0.0, 0.0, logp, nullptr);
}

JL_FHD double jl_fisher_greater_general_or_skip(uint32_t a, uint32_t n, uint32_t c, uint32_t m, double n_tests, double alpha,
                                                double *logp, bool *skipped)
{
    return jl_fisher_greater_general_impl<true>(a, n, c, m, n_tests, alpha, logp, skipped);
}
