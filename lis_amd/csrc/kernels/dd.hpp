/*
 * dd.hpp -- double-double ("quad") arithmetic, ONE source for the kernels (quad.hip) and for the host's scalar steps
 * (host/lis_solver_quad.c includes this file as C): plain C that hipcc compiles as __host__ __device__.
 *
 * The operation order is that of the reference's SSE2 forms (include/lis_precision.h with USE_SSE2, USE_FAST_QUAD_ADD and
 * USE_FMA2_SSE2 -- what its configure picks on x86-64); its plain-C macros compute something else and are NOT restated here.
 *   add   LIS_QUAD_ADD_SSE2_CORE / ADD2 (:461-474, :908-917): two-sum of the high parts, + b.lo, + c.lo, fast-two-sum (the "sloppy" add)
 *   mul   LIS_QUAD_MUL_SSE2_CORE (:346-371):  p = b.hi*c.hi, e = err(p) + c.hi*b.lo + b.hi*c.lo   (the scalar form: odd tails, lis_quad_mul)
 *   mul2  LIS_QUAD_MUL2_SSE2_CORE (:802-824): p = b.hi*c.hi, e = err(p) + b.hi*c.lo + c.hi*b.lo   (the packed form: element pairs)
 *         -- the two differ in the order of the cross terms, so mul(b, c) == mul2(c, b) and the reference's vector operations
 *         round an element by its position in its thread's chunk (pairs packed, an odd last element scalar)
 *   muld  LIS_QUAD_MULD_SSE2_CORE / MULD2 (:379-402, :832-852): p = b.hi*c, e = err(p) + b.lo*c    (both forms agree)
 *   div   LIS_QUAD_DIV_SSE2 (:523-581)
 * Two-prod's error term err(p) is fma(a, b, -p) -- one instruction on gfx950 -- where the reference sums Dekker's four partial
 * products of the halves split with 134217729.0.  Dekker's sum is exact, so the two agree in every bit wherever nothing overflows
 * or underflows (tests/quad_model.py restates Dekker's form and is held to the reference's bits).  dd_split / dd_two_prod_dekker
 * are here for completeness and for the tests of that equality.  Both compilers run with -ffp-contract=off: nothing below is fused
 * except the one fma that is written out.
 */
#ifndef LIS_AMD_DD_HPP
#define LIS_AMD_DD_HPP

#if defined(__HIPCC__)
#define DD_FN __host__ __device__ static inline
#else
#include <math.h>
#define DD_FN static inline
#endif

typedef struct { double hi, lo; } dd_t;

#define DD_SPLITTER 134217729.0

DD_FN dd_t dd_make(double hi, double lo) { dd_t r; r.hi = hi; r.lo = lo; return r; }
DD_FN dd_t dd_minus(dd_t a) { return dd_make(-a.hi, -a.lo); }

DD_FN dd_t dd_two_sum(double a, double b)
{
	const double s = a + b, v = s - a;
	return dd_make(s, (a - (s - v)) + (b - v));
}
DD_FN dd_t dd_fast_two_sum(double a, double b)
{
	const double s = a + b;
	return dd_make(s, b - (s - a));
}
DD_FN dd_t dd_two_diff(double a, double b)
{
	const double s = a - b, v = s - a;
	return dd_make(s, (a - (s - v)) - (b + v));
}
DD_FN dd_t dd_split(double a)
{
	const double t = DD_SPLITTER * a, hi = t - (t - a);
	return dd_make(hi, a - hi);
}
DD_FN dd_t dd_two_prod_dekker(double a, double b)
{
	const double p = a * b;
	const dd_t sa = dd_split(a), sb = dd_split(b);
	return dd_make(p, ((sa.hi * sb.hi - p) + sa.hi * sb.lo + sa.lo * sb.hi) + sa.lo * sb.lo);
}
DD_FN dd_t dd_two_prod(double a, double b)
{
	const double p = a * b;
	return dd_make(p, __builtin_fma(a, b, -p));
}

DD_FN dd_t dd_mul(dd_t b, dd_t c)
{
	const dd_t p = dd_two_prod(b.hi, c.hi);
	double e = p.lo + c.hi * b.lo;
	e = e + b.hi * c.lo;
	return dd_fast_two_sum(p.hi, e);
}
DD_FN dd_t dd_mul2(dd_t b, dd_t c)
{
	const dd_t p = dd_two_prod(b.hi, c.hi);
	double e = p.lo + b.hi * c.lo;
	e = e + c.hi * b.lo;
	return dd_fast_two_sum(p.hi, e);
}
DD_FN dd_t dd_muld(dd_t b, double c)
{
	const dd_t p = dd_two_prod(b.hi, c);
	const double e = p.lo + b.lo * c;
	return dd_fast_two_sum(p.hi, e);
}
DD_FN dd_t dd_add(dd_t b, dd_t c)
{
	const dd_t s = dd_two_sum(b.hi, c.hi);
	double e = s.lo + b.lo;
	e = e + c.lo;
	return dd_fast_two_sum(s.hi, e);
}
/* a + b*c: scalar form, packed form, and with c a double */
DD_FN dd_t dd_fma(dd_t a, dd_t b, dd_t c)  { return dd_add(a, dd_mul(b, c)); }
DD_FN dd_t dd_fma2(dd_t a, dd_t b, dd_t c) { return dd_add(a, dd_mul2(b, c)); }
DD_FN dd_t dd_fmad(dd_t a, dd_t b, double c) { return dd_add(a, dd_muld(b, c)); }

DD_FN dd_t dd_div(dd_t b, dd_t c)
{
	const double q1 = b.hi / c.hi;
	const dd_t r = dd_muld(c, q1);                  /* q1 * c */
	const dd_t d = dd_two_diff(b.hi, r.hi);
	double e = d.lo - r.lo;
	e = e + b.lo;
	const double q2 = (d.hi + e) / c.hi;
	return dd_fast_two_sum(q1, q2);
}

#endif
