/* es_softplus_dev.h -- the straight-line softplus of es_math.h (es_softplus_neg_fast) with fewer vector instructions, and the
 * f(a, b) built on it.  Same bits for every operand, same range flag; tests/test_softplus_dev.py compares it with es_math.h's
 * es_polar_f_fast_sp on the host, tests/test_softplus_dev_gpu.py on the device; tests/test_softplus_sl_edges.py and
 * tests/test_softplus_sl_gpu.py do the same at the edges of the integer rewrites further down (scale bits, corner test, kc, range flag).
 *
 * es_softplus_neg_fast evaluates four results and picks one with three 64-bit selects (two v_cndmask each):
 *     res0 = f - (hfsq - sR)                                   k == 0
 *     resk = ln2_hi - ((hfsq - (sR + (ln2_lo + c))) - f)       k == 1
 *     resc = ln2_hi - ((Rc - (ln2_lo + c)) - f)                 k == 1 and |f| < 2^-20 (fdlibm's corner)
 *     rt   = y - y*y*0.5                                        y < 2^-29
 * All four are ONE expression  kf*ln2_hi - ((P - (Q + kf*(ln2_lo + c))) - f)  with
 *     kf = 0 (k == 0) or 1,   Q = sR, or 0 in the corner and below 2^-29,   P = hfsq * (1 - kc*(2/3)*f),  kc = 1 in the corner,
 * because IEEE-754 round-to-nearest is sign-symmetric (x - y == -(y - x) bit for bit, and 0 - x == -x except 0 - (+0) == +0):
 *   k == 0:  fma(0, ln2_hi, -W) == -W == f - (hfsq - sR) where W = (hfsq - sR) - f (W is +0 when f == hfsq - sR, never -0: f > 0);
 *            fma(0, ln2_lo + c, sR) == sR (sR > 0);  below 2^-29 Q == 0 gives -(hfsq - y) == y - hfsq, and hfsq is formed as
 *            (f*f)*0.5 -- rt's rounding; elsewhere f*f is a normal number (|f| >= 2^-53 or 0), where (f*f)*0.5 == (0.5*f)*f.
 *   k == 1:  fma(1, x, y) rounds x + y once, as the adds do; 1 - 1*g == 1 - g and 1 - 0*g == 1 (fma rounds once);
 *            in the corner Q + (ln2_lo + c) == ln2_lo + c (that sum is never -0: x + -x is +0 under round-to-nearest).
 * kf and kc are 0.0 / 1.0, whose low words are zero: one 32-bit select each.  The three 64-bit selects of the result become
 * one (Q), and the arithmetic of res0, resc and rt (8 float64 instructions per softplus) is gone. */
#ifndef ES_SOFTPLUS_DEV_H
#define ES_SOFTPLUS_DEV_H

#include "es_math.h"

/* the double whose words are lo and hi */
ES_HD double es_words2d(uint32_t lo, uint32_t hi) { return es_u2d(((uint64_t)hi << 32) | lo); }

/* 0.0 or 1.0 by a flag: a select of the high word only, over the zero low word the caller passes */
ES_HD double es_flag01(int on, uint32_t zero_lo) { return es_words2d(zero_lo, on ? 0x3ff00000u : 0u); }

/* ES_EXP_SHIFT (0x1.8p+52) in a vector register pair the compiler knows nothing about.  Its low word is zero.  The flags kf and kc
 * are pairs (zero low word, selected high word), and a 64-bit operand is an aligned register pair: two flags alive at once over ONE
 * zero register cost a copy of it per softplus.  The fma that forms kd cannot read both of its constants from scalar registers, so
 * ES_EXP_SHIFT is moved into a vector pair for every f anyway: kc takes that pair's low word for its own, and the copy is gone. */
ES_HD double es_shift_reg(void)
{
#if defined(__HIP_DEVICE_COMPILE__)
    double x;
    asm volatile("v_mov_b64 %0, %1" : "=v"(x) : "s"(ES_EXP_SHIFT));
    return x;
#else
    return ES_EXP_SHIFT;
#endif
}

/* x, as a value the compiler knows nothing more about.  es_polar_f_slg reads a + b through it from its second range test on: that test's
 * |a + b| is then formed where it is used, as an operand modifier of the compare, and not carried over from the first softplus. */
ES_HD double es_opaque(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(x));
#endif
    return x;
}

typedef uint32_t __attribute__((may_alias)) es_u32_alias;

/* hi + (k << 13) mod 2^32: the high word of (hi:lo) + (k << 45).  One v_lshl_add_u32 on the device -- as long as no 64-bit value is
 * in sight: handed the table word as one uint64_t the compiler rebuilds a 64-bit add and an or from this, so the device reads its halves. */
ES_HD uint32_t es_scale_hi(uint32_t hi, uint32_t k) { return hi + (k << 13); }

/* log1p(exp(t)) for t <= 0 and |t| < 512, bit-identical to es_softplus_neg_fast (log1p's |f| < 2^-20 corner included); sh is ES_EXP_SHIFT (es_shift_reg).
 * Beside the float64 sequence of the header comment:
 *   scale bits  te1 + (ki << 45): the low word of ki << 45 is zero, so nothing carries into the high word, which alone changes, by
 *               (ki << 13) mod 2^32 (bits 0..18 of ki): one 32-bit shift-add on the high register (es_scale_hi).
 *   corner      the high word of u in 0x3FFFFFFD..0x3FFFFFFF is "hu0 > 0x3FFFFFFC" plus ONE more case, hu0 == 0x40000000: y <= 1 gives
 *               u <= 2, so that is u == 2 (y == 1, t == 0).  There k0 is false, f = fma(2, 0.5, -1) == +0, hfsq == +0, s == +0, z == 0,
 *               R == 0 and sR == +0 -- the Q == 0 that now replaces it -- and P == 0 * (1 - kc*0) == +0 for kc of 0 or 1: the same bits.
 *   -kc         fma(kc, -g, 1) == fma(-kc, g, 1) (the product has the same sign and magnitude), which leaves ONE select constant,
 *               0x3ff00000, for both flags. */
ES_HD double es_softplus_neg_sl_sh(double t, const uint64_t* tab, double sh)
{
    /* ---- exp(t), main path of es_exp (as es_softplus_neg_fast) ---- */
    double kd = ES_FMA(t, ES_EXP_INVLN2N, sh);
    const uint64_t ki = es_d2u(kd);
    kd = kd - ES_EXP_SHIFT;
    double r = ES_FMA(kd, ES_EXP_NLN2HI, t);
    r = ES_FMA(kd, ES_EXP_NLN2LO, r);
    const uint32_t idx = 2u * (uint32_t)(ki & 127u);
#if defined(__HIP_DEVICE_COMPILE__) && defined(ES_EXP_TAB_LDS_ADDR)
    typedef __attribute__((address_space(3))) const uint64_t es_lds_u64;
    es_lds_u64* const te = (es_lds_u64*)(uint32_t)((ES_EXP_TAB_LDS_ADDR) + idx * 8u);
    typedef __attribute__((address_space(3))) const es_u32_alias es_lds_u32;
    es_lds_u32* const tw = (es_lds_u32*)(uint32_t)((ES_EXP_TAB_LDS_ADDR) + idx * 8u);
    const double tail = es_u2d(te[0]);
    const uint32_t te1_lo = tw[2], te1_hi = tw[3];        /* the scale word as its halves: no 64-bit value to add to */
    (void)tab;
#else
    const double tail = es_u2d(tab[idx]);
    const uint32_t te1_lo = (uint32_t)tab[idx + 1], te1_hi = (uint32_t)(tab[idx + 1] >> 32);
#endif
    const double scale = es_words2d(te1_lo, es_scale_hi(te1_hi, (uint32_t)ki));
    const double p23 = ES_FMA(r, ES_EXP_C3, ES_EXP_C2);
    const double tr = r + tail;
    const double r2 = r * r;
    const double p45 = ES_FMA(r, ES_EXP_C5, ES_EXP_C4);
    const double tq = ES_FMA(p23, r2, tr);
    const double r4 = r2 * r2;
    const double tmp = ES_FMA(r4, p45, tq);
    const double y = ES_FMA(scale, tmp, scale);           /* in (0, 1] */

    /* ---- log1p(y) ---- */
    const int32_t hy = es_hi32(y);
    const int tiny29 = hy < 0x3e200000;                   /* y < 2^-29 */
    const int k0 = hy < 0x3FDA827A;                       /* y < sqrt(2)-1: k = 0, f = y */
    const double u = 1.0 + y;
    const uint32_t hu0 = (uint32_t)es_hi32(u);
    const int corner = hu0 > 0x3FFFFFFCu;                 /* k == 1 and |f| < 2^-20 (see es_softplus_neg_fast), or u == 2 */
    const double cn1 = y - (u - 1.0);
    const double f1 = ES_FMA(u, 0.5, -1.0);
    const double f = k0 ? y : f1;
    const double c = es_div_normal(cn1, u);
    const double hfsq = f * f * 0.5;
    const double s = es_div_normal(f, 2.0 + f);
    const double z = s * s;
    const double R1 = z * ES_LP1;
    const double z2 = z * z;
    const double R2 = ES_LP2 + z * ES_LP3;
    const double z4 = z2 * z2;
    const double R3 = ES_LP4 + z * ES_LP5;
    const double z6 = z4 * z2;
    const double R4 = ES_LP6 + z * ES_LP7;
    const double R = ((R1 + z2 * R2) + z4 * R3) + z6 * R4;
    const double sR = s * (hfsq + R);
    const double kf = es_flag01(!k0, 0u);
    const double kc = es_flag01(corner, (uint32_t)es_d2u(sh));
    const double P = hfsq * ES_FMA(kc, -(0.66666666666666666 * f), 1.0);
    const double Q = (corner | tiny29) ? 0.0 : sR;
    const double W = (P - ES_FMA(kf, ES_LN2_LO + c, Q)) - f;
    return ES_FMA(kf, ES_LN2_HI, -W);
}

/* the same with the range flag: *ok = 0 outside |t| < 512 */
ES_HD double es_softplus_neg_sl(double t, const uint64_t* tab, int* ok)
{
    *ok = (__builtin_fabs(t) < 512.0);
    return es_softplus_neg_sl_sh(t, tab, es_shift_reg());
}

/* es_polar_f_fast_sp with es_softplus_neg_sl_sh: the same value, softplus pair and *bad (or-ed in) */
ES_HD double es_polar_f_sl_sp_sh(double a, double b, const uint64_t* tab, double* sp_diff, double* sp_sum, int* bad, double sh)
{
    const double d1 = a - b;
    const double sum = a + b;
    const double L1 = es_softplus_neg_sl_sh(-__builtin_fabs(d1), tab, sh);
    const double L2 = es_softplus_neg_sl_sh(-__builtin_fabs(sum), tab, sh);
    *bad |= !((__builtin_fabs(d1) < 512.0) & (__builtin_fabs(sum) < 512.0));
    *sp_diff = L1;
    *sp_sum = L2;
    const double r1 = es_max_num(a, b) + L1;
    const double r2 = es_max_num(sum, 0.0) + L2;
    return r1 - r2;
}

ES_HD double es_polar_f_sl_sp(double a, double b, const uint64_t* tab, double* sp_diff, double* sp_sum, int* bad)
{
    return es_polar_f_sl_sp_sh(a, b, tab, sp_diff, sp_sum, bad, es_shift_reg());
}

ES_HD double es_polar_f_sl_sh(double a, double b, const uint64_t* tab, int* bad, double sh)
{
    double s0, s1;
    return es_polar_f_sl_sp_sh(a, b, tab, &s0, &s1, bad, sh);
}

ES_HD double es_polar_f_sl(double a, double b, const uint64_t* tab, int* bad)
{
    return es_polar_f_sl_sh(a, b, tab, bad, es_shift_reg());
}

/* es_polar_f (generic softplus right after an evaluation out of range) with es_softplus_neg_sl_sh */
ES_HD double es_polar_f_slg_sh(double a, double b, const uint64_t* tab, double sh)
{
    const double d1 = a - b;
    const double sum0 = a + b;
    double L1 = es_softplus_neg_sl_sh(-__builtin_fabs(d1), tab, sh);
    double L2 = es_softplus_neg_sl_sh(-__builtin_fabs(sum0), tab, sh);
    const double sum = es_opaque(sum0);
    if (!(__builtin_fabs(d1) < 512.0)) L1 = es_softplus_neg_generic(-__builtin_fabs(d1), tab);
    if (!(__builtin_fabs(sum) < 512.0)) L2 = es_softplus_neg_generic(-__builtin_fabs(sum), tab);
    const double r1 = es_max_num(a, b) + L1;
    const double r2 = es_max_num(sum, 0.0) + L2;
    return r1 - r2;
}

ES_HD double es_polar_f_slg(double a, double b, const uint64_t* tab)
{
    return es_polar_f_slg_sh(a, b, tab, es_shift_reg());
}

/* The leaf penalty's softplus log1p(exp(-al)), al = |leaf LLR|, on the straight-line form: the value es_metric_penalty (es_math.h) starts
 * from, bit for bit, while al < 512.  Outside that range (NaN included) *bad is set (or-ed in) and the result is unspecified: the caller
 * evaluates es_softplus_neg_generic(-al) instead, on a cold path after ONE test for all its lanes, as the f levels of depths 9 and 10 do --
 * no branch follows the evaluation.  tests/test_leaf_penalty_dev.py compares the three steps with es_metric_penalty on the host. */
ES_HD double es_leaf_softplus_sl_sh(double al, const uint64_t* tab, int* bad, double sh)
{
    *bad |= !(al < 512.0);
    return es_softplus_neg_sl_sh(-al, tab, sh);
}

/* ... and the penalty of deciding `bit` at a leaf whose LLR has magnitude al and preferred bit pref, from that softplus (fastpolar.py:32-40) */
ES_HD double es_leaf_penalty(double lp, double al, uint32_t pref, uint32_t bit) { return (bit != pref) ? lp + al : lp; }

#endif /* ES_SOFTPLUS_DEV_H */
