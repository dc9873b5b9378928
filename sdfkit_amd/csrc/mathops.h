// mathops.h -- MathF.Sin / Cos / Exp / Log / Atan2 of SDF programs (SDFK_OP_SIN .. SDFK_OP_ATAN2, include/sdfkit_hip.h), written
// ONCE as plain C++ that compiles for the host and for the device.  The includer defines SDFK_MATHOPS_EMIT(...): the code generator
// (sample_codegen.h) turns the text into a string and pastes it into the JIT source of programs that use one of these opcodes;
// a host test (tests/cpp/mathops_host.cpp) compiles the very same text as code.  The text itself uses two qualifiers the includer
// defines before it is compiled: SDFK_M_FN (functions) and SDFK_M_TABLE (constant tables).  No preprocessor directives inside the
// text (it is a macro argument), no fma, no library calls: binary64 + - * / rint ldexp frexp and 64-bit integer arithmetic only,
// each one IEEE-exact or correctly rounded, so numpy reproduces every result bit for bit (tests/mathops_model.py).
//
// Every function: float in -> widened to binary64 -> argument reduced in binary64 (or exactly, in integers) -> a fixed polynomial
// (Taylor coefficients rounded to binary64, Horner in the stated order) -> scaled -> rounded ONCE to float.  The binary64 result is
// within ~2^-50 relative of the true value, so the float is faithful (within 1 ulp) and correctly rounded unless the true value
// lies within ~2^-50 of a midpoint between two floats.
SDFK_MATHOPS_EMIT(
// 2/pi in binary, 32 bits per word after a leading zero word: bit k of 2/pi (k = 1 is the 2^-1 bit) is bit 31 - ((k + 31) & 31) of
// word (k + 31) >> 5.  288 bits; the large reduction reads bits up to 231.
SDFK_M_TABLE unsigned int sdfk_m_2opi[10] = {0x00000000u, 0xa2f9836eu, 0x4e441529u, 0xfc2757d1u, 0xf534ddc0u, 0xdb629599u,
                                             0x3c439041u, 0xfe5163abu, 0xdebbc561u, 0xb7246e3au};
// atan(j / 8), j = 0..8, rounded to binary64
SDFK_M_TABLE double sdfk_m_atanj[9] = {0.0, 0x1.fd5ba9aac2f6ep-4, 0x1.f5b75f92c80ddp-3, 0x1.6f61941e4def1p-2, 0x1.dac670561bb4fp-2,
                                       0x1.1e00babdefeb4p-1, 0x1.4978fa3269ee1p-1, 0x1.700a7c5784634p-1, 0x1.921fb54442d18p-1};

// 32 bits of 2/pi starting at bit k (k >= -31; bits k <= 0 are zero)
SDFK_M_FN unsigned long long sdfk_m_2opi_bits(int k)
{
    const int p = k + 31;
    const unsigned long long two = ((unsigned long long)sdfk_m_2opi[p >> 5] << 32) | sdfk_m_2opi[(p >> 5) + 1];
    return ((two << (p & 31)) >> 32) & 0xffffffffull;
}

// x = q (pi / 2) + r, |r| <= pi / 4 (slightly more at the rounding of q): returns r in binary64, q & 3 in *quad.  x finite.
//  |x| < 2^22: q = rint(x * (2/pi)_64); r = ((x - q P1) - q P2) - q P3 with pi/2 = P1 + P2 + P3 + O(2^-118), P1 and P2 of 30
//    significant bits, so that q P1 and q P2 are exact and x - q P1 is exact (Sterbenz).
//  |x| >= 2^22 (Payne-Hanek): x = m 2^e, m the 24-bit integer significand.  With w = the 96 bits of 2/pi from bit e - 1 on,
//    (m w) mod 2^96 = x (2/pi) mod 4 in 2.94 fixed point, up to less than 2^-70 (the bits of 2/pi before e - 1 contribute
//    multiples of 4, the ones after bit e + 94 less than m 2^-94).  q = that rounded to the nearest integer, the rest -- at most
//    29 leading zero bits for any float -- to binary64 from its top 64 and low 32 bits, times (pi/2)_64.
SDFK_M_FN double sdfk_m_reduce(float x, int* quad)
{
    const double xd = (double)x;
    if (__builtin_fabs(xd) < 0x1p22) {
        const double q = __builtin_rint(xd * 0x1.45f306dc9c883p-1);
        *quad = (int)q & 3;
        return ((xd - q * 0x1.921fb548p+0) - q * -0x1.de973dc8p-31) - q * -0x1.9d9cceba3f91fp-62;
    }
    const unsigned int bits = __builtin_bit_cast(unsigned int, x);
    const unsigned long long m = (unsigned long long)((bits & 0x7fffffu) | 0x800000u);
    const int s = (int)((bits >> 23) & 0xffu) - 151;   // e - 1, e = biased exponent - 150
    const unsigned long long p0 = m * sdfk_m_2opi_bits(s + 64);
    const unsigned long long p1 = m * sdfk_m_2opi_bits(s + 32) + (p0 >> 32);
    const unsigned long long p2 = m * sdfk_m_2opi_bits(s) + (p1 >> 32);
    const unsigned long long hi = (p2 << 32) | (p1 & 0xffffffffull);   // bits 95..32 of (m w) mod 2^96
    const unsigned long long lo = p0 & 0xffffffffull;
    const unsigned long long n = (hi + (1ull << 61)) >> 62;
    const long long rh = (long long)(hi - (n << 62));                   // in [-2^61, 2^61)
    const double r = ((double)rh * 0x1p-62 + (double)lo * 0x1p-94) * 0x1.921fb54442d18p+0;
    const int qn = (int)(n & 3ull);
    if (x < 0.0f) { *quad = (4 - qn) & 3; return -r; }
    *quad = qn;
    return r;
}
// sin(r) and cos(r), |r| <= ~pi/4: Taylor to r^15 and r^16 (truncation below 2^-55 relative)
SDFK_M_FN double sdfk_m_sin_poly(double r)
{
    const double r2 = r * r;
    const double p = -0x1.5555555555555p-3 + r2 * (0x1.1111111111111p-7 + r2 * (-0x1.a01a01a01a01ap-13 + r2 * (0x1.71de3a556c734p-19
                   + r2 * (-0x1.ae64567f544e4p-26 + r2 * (0x1.6124613a86d09p-33 + r2 * -0x1.ae7f3e733b81fp-41)))));
    return r + (r * r2) * p;
}
SDFK_M_FN double sdfk_m_cos_poly(double r)
{
    const double r2 = r * r;
    const double p = -0x1p-1 + r2 * (0x1.5555555555555p-5 + r2 * (-0x1.6c16c16c16c17p-10 + r2 * (0x1.a01a01a01a01ap-16
                   + r2 * (-0x1.27e4fb7789f5cp-22 + r2 * (0x1.1eed8eff8d898p-29 + r2 * (-0x1.93974a8c07c9dp-37 + r2 * 0x1.ae7f3e733b81fp-45))))));
    return 1.0 + r2 * p;
}
// sin(x) (phase 0) or cos(x) (phase 1) = the polynomial of quadrant (q + phase) & 3: sin, cos, -sin, -cos
SDFK_M_FN float sdfk_m_sincos(float x, int phase)
{
    if (!(__builtin_fabs((double)x) <= 0x1.fffffep+127)) return x - x;   // sin / cos (+-inf) = NaN, NaN -> NaN
    if (x == 0.0f) return phase ? 1.0f : x;                               // (sin(-0) = -0: a sum would give +0)
    int q;
    const double r = sdfk_m_reduce(x, &q);
    const int k = (q + phase) & 3;
    const double v = (k & 1) ? sdfk_m_cos_poly(r) : sdfk_m_sin_poly(r);
    return (float)((k & 2) ? -v : v);
}
SDFK_M_FN float sdfk_sinf(float x) { return sdfk_m_sincos(x, 0); }
SDFK_M_FN float sdfk_cosf(float x) { return sdfk_m_sincos(x, 1); }

// exp(x) = 2^k exp(r): k = rint(x * (log2 e)_64), r = (x - k L1) - k L2 with ln 2 = L1 + L2 + O(2^-102), L1 of 44 bits (k L1 exact,
// x - k L1 exact); exp(r), |r| <= ~0.347: Taylor to r^13; ldexp exact in binary64.  x >= 89: +inf; x <= -104 (exp < 2^-150): +0.
SDFK_M_FN float sdfk_expf(float x)
{
    if (x != x) return x + x;
    if (!(x < 89.0f)) return __builtin_inff();
    if (!(x > -104.0f)) return 0.0f;
    const double xd = (double)x;
    const double k = __builtin_rint(xd * 0x1.71547652b82fep+0);
    const double r = (xd - k * 0x1.62e42fefa3ap-1) - k * -0x1.0ca86c3898dp-49;
    const double p = 1.0 + r * (1.0 + r * (0x1p-1 + r * (0x1.5555555555555p-3 + r * (0x1.5555555555555p-5 + r * (0x1.1111111111111p-7
                   + r * (0x1.6c16c16c16c17p-10 + r * (0x1.a01a01a01a01ap-13 + r * (0x1.a01a01a01a01ap-16 + r * (0x1.71de3a556c734p-19
                   + r * (0x1.27e4fb7789f5cp-22 + r * (0x1.ae64567f544e4p-26 + r * (0x1.1eed8eff8d898p-29 + r * 0x1.6124613a86d09p-33))))))))))));
    return (float)__builtin_ldexp(p, (int)k);
}

// log(x) = e ln 2 + log(m): x = m 2^e, m in [sqrt(1/2), sqrt(2)) (frexp, then m + m, e - 1 below sqrt(1/2)); f = m - 1 (exact),
// s = f / (2 + f), log(m) = 2 atanh(s) = 2s + 2s s^2 (1/3 + s^2/5 + ... + s^20/21), |s| <= 0.172; e ln 2 as e L1 + e L2.
// log(+-0) = -inf, log(x < 0) = NaN, log(+inf) = +inf, log(1) = +0.
SDFK_M_FN float sdfk_logf(float x)
{
    if (x != x) return x + x;
    if (x == 0.0f) return -__builtin_inff();
    if (x < 0.0f) return __builtin_nanf("");
    if (x == __builtin_inff()) return x;
    int e;
    double m = __builtin_frexp((double)x, &e);
    if (m < 0x1.6a09e667f3bcdp-1) { m = m + m; e = e - 1; }
    const double f = m - 1.0;
    const double s = f / (2.0 + f);
    const double s2 = s * s;
    const double q = 0x1.5555555555555p-2 + s2 * (0x1.999999999999ap-3 + s2 * (0x1.2492492492492p-3 + s2 * (0x1.c71c71c71c71cp-4
                   + s2 * (0x1.745d1745d1746p-4 + s2 * (0x1.3b13b13b13b14p-4 + s2 * (0x1.1111111111111p-4 + s2 * (0x1.e1e1e1e1e1e1ep-5
                   + s2 * (0x1.af286bca1af28p-5 + s2 * 0x1.8618618618618p-5))))))));
    const double t = s + s;
    const double ed = (double)e;
    return (float)(ed * 0x1.62e42fefa3ap-1 + (ed * -0x1.0ca86c3898dp-49 + (t + t * (s2 * q))));
}

// atan2(y, x) (MathF.Atan2: a = y, b = x).  C99 Annex F for zeros, infinities and NaN; otherwise with t = min(|y|, |x|) /
// max(|y|, |x|) in [0, 1]: j = rint(8 t), u = (8 t - j) / (8 + t j) (exact numerator), atan(t) = atan(j/8) + u + u u^2 P(u^2),
// |u| <= 1/16, P = Taylor to u^15; then pi/2 - . when |y| > |x|, pi - . when x < 0, negated when y < 0.
SDFK_M_FN float sdfk_atan2f(float y, float x)
{
    if (x != x || y != y) return x + y;
    const bool xneg = __builtin_bit_cast(unsigned int, x) >> 31;
    if (y == 0.0f) return xneg ? ((__builtin_bit_cast(unsigned int, y) >> 31) ? -3.14159274101257324f : 3.14159274101257324f) : y;
    const double yd = (double)y, xd = (double)x;
    const double ay = __builtin_fabs(yd), ax = __builtin_fabs(xd);
    double a;
    if (ax == __builtin_inf() && ay == __builtin_inf()) a = x > 0.0f ? 0x1.921fb54442d18p-1 : 0x1.2d97c7f3321d2p+1;
    else {
        const bool swap = ay > ax;
        const double t = swap ? ax / ay : ay / ax;
        const double j = __builtin_rint(t * 8.0);
        const double u = (t * 8.0 - j) / (8.0 + t * j);
        const double u2 = u * u;
        const double p = -0x1.5555555555555p-2 + u2 * (0x1.999999999999ap-3 + u2 * (-0x1.2492492492492p-3 + u2 * (0x1.c71c71c71c71cp-4
                       + u2 * (-0x1.745d1745d1746p-4 + u2 * (0x1.3b13b13b13b14p-4 + u2 * -0x1.1111111111111p-4)))));
        a = sdfk_m_atanj[(int)j] + (u + (u * u2) * p);
        if (swap) a = 0x1.921fb54442d18p+0 - a;
        if (x < 0.0f) a = 0x1.921fb54442d18p+1 - a;
    }
    return (float)(y < 0.0f ? -a : a);
}
)
