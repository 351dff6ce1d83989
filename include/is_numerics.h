/*
 * is_numerics.h -- deterministic scalar numerics shared by the HIP column-DP core
 * and by the CPU oracle.
 *
 * The reference evaluates `__logf` / `logf` inside its device code
 * (/root/reference/InstanceStixels/src/StixelsKernels.cu:31-42, 88-199), built with
 * --use_fast_math, which is not reproducible off NVIDIA hardware.  The
 * canonical numerics of this project are IEEE fp32 with no contraction; for the logarithm we
 * use ONE implementation, written only with IEEE +,-,* on binary64, a 32-entry table of
 * binary64 literals and integer bit manipulation, so that host gcc and gfx950 hipcc produce
 * bit-identical results.  It sits on the serial critical path of the pairwise DP (two calls per
 * row), hence table + short polynomial and no division.
 *
 * Accuracy: the binary64 evaluation has relative error < 3e-10 of the result (worst case next
 * to x = 1, far below half an fp32 ulp = 6e-8), so the fp32 result is the correctly rounded
 * logarithm except when the true value lies that close to a rounding boundary;
 * tests/test_numerics.py pins |is_logf - libm logf| <= 1 ulp.
 *
 * Plain C99 / C++ / HIP.  Compile every user with -ffp-contract=off.
 */
#ifndef IS_NUMERICS_H_
#define IS_NUMERICS_H_

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define IS_HD __host__ __device__ __forceinline__
#define IS_TABLE_QUAL __device__ __constant__
#else
#define IS_HD static inline
#endif

IS_HD uint64_t is_bits_f64(double x) {
    uint64_t u;
    memcpy(&u, &x, sizeof(u));
    return u;
}
IS_HD double is_f64_bits(uint64_t u) {
    double x;
    memcpy(&x, &u, sizeof(x));
    return x;
}
IS_HD uint32_t is_bits_f32(float x) {
    uint32_t u;
    memcpy(&u, &x, sizeof(u));
    return u;
}
IS_HD float is_f32_bits(uint32_t u) {
    float x;
    memcpy(&x, &u, sizeof(x));
    return x;
}

/* log(x), x = 2^k * m, m in [1, 2): i = top 5 mantissa bits selects the centre
 * c_i = 1 + (i + 0.5)/32 (c_0 = 1 so that nothing cancels next to x = 1);
 * r = m * (1/c_i) - 1, |r| < 1/32;  log m = log c_i + (r - r^2/2 + r^3/3 - r^4/4 + r^5/5 - r^6/6).
 * Tables: IS_LOG_INVC[i] = RN(1/c_i), IS_LOG_LOGC[i] = log(1/IS_LOG_INVC[i]) (hex literals). */
#define IS_LOG_TABLE_BITS 5
/* The two 32-entry tables as literals.  `is_log_tables` copies them (e.g. into LDS, so that the
 * serial pairwise chain does not wait on global memory); `is_logf_t` evaluates with caller-
 * provided tables; `is_logf` uses the literals directly.  All three give identical bits. */
#define IS_LOG_TABLE_SIZE (1 << IS_LOG_TABLE_BITS)
IS_HD void is_log_tables(double* invc, double* logc) {
    const double INVC[32] = {
        0x1.0000000000000p+0,
        0x1.e9131abf0b767p-1,
        0x1.dae6076b981dbp-1,
        0x1.cd85689039b0bp-1,
        0x1.c0e070381c0e0p-1,
        0x1.b4e81b4e81b4fp-1,
        0x1.a98ef606a63bep-1,
        0x1.9ec8e951033d9p-1,
        0x1.948b0fcd6e9e0p-1,
        0x1.8acb90f6bf3aap-1,
        0x1.8181818181818p-1,
        0x1.78a4c8178a4c8p-1,
        0x1.702e05c0b8170p-1,
        0x1.6816816816817p-1,
        0x1.6058160581606p-1,
        0x1.58ed2308158edp-1,
        0x1.51d07eae2f815p-1,
        0x1.4afd6a052bf5bp-1,
        0x1.446f86562d9fbp-1,
        0x1.3e22cbce4a902p-1,
        0x1.3813813813814p-1,
        0x1.323e34a2b10bfp-1,
        0x1.2c9fb4d812ca0p-1,
        0x1.27350b8812735p-1,
        0x1.21fb78121fb78p-1,
        0x1.1cf06ada2811dp-1,
        0x1.1811811811812p-1,
        0x1.135c81135c811p-1,
        0x1.0ecf56be69c90p-1,
        0x1.0a6810a6810a7p-1,
        0x1.0624dd2f1a9fcp-1,
        0x1.0204081020408p-1};
    const double LOGC[32] = {
        0x0.0p+0,
        0x1.77458f632dcfcp-5,
        0x1.341d7961bd1d1p-4,
        0x1.a926d3a4ad563p-4,
        0x1.0d77e7cd08e59p-3,
        0x1.44d2b6ccb7d1ep-3,
        0x1.7ab890210d909p-3,
        0x1.af3c94e80bff3p-3,
        0x1.e27076e2af2e6p-3,
        0x1.0a324e27390e3p-2,
        0x1.22941fbcf7966p-2,
        0x1.3a64c556945eap-2,
        0x1.51aad872df82dp-2,
        0x1.686c81e9b14afp-2,
        0x1.7eaf83b82afc1p-2,
        0x1.947941c2116fbp-2,
        0x1.a9cec9a9a084ap-2,
        0x1.beb4d9da71b79p-2,
        0x1.d32fe7e00ebd5p-2,
        0x1.e744261d6878ap-2,
        0x1.faf588f78f31cp-2,
        0x1.0723e5c1cdf42p-1,
        0x1.109f39e2d4c97p-1,
        0x1.19ee6b467c96fp-1,
        0x1.23130d7bebf43p-1,
        0x1.2c0e9ed448e8cp-1,
        0x1.34e289d9ce1d2p-1,
        0x1.3d9026a7156fbp-1,
        0x1.4618bc21c5ec2p-1,
        0x1.4e7d811b75bb0p-1,
        0x1.56bf9d5b3f399p-1,
        0x1.5ee02a9241675p-1};
    for (int i = 0; i < IS_LOG_TABLE_SIZE; i++) {
        invc[i] = INVC[i];
        logc[i] = LOGC[i];
    }
}
IS_HD void is_log_table(int i, double* invc, double* logc) {
    const double INVC[32] = {
        0x1.0000000000000p+0,
        0x1.e9131abf0b767p-1,
        0x1.dae6076b981dbp-1,
        0x1.cd85689039b0bp-1,
        0x1.c0e070381c0e0p-1,
        0x1.b4e81b4e81b4fp-1,
        0x1.a98ef606a63bep-1,
        0x1.9ec8e951033d9p-1,
        0x1.948b0fcd6e9e0p-1,
        0x1.8acb90f6bf3aap-1,
        0x1.8181818181818p-1,
        0x1.78a4c8178a4c8p-1,
        0x1.702e05c0b8170p-1,
        0x1.6816816816817p-1,
        0x1.6058160581606p-1,
        0x1.58ed2308158edp-1,
        0x1.51d07eae2f815p-1,
        0x1.4afd6a052bf5bp-1,
        0x1.446f86562d9fbp-1,
        0x1.3e22cbce4a902p-1,
        0x1.3813813813814p-1,
        0x1.323e34a2b10bfp-1,
        0x1.2c9fb4d812ca0p-1,
        0x1.27350b8812735p-1,
        0x1.21fb78121fb78p-1,
        0x1.1cf06ada2811dp-1,
        0x1.1811811811812p-1,
        0x1.135c81135c811p-1,
        0x1.0ecf56be69c90p-1,
        0x1.0a6810a6810a7p-1,
        0x1.0624dd2f1a9fcp-1,
        0x1.0204081020408p-1};
    const double LOGC[32] = {
        0x0.0p+0,
        0x1.77458f632dcfcp-5,
        0x1.341d7961bd1d1p-4,
        0x1.a926d3a4ad563p-4,
        0x1.0d77e7cd08e59p-3,
        0x1.44d2b6ccb7d1ep-3,
        0x1.7ab890210d909p-3,
        0x1.af3c94e80bff3p-3,
        0x1.e27076e2af2e6p-3,
        0x1.0a324e27390e3p-2,
        0x1.22941fbcf7966p-2,
        0x1.3a64c556945eap-2,
        0x1.51aad872df82dp-2,
        0x1.686c81e9b14afp-2,
        0x1.7eaf83b82afc1p-2,
        0x1.947941c2116fbp-2,
        0x1.a9cec9a9a084ap-2,
        0x1.beb4d9da71b79p-2,
        0x1.d32fe7e00ebd5p-2,
        0x1.e744261d6878ap-2,
        0x1.faf588f78f31cp-2,
        0x1.0723e5c1cdf42p-1,
        0x1.109f39e2d4c97p-1,
        0x1.19ee6b467c96fp-1,
        0x1.23130d7bebf43p-1,
        0x1.2c0e9ed448e8cp-1,
        0x1.34e289d9ce1d2p-1,
        0x1.3d9026a7156fbp-1,
        0x1.4618bc21c5ec2p-1,
        0x1.4e7d811b75bb0p-1,
        0x1.56bf9d5b3f399p-1,
        0x1.5ee02a9241675p-1};
    *invc = INVC[i];
    *logc = LOGC[i];
}

/* Special values of C99 logf: log(+-0) = -inf, log(x<0) = NaN, log(+inf) = +inf,
 * log(NaN) = NaN, log(1) = +0.  Returns 1 and sets *out when x is one of them. */
IS_HD int is_logf_special(float x, float* out) {
    const uint32_t ix = is_bits_f32(x);
    if ((ix & 0x7fffffffu) == 0u) { *out = is_f32_bits(0xff800000u); return 1; }         /* +-0 */
    if ((ix & 0x7fffffffu) > 0x7f800000u) { *out = is_f32_bits(0x7fc00000u); return 1; } /* NaN */
    if (ix & 0x80000000u) { *out = is_f32_bits(0x7fc00000u); return 1; }                 /* x < 0 */
    if (ix == 0x7f800000u) { *out = x; return 1; }                                       /* +inf */
    if (ix == 0x3f800000u) { *out = 0.0f; return 1; }                                    /* 1 */
    return 0;
}
IS_HD int is_logf_index(float x) { /* table index of a positive finite x */
    const uint64_t dx = is_bits_f64((double)x);
    return (int)((dx >> (52 - IS_LOG_TABLE_BITS)) & ((1u << IS_LOG_TABLE_BITS) - 1u));
}
IS_HD float is_logf_eval(float x, double invc, double logc) { /* positive finite x, its table entry */
    /* exact widening: fp32 subnormals are normal binary64 numbers */
    const uint64_t dx = is_bits_f64((double)x);
    const int k = (int)((dx >> 52) & 0x7ffu) - 1023;
    const double m = is_f64_bits((dx & 0x000fffffffffffffull) | 0x3ff0000000000000ull); /* [1,2) */
    const double r = m * invc - 1.0;
    double p = -1.0 / 6.0;
    p = p * r + 1.0 / 5.0;
    p = p * r - 1.0 / 4.0;
    p = p * r + 1.0 / 3.0;
    p = p * r - 1.0 / 2.0;
    p = p * r + 1.0;
    p = p * r;
    const double res = ((double)k * 0x1.62e42fefa39efp-1 + logc) + p;
    return (float)res;
}

/* Natural logarithm with caller-provided copies of the tables. */
IS_HD float is_logf_t(float x, const double* invc_tab, const double* logc_tab) {
    float special;
    if (is_logf_special(x, &special)) return special;
    const int i = is_logf_index(x);
    return is_logf_eval(x, invc_tab[i], logc_tab[i]);
}

/* Natural logarithm of an fp32 value, fp32 result. */
IS_HD float is_logf(float x) {
    float special;
    if (is_logf_special(x, &special)) return special;
    double invc, logc;
    is_log_table(is_logf_index(x), &invc, &logc);
    return is_logf_eval(x, invc, logc);
}

/* ---- erf, atan and cos for the ground model (Stixels::PrecomputeGroundShared, k_ground_model) and the road
 * parameters (RoadEstimation::ChooseLineShared, k_road_choose) --------------------------------------------------
 * The host path calls libm's erff / atanf / cosf, whose bits no device function reproduces.  These three are the
 * project's own: evaluated in binary64 with + - * / and comparisons only (no libm, no ocml, no bit tricks), rounded
 * once to fp32, so host gcc and gfx950 hipcc give identical bits; each within 1 ulp of libm on its domain
 * (tests/test_ground_device_cpu.py).  The literals below are printed by tools/gen_is_numerics.py (piecewise
 * Chebyshev interpolants from 50-digit mpmath samples, converted to monomials and rounded once to binary64);
 * `tools/gen_is_numerics.py --check` compares them with this header. */
/* ---- GENERATED by tools/gen_is_numerics.py: do not edit by hand ---- */
/* erf: row 0 in t = (x^2 - 1/32) * 32 (times x), row k in t = (x - (k/4 + 1/8)) * 8; worst interpolation error of a piece, relative to its largest value: 3.11e-16 */
#define IS_ERF_N 11
#define IS_ERF_ROWS 16
#define IS_ERF_INIT { \
    {0x1.1de2518732898p+0, -0x1.7a0301be8a946p-7, 0x1.c3fde757c76d3p-14, -0x1.ad9cb9bf83c77p-21, 0x1.4db84517a0032p-28, -0x1.b47feaf799728p-36, 0x1.ec24393394868p-44, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0}, \
    {0x1.9dd0d2b721f39p-2, 0x1.f5f0cdaf1531dp-4, -0x1.78749a434fe19p-8, -0x1.e106c51d2bf5ep-12, 0x1.5529abccdf1d2p-15, 0x1.7488b8f0b375ap-20, -0x1.9a7945130e3fap-23, -0x1.65c2588161401p-29, 0x1.70990ba530b49p-31, 0x1.0e9169b80c3ccp-40, -0x1.05ab9f99c33c3p-39}, \
    {0x1.3f196dcd0f135p-1, 0x1.86e9694134bdap-4, -0x1.e8a3c39181e7ep-8, -0x1.c810502297c7dp-14, 0x1.6963c8a398d08p-15, -0x1.c1242aada7819p-21, -0x1.52b26674c9e79p-23, 0x1.c7c9cfba16e35p-28, 0x1.b62ed4d92b040p-32, -0x1.d86da2d7eeebdp-36, -0x1.802983f922e13p-41}, \
    {0x1.91724951b8fc6p-1, 0x1.0cab61f084bb6p-4, -0x1.d62beb64e8464p-8, 0x1.7c9d7569b9c35p-13, 0x1.cc60567da3f4ep-16, -0x1.1350f4377bd33p-19, -0x1.53bb4c3ee665ap-25, 0x1.30ab0925082abp-27, -0x1.e3ec2bd13dd7fp-34, -0x1.a8b0f2ff30348p-36, 0x1.d29001cab5ce5p-41}, \
    {0x1.c6dad2829ec62p-1, 0x1.45e99bcbb78f6p-5, -0x1.6ea6cf452e851p-8, 0x1.4cb3cf0ab46c7p-12, 0x1.ca508316f94bcp-18, -0x1.f65d16602ed45p-20, 0x1.fd1c6aadd7eaep-25, 0x1.3acd74d2f3c8bp-28, -0x1.8b422d2add308p-32, -0x1.8199d11c91797p-39, 0x1.2cbb1c8447d73p-40}, \
    {0x1.e5768c3b4a3fcp-1, 0x1.5ce595c455a91p-6, -0x1.dfbbadedf5d24p-9, 0x1.4374d82e2ac60p-12, -0x1.f3b8d52d4ecabp-18, -0x1.f572c67277989p-21, 0x1.6b16f54fecf13p-24, -0x1.73f073c7c6a6dp-31, -0x1.174098bd70b71p-32, 0x1.99d54a25e20bcp-37, 0x1.54967b580071dp-42}, \
    {0x1.f4f693b67bd77p-1, 0x1.499d478bca6dap-7, -0x1.0bcfca21947bcp-9, 0x1.d6631e1a45435p-13, -0x1.974c03688e991p-17, -0x1.17d435b34fb0ep-24, 0x1.d857f3a19faaap-25, -0x1.95494628d0679p-29, -0x1.2e4bd378fd609p-35, 0x1.7062c6c6e1c69p-37, -0x1.71521c1b4bf4bp-42}, \
    {0x1.fbe61eef4cf6ap-1, 0x1.12ceb37ff9c2cp-8, -0x1.01a1c847fa1edp-10, 0x1.143d1c6f3e9f8p-13, -0x1.5a316520c8606p-17, 0x1.779b1f0ef1cc5p-22, 0x1.0d099d315d932p-26, -0x1.42fd8d1a4be1cp-29, 0x1.76fdb76e846b3p-34, 0x1.7f265afba3fbap-39, -0x1.977bc87a93dc7p-42}, \
    {0x1.fea4218d65948p-1, 0x1.94624e78e1012p-10, -0x1.ada873603c84ap-12, 0x1.0ea475da288c2p-14, -0x1.afe5545f4bd72p-18, 0x1.9973b524de5e2p-22, -0x1.dd7483133dfe2p-28, -0x1.ea071ed15f0d0p-31, 0x1.695fec38c17f7p-34, -0x1.2bfad6a68611bp-39, 0x0.0p+0}, \
    {0x1.ff9960f3eb328p-1, 0x1.06918b6355667p-11, -0x1.37ccd586218cbp-13, 0x1.c1ec102e1c50ep-16, -0x1.ae59610730793p-19, 0x1.11dae4a74b1f9p-22, -0x1.982c1f1212385p-27, 0x1.027ac8f3bb3c2p-34, 0x1.3898529770943p-35, -0x1.60a02a85e8fa0p-39, 0x0.0p+0}, \
    {0x1.ffe514bbdc198p-1, 0x1.2ce89880923f9p-13, -0x1.8af14829b1776p-15, 0x1.407fbd1901c7cp-17, -0x1.62d4c5e316413p-20, 0x1.146c4b1cd3a5fp-23, -0x1.26808e02d3ee8p-27, 0x1.64f94ca0ea2a2p-32, 0x1.3acc8f118f38ap-39, -0x1.40dd1476dc43dp-40, 0x0.0p+0}, \
    {0x1.fff9ba420e835p-1, 0x1.30538fbb77cdep-15, -0x1.b5781e9f330abp-17, 0x1.89e17c07adfc0p-19, -0x1.ed4ac6244f0c7p-22, 0x1.c11f2644cc643p-25, -0x1.2ade4fdc91cf9p-28, 0x1.152087661ba8ap-32, -0x1.19a6b8d1476dfp-37, -0x1.1874ac470b4cfp-43, 0x0.0p+0}, \
    {0x1.fffeb3ebb267bp-1, 0x1.0f9e1b4dd3386p-17, -0x1.a8670aaa6afa5p-19, 0x1.a3737e2ad6750p-21, -0x1.24544e9aa1578p-23, 0x1.2e7e7595eebf0p-26, -0x1.da49ffd533f9ap-30, 0x1.176de0832283cp-33, -0x1.d2070dd988607p-38, 0x1.a6d0071aad20ap-43, 0x0.0p+0}, \
    {0x1.ffffc316d9ed0p-1, 0x1.abe09e914488cp-20, -0x1.690585c6d5389p-21, 0x1.84522fe8c7e57p-23, -0x1.298f8f2485da0p-25, 0x1.57757741ea125p-28, -0x1.33095c30e82f4p-31, 0x1.ac99fa42b26acp-35, -0x1.cd955edae4910p-39, 0x1.64555c901349dp-43, 0x0.0p+0}, \
    {0x1.fffff618c3da6p-1, 0x1.296a70c47fb81p-22, -0x1.0d887658cfff1p-23, 0x1.394b3379186c6p-25, -0x1.05760e78e25aep-27, 0x1.4c16f98544548p-30, -0x1.4b94d68355440p-33, 0x1.0b549efb35696p-36, -0x1.533b729f854e3p-40, 0x0.0p+0, 0x0.0p+0}, \
    {0x1.fffffe92ced93p-1, 0x1.6ce1a9bbe3519p-25, -0x1.617a9cde3405fp-26, 0x1.b95fda93973bcp-28, -0x1.8e1fd11e62e05p-30, 0x1.13651585b9f3dp-32, -0x1.2eacb35a7d273p-35, 0x1.11a9bd47eaeefp-38, -0x1.8c6db61d4c415p-42, 0x0.0p+0, 0x0.0p+0}, \
}
/* atan: row 0 in t = (x^2 - 1/128) * 128 (times x), row k in t = (x - (k/8 + 1/16)) * 16; worst interpolation error of a piece, relative to its largest value: 1.54e-16 */
#define IS_ATAN_N 11
#define IS_ATAN_ROWS 8
#define IS_ATAN_INIT { \
    {0x1.feac41fea8233p-1, -0x1.5228ef73d219cp-9, 0x1.92d3479bd5f9ep-17, -0x1.1d928d4d769a9p-24, 0x1.b8d980d5e3393p-32, -0x1.65f736dbc0065p-39, 0x1.2c922fe4a0160p-46, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0, 0x0.0p+0}, \
    {0x1.7b97b4bce5b02p-3, 0x1.ee9c7f8458e05p-5, -0x1.665c226d69ed8p-11, -0x1.1344bb7385ea4p-14, 0x1.42aca8b912297p-19, 0x1.c32d900d1ae3dp-24, -0x1.13e9ac9f0a9d3p-27, -0x1.17f6dffadd92dp-33, 0x1.bc2c87d58c6c6p-36, -0x1.230c35b1edf40p-43, -0x1.4893b29fd4c07p-44}, \
    {0x1.362773707ebccp-2, 0x1.d272ca3fc5b1bp-5, -0x1.0997e8aec91e9p-10, -0x1.6cf6666d66b34p-15, 0x1.8dd1e8e6c08bcp-19, 0x1.2483b88b5f38cp-27, -0x1.f49591bfccd0dp-28, 0x1.b905a699bea88p-33, 0x1.cfc3973c417f7p-37, -0x1.0fa1a76ba1239p-40, 0x0.0p+0}, \
    {0x1.a64eec3cc23fep-2, 0x1.adbe87f94905ep-5, -0x1.3b9d8eab581fbp-10, -0x1.57c09645aa763p-16, 0x1.679531b79aeecp-19, -0x1.f2d8bfc92f149p-25, -0x1.f38a7f347b786p-29, 0x1.32c4151558348p-32, -0x1.3436c1961c874p-39, -0x1.5beedb137d6b5p-41, 0x0.0p+0}, \
    {0x1.0657e94db30d0p-1, 0x1.84f00c2780613p-5, -0x1.4c62cb562eb34p-10, -0x1.e6495b39e62dbp-20, 0x1.063c2f9dd0c22p-19, -0x1.58b7848cbe22ep-24, -0x1.41d52a4600e48p-32, 0x1.938e8613a06d4p-33, -0x1.14ff0f536dc5dp-37, -0x1.be117514b315bp-45, 0x0.0p+0}, \
    {0x1.345f01cce37bbp-1, 0x1.5babcc647fa91p-5, -0x1.449db09428cdcp-10, 0x1.655caac4d7369p-17, 0x1.3bbbd29f54136p-20, -0x1.34a2f98404c00p-24, 0x1.84d692fb71e03p-30, 0x1.1f9c3cee62f09p-34, -0x1.b0651e2676ff4p-38, 0x1.9bab9c9811edep-43, 0x0.0p+0}, \
    {0x1.5d58987169b18p-1, 0x1.34679ace01346p-5, -0x1.2ddfb0391372bp-10, 0x1.2491307b47565p-16, 0x1.29c7e49f8d3b1p-21, -0x1.bca781fcd0fc0p-25, 0x1.e63d7d474e157p-30, -0x1.95254df17cc98p-38, -0x1.8d40429d2573bp-39, 0x1.6f9de705bda8bp-43, 0x0.0p+0}, \
    {0x1.819d0b7158a4dp-1, 0x1.107fbbe011080p-5, -0x1.0feeb40894954p-10, 0x1.50e5afb911e79p-16, 0x1.2a7c27dc35c4cp-23, -0x1.12bd24ad2f597p-25, 0x1.93fea02de75b5p-30, -0x1.11573156c70cep-35, -0x1.5491693973d7fp-41, 0x1.77cd8bdd7ecccp-44, 0x0.0p+0}, \
}
/* cos: row 0 cos(x), row 1 sin(y) / y, both in t = (u - 0.32) * 3.125, u = x^2 or y^2 <= 0.64; worst interpolation error of a piece, relative to its largest value: 1.08e-16 */
#define IS_COS_N 7
#define IS_COS_ROWS 2
#define IS_COS_INIT { \
    {0x1.b03dca0d68ddap-1, -0x1.367b320f4b193p-3, 0x1.0ec629cf4a15ep-8, -0x1.7520331e2e50fp-15, 0x1.12500e5d4e108p-22, -0x1.f4ff71c8df1dcp-31, 0x1.379ea5ea0d8b5p-39}, \
    {0x1.e5207e37e555ep-1, -0x1.a715a153e3c26p-5, 0x1.b541bbe7ee567p-11, -0x1.ac9d1671a9272p-18, 0x1.e94085041fa3ep-26, -0x1.6d2e0b40fe0f6p-34, 0x1.8029ad83648a6p-43}, \
}
#define IS_PIO2_HI 0x1.921fb54442d18p+0 /* RN(pi/2) */
#define IS_PIO2_LO 0x1.1a62633145c07p-54 /* RN(pi/2 - IS_PIO2_HI) */
/* ---- end of the generated literals ---- */

IS_HD double is_horner(const double* c, int n, double t) {
    double p = c[n - 1];
    for (int i = n - 2; i >= 0; i--) p = p * t + c[i];
    return p;
}

/* erf(x): odd, non-decreasing, |result| <= 1, +-1 from |x| >= 4 on (and wherever the value rounds to it:
 * |x| >= 3.8325); erf(+-0) = +-0, erf(+-inf) = +-1, erf(NaN) = NaN. */
IS_HD float is_erff(float xf) {
    const double C[IS_ERF_ROWS][IS_ERF_N] = IS_ERF_INIT;
    const double x = (double)xf;
    if (x != x) return xf + xf;
    const double ax = x < 0 ? -x : x; /* (-0 stays -0: row 0 returns it) */
    if (ax >= 4.0) return x < 0 ? -1.0f : 1.0f;
    int k = ax >= 2.0 ? 8 : 0; /* piece k: [k/4, (k+1)/4) */
    k += ax >= (k + 4) * 0.25 ? 4 : 0;
    k += ax >= (k + 2) * 0.25 ? 2 : 0;
    k += ax >= (k + 1) * 0.25 ? 1 : 0;
    double r;
    if (k == 0) r = ax * is_horner(C[0], IS_ERF_N, (ax * ax - 0.03125) * 32.0);
    else r = is_horner(C[k], IS_ERF_N, (ax - (k * 0.25 + 0.125)) * 8.0);
    const float rf = (float)r;
    return x < 0 ? -rf : rf;
}

/* atan(x): odd; atan(+-0) = +-0, atan(+-inf) = +-RN(pi/2), atan(NaN) = NaN. */
IS_HD float is_atanf(float xf) {
    const double C[IS_ATAN_ROWS][IS_ATAN_N] = IS_ATAN_INIT;
    const double x = (double)xf;
    if (x != x) return xf + xf;
    const double ax = x < 0 ? -x : x;
    const int inv = ax > 1.0;
    const double z = inv ? 1.0 / ax : ax; /* [0, 1] (1 / inf = 0) */
    int k = z >= 0.5 ? 4 : 0; /* piece k: [k/8, (k+1)/8), the last one closed */
    k += z >= (k + 2) * 0.125 ? 2 : 0;
    k += z >= (k + 1) * 0.125 ? 1 : 0;
    double r;
    if (k == 0) r = z * is_horner(C[0], IS_ATAN_N, (z * z - 0.0078125) * 128.0);
    else r = is_horner(C[k], IS_ATAN_N, (z - (k * 0.125 + 0.0625)) * 16.0);
    if (inv) r = IS_PIO2_HI - (r - IS_PIO2_LO);
    const float rf = (float)r;
    return x < 0 ? -rf : rf;
}

/* cos(x) for x in [-pi/2, pi/2] -- the range of is_atanf; RN(pi/2) as fp32 lies above pi/2 and gives the small
 * negative value cosf gives.  Outside (up to +-3.9) the result is a finite number without meaning; NaN gives NaN. */
IS_HD float is_cosf(float xf) {
    const double C[IS_COS_ROWS][IS_COS_N] = IS_COS_INIT;
    const double x = (double)xf;
    const double ax = x < 0 ? -x : x;
    if (ax < 0.7853981633974483) return (float)is_horner(C[0], IS_COS_N, (ax * ax - 0.32) * 3.125);
    const double y = (IS_PIO2_HI - ax) + IS_PIO2_LO; /* (exact difference for ax in [pi/4, pi]) */
    return (float)(y * is_horner(C[1], IS_COS_N, (y * y - 0.32) * 3.125));
}

#endif /* IS_NUMERICS_H_ */
