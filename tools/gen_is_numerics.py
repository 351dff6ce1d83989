#!/usr/bin/env python3
"""Generator of the coefficient literals of is_erff / is_atanf / is_cosf (include/is_numerics.h).

    python3 tools/gen_is_numerics.py            # prints the C fragment between the GENERATED markers
    python3 tools/gen_is_numerics.py --check    # compares it with the header, exit 1 on a difference

Method.  Every function is evaluated piecewise in binary64 by Horner's rule; each piece is the Chebyshev
interpolant of the function on that piece (Chebyshev nodes of the first kind, 50-digit mpmath samples), converted
to the monomial basis of the piece's own variable in 50 digits and rounded ONCE to binary64.  The pieces:

  erf   [0, 1/4):          erf(x) = x * P(u),  u = x^2            (relative accuracy down to the subnormals)
        [k/4, (k+1)/4):    erf(x) = Q_k(t),    t = (x - c_k) * 8  k = 1 .. 15, c_k the centre;  x >= 4: 1
  atan  [0, 1/8):          atan(x) = x * P(u), u = x^2
        [k/8, (k+1)/8]:    atan(x) = Q_k(t),   t = (x - c_k) * 16 k = 1 .. 7;  x > 1: pi/2 - atan(1/x)
  cos   [0, pi/4):         cos(x) = P(u),      u = x^2
        [pi/4, pi/2]:      cos(x) = y * S(y^2), y = (PIO2_HI - x) + PIO2_LO  (the subtraction is exact)

The degrees are the smallest at which the interpolation error, measured here in 50 digits on 400 points per piece,
is below 2^-51 of the piece's largest value (the binary64 rounding of the coefficients alone costs up to 2^-53); the script prints that error beside every table.
"""
import sys

import mpmath as mp

mp.mp.dps = 50


def cheb_monomial(f, a, b, deg):
    """monomial coefficients (ascending, in t = (x - c) / h on [-1, 1]) of the Chebyshev interpolant of f on [a, b]"""
    n = deg + 1
    c, h = (a + b) / 2, (b - a) / 2
    nodes = [mp.cos(mp.pi * (k + mp.mpf(1) / 2) / n) for k in range(n)]
    vals = [f(c + h * t) for t in nodes]
    coef = []
    for j in range(n):
        s = sum(vals[k] * mp.cos(mp.pi * j * (k + mp.mpf(1) / 2) / n) for k in range(n)) * 2 / n
        coef.append(s / 2 if j == 0 else s)
    # T_j in the monomial basis by the recurrence T_{j+1} = 2 t T_j - T_{j-1}
    T = [[mp.mpf(1)], [mp.mpf(0), mp.mpf(1)]]
    for j in range(2, n):
        nxt = [mp.mpf(0)] + [2 * v for v in T[j - 1]]
        for i, v in enumerate(T[j - 2]):
            nxt[i] -= v
        T.append(nxt)
    mono = [mp.mpf(0)] * n
    for j in range(n):
        for i, v in enumerate(T[j]):
            mono[i] += coef[j] * v
    return mono


def to_double(v):
    return float(mp.nstr(v, 40))


def horner_err(f, a, b, mono_d, scale):
    """largest |f - polynomial| on [a, b] relative to `scale`, the polynomial taken with its binary64 coefficients"""
    c, h = (a + b) / 2, (b - a) / 2
    worst = mp.mpf(0)
    for k in range(401):
        t = mp.mpf(-1) + mp.mpf(2) * k / 400
        p = mp.mpf(0)
        for v in reversed(mono_d):
            p = p * t + mp.mpf(v)
        worst = max(worst, abs(p - f(c + h * t)))
    return worst / scale


def piece(f, a, b, scale_of=None):
    a, b = mp.mpf(a), mp.mpf(b)
    scale = abs(f(b)) if scale_of is None else scale_of
    for deg in range(4, 30):
        mono = [to_double(v) for v in cheb_monomial(f, a, b, deg)]
        err = horner_err(f, a, b, mono, scale)
        if err < mp.mpf(2) ** -51:
            return mono, err
    raise SystemExit("no degree below 30 reaches 2^-51")


def table(name, rows, errs, comment):
    width = max(len(r) for r in rows)
    out = [f"/* {comment}; worst interpolation error of a piece, relative to its largest value: "
           f"{mp.nstr(max(errs), 3)} */",
           f"#define {name}_N {width}"]
    out.append(f"#define {name}_ROWS {len(rows)}")
    out.append(f"#define {name}_INIT {{ \\")
    for r in rows:
        r = r + [0.0] * (width - len(r))
        out.append("    {" + ", ".join(float(v).hex() for v in r) + "}, \\")
    out.append("}")
    return out


def generate():
    out = []
    # ---- erf
    rows, errs = [], []
    f0 = lambda u: mp.erf(mp.sqrt(u)) / mp.sqrt(u) if u > 0 else 2 / mp.sqrt(mp.pi)
    # in u = x^2 on [0, 1/16]; the table row is in t = (u - 1/32) * 32
    m, e = piece(f0, 0, mp.mpf(1) / 16, scale_of=mp.mpf(1))
    rows.append(m), errs.append(e)
    for k in range(1, 16):
        m, e = piece(mp.erf, mp.mpf(k) / 4, mp.mpf(k + 1) / 4)
        rows.append(m), errs.append(e)
    out += table("IS_ERF", rows, errs, "erf: row 0 in t = (x^2 - 1/32) * 32 (times x), row k in t = (x - (k/4 + 1/8)) * 8")
    # ---- atan
    rows, errs = [], []
    g0 = lambda u: mp.atan(mp.sqrt(u)) / mp.sqrt(u) if u > 0 else mp.mpf(1)
    m, e = piece(g0, 0, mp.mpf(1) / 64, scale_of=mp.mpf(1))
    rows.append(m), errs.append(e)
    for k in range(1, 8):
        m, e = piece(mp.atan, mp.mpf(k) / 8, mp.mpf(k + 1) / 8)
        rows.append(m), errs.append(e)
    out += table("IS_ATAN", rows, errs, "atan: row 0 in t = (x^2 - 1/128) * 128 (times x), row k in t = (x - (k/8 + 1/16)) * 16")
    # ---- cos / sin on [0, pi/4] (a little more: 0.8 > pi/4, so that both pieces overlap)
    c0 = lambda u: mp.cos(mp.sqrt(u)) if u > 0 else mp.mpf(1)
    s0 = lambda u: mp.sin(mp.sqrt(u)) / mp.sqrt(u) if u > 0 else mp.mpf(1)
    mc, ec = piece(c0, 0, mp.mpf("0.64"), scale_of=mp.mpf(1))
    ms, es = piece(s0, 0, mp.mpf("0.64"), scale_of=mp.mpf(1))
    out += table("IS_COS", [mc, ms], [ec, es], "cos: row 0 cos(x), row 1 sin(y) / y, both in t = (u - 0.32) * 3.125, u = x^2 or y^2 <= 0.64")
    # ---- pi/2 in two parts
    hi = to_double(mp.pi / 2)
    lo = to_double(mp.pi / 2 - mp.mpf(hi))
    out.append(f"#define IS_PIO2_HI {hi.hex()} /* RN(pi/2) */")
    out.append(f"#define IS_PIO2_LO {lo.hex()} /* RN(pi/2 - IS_PIO2_HI) */")
    return "\n".join(out) + "\n"


BEGIN = "/* ---- GENERATED by tools/gen_is_numerics.py: do not edit by hand ---- */\n"
END = "/* ---- end of the generated literals ---- */\n"

if __name__ == "__main__":
    text = generate()
    if "--check" in sys.argv:
        import os
        header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "is_numerics.h")).read()
        have = header.split(BEGIN)[1].split(END)[0]
        if have != text:
            sys.exit("include/is_numerics.h does not hold what this script generates")
        print("include/is_numerics.h holds the generated literals")
    else:
        sys.stdout.write(BEGIN + text + END)
