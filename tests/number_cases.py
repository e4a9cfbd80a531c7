"""Number texts for the device's conversions, with results from an arbiter outside the project (test infrastructure).

Pure Python, seeded, no project imports.  families() returns {name: [(text, expected), ...]} where expected is
    ("l", int)  ("u", int)  ("d", bits, flag)  or  "reject"
by the reference's parseNumber rule (parse_number.go:65-135) written out in expect(): no '.', 'e', 'E', at most 20
characters and fits int64 -> l; else no sign and fits uint64 -> u; else a float, with the overflowed-integer flag (bit 0 of
the tag word) when the text had no '.', 'e', 'E'; a float that rounds to +-Inf -> reject.  The double comes from CPython's
float(str) (David Gay's dtoa.c: correctly rounded, ties to even); rounded_bits() derives the same from Fraction(text)
alone, so that tests/test_number_cases.py can prove the arbiter without any C library.  go_format() lays Python's
shortest round-trip digits (repr) out by the reference's appendFloat rules (parsed_json.go:1250-1272).

Every text is a well-formed JSON number (no '+' in front, no leading zeros), and an exponent has at most four digits
unless the mantissa is zero: Go's readFloat clamps longer exponents at 10 000 where Python is exact, and nothing here
can arbitrate that.  REGRESSIONS is the place for texts that once showed a fault on the device."""
import decimal
import functools
import math
import random
import struct
from fractions import Fraction

TAG = {"l": ord("l") << 56, "u": ord("u") << 56, "d": ord("d") << 56}
INF_BITS = 0x7FF0000000000000
SIGN = 1 << 63

FAMILIES = ("binades", "bottom", "top", "clinger", "short_ties", "refine", "digits_19_20_21", "spellings", "integers", "tiebreak",
            "sticky", "random_fill", "regressions")

# texts that showed a fault of the device compile (none so far): (text, why)
REGRESSIONS = []


def f2bits(d):
    return struct.unpack("<Q", struct.pack("<d", d))[0]


def bits2f(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def go_format(x):
    """appendFloat(x) from Python's shortest digits."""
    if x == 0:
        return "-0" if math.copysign(1, x) < 0 else "0"
    sign, digits, exp = decimal.Decimal(repr(x)).as_tuple()
    digits = list(digits)
    while len(digits) > 1 and digits[-1] == 0:
        digits.pop()
        exp += 1
    nd, dp = len(digits), len(digits) + exp
    ds = "".join(map(str, digits))
    out = "-" if sign else ""
    a = abs(x)
    if 1e-6 <= a < 1e21:
        if dp > 0:
            out += ds[:min(nd, dp)] + "0" * max(0, dp - nd)
        else:
            out += "0"
        prec = max(nd - dp, 0)
        if prec:
            out += "." + "".join(ds[dp + i] if 0 <= dp + i < nd else "0" for i in range(prec))
        return out
    out += ds[0] + ("." + ds[1:] if nd > 1 else "")
    e = dp - 1
    es = "%s%02d" % ("-" if e < 0 else "+", abs(e))
    if es[0] == "-" and es[1] == "0":
        es = "-" + es[2:]
    return out + "e" + es


# ---- the arbiter -----------------------------------------------------------------------------------------------------------
def expect(text):
    """parseNumber (parse_number.go:65-135) on a well-formed number text"""
    float_only = any(c in text for c in ".eE")
    if not float_only and len(text) <= 20:
        v = int(text)
        if -(1 << 63) <= v < (1 << 63):
            return ("l", v)
        if text[0] != "-" and v < (1 << 64):
            return ("u", v)
    bits = f2bits(float(text))
    if bits & ~SIGN == INF_BITS:
        return "reject"
    return ("d", bits, 0 if float_only else 1)


def words(exp):
    """(tag word, value word) of the tape for an accepted expectation"""
    if exp[0] == "d":
        return TAG["d"] | exp[2], exp[1]
    return TAG[exp[0]], exp[1] & ((1 << 64) - 1)


def as_double(exp):
    """the arbiter's value as the double that Iter.Float returns (integers converted, round to nearest even)"""
    return bits2f(exp[1]) if exp[0] == "d" else float(exp[1])


def rounded_bits(text):
    """The binary64 nearest to the exact value of `text`, ties to even, from Fraction arithmetic alone; INF_BITS (with the sign)
    when that is beyond the largest double."""
    v = Fraction(text)
    sign = SIGN if text.lstrip()[0] == "-" else 0
    v = abs(v)
    if v == 0:
        return sign
    e = v.numerator.bit_length() - v.denominator.bit_length()  # 2^(e-1) < v < 2^(e+1)
    if Fraction(2) ** e > v:
        e -= 1
    e = max(e, -1022)
    q = v / Fraction(2) ** (e - 52)  # in [2^52, 2^53) for normals, below 2^52 for subnormals
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    bits = n if n < (1 << 52) and e == -1022 else ((e + 1023) << 52) + (n - (1 << 52))  # (a carry to 2^53 moves into the exponent)
    return sign | min(bits, INF_BITS)


# ---- building blocks ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pow5(k):
    return 5 ** k


def midpoint_above(bits):
    """exact decimal of the midpoint between the non-negative double `bits` and the next one -> (digit string, exponent of ten)"""
    ef, frac = bits >> 52, bits & ((1 << 52) - 1)
    m, e = (frac | (1 << 52), ef - 1075) if ef else (frac, -1074)
    n, p = 2 * m + 1, e - 1
    if p >= 0:
        return str(n << p), 0
    return str(n * _pow5(-p)), p


def sci(digits, e10, neg=False):
    """int(digits) * 10^e10 as d.ddd e+-x"""
    return ("-" if neg else "") + digits[0] + ("." + digits[1:] if len(digits) > 1 else "") + "e%d" % (e10 + len(digits) - 1)


def midpoint_texts(bits, neg=False):
    """the exact tie above `bits`, the tie with a far ...0001, and the tie with its last digit lowered by one"""
    digits, e10 = midpoint_above(bits)
    lower = str(int(digits) - 1)
    assert len(lower) == len(digits)  # (an odd number times a power of five or two is no power of ten)
    return [sci(digits, e10, neg), sci(digits + "0" * 20 + "1", e10 - 21, neg), sci(lower, e10, neg)]


def long_mantissa(text):
    """more than 19 significant digits with a non-zero one behind the 19th (the truncated-mantissa path)"""
    m = text.lstrip("-").split("e")[0].replace(".", "").lstrip("0")
    return len(m) > 19 and m[19:].strip("0") != ""


def with_point(w, q, k):
    """w * 10^q with the point behind the k-th digit of w (1 <= k <= digits of w)"""
    s = str(w)
    return s[:k] + "." + (s[k:] or "0") + ("e%d" % (q + len(s) - k) if q + len(s) - k else "")


# ---- families --------------------------------------------------------------------------------------------------------------
def _binades(rnd):
    out = []
    for e in range(0, 2047):
        for bits in (e << 52, (e << 52) | ((1 << 52) - 1), (e << 52) | rnd.getrandbits(52)):
            neg = rnd.random() < 0.25
            if bits:
                d = bits2f(bits)
                out += [("-" if neg else "") + t for t in (repr(d), format(d, ".16e"), format(d, ".24e"))]
                out += midpoint_texts(bits - 1, neg)  # the tie to the neighbour below (half the spacing below a power of two)
            else:
                out += ["0.0", "-0.0", "0e0"]
            out += midpoint_texts(bits, neg)
    return out


def _bottom(rnd):
    out = []
    for _ in range(300):
        d = bits2f(rnd.getrandbits(52) or 1)
        out += [repr(d), format(-d, ".16e"), format(d, ".24e")]
    for bits in (1, 2, 3, (1 << 51), (1 << 52) - 2, (1 << 52) - 1, 1 << 52, (1 << 52) + 1):
        out += [repr(bits2f(bits))] + midpoint_texts(bits) + midpoint_texts(bits - 1, True)
    half = str(_pow5(1075))  # 2^-1075 = 5^1075 * 10^-1075: the tie between 0 and the smallest subnormal -> even -> 0
    out += [half + "e-1075", sci(half, -1075), half + "0" * 10 + "1e-1086", sci(str(int(half) - 1), -1075), "-" + half + "e-1075"]
    out += ["2.2250738585072009e-308", "2.2250738585072011e-308", "2.2250738585072012e-308", "2.2250738585072013e-308",
            "2.2250738585072014e-308", "2.2250738585072016e-308", "2.225073858507201e-308", "4.9406564584124654e-324", "5e-324",
            "4.9e-324", "3e-324", "2.4703282292062327e-324", "2.4703282292062328e-324", "2.5e-324", "2.4e-324", "1e-323", "7.4e-324",
            "7.5e-324", "1e-400", "-1e-400", "1e-324", "-1e-324", "9e-325", "1e-9999", "-123456789012345678901234567890e-9999",
            "0e999999", "-0.0e-999999", "0e-999999", "0.000e+123456", "-0e1", "0.0", "-0.0", "0e0", "0.0e0"]
    for digits in ("1", "123", "22250738585072014", "49406564584124654417656879286822137236505980261"):
        for zeros in (5, 100, 307, 322, 323, 400):
            out += ["0." + "0" * zeros + digits, "-0." + "0" * zeros + digits + "e0", "0." + "0" * zeros + digits + "e-3"]
    return out


# (rejecting text, the accepted text one digit lower)
_MAX_TIE = str((1 << 1024) - (1 << 970))  # the exact midpoint between the largest double and 2^1024: tie -> even -> Inf


def reject_pairs():
    low30 = _MAX_TIE[:29] + str(int(_MAX_TIE[29]) - 1) + _MAX_TIE[30:]
    assert _MAX_TIE[29] != "0"
    pairs = [("1.7976931348623159e308", "1.7976931348623158e308"), (_MAX_TIE, low30), (sci(_MAX_TIE, 0), sci(low30, 0)),
             (_MAX_TIE + ".0", low30 + ".0"), (str(int(_MAX_TIE) + 1), low30), (sci(_MAX_TIE + "0" * 600 + "1", -601), sci(low30, 0)),
             ("1e309", "1e308"), ("1" + "0" * 309, "1" + "0" * 308), ("2e308", "1e308"), ("1.8e308", "1.7e308"),
             ("17976931348623159" + "0" * 292, "17976931348623158" + "0" * 292), ("9" * 400, "9" * 308), ("1" + "0" * 399, "1" + "0" * 308),
             ("1e9999", "1e99"), ("0.0001e313", "0.0001e312"), ("123456789012345678901234567890e290", "123456789012345678901234567890e270"),
             ("1" + "0" * 400 + ".5e-91", "1" + "0" * 400 + ".5e-92")]
    return pairs + [("-" + a, "-" + b) for a, b in pairs]


def _top():
    out = ["1.7976931348623157e308", "1.7976931348623158e308", "-1.7976931348623157e308", "1e308", "1" + "0" * 308,
           "17976931348623157" + "0" * 292, "8.98846567431158e307", "1.7976931348623155e308", "0.00017976931348623157e312"]
    for a, b in reject_pairs():
        out += [a, b]
    return out + midpoint_texts(0x7FEFFFFFFFFFFFFE) + midpoint_texts(0x7FEFFFFFFFFFFFFE, True)


def _clinger(rnd):
    out = []
    mants = [(1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 53) + 2, 1, 3, 9007199254740993]
    mants += [rnd.randrange(10 ** 14, 10 ** 16) for _ in range(40)]
    for w in mants:
        for q in range(-23, 24):
            neg = "-" if rnd.random() < 0.2 else ""
            out.append(neg + "%de%d" % (w, q))
            out.append(neg + with_point(w, q, rnd.randrange(1, len(str(w)) + 1)))
    return out


def _short_ties(rnd):
    """(2M+1) * 2^k exactly, in at most 19 digits and a power of ten of -4..23"""
    out = []
    for q in range(0, 24):
        p5 = 5 ** q
        lo, hi = -(-(1 << 53) // p5), ((1 << 54) - 1) // p5  # odd w in [lo, hi]: w * 5^q is an odd number of 54 bits
        for _ in range(60):
            w = rnd.randrange(lo, hi + 1) | 1  # (M = w * 5^q >> 1 comes out even and odd alike)
            if w > hi:
                continue
            for j in (0, 1, rnd.randrange(2, 12), rnd.randrange(12, 40), 60):  # * 2^j: past 2^53, so not Clinger's path
                ww = w << j
                if ww >= 10 ** 19:
                    break
                out.append("%de%d" % (ww, q))
                out.append(("-" if j & 1 else "") + with_point(ww, q, rnd.randrange(1, len(str(ww)) + 1)))
    for q in range(1, 5):
        for _ in range(150):
            n = rnd.randrange(1 << 53, min(1 << 54, 10 ** 19 // 5 ** q) - 1) | 1
            w = n * 5 ** q
            out += ["%de-%d" % (w, q), with_point(w, -q, len(str(w)) - q), "-" + with_point(w, -q, 1)]
    out += ["9007199254740993", "9007199254740995", "9007199254740993.0", "1e23", "2e23", "4e23", "8.5e23", "9007199254740993e0"]
    return out


def _pow5_hi64(q):
    """the high 64 bits of the 128-bit 5^q (q >= 0) or of its reciprocal (q < 0), computed here"""
    if q >= 0:
        p = 5 ** q
        return p << (64 - p.bit_length()) if p.bit_length() <= 64 else p >> (p.bit_length() - 64)
    p = 5 ** -q
    b = p.bit_length() + 127
    c = (1 << b) // p + 1
    while c >= 1 << 128:
        c >>= 1
    while c < 1 << 127:
        c <<= 1
    return c >> 64


def _refine(rnd, want=1200):
    """(w, q) for which the low nine bits of the high word of w * top64(5^q) are all ones: the 128-bit product is refined"""
    out = []
    while len(out) < want:
        q = rnd.randrange(-342, 309)
        hi = _pow5_hi64(q)
        for _ in range(3000):
            w = rnd.randrange(1 << 53, 10 ** 19) if rnd.random() < 0.8 else rnd.randrange(1, 1 << 53)
            if (((w << (64 - w.bit_length())) * hi) >> 64) & 0x1FF != 0x1FF:
                continue
            if w < (1 << 53) and -22 <= q <= 22:
                continue  # (Clinger's path)
            if q + len(str(w)) > 308 or q + len(str(w)) < -322:
                continue  # (finite and not zero)
            out.append("%de%d" % (w, q))
    return out


def _digits_19_20_21(rnd):
    out = []
    tails = ["", "0", "00", "1", "5", "9", "01", "50", "49", "51", "5" + "0" * 30 + "1", "4" + "9" * 30, "0" * 40, "0" * 40 + "7"]
    for _ in range(1500):
        w = str(rnd.randrange(10 ** 18, 10 ** 19))
        q = rnd.randrange(-320, 285)
        for t in rnd.sample(tails, 4):
            out.append(w + t + "e%d" % q)
            out.append(w[:1] + "." + w[1:] + t + "e%d" % q)
    for v in ((1 << 64) - 2, (1 << 64) - 1, 1 << 64, (1 << 64) + 1, (1 << 64) + 2, 10 ** 19 - 1, 10 ** 19, 10 ** 19 + 1, (1 << 63) + 1):
        for sfx in ("", ".0", "e0", "e1", "e-1", "0", "00", "e-30", "e280", ".5", "1", "9"):
            out += [str(v) + sfx, "-" + str(v) + sfx]
    return out


def _spellings(rnd):
    out = ["1E+2", "1e+2", "1e-0", "1E-0", "-1e+0", "1e0000000005", "1e-0000000005", "1.5e+007", "2E-00003", "1e00", "1E0300", "1e-0300",
           "-0", "-0.0", "0", "0.0", "-0e0", "0.5", "0.000123", "-0.25e2", "0.1", "0.2", "0.3", "0.7", "1.0", "10.0", "100.000",
           "0.1e1", "0.1E-1", "123.456e-2", "5e-1", "0.0000001", "0.000001", "1e21", "1e20", "999999999999999900000.0", "1e-7",
           "0.30000000000000004", "0.1000000000000000055511151231257827", "3.141592653589793238462643383279502884197",
           "1" + "0" * 300, "1.5" + "0" * 500, "1." + "0" * 700 + "1", "0." + "0" * 50 + "1" + "0" * 300, "12345678" + "0" * 200 + ".0" + "0" * 200,
           "1" + "0" * 100 + "e-100", "1." + "0" * 100 + "e+100", "100e-2", "1" + "0" * 30 + "e-30", "0." + "9" * 30, "0." + "9" * 17]
    src = "1234567890" * 5
    for pos in range(26, 37):  # the byte at index 31 of the text is a digit, a point, an 'e' or a sign in turn
        for sgn in ("", "-"):
            body = sgn + src[:pos - len(sgn)]
            out += [body + ".5", body + "e5", body + "e-5", body + "e+5", body + ".25e-3", body + "E-305", body + "0"]
            out += [sgn + "0." + src[:pos - len(sgn) - 2] + t for t in ("", "e5", "e-5", "E+5")]
    return out


def _integers(rnd):
    out = []
    for nd in range(1, 22):
        for _ in range(30):
            v = rnd.randrange(10 ** (nd - 1), 10 ** nd) if nd > 1 else rnd.randrange(10)
            out += [str(v), "-" + str(v)]
        out += ["9" * nd, "-" + "9" * nd, str(10 ** (nd - 1)), "-" + str(10 ** (nd - 1))]
    for c in (10 ** 18, 10 ** 19, 1 << 63, 1 << 64, 10 ** 9, 1 << 32, 1 << 53, 10 ** 20):
        for d in range(-2, 3):
            out += [str(c + d), "-" + str(c + d)]
    return out


def _tiebreak(rnd, n=5200):
    """numbers of more than 19 digits whose neighbours disagree (exact ties and texts next to them): the big-integer path"""
    out = []
    while len(out) < 3 * n:
        bits = (rnd.randrange(0, 2047) << 52) | rnd.getrandbits(52)
        if bits in (0, 0x7FEFFFFFFFFFFFFF):
            continue
        three = midpoint_texts(bits, rnd.random() < 0.3)
        if long_mantissa(three[0]) and long_mantissa(three[2]):  # (a tie of up to 19 digits is decided without the big integers)
            out += three
    return out


def _sticky(rnd):
    """ties of 700 and more digits with zeros up to and beyond the 800 digits that are kept, then a one; and ties
    longer than 400 digits with their last digit lowered"""
    out = []
    for _ in range(400):
        bits = (rnd.randrange(0, 60) << 52) | rnd.getrandbits(52) | 1 - (_ & 1)
        digits, e10 = midpoint_above(bits)
        if len(digits) < 700:
            continue
        pad = 801 - len(digits) + rnd.randrange(0, 40)
        out += [sci(digits + "0" * pad + "1", e10 - pad - 1, _ % 3 == 0), sci(digits + "0" * pad, e10 - pad), sci(digits, e10)]
        out.append(midpoint_texts(bits)[2])
    return out


def _random_fill(rnd, n_bits=200000, n_short=60000):
    out = []
    while len(out) < n_bits:
        d = bits2f(rnd.getrandbits(64))
        if d == d and abs(d) != math.inf:
            out.append(repr(d))
    for _ in range(n_short):  # short decimals of the kind documents contain
        k = rnd.randrange(5)
        if k == 0:
            out.append("%d.%02d" % (rnd.randrange(-100000, 100000), rnd.randrange(100)))
        elif k == 1:
            out.append(repr(round(rnd.uniform(-180, 180), rnd.randrange(1, 8))))
        elif k == 2:
            out.append(str(rnd.randrange(-10 ** 6, 10 ** 9)))
        elif k == 3:
            out.append(repr(round(rnd.uniform(-1e6, 1e6), rnd.randrange(0, 8)) * 10.0 ** rnd.randrange(-30, 30)))
        else:
            out.append("%d.%de%d" % (rnd.randrange(1000), rnd.randrange(10 ** 6), rnd.randrange(-40, 40)))
    return out


def _well_formed(t):
    s = t[1:] if t[0] == "-" else t
    m, _, e = s.replace("E", "e").partition("e")
    ip, _, fp = m.partition(".")
    ok = ip.isdigit() and (ip == "0" or ip[0] != "0") and ("." not in m or fp.isdigit())
    if "e" in s.lower():
        ed = e.lstrip("+-")
        ok = ok and ed.isdigit() and len(e) - len(ed) <= 1
        ok = ok and (len(ed.lstrip("0")) <= 4 or int(m.replace(".", "")) == 0)  # (the readFloat clamp: see the module text)
    return ok


@functools.lru_cache(maxsize=None)
def families(seed=20261016):
    """{family: [(text, expected), ...]}, the same for the same seed"""
    builders = [("binades", _binades), ("bottom", _bottom), ("top", lambda r: _top()), ("clinger", _clinger),
                ("short_ties", _short_ties), ("refine", _refine), ("digits_19_20_21", _digits_19_20_21), ("spellings", _spellings),
                ("integers", _integers), ("tiebreak", _tiebreak), ("sticky", _sticky), ("random_fill", _random_fill),
                ("regressions", lambda r: [t for t, _ in REGRESSIONS] + ["0"])]
    assert tuple(name for name, _ in builders) == FAMILIES
    fam = {}
    for k, (name, fn) in enumerate(builders):
        texts = fn(random.Random(seed * 100 + k))
        for t in texts:
            assert _well_formed(t), (name, t[:60])
        fam[name] = [(t, expect(t)) for t in texts]
    return fam


def accepted(cases):
    return [(t, e) for t, e in cases if e != "reject"]


def sample(rnd, n):
    """n accepted texts drawn over all families but the random fill (for generated documents)"""
    fam = families()
    names = [k for k in fam if k != "random_fill"]
    out = []
    while len(out) < n:
        t, e = rnd.choice(fam[rnd.choice(names)])
        if e != "reject":
            out.append(t)
    return out
