"""The weights-first launch divides the nine phi numerators by 2h as q = float32(float64(x) * R), R = RN64(1 / d), WITHOUT the guard that
sends numerators 0 < |x| < 2^-100 down the IEEE road (csrc/f3d_solve_pair8.h, weights_first_stage1): each quotient is only looked at as
q * q, and below 2^-100 both roads square to +0.  Checked here in numpy (IEEE binary32 / binary64, round to nearest):

  * for the divisors 2h of all 40 levels of the default 512^3 pyramid, and 2^-20 and 2^20 (the ends of udiv_divisor_ok), every binade
    below 2^-100 -- 26 normal ones and the 23 of the subnormals --, both signs, significand all zeros, all ones and random: both squares
    are +0, bit for bit;
  * from 2^-100 up the two quotients themselves are the same float: random numerators over all binades and numerators placed next to
    the rounding boundaries of the quotient.
"""
import numpy as np
import pytest

RANDOM_PER_BINADE = 64
RANDOM_NORMAL = 1 << 17
MIDPOINTS = 1 << 15


def pyramid_divisors():
    """2h of the default pyramid (optical_flow levels: size = ceil(512 x float pow(0.95f, level)), h = 512 / size), then the range's ends"""
    d = []
    for level in range(40):
        scale = np.power(np.float32(0.95), np.float32(level), dtype=np.float32)
        size = np.ceil(np.float32(512) * scale)
        h = np.float32(512) / np.float32(size)
        d.append(np.float32(2) * h)
    assert d[0] == 2 and len(set(float(x) for x in d)) >= 39
    return d + [np.float32(2.0 ** -20), np.float32(2.0 ** 20)]


DIVISORS = pyramid_divisors()


def tiny_numerators(rng):
    """every binade below 2^-100, as bit patterns: exponent fields 1 .. 26 are 2^-126 .. 2^-101; field 0 holds the subnormals, whose
    binades are told apart by the leading bit of the significand"""
    bits = []
    for field in range(1, 27):
        base = field << 23
        bits += [base, base | 0x7FFFFF]
        bits += list(base | rng.integers(0, 1 << 23, RANDOM_PER_BINADE))
    for lead in range(23):
        lo = 1 << lead
        bits += [lo, 2 * lo - 1]
        bits += list(lo + rng.integers(0, lo, RANDOM_PER_BINADE))
    pos = np.array(bits, np.uint32)
    x = np.concatenate([pos, pos | np.uint32(0x80000000)]).view(np.float32)
    assert np.all(np.abs(x) > 0) and np.all(np.abs(x) < np.float32(2.0 ** -100))
    assert np.abs(x).max() == np.nextafter(np.float32(2.0 ** -100), np.float32(0)) and np.abs(x).min() == np.float32(2.0 ** -149)
    return x


def udiv(x, d):
    r = np.float64(1.0) / np.float64(d)
    with np.errstate(over="ignore", under="ignore"):
        return (x.astype(np.float64) * r).astype(np.float32)


@pytest.mark.parametrize("d", DIVISORS, ids=lambda d: "d=%a" % float(d))
def test_both_roads_square_to_plus_zero_below_2_to_minus_100(d):
    x = tiny_numerators(np.random.default_rng(3))
    with np.errstate(under="ignore"):
        fast = udiv(x, d)
        ieee = x / d
        sq_fast, sq_ieee = fast * fast, ieee * ieee
    assert sq_fast.dtype == np.float32 and sq_ieee.dtype == np.float32
    assert np.abs(ieee).max() < np.float32(2.0 ** -80) and np.abs(fast).max() <= np.float32(2.0 ** -80)
    assert not sq_fast.view(np.uint32).any(), "a squared udiv quotient is not +0"
    assert not sq_ieee.view(np.uint32).any(), "a squared IEEE quotient is not +0"


def normal_numerators(rng, d):
    """random bit patterns from 2^-100 up (both signs), and numerators next to a rounding boundary of the quotient: x = RN32(m d) and its
    two neighbours, m the midpoint above a random float q (such an x / d lies as close to a tie as a binary32 numerator can put it)"""
    mag = rng.integers(0x0D800000, 0x7F800000, RANDOM_NORMAL, dtype=np.uint32)
    sign = rng.integers(0, 2, RANDOM_NORMAL, dtype=np.uint32) << np.uint32(31)
    out = [(mag | sign).view(np.float32)]
    q = rng.integers(0x00800000, 0x7F000000, MIDPOINTS, dtype=np.uint32).view(np.float32)
    mid = (q.astype(np.float64) + np.nextafter(q, np.float32(np.inf)).astype(np.float64)) * 0.5
    with np.errstate(over="ignore", under="ignore"):
        x = (mid * np.float64(d)).astype(np.float32)
    for step in (np.float32(-np.inf), None, np.float32(np.inf)):
        y = x if step is None else np.nextafter(x, step)
        y = y[np.isfinite(y) & (np.abs(y) >= np.float32(2.0 ** -100))]
        out += [y, -y]
    return np.concatenate(out)


@pytest.mark.parametrize("d", DIVISORS, ids=lambda d: "d=%a" % float(d))
def test_quotients_agree_from_2_to_minus_100_up(d):
    x = normal_numerators(np.random.default_rng(int(np.float32(d).view(np.uint32))), d)
    assert x.size > RANDOM_NORMAL + 3 * MIDPOINTS and np.abs(x).min() >= np.float32(2.0 ** -100)
    with np.errstate(over="ignore"):
        ieee = x / d
    fast = udiv(x, d)
    assert ieee.dtype == np.float32
    bad = fast.view(np.uint32) != ieee.view(np.uint32)
    assert not bad.any(), "x = %a: %a against %a" % (float(x[bad][0]), float(fast[bad][0]), float(ieee[bad][0]))
