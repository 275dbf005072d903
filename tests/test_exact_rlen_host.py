"""Host restatement of the reciprocal length the trace kernels ship (rays1bench_amd/csrc/r1_exact_math.h: r1_rlen_from_rsq,
r1_rlen_total_form), step for step in fp32 with exact fused multiply-adds, against RN(1 / RN(sqrt(x))).

The sequence starts from v_rsq_f32 and v_rcp_f32, whose bits only the chip knows: here each seed is the correctly rounded value and
its two neighbours, which is what a 1-ulp instruction can return.  This is evidence and a guard on the construction of the total
form, not the proof — the proof is the comparison of all 2^32 inputs on the GPU (tools/check_exact_rlen.hip,
tests/test_gpu_exact_rlen.py).

* the shipped sequence (form 4: form B's root g, q = rcp(g), one Newton step) and the fallback (form 3) on D = [2^-96, FLT_MAX]:
  10^7 random inputs (fixed seed) and the edges of D give RN(1 / RN(sqrt(x))) for all three rsq seeds and the rounded rcp seed;
* what the restatement says about the candidates that did not ship and about the rcp seed (FIGURES_* below; the chip's own figures
  are in r1_exact_math.h):
    - form 1, the one-step candidate from q = h + h: 5 of the 10^7 random inputs miss (rsq seed rounded), a rate of 5e-7 — the
      chip's is 3e-7 (560 mismatches among the 0x70000000 inputs of D).  A handful of misses per 10^7 meant the chip would almost
      surely find some among 1.9 * 10^9;
    - form 2, two steps from q = h + h: none of 2 * 10^6 random inputs, but every root with an all-ones mantissa: 1 / g then lies
      2^-48 above a rounding tie and the steps approach it from below.  The chip found exactly those, 224;
    - form 4 with the rcp seed 1 ulp ABOVE the rounded reciprocal misses 8 of 2 * 10^6 random inputs, 1 ulp below none; form 3
      misses none either way.  So form 4 leans on what v_rcp_f32 returns for a few dozen mantissas, and only the chip's comparison
      of all 2^32 inputs (0 mismatches) admits it; form 3 is the form to fall back to on a chip whose v_rcp_f32 differs;
* the scaling identity of the total form below 2^-96, and its class routing: the lanes whose sequence ends in a NaN are exactly
  +-0, +inf, NaN and the negative numbers."""
import os
import re

import numpy as np

from test_exact_math_host import F32, F64, fma32, from_bits, mul32, rsq_seed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = 0x0F800000, 0x7F7FFFFF
ONE = F32(1.0)


def bump(v, ulps):
    return (v.view(np.uint32).astype(np.int64) + ulps).astype(np.uint32).view(F32)


def root_and_h(x, y):
    """r1_rlen_from_rsq up to `g = RN(sqrt(x))`: form B's root, and its h ~ 1 / (2 sqrt(x))"""
    g = mul32(x, y)
    h = mul32(np.full_like(x, 0.5), y)
    r = fma32(-h, g, np.full_like(x, 0.5))
    g = fma32(g, r, g)
    h = fma32(h, r, h)
    d = fma32(-g, g, x)
    return fma32(d, h, g), h


def newton(g, q):
    e = fma32(-g, q, np.full_like(g, ONE))
    return fma32(e, q, q)


def rcp_seed(g, ulps):
    with np.errstate(divide="ignore", invalid="ignore"):
        return bump((1.0 / g.astype(F64)).astype(F32), ulps)


def rlen(form, x, y, rcp_ulps=0):
    """r1_rlen_from_rsq<form>(x, y)"""
    g, h = root_and_h(x, y)
    with np.errstate(over="ignore", invalid="ignore"):
        if form == 4:
            return newton(g, rcp_seed(g, rcp_ulps))
        if form == 3:
            q = newton(g, rcp_seed(g, rcp_ulps))
            p = newton_with(g, q, q)
            return newton_with(g, p, q)
        q = newton(g, (h.astype(F64) + h.astype(F64)).astype(F32))
        return newton(g, q) if form == 2 else q


def newton_with(g, p, q):
    """the division chain's step: e = fma(-g, p, 1); p = fma(e, q, p)"""
    return fma32(fma32(-g, p, np.full_like(g, ONE)), q, p)


def rlen_rounded(x):
    """RN(1 / RN(sqrt(x))): fp64 carries 53 >= 2 * 24 + 2 bits, so each fp64 result rounded to fp32 is the rounded fp32 one"""
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.sqrt(x.astype(F64)).astype(F32)
        return (1.0 / g.astype(F64)).astype(F32)


def mismatches(form, x, rsq_ulps, rcp_ulps=0):
    got, want = rlen(form, x, rsq_seed(x, rsq_ulps), rcp_ulps), rlen_rounded(x)
    return int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32)))


def random_on_domain(rng, n):
    return from_bits((rng.integers(31, 255, n, dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32))


def edges_of_domain():
    parts = [np.arange(LO, LO + 4096, dtype=np.uint32), np.arange(HI - 4095, HI + 1, dtype=np.uint32)]
    pow2 = np.arange(31, 255, dtype=np.uint32) << np.uint32(23)
    parts += [pow2, pow2 + np.uint32(1), pow2[1:] - np.uint32(1)]
    k = np.arange(1, 4096, dtype=np.float64)
    for e in (-94, -60, -20, 0, 20, 60, 100):  # squares times powers of four and their neighbours: exact roots and the nearest misses
        sq = (k * k * 2.0 ** e).astype(F32).view(np.uint32)
        parts += [sq, sq + np.uint32(1), sq - np.uint32(1)]
    bits = np.unique(np.concatenate(parts))
    return from_bits(bits[(bits >= LO) & (bits <= HI)])


def test_the_header_ships_the_form_restated_here():
    text = open(os.path.join(ROOT, "rays1bench_amd", "csrc", "r1_exact_math.h")).read()
    assert re.search(r"#define R1_RLEN_FORM 4\b", text), "the kernels ship another form: restate that one here"
    body = text[text.index("float r1_rlen_from_rsq("):]
    body = body[:body.index("\n}")]
    for want in ("float g = x * y;", "float h = 0.5f * y;", "const float r = __builtin_fmaf(-h, g, 0.5f);", "g = __builtin_fmaf(g, r, g);",
                 "h = __builtin_fmaf(h, r, h);", "const float d = __builtin_fmaf(-g, g, x);", "g = __builtin_fmaf(d, h, g);",
                 "float q = FORM == 4 ? __builtin_amdgcn_rcpf(g) : h + h;", "float e = __builtin_fmaf(-g, q, 1.0f);", "q = __builtin_fmaf(e, q, q);"):
        assert want in body, want
    total = text[text.index("float r1_rlen_total_form("):]
    total = total[:total.index("\n}")]
    for want in ("const bool tiny = x < 0x1p-96f;", "const float xs = tiny ? x * 0x1p+64f : x;", "const float y = __builtin_amdgcn_rsqf(xs);",
                 "r = tiny ? r * 0x1p+32f : r;", "return r != r ? y : r;"):
        assert want in total, want
    assert from_bits([LO])[0] == F32(2.0) ** F32(-96)


def test_random_inputs_on_the_domain():
    rng = np.random.default_rng(20261)
    total, bad, fallback, one_step = 0, [0, 0, 0], 0, 0
    for _ in range(5):
        x = random_on_domain(rng, 2_000_000)
        total += x.size
        for k, ulps in enumerate((-1, 0, 1)):
            bad[k] += mismatches(4, x, ulps)
        fallback += mismatches(3, x, 0)
        one_step += mismatches(1, x, 0)
    print(f"FIGURES_random: form 1 (one step from h + h) misses {one_step} of {total}")
    assert total >= 10_000_000
    assert bad == [0, 0, 0] and fallback == 0, f"mismatches for rsq seeds -1 / 0 / +1 ulp (rounded rcp seed): {bad}, fallback {fallback} of {total}"
    assert one_step < 100  # (rare, not absent: the module's docstring)


def test_edges_of_the_domain():
    x = edges_of_domain()
    assert x.size > 90_000 and from_bits([LO])[0] in x and from_bits([HI])[0] in x
    for rsq_ulps in (-1, 0, 1):
        assert mismatches(4, x, rsq_ulps) == 0, rsq_ulps
        assert mismatches(3, x, rsq_ulps) == 0, rsq_ulps  # the fallback


def test_what_the_restatement_says_about_the_candidates():
    """The asserts say which candidates the restatement accepts; the chip's exhaustive comparison says which ship."""
    x = random_on_domain(np.random.default_rng(20262), 2_000_000)
    off = [mismatches(4, x, 0, u) for u in (-1, 1)]
    fallback_off = [mismatches(3, x, 0, u) for u in (-1, 1)]
    two_steps = mismatches(2, x, 0)
    print(f"FIGURES_candidates: form 4, rcp seed -1 / +1 ulp: {off}; form 3, the same: {fallback_off}; form 2: {two_steps} of {x.size}")
    assert off[0] == 0 and off[1] < 100 and fallback_off == [0, 0] and two_steps == 0
    # two steps from h + h miss the roots with an all-ones mantissa: 1 / g lies 2^-48 above a tie and is approached from below
    ones = from_bits(np.array([HI, HI - 1, 0x407FFFFF, 0x407FFFFE], np.uint32))
    assert mismatches(2, ones, 0) == ones.size and mismatches(4, ones, 0) == 0 and mismatches(3, ones, 0) == 0


def test_the_scaling_of_the_total_form():
    """below 2^-96: x * 2^64 is exact and lies in D (subnormals included), and RN(1 / RN(sqrt(x))) == RN(1 / RN(sqrt(x 2^64))) * 2^32,
    bit for bit — both roundings commute with the powers of two, and no result is subnormal"""
    rng = np.random.default_rng(20263)
    bits = np.concatenate([rng.integers(1, LO, 2_000_000, dtype=np.uint32), np.arange(1, 4097, dtype=np.uint32),
                           np.arange(0x00800000 - 2048, 0x00800000 + 2048, dtype=np.uint32), np.arange(LO - 4096, LO, dtype=np.uint32)])
    x = from_bits(bits)
    xs = mul32(x, np.full_like(x, F32(2.0) ** F32(64)))
    assert (xs.astype(F64) == x.astype(F64) * 2.0 ** 64).all()
    assert ((xs.view(np.uint32) >= LO) & (xs.view(np.uint32) <= HI)).all()
    want = rlen_rounded(x)
    scaled = mul32(rlen_rounded(xs), np.full_like(x, F32(2.0) ** F32(32)))
    assert (scaled.view(np.uint32) == want.view(np.uint32)).all()
    assert np.isfinite(want).all() and (want <= F32(2.0) ** F32(75)).all() and (want >= F32(2.0) ** F32(47)).all()
    # and the whole function: tiny inputs through the shipped sequence
    got = mul32(rlen(4, xs, rsq_seed(xs, 0)), np.full_like(x, F32(2.0) ** F32(32)))
    assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_the_class_routing_of_the_total_form():
    """`r != r ? y : r`: with the value v_rsq_f32 returns for each class (+-0 -> +-inf, +inf -> 0, NaN and negative -> NaN) the
    sequence ends in a NaN for exactly those inputs, and y is what the compiler's expression gives: +-inf, 0, NaN"""
    special = from_bits(np.array([0x00000000, 0x80000000, 0x7F800000, 0x7FC00000, 0x7F800001, 0xFFC12345, 0xFF800000, 0xBF800000, 0x80000001, 0x8F800000],
                                 np.uint32))
    with np.errstate(divide="ignore", invalid="ignore"):
        y = (1.0 / np.sqrt(special.astype(F64))).astype(F32)
        y[1] = -np.inf  # v_rsq_f32(-0) (numpy's sqrt(-0) = -0 gives the same; said here once more)
        for form in (4, 3):
            r = rlen(form, special, y)
            assert np.isnan(r).all(), form
        want = rlen_rounded(special)
    assert np.array_equal(np.isnan(y), np.isnan(want)) and (y[~np.isnan(y)] == want[~np.isnan(want)]).all()
    assert y[0] == np.inf and y[1] == -np.inf and y[2] == 0 and np.isnan(y[3:]).all()
    # on D every step is finite: no lane of the domain is routed away
    x = np.concatenate([edges_of_domain(), random_on_domain(np.random.default_rng(20264), 1_000_000)])
    for u in (-1, 0, 1):
        assert np.isfinite(rlen(4, x, rsq_seed(x, u))).all()
