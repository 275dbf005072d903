"""Host restatement of the short square-root sequence the trace kernels ship (rays1bench_amd/csrc/r1_exact_math.h, form B:
r1_sqrt_rsq), step for step in fp32 with exact fused multiply-adds, against the correctly rounded root.

The sequence starts from v_rsq_f32, whose bits only the chip knows: here the seed is the correctly rounded 1/sqrt(x) and its two
neighbours, which is what a 1-ulp instruction can return.  This is evidence for the sequence and a guard on the domain's lower
edge, not the proof — the proof is the comparison of all 2^32 inputs on the GPU (tools/check_exact_math.hip,
tests/test_gpu_exact_math.py).

* on D = [2^-96, FLT_MAX] (exponent fields 31..254): 10^7 random inputs (fixed seed) and the edges — 2^-96 and its upper
  neighbours, FLT_MAX and its lower neighbours, every power of two, squares and their neighbours — give the rounded root for
  all three seeds;
* below 2^-96 the same restatement does NOT: the residual x - g^2 falls into the subnormals and loses the bits the last step
  needs.  The guard of r1_sqrt_exact ends D where the compiler's own scaling starts for a reason."""
import re
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """fp32 fma(a, b, c), one rounding: the product is exact in fp64, the sum is rounded to odd in fp64 (two-sum error
    term) and then to fp32 — 53 bits >= 2 * 24 + 2, so the double rounding is innocuous."""
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    need = (err != 0) & even
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(need, np.nextafter(s, toward), s)
    with np.errstate(over="ignore", under="ignore"):
        return s.astype(F32)


def mul32(a, b):
    with np.errstate(over="ignore", under="ignore"):
        return (a.astype(F64) * b.astype(F64)).astype(F32)  # (the product is exact in fp64: one rounding)


def rsq_seed(x, ulps):
    """the correctly rounded 1/sqrt(x), moved by `ulps` fp32 steps"""
    y = (1.0 / np.sqrt(x.astype(F64))).astype(F32)  # (fp64 carries 53 bits: the rounding to fp32 is the correct one but for ties that do not occur)
    return (y.view(np.uint32).astype(np.int64) + ulps).astype(np.uint32).view(F32)


def sqrt_rsq(x, ulps):
    """r1_sqrt_rsq, instruction for instruction"""
    y = rsq_seed(x, ulps)
    g = mul32(x, y)
    h = mul32(np.full_like(x, 0.5), y)
    r = fma32(-h, g, np.full_like(x, 0.5))
    g = fma32(g, r, g)
    h = fma32(h, r, h)
    d = fma32(-g, g, x)
    return fma32(d, h, g)


def sqrt_rounded(x):
    return np.sqrt(x.astype(F64)).astype(F32)  # (53 >= 2 * 24 + 2: fp64 sqrt rounded to fp32 is the rounded fp32 root)


def from_bits(b):
    return np.asarray(b, np.uint32).view(F32)


def mismatches(x, ulps):
    got, want = sqrt_rsq(x, ulps), sqrt_rounded(x)
    return int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32)))


def test_the_header_ships_the_form_restated_here():
    text = open(os.path.join(ROOT, "rays1bench_amd", "csrc", "r1_exact_math.h")).read()
    assert re.search(r"#define R1_SQRT_FORM 2\b", text), "the kernels ship another form: restate that one here"
    body = text[text.index("float r1_sqrt_rsq("):]
    body = body[:body.index("}")]
    steps = [s.strip() for s in body.split(";")]
    assert any("__builtin_amdgcn_rsqf(x)" in s for s in steps)
    for want in ("g = x * y", "h = 0.5f * y", "r = __builtin_fmaf(-h, g, 0.5f)", "g = __builtin_fmaf(g, r, g)", "h = __builtin_fmaf(h, r, h)",
                 "d = __builtin_fmaf(-g, g, x)", "return __builtin_fmaf(d, h, g)"):
        assert any(s.endswith(want) for s in steps), want
    # the guard's domain: bits 0x0F800000 (2^-96) .. 0x7F7FFFFF (FLT_MAX)
    assert "(__float_as_uint(x) - 0x0F800000u) >= 0x70000000u" in text
    assert from_bits([0x0F800000])[0] == F32(2.0) ** F32(-96) and 0x0F800000 + 0x70000000 - 1 == 0x7F7FFFFF


def test_fma32_rounds_once():
    # (1 + 2^-12)^2 + 2^-60 = 1 + 2^-11 + 2^-24 + 2^-60: just above an fp32 tie.  A sum rounded to fp64 first drops the 2^-60 and
    # then rounds the tie to even, down; one rounding goes up.
    a = np.array([1 + 2.0 ** -12], F32)
    tiny = np.array([2.0 ** -60], F32)
    assert fma32(a, a, tiny)[0] == F32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert fma32(a, a, -tiny)[0] == F32(1 + 2.0 ** -11)
    assert fma32(a, a, np.zeros(1, F32))[0] == F32(1 + 2.0 ** -11)  # the tie itself: to even


def test_random_inputs_on_the_domain():
    rng = np.random.default_rng(20241)
    total, bad = 0, [0, 0, 0]
    for _ in range(5):
        n = 2_000_000
        bits = (rng.integers(31, 255, n, dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
        x = from_bits(bits)
        total += n
        for k, ulps in enumerate((-1, 0, 1)):
            bad[k] += mismatches(x, ulps)
    assert total >= 10_000_000
    assert bad == [0, 0, 0], f"mismatches for seeds -1 / 0 / +1 ulp: {bad} of {total}"


def test_edges_of_the_domain():
    lo, hi = 0x0F800000, 0x7F7FFFFF
    parts = [np.arange(lo, lo + 4096, dtype=np.uint32), np.arange(hi - 4095, hi + 1, dtype=np.uint32)]
    pow2 = (np.arange(31, 255, dtype=np.uint32) << np.uint32(23))
    parts += [pow2, pow2 + np.uint32(1), pow2[1:] - np.uint32(1)]
    # squares k^2 (k < 2^12: exact in fp32) times powers of four, and their neighbours: roots that are exact, and the nearest misses
    k = np.arange(1, 4096, dtype=np.float64)
    for e in (-94, -60, -20, 0, 20, 60, 100):
        sq = (k * k * 2.0 ** e).astype(F32).view(np.uint32)
        parts += [sq, sq + np.uint32(1), sq - np.uint32(1)]
    # halfway cases of the root: (m + 1/2)^2 rounded, m around 2^23 (the inputs whose root lies closest to a rounding boundary)
    m = np.arange(1 << 23, (1 << 23) + 4096, dtype=np.float64) + 0.5
    parts += [((m * m) * 2.0 ** -46).astype(F32).view(np.uint32)]
    bits = np.unique(np.concatenate(parts))
    bits = bits[(bits >= lo) & (bits <= hi)]
    x = from_bits(bits)
    assert lo in bits and hi in bits and len(bits) > 90_000
    for ulps in (-1, 0, 1):
        assert mismatches(x, ulps) == 0, ulps


def test_the_sequence_fails_below_the_domain():
    """exponent fields 1..30 (normal numbers below 2^-96): the restatement misses the rounded root for part of them — with
    every seed — so the guard's lower edge cannot move down"""
    rng = np.random.default_rng(7)
    n = 1_000_000
    bits = (rng.integers(1, 31, n, dtype=np.uint32) << np.uint32(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint32)
    x = from_bits(bits)
    for ulps in (-1, 0, 1):
        assert mismatches(x, ulps) > 100, ulps
