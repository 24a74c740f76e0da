"""The GELU evaluations of csrc/common.hpp restated in float32 on the CPU and compared with float64 erf-GELU: gelu_fast / dgelu_fast (the
degree-15 odd minimax fits behind the bf16 GEMM epilogues, coefficients parsed out of common.hpp) and gelu_f / dgelu_f (Abramowitz-Stegun
7.1.26, the float32 path).

Restatement: every fmaf is a float64 product and sum rounded once to float32 (the product of two float32 values is exact in float64), every
other operation is float32 arithmetic.  __expf and __frcp_rn are taken as the correctly rounded float32 functions; what two ulp of error in
each adds is bounded separately (A_S_INTRINSICS below) and added to the exported bound, not measured.

Inputs: every finite bf16 value (the epilogues evaluate the fits on bf16-rounded inputs, so this is exhaustive for them) and a dense float32
grid on [-8, 8].

Bounds, with x the input:
    |gelu_fast(x)  - gelu(x)|  <= GELU_E0 + GELU_DELTA * max(0, |x| - 4)
    |dgelu_fast(x) - gelu'(x)| <= DGELU_E0
    |gelu_f(x)  - gelu(x)|  <= GELU_F_E0 + GELU_F_REL * |x|          (+ A_S_INTRINSICS on the device)
    |dgelu_f(x) - gelu'(x)| <= DGELU_F_E0                              (+ A_S_INTRINSICS on the device)
Outside the clamp gelu_fast(x) = x * (0.5 + s(+-4)): the residual of the fit at 4 is multiplied by |x|, so the absolute error grows linearly
(and one float32 rounding of the product, 2^-24 |x|, rides on it).  The constants are what this test measures against float64, times 1.25;
the test prints the measured figures and fails when a figure exceeds its constant or when a constant is more than twice its figure.

gelu_fit_err / dgelu_fit_err / gelu_f_err / dgelu_f_err export the bounds to tests/test_gemm_family_gpu.py."""
import functools
import math
import os
import re

import torch

F32, F64 = torch.float32, torch.float64
COMMON_HPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'vln-goat_amd', 'csrc', 'common.hpp')

# measured by test_fast_fit_bounds / test_float32_path_bounds (printed there), times 1.25
GELU_E0 = 5.7e-5          # gelu_fast, |x| <= 4
GELU_DELTA = 3.4e-4       # gelu_fast, growth per unit of |x| beyond 4
DGELU_E0 = 3.5e-4         # dgelu_fast, everywhere
GELU_F_E0 = 6.0e-9        # gelu_f: absolute part
GELU_F_REL = 2.4e-7       # gelu_f: part proportional to |x| (float32 roundings of 0.5 x (1 + erf))
DGELU_F_E0 = 3.8e-7       # dgelu_f, everywhere
# Two ulp (2^-22 relative) in __frcp_rn and in each __expf: erf = 1 - poly(t) e, with poly(t) e <= 1 and |t poly'(t) / poly(t)| <= 1.6 on
# (0, 1], moves by at most (1 + 1.6) 2^-22 = 6.2e-7; gelu_f = 0.5 x (1 + erf) by 0.5 |x| poly e 2.6 2^-22 <= 0.5 * 0.9 * 6.2e-7 (|x| poly e
# peaks below 0.9); dgelu_f adds x phi(x) 2^-22 <= 0.25 * 2^-22.  Rounded up:
A_S_INTRINSICS = 7e-7


@functools.lru_cache(maxsize=None)
def coefficients():
    """{'GELU': [C0..C7], 'DGELU': [C0..C7]} as float32 tensors, parsed from common.hpp"""
    text = open(COMMON_HPP).read()
    found = re.findall(r'^#define GOAT_(D?GELU)_C(\d) (\S+?)f\s*$', text, re.M)
    assert len(found) == 16, 'expected sixteen GOAT_GELU_C* / GOAT_DGELU_C* coefficients, found %d' % len(found)
    out = {'GELU': [None] * 8, 'DGELU': [None] * 8}
    for fam, i, val in found:
        out[fam][int(i)] = torch.tensor(float(val), dtype=F32)
    assert all(c is not None for fam in out.values() for c in fam)
    return out


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _fit(x, c):
    """fmaf(xc, p(xc^2), 0.5) with Horner steps in fmaf, as gelu_fast / dgelu_fast write it -> (value, x)"""
    x = x.float()
    xc = x.clamp(-4.0, 4.0)
    t = xc * xc
    p = c[7].expand_as(x)
    for i in range(6, -1, -1):
        p = _fma(p, t, c[i])
    return _fma(xc, p, torch.tensor(0.5))


def gelu_fast(x):
    return x.float() * _fit(x, coefficients()['GELU'])


def dgelu_fast(x):
    return _fit(x, coefficients()['DGELU'])


def _fast_erf(x):
    ax = x.abs()
    t = (1.0 / (1.0 + torch.tensor(0.3275911, dtype=F32) * ax))                           # __frcp_rn: correctly rounded here
    k = [torch.tensor(v, dtype=F32) for v in (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)]
    poly = t * (k[0] + t * (k[1] + t * (k[2] + t * (k[3] + t * k[4]))))
    e = torch.exp((-ax * ax).double()).float()                                            # __expf: correctly rounded here
    return torch.copysign(1.0 - poly * e, x)


_RSQRT2 = torch.tensor(0.70710678118654752, dtype=F32)


def gelu_f(x):
    x = x.float()
    return 0.5 * x * (1.0 + _fast_erf(x * _RSQRT2))


def dgelu_f(x):
    x = x.float()
    e = torch.exp((-0.5 * x * x).double()).float()
    return 0.5 * (1.0 + _fast_erf(x * _RSQRT2)) + x * torch.tensor(0.3989422804014327, dtype=F32) * e


def gelu64(x):
    """0.5 x erfc(-x / sqrt 2) in float64: no cancellation in the left tail"""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def dgelu64(x):
    x = x.double()
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------ exported bounds
def _abs64(x):
    return torch.as_tensor(x).double().abs()


def gelu_fit_err(x):
    """bound on |gelu_fast(x) - gelu(x)|, monotone in |x|"""
    return GELU_E0 + GELU_DELTA * (_abs64(x) - 4.0).clamp_min(0.0)


def dgelu_fit_err(x):
    return torch.full_like(_abs64(x), DGELU_E0)


def gelu_f_err(x):
    """bound on |gelu_f(x) - gelu(x)| on the device (two ulp in __expf and __frcp_rn included), monotone in |x|"""
    return GELU_F_E0 + A_S_INTRINSICS + GELU_F_REL * _abs64(x)


def dgelu_f_err(x):
    return torch.full_like(_abs64(x), DGELU_F_E0 + A_S_INTRINSICS)


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def every_finite_bf16():
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    v = bits.view(torch.bfloat16).float()
    v = v[torch.isfinite(v)]
    assert v.numel() == 65536 - 2 * 128                      # exponent 255: two infinities and 2 * 127 NaNs
    return v


@functools.lru_cache(maxsize=None)
def dense_grid():
    return torch.linspace(-8.0, 8.0, (1 << 21) + 1, dtype=F64).float()


def _pinned(name, figure, const):
    print('FIT %s measured %.4e constant %.4e' % (name, figure, const))
    assert figure <= const, '%s: measured %.4e exceeds the constant %.4e' % (name, figure, const)
    assert const <= 2.0 * figure, '%s: the constant %.4e is more than twice the measured %.4e' % (name, const, figure)


def test_coefficients_parse():
    c = coefficients()
    assert abs(float(c['GELU'][0]) - 1.0 / math.sqrt(2.0 * math.pi)) < 1e-3         # s(x) ~ x phi(0) near 0
    assert abs(float(c['DGELU'][0]) - 2.0 / math.sqrt(2.0 * math.pi)) < 2e-3        # g(x) ~ 2 x phi(0) near 0


def test_fast_fit_bounds():
    e0 = de0 = delta = 0.0
    for name, x in (('bf16', every_finite_bf16()), ('grid', dense_grid())):
        err = (gelu_fast(x).double() - gelu64(x)).abs()
        derr = (dgelu_fast(x).double() - dgelu64(x)).abs()
        assert bool(torch.isfinite(err).all()) and bool(torch.isfinite(derr).all())
        inside = x.abs() <= 4.0
        a = float(err[inside].max())
        d = float(((err[~inside] - GELU_E0).clamp_min(0.0) / (x[~inside].double().abs() - 4.0)).max())
        b = float(derr.max())
        print('FIT %s: gelu_fast |x| <= 4 %.4e, growth beyond 4 %.4e per unit, dgelu_fast %.4e' % (name, a, d, b))
        e0, delta, de0 = max(e0, a), max(delta, d), max(de0, b)
        assert bool((err <= gelu_fit_err(x)).all()), name
        assert bool((derr <= dgelu_fit_err(x)).all()), name
    _pinned('GELU_E0', e0, GELU_E0)
    _pinned('GELU_DELTA', delta, GELU_DELTA)
    _pinned('DGELU_E0', de0, DGELU_E0)
    for xv in (-8.0, -64.0, -1000.0):
        x = torch.tensor([xv])
        print('FIT gelu_fast(%g) = %.4e (true %.1e), bound %.4e' % (xv, float(gelu_fast(x)), float(gelu64(x)), float(gelu_fit_err(x))))


def test_float32_path_bounds():
    rel = e0 = de0 = 0.0
    for name, x in (('bf16', every_finite_bf16()), ('grid', dense_grid())):
        err = (gelu_f(x).double() - gelu64(x)).abs()
        derr = (dgelu_f(x).double() - dgelu64(x)).abs()
        assert bool(torch.isfinite(err).all()) and bool(torch.isfinite(derr).all())
        ax = x.double().abs()
        r = float((err / ax.clamp_min(1e-300))[ax >= 1.0].max())
        a = float((err - GELU_F_REL * ax).max())
        b = float(derr.max())
        print('FIT %s: gelu_f error / |x| over |x| >= 1 %.4e, error - GELU_F_REL |x| %.4e, dgelu_f %.4e' % (name, r, a, b))
        rel, e0, de0 = max(rel, r), max(e0, a), max(de0, b)
        assert bool((err <= GELU_F_E0 + GELU_F_REL * ax).all()), name
        assert bool((derr <= DGELU_F_E0).all()), name
    _pinned('GELU_F_REL', rel, GELU_F_REL)
    _pinned('GELU_F_E0', e0, GELU_F_E0)
    _pinned('DGELU_F_E0', de0, DGELU_F_E0)


def test_common_hpp_states_the_asserted_bound():
    """the comment above the coefficients quotes the constants of this file"""
    text = open(COMMON_HPP).read()
    for const in (GELU_E0, GELU_DELTA, DGELU_E0):
        assert ('%.1e' % const) in text, 'common.hpp does not state %.1e' % const
