"""References for the erf-GELU tests (a plain helper module: no fixtures, no pytest settings; CPU only).

  * `gelu_f64(u)`                       the kernel's contract in f64: gelu(u) = u Phi(u), gelu'(u) = Phi(u) + u phi(u), Phi through erfc;
  * `gelu_f32_restatement(u)`           the kernel's two formulas restated operation by operation in float32 on the CPU (torch.special.erfc, torch.exp);
  * `kernel_inputs(dtype)`              the input set of the kernel tests, already rounded to `dtype`;
  * `err_units(got, ref)`               |got - ref| in units of 2^-24 max(|ref|, 2^-126): the f32 bar's measure;
  * `ulp(ref, dtype)`                   one unit in the last place of a 2-byte type at |ref|, the type's smallest subnormal as the floor;
  * `erf_oracle(monkeypatch)`           the whole-model reference: the oracle with its module-level quick_gelu replaced by torch.nn.functional.gelu
                                        for the duration of a test (oracle/lpi_oracle.py looks the name up at call time).
"""
import math

import torch

INV_SQRT2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794
F32_BAR_FACTOR = 4.0      # the GPU's f32 bar = this times the restatement's measured error: erfcf / expf of the device are a-few-ulp functions like the host's


def gelu_f64(u):
    """(gelu(u), gelu'(u)) in f64 from the values of `u` (any floating dtype) as they are stored."""
    u = u.double()
    cdf = 0.5 * torch.special.erfc(-u * INV_SQRT2)
    pdf = torch.exp(-0.5 * u * u) * INV_SQRT_2PI
    return u * cdf, cdf + u * pdf


def gelu_f32_restatement(u):
    """The kernel's arithmetic in float32 on the CPU, in the kernel's order of operations (csrc/act.hip gelu_erf_both); the host's erfc / exp stand in for
    the device's."""
    u = u.float()
    cdf = 0.5 * torch.special.erfc(-u * torch.tensor(INV_SQRT2, dtype=torch.float32))
    g = u * cdf
    dg = cdf + u * (torch.exp((-0.5 * u) * u) * torch.tensor(INV_SQRT_2PI, dtype=torch.float32))
    return g, dg


def kernel_inputs(dtype, n_random=4096, seed=0):
    """A grid over [-12, 12], 3 N(0, 1) samples, +-0, +-(the largest finite value of the type) and, for f32, +-1e-30 — rounded to `dtype` (1-D tensor)."""
    gen = torch.Generator().manual_seed(seed)
    parts = [torch.linspace(-12.0, 12.0, 2401, dtype=torch.float64), 3.0 * torch.randn(n_random, generator=gen, dtype=torch.float64),
             torch.tensor([0.0, -0.0], dtype=torch.float64)]
    big = torch.finfo(dtype).max
    parts.append(torch.tensor([big, -big], dtype=torch.float64))
    if dtype == torch.float32:
        parts.append(torch.tensor([1e-30, -1e-30], dtype=torch.float64))
    return torch.cat(parts).to(dtype)


def err_units(got, ref):
    """max |got - ref| / (2^-24 max(|ref|, 2^-126)) in f64."""
    got, ref = got.double(), ref.double()
    return float(((got - ref).abs() / (2.0 ** -24 * ref.abs().clamp_min(2.0 ** -126))).max())


_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}      # (explicit mantissa bits, exponent of the smallest normal)


def ulp(ref, dtype):
    """One unit in the last place of `dtype` (bf16 / f16) at |ref| (f64 tensor); below the normals the subnormal spacing, which is also the floor."""
    mant, emin = _FMT[dtype]
    e = torch.floor(torch.log2(ref.double().abs().clamp_min(2.0 ** (emin - 1)))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def restatement_error(dtype=torch.float32):
    """(units of g, units of gelu') of the float32 restatement against f64 on kernel_inputs(dtype): the measured basis of the GPU test's f32 bar."""
    u = kernel_inputs(dtype)
    g, dg = gelu_f32_restatement(u)
    rg, rdg = gelu_f64(u)
    assert bool(torch.isfinite(g).all() and torch.isfinite(dg).all())
    return err_units(g, rg), err_units(dg, rdg)


def erf_oracle(monkeypatch):
    """Patch the oracle's activation to nn.GELU (erf) until the test ends; returns the oracle module."""
    from oracle import lpi_oracle
    monkeypatch.setattr(lpi_oracle, "quick_gelu", torch.nn.functional.gelu)
    return lpi_oracle


assert math.isclose(INV_SQRT2, 1 / math.sqrt(2)) and math.isclose(INV_SQRT_2PI, 1 / math.sqrt(2 * math.pi))
