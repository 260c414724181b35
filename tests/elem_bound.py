"""The element bound the route tests share (tests/test_gpu_grad_routes.py, tests/test_gpu_forward_fp64.py and their CPU companions):
|g_e - r_e| <= tau * s_e for every element e, with r the float64 reference and s_e = sqrt(sum_m t_m^2) over the products t_m summed into
e -- the size of a summation error, which does not shrink when the terms cancel -- and the least-squares scale <g, r> / <r, r> = 1 +- tau.

TAU_FP32 / TAU_BF16X3 were calibrated on an MI355X on the gradient routes (fp32 worst 3.5e-6, bf16x3 3.0e-5: products of the split
arithmetic carry ~16 mantissa bits); the bounds sit 6-10x above."""

TAU_FP32 = 2e-5
TAU_BF16X3 = 2e-4


def bound(g, r, s, tau):
    """(worst |g - r| / s, least-squares scale <g, r> / <r, r>, holds): the element bound and the scale check together."""
    g, r, s = g.double().reshape(-1), r.double().reshape(-1), s.double().reshape(-1)
    d = (g - r).abs()
    if bool(((s == 0) & (d > 0)).any()):
        worst = float("inf")
    else:
        nz = s > 0
        worst = float((d[nz] / s[nz]).max()) if bool(nz.any()) else 0.0
    rr = float((r * r).sum())
    scale = float((g * r).sum()) / rr if rr > 0 else 1.0
    return worst, scale, worst <= tau and abs(scale - 1.0) <= tau
