"""CPU model of the forward render's staging-time footprint test (csrc/footprint.h): does a splat's
alpha >= 1/255 ellipse reach a pixel centre of an 8x8 quadrant?

Restated in NumPy float32, one individually rounded operation per kernel operation (the kernel's compiler may
contract a multiply into an add; the perturbation arguments below stand in for that and for the 1-ulp hardware
reciprocal and logarithm):

* ``two_edge_hit``   -- the test the kernels run: the least Q on the two edges that face the mean, raw reciprocals,
                        raw base-2 logarithm;
* ``four_edge_hit``  -- the earlier form: mean-inside early exit, all four edges, exact 1/a and 1/c, natural log;
* ``brute_hit64`` / ``brute_hit32`` -- what both must cover: some pixel centre of the quadrant has
                        min(0.99, o exp2(p2)) >= 1/255 with p2 <= 0, in float64 and in the render loop's own float32
                        expression (stage_conic's coefficients, the five-operation exponent).

Only the ellipse side is modelled; the footprint box (preprocess.hip) is a separate, earlier test.
All functions take arrays: conic (a, b, c), opacity o, mean (mx, my) in float32 and the quadrant's integer pixel
origin (qx, qy).
"""
import numpy as np

F = np.float32
LOG2E = F(1.4426950408889634)
LN2 = 0.6931471805599453


def ulps(x, k):
    """x moved by k units in the last place (float32)."""
    x = np.asarray(x, F).copy()
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf if k > 0 else -np.inf))
    return x


def guard_ok(a, b, c, o):
    """The degenerate-conic guard: where it fails the ellipse test is not run (the box decides)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (a > 0) & (c > 0) & (a * c - b * b > 0) & (o > 0)


def _offsets(mx, my, qx, qy):
    x0 = qx.astype(F) - mx
    y0 = qy.astype(F) - my
    return x0, x0 + F(7), y0, y0 + F(7)


def _clamp(v, lo, hi):
    return np.minimum(np.maximum(v, lo), hi)


def two_edge_hit(a, b, c, o, mx, my, qx, qy, ra_ulp=0, rc_ulp=0, log_ulp=0):
    a, b, c, o, mx, my = (np.asarray(v, F) for v in (a, b, c, o, mx, my))
    with np.errstate(all="ignore"):
        ok = guard_ok(a, b, c, o)
        ra, rc = ulps(F(1) / a, ra_ulp), ulps(F(1) / c, rc_ulp)
        l2 = ulps(np.log2(F(255) * o).astype(F), log_ulp)
        lim = np.maximum(F(0), l2) * F(2.0 * 1.001 * LN2) + F(0.02)
        x0, x1, y0, y1 = _offsets(mx, my, qx, qy)
        cx, cy = _clamp(F(0), x0, x1), _clamp(F(0), y0, y1)
        dy = _clamp(-b * cx * rc, y0, y1)
        qv = a * cx * cx + (F(2) * b * cx + c * dy) * dy
        dx = _clamp(-b * cy * ra, x0, x1)
        qh = c * cy * cy + (F(2) * b * cy + a * dx) * dx
        miss = (qv > lim) & (qh > lim)
    return ~(ok & miss)


def four_edge_hit(a, b, c, o, mx, my, qx, qy):
    a, b, c, o, mx, my = (np.asarray(v, F) for v in (a, b, c, o, mx, my))
    with np.errstate(all="ignore"):
        ok = guard_ok(a, b, c, o)
        tau = np.maximum(F(0), np.log(F(255) * o).astype(F)) * F(1.001) + F(0.01)
        lim = F(2) * tau
        ra, rc = F(1) / a, F(1) / c
        x0, x1, y0, y1 = _offsets(mx, my, qx, qy)
        best = np.full(a.shape, np.inf, F)
        for ex, ey in ((x0, y0), (x1, y1)):
            dy = np.minimum(y1, np.maximum(y0, -b * ex * rc))
            best = np.fmin(best, a * ex * ex + (F(2) * b * ex + c * dy) * dy)
            dx = np.minimum(x1, np.maximum(x0, -b * ey * ra))
            best = np.fmin(best, c * ey * ey + (F(2) * b * ey + a * dx) * dx)
        inside = (x0 <= 0) & (x1 >= 0) & (y0 <= 0) & (y1 >= 0)
        best = np.where(inside, F(0), best)
    return ~(ok & (best > lim))


def _pixels(qx, qy):
    i = np.arange(8)
    px = (qx[:, None, None] + i[None, None, :]).astype(F)  # [n, 1, 8]
    py = (qy[:, None, None] + i[None, :, None]).astype(F)  # [n, 8, 1]
    return px, py


def brute_hit64(a, b, c, o, mx, my, qx, qy):
    px, py = _pixels(qx, qy)
    a, b, c, o = (np.asarray(v, np.float64)[:, None, None] for v in (a, b, c, o))
    dx = np.asarray(mx, np.float64)[:, None, None] - px
    dy = np.asarray(my, np.float64)[:, None, None] - py
    p = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
    with np.errstate(over="ignore", invalid="ignore"):
        alpha = np.minimum(0.99, o * np.exp(p))
        return ((p <= 0) & (alpha >= 1.0 / 255.0)).any(axis=(1, 2))


def brute_hit32(a, b, c, o, mx, my, qx, qy):
    px, py = _pixels(qx, qy)
    a, b, c, o, mx, my = (np.asarray(v, F)[:, None, None] for v in (a, b, c, o, mx, my))
    A, B, C = F(-0.5) * LOG2E * a, -LOG2E * b, F(-0.5) * LOG2E * c  # stage_conic
    dx, dy = mx - px, my - py
    with np.errstate(over="ignore", invalid="ignore"):
        p2 = dx * (A * dx + B * dy) + C * dy * dy
        alpha = np.minimum(F(0.99), o * np.exp2(p2).astype(F))
        return ((p2 <= 0) & (alpha >= F(1.0) / F(255.0))).any(axis=(1, 2))
