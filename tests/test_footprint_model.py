"""The staging-time footprint test (csrc/footprint.h) is conservative and as tight as the form it replaced.

tests/footprint_model.py restates the two-edge test the kernels run and the earlier four-edge test in NumPy
float32.  Both are held against brute force over the 64 pixel centres of a quadrant, in float64 and in the
render loop's own float32 expression:

* whenever brute force finds a pixel with alpha >= 1/255, the test reports a hit -- no exceptions, and for the
  two-edge test also with the reciprocals and the logarithm each moved by +-2 ulp (the hardware's v_rcp_f32 and
  v_log_f32 are good to 1 ulp);
* on the random set the two-edge test's false hits number at most 1.02 x the four-edge test's.

Inputs: 240k random cases (conics with axis ratios up to 50:1 at all angles, means from 40 px outside the
quadrant to inside it, opacities from 0.9/255 to 1) and an adversarial set: means within 1e-3 px of the
rectangle's edges and corners, ellipses whose alpha = 1/255 contour passes within 1e-3 px of a corner pixel
centre, b = 0, a = c, and degenerate conics, which the guard must hand to the box (a hit).
"""
import itertools

import numpy as np
import pytest

from tests import footprint_model as M

F = np.float32
N_RANDOM = 240_000
N_ADV = 30_000


def _conic(rng, n, s_lo=0.3, s_hi=30.0, ratio=50.0):
    """Conics of ellipses with sigmas log-uniform in [s_lo, s_hi] px, axis ratio <= ratio, any angle."""
    s1 = np.exp(rng.uniform(np.log(s_lo), np.log(s_hi), n))
    s2 = np.clip(s1 * np.exp(rng.uniform(-np.log(ratio), np.log(ratio), n)), s1 / ratio, s1 * ratio)
    s2 = np.clip(s2, s_lo / ratio, s_hi * ratio)
    s2 = np.where(np.maximum(s1, s2) / np.minimum(s1, s2) > ratio, s1, s2)
    th = rng.uniform(0, np.pi, n)
    l1, l2 = 1 / s1 ** 2, 1 / s2 ** 2
    cs, sn = np.cos(th), np.sin(th)
    return l1 * cs * cs + l2 * sn * sn, (l1 - l2) * cs * sn, l1 * sn * sn + l2 * cs * cs


def _origin(rng, n):
    return 8 * rng.integers(0, 480, n), 8 * rng.integers(0, 270, n)  # quadrants of a 3840 x 2160 frame


def _opacity(rng, n):
    return np.exp(rng.uniform(np.log(0.9 / 255), 0.0, n))


def _pack(a, b, c, o, mx, my, qx, qy):
    return tuple(np.asarray(v, F) for v in (a, b, c, o, mx, my)) + (np.asarray(qx, np.int64), np.asarray(qy, np.int64))


def _random_set():
    rng = np.random.default_rng(20240607)
    n = N_RANDOM
    a, b, c = _conic(rng, n)
    qx, qy = _origin(rng, n)
    mx, my = qx + rng.uniform(-40, 47, n), qy + rng.uniform(-40, 47, n)
    return _pack(a, b, c, _opacity(rng, n), mx, my, qx, qy)


def _adversarial_sets():
    rng = np.random.default_rng(977)
    n = N_ADV
    sets = {}
    # means within 1e-3 px of the rectangle's edges (one coordinate snapped) and corners (both)
    a, b, c = _conic(rng, n)
    qx, qy = _origin(rng, n)
    snap_x = qx + 7 * rng.integers(0, 2, n) + rng.uniform(-1e-3, 1e-3, n)
    snap_y = qy + 7 * rng.integers(0, 2, n) + rng.uniform(-1e-3, 1e-3, n)
    kind = rng.integers(0, 3, n)
    mx = np.where(kind != 1, snap_x, qx + rng.uniform(-40, 47, n))
    my = np.where(kind != 0, snap_y, qy + rng.uniform(-40, 47, n))
    sets["mean_on_edges"] = _pack(a, b, c, _opacity(rng, n), mx, my, qx, qy)
    # the alpha = 1/255 contour within 1e-3 px of a corner pixel centre: the conic is scaled so that the corner
    # has Q = Qt, the contour moved by d px along the ray from the mean, and o = exp(Qt / 2) / 255
    a, b, c = _conic(rng, n)
    qx, qy = _origin(rng, n)
    mx, my = qx + rng.uniform(-40, 47, n), qy + rng.uniform(-40, 47, n)
    px, py = qx + 7 * rng.integers(0, 2, n), qy + 7 * rng.integers(0, 2, n)
    near = rng.integers(0, 2, n) == 1  # half of them: the corner next to the mean, often the only pixel in reach
    px, py = np.where(near, qx + 7 * (mx > qx + 3.5), px), np.where(near, qy + 7 * (my > qy + 3.5), py)
    dx, dy = mx - px, my - py
    r = np.maximum(np.hypot(dx, dy), 1e-2)
    qt = rng.uniform(0.05, 2 * np.log(255.0), n)
    q = a * dx * dx + 2 * b * dx * dy + c * dy * dy
    s = qt / np.maximum(q, 1e-12) * (r / (r + rng.uniform(-1e-3, 1e-3, n))) ** 2
    sets["contour_on_corner"] = _pack(a * s, b * s, c * s, np.minimum(1.0, np.exp(qt / 2) / 255), mx, my, qx, qy)
    # b = 0 and a = c
    a, b, c = _conic(rng, n)
    qx, qy = _origin(rng, n)
    mx, my = qx + rng.uniform(-40, 47, n), qy + rng.uniform(-40, 47, n)
    o = _opacity(rng, n)
    sets["b_zero"] = _pack(a, 0 * b, c, o, mx, my, qx, qy)
    sets["a_equals_c"] = _pack(a, b * 0.999 * a / np.maximum(np.abs(b), np.sqrt(a * c)), a, o, mx, my, qx, qy)
    return sets


def _degenerate_set():
    rng = np.random.default_rng(5)
    n = 4096
    a, b, c = _conic(rng, n)
    qx, qy = _origin(rng, n)
    mx, my = qx + rng.uniform(-40, 47, n), qy + rng.uniform(-40, 47, n)
    o = _opacity(rng, n)
    kind = np.arange(n) % 8
    a = np.select([kind == 0, kind == 1, kind == 2], [0.0, -a, np.nan], a)
    c = np.select([kind == 3, kind == 4], [0.0, -c], c)
    b = np.select([kind == 5, kind == 6], [np.sqrt(np.abs(a * c)) * 1.001, np.inf], b)  # det <= 0
    o = np.where(kind == 7, np.where(np.arange(n) % 16 == 7, 0.0, -o), o)
    return _pack(a, b, c, o, mx, my, qx, qy)


@pytest.fixture(scope="module")
def random_set():
    case = _random_set()
    return case, M.brute_hit64(*case), M.brute_hit32(*case)


PERTURBATIONS = list(itertools.product((-2, 0, 2), repeat=3))


def _assert_covers(name, case, brute, hit, what):
    missed = brute & ~hit
    assert not missed.any(), (name, what, int(missed.sum()), [np.asarray(v)[missed][:3].tolist() for v in case])


def test_random_set_is_informative(random_set):
    case, b64, b32 = random_set
    a, b, c = (case[i].astype(np.float64) for i in range(3))
    lam = np.stack([np.linalg.eigvalsh(np.array([[x, y], [y, z]])) for x, y, z in zip(a[:2000], b[:2000], c[:2000])])
    assert 40.0 < np.sqrt(lam[:, 1] / lam[:, 0]).max() <= 50.5  # axis ratios up to 50:1
    frac = b64.mean()
    assert 0.2 < frac < 0.8, frac  # both outcomes are well represented
    assert (b64 != b32).mean() < 1e-3  # the float32 expression flips only threshold cases


def test_two_edge_test_covers_brute_force_random(random_set):
    case, b64, b32 = random_set
    for ra, rc, lg in PERTURBATIONS:
        hit = M.two_edge_hit(*case, ra_ulp=ra, rc_ulp=rc, log_ulp=lg)
        _assert_covers("random", case, b64, hit, ("f64", ra, rc, lg))
        _assert_covers("random", case, b32, hit, ("f32", ra, rc, lg))


def test_four_edge_test_covers_brute_force_random(random_set):
    case, b64, b32 = random_set
    hit = M.four_edge_hit(*case)
    _assert_covers("random", case, b64, hit, "f64")
    _assert_covers("random", case, b32, hit, "f32")


def test_two_edge_test_is_as_tight_as_four_edge(random_set):
    case, b64, b32 = random_set
    brute = b64 | b32
    false_new = int((M.two_edge_hit(*case) & ~brute).sum())
    false_old = int((M.four_edge_hit(*case) & ~brute).sum())
    print(f"false hits of {len(brute)}: two-edge {false_new}, four-edge {false_old}")
    assert false_old > 100  # the ratio means something
    assert false_new <= 1.02 * false_old, (false_new, false_old)


@pytest.mark.parametrize("name", ["mean_on_edges", "contour_on_corner", "b_zero", "a_equals_c"])
def test_adversarial_sets(name):
    case = _adversarial_sets()[name]
    b64, b32 = M.brute_hit64(*case), M.brute_hit32(*case)
    assert 0.02 < b64.mean() < 0.98, b64.mean()
    if name == "contour_on_corner":  # the set is at the threshold: the two brute-force precisions disagree on some
        assert (b64 != b32).any()
    for ra, rc, lg in PERTURBATIONS:
        hit = M.two_edge_hit(*case, ra_ulp=ra, rc_ulp=rc, log_ulp=lg)
        _assert_covers(name, case, b64, hit, ("f64", ra, rc, lg))
        _assert_covers(name, case, b32, hit, ("f32", ra, rc, lg))
    old = M.four_edge_hit(*case)
    _assert_covers(name, case, b64, old, "four-edge f64")
    _assert_covers(name, case, b32, old, "four-edge f32")


def test_mean_inside_is_a_hit_without_a_special_case():
    rng = np.random.default_rng(11)
    n = 20_000
    a, b, c = _conic(rng, n)
    qx, qy = _origin(rng, n)
    case = _pack(a, b, c, _opacity(rng, n), qx + rng.uniform(0, 7, n), qy + rng.uniform(0, 7, n), qx, qy)
    assert M.two_edge_hit(*case).all()


def test_degenerate_conics_go_to_the_box():
    case = _degenerate_set()
    assert not M.guard_ok(*case[:4]).any()
    assert M.two_edge_hit(*case).all()
    assert M.four_edge_hit(*case).all()
