"""TEST INFRASTRUCTURE: the inputs of the sin/cos/atan2 accuracy tests
(tests/test_transcendentals_cpu.py, tests/test_gpu_transcendentals.py), built
once per process and deterministic: no test changes them.

pi is held as a Python integer (Machin's formula, 260 bits), so the float32
nearest a multiple of pi/2 is found without any float32 arithmetic."""
from fractions import Fraction

import numpy as np

F = np.float32
FLT_MAX = F(np.finfo(np.float32).max)
SEAM = F(8192.0)  # sincos32: three-constant reduction up to here, the exact one beyond
SINCOS_TOL = 2.0 ** -23  # one ulp of 1.0, the coarsest spacing of the results
UNIT_TOL = 2.0 ** -22  # |s^2 + c^2 - 1|

_PI_BITS = 260


def _arctan_inv(n, bits):
    """atan(1/n) * 2**bits, truncated (alternating series in integers)."""
    x = (1 << bits) // n
    n2, total, k, sign = n * n, 0, 1, 1
    while x:
        total += sign * (x // k)
        x //= n2
        k += 2
        sign = -sign
    return total


PI_INT = 4 * (4 * _arctan_inv(5, _PI_BITS + 16) - _arctan_inv(239, _PI_BITS + 16)) >> 16  # pi * 2**260, truncated
HALF_PI = Fraction(PI_INT, 1 << (_PI_BITS + 1))


def nearest_f32(k):
    """The float32 nearest k * pi/2 (through float64: at most one ulp off the
    nearest, and every use takes the two neighbours as well)."""
    return F(float(k * HALF_PI))


def with_neighbours(v):
    v = np.asarray(v, F)
    return np.concatenate([v, np.nextafter(v, F(np.inf)), np.nextafter(v, F(-np.inf))])


def edge_specials():
    """The specials of tests/test_emu_cpu.py _edge_floats."""
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-38, np.pi, -np.pi, np.pi / 2,
                     -np.pi / 2, np.pi / 4, 3 * np.pi / 4, 1e4, -1e4, 0.41421356, 0.41421357, 1.0, -1.0], F)


def _probes():
    rng = np.random.default_rng(20240)
    out = [edge_specials()]
    for e in range(-126, 128):  # every binade: 64 random floats of both signs
        bits = (np.uint32(e + 127) << np.uint32(23)) | rng.integers(0, 1 << 23, 64, dtype=np.uint32)
        bits |= rng.integers(0, 2, 64, dtype=np.uint32) << np.uint32(31)
        out.append(bits.view(F))
        if e >= 0:  # ... and the multiple of pi/2 nearest 2^e
            k = round(Fraction(1 << e) / HALF_PI)
            v = with_neighbours([nearest_f32(k)])
            out.append(v[np.isfinite(v)])
    ks = list(range(0, 5401)) + list(range(20000, 20101))  # dense across the seam (k = 5215 | 5216)
    m = with_neighbours([nearest_f32(k) for k in ks])
    out += [m, -m]
    out.append(with_neighbours([SEAM, -SEAM]))
    dense = np.linspace(6.5e6, 6.7e6, 2001).astype(F)  # where the parent's rounding trick stops rounding
    out += [dense, -dense[::4]]
    big = nearest_f32(1 << 31)  # 2^31 * pi/2: (int)k was undefined from here on
    ladder = [big]
    for _ in range(4):
        ladder.append(np.nextafter(ladder[-1], F(np.inf)))
    for _ in range(4):
        ladder.insert(0, np.nextafter(ladder[0], F(-np.inf)))
    out += [np.array(ladder, F), -np.array(ladder, F)]
    out.append(np.array([FLT_MAX, -FLT_MAX, np.nextafter(FLT_MAX, F(0)), 3.0e4, 1.0e6, 7.0e6, 1.0e7, 4.0e9, 1.0e20], F))
    return np.ascontiguousarray(np.concatenate(out).astype(F))


PROBES = _probes()
PROBES.setflags(write=False)


def atan2_pairs(n=20000, seed=5):
    """(y, x) with exponents drawn from -149 .. 127 (subnormals included),
    both signs; as many of comparable size (N(0, 10), where neither ratio is
    tiny and the result is no near copy of it) and pairs whose ratio lies
    next to atan01's breakpoints tan(pi/8), 0.6 and 1; then the signed
    zeros, the axes, and ratios that underflow and whose inverse would
    overflow."""
    rng = np.random.default_rng(seed)

    def draw():
        e = rng.integers(-149, 128, n)
        v = np.ldexp(rng.uniform(1.0, 2.0, n), e).astype(F)  # e < -126: a subnormal (rounded to its grid)
        return np.where(rng.integers(0, 2, n) == 1, -v, v).astype(F)

    y, x = draw(), draw()
    cy, cx = (rng.normal(size=n) * 10).astype(F), (rng.normal(size=n) * 10).astype(F)
    bx = np.ldexp(rng.uniform(1.0, 2.0, n // 4), rng.integers(-20, 21, n // 4))
    bt = rng.choice([0.4142135623730950, 0.6, 1.0], n // 4) + rng.uniform(-2e-3, 2e-3, n // 4)
    by, bx = (bx * bt).astype(F), bx.astype(F)
    flip = rng.integers(0, 2, n // 4) == 1  # either argument the larger, every quadrant
    by, bx = np.where(flip, bx, by), np.where(flip, by, bx)
    by, bx = by * rng.choice([-1, 1], n // 4).astype(F), bx * rng.choice([-1, 1], n // 4).astype(F)
    y, x = np.concatenate([y, cy, by]).astype(F), np.concatenate([x, cx, bx]).astype(F)
    tiny, huge, mn = F(1e-45), FLT_MAX, F(np.finfo(np.float32).tiny)
    ax = [(0.0, 1.0), (-0.0, 1.0), (0.0, -1.0), (-0.0, -1.0), (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0),
          (1.0, 0.0), (-1.0, 0.0), (1.0, -0.0), (-1.0, -0.0), (tiny, 0.0), (-tiny, -0.0), (0.0, tiny), (-0.0, -tiny)]
    for a, b in [(tiny, huge), (mn, huge), (tiny, 1.0), (mn, 1.0), (1.0, huge), (tiny, tiny), (huge, huge),
                 (F(3e-39), F(2e-39)), (F(1e-30), F(1e30)), (mn, F(4.0))]:
        for sa in (1, -1):
            for sb in (1, -1):
                ax += [(sa * a, sb * b), (sb * b, sa * a)]
    ey = np.array([p[0] for p in ax], F)
    ex = np.array([p[1] for p in ax], F)
    return np.ascontiguousarray(np.concatenate([y, ey])), np.ascontiguousarray(np.concatenate([x, ex]))


def atan2_grid(n=200, seed=9):
    """n x n grid of edge floats (the specials, N(0, 3), U(-1e3, 1e3), and
    the extremes of the exponent range)."""
    rng = np.random.default_rng(seed)
    k = (n - 20 - 8) // 2
    v = np.concatenate([edge_specials(), np.array([FLT_MAX, -FLT_MAX, 1e-38, -1e-38, 1e30, -1e30, 1e-30, -1e-30], F),
                        rng.normal(0, 3, k).astype(F), rng.uniform(-1e3, 1e3, n - 28 - k).astype(F)])
    yy, xx = np.meshgrid(v, v)
    return np.ascontiguousarray(yy.ravel()), np.ascontiguousarray(xx.ravel())


# ---------------------------------------------------------------------------
# scenes (oracle bodies) of the device-path tests
# ---------------------------------------------------------------------------
def probe_triangle_bodies():
    """One body at the origin whose only part is the triangle (0,0), (1,0),
    (0,1): the render path's world vertices are (0,0), (c, s) and (-s, c) of
    the body's angle -- c * 1 + (-s) * 0 and its like add only signed zeros."""
    from cotix_oracle import geometry as G
    from cotix_oracle import physics as P
    return [P.Body([G.Polygon([(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)], kind="Polygon3")], mass=1.0, inertia=1.0)]


def probe_dyn(x):
    dyn = np.zeros((1, 6, x.size), F)
    dyn[0, 4, :] = x
    return dyn


def sincos_from_triangle(prims):
    """(sin, cos) f32 [B] out of the rendered probe triangle, prims f32
    [B, 3, 4] = edges (v_k, v_{k-1}) in the world's clockwise order: the vertex
    after the origin is (c, s), the one after it (-s, c); both must tell the
    same, up to the sign of a zero.  A NaN row gives (NaN, NaN)."""
    v = np.asarray(prims, F)[:, :, :2]
    B = v.shape[0]
    nan = np.isnan(v).any(axis=(1, 2))
    zero = (v[:, :, 0] == 0) & (v[:, :, 1] == 0)
    assert np.array_equal(zero.sum(1)[~nan], np.ones((~nan).sum(), int)), "one vertex at the origin per probe"
    z = np.argmax(zero, 1)
    a = v[np.arange(B), (z + 1) % 3]
    b = v[np.arange(B), (z + 2) % 3]
    ok = ((b[:, 0] + F(0)).view(np.uint32) == (-a[:, 1] + F(0)).view(np.uint32)) & \
         ((b[:, 1] + F(0)).view(np.uint32) == (a[:, 0] + F(0)).view(np.uint32))
    assert ok[~nan].all(), "the triangle's two moving vertices disagree"
    s, c = a[:, 1].copy(), a[:, 0].copy()
    s[nan], c[nan] = np.nan, np.nan
    return s, c


LARGE_ANGLES = np.array([8191.9, 8192.1, 3.0e4, 1.0e6, 7.0e6, 1.0e7, 4.0e9, 1.0e20], F)


def large_angle_case(scene, B=16):
    """(bodies, dyn f32 [nb, 6, B], keys u32 [B, 2], dynamic body indices) of
    the fused-kernel test: every finite-mass body starts at one of
    LARGE_ANGLES (envs B/2 .. at their negatives), the bodies of one env at
    different ones; those next to the 8192 seam spin towards it at 3 rad/s,
    across it within the first 7 steps."""
    import grad_cases as GC
    import scene_cases
    bodies = GC.poly_box_bodies() if scene == "poly_box" else scene_cases.mixed_scene(True)
    dynamic = [i for i, b in enumerate(bodies) if np.isfinite(b.mass)]
    base = np.array([b.dyn() for b in bodies], F)
    dyn = np.ascontiguousarray(np.repeat(base[:, :, None], B, axis=2))
    spin = np.array([-1.0, 0.5, 2.0, -0.25, 4.0, -8.0], F)
    for e in range(B):
        sign = F(1.0) if e < B // 2 else F(-1.0)
        for q, b in enumerate(dynamic):
            k = (e + q) % LARGE_ANGLES.size
            dyn[b, 4, e] = sign * LARGE_ANGLES[k]
            dyn[b, 5, e] = sign * F(3.0) if k == 0 else (sign * F(-3.0) if k == 1 else spin[(e + 2 * q) % spin.size])
    keys = np.ascontiguousarray(np.stack([np.arange(B) + 11, np.arange(B) * 7 + 2], 1).astype(np.uint32))
    return bodies, dyn, keys, dynamic


def local_edge_lengths(part):
    v = np.array(part.vertices_, np.float64)
    return np.sort(np.linalg.norm(v - np.roll(v, 1, axis=0), axis=1))


def rendered_edge_lengths(prims, off, n):
    """Sorted float64 lengths [B, n] of one polygon part's rendered edges."""
    p = np.asarray(prims, np.float64)[:, off:off + n]
    return np.sort(np.hypot(p[:, :, 0] - p[:, :, 2], p[:, :, 1] - p[:, :, 3]), axis=1)


def polygon_part_offsets(bodies):
    """[(body, part, first primitive, n)] of the polygon parts in the render
    layout (circle 1, AABB 4, polygon n primitives, parts in scene order)."""
    out, off = [], 0
    for i, b in enumerate(bodies):
        for p in b.parts:
            n = 1 if p.kind == "Circle" else (4 if p.kind == "AABB" else len(p.vertices_))
            if p.kind.startswith("Polygon"):
                out.append((i, p, off, n))
            off += n
    return out


OCW_MIN_GAP = 1e-3


def clockwise_cases(nv, count=200, seed=0):
    """Polygons f32 [count, nv, 2] for order_clockwise, in shuffled order,
    and the order (indices) a float64 arctan2 about the float64 mean of the
    same float32 vertices gives.  Scale 2^e, e = -60 .. 60; the mean lies up
    to 16 scales off the origin (every coordinate of one sign), the vertices
    0.5 .. 2 scales around it, some within 2e-3 rad of an axis.  Every angular
    gap, the one across the +-pi cut included, exceeds OCW_MIN_GAP = 1e-3: the
    float32 mean is off by at most about nv * 2^-24 * 16 scales, 1.6e-5 rad
    seen from a vertex 0.5 scales away, and atan2_32's own 2 ulp are 5e-7, so
    the float64 order is the only right answer."""
    rng = np.random.default_rng(1000 * nv + seed)
    out, order = [], []
    while len(out) < count:
        e = int(rng.integers(-60, 61))
        th = np.sort(rng.uniform(-np.pi, np.pi, nv))
        near = rng.integers(0, nv)  # one vertex next to an axis
        th[near] = rng.choice([0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi]) + rng.choice([-1, 1]) * 2e-3
        th = (th + np.pi) % (2 * np.pi) - np.pi
        r = rng.uniform(0.5, 2.0, nv)
        c = rng.uniform(-16, 16, 2) if len(out) % 4 else np.zeros(2)
        v = np.ldexp(np.stack([c[0] + r * np.cos(th), c[1] + r * np.sin(th)], 1), e).astype(F)
        v = v[rng.permutation(nv)]
        v64 = v.astype(np.float64)
        d = v64 - v64.mean(0)
        a = np.arctan2(d[:, 1], d[:, 0])
        s = np.sort(a)
        gaps = np.concatenate([np.diff(s), [s[0] + np.pi, np.pi - s[-1]]])
        if gaps.min() <= OCW_MIN_GAP:
            continue
        out.append(v)
        order.append(np.argsort(a, kind="stable"))
    return np.ascontiguousarray(np.stack(out)), np.stack(order)


def large_angle_grad_case(B=4, T=8):
    """grad_cases.poly_box_case with the box and the hexagon started at
    angles 3.0e4 and 1.0e7 (and their negatives, swapped, in the odd envs):
    the rollout gradients at that case's own tolerance."""
    import grad_cases as GC
    case = GC.poly_box_case(B, T, seed=3)
    for e in range(B):
        sign = F(1.0) if e % 4 < 2 else F(-1.0)
        a = (F(3.0e4), F(1.0e7)) if e % 2 == 0 else (F(1.0e7), F(3.0e4))
        case["S0"][e, 2, 4], case["S0"][e, 3, 4] = sign * a[0], sign * a[1]
    case["name"] = "poly_box_large_angle"
    return case
