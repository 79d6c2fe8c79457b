"""TEST INFRASTRUCTURE: the cases of the range-sensor tests (cotix_raycast,
DESIGN.md section 17), the oracle restatement of its semantics over
cotix_oracle.geometry alone, the same semantics in float64 (an independent
check of the restatement) and the ctypes front-end of the host checker
(tests/emu/cotix_raycast_host.cpp), shared by tests/test_raycast_cpu.py and
tests/test_gpu_raycast.py.

A case is a scene maker of tests/raster_cases.py (env -> oracle bodies), a
sensor and a table of ray directions.  The oracle's readings of an env are
computed once per process."""
import collections
import ctypes
import functools
import math
import os
import subprocess

import numpy as np

import raster_cases as RC
from raster_cases import F, G, _p, batch_arrays, part_table  # noqa: F401  (shared with the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
B = 5  # a partial workgroup: not a multiple of the kernel's 4 envs
INF = F(np.inf)
Sensor = collections.namedtuple("Sensor", "body offset follow_angle max_range ignore",
                                defaults=(None, (0.0, 0.0), False, 8.0, ()))
# ids: the hit values envs 0 .. B-1 of the oracle produce between them (exactly)
Case = collections.namedtuple("Case", "make sensor dirs ids")


def fan(n, fov=2.0 * math.pi, start=0.0):
    """f32 [n, 2]: cos / sin, taken in float64, of start + (k + 1/2) fov / n."""
    a = start + (np.arange(n, dtype=np.float64) + 0.5) * (fov / n)
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], 1).astype(F))


# ----------------------------------------------------------------------------
# the oracle: the semantics restated over cotix_oracle.geometry alone
# ----------------------------------------------------------------------------
def _cross(u, v):
    return u[0] * v[1] - v[0] * u[1]  # the form of geometry._edge_vs_edge


def oracle_rays(bodies, sensor, dirs):
    """(dist f32 [R], hit u8 [R]) of one env."""
    world = [(k, p.transform(b.transformer())) for k, b in enumerate(bodies) if k not in sensor.ignore
             for p in b.parts]
    off, rng = (F(sensor.offset[0]), F(sensor.offset[1])), F(sensor.max_range)
    T = None if sensor.body is None else bodies[sensor.body].transformer()
    if T is None:
        o = off
    elif sensor.follow_angle:
        o = T.forward_vector(off)
    else:
        o = G.vadd(off, bodies[sensor.body].position)
    dist, hit = np.zeros(len(dirs), F), np.zeros(len(dirs), np.uint8)
    with np.errstate(all="ignore"):
        for k, (x, y) in enumerate(dirs):
            x, y = F(x), F(y)
            d = (T.cos * x + (-T.sin) * y, T.sin * x + T.cos * y) if sensor.follow_angle else (x, y)
            best, who = INF, 0
            for body, s in world:
                if s.kind == "Circle":
                    m = G.vsub(o, s.position)
                    a, b = G.dot(d, d), G.dot(m, d)
                    q = G.dot(m, m) - s.radius * s.radius
                    sq = np.sqrt(b * b - a * q)
                    t0, t1 = (-b - sq) / a, (-b + sq) / a
                    t = t0 if t0 >= 0 else t1
                    if t >= 0 and t <= rng and t < best:
                        best, who = t, 1 + body
                    continue
                for e0, e1 in s.edges():
                    sv, w = G.vsub(e1, e0), G.vsub(e0, o)
                    c = _cross(d, sv)
                    t, u = _cross(w, sv) / c, _cross(w, d) / c
                    if c != 0 and t >= 0 and t <= rng and u >= 0 and u <= 1 and t < best:
                        best, who = t, 1 + body
            assert isinstance(best, np.float32)
            dist[k], hit[k] = (best, who) if who else (rng, 0)
    return dist, hit


@functools.lru_cache(maxsize=None)
def oracle_env(name, env):
    c = CASES[name]
    return oracle_rays(c.make(env), c.sensor, c.dirs)


def oracle_batch(name, n=B):
    """(dist f32 [n, R], hit u8 [n, R])"""
    r = [oracle_env(name, e) for e in range(n)]
    return np.stack([x[0] for x in r]), np.stack([x[1] for x in r])


def case_envs(name, n=B):
    return [CASES[name].make(e) for e in range(n)]


# ----------------------------------------------------------------------------
# the same semantics in float64 on the same f32 inputs, written without the
# oracle's arithmetic (only the discrete vertex order of a polygon is taken
# from it), with the rays whose answer hangs on a near-degenerate crossing
# marked (test_raycast_cpu.py states the rule)
# ----------------------------------------------------------------------------
def f64_rays(bodies, sensor, dirs):
    """(dist f64 [R], hit [R], fragile bool [R]) of one env."""
    def frame(b):
        px, py, a = float(b.position[0]), float(b.position[1]), float(b.angle)
        return px, py, math.cos(a), math.sin(a)

    nan = float("nan")
    world = []  # (body, "c", r, cx, cy) | (body, "e", [(e0, e1)])
    for k, b in enumerate(bodies):
        if k in sensor.ignore:
            continue
        px, py, c, s = frame(b)
        for p in b.parts:
            if p.kind == "Circle":
                world.append((k, "c", float(p.radius), float(p.position[0]) + px, float(p.position[1]) + py))
                continue
            if p.kind == "AABB":
                lo = (float(p.lower[0]) + px, float(p.lower[1]) + py)
                up = (float(p.upper[0]) + px, float(p.upper[1]) + py)
                v = [up, (up[0], lo[1]), lo, (lo[0], up[1])]
                world.append((k, "e", [(v[i], v[(i + 1) % 4]) for i in range(4)]))
                continue
            v = [(c * float(x) - s * float(y) + px, s * float(x) + c * float(y) + py) for x, y in p.vertices_]
            idx = G.order_clockwise_idx([b.transformer().forward_vector(q) for q in p.vertices_])
            v = [v[i] for i in idx]
            world.append((k, "e", [(v[i], v[i - 1]) for i in range(len(v))]))
    ox, oy, rng = float(F(sensor.offset[0])), float(F(sensor.offset[1])), float(F(sensor.max_range))
    rot = None
    if sensor.body is not None:
        px, py, c, s = frame(bodies[sensor.body])
        if sensor.follow_angle:
            ox, oy, rot = c * ox - s * oy + px, s * ox + c * oy + py, (c, s)
        else:
            ox, oy = ox + px, oy + py
    R = len(dirs)
    dist, hit, fragile = np.zeros(R), np.zeros(R, np.uint8), np.zeros(R, bool)

    def div(a, b):
        if b == 0.0:
            return nan if a == 0.0 or a != a else math.copysign(math.inf, a)
        return a / b

    for k in range(R):
        x, y = float(dirs[k][0]), float(dirs[k][1])
        dx, dy = (rot[0] * x - rot[1] * y, rot[1] * x + rot[0] * y) if rot else (x, y)
        dn = math.hypot(dx, dy)
        best, who = math.inf, 0
        for part in world:
            body = part[0]
            if part[1] == "c":
                _, _, r, cx, cy = part
                mx, my = ox - cx, oy - cy
                a, b, q = dx * dx + dy * dy, mx * dx + my * dy, mx * mx + my * my - r * r
                disc = b * b - a * q
                sq = math.sqrt(disc) if disc >= 0.0 else nan
                t0, t1 = div(-b - sq, a), div(-b + sq, a)
                t = t0 if t0 >= 0 else t1
                for tt in (t0, t1):  # either root near the range's ends, or a grazing ray
                    if -1e-2 <= tt <= rng + 1e-2 and (abs(tt) < 1e-2 or abs(tt - rng) < 1e-2
                                                      or disc < 0.05 * a * r * r):
                        fragile[k] = True
                if t >= 0 and t <= rng and t < best:
                    best, who = t, 1 + body
                continue
            for (e0, e1) in part[2]:
                sx, sy, wx, wy = e1[0] - e0[0], e1[1] - e0[1], e0[0] - ox, e0[1] - oy
                c = dx * sy - sx * dy
                t, u = div(wx * sy - sx * wy, c), div(wx * dy - dx * wy, c)
                if -1e-2 <= t <= rng + 1e-2:
                    if u != u:
                        fragile[k] = True
                    elif abs(t) < 1e-2 or abs(t - rng) < 1e-2:
                        fragile[k] = True
                    elif -0.01 <= u <= 1.01 and (abs(c) < 0.05 * dn * math.hypot(sx, sy) or abs(u) < 0.01
                                                 or abs(u - 1.0) < 0.01):
                        fragile[k] = True
                if c != 0 and t >= 0 and t <= rng and u >= 0 and u <= 1 and t < best:
                    best, who = t, 1 + body
        dist[k], hit[k] = (best, who) if who else (rng, 0)
    return dist, hit, fragile


# ----------------------------------------------------------------------------
# the host checker
# ----------------------------------------------------------------------------
def build_host(*targets):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu"), "-f", "raycast.mk",
                    *["build/" + t for t in (targets or ("libcotix_raycast_host.so",))]], check=True)


@functools.lru_cache(maxsize=None)
def host_lib():
    build_host()
    lib = ctypes.CDLL(os.path.join(HERE, "emu", "build", "libcotix_raycast_host.so"))
    P_, I_ = ctypes.c_void_p, ctypes.c_int
    lib.raycast_host.argtypes = [I_, P_, P_, P_, P_, P_, P_, I_, I_, P_, I_, I_, ctypes.c_uint, P_, I_, P_, P_]
    return lib


def sensor_words(sensor):
    """(ox, oy, max_range) f32, body or -1, follow_angle 0 / 1, the ignore mask."""
    mask = 0
    for b in sensor.ignore:
        mask |= 1 << b
    return np.array([*sensor.offset, sensor.max_range], F), -1 if sensor.body is None else sensor.body, \
        1 if sensor.follow_angle else 0, mask


def host_rays(envs, sensor, dirs, want_hit=True):
    """The host checker's readings of a batch: (dist f32 [B, R], hit u8 [B, R] or None)."""
    (body, kind, nv, goff), _ = part_table(envs[0])
    dyn, geom = batch_arrays(envs)
    n, R = len(envs), len(dirs)
    sw, sb, fa, mask = sensor_words(sensor)
    dirs = np.ascontiguousarray(dirs, F)
    dist = np.full((n, R), -77.0, F)
    hit = np.full((n, R), 0xA5, np.uint8) if want_hit else None
    rc = host_lib().raycast_host(len(body), _p(body), _p(kind), _p(nv), _p(goff), _p(dyn), _p(geom),
                                 0 if geom.ndim == 1 else geom.shape[1], n, _p(sw), sb, fa, mask, _p(dirs), R,
                                 _p(dist), _p(hit))
    assert rc == 0
    return dist, hit


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ----------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------
AXES = np.array([(1, 0), (0, 1), (-1, 0), (0, -1), (4.5, 3), (-4.5, 3), (-4.5, -3), (4.5, -3)], F)
ON_BALL = Sensor(body=4, max_range=5.0, ignore=(4,))
ON_LANDER = Sensor(body=0, follow_angle=True, max_range=6.0, ignore=(0,))
CASES = {
    # cast from the ball: the play area (id 2) answers from inside, with the distance to the touch line
    "robocup_ball": Case(RC.robocup_reset, ON_BALL, fan(16), {0, 2}),
    "robocup_goals": Case(RC.robocup_reset, Sensor(body=4, max_range=6.0, ignore=(0, 1, 4)), fan(32), {0, 3, 4}),
    # a quarter turn around +x from beside the ball: the circle branch
    "robocup_fixed": Case(RC.robocup_reset, Sensor(offset=(-1.0, 0.02), max_range=6.0, ignore=(0, 1)),
                          fan(16, math.pi / 2, -math.pi / 4), {0, 4, 5}),
    # rays parallel to edges, rays through corners (ties), directions that are not unit vectors
    "robocup_axes": Case(RC.robocup_reset, Sensor(max_range=8.0, ignore=(4,)), AXES, None),
    "robocup_2_steps": Case(RC.robocup_stepped, ON_BALL, fan(16), {0, 2}),  # body 0's state is NaN
    "lunar_reset": Case(RC.lunar_reset, ON_LANDER, fan(16), {0, 2, 3, 4}),  # a terrain per env
    # 80 rays: more than one per lane
    "lunar_down": Case(RC.lunar_reset, Sensor(body=0, offset=(0.0, -0.5), follow_angle=True, max_range=6.0,
                                              ignore=(0, 1, 2)), fan(80), {0, 4}),
    "lunar_large_angle": Case(RC.lunar_large_angle, ON_LANDER, fan(16), None),  # sincos32's large-argument path
    "octagons": Case(RC.octagons, Sensor(offset=(0.1, -0.2), max_range=8.0), fan(80), {1, 2}),
    "adversarial": Case(RC.adversarial, Sensor(max_range=8.0), fan(16), {0, 1, 2}),  # NaN / inf vertices
    "one_ray": Case(RC.robocup_reset, ON_BALL, fan(1, start=0.3), None),
    # 60 of the 5 x 16 rays miss: dist == max_range exactly
    "clipped": Case(RC.robocup_reset, ON_BALL._replace(max_range=3.5), fan(16), {0, 2}),
}
