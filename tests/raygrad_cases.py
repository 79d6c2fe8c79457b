"""TEST INFRASTRUCTURE: the cases of the range-sensor gradient tests
(cotix_raycast_backward): the twelve cases of
tests/raycast_cases.py and two of their own, the cotangents, the float64
vector-Jacobian product that judges the f32 expressions, and the ctypes
front-end of the host checker (tests/emu/cotix_raygrad_host.cpp), shared by
tests/test_raygrad_cpu.py and tests/test_gpu_raygrad.py.

The float64 VJP finds each ray's winning feature by the discrete search of
RC.f64_rays (restated here because f64_rays does not return it; the tests hold
the two to each other), writes t of that feature in torch.float64 over leaves
for every body's (px, py, angle) and every local geometry word, and takes
backward of sum(g * t)."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import torch

import raster_cases
import raycast_cases as RC
from raycast_cases import B, F, Case, Sensor, _p, batch_arrays, bits, fan, part_table, sensor_words  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
G, P = RC.G, raster_cases.P

# max |host - float64| / max |float64| over an env's g_dyn (or g_geom) words: 4 x the worst measured over the
# cases, rounded up to one digit.  The worst is 2.64e-4 (robocup_fixed, env 2, g_geom; its g_dyn 2.56e-4): ray 6
# crosses the ball with disc = 4.0e-4 = 0.09 a r^2 -- just clear of the fragility rule's 0.05 -- under b^2 = 1.28,
# so the f32 disc carries 3 * 2^-24 * b^2 / disc = 5.8e-4 of relative error and g_disc = g_sq / (2 sq) half of it.
# Every other case and env stays below 3.3e-5, the edge-only ones below 1.2e-5.
VJP_LIMIT = 2e-3


def dup_vertex(env):
    """A fixed square with its corner (1.5, 1.5) stored twice, seen from inside, and a turned one beside it
    with another corner doubled: equal sort keys, which only the rank's stable order tells apart."""
    inf = float("inf")
    sq = [(1.5, 1.5), (1.5, 1.5), (1.5, -1.5), (-1.5, -1.5), (-1.5, 1.5)]
    tri = [(0.5, 0.4), (-0.5, 0.4), (-0.5, 0.4), (0.0, -0.6)]
    out = [P.Body([G.Polygon(sq, kind="Polygon")], mass=inf, inertia=inf, position=(0.02 * env, -0.01 * env),
                  angle=0.3 + 0.1 * env),
           P.Body([G.Polygon(tri, kind="Polygon")], position=(0.6, 0.1 + 0.05 * env), angle=-0.7 + 0.2 * env)]
    for b in out:
        assert len({tuple(map(float, v)) for v in b.parts[0].vertices_}) == len(b.parts[0].vertices_) - 1
    return out


CASES = dict(RC.CASES)
# cast from the ball with nothing masked: every ray leaves the ball's own circle (root t1).  The four axis
# directions, four times over: d . d is exactly 1, which is what makes d dist / d r exactly 1 in f32 (a fan's
# cos^2 + sin^2 is 1 only to an ulp, and d dist / d r is 1 / |d|)
CASES["own_body"] = Case(raster_cases.robocup_reset, Sensor(body=4, max_range=5.0, ignore=()),
                         np.ascontiguousarray(np.tile(RC.AXES[:4], (4, 1))), {5})
CASES["dup_vertex"] = Case(dup_vertex, Sensor(offset=(0.1, -0.2), max_range=8.0), fan(32), {1, 2})
NEW = ("own_body", "dup_vertex")


def envs_of(name, n=B):
    return [CASES[name].make(e) for e in range(n)]


@functools.lru_cache(maxsize=None)
def f64_batch(name):
    """(dist f64 [B, R], hit [B, R], fragile bool [B, R]) of RC.f64_rays."""
    c = CASES[name]
    r = [RC.f64_rays(bodies, c.sensor, c.dirs) for bodies in envs_of(name)]
    return tuple(np.stack([x[k] for x in r]) for k in range(3))


@functools.lru_cache(maxsize=None)
def cotangent(name, seed=0):
    """f32 [B, R], uniform in [-1, 1]; exactly 0 on every ray RC.f64_rays marks fragile."""
    c = CASES[name]
    g = np.random.default_rng(seed).uniform(-1.0, 1.0, (B, len(c.dirs))).astype(F)
    g[f64_batch(name)[2]] = 0.0
    g.setflags(write=False)
    return g


# ----------------------------------------------------------------------------
# the float64 VJP
# ----------------------------------------------------------------------------
def f64_vjp(bodies, sensor, dirs, g):
    """(t f64 [R], hit [R], g_pose f64 [nb, 3], g_row f64 [GW]) of one env; t is max_range on a miss.  Rays
    with g == 0 and misses are left out of the objective."""
    T = torch.float64
    nb = len(bodies)
    pose = torch.tensor([[float(b.position[0]), float(b.position[1]), float(b.angle)] for b in bodies], dtype=T,
                        requires_grad=True)
    row = torch.tensor(raster_cases.geometry_row(bodies).astype(np.float64), dtype=T, requires_grad=True)
    (pbody, pkind, pnv, pgoff), _ = part_table(bodies)
    cs, sn = torch.cos(pose[:, 2]), torch.sin(pose[:, 2])

    def fwd(k, x, y):
        return cs[k] * x - sn[k] * y + pose[k, 0], sn[k] * x + cs[k] * y + pose[k, 1]

    world, part = [], 0  # (body, "c", r, cx, cy) | (body, "e", [(e0, e1)]), tensors
    for k, b in enumerate(bodies):
        for p in b.parts:
            o_ = int(pgoff[part])
            part += 1
            if k in sensor.ignore:
                continue
            if p.kind == "Circle":
                world.append((k, "c", row[o_], row[o_ + 1] + pose[k, 0], row[o_ + 2] + pose[k, 1]))
            elif p.kind == "AABB":
                lo = (row[o_] + pose[k, 0], row[o_ + 1] + pose[k, 1])
                up = (row[o_ + 2] + pose[k, 0], row[o_ + 3] + pose[k, 1])
                v = [up, (up[0], lo[1]), lo, (lo[0], up[1])]
                world.append((k, "e", [(v[i], v[(i + 1) % 4]) for i in range(4)]))
            else:
                n = len(p.vertices_)
                v = [fwd(k, row[o_ + 2 * j], row[o_ + 2 * j + 1]) for j in range(n)]
                idx = G.order_clockwise_idx([b.transformer().forward_vector(q) for q in p.vertices_])
                v = [v[i] for i in idx]
                world.append((k, "e", [(v[i], v[i - 1]) for i in range(n)]))
    ox, oy, rng = float(F(sensor.offset[0])), float(F(sensor.offset[1])), float(F(sensor.max_range))
    o, sb = (torch.tensor(ox, dtype=T), torch.tensor(oy, dtype=T)), sensor.body
    if sb is not None:
        o = fwd(sb, ox, oy) if sensor.follow_angle else (ox + pose[sb, 0], oy + pose[sb, 1])

    def fl(v):
        return float(v.detach()) if torch.is_tensor(v) else float(v)

    plain = [(w[0], w[1], fl(w[2]), fl(w[3]), fl(w[4])) if w[1] == "c" else
             (w[0], w[1], [((fl(a[0]), fl(a[1])), (fl(b_[0]), fl(b_[1]))) for a, b_ in w[2]])
             for w in world]
    pox, poy = fl(o[0]), fl(o[1])
    prot = (fl(cs[sb]), fl(sn[sb])) if sb is not None and sensor.follow_angle else None
    nan = float("nan")

    def div(a, b_):
        if b_ == 0.0:
            return nan if a == 0.0 or a != a else math.copysign(math.inf, a)
        return a / b_

    R = len(dirs)
    ts, hits, terms = np.full(R, rng), np.zeros(R, np.uint8), []
    for r in range(R):
        x, y = float(dirs[r][0]), float(dirs[r][1])
        dx, dy = (prot[0] * x - prot[1] * y, prot[1] * x + prot[0] * y) if prot else (x, y)
        best, win = math.inf, None
        for pi, w in enumerate(plain):  # the discrete search of RC.f64_rays
            if w[1] == "c":
                _, _, rr, cx, cy = w
                mx, my = pox - cx, poy - cy
                a, b_, q = dx * dx + dy * dy, mx * dx + my * dy, mx * mx + my * my - rr * rr
                disc = b_ * b_ - a * q
                sq = math.sqrt(disc) if disc >= 0.0 else nan
                t0, t1 = div(-b_ - sq, a), div(-b_ + sq, a)
                t, root = (t0, 0) if t0 >= 0 else (t1, 1)
                if t >= 0 and t <= rng and t < best:
                    best, win = t, (pi, root)
                continue
            for ei, (e0, e1) in enumerate(w[2]):
                sx, sy, wx, wy = e1[0] - e0[0], e1[1] - e0[1], e0[0] - pox, e0[1] - poy
                c = dx * sy - sx * dy
                t, u = div(wx * sy - sx * wy, c), div(wx * dy - dx * wy, c)
                if c != 0 and t >= 0 and t <= rng and u >= 0 and u <= 1 and t < best:
                    best, win = t, (pi, ei)
        if win is None:
            continue
        w = world[win[0]]
        d = (cs[sb] * x - sn[sb] * y, sn[sb] * x + cs[sb] * y) if prot else (x, y)
        if w[1] == "c":
            _, _, rr, cx, cy = w
            mx, my = o[0] - cx, o[1] - cy
            a, b_, q = d[0] * d[0] + d[1] * d[1], mx * d[0] + my * d[1], mx * mx + my * my - rr * rr
            sq = torch.sqrt(b_ * b_ - a * q)
            t = (-b_ - sq) / a if win[1] == 0 else (-b_ + sq) / a
        else:
            e0, e1 = w[2][win[1]]
            sx, sy, wx, wy = e1[0] - e0[0], e1[1] - e0[1], e0[0] - o[0], e0[1] - o[1]
            t = (wx * sy - sx * wy) / (d[0] * sy - sx * d[1])
        ts[r], hits[r] = fl(t), 1 + w[0]
        if g[r] != 0:
            terms.append(float(g[r]) * t)
    if not terms:
        return ts, hits, np.zeros((nb, 3)), np.zeros(len(row))
    torch.stack(terms).sum().backward()
    return ts, hits, pose.grad.numpy(), row.grad.numpy()


@functools.lru_cache(maxsize=None)
def f64_vjp_batch(name, seed=0):
    """(t [B, R], hit [B, R], g_pose [B, nb, 3], g_row [B, GW]) with cotangent(name, seed)."""
    c, g = CASES[name], cotangent(name, seed)
    r = [f64_vjp(bodies, c.sensor, c.dirs, g[e]) for e, bodies in enumerate(envs_of(name))]
    return tuple(np.stack([x[k] for x in r]) for k in range(4))


# ----------------------------------------------------------------------------
# the host checker
# ----------------------------------------------------------------------------
def build_host(*targets):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu"), "-f", "raygrad.mk",
                    *["build/" + t for t in (targets or ("libcotix_raygrad_host.so",))]], check=True)


def load_host():
    """The library as __graft_entry__.build_checkers left it: no build here (the -m gpu tests fail without it)."""
    lib = ctypes.CDLL(os.path.join(HERE, "emu", "build", "libcotix_raygrad_host.so"))
    P_, I_, U_ = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
    lib.raygrad_host.argtypes = [I_, P_, P_, P_, P_, P_, P_, I_, I_, P_, I_, I_, U_, P_, I_, I_, I_, P_, P_, P_]
    lib.raywin_host.argtypes = [I_, P_, P_, P_, P_, P_, P_, I_, I_, P_, I_, I_, U_, P_, I_, P_, P_, P_, P_]
    lib.rayrank_host.argtypes = [I_, I_, P_, P_, P_, P_]
    return lib


@functools.lru_cache(maxsize=None)
def host_lib():
    build_host()
    return load_host()


SENTINEL = F(-77.0)


def host_vjp(envs, sensor, dirs, g, want_dyn=True, want_geom=True, lib=None):
    """The host checker's (g_dyn f32 [nb, 6, B] | None, g_geom f32 [GW, B] | None); the outputs start as SENTINEL."""
    (body, kind, nv, goff), gw = part_table(envs[0])
    dyn, geom = batch_arrays(envs)
    n, R = len(envs), len(dirs)
    sw, sb, fa, mask = sensor_words(sensor)
    dirs, g = np.ascontiguousarray(dirs, F), np.ascontiguousarray(g, F)
    assert g.shape == (n, R)
    gd = np.full(dyn.shape, SENTINEL, F) if want_dyn else None
    gg = np.full((gw, n), SENTINEL, F) if want_geom else None
    rc = (lib or host_lib()).raygrad_host(len(body), _p(body), _p(kind), _p(nv), _p(goff), _p(dyn), _p(geom),
                                          0 if geom.ndim == 1 else geom.shape[1], n, _p(sw), sb, fa, mask, _p(dirs),
                                          R, dyn.shape[0], gw, _p(g), _p(gd), _p(gg))
    assert rc == 0
    return gd, gg


def host_win(envs, sensor, dirs):
    """ray_cast_win on a batch: (dist f32, hit u8, part i32, feat i32), [B, R] each."""
    (body, kind, nv, goff), _ = part_table(envs[0])
    dyn, geom = batch_arrays(envs)
    n, R = len(envs), len(dirs)
    sw, sb, fa, mask = sensor_words(sensor)
    dirs = np.ascontiguousarray(dirs, F)
    dist, hit = np.full((n, R), SENTINEL, F), np.full((n, R), 0xA5, np.uint8)
    part, feat = np.full((n, R), -9, np.int32), np.full((n, R), -9, np.int32)
    rc = host_lib().raywin_host(len(body), _p(body), _p(kind), _p(nv), _p(goff), _p(dyn), _p(geom),
                                0 if geom.ndim == 1 else geom.shape[1], n, _p(sw), sb, fa, mask, _p(dirs), R,
                                _p(dist), _p(hit), _p(part), _p(feat))
    assert rc == 0
    return dist, hit, part, feat


def host_rank(xy):
    """xy f32 [n, nv, 2] -> (cx::order_clockwise's vertices, the vertices gathered by poly_rank, the ranks)."""
    xy = np.ascontiguousarray(xy, F)
    n, nv, _ = xy.shape
    srt, gat, rank = np.zeros_like(xy), np.full_like(xy, SENTINEL), np.zeros((n, nv), np.int32)
    assert host_lib().rayrank_host(n, nv, _p(xy), _p(srt), _p(gat), _p(rank)) == 0
    return srt, gat, rank


def pose_rows(g_dyn):
    """[nb, 6, B] -> the pose words [B, nb, 3] (rows 0, 1 and 4)."""
    return np.ascontiguousarray(g_dyn[:, [0, 1, 4], :].transpose(2, 0, 1))


def ratio(got, want):
    """max |got - want| / max |want| in float64; inf when they differ in a NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return math.inf
    den = np.nanmax(np.abs(want)) if want.size else 0.0
    num = np.nanmax(np.abs(got - want)) if want.size else 0.0
    if den == 0.0 or np.isnan(den):
        return 0.0 if (num == 0.0 or np.isnan(num)) else math.inf
    return float(num / den)
