"""TEST INFRASTRUCTURE: the cases of the pixel-observation tests
(cotix_rasterize), the oracle restatement of its
semantics, and the ctypes front-end of the host checker
(tests/emu/cotix_raster_host.cpp), shared by tests/test_raster_cpu.py and
tests/test_gpu_raster.py.

A case is a function env -> oracle bodies (env 0 is the state the case is
named after; envs >= 1 differ by perturbed state or PRNG keys), an image size
and a camera.  The oracle image of an env is computed once per process."""
import collections
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "emu")):
    if p not in sys.path:
        sys.path.insert(0, p)

from cotix_oracle import geometry as G  # noqa: E402
from cotix_oracle import physics as P  # noqa: E402
from cotix_oracle import prng  # noqa: E402

F = np.float32
Cam = collections.namedtuple("Cam", "center half_extent follow_body follow_angle", defaults=((0.0, 0.0), (8.0, 6.0),
                                                                                             None, False))
Case = collections.namedtuple("Case", "make W H cam ids")  # ids: the ids env 0's oracle image must hold (exactly)
KIND = {"Circle": 0, "AABB": 1}  # else polygon: 2 (cx::KIND_*)


# ----------------------------------------------------------------------------
# the oracle: the semantics restated over cotix_oracle.geometry alone
# ----------------------------------------------------------------------------
def oracle_image(bodies, W, H, cam):
    """(ids u8 [H, W], cover u8 [H, W]: how many bodies contain the pixel)."""
    world = [(k, p.transform(b.transformer())) for k, b in enumerate(bodies) for p in b.parts]
    fb = cam.follow_body
    T = None if fb is None else bodies[fb].transformer()
    cx, cy, hw, hh = F(cam.center[0]), F(cam.center[1]), F(cam.half_extent[0]), F(cam.half_extent[1])
    ids, cover = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    for j in range(H):
        v = F(H - (2 * j + 1)) / F(H)
        for i in range(W):
            u = F(2 * i + 1 - W) / F(W)
            loc = (cx + u * hw, cy + v * hh)
            if T is None:
                p = loc
            elif cam.follow_angle:
                p = T.forward_vector(loc)
            else:
                p = G.vadd(loc, bodies[fb].position)
            hit = [k for k, s in world if s.contains(p)]
            if hit:
                ids[j, i], cover[j, i] = 1 + hit[-1], len(set(hit))
    return ids, cover


@functools.lru_cache(maxsize=None)
def oracle_env(name, env):
    c = CASES[name]
    return oracle_image(c.make(env), c.W, c.H, c.cam)


def oracle_batch(name, B):
    return np.stack([oracle_env(name, e)[0] for e in range(B)])


# ----------------------------------------------------------------------------
# plain arrays of a batch of envs (the host checker's and the library's inputs)
# ----------------------------------------------------------------------------
def part_table(bodies):
    """body, kind, nv, goff (i32 [np] each) and the scene's geometry words."""
    body, kind, nv, goff, off = [], [], [], [], 0
    for k, b in enumerate(bodies):
        for p in b.parts:
            body.append(k)
            kind.append(KIND.get(p.kind, 2))
            n = len(p.vertices_) if kind[-1] == 2 else 0
            nv.append(n)
            goff.append(off)
            off += 2 * n if kind[-1] == 2 else 4
    return tuple(np.array(x, np.int32) for x in (body, kind, nv, goff)), off


def geometry_row(bodies):
    row = []
    for b in bodies:
        for p in b.parts:
            if p.kind == "Circle":
                row += [p.radius, p.position[0], p.position[1], 0.0]
            elif p.kind == "AABB":
                row += [*p.lower, *p.upper]
            else:
                row += [c for v in p.vertices_ for c in v]
    return np.array(row, F)


def batch_arrays(envs):
    """dyn f32 [nb, 6, B]; geom f32 [G] when every env has the same geometry, else [B, G]."""
    dyn = np.ascontiguousarray(np.array([[b.dyn() for b in bodies] for bodies in envs], F).transpose(1, 2, 0))
    rows = np.stack([geometry_row(bodies) for bodies in envs])
    same = all(np.array_equal(rows[0].view(np.uint32), r.view(np.uint32)) for r in rows)
    return dyn, np.ascontiguousarray(rows[0] if same else rows)


def case_envs(name, B):
    return [CASES[name].make(e) for e in range(B)]


# ----------------------------------------------------------------------------
# the host checker
# ----------------------------------------------------------------------------
def build_host(*targets):
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu"), "-f", "raster.mk",
                    *["build/" + t for t in (targets or ("libcotix_raster_host.so",))]], check=True)


@functools.lru_cache(maxsize=None)
def host_lib():
    build_host()
    lib = ctypes.CDLL(os.path.join(HERE, "emu", "build", "libcotix_raster_host.so"))
    P_, I_ = ctypes.c_void_p, ctypes.c_int
    lib.raster_host.argtypes = [I_, P_, P_, P_, P_, P_, P_, I_, I_, P_, I_, I_, I_, I_, I_, P_, P_]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def cam_words(cam):
    return np.array([*cam.center, *cam.half_extent], F), -1 if cam.follow_body is None else cam.follow_body, \
        1 if cam.follow_angle else 0


def host_image(envs, W, H, cam, palette=None):
    """The host checker's image of a batch: u8 [B, H, W], or [B, 3, H, W] with a palette (u8 [nb + 1, 3])."""
    (body, kind, nv, goff), _ = part_table(envs[0])
    dyn, geom = batch_arrays(envs)
    B = len(envs)
    cw, fb, fa = cam_words(cam)
    pal = None if palette is None else np.ascontiguousarray(palette, np.uint8)
    out = np.full((B, H, W) if pal is None else (B, 3, H, W), 0xA5, np.uint8)
    rc = host_lib().raster_host(len(body), _p(body), _p(kind), _p(nv), _p(goff), _p(dyn), _p(geom),
                                0 if geom.ndim == 1 else geom.shape[1], B, _p(cw), fb, fa, W, H,
                                1 if pal is None else 3, _p(pal), _p(out))
    assert rc == 0
    return out


# ----------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------
def _nudged(bodies, env):
    """env >= 1: every body moved by a few centimetres (env 0: as given)."""
    for k, b in enumerate(bodies):
        b.position = (b.position[0] + F(0.013 * env * (k + 1)), b.position[1] - F(0.007 * env * (k + 2)))
    return bodies


def robocup_reset(env):
    return _nudged(P.robocup_bodies(), env)


@functools.lru_cache(maxsize=None)
def _robocup_stepped(env):
    bodies, key, d0 = P.robocup_bodies(), prng.PRNGKey(env), prng.gjk_initial_direction()
    for _ in range(2):
        bodies, key = P.robocup_step(bodies, key, d0, G.ErrorFlag())
    return bodies


def robocup_stepped(env):
    return P.clone_bodies(_robocup_stepped(env))


def lunar_reset(env):
    return P.lunar_lander_bodies(prng.PRNGKey(env))  # a terrain per env: per-env geometry rows


@functools.lru_cache(maxsize=None)
def _lunar_stepped(env):
    bodies, key, d0 = P.lunar_lander_bodies(prng.PRNGKey(env)), prng.PRNGKey(env), prng.gjk_initial_direction()
    for _ in range(5):
        bodies, key = P.lunar_lander_step(bodies, key, d0, G.ErrorFlag())
    return bodies


def lunar_stepped(env):
    return P.clone_bodies(_lunar_stepped(env))


def lunar_large_angle(env):
    bodies = lunar_stepped(env)
    bodies[0].angle = F(1e5 + 3.0 * env)  # the large-argument path of sincos32 (|x| > 8192)
    return bodies


def octagons(env):
    import scene_cases
    return _nudged(scene_cases.octagon_row(4), env)


@functools.lru_cache(maxsize=None)
def _adversarial_pairs():
    """Pairs of the broadphase tests' "nonfinite" set (a NaN or inf vertex in
    one polygon) whose finite vertices lie inside the default window."""
    import bp_cases
    A, B = bp_cases.gen_set("nonfinite", 4, 6, 96, 36)
    keep = []
    for a, b in zip(A, B):
        fin = np.concatenate([a, b])
        fin = fin[np.isfinite(fin).all(1)]
        whole = [x for x in (a, b) if np.isfinite(x).all()]  # the pair's polygon without the bad vertex
        if np.abs(fin).max() < 8.0 and whole and np.ptp(whole[0], 0).min() > 1.2:  # some pixel pitches wide
            keep.append((a, b))
    return keep


def adversarial(env):
    a, b = _adversarial_pairs()[env]
    inf = float("inf")
    return [P.Body([G.Polygon([tuple(v) for v in a], kind="Polygon4")], mass=inf, inertia=inf),
            P.Body([G.Polygon([tuple(v) for v in b], kind="Polygon6")], mass=1.0, inertia=1.0)]


EGO = Cam(half_extent=(1.0, 0.75), follow_body=0, follow_angle=True)
CASES = {
    "robocup_reset": Case(robocup_reset, 32, 24, Cam(), {0, 1, 2}),
    # thin goal AABBs over the play area over the field: the overlap order
    "robocup_goal_zoom": Case(robocup_reset, 16, 12, Cam(center=(-4.6, 0.45), half_extent=(0.16, 0.12)), {1, 2, 3}),
    # the circle's eps rule, a camera that follows the ball
    "robocup_ball_zoom": Case(robocup_reset, 16, 12, Cam(half_extent=(0.125, 0.09375), follow_body=4), {2, 5}),
    # pixel centres on the play area's +-4.5 edge (4.8 * 15/16): the window lies inside the field, no background
    "robocup_field_edge": Case(robocup_reset, 16, 12, Cam(half_extent=(4.8, 3.2)), {2}),
    "robocup_2_steps": Case(robocup_stepped, 16, 12, Cam(), {0, 2, 3}),  # body 0's state is NaN: it paints nothing
    "lunar_reset": Case(lunar_reset, 32, 24, Cam(), {0, 1, 2, 3, 4}),
    "lunar_terrain": Case(lunar_reset, 16, 12, Cam(), None),
    "lunar_egocentric": Case(lunar_stepped, 16, 12, EGO, {0, 1}),
    "lunar_large_angle": Case(lunar_large_angle, 16, 12, EGO, {0, 1}),
    "octagons": Case(octagons, 64, 48, Cam(), None),  # 16 x 12 pixel centres miss the 0.25-radius octagons
    "adversarial": Case(adversarial, 16, 12, Cam(), None),
}
