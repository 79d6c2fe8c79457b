"""Range-sensor gradients without a GPU: the
winner-reporting cast and the restated rank of cotix_raycast_grad.h equal what
they restate, bit for bit; the host checker (tests/emu/cotix_raygrad_host.cpp --
the functions the gfx950 kernel runs, in a plain loop) is held against a
float64 vector-Jacobian product; the zero-contribution and layout rules;
cotix_raycast_backward's refusals, before any device call; the Python
surface's argument checks; the stand-alone sanitizer driver."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import raygrad_cases as GC

RC = GC.RC
HERE = os.path.dirname(os.path.abspath(__file__))
B = GC.B
NAMES = list(GC.CASES)


def _host(name, g=None, **kw):
    c = GC.CASES[name]
    return GC.host_vjp(GC.envs_of(name), c.sensor, c.dirs, GC.cotangent(name) if g is None else g, **kw)


def _same(a, b):
    return np.array_equal(GC.bits(a), GC.bits(b))


# ----------------------------------------------------------------------------
# 1. the restatements
# ----------------------------------------------------------------------------
def test_there_are_fourteen_cases():
    assert len(NAMES) == 14 and set(GC.NEW) <= set(NAMES) and set(RC.CASES) <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_winner_cast_equals_ray_cast(name):
    """ray_cast_win's t and id are ray_cast's on every ray, and its winner names a feature of a visible part."""
    c = GC.CASES[name]
    envs = GC.envs_of(name)
    want_d, want_h = RC.host_rays(envs, c.sensor, c.dirs)
    if c.ids is not None:
        assert set(want_h.ravel().tolist()) == c.ids, (name, set(want_h.ravel().tolist()))
    d, h, part, feat = GC.host_win(envs, c.sensor, c.dirs)
    assert _same(d, want_d) and np.array_equal(h, want_h)
    (body, kind, nv, _), _ = GC.part_table(envs[0])
    vis = [p for p in range(len(body)) if body[p] not in c.sensor.ignore]
    assert ((part == -1) == (h == 0)).all()
    for e, k in zip(*np.nonzero(h)):
        p = vis[part[e, k]]
        assert body[p] + 1 == h[e, k]
        assert 0 <= feat[e, k] < (2 if kind[p] == 0 else 4 if kind[p] == 1 else nv[p])


def _polygons():
    """{nv: [world vertices before the sort]} of every polygon of every case and env."""
    out = {}
    for name in NAMES:
        for bodies in GC.envs_of(name):
            for b in bodies:
                T = b.transformer()
                for p in b.parts:
                    if p.kind not in ("Circle", "AABB"):
                        out.setdefault(len(p.vertices_), []).append([T.forward_vector(v) for v in p.vertices_])
    return out


def test_restated_rank_reproduces_order_clockwise():
    polys = _polygons()
    assert {4, 5, 6, 8} <= set(polys)
    seen_bad = seen_dup = 0
    for nv, ps in polys.items():
        xy = np.array(ps, GC.F)
        srt, gat, rank = GC.host_rank(xy)
        assert _same(srt, gat), nv
        assert (np.sort(rank, 1) == np.arange(nv)).all()
        for i, q in enumerate(ps):  # ... and both are the oracle's order
            assert rank[i][GC.G.order_clockwise_idx(q)].tolist() == list(range(nv))
        seen_bad += int((~np.isfinite(xy).all((1, 2))).sum())
        seen_dup += sum(len({tuple(map(float, v)) for v in q}) < nv for q in ps)
    assert seen_bad >= B and seen_dup >= 2 * B


# ----------------------------------------------------------------------------
# 2. the host VJP against the float64 VJP
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_f64_vjp_forward_is_f64_rays(name):
    """What makes the float64 VJP a check: the t it differentiates is RC.f64_rays' distance (within 1e-12)
    and its hit RC.f64_rays' hit, on every ray that is not fragile."""
    d64, h64, fragile = GC.f64_batch(name)
    t, hit, _, _ = GC.f64_vjp_batch(name)
    keep = ~fragile
    assert np.array_equal(hit[keep], h64[keep])
    assert (np.abs(t - d64)[keep] <= 1e-12).all()
    if name in GC.NEW:  # (the other twelve: tests/test_raycast_cpu.py)
        print("%s: %d of %d rays fragile" % (name, int(fragile.sum()), fragile.size))
        assert 4 * int(fragile.sum()) <= fragile.size


@pytest.mark.parametrize("name", NAMES)
def test_host_vjp_equals_float64(name):
    """max |got - want| / max |want| per env, g_dyn and g_geom apart, within GC.VJP_LIMIT; fragile rays carry a
    zero cotangent and at most a quarter of a case's rays are fragile -- but for robocup_axes, the degenerate set
    by construction (rays through corners and along edges: 14 of its 40 rays), which the forward's float64 test
    leaves out altogether and which is compared here on its other 26.  own_body's g_dyn is the other exception:
    its float64 value is 0 (the sensor's and the crossed body's contributions cancel), so there is nothing to
    divide by, and test_own_body holds it to the same limit relative to max |g|."""
    g = GC.cotangent(name)
    fragile = GC.f64_batch(name)[2]
    assert 4 * int(fragile.sum()) <= fragile.size or name == "robocup_axes"
    assert not g[fragile].any() and g[~fragile].all()
    _, _, want_p, want_r = GC.f64_vjp_batch(name)
    gd, gg = _host(name)
    pose = GC.pose_rows(gd)
    rd = [GC.ratio(pose[e], want_p[e]) for e in range(B)] if name != "own_body" else [0.0]
    rg = [GC.ratio(gg[:, e], want_r[e]) for e in range(B)]
    print("%s: worst ratio g_dyn %.3g, g_geom %.3g" % (name, max(rd), max(rg)))
    assert max(rd) <= GC.VJP_LIMIT and max(rg) <= GC.VJP_LIMIT, (name, rd, rg)
    assert np.abs(want_r).max() > 0.1 and (name == "own_body" or np.abs(want_p).max() > 0.1)  # (not vacuous)


# ----------------------------------------------------------------------------
# 3. what contributes nothing
# ----------------------------------------------------------------------------
def test_nan_and_inf_cotangents_on_misses_reach_nothing():
    c = GC.CASES["clipped"]
    envs = GC.envs_of("clipped")
    _, hit = RC.host_rays(envs, c.sensor, c.dirs)
    assert int((hit == 0).sum()) == 60 and hit.size == 80
    g = GC.cotangent("clipped").copy()
    g[hit == 0] = 0.0
    want = GC.host_vjp(envs, c.sensor, c.dirs, g)
    assert np.abs(want[0]).max() > 0 and np.abs(want[1]).max() > 0
    for bad in (np.nan, np.inf, -np.inf):
        g2 = g.copy()
        g2[hit == 0] = bad
        got = GC.host_vjp(envs, c.sensor, c.dirs, g2)
        assert _same(got[0], want[0]) and _same(got[1], want[1])
    # an env with no hit at all: every word is +0.0
    none = [e for e in range(B) if not hit[e].any()]
    g3 = np.full_like(g, np.nan)
    got = GC.host_vjp(envs, c.sensor, c.dirs, g3)
    for e in none:
        assert not GC.bits(got[0][:, :, e]).any() and not GC.bits(got[1][:, e]).any()


@pytest.mark.parametrize("zero", [0.0, -0.0])
@pytest.mark.parametrize("name", ["lunar_reset", "robocup_fixed", "octagons"])
def test_zero_cotangent_equals_leaving_the_ray_out(name, zero):
    c = GC.CASES[name]
    envs = GC.envs_of(name)
    _, hit = RC.host_rays(envs, c.sensor, c.dirs)
    k = int(np.argmax((hit != 0).sum(0)))  # the ray that hits in the most envs
    assert hit[:, k].any()
    g = np.random.default_rng(3).uniform(-1.0, 1.0, hit.shape).astype(GC.F)
    g[:, k] = zero
    keep = [j for j in range(len(c.dirs)) if j != k]
    got = GC.host_vjp(envs, c.sensor, c.dirs, g)
    want = GC.host_vjp(envs, c.sensor, c.dirs[keep], g[:, keep])
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    g[:, k] = 0.5  # (and the ray does matter)
    other = GC.host_vjp(envs, c.sensor, c.dirs, g)
    assert not _same(other[1], want[1])


def test_nan_bodies_get_zeros_and_a_nan_sensor_sees_nothing():
    name = "robocup_2_steps"
    envs = GC.envs_of(name)
    nan_envs = [e for e in range(B) if np.isnan(envs[e][0].dyn()[0])]
    assert 0 in nan_envs
    gd, gg = _host(name)
    (body, _, _, goff), _ = GC.part_table(envs[0])
    for e in nan_envs:
        assert not GC.bits(gd[0, :, e]).any()
        for p in np.nonzero(body == 0)[0]:
            assert not GC.bits(gg[goff[p]:goff[p] + 4, e]).any()
    assert np.abs(gd[:, :, nan_envs]).max() > 0  # the other bodies of those envs are seen
    # a sensor on the NaN body: all zeros in those envs, whatever the cotangent
    sensor, dirs = GC.Sensor(body=0, max_range=5.0, ignore=()), GC.fan(16)
    g = np.random.default_rng(5).uniform(-1.0, 1.0, (B, 16)).astype(GC.F)
    g[:, 3] = np.nan
    gd, gg = GC.host_vjp(envs, sensor, dirs, g)
    for e in nan_envs:
        assert not GC.bits(gd[:, :, e]).any() and not GC.bits(gg[:, e]).any()
    # a NaN cotangent on a ray that hits reaches the words that ray touches, and only those
    c = GC.CASES[name]
    _, hit = RC.host_rays(envs, c.sensor, c.dirs)
    e, k = [int(x[0]) for x in np.nonzero(hit)]
    g = GC.cotangent(name).copy()
    g[e, k] = np.nan
    gd, gg = _host(name, g)
    crossed = int(hit[e, k]) - 1
    assert np.isnan(gd[4, :2, e]).all() and np.isnan(gd[crossed, :2, e]).all()
    gd[[4, crossed], :, e] = 0
    assert not np.isnan(gd).any() and 0 < np.isnan(gg[:, e]).sum() <= 4 and not np.isnan(np.delete(gg, e, 1)).any()


# ----------------------------------------------------------------------------
# 4. own_body
# ----------------------------------------------------------------------------
def test_own_body():
    """Every ray leaves the ball's own circle from its centre: dist = r / |d| with |d| = 1 exactly, so g_r is
    the f32 sum of the cotangents in ray order, bit for bit, and the pose gradients cancel to rounding."""
    name = "own_body"
    c = GC.CASES[name]
    envs = GC.envs_of(name)
    dist, hit = RC.host_rays(envs, c.sensor, c.dirs)
    assert (hit == 5).all()
    (body, kind, _, goff), _ = GC.part_table(envs[0])
    ball = int(np.nonzero(body == 4)[0][0])
    assert kind[ball] == 0
    assert (GC.bits(dist) == GC.bits(GC.F(envs[0][4].parts[0].radius))).all()
    g = GC.cotangent(name)
    assert np.count_nonzero(g) >= 3 * g.size // 4
    gd, gg = _host(name)
    for e in range(B):
        acc = GC.F(0.0)
        for v in g[e]:
            if v != 0:
                acc = GC.F(acc + v)
        assert GC.bits(gg[goff[ball], e]) == GC.bits(acc), (e, gg[goff[ball], e], acc)
    lim = GC.VJP_LIMIT * float(np.abs(g).max())
    print("own_body: max |g_px|, |g_py| %.3g" % float(np.abs(gd[4, :2, :]).max()))
    assert float(np.abs(gd[:, [0, 1, 4], :]).max()) <= lim
    assert not GC.bits(gg[goff[ball] + 3]).any()  # the circle's pad word


# ----------------------------------------------------------------------------
# 5. layout
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_layout_zeros_and_single_outputs(name):
    c = GC.CASES[name]
    envs = GC.envs_of(name)
    gd, gg = _host(name)
    assert gd.dtype == gg.dtype == np.float32 and not (gd == GC.SENTINEL).any() and not (gg == GC.SENTINEL).any()
    assert not GC.bits(gd[:, [2, 3, 5], :]).any()  # the velocity rows: +0.0
    (body, kind, nv, goff), gw = GC.part_table(envs[0])
    words = np.where(kind == 2, 2 * nv, 4)
    assert gg.shape == (gw, B)
    for p in np.nonzero(kind == 0)[0]:
        assert not GC.bits(gg[goff[p] + 3]).any()  # a circle's pad word
    _, hit = RC.host_rays(envs, c.sensor, c.dirs)
    g = GC.cotangent(name)
    for e in range(B):
        touched = set((hit[e][g[e] != 0] - 1).tolist()) - {-1}
        if touched and c.sensor.body is not None:
            touched.add(c.sensor.body)
        for k in range(len(envs[0])):
            if k not in touched:
                assert not GC.bits(gd[k, :, e]).any(), (name, e, k)
                for p in np.nonzero(body == k)[0]:
                    assert not GC.bits(gg[goff[p]:goff[p] + words[p], e]).any()
    # either output alone is the same bits
    assert _same(_host(name, want_geom=False)[0], gd) and _host(name, want_geom=False)[1] is None
    assert _same(_host(name, want_dyn=False)[1], gg) and _host(name, want_dyn=False)[0] is None


def test_shared_and_per_env_geometry_give_the_same_columns(monkeypatch):
    name = "robocup_goals"
    envs = GC.envs_of(name)
    assert GC.batch_arrays(envs)[1].ndim == 1  # shared
    want = _host(name)

    def per_env(es):
        dyn, geom = RC.batch_arrays(es)
        return dyn, np.ascontiguousarray(np.tile(geom, (len(es), 1)))

    monkeypatch.setattr(GC, "batch_arrays", per_env)
    got = _host(name)
    assert _same(got[0], want[0]) and _same(got[1], want[1])


# ----------------------------------------------------------------------------
# 6. the C ABI's refusals: every check runs before any device call (no GPU here)
# ----------------------------------------------------------------------------
def _call(pa, scene, dyn=4096, geom=4096, stride=0, B=4, sensor=(4, 0, 0.0, 0.0, 5.0, 16), dirs=4096, R=16,
          g_dist=4096, g_dyn=4096, g_geom=4096):
    v = lambda x: None if x is None else ctypes.c_void_p(x)  # noqa: E731  (fake pointers: never dereferenced)
    s = None if sensor is None else pa._ffi.CotixRaySensor(*sensor)
    rc = pa._ffi.lib.cotix_raycast_backward(scene, v(dyn), v(geom), stride, B, s, v(dirs), R, v(g_dist), v(g_dyn),
                                            v(g_geom), None)
    return rc, pa._ffi.lib.cotix_last_error().decode()


NAN, INF = float("nan"), float("inf")
REFUSALS = [
    (dict(scene=None), "null scene"),
    (dict(dyn=None), "null dyn"),
    (dict(sensor=None), "null sensor"),
    (dict(dirs=None), "null dirs"),
    (dict(g_dist=None), "null g_dist"),
    (dict(g_dyn=None, g_geom=None), "g_dyn and g_geom are both null"),
    (dict(B=0), "B must be positive"),
    (dict(B=-3), "B must be positive"),
    (dict(R=0), "n_rays must be in [1, 1024]"),
    (dict(R=-1), "n_rays must be in [1, 1024]"),
    (dict(R=1025), "n_rays must be in [1, 1024]"),
    (dict(sensor=(5, 0, 0.0, 0.0, 5.0, 0)), "body out of range"),
    (dict(sensor=(-2, 0, 0.0, 0.0, 5.0, 0)), "body out of range"),
    (dict(sensor=(4, 2, 0.0, 0.0, 5.0, 0)), "follow_angle must be 0 or 1"),
    (dict(sensor=(4, -1, 0.0, 0.0, 5.0, 0)), "follow_angle must be 0 or 1"),
    (dict(sensor=(-1, 1, 0.0, 0.0, 5.0, 0)), "follow_angle needs a body"),
    (dict(sensor=(4, 0, NAN, 0.0, 5.0, 0)), "offset must be finite"),
    (dict(sensor=(4, 0, 0.0, -INF, 5.0, 0)), "offset must be finite"),
    (dict(sensor=(4, 0, 0.0, 0.0, 0.0, 0)), "max_range must be finite and positive"),
    (dict(sensor=(4, 0, 0.0, 0.0, -1.0, 0)), "max_range must be finite and positive"),
    (dict(sensor=(4, 0, 0.0, 0.0, INF, 0)), "max_range must be finite and positive"),
    (dict(sensor=(4, 0, 0.0, 0.0, NAN, 0)), "max_range must be finite and positive"),
    (dict(sensor=(4, 0, 0.0, 0.0, 5.0, 1 << 5)), "ignore_mask names a body the scene lacks"),
    (dict(sensor=(4, 0, 0.0, 0.0, 5.0, 1 << 31)), "ignore_mask names a body the scene lacks"),
    (dict(geom=None), "geometry required"),
    (dict(stride=7), "geom_stride smaller than the scene geometry"),
]


def test_refusals_hold_the_forwards_list():
    """The forward's list (tests/test_raycast_cpu.py) with `null dist` replaced by the backward's two."""
    import test_raycast_cpu as fwd
    mine = [(repr(sorted(k.items())), m) for k, m in REFUSALS if "g_d" not in m]
    theirs = [(repr(sorted(k.items())), m) for k, m in fwd.REFUSALS if m != "null dist"]
    assert mine == theirs


@pytest.mark.parametrize("kw,msg", REFUSALS, ids=[m[1].replace(" ", "_") + str(i) for i, m in enumerate(REFUSALS)])
def test_raycast_backward_refuses(kw, msg):
    import parallax_amd as pa
    s = pa.Scene(pa.scenarios.robocup_bodies())
    kw = dict(kw)
    scene = kw.pop("scene", s.handle)
    rc, err = _call(pa, scene, **kw)
    assert rc < 0 and msg in err, (rc, err)


# ----------------------------------------------------------------------------
# 7. the Python surface: argument checks (a "cpu" world: nothing is launched)
# ----------------------------------------------------------------------------
def _cpu_world(pa):
    return pa.World(pa.scenarios.robocup_bodies(), 4, "cpu", torch.zeros(4, 2, dtype=torch.int32))


def test_rays_backward_checks_its_arguments():
    import parallax_amd as pa
    assert pa.differentiable_rays is pa.render.differentiable_rays
    w = _cpu_world(pa)
    s, dirs, g = pa.RaySensor(body=4, max_range=5.0), pa.RaySensor.fan(16), torch.zeros(4, 16)
    for bad in (torch.zeros(4, 15), torch.zeros(16, 4), torch.zeros(4, 16, dtype=torch.float64),
                torch.zeros(4, 32)[:, ::2], torch.zeros(4, 16, device="meta"), np.zeros((4, 16), np.float32)):
        with pytest.raises(ValueError, match="grad_dist must be"):
            pa.render.rays_backward(w, s, dirs, bad)
    with pytest.raises(ValueError, match="both False"):
        pa.render.rays_backward(w, s, dirs, g, want_dyn=False, want_geom=False)
    with pytest.raises(ValueError, match="dirs must be"):
        pa.render.rays_backward(w, s, torch.zeros(16, 3), g)
    with pytest.raises(ValueError, match="dyn must be"):
        pa.render.rays_backward(w, s, dirs, g, dyn=torch.zeros(5, 6, 3))
    with pytest.raises(TypeError, match="RaySensor"):
        pa.render.rays_backward(w, pa.Camera(), dirs, g)
    assert pa.BatchedEnv.rays_backward.__doc__


def test_differentiable_rays_checks_its_arguments():
    import parallax_amd as pa
    w = _cpu_world(pa)
    s, dirs = pa.RaySensor(body=4, max_range=5.0), pa.RaySensor.fan(16)
    have = w.geometry()
    assert have.dim() == 1
    for bad in (torch.zeros(have.shape[0] + 1), torch.zeros(4, have.shape[0]), torch.zeros(())):
        with pytest.raises(ValueError, match="geometry must be"):
            pa.differentiable_rays(w, s, dirs, geometry=bad)
    with pytest.raises(ValueError, match="geometry must be a float32"):
        pa.differentiable_rays(w, s, dirs, geometry=torch.zeros(have.shape[0], dtype=torch.float64))
    with pytest.raises(ValueError, match="dyn must be"):
        pa.differentiable_rays(w, s, dirs, dyn=torch.zeros(5, 6, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="dirs must be"):
        pa.differentiable_rays(w, s, torch.zeros(16, 2, dtype=torch.float64))
    with pytest.raises(TypeError, match="RaySensor"):
        pa.differentiable_rays(w, None, dirs)


# ----------------------------------------------------------------------------
# 8. the stand-alone sanitizer driver
# ----------------------------------------------------------------------------
def test_host_checker_under_sanitizers(tmp_path):
    """The stand-alone ASan/UBSan driver of the host checker (exactly sized buffers) exits cleanly and writes
    the plain build's bytes."""
    GC.build_host("raygrad_asan_driver")
    for name, wd, wg in (("lunar_large_angle", 1, 1), ("octagons", 1, 1), ("adversarial", 0, 1), ("own_body", 1, 0),
                         ("one_ray", 1, 1)):
        c = GC.CASES[name]
        envs = GC.envs_of(name, 3)
        (body, kind, nv, goff), gw = GC.part_table(envs[0])
        dyn, geom = GC.batch_arrays(envs)
        sw, sb, fa, mask = GC.sensor_words(c.sensor)
        R, g = len(c.dirs), np.ascontiguousarray(GC.cotangent(name)[:3])
        inp, out = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        with open(inp, "wb") as f:
            np.array([len(body), dyn.shape[0], 3, gw, 0 if geom.ndim == 1 else geom.shape[1], R, sb, fa, mask, gw,
                      wd, wg], np.int32).tofile(f)
            for x in (body, kind, nv, goff, sw, c.dirs, dyn, geom, g):
                np.ascontiguousarray(x).tofile(f)
        r = subprocess.run([os.path.join(HERE, "emu", "build", "raygrad_asan_driver"), inp, out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        want_d, want_g = GC.host_vjp(envs, c.sensor, c.dirs, g, want_dyn=bool(wd), want_geom=bool(wg))
        raw = np.fromfile(out, np.uint32)
        nd = dyn.size if wd else 0
        assert raw.size == nd + (gw * 3 if wg else 0)
        if wd:
            assert np.array_equal(raw[:nd].reshape(dyn.shape), GC.bits(want_d))
        if wg:
            assert np.array_equal(raw[nd:].reshape(gw, 3), GC.bits(want_g))
