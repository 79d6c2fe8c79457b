"""Range-sensor observations without a GPU: the host
checker (tests/emu/cotix_raycast_host.cpp -- the functions of cotix_raycast.h
the gfx950 kernel runs, in a plain loop) equals the oracle restatement of the
semantics on every ray of every case, bit for bit (the same f32 expressions,
so no tolerance); the restatement itself is held against the same semantics
in float64; cotix_raycast refuses every bad argument before any device call;
the Python surface (RaySensor, fan, out=) checks its arguments."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import raster_cases
import raycast_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
B = RC.B


def check_not_vacuous(name):
    """The oracle's readings of envs 0 .. 4 hold what the case is about."""
    c = RC.CASES[name]
    dist, hit = RC.oracle_batch(name)
    if c.ids is not None:
        assert set(hit.ravel().tolist()) == c.ids, (name, set(hit.ravel().tolist()))
    rng = np.float32(c.sensor.max_range)
    assert (dist[hit == 0] == rng).all() and (dist[hit != 0] <= rng).all() and (dist[hit != 0] >= 0).all()
    return dist, hit


@pytest.mark.parametrize("name", list(RC.CASES))
def test_host_checker_equals_oracle(name):
    c = RC.CASES[name]
    want_d, want_h = check_not_vacuous(name)
    got_d, got_h = RC.host_rays(RC.case_envs(name), c.sensor, c.dirs)
    assert got_d.shape == want_d.shape == (B, len(c.dirs)) and got_d.dtype == np.float32 and got_h.dtype == np.uint8
    diff = (RC.bits(got_d) != RC.bits(want_d)) | (got_h != want_h)
    assert not diff.any(), "%s: %d rays differ" % (name, int(diff.sum()))


def test_null_hit_leaves_dist_unchanged_host():
    c = RC.CASES["lunar_reset"]
    envs = RC.case_envs("lunar_reset")
    d0, _ = RC.host_rays(envs, c.sensor, c.dirs)
    d1, h1 = RC.host_rays(envs, c.sensor, c.dirs, want_hit=False)
    assert h1 is None and np.array_equal(RC.bits(d0), RC.bits(d1))


def test_axes_values_and_the_tie_rule():
    """From the origin of the reset pitch, ball masked out: along the axes the
    play area's touch and goal lines at 4.5 and 3 (the two edges parallel to
    each ray do not count), and the four directions (+-4.5, +-3), which are
    not unit vectors, reach its corners at t = 1, where two edges tie.  Every
    answer is the play area's (id 2), never the larger field's (id 1) behind
    it; a tie keeps the earlier edge, so it changes no reading here, and the
    restatement with the edges reversed gives the same bits."""
    dist, hit = check_not_vacuous("robocup_axes")
    assert dist[0].tolist() == [4.5, 3.0, 4.5, 3.0, 1.0, 1.0, 1.0, 1.0]
    assert (hit == 2).all()
    # the corner rays cross two edges of the play area at the same t, and both count
    c = RC.CASES["robocup_axes"]
    area = RC.case_envs("robocup_axes", 1)[0][1]
    s = area.parts[0].transform(area.transformer())
    o = (RC.F(0), RC.F(0))
    for d in c.dirs[4:]:
        ts = []
        for e0, e1 in s.edges():
            sv, w = RC.G.vsub(e1, e0), RC.G.vsub(e0, o)
            with np.errstate(all="ignore"):
                cc = RC._cross(tuple(d), sv)
                t, u = RC._cross(w, sv) / cc, RC._cross(w, tuple(d)) / cc
            if cc != 0 and 0 <= t <= 8 and 0 <= u <= 1:
                ts.append(float(t))
        assert ts == [1.0, 1.0], ts


def test_tie_keeps_the_earlier_part():
    """Two bodies with the same AABB: every crossing ties, and the first body
    in scene order answers."""
    P = raster_cases.P
    inf = float("inf")
    box = lambda: P.Body([RC.G.AABB((-1.0, -1.0), (1.0, 1.0))], mass=inf, inertia=inf)  # noqa: E731
    bodies = [box(), box()]
    dist, hit = RC.oracle_rays(bodies, RC.Sensor(max_range=4.0), RC.fan(16))
    assert (hit == 1).all() and (dist <= np.float32(1.5)).all()
    hd, hh = RC.host_rays([bodies], RC.Sensor(max_range=4.0), RC.fan(16))
    assert np.array_equal(RC.bits(hd[0]), RC.bits(dist)) and np.array_equal(hh[0], hit)
    # masking the first one out hands the same distances to the second
    d2, h2 = RC.host_rays([bodies], RC.Sensor(max_range=4.0, ignore=(0,)), RC.fan(16))
    assert np.array_equal(RC.bits(d2[0]), RC.bits(dist)) and (h2 == 2).all()


def test_ray_from_inside_reports_the_exit():
    """Cast from the ball with only the ball masked out, the play area around
    it answers with the distance to its boundary: crossings, not entries."""
    dist, hit = check_not_vacuous("robocup_ball")
    assert (hit[0] == 2).sum() >= 8 and not (hit == 1).any()
    near = dist[0][hit[0] == 2]
    assert (near >= 3.0).all() and (near <= 5.0).all()  # the 9 x 6 play area from its centre


def test_nan_body_is_invisible_and_a_sensor_on_one_sees_nothing():
    bodies = RC.CASES["robocup_2_steps"].make(0)
    assert all(np.isnan(x) for x in bodies[0].dyn()[:2])
    _, hit = check_not_vacuous("robocup_2_steps")
    assert not (hit == 1).any()
    sensor, dirs = RC.Sensor(body=0, max_range=5.0, ignore=()), RC.fan(16)
    envs = RC.case_envs("robocup_2_steps")
    nan_envs = [e for e in range(B) if np.isnan(envs[e][0].dyn()[0])]
    assert 0 in nan_envs
    d, h = RC.host_rays(envs, sensor, dirs)
    assert (d[nan_envs] == np.float32(5.0)).all() and (h[nan_envs] == 0).all()
    for e in nan_envs:
        od, oh = RC.oracle_rays(envs[e], sensor, dirs)
        assert (od == np.float32(5.0)).all() and (oh == 0).all()


def test_per_env_terrain_gives_per_env_readings():
    envs = RC.case_envs("lunar_reset", 2)
    _, geom = RC.batch_arrays(envs)
    assert geom.ndim == 2  # one geometry row per env
    assert not np.array_equal(geom[0], geom[1])
    # the lander starts at the same pose in every env, so whatever differs is the terrain's.  Envs 0 and 1 keep
    # theirs beyond the 6-unit range (the lander hangs 5 above the origin); envs 2, 3 and 4 each read their own
    for name in ("lunar_reset", "lunar_down"):
        dist, hit = RC.oracle_batch(name)
        assert (hit[2] == 4).any() and not (hit[:2] == 4).any()
        assert not np.array_equal(dist[0], dist[2])
    dist, hit = RC.oracle_batch("lunar_down")
    seen = [dist[e][hit[e] == 4] for e in (2, 3, 4)]
    assert all(len(s) for s in seen) and len({s.tobytes() for s in seen}) == 3


def test_large_angle_and_many_rays_per_lane():
    big = RC.CASES["lunar_large_angle"].make(0)
    assert abs(float(big[0].angle)) > 8192.0  # sincos32's large-argument reduction
    _, hit = check_not_vacuous("lunar_large_angle")
    assert len(set(hit.ravel().tolist())) > 1
    assert len(RC.CASES["lunar_down"].dirs) > 64 and len(RC.CASES["octagons"].dirs) > 64
    _, hit = check_not_vacuous("octagons")
    assert not (hit == 0).any()


def test_clipped_and_single_ray():
    dist, hit = check_not_vacuous("clipped")
    assert int((hit == 0).sum()) == 60 and hit.size == 80
    assert (RC.bits(dist[hit == 0]) == RC.bits(np.float32(3.5))).all()
    dist, hit = check_not_vacuous("one_ray")
    assert dist.shape == (B, 1) and (hit != 0).all()


def test_adversarial_set_has_bad_vertices():
    for e in range(B):
        a, b = raster_cases._adversarial_pairs()[e]
        assert not (np.isfinite(a).all() and np.isfinite(b).all())
    check_not_vacuous("adversarial")


# ----------------------------------------------------------------------------
# the independent float64 check of the restatement
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in RC.CASES if n != "robocup_axes"])  # the degenerate set, by construction
def test_restatement_equals_float64(name):
    """The same semantics in float64 on the same f32 inputs (RC.f64_rays).  A
    ray is left out when, in float64, an edge or circle root with t in
    [-1e-2, max_range + 1e-2] has t within 1e-2 of 0 or max_range, or is an
    edge with u in [-0.01, 1.01] and |c| < 0.05 |d||s| or u within 0.01 of an
    endpoint, or a circle with disc < 0.05 a r^2, or has a NaN u.  At most a
    quarter of a case's rays may be left out.  On the others the hit is the
    float64 one and the distance within 1e-3: with coordinates <= 8 and
    u = 2^-24 the numerator's error is <= 4 u |w|_1 |s|_1, and dividing by
    |c| >= 0.05 |s| leaves about 1.5e-4."""
    c = RC.CASES[name]
    dist, hit = RC.oracle_batch(name)
    envs = RC.case_envs(name)
    left_out = worst = 0
    for e in range(B):
        d64, h64, fragile = RC.f64_rays(envs[e], c.sensor, c.dirs)
        keep = ~fragile
        left_out += int(fragile.sum())
        assert np.array_equal(hit[e][keep], h64[keep]), (name, e)
        err = np.abs(dist[e][keep].astype(np.float64) - d64[keep])
        worst = max(worst, float(err.max()) if keep.any() else 0.0)
    print("%s: %d of %d rays left out, worst |dist32 - dist64| %.3g" % (name, left_out, hit.size, worst))
    assert 4 * left_out <= hit.size, (name, left_out, hit.size)
    assert worst <= 1e-3, (name, worst)


# ----------------------------------------------------------------------------
# the stand-alone sanitizer driver
# ----------------------------------------------------------------------------
def test_host_checker_under_sanitizers(tmp_path):
    """The stand-alone ASan/UBSan driver of the host checker (exactly sized
    buffers) exits cleanly and writes the plain build's bytes."""
    RC.build_host("raycast_asan_driver")
    for name, want_hit in (("lunar_large_angle", True), ("octagons", True), ("adversarial", False),
                           ("robocup_fixed", True), ("one_ray", True)):
        c = RC.CASES[name]
        envs = RC.case_envs(name, 3)
        (body, kind, nv, goff), G_ = RC.part_table(envs[0])
        dyn, geom = RC.batch_arrays(envs)
        sw, sb, fa, mask = RC.sensor_words(c.sensor)
        R = len(c.dirs)
        inp, out = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        with open(inp, "wb") as f:
            np.array([len(body), dyn.shape[0], 3, G_, 0 if geom.ndim == 1 else geom.shape[1], R, sb, fa, mask,
                      int(want_hit)], np.int32).tofile(f)
            for x in (body, kind, nv, goff, sw, c.dirs, dyn, geom):
                np.ascontiguousarray(x).tofile(f)
        r = subprocess.run([os.path.join(HERE, "emu", "build", "raycast_asan_driver"), inp, out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        want_d, want_h = RC.host_rays(envs, c.sensor, c.dirs, want_hit=want_hit)
        raw = np.fromfile(out, np.uint8)
        assert raw.size == 3 * R * (5 if want_hit else 4)
        assert np.array_equal(raw[:12 * R].view(np.uint32).reshape(3, R), RC.bits(want_d))
        if want_hit:
            assert np.array_equal(raw[12 * R:].reshape(3, R), want_h)


# ----------------------------------------------------------------------------
# the C-ABI's refusals: every check runs before any device call (no GPU here)
# ----------------------------------------------------------------------------
def _call(pa, scene, dyn=4096, geom=4096, stride=0, B=4, sensor=(4, 0, 0.0, 0.0, 5.0, 16), dirs=4096, R=16, dist=4096,
          hit=4096):
    v = lambda x: None if x is None else ctypes.c_void_p(x)  # noqa: E731  (fake pointers: never dereferenced)
    s = None if sensor is None else pa._ffi.CotixRaySensor(*sensor)
    rc = pa._ffi.lib.cotix_raycast(scene, v(dyn), v(geom), stride, B, s, v(dirs), R, v(dist), v(hit), None)
    return rc, pa._ffi.lib.cotix_last_error().decode()


NAN, INF = float("nan"), float("inf")
REFUSALS = [
    (dict(scene=None), "null scene"),
    (dict(dyn=None), "null dyn"),
    (dict(sensor=None), "null sensor"),
    (dict(dirs=None), "null dirs"),
    (dict(dist=None), "null dist"),
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


@pytest.mark.parametrize("kw,msg", REFUSALS, ids=[m[1].replace(" ", "_") + str(i) for i, m in enumerate(REFUSALS)])
def test_raycast_refuses(kw, msg):
    import parallax_amd as pa
    s = pa.Scene(pa.scenarios.robocup_bodies())
    kw = dict(kw)
    scene = kw.pop("scene", s.handle)
    rc, err = _call(pa, scene, **kw)
    assert rc < 0 and msg in err, (rc, err)


def test_raycast_refuses_short_rows_of_a_per_env_parameter_scene():
    """A per-env-parameter scene's geometry rows carry its 4 words per body
    after the parts' words: a stride of the parts' words alone is refused."""
    import parallax_amd as pa
    bodies = pa.scenarios.robocup_bodies()
    bodies[4] = pa.AnyBody(shape=bodies[4].shape, mass=torch.tensor([0.5, 0.7]), elasticity=1.0)
    s = pa.Scene(bodies)
    assert s.per_env_params and s.geom_floats == s.geom_part_words + 4 * 5
    rc, err = _call(pa, s.handle, stride=s.geom_part_words, B=2)
    assert rc < 0 and "geom_stride smaller than the scene geometry" in err


# ----------------------------------------------------------------------------
# the Python surface
# ----------------------------------------------------------------------------
def test_ray_sensor_is_immutable_and_marshals():
    import parallax_amd as pa
    assert pa.RaySensor is pa.render.RaySensor
    s = pa.RaySensor(max_range=8.0)
    c = s.c_struct()
    assert (c.body, c.follow_angle, c.ox, c.oy, c.max_range, c.ignore_mask) == (-1, 0, 0.0, 0.0, 8.0, 0)
    assert s.ignore == ()
    with pytest.raises(AttributeError, match="immutable"):
        s.max_range = 2.0
    with pytest.raises(AttributeError, match="immutable"):
        del s.body
    s = pa.RaySensor(body=4, offset=(0.25, -0.5), follow_angle=True, max_range=6)
    assert s.ignore == (4,)  # the sensor's own body, by default
    c = s.c_struct()
    assert (c.body, c.follow_angle, c.ox, c.oy, c.max_range, c.ignore_mask) == (4, 1, 0.25, -0.5, 6.0, 1 << 4)
    assert pa.RaySensor(body=4, max_range=6, ignore=()).c_struct().ignore_mask == 0
    assert pa.RaySensor(body=4, max_range=6, ignore=(0, 1, 4, 1)).c_struct().ignore_mask == 0b10011
    with pytest.raises(ValueError, match="ignore"):
        pa.RaySensor(max_range=6, ignore=(32,))


def test_fan():
    import parallax_amd as pa
    d = pa.RaySensor.fan(16, start=0.0)
    assert d.shape == (16, 2) and d.dtype == torch.float32 and d.device.type == "cpu"
    ang = (np.arange(16) + 0.5) * (2 * math.pi / 16)
    assert np.abs(d.numpy().astype(np.float64) - np.stack([np.cos(ang), np.sin(ang)], 1)).max() <= 2.0 ** -24
    d = pa.RaySensor.fan(5, fov=math.pi / 2)  # centred on the sensor's x axis
    a = np.arctan2(d[:, 1].numpy().astype(np.float64), d[:, 0].numpy().astype(np.float64))
    assert np.allclose(a, (np.arange(5) - 2) * (math.pi / 10), atol=1e-7)
    assert pa.RaySensor.fan(1).shape == (1, 2)
    with pytest.raises(ValueError, match="at least one ray"):
        pa.RaySensor.fan(0)


def test_rays_checks_dirs_out_and_dyn():
    import parallax_amd as pa
    w = pa.World(pa.scenarios.robocup_bodies(), 4, "cpu", torch.zeros(4, 2, dtype=torch.int32))
    s, dirs = pa.RaySensor(body=4, max_range=5.0), pa.RaySensor.fan(16)
    for bad in (torch.zeros(16, 3), torch.zeros(16, 2, dtype=torch.float64), torch.zeros(32), torch.zeros(2, 16).T):
        with pytest.raises(ValueError, match="dirs must be"):
            pa.render.rays(w, s, bad)
    for bad in (torch.zeros(4, 16, dtype=torch.float64), torch.zeros(16, 4), torch.zeros(4, 32)[:, ::2]):
        with pytest.raises(ValueError, match="out must be"):
            pa.render.rays(w, s, dirs, out=bad)
    for bad in (torch.zeros(4, 16), torch.zeros(4, 15, dtype=torch.uint8),
                torch.zeros(4, 32, dtype=torch.uint8)[:, ::2]):
        with pytest.raises(ValueError, match="hit_out must be"):
            pa.render.rays(w, s, dirs, hit_out=bad)
    with pytest.raises(ValueError, match="dyn must be"):
        pa.render.rays(w, s, dirs, dyn=torch.zeros(5, 6, 3))
    with pytest.raises(TypeError, match="RaySensor"):
        pa.render.rays(w, pa.Camera(), dirs)
