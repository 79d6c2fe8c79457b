"""Pixel observations without a GPU: the host checker
(tests/emu/cotix_raster_host.cpp -- the functions of cotix_raster.h the gfx950
kernel runs, in a plain loop) equals the oracle restatement of the semantics
on every pixel of every case, byte for byte (the same f32 expressions, so no
tolerance); cotix_rasterize refuses every bad argument before any device
call; the Python surface (Camera, palettes, out=) checks its arguments."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import raster_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
B = 5


def check_not_vacuous(name):
    """The oracle image of env 0 holds what the case is about."""
    c = RC.CASES[name]
    ids, cover = RC.oracle_env(name, 0)
    got = set(ids.ravel().tolist())
    if c.ids is not None:  # the ids the case names, exactly (the zooms lie inside the field: no background)
        assert got == c.ids and len(got) > 1 or name == "robocup_field_edge" and got == {2}, (name, got)
    else:
        assert 0 in got and len(got) > 1, (name, got)
    return ids, cover


@pytest.mark.parametrize("name", list(RC.CASES))
def test_host_checker_equals_oracle(name):
    c = RC.CASES[name]
    check_not_vacuous(name)
    want = RC.oracle_batch(name, B)
    got = RC.host_image(RC.case_envs(name, B), c.W, c.H, c.cam)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), "%s: %d pixels differ" % (name, int((got != want).sum()))


def test_overlap_carries_the_later_body():
    """Goal zoom: the goal (body 2) and the play area (body 1) both lie over
    the field (body 0); a pixel inside two bodies carries the later one's id,
    never the field's."""
    ids, cover = check_not_vacuous("robocup_goal_zoom")
    assert ((cover == 2) & (ids == 3)).any() and ((cover == 2) & (ids == 2)).any()
    assert (ids[cover == 2] > 1).all()
    assert (cover == 1).any() and (ids[cover == 1] == 1).all()  # the field alone


def test_field_edge_is_inclusive():
    """Pixel centres of the first and last column lie on the play area's
    x = -+4.5 edge: AABB.contains is inclusive (and has its eps)."""
    c = RC.CASES["robocup_field_edge"]
    u = np.float32(15) / np.float32(16)
    assert np.float32(0.0) + u * np.float32(c.cam.half_extent[0]) == np.float32(4.5)
    ids, _ = check_not_vacuous("robocup_field_edge")
    assert (ids[:, 0] == 2).all() and (ids[:, -1] == 2).all()


def test_nan_body_paints_nothing():
    bodies = RC.CASES["robocup_2_steps"].make(0)
    assert all(np.isnan(x) for x in bodies[0].dyn()[:2])
    ids, _ = check_not_vacuous("robocup_2_steps")
    assert not (ids == 1).any()


def test_per_env_terrain_gives_per_env_images():
    envs = RC.case_envs("lunar_terrain", 2)
    _, geom = RC.batch_arrays(envs)
    assert geom.ndim == 2  # one geometry row per env
    a, b = RC.oracle_env("lunar_terrain", 0)[0], RC.oracle_env("lunar_terrain", 1)[0]
    assert not np.array_equal(a, b)


def test_egocentric_views():
    ids, _ = check_not_vacuous("lunar_egocentric")
    assert int((ids == 1).sum()) == 132 and ids.size == 192
    big = RC.CASES["lunar_large_angle"].make(0)
    assert abs(float(big[0].angle)) > 8192.0  # sincos32's large-argument reduction
    check_not_vacuous("lunar_large_angle")


def test_adversarial_set_has_bad_vertices():
    for e in range(B):
        a, b = RC._adversarial_pairs()[e]
        assert not (np.isfinite(a).all() and np.isfinite(b).all())
    check_not_vacuous("adversarial")


def test_palette_mapping_host():
    name = "robocup_reset"
    c = RC.CASES[name]
    envs = RC.case_envs(name, 3)
    pal = np.array([(1, 2, 3), (0, 180, 0), (10, 180, 0), (255, 255, 0), (0, 128, 255), (255, 0, 7)], np.uint8)
    ids = RC.host_image(envs, c.W, c.H, c.cam)
    rgb = RC.host_image(envs, c.W, c.H, c.cam, palette=pal)
    assert rgb.shape == (3, 3, c.H, c.W)
    assert np.array_equal(rgb, pal[ids].transpose(0, 3, 1, 2))


def test_host_checker_under_sanitizers(tmp_path):
    """The stand-alone ASan/UBSan driver of the host checker (exactly sized
    buffers) exits cleanly and writes the plain build's bytes."""
    RC.build_host("raster_asan_driver")
    for name, pal in (("lunar_large_angle", None), ("octagons", np.arange(15, dtype=np.uint8).reshape(5, 3) * 17)):
        c = RC.CASES[name]
        envs = RC.case_envs(name, 2)
        (body, kind, nv, goff), G_ = RC.part_table(envs[0])
        dyn, geom = RC.batch_arrays(envs)
        cw, fb, fa = RC.cam_words(c.cam)
        inp, out = str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))
        with open(inp, "wb") as f:
            np.array([len(body), dyn.shape[0], 2, G_, 0 if geom.ndim == 1 else geom.shape[1], c.W, c.H,
                      1 if pal is None else 3, fb, fa], np.int32).tofile(f)
            for x in (body, kind, nv, goff, cw, dyn, geom) + (() if pal is None else (pal,)):
                np.ascontiguousarray(x).tofile(f)
        r = subprocess.run([os.path.join(HERE, "emu", "build", "raster_asan_driver"), inp, out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        want = RC.host_image(envs, c.W, c.H, c.cam, palette=pal)
        assert np.array_equal(np.fromfile(out, np.uint8).reshape(want.shape), want)


# ----------------------------------------------------------------------------
# the C-ABI's refusals: every check runs before any device call (no GPU here)
# ----------------------------------------------------------------------------
def _call(pa, scene, dyn=4096, geom=4096, stride=0, B=4, cam=None, W=16, H=12, ch=1, pal=None, image=4096):
    v = lambda x: None if x is None else ctypes.c_void_p(x)  # noqa: E731  (fake pointers: never dereferenced)
    c = pa._ffi.CotixCamera(0.0, 0.0, 8.0, 6.0, -1, 0) if cam is None else cam
    rc = pa._ffi.lib.cotix_rasterize(scene, v(dyn), v(geom), stride, B, None if cam == "null" else c, W, H, ch, pal,
                                     v(image), None)
    return rc, pa._ffi.lib.cotix_last_error().decode()


REFUSALS = [
    (dict(scene=None), "null scene"),
    (dict(dyn=None), "null dyn"),
    (dict(cam="null"), "null camera"),
    (dict(image=None), "null image"),
    (dict(B=0), "B must be positive"),
    (dict(B=-3), "B must be positive"),
    (dict(W=0), "width must be a multiple of 4"),
    (dict(W=18), "width must be a multiple of 4"),
    (dict(W=1028), "width must be a multiple of 4"),
    (dict(H=0), "height must be in"),
    (dict(H=1025), "height must be in"),
    (dict(ch=2), "channels must be 1"),
    (dict(ch=4), "channels must be 1"),
    (dict(ch=3), "palette is required"),
    (dict(ch=1, pal=bytes(18)), "palette needs 3 channels"),
    (dict(cam=(0, 0, 8, 6, 5, 0)), "follow_body out of range"),
    (dict(cam=(0, 0, 8, 6, -2, 0)), "follow_body out of range"),
    (dict(cam=(0, 0, 8, 6, 4, 2)), "follow_angle must be 0 or 1"),
    (dict(cam=(0, 0, 8, 6, -1, 1)), "follow_angle needs a followed body"),
    (dict(cam=(0, 0, 0, 6, -1, 0)), "half extent must be finite and positive"),
    (dict(cam=(0, 0, 8, -1, -1, 0)), "half extent must be finite and positive"),
    (dict(cam=(0, 0, float("inf"), 6, -1, 0)), "half extent must be finite and positive"),
    (dict(cam=(0, 0, 8, float("nan"), -1, 0)), "half extent must be finite and positive"),
    (dict(cam=(float("nan"), 0, 8, 6, -1, 0)), "centre must be finite"),
    (dict(cam=(0, float("-inf"), 8, 6, -1, 0)), "centre must be finite"),
    (dict(geom=None), "geometry required"),
    (dict(stride=7), "geom_stride smaller than the scene geometry"),
    (dict(image=4098), "4-byte aligned"),
]


@pytest.mark.parametrize("kw,msg", REFUSALS, ids=[m[1].replace(" ", "_") + str(i) for i, m in enumerate(REFUSALS)])
def test_rasterize_refuses(kw, msg):
    import parallax_amd as pa
    s = pa.Scene(pa.scenarios.robocup_bodies())
    kw = dict(kw)
    scene = kw.pop("scene", s.handle)
    if isinstance(kw.get("cam"), tuple):
        kw["cam"] = pa._ffi.CotixCamera(*kw["cam"])
    rc, err = _call(pa, scene, **kw)
    assert rc < 0 and msg in err, (rc, err)


def test_rasterize_refuses_short_rows_of_a_per_env_parameter_scene():
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
def test_camera_is_immutable_and_marshals():
    import parallax_amd as pa
    cam = pa.Camera()
    c = cam.c_struct()
    assert (c.cx, c.cy, c.half_w, c.half_h, c.follow_body, c.follow_angle) == (0.0, 0.0, 8.0, 6.0, -1, 0)
    with pytest.raises(AttributeError, match="immutable"):
        cam.center = (1.0, 1.0)
    c = pa.render.Camera(center=(-4.6, 0.45), half_extent=(1, 0.75), follow_body=0, follow_angle=True).c_struct()
    assert (c.cx, c.half_w, c.follow_body, c.follow_angle) == (np.float32(-4.6), 1.0, 0, 1)


def test_scenario_palettes():
    import parallax_amd as pa
    assert pa.RoboCupEnv.palette == [(0, 0, 0), (0, 180, 0), (0, 180, 0), (255, 255, 0), (0, 128, 255), (255, 0, 0)]
    lunar = pa.render.default_palette(pa.scenarios.lunar_lander_bodies(torch.zeros(1, 7, 4, 2)))
    assert lunar == [(0, 0, 0)] + [(255, 255, 255)] * 4
    box = pa.render.default_palette(pa.scenarios.box_world_bodies())
    assert box == [(0, 0, 0)] + [(128, 128, 128)] * 7
    assert isinstance(pa.LunarLander.palette, property) and isinstance(pa.BoxWorld.palette, property)
    assert pa.render.palette_bytes(lunar, 4) == bytes([0, 0, 0] + [255] * 12)
    with pytest.raises(ValueError, match="palette"):
        pa.render.palette_bytes(lunar, 5)
    with pytest.raises(ValueError, match="palette"):
        pa.render.palette_bytes([(0, 0, 256)] * 5, 4)


def test_pixels_checks_out_and_dyn():
    import parallax_amd as pa
    w = pa.World(pa.scenarios.robocup_bodies(), 4, "cpu", torch.zeros(4, 2, dtype=torch.int32))
    for bad in (torch.zeros(4, 12, 16, dtype=torch.int8), torch.zeros(4, 16, 12, dtype=torch.uint8),
                torch.zeros(4, 12, 32, dtype=torch.uint8)[:, :, ::2], torch.zeros(4, 3, 12, 16, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out must be"):
            pa.render.pixels(w, 16, 12, out=bad)
    with pytest.raises(ValueError, match="out must be"):
        pa.render.pixels(w, 16, 12, palette=pa.RoboCupEnv.palette, out=torch.zeros(4, 12, 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="dyn must be"):
        pa.render.pixels(w, 16, 12, dyn=torch.zeros(5, 6, 3))
