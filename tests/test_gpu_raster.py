"""Pixel observations on the MI355X (cotix_rasterize):
every case of tests/raster_cases.py through the library equals the oracle
restatement byte for byte, in both decompositions (a workgroup or a wave per
env); larger batches and images equal the host checker, which
tests/test_raster_cpu.py pins to the oracle."""
import ctypes

import numpy as np
import pytest

import raster_cases as RC

pytestmark = pytest.mark.gpu
FORMS = ("0", "1")  # COTIX_RASTER_WAVE_PER_ENV: the workgroup's four waves per env (default), one wave per env


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu test without a visible GPU (torch.cuda.is_available() is False)")
    return torch


def _camera(pa, cam):
    return pa.Camera(cam.center, cam.half_extent, cam.follow_body, cam.follow_angle)


def _world(torch, pa, envs):
    """A World holding a batch of oracle envs: the scene of env 0, the state
    and (shared or per-env) geometry rows of tests/raster_cases.py."""
    from test_gpu_parity import _pa_bodies
    B = len(envs)
    w = pa.World(_pa_bodies(pa, envs[0]), B, "cuda", torch.zeros(B, 2, dtype=torch.int32))
    (_, _, _, goff), words = RC.part_table(envs[0])
    assert words == w.scene.geom_floats
    off, cnt = ctypes.c_int(), ctypes.c_int()
    for p, g in enumerate(goff):  # the library's part offsets are the table's
        pa._ffi.check(pa._ffi.lib.cotix_scene_part_geom(w.scene.handle, p, ctypes.byref(off), ctypes.byref(cnt)))
        assert off.value == g
    dyn, geom = RC.batch_arrays(envs)
    w.dyn.copy_(torch.from_numpy(dyn))
    w.geom = torch.from_numpy(geom).cuda().contiguous()
    w.geom_stride = 0 if geom.ndim == 1 else geom.shape[1]
    return w


def _pixels(torch, pa, envs, W, H, cam, **kw):
    out = pa.render.pixels(_world(torch, pa, envs), W, H, _camera(pa, cam), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(RC.CASES))
def test_device_equals_oracle(torch_cuda, monkeypatch, name, form):
    """B = 5: ragged, not a multiple of 4; envs differ by perturbed state or keys."""
    import parallax_amd as pa
    monkeypatch.setenv("COTIX_RASTER_WAVE_PER_ENV", form)
    c = RC.CASES[name]
    want = RC.oracle_batch(name, 5)
    assert len(set(want.ravel().tolist())) > 1  # (per case and env 0: tests/test_raster_cpu.py)
    got = _pixels(torch_cuda, pa, RC.case_envs(name, 5), c.W, c.H, c.cam)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), "%s: %d pixels differ" % (name, int((got != want).sum()))


def _many(name, B):
    """B envs from the case's first 5 (the oracle's steps are slow), moved apart."""
    return [RC._nudged(RC.CASES[name].make(e % 5), e // 5) for e in range(B)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["robocup_reset", "lunar_egocentric"])
def test_many_groups_tiny_image(torch_cuda, monkeypatch, name, form):
    """B = 130 at 8 x 4: many groups, 8 pixel quads per env, most lanes idle."""
    import parallax_amd as pa
    monkeypatch.setenv("COTIX_RASTER_WAVE_PER_ENV", form)
    envs, cam = _many(name, 130), RC.CASES[name].cam
    want = RC.host_image(envs, 8, 4, cam)
    assert len(set(want.ravel().tolist())) > 1
    assert np.array_equal(_pixels(torch_cuda, pa, envs, 8, 4, cam), want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["robocup_goal_zoom", "lunar_egocentric"])
def test_larger_image(torch_cuda, monkeypatch, name, form):
    """B = 3 at 64 x 48 (768 quads: several passes of either group size)
    against the host checker -- pinned to the oracle on the CPU; the scalar
    oracle would take too long here."""
    import parallax_amd as pa
    monkeypatch.setenv("COTIX_RASTER_WAVE_PER_ENV", form)
    envs, cam = RC.case_envs(name, 3), RC.CASES[name].cam
    want = RC.host_image(envs, 64, 48, cam)
    assert len(set(want.ravel().tolist())) > 1
    assert np.array_equal(_pixels(torch_cuda, pa, envs, 64, 48, cam), want)


@pytest.mark.parametrize("form", FORMS)
def test_rgb_planar_is_palette_of_ids(torch_cuda, monkeypatch, form):
    import parallax_amd as pa
    monkeypatch.setenv("COTIX_RASTER_WAVE_PER_ENV", form)
    torch = torch_cuda
    for name, pal in (("robocup_reset", pa.RoboCupEnv.palette),
                      ("lunar_reset", [(9, 8, 7), (255, 255, 255), (250, 0, 1), (2, 251, 3), (4, 5, 252)])):
        c = RC.CASES[name]
        envs = RC.case_envs(name, 5)
        ids = _pixels(torch, pa, envs, c.W, c.H, c.cam)
        rgb = _pixels(torch, pa, envs, c.W, c.H, c.cam, palette=pal)
        assert rgb.shape == (5, 3, c.H, c.W)
        assert np.array_equal(rgb, np.array(pal, np.uint8)[ids].transpose(0, 3, 1, 2))
        assert np.array_equal(rgb, RC.host_image(envs, c.W, c.H, c.cam, palette=np.array(pal, np.uint8)))


def test_out_is_reused(torch_cuda):
    import parallax_amd as pa
    torch = torch_cuda
    c = RC.CASES["robocup_reset"]
    w = _world(torch, pa, RC.case_envs("robocup_reset", 5))
    out = torch.full((5, c.H, c.W), 77, dtype=torch.uint8, device="cuda")
    got = pa.render.pixels(w, c.W, c.H, out=out)
    assert got is out and got.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), RC.oracle_batch("robocup_reset", 5))
    rgb = torch.empty(5, 3, c.H, c.W, dtype=torch.uint8, device="cuda")
    assert pa.render.pixels(w, c.W, c.H, palette=pa.RoboCupEnv.palette, out=rgb) is rgb


def test_batched_env_pixels(torch_cuda):
    """BatchedEnv.pixels after env.step(3) is render.pixels of its world (the
    perturbed RoboCup batch: env 0 NaN from step 1, the others' balls apart)."""
    import parallax_amd as pa
    torch = torch_cuda
    env = pa.BatchedEnv(pa.RoboCupEnv(batch=5, device="cuda", perturb=True))
    env.reset()
    env.step(3)
    cam = pa.Camera(half_extent=(5.6, 4.2))
    ids = env.pixels(32, 24, cam)
    assert ids.shape == (5, 24, 32) and ids.dtype == torch.uint8 and ids.device.type == "cuda"
    assert torch.equal(ids, pa.render.pixels(env.world, 32, 24, cam))
    assert len(ids.unique()) > 1
    rgb = env.pixels(32, 24, cam, rgb=True)
    pal = torch.tensor(env.scenario.palette, dtype=torch.uint8, device="cuda")
    assert torch.equal(rgb, pal[ids.long()].permute(0, 3, 1, 2))
    ll = pa.BatchedEnv(pa.LunarLander(batch=5, device="cuda"))
    ego = pa.Camera(half_extent=(1.0, 0.75), follow_body=0, follow_angle=True)
    ll.step(5)
    img = ll.pixels(16, 12, ego)
    # the lander in its own frame: its area 2.1675 over the pixel's 1/64 is 139 pixels, give or take half the
    # 46 pixels its 5.8-long outline crosses
    assert all(139 - 23 <= n <= 139 + 23 for n in (img == 1).sum(dim=(1, 2)).tolist())
