"""Range-sensor observations on the MI355X (cotix_raycast, DESIGN.md section
17): every case of tests/raycast_cases.py through render.rays equals the
oracle restatement bit for bit at B = 5 (a partial workgroup); the NULL hit,
out= tensors and BatchedEnv.rays after real steps are held to the host
checker, which tests/test_raycast_cpu.py pins to the oracle."""
import numpy as np
import pytest

import raster_cases
import raycast_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu test without a visible GPU (torch.cuda.is_available() is False)")
    return torch


def _sensor(pa, s):
    return pa.RaySensor(s.body, s.offset, s.follow_angle, s.max_range, s.ignore)


def _world(torch, pa, envs):
    from test_gpu_raster import _world as world  # a World holding a batch of oracle envs
    return world(torch, pa, envs)


def _rays(torch, pa, name, **kw):
    c = RC.CASES[name]
    w = _world(torch, pa, RC.case_envs(name))
    dirs = torch.from_numpy(c.dirs).cuda()
    return w, dirs, pa.render.rays(w, _sensor(pa, c.sensor), dirs, **kw)


@pytest.mark.parametrize("name", list(RC.CASES))
def test_device_equals_oracle(torch_cuda, name):
    """B = 5: not a multiple of the 4 envs of a workgroup; envs differ by perturbed state or keys."""
    import parallax_amd as pa
    torch = torch_cuda
    c = RC.CASES[name]
    want_d, want_h = RC.oracle_batch(name)
    if c.ids is not None:  # (the cases' contents: tests/test_raycast_cpu.py)
        assert set(want_h.ravel().tolist()) == c.ids
    hit = torch.full((RC.B, len(c.dirs)), 0xA5, dtype=torch.uint8, device="cuda")
    _, _, (dist, got_hit) = _rays(torch, pa, name, hit_out=hit)
    torch.cuda.synchronize()
    assert got_hit is hit and dist.dtype == torch.float32 and tuple(dist.shape) == want_d.shape
    got_d, got_h = dist.cpu().numpy(), hit.cpu().numpy()
    diff = (RC.bits(got_d) != RC.bits(want_d)) | (got_h != want_h)
    assert not diff.any(), "%s: %d rays differ" % (name, int(diff.sum()))


@pytest.mark.parametrize("name", ["lunar_down", "robocup_fixed"])
def test_null_hit_leaves_dist_unchanged(torch_cuda, name):
    import parallax_amd as pa
    torch = torch_cuda
    dist, hit = _rays(torch, pa, name)[2]
    assert hit is None
    torch.cuda.synchronize()
    assert np.array_equal(RC.bits(dist.cpu().numpy()), RC.bits(RC.oracle_batch(name)[0]))


def test_out_tensors_are_written_in_place(torch_cuda):
    import parallax_amd as pa
    torch = torch_cuda
    name = "robocup_goals"
    c = RC.CASES[name]
    out = torch.full((RC.B, len(c.dirs)), -7.0, dtype=torch.float32, device="cuda")
    hit = torch.full((RC.B, len(c.dirs)), 77, dtype=torch.uint8, device="cuda")
    w, dirs, (d, h) = _rays(torch, pa, name, out=out, hit_out=hit)
    assert d is out and h is hit
    want_d, want_h = RC.oracle_batch(name)
    assert np.array_equal(RC.bits(out.cpu().numpy()), RC.bits(want_d)) and np.array_equal(hit.cpu().numpy(), want_h)
    # dyn=: another state tensor in the world's layout (every body moved 0.25 to the right: the same readings
    # from the ball's sensor but for rounding, other ones from a world-fixed sensor)
    moved = w.dyn.clone()
    moved[:, 0, :] += 0.25
    fixed = pa.RaySensor(offset=(-1.0, 0.02), max_range=6.0, ignore=(0, 1))
    d0, _ = pa.render.rays(w, fixed, dirs)
    d1, _ = pa.render.rays(w, fixed, dirs, dyn=moved)
    assert not torch.equal(d0, d1)
    assert torch.equal(out, torch.from_numpy(want_d).cuda())  # and out is not touched by later calls


def test_batched_env_rays_after_real_steps(torch_cuda):
    """BatchedEnv.rays after two env.step calls on RoboCup equals the host
    checker on the state read back (the perturbed batch: degenerate envs are
    NaN from step 1, their NaN bodies invisible)."""
    import parallax_amd as pa
    torch = torch_cuda
    env = pa.BatchedEnv(pa.RoboCupEnv(batch=RC.B, device="cuda", perturb=True))
    env.reset()
    env.step(1)
    env.step(1)
    dirs = RC.fan(80)
    dyn = env.world.dyn.cpu().numpy()  # [nb, 6, B]
    assert dyn.shape == (5, 6, RC.B)
    envs = []
    for e in range(RC.B):
        bodies = raster_cases.P.robocup_bodies()
        for k, b in enumerate(bodies):
            b.set_dyn(dyn[k, :, e])
        envs.append(bodies)
    # from the ball (in an env whose ball is NaN by now every ray reports max_range, 0), and from a fixed point
    seen = set()
    for sensor in (RC.Sensor(body=4, max_range=5.0, ignore=(4,)), RC.Sensor(offset=(0.5, -0.25), max_range=8.0)):
        hit = torch.empty(RC.B, 80, dtype=torch.uint8, device="cuda")
        dist, got = env.rays(_sensor(pa, sensor), torch.from_numpy(dirs).cuda(), hit_out=hit)
        assert got is hit and tuple(dist.shape) == (RC.B, 80) and dist.device.type == "cuda"
        want_d, want_h = RC.host_rays(envs, sensor, dirs)
        seen |= set(want_h.ravel().tolist())
        assert np.array_equal(RC.bits(dist.cpu().numpy()), RC.bits(want_d))
        assert np.array_equal(hit.cpu().numpy(), want_h)
    assert len(seen) > 1
