"""Range-sensor gradients on the MI355X (cotix_raycast_backward, DESIGN.md
section 18): render.rays_backward equals the host checker bit for bit on every
case of tests/raygrad_cases.py at B = 5 (a partial workgroup), with both outputs
and with either alone, and overwrites every word; differentiable_rays is
render.rays forward and rays_backward backward; BatchedEnv.rays_backward after
real steps.  tests/test_raygrad_cpu.py pins the host checker to a float64
vector-Jacobian product."""
import numpy as np
import pytest

import raster_cases
import raygrad_cases as GC

RC = GC.RC
pytestmark = pytest.mark.gpu
B = GC.B


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu test without a visible GPU (torch.cuda.is_available() is False)")
    return torch


@pytest.fixture(scope="module")
def host():
    """The host checker as build() left it: a missing library fails the test."""
    return GC.load_host()


def _sensor(pa, s):
    return pa.RaySensor(s.body, s.offset, s.follow_angle, s.max_range, s.ignore)


def _world(torch, pa, envs):
    from test_gpu_raster import _world as world  # a World holding a batch of oracle envs
    return world(torch, pa, envs)


def _setup(torch, pa, name):
    c = GC.CASES[name]
    w = _world(torch, pa, GC.envs_of(name))
    g = torch.from_numpy(GC.cotangent(name).copy()).cuda()
    return c, w, _sensor(pa, c.sensor), torch.from_numpy(c.dirs).cuda(), g


def _same(t, a):
    return np.array_equal(GC.bits(t.cpu().numpy()), GC.bits(a))


@pytest.mark.parametrize("name", list(GC.CASES))
def test_device_equals_host_checker(torch_cuda, host, name):
    """80 rays are two chunks, the second partial; the LunarLander cases have more than 64 output slots (two
    slot passes), per-env rows and follow_angle; adversarial and robocup_2_steps hold NaNs."""
    import parallax_amd as pa
    torch = torch_cuda
    c, w, sensor, dirs, g = _setup(torch, pa, name)
    want_d, want_g = GC.host_vjp(GC.envs_of(name), c.sensor, c.dirs, GC.cotangent(name), lib=host)
    gd, gg = pa.render.rays_backward(w, sensor, dirs, g, want_geom=True)
    torch.cuda.synchronize()
    assert tuple(gd.shape) == want_d.shape and tuple(gg.shape) == want_g.shape == (w.scene.geom_part_words, B)
    assert _same(gd, want_d), "%s: %d g_dyn words differ" % (name, int((GC.bits(gd.cpu().numpy()) !=
                                                                         GC.bits(want_d)).sum()))
    assert _same(gg, want_g), "%s: %d g_geom words differ" % (name, int((GC.bits(gg.cpu().numpy()) !=
                                                                          GC.bits(want_g)).sum()))
    only_d = pa.render.rays_backward(w, sensor, dirs, g)
    only_g = pa.render.rays_backward(w, sensor, dirs, g, want_dyn=False, want_geom=True)
    assert only_d[1] is None and only_g[0] is None
    assert _same(only_d[0], want_d) and _same(only_g[1], want_g)


@pytest.mark.parametrize("name", ["lunar_down", "robocup_2_steps", "one_ray"])
def test_every_word_is_overwritten(torch_cuda, host, name, monkeypatch):
    """The outputs start as a sentinel (torch.empty replaced by a filling one for the call)."""
    import parallax_amd as pa
    torch = torch_cuda
    c, w, sensor, dirs, g = _setup(torch, pa, name)
    want_d, want_g = GC.host_vjp(GC.envs_of(name), c.sensor, c.dirs, GC.cotangent(name), lib=host)
    made = []

    def filled(*shape, **kw):
        t = torch.full(shape[0] if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape, -77.0, **kw)
        made.append(t)
        return t

    monkeypatch.setattr(pa.render.torch, "empty", filled)
    gd, gg = pa.render.rays_backward(w, sensor, dirs, g, want_geom=True)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(made) == 2 and made[0] is gd and made[1] is gg
    assert _same(gd, want_d) and _same(gg, want_g)
    assert not (gd == -77.0).any() and not (gg == -77.0).any()


@pytest.mark.parametrize("name", ["lunar_reset", "robocup_fixed", "dup_vertex"])
def test_differentiable_rays(torch_cuda, name):
    """lunar_reset: per-env geometry rows (the gradient is g_geom.T); the others: shared (g_geom.sum(1))."""
    import parallax_amd as pa
    torch = torch_cuda
    c, w, sensor, dirs, g = _setup(torch, pa, name)
    want_dist, _ = pa.render.rays(w, sensor, dirs)
    g_dyn, g_geom = pa.render.rays_backward(w, sensor, dirs, g, want_geom=True)
    dyn = w.dyn.clone().requires_grad_(True)
    geometry = w.geometry().clone().requires_grad_(True)
    hit = torch.zeros(B, len(c.dirs), dtype=torch.uint8, device="cuda")
    dist = pa.differentiable_rays(w, sensor, dirs, dyn=dyn, geometry=geometry, hit_out=hit)
    assert dist.requires_grad and torch.equal(dist.view(torch.int32), want_dist.view(torch.int32))
    assert hit.any()
    # stepping the world between forward and backward changes nothing: the graph holds its own state
    before = w.dyn.clone()
    w.dyn.add_(0.25)
    dist.backward(g)
    assert torch.equal(dyn.grad.view(torch.int32), g_dyn.view(torch.int32))
    per_env = w.geom.dim() == 2
    assert per_env == (name == "lunar_reset")
    want = g_geom.T.contiguous() if per_env else g_geom.sum(dim=1)
    assert geometry.grad.shape == geometry.shape and torch.equal(geometry.grad.view(torch.int32),
                                                                 want.view(torch.int32))
    assert geometry.grad.abs().max() > 0 and dyn.grad.abs().max() > 0
    w.dyn.copy_(before)
    # the state alone, the default state (no gradient asked: none computed), and a loss as a user writes it
    dyn2 = w.dyn.clone().requires_grad_(True)
    (pa.differentiable_rays(w, sensor, dirs, dyn=dyn2) * g).sum().backward()
    assert torch.equal(dyn2.grad.view(torch.int32), g_dyn.view(torch.int32))
    assert not pa.differentiable_rays(w, sensor, dirs).requires_grad


def test_differentiable_rays_refuses_changed_geometry(torch_cuda):
    import parallax_amd as pa
    torch = torch_cuda
    c, w, sensor, dirs, g = _setup(torch, pa, "dup_vertex")
    geometry = w.geometry().clone().requires_grad_(True)
    dist = pa.differentiable_rays(w, sensor, dirs, geometry=geometry)
    w.geometry().mul_(1.0)  # a write, whatever it writes
    with pytest.raises(RuntimeError, match="geometry changed"):
        dist.backward(g)
    assert geometry.grad is None


def test_batched_env_rays_backward_after_real_steps(torch_cuda, host):
    """BatchedEnv.rays_backward after two env.step calls on perturbed RoboCup equals the host checker on the
    state read back; degenerate envs are NaN by then and their rows zeros."""
    import parallax_amd as pa
    torch = torch_cuda
    env = pa.BatchedEnv(pa.RoboCupEnv(batch=B, device="cuda", perturb=True))
    env.reset()
    env.step(1)
    env.step(1)
    dirs = GC.fan(80)
    dyn = env.world.dyn.cpu().numpy()
    assert dyn.shape == (5, 6, B)
    envs = []
    for e in range(B):
        bodies = raster_cases.P.robocup_bodies()
        for k, b in enumerate(bodies):
            b.set_dyn(dyn[k, :, e])
        envs.append(bodies)
    nan_ball = [e for e in range(B) if np.isnan(dyn[4, 0, e])]
    g = np.random.default_rng(7).uniform(-1.0, 1.0, (B, 80)).astype(GC.F)
    seen = 0.0
    for sensor in (GC.Sensor(body=4, max_range=5.0, ignore=(4,)), GC.Sensor(offset=(0.5, -0.25), max_range=8.0)):
        gd, gg = env.rays_backward(_sensor(pa, sensor), torch.from_numpy(dirs).cuda(), torch.from_numpy(g).cuda(),
                                   want_geom=True)
        want_d, want_g = GC.host_vjp(envs, sensor, dirs, g, lib=host)
        assert _same(gd, want_d) and _same(gg, want_g)
        seen = max(seen, float(np.abs(np.nan_to_num(want_d)).max()), float(np.abs(np.nan_to_num(want_g)).max()))
        if sensor.body == 4:
            for e in nan_ball:
                assert not GC.bits(want_d[:, :, e]).any() and not GC.bits(want_g[:, e]).any()
    assert np.isnan(dyn).any() and seen > 0
