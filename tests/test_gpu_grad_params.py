"""Gradients with respect to the body parameters on the GPU
(cotix_rollout_backward_ex2 through parallax_amd.rollout_backward(...,
want_params=True) and differentiable_rollout(body_params=...)): against the
torch VJP oracle with the parameters as a leaf (tests/grad_param_cases.py,
the tolerances and conditions of tests/test_grad_params_cpu.py), tape ==
re-play, set_variant(1) == the default tiling, GPU == host emulation bit for
bit, and torch.autograd through the per-env LunarLander."""
import os
import sys

import numpy as np
import pytest

import grad_cases as GC
import grad_param_cases as GPC
import ref_standins as RS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu test without a visible GPU (torch.cuda.is_available() is False)")
    return torch


def _pa_bodies(pa, oracle_bodies):
    out = []
    for b in oracle_bodies:
        parts = []
        for p in b.parts:
            if p.kind == "AABB":
                parts.append(pa.AABB(list(p.lower), list(p.upper)))
            elif p.kind == "Circle":
                parts.append(pa.Circle(p.radius, list(p.position)))
            else:
                parts.append(getattr(pa, p.kind)([list(v) for v in p.vertices_], presorted=True))
        out.append(pa.AnyBody(shape=pa.UniversalShape(*parts), mass=b.mass, inertia=b.inertia,
                              position=list(b.position), velocity=list(b.velocity), angle=b.angle,
                              angular_velocity=b.angular_velocity, elasticity=b.elasticity,
                              friction_coefficient=b.friction_coefficient))
    return out


def _world(torch, name):
    """The case's World on the GPU with the case's state and keys."""
    import parallax_amd as pa
    case, stages, per_env, _ = GPC.cases()[name]
    B = case["S0"].shape[0]
    keys = torch.tensor(np.asarray(case["keys"], np.uint32).view(np.int32), device="cuda")
    if per_env:
        w = pa.World.from_bodies(RS.stack([RS.from_oracle(ob) for ob in case["obs"]]), device="cuda", keys=keys)
        assert w.scene.per_env_params
    else:
        w = pa.World(_pa_bodies(pa, case["make"]()), B, "cuda", keys)
    w.dyn.copy_(torch.tensor(case["S0"], device="cuda").permute(1, 2, 0))
    return w, case, stages


def _run(torch, name, envs_per_wave=0, replay=False):
    import parallax_amd as pa
    w, case, stages = _world(torch, name)
    if envs_per_wave:
        w.set_variant(envs_per_wave)
    ret, saved = pa.rollout_forward(w, torch.tensor(case["actions"], device="cuda"), case["ab"], case["w"],
                                    stages=stages)
    ga, gd, gp = pa.rollout_backward(w, saved, want_dyn0=True, want_params=True, replay=replay)
    pa_, pd_ = pa.rollout_backward(w, saved, want_dyn0=True, replay=replay)
    torch.cuda.synchronize()
    out = [x.cpu().numpy() for x in (ret, ga, gd, gp)]
    # the request changes nothing else
    assert GPC.same_bits(out[1], pa_.cpu().numpy()) and GPC.same_bits(out[2], pd_.cpu().numpy())
    return out


_RUNS = {}


def _default_run(torch, name):
    if name not in _RUNS:
        _RUNS[name] = _run(torch, name)
    return _RUNS[name]


NAMES = list(GPC.cases())


@pytest.mark.parametrize("name", NAMES)
def test_grad_params_vs_oracle(torch_cuda, name):
    case = GPC.cases()[name][0]
    orc = GPC.oracle_of(name, case)
    GPC.check_conditions(name, orc)
    ret, ga, gd, gp = _default_run(torch_cuda, name)
    assert gp.shape == (case["S0"].shape[1], 4, case["S0"].shape[0])
    for e in orc:
        r, oga, ogS, ogp = orc[e]
        same = (np.isnan(ret[e]) and np.isnan(r)) or np.float32(ret[e]).view(np.uint32) == np.float32(r).view(
            np.uint32)
        assert same, (e, ret[e], r)
        ok, msg = GC.close(gp[:, :, e], ogp, case["tol"], case["name"] + "_params_gpu")
        assert ok, "env %d grad_params: %s\n%s\n%s" % (e, msg, gp[:, :, e], ogp)
        ok, msg = GC.close(ga[:, e], oga, case["tol"])
        assert ok, "env %d grad_action: %s" % (e, msg)
        if np.all(ogp == 0):
            assert np.array_equal(gp[:, :, e].view(np.uint32), np.zeros((gp.shape[0], 4), np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_tape_equals_replay(torch_cuda, name):
    a, b = _default_run(torch_cuda, name), _run(torch_cuda, name, replay=True)
    for x, y, what in zip(a, b, ("ret", "grad_action", "grad_dyn0", "grad_params")):
        assert GPC.same_bits(x, y), what


@pytest.mark.parametrize("name", NAMES)
def test_one_env_per_wave_equals_default_tiling(torch_cuda, name):
    """set_variant(1): the generic one-env-per-wave programs against the
    default tiling (RoboCup's and the box world's specializations there)."""
    a, b = _default_run(torch_cuda, name), _run(torch_cuda, name, envs_per_wave=1)
    for x, y, what in zip(a, b, ("ret", "grad_action", "grad_dyn0", "grad_params")):
        assert GPC.same_bits(x, y), what


@pytest.mark.parametrize("name", ["box6x32", "lunar4x8"])
def test_gpu_equals_emulation(torch_cuda, name):
    sys.path.insert(0, os.path.join(HERE, "emu"))
    import emu
    import emu_gradp
    from test_grad_params_cpu import emu_run
    lib = emu_gradp.load()
    case, stages, per_env, _ = GPC.cases()[name]
    want = emu_run(emu, emu_gradp, lib, case, stages, per_env, 4)[:4]
    for x, y, what in zip(_default_run(torch_cuda, name), want, ("ret", "grad_action", "grad_dyn0", "grad_params")):
        assert GPC.same_bits(x, y), what


def test_autograd_body_params(torch_cuda):
    """differentiable_rollout(body_params=theta) on the per-env LunarLander
    (B 4, T 8): theta.grad is grad_params weighted by the incoming cotangent,
    as [B, n_bodies, 4]; the actions' gradient is unchanged; a shared-scene
    tensor that differs from the scene's constants is refused."""
    torch = torch_cuda
    import parallax_amd as pa
    name = "lunar_penv4x8"
    ret0, ga0, gd0, gp0 = _default_run(torch, name)
    w, case, stages = _world(torch, name)
    theta = w.body_params().clone().requires_grad_(True)
    acts = torch.tensor(case["actions"], device="cuda", requires_grad=True)
    ret = pa.differentiable_rollout(w, acts, case["ab"], case["w"], stages=stages, body_params=theta)
    g_ret = torch.tensor([1.0, -2.0, 0.5, 3.0], device="cuda")
    (ret * g_ret).sum().backward()
    torch.cuda.synchronize()
    assert GPC.same_bits(ret.detach().cpu().numpy(), ret0)
    want = (torch.tensor(gp0) * g_ret.cpu()[None, None, :]).permute(2, 0, 1).numpy()
    assert tuple(theta.grad.shape) == (4, 4, 4) and GPC.same_bits(theta.grad.cpu().numpy(), want)
    assert GPC.same_bits(acts.grad.cpu().numpy(), (torch.tensor(ga0) * g_ret.cpu()[None, :, None]).numpy())
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    shared, _, _ = _world(torch, "box5x16")
    with pytest.raises(ValueError, match="bit for bit"):
        pa.differentiable_rollout(shared, torch.zeros(2, 5, 2, device="cuda"),
                                  body_params=shared.body_params() * 1.5)
    # the shared scene's own constants pass: the gradient is the sum over envs
    sp = shared.body_params().clone().requires_grad_(True)
    c = GPC.cases()["box5x16"][0]
    r = pa.differentiable_rollout(shared, torch.tensor(c["actions"], device="cuda"), c["ab"], c["w"],
                                  stages=GPC.BOX_STAGES, body_params=sp)
    r.sum().backward()
    gp5 = _default_run(torch, "box5x16")[3].astype(np.float64).sum(axis=2)  # (the device's sum order is its own)
    np.testing.assert_allclose(sp.grad.cpu().numpy(), gp5, rtol=1e-5, atol=1e-6 * np.abs(gp5).max())
    assert np.abs(gp5).max() > 0
