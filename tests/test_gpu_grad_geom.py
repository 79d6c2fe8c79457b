"""Gradients with respect to the shape geometry on the GPU
(cotix_rollout_backward_ex3 through parallax_amd.rollout_backward(...,
want_geom=True) and differentiable_rollout(geometry=...)): against the torch
VJP oracle with the geometry row as a leaf (tests/grad_geom_cases.py, the
tolerances and conditions of tests/test_grad_geom_cpu.py), tape == re-play,
set_variant(1) == the default tiling, GPU == host emulation bit for bit, and
torch.autograd through per-env and shared geometry."""
import os
import sys

import numpy as np
import pytest

import grad_cases as GC
import grad_geom_cases as GGC
import ref_standins as RS
from test_gpu_grad_params import _pa_bodies

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WHAT = ("ret", "grad_action", "grad_dyn0", "grad_geom")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu test without a visible GPU (torch.cuda.is_available() is False)")
    return torch


def _world(torch, name):
    """The case's World on the GPU with the case's state and keys."""
    import parallax_amd as pa
    case, stages, per_env, _ = GGC.cases()[name]
    B = case["S0"].shape[0]
    keys = torch.tensor(np.asarray(case["keys"], np.uint32).view(np.int32), device="cuda")
    if per_env:
        w = pa.World.from_bodies(RS.stack([RS.from_oracle(ob) for ob in case["obs"]]), device="cuda", keys=keys)
        assert w.scene.per_env_params and w.geom.dim() == 2
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
    ga, gd, gg = pa.rollout_backward(w, saved, want_dyn0=True, want_geom=True, replay=replay)
    pa_, pd_ = pa.rollout_backward(w, saved, want_dyn0=True, replay=replay)
    torch.cuda.synchronize()
    out = [x.cpu().numpy() for x in (ret, ga, gd, gg)]
    # the request changes nothing else (phase GE keeps the poses of the GJK / EPA scenes)
    assert GGC.same_bits(out[1], pa_.cpu().numpy()) and GGC.same_bits(out[2], pd_.cpu().numpy())
    return out


_RUNS = {}


def _default_run(torch, name):
    if name not in _RUNS:
        _RUNS[name] = _run(torch, name)
    return _RUNS[name]


NAMES = list(GGC.cases())


@pytest.mark.parametrize("name", NAMES)
def test_grad_geom_vs_oracle(torch_cuda, name):
    case = GGC.cases()[name][0]
    orc = GGC.oracle_of(name, case)
    GGC.check_conditions(name, orc)
    ret, ga, gd, gg = _default_run(torch_cuda, name)
    assert gg.shape == (orc[0][3].size, case["S0"].shape[0])
    pads = GGC.pad_words(case)
    for e in orc:
        r, oga, ogS, ogg = orc[e]
        same = (np.isnan(ret[e]) and np.isnan(r)) or np.float32(ret[e]).view(np.uint32) == np.float32(r).view(
            np.uint32)
        assert same, (e, ret[e], r)
        ok, msg = GC.close(gg[:, e], ogg, GGC.tol_of(name, case), name + "_geom_gpu")
        assert ok, "env %d grad_geom: %s\n%s" % (e, msg, np.stack([gg[:, e], ogg], 1))
        ok, msg = GC.close(ga[:, e], oga, case["tol"])
        assert ok, "env %d grad_action: %s" % (e, msg)
        if np.all(ogg == 0):
            assert not gg[:, e].view(np.uint32).any(), (e, gg[:, e])
        assert not gg[pads, e].view(np.uint32).any(), "a circle's pad word is not an exact zero"


@pytest.mark.parametrize("name", NAMES)
def test_tape_equals_replay(torch_cuda, name):
    a, b = _default_run(torch_cuda, name), _run(torch_cuda, name, replay=True)
    for x, y, what in zip(a, b, WHAT):
        assert GGC.same_bits(x, y), what


@pytest.mark.parametrize("name", NAMES)
def test_one_env_per_wave_equals_default_tiling(torch_cuda, name):
    a, b = _default_run(torch_cuda, name), _run(torch_cuda, name, envs_per_wave=1)
    for x, y, what in zip(a, b, WHAT):
        assert GGC.same_bits(x, y), what


@pytest.mark.parametrize("name", ["box5x16", "lunar4x8", "ball_poly4x8"])
def test_gpu_equals_emulation(torch_cuda, name):
    sys.path.insert(0, os.path.join(HERE, "emu"))
    import emu
    import emu_gradg
    from test_grad_geom_cpu import emu_run
    lib = emu_gradg.load()
    case, stages, per_env, _ = GGC.cases()[name]
    want = emu_run(emu, emu_gradg, lib, case, stages, per_env, 4)[:4]
    for x, y, what in zip(_default_run(torch_cuda, name), want, WHAT):
        assert GGC.same_bits(x, y), what


def test_autograd_geometry_per_env(torch_cuda):
    """differentiable_rollout(geometry=theta) on the per-env LunarLander (B 4,
    T 8): theta.grad is grad_geom weighted by a non-uniform cotangent, as
    [B, GW], bit for bit; finite and nonzero; the actions' gradient is
    unchanged."""
    torch = torch_cuda
    import parallax_amd as pa
    name = "lunar_penv4x8"
    ret0, ga0, gd0, gg0 = _default_run(torch, name)
    w, case, stages = _world(torch, name)
    theta = w.geometry().clone().requires_grad_(True)
    acts = torch.tensor(case["actions"], device="cuda", requires_grad=True)
    ret = pa.differentiable_rollout(w, acts, case["ab"], case["w"], stages=stages, geometry=theta)
    g_ret = torch.tensor([1.0, -2.0, 0.5, 3.0], device="cuda")
    (ret * g_ret).sum().backward()
    torch.cuda.synchronize()
    assert GGC.same_bits(ret.detach().cpu().numpy(), ret0)
    want = (torch.tensor(gg0) * g_ret.cpu()[None, :]).T.numpy()
    assert tuple(theta.grad.shape) == (4, 84) and GGC.same_bits(theta.grad.cpu().numpy(), want)
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert GGC.same_bits(acts.grad.cpu().numpy(), (torch.tensor(ga0) * g_ret.cpu()[None, :, None]).numpy())
    # the guard: geometry written between the forward and the backward
    theta2 = w.geometry().clone().requires_grad_(True)
    w.dyn.copy_(torch.tensor(case["S0"], device="cuda").permute(1, 2, 0))
    r2 = pa.differentiable_rollout(w, acts.detach(), case["ab"], case["w"], stages=stages, geometry=theta2)
    w.geometry()[0, 0] += 0.0
    with pytest.raises(RuntimeError, match="changed between"):
        r2.sum().backward()


def test_autograd_geometry_shared(torch_cuda):
    """On the shared box world theta.grad is the sum over the envs."""
    torch = torch_cuda
    import parallax_amd as pa
    gg5 = _default_run(torch, "box5x16")[3].astype(np.float64).sum(axis=1)  # (the device's sum order is its own)
    shared, c, stages = _world(torch, "box5x16")
    theta = shared.geometry().clone().requires_grad_(True)
    r = pa.differentiable_rollout(shared, torch.tensor(c["actions"], device="cuda"), c["ab"], c["w"], stages=stages,
                                  geometry=theta)
    r.sum().backward()
    torch.cuda.synchronize()
    assert tuple(theta.grad.shape) == (28,)
    np.testing.assert_allclose(theta.grad.cpu().numpy(), gg5, rtol=1e-5, atol=1e-6 * np.abs(gg5).max())
    assert np.abs(gg5).max() > 0


def test_autograd_geometry_with_body_params(torch_cuda):
    """geometry= together with body_params= on the per-env LunarLander: each
    gradient equals that of the separate calls."""
    torch = torch_cuda
    import parallax_amd as pa
    name = "lunar_penv4x8"
    g_ret = torch.tensor([1.0, -2.0, 0.5, 3.0], device="cuda")

    def run(with_p, with_g):
        w, case, stages = _world(torch, name)
        th_p = w.body_params().clone().requires_grad_(True) if with_p else None
        th_g = w.geometry().clone().requires_grad_(True) if with_g else None
        acts = torch.tensor(case["actions"], device="cuda", requires_grad=True)
        ret = pa.differentiable_rollout(w, acts, case["ab"], case["w"], stages=stages, body_params=th_p,
                                        geometry=th_g)
        (ret * g_ret).sum().backward()
        torch.cuda.synchronize()
        return [None if x is None else x.grad.cpu().numpy() for x in (acts, th_p, th_g)]

    both, only_p, only_g = run(True, True), run(True, False), run(False, True)
    assert GGC.same_bits(both[0], only_p[0]) and GGC.same_bits(both[0], only_g[0])
    assert both[1].shape == (4, 4, 4) and GGC.same_bits(both[1], only_p[1])
    assert both[2].shape == (4, 84) and GGC.same_bits(both[2], only_g[2])
    assert np.abs(both[1]).max() > 0 and np.abs(both[2]).max() > 0
