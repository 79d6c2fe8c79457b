"""The differentiable eval on the GPU, through the C ABI and the Python layer
(parallax_amd.eval_grad): the saving forward == env.eval bit for bit, the
gradients against the torch-f32 oracle (tests/eval_grad_cases.py) at the
project's gradient tolerances, a ragged batch, the generic kernel == the
specialised one, GPU == host emulation bit for bit on a larger batch with a
partly filled last workgroup, and torch.autograd through differentiable_eval."""
import os
import sys

import numpy as np
import pytest

import eval_device_cases as EDC
import eval_grad_cases as EGC
import grad_cases as GC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu test without a visible GPU (torch.cuda.is_available() is False)")
    return torch


def setup(name):
    from test_eval_grad_cpu import setup as cpu_setup
    return cpu_setup(name)


def orc_of(name):
    from test_eval_grad_cpu import orc_of as cpu_orc
    return cpu_orc(name)


def make_env(torch, name, envs=None, specialize=None):
    """(env, case) of a named case on the GPU; envs: a slice of the case's batch."""
    import parallax_amd as pa
    from parallax_amd import envs as E
    from test_gpu_grad_params import _pa_bodies
    case, j, c, _, _, nfe, wfe, period, stages = setup(name)
    S0, keys = case["S0"], np.asarray(case["keys"], np.uint32)
    if envs is not None:
        S0, keys = S0[envs], keys[envs]
    B = S0.shape[0]
    w = pa.World(_pa_bodies(pa, case["make"]()), B, "cuda", torch.tensor(keys.view(np.int32), device="cuda"))
    w.dyn.copy_(torch.tensor(np.ascontiguousarray(S0.transpose(1, 2, 0)), device="cuda"))
    if specialize is not None:
        w.set_variant(4, bool(specialize))
    state = E.WorldState(w.dyn.clone(), w.keys.clone(), w.err.clone())
    return E.AbstractEnvironment(E.PhysicsWorld(w, stages), state, c, j), (nfe, wfe, period)


def run(torch, env, args):
    import parallax_amd as pa
    nfe, wfe, period = args
    out, reward, saved = pa.eval_forward(env, period, nfe, wfe)
    gc, gd, gv = pa.eval_backward(saved)
    torch.cuda.synchronize()
    return dict(dyn=out.state.dyn.cpu().numpy(), keys=out.state.keys.cpu().numpy().view(np.uint32),
                err=out.state.err.cpu().numpy(), reward=reward.cpu().numpy(), gc=gc.cpu().numpy(),
                gd=gd.cpu().numpy(), gv=gv.cpu().numpy(), rec=saved["rec"].cpu().numpy().view(np.uint32))


def check_vs_oracle(got, orc, tol, tag, envs=None):
    from test_eval_grad_cpu import check_vs_oracle as chk
    chk(got, orc, tol, tag, envs)


@pytest.mark.parametrize("name", ["x_done", "multi", "piecewise", "lunar", "goal"])
def test_forward_equals_eval_and_gradients_vs_oracle(torch_cuda, name):
    torch = torch_cuda
    env, args = make_env(torch, name)
    got = run(torch, env, args)
    nfe, wfe, period = args
    out, reward = env.eval(period, nfe, wfe)  # the fused cotix_eval on the same inputs
    torch.cuda.synchronize()
    assert EGC.same_bits(got["dyn"], out.state.dyn.cpu().numpy())
    assert np.array_equal(got["keys"], out.state.keys.cpu().numpy().view(np.uint32))
    assert np.array_equal(got["err"], out.state.err.cpu().numpy())
    assert EGC.same_bits(got["reward"], reward.cpu().numpy())
    check_vs_oracle(got, orc_of(name), setup(name)[0]["tol"], "gpu_" + name)


@pytest.mark.parametrize("name", ["x_done", "piecewise"])
def test_ragged_batch(torch_cuda, name):
    """Envs 0..5 sliced out of the 8-env case: a partly filled wave."""
    torch = torch_cuda
    envs = list(range(6))
    env, args = make_env(torch, name, envs=envs)
    check_vs_oracle(run(torch, env, args), orc_of(name), GC.ANALYTIC_TOL, "gpu_%s_ragged" % name, envs=envs)


@pytest.mark.parametrize("name", ["piecewise", "goal"])
def test_generic_equals_specialised(torch_cuda, name):
    """The box world's and RoboCup's specialised kernels (4 envs per wave)
    against the generic kernel, bit for bit."""
    torch = torch_cuda
    a = run(torch, *make_env(torch, name, specialize=1))
    b = run(torch, *make_env(torch, name, specialize=0))
    for k in a:
        ok = EGC.same_bits(a[k], b[k]) if a[k].dtype == np.float32 else np.array_equal(a[k], b[k])
        assert ok, k


def test_gpu_equals_emulation_1030_envs(torch_cuda):
    """RoboCup, 1030 perturbed envs (a partly filled last workgroup), the goal
    judge, 3 NFEs x 8: reward, grad_control, grad_dyn0, grad_dv and the judge
    record equal the host emulation's bit for bit; finite and NaN envs both
    occur."""
    torch = torch_cuda
    sys.path.insert(0, os.path.join(HERE, "emu"))
    import emu
    import emu_evalgrad
    import parallax_amd as pa
    from parallax_amd import envs as E
    from cotix_oracle import physics as P
    B, nfe, wfe, period = 1030, 3, 8, 0.24
    lib = emu_evalgrad.load()
    scen = pa.RoboCupEnv(batch=B, device="cuda", perturb=True)
    w = scen.world
    j, c = EDC.device("goal", 4)
    dyn = np.ascontiguousarray(w.dyn.cpu().numpy())
    keys = np.ascontiguousarray(w.keys.cpu().numpy().view(np.uint32))
    state = E.WorldState(w.dyn.clone(), w.keys.clone(), w.err.clone())
    env = E.AbstractEnvironment(E.PhysicsWorld(w), state, c, j)
    got = run(torch, env, (nfe, wfe, period))
    h, geom = emu.oracle_scene(lib, P.robocup_bodies())
    err, rw, fin = np.zeros(B, np.uint32), np.zeros(B, np.float32), np.zeros(B, np.uint32)
    dt = float(F(F(period / nfe) / F(float(wfe))))
    sd, sk, tp, rec = emu_evalgrad.eval_rollout(lib, h, dyn, keys, err, geom, 0, nfe, wfe, dt, 1 | 4 | 16, j.c_struct(),
                                                c.c_struct(), rw, fin)
    gc, gd, gv = emu_evalgrad.eval_backward(lib, h, sd, sk, tp, rec, geom, 0, nfe, wfe, dt, 1 | 4 | 16, j.c_struct(),
                                            c.c_struct())
    assert EGC.same_bits(got["dyn"], dyn) and EGC.same_bits(got["reward"], rw)
    assert np.array_equal(got["rec"], rec)
    assert EGC.same_bits(got["gc"], gc), "grad_control"
    assert EGC.same_bits(got["gd"], gd), "grad_dyn0"
    assert EGC.same_bits(got["gv"], gv), "grad_dv"
    nan_env = np.isnan(gc).any(axis=0)
    assert nan_env.any() and (~nan_env).any(), (int(nan_env.sum()), B)
    assert np.any(gc[:, ~nan_env] != 0)


def test_differentiable_eval_autograd(torch_cuda):
    """differentiable_eval(...).sum().backward(): control_params.grad is the sum
    over the envs of eval_backward's columns, dyn0.grad its grad_dyn0, and two
    entries match a central difference of env.eval's own summed reward on the
    finite box batch (x_done; h = 1e-3, 2e-3 (1 + |fd|): the bar of the oracle's
    own finite-difference check)."""
    torch = torch_cuda
    import parallax_amd as pa
    from parallax_amd import envs as E
    env, (nfe, wfe, period) = make_env(torch, "x_done")
    theta = env.control.params().clone().requires_grad_(True)  # a CPU leaf
    dyn0 = env.state.dyn.clone().requires_grad_(True)
    reward = pa.differentiable_eval(env, period, nfe, wfe, control_params=theta, dyn0=dyn0)
    plain, want_reward = env.eval(period, nfe, wfe)
    assert EGC.same_bits(reward.detach().cpu().numpy(), want_reward.cpu().numpy())
    reward.sum().backward()
    _, _, saved = pa.eval_forward(env, period, nfe, wfe)
    gc, gd, _ = pa.eval_backward(saved)
    assert tuple(theta.grad.shape) == (26,) and theta.grad.device.type == "cpu"
    assert torch.equal(theta.grad, gc.sum(dim=1).cpu())
    assert torch.equal(dyn0.grad, gd)
    for k in (14, 21):  # target[0][2], target[1][3]: smooth in every env of the batch within +-h
        vals = []
        for s in (1.0, -1.0):
            th = env.control.params().clone()
            th[k] = th[k] + s * 1e-3
            e2 = E.AbstractEnvironment(env.world, env.state, env.control.with_params(th), env.judge)
            vals.append((float(e2.eval(period, nfe, wfe)[1].double().sum()), float(th[k])))
        fd = (vals[0][0] - vals[1][0]) / (vals[0][1] - vals[1][1])
        g = float(theta.grad[k])
        print("theta[%d]: autograd %.6g fd %.6g" % (k, g, fd))
        assert abs(fd - g) <= 2e-3 * (1 + abs(fd)), (k, fd, g)
