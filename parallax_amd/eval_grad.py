"""Differentiable eval: the gradient of AbstractEnvironment.eval's reward with
respect to the 26 parameters of the device control (AffineControl: gain 2x6,
target 2x6, bias 2) and to the entry state, forward and backward one HIP
launch each (cotix_eval_rollout / cotix_eval_backward, include/cotix_amd.h).

In the reference eval is a lax.scan (cotix/_envs.py:37-132), so jax.grad of
the reward in a controller's parameters works there: policy fitting and
trajectory optimisation through the simulator.  Derivatives follow the
differentiable rollout's rule (rollout.py): the executed branch of every
lax.cond, collider choices held fixed, balanced ties for max / min / clip.
Per env, with s_t the state after env-step t (s_0 the entry state), t* the
first t at which the judge says is_done and dv_t = clip(gain (target -
s_{t-1}[body]) + bias):

    reward = sum_{1 <= t < t*} dt * rate(s_t) + end_reward(s_t*)

(no last term for an env that is live to the end).  The judge's region
membership, region rewards, biases and the clip bounds are constants; env-steps
after t* contribute exact zeros.

The control parameter vector theta is float32 [26]: theta[6 i + q] = gain[i][q],
theta[12 + 6 i + q] = target[i][q], theta[24 + i] = bias[i]
(AffineControl.params() / AffineControl.with_params(theta)).
"""
import numpy as np
import torch

from . import _ffi
from .envs import AbstractEnvironment, AffineControl, LinearJudge, PhysicsWorld, WorldState

N_CONTROL_PARAMS = 26


def _eval_dt(eval_period, num_NFEs, WFE_scale):
    """AbstractEnvironment.eval's f32 step: time_per_NFE / WFE_scale."""
    tpn = np.float32(eval_period / num_NFEs)
    return float(np.float32(tpn / np.float32(float(WFE_scale))))


def _check_env(env):
    if not isinstance(env.world, PhysicsWorld) or not isinstance(env.judge, LinearJudge):
        raise ValueError("the differentiable eval needs a PhysicsWorld and a device judge (LinearJudge)")
    if env.control is not None and not isinstance(env.control, AffineControl):
        raise ValueError("the differentiable eval needs a device control (AffineControl) or none")


def eval_forward(env, eval_period, num_NFEs, WFE_scale=10):
    """env.eval(eval_period, num_NFEs, WFE_scale) as one launch that also saves
    what eval_backward needs -> (new_env, reward [B], saved).  State, keys,
    err and reward equal env.eval's bit for bit.

    Memory: as rollout_forward's, with T = num_NFEs * WFE_scale -- the saved
    trajectory is T * (24 * n_bodies + 8) bytes per env, the decision tape
    T * tape_words * 4 bytes per env (tape_words =
    cotix_rollout_tape_words(scene): 12 * n_bodies in analytic scenes,
    5 * n_bodies + 4 * n_contacts in polygon scenes), the judge record
    (T + 1) * 4 bytes per env.  The tape is mandatory here (there is no re-play
    backward of the eval); an allocation failure of it says so."""
    _check_env(env)
    w = env.world.world
    nb, B, T = len(w.bodies), w.B, int(num_NFEs) * int(WFE_scale)
    dt = _eval_dt(eval_period, num_NFEs, WFE_scale)
    st = env.state.clone()
    dev = st.dyn.device
    reward = torch.zeros(B, dtype=torch.float32, device=dev)
    finished = torch.zeros(B, dtype=torch.int32, device=dev)
    nblk = (B + 3) // 4  # the saved rows in env blocks of 4 (include/cotix_amd.h)
    saved_dyn = torch.empty(T, nblk, nb * 6, 4, device=dev, dtype=torch.float32)
    saved_keys = torch.empty(T, B, 2, device=dev, dtype=torch.int32)
    tw = _ffi.lib.cotix_rollout_tape_words(w.scene.handle)
    try:
        tape = torch.empty(T, nblk, tw, 4, device=dev, dtype=torch.int32)
    except torch.OutOfMemoryError as e:
        raise torch.OutOfMemoryError(
            "eval decision tape: %d x %d x %d u32 words (%.1f MiB) do not fit; the differentiable eval has no "
            "re-play backward, so fewer envs or env-steps per call are the way out (%s)"
            % (T, tw, B, T * tw * B * 4 / 2**20, e)) from e
    rec = torch.empty(T + 1, B, device=dev, dtype=torch.int32)
    judge = env.judge.c_struct()
    control = env.control.c_struct() if env.control is not None else None
    _ffi.check(_ffi.lib.cotix_eval_rollout(
        w.scene.handle, _ffi.ptr(st.dyn), _ffi.ptr(st.keys), _ffi.ptr(st.err), _ffi.ptr(w.geom), w.geom_stride, B,
        int(num_NFEs), int(WFE_scale), dt, int(env.world.stages), judge, control, None, 0, _ffi.ptr(reward),
        _ffi.ptr(finished), _ffi.ptr(saved_dyn), _ffi.ptr(saved_keys), _ffi.ptr(tape), _ffi.ptr(rec),
        _ffi.stream_ptr(dev)), "cotix_eval_rollout")
    saved = dict(world=w, dyn=saved_dyn, keys=saved_keys, tape=tape, rec=rec, judge=judge, control=control,
                 n_nfe=int(num_NFEs), wfe=int(WFE_scale), dt=dt, stages=int(env.world.stages), finished=finished,
                 geom_version=w.geom._version)
    return AbstractEnvironment(env.world, st, env.control, env.judge), reward, saved


def eval_backward(saved, want_control=True, want_dyn0=True, want_dv=True):
    """-> (g_control [26, B], g_dyn0 [n_bodies, 6, B], g_dv [T, B, 2]) of the
    reward of eval_forward, per env (None where not wanted; g_control is None
    without a control)."""
    w = saved["world"]
    if w.geom._version != saved["geom_version"]:
        raise RuntimeError("the world's geometry changed between eval_forward() and eval_backward()")
    nb, B, T = len(w.bodies), w.B, saved["n_nfe"] * saved["wfe"]
    dev = saved["dyn"].device
    gc = (torch.empty(N_CONTROL_PARAMS, B, device=dev, dtype=torch.float32)
          if want_control and saved["control"] is not None else None)
    gd = torch.empty(nb, 6, B, device=dev, dtype=torch.float32) if want_dyn0 else None
    gv = torch.empty(T, B, 2, device=dev, dtype=torch.float32) if want_dv else None
    _ffi.check(_ffi.lib.cotix_eval_backward(
        w.scene.handle, _ffi.ptr(saved["dyn"]), _ffi.ptr(saved["keys"]), _ffi.ptr(saved["tape"]),
        _ffi.ptr(saved["rec"]), _ffi.ptr(w.geom), w.geom_stride, B, saved["n_nfe"], saved["wfe"], saved["dt"],
        saved["stages"], saved["judge"], saved["control"], None, _ffi.ptr(gc), _ffi.ptr(gd), _ffi.ptr(gv), None,
        _ffi.stream_ptr(dev)), "cotix_eval_backward")
    return gc, gd, gv


class _Eval(torch.autograd.Function):
    @staticmethod
    def forward(ctx, control_params, dyn0, env, eval_period, num_NFEs, WFE_scale):
        control = env.control
        if control_params is not None:
            control = control.with_params(control_params.detach())
        state = env.state
        if dyn0 is not None:
            state = WorldState(dyn0.detach().contiguous(), state.keys, state.err)
        run = AbstractEnvironment(env.world, state, control, env.judge)
        _, reward, saved = eval_forward(run, eval_period, num_NFEs, WFE_scale)
        ctx.saved = saved
        ctx.theta_device = None if control_params is None else control_params.device
        return reward

    @staticmethod
    def backward(ctx, g_reward):
        want_c, want_d = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gc, gd, _ = eval_backward(ctx.saved, want_control=want_c, want_dyn0=want_d, want_dv=False)
        g = g_reward.to(torch.float32)
        g_theta = (gc * g[None, :]).sum(dim=1).to(ctx.theta_device) if want_c else None
        g_dyn = gd * g[None, None, :] if want_d else None
        return g_theta, g_dyn, None, None, None, None


def differentiable_eval(env, eval_period, num_NFEs, WFE_scale=10, control_params=None, dyn0=None):
    """reward [B] of env.eval(eval_period, num_NFEs, WFE_scale), differentiable
    through torch.autograd (env itself is not advanced).

    control_params: a float32 [26] tensor (the layout above) replacing the
    parameters of env.control, an AffineControl whose body and clip are kept;
    its gradient is sum_env g_reward[env] * d reward[env] / d theta.
    dyn0: an optional [n_bodies, 6, B] tensor replacing the env's state; its
    gradient is g_reward[env] * d reward[env] / d the entry state."""
    _check_env(env)
    if control_params is not None:
        if env.control is None:
            raise ValueError("control_params needs an env with an AffineControl")
        if tuple(control_params.shape) != (N_CONTROL_PARAMS,) or control_params.dtype != torch.float32:
            raise ValueError("control_params must be a float32 [26] tensor (AffineControl.params())")
    if dyn0 is not None and (tuple(dyn0.shape) != tuple(env.state.dyn.shape) or dyn0.dtype != torch.float32
                             or dyn0.device != env.state.dyn.device):
        raise ValueError("dyn0 must be a float32 %s tensor on the env's device" % (tuple(env.state.dyn.shape),))
    return _Eval.apply(control_params, dyn0, env, eval_period, num_NFEs, WFE_scale)
