"""The checker of the body parameters' gradient (cotix_rollout_backward_ex2's
grad_params), shared by the CPU-emulation and GPU tests.

oracle/cotix_oracle/grad.py builds every body's mass, inertia, elasticity and
friction_coefficient as constants (_B.__init__).  Here _B is replaced, for
the duration of a call, by a subclass that takes them from a leaf tensor
theta [n_bodies, 4]; the chain is rollout_grad's: the faithful oracle's
forward with its traces, per step the torch restatement (asserted bit-equal
to the oracle state), torch.autograd.grad of it in (state, action, theta),
the per-step parameter gradients summed T-1 .. 0."""
import numpy as np
import torch

import grad_cases as GC
import penv_cases as PC

G, P = GC.G, GC.P
F32 = torch.float32


def _body_params(bodies):
    return np.array([[b.mass, b.inertia, b.elasticity, b.friction_coefficient] for b in bodies], np.float32)


def rollout_grad_params(make_bodies, S0, key0, actions, w, action_body, d0, dt=P.DT, step=P.robocup_step):
    """(ret, grad_actions [T,2], grad_S0 [nb,6], grad_params [nb,4]) of one env."""
    T = actions.shape[0]
    bodies = make_bodies()
    for b, row in zip(bodies, S0):
        b.set_dyn(row)
    key = np.asarray(key0, np.uint32)
    states, traces = [np.array([b.dyn() for b in bodies], np.float32)], []
    for t in range(T):
        tr = {}
        bodies, key = step(bodies, key, d0, None, tr, dt, action=actions[t], action_body=action_body)
        states.append(np.array([b.dyn() for b in bodies], np.float32))
        traces.append(tr)
    wm = np.asarray(w, np.float32).reshape(-1, 6)
    ret = np.float32(0.0)
    for t in range(1, T + 1):
        for k in np.flatnonzero(wm.reshape(-1)):
            ret = np.float32(ret + np.float32(wm.reshape(-1)[k]) * states[t].reshape(-1)[k])
    meta = make_bodies()
    index = {id(b): k for k, b in enumerate(meta)}
    theta = torch.tensor(_body_params(meta), dtype=F32, requires_grad=True)

    class ThetaB(G._B):
        def __init__(self, p, v, ang, w_, body):
            super().__init__(p, v, ang, w_, body)
            k = index[id(body)]
            self.m, self.I, self.e, self.mu = theta[k, 0], theta[k, 1], theta[k, 2], theta[k, 3]

    lam = torch.tensor(wm, dtype=F32)
    ga = np.zeros((T, 2), np.float32)
    gp = np.zeros(theta.shape, np.float32)
    real = G._B
    G._B = ThetaB  # (step_torch resolves _B at call time)
    try:
        for t in range(T - 1, -1, -1):
            S = torch.tensor(states[t], dtype=F32, requires_grad=True)
            a = torch.tensor(actions[t], dtype=F32, requires_grad=True)
            ll = step is P.lunar_lander_step
            out = G.step_torch(S, a, meta, traces[t], dt, action_body, gravity=ll, d0=d0, joints=ll)
            o = out.detach().numpy()
            same = (o.view(np.uint32) == states[t + 1].view(np.uint32)) | (np.isnan(o) & np.isnan(states[t + 1]))
            assert same.all(), "torch restatement diverged from the oracle at step %d" % t
            gS, gA, gT = torch.autograd.grad(out, (S, a, theta), lam, allow_unused=True)
            ga[t] = gA.numpy() if gA is not None else 0.0
            if gT is not None:
                gp = gp + gT.numpy()
            lam = gS.detach().clone()
            if t >= 1:
                lam = lam + torch.tensor(wm, dtype=F32)
    finally:
        G._B = real
    return ret, ga, lam.numpy(), gp


def oracle(case, envs=None):
    """Per env (ret, ga [T,2], gS0 [nb,6], gp [nb,4]).  case["make"] gives the
    scene's bodies, or case["make_env"](e) env e's own (per-env scenes)."""
    B = case["S0"].shape[0]
    out = {}
    for e in (range(B) if envs is None else envs):
        make = (lambda e=e: case["make_env"](e)) if "make_env" in case else case["make"]
        out[e] = rollout_grad_params(make, case["S0"][e], case["keys"][e], case["actions"][:, e], case["w"],
                                     case["ab"], GC.D0, step=case["step"])
    return out


def fd_params(case, e, entries):
    """Central differences of the faithful oracle's return in the parameter
    entries (body, k), h = 1e-2 max(1, |p|)."""
    names = ("mass", "inertia", "elasticity", "friction_coefficient")
    T = case["actions"].shape[0]
    make = (lambda: case["make_env"](e)) if "make_env" in case else case["make"]
    out = []
    for (b, k) in entries:
        p0 = float(_body_params(make())[b, k])
        h = 1e-2 * max(1.0, abs(p0))
        vals = []
        for s in (1, -1):
            bodies = make()
            setattr(bodies[b], names[k], np.float32(p0 + s * h))
            for bd, row in zip(bodies, case["S0"][e]):
                bd.set_dyn(row)
            key, tot = case["keys"][e], 0.0
            for tt in range(T):
                bodies, key = case["step"](bodies, key, GC.D0, action=case["actions"][tt, e],
                                           action_body=case["ab"])
                tot += float(np.dot(case["w"], np.array([x.dyn() for x in bodies], np.float64).reshape(-1)))
            vals.append(tot)
        # (the f32 parameter values actually set)
        hp = float(np.float32(p0 + h)) - float(np.float32(p0 - h))
        out.append((vals[0] - vals[1]) / hp)
    return out


def lunar_penv_case(B, T, seed=0):
    """The per-env LunarLander of penv_cases (terrain and the lander's / legs'
    parameters vary per env) as a gradient case: env e's own bodies give its
    parameters, state and theta."""
    obs = PC.lunar_penv_bodies(B, seed)
    dyn, keys = PC.state(obs)
    rng = np.random.default_rng(100 + seed)
    actions = (rng.normal(size=(T, B, 2)) * 0.1).astype(np.float32)
    w = np.zeros(4 * 6, np.float32)
    w[0], w[1], w[4], w[2 * 6 + 3] = 1.0, 0.5, 2.0, 0.25  # GC.lunar_case's return
    return dict(make_env=lambda e: PC.lunar_penv_bodies(B, seed)[e], obs=obs,
                S0=np.ascontiguousarray(dyn.transpose(2, 0, 1)), keys=keys, actions=actions, w=w, ab=0,
                step=P.lunar_lander_step, tol=GC.POLYGON_TOL, name="lunar_penv")


LUNAR_STAGES = 1 | 2 | 4 | 8 | 16 | 32
BOX_STAGES = 1 | 4 | 16


def cases():
    """name -> (case, stages, per_env, E list): the five compared cases."""
    return {
        "box6x32": (GC.box_case(6, 32, seed=1), BOX_STAGES, False, (4,)),
        "box5x16": (GC.box_case(5, 16, seed=1), BOX_STAGES, False, (1,)),
        "lunar4x8": (GC.lunar_case(4, 8, seed=0), LUNAR_STAGES, False, (1, 4)),
        "robocup8x6": (GC.robocup_case(8, 6), BOX_STAGES, False, (4,)),
        "lunar_penv4x8": (lunar_penv_case(4, 8), LUNAR_STAGES, True, (4,)),
    }


_ORACLE = {}


def oracle_of(name, case):
    """The case's oracle, computed once per process and left unchanged."""
    if name not in _ORACLE:
        _ORACLE[name] = oracle(case)
    return _ORACLE[name]


def same_bits(x, y):
    """Bit for bit, NaN patterns included (NaN payloads aside: the sign of a
    NaN follows the operand order of the instruction that made it)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    nx, ny = np.isnan(x), np.isnan(y)
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(x[~nx].view(np.uint32),
                                                                             y[~ny].view(np.uint32))


def check_conditions(name, orc):
    """What the oracle alone says about each case's parameter blocks (the
    tests assert the kernel against the oracle entrywise besides)."""
    blocks = [orc[e][3] for e in sorted(orc)]
    fin_nz = [bool(np.isfinite(b).all() and np.any(b != 0)) for b in blocks]
    if name == "box6x32":
        assert sum(fin_nz) == 5 and np.all(blocks[0] == 0), fin_nz
    elif name == "box5x16":
        assert sum(bool(np.any(np.nan_to_num(b) != 0)) for b in blocks) >= 3
    elif name in ("lunar4x8", "lunar_penv4x8"):
        assert all(fin_nz), fin_nz
    elif name == "robocup8x6":
        assert all(np.isnan(b).any() for b in blocks)
        b7 = blocks[7]
        assert np.any(np.isfinite(b7) & (b7 != 0))
