"""The checker of the differentiable eval (cotix_eval_rollout /
cotix_eval_backward), shared by the CPU-emulation and GPU tests.

Per env, after grad_param_cases.rollout_grad_params: the faithful oracle's
forward along the reward's chain with its traces (steps 1 .. t*, t* the first
state at which the judge says is_done, or all T steps), per step the torch
restatement grad.step_torch with the action a = control(S, theta) built in
torch from a leaf theta [26] (gain 2x6, target 2x6, bias 2) -- asserted
bit-equal to the oracle state -- and torch.autograd.grad of it in (S, theta,
a), chained from the last chain state's seed with the direct seeds added:

  reward = sum_{1 <= t < t*} dt rate(s_t) + end_reward(s_t*)   (no last term
           for an env live to the end)
  seed_t = dt (rate_w + rate_region_w[r_t]) for 1 <= t < t*, end_w at t = t*

Region membership, region rewards and biases are constants.  A parameter
whose gain or bias is zero gets its gradient through a term that adds an exact
zero to the value (Z - Z.detach()).  The reward rebuilt this way equals
eval_device_cases.oracle_eval's bit for bit (asserted by the tests)."""
import copy

import numpy as np
import torch

import eval_device_cases as EDC
import grad_cases as GC

G, P = GC.G, GC.P
F = np.float32
F32 = torch.float32
NPAR = 26


def theta_of(ctl_kwargs):
    """[26] f32: gain[0][0..5], gain[1][0..5], target[0], target[1], bias."""
    z = [[0.0] * 6, [0.0] * 6]
    gain, target = ctl_kwargs.get("gain") or z, ctl_kwargs.get("target") or z
    return np.array([*gain[0], *gain[1], *target[0], *target[1], *ctl_kwargs.get("bias", (0.0, 0.0))], np.float32)


def control_kwargs(ctl_kwargs, theta):
    """The control's kwargs with the 26 parameters replaced."""
    th = [float(v) for v in np.asarray(theta, np.float32)]
    out = dict(ctl_kwargs)
    out["gain"], out["target"], out["bias"] = [th[0:6], th[6:12]], [th[12:18], th[18:24]], (th[24], th[25])
    return out


def control_torch(s, theta, theta0, clip):
    """dv [2] of the affine control on one body's state s [6] with theta as a
    torch leaf: the device control's sum (nonzero gains in q order from the
    first term, the bias last when nonzero), the zero-valued parameters
    through exact-zero terms, then the clip."""
    out = []
    for i in range(2):
        acc, zs = None, None
        for q in range(6):
            term = theta[6 * i + q] * (theta[12 + 6 * i + q] - s[q])
            if theta0[6 * i + q] != 0:
                acc = term if acc is None else acc + term
            else:
                z = term - term.detach()
                zs = z if zs is None else zs + z
        b = theta[24 + i]
        if theta0[24 + i] != 0:
            acc = b if acc is None else acc + b
        else:
            z = b - b.detach()
            zs = z if zs is None else zs + z
        acc = torch.zeros((), dtype=F32) if acc is None else acc
        if zs is not None:
            acc = acc + zs
        if clip is not None:
            acc = G._clip(acc, torch.tensor(float(F(clip[i][0])), dtype=F32), torch.tensor(float(F(clip[i][1])), dtype=F32))
        out.append(acc)
    return torch.stack(out)


def _dense(terms, n):
    w = np.zeros(n, np.float32)
    for k, v in terms:
        w[k] = v
    return w


def eval_grad_env(case, jk, ck, e, nfe, wfe, period, theta=None):
    """One env: dict(reward, tstar (None: live), g_control [26], g_dyn0
    [nb, 6], g_dv [T, 2], regions [T + 1] (rate region of s_t, -1 none),
    sat [T, 2] (the clip's slope at each chain step), states)."""
    from cotix_oracle import envs as OE
    from cotix_oracle.geometry import ErrorFlag
    ab, T = case["ab"], nfe * wfe
    dt = F(F(period / nfe) / F(float(wfe)))
    theta0 = theta_of(ck) if theta is None else np.asarray(theta, np.float32)
    ckw = control_kwargs(ck, theta0)
    oj, oc = OE.LinearJudge(**jk), OE.AffineControl(**ckw)
    bodies = case["make"]()
    for b, row in zip(bodies, case["S0"][e]):
        b.set_dyn(row)
    key, err = np.asarray(case["keys"][e], np.uint32), 0
    snap = lambda: np.array([b.dyn() for b in bodies], np.float32)  # noqa: E731
    states, traces, dvs = [snap()], [], []
    tstar = 0 if oj.is_done((bodies, key, err), None) else None
    while tstar is None and len(traces) < T:
        dv = oc.dv((bodies, key, err))
        ef = ErrorFlag()
        ef.bits = err
        tr = {}
        bodies, key = case["step"]([copy.copy(b) for b in bodies], key, GC.D0, ef, tr, dt, action=dv, action_body=ab)
        err = ef.bits
        states.append(snap())
        traces.append(tr)
        dvs.append(np.array(dv, np.float32))
        if oj.is_done((bodies, key, err), None):
            tstar = len(traces)
    n = len(traces)  # the chain's steps
    mk = case["make"]

    def as_state(S):
        bs = mk()
        for b, row in zip(bs, S):
            b.set_dyn(row)
        return (bs, None, 0)

    regions = [-1] + [oj.region(as_state(states[t]), oj.rate_regions) if oj.rate_regions else -1
                      for t in range(1, n + 1)]
    reward = F(0.0)
    with np.errstate(all="ignore"):
        for t in range(1, n if tstar is not None else n + 1):
            reward = F(reward + F(oj.rate(as_state(states[t]), None)) * dt)
        if tstar is not None:
            reward = F(reward + oj.end_reward(as_state(states[tstar]), None))
    nw = states[0].size
    wr, we = _dense(oj.rate_terms, nw), _dense(oj.end_terms, nw)
    wrr = [_dense(rr[3], nw) for rr in oj.rate_regions]

    def seed(t):
        if tstar is not None and t == tstar:
            return we.copy()
        if t >= 1:
            s = wr * dt
            if regions[t] >= 0:
                s = s + wrr[regions[t]] * dt
            return s.astype(np.float32)
        return np.zeros(nw, np.float32)

    nb = states[0].shape[0]
    lam = torch.tensor(seed(n).reshape(nb, 6), dtype=F32)
    g_dv = np.zeros((T, 2), np.float32)
    g_c = np.zeros(NPAR, np.float32)
    sat = np.ones((T, 2), np.float32)
    meta = mk()
    ll = case["step"] is P.lunar_lander_step
    clip = ckw.get("clip")
    for t in range(n - 1, -1, -1):
        S = torch.tensor(states[t], dtype=F32, requires_grad=True)
        th = torch.tensor(theta0, dtype=F32, requires_grad=True)
        a = control_torch(S[ab], th, theta0, clip)
        av = a.detach().numpy()
        assert same_bits(av, dvs[t]), "torch control diverged from the oracle at step %d" % t
        out = G.step_torch(S, a, meta, traces[t], dt, ab, gravity=ll, d0=GC.D0, joints=ll)
        o = out.detach().numpy()
        same = (o.view(np.uint32) == states[t + 1].view(np.uint32)) | (np.isnan(o) & np.isnan(states[t + 1]))
        assert same.all(), "torch restatement diverged from the oracle at step %d" % t
        gS, gT, gA = torch.autograd.grad(out, (S, th, a), lam, allow_unused=True)
        g_dv[t] = gA.numpy() if gA is not None else 0.0
        if gT is not None:
            g_c = g_c + gT.numpy()
        if clip is not None:  # whether the clip is active, for the tests' conditions
            raw = control_torch(S[ab], th, theta0, None).detach().numpy()
            sat[t] = np.where(raw != av, 0.0, 1.0)
        lam = gS.detach().clone() + torch.tensor(seed(t).reshape(nb, 6), dtype=F32)
    return dict(reward=reward, tstar=tstar, g_control=g_c, g_dyn0=lam.numpy(), g_dv=g_dv, regions=regions, sat=sat,
                states=states, n=n)


def oracle(case, name, nfe, wfe, period, envs=None, judge=None, control=None):
    """Per env the dict of eval_grad_env, for the named judge / control pair of
    eval_device_cases (or the given kwargs)."""
    jk, ck = EDC.judges(name, case["ab"]) if judge is None else (judge, control)
    B = case["S0"].shape[0]
    return {e: eval_grad_env(case, jk, ck, e, nfe, wfe, period) for e in (range(B) if envs is None else envs)}


_ORACLE = {}


def oracle_of(tag, case, name, nfe, wfe, period, **kw):
    """The case's oracle, computed once per process and left unchanged."""
    if tag not in _ORACLE:
        _ORACLE[tag] = oracle(case, name, nfe, wfe, period, **kw)
    return _ORACLE[tag]


def fd_theta(case, jk, ck, e, nfe, wfe, period, entries, h=1e-2):
    """Central differences of the faithful oracle's eval reward (eval_env) in
    the theta entries, f64 difference of the f32 rewards."""
    from cotix_oracle import envs as OE
    th0 = theta_of(ck)
    out = []
    for k in entries:
        vals = []
        for s in (1, -1):
            th = th0.copy()
            th[k] = F(th0[k] + s * h)
            bodies = case["make"]()
            for b, row in zip(bodies, case["S0"][e]):
                b.set_dyn(row)
            st = (bodies, np.asarray(case["keys"][e], np.uint32), 0)
            r = OE.eval_env(case["step"], st, OE.AffineControl(**control_kwargs(ck, th)), OE.LinearJudge(**jk), period,
                            nfe, wfe, GC.D0, case["ab"], carry=(0.0, False))[1]
            vals.append((float(r), float(th[k])))
        out.append((vals[0][0] - vals[1][0]) / (vals[0][1] - vals[1][1]))
    return out


# the issue's cases: (scene case, judge name, NFEs, WFE scale, period)
BOX_STAGES = 1 | 4 | 16
LUNAR_STAGES = 1 | 2 | 4 | 8 | 16 | 32


def box8():
    return EDC.case("box", 8, seed=5)


BOX = {"x_done": (3, 10, 0.6), "multi": (4, 6, 0.5), "piecewise": (4, 8, 0.64)}
BOX_TSTAR = {  # env -> t* (None: live to the end), checked on the oracle alone
    "x_done": {1: 0, 3: 13, 2: 17, 0: 26, 7: 26, 4: None, 5: None, 6: None},
    "multi": {0: 0, 1: 0, 7: 3, 3: 7, 6: 11, 2: 12, 4: None, 5: None},
    "piecewise": {3: 12, 7: 17, 2: 16},
}

LUNAR_JUDGE = dict(rate_w={1: 1.0, 4: -0.5, 15: 0.25}, end_w={0: 1.0, 3: 2.0},
                   regions=[(0, [-np.inf] * 4 + [0.025, -np.inf], [np.inf] * 6, 3.0)])
LUNAR_CONTROL = dict(body=0, gain=[[0, 0, .2, 0, .1, 0], [0, .05, 0, .3, 0, .02]],
                     target=[[0] * 6, [0, -6, 0, .1, 0, 0]], bias=(0, .002), clip=((-.05, .05), (-.01, .04)))
LUNAR = (2, 4, 0.08)  # 2 NFE x 4, dt 0.01


def lunar4():
    return GC.lunar_case(4, 1, seed=0)


def same_bits(x, y):
    """Bit for bit, NaN patterns included (NaN payloads aside)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    nx, ny = np.isnan(x), np.isnan(y)
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(x[~nx].view(np.uint32),
                                                                             y[~ny].view(np.uint32))
