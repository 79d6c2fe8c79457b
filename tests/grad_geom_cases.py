"""The checker of the shape geometry's gradient (cotix_rollout_backward_ex3's
grad_geom), shared by the CPU-emulation and GPU tests.

oracle/cotix_oracle/grad.py builds every part's world form from constants
(_world_part).  Here _world_part is replaced, for the duration of a call, by
one that reads the part's local words from a leaf tensor theta [GW] -- the
scene's geometry row in its stored order: circle (r, cx, cy, pad), AABB (lo.x,
lo.y, up.x, up.y), polygon x, y per vertex as uploaded.  The chain is
rollout_grad's: the faithful oracle's forward with its traces, per step the
torch restatement (asserted bit-equal to the oracle state), torch.autograd.grad
of it in (state, action, theta), the per-step geometry gradients summed T-1 ..
0."""
import numpy as np
import torch

import grad_cases as GC
import grad_param_cases as GPC

G, P = GC.G, GC.P
F32 = torch.float32


def part_words(bodies):
    """(the geometry row f32 [GW], {id(part): (offset, count)}) of a scene's
    bodies: parts in body order (tests/emu/emu.py oracle_scene's row)."""
    row, where = [], {}
    for b in bodies:
        for p in b.parts:
            o = len(row)
            if p.kind == "Circle":
                row += [p.radius, p.position[0], p.position[1], 0.0]
            elif p.kind == "AABB":
                row += [p.lower[0], p.lower[1], p.upper[0], p.upper[1]]
            else:
                for v in p.vertices_:
                    row += [v[0], v[1]]
            where[id(p)] = (o, len(row) - o)
    return np.array(row, np.float32), where


def _theta_world_part(theta, where):
    """G._world_part with the local geometry read from theta (the same
    expressions in the same order: the same forward bits)."""

    def world_part(part, p, ang):
        o, n = where[id(part)]
        if part.kind == "Circle":
            return (theta[o], (theta[o + 1] + p[0], theta[o + 2] + p[1]))
        if part.kind == "AABB":
            return G._Box((theta[o] + p[0], theta[o + 1] + p[1]), (theta[o + 2] + p[0], theta[o + 3] + p[1]))
        s, c = G._SinCos.apply(ang)
        ws = [((c * theta[o + 2 * k] + (-s) * theta[o + 2 * k + 1]) + p[0] * 1.0,
               (s * theta[o + 2 * k] + c * theta[o + 2 * k + 1]) + p[1] * 1.0) for k in range(n // 2)]
        idx = G.G.order_clockwise_idx([(np.float32(x.item()), np.float32(y.item())) for x, y in ws])
        return G._Poly([ws[k] for k in idx])

    return world_part


def rollout_grad_geom(make_bodies, S0, key0, actions, w, action_body, d0, dt=P.DT, step=P.robocup_step):
    """(ret, grad_actions [T,2], grad_S0 [nb,6], grad_geom [GW]) of one env."""
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
    row, where = part_words(meta)
    theta = torch.tensor(row, dtype=F32, requires_grad=True)
    lam = torch.tensor(wm, dtype=F32)
    ga = np.zeros((T, 2), np.float32)
    gg = np.zeros(theta.shape, np.float32)
    real = G._world_part
    G._world_part = _theta_world_part(theta, where)  # (step_torch resolves _world_part at call time)
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
                gg = gg + gT.numpy()
            lam = gS.detach().clone()
            if t >= 1:
                lam = lam + torch.tensor(wm, dtype=F32)
    finally:
        G._world_part = real
    return ret, ga, lam.numpy(), gg


def oracle(case, envs=None):
    """Per env (ret, ga [T,2], gS0 [nb,6], gg [GW]).  case["make"] gives the
    scene's bodies, or case["make_env"](e) env e's own (per-env scenes)."""
    B = case["S0"].shape[0]
    out = {}
    for e in (range(B) if envs is None else envs):
        make = (lambda e=e: case["make_env"](e)) if "make_env" in case else case["make"]
        out[e] = rollout_grad_geom(make, case["S0"][e], case["keys"][e], case["actions"][:, e], case["w"],
                                   case["ab"], GC.D0, step=case["step"])
    return out


def pad_words(case):
    """The circles' pad words of the case's geometry row."""
    bodies = case["make_env"](0) if "make_env" in case else case["make"]()
    _, where = part_words(bodies)
    return [where[id(p)][0] + 3 for b in bodies for p in b.parts if p.kind == "Circle"]


def _set_word(bodies, k, value):
    """Set word k of the bodies' geometry row (a finite-difference probe)."""
    _, where = part_words(bodies)
    for b in bodies:
        for p in b.parts:
            o, n = where[id(p)]
            if not o <= k < o + n:
                continue
            q, v = k - o, np.float32(value)
            if p.kind == "Circle":
                assert q < 3
                if q == 0:
                    p.radius = v
                else:
                    pos = list(p.position)
                    pos[q - 1] = v
                    p.position = tuple(pos)
            elif p.kind == "AABB":
                lo, up = list(p.lower), list(p.upper)
                (lo if q < 2 else up)[q % 2] = v
                p.lower, p.upper = tuple(lo), tuple(up)
            else:
                raise NotImplementedError("polygon words are not probed")
            return
    raise IndexError(k)


def fd_geom(case, e, words, rel=1e-3):
    """Central differences of the faithful oracle's return in the geometry
    words, h = rel max(1, |p|)."""
    T = case["actions"].shape[0]
    make = (lambda: case["make_env"](e)) if "make_env" in case else case["make"]
    row, _ = part_words(make())
    out = []
    for k in words:
        p0 = float(row[k])
        h = rel * max(1.0, abs(p0))
        vals = []
        for s in (1, -1):
            bodies = make()
            _set_word(bodies, k, p0 + s * h)
            for bd, r in zip(bodies, case["S0"][e]):
                bd.set_dyn(r)
            key, tot = case["keys"][e], 0.0
            for tt in range(T):
                bodies, key = case["step"](bodies, key, GC.D0, action=case["actions"][tt, e],
                                           action_body=case["ab"])
                tot += float(np.dot(case["w"], np.array([x.dyn() for x in bodies], np.float64).reshape(-1)))
            vals.append(tot)
        hp = float(np.float32(p0 + h)) - float(np.float32(p0 - h))  # (the f32 values actually set)
        out.append((vals[0] - vals[1]) / hp)
    return out


LUNAR_STAGES, BOX_STAGES = GPC.LUNAR_STAGES, GPC.BOX_STAGES
# The floor of GC.close a case's grad_geom blocks get where the project's
# constant (case["tol"]) is too small: four times the measured need (the margin
# the project's constants keep), DESIGN.md "Shape-geometry gradients"
GEOM_FLOOR = {}


def cases():
    """name -> (case, stages, per_env, E list): the seven compared cases."""
    return {
        "box5x16": (GC.box_case(5, 16, seed=1), BOX_STAGES, False, (4, 1)),
        "robocup8x6": (GC.robocup_case(8, 6), BOX_STAGES, False, (4,)),
        "lunar4x8": (GC.lunar_case(4, 8, seed=0), LUNAR_STAGES, False, (4, 1)),
        "poly_box4x8": (GC.poly_box_case(4, 8), BOX_STAGES, False, (4,)),
        "ball_poly4x8": (GC.ball_poly_case(4, 8), BOX_STAGES, False, (4, 1)),
        "lunar_penv4x8": (GPC.lunar_penv_case(4, 8), LUNAR_STAGES, True, (4,)),
        "quad_row4x6": (GC.quad_row_case(4, 6), BOX_STAGES, False, (4,)),
    }


def tol_of(name, case):
    rtol, floor = case["tol"]
    return (rtol, GEOM_FLOOR.get(name, floor))


_ORACLE = {}


def oracle_of(name, case):
    """The case's oracle, computed once per process and left unchanged."""
    if name not in _ORACLE:
        _ORACLE[name] = oracle(case)
    return _ORACLE[name]


same_bits = GPC.same_bits


def _nnz(b):
    return int(np.count_nonzero(np.nan_to_num(b, nan=1.0)))


def check_conditions(name, orc):
    """What the oracle alone says about each case's geometry blocks (the tests
    assert the kernel against the oracle entrywise besides)."""
    blocks = [orc[e][3] for e in sorted(orc)]
    zero = [bool(np.all(b == 0)) for b in blocks]
    fin = [bool(np.isfinite(b).all()) for b in blocks]
    nz = [int(np.count_nonzero(b)) for b in blocks]
    nan = [int(np.isnan(b).sum()) for b in blocks]
    if name == "box5x16":
        assert blocks[0].size == 28 and zero == [True, False, False, False, True], zero
        assert all(fin) and nz[1:4] == [6, 13, 7], nz
    elif name == "robocup8x6":
        assert blocks[0].size == 36 and nan == [18, 15, 15, 5, 19, 15, 18, 5], nan
        b7 = blocks[7]
        assert int(np.sum(np.isfinite(b7) & (b7 != 0))) == 4
    elif name == "lunar4x8":
        assert blocks[0].size == 84 and all(fin) and nz == [18, 16, 16, 16], nz
    elif name == "poly_box4x8":
        assert blocks[0].size == 28 and all(fin) and zero[1] and [nz[0], nz[2], nz[3]] == [9, 15, 9], nz
    elif name == "ball_poly4x8":
        assert blocks[0].size == 24 and all(fin) and zero[3] and nz[:3] == [9, 12, 9], nz
        assert blocks[1][16] != 0 and blocks[1][20] != 0
    elif name == "lunar_penv4x8":
        assert blocks[0].size == 84 and all(fin) and nz == [20, 16, 19, 8], nz
    elif name == "quad_row4x6":
        assert blocks[0].size == 72 and all(fin) and nz == [40, 40, 31, 48], nz
    else:
        raise KeyError(name)
