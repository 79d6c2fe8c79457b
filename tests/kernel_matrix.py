"""TEST INFRASTRUCTURE: the kernel ledger -- one row per launch recipe, and the
kernel instantiation(s) of parallax_amd/csrc/cotix_plan.h each recipe is meant
to run.  Data plus helpers; the tests are tests/test_kernel_matrix_cpu.py (the
ledger is exact and closed over the kernel list, every row runs on the host
emulation and meets its reference) and tests/test_gpu_kernel_matrix.py (every
row on the GPU).

A row names everything a launch needs: the case (an existing one, with its
existing oracle and tolerance), the variant (envs_per_wave, specialize), the
batch, the steps, the stages, the launches it does and, per launch, the kernel
key.  Keys are literals, written from the kernel list's comments -- the plan
(cxl::plan_launch through emu_launch_plan_ex) is checked against them, not the
other way round:

  ("step", fnset, mode, spec, gp)        step_kernel<EW, fnset, mode, spec, gp>
  ("help", fnset, spec, sdefer, l1)      step_help_kernel<fnset, spec, sdefer, l1>
  ("split", nb, spec)                    bwd_split_kernel<nb, spec>

Launches: fwd (mode 1), tapeN / replayN (modes 4 / 2 at gradient level N: 0
none, 1 want_params, 2 want_geom), eval / eval_fwd / eval_bwd (modes 3 / 5 /
6), step (mode 0)."""
import collections
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "emu"), os.path.join(HERE, "golden"), os.path.join(HERE, "..", "oracle"),
           os.path.join(HERE, "..")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STEP, HELP, HELP_L1, SPLIT = 0, 1, 2, 3  # cxl::FAM_*
GENERIC, ROBOCUP, LUNAR, ROBOCUP_PART, LUNAR_PART, BOX = range(6)  # cxk::SPEC_*
AN, PP, AP, ALL = 1, 3, 11, 15  # the contact-function programs
EWS = (1, 2, 4, 8)
BOX_STAGES = 1 | 4 | 16
LUNAR_STAGES = 1 | 2 | 4 | 8 | 16 | 32  # (with the broadphase: the backwards drop it)
LUNAR_STEP_STAGES = 1 | 2 | 4 | 8 | 16
NO_COLLIDER = 1 | 16
# launch -> (mode, gradient level)
LAUNCH = {"fwd": (1, 0), "tape0": (4, 0), "tape1": (4, 1), "tape2": (4, 2), "replay0": (2, 0), "replay1": (2, 1),
          "replay2": (2, 2), "eval": (3, 0), "eval_fwd": (5, 0), "eval_bwd": (6, 0), "step": (0, 0)}

# keys: ((launch, key), ...); envs: the case's envs the row runs (None: all);
# cus_free: the plan does not depend on the device's compute-unit count
Row = collections.namedtuple("Row", "id kind case ew specialize B n_steps stages keys envs cus_free")


def _sk(fn, mode, spec=GENERIC, gp=0):
    return ("step", fn, mode, spec, gp)


def _rollout_keys(fn, fwd=GENERIC, tape0=GENERIC, tape1=GENERIC):
    """The seven launches of a rollout row: the forward, the tape backward and
    the re-play at each gradient level (the re-play and level 2 are generic)."""
    return (("fwd", _sk(fn, 1, fwd)), ("tape0", _sk(fn, 4, tape0)), ("tape1", _sk(fn, 4, tape1, 1)),
            ("tape2", _sk(fn, 4, GENERIC, 2)), ("replay0", _sk(fn, 2)), ("replay1", _sk(fn, 2, GENERIC, 1)),
            ("replay2", _sk(fn, 2, GENERIC, 2)))


def _eval_keys(fn, ev=GENERIC, diff=GENERIC):
    return (("eval", _sk(fn, 3, ev)), ("eval_fwd", _sk(fn, 5, diff)), ("eval_bwd", _sk(fn, 6, diff)))


# case -> (program, B, T, stages, tilings)
ROLLOUT_CASES = {
    "box5x16": (AN, 5, 16, BOX_STAGES, EWS),  # ragged at every tiling, two waves at 2 and 4, the tape's blocks of 4
    "lunar4x8": (ALL, 4, 8, LUNAR_STAGES, EWS),  # the full program, the joints, half a wave at 8
    "ball_poly4x8": (ALL, 4, 8, BOX_STAGES, (2, 8)),  # the circle x polygon VJP
    "lunar_penv4x8": (ALL, 4, 8, LUNAR_STAGES, (2, 8)),  # per-env geometry rows
}
# case (tests/test_eval_grad_cpu.py setup) -> (program, B, T, stages)
EVAL_CASES = {"piecewise": (AN, 8, 32, BOX_STAGES), "lunar": (ALL, 4, 8, LUNAR_STAGES)}
# the generic step programs, one scene per contact-function set (tests/test_launch_plan_cpu.py's)
STEP_SCENES = {"robocup_cp": AN, "convex": PP, "aabb_poly": AP, "circle_poly": ALL}
# the reference scenes' step specializations, at 2 and 4 envs per wave
STEP_SPECS = {"robocup": (AN, ROBOCUP, BOX_STAGES), "robocup_part": (AN, ROBOCUP_PART, BOX_STAGES),
              "lunar": (PP, LUNAR, LUNAR_STEP_STAGES), "lunar_part": (PP, LUNAR_PART, LUNAR_STEP_STAGES)}


def _rows():
    out = []
    # the generic rollout programs at every tiling (specialize off: the box
    # world's specializations at 4 envs per wave have a row of their own)
    for case, (fn, B, T, stages, ews) in ROLLOUT_CASES.items():
        for ew in ews:
            out.append(Row("rollout-%s-ew%d" % (case, ew), "rollout", case, ew, 0, B, T, stages, _rollout_keys(fn),
                           None, True))
    # the generic eval programs at every tiling
    for case, (fn, B, T, stages) in EVAL_CASES.items():
        for ew in EWS:
            out.append(Row("eval-%s-ew%d" % (case, ew), "eval", case, ew, 0, B, T, stages, _eval_keys(fn), None, True))
    # the generic step programs: 13 envs (ragged at every tiling), 20 steps (two key windows)
    for scene, fn in STEP_SCENES.items():
        for ew in EWS:
            out.append(Row("step-%s-ew%d" % (scene, ew), "step", scene, ew, 1, 13, 20, BOX_STAGES,
                           (("step", _sk(fn, 0)),), None, True))
    # the reference scenes' step specializations (one key window: at 4 envs per
    # wave a longer RoboCup launch is the helper form's, below)
    for scene, (fn, spec, stages) in STEP_SPECS.items():
        for ew in (2, 4):
            out.append(Row("step-%s-ew%d-spec" % (scene, ew), "step", scene, ew, 1, 13, 16, stages,
                           (("step", _sk(fn, 0, spec)),), None, True))
    out.append(Row("step-box-ew4-spec", "step", "box", 4, 1, 13, 16, BOX_STAGES, (("step", _sk(AN, 0, BOX)),), None,
                   True))
    # RoboCup's and the box world's programs at the default tiling.  RoboCup's
    # six envs are not whole groups of 4: the tape backward stays step_kernel
    out.append(Row("rollout-box5x16-ew4-spec", "rollout", "box5x16", 4, 1, 5, 16, BOX_STAGES,
                   _rollout_keys(AN, BOX, BOX, BOX), None, True))
    out.append(Row("rollout-robocup6x6-ew4-spec", "rollout", "robocup8x6", 4, 1, 6, 6, BOX_STAGES,
                   _rollout_keys(AN, ROBOCUP, ROBOCUP, ROBOCUP), tuple(range(6)), True))
    out.append(Row("eval-piecewise-ew4-spec", "eval", "piecewise", 4, 1, 8, 32, BOX_STAGES,
                   _eval_keys(AN, GENERIC, BOX), None, True))
    out.append(Row("eval-goal-ew4-spec", "eval", "goal", 4, 1, 6, 12, BOX_STAGES, _eval_keys(AN, ROBOCUP, ROBOCUP),
                   None, True))
    # the two-wave forms: the key helper with the level-1 ring (one workgroup:
    # the ring's LDS costs no residency on any device whose CU count is known)
    # and without it (no collider: nothing reads the ring), and the tape
    # backward at two waves per env group (whole groups of 4 envs)
    out.append(Row("help-l1-robocup-ew4", "step", "robocup", 4, 1, 16, 20, BOX_STAGES,
                   (("step", ("help", AN, ROBOCUP, 1, 1)),), None, False))
    out.append(Row("help-robocup-ew4", "step", "robocup", 4, 1, 16, 20, NO_COLLIDER,
                   (("step", ("help", AN, ROBOCUP, 1, 0)),), None, True))
    out.append(Row("split-robocup16x8-ew4", "rollout", "robocup16x8", 4, 1, 16, 8, BOX_STAGES,
                   (("fwd", _sk(AN, 1, ROBOCUP)), ("tape0", ("split", 5, ROBOCUP)), ("replay0", _sk(AN, 2))), None,
                   True))
    return out


ROWS = _rows()
IDS = [r.id for r in ROWS]
assert len(set(IDS)) == len(IDS)


def row_keys(row):
    """{(key, ew)} of a row."""
    return {(k, row.ew) for _, k in row.keys}


def launches(row):
    return [name for name, _ in row.keys]


def step_form(row):
    """What cotix_scene_last_step_form reports after a step row's launch."""
    key = dict(row.keys)["step"]
    return STEP if key[0] == "step" else HELP_L1 if key[4] else HELP


# ---------------------------------------------------------------------------
# the kernel list and the plan, through the host emulation's exports
# ---------------------------------------------------------------------------
PLAN_FIELDS = ("family", "ew", "wpb", "fnset", "mode", "spec", "gp", "sdefer", "nb", "grid", "block", "lds", "error",
               "listed")


def bind(lib):
    """The ledger's exports of a host-emulation library (cotix_emu.cpp)."""
    lib.emu_kernel_list.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    lib.emu_launch_plan_ex.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 11 + [ctypes.c_void_p]
    lib.emu_set_key_helper.argtypes = [ctypes.c_int]
    lib.emu_set_split_bwd.argtypes = [ctypes.c_int]
    return lib


def kernel_list(lib):
    """{(key, ew)} of cxl::STEP_KERNELS, HELP_KERNELS and SPLIT_KERNELS."""
    out = set()
    for which in (0, 1, 2):
        n = lib.emu_kernel_list(which, None, 0)
        assert n > 0
        buf = (ctypes.c_int * (5 * n))()
        assert lib.emu_kernel_list(which, ctypes.cast(buf, ctypes.c_void_p), n) == n
        for i in range(n):
            a, b, c, d, ews = buf[5 * i:5 * i + 5]
            key = ("step", a, b, c, d) if which == 0 else ("help", a, b, c, d) if which == 1 else ("split", a, b)
            assert ews and not ews & ~15, (key, ews)
            for ew in EWS:
                if ews & ew:
                    assert (key, ew) not in out, "listed twice: %s" % ((key, ew),)
                    out.add((key, ew))
    return out


def plan(lib, h, row, launch, cus=256, key_helper=True, split_bwd=True):
    """cxl::plan_launch of one launch of a row, as a dict."""
    mode, gp = LAUNCH[launch]
    out = (ctypes.c_long * len(PLAN_FIELDS))()
    n = lib.emu_launch_plan_ex(h, row.ew, row.specialize, mode, row.B, row.n_steps, row.stages, int(gp >= 1),
                               int(gp == 2), cus, int(key_helper), int(split_bwd), ctypes.cast(out, ctypes.c_void_p))
    assert n == len(PLAN_FIELDS)
    return dict(zip(PLAN_FIELDS, out))


def plan_key(p):
    """The ledger's key of a plan."""
    assert not p["error"] and p["listed"] == 1, p
    if p["family"] == STEP:
        return ("step", p["fnset"], p["mode"], p["spec"], p["gp"])
    if p["family"] == SPLIT:
        return ("split", p["nb"], p["spec"])
    return ("help", p["fnset"], p["spec"], p["sdefer"], int(p["family"] == HELP_L1))


# ---------------------------------------------------------------------------
# the rows' scenes, cases and states
# ---------------------------------------------------------------------------
_CASES = {}


def rollout_case(row):
    """(case, per_env) of a rollout row, sliced to the row's envs."""
    import grad_cases as GC
    import grad_geom_cases as GGC
    if row.case not in _CASES:
        if row.case == "robocup16x8":  # tests/test_gpu_parity.py test_rollout_grad_robocup_vs_oracle's
            _CASES[row.case] = (GC.robocup_case(16, 8), False)
        else:
            c = GGC.cases()[row.case]
            _CASES[row.case] = (c[0], c[2])
    case, per_env = _CASES[row.case]
    if row.envs is not None:
        assert not per_env
        e = list(row.envs)
        case = dict(case, S0=case["S0"][e], keys=np.asarray(case["keys"])[e],
                    actions=np.ascontiguousarray(case["actions"][:, e]))
    assert case["S0"].shape[0] == row.B and case["actions"].shape[0] == row.n_steps
    return case, per_env


def eval_setup(row):
    from test_eval_grad_cpu import setup
    s = setup(row.case)
    assert s[0]["S0"].shape[0] == row.B and s[5] * s[6] == row.n_steps and s[8] == row.stages
    return s


def step_scene(row):
    """(bodies, oracle Params or None, dyn f32 [nb, 6, B], keys u32 [B, 2]) of
    a step row: the scenes of tests/test_launch_plan_cpu.py with the states
    their own tests start them from."""
    import grad_cases as GC
    import scene_cases
    from cotix_oracle import cport
    from cotix_oracle import physics as P
    from cotix_oracle.params import Params
    B, name = row.B, row.case
    prm = (Params(prng_layout="partitionable") if name.endswith("_part") else Params(contact_p=0.25)
           if name == "robocup_cp" else None)
    if name.startswith("robocup"):
        dyn, keys = cport.robocup_batch(B)
        return P.robocup_bodies(), prm, dyn, keys
    if name.startswith("lunar") or name == "box":
        case = GC.lunar_case(B, 1, seed=0) if name != "box" else GC.box_case(B, 1, seed=1)
        return (case["make"](), prm, np.ascontiguousarray(case["S0"].transpose(1, 2, 0)),
                np.array(case["keys"], np.uint32))
    bodies = {"convex": lambda: scene_cases.straddle_scene(0.3), "aabb_poly": lambda: scene_cases.mixed_scene(False),
              "circle_poly": lambda: scene_cases.mixed_scene(True)}[name]()
    base = np.array([b.dyn() for b in bodies], np.float32)
    dyn = np.ascontiguousarray(np.repeat(base[:, :, None], B, axis=2))
    dyn[0, 0, :] += np.linspace(-0.3, 0.3, B).astype(np.float32)
    keys = np.ascontiguousarray(np.stack([np.arange(B) + 3, np.arange(B) * 5 + 1], 1).astype(np.uint32))
    return bodies, prm, dyn, keys


def plan_scene(emu, lib, row):
    """The row's scene on an emulation library (for the plan and the runs)."""
    if row.kind == "rollout":
        case, per_env = rollout_case(row)
        return emu.oracle_scene(lib, case["obs"][0] if per_env else case["make"](), per_env_params=per_env)[0]
    if row.kind == "eval":
        return emu.oracle_scene(lib, eval_setup(row)[0]["make"]())[0]
    bodies, prm, _, _ = step_scene(row)
    return emu.oracle_scene(lib, bodies, prm)[0]


# ---------------------------------------------------------------------------
# the rows on the host emulation
# ---------------------------------------------------------------------------
class Libs:
    """The emulation's libraries: the backward with grad_geom (which carries
    cotix_emu.cpp's entry points: forwards, steps, the level-0 backward), with
    grad_params, and the differentiable eval."""

    def __init__(self):
        import emu
        import emu_evalgrad
        import emu_gradg
        import emu_gradp
        self.emu, self.gradg, self.gradp, self.evalgrad = emu, emu_gradg, emu_gradp, emu_evalgrad
        self.g, self.p, self.e = bind(emu_gradg.load()), bind(emu_gradp.load()), bind(emu_evalgrad.load())


_LIBS = []


def libs():
    if not _LIBS:
        _LIBS.append(Libs())
    return _LIBS[0]


def _emu_rollout_scene(L, lib, case, per_env):
    import penv_cases as PC
    if per_env:
        h, _ = L.emu.oracle_scene(lib, case["obs"][0], per_env_params=True)
        geom = PC.rows(lambda ob: L.emu.oracle_scene(lib, ob)[1], case["obs"])
        return h, geom, geom.shape[1]
    h, geom = L.emu.oracle_scene(lib, case["make"]())
    return h, geom, 0


def emu_rollout(row):
    """Every launch of a rollout row on the emulation: ret, the advanced state
    and, per launch, ga / gd / gp / gg under "<what>:<launch>".  tape2 also runs
    with want_params ("gp:tape2")."""
    L = libs()
    case, per_env = rollout_case(row)
    E = row.ew
    h, geom, gs = _emu_rollout_scene(L, L.g, case, per_env)
    hp = _emu_rollout_scene(L, L.p, case, per_env)[0]
    dyn = np.ascontiguousarray(case["S0"].transpose(1, 2, 0))
    keys = np.array(case["keys"], np.uint32, copy=True)
    err = np.zeros(row.B, np.uint32)
    ret, sd, sk, tape = L.emu.rollout(L.g, h, dyn, keys, err, geom, gs, row.stages, case["actions"], case["ab"],
                                      case["w"], E=E)
    out = dict(ret=ret, dyn=dyn, keys=keys, err=err)
    rest = (geom, gs, row.stages, case["actions"], case["ab"], case["w"])
    for launch in launches(row):
        if launch == "fwd":
            continue
        mode, gp = LAUNCH[launch]
        tp = tape if mode == 4 else None
        if gp == 0:
            split = dict(row.keys)[launch][0] == "split"
            L.g.emu_set_split_bwd(int(split))
            try:
                ga, gd = L.emu.rollout_backward(L.g, h, sd, sk, *rest, E=E, tape=tp)
            finally:
                L.g.emu_set_split_bwd(0)
        elif gp == 1:
            ga, gd, out["gp:" + launch] = L.gradp.rollout_backward_params(L.p, hp, sd, sk, *rest, E=E, tape=tp)
        else:
            ga, gd, _, out["gg:" + launch] = L.gradg.rollout_backward_geom(L.g, h, sd, sk, *rest, E=E, tape=tp)
            if mode == 4:
                a2, d2, out["gp:" + launch], g2 = L.gradg.rollout_backward_geom(L.g, h, sd, sk, *rest, E=E, tape=tp,
                                                                                want_params=True)
                assert same_bits(a2, ga) and same_bits(d2, gd) and same_bits(g2, out["gg:" + launch])
        out["ga:" + launch], out["gd:" + launch] = ga, gd
    return out


def emu_eval(row):
    """The three launches of an eval row on the emulation: the fused eval's
    outputs under "<what>:eval", the differentiable eval's as
    tests/test_eval_grad_cpu.py emu_run returns them."""
    from test_eval_grad_cpu import emu_run, eval_dt, state
    L = libs()
    case, j, c, _, _, nfe, wfe, period, stages = eval_setup(row)
    out = emu_run((L.emu, L.evalgrad, L.e), row.case, row.ew)
    dyn, keys, err = state(case)
    rw, fin = np.zeros(row.B, np.float32), np.zeros(row.B, np.uint32)
    L.emu.eval_(L.e, out["h"], dyn, keys, err, out["geom"], 0, nfe, wfe, eval_dt(nfe, wfe, period), stages,
                judge=j.c_struct(), control=c.c_struct(), reward=rw, finished=fin, E=row.ew)
    out.update({"dyn:eval": dyn, "keys:eval": keys, "err:eval": err, "reward:eval": rw, "finished:eval": fin})
    return out


def emu_step(row):
    """A step row on the emulation (the helper form where the row's key is
    one): state, keys, err and the collider trace."""
    L = libs()
    bodies, prm, dyn, keys = step_scene(row)
    h, geom = L.emu.oracle_scene(L.g, bodies, prm)
    dyn, keys, err = dyn.copy(), keys.copy(), np.zeros(row.B, np.uint32)
    L.g.emu_set_key_helper(int(row.keys[0][1][0] == "help"))
    try:
        ch, cl = L.emu.step_ex(L.g, h, dyn, keys, err, geom, 0, row.n_steps, row.stages, len(bodies), E=row.ew)
    finally:
        L.g.emu_set_key_helper(0)
    return dict(dyn=dyn, keys=keys, err=err, chosen=ch, cells=cl)


_EMU = {}


def emu_row(row):
    """A row's emulation run, once per process."""
    if row.id not in _EMU:
        _EMU[row.id] = {"rollout": emu_rollout, "eval": emu_eval, "step": emu_step}[row.kind](row)
    return _EMU[row.id]


# ---------------------------------------------------------------------------
# the rows against their references (emulation and GPU outputs alike)
# ---------------------------------------------------------------------------
def same_bits(x, y):
    """Bit for bit; floats with NaN patterns included (payloads aside)."""
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype != np.float32:
        return x.shape == y.shape and np.array_equal(x.view(np.uint32), np.asarray(y, x.dtype).view(np.uint32))
    y = np.asarray(y, np.float32)
    nx, ny = np.isnan(x), np.isnan(y)
    return x.shape == y.shape and np.array_equal(nx, ny) and np.array_equal(x[~nx].view(np.uint32),
                                                                             y[~ny].view(np.uint32))


def _same_scalar(a, b):
    return (np.isnan(a) and np.isnan(b)) or np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


def check_rollout(row, out, tag):
    """A rollout row's outputs against the torch VJP oracles of its case, at
    the case's tolerances: the return bit for bit, every launch's grad_action
    and grad_dyn0, grad_params (GPC), grad_geom (GGC, with its exact zeros);
    and what the requests may not change."""
    import grad_cases as GC
    import grad_geom_cases as GGC
    import grad_param_cases as GPC
    case, _ = rollout_case(row)
    names = launches(row)
    envs = list(range(row.B)) if row.envs is None else list(row.envs)
    full = _CASES[row.case][0]  # the oracles are per env: a sliced row reads its envs of the whole case's
    if any(LAUNCH[n][1] == 2 for n in names):
        orc = GGC.oracle_of(row.case, full)
        GGC.check_conditions(row.case, orc)
    else:
        if ("GC", row.case) not in _CASES:
            _CASES[("GC", row.case)] = GC.oracle(full)
        orc = _CASES[("GC", row.case)]
    orc_p = None
    if any(LAUNCH[n][1] == 1 for n in names):
        orc_p = GPC.oracle_of(row.case, full)
        GPC.check_conditions(row.case, orc_p)
    pads = GGC.pad_words(full)
    for col, e in enumerate(envs):
        assert _same_scalar(out["ret"][col], orc[e][0]), (row.id, e, out["ret"][col], orc[e][0])
        if orc_p is not None:
            assert _same_scalar(orc_p[e][0], orc[e][0])
        for n in names:
            if n == "fwd":
                continue
            ok, msg = GC.close(out["ga:" + n][:, col], orc[e][1], case["tol"], "%s_%s" % (tag, case["name"]))
            assert ok, "%s %s env %d grad_action: %s" % (row.id, n, e, msg)
            ok, msg = GC.close(out["gd:" + n][:, :, col], orc[e][2], case["tol"], "%s_%s" % (tag, case["name"]))
            assert ok, "%s %s env %d grad_dyn0: %s" % (row.id, n, e, msg)
            if "gp:" + n in out:
                gp, ogp = out["gp:" + n][:, :, col], orc_p[e][3]
                ok, msg = GC.close(gp, ogp, case["tol"], "%s_%s_params" % (tag, case["name"]))
                assert ok, "%s %s env %d grad_params: %s\n%s\n%s" % (row.id, n, e, msg, gp, ogp)
                if np.all(ogp == 0):
                    assert not np.ascontiguousarray(gp).view(np.uint32).any(), (row.id, n, e)
            if "gg:" + n in out:
                gg, ogg = out["gg:" + n][:, col], orc[e][3]
                ok, msg = GC.close(gg, ogg, GGC.tol_of(row.case, case), "%s_%s_geom" % (tag, case["name"]))
                assert ok, "%s %s env %d grad_geom: %s\n%s" % (row.id, n, e, msg, np.stack([gg, ogg], 1))
                if np.all(ogg == 0):
                    assert not np.ascontiguousarray(gg).view(np.uint32).any(), (row.id, n, e)
                assert not np.ascontiguousarray(gg[pads]).view(np.uint32).any(), "a circle's pad word is not zero"
    # tape == re-play; grad_action / grad_dyn0 do not change with the request;
    # the level-2 programs' grad_params are level 1's
    first = None
    for n in names:
        if n == "fwd":
            continue
        first = first or n
        for what in ("ga:", "gd:"):
            assert same_bits(out[what + n], out[what + first]), "%s: %s%s != %s" % (row.id, what, n, first)
    for what, a, b in (("gp:", "tape1", "replay1"), ("gg:", "tape2", "replay2"), ("gp:", "tape2", "tape1")):
        if what + a in out and what + b in out:
            assert same_bits(out[what + a], out[what + b]), "%s: %s %s != %s" % (row.id, what, a, b)
            # every word written: neither the emulation's poison nor the GPU buffers' sentinel is left
            assert not np.any(out[what + a] == np.float32(-7.0)) and not np.any(out[what + a] == SENTINEL_F)


def check_eval(row, out, tag):
    """An eval row's outputs: the saving forward == the fused eval bit for
    bit, the gradients against the oracle (tests/test_eval_grad_cpu.py
    check_vs_oracle: the reward bit for bit), and for the box world's and
    RoboCup's judges the state, keys and error bits against the oracle's
    restatement of the reference loop."""
    import eval_device_cases as EDC
    from test_eval_grad_cpu import check_vs_oracle, orc_of
    case, _, _, _, _, nfe, wfe, period, _ = eval_setup(row)
    for k in ("dyn", "keys", "err", "reward"):
        assert same_bits(out[k], out[k + ":eval"]), "%s: %s of the saving forward != the eval's" % (row.id, k)
    if "finished" in out:
        assert same_bits(out["finished"], out["finished:eval"])
    assert not (out["rec"] == 0xFFFFFFFF).any()  # every record word written
    check_vs_oracle(out, orc_of(row.case), case["tol"], "%s_%s" % (tag, row.case))
    if row.case != "lunar":
        if ("EDC", row.case) not in _CASES:  # once per process, as the other oracles
            _CASES[("EDC", row.case)] = EDC.oracle_eval(case, row.case, nfe, wfe, period)
        want = _CASES[("EDC", row.case)]
        for e, ((bodies, okey, oerr), orew, _) in enumerate(want):
            wd = np.array([b.dyn() for b in bodies], np.float32)
            assert same_bits(np.ascontiguousarray(out["dyn:eval"][:, :, e]), wd), (row.id, e)
            assert np.array_equal(out["keys:eval"][e], okey) and int(out["err:eval"][e]) == int(oerr), (row.id, e)
            assert _same_scalar(out["reward:eval"][e], orew), (row.id, e)


_CPORT = {}


def cport_step(row):
    """The C port of the oracle on a step row's inputs, once per (scene, B,
    steps, stages): the tilings of a scene share it."""
    from cotix_oracle import cport
    key = (row.case, row.B, row.n_steps, row.stages)
    if key not in _CPORT:
        assert os.path.exists(cport.LIB), "oracle C port %s missing: build it first" % cport.LIB
        bodies, prm, dyn, keys = step_scene(row)
        sc = cport.Scene(cport.load(), bodies, prm)
        dyn, keys, err = dyn.copy(), keys.copy(), np.zeros(row.B, np.uint32)
        ch, cl = sc.step_ex(dyn, keys, err, row.n_steps, row.stages, trace=True)
        _CPORT[key] = dict(dyn=dyn, keys=keys, err=err, chosen=ch, cells=cl)
    return _CPORT[key]


def check_step(row, out):
    """State, keys and error bits (and the collider trace where the run has
    one) against the C port, bit for bit."""
    want = cport_step(row)
    if row.stages & 4 and row.case != "lunar" and row.case != "lunar_part":
        assert (want["cells"] >= 0).sum() > 0, "%s: the scene never finds a contact" % row.id
    for k in ("dyn", "keys", "err", "chosen", "cells"):
        if k in out:
            assert same_bits(out[k], want[k]), "%s: %s != the C port's" % (row.id, k)


# ---------------------------------------------------------------------------
# the rows on the GPU (called by tests/test_gpu_kernel_matrix.py only)
# ---------------------------------------------------------------------------
SENTINEL = 0x5EA15EA1  # the guard words' pattern (an int32; as a float 1.4513e18)
SENTINEL_F = np.array([SENTINEL], np.uint32).view(np.float32)[0]
GUARD = 64


class Guarded:
    """Output buffers for the C ABI with GUARD sentinel words after their last
    element.  Every output is packed with the env index innermost or next to
    innermost, so a store past env B - 1 of the last row lands in the guard
    (one past B - 1 of an inner row lands on env 0 of the next row, which the
    comparisons against the references see).  check() asserts the guards
    untouched."""

    def __init__(self, torch):
        self.torch, self.bufs = torch, []

    def new(self, shape, dtype, fill=None):
        torch = self.torch
        n = int(np.prod(shape))
        whole = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.bufs.append((whole, n))
        t = whole[:n].view(dtype).view(*shape)
        if fill is not None:
            t.copy_(fill) if hasattr(fill, "shape") else t.fill_(fill)
        return t

    def f32(self, *shape, fill=None):
        return self.new(shape, self.torch.float32, fill)

    def i32(self, *shape, fill=None):
        return self.new(shape, self.torch.int32, fill)

    def check(self, what):
        self.torch.cuda.synchronize()
        for k, (whole, n) in enumerate(self.bufs):
            assert bool((whole[n:] == SENTINEL).all()), "%s: buffer %d (%d words) was written past its end" % (
                what, k, n)


def device_inputs(torch):
    """The plan's device inputs as the library reads them (cotix_step.hip):
    the compute units, COTIX_KEY_HELPER and COTIX_SPLIT_BWD."""
    def on(name):
        import re
        v = os.environ.get(name)
        if v is None:
            return True
        m = re.match(r"\s*([+-]?\d+)", v)  # atoi
        return bool(m) and int(m.group(1)) != 0
    return dict(cus=torch.cuda.get_device_properties(0).multi_processor_count, key_helper=on("COTIX_KEY_HELPER"),
                split_bwd=on("COTIX_SPLIT_BWD"))


def _np(t):
    return t.detach().cpu().numpy()


def _guard_state(G, w):
    """The world's state tensors re-allocated with guards."""
    w.dyn, w.keys, w.err = G.f32(*w.dyn.shape, fill=w.dyn), G.i32(*w.keys.shape, fill=w.keys), G.i32(
        *w.err.shape, fill=w.err)


def gpu_rollout(torch, row):
    """emu_rollout's dict from the GPU: the row's world as
    tests/test_gpu_grad_geom.py _world builds it, the launches through the C
    ABI with guarded outputs (the calls of parallax_amd/rollout.py)."""
    import parallax_amd as pa
    import ref_standins as RS
    from test_gpu_grad_params import _pa_bodies
    ffi = pa._ffi
    case, per_env = rollout_case(row)
    B, T = row.B, row.n_steps
    keys = torch.tensor(np.asarray(case["keys"], np.uint32).view(np.int32), device="cuda")
    if per_env:
        w = pa.World.from_bodies(RS.stack([RS.from_oracle(ob) for ob in case["obs"]]), device="cuda", keys=keys)
        assert w.scene.per_env_params and w.geom.dim() == 2
    else:
        w = pa.World(_pa_bodies(pa, case["make"]()), B, "cuda", keys)
    w.dyn.copy_(torch.tensor(case["S0"], device="cuda").permute(1, 2, 0))
    w.set_variant(row.ew, bool(row.specialize))
    G = Guarded(torch)
    _guard_state(G, w)
    nb, nblk, h, st = len(w.bodies), (B + 3) // 4, w.scene.handle, ffi.stream_ptr(w.device)
    acts = torch.tensor(case["actions"], device="cuda").contiguous()
    wts = np.ascontiguousarray(np.asarray(case["w"], np.float32).reshape(-1))
    wp = wts.ctypes.data_as(ffi._P)
    ret = G.f32(B, fill=0.0)
    sd, sk = G.f32(T, nblk, nb * 6, 4), G.i32(T, B, 2)
    tape = G.i32(T, nblk, ffi.lib.cotix_rollout_tape_words(h), 4)
    ffi.check(ffi.lib.cotix_rollout_ex(h, ffi.ptr(w.dyn), ffi.ptr(w.keys), ffi.ptr(w.err), ffi.ptr(w.geom),
                                       w.geom_stride, B, T, 1e-2, row.stages, ffi.ptr(acts), case["ab"], wp,
                                       ffi.ptr(ret), ffi.ptr(sd), ffi.ptr(sk), ffi.ptr(tape), st), "cotix_rollout_ex")
    G.check(row.id + " fwd")
    out = dict(ret=_np(ret), dyn=_np(w.dyn), keys=_np(w.keys).view(np.uint32), err=_np(w.err).view(np.uint32))

    def backward(launch, want_params, want_geom):
        mode = LAUNCH[launch][0]
        ga, gd = G.f32(T, B, 2), G.f32(nb, 6, B)
        gp = G.f32(nb, 4, B) if want_params else None
        gg = G.f32(w.scene.geom_part_words, B) if want_geom else None
        ffi.check(ffi.lib.cotix_rollout_backward_ex3(
            h, ffi.ptr(sd), ffi.ptr(sk), ffi.ptr(tape if mode == 4 else None), ffi.ptr(w.geom), w.geom_stride, B, T,
            1e-2, row.stages, ffi.ptr(acts), case["ab"], wp, ffi.ptr(ga), ffi.ptr(gd), ffi.ptr(gp), ffi.ptr(gg), st),
            "cotix_rollout_backward_ex3")
        G.check("%s %s" % (row.id, launch))
        return [None if x is None else _np(x) for x in (ga, gd, gp, gg)]

    for launch in launches(row):
        if launch == "fwd":
            continue
        mode, gp = LAUNCH[launch]
        ga, gd, p, g = backward(launch, gp == 1, gp == 2)
        out["ga:" + launch], out["gd:" + launch] = ga, gd
        if p is not None:
            out["gp:" + launch] = p
        if g is not None:
            out["gg:" + launch] = g
            if mode == 4:  # ... and with want_params: the same kernel, its grad_params level 1's bits
                a2, d2, out["gp:" + launch], g2 = backward(launch, True, True)
                assert same_bits(a2, ga) and same_bits(d2, gd) and same_bits(g2, g)
    return out


def gpu_eval(torch, row):
    """emu_eval's dict from the GPU: the env of tests/test_gpu_eval_grad.py
    make_env at the row's variant, env.eval's launch on guarded state tensors
    (World.eval_state) and the differentiable eval's two through the C ABI
    with guarded outputs (the calls of parallax_amd/eval_grad.py)."""
    import parallax_amd as pa
    from test_gpu_eval_grad import make_env
    ffi = pa._ffi
    env, (nfe, wfe, period) = make_env(torch, row.case)
    w = env.world.world
    w.set_variant(row.ew, bool(row.specialize))
    B, T, nb = row.B, nfe * wfe, len(w.bodies)
    dt = pa.eval_grad._eval_dt(period, nfe, wfe)
    judge, control = env.judge.c_struct(), env.control.c_struct()
    G = Guarded(torch)
    out = {}
    # mode 3
    s = env.state
    dyn, keys, err = G.f32(*s.dyn.shape, fill=s.dyn), G.i32(*s.keys.shape, fill=s.keys), G.i32(*s.err.shape,
                                                                                                 fill=s.err)
    rw, fin = G.f32(B, fill=0.0), G.i32(B, fill=0)
    w.eval_state(dyn, keys, err, nfe, wfe, dt, int(env.world.stages), judge=judge, control=control, reward=rw,
                 finished=fin)
    G.check(row.id + " eval")
    out.update({"dyn:eval": _np(dyn), "keys:eval": _np(keys).view(np.uint32), "err:eval": _np(err).view(np.uint32),
                "reward:eval": _np(rw), "finished:eval": _np(fin).view(np.uint32)})
    # mode 5
    dyn, keys, err = G.f32(*s.dyn.shape, fill=s.dyn), G.i32(*s.keys.shape, fill=s.keys), G.i32(*s.err.shape,
                                                                                                 fill=s.err)
    rw, fin = G.f32(B, fill=0.0), G.i32(B, fill=0)
    nblk, h, st = (B + 3) // 4, w.scene.handle, ffi.stream_ptr(w.device)
    sd, sk = G.f32(T, nblk, nb * 6, 4), G.i32(T, B, 2)
    tape = G.i32(T, nblk, ffi.lib.cotix_rollout_tape_words(h), 4)
    rec = G.i32(T + 1, B, fill=-1)
    ffi.check(ffi.lib.cotix_eval_rollout(h, ffi.ptr(dyn), ffi.ptr(keys), ffi.ptr(err), ffi.ptr(w.geom), w.geom_stride,
                                         B, nfe, wfe, dt, int(env.world.stages), judge, control, None, 0, ffi.ptr(rw),
                                         ffi.ptr(fin), ffi.ptr(sd), ffi.ptr(sk), ffi.ptr(tape), ffi.ptr(rec), st),
              "cotix_eval_rollout")
    G.check(row.id + " eval_fwd")
    # mode 6
    gc, gd, gv = G.f32(26, B), G.f32(nb, 6, B), G.f32(T, B, 2)
    ffi.check(ffi.lib.cotix_eval_backward(h, ffi.ptr(sd), ffi.ptr(sk), ffi.ptr(tape), ffi.ptr(rec), ffi.ptr(w.geom),
                                          w.geom_stride, B, nfe, wfe, dt, int(env.world.stages), judge, control, None,
                                          ffi.ptr(gc), ffi.ptr(gd), ffi.ptr(gv), None, st), "cotix_eval_backward")
    G.check(row.id + " eval_bwd")
    out.update(dyn=_np(dyn), keys=_np(keys).view(np.uint32), err=_np(err).view(np.uint32), reward=_np(rw),
               finished=_np(fin).view(np.uint32), rec=_np(rec).view(np.uint32), gc=_np(gc), gd=_np(gd), gv=_np(gv))
    return out


def gpu_step(torch, row):
    """A step row on the GPU: World.step_state on guarded state tensors;
    (outputs, cotix_scene_last_step_form)."""
    import parallax_amd as pa
    from test_gpu_parity import _world_from_oracle
    bodies, prm, dyn0, keys0 = step_scene(row)
    if prm is None:
        w = _world_from_oracle(pa, torch, bodies, row.B, keys0)
    else:  # (the same world under the scene's parameter block)
        from test_gpu_grad_params import _pa_bodies
        kw = {"prng_layout": "partitionable"} if row.case.endswith("_part") else {"contact_p": 0.25}
        w = pa.World(_pa_bodies(pa, bodies), row.B, "cuda", torch.tensor(keys0.view(np.int32), device="cuda"),
                     params=pa.Params(**kw))
    w.set_variant(row.ew, bool(row.specialize))
    G = Guarded(torch)
    dyn, keys = G.f32(*dyn0.shape, fill=torch.tensor(dyn0)), G.i32(row.B, 2, fill=torch.tensor(keys0.view(np.int32)))
    err = G.i32(row.B, fill=0)
    w.step_state(dyn, keys, err, row.n_steps, 1e-2, row.stages)
    G.check(row.id)
    form = pa._ffi.lib.cotix_scene_last_step_form(w.scene.handle)
    return dict(dyn=_np(dyn), keys=_np(keys).view(np.uint32), err=_np(err).view(np.uint32)), form
