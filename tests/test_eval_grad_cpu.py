"""The differentiable eval (cotix_eval_rollout / cotix_eval_backward) on CPU:
the kernel's saving eval forward and its tape backward (host emulation,
tests/emu/cotix_emu_evalgrad.cpp -- the GPU's bits by construction) against
the torch-f32 VJP oracle with the control's 26 parameters as a leaf
(tests/eval_grad_cases.py), itself checked against central differences of the
faithful oracle's eval reward."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import eval_device_cases as EDC
import eval_grad_cases as EGC
import grad_cases as GC

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
F = np.float32


@pytest.fixture(scope="module")
def libs():
    import emu
    import emu_evalgrad
    emu_evalgrad.build("libcotix_emu_evalgrad.so", "libcotix_emu_evalgrad_nogregs.so", "evalgrad_asan_driver")
    return emu, emu_evalgrad, emu_evalgrad.load()


def setup(name):
    """(case, judge, control, judge kwargs, control kwargs, nfe, wfe, period, stages) of a named case."""
    from parallax_amd import envs as PE
    if name == "lunar":
        case = EGC.lunar4()
        jk, ck = EGC.LUNAR_JUDGE, EGC.LUNAR_CONTROL
        return (case, PE.LinearJudge(**jk), PE.AffineControl(**ck), jk, ck, *EGC.LUNAR, EGC.LUNAR_STAGES)
    if name == "goal":
        case = EDC.case("robocup", 6, seed=5)
        jk, ck = EDC.judges("goal", case["ab"])
        return (case, *EDC.device("goal", case["ab"]), jk, ck, 3, 4, 0.24, EGC.BOX_STAGES)
    case = EGC.box8()
    jk, ck = EDC.judges(name, case["ab"])
    return (case, *EDC.device(name, case["ab"]), jk, ck, *EGC.BOX[name], EGC.BOX_STAGES)


def orc_of(name):
    case, _, _, jk, ck, nfe, wfe, period, _ = setup(name)
    return EGC.oracle_of(name, case, None, nfe, wfe, period, judge=jk, control=ck)


def eval_dt(nfe, wfe, period):
    return float(F(F(period / nfe) / F(float(wfe))))


def state(case, envs=None):
    S0, keys = case["S0"], np.asarray(case["keys"], np.uint32)
    if envs is not None:
        S0, keys = S0[envs], keys[envs]
    dyn = np.ascontiguousarray(S0.transpose(1, 2, 0)).astype(np.float32)
    return dyn, np.array(keys, np.uint32), np.zeros(dyn.shape[2], np.uint32)


def emu_run(libs_, name, E=4, lib=None, envs=None, finished=None, reward=None):
    """The saving forward then the backward: dict of everything they return."""
    emu, eg, plain = libs_
    lib = plain if lib is None else lib
    case, j, c, _, _, nfe, wfe, period, stages = setup(name)
    h, geom = emu.oracle_scene(lib, case["make"]())
    dyn, keys, err = state(case, envs)
    B = dyn.shape[2]
    rw = np.zeros(B, np.float32) if reward is None else np.array(reward, np.float32)
    fin = np.zeros(B, np.uint32) if finished is None else np.array(finished, np.uint32)
    dt = eval_dt(nfe, wfe, period)
    sd, sk, tp, rec = eg.eval_rollout(lib, h, dyn, keys, err, geom, 0, nfe, wfe, dt, stages, j.c_struct(), c.c_struct(),
                                      rw, fin, E=E)
    gc, gd, gv = eg.eval_backward(lib, h, sd, sk, tp, rec, geom, 0, nfe, wfe, dt, stages, j.c_struct(), c.c_struct(),
                                  E=E)
    return dict(dyn=dyn, keys=keys, err=err, reward=rw, finished=fin, rec=rec, gc=gc, gd=gd, gv=gv, sd=sd, sk=sk,
                tape=tp, h=h, geom=geom)


def check_vs_oracle(got, orc, tol, tag, envs=None):
    """grad_control, grad_dyn0, grad_dv of every env against the oracle; exact
    zeros after the episode's end."""
    for col, e in enumerate(sorted(orc) if envs is None else envs):
        o = orc[e]
        assert EGC.same_bits(got["reward"][col], o["reward"]), (e, got["reward"][col], o["reward"])
        for nm, g, w in (("control", got["gc"][:, col], o["g_control"]), ("dyn0", got["gd"][:, :, col], o["g_dyn0"]),
                         ("dv", got["gv"][:, col], o["g_dv"])):
            ok, msg = GC.close(g, w, tol, "eval_%s_%s" % (tag, nm))
            assert ok, "env %d grad_%s: %s\n%s\n%s" % (e, nm, msg, g, w)
        n = o["n"]  # the chain's steps: t* or T
        assert not got["gv"][n:, col].view(np.uint32).any(), "env %d: d reward / d dv after the episode's end" % e
        if o["tstar"] == 0:  # done at entry: no step counts, the entry state's adjoint is end_w
            assert not got["gc"][:, col].view(np.uint32).any()


# ---------------------------------------------------------------------------
# 1. the checker of the checker
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["x_done", "multi", "piecewise", "lunar", "goal"])
def test_oracle_conditions(name):
    """What the oracle alone says about each case (the issue's conditions), and
    its reward == the restated reference loop's (oracle_eval) bit for bit."""
    case, _, _, jk, ck, nfe, wfe, period, _ = setup(name)
    orc = orc_of(name)
    T = nfe * wfe
    if name in EGC.BOX or name == "goal":
        want = EDC.oracle_eval(case, name, nfe, wfe, period)
        for e in orc:
            assert EGC.same_bits(orc[e]["reward"], want[e][1]), (e, orc[e]["reward"], want[e][1])
            assert bool(want[e][2]) == (orc[e]["tstar"] is not None)
    if name in EGC.BOX:
        for e, ts in EGC.BOX_TSTAR[name].items():
            assert orc[e]["tstar"] == ts, (e, orc[e]["tstar"], ts)
    if name in ("x_done", "piecewise"):
        assert T > 16  # the launch crosses the 16-step key window
    if name == "multi":
        assert orc[2]["tstar"] % wfe == 0  # the last step of an NFE
    if name == "piecewise":
        assert orc[2]["tstar"] % wfe == 0
        # both clip regimes on the chain (the steps up to t*) of envs 0, 3, 4, 5; env 7's 17 chain steps are
        # all saturated (its unsaturated outputs come after its t*, where the forward steps on off the chain)
        for e in (0, 3, 4, 5):
            s = orc[e]["sat"][:orc[e]["n"]]
            assert (s == 0).any() and (s == 1).any(), e
        assert (orc[7]["sat"][:orc[7]["n"]] == 0).all()
        regs = set(r for e in orc for r in orc[e]["regions"][1:])
        assert regs == {-1, 0, 1}, regs
        assert all(np.isfinite(np.stack(orc[e]["states"])).all() for e in orc)
    if name == "lunar":
        ts = [orc[e]["tstar"] for e in sorted(orc)]
        assert any(t is not None and 0 < t < T for t in ts) and any(t is None for t in ts), ts
        s = np.concatenate([orc[e]["sat"][:orc[e]["n"]].reshape(-1) for e in orc])
        assert (s == 0).any() and (s == 1).any()
    if name == "goal":
        assert all(orc[e]["tstar"] == 2 for e in orc)
        assert all(np.isnan(orc[e]["g_control"]).any() for e in orc)


@pytest.mark.parametrize("e", [0, 4])
def test_oracle_vs_finite_differences(e):
    """The theta-leaf VJP chain against central differences (h = 1e-3) of the
    faithful oracle's eval reward in gain, target and bias entries of two
    finite box envs (x_done: env 0 done at step 26 of 30, env 4 live), at
    2e-3 (1 + |fd|) -- the bar of test_oracle_grad_vs_finite_differences."""
    case, _, _, jk, ck, nfe, wfe, period, _ = setup("x_done")
    o = orc_of("x_done")[e]
    entries = [0, 2, 9, 14, 21, 24, 25]  # structurally zero gains (0) and biases (24, 25) included
    fds = EGC.fd_theta(case, jk, ck, e, nfe, wfe, period, entries, h=1e-3)
    assert np.isfinite(o["g_control"]).all() and np.any(o["g_control"] != 0)
    for k, fd in zip(entries, fds):
        g = float(o["g_control"][k])
        print("env %d theta[%d]: vjp %.6g fd %.6g" % (e, k, g, fd))
        assert abs(fd - g) <= 2e-3 * (1 + abs(fd)), (k, fd, g)


# ---------------------------------------------------------------------------
# 2. emulation: the saving forward == the eval, the gradients vs the oracle
# ---------------------------------------------------------------------------
CASES = [("x_done", 4), ("x_done", 1), ("multi", 4), ("piecewise", 4), ("piecewise", 2), ("lunar", 1), ("lunar", 4),
         ("goal", 4)]


@pytest.mark.parametrize("name,E", CASES)
def test_saving_forward_equals_eval(libs, name, E):
    emu, eg, lib = libs
    case, j, c, _, _, nfe, wfe, period, stages = setup(name)
    got = emu_run(libs, name, E)
    dyn, keys, err = state(case)
    B = dyn.shape[2]
    rw, fin = np.zeros(B, np.float32), np.zeros(B, np.uint32)
    emu.eval_(lib, got["h"], dyn, keys, err, got["geom"], 0, nfe, wfe, eval_dt(nfe, wfe, period), stages,
              judge=j.c_struct(), control=c.c_struct(), reward=rw, finished=fin, E=E)
    assert EGC.same_bits(got["dyn"], dyn) and np.array_equal(got["keys"], keys) and np.array_equal(got["err"], err)
    assert EGC.same_bits(got["reward"], rw) and np.array_equal(got["finished"], fin)
    assert not (got["rec"] == 0xFFFFFFFF).any()  # every record word written


@pytest.mark.parametrize("name,E", CASES)
def test_emu_gradients_vs_oracle(libs, name, E):
    case = setup(name)[0]
    check_vs_oracle(emu_run(libs, name, E), orc_of(name), case["tol"], name)


def test_ragged_batch(libs):
    """Envs 0..5 sliced out of the 8-env case (a batch's keys depend on its
    size): a partly filled wave, and the restore without 16-byte rows."""
    envs = list(range(6))
    for name in ("x_done", "piecewise"):
        got = emu_run(libs, name, 4, envs=envs)
        check_vs_oracle(got, orc_of(name), GC.ANALYTIC_TOL, name + "_ragged", envs=envs)
        full = emu_run(libs, name, 4)
        for k in ("gc", "gd", "gv"):
            assert EGC.same_bits(got[k], full[k][..., :6] if k != "gv" else full[k][:, :6]), k


def test_finished_at_entry_is_exact_zero(libs):
    """An env whose carry says finished contributes exact zeros everywhere and
    keeps its reward (x_done env 1, done at entry; env 3 for contrast)."""
    fin = np.zeros(8, np.uint32)
    fin[1] = 1
    rin = np.full(8, 0.5, np.float32)
    got = emu_run(libs, "x_done", 4, finished=fin, reward=rin)
    assert got["reward"][1] == np.float32(0.5) and got["finished"][1] == 1
    assert (got["rec"][:, 1] == 4).all()
    for k, sl in (("gc", got["gc"][:, 1]), ("gd", got["gd"][:, :, 1]), ("gv", got["gv"][:, 1])):
        assert not np.ascontiguousarray(sl).view(np.uint32).any(), k
    ref = emu_run(libs, "x_done", 4)
    for k in ("gc", "gd", "gv"):  # the other envs' gradients do not see the carry
        a, b = np.delete(got[k], 1, axis=-1 if k != "gv" else 1), np.delete(ref[k], 1, axis=-1 if k != "gv" else 1)
        assert EGC.same_bits(a, b), k
    assert np.any(ref["gd"][:, :, 1] != 0)  # (not finished: the entry state's adjoint is end_w)


# ---------------------------------------------------------------------------
# 3. form equalities (bit for bit, NaN patterns included)
# ---------------------------------------------------------------------------
KEYS = ("dyn", "keys", "err", "reward", "finished", "rec", "gc", "gd", "gv")


def same_any(a, b):
    return EGC.same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b)


@pytest.mark.parametrize("name", ["x_done", "piecewise", "lunar", "goal"])
def test_tilings_agree(libs, name):
    ref = emu_run(libs, name, 1)
    for E in (2, 4, 8):
        got = emu_run(libs, name, E)
        for k in KEYS:
            assert same_any(ref[k], got[k]), (E, k)


def test_register_chain_equals_tile_form(libs):
    """g_chain in registers (5 and 7 bodies) against ph_G's tile form on the
    same scenes (the -DCOTIX_NO_GREGS build)."""
    _, eg, _ = libs
    tile = eg.load(nogregs=True)
    for name in ("x_done", "piecewise", "goal"):
        a, b = emu_run(libs, name, 4), emu_run(libs, name, 4, lib=tile)
        for k in ("gc", "gd", "gv", "reward"):
            assert EGC.same_bits(a[k], b[k]), (name, k)


# ---------------------------------------------------------------------------
# 4. the sanitizers, on a stand-alone program
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,E", [("piecewise", 4), ("lunar", 4)])
def test_asan_driver(libs, tmp_path, name, E):
    """tests/emu/evalgrad_asan_driver (-fsanitize=address,undefined
    -fno-sanitize-recover=all, its own main, no preloaded runtime): both
    launches into exactly sized buffers exit cleanly, the forward == the eval
    inside it, and its output equals the plain emulation's bits."""
    from test_emu_asan import _scene_arrays
    case, j, c, _, _, nfe, wfe, period, stages = setup(name)
    params, pb, pt, pn, geom = _scene_arrays(case["make"]())
    dyn, keys, _ = state(case)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([dyn.shape[0], len(pb), dyn.shape[2], nfe, wfe, stages, len(geom), 0, E], np.int32).tofile(f)
        np.array([eval_dt(nfe, wfe, period)], np.float32).tofile(f)
        for x in (params, pb, pt, pn, geom, dyn, keys):
            np.ascontiguousarray(x).tofile(f)
        f.write(bytes(j.c_struct()))
        f.write(bytes(c.c_struct()))
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([os.path.join(HERE, "emu", "build", "evalgrad_asan_driver"), inp, out], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    got = emu_run(libs, name, E)
    want = np.concatenate([np.ascontiguousarray(got[k]).reshape(-1).view(np.uint8) for k in KEYS])
    assert np.array_equal(np.fromfile(out, np.uint8), want)


# ---------------------------------------------------------------------------
# 5. the C ABI's argument checks (nothing is launched) and the Python surface
# ---------------------------------------------------------------------------
def test_argument_checks():
    import torch
    import parallax_amd as pa
    lib = pa._ffi.lib
    for name in ("cotix_eval", "cotix_rollout_ex", "cotix_rollout_backward_ex2", "cotix_eval_rollout",
                 "cotix_eval_backward"):
        assert hasattr(lib, name) and name in pa._ffi.SIGNATURES
    w = pa.World(pa.scenarios.robocup_bodies(), 4, "cpu", torch.zeros(4, 2, dtype=torch.int32))
    j, c = EDC.device("goal", 4)
    js, cs = j.c_struct(), c.c_struct()
    fake = ctypes.c_void_p(4096)  # never dereferenced: the checks fail first
    st = pa._ffi.STAGES_ROBOCUP

    def fwd(judge=js, action=None, tape=fake, rec=fake):
        return lib.cotix_eval_rollout(w.scene.handle, fake, fake, fake, fake, 0, 4, 2, 3, 1e-2, st, judge, cs, action, 0,
                                      fake, fake, fake, fake, tape, rec, None)

    def bwd(judge=js, control=cs, action=None, tape=fake, gc=fake, gp=None, rec=fake, stages=st):
        return lib.cotix_eval_backward(w.scene.handle, fake, fake, tape, rec, fake, 0, 4, 2, 3, 1e-2, stages, judge,
                                       control, action, gc, None, None, gp, None)

    for call, word in ((lambda: fwd(judge=None), b"judge"), (lambda: fwd(tape=None), b"tape"),
                       (lambda: fwd(action=fake), b"held action"), (lambda: fwd(rec=None), b"null"),
                       (lambda: bwd(judge=None), b"judge"), (lambda: bwd(tape=None), b"tape"),
                       (lambda: bwd(control=None), b"grad_control"), (lambda: bwd(action=fake), b"held action"),
                       (lambda: bwd(gp=fake), b"grad_params"), (lambda: bwd(rec=None), b"null"),
                       (lambda: bwd(stages=pa._ffi.STAGES_LUNAR), b"LunarLander")):
        assert call() != 0 and word in lib.cotix_last_error(), (word, lib.cotix_last_error())
    # AffineControl.params() / with_params(): the control stays immutable
    th = c.params()
    assert tuple(th.shape) == (26,) and th.dtype == torch.float32
    assert np.array_equal(th.numpy(), EGC.theta_of(EDC.judges("goal", 4)[1]))
    c2 = c.with_params(th + 1.0)
    assert c2 is not c and c2.body == c.body and c2.clip == c.clip
    assert np.array_equal(c2.params().numpy(), (th + 1.0).numpy()) and np.array_equal(c.params().numpy(), th.numpy())
    pj, pc = EDC.device("piecewise", 6)
    assert pc.with_params(pc.params()).clip == pc.clip and pc.with_params(pc.params()).gain == pc.gain
    with pytest.raises(ValueError, match="26"):
        c.with_params(torch.zeros(25))
    assert pa.differentiable_eval is pa.eval_grad.differentiable_eval
    env = pa.AbstractEnvironment(pa.PhysicsWorld(w), pa.WorldState(w.dyn, w.keys, w.err), c, j)
    with pytest.raises(ValueError, match=r"float32 \[26\]"):
        pa.differentiable_eval(env, 0.1, 1, 2, control_params=torch.zeros(25))
