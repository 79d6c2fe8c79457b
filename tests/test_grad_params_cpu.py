"""Gradients of the rollout's return with respect to the body parameters
(mass, inertia, elasticity, friction_coefficient; cotix_rollout_backward_ex2's
grad_params) on CPU: the kernel's backward wave programs with the parameter
adjoint (host emulation, tests/emu/cotix_emu_gradp.cpp -- the GPU's bits by
construction) against the torch-f32 VJP oracle with the parameters as a leaf
(tests/grad_param_cases.py), itself checked against central differences of
the faithful oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grad_cases as GC
import grad_param_cases as GPC
import penv_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))


@pytest.fixture(scope="module")
def libs():
    import emu
    import emu_gradp
    emu_gradp.build("libcotix_emu_gradp.so", "libcotix_emu_gradp_nogregs.so", "gradp_asan_driver")
    return emu, emu_gradp, emu_gradp.load()


def emu_scene(emu, lib, case, per_env):
    """(scene handle, geometry, geometry stride) of a case on the emulation."""
    if per_env:
        h, _ = emu.oracle_scene(lib, case["obs"][0], per_env_params=True)
        geom = PC.rows(lambda ob: emu.oracle_scene(lib, ob)[1], case["obs"])
        return h, geom, geom.shape[1]
    h, geom = emu.oracle_scene(lib, case["make"]())
    return h, geom, 0


def emu_run(emu, emu_gradp, lib, case, stages, per_env=False, E=4, replay=False):
    """Forward, then the backward with grad_params: (ret, ga, gd, gp) and the
    arguments to run another backward on the same forward."""
    h, geom, gs = emu_scene(emu, lib, case, per_env)
    dyn = np.ascontiguousarray(case["S0"].transpose(1, 2, 0))
    keys = np.array(case["keys"], np.uint32, copy=True)
    err = np.zeros(dyn.shape[2], np.uint32)
    ret, sd, sk, tape = emu.rollout(lib, h, dyn, keys, err, geom, gs, stages, case["actions"], case["ab"], case["w"],
                                    E=E)
    args = (h, sd, sk, geom, gs, stages, case["actions"], case["ab"], case["w"])
    ga, gd, gp = emu_gradp.rollout_backward_params(lib, *args, E=E, tape=None if replay else tape)
    return ret, ga, gd, gp, args, tape


# ---------------------------------------------------------------------------
# 1. the checker of the checker
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["box", "lunar"])
def test_param_oracle_vs_finite_differences(scene):
    """The theta-leaf VJP chain against central differences of the faithful
    oracle's return (h = 1e-2 max(1, |p|)): six parameter entries with a
    nonzero finite gradient and a finite parameter, 2e-3 (1 + |fd|) -- the bar
    of test_oracle_grad_vs_finite_differences -- and 5e-2 (1 + |fd|) for
    gradients below 1e-3, where the differences' noise dominates.  The action
    gradients stay bit-identical to the constant-parameter oracle's."""
    case, e = (GC.box_case(5, 16, seed=1), 1) if scene == "box" else (GC.lunar_case(2, 6, seed=0), 0)
    ret, ga, gS, gp = GPC.oracle(case, [e])[e]
    r0, ga0, gS0 = GC.oracle(case, [e])[e]
    assert np.array_equal(ga.view(np.uint32), ga0.view(np.uint32))
    assert np.array_equal(gS.view(np.uint32), gS0.view(np.uint32))
    par = GPC._body_params(case["make"]())
    cand = [(b, k) for b in range(par.shape[0]) for k in range(4)
            if np.isfinite(par[b, k]) and np.isfinite(gp[b, k]) and gp[b, k] != 0]
    cand.sort(key=lambda bk: -abs(gp[bk]))
    entries = cand[:6]
    assert len(entries) == 6, cand
    for (b, k), fd in zip(entries, GPC.fd_params(case, e, entries)):
        g = float(gp[b, k])
        print("%s env %d body %d param %d: vjp %.6g fd %.6g" % (scene, e, b, k, g, fd))
        tol = (5e-2 if abs(g) < 1e-3 else 2e-3) * (1 + abs(fd))
        assert abs(fd - g) <= tol, (b, k, fd, g)


# ---------------------------------------------------------------------------
# 2. emulation vs oracle
# ---------------------------------------------------------------------------
CASES = [(n, E) for n, (_, _, _, Es) in GPC.cases().items() for E in Es]


@pytest.mark.parametrize("name,E", CASES)
def test_emu_grad_params_vs_oracle(libs, name, E):
    emu, emu_gradp, lib = libs
    case, stages, per_env, _ = GPC.cases()[name]
    orc = GPC.oracle_of(name, case)
    GPC.check_conditions(name, orc)
    ret, ga, gd, gp, args, tape = emu_run(emu, emu_gradp, lib, case, stages, per_env, E)
    for e in orc:
        r, oga, ogS, ogp = orc[e]
        same = (np.isnan(ret[e]) and np.isnan(r)) or np.float32(ret[e]).view(np.uint32) == np.float32(r).view(
            np.uint32)
        assert same, (e, ret[e], r)
        ok, msg = GC.close(gp[:, :, e], ogp, case["tol"], case["name"] + "_params")
        assert ok, "env %d grad_params: %s\n%s\n%s" % (e, msg, gp[:, :, e], ogp)
        ok, msg = GC.close(ga[:, e], oga, case["tol"])
        assert ok, "env %d grad_action: %s" % (e, msg)
        if np.all(ogp == 0):  # (box 6x32 env 0: nothing resolved) exact zeros from the kernel
            assert np.array_equal(gp[:, :, e].view(np.uint32), np.zeros((gp.shape[0], 4), np.uint32))
    # the call with grad_params changes nothing else
    pa_, pd_ = emu.rollout_backward(lib, *args, E=E, tape=tape)
    assert GPC.same_bits(ga, pa_), "grad_action changes with grad_params"
    assert GPC.same_bits(gd, pd_), "grad_dyn0 changes with grad_params"


# ---------------------------------------------------------------------------
# 3. form equalities (bit for bit, NaN patterns included)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,E", CASES)
def test_tape_equals_replay(libs, name, E):
    emu, emu_gradp, lib = libs
    case, stages, per_env, _ = GPC.cases()[name]
    _, ga, gd, gp, args, tape = emu_run(emu, emu_gradp, lib, case, stages, per_env, E)
    ra, rd, rp = emu_gradp.rollout_backward_params(lib, *args, E=E)
    assert GPC.same_bits(ga, ra) and GPC.same_bits(gd, rd)
    assert GPC.same_bits(gp, rp), "grad_params: tape != re-play"


def test_register_chain_equals_tile_form(libs):
    """g_chain in registers (5 and 7 bodies) against ph_G's tile form on the
    same scenes (the -DCOTIX_NO_GREGS build)."""
    emu, emu_gradp, lib = libs
    tile = emu_gradp.load(nogregs=True)
    for case in (GC.box_case(6, 32, seed=1), GC.robocup_case(8, 6)):
        a = emu_run(emu, emu_gradp, lib, case, GPC.BOX_STAGES)
        b = emu_run(emu, emu_gradp, tile, case, GPC.BOX_STAGES)
        for x, y, what in zip(a[:4], b[:4], ("ret", "grad_action", "grad_dyn0", "grad_params")):
            assert GPC.same_bits(x, y), what


@pytest.mark.parametrize("name", ["box6x32", "lunar4x8", "robocup8x6", "lunar_penv4x8"])
def test_tilings_agree(libs, name):
    """One env per wave == four == eight (every envs_per_wave tiling runs the
    same chain per env)."""
    emu, emu_gradp, lib = libs
    case, stages, per_env, _ = GPC.cases()[name]
    ref = emu_run(emu, emu_gradp, lib, case, stages, per_env, 1)
    for E in (2, 4, 8):
        got = emu_run(emu, emu_gradp, lib, case, stages, per_env, E)
        for x, y, what in zip(ref[:4], got[:4], ("ret", "grad_action", "grad_dyn0", "grad_params")):
            assert GPC.same_bits(x, y), (E, what)


# (the split producer / consumer form does not carry the parameter adjoint:
# the library launches the one-wave tape backward when grad_params is
# requested, DESIGN.md section 13 -- so there is no split == one-wave case)


# ---------------------------------------------------------------------------
# 4. the sanitizers, on a stand-alone program
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scene,E", [("box", 1), ("box", 4), ("lunar", 1), ("lunar", 4)])
def test_asan_driver(libs, tmp_path, scene, E):
    """tests/emu/gradp_asan_driver (-fsanitize=address,undefined
    -fno-sanitize-recover=all, its own main, no preloaded runtime): the
    backward with grad_params into exactly sized buffers exits cleanly, tape ==
    re-play inside it, and its output equals the plain emulation's bits."""
    emu, emu_gradp, lib = libs
    from test_emu_asan import _scene_arrays
    case, stages = (GC.box_case(5, 8, seed=1), GPC.BOX_STAGES) if scene == "box" else (GC.lunar_case(2, 4, seed=0),
                                                                                     GPC.LUNAR_STAGES)
    params, pb, pt, pn, geom = _scene_arrays(case["make"]())
    B, T = case["S0"].shape[0], case["actions"].shape[0]
    dyn = np.ascontiguousarray(case["S0"].transpose(1, 2, 0))
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([dyn.shape[0], len(pb), B, T, stages, len(geom), 0, 1, E, case["ab"]], np.int32).tofile(f)
        for x in (params, pb, pt, pn, geom, dyn, np.asarray(case["keys"], np.uint32),
                  np.ascontiguousarray(case["actions"], np.float32), np.asarray(case["w"], np.float32)):
            np.ascontiguousarray(x).tofile(f)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([os.path.join(HERE, "emu", "build", "gradp_asan_driver"), inp, out], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    ret, ga, gd, gp, _, _ = emu_run(emu, emu_gradp, lib, case, stages, False, E)
    want = np.concatenate([x.reshape(-1).view(np.uint8) for x in (ret, ga, gd, gp)])
    assert np.array_equal(np.fromfile(out, np.uint8), want)


# ---------------------------------------------------------------------------
# 5. the C ABI's argument checks (nothing is launched)
# ---------------------------------------------------------------------------
def test_ex2_argument_checks_and_old_entry_points():
    import ctypes
    import torch
    import parallax_amd as pa
    import ref_standins as RS
    lib = pa._ffi.lib
    for name in ("cotix_rollout_backward", "cotix_rollout_backward_ex", "cotix_rollout_backward_ex2"):
        assert hasattr(lib, name) and name in pa._ffi.SIGNATURES
    w = pa.World.from_bodies(RS.stack([RS.from_oracle(ob) for ob in PC.lunar_penv_bodies(2)]), device="cpu")
    assert w.scene.per_env_params
    fake = ctypes.c_void_p(4096)  # never dereferenced: the checks fail first
    wts = np.zeros(24, np.float32)
    call = lambda geom, stride: lib.cotix_rollout_backward_ex2(  # noqa: E731
        w.scene.handle, fake, fake, None, geom, stride, 2, 4, 1e-2, pa._ffi.STAGES_LUNAR, fake, 0,
        wts.ctypes.data_as(ctypes.c_void_p), fake, None, fake, None)
    assert call(fake, 0) != 0 and b"geom_stride" in lib.cotix_last_error()
    assert call(None, w.geom_stride) != 0
    # World.body_params(): the per-env view of the geometry rows / the shared constants
    bp = w.body_params()
    assert tuple(bp.shape) == (2, 4, 4) and bp.data_ptr() == w.geom[0, w.geom.shape[1] - 16:].data_ptr()
    assert torch.equal(bp[:, 0, 0], w.bodies[0].mass)
    shared = pa.World(pa.scenarios.robocup_bodies(), 3, "cpu", torch.zeros(3, 2, dtype=torch.int32))
    sp = shared.body_params()
    assert torch.equal(sp, torch.tensor([b.params() for b in shared.bodies], dtype=torch.float32))
    with pytest.raises(ValueError, match="bit for bit"):
        pa.differentiable_rollout(shared, torch.zeros(2, 3, 2), body_params=sp + 1.0)
    with pytest.raises(ValueError, match="body_params must be"):
        pa.differentiable_rollout(shared, torch.zeros(2, 3, 2), body_params=torch.zeros(3, 5, 4))
