"""Gradients of the rollout's return with respect to the shape geometry of
every part (Circle.radius / position, AABB.lower / upper, polygon vertices;
cotix_rollout_backward_ex3's grad_geom) on CPU: the kernel's backward wave
programs with the geometry adjoint (host emulation,
tests/emu/cotix_emu_gradg.cpp -- the GPU's bits by construction) against the
torch-f32 VJP oracle with the geometry row as a leaf
(tests/grad_geom_cases.py), itself checked against central differences of the
faithful oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grad_cases as GC
import grad_geom_cases as GGC
import penv_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
WHAT = ("ret", "grad_action", "grad_dyn0", "grad_geom")


@pytest.fixture(scope="module")
def libs():
    import emu
    import emu_gradg
    emu_gradg.build("libcotix_emu_gradg.so", "libcotix_emu_gradg_nogregs.so", "gradg_asan_driver")
    return emu, emu_gradg, emu_gradg.load()


def emu_scene(emu, lib, case, per_env):
    """(scene handle, geometry, geometry stride) of a case on the emulation."""
    if per_env:
        h, _ = emu.oracle_scene(lib, case["obs"][0], per_env_params=True)
        geom = PC.rows(lambda ob: emu.oracle_scene(lib, ob)[1], case["obs"])
        return h, geom, geom.shape[1]
    h, geom = emu.oracle_scene(lib, case["make"]())
    return h, geom, 0


def emu_run(emu, emu_gradg, lib, case, stages, per_env=False, E=4, replay=False, want_params=False):
    """Forward, then the backward with grad_geom: (ret, ga, gd, gg, gp) and the
    arguments to run another backward on the same forward."""
    h, geom, gs = emu_scene(emu, lib, case, per_env)
    dyn = np.ascontiguousarray(case["S0"].transpose(1, 2, 0))
    keys = np.array(case["keys"], np.uint32, copy=True)
    err = np.zeros(dyn.shape[2], np.uint32)
    ret, sd, sk, tape = emu.rollout(lib, h, dyn, keys, err, geom, gs, stages, case["actions"], case["ab"], case["w"],
                                    E=E)
    args = (h, sd, sk, geom, gs, stages, case["actions"], case["ab"], case["w"])
    ga, gd, gp, gg = emu_gradg.rollout_backward_geom(lib, *args, E=E, tape=None if replay else tape,
                                                     want_params=want_params)
    return ret, ga, gd, gg, gp, args, tape


_RUNS = {}


def default_run(libs, name, E):
    """The tape backward of a case at E envs per wave, run once per process."""
    if (name, E) not in _RUNS:
        emu, emu_gradg, lib = libs
        case, stages, per_env, _ = GGC.cases()[name]
        _RUNS[(name, E)] = emu_run(emu, emu_gradg, lib, case, stages, per_env, E)
    return _RUNS[(name, E)]


# ---------------------------------------------------------------------------
# 1. the checker of the checker
# ---------------------------------------------------------------------------
FD_ENTRIES = {"box5x16": (1, (16, 17, 18, 24, 25, 26)), "ball_poly4x8": (0, (16, 17))}


@pytest.mark.parametrize("name", sorted(FD_ENTRIES))
def test_geom_oracle_vs_finite_differences(name):
    """The geometry-leaf VJP chain against central differences of the faithful
    oracle's return, h = 1e-3 max(1, |p|), at 2e-3 (1 + |fd|) -- the bar of
    test_oracle_grad_vs_finite_differences.  Measured: the largest relative
    gap 1.2e-4 on the box world's entries, 6.3e-4 on word 17 of ball_poly.
    (Longer horizons cross collider decisions: no valid difference quotient.)
    The action / state gradients stay bit-identical to the constant-geometry
    oracle's."""
    case = GGC.cases()[name][0]
    e, words = FD_ENTRIES[name]
    ret, ga, gS, gg = GGC.oracle_of(name, case)[e]
    r0, ga0, gS0 = GC.oracle(case, [e])[e]
    assert np.float32(ret).view(np.uint32) == np.float32(r0).view(np.uint32)
    assert GGC.same_bits(ga, ga0) and GGC.same_bits(gS, gS0)
    for k, fd in zip(words, GGC.fd_geom(case, e, words)):
        g = float(gg[k])
        print("%s env %d word %d: vjp %.6g fd %.6g rel %.3g" % (name, e, k, g, fd, abs(fd - g) / max(abs(fd), 1e-30)))
        assert np.isfinite(g) and g != 0, (k, g)
        assert abs(fd - g) <= 2e-3 * (1 + abs(fd)), (k, fd, g)


# ---------------------------------------------------------------------------
# 2. emulation vs oracle; 3. the request changes nothing else
# ---------------------------------------------------------------------------
CASES = [(n, E) for n, (_, _, _, Es) in GGC.cases().items() for E in Es]


@pytest.mark.parametrize("name,E", CASES)
def test_emu_grad_geom_vs_oracle(libs, name, E):
    emu, emu_gradg, lib = libs
    case = GGC.cases()[name][0]
    orc = GGC.oracle_of(name, case)
    GGC.check_conditions(name, orc)
    ret, ga, gd, gg, _, args, tape = default_run(libs, name, E)
    assert gg.shape == (orc[0][3].size, case["S0"].shape[0])
    pads = GGC.pad_words(case)
    for e in orc:
        r, oga, ogS, ogg = orc[e]
        same = (np.isnan(ret[e]) and np.isnan(r)) or np.float32(ret[e]).view(np.uint32) == np.float32(r).view(
            np.uint32)
        assert same, (e, ret[e], r)
        ok, msg = GC.close(gg[:, e], ogg, GGC.tol_of(name, case), name + "_geom")
        assert ok, "env %d grad_geom: %s\n%s" % (e, msg, np.stack([gg[:, e], ogg], 1))
        ok, msg = GC.close(ga[:, e], oga, case["tol"])
        assert ok, "env %d grad_action: %s" % (e, msg)
        if np.all(ogg == 0):  # nothing resolved: exact zeros from the kernel
            assert not gg[:, e].view(np.uint32).any(), (e, gg[:, e])
        assert not gg[pads, e].view(np.uint32).any(), "a circle's pad word is not an exact zero"
    # the call with grad_geom changes nothing else.  The GJK / EPA scenes whose
    # pose responses come from phase GE (lunar*, poly_box) keep them: the
    # geometry's contact VJP is a second one, so these are bit-identical too
    pa_, pd_ = emu.rollout_backward(lib, *args, E=E, tape=tape)
    assert GGC.same_bits(ga, pa_), "grad_action changes with grad_geom"
    assert GGC.same_bits(gd, pd_), "grad_dyn0 changes with grad_geom"


# ---------------------------------------------------------------------------
# 4. form equalities (bit for bit, NaN patterns included)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,E", CASES)
def test_tape_equals_replay(libs, name, E):
    emu, emu_gradg, lib = libs
    _, ga, gd, gg, _, args, _ = default_run(libs, name, E)
    ra, rd, _, rg = emu_gradg.rollout_backward_geom(lib, *args, E=E)
    assert GGC.same_bits(ga, ra) and GGC.same_bits(gd, rd)
    assert GGC.same_bits(gg, rg), "grad_geom: tape != re-play"
    # ... and the re-play's grad_action / grad_dyn0 without the request
    pa_, pd_ = emu.rollout_backward(lib, *args, E=E)
    assert GGC.same_bits(ra, pa_) and GGC.same_bits(rd, pd_)


def test_register_chain_equals_tile_form(libs):
    """g_chain in registers (5 and 7 bodies) against ph_G's tile form on the
    same scenes (the -DCOTIX_NO_GREGS build)."""
    emu, emu_gradg, lib = libs
    tile = emu_gradg.load(nogregs=True)
    for name in ("box5x16", "robocup8x6"):
        case, stages, _, _ = GGC.cases()[name]
        a = default_run(libs, name, 4)
        b = emu_run(emu, emu_gradg, tile, case, stages)
        for x, y, what in zip(a[:4], b[:4], WHAT):
            assert GGC.same_bits(x, y), (name, what)


@pytest.mark.parametrize("name", list(GGC.cases()))
def test_tilings_agree(libs, name):
    """One env per wave == two == four == eight (every envs_per_wave tiling
    runs the same chain per env)."""
    emu, emu_gradg, lib = libs
    case, stages, per_env, _ = GGC.cases()[name]
    ref = default_run(libs, name, 4)
    for E in (1, 2, 8):
        got = default_run(libs, name, E) if (name, E) in CASES else emu_run(emu, emu_gradg, lib, case, stages,
                                                                             per_env, E)
        for x, y, what in zip(ref[:4], got[:4], WHAT):
            assert GGC.same_bits(x, y), (E, what)


@pytest.mark.parametrize("name", ["box5x16", "robocup8x6", "lunar4x8", "lunar_penv4x8"])
def test_with_and_without_params(libs, name):
    """want_geom with and without want_params give the same grad_geom, and
    the level-2 programs' grad_params are the level-1 programs' bits."""
    import emu_gradp
    emu, emu_gradg, lib = libs
    case, stages, per_env, _ = GGC.cases()[name]
    a = default_run(libs, name, 4)
    for replay in (False, True):
        b = emu_run(emu, emu_gradg, lib, case, stages, per_env, 4, replay=replay, want_params=True)
        for x, y, what in zip(a[:4], b[:4], WHAT):
            assert GGC.same_bits(x, y), (replay, what)
        assert not np.any(b[4] == -7.0)
    libp = emu_gradp.load()
    from test_grad_params_cpu import emu_run as emu_run_p
    gp1 = emu_run_p(emu, emu_gradp, libp, case, stages, per_env, 4)[3]
    assert GGC.same_bits(b[4], gp1), "grad_params differ between the level-1 and level-2 programs"


# ---------------------------------------------------------------------------
# 5. the sanitizers, on a stand-alone program
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("scene,E", [("box", 1), ("box", 4), ("lunar", 1), ("lunar", 4)])
def test_asan_driver(libs, tmp_path, scene, E):
    """tests/emu/gradg_asan_driver (-fsanitize=address,undefined
    -fno-sanitize-recover=all, its own main, no preloaded runtime): the
    backward with grad_geom into exactly sized buffers exits cleanly, tape ==
    re-play and with == without grad_params inside it, and its output equals
    the plain emulation's bits."""
    emu, emu_gradg, lib = libs
    from test_emu_asan import _scene_arrays
    case, stages = (GC.box_case(5, 8, seed=1), GGC.BOX_STAGES) if scene == "box" else (GC.lunar_case(2, 4, seed=0),
                                                                                     GGC.LUNAR_STAGES)
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
    r = subprocess.run([os.path.join(HERE, "emu", "build", "gradg_asan_driver"), inp, out], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    ret, ga, gd, gg = emu_run(emu, emu_gradg, lib, case, stages, False, E)[:4]
    assert np.any(np.nan_to_num(gg) != 0)
    want = np.concatenate([x.reshape(-1).view(np.uint8) for x in (ret, ga, gd, gg)])
    assert np.array_equal(np.fromfile(out, np.uint8), want)


# ---------------------------------------------------------------------------
# 6. the C ABI's argument checks (nothing is launched) and the plan
# ---------------------------------------------------------------------------
def test_ex3_argument_checks_and_old_entry_points():
    import ctypes
    import torch
    import parallax_amd as pa
    import ref_standins as RS
    lib = pa._ffi.lib
    for name in ("cotix_rollout_backward", "cotix_rollout_backward_ex", "cotix_rollout_backward_ex2",
                 "cotix_rollout_backward_ex3", "cotix_scene_geom_part_words", "cotix_scene_part_geom"):
        assert hasattr(lib, name) and name in pa._ffi.SIGNATURES
    w = pa.World.from_bodies(RS.stack([RS.from_oracle(ob) for ob in PC.lunar_penv_bodies(2)]), device="cpu")
    assert w.scene.per_env_params
    fake = ctypes.c_void_p(4096)  # never dereferenced: the checks fail first
    wts = np.zeros(24, np.float32)
    call = lambda geom, stride, B=2: lib.cotix_rollout_backward_ex3(  # noqa: E731
        w.scene.handle, fake, fake, None, geom, stride, B, 4, 1e-2, pa._ffi.STAGES_LUNAR, fake, 0,
        wts.ctypes.data_as(ctypes.c_void_p), fake, None, None, fake, None)
    assert call(fake, 0) != 0 and b"grad_geom of a per-env scene" in lib.cotix_last_error()
    assert call(None, w.geom_stride) != 0
    assert call(fake, w.geom_stride - 1) != 0 and b"geom_stride smaller" in lib.cotix_last_error()
    assert call(fake, w.geom_stride, B=0) == 0  # (an empty batch: nothing to launch)
    # grad_geom == NULL is ex2: the same checks in the same order
    ex2 = lib.cotix_rollout_backward_ex2(w.scene.handle, fake, fake, None, fake, 0, 2, 4, 1e-2,
                                         pa._ffi.STAGES_LUNAR, fake, 0, wts.ctypes.data_as(ctypes.c_void_p), fake,
                                         None, fake, None)
    msg2 = lib.cotix_last_error()
    ex3 = lib.cotix_rollout_backward_ex3(w.scene.handle, fake, fake, None, fake, 0, 2, 4, 1e-2,
                                         pa._ffi.STAGES_LUNAR, fake, 0, wts.ctypes.data_as(ctypes.c_void_p), fake,
                                         None, fake, None, None)
    assert ex2 != 0 and ex3 == ex2 and lib.cotix_last_error() == msg2 and b"grad_params" in msg2
    # World.geometry(): the parts' words of every row, without the parameter words
    GW = w.scene.geom_part_words
    assert GW == 84 and w.scene.geom_floats == GW + 16
    geo = w.geometry()
    assert tuple(geo.shape) == (2, GW) and geo.data_ptr() == w.geom.data_ptr()
    assert w.body_params().data_ptr() == w.geom[0, GW:].data_ptr()
    off = 0
    for bi, b in enumerate(w.bodies):
        for pi, p in enumerate(b.shape.parts):
            v = w.part_geometry(bi, pi)
            assert tuple(v.shape) == (2, p.geom_floats()) and v.data_ptr() == w.geom[0, off:].data_ptr()
            off += p.geom_floats()
    assert off == GW
    with pytest.raises(IndexError):
        w.part_geometry(0, 7)
    shared = pa.World(pa.scenarios.robocup_bodies(), 3, "cpu", torch.zeros(3, 2, dtype=torch.int32))
    sg = shared.geometry()
    assert tuple(sg.shape) == (shared.scene.geom_floats,) and sg.data_ptr() == shared.geom.data_ptr()
    assert tuple(shared.part_geometry(4).shape) == (4,)
    with pytest.raises(ValueError, match="geometry must be"):
        pa.differentiable_rollout(shared, torch.zeros(2, 3, 2), geometry=torch.zeros(3, sg.shape[0]))
    with pytest.raises(ValueError, match="float32"):
        pa.differentiable_rollout(shared, torch.zeros(2, 3, 2), geometry=sg.double())


def test_plan_picks_level_two_and_never_the_split_form(libs):
    """cxl::plan_launch through the emulation: a launch with grad_geom runs
    step_kernel at level 2 (generic, every tiling, listed), never the
    producer / consumer form; without it the level is 0 / 1 as before."""
    emu, emu_gradg, lib = libs
    rc_case, box_case, lunar_case = (GGC.cases()[n][0] for n in ("robocup8x6", "box5x16", "lunar4x8"))
    FAM_STEP, FAM_SPLIT, SPEC_GENERIC = 0, 3, 0
    for case, stages in ((rc_case, GGC.BOX_STAGES), (box_case, GGC.BOX_STAGES), (lunar_case, GGC.LUNAR_STAGES)):
        h, _ = emu.oracle_scene(lib, case["make"]())
        for mode in (2, 4):
            for ew in (1, 2, 4, 8):
                for par in (False, True):
                    p = emu_gradg.launch_plan(lib, h, mode, 4096, 64, stages, grad_params=par, grad_geom=True,
                                              envs_per_wave=ew)
                    assert (p["family"], p["gp"], p["spec"], p["listed"], p["error"]) == (FAM_STEP, 2, SPEC_GENERIC,
                                                                                          1, 0), (mode, ew, par, p)
                    assert p["block"] == 64 * p["wpb"]
                p = emu_gradg.launch_plan(lib, h, mode, 4096, 64, stages, grad_params=True, envs_per_wave=ew)
                assert (p["family"], p["gp"], p["listed"]) == (FAM_STEP, 1, 1), p
                p = emu_gradg.launch_plan(lib, h, mode, 4096, 64, stages, envs_per_wave=ew)
                assert p["gp"] == 0 and p["listed"] == 1, p
    # RoboCup's tape backward without a request is still the split form
    h, _ = emu.oracle_scene(lib, rc_case["make"]())
    assert emu_gradg.launch_plan(lib, h, 4, 4096, 64, GGC.BOX_STAGES)["family"] == FAM_SPLIT
    assert emu_gradg.launch_plan(lib, h, 4, 4096, 64, GGC.BOX_STAGES, grad_geom=True)["family"] == FAM_STEP
