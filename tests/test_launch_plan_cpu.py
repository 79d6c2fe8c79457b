"""The launch plan (parallax_amd/csrc/cotix_plan.h): which kernel of the list a
launch runs, through the host emulation's emu_launch_plan.  The expected rows
are literals written from the launcher the plan replaced (its launch(), the
two form launchers and the per-tiling ladder), and every plan over the cross
product of scenes, variants and launch arguments names a kernel of the list --
the differentiable eval's programs (modes 5 / 6) and the backward with the
shape geometry's gradient (gp 2) included, through emu_launch_plan_ex.  Which
row of tests/kernel_matrix.py runs each kernel of the list is
tests/test_kernel_matrix_cpu.py's."""
import ctypes
import itertools
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

STEP, HELP, HELP_L1, SPLIT = 0, 1, 2, 3  # cxl::FAM_*
GENERIC, ROBOCUP, LUNAR, ROBOCUP_PART, LUNAR_PART, BOX = range(6)  # cxk::SPEC_*
AN, PP, AP, ALL = 1, 3, 11, 15  # the contact-function programs
ADVANCE, COLLIDER = 1 | 16, 4  # stages: the RoboCup step's without / the collider
FIELDS = ("family", "ew", "wpb", "fnset", "mode", "spec", "gp", "sdefer", "nb", "grid", "block", "lds", "error",
          "listed")


@pytest.fixture(scope="module")
def planner():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "emu"), "build/libcotix_emu.so"], check=True)
    import emu
    import grad_cases as GC
    import make_golden as mg
    import scene_cases
    from cotix_oracle import physics as P
    from cotix_oracle.params import Params
    lib = emu.load()
    lib.emu_launch_plan.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 10 + [ctypes.POINTER(ctypes.c_long)]
    lib.emu_launch_plan_ex.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 11 + [ctypes.POINTER(ctypes.c_long)]
    lib.emu_lds_bytes_w.restype = ctypes.c_long
    lib.emu_lds_bytes_w.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    part = Params(prng_layout="partitionable")
    made = {
        "robocup": (P.robocup_bodies(), None), "robocup_part": (P.robocup_bodies(), part),
        "robocup_cp": (P.robocup_bodies(), Params(contact_p=0.25)),
        "lunar": (P.lunar_lander_bodies(), None), "lunar_part": (P.lunar_lander_bodies(), part),
        "box": (mg.box_world_bodies(0), None),
        "convex": (scene_cases.straddle_scene(0.3), None), "aabb_poly": (scene_cases.mixed_scene(False), None),
        "circle_poly": (scene_cases.mixed_scene(True), None),
        "octagon12": (scene_cases.octagon_row(12), None), "octagon15": (scene_cases.octagon_row(15), None),
        "quad_row": (GC.quad_row_case(1, 1)["make"](), None),
    }
    scenes = {k: emu.oracle_scene(lib, b, p)[0] for k, (b, p) in made.items()}
    out = (ctypes.c_long * len(FIELDS))()

    def plan(scene, ew=4, specialize=1, mode=0, B=4096, n_steps=16, collider=True, grad_params=False, cus=256,
             key_helper=True, split_bwd=True):
        n = lib.emu_launch_plan(scenes[scene], ew, specialize, mode, B, n_steps, ADVANCE | (COLLIDER if collider else 0),
                                int(grad_params), cus, int(key_helper), int(split_bwd), out)
        assert n == len(FIELDS)
        return dict(zip(FIELDS, out))

    def plan_ex(scene, ew, specialize, mode, B, n_steps, collider, gp, cus, key_helper, split_bwd):
        """Every program (modes 0 .. 6) at gradient level gp 0, 1 or 2."""
        n = lib.emu_launch_plan_ex(scenes[scene], ew, specialize, mode, B, n_steps,
                                   ADVANCE | (COLLIDER if collider else 0), int(gp >= 1), int(gp == 2), cus,
                                   int(key_helper), int(split_bwd), out)
        assert n == len(FIELDS)
        return dict(zip(FIELDS, out))

    plan.ex = plan_ex
    plan.lds = lambda scene, ew, wpb: lib.emu_lds_bytes_w(scenes[scene], ew, wpb)
    plan.scenes = tuple(scenes)
    return plan


def key(p):
    return p["family"], p["fnset"], p["mode"], p["spec"], p["gp"]


def test_robocup_step_forms(planner):
    """The step launches of RoboCup at the default tiling: step_kernel up to
    one key window, then the helper forms; the level-1 ring only where its LDS
    costs no residency (one workgroup per CU is all the launch needs: 4096 envs
    are 256 workgroups on 256 CUs) and the collider's scan reads it."""
    p = planner("robocup", n_steps=16)
    assert key(p) == (STEP, AN, 0, ROBOCUP, 0) and (p["wpb"], p["grid"], p["block"]) == (4, 256, 256)
    assert p["lds"] == planner.lds("robocup", 4, 4)
    p = planner("robocup", n_steps=17)
    assert (p["family"], p["fnset"], p["spec"], p["sdefer"]) == (HELP_L1, AN, ROBOCUP, 1)
    assert (p["grid"], p["block"]) == (256, 512)
    l1_lds = p["lds"]
    for B in (4097, 8192):  # two workgroups on some CU: the ring's LDS would halve the residency
        p = planner("robocup", n_steps=17, B=B)
        assert (p["family"], p["spec"], p["sdefer"], p["block"]) == (HELP, ROBOCUP, 1, 512)
        assert p["grid"] == (B + 15) // 16 and p["lds"] < l1_lds
        # the residency rule's inputs: two of these workgroups fit a CU's LDS, one with the ring
        assert 160 * 1024 // p["lds"] >= 2 and 160 * 1024 // l1_lds == 1
    # an unknown CU count plans for two workgroups per CU
    assert planner("robocup", n_steps=17, cus=0)["family"] == HELP
    assert planner("robocup", n_steps=17, collider=False)["family"] == HELP
    p = planner("robocup", n_steps=17, key_helper=False)
    assert key(p) == (STEP, AN, 0, ROBOCUP, 0) and p["block"] == 256
    # the helper forms are RoboCup's specialization at the default tiling only
    for scene, spec in (("robocup_part", ROBOCUP_PART), ("box", BOX), ("robocup_cp", GENERIC)):
        assert key(planner(scene, n_steps=64)) == (STEP, AN, 0, spec, 0)
    assert key(planner("robocup", n_steps=64, specialize=0)) == (STEP, AN, 0, GENERIC, 0)
    assert key(planner("robocup", n_steps=64, ew=2)) == (STEP, AN, 0, ROBOCUP, 0)


def test_specializations_per_tiling(planner):
    assert key(planner("robocup", ew=2, mode=0)) == (STEP, AN, 0, ROBOCUP, 0)
    assert key(planner("robocup_part", ew=2, mode=0)) == (STEP, AN, 0, ROBOCUP_PART, 0)
    for mode in (1, 2, 3, 4):
        assert key(planner("robocup", ew=2, mode=mode)) == (STEP, AN, mode, GENERIC, 0)
        assert key(planner("robocup_part", ew=4, mode=mode, split_bwd=False)) == (STEP, AN, mode, GENERIC, 0)
    for ew, mode in itertools.product((1, 8), range(5)):
        assert key(planner("robocup", ew=ew, mode=mode)) == (STEP, AN, mode, GENERIC, 0)
    for mode in (0, 1, 3, 4):
        assert key(planner("robocup", mode=mode, split_bwd=False)) == (STEP, AN, mode, ROBOCUP, 0)
        assert key(planner("robocup", mode=mode, specialize=0)) == (STEP, AN, mode, GENERIC, 0)
    for mode in range(5):
        assert key(planner("box", ew=2, mode=mode)) == (STEP, AN, mode, GENERIC, 0)
        want = BOX if mode in (0, 1, 4) else GENERIC
        assert key(planner("box", ew=4, mode=mode)) == (STEP, AN, mode, want, 0)
    for scene, spec in (("lunar", LUNAR), ("lunar_part", LUNAR_PART)):
        for ew in (2, 4):
            assert key(planner(scene, ew=ew, mode=0)) == (STEP, PP, 0, spec, 0)
            assert key(planner(scene, ew=ew, mode=1)) == (STEP, ALL, 1, GENERIC, 0)
        assert key(planner(scene, ew=1, mode=0)) == (STEP, PP, 0, GENERIC, 0)
        assert key(planner(scene, ew=4, mode=0, specialize=0)) == (STEP, PP, 0, GENERIC, 0)
    # mode 2 (the re-play backward, the tape backward's check) is always generic
    for scene, ew, gp in itertools.product(planner.scenes, (1, 2, 4, 8), (False, True)):
        p = planner(scene, ew=ew, mode=2, grad_params=gp)
        assert p["error"] or (p["family"], p["mode"], p["spec"], p["gp"]) == (STEP, 2, GENERIC, int(gp))


def test_generic_programs(planner):
    for scene, fn in (("robocup_cp", AN), ("convex", PP), ("aabb_poly", AP), ("circle_poly", ALL)):
        for ew in (1, 2, 4, 8):
            p = planner(scene, ew=ew, mode=0, n_steps=64)
            assert p["error"] or key(p) == (STEP, fn, 0, GENERIC, 0)
            for mode in (1, 2, 3, 4):
                p = planner(scene, ew=ew, mode=mode)
                assert p["error"] or key(p) == (STEP, AN if fn == AN else ALL, mode, GENERIC, 0)


def test_tape_backward_forms(planner):
    """Mode 4: the split form for RoboCup's specialization (two waves per env
    group: the same grid, 512 threads, eight tiles), the one-wave kernel for
    the box world, for any launch with grad_params, and at every other tiling."""
    p = planner("robocup", mode=4)
    assert (p["family"], p["nb"], p["spec"], p["grid"], p["block"]) == (SPLIT, 5, ROBOCUP, 256, 512)
    assert p["lds"] == planner.lds("robocup", 4, 8)
    assert key(planner("robocup", mode=4, split_bwd=False)) == (STEP, AN, 4, ROBOCUP, 0)
    assert key(planner("robocup", mode=4, collider=False)) == (STEP, AN, 4, ROBOCUP, 0)  # (no row restore)
    assert key(planner("robocup", mode=4, B=13)) == (STEP, AN, 4, ROBOCUP, 0)  # (B not whole groups)
    assert key(planner("robocup", mode=4, specialize=0)) == (STEP, AN, 4, GENERIC, 0)
    assert key(planner("box", mode=4)) == (STEP, AN, 4, BOX, 0)
    for scene in planner.scenes:
        for ew, specialize in itertools.product((1, 2, 4, 8), (0, 1)):
            p = planner(scene, ew=ew, specialize=specialize, mode=4, grad_params=True)
            if p["error"]:
                continue
            spec = {"robocup": ROBOCUP, "box": BOX}.get(scene, GENERIC) if ew == 4 and specialize else GENERIC
            assert (p["family"], p["mode"], p["spec"], p["gp"]) == (STEP, 4, spec, 1), (scene, ew)


def test_scenes_of_fewer_waves_per_group(planner):
    for scene in ("octagon12", "octagon15"):
        for mode in range(5):
            p = planner(scene, ew=1, mode=mode, n_steps=64)
            assert p["wpb"] in (1, 2) and p["family"] == STEP and p["spec"] == GENERIC
            assert (p["grid"], p["block"]) == ((4096 + p["wpb"] - 1) // p["wpb"], 64 * p["wpb"])
            assert p["lds"] == planner.lds(scene, 1, p["wpb"])
    assert planner("octagon15", ew=8)["error"] == 1  # (rejected by cotix_scene_set_variant before any launch)


def test_every_plan_is_in_the_kernel_list(planner):
    """Closure: whatever the plan chooses is compiled for its tiling."""
    n = 0
    for scene in planner.scenes:
        for ew, specialize, mode, gp in itertools.product((1, 2, 4, 8), (0, 1), range(5), (False, True)):
            if gp and mode not in (2, 4):
                continue
            for n_steps, B, cus, kh, sb, coll in itertools.product((1, 16, 17, 64), (1, 13, 4096, 4097, 8192),
                                                                   (0, 256), (0, 1), (0, 1), (0, 1)):
                p = planner(scene, ew, specialize, mode, B, n_steps, bool(coll), gp, cus, kh, sb)
                assert p["listed"] == 1 or p["error"] == 1, (scene, ew, specialize, mode, gp, n_steps, B, cus, kh, sb)
                n += not p["error"]
    assert n > 100000
    # ... the differentiable eval's programs (5, 6) and the gradient levels 0,
    # 1 (the body parameters) and 2 (the shape geometry) of the backwards
    # included, and the plan says what was asked for
    m = 0
    for scene in planner.scenes:
        for ew, specialize, mode, gp in itertools.product((1, 2, 4, 8), (0, 1), range(7), (0, 1, 2)):
            if gp and mode not in (2, 4):
                continue
            for n_steps, B, cus, kh, sb, coll in itertools.product((1, 17), (13, 4096, 4097), (0, 256), (0, 1), (0, 1),
                                                                   (0, 1)):
                p = planner.ex(scene, ew, specialize, mode, B, n_steps, bool(coll), gp, cus, kh, sb)
                what = (scene, ew, specialize, mode, gp, n_steps, B, cus, kh, sb)
                assert p["listed"] == 1 or p["error"] == 1, what
                if not p["error"]:
                    assert (p["ew"], p["gp"]) == (ew, gp) and (p["family"] != STEP or p["mode"] == mode), what
                    if mode <= 4 and gp <= 1:  # the older query plans the same launch
                        q = planner(scene, ew, specialize, mode, B, n_steps, bool(coll), bool(gp), cus, kh, sb)
                        assert all(p[f] == q[f] for f in FIELDS), what
                m += not p["error"]
    assert m > 30000
