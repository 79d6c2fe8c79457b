"""TEST INFRASTRUCTURE ONLY: ctypes front-end of the host emulation's backward
with the shape geometry's gradient (tests/emu/cotix_emu_gradg.cpp, built by
tests/emu/gradg.mk).  The library also carries every entry point of
cotix_emu.cpp, so emu.py's functions work on it."""
import ctypes
import os
import subprocess

import numpy as np

import emu

HERE = os.path.dirname(os.path.abspath(__file__))
P_ = ctypes.c_void_p


def build(*targets):
    subprocess.run(["make", "-s", "-j3", "-C", HERE, "-f", "gradg.mk", *["build/" + t for t in targets]], check=True)


def load(nogregs=False):
    """The plain build, or phase G's tile form on every scene (COTIX_NO_GREGS)."""
    name = "libcotix_emu_gradg_nogregs.so" if nogregs else "libcotix_emu_gradg.so"
    build(name)
    lib = emu.load(path=os.path.join(HERE, "build", name))
    lib.emu_rollout_backward_geom.argtypes = [P_, P_, P_, P_, P_, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_float, ctypes.c_int, P_, ctypes.c_int, P_, P_, P_, P_, P_,
                                              ctypes.c_int]
    lib.emu_geom_part_words.argtypes = [P_]
    lib.emu_launch_plan_geom.argtypes = [P_] + [ctypes.c_int] * 10 + [P_]
    return lib


def rollout_backward_geom(lib, h, sd, sk, geom, gstride, stages, actions, action_body, w, dt=1e-2, E=4, tape=None,
                          want_params=False):
    """emu.rollout_backward plus gg f32 [GW, B] (and gp f32 [nb, 4, B] or
    None), poisoned first: the kernel writes every word of the batch."""
    T, B = actions.shape[0], actions.shape[1]
    nb = sd.shape[2] // 6
    ga = np.zeros((T, B, 2), np.float32)
    gd = np.zeros((nb, 6, B), np.float32)
    gp = np.full((nb, 4, B), -7.0, np.float32) if want_params else None
    gg = np.full((lib.emu_geom_part_words(h), B), -7.0, np.float32)
    actions = np.ascontiguousarray(actions, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    rc = lib.emu_rollout_backward_geom(h, emu._p(sd), emu._p(sk), emu._p(tape), emu._p(geom), gstride, B, T, dt,
                                       stages, emu._p(actions), action_body, emu._p(w), emu._p(ga), emu._p(gd),
                                       emu._p(gp), emu._p(gg), E)
    if rc:
        raise RuntimeError(lib.emu_last_error().decode())
    return ga, gd, gp, gg


PLAN_FIELDS = ("family", "ew", "wpb", "fnset", "mode", "spec", "gp", "sdefer", "nb", "grid", "block", "lds", "error",
               "listed")


def launch_plan(lib, h, mode, B, n_steps, stages, grad_params=False, grad_geom=False, envs_per_wave=4, specialize=1,
                cus=256, split_bwd_on=True):
    """The library's plan (cxl::plan_launch) of a backward launch as a dict."""
    out = (ctypes.c_long * 14)()
    n = lib.emu_launch_plan_geom(h, envs_per_wave, specialize, mode, B, n_steps, stages, int(grad_params),
                                 int(grad_geom), cus, int(split_bwd_on), ctypes.cast(out, P_))
    assert n == 14
    return dict(zip(PLAN_FIELDS, list(out)))
