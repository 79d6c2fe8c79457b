"""TEST INFRASTRUCTURE ONLY: ctypes front-end of the host emulation's backward
with the body parameters' gradient (tests/emu/cotix_emu_gradp.cpp, built by
tests/emu/gradp.mk).  The library also carries every entry point of
cotix_emu.cpp, so emu.py's functions work on it."""
import ctypes
import os
import subprocess

import numpy as np

import emu

HERE = os.path.dirname(os.path.abspath(__file__))
P_ = ctypes.c_void_p


def build(*targets):
    subprocess.run(["make", "-s", "-j3", "-C", HERE, "-f", "gradp.mk", *["build/" + t for t in targets]], check=True)


def load(nogregs=False):
    """The plain build, or phase G's tile form on every scene (COTIX_NO_GREGS)."""
    name = "libcotix_emu_gradp_nogregs.so" if nogregs else "libcotix_emu_gradp.so"
    build(name)
    lib = emu.load(path=os.path.join(HERE, "build", name))
    lib.emu_rollout_backward_params.argtypes = [P_, P_, P_, P_, P_, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_float, ctypes.c_int, P_, ctypes.c_int, P_, P_, P_, P_,
                                                ctypes.c_int]
    return lib


def rollout_backward_params(lib, h, sd, sk, geom, gstride, stages, actions, action_body, w, dt=1e-2, E=4, tape=None):
    """emu.rollout_backward plus gp f32 [nb, 4, B] (poisoned first: the kernel
    writes every word of the batch)."""
    T, B = actions.shape[0], actions.shape[1]
    nb = sd.shape[2] // 6
    ga = np.zeros((T, B, 2), np.float32)
    gd = np.zeros((nb, 6, B), np.float32)
    gp = np.full((nb, 4, B), -7.0, np.float32)
    actions = np.ascontiguousarray(actions, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    rc = lib.emu_rollout_backward_params(h, emu._p(sd), emu._p(sk), emu._p(tape), emu._p(geom), gstride, B, T, dt,
                                         stages, emu._p(actions), action_body, emu._p(w), emu._p(ga), emu._p(gd),
                                         emu._p(gp), E)
    if rc:
        raise RuntimeError(lib.emu_last_error().decode())
    return ga, gd, gp
