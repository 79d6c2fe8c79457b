"""TEST INFRASTRUCTURE ONLY: ctypes front-end of the host emulation of the step
program with the key helper's level-1 key ring (tests/emu/cotix_emu_keyl1.cpp,
built by tests/emu/keyl1.mk).  The library also carries every entry point of
cotix_emu.cpp, so emu.py's functions work on it."""
import ctypes
import os
import subprocess

import numpy as np

import emu

HERE = os.path.dirname(os.path.abspath(__file__))
P_ = ctypes.c_void_p
_I = ctypes.c_int


def build(*targets):
    subprocess.run(["make", "-s", "-j2", "-C", HERE, "-f", "keyl1.mk", *["build/" + t for t in targets]], check=True)


def load():
    build("libcotix_emu_keyl1.so")
    lib = emu.load(path=os.path.join(HERE, "build", "libcotix_emu_keyl1.so"))
    lib.emu_step_keyl1.argtypes = [P_, P_, P_, P_, P_, _I, _I, _I, ctypes.c_float, _I, P_, _I, P_, P_, P_, P_]
    lib.emu_keyl1_tn2.argtypes = [P_, P_, _I]
    lib.emu_keyl1_fill.argtypes = [P_, P_, _I, _I, P_]
    lib.emu_keyl1_split_at.argtypes = [P_, P_, _I, _I, P_]
    return lib


def step_keyl1(lib, h, dyn, keys, err, geom, gstride, n_steps, stages, nb, dt=1e-2, action=None, action_body=0,
               dyn_reset=None, resets=None):
    """emu.step_ex at 4 envs per wave through the level-1 key form; raises
    where the barrier counts of the step wave, the helper and
    cxk::key_l1_barriers differ."""
    B = dyn.shape[2]
    ch = np.full((n_steps, nb, B), -7, np.int32)
    cl = np.full((n_steps, nb, nb, B), -7, np.int32)
    act = None if action is None else np.ascontiguousarray(action, np.float32)
    rc = lib.emu_step_keyl1(h, emu._p(dyn), emu._p(keys), emu._p(err), emu._p(geom), gstride, B, n_steps, dt, stages,
                            emu._p(act), action_body, emu._p(dyn_reset), emu._p(resets), emu._p(ch), emu._p(cl))
    if rc:
        raise RuntimeError(lib.emu_last_error().decode())
    return ch, cl


def tn2(lib, h):
    out = np.zeros(16, np.int32)
    nt = lib.emu_keyl1_tn2(h, emu._p(out), 16)
    return out[:nt].copy()


def fill(lib, h, tkeys, s0):
    """The ring producer alone: tkeys u32 [n, nt, 2, 4] -> u32 [n, nk1, 2, 4]."""
    tkeys = np.ascontiguousarray(tkeys, np.uint32)
    n, nk1 = tkeys.shape[0], int(tn2(lib, h).sum())
    out = np.zeros((n, nk1, 2, 4), np.uint32)
    rc = lib.emu_keyl1_fill(h, emu._p(tkeys), s0, n, emu._p(out))
    if rc < 0:
        raise RuntimeError(lib.emu_last_error().decode())
    return out


def split_at(lib, h, key, num, idx):
    key = np.ascontiguousarray(key, np.uint32)
    out = np.zeros(2, np.uint32)
    lib.emu_keyl1_split_at(h, emu._p(key), num, idx, emu._p(out))
    return out
