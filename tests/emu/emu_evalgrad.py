"""TEST INFRASTRUCTURE ONLY: ctypes front-end of the host emulation of the
differentiable eval (tests/emu/cotix_emu_evalgrad.cpp, built by
tests/emu/evalgrad.mk).  The library also carries every entry point of
cotix_emu.cpp, so emu.py's functions work on it."""
import ctypes
import os
import subprocess

import numpy as np

import emu

HERE = os.path.dirname(os.path.abspath(__file__))
P_ = ctypes.c_void_p
I_, F_ = ctypes.c_int, ctypes.c_float


def build(*targets):
    subprocess.run(["make", "-s", "-j3", "-C", HERE, "-f", "evalgrad.mk", *["build/" + t for t in targets]],
                   check=True)


def load(nogregs=False):
    """The plain build, or phase G's tile form on every scene (COTIX_NO_GREGS)."""
    name = "libcotix_emu_evalgrad_nogregs.so" if nogregs else "libcotix_emu_evalgrad.so"
    build(name)
    lib = emu.load(path=os.path.join(HERE, "build", name))
    lib.emu_eval_rollout.argtypes = [P_, P_, P_, P_, P_, I_, I_, I_, I_, F_, I_, P_, P_, P_, P_, P_, P_, P_, P_, I_]
    lib.emu_eval_backward.argtypes = [P_, P_, P_, P_, P_, P_, I_, I_, I_, I_, F_, I_, P_, P_, P_, P_, P_, I_]
    return lib


def _ref(s):
    return None if s is None else ctypes.cast(ctypes.pointer(s), P_)


def eval_rollout(lib, h, dyn, keys, err, geom, gstride, n_nfe, wfe, dt, stages, judge, control, reward, finished,
                 E=4, tape=True):
    """The saving eval forward: dyn / keys / err / reward / finished advanced in
    place; returns (saved_dyn, saved_keys, tape, judge_rec) in the library's
    layouts, poisoned first (the forward writes every word the backward reads)."""
    nb, B, T = dyn.shape[0], dyn.shape[2], n_nfe * wfe
    nblk = (B + 3) // 4
    sd = np.zeros((T, nblk, nb * 6, 4), np.float32)
    sk = np.zeros((T, B, 2), np.uint32)
    tp = np.full((T, nblk, lib.emu_rollout_tape_words(h), 4), 0x7FBADBAD, np.uint32) if tape else None
    rec = np.full((T + 1, B), 0xFFFFFFFF, np.uint32)
    rc = lib.emu_eval_rollout(h, emu._p(dyn), emu._p(keys), emu._p(err), emu._p(geom), gstride, B, n_nfe, wfe, dt,
                              stages, _ref(judge), _ref(control), emu._p(reward), emu._p(finished), emu._p(sd),
                              emu._p(sk), emu._p(tp), emu._p(rec), E)
    if rc:
        raise RuntimeError(lib.emu_last_error().decode())
    return sd, sk, tp, rec


def eval_backward(lib, h, sd, sk, tp, rec, geom, gstride, n_nfe, wfe, dt, stages, judge, control, E=4,
                  want=(True, True, True)):
    """(grad_control [26, B], grad_dyn0 [nb, 6, B], grad_dv [T, B, 2]), each
    poisoned first (the kernel writes every word of the batch) or None."""
    T, B, nb = sd.shape[0], sk.shape[1], sd.shape[2] // 6
    gc = np.full((26, B), -7.0, np.float32) if want[0] else None
    gd = np.full((nb, 6, B), -7.0, np.float32) if want[1] else None
    gv = np.full((T, B, 2), -7.0, np.float32) if want[2] else None
    rc = lib.emu_eval_backward(h, emu._p(sd), emu._p(sk), emu._p(tp), emu._p(rec), emu._p(geom), gstride, B, n_nfe,
                               wfe, dt, stages, _ref(judge), _ref(control), emu._p(gc), emu._p(gd), emu._p(gv), E)
    if rc:
        raise RuntimeError(lib.emu_last_error().decode())
    return gc, gd, gv
