"""TEST INFRASTRUCTURE ONLY: ctypes front-end of the host emulation of the step
program with the key helper's speculative draw words
(tests/emu/cotix_emu_scanspec.cpp, built by tests/emu/scanspec.mk).  The
library also carries every entry point of cotix_emu.cpp and
cotix_emu_keyl1.cpp."""
import ctypes
import os
import subprocess

import numpy as np

import emu

HERE = os.path.dirname(os.path.abspath(__file__))
P_ = ctypes.c_void_p
_I = ctypes.c_int


def build(*targets):
    subprocess.run(["make", "-s", "-j2", "-C", HERE, "-f", "scanspec.mk", *["build/" + t for t in targets]], check=True)


def load(name="libcotix_emu_scanspec.so"):
    build(name)
    lib = emu.load(path=os.path.join(HERE, "build", name))
    lib.emu_step_scanspec.argtypes = [P_, P_, P_, P_, P_, _I, _I, _I, ctypes.c_float, _I, P_, _I, P_, P_, P_, P_]
    lib.emu_keyl1_tn2.argtypes = [P_, P_, _I]
    lib.emu_keyl1_fill.argtypes = [P_, P_, _I, _I, P_]
    lib.emu_keyl1_split_at.argtypes = [P_, P_, _I, _I, P_]
    lib.emu_scanspec_m.argtypes = [P_]
    lib.emu_scanspec_round0_done.argtypes = []
    lib.emu_scanspec_round0_done.restype = ctypes.c_ulonglong
    lib.emu_scanspec_lists.argtypes = [P_, P_, P_, P_, P_, _I]
    lib.emu_scanspec_fill.argtypes = [P_, P_, _I, _I, P_]
    return lib


def m_of(lib):
    """(this build's M, the kernel's SCAN_M)."""
    k = ctypes.c_int(0)
    return lib.emu_scanspec_m(ctypes.byref(k)), k.value


def step_scanspec(lib, h, dyn, keys, err, geom, gstride, n_steps, stages, nb, dt=1e-2, action=None, action_body=0,
                  dyn_reset=None, resets=None):
    """emu_keyl1.step_keyl1 through the form with the draw words."""
    B = dyn.shape[2]
    ch = np.full((n_steps, nb, B), -7, np.int32)
    cl = np.full((n_steps, nb, nb, B), -7, np.int32)
    act = None if action is None else np.ascontiguousarray(action, np.float32)
    rc = lib.emu_step_scanspec(h, emu._p(dyn), emu._p(keys), emu._p(err), emu._p(geom), gstride, B, n_steps, dt,
                               stages, emu._p(act), action_body, emu._p(dyn_reset), emu._p(resets), emu._p(ch),
                               emu._p(cl))
    if rc:
        raise RuntimeError(lib.emu_last_error().decode())
    return ch, cl


def round0_done(lib):
    """The items that the scan's round 0 settled or finished since the last call."""
    return int(lib.emu_scanspec_round0_done())


def lists(lib, h):
    """The scene's cells: (ci, cj, length) arrays and the candidates' trace
    codes in list order, i32 [nl, longest list] (-1 past a list's end)."""
    ci, cj, ln = (np.zeros(256, np.int32) for _ in range(3))
    nl = lib.emu_scanspec_lists(h, emu._p(ci), emu._p(cj), emu._p(ln), None, 0)
    stride = int(ln[:nl].max())
    cand = np.full((nl, stride), -1, np.int32)
    lib.emu_scanspec_lists(h, emu._p(ci), emu._p(cj), emu._p(ln), emu._p(cand), stride)
    return ci[:nl].copy(), cj[:nl].copy(), ln[:nl].copy(), cand


def settle_positions(cells, cl):
    """The list position of every written cell of a collider trace `cl`
    i32 [T, nb, nb, B] (flattened), from lists()'s `cells`."""
    ci, cj, ln, cand = cells
    out = []
    for l in range(len(ci)):
        w = cl[:, ci[l], cj[l], :]
        w = w[w >= 0]
        for code in np.unique(w):
            pos = np.nonzero(cand[l, :ln[l]] == code)[0]
            assert len(pos) >= 1, "a traced candidate that is not in its cell's list"
            out.append(np.full(int((w == code).sum()), pos[0]))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def fill(lib, h, l1keys, s0):
    """The draw-word producer alone: ring keys u32 [n, nk1, 2, 4] -> words u32 [n, nl, 4]."""
    l1keys = np.ascontiguousarray(l1keys, np.uint32)
    n, nl = l1keys.shape[0], len(lists(lib, h)[0])
    out = np.zeros((n, nl, 4), np.uint32)
    rc = lib.emu_scanspec_fill(h, emu._p(l1keys), s0, n, emu._p(out))
    if rc < 0:
        raise RuntimeError(lib.emu_last_error().decode())
    return out
