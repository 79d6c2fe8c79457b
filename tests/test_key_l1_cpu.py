"""The key helper's level-1 key ring on CPU (cotix_kernel.h KeyL1: the helper
wave computes every first-level key split(skey_t, N2)[i2] of the collider
scan into an LDS ring, the scan's draw reads it): the kernel's own step and
helper code on the host emulation (tests/emu/cotix_emu_keyl1.cpp), the
helper's work run at each barrier of the step wave, and the number of barriers
compared with cxk::key_l1_barriers, to which the GPU's helper and idle waves
loop -- a miscounted barrier is a hang on the GPU.  The emulation runs the
helper's work at the latest point the schedule allows, so it shows wrong or
missing keys, not a buffer overwritten too early (cotix_emu_keyl1.cpp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

B = 12
STAGES = 1 | 4 | 16


@pytest.fixture(scope="module")
def libs():
    import emu
    import emu_keyl1
    emu_keyl1.build("libcotix_emu_keyl1.so", "keyl1_asan_driver")
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "..", "oracle")], check=True)  # the C port: never a skip
    return emu, emu_keyl1, emu_keyl1.load()


def same_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def start(T):
    from cotix_oracle import cport
    dyn, keys = cport.robocup_batch(B)
    dyn, keys = np.ascontiguousarray(dyn, np.float32), np.ascontiguousarray(keys, np.uint32)
    act = np.ascontiguousarray((np.random.default_rng(T).normal(size=(T, B, 2)) * 0.1).astype(np.float32))
    return dyn, keys, act


def fresh(dyn, keys):
    return [dyn.copy(), keys.copy(), np.zeros(B, np.uint32), np.zeros(B, np.uint32)]


# one half and a step; two halves and a window's first step; whole windows; a
# window and a one-step half; a partial third window of one half; four windows;
# five (the ring and both window buffers reused twice over)
@pytest.mark.parametrize("T", [17, 20, 32, 33, 40, 64, 80])
def test_key_l1_vs_cport_and_plain(libs, T):
    """RoboCup, B = 12 (three env groups), autoreset, actions and the collider
    trace through the level-1 key form == the C port == the emulation without a
    helper, bit for bit: state, keys, error bits, restart counters and both
    trace arrays.  The barriers passed are compared with cxk::key_l1_barriers
    inside, and the helper's last half with the launch's (emu_step_keyl1 fails
    otherwise)."""
    emu, emu_keyl1, lib = libs
    from cotix_oracle import cport
    from cotix_oracle import physics as P
    dyn, keys, act = start(T)
    reset = dyn.copy()
    h, geom = emu.oracle_scene(lib, P.robocup_bodies())
    got = fresh(dyn, keys)
    gch, gcl = emu_keyl1.step_keyl1(lib, h, got[0], got[1], got[2], geom, 0, T, STAGES, 5, action=act, action_body=4,
                                    dyn_reset=reset, resets=got[3])
    plain = fresh(dyn, keys)
    pch, pcl = emu.step_ex(lib, h, plain[0], plain[1], plain[2], geom, 0, T, STAGES, 5, E=4, action=act,
                           action_body=4, dyn_reset=reset, resets=plain[3])
    want = fresh(dyn, keys)
    sc = cport.Scene(cport.load(), P.robocup_bodies())
    wch, wcl = sc.step_ex(want[0], want[1], want[2], T, cport.STAGES_ROBOCUP, None, act, 4, reset, want[3],
                          trace=True)
    if T >= 33:
        assert want[3].sum() > 0  # restarts happen
    for other, och, ocl in ((want, wch, wcl), (plain, pch, pcl)):
        assert same_f32(got[0], other[0])
        for g, w in zip(got[1:], other[1:]):
            assert np.array_equal(g, w)
        assert np.array_equal(gch, och) and np.array_equal(gcl, ocl)
    assert np.array_equal(got[0].view(np.uint32), plain[0].view(np.uint32))


@pytest.mark.parametrize("layout", ["legacy", "partitionable"])
def test_ring_producer_vs_split_at(libs, layout):
    """The ring producer alone (key_l1_fill), in either PRNG layout, against
    split_at_l key by key: every key of every type, for a half starting in
    either ring half and a short last half."""
    emu, emu_keyl1, lib = libs
    from cotix_oracle import physics as P
    from cotix_oracle.params import Params
    h, _ = emu.oracle_scene(lib, P.robocup_bodies(), None if layout == "legacy" else Params(prng_layout=layout))
    tn2 = emu_keyl1.tn2(lib, h)
    assert tn2.tolist() == [22, 8]
    rng = np.random.default_rng(5)
    for s0, n in ((0, 8), (8, 8), (24, 3), (16, 1)):
        tk = rng.integers(0, 2 ** 32, size=(n, len(tn2), 2, 4), dtype=np.uint64).astype(np.uint32)
        ring = emu_keyl1.fill(lib, h, tk, s0)
        assert ring.shape == (n, int(tn2.sum()), 2, 4)
        for s in range(n):
            off = 0
            for ty, N in enumerate(tn2):
                for i in range(N):
                    for e in range(4):
                        want = emu_keyl1.split_at(lib, h, tk[s, ty, :, e], int(N), i)
                        assert ring[s, off + i, :, e].tolist() == want.tolist(), (s0, s, ty, i, e)
                off += N


@pytest.mark.parametrize("T", [33, 64])
def test_key_l1_asan_driver(libs, tmp_path, T):
    """tests/emu/keyl1_asan_driver (-fsanitize=address,undefined
    -fno-sanitize-recover=all, its own main, no preloaded runtime): the level-1
    key form into exactly sized buffers exits cleanly (ring indexing; a short
    half leaves the poison pattern unread), and its output equals the plain
    emulation's bits."""
    emu, emu_keyl1, lib = libs
    from cotix_oracle import physics as P
    from test_emu_asan import _scene_arrays
    dyn, keys, act = start(T)
    params, pb, pt, pn, geom = _scene_arrays(P.robocup_bodies())
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([dyn.shape[0], len(pb), B, T, STAGES, len(geom), 0, 0, 4, 4], np.int32).tofile(f)
        for x in (params, pb, pt, pn, geom, dyn, keys, act):
            np.ascontiguousarray(x).tofile(f)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([os.path.join(HERE, "emu", "build", "keyl1_asan_driver"), inp, out], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    h, g = emu.oracle_scene(lib, P.robocup_bodies())
    plain = fresh(dyn, keys)
    ch, cl = emu.step_ex(lib, h, plain[0], plain[1], plain[2], g, 0, T, STAGES, 5, E=4, action=act, action_body=4,
                         dyn_reset=dyn.copy(), resets=plain[3])
    want = np.concatenate([x.reshape(-1).view(np.uint8) for x in (*plain, ch, cl)])
    assert np.array_equal(np.fromfile(out, np.uint8), want)
