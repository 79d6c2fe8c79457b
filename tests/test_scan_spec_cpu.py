"""The key helper's speculative draw words on CPU (cotix_kernel.h
scan_spec_fill / m_spec: the helper wave draws each cell's first M scan
candidates ahead of the physics, one word per (cell, env) item and step, and
the fused scan's round 0 settles from it every item whose first valid passing
candidate lies among them): the kernel's own producer and step code on the
host emulation (tests/emu/cotix_emu_scanspec.cpp).

The producer is checked against the oracle's prng draw by draw, the form
against the C port bit for bit with the collider trace, from which each written
cell's settle position (the winner's index in its cell's list) shows that both
paths ran: round 0 (position < M) and the lazy rounds after it (>= M), among
the steps that have draw words (all but a launch's first ring half, whose
words stay poisoned in this build).  The
barrier counts are compared with cxk::key_l1_barriers inside the emulation."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))

STAGES = 1 | 4 | 16
KL1R = 8  # cxk::KL1R: a launch's first ring half (steps 0 .. 7) has no draw words and scans lazily
LIBS = {4: "libcotix_emu_scanspec.so", 8: "libcotix_emu_scanspec_m8.so"}


@pytest.fixture(scope="module")
def libs():
    import emu
    import emu_scanspec
    emu_scanspec.build(*LIBS.values(), "scanspec_asan_driver")
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "..", "oracle")], check=True)  # the C port: never a skip
    return emu, emu_scanspec, {m: emu_scanspec.load(name) for m, name in LIBS.items()}


def same_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def start(B, T):
    from cotix_oracle import cport
    dyn, keys = cport.robocup_batch(B)
    dyn, keys = np.ascontiguousarray(dyn, np.float32), np.ascontiguousarray(keys, np.uint32)
    act = np.ascontiguousarray((np.random.default_rng(100 * B + T).normal(size=(T, B, 2)) * 0.1).astype(np.float32))
    return dyn, keys, act


def fresh(dyn, keys):
    B = dyn.shape[2]
    return [dyn.copy(), keys.copy(), np.zeros(B, np.uint32), np.zeros(B, np.uint32)]


def test_builds_m(libs):
    """The default build runs the kernel's M; the second build an M past
    RoboCup's shortest lists."""
    emu, emu_scanspec, L = libs
    from cotix_oracle import physics as P
    assert emu_scanspec.m_of(L[4])[0] == emu_scanspec.m_of(L[4])[1]
    assert emu_scanspec.m_of(L[8])[0] == 8
    h, _ = emu.oracle_scene(L[8], P.robocup_bodies())
    ln = emu_scanspec.lists(L[8], h)[2]
    assert ln.min() < 8 <= ln.max() and ln.min() >= emu_scanspec.m_of(L[4])[0]


@pytest.mark.parametrize("M", [4, 8])
@pytest.mark.parametrize("layout", ["legacy", "partitionable"])
def test_draw_word_producer_vs_oracle_prng(libs, layout, M):
    """scan_spec_fill alone, in either PRNG layout: bit m of every (cell, env)
    word of every step == bernoulli(split(split(ring key, N1)[i1])[0], p) of
    the cell's candidate m by the oracle's prng, 0 past the list's end (M = 8:
    RoboCup's lists of 6 and 7) -- for a whole half, and a short one in the
    other ring half."""
    emu, emu_scanspec, L = libs
    import emu_keyl1
    from cotix_oracle import params as PR
    from cotix_oracle import physics as P
    from cotix_oracle import prng
    lib = L[M]
    assert emu_scanspec.m_of(lib)[0] == M
    prm = PR.Params(prng_layout=layout)
    bodies = P.robocup_bodies()
    h, _ = emu.oracle_scene(lib, bodies, None if layout == "legacy" else prm)
    tn2 = emu_keyl1.tn2(lib, h)
    n1n2 = [(len(l1), len(l2)) for l1, l2 in P.enumerate_candidates(bodies).values()]
    assert [n2 for _, n2 in n1n2] == tn2.tolist()
    off = np.concatenate([[0], np.cumsum(tn2)])
    ci, cj, ln, cand = emu_scanspec.lists(lib, h)
    rng = np.random.default_rng(11)
    with PR.use(prm):
        for s0, n in ((0, 8), (24, 3)):
            keys = rng.integers(0, 2 ** 32, size=(n, int(tn2.sum()), 2, 4), dtype=np.uint64).astype(np.uint32)
            got = emu_scanspec.fill(lib, h, keys, s0)
            assert got.shape == (n, len(ci), 4)
            for s in range(n):
                for l in range(len(ci)):
                    for e in range(4):
                        want = 0
                        for m in range(min(M, int(ln[l]))):
                            code = int(cand[l, m])
                            i1, i2, ty = code & 511, (code >> 9) & 511, code >> 18
                            k2 = keys[s, off[ty] + i2, :, e]
                            k1 = prng.split(prng.split(k2, n1n2[ty][0])[i1])[0]
                            want |= int(prng.bernoulli(k1, prm.contact_p)) << m
                        assert int(got[s, l, e]) == want, (s0, s, l, e)


def run_form(libs, M, B, T):
    """One launch of T steps through the form with the draw words and on the C
    port; returns the settle positions of the C port's written cells."""
    emu, emu_scanspec, L = libs
    from cotix_oracle import cport
    from cotix_oracle import physics as P
    lib = L[M]
    dyn, keys, act = start(B, T)
    reset = dyn.copy()
    h, geom = emu.oracle_scene(lib, P.robocup_bodies())
    want = fresh(dyn, keys)
    sc = cport.Scene(cport.load(), P.robocup_bodies())
    wch, wcl = sc.step_ex(want[0], want[1], want[2], T, cport.STAGES_ROBOCUP, None, act, 4, reset, want[3],
                          trace=True)
    # the C port alone first: the launch must take both paths before it can show anything about them
    pos = emu_scanspec.settle_positions(emu_scanspec.lists(lib, h), wcl[KL1R:])  # the steps with a round 0
    assert (pos < M).any() and (pos >= M).any(), "B %d T %d: not both scan paths (M %d)" % (B, T, M)
    got = fresh(dyn, keys)
    emu_scanspec.round0_done(lib)
    gch, gcl = emu_scanspec.step_scanspec(lib, h, got[0], got[1], got[2], geom, 0, T, STAGES, 5, action=act,
                                          action_body=4, dyn_reset=reset, resets=got[3])
    # round 0 itself ran (the same bits come out without it): it settled at least the cells that the C
    # port settled inside M in the steps with draw words, and nothing in a launch without such steps
    n0 = emu_scanspec.round0_done(lib)
    assert n0 >= int((pos < M).sum()) > 0, "round 0 settled %d items" % n0
    assert same_f32(got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        assert np.array_equal(g, w)
    assert np.array_equal(gch, wch) and np.array_equal(gcl, wcl)
    if T >= 33:
        assert want[3].sum() > 0  # restarts happen
    return pos


# T: one ring half into the second window; a one-step last half and window; a
# partial third window; four whole windows.  B: a ragged last env group; whole groups
@pytest.mark.parametrize("T", [17, 33, 40, 64])
@pytest.mark.parametrize("B", [13, 16])
def test_scan_spec_vs_cport(libs, B, T):
    """RoboCup with autoreset, actions and the collider trace through the form
    with the draw words == the C port, bit for bit (state, keys, error bits,
    restart counters, both trace arrays), the barriers passed == key_l1_barriers
    (emu_step_scanspec fails otherwise), and the launch settled cells both in
    round 0 and in the lazy rounds."""
    run_form(libs, 4, B, T)


def test_lists_shorter_than_m(libs):
    """M = 8 on RoboCup, whose shortest lists hold 6 and 7 candidates: a word's
    bits past the list's end are 0, an item whose whole list lies inside M
    settles or finishes in round 0, and the bits still equal the C port's."""
    pos = run_form(libs, 8, 13, 33)
    assert (pos >= 8).any()


@pytest.mark.parametrize("T", [17, 33])
def test_scan_spec_asan_driver(libs, tmp_path, T):
    """tests/emu/scanspec_asan_driver (-fsanitize=address,undefined
    -fno-sanitize-recover=all, its own main, no preloaded runtime): the
    producer and round 0 into exactly sized buffers, with a short last half
    (one step), exit cleanly and give the plain emulation's bits."""
    emu, emu_scanspec, L = libs
    from cotix_oracle import physics as P
    from test_emu_asan import _scene_arrays
    B = 12
    dyn, keys, act = start(B, T)
    params, pb, pt, pn, geom = _scene_arrays(P.robocup_bodies())
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        np.array([dyn.shape[0], len(pb), B, T, STAGES, len(geom), 0, 0, 4, 4], np.int32).tofile(f)
        for x in (params, pb, pt, pn, geom, dyn, keys, act):
            np.ascontiguousarray(x).tofile(f)
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "UBSAN_OPTIONS")}
    r = subprocess.run([os.path.join(HERE, "emu", "build", "scanspec_asan_driver"), inp, out], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lib = L[4]
    h, g = emu.oracle_scene(lib, P.robocup_bodies())
    plain = fresh(dyn, keys)
    ch, cl = emu.step_ex(lib, h, plain[0], plain[1], plain[2], g, 0, T, STAGES, 5, E=4, action=act, action_body=4,
                         dyn_reset=dyn.copy(), resets=plain[3])
    want = np.concatenate([x.reshape(-1).view(np.uint8) for x in (*plain, ch, cl)])
    assert np.array_equal(np.fromfile(out, np.uint8), want)
