"""The key helper's speculative draw words on the GPU (step_help_kernel's L1
form: the helper wave draws each cell's first cxk::SCAN_M scan candidates
ahead of the physics, the fused scan's round 0 settles from them;
cotix_kernel.h scan_spec_fill / m_spec): RoboCup through BatchedEnv with
autoreset, actions and the collider trace, bit for bit against the C port of
the oracle and against the same trajectory in launches of at most 16 steps,
which run step_kernel -- with cotix_scene_last_step_form proving which kernel
ran, and each written cell's settle position (the winner's index in its cell's
list, from the C port's trace) proving that every launch settled cells both
in round 0 and in the lazy rounds after it (among the steps past the launch's
first ring half, which has no draw words)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KL1R = 8  # cxk::KL1R: a launch's first ring half (steps 0 .. 7) has no draw words and scans lazily

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))


def same_f32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.fixture(scope="module")
def ctx():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu test without a visible GPU (torch.cuda.is_available() is False)")
    from cotix_oracle import cport
    from cotix_oracle import physics as P
    assert os.path.exists(cport.LIB), "oracle C port %s missing: build it before the GPU run" % cport.LIB
    import emu
    import emu_scanspec
    import parallax_amd as pa
    # the scene's cell lists and the kernel's M, from the host build of the kernel's own scene code
    elib = emu_scanspec.load()
    h, _ = emu.oracle_scene(elib, P.robocup_bodies())
    cells, (_, M) = emu_scanspec.lists(elib, h), emu_scanspec.m_of(elib)
    return torch, pa, cport, cport.load(), emu_scanspec, cells, M


def state(env):
    w = env.world
    return (w.dyn.cpu().numpy(), w.keys.cpu().numpy().view(np.uint32), w.err.cpu().numpy().view(np.uint32),
            env.resets.cpu().numpy().view(np.uint32))


# B: one full workgroup (4 env groups); a ragged last env group; a second
# workgroup with idle step and helper waves (env groups 4 and 5 of 8)
# T: one ring half into the second window; a one-step last half and window; a
# partial third window; four whole windows
@pytest.mark.parametrize("T", [17, 33, 40, 64])
@pytest.mark.parametrize("B", [16, 13, 22])
def test_scan_spec_vs_cport_and_short_launches(ctx, B, T):
    torch, pa, cport, clib, emu_scanspec, cells, M = ctx
    from cotix_oracle import physics as P
    form = lambda env: pa._ffi.lib.cotix_scene_last_step_form(env.world.scene.handle)  # noqa: E731
    envs = [pa.BatchedEnv(pa.RoboCupEnv(batch=B, device="cuda", perturb=True), autoreset=True) for _ in range(2)]
    for env in envs:
        env.reset()
    long_, short = envs
    dyn, keys = (np.ascontiguousarray(x) for x in state(long_)[:2])
    reset, err, resets = dyn.copy(), np.zeros(B, np.uint32), np.zeros(B, np.uint32)
    sc = cport.Scene(clib, P.robocup_bodies())
    rng = np.random.default_rng(1000 * B + T)
    for q in range(2):
        act = np.ascontiguousarray((rng.normal(size=(T, B, 2)) * 0.1).astype(np.float32))
        wch, wcl = sc.step_ex(dyn, keys, err, T, cport.STAGES_ROBOCUP, None, act, 4, reset, resets, trace=True,
                              nthreads=4)
        pos = emu_scanspec.settle_positions(cells, wcl[KL1R:])  # the steps with a round 0
        assert (pos < M).any() and (pos >= M).any(), "launch %d: not both scan paths (M %d)" % (q, M)
        trc = {}
        long_.step(T, action=torch.tensor(act, device="cuda"), trace=trc)
        assert form(long_) == 2, "the %d-step launch did not run the level-1 key form" % T
        sch, scl = [], []
        for s in range(0, T, 16):
            tr = {}
            short.step(min(16, T - s), action=torch.tensor(act[s:s + 16], device="cuda"), trace=tr)
            assert form(short) == 0, "a launch of at most 16 steps did not run step_kernel"
            sch.append(tr["chosen"].cpu().numpy())
            scl.append(tr["cells"].cpu().numpy())
        torch.cuda.synchronize()
        gch, gcl = trc["chosen"].cpu().numpy(), trc["cells"].cpu().numpy()
        assert np.array_equal(gch, wch) and np.array_equal(gcl, wcl), "launch %d trace vs the C port" % q
        assert np.array_equal(gch, np.concatenate(sch)) and np.array_equal(gcl, np.concatenate(scl)), \
            "launch %d trace vs the short launches" % q
        got, sht = state(long_), state(short)
        assert same_f32(got[0], dyn) and same_f32(got[0], sht[0]), "launch %d state" % q
        for g, w, s in zip(got[1:], (keys, err, resets), sht[1:]):
            assert np.array_equal(g, w) and np.array_equal(g, s), "launch %d keys / err / resets" % q
    if T >= 33:
        assert resets.sum() > 0  # restarts happen
