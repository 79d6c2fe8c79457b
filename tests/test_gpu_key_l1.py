"""The key helper's level-1 key ring on the GPU (step_help_kernel's L1 form:
the helper wave computes the collider scan's first-level keys into an LDS
ring, cotix_kernel.h KeyL1): RoboCup through BatchedEnv with autoreset,
actions and the collider trace, bit for bit against the C port of the oracle
and against the same trajectory in launches of at most 16 steps, which run
step_kernel -- with cotix_scene_last_step_form proving which kernel ran."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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
    assert os.path.exists(cport.LIB), "oracle C port %s missing: build it before the GPU run" % cport.LIB
    import parallax_amd as pa
    return torch, pa, cport, cport.load()


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
def test_key_l1_vs_cport_and_short_launches(ctx, B, T):
    torch, pa, cport, clib = ctx
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
